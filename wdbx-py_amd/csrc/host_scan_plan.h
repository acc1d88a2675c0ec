// host_scan_plan.h -- the device-free shape rules of the fp32 scan and range kernels: which instance serves a row pitch, and
// the grid, partial-list, chunk and LDS arithmetic of a scan launch.  The function-pointer pickers that turn a form into a
// kernel live next to the kernels (kernels_scan.h, kernels_range.h); choose_scan / plan_scan (host_index.h) call both.
// Included by wdbx_hip.hip and tests/kernel_harness/scan_harness.hip and, on its own, by tests/host_harness/scan_plan_harness.cpp
// (plain g++ in the CPU suite, tests/test_scan_plan_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

// an instance of the scan: L lanes per row; specialised (scan_kernel): QPL quads per lane, ragged = L * QPL > pitch4 (or forced);
// generic (scan_kernel_generic / scan_kernel_listed): QPL = 0, never ragged
struct ScanForm {
  int L = 8;
  int QPL = 0;
  bool ragged = false;
  bool generic = true;
};

// the unrolled instances that exist (pick_specialised of kernels_scan.h returns a kernel for exactly these)
static inline bool scan_has_instance(int L, int qpl) {
  if (L == 1 || L == 2) return qpl == 1;
  if (L == 4) return qpl >= 1 && qpl <= 3;
  if (L == 8 || L == 16 || L == 32 || L == 64) return qpl == 1 || qpl == 2 || qpl == 3 || qpl == 4 || qpl == 6 || qpl == 8 || qpl == 12;
  return false;
}

// lanes per row of the generic body (and of the listed repair scan): the row's quads rounded up to a power of two, at most 8;
// 64 for rows longer than the largest unrolled instance
static inline int scan_generic_lanes(int pitch4) {
  int L = 1;
  while (L < 8 && L < pitch4) L <<= 1;
  if (pitch4 > 768) L = 64;
  return L;
}

static inline ScanForm scan_generic_form(int pitch4) {
  ScanForm f;
  f.L = scan_generic_lanes(pitch4);
  return f;
}

// lanes: option scan_lanes (0 = free choice); generic: option scan_generic; force_ragged: the ragged form also on an exact fit
static inline ScanForm scan_form(int pitch4, int64_t lanes, bool generic, bool force_ragged) {
  if (!generic && pitch4 < 16 && !lanes) {
    // short rows (d < 64): the smallest instance that holds the row, up to 3/8 of its slots idle
    const int cand[7][2] = {{1, 1}, {2, 1}, {4, 1}, {8, 1}, {4, 2}, {4, 3}, {8, 2}};
    for (int t = 0; t < 7; ++t) {
      const int slots = cand[t][0] * cand[t][1], waste = slots - pitch4;
      if (waste < 0 || waste * 8 > slots * 3) continue;
      if (scan_has_instance(cand[t][0], cand[t][1])) {
        ScanForm f;
        f.L = cand[t][0];
        f.QPL = cand[t][1];
        f.ragged = waste != 0 || force_ragged;
        f.generic = false;
        return f;
      }
    }
  }
  if (!generic && pitch4 >= 16) {
    // unrolled instances exist for L in {8,16,32,64} x QPL in {3,4,6,8,12} (+ {1,2} for L >= 16); slots past the row end idle
    // (RAGGED form), at most a third of them.  Rows whose byte pitch is a multiple of 128 take the
    // instance with the fewest idle slots (smaller L on ties: all L measure alike there).  Rows that
    // do NOT start on cache-line boundaries take the LARGEST admissible L: a lane group then reads one
    // long contiguous span per instruction instead of many short ones that each straddle two lines
    // (d=300: L=8 5.35 TB/s, L=32 6.89 TB/s; d=200: L=8 5.87, L=16 6.84; profiles/r01/bench_dims.txt)
    const int Ls[4] = {8, 16, 32, 64}, Qs[7] = {1, 2, 3, 4, 6, 8, 12};
    const bool line_aligned = pitch4 % 8 == 0;
    int bestL = 0, bestQ = 0, best_waste = 1 << 30;
    // tier 0: QPL >= 3 (enough loads in flight per pass, several rows per pass).  tier 1, only for
    // misaligned short rows that tier 0 can serve with L = 8 at best: QPL 1 or 2 on L = 16 / 32
    // (d=100: (8,4) 5.63 TB/s, (32,1) 6.08 TB/s; for d=200 the wide short form is slower, 5.3 vs 6.6)
    for (int tier = 0; tier < 2; ++tier) {
      if (tier == 1 && (line_aligned || bestL >= 16)) break;
      for (int li = 0; li < 4; ++li) {
        if (lanes && Ls[li] != lanes) continue;
        if (tier == 1 && (Ls[li] < 16 || Ls[li] > 32)) continue;
        for (int qi = (tier == 0 ? 2 : 0); qi < (tier == 0 ? 7 : 2); ++qi) {
          const int slots = Ls[li] * Qs[qi], waste = slots - pitch4;
          if (waste < 0 || waste * 3 > slots) continue;
          const bool better = line_aligned ? waste < best_waste
                                           : (Ls[li] > bestL || (Ls[li] == bestL && waste < best_waste));
          if (better) {
            best_waste = waste;
            bestL = Ls[li];
            bestQ = Qs[qi];
          }
        }
      }
    }
    // a ragged instance may idle at most a third of its slots; beyond that the generic kernel is better
    if (bestL && best_waste * 3 <= bestL * bestQ && scan_has_instance(bestL, bestQ)) {
      ScanForm f;
      f.L = bestL;
      f.QPL = bestQ;
      f.ragged = best_waste != 0 || force_ragged;
      f.generic = false;
      return f;
    }
  }
  return scan_generic_form(pitch4);
}

// passes a wave of scan_kernel<L, QPL> keeps in flight (U of scan_body)
static inline int scan_passes_in_flight(int qpl) {
  return (qpl >= 12) ? 1 : (qpl >= 6) ? 2 : (qpl >= 4) ? 3 : (qpl == 3) ? 4 : (qpl == 2) ? 6 : 8;
}

// range_scan_kernel<METRIC, P, NI>: lanes per row = the row's quads rounded up to a power of two (up to 64), and the unrolled
// loads per lane (0: the loop)
struct RangeForm {
  int P;
  int NI;
};

static inline RangeForm range_scan_form(uint32_t pitch4) {
  if (pitch4 <= 1) return {1, 1};
  if (pitch4 <= 2) return {2, 1};
  if (pitch4 <= 4) return {4, 1};
  if (pitch4 <= 8) return {8, 1};
  if (pitch4 <= 16) return {16, 1};
  if (pitch4 <= 32) return {32, 1};
  if (pitch4 <= 64) return {64, 1};
  if (pitch4 <= 128) return {64, 2};
  if (pitch4 <= 192) return {64, 3};
  if (pitch4 <= 256) return {64, 4};
  return {64, 0};
}

// ---- a scan launch in numbers ---------------------------------------------------------------------
// list mode of a top-k scan: 2 = no list, every row's key dumped (the radix select ranks them), 1 = register lists, 0 = LDS lists
static inline int scan_list_mode(bool select, int k, bool lds_lists) { return select ? 2 : (k <= 128 && !lds_lists) ? 1 : 0; }

// bytes of LDS beyond the 4 lists: the generic body stages the query
static inline size_t scan_lds_extra(bool generic, int pitch4) { return generic ? (size_t)pitch4 * 16 : 0; }

// dynamic LDS of a launch: 4 lists of k keys unless the keys are dumped, + the staged query
static inline size_t scan_lds_bytes(bool select, int k, size_t lds_extra) {
  return (select ? 0 : (size_t)4 * k * sizeof(uint64_t)) + lds_extra;
}

// above this the launch needs hipFuncAttributeMaxDynamicSharedMemorySize raised first
static inline bool scan_lds_needs_attribute(size_t lds) { return lds > 64 * 1024; }

// row groups of 64 / L rows (one wave pass each)
static inline uint32_t scan_groups(uint64_t n_rows, int L) {
  const int R = 64 / L;
  return (uint32_t)((n_rows + R - 1) / R);
}

// every wave should have a few passes of work; small corpora get a smaller grid
static inline uint32_t scan_max_blocks(uint32_t groups) {
  const uint32_t min_groups_per_wave = 1;
  return std::max<uint32_t>(1, (groups + 4 * min_groups_per_wave - 1) / (4 * min_groups_per_wave));
}

// workgroups of a launch: at most 2 per CU (8 waves/CU x 8 KiB in flight: sweep in profiles/sweep_r01.txt) of the per_cu the
// occupancy allows, or option scan_blocks; never more than the corpus has work for
static inline uint32_t scan_blocks(uint32_t cu_count, int per_cu, int64_t opt_blocks, uint32_t groups) {
  uint32_t blocks = cu_count * (uint32_t)std::min(per_cu, 2);
  if (opt_blocks > 0) blocks = (uint32_t)opt_blocks;
  return std::max<uint32_t>(1, std::min(blocks, scan_max_blocks(groups)));
}

// partial lists: one per workgroup or one per wave
static inline uint32_t scan_partial_lists(bool wg_merge, uint32_t blocks) { return wg_merge ? blocks : blocks * 4; }

// groups per wave of a blocked launch (contiguous groups); 0: the waves interleave
static inline uint32_t scan_chunk(bool blocked, uint32_t groups, uint32_t blocks) {
  return blocked ? (groups + blocks * 4 - 1) / (blocks * 4) : 0;
}
