// scan_harness.hip -- test-only launcher of the library's fp32 scan and range kernels (tests/scan_harness.py,
// tests/test_gpu_scan_kernels.py, tests/test_gpu_range_kernels.py): scan_kernel (every unrolled instance), scan_kernel_generic,
// scan_kernel_listed, range_scan_kernel and range_filter_kernel.
//
// Built from the very headers libwdbx_hip.so is built from (host_scan_plan.h, kernels_common.h, kernels_scan.h, kernels_aux.h,
// kernels_range.h are included below); the instance of every launch is chosen by the shape rules of host_scan_plan.h
// (scan_form, scan_generic_form, range_scan_form) and the pickers next to the kernels (pick_scan_form, pick_listed,
// pick_range_scan), the LDS bytes and the row groups by the plan arithmetic plan_scan uses.  This file defines no kernel of its
// own.  Each entry point takes HOST pointers: copy in, launch on the null stream, synchronise, copy out; it returns the HIP
// error code, or -1 when the arguments would make a kernel read or write outside the uploaded arrays (checked here, before
// anything is launched).  Output arrays are copied IN as well, so a slot the kernel leaves alone comes back with whatever the
// caller put there.  Every array comes with its length: the checks are against those.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "wdbx_hip.h"

typedef unsigned long long u64;
typedef float f4 __attribute__((ext_vector_type(4)));

#include "host_scan_plan.h"
#include "kernels_common.h"
#include "kernels_scan.h"
#include "kernels_aux.h"
#include "kernels_range.h"

namespace {

// device buffers of one call: freed when the call returns, whichever way
struct Bufs {
  void* p[16];
  int n = 0;
  hipError_t err = hipSuccess;
  // a device copy of host[0 .. bytes) (null stays null)
  void* up(const void* host, size_t bytes) {
    if (!host || err != hipSuccess) return nullptr;
    void* d = nullptr;
    err = hipMalloc(&d, std::max<size_t>(bytes, 16));
    if (err != hipSuccess) return nullptr;
    p[n++] = d;
    if (bytes) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    return d;
  }
  void down(void* host, const void* dev, size_t bytes) {
    if (host && dev && bytes && err == hipSuccess) err = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
  }
  ~Bufs() {
    for (int i = 0; i < n; ++i) (void)hipFree(p[i]);
  }
};

int finish(Bufs& b) {
  if (b.err != hipSuccess) (void)hipGetLastError();
  return (int)b.err;
}

bool metric_ok(int metric) { return metric == WDBX_METRIC_COSINE || metric == WDBX_METRIC_L2; }

constexpr uint64_t MAX_ROWS = 0xFFFFFF00ull;  // the library's own limit: row numbers and their group arithmetic stay in 32 bits

}  // namespace

extern "C" {

// the form scan_form answers for a pitch and the scan options; has_fn: 1 when the pickers return a kernel for it in every
// metric, list mode and load flavour
int scn_scan_form(int pitch4, int lanes, int generic, int force_ragged, int* L, int* QPL, int* ragged, int* is_generic, int* has_fn) {
  if (pitch4 < 1) return -1;
  const ScanForm f = scan_form(pitch4, lanes, generic != 0, force_ragged != 0);
  *L = f.L;
  *QPL = f.QPL;
  *ragged = f.ragged ? 1 : 0;
  *is_generic = f.generic ? 1 : 0;
  int all = 1;
  for (int metric : {WDBX_METRIC_COSINE, WDBX_METRIC_L2})
    for (int mode = 0; mode < 3; ++mode)
      for (int nt = 0; nt < 2; ++nt)
        if (!pick_scan_form(f, metric, nt != 0, mode)) all = 0;
  *has_fn = all;
  return 0;
}

// lanes per row of the listed repair scan (and of the generic kernel)
int scn_listed_lanes(int pitch4) { return pitch4 < 1 ? -1 : scan_generic_form(pitch4).L; }

int scn_range_form(uint32_t pitch4, int* P, int* NI, int* has_fn) {
  const RangeForm f = range_scan_form(pitch4);
  *P = f.P;
  *NI = f.NI;
  *has_fn = pick_range_scan<WDBX_METRIC_COSINE>(pitch4) && pick_range_scan<WDBX_METRIC_L2>(pitch4) ? 1 : 0;
  return 0;
}

// the plan arithmetic of a scan launch as plan_scan computes it: out = {mode, groups, max_blocks, blocks, partial lists, chunk,
// LDS bytes, 1 when the LDS needs the function attribute}
int scn_plan(uint64_t n_rows, int L, int k, int select, int lds_lists, uint64_t lds_extra, uint32_t cu_count, int per_cu,
             int64_t opt_blocks, int wg_merge, int blocked, uint64_t* out) {
  if (L < 1 || L > 64 || (L & (L - 1)) || k < 1 || n_rows < 1 || n_rows >= MAX_ROWS) return -1;
  const uint32_t groups = scan_groups(n_rows, L);
  const uint32_t blocks = scan_blocks(cu_count, per_cu, opt_blocks, groups);
  const size_t lds = scan_lds_bytes(select != 0, k, (size_t)lds_extra);
  out[0] = (uint64_t)scan_list_mode(select != 0, k, lds_lists != 0);
  out[1] = groups;
  out[2] = scan_max_blocks(groups);
  out[3] = blocks;
  out[4] = scan_partial_lists(wg_merge != 0, blocks);
  out[5] = scan_chunk(blocked != 0, groups, blocks);
  out[6] = lds;
  out[7] = scan_lds_needs_attribute(lds) ? 1 : 0;
  return 0;
}

// the scalar arguments of one scan launch
struct ScnScan {
  int32_t listed;  // 0: scan_kernel / scan_kernel_generic as scan_form picks them; 1: scan_kernel_listed (generic body)
  int32_t lanes, generic, force_ragged, nt;  // the form inputs (options scan_lanes, scan_generic, force_ragged, scan_nt)
  int32_t metric;
  int32_t mode;    // 0 LDS lists, 1 register lists (k <= 128), 2 key dump
  int32_t k;
  uint32_t n_rows, pitch4;
  uint32_t grid_x, grid_y;
  uint32_t chunk;  // 0: the waves interleave the row groups; else groups per wave
  int32_t wg_merge;
  uint32_t over_cap;
  uint32_t y_partials;  // u64s between consecutive queries' partials
};

// rows: [n_rows][pitch4 * 4]; queries: [queries_len] floats -- a plain launch reads grid_y queries, a listed one those the list
// names; mask: [mask_words] or null; partials: [partials_len] keys (the caller's guard behind what the launch may write counts
// as part of the array: the checks are against what the kernels really touch); only_if_over: [over_len] counters or null;
// over_list: [over_list_len] words {n, q_0 ..} (listed launches).
int scn_scan(const ScnScan* d, const float* rows, uint64_t rows_len, const float* queries, uint64_t queries_len, const uint32_t* mask,
             uint64_t mask_words, u64* partials, uint64_t partials_len, const uint32_t* only_if_over, uint64_t over_len,
             const uint32_t* over_list, uint64_t over_list_len) {
  if (!d || !rows || !queries || !partials || !metric_ok(d->metric)) return -1;
  if (d->n_rows < 1 || (uint64_t)d->n_rows >= MAX_ROWS || d->pitch4 < 1 || d->pitch4 > (1u << 20)) return -1;  // (n_rows == 0: last_row wraps)
  if (d->grid_x < 1 || d->grid_y < 1 || d->grid_y > 65535 || d->k < 1 || d->k > 2048 || d->mode < 0 || d->mode > 2) return -1;
  if (d->mode == 1 && d->k > 128) return -1;  // (a register list holds two keys per lane)
  const uint64_t row_floats = (uint64_t)d->pitch4 * 4;
  // every row read is clamped to the last row and every quad offset to the last quad: the reads stay inside n_rows * pitch4 quads
  if (rows_len != (uint64_t)d->n_rows * row_floats) return -1;
  if (mask && mask_words < ((uint64_t)d->n_rows + 31) / 32) return -1;
  ScanForm f;
  scan_fn fn = nullptr;
  if (d->listed) {
    if (d->mode == 2) return -1;  // (no instance)
    f = scan_generic_form((int)d->pitch4);
    fn = pick_listed(f.L, d->metric, d->mode);
  } else {
    f = scan_form((int)d->pitch4, d->lanes, d->generic != 0, d->force_ragged != 0);
    fn = pick_scan_form(f, d->metric, d->nt != 0, d->mode);
  }
  if (!fn) return -1;
  if (!f.generic && (uint64_t)f.L * f.QPL < d->pitch4) return -1;                       // (an instance shorter than the row)
  if (!f.generic && !f.ragged && (uint64_t)f.L * f.QPL != d->pitch4) return -1;         // (an exact form reads L * QPL quads of every row)
  const uint32_t groups = scan_groups(d->n_rows, f.L);
  const uint64_t waves = (uint64_t)d->grid_x * 4;
  // the group counters of a wave stay in 32 bits: cur + u * stride for up to 8 passes in flight, or wave * chunk
  if ((uint64_t)groups + 8 * waves >= (1ull << 32) || waves * (uint64_t)d->chunk + d->chunk >= (1ull << 32)) return -1;
  // what one query's launch may write
  const uint64_t lists = d->wg_merge ? d->grid_x : waves;
  const uint64_t need = d->mode == 2 ? (uint64_t)d->n_rows : (uint64_t)d->k * lists;
  if (d->listed) {
    if (!over_list || over_list_len < 1 || over_list_len < (uint64_t)over_list[0] + 1) return -1;
    for (uint32_t i = 0; i < over_list[0]; ++i) {
      const uint64_t qi = over_list[1 + i];
      if ((qi + 1) * row_floats > queries_len || qi * d->y_partials + need > partials_len) return -1;
      if (over_list[0] > 1 && d->y_partials < need) return -1;
    }
    if (only_if_over) return -1;  // (the listed kernel does not look at the counters)
  } else {
    if ((uint64_t)d->grid_y * row_floats > queries_len) return -1;
    if ((uint64_t)(d->grid_y - 1) * d->y_partials + need > partials_len) return -1;
    if (d->grid_y > 1 && d->y_partials < need) return -1;  // (the queries' partials would overlap)
    if (only_if_over && over_len < d->grid_y) return -1;
  }
  const bool select = d->mode == 2;
  const size_t lds = scan_lds_bytes(select, d->k, scan_lds_extra(f.generic, (int)d->pitch4));
  Bufs b;
  if (scan_lds_needs_attribute(lds)) {
    if ((b.err = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess) {
      (void)hipGetLastError();
      return -1;  // (more LDS than a workgroup can have)
    }
  }
  int per_cu = 0;
  if ((b.err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)fn, 256, lds)) != hipSuccess) return finish(b);
  if (per_cu < 1) return -1;
  ScanArgs a = {};
  a.rows = (const f4*)b.up(rows, (size_t)rows_len * sizeof(float));
  a.query = (const f4*)b.up(queries, (size_t)queries_len * sizeof(float));
  a.partials = (u64*)b.up(partials, (size_t)partials_len * sizeof(u64));
  a.mask = (const uint32_t*)b.up(mask, (size_t)mask_words * sizeof(uint32_t));
  a.n_rows = d->n_rows;
  a.pitch4 = d->pitch4;
  a.groups = groups;
  a.chunk = d->chunk;
  a.k = d->k;
  a.wg_merge = d->wg_merge ? 1 : 0;
  a.only_if_over = (const uint32_t*)b.up(only_if_over, (size_t)over_len * sizeof(uint32_t));
  a.over_cap = d->over_cap;
  a.y_partials = d->y_partials;
  a.over_list = (const uint32_t*)b.up(over_list, (size_t)over_list_len * sizeof(uint32_t));
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(d->grid_x, d->grid_y), dim3(256), lds, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(partials, a.partials, (size_t)partials_len * sizeof(u64));
  return finish(b);
}

// range_scan_kernel<metric, P, NI> as pick_range_scan picks it, grid (grid_x, nq): rows: [n_rows][pitch4 * 4]; queries:
// [nq][pitch4 * 4]; thr: [nq]; mask: [mask_words] or null; out: [out_len] >= nq * cap keys (what lies behind is the caller's
// guard); count: [nq], copied in (the library zeroes it before the launch).
int scn_range_scan(int metric, const float* rows, uint64_t n_rows, uint32_t pitch4, const float* queries, uint32_t nq, const float* thr,
                   const uint32_t* mask, uint64_t mask_words, u64* out, uint64_t out_len, uint32_t* count, uint32_t cap, uint32_t grid_x) {
  if (!rows || !queries || !thr || !out || !count || !metric_ok(metric)) return -1;
  if (n_rows < 1 || n_rows >= MAX_ROWS || pitch4 < 1 || pitch4 > (1u << 20) || nq < 1 || nq > 65535 || grid_x < 1) return -1;
  if ((uint64_t)nq * cap > out_len) return -1;
  if (mask && mask_words < (n_rows + 31) / 32) return -1;
  const range_fn fn = metric == WDBX_METRIC_L2 ? pick_range_scan<WDBX_METRIC_L2>(pitch4) : pick_range_scan<WDBX_METRIC_COSINE>(pitch4);
  if (!fn) return -1;
  const RangeForm f = range_scan_form(pitch4);
  if (f.NI && (uint64_t)f.P * f.NI < pitch4) return -1;  // (an unrolled instance shorter than the row)
  const uint64_t groups = (n_rows + (64 / f.P) - 1) / (64 / f.P);
  if (groups + 4 * 4 * (uint64_t)grid_x >= (1ull << 32)) return -1;  // (cur + u * W for up to 4 passes)
  Bufs b;
  RangeArgs a = {};
  a.rows = (const f4*)b.up(rows, (size_t)n_rows * pitch4 * sizeof(f4));
  a.queries = (const f4*)b.up(queries, (size_t)nq * pitch4 * sizeof(f4));
  a.thr = (const float*)b.up(thr, (size_t)nq * sizeof(float));
  a.mask = (const uint32_t*)b.up(mask, (size_t)mask_words * sizeof(uint32_t));
  a.n_rows = (uint32_t)n_rows;
  a.pitch4 = pitch4;
  a.out = (u64*)b.up(out, (size_t)out_len * sizeof(u64));
  a.count = (uint32_t*)b.up(count, (size_t)nq * sizeof(uint32_t));
  a.cap = cap;
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(grid_x, nq), dim3(256), 0, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, a.out, (size_t)out_len * sizeof(u64));
  b.down(count, a.count, (size_t)nq * sizeof(uint32_t));
  return finish(b);
}

// range_filter_kernel<metric>, grid (grid_x, nq): cand: [cand_len] >= nq * cand_cap keys, of which query q's first
// min(cand_count[q], cand_cap) are read -- each must name a row < n_rows; out, count as for scn_range_scan.
int scn_range_filter(int metric, const float* rows, uint64_t n_rows, uint32_t pitch4, const float* queries, uint32_t nq, const float* thr,
                     const u64* cand, uint64_t cand_len, const uint32_t* cand_count, uint32_t cand_cap, u64* out, uint64_t out_len,
                     uint32_t* count, uint32_t cap, uint32_t grid_x) {
  if (!rows || !queries || !thr || !cand || !cand_count || !out || !count || !metric_ok(metric)) return -1;
  if (n_rows < 1 || n_rows >= MAX_ROWS || pitch4 < 1 || pitch4 > (1u << 20) || nq < 1 || nq > 65535 || grid_x < 1 || grid_x > (1u << 20)) return -1;
  if ((uint64_t)nq * cap > out_len || (uint64_t)nq * cand_cap > cand_len) return -1;
  for (uint32_t q = 0; q < nq; ++q)
    for (uint32_t j = 0; j < std::min(cand_count[q], cand_cap); ++j)
      if ((uint64_t)(~(uint32_t)(cand[(size_t)q * cand_cap + j] & 0xFFFFFFFFull)) >= n_rows) return -1;
  Bufs b;
  RangeArgs a = {};
  a.rows = (const f4*)b.up(rows, (size_t)n_rows * pitch4 * sizeof(f4));
  a.queries = (const f4*)b.up(queries, (size_t)nq * pitch4 * sizeof(f4));
  a.thr = (const float*)b.up(thr, (size_t)nq * sizeof(float));
  a.n_rows = (uint32_t)n_rows;
  a.pitch4 = pitch4;
  a.out = (u64*)b.up(out, (size_t)out_len * sizeof(u64));
  a.count = (uint32_t*)b.up(count, (size_t)nq * sizeof(uint32_t));
  a.cap = cap;
  a.cand = (const u64*)b.up(cand, (size_t)cand_len * sizeof(u64));
  a.cand_count = (const uint32_t*)b.up(cand_count, (size_t)nq * sizeof(uint32_t));
  a.cand_cap = cand_cap;
  if (b.err != hipSuccess) return finish(b);
  if (metric == WDBX_METRIC_L2)
    hipLaunchKernelGGL(range_filter_kernel<WDBX_METRIC_L2>, dim3(grid_x, nq), dim3(256), 0, nullptr, a);
  else
    hipLaunchKernelGGL(range_filter_kernel<WDBX_METRIC_COSINE>, dim3(grid_x, nq), dim3(256), 0, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, a.out, (size_t)out_len * sizeof(u64));
  b.down(count, a.count, (size_t)nq * sizeof(uint32_t));
  return finish(b);
}

}  // extern "C"
