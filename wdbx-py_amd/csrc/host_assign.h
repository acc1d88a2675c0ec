// host_assign.h -- the device-free host side of wdbx_index_assign: argument checks, the centre blocks of the tile pass, its LDS
// and grid, the grids of the exact and the sums passes, the partial sums one call combines, scratch sizes and the coefficients of
// the certainty bound.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/assign_harness.cpp (plain g++ in the CPU suite,
// tests/test_assign_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

constexpr int ASSIGN_MAX_CENTERS = 4096;  // = WDBX_MAX_CENTERS
// the tile pass: a workgroup's 4 waves take 32 stored rows each (one MFMA column tile), against a block of 32 * mt centres
constexpr int ASSIGN_TILE_ROWS = 128;
constexpr int ASSIGN_BK = 32;             // floats of K staged per chunk
constexpr int ASSIGN_LD = ASSIGN_BK + 4;  // padded LDS row (floats): conflict-free ds_read_b128, as the fp32 tile kernel's
constexpr int ASSIGN_BLOCK_MAX = 128;     // centres per block at most (mt = 4: 64 accumulator registers per lane)
// what two resident workgroups may take each of a CU's 160 KiB
constexpr size_t ASSIGN_LDS_LIMIT = 80 * 1024;
// the partial sums of one call (one per wave of the sums pass) stay within this much scratch
constexpr size_t ASSIGN_PARTIALS_BUDGET = 256u << 20;
constexpr size_t ASSIGN_PARTIALS_KEEP = 64u << 20;  // ... and more than this is released when the call ends
constexpr int ASSIGN_EXACT_BLOCK = 8;    // centres per exact_score_block of the pass over the ambiguous rows

// Workgroups of the tile pass a CU holds at once (= waves per SIMD its registers are held to, kernels_assign.h): two, which
// the LDS limit above allows -- except the L2 instance with 128 centres per block, whose norm hand-over needs a few registers
// more than 256 and gets one.  The persistent grid follows it.
constexpr int assign_tile_waves(bool l2, int mt) { return l2 && mt == 4 ? 1 : 2; }

enum AssignCheck { ASSIGN_OK = 0, ASSIGN_BAD_COUNT, ASSIGN_NULL_CENTERS, ASSIGN_NO_OUTPUT };

// what can be refused before the handle is looked at (the mask's length is checked under the lock: check_mask_words)
static inline AssignCheck assign_validate(int n_centers, bool have_centers, bool any_output) {
  if (n_centers < 1 || n_centers > ASSIGN_MAX_CENTERS) return ASSIGN_BAD_COUNT;
  if (!have_centers) return ASSIGN_NULL_CENTERS;
  if (!any_output) return ASSIGN_NO_OUTPUT;
  return ASSIGN_OK;
}

struct AssignPlan {
  int mt = 0;               // 32-centre MFMA row tiles per block: 1, 2 or 4 (the instance)
  int block = 0;            // centres per block = 32 * mt
  int n_blocks = 0;         // blocks [b * block, min(n_centers, (b + 1) * block)): every centre in exactly one
  int slots = 0;            // n_blocks * block centre slots staged on the device, the unused ones zero and never chosen
  size_t lds = 0;           // dynamic LDS of the tile pass: two buffers of (rows + centres) K-chunks and the blocks' norms
  uint32_t tiles = 0;       // tiles of ASSIGN_TILE_ROWS stored rows
  uint32_t grid = 0;        // persistent workgroups of the tile pass: as many as are resident at once (assign_tile_waves per CU)
  uint32_t prep_grid = 0;   // one wave per centre slot
  uint32_t exact_grid = 0;  // of the pass over all rows (winner's score); the list pass is sized by the list
  uint32_t partials = 0;    // P: waves of the sums pass, each with consecutive rows and partial sums of its own
  uint32_t sums_grid = 0;   // = ceil(P / 4)
  uint64_t rows_per_partial = 0;
  size_t centre_bytes = 0;  // slots * pitch floats
  size_t aux_bytes = 0;     // slots norms, then {largest centre norm, listed rows} words
  size_t partial_bytes = 0; // P * (n_centers * pitch floats + n_centers counters)
};

// centres of block b
static inline int assign_block_first(const AssignPlan& p, int b) { return b * p.block; }
static inline int assign_block_count(const AssignPlan& p, int n_centers, int b) {
  return std::min(p.block, n_centers - assign_block_first(p, b));
}

static inline size_t assign_lds_bytes(int block) {
  return (size_t)2 * (ASSIGN_TILE_ROWS + block) * ASSIGN_LD * sizeof(float) + (size_t)2 * block * sizeof(float);
}

// grid of a pass with one wave per item, four waves per workgroup, at most `cap` workgroups
static inline uint32_t assign_wave_grid(uint64_t items, uint32_t cap) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((items + 3) / 4, cap));
}

// n_centers in [1, ASSIGN_MAX_CENTERS] (assign_validate), pitch = the handle's row pitch in floats (a multiple of 4).
// The LDS bytes do not depend on the pitch: K is walked in chunks of ASSIGN_BK floats whatever the row length.
static inline AssignPlan assign_plan(uint64_t n_rows, int n_centers, uint32_t pitch, int cu_count, bool l2) {
  AssignPlan p;
  p.mt = n_centers <= 32 ? 1 : n_centers <= 64 ? 2 : 4;
  p.block = 32 * p.mt;
  p.n_blocks = (n_centers + p.block - 1) / p.block;
  p.slots = p.n_blocks * p.block;
  p.lds = assign_lds_bytes(p.block);
  const uint32_t cus = (uint32_t)std::max(cu_count, 1);
  p.tiles = (uint32_t)((n_rows + ASSIGN_TILE_ROWS - 1) / ASSIGN_TILE_ROWS);
  p.grid = std::max<uint32_t>(1, std::min<uint32_t>(p.tiles, (uint32_t)assign_tile_waves(l2, p.mt) * cus));
  p.prep_grid = (uint32_t)(p.slots + 3) / 4;
  p.exact_grid = assign_wave_grid(n_rows, 8 * cus);
  const size_t per_partial = (size_t)n_centers * pitch * sizeof(float) + (size_t)n_centers * sizeof(uint32_t);
  uint64_t P = std::min<uint64_t>((uint64_t)8 * cus, ASSIGN_PARTIALS_BUDGET / per_partial);
  P = std::max<uint64_t>(1, std::min<uint64_t>(P, (n_rows + 63) / 64));  // (at least 64 rows per partial: its zeroing is amortised)
  p.rows_per_partial = n_rows ? (n_rows + P - 1) / P : 0;
  if (p.rows_per_partial) P = (n_rows + p.rows_per_partial - 1) / p.rows_per_partial;  // (no empty partial)
  p.partials = (uint32_t)P;
  p.sums_grid = (uint32_t)((P + 3) / 4);
  p.centre_bytes = (size_t)p.slots * pitch * sizeof(float);
  p.aux_bytes = (size_t)p.slots * sizeof(float) + 2 * sizeof(uint32_t);
  p.partial_bytes = (size_t)P * per_partial;
  return p;
}

// The certainty bound's coefficients.  Both arithmetics -- the MFMA chain of the tile pass and
// exact_score's lane-strided chain with its tree -- are fp32 fma chains of at most pitch + 18 roundings: gamma = n u / (1 - n u),
// u = 2^-24, widened as the selection paths widen it; under = the absolute term of gradual underflow per dot product.
struct AssignBound {
  float gamma;
  float under;
};
static inline AssignBound assign_bound(uint32_t pitch) {
  const float nu = (float)(pitch + 18) * 5.9604645e-08f;
  AssignBound b;
  b.gamma = 1.02f * nu / (1.0f - nu) * 1.0102f;
  b.under = ldexpf((float)(pitch + 18), -149);
  return b;
}
