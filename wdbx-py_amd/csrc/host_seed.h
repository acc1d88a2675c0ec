// host_seed.h -- the device-free host side of wdbx_index_seed_centers (k-means++ seeding): argument
// checks, the L2 shift, the chunks of resident candidates with their LDS bytes, the grids, the scratch sizes -- and the two
// functions the kernels and their host check share: the integer weight of a score and the target of a draw.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/seed_harness.cpp (plain g++ in the CPU suite,
// tests/test_seed_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SEED_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define SEED_HD static inline
#endif

constexpr int SEED_MAX_CENTERS = 4096;          // = WDBX_MAX_CENTERS
constexpr int SEED_MAX_TRIALS = 16;             // = WDBX_MAX_SEED_TRIALS
constexpr uint32_t SEED_BLOCK_ROWS = 1024;      // rows behind one u64 block sum: a workgroup of 256 threads, 4 rows each
constexpr size_t SEED_LDS_BUDGET = 64 * 1024;   // the resident candidates of one eval launch
constexpr size_t SEED_LDS_MAX = 160 * 1024;     // what a workgroup may take at all: one candidate row must fit
constexpr uint32_t SEED_W_UNSET = 0xFFFFFFFFu;  // a row's weight before the first centre: the minimum with anything is the other
constexpr int SEED_SHIFT_LIMIT = 100;           // |shift| at most: ldexpf stays within fp32 for every finite distance

enum SeedCheck { SEED_OK = 0, SEED_BAD_CENTERS, SEED_BAD_TRIALS, SEED_NULL_DRAWS, SEED_NULL_OUTPUT };

// what can be refused before the handle is looked at (the mask's length and the eligible rows are checked under the lock)
static inline SeedCheck seed_validate(int n_centers, int n_trials, bool have_draws, bool have_rows) {
  if (n_centers < 1 || n_centers > SEED_MAX_CENTERS) return SEED_BAD_CENTERS;
  if (n_trials < 1 || n_trials > SEED_MAX_TRIALS) return SEED_BAD_TRIALS;
  if (!have_draws) return SEED_NULL_DRAWS;
  if (!have_rows) return SEED_NULL_OUTPUT;
  return SEED_OK;
}

// ---- what host and device share ---------------------------------------------------------------------------------------------
// The weight of a row whose exact score against a centre row is s (exact_score's bits: the inner product, or the negated squared
// distance).  Cosine: the distance 1 - s clamped to [0, 2] in units of 2^-30.  L2: the squared distance in units of 2^-shift,
// saturated at 2^31 - 1.  A NaN score (it cannot come from two eligible rows unless a sum overflowed) is 0 for cosine and the
// saturation for L2.  Every step is exact in fp32 (a subtraction from 1 aside, which rounds once, the same way on both sides):
// a power-of-two scaling and a truncation.
SEED_HD uint32_t seed_weight(bool l2, float s, int shift) {
  if (l2) {
    const float v = ldexpf(-s, shift);
    if (!(v < 2147483648.0f)) return 2147483647u;
    return v > 0.0f ? (uint32_t)v : 0u;
  }
  float t = 1.0f - s;
  if (!(t > 0.0f)) t = 0.0f;
  if (t > 2.0f) t = 2.0f;
  return (uint32_t)(t * 1073741824.0f);
}

// the high half of a 64 x 64 bit product: the target floor(draw * W / 2^64) of a raw 64-bit draw over a total weight W, always < W
SEED_HD uint64_t seed_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------
// The largest shift with 4 M 2^shift < 2^31 for the largest finite eligible squared norm M: no squared distance between two
// eligible rows (<= 4 M) saturates but by rounding.  M = m 2^e with m in [0.5, 1), so that is 29 - e; M = 0 (every eligible row
// is zero, every distance too) and tiny or huge M stop at the limit.
static inline int seed_shift(float max_norm2) {
  if (!(max_norm2 > 0.0f)) return SEED_SHIFT_LIMIT;
  int e = 0;
  (void)frexpf(max_norm2, &e);
  return std::max(-SEED_SHIFT_LIMIT, std::min(SEED_SHIFT_LIMIT, 29 - e));
}

struct SeedPlan {
  bool fits = false;         // one candidate row fits a workgroup's LDS
  uint32_t resident = 0;     // candidates of one eval launch at most
  uint32_t passes = 0;       // eval launches of a step with n_trials candidates (the first step has one candidate: one launch)
  size_t lds = 0;            // dynamic LDS of an eval launch with `resident` candidates (a short last chunk takes less)
  uint32_t eval_grid = 0;    // persistent grid: workgroups of 4 waves, each wave a contiguous span of rows
  uint32_t span = 0;         // rows of one wave's span (even: a wave walks its span two rows at a time)
  uint32_t blocks = 0;       // blocks of SEED_BLOCK_ROWS rows = block sums
  uint32_t apply_grid = 0;   // workgroups of the apply and the init launch (a grid-stride walk over the blocks)
  // one allocation of the call's state, offsets in bytes: the rows' weights | the dead bits (ineligible or chosen) | the block
  // sums | the step's potentials | the step's candidate rows | the chosen rows | their potentials | the draws
  size_t off_dead = 0, off_sums = 0, off_pot = 0, off_cand = 0, off_rows = 0, off_outpot = 0, off_draws = 0, state_bytes = 0;
  size_t scratch_bytes = 0;  // u32 [n_trials][rows]: every candidate's weights of the step
};

// bytes of LDS for n resident candidates of `pitch` floats: the rows themselves; the workgroup's reduction (4 waves x 16 sums)
// reuses their first bytes behind a barrier and needs 512 of them, which a single short row may not have
static inline size_t seed_lds_bytes(uint32_t n, uint32_t pitch) {
  return std::max<size_t>((size_t)n * pitch * sizeof(float), (size_t)4 * SEED_MAX_TRIALS * sizeof(uint64_t));
}
// the instance of the eval kernel for n resident candidates: its candidate block (1, 4 or 16 accumulators per loaded row)
static inline int seed_block(uint32_t n) { return n <= 1 ? 1 : n <= 4 ? 4 : 16; }

// pitch: floats of a stored row (a multiple of 4); max_resident: option "seed_max_resident" (0 = the plan's choice)
static inline SeedPlan seed_plan(uint64_t n_rows, int n_centers, int n_trials, uint32_t pitch, int cu_count, uint64_t max_resident = 0) {
  SeedPlan p;
  const size_t row_bytes = (size_t)pitch * sizeof(float);
  p.fits = row_bytes > 0 && row_bytes <= SEED_LDS_MAX;
  if (!p.fits || !n_rows) return p;
  uint64_t r = std::max<uint64_t>(1, SEED_LDS_BUDGET / row_bytes);
  r = std::min<uint64_t>(r, (uint64_t)n_trials);
  if (max_resident) r = std::min<uint64_t>(r, max_resident);
  p.resident = (uint32_t)r;
  p.passes = ((uint32_t)n_trials + p.resident - 1) / p.resident;
  p.lds = seed_lds_bytes(p.resident, pitch);
  const uint64_t cus = (uint64_t)std::max(cu_count, 1);
  // two workgroups per CU are resident beside 64 KiB of LDS each; no more waves than pairs of rows
  p.eval_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(2 * cus, (n_rows + 7) / 8));
  const uint64_t waves = (uint64_t)p.eval_grid * 4;
  p.span = (uint32_t)(((n_rows + waves - 1) / waves + 1) / 2 * 2);
  p.blocks = (uint32_t)((n_rows + SEED_BLOCK_ROWS - 1) / SEED_BLOCK_ROWS);
  p.apply_grid = (uint32_t)std::min<uint64_t>(p.blocks, 8 * cus);
  auto up8 = [](size_t v) { return (v + 7) / 8 * 8; };
  p.off_dead = up8((size_t)n_rows * sizeof(uint32_t));
  p.off_sums = p.off_dead + up8((size_t)p.blocks * (SEED_BLOCK_ROWS / 32) * sizeof(uint32_t));
  p.off_pot = p.off_sums + (size_t)p.blocks * sizeof(uint64_t);
  p.off_cand = p.off_pot + (size_t)SEED_MAX_TRIALS * sizeof(uint64_t);
  p.off_rows = p.off_cand + (size_t)SEED_MAX_TRIALS * sizeof(uint32_t);
  p.off_outpot = p.off_rows + (size_t)n_centers * sizeof(uint64_t);
  p.off_draws = p.off_outpot + (size_t)n_centers * sizeof(uint64_t);
  p.state_bytes = p.off_draws + (size_t)n_centers * n_trials * sizeof(uint64_t);
  p.scratch_bytes = (size_t)n_trials * n_rows * sizeof(uint32_t);
  return p;
}
