// host_join.h -- the device-free host side of wdbx_index_self_join: argument checks, the anchor block by row pitch, the blocks
// and tiles of the triangle, LDS, grid, the first size of the candidate buffer, the route cut, and the tile test (DESIGN.md
// section 4.23) -- the functions the sweep's epilogue and its host check share.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/join_harness.cpp (plain g++ in the CPU suite,
// tests/test_join_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define JOIN_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define JOIN_HD static inline
#endif

constexpr int JOIN_TILE_ROWS = 256;                 // candidate rows of one tile: 8 waves x 32 rows (G8_ROWS)
constexpr uint32_t JOIN_MAX_PITCH8 = 1536;          // bytes of a row's i8 image the sweep serves
constexpr size_t JOIN_LDS_BLOCK_MAX = 96 * 1024;    // the resident anchor block
constexpr uint64_t JOIN_PAIR_BYTES_MAX = 2ull << 30;  // a candidate buffer grown past this fails the call
constexpr uint64_t JOIN_PAIR_CAP_MIN = 64;
// eligible rows below which the exact route answers: under four anchor blocks the sweep keeps four workgroups busy while the
// fp32 range scan spreads the same rows over every CU.  Arithmetic, not a measurement.
constexpr int64_t JOIN_MIN_ROWS_DEFAULT = 1024;
constexpr int64_t JOIN_EXACT_MAX_ROWS_DEFAULT = 65536;
// exact_score's rounding: a product passes through at most pitch / 256 + 8 <= 14 roundings up to 1536 dimensions,
// gamma_14 = 14 u / (1 - 14 u) < 8.4e-7, u = 2^-24 (section 4.23 derives it)
constexpr float JOIN_GAMMA = 2e-6f;

enum { JOIN_PATH_NONE = 0, JOIN_PATH_SWEEP = 1, JOIN_PATH_EXACT = 2 };  // read-only option "last_join_path"
enum JoinCheck { JOIN_OK = 0, JOIN_NAN_THRESHOLD, JOIN_NULL_OFFSETS, JOIN_NO_BUFFERS };
// why a call left the sweep (the refusal above join_exact_max_rows names it)
enum JoinWhy { JOIN_WHY_NONE = 0, JOIN_WHY_PITCH, JOIN_WHY_SHADOW, JOIN_WHY_FEW_ROWS };

// what can be refused before the handle is looked at (the mask's length is checked under the lock: check_mask_words)
static inline JoinCheck join_validate(float threshold, bool have_offsets, uint64_t capacity, bool have_rows, bool have_scores) {
  if (threshold != threshold) return JOIN_NAN_THRESHOLD;
  if (!have_offsets) return JOIN_NULL_OFFSETS;
  if (capacity && (!have_rows || !have_scores)) return JOIN_NO_BUFFERS;
  return JOIN_OK;
}

// 32-row units of an anchor block: 128 rows up to 768 bytes of i8 image, 64 up to 1536; 0: no sweep.  (A 256-row block for rows
// up to 384 bytes fits the LDS but not the registers: its 128 accumulators leave the epilogue no room without scratch.)
static inline int join_ct8(uint32_t pitch8) {
  if (!pitch8 || pitch8 % 128 || pitch8 > JOIN_MAX_PITCH8) return 0;
  return pitch8 <= 768 ? 4 : 2;
}

struct JoinPlan {
  int path = JOIN_PATH_NONE;
  int why = JOIN_WHY_NONE;
  bool refused = false;      // the exact route above join_exact_max_rows
  int ct8 = 0;
  uint32_t block_rows = 0;   // anchors of one block
  uint32_t blocks = 0;       // anchor blocks: [i * block_rows, (i + 1) * block_rows) cut at n_rows
  uint32_t tiles = 0;        // candidate tiles of 256 rows
  size_t lds = 0;            // dynamic LDS: the anchor block verbatim + its anchors' squared norms (L2)
  uint32_t grid = 0;         // persistent workgroups: one per CU at most
  uint64_t pair_cap = 0;     // entries of the candidate buffer at the first sweep
  uint64_t tile_visits = 0;  // sum over the blocks of the tiles each one streams
};

// first tile of block i (the one that holds its own rows) and how many it streams
static inline uint32_t join_block_first_tile(const JoinPlan& p, uint32_t i) {
  return (uint32_t)((uint64_t)i * p.block_rows / JOIN_TILE_ROWS);
}
static inline uint32_t join_block_tiles(const JoinPlan& p, uint32_t i) { return p.tiles - join_block_first_tile(p, i); }

static inline size_t join_lds_bytes(int ct8, uint32_t pitch8) { return (size_t)32 * ct8 * pitch8 + (size_t)32 * ct8 * sizeof(float); }

// n_rows: the handle's rows; eligible: unmasked rows without a NaN; pitch8: the i8 image's bytes per row (0: the batched path
// would not use the int8 tiles for this handle); shadow: shadow copy G is in place; max_grid / pair_cap_opt / min_rows /
// exact_max_rows: the options join_max_grid, join_pair_cap, join_min_rows, join_exact_max_rows.
static inline JoinPlan join_plan(uint64_t n_rows, uint64_t eligible, uint32_t pitch8, bool shadow, int cu_count, uint64_t max_grid,
                                 uint64_t pair_cap_opt, uint64_t min_rows, uint64_t exact_max_rows) {
  JoinPlan p;
  if (!n_rows || eligible < 2) return p;  // (no pair: nothing launched)
  p.ct8 = join_ct8(pitch8);
  // (the caller asks for the shadow copy only when the first two conditions let the sweep run)
  p.why = !p.ct8 ? JOIN_WHY_PITCH : eligible < min_rows ? JOIN_WHY_FEW_ROWS : !shadow ? JOIN_WHY_SHADOW : JOIN_WHY_NONE;
  if (p.why != JOIN_WHY_NONE) {
    p.path = JOIN_PATH_EXACT;
    p.refused = n_rows > exact_max_rows;
    return p;
  }
  p.path = JOIN_PATH_SWEEP;
  p.block_rows = 32u * (uint32_t)p.ct8;
  p.blocks = (uint32_t)((n_rows + p.block_rows - 1) / p.block_rows);
  p.tiles = (uint32_t)((n_rows + JOIN_TILE_ROWS - 1) / JOIN_TILE_ROWS);
  p.lds = join_lds_bytes(p.ct8, pitch8);
  const uint64_t cus = (uint64_t)std::max(cu_count, 1);
  p.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)p.blocks, cus, max_grid ? max_grid : cus}));
  // the first buffer: four candidates per row (duplicates at join thresholds are a few per cent of the rows), 64 Ki at least
  p.pair_cap = pair_cap_opt ? std::max<uint64_t>(pair_cap_opt, JOIN_PAIR_CAP_MIN)
                            : std::min<uint64_t>(std::max<uint64_t>(4 * n_rows, 65536), JOIN_PAIR_BYTES_MAX / 8);
  for (uint32_t i = 0; i < p.blocks; ++i) p.tile_visits += join_block_tiles(p, i);
  return p;
}
// whether a buffer of `pairs` entries may be allocated at all
static inline bool join_pairs_fit(uint64_t pairs) { return pairs <= JOIN_PAIR_BYTES_MAX / 8; }

// ---- the tile test -----------------------------------------------------------------------------
// Rows a of group A and b of group B: a = s_A (n_a + delta_a), b = s_B (n_b + delta_b), D = n_a . n_b, and the group table's
// {s, a_g >= s |n|_2, b_g >= s |delta|_2} of both:
//     |a.b - s_A s_B D| <= a_A b_B + b_A (a_B + b_B) = slack
// exact_score's fp32 value exceeds the real one by at most gamma |a| |b| <= gamma (a_A + b_A)(a_B + b_B).
//   cosine / inner product: fl(a.b) >= t  =>  D >= (t - slack - gamma term) / (s_A s_B): ONE integer T per group pair.
//   L2: fl(|a - b|^2) <= t  =>  real <= t (1 + 1e-5)  =>  D - (|a|^2 + |b|^2) w >= Tf,  w = 1 / (2 s_A s_B),
//       Tf = (-t (1 + 1e-5) / 2 - slack) / (s_A s_B); the norms are the cached fp32 ones taken 1e-4 low.
// Every rounding goes to the keeping side.  T = INT_MIN / Tf = -inf keep every pair of the two groups: a threshold that is not
// finite (an infinite bound, an infinite t), and a product of scales too small to divide by.
struct JoinGroup {
  float s, a, b;
};
struct JoinCut {
  int T;        // cosine: keep iff D >= T
  float Tf, w;  // L2: keep iff D - (|a|^2 + |b|^2) w >= Tf (join_l2_col, join_l2_keep)
};
JOIN_HD JoinCut join_cut(bool l2, float t, JoinGroup A, JoinGroup B) {
  JoinCut c;
  c.T = INT_MIN;
  c.Tf = -INFINITY;
  c.w = 0.f;
  const float ss = A.s * B.s;
  if (!(ss >= 1e-30f)) return c;
  const float slack = (A.a * B.b + A.b * (B.a + B.b)) * 1.00001f + 1e-37f;
  float num, mag;
  if (l2) {
    const float tt = t + 1e-5f * fabsf(t) + 1e-37f;
    num = -0.5f * tt - slack;
    mag = fabsf(tt) + slack;
  } else {
    const float gam = JOIN_GAMMA * (A.a + A.b) * (B.a + B.b) * 1.00001f;
    num = t - slack - gam;
    mag = fabsf(t) + slack + gam;
  }
  num -= 1e-6f * mag;
  float q = num / ss;
  q = q - 1e-5f * fabsf(q) - 1.0f;
  if (!(fabsf(q) < INFINITY)) return c;  // (NaN too)
  // |D| <= 127^2 * 1536 < 3e7: beyond it nothing, or everything, passes
  c.T = q > 3e7f ? INT_MAX : q < -3e7f ? INT_MIN : (int)floorf(q);
  c.Tf = q;
  c.w = 0.5f / ss;
  return c;
}
// L2: a cached squared norm taken to the keeping side: NaN (a removed row, never a result) -> +inf, overflowed -> -inf
JOIN_HD float join_norm_low(float cn) { return cn != cn ? INFINITY : cn < INFINITY ? cn * 0.9999f : -INFINITY; }
// L2: the threshold of one anchor column, rounded down; ua = join_norm_low(|a|^2)
JOIN_HD float join_l2_col(float ua, JoinCut c) {
  const float x = ua * c.w;
  return (c.Tf + x) - 1e-5f * (fabsf(c.Tf) + fabsf(x)) - 1.0f;
}
// L2: the test of one accumulator against its column's threshold; ub = join_norm_low(|b|^2).  A NaN keeps.
JOIN_HD bool join_l2_keep(int D, float ub, JoinCut c, float col) {
  const float d = (float)D;
  const float f = fmaf(-ub, c.w, d) + 1e-5f * fabsf(d);
  return !(f < col);
}
