// host_assign8.h -- the device-free host side of the int8 route of wdbx_index_assign (kernels_assign8.h, DESIGN.md section
// 4.20b): which calls take it and why not, the centre blocks, LDS, grid and first candidate capacity of the sweep, and the
// inequality behind "every possible winner is a candidate" -- the functions the sweep's epilogue and its host check share.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/assign8_harness.cpp (plain g++ in the CPU suite,
// tests/test_assign8_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "host_assign.h"
#include "host_join.h"

constexpr int ASSIGN8_TILE_ROWS = 256;               // stored rows of one tile: 8 waves x 32 rows (G8_ROWS)
constexpr uint32_t ASSIGN8_MAX_PITCH8 = 1024;        // bytes of a row's i8 image the sweep serves: two centre blocks fit the LDS
constexpr size_t ASSIGN8_LDS_LIMIT = 160 * 1024;     // a CU's LDS: one workgroup of 512 threads is resident
constexpr int64_t ASSIGN8_MIN_ROWS_DEFAULT = 65536;  // option assign_i8_min_rows
constexpr int64_t ASSIGN8_MIN_ROWS_FLOOR = 32768;    // ... which never goes below this: smaller handles keep the fp32 tiles
// What option assign_i8 = -1 means.  The int8 route has not been timed against the fp32 tiles at corpus size yet (DESIGN.md
// section 4.20b, profiles/assign_i8/README.md): until it has, "auto" keeps the fp32 route at every size.
constexpr bool ASSIGN8_AUTO_ON = false;

enum { ASSIGN_PATH_NONE = 0, ASSIGN_PATH_FP32 = 1, ASSIGN_PATH_I8 = 2 };  // read-only option "last_assign_path"
// why a call left the int8 route (read-only option "last_assign_why")
enum Assign8Why { ASSIGN8_WHY_NONE = 0, ASSIGN8_WHY_OFF, ASSIGN8_WHY_PITCH, ASSIGN8_WHY_FEW_ROWS, ASSIGN8_WHY_SHADOW };

// 32-centre units of a centre block: 128 centres up to 512 bytes of i8 image, 64 up to 1024 (two blocks resident: the next one
// is staged under the current one's matrix ops); 0: no sweep
static inline int assign8_ct8(uint32_t pitch8) {
  if (!pitch8 || pitch8 % 128 || pitch8 > ASSIGN8_MAX_PITCH8) return 0;
  return pitch8 <= 512 ? 4 : 2;
}
// two centre blocks as they lie in the quantised image, and {s_c, |c|^2} per centre of both
static inline size_t assign8_lds_bytes(int ct8, uint32_t pitch8) { return (size_t)2 * 32 * ct8 * (pitch8 + 2 * sizeof(float)); }

// What can be said before shadow copy G is asked for (a call on the fp32 route must not allocate it).  opt: option assign_i8
// (-1 auto, 0 never, 1 whenever the shape allows); pitch8: bytes of a row's i8 image, 0 = the handle has none.
static inline Assign8Why assign8_why(int64_t opt, uint64_t n_rows, uint64_t min_rows, uint32_t pitch8) {
  if (opt == 0 || (opt < 0 && !ASSIGN8_AUTO_ON)) return ASSIGN8_WHY_OFF;
  if (!assign8_ct8(pitch8)) return ASSIGN8_WHY_PITCH;
  if (opt < 0 && n_rows < std::max<uint64_t>(min_rows, (uint64_t)ASSIGN8_MIN_ROWS_FLOOR)) return ASSIGN8_WHY_FEW_ROWS;
  return ASSIGN8_WHY_NONE;
}

struct Assign8Plan {
  int path = ASSIGN_PATH_FP32;
  int why = ASSIGN8_WHY_NONE;
  int ct8 = 0;
  int block = 0;            // centres per block = 32 * ct8
  int n_blocks = 0;         // blocks [b * block, min(n_centers, (b + 1) * block)): every centre in exactly one
  int slots = 0;            // n_blocks * block quantised centre slots, the unused ones zero bytes and excluded
  size_t lds = 0;
  uint32_t tiles = 0;       // tiles of ASSIGN8_TILE_ROWS stored rows
  uint32_t grid = 0;        // persistent workgroups: one per CU at most
  uint32_t quant_grid = 0;  // one wave per centre slot
  uint64_t pair_cap = 0;    // entries of the candidate buffer at the first sweep
  size_t centre_bytes = 0;  // slots * pitch8
  size_t par_bytes = 0;     // slots * {s_c, |c|^2}, then the words {a_max, b_max}
};
static inline int assign8_block_first(const Assign8Plan& p, int b) { return b * p.block; }
static inline int assign8_block_count(const Assign8Plan& p, int n_centers, int b) {
  return std::min(p.block, n_centers - assign8_block_first(p, b));
}

// why: assign8_why's answer; shadow: shadow copy G is in place (asked for only when why is NONE); max_grid / pair_cap_opt: the
// options assign_max_grid and assign_pair_cap (0: the plan's choice).  The capacity rule, its floor and the byte limit are the
// self-join's (host_join.h): four candidates per row, 64 Ki at least; a count past the buffer grows it to that count.
static inline Assign8Plan assign8_plan(Assign8Why why, bool shadow, uint64_t n_rows, int n_centers, uint32_t pitch8, int cu_count,
                                       uint64_t max_grid, uint64_t pair_cap_opt) {
  Assign8Plan p;
  p.why = why != ASSIGN8_WHY_NONE ? why : !shadow ? ASSIGN8_WHY_SHADOW : ASSIGN8_WHY_NONE;
  if (p.why != ASSIGN8_WHY_NONE || !n_rows) return p;
  p.path = ASSIGN_PATH_I8;
  p.ct8 = assign8_ct8(pitch8);
  p.block = 32 * p.ct8;
  p.n_blocks = (n_centers + p.block - 1) / p.block;
  p.slots = p.n_blocks * p.block;
  p.lds = assign8_lds_bytes(p.ct8, pitch8);
  p.tiles = (uint32_t)((n_rows + ASSIGN8_TILE_ROWS - 1) / ASSIGN8_TILE_ROWS);
  const uint64_t cus = (uint64_t)std::max(cu_count, 1);
  p.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)p.tiles, cus, max_grid ? max_grid : cus}));
  p.quant_grid = (uint32_t)(p.slots + 3) / 4;
  p.pair_cap = pair_cap_opt ? std::max<uint64_t>(pair_cap_opt, JOIN_PAIR_CAP_MIN)
                            : std::min<uint64_t>(std::max<uint64_t>(4 * n_rows, 65536), JOIN_PAIR_BYTES_MAX / 8);
  p.centre_bytes = (size_t)p.slots * pitch8;
  p.par_bytes = (size_t)p.slots * 2 * sizeof(float) + 2 * sizeof(uint32_t);
  return p;
}

// ---- the inequality ---------------------------------------------------------------------------
// Row r of group A and centre c: r = s_A (n_r + delta_r), c = s_c (n_c + delta_c), D = n_r . n_c; the group table's
// {s_A, a_A >= s_A |n_r|_2, b_A >= s_A |delta_r|_2} and, over the call's centres, a_max >= s_c |n_c|_2, b_max >= s_c |delta_c|_2:
//     |r.c - s_A s_c D| <= a_A b_max + b_A (a_max + b_max) = slack_A                     (Cauchy-Schwarz, as host_join.h)
// The sweep ranks by T(c) = s_A s_c D (cosine / inner product) or 2 s_A s_c D - |c|^2 (L2, |c|^2 the prepared fp32 norm);
// S(c) is the real r.c or 2 r.c - |c|^2.  assign8_bound >= |S(c) - T(c)|: slack_A (doubled for L2), the fp32 roundings of
// forming T (b_T: a convert, two products, one fma -- each relative 2^-24 of at most a_A a_max, or of that doubled plus
// |c|^2), the prepared norm's own rounding (gamma |c|^2, |c| <= a_max + b_max) and gradual underflow.
// exact_score's value E(c) is within b_E of S(c) (cosine) or of S(c) - |r|^2 (L2): section 4.20's bound, with the group's
// a_A + b_A >= |r| and a_max + b_max >= |c| for the norms.  With c* = exact_score's argmax and x the centre of the row's
// final best T:
//     T(c*) >= S(c*) - bound >= E(c*) - b_E - bound >= E(x) - b_E - bound >= S(x) - 2 b_E - bound >= T(x) - 2 (bound + b_E)
// and T(x) >= best_T(r) at every earlier moment: with margin = 2 (bound + b_E) the winner is always appended, and so is every
// centre whose E equals the winner's.  Every rounding goes to the keeping side; a margin that is not finite keeps nothing: the
// row goes to the listed exact pass (assign8_listed).
struct Assign8Group {
  float s, a, b;
};
struct Assign8Call {
  float a_max, b_max;  // over the call's centres (assign_quant_kernel)
  float gamma, under;  // assign_bound (host_assign.h)
};

// the value the sweep ranks centre c by for a row of a group with scale sA: D the integer dot product, sc the centre's scale,
// c2 its prepared squared norm (L2)
JOIN_HD float assign8_T(bool l2, float sA, float sc, int D, float c2) {
  const float p = sA * (sc * (float)D);
  return l2 ? fmaf(2.0f, p, -c2) : p;
}

// >= |S(c) - T(c)| for every row of the group and every centre of the call
JOIN_HD float assign8_bound(bool l2, Assign8Group A, Assign8Call c) {
  const float slack = (A.a * c.b_max + A.b * (c.a_max + c.b_max)) * 1.00001f + 1e-37f;
  const float nc = (c.a_max + c.b_max) * 1.00001f;
  const float prod = A.a * c.a_max * 1.00001f;  // >= |s_A s_c D|
  if (!l2) return (slack + 4e-7f * prod + 4.0f * c.under) * 1.0001f;
  return (2.0f * slack + 4e-7f * (2.0f * prod + nc * nc) + (c.gamma + 2e-7f) * nc * nc + 8.0f * c.under) * 1.0001f;
}

// b_E: exact_score's distance from S (section 4.20's b_exact, with the norms bounded through the tables)
JOIN_HD float assign8_exact_bound(bool l2, Assign8Group A, Assign8Call c) {
  const float nr = (A.a + A.b) * 1.00001f, nc = (c.a_max + c.b_max) * 1.00001f;
  return l2 ? (c.gamma * (nr + nc) * (nr + nc) + 6.0f * c.under) * 1.0001f : (c.gamma * nr * nc + c.under) * 1.0001f;
}

// one value per 64-row group and call: centre c is a candidate of row r while T(c) >= best_T(r) - margin
JOIN_HD float assign8_margin(bool l2, Assign8Group A, Assign8Call c) {
  return 2.0f * (assign8_bound(l2, A, c) + assign8_exact_bound(l2, A, c)) * 1.0001f;
}
// whether the rows of a group go to the listed exact pass: G does not vouch for the group, or its margin is not finite
JOIN_HD bool assign8_listed(float margin, float vouch) { return !(vouch > 0.f) || !(margin >= 0.f && margin < INFINITY); }
