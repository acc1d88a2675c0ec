// host_knn.h -- the device-free host side of wdbx_index_knn_graph: argument checks, the anchor and candidate tiles of the sweep,
// the capacity of an anchor's candidate list, LDS, scratch, the grid and passes, the cut below which the whole call takes the
// repair route, and the selection margin -- the one function the sweep and its host check share.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/knn_harness.cpp (plain g++ in the CPU suite,
// tests/test_knn_graph_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define KNN_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define KNN_HD static inline
#endif

constexpr int KNN_MAX_K = 64;            // = WDBX_MAX_GRAPH_K
// the sweep: a workgroup's 4 waves take 32 anchors each (one MFMA column tile) against candidate tiles of 4 MFMA row tiles
constexpr int KNN_ANCHOR_TILE = 128;
constexpr int KNN_CAND_TILE = 128;
constexpr int KNN_BK = 64;               // bf16 elements of K staged per chunk
constexpr int KNN_LDB = KNN_BK * 2 + 16; // bytes of a padded LDS row: conflict-free ds_read_b128, as gemm_bf16w8_kernel's
// what two resident workgroups may take each of a CU's 160 KiB: the limit of assign's plan
constexpr size_t KNN_LDS_LIMIT = 80 * 1024;
constexpr size_t KNN_SCRATCH_BUDGET = 256u << 20;
// eligible rows below which the whole call is answered by the repair route: under four anchor tiles the sweep keeps at most
// three workgroups busy while matrix_kernel's rounds spread the same few rows over every CU
constexpr uint64_t KNN_TILE_MIN_ROWS = 4 * KNN_ANCHOR_TILE;

enum { KNN_PATH_NONE = 0, KNN_PATH_TILES = 1, KNN_PATH_REPAIR = 2 };  // read-only option "last_knn_path"
enum KnnCheck { KNN_OK = 0, KNN_BAD_K, KNN_NULL_OUTPUT };

// what can be refused before the handle is looked at (the mask's length is checked under the lock: check_mask_words)
static inline KnnCheck knn_validate(int k, bool have_idx, bool have_score) {
  if (k < 1 || k > KNN_MAX_K) return KNN_BAD_K;
  if (!have_idx || !have_score) return KNN_NULL_OUTPUT;
  return KNN_OK;
}

struct KnnPlan {
  int path = KNN_PATH_NONE;
  uint32_t cap = 0;          // entries of one anchor's candidate list: >= k + one candidate tile, a multiple of 64
  size_t lds = 0;            // dynamic LDS of the sweep: two buffers of (anchor + candidate) K-chunks, two sets of candidate
                             // norms, the anchors' fill counters
  uint32_t anchor_tiles = 0, cand_tiles = 0;
  uint32_t grid = 0;         // workgroups of one pass = anchor tiles swept at once: what is resident, within the scratch budget
  uint32_t passes = 0;       // launches of the sweep: anchor tiles [p * grid, (p + 1) * grid), in order
  uint32_t exact_grid = 0;   // of the exact pass over one pass's anchors (one wave per anchor)
  size_t list_bytes = 0;     // grid * KNN_ANCHOR_TILE lists of cap keys
  size_t count_bytes = 0;    // grid * KNN_ANCHOR_TILE fill counters, then the call's appends counter (u64) and largest norm (a word)
  size_t flag_bytes = 0;     // one word per stored row
};

// list capacity: the k kept entries, the rows within the margin of them (as many again and a tile's worth are allowed for)
// and one candidate tile of appends before the next compaction.  What is allowed for the margin holds about k + 128 rows
// within 2b of the k-th neighbour: an anchor with more of them there overflows and takes the repair route.
constexpr uint32_t knn_list_cap(int k) { return ((uint32_t)(2 * k) + 2 * KNN_CAND_TILE + 63) / 64 * 64; }

static inline size_t knn_lds_bytes() {
  return (size_t)2 * (KNN_ANCHOR_TILE + KNN_CAND_TILE) * KNN_LDB + (size_t)2 * KNN_CAND_TILE * sizeof(float) +
         (size_t)KNN_ANCHOR_TILE * sizeof(uint32_t);
}

// anchors of pass p and its first anchor row
static inline uint64_t knn_pass_first(const KnnPlan& p, uint32_t pass) { return (uint64_t)pass * p.grid * KNN_ANCHOR_TILE; }
static inline uint32_t knn_pass_anchors(const KnnPlan& p, uint64_t n_rows, uint32_t pass) {
  return (uint32_t)std::min<uint64_t>((uint64_t)p.grid * KNN_ANCHOR_TILE, n_rows - knn_pass_first(p, pass));
}

// n_rows: the handle's rows (anchor and candidate tiles walk row numbers, eligible or not); eligible: unmasked rows with a
// norm that is not NaN; shadow: the bf16 copy covers the rows; finite: no eligible row has an infinite norm; max_grid: the
// option "knn_max_grid", a cap on the workgroups of one pass (0: none).
// The LDS bytes do not depend on the row length: K is walked in chunks of KNN_BK elements.
static inline KnnPlan knn_plan(uint64_t n_rows, uint64_t eligible, int k, int cu_count, bool shadow, bool finite, uint64_t max_grid = 0) {
  KnnPlan p;
  if (!n_rows || !eligible) return p;
  p.path = (eligible < KNN_TILE_MIN_ROWS || !shadow || !finite) ? KNN_PATH_REPAIR : KNN_PATH_TILES;
  p.cap = knn_list_cap(k);
  p.lds = knn_lds_bytes();
  p.anchor_tiles = (uint32_t)((n_rows + KNN_ANCHOR_TILE - 1) / KNN_ANCHOR_TILE);
  p.cand_tiles = (uint32_t)((n_rows + KNN_CAND_TILE - 1) / KNN_CAND_TILE);
  const uint64_t per_wg = (uint64_t)KNN_ANCHOR_TILE * (p.cap * sizeof(uint64_t) + sizeof(uint32_t));
  const uint64_t fit = std::max<uint64_t>(1, (KNN_SCRATCH_BUDGET - 64) / per_wg);
  const uint64_t resident = (uint64_t)2 * (uint64_t)std::max(cu_count, 1);
  p.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)p.anchor_tiles, resident, fit, max_grid ? max_grid : fit}));
  p.passes = (p.anchor_tiles + p.grid - 1) / p.grid;
  const uint64_t pass_anchors = std::min<uint64_t>((uint64_t)p.grid * KNN_ANCHOR_TILE, n_rows);
  p.exact_grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((pass_anchors + 3) / 4, (uint64_t)8 * std::max(cu_count, 1)));
  p.list_bytes = (size_t)p.grid * KNN_ANCHOR_TILE * p.cap * sizeof(uint64_t);
  p.count_bytes = (size_t)p.grid * KNN_ANCHOR_TILE * sizeof(uint32_t) + 2 * sizeof(uint64_t);
  p.flag_bytes = (size_t)n_rows * sizeof(uint32_t);
  return p;
}

// ---- the margin --------------------------------------------------------------------------------
// S: the real value of the ranking form (a.c, or 2 a.c - |c|^2), T: the sweep's value, E: exact_score's (up to the anchor's own
// constant |a|^2 for L2).  Coefficients: gamma bounds an fp32 fma chain of at most pitch + 18 roundings, eps adds the two
// operands' rounding to bf16 (2^-8 relative each under to_bf16_sel: 2^-7 + 2^-16 < 1.05 * 2^-7), floor_abs covers operands in
// the denormal range (rounded to bf16 they keep no relative precision, or are flushed), under the gradual underflow of a chain.
// The same terms tau_margin_kernel charges the bf16 tiles with (kernels_aux.h) -- written out here as a function of its own:
// that kernel folds them into one doubled expression per query in another order, and its bits stay as they are.
struct KnnBound {
  float gamma, eps, floor_abs, under;
};
static inline KnnBound knn_bound(uint32_t pitch) {
  const float nu = (float)(pitch + 18) * 5.9604645e-08f;
  KnnBound b;
  b.gamma = 1.02f * nu / (1.0f - nu) * 1.0102f;
  b.eps = (b.gamma + 1.05f * 0.0078125f) * 1.0102f;
  b.floor_abs = 7.5e-37f * sqrtf((float)pitch);
  b.under = ldexpf((float)(pitch + 18), -149);
  return b;
}
// a norm from its computed square, rounded up
KNN_HD float knn_norm_up(float n2, KnnBound c) { return sqrtf(n2 + c.under) * (1.0f + c.gamma); }
// b_T >= |T - S| for an anchor and a candidate of squared norms an2, cn2 (as ensure_row_norms computes them)
KNN_HD float knn_tile_margin(bool l2, float an2, float cn2, KnnBound c) {
  const float na = knn_norm_up(an2, c), nc = knn_norm_up(cn2, c);
  const float dot = c.eps * na * nc + c.floor_abs * (na + nc) + c.under;
  return l2 ? 2.0f * dot + c.gamma * nc * nc : dot;
}
// b_E >= |E - S|: section 4.20's bound of exact_score's chain
KNN_HD float knn_exact_margin(bool l2, float an2, float cn2, KnnBound c) {
  const float na = knn_norm_up(an2, c), nc = knn_norm_up(cn2, c);
  return l2 ? c.gamma * (na + nc) * (na + nc) + 4.0f * c.under : c.gamma * na * nc + c.under;
}
// b = b_T + b_E with the anchor's norm and the largest eligible norm, widened; not finite: the anchor takes the repair route
KNN_HD float knn_margin(bool l2, float an2, float cmax2, KnnBound c) {
  return (knn_tile_margin(l2, an2, cmax2, c) + knn_exact_margin(l2, an2, cmax2, c)) * 1.01f;
}
