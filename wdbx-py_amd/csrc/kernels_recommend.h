// kernels_recommend.h -- wdbx_index_search_recommend on the device: one pass over the WHOLE corpus per query, one wave per row,
// every fetched row scored against all of the query's examples (positives and negatives) and the scores folded in registers
// into one key.  The frame of kernels_rowblock.h with the corpus as row source and a fold between the scores and the key.
// Part of the single translation unit wdbx_hip.hip (included there, in order); not a standalone header.

constexpr int RECOMMEND_EXAMPLE_BLOCK = 8;  // examples scored per pass over a loaded row (then 4, then one by one)

struct RecommendArgs {
  const f4* rows;           // [n_rows, pitch4] quads
  const f4* examples;       // [examples of the call, pitch4] quads, back to back
  const uint32_t* table;    // [grid.y][3]: first positive, first negative (= end of the positives), end of the negatives
  const uint32_t* mask;     // optional row filter: bit r % 32 of word r / 32 set = row r may be returned
  const uint32_t* exclude;  // [n_exclude] strictly increasing row numbers that are never returned (validated on the host)
  u64* out;                 // lists: [grid.y][k][P] as the fp32 scan's partial lists; keys: [grid.y][key_stride], entry r = row r
  uint64_t key_stride;
  uint32_t n_exclude;
  uint32_t n_rows;
  uint32_t pitch4;
  int k;
  int side;                 // 1: favoured rows (p > n) emit make_key(p + 0.0f, row); 0: the others emit make_key((-n) + 0.0f, row)
};

// EB examples [e, e + EB) against one loaded row: exact_score_block's arithmetic (so every r is rescore_kernel's score bit for
// bit), then the running maximum; a NaN r is remembered, fmaxf would drop it
template <int METRIC, int EB, int NI>
__device__ __forceinline__ void recommend_fold_block(const f4 (&c)[NI > 0 ? NI : 1], const f4* cp, const f4* examples, uint32_t e,
                                                     uint32_t pitch4, uint32_t j, float& best, bool& nan) {
  constexpr int NR = row_block_nr(NI);
  const f4* qp[EB];
  f4 q[EB][NR];
#pragma unroll
  for (int b = 0; b < EB; ++b) {
    qp[b] = examples + (size_t)(e + (uint32_t)b) * pitch4;
#pragma unroll
    for (int t = 0; t < NR; ++t) {
      q[b][t] = f4{0.f, 0.f, 0.f, 0.f};
      if (NI > 0 && j + (uint32_t)t * 64 < pitch4) q[b][t] = qp[b][j + (uint32_t)t * 64];
    }
  }
  float s[EB];
  exact_score_block<METRIC, EB, NI>(c, cp, q, qp, pitch4, j, s);
#pragma unroll
  for (int b = 0; b < EB; ++b) {
    nan = nan || s[b] != s[b];
    best = fmaxf(best, s[b]);
  }
}

// max r over examples [e, end) (wave-uniform bounds): blocks of 8, one of 4, the rest one by one -- a maximum does not depend
// on the cut
template <int METRIC, int NI>
__device__ __forceinline__ float recommend_fold(const f4 (&c)[NI > 0 ? NI : 1], const f4* cp, const f4* examples, uint32_t e,
                                                uint32_t end, uint32_t pitch4, uint32_t j, bool& nan) {
  float best = -INFINITY;
  for (; e + RECOMMEND_EXAMPLE_BLOCK <= end; e += RECOMMEND_EXAMPLE_BLOCK)
    recommend_fold_block<METRIC, RECOMMEND_EXAMPLE_BLOCK, NI>(c, cp, examples, e, pitch4, j, best, nan);
  if (e + 4 <= end) {
    recommend_fold_block<METRIC, 4, NI>(c, cp, examples, e, pitch4, j, best, nan);
    e += 4;
  }
  for (; e < end; ++e) recommend_fold_block<METRIC, 1, NI>(c, cp, examples, e, pitch4, j, best, nan);
  return best;
}

// is row in the sorted exclusion list (scalar: the row number is wave-uniform)
__device__ __forceinline__ bool recommend_excluded(const uint32_t* list, uint32_t n, uint32_t row) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (list[mid] < row)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n && list[lo] == row;
}

// MODE as subset_kernel: 0 a sorted list of k keys per wave in LDS, 1 in registers (k <= 128), 2 no list, every row's key goes
// to out[y][row] for the radix-select chain (an ineligible row's key is 0).
// Grid: x = workgroups along the corpus (wave w of the grid takes rows w, w + W, ...; U rows' loads in flight per wave), y = the
// query (its table entry).  NI > 0: the row's quads stay in registers for all example blocks; NI = 0: any pitch, the row is read
// again per block through the caches.  The examples are read through the caches: every wave of the grid row reads the same few.
// The mask bit and the exclusion list are tested on the wave-uniform row number; an ineligible row is not scored.
template <int METRIC, int NI, int MODE>
__global__ __launch_bounds__(256) void recommend_kernel(RecommendArgs a) {
  constexpr bool REG = MODE == 1;
  constexpr int U = NI == 0 ? 1 : 2;  // (this kernel's own, not row_block_u: the figures of DESIGN.md 4.15 were measured with it)
  constexpr int NR = row_block_nr(NI);
  extern __shared__ u64 lds_lists[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t j = (uint32_t)lane;
  TopList<REG> top;
  u64 thr = 0;
  if constexpr (MODE != 2) top.init(lds_lists + (size_t)wave * a.k, a.k, lane);
  const uint32_t* tab = a.table + (size_t)blockIdx.y * 3;
  const uint32_t e0 = tab[0], e1 = tab[1], e2 = tab[2];
  const uint32_t W = gridDim.x * 4, wg = blockIdx.x * 4 + (uint32_t)wave;
  for (uint32_t cur = wg; cur < a.n_rows; cur += U * W) {
    f4 c[U][NR];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t row = min(cur + (uint32_t)u * W, a.n_rows - 1);  // (past the end: the last row again, dropped below)
      const f4* cp = a.rows + (size_t)row * a.pitch4;
#pragma unroll
      for (int t = 0; t < NR; ++t) {
        c[u][t] = f4{0.f, 0.f, 0.f, 0.f};
        if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) c[u][t] = ld16<true>(cp + j + (uint32_t)t * 64);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t idx = cur + (uint32_t)u * W;
      const bool live = idx < a.n_rows;  // (wave-uniform, as everything about the row number)
      const uint32_t row = min(idx, a.n_rows - 1);
      bool ok = live;
      if (ok && a.mask) ok = row_allowed(a.mask, row);
      if (ok && a.n_exclude) ok = !recommend_excluded(a.exclude, a.n_exclude, row);
      u64 mine = 0;
      if (ok) {
        const f4* cp = a.rows + (size_t)row * a.pitch4;
        bool nan = false;
        const float p = recommend_fold<METRIC, NI>(c[u], cp, a.examples, e0, e1, a.pitch4, j, nan);
        const float n = recommend_fold<METRIC, NI>(c[u], cp, a.examples, e1, e2, a.pitch4, j, nan);
        const bool favoured = p > n;
        if (!nan && favoured == (a.side != 0)) mine = make_key((favoured ? p : -n) + 0.0f, row);  // a NaN score kills the row
      }
      if constexpr (MODE == 2) {
        if (lane == 0 && live) a.out[(size_t)blockIdx.y * a.key_stride + idx] = mine;
      } else {
        const u64 key = readlane64(mine, 0);
        if (key > thr) thr = top.insert(key, lane);
      }
    }
  }
  if constexpr (MODE != 2) {
    if constexpr (REG) top.store(lds_lists + (size_t)wave * a.k, 1, lane);
    __syncthreads();
    if (wave == 0) {
      const u64* other = lds_lists + (size_t)lane * a.k;  // (lanes 1 .. 3: the other waves' lists)
      walk_lists<REG>([&](int ptr) { return other[ptr]; }, lane >= 1 && lane < 4, a.k, top, thr, lane);
      top.store(a.out + (size_t)blockIdx.y * a.k * gridDim.x + blockIdx.x, gridDim.x, lane);
    }
  }
}

typedef void (*recommend_fn)(RecommendArgs);

template <int METRIC>
static recommend_fn pick_recommend_metric(int mode, uint32_t pitch4) {
  return with_row_block_ni(pitch4, [&](auto ni) -> recommend_fn {
    constexpr int NI = decltype(ni)::value;
    if (mode == 0) return recommend_kernel<METRIC, NI, 0>;
    if (mode == 1) return recommend_kernel<METRIC, NI, 1>;
    if (mode == 2) return recommend_kernel<METRIC, NI, 2>;
    return nullptr;
  });
}

static recommend_fn pick_recommend(int metric, int mode, uint32_t pitch4) {
  return metric == WDBX_METRIC_L2 ? pick_recommend_metric<WDBX_METRIC_L2>(mode, pitch4)
                                  : pick_recommend_metric<WDBX_METRIC_COSINE>(mode, pitch4);
}
