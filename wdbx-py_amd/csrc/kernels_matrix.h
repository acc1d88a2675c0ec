// kernels_matrix.h -- distance matrix among LISTED rows (wdbx_index_search_matrix): subset_kernel's sibling whose queries are
// listed rows themselves.  A workgroup's QB anchors are read where they lie -- from the corpus through the list, no staged
// copy -- and every listed row is scored against them (the frame of kernels_rowblock.h); the candidate at the anchor's own
// list position is left out by position, so another row holding an equal vector is a neighbour like any other.
// Part of the single translation unit wdbx_hip.hip (included there, behind kernels_subset.h); not a standalone header.

struct MatrixArgs {
  const f4* rows;       // [n_rows, pitch4] quads
  const uint32_t* ids;  // [n_ids] strictly increasing row numbers (validated on the host): candidates AND anchors
  u64* out;             // lists: [na][k][P] as the fp32 scan's partial lists; keys: [na][key_stride], entry i = listed row i
  uint64_t key_stride;
  uint32_t n_ids;
  uint32_t pitch4;
  uint32_t first;       // list position of the round's first anchor
  uint32_t na;          // anchors of the round, first + na <= n_ids (the last block may be short: its idle slots repeat the last anchor)
  int k;
};

// MODE as subset_kernel: 0 a sorted list of k keys per wave and anchor in LDS (QB = 1), 1 in registers (k <= 128), 2 no list,
// the key of every (anchor, listed row) goes to out[anchor][i]; the anchor's own entry is 0 there, the key a NaN score gets.
// Grid: x = workgroups along the list (wave w of the grid takes listed rows w, w + W, ...; U rows' loads in flight per
// wave), y = blocks of QB anchors.  The list position of a candidate is wave-uniform and so is the anchor's, so "is this the
// anchor itself" is a uniform branch; with lists the zero key is simply never above the threshold.  No atomics: every output
// word has one writer.
template <int METRIC, int QB, int NI, int MODE>
__global__ __launch_bounds__(256) void matrix_kernel(MatrixArgs a) {
  constexpr bool REG = MODE == 1;
  constexpr int U = row_block_u(NI), NR = row_block_nr(NI);
  extern __shared__ u64 lds_lists[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t j = (uint32_t)lane;
  const uint32_t q0 = blockIdx.y * QB;
  TopList<REG> top[QB];
  u64 thr[QB];
  uint32_t self[QB];  // the anchors' list positions
  const f4* qp[QB];
  f4 q[QB][NR];
#pragma unroll
  for (int b = 0; b < QB; ++b) {
    if constexpr (MODE != 2) top[b].init(lds_lists + (size_t)(wave * QB + b) * a.k, a.k, lane);
    thr[b] = 0;
    self[b] = a.first + min(q0 + (uint32_t)b, a.na - 1);
    qp[b] = a.rows + (size_t)a.ids[self[b]] * a.pitch4;
#pragma unroll
    for (int t = 0; t < NR; ++t) {
      q[b][t] = f4{0.f, 0.f, 0.f, 0.f};
      if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) q[b][t] = qp[b][j + (uint32_t)t * 64];
    }
  }
  const uint32_t W = gridDim.x * 4, wg = blockIdx.x * 4 + wave;
  for (uint32_t cur = wg; cur < a.n_ids; cur += U * W) {
    f4 c[U][NR];
    uint32_t row[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t idx = cur + (uint32_t)u * W;
      row[u] = a.ids[min(idx, a.n_ids - 1)];  // (past the end: the last listed row again, dropped below)
      const f4* cp = a.rows + (size_t)row[u] * a.pitch4;
#pragma unroll
      for (int t = 0; t < NR; ++t) {
        c[u][t] = f4{0.f, 0.f, 0.f, 0.f};
        if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) c[u][t] = ld16<true>(cp + j + (uint32_t)t * 64);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t idx = cur + (uint32_t)u * W;
      const bool live = idx < a.n_ids;  // (wave-uniform)
      float s[QB];
      exact_score_block<METRIC, QB, NI>(c[u], a.rows + (size_t)row[u] * a.pitch4, q, qp, a.pitch4, j, s);
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        const u64 mine = live && idx != self[b] ? row_key(s[b], row[u]) : 0ull;
        if constexpr (MODE == 2) {
          if (lane == 0 && live && q0 + (uint32_t)b < a.na) a.out[(size_t)(q0 + b) * a.key_stride + idx] = mine;
        } else {
          const u64 key = readlane64(mine, 0);
          if (key > thr[b]) thr[b] = top[b].insert(key, lane);
        }
      }
    }
  }
  if constexpr (MODE != 2) {
    if constexpr (REG) {
#pragma unroll
      for (int b = 0; b < QB; ++b) top[b].store(lds_lists + (size_t)(wave * QB + b) * a.k, 1, lane);
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        const u64* other = lds_lists + (size_t)(lane * QB + b) * a.k;  // (lanes 1 .. 3: the other waves' lists of anchor b)
        walk_lists<REG>([&](int ptr) { return other[ptr]; }, lane >= 1 && lane < 4, a.k, top[b], thr[b], lane);
        if (q0 + (uint32_t)b < a.na) top[b].store(a.out + (size_t)(q0 + b) * a.k * gridDim.x + blockIdx.x, gridDim.x, lane);
      }
    }
  }
}

typedef void (*matrix_fn)(MatrixArgs);

// mode / qb as subset_query_block (host_subset.h) pairs them for matrix_plan (host_matrix.h): lists in LDS only with the
// block of one, register lists with 1, 4 or 8, keys with 1 or 8; null for any other pair
template <int METRIC>
static matrix_fn pick_matrix_metric(int mode, int qb, uint32_t pitch4) {
  return with_row_block_ni(pitch4, [&](auto ni) -> matrix_fn {
    constexpr int NI = decltype(ni)::value;
    if (mode == 0 && qb == 1) return matrix_kernel<METRIC, 1, NI, 0>;
    if (mode == 1 && qb == 1) return matrix_kernel<METRIC, 1, NI, 1>;
    if (mode == 1 && qb == 4) return matrix_kernel<METRIC, 4, NI, 1>;
    if (mode == 1 && qb == 8) return matrix_kernel<METRIC, 8, NI, 1>;
    if (mode == 2 && qb == 1) return matrix_kernel<METRIC, 1, NI, 2>;
    if (mode == 2 && qb == 8) return matrix_kernel<METRIC, 8, NI, 2>;
    return nullptr;
  });
}

static matrix_fn pick_matrix(int metric, int mode, int qb, uint32_t pitch4) {
  return metric == WDBX_METRIC_L2 ? pick_matrix_metric<WDBX_METRIC_L2>(mode, qb, pitch4)
                                  : pick_matrix_metric<WDBX_METRIC_COSINE>(mode, qb, pitch4);
}
