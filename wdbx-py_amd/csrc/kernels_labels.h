// kernels_labels.h -- the full pass of wdbx_index_search_distinct (exact top-k with at most one row per label): label_keys_kernel
// walks the label order (host_labels.h) span by span, scores every fetched row against a block of QB queries and writes the best
// key of each ITEM (a run of one label inside a span); label_rank_kernel takes the best key of each label over its consecutive
// items and ranks the labels.  Plain stores, one writer per key: no atomics, answers bit-identical from run to run.
// Part of the single translation unit wdbx_hip.hip (included there, in order); not a standalone header.

constexpr uint32_t LABEL_SPAN_DEV = 64;  // (= LABEL_SPAN, host_labels.h; checked where both are visible)

struct LabelKeysArgs {
  const f4* rows;              // [n_rows, pitch4] quads
  const f4* queries;           // [nq, pitch4] the round's queries
  const uint32_t* order;       // [n] row of each position of the label order
  const uint32_t* dense;       // [n] dense label index of each position
  const uint32_t* span_item0;  // [n_spans + 1] first item of each span
  const uint32_t* mask;        // optional row filter: bit r set = row r may be returned
  u64* keys;                   // [nq][key_stride], entry i = item i
  uint64_t key_stride;
  uint32_t n;                  // positions (= rows of the index)
  uint32_t n_spans;
  uint32_t pitch4;
  uint32_t nq;                 // queries of the round (the last query block may be short: its idle slots repeat the last query)
};

// Grid: x = workgroups along the spans (wave w of the grid takes spans w, w + W, ...; U rows' loads in flight per wave), y =
// query blocks.  A row's QB scores are exact_score_block's (kernels_rowblock.h): rescore_kernel's arithmetic bit for bit, wave-
// uniform.  A masked-out row, a NaN score (removed rows) give key 0.  The wave keeps the running maximum of make_key(score, row)
// per query; at every label boundary and at the span's end lane b stores query b's maximum as the item's key (0 = no row).
template <int METRIC, int QB, int NI>
__global__ __launch_bounds__(256) void label_keys_kernel(LabelKeysArgs a) {
  constexpr int U = row_block_u(NI), NR = row_block_nr(NI);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t j = (uint32_t)lane;
  const uint32_t q0 = blockIdx.y * QB;
  const f4* qp[QB];
  f4 q[QB][NR];
#pragma unroll
  for (int b = 0; b < QB; ++b) {
    qp[b] = a.queries + (size_t)min(q0 + (uint32_t)b, a.nq - 1) * a.pitch4;
#pragma unroll
    for (int t = 0; t < NR; ++t) {
      q[b][t] = f4{0.f, 0.f, 0.f, 0.f};
      if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) q[b][t] = qp[b][j + (uint32_t)t * 64];
    }
  }
  const bool writer = j < (uint32_t)QB && q0 + j < a.nq;
  u64* const my_keys = a.keys + (size_t)min(q0 + j, a.nq - 1) * a.key_stride;  // (lanes that are no writer never store)
  u64 best[QB];
  auto flush = [&](uint32_t item) {
    u64 v = 0;
#pragma unroll
    for (int b = 0; b < QB; ++b) {
      if (lane == b) v = best[b];
      best[b] = 0;
    }
    if (writer) my_keys[item] = v;
  };
  const uint32_t W = gridDim.x * 4;
  for (uint32_t span = blockIdx.x * 4 + wave; span < a.n_spans; span += W) {
    const uint32_t p0 = span * LABEL_SPAN_DEV, p1 = min(p0 + LABEL_SPAN_DEV, a.n);
    uint32_t item = a.span_item0[span];
    uint32_t cur_label = a.dense[p0];
#pragma unroll
    for (int b = 0; b < QB; ++b) best[b] = 0;
    for (uint32_t cur = p0; cur < p1; cur += U) {
      f4 c[U][NR];
      uint32_t row[U], lab[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t pos = min(cur + (uint32_t)u, p1 - 1);  // (past the span's end: its last position again, dropped below)
        row[u] = a.order[pos];
        lab[u] = a.dense[pos];
        const f4* cp = a.rows + (size_t)row[u] * a.pitch4;
#pragma unroll
        for (int t = 0; t < NR; ++t) {
          c[u][t] = f4{0.f, 0.f, 0.f, 0.f};
          if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) c[u][t] = ld16<true>(cp + j + (uint32_t)t * 64);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (cur + (uint32_t)u >= p1) break;  // (wave-uniform)
        float s[QB];
        exact_score_block<METRIC, QB, NI>(c[u], a.rows + (size_t)row[u] * a.pitch4, q, qp, a.pitch4, j, s);
        if (lab[u] != cur_label) {  // (wave-uniform) the label's run inside this span has ended
          flush(item);
          ++item;
          cur_label = lab[u];
        }
        const bool allowed = row_allowed(a.mask, row[u]);
#pragma unroll
        for (int b = 0; b < QB; ++b) best[b] = max(best[b], allowed ? row_key(s[b], row[u]) : 0ull);
      }
    }
    flush(item);
  }
}

typedef void (*label_keys_fn)(LabelKeysArgs);

// qb as distinct_plan (host_labels.h) chooses it: 1 or 8; null for any other
static label_keys_fn pick_label_keys(int metric, int qb, uint32_t pitch4) {
  return with_row_block_ni(pitch4, [&](auto ni) -> label_keys_fn {
    constexpr int NI = decltype(ni)::value;
    const bool l2 = metric == WDBX_METRIC_L2;
    if (qb == 1) return l2 ? label_keys_kernel<WDBX_METRIC_L2, 1, NI> : label_keys_kernel<WDBX_METRIC_COSINE, 1, NI>;
    if (qb == 8) return l2 ? label_keys_kernel<WDBX_METRIC_L2, 8, NI> : label_keys_kernel<WDBX_METRIC_COSINE, 8, NI>;
    return nullptr;
  });
}

struct LabelRankArgs {
  const u64* keys;              // [nq][key_stride] item keys of the round
  uint64_t key_stride;
  const uint32_t* label_item0;  // [n_labels + 1] first item of each label
  uint32_t n_labels;
  u64* out;                     // lists: [nq][k][P] as the fp32 scan's partial lists; keys: [nq][n_labels], entry l = label l
  int k;
};

// MODE 0: a sorted list of k keys per wave in LDS, 1: in registers (k <= 128), 2: no list, every label's key goes to
// out[query][label] (ranked by the radix-select chain).  Grid: x = workgroups along the labels (a lane per label, 64 labels per
// wave and trip), y = the round's queries.  A label's key is the maximum over its consecutive items (most labels have one).
// Lists: the workgroup's four wave lists are merged here as in subset_kernel, so out holds one partial list per workgroup and
// query, in the layout merge_kernel merges for the fp32 scan.  Labels are disjoint over the workgroups: every key is unique.
template <int MODE>
__global__ __launch_bounds__(256) void label_rank_kernel(LabelRankArgs a) {
  constexpr bool REG = MODE == 1;
  extern __shared__ u64 lds_lists[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t qi = blockIdx.y;
  const u64* kq = a.keys + (size_t)qi * a.key_stride;
  TopList<REG> top;
  u64 thr = 0;
  if constexpr (MODE != 2) top.init(lds_lists + (size_t)wave * a.k, a.k, lane);
  for (uint32_t l0 = (blockIdx.x * 4 + wave) * 64; l0 < a.n_labels; l0 += gridDim.x * 256) {
    const uint32_t l = l0 + (uint32_t)lane;
    u64 key = 0;
    if (l < a.n_labels) {
      const uint32_t i1 = a.label_item0[l + 1];
      for (uint32_t i = a.label_item0[l]; i < i1; ++i) key = max(key, kq[i]);
    }
    if constexpr (MODE == 2) {
      if (l < a.n_labels) a.out[(size_t)qi * a.n_labels + l] = key;
    } else {
      thr = top.offer(key, key > thr, thr, lane);
    }
  }
  if constexpr (MODE != 2) {
    if constexpr (REG) top.store(lds_lists + (size_t)wave * a.k, 1, lane);
    __syncthreads();
    if (wave == 0) {
      const u64* other = lds_lists + (size_t)lane * a.k;  // (lanes 1 .. 3: the other waves' lists)
      walk_lists<REG>([&](int ptr) { return other[ptr]; }, lane >= 1 && lane < 4, a.k, top, thr, lane);
      top.store(a.out + (size_t)qi * a.k * gridDim.x + blockIdx.x, gridDim.x, lane);
    }
  }
}

typedef void (*label_rank_fn)(LabelRankArgs);

static label_rank_fn pick_label_rank(int mode) {
  return mode == 0 ? label_rank_kernel<0> : mode == 1 ? label_rank_kernel<1> : label_rank_kernel<2>;
}
