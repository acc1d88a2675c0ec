// kernels_discover.h -- wdbx_index_search_discover on the device.  discover_kernel is recommend_kernel's
// frame (one pass over the WHOLE corpus per query, one wave per row) with a fold PER PAIR between the scores and the sink: a
// query's staged vectors are [target?, p0, n0, p1, n1, ...], every pair (positive, negative) adds a win or a loss term.
// Context mode (no target) ranks by the loss alone, so its sinks are recommend's three ranking modes.  Target mode ranks by
// (wins, target score), which the 64-bit key has no room for: the pass writes a RECORD per row (the target's key and the wins
// byte) and the per-zone row counts, and discover_zone_kernel ranks the rows of one zone (one wins value) from the records.
// Part of the single translation unit wdbx_hip.hip (included there, in order); not a standalone header.

constexpr int DISCOVER_ZONES = 33;  // wins values 0 .. WDBX_MAX_CONTEXT_PAIRS

struct DiscoverArgs {
  const f4* rows;           // [n_rows, pitch4] quads
  const f4* vectors;        // the call's staged vectors, [.., pitch4] quads: per query [target?, p0, n0, p1, n1, ...]
  const uint32_t* table;    // [grid.y][2]: the query's first staged vector, its pairs
  const uint32_t* mask;     // optional row filter: bit r % 32 of word r / 32 set = row r may be returned
  const uint32_t* exclude;  // [n_exclude] strictly increasing row numbers that are never returned (validated on the host)
  u64* out;                 // modes 0, 1: [grid.y][k][P] partial lists; mode 2: [grid.y][key_stride] keys; mode 3: the records' keys
  uint8_t* wins;            // mode 3: [grid.y][key_stride], entry r = row r's wins (0 where its key is 0)
  uint32_t* counts;         // mode 3: [grid.y][DISCOVER_ZONES], ADDED to: rows with a key per wins value
  uint64_t key_stride;
  uint32_t n_exclude;
  uint32_t n_rows;
  uint32_t pitch4;
  int k;
};

// EB staged vectors [e, e + EB) against one loaded row: exact_score_block's arithmetic, so every s is rescore_kernel's score
// bit for bit
template <int METRIC, int EB, int NI>
__device__ __forceinline__ void discover_score_block(const f4 (&c)[NI > 0 ? NI : 1], const f4* cp, const f4* vectors, uint32_t e,
                                                     uint32_t pitch4, uint32_t j, float (&s)[EB]) {
  constexpr int NR = row_block_nr(NI);
  const f4* qp[EB];
  f4 q[EB][NR];
#pragma unroll
  for (int b = 0; b < EB; ++b) {
    qp[b] = vectors + (size_t)(e + (uint32_t)b) * pitch4;
#pragma unroll
    for (int t = 0; t < NR; ++t) {
      q[b][t] = f4{0.f, 0.f, 0.f, 0.f};
      if (NI > 0 && j + (uint32_t)t * 64 < pitch4) q[b][t] = qp[b][j + (uint32_t)t * 64];
    }
  }
  exact_score_block<METRIC, EB, NI>(c, cp, q, qp, pitch4, j, s);
}

// EB / 2 pairs starting at staged vector e, in pair order: a win where r(p) > r(n) (a tie is none), the loss term
// fminf(r(p) - r(n), 0); a NaN difference (a NaN score, inf - inf) is remembered, the comparisons would drop it
template <int METRIC, int EB, int NI>
__device__ __forceinline__ void discover_pair_block(const f4 (&c)[NI > 0 ? NI : 1], const f4* cp, const f4* vectors, uint32_t e,
                                                    uint32_t pitch4, uint32_t j, uint32_t& wins, float& loss, bool& nan) {
  float s[EB];
  discover_score_block<METRIC, EB, NI>(c, cp, vectors, e, pitch4, j, s);
#pragma unroll
  for (int b = 0; b < EB; b += 2) {
    const float d = s[b] - s[b + 1];
    nan = nan || d != d;
    wins += s[b] > s[b + 1] ? 1u : 0u;
    loss += fminf(d, 0.0f);
  }
}

// the pairs at staged vectors [e, e + 2 * pairs) (wave-uniform bounds): blocks of 8 vectors, one of 4, one of 2 -- a pair never
// straddles a block, and the terms are added in pair order whatever the cut
template <int METRIC, int NI>
__device__ __forceinline__ void discover_fold(const f4 (&c)[NI > 0 ? NI : 1], const f4* cp, const f4* vectors, uint32_t e,
                                              uint32_t pairs, uint32_t pitch4, uint32_t j, uint32_t& wins, float& loss, bool& nan) {
  const uint32_t end = e + 2 * pairs;
  for (; e + 8 <= end; e += 8) discover_pair_block<METRIC, 8, NI>(c, cp, vectors, e, pitch4, j, wins, loss, nan);
  if (e + 4 <= end) {
    discover_pair_block<METRIC, 4, NI>(c, cp, vectors, e, pitch4, j, wins, loss, nan);
    e += 4;
  }
  if (e + 2 <= end) discover_pair_block<METRIC, 2, NI>(c, cp, vectors, e, pitch4, j, wins, loss, nan);
}

// MODE 0 / 1 / 2: context mode, ranked as recommend_kernel ranks (LDS lists, register lists for k <= 128, a key per row for the
// radix-select chain) by make_key(loss + 0.0f, row).  MODE 3: target mode, the staged vectors start with the target; every live
// row gets its record -- out[y][row] = make_key(t, row) with t the target's score, wins[y][row] -- or 0 / 0 when the row is
// ineligible or a score is NaN, and the workgroup's rows per wins value go through an LDS histogram into counts[y] (integer
// adds: the sums do not depend on the order).
// Grid, NI, the loads, the mask and the exclusion list: as recommend_kernel.
template <int METRIC, int NI, int MODE>
__global__ __launch_bounds__(256) void discover_kernel(DiscoverArgs a) {
  constexpr bool REG = MODE == 1;
  constexpr bool LISTS = MODE == 0 || MODE == 1;
  constexpr bool TARGET = MODE == 3;
  constexpr int U = NI == 0 ? 1 : 2;
  constexpr int NR = row_block_nr(NI);
  extern __shared__ u64 lds_lists[];
  __shared__ uint32_t hist[TARGET ? DISCOVER_ZONES : 1];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t j = (uint32_t)lane;
  TopList<REG> top;
  u64 thr = 0;
  if constexpr (LISTS) top.init(lds_lists + (size_t)wave * a.k, a.k, lane);
  if constexpr (TARGET) {
    if (threadIdx.x < DISCOVER_ZONES) hist[threadIdx.x] = 0;
    __syncthreads();
  }
  const uint32_t* tab = a.table + (size_t)blockIdx.y * 2;
  const uint32_t v0 = tab[0], pairs = tab[1];
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
      uint32_t wins = 0;
      if (ok) {
        const f4* cp = a.rows + (size_t)row * a.pitch4;
        bool nan = false;
        float loss = 0.0f;
        float t[1] = {0.0f};
        if constexpr (TARGET) {
          discover_score_block<METRIC, 1, NI>(c[u], cp, a.vectors, v0, a.pitch4, j, t);
          nan = t[0] != t[0];
        }
        discover_fold<METRIC, NI>(c[u], cp, a.vectors, v0 + (TARGET ? 1u : 0u), pairs, a.pitch4, j, wins, loss, nan);
        if (!nan) mine = make_key((TARGET ? t[0] : loss) + 0.0f, row);
      }
      if constexpr (TARGET) {
        if (lane == 0 && live) {
          const size_t o = (size_t)blockIdx.y * a.key_stride + idx;
          a.out[o] = mine;
          a.wins[o] = mine ? (uint8_t)wins : (uint8_t)0;
          if (mine) atomicAdd(&hist[wins], 1u);
        }
      } else if constexpr (MODE == 2) {
        if (lane == 0 && live) a.out[(size_t)blockIdx.y * a.key_stride + idx] = mine;
      } else {
        const u64 key = readlane64(mine, 0);
        if (key > thr) thr = top.insert(key, lane);
      }
    }
  }
  if constexpr (TARGET) {
    __syncthreads();
    if (threadIdx.x < DISCOVER_ZONES && hist[threadIdx.x])
      atomicAdd(a.counts + (size_t)blockIdx.y * DISCOVER_ZONES + threadIdx.x, hist[threadIdx.x]);
  }
  if constexpr (LISTS) {
    if constexpr (REG) top.store(lds_lists + (size_t)wave * a.k, 1, lane);
    __syncthreads();
    if (wave == 0) {
      const u64* other = lds_lists + (size_t)lane * a.k;  // (lanes 1 .. 3: the other waves' lists)
      walk_lists<REG>([&](int ptr) { return other[ptr]; }, lane >= 1 && lane < 4, a.k, top, thr, lane);
      top.store(a.out + (size_t)blockIdx.y * a.k * gridDim.x + blockIdx.x, gridDim.x, lane);
    }
  }
}

struct DiscoverZoneArgs {
  const u64* rec_key;       // [query slots][rec_stride] the records' keys
  const uint8_t* rec_wins;  // [query slots][rec_stride] the records' wins
  const uint32_t* table;    // [grid.y][2]: query slot, zone (a wins value)
  u64* out;                 // modes 0, 1: [grid.y][k][P] partial lists; mode 2: [grid.y][rec_stride] keys
  uint64_t rec_stride;
  uint32_t n_rows;
  int k;
};

// The second stage of target mode: the rows of ONE zone of one query, ranked by their records' keys.  A lane per row, 9 bytes
// read per row; wave w of the grid takes the 64-row chunks w, w + W, ...  MODE 0 / 1: a sorted list of k keys per wave (LDS /
// registers), merged in the workgroup as in discover_kernel; MODE 2: out[y][row] = the key, or 0 outside the zone, for the
// radix-select chain.  A key of 0 (an ineligible or NaN row) is in no zone.
template <int MODE>
__global__ __launch_bounds__(256) void discover_zone_kernel(DiscoverZoneArgs a) {
  constexpr bool REG = MODE == 1;
  extern __shared__ u64 lds_lists[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t* tab = a.table + (size_t)blockIdx.y * 2;
  const uint32_t slot = tab[0], zone = tab[1];
  const u64* keys = a.rec_key + (size_t)slot * a.rec_stride;
  const uint8_t* wins = a.rec_wins + (size_t)slot * a.rec_stride;
  const uint32_t W = gridDim.x * 4, wg = blockIdx.x * 4 + (uint32_t)wave;
  const uint32_t chunks = (a.n_rows + 63) / 64;
  TopList<REG> top;
  u64 thr = 0;
  if constexpr (MODE != 2) top.init(lds_lists + (size_t)wave * a.k, a.k, lane);
  for (uint32_t ch = wg; ch < chunks; ch += W) {
    const uint32_t row = ch * 64 + (uint32_t)lane;
    u64 key = 0;
    if (row < a.n_rows && (uint32_t)wins[row] == zone) key = keys[row];
    if constexpr (MODE == 2) {
      if (row < a.n_rows) a.out[(size_t)blockIdx.y * a.rec_stride + row] = key;
    } else {
      thr = top.offer(key, key > thr, thr, lane);
    }
  }
  if constexpr (MODE != 2) {
    if constexpr (REG) top.store(lds_lists + (size_t)wave * a.k, 1, lane);
    __syncthreads();
    if (wave == 0) {
      const u64* other = lds_lists + (size_t)lane * a.k;
      walk_lists<REG>([&](int ptr) { return other[ptr]; }, lane >= 1 && lane < 4, a.k, top, thr, lane);
      top.store(a.out + (size_t)blockIdx.y * a.k * gridDim.x + blockIdx.x, gridDim.x, lane);
    }
  }
}

typedef void (*discover_fn)(DiscoverArgs);
typedef void (*discover_zone_fn)(DiscoverZoneArgs);

template <int METRIC>
static discover_fn pick_discover_metric(int mode, uint32_t pitch4) {
  return with_row_block_ni(pitch4, [&](auto ni) -> discover_fn {
    constexpr int NI = decltype(ni)::value;
    if (mode == 0) return discover_kernel<METRIC, NI, 0>;
    if (mode == 1) return discover_kernel<METRIC, NI, 1>;
    if (mode == 2) return discover_kernel<METRIC, NI, 2>;
    if (mode == 3) return discover_kernel<METRIC, NI, 3>;
    return nullptr;
  });
}

// mode: 0 .. 2 context mode's ranking modes, 3 target mode's record pass
static discover_fn pick_discover(int metric, int mode, uint32_t pitch4) {
  return metric == WDBX_METRIC_L2 ? pick_discover_metric<WDBX_METRIC_L2>(mode, pitch4)
                                  : pick_discover_metric<WDBX_METRIC_COSINE>(mode, pitch4);
}

static discover_zone_fn pick_discover_zone(int mode) {
  if (mode == 0) return discover_zone_kernel<0>;
  if (mode == 1) return discover_zone_kernel<1>;
  if (mode == 2) return discover_zone_kernel<2>;
  return nullptr;
}
