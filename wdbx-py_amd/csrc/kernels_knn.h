// kernels_knn.h -- the k-nearest-neighbour graph of the stored rows (wdbx_index_knn_graph): MANY anchors against MANY candidates,
// both the corpus itself, a top-k kept per anchor.
//   knn_tile_kernel    the sweep on the bf16 matrix cores over the bf16 shadow copy: candidates are the M operand, anchors the
//                      N operand, so an anchor is one lane's COLUMN of the 32x32 accumulator and its running threshold lives
//                      in that lane's registers; what beats the threshold less the margin goes to the anchor's bounded list,
//                      and a list about to fill up is compacted around the k-th largest of its own entries
//   knn_exact_kernel   exact_score's arithmetic over every anchor's surviving list: the entries become row keys in place, which
//                      the ranking tail ranks (enqueue_rank_tail) -- the returned bits
// Plan, capacities and the margin: host_knn.h.  The inequality behind the margin: DESIGN.md section 4.22.
// Part of the single translation unit wdbx_hip.hip (included there, behind kernels_matrix.h); not a standalone header.

struct KnnArgs {
  const char* rows16;         // the bf16 shadow copy: [n_rows + slack, pitch16] elements
  const float* cn;            // squared fp32 norm of every stored row (NaN: removed, or a NaN element)
  const uint32_t* mask;       // optional row filter
  const uint32_t* cmax_bits;  // the largest eligible squared norm, float bits
  u64* lists;                 // [gridDim.x * KNN_ANCHOR_TILE][cap] keys (approximate score, row), in no order
  uint32_t* counts;           // [gridDim.x * KNN_ANCHOR_TILE] entries left in each list (0: no result here, or flagged)
  uint32_t* flags;            // [n_rows] 1: the anchor is finished by the repair route
  unsigned long long* appends;  // the call's appended entries (a statistic)
  uint32_t n_rows, pitch16, cap, tile0, cand_tiles;
  int k;
  KnnBound bound;
};

// The k-th largest approximate score of one anchor's list and the list compacted around it, by one whole wave.  The entries are
// read into registers first (R per lane), the threshold is found by the bitwise search over their ordered score halves (the
// largest t with at least k entries >= t: exactly the k-th largest), and the entries with score >= threshold - twob are written
// back to the front.  Every compare is >=, so equal values are kept together, and what is kept does not depend on the order
// the entries were appended in.  Fewer than k entries: nothing is dropped and the threshold stays where it was.
// Returns the threshold; *fill (LDS) gets the new length.
template <int R>
__device__ __forceinline__ float knn_compact(u64* list, uint32_t n, int k, float twob, float theta, uint32_t* fill, int lane) {
  if (n < (uint32_t)k) return theta;  // (wave-uniform)
  u64 key[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const uint32_t e = (uint32_t)lane + 64u * i;
    key[i] = e < n ? list[e] : 0ull;  // (0: no entry -- a real entry's row half is never all zeros below 2^32 - 256 rows)
  }
  uint32_t t = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = t | (1u << bit);
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) cnt += (uint32_t)__popcll(__ballot(key[i] != 0ull && (uint32_t)(key[i] >> 32) >= cand));
    if (cnt >= (uint32_t)k) t = cand;
  }
  const float th = ord2f(t);
  const float lo = th - twob;
  uint32_t base = 0;
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const bool keep = key[i] != 0ull && key_score(key[i]) >= lo;
    const u64 bal = __ballot(keep);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    if (keep) list[base + rank] = key[i];  // (base + rank <= the entry's own position: never past the list)
    base += (uint32_t)__popcll(bal);
  }
  if (lane == 0) *fill = base;
  return th;
}

// Workgroup = 4 waves, anchor tile = 128 stored rows: wave w owns anchors 32 w .. 32 w + 31 of the tile as the 32 columns of 4
// accumulators (a candidate tile of 128 rows).  Both operands are staged K-chunk by K-chunk (64 bf16, rows of 144 bytes:
// gemm_bf16w8_kernel's conflict-free padding) through two LDS buffers; the loader's cursor (candidate tile, chunk) runs one
// chunk ahead of the compute cursor across candidate tiles, so a tile's first chunk is in LDS when the previous tile's fold
// ends.  The anchors' chunks are re-read per candidate tile from L2; the candidates' norms (NaN for a row that may not be
// returned: masked, removed, a NaN element, past the end) travel through LDS with their tile's first chunk.
// A launch sweeps gridDim.x anchor tiles, one per workgroup, all starting at candidate row 0 and walking the same way: the
// candidate stream is shared through L2 / MALL.  An anchor's list, its fill counter (LDS) and its threshold are touched by its
// own wave only -- lanes l and l ^ 32 hold the same anchor against different candidates -- so no workgroup barrier orders them.
// C layout: column (anchor) = lane & 31, row (candidate) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
template <int METRIC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void knn_tile_kernel(KnnArgs a) {
  constexpr int AT = KNN_ANCHOR_TILE, CT = KNN_CAND_TILE, LDB = KNN_LDB, MT = CT / 32, S = KNN_BK / 16;
  constexpr int PPR = KNN_BK / 8;   // 16-byte pieces per row per chunk
  constexpr int RPP = 256 / PPR;    // rows staged per pass of the 256 threads
  constexpr int NA = AT / RPP, NB = CT / RPP;
  constexpr int R = knn_list_cap(KNN_MAX_K) / 64;  // registers of keys per lane that hold the longest list
  static_assert(R * 64 >= (int)knn_list_cap(KNN_MAX_K), "knn_compact reads every entry of the longest list");
  extern __shared__ float lds_f[];
  char* const As = (char*)lds_f;             // [2][AT][LDB] anchors
  char* const Cs = As + 2 * AT * LDB;        // [2][CT][LDB] candidates
  float* const Ns = (float*)(Cs + 2 * CT * LDB);  // [2][CT] the norms of the tile being computed / being staged
  uint32_t* const fill = (uint32_t*)(Ns + 2 * CT);  // [AT] entries in each anchor's list
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const uint32_t kchunks = a.pitch16 / KNN_BK;
  const uint32_t srow = tid / PPR, spiece = tid % PPR;
  const uint32_t last_row = a.n_rows - 1;
  const size_t row_bytes = (size_t)a.pitch16 * 2;
  const uint32_t a0 = (a.tile0 + blockIdx.x) * AT;
  if (a0 >= a.n_rows) return;

  // loader: one chunk of (the anchor tile, candidate tile ld_ct) into registers, later into the other LDS buffer
  uint32_t ld_ct = 0, ld_kc = 0;
  f4 sa[NA], sc[NB];
  float sn = 0.f;
  bool st_first = false, ld_wrapped = false;
  uint32_t st_par = 0;
  auto gload = [&]() __attribute__((always_inline)) {
    const size_t o = (size_t)ld_kc * (KNN_BK * 2) + spiece * 16;
#pragma unroll
    for (int i = 0; i < NA; ++i)  // rows past the end are clamped to the last row (their columns are dead anchors)
      sa[i] = *(const f4*)(a.rows16 + (size_t)min(a0 + srow + RPP * i, last_row) * row_bytes + o);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      sc[i] = *(const f4*)(a.rows16 + (size_t)min(ld_ct * CT + srow + RPP * i, last_row) * row_bytes + o);
    st_first = ld_kc == 0 && !ld_wrapped;  // (the re-read last tile brings no norms: its own are being folded)
    st_par = ld_ct & 1;
    if (st_first && tid < CT) {
      const uint32_t row = ld_ct * CT + tid;
      sn = (row < a.n_rows && row_allowed(a.mask, row)) ? a.cn[row] : __uint_as_float(0x7FC00000u);
    }
    if (++ld_kc == kchunks) {
      ld_kc = 0;
      if (ld_ct + 1 < a.cand_tiles) ++ld_ct;  // past the last tile the loader re-reads it (valid memory, never consumed)
      else ld_wrapped = true;
    }
  };
  auto lstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NA; ++i) *(f4*)(As + (buf * AT + srow + RPP * i) * LDB + spiece * 16) = sa[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) *(f4*)(Cs + (buf * CT + srow + RPP * i) * LDB + spiece * 16) = sc[i];
    if (st_first && tid < CT) Ns[st_par * CT + tid] = sn;
  };

  // this lane's anchor: its row, whether it has a line at all, its margin and its threshold
  const uint32_t al = (uint32_t)wave * 32 + l31, arow = a0 + al;
  const float an2 = arow < a.n_rows ? a.cn[arow] : __uint_as_float(0x7FC00000u);
  bool live = arow < a.n_rows && row_allowed(a.mask, arow) && an2 == an2;
  const float twob = 2.0f * knn_margin(METRIC == WDBX_METRIC_L2, an2, __uint_as_float(*a.cmax_bits), a.bound);
  bool flagged = live && !(twob < INFINITY);  // (an infinite norm of its own, or a bound that overflowed)
  float theta = -INFINITY;
  u64* const my_list = a.lists + ((size_t)blockIdx.x * AT + al) * a.cap;
  if (lh == 0) fill[al] = 0;
  uint32_t appended = 0;

  gload();
  lstore(0);
  __syncthreads();
  uint32_t it = 0;  // running chunk counter (LDS buffer = it & 1)
  for (uint32_t ct = 0; ct < a.cand_tiles; ++ct) {
    f16v acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    for (uint32_t kc = 0; kc < kchunks; ++kc, ++it) {
      const int buf = it & 1;
      gload();  // the next chunk's global loads, in flight under this chunk's matrix ops
#pragma unroll 2
      for (int s = 0; s < S; ++s) {
        const bh8 af = *(const bh8*)(As + (buf * AT + wave * 32 + l31) * LDB + s * 32 + lh * 16);
        bh8 cf[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) cf[mt] = *(const bh8*)(Cs + (buf * CT + mt * 32 + l31) * LDB + s * 32 + lh * 16);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cf[mt], af, acc[mt], 0, 0, 0);
      }
      if (kc + 1 == kchunks) {
        // the tile's fold, BEFORE this iteration's LDS stores and barrier: the norms it reads were stored before the previous
        // barrier, and the stores below write the NEXT tile's norms to the other half of Ns (none after the last tile), which
        // was last read by the previous tile's fold, a barrier ago
        // (this lane's candidates: a base that carries its half-wave's offset 4 lh, then compile-time steps)
        const float* ns = Ns + (ct & 1) * CT + 4 * lh;
        const uint32_t crow0 = ct * CT + 4u * (uint32_t)lh;
        const bool open = live && !flagged;
        const float lo = open ? theta - twob : INFINITY;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ml = mt * 32 + (r & 3) + 8 * (r >> 2);
            const float cn2 = ns[ml];
            float v = acc[mt][r];
            if constexpr (METRIC == WDBX_METRIC_L2) v = fmaf(2.0f, v, -cn2);  // 2 a.c - |c|^2: |a|^2 is the anchor's own
            else v = cn2 == cn2 ? v : cn2;                                    // (a NaN norm: never a candidate)
            if (v >= lo && open) {  // (a NaN is never appended)
              uint32_t cbase = crow0;
              asm volatile("" : "+v"(cbase));  // (opaque: or 64 precomputed row numbers are held in registers across the K loop)
              const uint32_t crow = cbase + (uint32_t)ml;
              if (crow != arow) {  // self is left out by row number
                const uint32_t pos = atomicAdd(&fill[al], 1u);
                if (pos < a.cap) my_list[pos] = make_key(v + 0.0f, crow);
                ++appended;
              }
            }
          }
        // (the wave's own LDS atomics are complete in program order)
        uint32_t f = fill[al];
        if (f > a.cap) {  // appends were dropped: the repair route answers this anchor
          flagged = true;
          f = 0;
        }
        const bool last = ct + 1 == a.cand_tiles;
        const bool need = live && !flagged && lh == 0 && (f + CT > a.cap || (last && f > (uint32_t)a.k));
        u64 m = __ballot(need);
        if (m) {  // (wave-uniform)
          __threadfence();  // the two half-waves' appends are visible to the whole wave
          while (m) {
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const uint32_t sl = (uint32_t)wave * 32 + (uint32_t)src;
            const float tb = __shfl(twob, src), th0 = __shfl(theta, src);
            const float th = knn_compact<R>(a.lists + ((size_t)blockIdx.x * AT + sl) * a.cap, min(fill[sl], a.cap), a.k, tb, th0,
                                            &fill[sl], lane);
            if (l31 == src) theta = th;
          }
          __threadfence();
        }
        if (last && lh == 0) {
          const uint32_t left = fill[al];
          a.counts[blockIdx.x * AT + al] = (live && !flagged) ? min(left, a.cap) : 0u;
          if (arow < a.n_rows) a.flags[arow] = flagged ? 1u : 0u;
        }
      }
      lstore(buf ^ 1);
      __syncthreads();
    }
  }
  // the statistic: entries appended over the sweep
  for (int o = 32; o > 0; o >>= 1) appended += __shfl_xor(appended, o);
  if (lane == 0 && appended) atomicAdd(a.appends, (unsigned long long)appended);
}

typedef void (*knn_tile_fn)(KnnArgs);
static knn_tile_fn pick_knn_tile(int metric) {
  return metric == WDBX_METRIC_L2 ? knn_tile_kernel<WDBX_METRIC_L2> : knn_tile_kernel<WDBX_METRIC_COSINE>;
}

struct KnnExactArgs {
  const f4* rows;        // [n_rows, pitch4] quads
  u64* lists;            // [anchors][cap]: (approximate score, row) in, row_key(exact score, row) out
  const uint32_t* counts;
  uint32_t first;        // the stored row of anchor 0
  uint32_t anchors, cap, pitch4;
};

// One wave per anchor, the anchor's quads in registers (the frame of kernels_rowblock.h: the anchor is the block's one query,
// as in matrix_kernel), its listed candidates fetched and scored one after the other through exact_score_block: a key here is
// the key matrix_kernel makes for (this anchor, this row), bit for bit.
template <int METRIC, int NI>
__global__ __launch_bounds__(256) void knn_exact_kernel(KnnExactArgs a) {
  constexpr int NR = row_block_nr(NI);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t j = (uint32_t)lane;
  const uint32_t W = gridDim.x * 4;
  for (uint32_t i = blockIdx.x * 4 + wave; i < a.anchors; i += W) {
    const uint32_t n = min(a.counts[i], a.cap);  // (wave-uniform)
    if (!n) continue;
    const f4* qp[1] = {a.rows + (size_t)(a.first + i) * a.pitch4};
    f4 q[1][NR];
#pragma unroll
    for (int t = 0; t < NR; ++t) {
      q[0][t] = f4{0.f, 0.f, 0.f, 0.f};
      if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) q[0][t] = qp[0][j + (uint32_t)t * 64];
    }
    u64* const list = a.lists + (size_t)i * a.cap;
    for (uint32_t e = 0; e < n; ++e) {
      const uint32_t row = key_row(list[e]);
      const f4* cp = a.rows + (size_t)row * a.pitch4;
      f4 c[NR];
#pragma unroll
      for (int t = 0; t < NR; ++t) {
        c[t] = f4{0.f, 0.f, 0.f, 0.f};
        if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) c[t] = ld16<true>(cp + j + (uint32_t)t * 64);
      }
      float s[1];
      exact_score_block<METRIC, 1, NI>(c, cp, q, qp, a.pitch4, j, s);
      if (lane == 0) list[e] = row_key(s[0], row);
    }
  }
}

typedef void (*knn_exact_fn)(KnnExactArgs);
template <int METRIC>
static knn_exact_fn pick_knn_exact_metric(uint32_t pitch4) {
  return with_row_block_ni(pitch4, [&](auto ni) -> knn_exact_fn { return knn_exact_kernel<METRIC, decltype(ni)::value>; });
}
static knn_exact_fn pick_knn_exact(int metric, uint32_t pitch4) {
  return metric == WDBX_METRIC_L2 ? pick_knn_exact_metric<WDBX_METRIC_L2>(pitch4) : pick_knn_exact_metric<WDBX_METRIC_COSINE>(pitch4);
}
