// kernels_mmr.h -- wdbx_index_search_mmr on the device: the similarity square of a query's gathered candidates
// (mmr_pairs_kernel) and the greedy selection over it (mmr_select_kernel).  MmrQuery and the grid constants come from
// host_mmr.h.  Part of the single translation unit wdbx_hip.hip (included there, in order); not a standalone header.

struct MmrPairsArgs {
  const f4* rows;        // [sum m, pitch4] the round's gathered candidate rows, query after query
  const MmrQuery* qs;    // [grid.z] the round's queries
  float* G;              // the round's similarity squares: query q's is m x m floats from qs[q].g0, row-major
  uint32_t pitch4;
};

// G[i][j] = the score of candidate row i with candidate row j as the query, exact_score's arithmetic (exact_score_block,
// kernels_rowblock.h: lane order, fma chain, fold and xor tree of kernels_aux.h), in the ranking domain: the inner product + 0.0f
// (as every key normalises it), the negated squared distance as it is.  EVERY (i, j) is computed, nothing is mirrored: the
// products (and the squared differences) commute and the order of summation depends on the element index only, so G[i][j] and
// G[j][i] are the same bits anyway, and each word has the one writer below.
// Grid: x = chunks of MMR_CHUNK_ROWS candidate rows i (wave w of the workgroup takes rows i0 + w, i0 + w + 4, ..., U rows' loads
// in flight), y = blocks of QB candidate columns j0 .. j0 + QB - 1 (their quads in registers for the whole launch when NI > 0,
// read through the caches in the loop form), z = query.  A workgroup past its query's pool returns; the idle column slots of a
// short last block repeat the last candidate and write nothing.  Every lane of a wave ends with the same sum; lane 0 writes.
template <int METRIC, int QB, int NI>
__global__ __launch_bounds__(256) void mmr_pairs_kernel(MmrPairsArgs a) {
  constexpr int U = row_block_u(NI), NR = row_block_nr(NI);
  const MmrQuery mq = a.qs[blockIdx.z];
  const uint32_t m = mq.m, j0 = blockIdx.y * QB, i0 = blockIdx.x * MMR_CHUNK_ROWS;
  if (j0 >= m || i0 >= m) return;  // (workgroup-uniform)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t j = (uint32_t)lane;
  const f4* const base = a.rows + (size_t)mq.row0 * a.pitch4;
  float* const G = a.G + mq.g0;
  const f4* qp[QB];
  f4 q[QB][NR];
#pragma unroll
  for (int b = 0; b < QB; ++b) {
    qp[b] = base + (size_t)min(j0 + (uint32_t)b, m - 1) * a.pitch4;
#pragma unroll
    for (int t = 0; t < NR; ++t) {
      q[b][t] = f4{0.f, 0.f, 0.f, 0.f};
      if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) q[b][t] = qp[b][j + (uint32_t)t * 64];
    }
  }
  const uint32_t i_end = min(i0 + MMR_CHUNK_ROWS, m);
  for (uint32_t cur = i0 + (uint32_t)wave; cur < i_end; cur += U * 4) {
    f4 c[U][NR];
    const f4* cp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      cp[u] = base + (size_t)min(cur + (uint32_t)u * 4, m - 1) * a.pitch4;  // (past the chunk: a row of the pool again, dropped below)
#pragma unroll
      for (int t = 0; t < NR; ++t) {
        c[u][t] = f4{0.f, 0.f, 0.f, 0.f};
        if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) c[u][t] = cp[u][j + (uint32_t)t * 64];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = cur + (uint32_t)u * 4;
      float s[QB];
      exact_score_block<METRIC, QB, NI>(c[u], cp[u], q, qp, a.pitch4, j, s);
      if (lane == 0 && i < i_end) {
#pragma unroll
        for (int b = 0; b < QB; ++b)
          if (j0 + (uint32_t)b < m) G[(size_t)i * m + j0 + b] = METRIC == WDBX_METRIC_L2 ? s[b] : s[b] + 0.0f;
      }
    }
  }
}

typedef void (*mmr_pairs_fn)(MmrPairsArgs);

static mmr_pairs_fn pick_mmr_pairs(int metric, uint32_t pitch4) {
  return with_row_block_ni(pitch4, [&](auto ni) -> mmr_pairs_fn {
    constexpr int NI = decltype(ni)::value;
    return metric == WDBX_METRIC_L2 ? mmr_pairs_kernel<WDBX_METRIC_L2, MMR_BLOCK, NI> : mmr_pairs_kernel<WDBX_METRIC_COSINE, MMR_BLOCK, NI>;
  });
}

struct MmrSelectArgs {
  const MmrQuery* qs;    // [grid.x] the round's queries
  const float* G;        // the round's similarity squares
  const u64* cand;       // [sum m] the candidates' row numbers, position order per query
  const float* rel;      // [sum m] their relevance in the ranking domain (L2: the negated squared distance)
  int64_t* out_idx;      // [grid.x, k] the round's slice of the call's outputs, pick order
  float* out_score;      // ... the pick's relevance as the search returned it (negate: -rel)
  float* out_mmr;        // ... the value the pick won with; may be null
  float lambda;
  int k;
  int negate;            // L2: out_score = -rel
};

// One correctly rounded fp32 multiply / subtract that no later pass may contract with its neighbour into an fma.  The
// toolchain's __fmul_rn / __fsub_rn are a plain `x * y` / `x - y` compiled under the default contraction mode, so the pair
// lambda (x) rel (-) t did fuse; here contraction is switched off for the expression and the result passes an empty asm, which
// ends every fusion across it.
__device__ __forceinline__ float mmr_mul_rn(float x, float y) {
#pragma clang fp contract(off)
  float r = x * y;
  asm volatile("" : "+v"(r));
  return r;
}
__device__ __forceinline__ float mmr_sub_rn(float x, float y) {
#pragma clang fp contract(off)
  float r = x - y;
  asm volatile("" : "+v"(r));
  return r;
}

// the ordering word of a value: NaN below everything (0 < f2ord(-inf)), -0 and +0 one value
__device__ __forceinline__ uint32_t mmr_value_ord(float v) { return v == v ? f2ord(v + 0.0f) : 0u; }

// One workgroup of 256 threads per query; thread t owns positions t, t + 256, ... (8 at the most: m <= MMR_MAX_POOL) and keeps
// their lambda (x) rel, maxsim and picked bit in registers.  Pick 0 is position 0 with the value lambda (x) rel_0.  Every later
// step: v_i = (lambda (x) rel_i) (-) ((1 (-) lambda) (x) maxsim_i) for the unpicked positions -- each operation one rounded fp32
// instruction (mmr_mul_rn / mmr_sub_rn: never contracted) --, the key (mmr_value_ord(v) << 32) | (0xFFFFFFFF - position), the
// wave maxima by __shfl_xor, the four of them through LDS (one barrier pair per step), so every thread knows the winner p: ties
// go to the smaller position, NaN values rank below every number and among themselves by position.  The owner of p writes the
// step's three output words; every thread folds row p of G into its maxsim (a coalesced read; a NaN similarity is skipped).
// Slots behind the last pick get -1 / 0 / 0.  No atomics, no scratch: every output word and every maxsim has one writer.
__global__ __launch_bounds__(256) void mmr_select_kernel(MmrSelectArgs a) {
  constexpr int S = MMR_MAX_POOL / 256;
  __shared__ u64 wave_best[4];
  const MmrQuery mq = a.qs[blockIdx.x];
  const uint32_t m = min(mq.m, (uint32_t)MMR_MAX_POOL), t = threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t picks = min((uint32_t)a.k, m);
  const float* const G = a.G + mq.g0;
  const size_t o0 = (size_t)blockIdx.x * a.k;
  const float one_minus = mmr_sub_rn(1.0f, a.lambda);
  float rel[S], lrel[S], maxsim[S];
  uint32_t picked = 0;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const uint32_t pos = t + (uint32_t)s * 256;
    rel[s] = pos < m ? a.rel[mq.row0 + pos] : 0.0f;
    lrel[s] = mmr_mul_rn(a.lambda, rel[s]);
    maxsim[s] = -INFINITY;
  }
  for (uint32_t step = 0; step < picks; ++step) {
    float v[S] = {};
    u64 best = 0;
    if (step == 0) {
      v[0] = lrel[0];
      if (t == 0) best = 0xFFFFFFFFull;  // position 0, whatever its value
    } else {
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const uint32_t pos = t + (uint32_t)s * 256;
        v[s] = mmr_sub_rn(lrel[s], mmr_mul_rn(one_minus, maxsim[s]));
        if (pos < m && !((picked >> s) & 1u)) best = max(best, ((u64)mmr_value_ord(v[s]) << 32) | (u64)(0xFFFFFFFFu - pos));
      }
    }
    for (int o = 32; o > 0; o >>= 1) best = max(best, (u64)__shfl_xor((unsigned long long)best, o));
    if (lane == 0) wave_best[wave] = best;
    __syncthreads();
    best = max(max(wave_best[0], wave_best[1]), max(wave_best[2], wave_best[3]));
    __syncthreads();
    const uint32_t p = 0xFFFFFFFFu - (uint32_t)best;
    if (p >= m) break;  // (cannot happen while step < picks <= m: an unpicked position always offers a non-zero key; uniform)
    if ((p & 255u) == t) {
      const uint32_t ps = p >> 8;
      float pv = 0.0f, pr = 0.0f;
#pragma unroll
      for (int s = 0; s < S; ++s)
        if ((uint32_t)s == ps) {
          pv = v[s];
          pr = rel[s];
        }
      picked |= 1u << ps;
      a.out_idx[o0 + step] = (int64_t)a.cand[mq.row0 + p];
      a.out_score[o0 + step] = a.negate ? -pr : pr;
      if (a.out_mmr) a.out_mmr[o0 + step] = pv;
    }
    if (step + 1 == picks) break;
    const float* const gp = G + (size_t)p * m;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const uint32_t pos = t + (uint32_t)s * 256;
      if (pos < m) {
        const float g = gp[pos];
        if (g == g) maxsim[s] = fmaxf(maxsim[s], g);
      }
    }
  }
  for (uint32_t slot = picks + t; slot < (uint32_t)a.k; slot += 256) {
    a.out_idx[o0 + slot] = -1;
    a.out_score[o0 + slot] = 0.0f;
    if (a.out_mmr) a.out_mmr[o0 + slot] = 0.0f;
  }
}
