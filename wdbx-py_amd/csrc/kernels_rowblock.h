// kernels_rowblock.h -- the frame the listed-row kernels share: a wave fetches one gathered fp32 row and scores it against a
// block of QB queries held in registers.  subset_kernel, rowlists_kernel, label_keys_kernel, group_members_kernel,
// mmr_pairs_kernel and recommend_kernel are built from these pieces; each keeps its row source, its loads and list tail
// (as functions here they compiled to other code, profiles/rowblock/README.md), its conditions and its sink.  NI is the row's loads per lane (row_block_ni, host_subset.h): NI > 0 keeps a row's and a
// query's quads j, j + 64, ... in NI registers per lane (pitch4 <= 64 NI), NI = 0 is the loop form for any pitch4.
// Part of the single translation unit wdbx_hip.hip (included there, behind kernels_aux.h); not a standalone header.

// registers of quads per lane that hold one row (or one query), and the rows whose loads a wave keeps in flight
constexpr int row_block_nr(int ni) { return ni > 0 ? ni : 1; }
constexpr int row_block_u(int ni) { return ni == 0 ? 1 : (ni <= 2 ? 4 : 2); }

// One loaded row against QB queries, each with exact_score's arithmetic (kernels_aux.h): lane j accumulates quads j, j + 64,
// ... in that order with accum<METRIC> and exact_finish folds and reduces, so a score here is rescore_kernel's score bit for
// bit -- the row's quads are simply used QB times once they are in registers.
//   NI > 0 (pitch4 <= 64 NI): the queries' quads live in registers for the whole launch (q), the row's NI loads are issued by
//   the caller (c), nothing is loaded here.  NI = 0: any pitch4, the loop, the queries read through the caches (qp).
template <int METRIC, int QB, int NI>
__device__ __forceinline__ void exact_score_block(const f4 (&c)[NI > 0 ? NI : 1], const f4* cp, const f4 (&q)[QB][NI > 0 ? NI : 1],
                                                  const f4* const (&qp)[QB], uint32_t pitch4, uint32_t j, float (&s)[QB]) {
  f4 acc[QB];
#pragma unroll
  for (int b = 0; b < QB; ++b) acc[b] = f4{0.f, 0.f, 0.f, 0.f};
  if constexpr (NI == 0) {
    for (uint32_t i = j; i < pitch4; i += 64) {
      const f4 v = ld16<true>(cp + i);
#pragma unroll
      for (int b = 0; b < QB; ++b) acc[b] = accum<METRIC>(acc[b], v, qp[b][i]);
    }
  } else {
#pragma unroll
    for (int t = 0; t < NI; ++t)
      if (j + (uint32_t)t * 64 < pitch4) {
#pragma unroll
        for (int b = 0; b < QB; ++b) acc[b] = accum<METRIC>(acc[b], c[t], q[b][t]);
      }
  }
#pragma unroll
  for (int b = 0; b < QB; ++b) s[b] = exact_finish<METRIC, 64>(acc[b]);
}

// the key of a scored row: a NaN score is never a result, -0 and +0 are one score
__device__ __forceinline__ u64 row_key(float s, uint32_t row) { return s == s ? make_key(s + 0.0f, row) : 0ull; }

// optional row filter: bit r % 32 of word r / 32 set = row r may be returned; no mask allows every row
__device__ __forceinline__ bool row_allowed(const uint32_t* mask, uint32_t row) {
  return !mask || ((mask[row >> 5] >> (row & 31)) & 1u);
}
