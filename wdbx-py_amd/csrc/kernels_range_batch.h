// kernels_range_batch.h -- batched range search (wdbx_index_range_search_batch): what a block of range queries needs in front
// of the int8 tile kernel's full pass.  Part of the single translation unit wdbx_hip.hip (included there, in order); not a
// standalone header.
//
// The block runs queries_to_i8_kernel, range_batch_bound_kernel (here), gemm_i8_kernel<PHASE 1> (the product instances,
// unchanged), scatter_pairs_kernel and range_filter_kernel.  Only the bound kernel is new: the top-k path takes tau from a sample
// of the corpus and its exact pass RANKS, so nothing there has to cover the exact pass's own rounding; here the caller chose
// the threshold and the exact pass DECIDES on its fp32 score, which may exceed the real c.q.  
//
//   The tiles keep row r iff  s_g s_q D + a_g E_q + b_g M_q >= tau,  an upper bound of the REAL c.q.
//   exact_score (kernels_aux.h) sums the products per lane by fmas (pitch / 256 deep), folds 4 components (2 adds) and 64
//   lanes (6 adds): every product passes through at most pitch / 256 + 8 <= 24 roundings up to 4096 dimensions, so
//       |fl(c.q) - c.q| <= gamma_24 sum |c_i q_i| <= RANGE_BATCH_GAMMA |c|_2 |q|_2,   RANGE_BATCH_GAMMA = 2e-6 > 24 u / (1 - 24 u),  u = 2^-24
//   (no overflow: |c|_2 |q|_2 below 2^127; and no underflow: a product or partial sum below 2^-126 is rounded with an ABSOLUTE
//   error of up to 2^-149, (d + 8) 2^-149 < 6e-42 in all, which gamma does not scale with.  The tile test covers it by the
//   a_g * 2e-5 sqrt(d) s_q part of a_g E_q alone, >= 2.5e-3 sqrt(d) s_g s_q for a group that is not vanishing, whenever
//   max|c| of the group times max|q| is at least 1e-36; below that the guarantee is not claimed, as above 2^127.)  Two facts turn that into the tile test's own terms:
//       |q|_2 = s_q |m + eps|_2 <= s_q (|m|_2 + |eps|_2) = M_q          (M_q is rounded up by the quantiser, whatever the query's scale)
//       |c_r|_2 = s_g |n_r + delta_r|_2 <= a_r + b_r <= a_g + b_g
//   so adding G = RANGE_BATCH_GAMMA M_q (rounded up, and the sums as well) to BOTH E_q and M_q widens the test by G (a_g + b_g) >= gamma |q|_2 |c_r|_2:
//   every row whose fp32 score reaches t has  real c.q >= t - gamma |c||q|  and passes.  Nothing here assumes unit rows or
//   unit queries.  L2 decides on the fp32 sum of (c - q)^2, whose rounding the caller's tau already covers
//   (range_selection_tau_l2); the widened E, M are kept for L2 too (a wider test is never wrong).
//
// tau: the host's selection thresholds (cosine: t; L2: range_selection_tau_l2), limited to 1e38 s_q so that the tile kernel's
// tau / s_q stays finite (lowering tau only keeps more rows; with t = +inf the rows of groups holding an infinite element
// still reach the exact pass, which alone can find a score of +inf); padded slots: +inf (pad_tau_kernel's rule).
// Also zeroes the block's result counters, so that no memset launch sits between the kernels of a block.
constexpr float RANGE_BATCH_GAMMA = 2e-6f;

// one thread per slot of the query block, behind queries_to_i8_kernel on the same stream
__global__ __launch_bounds__(256) void range_batch_bound_kernel(uint32_t nv, uint32_t gbn, f4* qpar, const float* tau_in, float* tau,
                                                                uint32_t* result_count_zero) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= gbn) return;
  result_count_zero[r] = 0u;
  if (r >= nv) {
    tau[r] = INFINITY;
    return;
  }
  f4 par = qpar[r];  // {s_q, E_q, M_q, 1 / s_q}
  const float G = RANGE_BATCH_GAMMA * par.z * 1.000001f;
  // (the sums are taken one ulp UP: rounded to nearest, E + G loses up to half an ulp of E -- far more than G's own margins,
  // G = 2e-6 M being a few ulps of M and of a typical E -- and the widening would fall short of RANGE_BATCH_GAMMA M)
  constexpr float ULP_UP = 1.0f + 1.1920929e-7f;  // 1 + 2^-23: x * ULP_UP >= x + ulp(x)
  par.y = (par.y + G * 1.000001f) * ULP_UP;  // (a non-finite query has E = +inf already and stays there)
  par.z = (par.z + G * 1.000001f) * ULP_UP;
  qpar[r] = par;
  tau[r] = fminf(tau_in[r], 1e38f * (par.x > 0.f ? par.x : 1.0f));
}
static inline uint32_t range_batch_bound_grid(uint32_t gbn) { return (gbn + 255) / 256; }
