// kernels_scan42.h -- the six-bit selection scan split in two planes: every query streams the codes' top four bits, the low
// two bits are read only for the rows the four-bit bound cannot rule out ("u42").
// Part of the single translation unit wdbx_hip.hip (included there, after kernels_scan6.h); not a standalone header.

// ------------------------------------------------------------------------------------------------
// The u6 full pass is the bytes it reads (288 B of codes + 8 B per row at d = 384).  The SAME six-bit code u = rint(c / s) + 32
// (rows_to_u6_kernel's quantiser: u6_row_scale / u6_unit_codes) is stored as u = 4 h + l, h in 0 .. 15, l in 0 .. 3:
//   h plane   tiles of 64 rows, unit-major, a unit = 32 codes = 16 bytes:  [tile][unit][row 0..63][4 dwords].  Lane = row; one
//             16-byte load per lane and unit is 1 KiB contiguous per wave.  Dword t byte b holds h of element 8 t + b in its
//             low nibble and of element 8 t + 4 + b in its high nibble: (d & 0x0F0F0F0F) and (d >> 4 & 0x0F0F0F0F) feed two
//             packed converts each (u42_cvt4) -- 3 logic ops + 4 converts + 4 v_pk_fma_f32 per dword of eight elements.
//   {s, a4}   per row: the u6 scale and  a4 >= |c - s (4 h + 1.5 - 32)|_2,  the residual of the row against the MIDPOINT of
//             what the low bits can add, rounded up with the allowances rows_to_u6_kernel derives for a (same arithmetic:
//             rho4 = fmaf(-s, 4 h - 30.5, x) * inv -- 4 h - 30.5 is exact in fp32 --, a sum of at most dimp squares, one root).
//             Padding elements (query 0 there) are left out of a4.
//   l plane   row-major, one 128-byte-aligned record per row: dimp / 4 bytes of two-bit remainders (dword g of a unit holds
//             elements 16 g .. 16 g + 15, element 4 j + b in bits [8 b + 2 j, 8 b + 2 j + 1]: (w >> 2 j) & 0x03030303 is four of
//             them as bytes), then a6 = the u6 shadow's a, bit for bit (the same sum in the same order).
// scan_u42_kernel, lane = row, forms P = sum h_i q_i (query through scalar loads, v_pk_fma_f32 as scan8_u6_kernel) and
//   w4 = s (4 P - 30.5 sum q),   |w4 - c.q| <= m4 = a4 |q|_2 (1 + 1e-5) + 6e-6 (dimp + 8) s |q|_1 (1 + 1e-5).
// First term: Cauchy-Schwarz on the stored residual, as in kernels_scan6.h.  Second term, the fp32 roundings of the kernel's
// own arithmetic: the sum of dimp products |h_i q_i| <= 15 |q_i| in any order, times 4 exactly (gamma_dimp * 60 |q|_1), the sum
// behind 30.5 sum q and that product (gamma_(dimp + 1) * 30.5 |q|_1), their difference (a fused multiply-add or two roundings)
// and the product with s, of a value of at most 90.5 |q|_1: (dimp + 8) * 2^-24 * 90.5 < 5.4e-6 (dimp + 8), taken as 6e-6.
// A row with !(w4 + m4 < tau) is a SURVIVOR: {row, P, s} go to a list of the wave in LDS.  When the list holds 64 (and once
// more, masked, behind the wave's last tile) the wave refines densely, lane = survivor: the lane walks its own l record with
// the same scalar query, Q = sum l_i q_i, and
//   w6 = s ((4 P + Q) - 32 sum q),   |w6 - c.q| <= m6 = a6 |q|_2 (1 + 1e-5) + 6e-6 (dimp + 8) s |q|_1 (1 + 1e-5):
// 4 P as above (gamma_dimp * 60 |q|_1), the sum of dimp products |l_i q_i| <= 3 |q_i| (gamma_dimp * 3 |q|_1), their sum (one
// rounding of at most 63 |q|_1), 32 sum q (gamma_dimp * 32 |q|_1), the difference and the product with s (of at most 95 |q|_1):
// (dimp + 8) * 2^-24 * 95 < 5.7e-6 (dimp + 8), the u6 scan's own term.  w6 estimates the u6 scan's w (the same codes) and m6
// is its m; rows with !(w6 + m6 < tau) go to the candidate buffer through the WaveStage exactly as there.  Both bounds are
// rigorous, so no row whose score reaches tau is lost; the re-scoring, the cut and the merge behind the pass are the u6
// scan's, the threshold in front of it is too.  NaN / inf rows: a negative scale skips the row, a NaN scale makes w4 and w6
// NaN, so the row survives both comparisons and is appended with +inf.
// The converts return h_i 2^-9 and l_i 2^-9 (u42_cvt4), so the kernel carries P' = 2^-9 P and Q' = 2^-9 Q and forms 2048 P' and
// 512 Q'.  Every fma sees the operands above in the order above scaled by an exact power of two, so 512 P' is P bit for bit
// unless a partial sum falls below 2^-126: there a rounding errs by at most 2^-150 instead of relatively (unscaled, sums of
// the multiples h_i q_i of 2^-149 are exact down there).  dimp fmas feed P', dimp feed Q': 2048 P' is off by at most
// dimp 2^-139 and 512 Q' by dimp 2^-141, together below dimp 2^-138, which the kernel adds to the rounding term inside the
// product with s: m = a |q|_2 (1 + 1e-5) + s (6e-6 (dimp + 8) |q|_1 (1 + 1e-5) + dimp 2^-138).  For |q|_1 above 1e-33 the
// addend vanishes in the sum's own rounding and m is the number it was.  Premise: the kernel runs with fp32 denormals KEPT
// (the compiler's default for this target, float_denorm_mode_32 = 3 in the kernel descriptor; the build sets no flush flag):
// flushed, a rounding down there would err by 2^-126 and the addend itself would be 0
// (tests/test_gpu_u42_edges.py runs a query of magnitude 1e-36, whose partial sums are all subnormal, against -inf: it checks
// the returned w6; NO device test exercises the addend in a decision w + m < tau, since at that magnitude the squares in
// u6_query_sums underflow and q2 is its floor of 1e-37).  The product with s
// has its own underflow, as before the scaling: s * (...) and w = s * (...) round to within 2^-150 once they fall below
// 2^-126, so for rows whose bounds are of the order of 1e-40 and less m can lose the addend or part of the term; the
// comparison w + m < tau then decides between scores no fp32 re-scoring tells apart from 0.
// ------------------------------------------------------------------------------------------------
typedef uint32_t u4v __attribute__((ext_vector_type(4)));

struct Scan42Args {
  const uint32_t* hcodes;  // [tiles][units][64][4]
  const f2v* sa4;          // [rows] {s, a4}
  const uint32_t* lrec;    // [rows][lpitch]: units * 2 dwords of remainders, then a6
  const float* query;      // fp32 [units * 32] per query, pitch qpitch floats (zero padded)
  uint32_t n_rows, units, qpitch, lpitch;
  const float* tau;
  u64* cand;
  uint32_t* count;
  uint32_t* survivors;     // optional: rows that passed the four-bit bound, per query (probes and tests)
  uint32_t cap;
};

// dwords of one l record: the remainders and a6, rounded up to whole 128-byte lines
static inline uint32_t u42_lpitch(uint32_t units) { return (units * 2 + 1 + 31) / 32 * 32; }

template <bool NT>
__device__ __forceinline__ u4v u42_load(const uint32_t* p) {
  const u4v* q = (const u4v*)p;
  if constexpr (NT) return __builtin_nontemporal_load(q);
  return *q;
}

// four masked bytes 0 .. 15 of one dword as two float pairs SCALED BY 2^-9: {byte 0, byte 1} and {byte 2, byte 3}.  Read as OCP
// e4m3 the byte 0x0h is exactly h * 2^-9 (0 .. 7: the subnormals m * 2^-9; 8 .. 15: exponent field 1, (8 + m) * 2^-9), so one
// v_cvt_pk_f32_fp8 makes the pair a v_pk_fma_f32 takes (tests/test_gpu_u42_convert.py: every value in every position, bitwise)
__device__ __forceinline__ void u42_cvt4(uint32_t w, f2v& lo, f2v& hi) {
  asm volatile("" : "+v"(w));  // (the masked dword stays ONE value, as in u6_cvt4)
  lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
}

// the eight nibbles of one dword as pairs scaled by 2^-9: elements {0,1} {2,3} from the low nibbles, {4,5} {6,7} from the high ones
__device__ __forceinline__ void u42_unpack8(uint32_t d, f2v (&f)[4]) {
  u42_cvt4(d & 0x0F0F0F0Fu, f[0], f[1]);
  u42_cvt4((d >> 4) & 0x0F0F0F0Fu, f[2], f[3]);
}

// remainders 4 j .. 4 j + 3 of one l dword as pairs scaled by 2^-9
__device__ __forceinline__ void u42_rem4(uint32_t w, int j, f2v& lo, f2v& hi) { u42_cvt4((w >> (2 * j)) & 0x03030303u, lo, hi); }

// the wave's survivor list: 128 entries, < 64 held between tiles; p = 2^-9 P
struct U42List {
  uint32_t row[128];
  float p[128];
  float s[128];
};

__device__ __forceinline__ void u42_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// dense refine of the first n (<= 64) entries of the wave's list, lane = survivor; the rest moves to the front
__device__ __forceinline__ void u42_refine(const Scan42Args& a, cfloat* q, U42List& ls, uint32_t& fill, uint32_t n, float qsum32,
                                           float q2, float round1, float thr, WaveStage& st, int lane) {
  u42_wave_sync();
  const uint32_t l = (uint32_t)lane;
  const bool active = l < n;
  const uint32_t row = active ? ls.row[l] : 0u;  // (idle lanes walk record 0: always there)
  const float p4 = active ? ls.p[l] : 0.f;
  const float s = active ? ls.s[l] : 0.f;
  const uint32_t rest = fill - n;  // (< 64)
  const uint32_t m_row = l < rest ? ls.row[n + l] : 0u;
  const float m_p = l < rest ? ls.p[n + l] : 0.f, m_s = l < rest ? ls.s[n + l] : 0.f;
  u42_wave_sync();
  if (l < rest) ls.row[l] = m_row, ls.p[l] = m_p, ls.s[l] = m_s;
  fill = rest;
  u42_wave_sync();
  if (a.survivors && lane == 0) atomicAdd(a.survivors, n);
  const uint32_t* rec = a.lrec + (size_t)row * a.lpitch;
  f2v a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
  for (uint32_t u = 0; u < a.units; ++u) {
    const uint32_t w0 = rec[2 * u], w1 = rec[2 * u + 1];
    cfloat* qu = q + u * 32;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const uint32_t w = g ? w1 : w0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f2v lo, hi;
        u42_rem4(w, j, lo, hi);
        const int i = 16 * g + 4 * j;
        a0 = __builtin_elementwise_fma(lo, f2v{qu[i], qu[i + 1]}, a0);
        a1 = __builtin_elementwise_fma(hi, f2v{qu[i + 2], qu[i + 3]}, a1);
      }
    }
  }
  const float a6 = __uint_as_float(rec[2 * a.units]);
  const float qq = (a0.x + a0.y) + (a1.x + a1.y);
  const float w = s * (fmaf(2048.0f, p4, 512.0f * qq) - qsum32);  // (= 4 P + Q in one rounding: both products are exact)
  const float m = fmaf(a6, q2, s * round1);
  const bool keep = active && !(w + m < thr);
  st.push(keep, make_key((w == w) ? w + 0.0f : INFINITY, row), a.cand, a.count, a.cap, lane);
}

// full pass: UC units in flight per wave (a last, shorter chunk when UC does not divide the row's units), one 64-row tile per
// wave at a time.  QP consecutive queries of the round (blockIdx.y = the group) share the wave's loads: the unit loads, the
// {s, a4} load and the unpack of every dword happen once, the four packed fmas follow once per query with that query's scalar
// operands in the lone pass's order of t and of a0 / a1.  Everything behind the sum -- threshold, bounds, survivor list, refine,
// stage, candidate buffer and counters -- is the query's own, so P', w, m, the survivors and the candidate keys of a query are
// bit for bit what its lone pass (QP = 1) computes; only the order in which waves append to a buffer differs, as it does from
// run to run.  LDS: QP x (4 KiB stage + 6 KiB lists) per workgroup.
// QP = 1 is the kernel as it was before the parameter existed in its vector instructions (at UC = 6: 128 packed fmas, 128
// packed converts, 60 VGPRs, the same loop), NOT in its scalar bookkeeping: six more scalar instructions in the prologue and
// another register assignment.  The per-query state lives in arrays here (a copy of the arguments per query, aq[j] = a plus
// the pointer adds, where the lone kernel advanced `a` in place); indexing the survivor lists directly instead of through
// ls[] did not bring the old code back, nothing else was tried.  Measured, the instance runs at the old kernel's rate
// (profiles/u42_share/README.md).
template <int UC, int QP = 1>
__global__ __launch_bounds__(256) void scan_u42_kernel(Scan42Args a) {
  __shared__ u64 stage42[QP][4][128];
  __shared__ U42List list42[QP][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Scan42Args aq[QP];  // (the query's own tau, cand, count and survivors; the planes are the group's)
  cfloat* q[QP];
  float qsum32[QP], qsum305[QP], q2[QP], thr[QP], round1[QP];
  WaveStage st[QP];
  U42List* ls[QP];
  uint32_t fill[QP];
#pragma unroll
  for (int j = 0; j < QP; ++j) {
    const uint32_t qi = blockIdx.y * QP + j;
    const float* qg = a.query + (size_t)qi * a.qpitch;
    q[j] = (cfloat*)qg;
    aq[j] = a;
    aq[j].tau += qi;
    aq[j].cand += (size_t)qi * a.cap;
    aq[j].count += qi;
    if (a.survivors) aq[j].survivors += qi;
    float q1;
    u6_query_sums(qg, a.units * 32, lane, qsum32[j], q1, q2[j]);
    qsum305[j] = 30.5f * (qsum32[j] * 0.03125f);
    thr[j] = aq[j].tau[0];
    round1[j] = fmaf(6e-6f * (float)(a.units * 32 + 8), q1, (float)(a.units * 32) * 0x1p-138f);
    st[j] = {stage42[j][wave], 0u};
    ls[j] = &list42[j][wave];
    fill[j] = 0;
  }
  const uint32_t tiles = (a.n_rows + 63) / 64;
  const size_t tile_dw = (size_t)a.units * 256;
  for (uint32_t tile = blockIdx.x * 4 + wave; tile < tiles; tile += gridDim.x * 4) {
    const uint32_t row = tile * 64 + (uint32_t)lane;
    const uint32_t* p = a.hcodes + tile * tile_dw + lane * 4;
    const f2v sa = __builtin_nontemporal_load(a.sa4 + min(row, a.n_rows - 1));
    f2v a0[QP], a1[QP];
#pragma unroll
    for (int j = 0; j < QP; ++j) a0[j] = f2v{0.f, 0.f}, a1[j] = f2v{0.f, 0.f};
    for (uint32_t u0 = 0; u0 < a.units; u0 += UC) {
      u4v v[UC];
#pragma unroll
      for (int u = 0; u < UC; ++u) v[u] = u42_load<true>(p + (size_t)min(u0 + u, a.units - 1) * 256);  // (the last chunk may be short)
#pragma unroll
      for (int u = 0; u < UC; ++u) {
        if (u0 + u < a.units) {  // (wave-uniform)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            f2v f[4];
            u42_unpack8(v[u][t], f);
#pragma unroll
            for (int j = 0; j < QP; ++j) {
              cfloat* qu = q[j] + (u0 + u) * 32;
              a0[j] = __builtin_elementwise_fma(f[0], f2v{qu[8 * t], qu[8 * t + 1]}, a0[j]);
              a1[j] = __builtin_elementwise_fma(f[1], f2v{qu[8 * t + 2], qu[8 * t + 3]}, a1[j]);
              a0[j] = __builtin_elementwise_fma(f[2], f2v{qu[8 * t + 4], qu[8 * t + 5]}, a0[j]);
              a1[j] = __builtin_elementwise_fma(f[3], f2v{qu[8 * t + 6], qu[8 * t + 7]}, a1[j]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < QP; ++j) {
      const float p4 = (a0[j].x + a0[j].y) + (a1[j].x + a1[j].y);  // = 2^-9 P
      const float w = sa.x * (2048.0f * p4 - qsum305[j]);
      const float m = fmaf(sa.y, q2[j], sa.x * round1[j]);
      // (as the u6 pass: a NaN bound keeps the row, a negative scale marks a row with a NaN element)
      const bool surv = row < a.n_rows && !(sa.x < 0.f) && !(w + m < thr[j]);
      const u64 bal = __ballot(surv);
      if (bal) {
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (surv) ls[j]->row[fill[j] + rank] = row, ls[j]->p[fill[j] + rank] = p4, ls[j]->s[fill[j] + rank] = sa.x;
        fill[j] += (uint32_t)__popcll(bal);
        if (fill[j] >= 64) u42_refine(aq[j], q[j], *ls[j], fill[j], 64u, qsum32[j], q2[j], round1[j], thr[j], st[j], lane);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < QP; ++j) {
    if (fill[j]) u42_refine(aq[j], q[j], *ls[j], fill[j], fill[j], qsum32[j], q2[j], round1[j], thr[j], st[j], lane);
    st[j].finish(aq[j].cand, aq[j].count, aq[j].cap, lane);
  }
}

// ------------------------------------------------------------------------------------------------
// The full pass on the matrix cores: 16 queries of a round per read of the four-bit plane (scan_u42_mfma_kernel).
//
// The first stage is a small integer GEMM, rows x 16 queries x dimp, on v_mfma_i32_16x16x64_i8.  The h plane serves as the A
// operand as it is stored: for the 16-row block rb of a tile and the chunk of four units from u0, lane L loads the 16 bytes of
// row 16 rb + (L & 15), unit u0 + (L >> 4); d & 0x0F0F0F0F and (d >> 4) & 0x0F0F0F0F of its four dwords are two A operands of
// K = 64 (elements 8 t + b and 8 t + 4 + b of the four units).  The B operand holds, in the lane with the same L >> 4, the 16
// bytes of query L & 15 for the same unit in the same byte order: lane groups and byte positions of A and B pair up, so the
// sum does not depend on the instruction's internal order of k.  Lane groups past the row's units (a short last chunk) load
// nothing and contribute zero.  The B fragments of the group stay in registers for the whole pass (units <= 12: 3 chunks x 2
// nibble parities x 2 query bytes x 4 = 48 VGPRs); no operand goes through LDS, no barrier in the loop.
//
// THE QUERY is a 16-bit fixed-point number per element (u42_query_i16_kernel, once per round): delta = the power of two with
// 16256 < max|q_i| / delta <= 32512, Q_i = rint(q_i / delta) = 256 H_i + L_i with H_i = (Q_i + 128) >> 8 in -127 .. 127 and L_i in
// -128 .. 127 (32512 = 127 * 256: the largest magnitude whose H fits a signed byte for both signs).  q_i / delta, Q_i and the
// residual rho_i = q_i / delta - Q_i are exact in fp32 (a power-of-two quotient, an integer below 2^15, a difference of
// neighbours), e2 = delta * (sqrt(sum rho_i^2) * 1.0005 + 1e-20) >= |q - delta Q|_2: 5e-4 covers the sum of up to 4096 squares in
// any order (gamma / 2 <= 1.25e-4), the root and the products, 1e-20 the squares that underflow (each below 2^-149, together
// below 2^-137: 2^-68.5 under the root).  An all-zero query: delta = 1, Q = 0, e2 = 0.
// A query is MARKED when an element is not finite, when max|q_i| >= 2^64 or when 0 < max|q_i| < 2^-44.  Above 2^64 the fp32
// sum of squares behind |q|_2 is infinite and every kernel of this family keeps every row anyway; below 2^-44 delta would fall
// under 2^-58 and delta * 1e-20, the smallest e2, under the normal range (2^-58 * 2^-66.4 > 2^-126 is the limit taken).  Inside
// the limits delta is in [2^-58, 2^50]: delta, 1 / delta, 2^-9 delta and their products with integers below 2^31 are normal or zero.
// A marked query takes no part in the integer sum (its bytes are zero); its threshold is read as -inf in BOTH stages, so every
// row is its candidate, as the VALU pass keeps every row of a NaN query: on a corpus beyond the capacity the counter ends above
// cap behind cap real keys (rescore_kernel reads them, so they must name rows) and the conditional repair launches answer the
// query exactly; on a smaller corpus every row is re-scored, which is exact too.
//
// ACCUMULATORS.  Dh = sum h_i H_i and Dl = sum h_i L_i, exact in int32; P_int = 256 Dh + Dl = sum h_i Q_i with
// |P_int| <= 15 * 32512 * dimp = 487 680 dimp < 2^31 up to dimp = 4403; the largest instance has dimp = 384: 1.9e8 (and |Dh| <=
// 15 * 127 * 384, |Dl| <= 15 * 128 * 384).
// EPILOGUE.  The D layout gives lane L query L & 15 and rows 4 (L >> 4) + i of the block.  P^ = delta float(P_int) (ONE rounding,
// the conversion), the survivor entry carries 2^-9 P^ as the VALU pass carries 2^-9 P, and
//   w4 = s (4 P^ - 30.5 sum q),   |w4 - c.q| <= m4' = a4 |q|_2 (1 + 1e-5) + s round1',
//   round1' = round1 + 60 sqrt(dimp) e2 (1 + 1e-5),   round1 = 6e-6 (dimp + 8) |q|_1 (1 + 1e-5) + dimp 2^-138 as above.
// Query term: sum h_i q_i - delta P_int = sum h_i (q_i - delta Q_i), at most |h|_2 |e|_2 <= 15 sqrt(dimp) e2 by Cauchy-Schwarz; times
// 4 s.  Rounding term: |P^| can exceed 15 |q|_1 by that quantisation, |delta P_int| <= 15 (|q|_1 + sqrt(dimp) e2) and sqrt(dimp) e2 <=
// dimp delta / 2 (1 + 5e-4) < dimp |q|_1 / 32512 <= 0.127 |q|_1 up to dimp = 4096, so 4 |P^| <= 67.6 |q|_1.  The roundings of w4 are
// the conversion (of at most 67.6 |q|_1), the sum behind 30.5 sum q and that product (gamma_(dimp + 1) * 30.5 |q|_1), the
// difference and the product with s (of at most 98.1 |q|_1): (67.6 + 30.5 (dimp + 1) + 3 * 98.1) 2^-24 |q|_1, below the
// 90.5 (dimp + 8) 2^-24 |q|_1 the term was derived for at every dimp >= 32 (dimp = 32: 1368 against 3620).  The sum round1 + query
// term rounds once more (2^-24 relative): inside the step from 5.4e-6 to the 6e-6 taken.
// REFINE.  u42_mfma_finish forms u42_refine's w6 = s ((4 P^ + Q) - 32 sum q) from the carried P^ and the fp32 query's remainders.  Its
// roundings: the conversion (67.6 |q|_1), the remainders' sum (gamma_dimp * 3 |q|_1), 4 P^ + Q in one rounding (70.6 |q|_1), 32 sum q
// (gamma_dimp * 32 |q|_1), the difference and the product with s (102.6 |q|_1): (67.6 + 35 dimp + 70.6 + 3 * 102.6) 2^-24 |q|_1, below
// 95 (dimp + 8) 2^-24 |q|_1 likewise.  4 P^ misses 4 sum h_i q_i by the same query term, so m6' = a6 |q|_2 (1 + 1e-5) + s round1': the
// refine takes round1' where u42_refine takes round1.
// SURVIVOR LISTS.  Per wave and query a list of U42_MFMA_LIST_CAP = 128 {row, 2^-9 P^} pairs in LDS (8 bytes: s is read again from
// {s, a4} when the list is refined -- the same bits); lanes append through an LDS counter, one add per survivor.  A tile adds at
// most 64 entries to a list and a list holds fewer than U42_MFMA_TRIGGER = 64 between tiles (63 + 64 < 128); behind a tile in which
// any lane appended, ONE ballot finds the lists of 64 or more and the wave refines the LAST 64 entries of each (what stays is in
// front already, nothing moves).  MEASURED AND LEFT OUT (profiles/u42_mfma_pipe/README.md): deciding a lane's sixteen pairs into a
// mask first and appending with one LDS add of popcount(mask) per lane and tile -- no faster than the add per survivor once the
// refine is short (0.8 % of the pairs survive on the headline corpus: about six adds per tile and wave); the next tile's twelve
// loads in flight under this tile's MFMAs (203 VGPRs) -- 3.5 % on the pass alone at two workgroups per CU, below the bar.
// REFINE in two halves.  u42_mfma_gather issues every load of up to 64 entries, lane = entry, all addressed by the entry's row:
// the row's scale and the 128-byte l record as six 16-byte loads plus a6 -- no load waits for another.  u42_mfma_finish forms
// u42_refine's sums in its order (units, dwords, j; a0 / a1), w6, m6 and the key.  Behind the last tile about sixteen short lists
// are left per wave (on the headline corpus a wave meets about 40 survivors per query, below the trigger): the gather of the next
// list is issued before the finish of the current one.
// ONE STAGE for the sixteen columns (U42Stage16): kept keys wait in LDS with their column and go out 64 at a time or at the wave's
// end.  A flush ranks the 64 keys inside their columns (sixteen ballots), the first lane of every column adds the column's number
// to the column's counter -- one atomic instruction of up to sixteen lanes -- and every lane stores at base + rank of its column.
// Capacity and overflow are per column as before: the counter ends above cap, keys at base + rank >= cap are dropped, the keys below
// cap name real rows.  A wave keeps about two candidates per query, so this is one atomic latency per wave where a stage flushed
// per refine paid sixteen; only the order of the keys inside a buffer differs.  The survivors counter takes the wave's sum per
// column in one instruction of sixteen lanes at the wave's end.
// LDS: 4 waves x (16 KiB lists + 1 KiB + 128 B stage + 512 B of {s, a4} + 64 B of counters) = 70.6 KiB per workgroup: two fit a CU and
// two run, one wave of each per SIMD (the sweep in host_index.h).
// ------------------------------------------------------------------------------------------------
typedef int i4v __attribute__((ext_vector_type(4)));

constexpr uint32_t U42_MFMA_QUERIES = 16;    // queries per group
constexpr uint32_t U42_MFMA_MAX_UNITS = 12;  // the one instance: three chunks of four units (d <= 384)
constexpr uint32_t U42Q_MARKED = 1u, U42Q_ABSENT = 2u;

// what the epilogue and the refine need of one query, computed once per round
struct U42QConst {
  float dp;       // 2^-9 delta
  float qsum305;  // 30.5 sum q
  float qsum32;   // 32 sum q
  float q2;       // |q|_2 (1 + 1e-5) + 1e-37
  float round1;   // round1'
  float e2;
  float delta;
  uint32_t flags;
};

// chunks of four units, fragments of 64 lanes x 16 bytes per group (chunk x nibble parity x query byte)
__host__ __device__ static inline uint32_t u42_mfma_chunks(uint32_t units) { return (units + 3) / 4; }
static inline uint32_t u42_mfma_group_dwords(uint32_t units) { return u42_mfma_chunks(units) * 4 * 256; }
// THE dispatch rule: unit counts with an instance of scan_u42_mfma_kernel; every other count stays on scan_u42_kernel
static inline bool u42_mfma_has_instance(uint32_t units) { return units >= 9 && units <= U42_MFMA_MAX_UNITS; }

// query `blockIdx.x` of the round -> its B fragments in group blockIdx.x / 16, column blockIdx.x % 16, and its U42QConst; one wave
// per query.  Queries [nq, gridDim.x) are absent columns of a short group: zero bytes, flag U42Q_ABSENT.
// qb: [groups][chunk][parity][H, L][64 lanes][4 dwords]; lane (kg, col) dword t byte b = element 32 (4 chunk + kg) + 8 t + 4 parity + b.
__global__ __launch_bounds__(64) void u42_query_i16_kernel(const float* queries, uint32_t qpitch, uint32_t units, uint32_t nq,
                                                           uint32_t* qb, U42QConst* qc) {
  const int lane = threadIdx.x;
  const uint32_t qi = blockIdx.x, dimp = units * 32, chunks = u42_mfma_chunks(units);
  const bool present = qi < nq;
  const float* qg = queries + (size_t)(present ? qi : 0u) * qpitch;
  float qsum32, q1, q2;
  u6_query_sums(qg, dimp, lane, qsum32, q1, q2);
  float mx = 0.f;
  bool finite = true;
  for (uint32_t i = (uint32_t)lane; i < dimp; i += 64) {
    const float v = fabsf(qg[i]);
    finite = finite && v < INFINITY;  // (false for NaN too)
    mx = fmaxf(mx, v);
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  finite = __ballot(!finite) == 0ull;
  const bool marked = !finite || mx >= 0x1p64f || (mx > 0.f && mx < 0x1p-44f);
  const bool zero = !present || marked || mx == 0.f;
  float delta = 1.0f, inv = 1.0f;
  if (!zero) {
    const uint32_t e = __float_as_uint(mx) >> 23;  // mx in [2^(e - 127), 2^(e - 126)): mx / 2^(e - 141) in [2^14, 2^15)
    delta = __uint_as_float((e - 14u) << 23);
    if (mx * __uint_as_float((254u - (e - 14u)) << 23) > 32512.0f) delta *= 2.0f;
    inv = 1.0f / delta;  // (a power of two in [2^-50, 2^58]: exact)
  }
  float rr = 0.f;
  uint32_t* out = qb + (size_t)(qi / U42_MFMA_QUERIES) * (chunks * 4 * 256) + (qi % U42_MFMA_QUERIES) * 4;
  // a lane per quad of elements: unit u, dword t, nibble parity par
  for (uint32_t j = (uint32_t)lane; j < chunks * 32; j += 64) {
    const uint32_t u = j >> 3, t = (j >> 1) & 3u, par = j & 1u;
    uint32_t hw = 0u, lw = 0u;
    if (!zero && u < units) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float x = qg[u * 32 + 8 * t + 4 * par + b] * inv;
        const float r = rintf(x);
        const float rho = x - r;
        rr = fmaf(rho, rho, rr);
        const int qv = (int)r, h = (qv + 128) >> 8, l = qv - 256 * h;
        hw |= ((uint32_t)h & 0xFFu) << (8 * b);
        lw |= ((uint32_t)l & 0xFFu) << (8 * b);
      }
    }
    uint32_t* frag = out + (size_t)((u >> 2) * 2 + par) * 2 * 256 + (u & 3u) * 64 + t;
    frag[0] = hw;
    frag[256] = lw;
  }
  for (int o = 32; o > 0; o >>= 1) rr += __shfl_xor(rr, o);
  if (lane == 0) {
    const float e2 = zero ? 0.f : delta * fmaf(sqrtf(rr), 1.0005f, 1e-20f);
    const float round1 = fmaf(6e-6f * (float)(dimp + 8), q1, (float)dimp * 0x1p-138f);
    U42QConst c;
    c.dp = delta * 0x1p-9f;
    c.qsum305 = 30.5f * (qsum32 * 0.03125f);
    c.qsum32 = qsum32;
    c.q2 = q2;
    c.round1 = round1 + 60.0f * sqrtf((float)dimp) * e2 * (1.0f + 1e-5f);
    c.e2 = e2;
    c.delta = delta;
    c.flags = !present ? U42Q_ABSENT : marked ? U42Q_MARKED : 0u;
    qc[qi] = c;
  }
}

struct Scan42MfmaArgs {
  Scan42Args a;         // planes; query, tau, cand, count, survivors of the launch's first query; grid y = its groups of 16
  const uint32_t* qb;   // the launch's first group's fragments (u42_query_i16_kernel)
  const U42QConst* qc;  // the launch's first query's constants
  uint32_t nq;          // queries of the launch: the last group may be short
  uint32_t* surv_p;     // optional: [nq][n_rows], the bits of 2^-9 P^ of every survivor entry, other words untouched (tests)
};

constexpr uint32_t U42_MFMA_TRIGGER = 64;    // a list of this many entries is refined behind the tile that filled it
constexpr uint32_t U42_MFMA_LIST_CAP = 128;  // TRIGGER - 1 held between tiles + the 64 a tile can append

// the wave's ONE stage for the sixteen columns of its group: keys with their column, flushed 64 at a time.  A flush is one atomic
// instruction (a lane per column that has keys among the 64 adds that column's number to the column's counter) and one store
// instruction; capacity and overflow stay per column: the counter ends at the exact total, keys at base + rank >= cap are dropped.
struct U42Stage16 {
  u64* key;       // 128 keys of LDS, this wave's
  uint8_t* col;   // their columns
  uint32_t fill;  // keys staged (wave-uniform, < 64 between pushes)
  // cand, count: of the group's first query
  __device__ __forceinline__ void push(bool keep, u64 k, uint32_t c, u64* cand, uint32_t* count, uint32_t cap, int lane) {
    const u64 bal = __ballot(keep);
    if (!bal) return;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    if (keep) key[fill + rank] = k, col[fill + rank] = (uint8_t)c;
    fill += (uint32_t)__popcll(bal);
    if (fill >= 64) flush(64, cand, count, cap, lane);
  }
  __device__ __forceinline__ void finish(u64* cand, uint32_t* count, uint32_t cap, int lane) {
    if (fill) flush(fill, cand, count, cap, lane);
  }
  __device__ __forceinline__ void flush(uint32_t n, u64* cand, uint32_t* count, uint32_t cap, int lane) {
    u42_wave_sync();
    const uint32_t l = (uint32_t)lane;
    const bool on = l < n;
    const u64 k = on ? key[l] : 0ull;
    const uint32_t c = on ? (uint32_t)col[l] : U42_MFMA_QUERIES;  // (no column)
    const uint32_t rest = fill - n;                                // (< 64) moved to the front
    const u64 mk = l < rest ? key[n + l] : 0ull;
    const uint8_t mc = l < rest ? col[n + l] : (uint8_t)0;
    uint32_t rank = 0, cnt = 0, lead = 0;  // among the lanes of this lane's column: its rank, their number, the first of them
#pragma unroll
    for (uint32_t cc = 0; cc < U42_MFMA_QUERIES; ++cc) {
      const u64 b = __ballot(c == cc);
      if (c == cc) {
        rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        cnt = (uint32_t)__popcll(b);
        lead = (uint32_t)__builtin_ctzll(b);
      }
    }
    uint32_t base = 0;
    if (on && rank == 0) base = atomicAdd(count + c, cnt);
    base = (uint32_t)__shfl((int)base, (int)lead);
    if (on && base + rank < cap) cand[(size_t)c * cap + base + rank] = k;
    u42_wave_sync();
    if (l < rest) key[l] = mk, col[l] = mc;
    fill = rest;
    u42_wave_sync();
  }
};

// what the refine of one list entry reads, all of it addressed by the entry's row alone: the row's scale and its l record as
// six 16-byte loads (the record is 128-byte aligned and a whole line for units <= 15) plus a6
struct U42Gather {
  uint32_t row;
  float p4, s;
  u4v w[U42_MFMA_MAX_UNITS / 2];
  uint32_t a6;
};

// the loads of the refine of n (<= 64) list entries, lane = entry; idle lanes walk record 0 (always there)
__device__ __forceinline__ U42Gather u42_mfma_gather(const Scan42Args& a, const uint2* list, uint32_t n, int lane) {
  U42Gather g;
  const uint2 e = (uint32_t)lane < n ? list[lane] : make_uint2(0u, 0u);
  g.row = e.x;
  g.p4 = __uint_as_float(e.y);
  const uint32_t* rec = a.lrec + (size_t)e.x * a.lpitch;
  g.s = a.sa4[e.x].x;
#pragma unroll
  for (uint32_t i = 0; i < U42_MFMA_MAX_UNITS / 2; ++i) g.w[i] = *(const u4v*)(rec + 4 * i);
  g.a6 = rec[2 * a.units];
  return g;
}

// u42_refine's sums, bounds and key on gathered entries of query c of the group (the same operations in the same order), kept
// keys to the wave's stage
__device__ __forceinline__ void u42_mfma_finish(const Scan42MfmaArgs& m, uint32_t q0, uint32_t c, uint32_t n, const U42Gather& g,
                                                U42Stage16& st, int lane) {
  const Scan42Args& a = m.a;
  const uint32_t qi = q0 + c;
  const __attribute__((address_space(4))) U42QConst* kc = (const __attribute__((address_space(4))) U42QConst*)(m.qc + qi);
  const float thr = (kc->flags & U42Q_MARKED) ? -INFINITY : a.tau[qi];
  const float qsum32 = kc->qsum32, q2 = kc->q2, round1 = kc->round1;
  cfloat* q = (cfloat*)(a.query + (size_t)qi * a.qpitch);
  const bool active = (uint32_t)lane < n;
  const float p4 = active ? g.p4 : 0.f, s = active ? g.s : 0.f;
  f2v a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
#pragma unroll
  for (uint32_t u = 0; u < U42_MFMA_MAX_UNITS; ++u) {
    if (u < a.units) {  // (wave-uniform)
      cfloat* qu = q + u * 32;
#pragma unroll
      for (int gg = 0; gg < 2; ++gg) {
        const uint32_t w = g.w[u >> 1][2 * (u & 1) + gg];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f2v lo, hi;
          u42_rem4(w, j, lo, hi);
          const int i = 16 * gg + 4 * j;
          a0 = __builtin_elementwise_fma(lo, f2v{qu[i], qu[i + 1]}, a0);
          a1 = __builtin_elementwise_fma(hi, f2v{qu[i + 2], qu[i + 3]}, a1);
        }
      }
    }
  }
  const float a6 = __uint_as_float(g.a6);
  const float qq = (a0.x + a0.y) + (a1.x + a1.y);
  const float w = s * (fmaf(2048.0f, p4, 512.0f * qq) - qsum32);
  const float mm = fmaf(a6, q2, s * round1);
  const bool keep = active && !(w + mm < thr);
  st.push(keep, make_key((w == w) ? w + 0.0f : INFINITY, g.row), c, a.cand + (size_t)q0 * a.cap, a.count + q0, a.cap, lane);
}

// NCH chunks of four units: units in (4 NCH - 4, 4 NCH]
template <int NCH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_u42_mfma_kernel(Scan42MfmaArgs m) {
  static_assert(4 * NCH <= (int)U42_MFMA_MAX_UNITS, "the refine gathers six 16-byte loads per record");
  static_assert(U42_MFMA_TRIGGER == 64 && U42_MFMA_LIST_CAP >= U42_MFMA_TRIGGER - 1 + 64, "a refine takes 64 entries, a tile adds up to 64");
  __shared__ uint2 lists[4][U42_MFMA_QUERIES][U42_MFMA_LIST_CAP];
  __shared__ u64 stage_key[4][128];
  __shared__ uint8_t stage_col[4][128];
  __shared__ f2v sas[4][64];
  __shared__ uint32_t fills[4][U42_MFMA_QUERIES];
  const Scan42Args& a = m.a;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t col = (uint32_t)lane & 15u, kg = (uint32_t)lane >> 4;
  const uint32_t q0 = blockIdx.y * U42_MFMA_QUERIES;
  const bool present = q0 + col < m.nq;
  const U42QConst kc = m.qc[min(q0 + col, m.nq - 1)];
  const float thr = !present ? INFINITY : (kc.flags & U42Q_MARKED) ? -INFINITY : a.tau[q0 + col];
  i4v bf[NCH][2][2];
  {
    const i4v* src = (const i4v*)(m.qb + (size_t)blockIdx.y * (NCH * 4 * 256)) + lane;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int par = 0; par < 2; ++par)
#pragma unroll
        for (int hl = 0; hl < 2; ++hl) bf[c][par][hl] = src[((c * 2 + par) * 2 + hl) * 64];
  }
  if (lane < (int)U42_MFMA_QUERIES) fills[wave][lane] = 0u;
  U42Stage16 st = {stage_key[wave], stage_col[wave], 0u};
  uint32_t refined = 0;  // lane c < 16: entries of column c this wave has refined
  u42_wave_sync();
  const uint32_t tiles = (a.n_rows + 63) / 64;
  const size_t tile_dw = (size_t)a.units * 256;
  for (uint32_t tile = blockIdx.x * 4 + wave; tile < tiles; tile += gridDim.x * 4) {
    const uint32_t* p = a.hcodes + tile * tile_dw + kg * 256 + col * 4;
    const f2v sa = __builtin_nontemporal_load(a.sa4 + min(tile * 64 + (uint32_t)lane, a.n_rows - 1));
    u4v v[4][NCH];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if (c < NCH - 1 || 4 * c + kg < a.units) v[rb][c] = u42_load<true>(p + (size_t)c * 1024 + rb * 64);
        else v[rb][c] = u4v{0u, 0u, 0u, 0u};  // (a short last chunk: this lane group's unit is past the row)
      }
    u42_wave_sync();  // (the last tile's reads of sas are done)
    sas[wave][lane] = sa;
    u42_wave_sync();
    bool any = false;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      i4v dh = {0, 0, 0, 0}, dl = {0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const u4v lo = v[rb][c] & 0x0F0F0F0Fu, hi = (v[rb][c] >> 4) & 0x0F0F0F0Fu;
        dh = __builtin_amdgcn_mfma_i32_16x16x64_i8((i4v)lo, bf[c][0][0], dh, 0, 0, 0);
        dl = __builtin_amdgcn_mfma_i32_16x16x64_i8((i4v)lo, bf[c][0][1], dl, 0, 0, 0);
        dh = __builtin_amdgcn_mfma_i32_16x16x64_i8((i4v)hi, bf[c][1][0], dh, 0, 0, 0);
        dl = __builtin_amdgcn_mfma_i32_16x16x64_i8((i4v)hi, bf[c][1][1], dl, 0, 0, 0);
      }
      const uint32_t r0 = 16u * rb + 4u * kg;  // this lane's rows of the tile: r0 .. r0 + 3
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f2v s = sas[wave][r0 + i];
        const uint32_t row = tile * 64 + r0 + i;
        const float p4 = (float)(dh[i] * 256 + dl[i]) * kc.dp;  // = 2^-9 P^
        const float w = s.x * fmaf(2048.0f, p4, -kc.qsum305);
        const float mm = fmaf(s.y, kc.q2, s.x * kc.round1);
        const bool surv = present && row < a.n_rows && !(s.x < 0.f) && !(w + mm < thr);
        if (surv) {
          const uint32_t slot = atomicAdd(&fills[wave][col], 1u);
          lists[wave][col][slot] = make_uint2(row, __float_as_uint(p4));
          if (m.surv_p) m.surv_p[(size_t)(q0 + col) * a.n_rows + row] = __float_as_uint(p4);
        }
        any = any || surv;
      }
    }
    if (__ballot(any)) {
      u42_wave_sync();
      u64 due = __ballot(kg == 0 && fills[wave][col] >= U42_MFMA_TRIGGER);
      while (due) {  // refine the list's LAST 64 entries: what stays is in front already
        const uint32_t c = (uint32_t)__builtin_ctzll(due);
        due &= due - 1;
        const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)fills[wave][c]) - 64u;
        u42_wave_sync();
        if (lane == 0) fills[wave][c] = n;
        const U42Gather g = u42_mfma_gather(a, lists[wave][c] + n, 64u, lane);
        u42_wave_sync();  // (the entries are read before the next tile appends over them)
        if ((uint32_t)lane == c) refined += 64u;
        u42_mfma_finish(m, q0, c, 64u, g, st, lane);
      }
    }
  }
  // behind the last tile: what is left in the sixteen lists, the loads of the next list in flight while this one is finished
  u42_wave_sync();
  u64 due = __ballot(kg == 0 && fills[wave][col] > 0u);
  if (due) {
    uint32_t c = (uint32_t)__builtin_ctzll(due);
    due &= due - 1;
    uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)fills[wave][c]);
    U42Gather g = u42_mfma_gather(a, lists[wave][c], n, lane);
    while (due) {
      const uint32_t c1 = (uint32_t)__builtin_ctzll(due);
      due &= due - 1;
      const uint32_t n1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)fills[wave][c1]);
      const U42Gather g1 = u42_mfma_gather(a, lists[wave][c1], n1, lane);
      if ((uint32_t)lane == c) refined += n;
      u42_mfma_finish(m, q0, c, n, g, st, lane);
      g = g1, c = c1, n = n1;
    }
    if ((uint32_t)lane == c) refined += n;
    u42_mfma_finish(m, q0, c, n, g, st, lane);
  }
  st.finish(a.cand + (size_t)q0 * a.cap, a.count + q0, a.cap, lane);
  // (only present columns have entries, so every address is a query's of the launch)
  if (a.survivors && lane < (int)U42_MFMA_QUERIES && refined) atomicAdd(a.survivors + q0 + lane, refined);
}

typedef void (*scan42_mfma_fn)(Scan42MfmaArgs);
static scan42_mfma_fn pick_scan42_mfma(uint32_t units) { return u42_mfma_has_instance(units) ? scan_u42_mfma_kernel<3> : nullptr; }

// rows [r0, n) fp32 -> h plane, {s, a4} and l records, one wave per row, one lane per 16 elements (half a unit): the walk of
// rows_to_u6_kernel, so that a6 is its a bit for bit.  units = 32-element units (the pitch is a multiple of 32).
// (row r, its fp32 elements at p, by the whole wave.  Shared with the list form of kernels_update.h)
__device__ __forceinline__ void row_to_u42(const float* p, u64 r, uint32_t dim, uint32_t units, uint32_t* hcodes, f2v* sa4, uint32_t* lrec,
                                           uint32_t lpitch, int lane) {
  {
    const U6RowScale rs = u6_row_scale(p, dim, lane);
    float rr = 0.f, rr4 = 0.f;  // sums of squared residuals in units of s: against the six-bit code, against 4 h + 1.5
    uint32_t* hout = hcodes + ((size_t)(r >> 6) * units * 64 + (size_t)(r & 63)) * 4;
    uint32_t* lout = lrec + (size_t)r * lpitch;
    for (uint32_t u = lane; u < units * 2; u += 64) {
      uint32_t code[16];
      u6_unit_codes(p, u, dim, rs, code, rr);
      uint32_t hw[2] = {0u, 0u}, lw = 0u;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t c = u * 16 + i;
        const uint32_t h = code[i] >> 2, l = code[i] & 3u;
        hw[i >> 3] |= h << (8 * (i & 3) + 4 * ((i >> 2) & 1));
        lw |= l << (8 * (i & 3) + 2 * (i >> 2));
        if (c < dim && rs.quant) {
          const float rho4 = fmaf(-rs.s, 4.0f * (float)h - 30.5f, p[c]) * rs.inv;
          rr4 = fmaf(rho4, rho4, rr4);
        }
      }
      hout[(size_t)(u >> 1) * 256 + 2 * (u & 1)] = hw[0];
      hout[(size_t)(u >> 1) * 256 + 2 * (u & 1) + 1] = hw[1];
      lout[u] = lw;
    }
    for (int o = 32; o > 0; o >>= 1) {
      rr += __shfl_xor(rr, o);
      rr4 += __shfl_xor(rr4, o);
    }
    const f2v sa = u6_row_pair(rs, rr, dim);
    if (lane == 0) {
      sa4[r] = f2v{sa.x, u6_row_pair(rs, rr4, dim).y};
      lout[units * 2] = __float_as_uint(sa.y);
    }
  }
}

__global__ __launch_bounds__(256) void rows_to_u42_kernel(const float* rows, u64 r0, u64 n, uint32_t dim, uint32_t pitch,
                                                          uint32_t units, uint32_t* hcodes, f2v* sa4, uint32_t* lrec,
                                                          uint32_t lpitch) {
  const int lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (u64)gridDim.x * 4;
  for (u64 r = r0 + wave; r < n; r += nw) row_to_u42(rows + r * pitch, r, dim, units, hcodes, sa4, lrec, lpitch, lane);
}

// ---- host side ---------------------------------------------------------------------------------
// workgroups of a rows_to_u42_kernel launch over `rows` rows: four waves = four rows per workgroup at a time
static inline uint32_t rows_to_u42_grid(uint64_t rows) { return (uint32_t)std::min<uint64_t>((rows + 3) / 4, 65536); }

// units in flight per wave: the largest of 8, 6, 4 that divides the row's units, else the smallest of them that holds the row
// or 8 (13 units: 8 + 5); 6 x 16 bytes per lane are the 6 KiB per wave the u6 pass keeps in flight
static int u42_unit_chunk(uint32_t units) {
  if (!units) return 0;
  for (int uc = 8; uc >= 4; uc -= 2)
    if (units % (uint32_t)uc == 0) return uc;
  return units <= 4 ? 4 : units <= 6 ? 6 : 8;
}

typedef void (*scan42_fn)(Scan42Args);
// the instance for uc units in flight and qp (1, 2 or 4) queries per group
template <int QP>
static scan42_fn pick_scan42_qp(int uc) {
  switch (uc) {
    case 4: return scan_u42_kernel<4, QP>;
    case 6: return scan_u42_kernel<6, QP>;
    case 8: return scan_u42_kernel<8, QP>;
  }
  return nullptr;
}
static scan42_fn pick_scan42(int uc, int qp = 1) {
  switch (qp) {
    case 1: return pick_scan42_qp<1>(uc);
    case 2: return pick_scan42_qp<2>(uc);
    case 4: return pick_scan42_qp<4>(uc);
  }
  return nullptr;
}
