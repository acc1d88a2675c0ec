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

// rows [r0, n) fp32 -> h plane, {s, a4} and l records, one wave per row, one lane per 16 elements (half a unit): the walk of
// rows_to_u6_kernel, so that a6 is its a bit for bit.  units = 32-element units (the pitch is a multiple of 32).
__global__ __launch_bounds__(256) void rows_to_u42_kernel(const float* rows, u64 r0, u64 n, uint32_t dim, uint32_t pitch,
                                                          uint32_t units, uint32_t* hcodes, f2v* sa4, uint32_t* lrec,
                                                          uint32_t lpitch) {
  const int lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (u64)gridDim.x * 4;
  for (u64 r = r0 + wave; r < n; r += nw) {
    const float* p = rows + r * pitch;
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
