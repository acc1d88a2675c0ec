// kernels_scan6.h -- single queries over the u6 shadow copy: six-bit codes, a stored residual norm per row.
// Part of the single translation unit wdbx_hip.hip (included there, in order); not a standalone header.

// ------------------------------------------------------------------------------------------------
// SIX-BIT SELECTION scan for rounds of single queries.  The step is bound by the bytes a query reads, so the rows are kept
// once more as six-bit codes u = round(c / s) + 32 (k = u - 32 in [-31, 31]), s = max|c| / 31, with TWO floats per row: the
// scale s and  a >= |c - s k|_2,  the Euclidean norm of the row's ACTUAL quantisation residual, rounded up.  The scan forms
//   w = s * (sum u_i q_i - 32 sum q_i)  ~  s k.q      (query in full fp32)
// and Cauchy-Schwarz on the residual gives the rigorous bound
//   |w - c.q|  <=  m  =  a |q|_2 (1 + 1e-5)  +  6e-6 (dimp + 8) s |q|_1 (1 + 1e-5)
// First term: |(c - s k).q| <= |c - s k|_2 |q|_2 holds in exact arithmetic for whatever codes the quantiser chose; a carries
// the margin of its own computation (rows_to_u6_kernel), |q|_2 and |q|_1 that of theirs (u6_query_sums: relative 1e-5 covers
// gamma of a dimp-term fp32 sum up to dimp = 4096 elements with any order of summation, and the square root).  Second term:
// the fp32 roundings of this kernel's own arithmetic -- the sum of dimp products |u_i q_i| <= 63 |q_i| in any order
// (gamma_dimp * 63 |q|_1), the sum behind 32 sum q (gamma_dimp * 32 |q|_1), their difference and the product with s (three
// more roundings of a value of at most 95 |q|_1): (dimp + 8) * 2^-24 * 95 < 5.7e-6 (dimp + 8), taken as 6e-6.
// On dense rows a ~ s sqrt(d / 12) and the bound is about 1.4 x tighter than the L-infinity x L1 form of the u8 shadow, which
// is what makes six bits pay: 3.8 k candidates per query on the bench corpus at 10 M x 384 (an estimated 25 k on Gaussian
// rows, where the L-infinity x L1 form would keep 100 k).
//
// LAYOUT.  Tiles of 64 rows stored unit-major, a unit = 16 codes = 12 bytes:  [tile][unit][row 0..63][3 dwords].  Lane = row;
// one 12-byte load per lane and unit is 768 contiguous bytes per wave (six whole 128-byte lines, each covered once); the
// {s, a} pairs are 8 bytes per lane = four whole lines.  No lane-group sum and no query registers: the 16 query floats of a
// unit come through scalar loads (the query is read through the constant address space) and feed the fmas as scalar operands.
// Inside a unit, dword t byte b holds code 4 t + b in its low six bits and bits [2 t, 2 t + 1] of code 12 + b in its top two:
// one v_and per dword feeds four byte converts, and (d0 >> 6 & 0x03030303) | (d1 >> 4 & 0x0C0C0C0C) | (d2 >> 2 & 0x30303030)
// is a dword whose four bytes are codes 12 .. 15 -- 9 logic ops + 16 converts + 16 fmas per 16 elements (2.6 per element).
//   scan8_u6_sample_kernel (sampled 64-row tiles, QN queries of the round per wave: the extraction is shared): per tile the
//            maximum of the LOWER bounds w - m; the k-th largest of them, tau, is a lower bound of the true k-th best score.
//   scan8_u6_kernel (all rows): every row with !(w + m < tau) is appended to the candidate buffer through the wave's LDS stage.
// rescore_kernel then computes the candidates' exact fp32 scores (the same kernel as behind the u8 scan: bit-identical
// scores), u6_cut_kernel cuts the thousands of re-scored keys per query to the few that can be among the best k, merge_kernel
// ranks those.  Rows with an infinite element carry a NaN scale (never sampled, always candidates), rows with a NaN element
// a negative scale (skipped), as on the u8 shadow.  Inner product / cosine only.
// ------------------------------------------------------------------------------------------------
typedef uint32_t u3v __attribute__((ext_vector_type(3)));
typedef float f2v __attribute__((ext_vector_type(2)));
typedef const float __attribute__((address_space(4))) cfloat;  // uniform addresses: scalar loads

struct Scan6Args {
  const uint32_t* codes;  // [tiles][units][64][3]
  const f2v* sa;          // [rows] {s, a}
  const float* query;     // fp32 [units * 16] per query, pitch qpitch floats (zero padded)
  uint32_t n_rows, units, qpitch;
  u64* halfmax;           // sample: one key per sampled tile and query
  uint32_t num_tiles, tile_stride;  // sample: 256-row tiles = 4 groups of 64 rows, every tile_stride-th (as scan8_kernel's)
  uint32_t nq;            // sample: queries of the launch
  const float* tau;       // full pass
  u64* cand;
  uint32_t* count;        // candidate counters (reset by the sample launch)
  uint32_t* count2;       // the cut's counters (reset by the sample launch)
  uint32_t cap;
};

// sum q, |q|_1 and |q|_2 of one query over its units * 16 floats, the latter two rounded up past their own fp32 error; the
// same arithmetic in every wave of both kernels
__device__ __forceinline__ void u6_query_sums(const float* q, uint32_t n, int lane, float& qsum32, float& q1, float& q2) {
  float ss = 0.f, s1 = 0.f, s2 = 0.f;
  for (uint32_t i = (uint32_t)lane; i < n; i += 64) {
    const float v = q[i];
    ss += v;
    s1 += fabsf(v);
    s2 = fmaf(v, v, s2);
  }
  for (int o = 32; o > 0; o >>= 1) {
    ss += __shfl_xor(ss, o);
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  qsum32 = 32.0f * ss;
  q1 = s1 * (1.0f + 1e-5f);
  q2 = sqrtf(s2) * (1.0f + 1e-5f) + 1e-37f;  // (squares that underflow: |q|_2 of such a query is below 1e-17 either way)
}

// the 12 bytes of one lane and unit (dword aligned: three adjacent loads, merged into one global_load_dwordx3)
template <bool NT>
__device__ __forceinline__ u3v u6_load(const uint32_t* p) {
  if constexpr (NT) return u3v{__builtin_nontemporal_load(p), __builtin_nontemporal_load(p + 1), __builtin_nontemporal_load(p + 2)};
  return u3v{p[0], p[1], p[2]};
}

// the low-six-bit bytes of one dword as four floats
__device__ __forceinline__ void u6_cvt4(uint32_t w, float (&f)[4]) {
  asm volatile("" : "+v"(w));  // (the masked dword stays ONE value: without this the mask is folded into a shift + and per byte)
  f[0] = (float)(w & 0xFFu);  // (v_cvt_f32_ubyte0..3)
  f[1] = (float)((w >> 8) & 0xFFu);
  f[2] = (float)((w >> 16) & 0xFFu);
  f[3] = (float)(w >> 24);
}

// the 16 codes of a unit as floats (codes 12 .. 15 from the bytes' top two bits)
__device__ __forceinline__ void u6_unpack(u3v d, float (&f)[16]) {
  float t[4];
  u6_cvt4(d.x & 0x3F3F3F3Fu, t);
  f[0] = t[0], f[1] = t[1], f[2] = t[2], f[3] = t[3];
  u6_cvt4(d.y & 0x3F3F3F3Fu, t);
  f[4] = t[0], f[5] = t[1], f[6] = t[2], f[7] = t[3];
  u6_cvt4(d.z & 0x3F3F3F3Fu, t);
  f[8] = t[0], f[9] = t[1], f[10] = t[2], f[11] = t[3];
  const uint32_t hi = ((d.x >> 6) & 0x03030303u) | ((d.y >> 4) & 0x0C0C0C0Cu) | ((d.z >> 2) & 0x30303030u);
  u6_cvt4(hi, t);
  f[12] = t[0], f[13] = t[1], f[14] = t[2], f[15] = t[3];
}

// full pass: UC units in flight per wave (UC divides the row's units), one 64-row tile per wave at a time
template <int UC>
__global__ __launch_bounds__(256) void scan8_u6_kernel(Scan6Args a) {
  __shared__ u64 stage6[4][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* qg = a.query + (size_t)blockIdx.y * a.qpitch;
  cfloat* q = (cfloat*)qg;
  a.tau += blockIdx.y;
  a.cand += (size_t)blockIdx.y * a.cap;
  a.count += blockIdx.y;
  float qsum32, q1, q2;
  u6_query_sums(qg, a.units * 16, lane, qsum32, q1, q2);
  const float thr = a.tau[0];
  const float round1 = 6e-6f * (float)(a.units * 16 + 8) * q1;
  WaveStage st = {stage6[wave], 0u};
  const uint32_t tiles = (a.n_rows + 63) / 64;
  const size_t tile_dw = (size_t)a.units * 192;
  for (uint32_t tile = blockIdx.x * 4 + wave; tile < tiles; tile += gridDim.x * 4) {
    const uint32_t row = tile * 64 + (uint32_t)lane;
    const uint32_t* p = a.codes + tile * tile_dw + lane * 3;
    const f2v sa = __builtin_nontemporal_load(a.sa + min(row, a.n_rows - 1));
    f2v a0 = {0.f, 0.f}, a1 = {0.f, 0.f};  // (even, odd) elements: v_pk_fma_f32 with the query pair as its scalar operand
    for (uint32_t u0 = 0; u0 < a.units; u0 += UC) {
      u3v v[UC];
#pragma unroll
      for (int u = 0; u < UC; ++u) v[u] = u6_load<true>(p + (size_t)(u0 + u) * 192);
#pragma unroll
      for (int u = 0; u < UC; ++u) {
        float f[16];
        u6_unpack(v[u], f);
        cfloat* qu = q + (u0 + u) * 16;
#pragma unroll
        for (int i = 0; i < 16; i += 4) {
          a0 = __builtin_elementwise_fma(f2v{f[i], f[i + 1]}, f2v{qu[i], qu[i + 1]}, a0);
          a1 = __builtin_elementwise_fma(f2v{f[i + 2], f[i + 3]}, f2v{qu[i + 2], qu[i + 3]}, a1);
        }
      }
    }
    const float w = sa.x * (((a0.x + a0.y) + (a1.x + a1.y)) - qsum32);
    const float m = fmaf(sa.y, q2, sa.x * round1);
    // !(w + m < thr): also true for a NaN bound, so rows with an infinite element always go to the exact pass; a negative
    // scale marks a row with a NaN element (never a result)
    const bool keep = row < a.n_rows && !(sa.x < 0.f) && !(w + m < thr);
    st.push(keep, make_key((w == w) ? w + 0.0f : INFINITY, row), a.cand, a.count, a.cap, lane);
  }
  st.finish(a.cand, a.count, a.cap, lane);
}

// sample pass: QN queries of the round per wave (blockIdx.y = query group); a sampled tile is loaded and unpacked once for them
template <int UC>
__global__ __launch_bounds__(256) void scan8_u6_sample_kernel(Scan6Args a) {
  constexpr int QN = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t qbase = blockIdx.y * QN;
  if (blockIdx.x == 0 && threadIdx.x < QN && qbase + threadIdx.x < a.nq) {
    a.count[qbase + threadIdx.x] = 0;
    a.count2[qbase + threadIdx.x] = 0;
  }
  cfloat* q[QN];
  float qsum32[QN], q1[QN], q2[QN];
#pragma unroll
  for (int t = 0; t < QN; ++t) {
    const float* qg = a.query + (size_t)min(qbase + t, a.nq - 1) * a.qpitch;
    q[t] = (cfloat*)qg;
    u6_query_sums(qg, a.units * 16, lane, qsum32[t], q1[t], q2[t]);
  }
  const float round0 = 6e-6f * (float)(a.units * 16 + 8);
  const uint32_t ngroups = a.num_tiles * 4;
  const size_t tile_dw = (size_t)a.units * 192;
  for (uint32_t grp = blockIdx.x * 4 + wave; grp < ngroups; grp += gridDim.x * 4) {
    const uint32_t row0 = (grp >> 2) * a.tile_stride * 256 + (grp & 3) * 64;
    const uint32_t row = row0 + (uint32_t)lane;
    const bool live = row0 < a.n_rows;  // (wave-uniform; the last sampled 256-row tile may end early)
    const uint32_t* p = a.codes + (live ? row0 / 64 : 0u) * tile_dw + lane * 3;
    const f2v sa = a.sa[min(row, a.n_rows - 1)];
    f2v acc[QN];
#pragma unroll
    for (int t = 0; t < QN; ++t) acc[t] = f2v{0.f, 0.f};
    for (uint32_t u0 = 0; u0 < a.units; u0 += UC) {
      u3v v[UC];
#pragma unroll
      for (int u = 0; u < UC; ++u) v[u] = u6_load<false>(p + (size_t)(u0 + u) * 192);
#pragma unroll
      for (int u = 0; u < UC; ++u) {
        float f[16];
        u6_unpack(v[u], f);
#pragma unroll
        for (int t = 0; t < QN; ++t) {
          cfloat* qu = q[t] + (u0 + u) * 16;
#pragma unroll
          for (int i = 0; i < 16; i += 2) acc[t] = __builtin_elementwise_fma(f2v{f[i], f[i + 1]}, f2v{qu[i], qu[i + 1]}, acc[t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < QN; ++t) {
      const float w = sa.x * ((acc[t].x + acc[t].y) - qsum32[t]);
      const float m = fmaf(sa.y, q2[t], sa.x * (round0 * q1[t]));
      const float lo = w - m;
      // (NaN or negative scale: the row cannot vouch for the threshold)
      float b = (live && row < a.n_rows && sa.x >= 0.f && lo == lo) ? lo : -INFINITY;
      for (int o = 32; o > 0; o >>= 1) b = fmaxf(b, __shfl_xor(b, o));
      if (lane == 0 && qbase + t < a.nq)
        a.halfmax[(size_t)(qbase + t) * ngroups + grp] = (b == -INFINITY) ? 0ull : make_key(b + 0.0f, grp);
    }
  }
}

// ---- the six-bit quantiser, shared by rows_to_u6_kernel and the split planes of kernels_scan42.h ----
// a row's scale, by the whole wave
struct U6RowScale {
  float mx, s, inv;
  bool finite, has_nan, vanishing, quant;
};
__device__ __forceinline__ U6RowScale u6_row_scale(const float* p, uint32_t dim, int lane) {
  U6RowScale rs;
  float mx = 0.f;
  bool finite = true, has_nan = false;
  for (uint32_t c = lane; c < dim; c += 64) {
    const float v = p[c];
    finite = finite && (fabsf(v) <= 3.4028235e38f);
    has_nan = has_nan || (v != v);
    mx = fmaxf(mx, fabsf(v));
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  rs.mx = mx;
  rs.finite = __all(finite);
  rs.has_nan = __any(has_nan);
  // rows of vanishing magnitude (31 / max would overflow): every code is 32, the scale 0 (w = 0 exactly) and
  // a = max|c| (sqrt(dim) + 1) >= |c|_2 covers the whole (negligible) score
  rs.vanishing = mx < 1.2e-30f;
  rs.quant = rs.finite && !rs.vanishing;
  rs.s = rs.quant ? mx / 31.0f : 0.f;
  rs.inv = rs.quant ? 31.0f / mx : 0.f;
  return rs;
}

// the 16 codes of elements [16 u, 16 u + 16) of the row; rr gathers the squared residuals in units of s
__device__ __forceinline__ void u6_unit_codes(const float* p, uint32_t u, uint32_t dim, const U6RowScale& rs, uint32_t (&code)[16],
                                              float& rr) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t c = u * 16 + i;
    const float x = (c < dim && rs.quant) ? p[c] : 0.f;
    const float k = fminf(fmaxf(rintf(x * rs.inv), -31.f), 31.f);
    const float rho = fmaf(-rs.s, k, x) * rs.inv;  // (c - s k) / s: one rounding in the residual, one in the quotient
    rr = fmaf(rho, rho, rr);
    code[i] = (uint32_t)((int)k + 32);
  }
}

// {s, a} of the row from the wave's sum of squared residuals (NaN / inf rows: the conventions of the header comment).
// a, rounded up: 5e-4 relative covers the roundings of the residuals (2^-24 each), of their quotients by s (s * inv = 1
// within 3 * 2^-24), of the sum of dimp squares in any order (gamma_dimp <= 2.5e-4 up to 4096 elements, halved by the root)
// and of the root and the product; 1e-4 s absolute covers residuals and squares that underflow
__device__ __forceinline__ f2v u6_row_pair(const U6RowScale& rs, float rr, uint32_t dim) {
  const float a = rs.quant ? rs.s * fmaf(sqrtf(rr), 1.0005f, 1e-4f) : rs.vanishing ? rs.mx * (sqrtf((float)dim) + 1.0f) : 0.f;
  return rs.has_nan ? f2v{-1.0f, 0.f} : !rs.finite ? f2v{NAN, 0.f} : f2v{rs.s, a};
}

// row r (its fp32 elements at p) -> its codes of the u6 shadow and its {s, a}, by the whole wave, one lane per unit of 16
// elements.  Shared with the list form of kernels_update.h
__device__ __forceinline__ void row_to_u6(const float* p, u64 r, uint32_t dim, uint32_t units, uint32_t* codes, f2v* sa, int lane) {
  {
    const U6RowScale rs = u6_row_scale(p, dim, lane);
    float rr = 0.f;  // sum of squared residuals in units of s
    uint32_t* out = codes + ((size_t)(r >> 6) * units * 64 + (size_t)(r & 63)) * 3;
    for (uint32_t u = lane; u < units; u += 64) {
      uint32_t code[16];
      u6_unit_codes(p, u, dim, rs, code, rr);
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) w |= (code[4 * t + b] | (((code[12 + b] >> (2 * t)) & 3u) << 6)) << (8 * b);
        out[(size_t)u * 192 + t] = w;
      }
    }
    for (int o = 32; o > 0; o >>= 1) rr += __shfl_xor(rr, o);
    const f2v pair = u6_row_pair(rs, rr, dim);
    if (lane == 0) sa[r] = pair;
  }
}

// rows [r0, n) fp32 -> u6 shadow + {s, a} per row, one wave per row
__global__ __launch_bounds__(256) void rows_to_u6_kernel(const float* rows, u64 r0, u64 n, uint32_t dim, uint32_t pitch,
                                                         uint32_t units, uint32_t* codes, f2v* sa) {
  const int lane = threadIdx.x & 63;
  const u64 wave = (u64)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (u64)gridDim.x * 4;
  for (u64 r = r0 + wave; r < n; r += nw) row_to_u6(rows + r * pitch, r, dim, units, codes, sa, lane);
}

// ------------------------------------------------------------------------------------------------
// The cut behind the re-scoring: merge_kernel is built for about a thousand keys per query, the u6 scan leaves tens of
// thousands.  Workgroup (x, q) takes segment x of query q's re-scored keys (U6_CUT_SEG keys at most), finds a threshold at or
// below the segment's k-th largest score (block_kth_threshold: short of it by less than 2^-15 relative; none when the
// segment holds fewer than k keys) and appends every key that reaches it to the query's short list.  A key among the best k
// of all segments is among the best k of its own, so the short list holds the query's best k; merge_kernel ranks it.
// count2[q] ends above cap2 -- "repair this query", for merge_kernel's over_out and the conditional repair launches -- when the
// short list overflowed (thousands of ties) or the candidate buffer in front of it had (count[q] > cap).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t U6_CUT_SEG = KTH_R * 1024;
__global__ __launch_bounds__(1024) void u6_cut_kernel(const u64* cand, const uint32_t* count, uint32_t cap, int k, u64* out,
                                                      uint32_t* count2, uint32_t cap2) {
  __shared__ uint32_t s_k[KTH_SCRATCH];
  if (threadIdx.x < KTH_SCRATCH) s_k[threadIdx.x] = 0;
  const uint32_t q = blockIdx.y, total = count[q], have = min(total, cap);
  const uint32_t lo = blockIdx.x * U6_CUT_SEG;
  if (blockIdx.x == 0 && threadIdx.x == 0 && total > cap) atomicAdd(count2 + q, cap2 + 1u);
  if (lo >= have) return;  // (block-uniform)
  const uint32_t n = min(have - lo, U6_CUT_SEG);
  const u64* in = cand + (size_t)q * cap + lo;
  u64 key[KTH_R];
  uint32_t v[KTH_R];
#pragma unroll
  for (int r = 0; r < KTH_R; ++r) {
    const uint32_t i = (uint32_t)r * 1024u + threadIdx.x;
    key[r] = i < n ? in[i] : 0ull;
    v[r] = (uint32_t)(key[r] >> 32);
  }
  __syncthreads();
  const uint32_t thr = max(block_kth_threshold<KTH_R>(v, (uint32_t)k, s_k), 1u);  // (0: fewer than k keys -- all of them)
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < KTH_R; ++r) wave_append(v[r] >= thr, key[r], out + (size_t)q * cap2, count2 + q, cap2, lane);
}

// workgroups of a rows_to_u6_kernel launch over `rows` rows: four waves = four rows per workgroup at a time
static inline uint32_t rows_to_u6_grid(uint64_t rows) { return (uint32_t)std::min<uint64_t>((rows + 3) / 4, 65536); }

// ---- host side: the instances of the scans above and which one serves a row ----------------------
// units in flight per wave = the largest of 8 .. 4 that divides the row's units (24 -> 8, 25 -> 5, 6 -> 6); 0 = none
static int u6_unit_chunk(uint32_t units) {
  for (int uc = 8; uc >= 4; --uc)
    if (units % (uint32_t)uc == 0) return uc;
  return 0;
}

typedef void (*scan6_fn)(Scan6Args);
static scan6_fn pick_scan6(int uc, bool sample) {
  switch (uc) {
    case 4: return sample ? scan8_u6_sample_kernel<4> : scan8_u6_kernel<4>;
    case 5: return sample ? scan8_u6_sample_kernel<5> : scan8_u6_kernel<5>;
    case 6: return sample ? scan8_u6_sample_kernel<6> : scan8_u6_kernel<6>;
    case 7: return sample ? scan8_u6_sample_kernel<7> : scan8_u6_kernel<7>;
    case 8: return sample ? scan8_u6_sample_kernel<8> : scan8_u6_kernel<8>;
  }
  return nullptr;
}
