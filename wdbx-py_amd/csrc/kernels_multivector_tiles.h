// kernels_multivector_tiles.h -- the matrix-core scoring route of wdbx_index_search_multivector (metric 0): one read of a stored
// row for up to 128 query vectors.
//   multivector_norms_kernel   the squared norm of every vector of the call, next to the query staging
//   label_keys_tile_kernel     fills the keys[vector][item] array label_keys_kernel (kernels_labels.h) fills, bit for bit: a fp32
//                              tile pass on v_mfma_f32_32x32x2_f32 over a span's gathered rows finds each (vector, item)'s winner
//                              row, a rigorous margin says whether it is exact_score's winner too, and the resolve -- in the same
//                              launch, while the span's rows are in cache -- scores with exact_score's own arithmetic: the
//                              winner alone (certain) or every eligible row of the item (ambiguous)
// Plan, LDS and grid: host_multivector_tiles.h.  The inequality behind "certain": DESIGN.md sections 4.20 and 4.12b.
// Part of the single translation unit wdbx_hip.hip (included there, behind kernels_multivector.h); not a standalone header.

// one wave per vector: fma chain over the lane's columns, then the tree (any fp32 order within gamma of the norm serves the bound)
ASSIGN_KERNEL __launch_bounds__(256) void multivector_norms_kernel(const float* vectors, float* vnorm, uint32_t pitch, uint32_t n) {
  const int lane = threadIdx.x & 63;
  const uint32_t v = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (v >= n) return;
  const float* p = vectors + (size_t)v * pitch;
  float s = 0.f;
  for (uint32_t c = lane; c < pitch; c += 64) s = fmaf(p[c], p[c], s);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) vnorm[v] = s;
}

struct LabelKeysTileArgs {
  LabelKeysArgs k;     // rows, the round's vectors, the label order, the mask and the keys, as label_keys_kernel reads them
  const float* cn;     // squared norm of every stored row (NaN: removed, or a NaN element)
  const float* vnorm;  // [k.nq] squared norms of the round's vectors
  u64* ambiguous;      // += the (vector, item) pairs the margin did not decide
  float gamma, under;  // host_assign.h: assign_bound
};

// Grid: x = workgroups along the spans (wave w of the grid takes spans w, w + W, ..., as label_keys_kernel), y = vector blocks
// of 32 VT vectors.  Workgroup = 4 waves; a wave owns one span at a time: its 64 gathered rows are the M operand (two 32-row
// tiles), the block's vectors the N operand, so in the 32x32 C layout a VECTOR is one lane's column (lane & 31 of tile vt) and
// the span's 64 scores against it lie along that lane's 2 * 16 accumulator registers, position
//   m = 32 rt + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)      (register r of row tile rt),
// the lane ^ 32 partner holding the other half of every 8 positions.  Rows and vectors are staged K-chunk by K-chunk (32 floats,
// rows of 36) through two LDS buffers, the loader one chunk ahead of the matrix ops across spans; the vector chunks are the
// workgroup's (hence one barrier per chunk, and waves without a span of their own in the last trip walk the last span again
// and store nothing), the row chunks each wave's own.  LDS does not depend on the row length.
// After the last chunk the wave folds and resolves item by item (item boundaries, eligibility and the largest row norm R of
// the span are wave-uniform: ballots over one lane per position):
//   fold     (best, its position, second best) over the lane's registers of the item's eligible positions, in ascending
//            position, then ONE lane ^ 32 exchange per item and vector tile
//   certain  <=> everything finite and best - second > 4 (gamma R |c| + under): exact_score's maximum over the item is then
//            the tile winner's, uniquely
//   resolve  vector by vector (wave-uniform, the lane's word read with readlane): the winner row alone, G pairs' loads in
//            flight, or -- ambiguous -- every eligible row of the item, through exact_score_block<., 1, NI>; the key is
//            row_key's, the maximum as label_keys_kernel takes it.  The lane that owns the vector keeps it and stores the
//            item's key with a plain store: one writer per key.
template <int VT, int NI>
ASSIGN_KERNEL __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void label_keys_tile_kernel(LabelKeysTileArgs t) {
  constexpr int METRIC = WDBX_METRIC_COSINE;
  constexpr int BK = MVT_BK, QPC = BK / 4, LD = MVT_LD, S = BK / 8;
  constexpr int SP = MVT_SPAN, VB = 32 * VT;
  constexpr int NA = SP * QPC / 64;  // row quads a lane stages per chunk: QPC lanes per row, 64 / QPC rows per pass
  constexpr int RPP = 64 / QPC;
  constexpr int NR = row_block_nr(NI);
  // certain pairs resolved together: what their rows' and vectors' quads leave of the registers next to the accumulators
  constexpr int G = NI == 0 ? 4 : (VT == 4 ? 8 : 16) / NI;
  constexpr int AMBIGUOUS = 255;
  static_assert(QPC == 8 && 256 / QPC == 32, "a pass of the 256 threads stages one 32-vector tile");
  extern __shared__ float lds_f[];
  __shared__ u64 amb_s[MVT_WAVES];
  float* Rs = lds_f;                         // [2][4 waves][SP][LD] gathered rows
  float* Vs = Rs + 2 * MVT_WAVES * SP * LD;  // [2][VB][LD] vectors
  const LabelKeysArgs& a = t.k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const uint32_t j = (uint32_t)lane;
  const uint32_t pitch4 = a.pitch4, kchunks = (pitch4 + QPC - 1) / QPC;
  const uint32_t v0 = blockIdx.y * VB;
  const uint32_t nvb = min((uint32_t)VB, a.nq - v0);  // vectors of this block
  const uint32_t W = gridDim.x * MVT_WAVES, base0 = blockIdx.x * MVT_WAVES;
  if (base0 >= a.n_spans) return;  // (the whole workgroup)
  const uint32_t trips = (a.n_spans - base0 + W - 1) / W;
  const uint32_t srow = (uint32_t)lane / QPC, squad = (uint32_t)lane % QPC;  // (tid % QPC is the same quad)

  // loader: one chunk of (trip's span, the vectors) into registers, later into the other LDS buffer
  uint32_t ld_trip = 0, ld_kc = 0;
  uint32_t ld_row[NA];
  auto span_rows = [&]() ASSIGN_INLINE {
    const uint32_t span = min(base0 + ld_trip * W + (uint32_t)wave, a.n_spans - 1);
    const uint32_t p0 = span * SP, p1 = min(p0 + SP, a.n);
#pragma unroll
    for (int i = 0; i < NA; ++i) ld_row[i] = a.order[min(p0 + srow + RPP * i, p1 - 1)];  // (past the span's end: its last row again, never eligible)
  };
  f4 sr[NA], sv[VT];
  auto gload = [&]() ASSIGN_INLINE {
    const uint32_t kq = ld_kc * QPC + squad;
    const bool in = kq < pitch4;  // (K tail: quads past the row end re-read its last quad and count as zero)
    const uint32_t o = min(kq, pitch4 - 1);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const f4 v = a.rows[(size_t)ld_row[i] * pitch4 + o];
      sr[i] = in ? v : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < VT; ++i) {
      // (past the block's end: the round's last vector again, never stored)
      const f4 v = a.queries[(size_t)min(v0 + 32u * i + (uint32_t)tid / QPC, a.nq - 1) * pitch4 + o];
      sv[i] = in ? v : f4{0.f, 0.f, 0.f, 0.f};
    }
    if (++ld_kc == kchunks) {
      ld_kc = 0;
      if (ld_trip + 1 < trips) {  // (past the last trip the loader re-reads it: valid memory, never consumed)
        ++ld_trip;
        span_rows();
      }
    }
  };
  auto lstore = [&](int buf) ASSIGN_INLINE {
#pragma unroll
    for (int i = 0; i < NA; ++i) *(f4*)&Rs[((buf * MVT_WAVES + wave) * SP + srow + RPP * i) * LD + squad * 4] = sr[i];
#pragma unroll
    for (int i = 0; i < VT; ++i) *(f4*)&Vs[(buf * VB + 32 * i + tid / QPC) * LD + squad * 4] = sv[i];
  };
  // exact_score's score of one stored row against one vector of the block, wave-uniform
  auto exact_one = [&](uint32_t row, uint32_t vec) ASSIGN_INLINE {
    const f4* cp = a.rows + (size_t)row * pitch4;
    const f4* const qp[1] = {a.queries + (size_t)vec * pitch4};
    f4 c[NR], q[1][NR];
#pragma unroll
    for (int n = 0; n < NR; ++n) {
      c[n] = q[0][n] = f4{0.f, 0.f, 0.f, 0.f};
      if (NI > 0 && j + (uint32_t)n * 64 < pitch4) {
        c[n] = cp[j + (uint32_t)n * 64];
        q[0][n] = qp[0][j + (uint32_t)n * 64];
      }
    }
    float s[1];
    exact_score_block<METRIC, 1, NI>(c, cp, q, qp, pitch4, j, s);
    return row_key(s[0], row);
  };

  span_rows();
  gload();
  lstore(0);
  __syncthreads();
  const float up = 1.0f + t.gamma;
  float nc[VT];
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) nc[vt] = sqrtf(t.vnorm[min(v0 + 32u * vt + (uint32_t)l31, a.nq - 1)] + t.under) * up;
  uint32_t it = 0;  // running chunk counter (LDS buffer = it & 1)
  u64 amb = 0;      // (wave-uniform)
  for (uint32_t trip = 0; trip < trips; ++trip) {
    const uint32_t span = base0 + trip * W + (uint32_t)wave;
    f16v acc[2][VT];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int vt = 0; vt < VT; ++vt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rt][vt][r] = 0.f;
    for (uint32_t kc = 0; kc < kchunks; ++kc, ++it) {
      const int buf = it & 1;
      gload();  // the next chunk's global loads, in flight under this chunk's matrix ops
#pragma unroll 2
      for (int s = 0; s < S; ++s) {
        f4 rf[2], cf[VT];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) rf[rt] = *(const f4*)&Rs[((buf * MVT_WAVES + wave) * SP + rt * 32 + l31) * LD + (2 * s + lh) * 4];
#pragma unroll
        for (int vt = 0; vt < VT; ++vt) cf[vt] = *(const f4*)&Vs[(buf * VB + vt * 32 + l31) * LD + (2 * s + lh) * 4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int vt = 0; vt < VT; ++vt) acc[rt][vt] = __builtin_amdgcn_mfma_f32_32x32x2f32(rf[rt][e], cf[vt][e], acc[rt][vt], 0, 0, 0);
      }
      lstore(buf ^ 1);
      __syncthreads();
    }
    if (span >= a.n_spans) continue;  // (a wave without a span in the last trip; it has met every barrier)

    // ---- the span: one lane per position ----
    const uint32_t p0 = span * SP, cnt = min((uint32_t)SP, a.n - p0);
    const uint32_t mpos = p0 + min(j, cnt - 1);
    const uint32_t myrow = a.order[mpos], mylab = a.dense[mpos];
    const uint32_t prevlab = (uint32_t)__shfl_up((int)mylab, 1);
    const u64 bmask = __ballot(j < cnt && (lane == 0 || mylab != prevlab));  // the items' first positions
    const float rn2 = t.cn[myrow];
    const bool elig = j < cnt && row_allowed(a.mask, myrow) && rn2 == rn2;  // (a NaN norm: every score of the row is NaN)
    const u64 emask = __ballot(elig);
    float R2 = elig ? rn2 : 0.f;
    for (int o = 32; o > 0; o >>= 1) R2 = fmaxf(R2, __shfl_xor(R2, o));
    const float nr = sqrtf(R2 + t.under) * up;  // norms rounded up, as assign_tile_kernel's
    float margin[VT];
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) margin[vt] = 4.0f * (t.gamma * nr * nc[vt] + t.under);
    uint32_t item = a.span_item0[span];
    for (u64 rest = bmask; rest; ++item) {
      const int s0 = __builtin_ctzll(rest);
      rest &= rest - 1;
      const int s1 = rest ? __builtin_ctzll(rest) : (int)cnt;  // the item: positions [s0, s1)
      const u64 imask = emask & (~0ull << s0) & (s1 >= 64 ? ~0ull : ((1ull << s1) - 1));
      u64 out[VT];
#pragma unroll
      for (int vt = 0; vt < VT; ++vt) out[vt] = 0;
      if (imask) {
        // ---- fold ----
        float best[VT], second[VT];
        int bpos[VT];
        bool bad[VT];
#pragma unroll
        for (int vt = 0; vt < VT; ++vt) best[vt] = second[vt] = -INFINITY, bpos[vt] = 64, bad[vt] = false;
#pragma unroll
        for (int blk = 0; blk < 8; ++blk) {
          if (blk * 8 >= s1 || blk * 8 + 8 <= s0) continue;  // (wave-uniform)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int m = blk * 8 + 4 * lh + i;
            const bool ok = (imask >> m) & 1;
#pragma unroll
            for (int vt = 0; vt < VT; ++vt) {
              const float v = acc[blk >> 2][vt][(blk & 3) * 4 + i];
              if (ok) {
                bad[vt] |= v != v;
                if (v > best[vt]) {
                  second[vt] = best[vt];
                  best[vt] = v;
                  bpos[vt] = m;
                } else {
                  second[vt] = fmaxf(second[vt], v);
                }
              }
            }
          }
        }
        int res[VT];  // the winner's position, or AMBIGUOUS
#pragma unroll
        for (int vt = 0; vt < VT; ++vt) {
          const float ob = __shfl_xor(best[vt], 32), os = __shfl_xor(second[vt], 32);
          const int op = __shfl_xor(bpos[vt], 32);
          const bool obad = __shfl_xor((int)bad[vt], 32);
          const bool take = ob > best[vt] || (ob == best[vt] && op < bpos[vt]);
          second[vt] = fmaxf(fmaxf(second[vt], os), take ? best[vt] : ob);
          if (take) best[vt] = ob, bpos[vt] = op;
          // (an infinite or NaN margin, an infinite best, a NaN among the item's tile scores: not certain)
          const bool certain = !(bad[vt] || obad) && fabsf(best[vt]) < INFINITY && best[vt] - second[vt] > margin[vt];
          res[vt] = certain ? bpos[vt] : AMBIGUOUS;
        }
        // ---- resolve ----
        const int first = __builtin_ctzll(imask);
#pragma unroll
        for (int vt = 0; vt < VT; ++vt) {
          const int nv = min(32, (int)nvb - 32 * vt);  // (wave-uniform; the last block may be short)
          if (nv <= 0) continue;
          amb += (u64)__popcll(__ballot(lh == 0 && l31 < nv && res[vt] == AMBIGUOUS));
          for (int b0 = 0; b0 < nv; b0 += G) {
            int bg[G], pg[G];
            uint32_t rowg[G];
            const f4* cp[G];
            const f4* qp[G][1];
            f4 c[G][NR], q[G][1][NR];
#pragma unroll
            for (int g = 0; g < G; ++g) {
              bg[g] = min(b0 + g, nv - 1);  // (past the end: the last vector again, the same key to the same lane)
              pg[g] = __builtin_amdgcn_readlane(res[vt], bg[g]);
              // (an ambiguous pair loads and scores the item's first eligible row here and is decided below)
              rowg[g] = (uint32_t)__builtin_amdgcn_readlane((int)myrow, pg[g] == AMBIGUOUS ? first : pg[g]);
              cp[g] = a.rows + (size_t)rowg[g] * pitch4;
              qp[g][0] = a.queries + (size_t)(v0 + 32u * vt + (uint32_t)bg[g]) * pitch4;
#pragma unroll
              for (int n = 0; n < NR; ++n) {
                c[g][n] = q[g][0][n] = f4{0.f, 0.f, 0.f, 0.f};
                if (NI > 0 && j + (uint32_t)n * 64 < pitch4) {
                  c[g][n] = cp[g][j + (uint32_t)n * 64];
                  q[g][0][n] = qp[g][0][j + (uint32_t)n * 64];
                }
              }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
              float s[1];
              exact_score_block<METRIC, 1, NI>(c[g], cp[g], q[g], qp[g], pitch4, j, s);
              u64 key = row_key(s[0], rowg[g]);
              if (pg[g] == AMBIGUOUS) {  // (wave-uniform) every eligible row of the item, as label_keys_kernel
                for (u64 mm = imask & (imask - 1); mm; mm &= mm - 1)
                  key = max(key, exact_one((uint32_t)__builtin_amdgcn_readlane((int)myrow, __builtin_ctzll(mm)), v0 + 32u * vt + (uint32_t)bg[g]));
              }
              if (l31 == bg[g] && lh == (vt & 1)) out[vt] = key;
            }
          }
        }
      }
#pragma unroll
      for (int vt = 0; vt < VT; ++vt)
        if (lh == (vt & 1) && 32u * vt + (uint32_t)l31 < nvb) a.keys[(size_t)(v0 + 32u * vt + (uint32_t)l31) * a.key_stride + item] = out[vt];
    }
  }
  if (lane == 0) amb_s[wave] = amb;
  __syncthreads();
  if (tid == 0) {
    const u64 sum = amb_s[0] + amb_s[1] + amb_s[2] + amb_s[3];
    if (sum) atomicAdd(t.ambiguous, sum);
  }
}

typedef void (*label_keys_tile_fn)(LabelKeysTileArgs);

// vt as multivector_tile_plan (host_multivector_tiles.h) chooses it: 1, 2 or 4; null for any other
static label_keys_tile_fn pick_label_keys_tile(int vt, uint32_t pitch4) {
  return with_row_block_ni(pitch4, [&](auto ni) -> label_keys_tile_fn {
    constexpr int NI = decltype(ni)::value;
    switch (vt) {
      case 1: return label_keys_tile_kernel<1, NI>;
      case 2: return label_keys_tile_kernel<2, NI>;
      case 4: return label_keys_tile_kernel<4, NI>;
      default: return nullptr;
    }
  });
}
