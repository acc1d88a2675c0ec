// kernels_assign.h -- nearest-centre assignment (wdbx_index_assign): the transposed search.  MANY stored rows against FEW given
// vectors, a top-1 kept per stored row:
//   assign_prep_kernel    the call's centres in place: pad columns zeroed, normalised (cosine, on request), squared norms, the
//                         largest of them; unused slots of the last block zero-filled
//   assign_tile_kernel    the tile pass on the matrix cores with the operand roles of gemm_topk_kernel exchanged: centres are the
//                         M operand, stored rows the N operand, so a stored row is one lane's COLUMN of the 32x32 accumulator and
//                         its running (best, best centre, second best) is a fold over that lane's registers
//   assign_exact_kernel   exact_score's arithmetic: the ambiguous rows against every centre (blocks of 8), or every certain
//                         row against its winner (a block of one) for the returned score
//   assign_sums_kernel,   per-centre sums of the assigned rows: one partial per wave over consecutive rows, combined in partial
//   assign_combine_kernel order -- no floating-point atomics, the same bits on every run
// Plan, grids and the bound's coefficients: host_assign.h.  The inequality behind "certain": DESIGN.md section 4.20.
// Part of the single translation unit wdbx_hip.hip (included there, behind kernels_rowblock.h); not a standalone header.

// (no packed fp32 instructions in these kernels: their quads are added and multiplied element by element)
#if defined(__HIP_DEVICE_COMPILE__)
#define ASSIGN_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#define ASSIGN_INLINE __attribute__((always_inline, target("no-packed-fp32-ops")))  // (a kernel's lambdas: inlined, or their captured arrays go to scratch)
#else
#define ASSIGN_KERNEL __global__
#define ASSIGN_INLINE __attribute__((always_inline))
#endif

struct AssignPrepArgs {
  float* centres;       // [slots, pitch]: the caller's rows copied at the row pitch; everything else is written here
  float* cnorm;         // [slots] squared norms (of the normalised centre); a NaN centre's is NaN
  uint32_t* cmax_bits;  // the largest non-NaN norm, float bits (zero before the launch)
  uint32_t pitch, dim, n_centers, slots;
  int normalize;
};

// one wave per centre slot
ASSIGN_KERNEL __launch_bounds__(256) void assign_prep_kernel(AssignPrepArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= a.slots) return;
  float* p = a.centres + (size_t)slot * a.pitch;
  // (a lane touches columns lane, lane + 64, ... only, here and in normalize_row: no value crosses lanes through memory)
  const uint32_t keep = slot < a.n_centers ? a.dim : 0;
  for (uint32_t c = lane; c < a.pitch; c += 64)
    if (c >= keep) p[c] = 0.f;
  if (slot >= a.n_centers) {
    if (lane == 0) a.cnorm[slot] = 0.f;
    return;
  }
  if (a.normalize) normalize_row(p, a.pitch, lane);  // (normalize_rows_kernel's arithmetic: what normalize_queries does)
  float s = 0.f;
  for (uint32_t c = lane; c < a.pitch; c += 64) s = fmaf(p[c], p[c], s);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) {
    a.cnorm[slot] = s;
    if (s == s) atomicMax(a.cmax_bits, __float_as_uint(s));
  }
}

struct AssignArgs {
  const f4* rows;             // [n_rows, pitch4] quads
  const f4* centres;          // [n_blocks * 32 MT, pitch4], prepared
  const float* cnorm;         // [n_blocks * 32 MT]
  const uint32_t* cmax_bits;  // largest centre norm (squared), float bits
  const float* cn;            // squared norm of every stored row (NaN: removed, or a NaN element)
  const uint32_t* mask;       // optional row filter
  int32_t* out_center;        // [n_rows]: the winner of a certain row, -1 (no result), -2 (listed: the exact pass decides)
  u64* list;                  // the ambiguous rows, in no order
  uint32_t* list_count;
  uint32_t n_rows, pitch4, n_centers, n_blocks, num_tiles;
  float gamma, under;         // host_assign.h: assign_bound
};

// Workgroup = 4 waves, tile = 128 stored rows: wave w owns rows 32 w .. 32 w + 31 of the tile as the 32 columns of MT
// accumulators (32 MT centres of a block).  Rows and centres are staged K-chunk by K-chunk (32 floats, rows of 36: the fp32 tile
// kernel's conflict-free padding) through two LDS buffers; the loader's cursor (tile, block, chunk) runs one chunk ahead of the
// compute cursor across blocks and tiles, so a block's first chunk is in LDS when the previous block's fold ends.  A row tile
// is streamed once per centre block; re-reads come from L2 / MALL (plain loads, not non-temporal).
// C layout: column (stored row) = lane & 31, row (centre) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  Lanes l and l ^ 32 hold
// the same stored row against different centres: each folds its own 16 MT values per block -- in ascending centre order, so an
// equal value never displaces a lower index -- and the two meet in ONE exchange per row tile.
// The registers are held to assign_tile_waves (host_assign.h) waves per SIMD = resident workgroups per CU, which the grid follows:
// two, except the L2 instance with 128 centres per block (one workgroup per CU rather than scratch).
template <int METRIC, int MT>
ASSIGN_KERNEL __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(assign_tile_waves(METRIC == WDBX_METRIC_L2, MT)))) void assign_tile_kernel(AssignArgs a) {
  constexpr int BK = ASSIGN_BK, QPC = BK / 4, LD = ASSIGN_LD, S = BK / 8;
  constexpr int TR = ASSIGN_TILE_ROWS, CB = 32 * MT;
  constexpr int RPP = 256 / QPC;  // rows staged per pass of the 256 threads
  constexpr int NA = TR / RPP, NB = CB / RPP;
  extern __shared__ float lds_f[];
  float* Rs = lds_f;                // [2][TR][LD] stored rows
  float* Cs = Rs + 2 * TR * LD;     // [2][CB][LD] centres
  float* Ns = Cs + 2 * CB * LD;     // [2][CB] the norms of the block being computed / being staged (L2)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const uint32_t kchunks = (a.pitch4 + QPC - 1) / QPC;
  const uint32_t srow = tid / QPC, squad = tid % QPC;
  const uint32_t last_row = a.n_rows - 1;
  if (blockIdx.x >= a.num_tiles) return;

  // loader: one chunk of (tile, block) into registers, later into the other LDS buffer
  uint32_t ld_tile = blockIdx.x, ld_blk = 0, ld_kc = 0, ld_count = 0;  // ld_count: blocks begun (parity of Ns)
  f4 sr[NA], sc[NB];
  float sn = 0.f;
  bool st_first = false;
  uint32_t st_par = 0;
  auto gload = [&]() ASSIGN_INLINE {
    const uint32_t kq = ld_kc * QPC + squad;
    const bool in = kq < a.pitch4;  // (K tail: quads past the row end re-read its last quad and count as zero)
    const uint32_t o = min(kq, a.pitch4 - 1);
    const uint32_t r0 = ld_tile * TR;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      // rows past the end are clamped to the last row (their columns are dropped at the end of the tile)
      const f4 v = a.rows[(size_t)min(r0 + srow + RPP * i, last_row) * a.pitch4 + o];
      sr[i] = in ? v : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const f4 v = a.centres[(size_t)(ld_blk * CB + srow + RPP * i) * a.pitch4 + o];
      sc[i] = in ? v : f4{0.f, 0.f, 0.f, 0.f};
    }
    st_first = ld_kc == 0;
    st_par = ld_count & 1;
    if constexpr (METRIC == WDBX_METRIC_L2)
      if (st_first && tid < CB) sn = a.cnorm[ld_blk * CB + tid];
    if (++ld_kc == kchunks) {
      ld_kc = 0;
      ++ld_count;
      if (++ld_blk == a.n_blocks) {
        ld_blk = 0;
        // past the last tile the loader re-reads it (valid memory, never consumed)
        if (ld_tile + gridDim.x < a.num_tiles) ld_tile += gridDim.x;
      }
    }
  };
  auto lstore = [&](int buf) ASSIGN_INLINE {
#pragma unroll
    for (int i = 0; i < NA; ++i) *(f4*)&Rs[(buf * TR + srow + RPP * i) * LD + squad * 4] = sr[i];
#pragma unroll
    for (int i = 0; i < NB; ++i) *(f4*)&Cs[(buf * CB + srow + RPP * i) * LD + squad * 4] = sc[i];
    if constexpr (METRIC == WDBX_METRIC_L2)
      if (st_first && tid < CB) Ns[st_par * CB + tid] = sn;
  };

  gload();
  lstore(0);
  __syncthreads();
  uint32_t it = 0, done_blocks = 0;  // running chunk counter (LDS buffer = it & 1) and block counter (parity of Ns)
  for (uint32_t t = blockIdx.x; t < a.num_tiles; t += gridDim.x) {
    float best = -INFINITY, second = -INFINITY;
    int bidx = -1;
    for (uint32_t blk = 0; blk < a.n_blocks; ++blk, ++done_blocks) {
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
          const f4 rf = *(const f4*)&Rs[(buf * TR + wave * 32 + l31) * LD + (2 * s + lh) * 4];
          f4 cf[MT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) cf[mt] = *(const f4*)&Cs[(buf * CB + mt * 32 + l31) * LD + (2 * s + lh) * 4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(cf[mt][e], rf[e], acc[mt], 0, 0, 0);
        }
        if (kc + 1 == kchunks) {
          // the block's fold, BEFORE this iteration's LDS stores and barrier: the norms it reads were stored before the
          // previous barrier, and the stores below (the norms of the block after next among them) come after every wave's fold
          const float* ns = Ns + (done_blocks & 1) * CB;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int ml = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
              float v = acc[mt][r];
              if constexpr (METRIC == WDBX_METRIC_L2) v = fmaf(2.0f, v, -ns[ml]);  // 2 r.c - |c|^2: |r|^2 is the row's own
              if (blk * CB + ml >= a.n_centers) v = -INFINITY;                      // a padded slot never wins
              if (v > best) {  // (a NaN is neither: a centre with a NaN element is never chosen)
                second = best;
                best = v;
                bidx = (int)(blk * CB + ml);
              } else {
                second = fmaxf(second, v);
              }
            }
        }
        lstore(buf ^ 1);
        __syncthreads();
      }
    }
    // the row tile is finished: the two lanes of a stored row meet
    const float ob = __shfl_xor(best, 32), os = __shfl_xor(second, 32);
    const int oi = __shfl_xor(bidx, 32);
    const bool take = ob > best || (ob == best && (uint32_t)oi < (uint32_t)bidx);
    second = fmaxf(fmaxf(second, os), take ? best : ob);
    if (take) {
      best = ob;
      bidx = oi;
    }
    const uint32_t row = t * TR + wave * 32 + l31;
    bool listed = false;
    if (lh == 0 && row < a.n_rows) {
      int32_t outc = -1;
      const float rn2 = a.cn[row];
      if (row_allowed(a.mask, row) && rn2 == rn2) {  // (a NaN norm: a removed row or a NaN element -- every score is NaN)
        // certain <=> best - second > 2 (b_tile + b_exact); norms rounded up
        const float up = 1.0f + a.gamma;
        const float nr = sqrtf(rn2 + a.under) * up, nc = sqrtf(__uint_as_float(*a.cmax_bits) + a.under) * up;
        float margin;
        if constexpr (METRIC == WDBX_METRIC_L2)
          margin = 2.0f * a.gamma * ((2.0f * nr * nc + nc * nc) + (nr + nc) * (nr + nc)) + 12.0f * a.under;
        else
          margin = 4.0f * (a.gamma * nr * nc + a.under);
        const bool certain = fabsf(best) < INFINITY && best - second > margin;  // (an infinite or NaN margin: not certain)
        listed = !certain;
        outc = certain ? bidx : -2;
      }
      a.out_center[row] = outc;
    }
    wave_append(listed, (u64)row, a.list, a.list_count, a.n_rows, lane);
  }
}

typedef void (*assign_tile_fn)(AssignArgs);

static assign_tile_fn pick_assign_tile(int metric, int mt) {
  const bool l2 = metric == WDBX_METRIC_L2;
  switch (mt) {
    case 1: return l2 ? assign_tile_kernel<WDBX_METRIC_L2, 1> : assign_tile_kernel<WDBX_METRIC_COSINE, 1>;
    case 2: return l2 ? assign_tile_kernel<WDBX_METRIC_L2, 2> : assign_tile_kernel<WDBX_METRIC_COSINE, 2>;
    case 4: return l2 ? assign_tile_kernel<WDBX_METRIC_L2, 4> : assign_tile_kernel<WDBX_METRIC_COSINE, 4>;
    default: return nullptr;
  }
}

struct AssignExactArgs {
  const f4* rows;
  const f4* centres;
  const u64* list;             // QB = 8: the ambiguous rows
  const uint32_t* list_count;
  int32_t* out_center;         // QB = 8: written; QB = 1: read (the winner)
  float* out_score;            // may be null (QB = 8 then decides centres only)
  uint32_t n_rows, pitch4, n_centers;
};

// One wave per row, the row's quads in registers (the frame of kernels_rowblock.h), centres in blocks of QB through
// exact_score_block: a score here is the score wdbx_index_search_rows returns for (query = centre, this row), bit for bit.
//   QB = ASSIGN_EXACT_BLOCK: the listed rows against every centre, ascending; the best (score, lowest centre) is kept.
//   QB = 1: every row whose out_center is a centre, against that centre alone -- the returned score of the certain rows.
// The returned score is in the caller's convention: -0 and +0 are one score, L2 a positive squared distance.
template <int METRIC, int QB, int NI>
ASSIGN_KERNEL __launch_bounds__(256) void assign_exact_kernel(AssignExactArgs a) {
  constexpr int NR = row_block_nr(NI);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t j = (uint32_t)lane;
  const uint32_t W = gridDim.x * 4;
  const uint32_t items = QB == 1 ? a.n_rows : min(*a.list_count, a.n_rows);
  for (uint32_t i = blockIdx.x * 4 + wave; i < items; i += W) {
    uint32_t row = i, c_first = 0, c_end = a.n_centers;
    if constexpr (QB == 1) {
      const int32_t win = a.out_center[row];  // (wave-uniform)
      if (win < 0) {
        if (lane == 0 && a.out_score) a.out_score[row] = 0.f;
        continue;
      }
      c_first = (uint32_t)win;
      c_end = c_first + 1;
    } else {
      row = (uint32_t)a.list[i];
    }
    const f4* cp = a.rows + (size_t)row * a.pitch4;
    f4 c[NR];
#pragma unroll
    for (int t = 0; t < NR; ++t) {
      c[t] = f4{0.f, 0.f, 0.f, 0.f};
      if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) c[t] = ld16<true>(cp + j + (uint32_t)t * 64);
    }
    bool have = false;
    float best = 0.f;
    int32_t bidx = -1;
    for (uint32_t c0 = c_first; c0 < c_end; c0 += QB) {
      const f4* qp[QB];
      f4 q[QB][NR];
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        qp[b] = a.centres + (size_t)min(c0 + (uint32_t)b, a.n_centers - 1) * a.pitch4;  // (past the end: the last centre again, dropped below)
#pragma unroll
        for (int t = 0; t < NR; ++t) {
          q[b][t] = f4{0.f, 0.f, 0.f, 0.f};
          if (NI > 0 && j + (uint32_t)t * 64 < a.pitch4) q[b][t] = qp[b][j + (uint32_t)t * 64];
        }
      }
      float s[QB];
      exact_score_block<METRIC, QB, NI>(c, cp, q, qp, a.pitch4, j, s);
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        const float s0 = s[b] + 0.0f;
        if (c0 + (uint32_t)b < c_end && s[b] == s[b] && (!have || s0 > best)) {
          have = true;
          best = s0;
          bidx = (int32_t)(c0 + (uint32_t)b);
        }
      }
    }
    if (lane == 0) {
      a.out_center[row] = have ? bidx : -1;
      if (a.out_score) a.out_score[row] = !have ? 0.f : METRIC == WDBX_METRIC_L2 ? -best + 0.0f : best;
    }
  }
}

typedef void (*assign_exact_fn)(AssignExactArgs);

template <int METRIC>
static assign_exact_fn pick_assign_exact_metric(bool winners, uint32_t pitch4) {
  return with_row_block_ni(pitch4, [&](auto ni) -> assign_exact_fn {
    constexpr int NI = decltype(ni)::value;
    return winners ? assign_exact_kernel<METRIC, 1, NI> : assign_exact_kernel<METRIC, ASSIGN_EXACT_BLOCK, NI>;
  });
}

static assign_exact_fn pick_assign_exact(int metric, bool winners, uint32_t pitch4) {
  return metric == WDBX_METRIC_L2 ? pick_assign_exact_metric<WDBX_METRIC_L2>(winners, pitch4)
                                  : pick_assign_exact_metric<WDBX_METRIC_COSINE>(winners, pitch4);
}

struct AssignSumsArgs {
  const f4* rows;
  const int32_t* center;      // [n_rows], < 0: the row is assigned to no centre
  f4* partial;                // [partials][n_centers][pitch4]
  uint32_t* partial_count;    // [partials][n_centers]
  float* out_sums;            // [n_centers][dim] (combine)
  u64* out_counts;            // [n_centers] (combine)
  uint32_t n_rows, pitch4, dim, n_centers, partials;
  u64 rows_per_partial;
};

// Wave p owns rows [p rpp, (p + 1) rpp) and partial p: it zeroes the partial, then adds its rows to their centres' sums in
// row order.  Lane l holds quads l, l + 64, ... of every sum and the counter of centres c with c % 64 == l -- in the zeroing
// as in the adding, so no value passes between lanes through memory.  Every assigned row is read once.
ASSIGN_KERNEL __launch_bounds__(256) void assign_sums_kernel(AssignSumsArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= a.partials) return;
  f4* mine = a.partial + (size_t)p * a.n_centers * a.pitch4;
  uint32_t* cnt = a.partial_count + (size_t)p * a.n_centers;
  for (uint32_t c = 0; c < a.n_centers; ++c)
    for (uint32_t q = lane; q < a.pitch4; q += 64) mine[(size_t)c * a.pitch4 + q] = f4{0.f, 0.f, 0.f, 0.f};
  for (uint32_t c = lane; c < a.n_centers; c += 64) cnt[c] = 0;
  const u64 r0 = (u64)p * a.rows_per_partial, r1 = min((u64)a.n_rows, r0 + a.rows_per_partial);
  for (u64 base = r0; base < r1; base += 64) {
    const int32_t my = base + lane < r1 ? a.center[base + lane] : -1;
    const int nb = (int)min((u64)64, r1 - base);
    for (int u = 0; u < nb; ++u) {
      const int32_t c = __shfl(my, u);  // (wave-uniform)
      if (c < 0) continue;
      const f4* rp = a.rows + (size_t)(base + u) * a.pitch4;
      f4* sp = mine + (size_t)c * a.pitch4;
      for (uint32_t q = lane; q < a.pitch4; q += 64) {
        const f4 v = ld16<true>(rp + q);
        f4 s = sp[q];
        s.x += v.x;
        s.y += v.y;
        s.z += v.z;
        s.w += v.w;
        sp[q] = s;
      }
      if (lane == (c & 63)) cnt[c] += 1;
    }
  }
}

// out_sums[c][e] = ((partial 0 + partial 1) + partial 2) + ..., out_counts[c] likewise: one thread per element, partial order
ASSIGN_KERNEL __launch_bounds__(256) void assign_combine_kernel(AssignSumsArgs a) {
  const uint32_t pitch = a.pitch4 * 4;
  const u64 total = (u64)a.n_centers * a.dim;
  const float* part = (const float*)a.partial;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < total; i += (u64)gridDim.x * 256) {
    const uint32_t c = (uint32_t)(i / a.dim), e = (uint32_t)(i - (u64)c * a.dim);
    if (a.out_sums) {
      float s = 0.f;
      for (uint32_t p = 0; p < a.partials; ++p) s += part[((size_t)p * a.n_centers + c) * pitch + e];
      a.out_sums[i] = s;
    }
    if (e == 0 && a.out_counts) {
      u64 n = 0;
      for (uint32_t p = 0; p < a.partials; ++p) n += a.partial_count[(size_t)p * a.n_centers + c];
      a.out_counts[c] = n;
    }
  }
}
