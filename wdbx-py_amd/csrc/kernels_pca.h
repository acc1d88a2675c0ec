// kernels_pca.h -- device PCA (wdbx_index_moments, wdbx_index_project):
//   moments_sum_kernel      column sums and the count of the counted rows, one wave per range of consecutive rows
//   moments_mean_kernel     the ranges' sums folded in range order, one division by the count: the fp32 mean
//   scatter_tile_kernel     split-K SYRK on the matrix cores, K = stored rows: S = sum (x - mean)(x - mean)^T.  Both MFMA operands
//                           of a tile are 32 consecutive floats of each of two consecutive staged rows -- no transposition
//   scatter_combine_kernel  the ranges' fp32 partials folded in float64 in range order, mirrored by the folding thread
//   project_tile_kernel     every row's (x - offset) . basis[c], basis vectors as the M operand so that a lane owns four
//                           consecutive components of one row: 16-byte stores
// A row is COUNTED when the call's mask allows it and its cached squared norm is finite (removed rows and rows with a NaN or
// infinite element drop out).  Plan, tile groups, LDS and grids: host_pca.h, whose constexpr functions these kernels call.
// Part of the single translation unit wdbx_hip.hip (included there, behind kernels_assign.h); not a standalone header.

// (no packed fp32 instructions in these kernels: their quads are subtracted and added element by element)
#if defined(__HIP_DEVICE_COMPILE__)
#define PCA_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#define PCA_INLINE __attribute__((always_inline, target("no-packed-fp32-ops")))
#else
#define PCA_KERNEL __global__
#define PCA_INLINE __attribute__((always_inline))
#endif

__device__ __forceinline__ bool pca_counted(const uint32_t* mask, const float* cn, uint32_t row) {
  return row_allowed(mask, row) && fabsf(cn[row]) < INFINITY;  // (a NaN norm compares false)
}

struct MomentsSumArgs {
  const f4* rows;
  const float* cn;         // squared norm of every stored row
  const uint32_t* mask;    // optional row filter
  f4* partial;             // [ranges][pitch4]
  uint32_t* partial_count; // [ranges]
  float* mean;             // [mean_len]: columns < dim the mean, the others zero (mean kernel)
  u64* count;              // the counted rows (mean kernel)
  uint32_t n_rows, pitch4, dim, mean_len, ranges;
  u64 rows_per_range;
};

// Wave p owns rows [p L, (p + 1) L) and partial p.  Lane l holds quads l, l + 64, l + 128, l + 192 of a panel of 256 quads in
// registers and adds the range's counted rows to them in row order; rows longer than a panel are walked panel by panel, so
// every quad of a counted row is still read once.
PCA_KERNEL __launch_bounds__(256) void moments_sum_kernel(MomentsSumArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= a.ranges) return;
  const u64 r0 = (u64)p * a.rows_per_range, r1 = min((u64)a.n_rows, r0 + a.rows_per_range);
  uint32_t counted = 0;
  for (uint32_t q0 = 0; q0 < a.pitch4; q0 += 256) {
    f4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) s[t] = f4{0.f, 0.f, 0.f, 0.f};
    for (u64 base = r0; base < r1; base += 64) {
      const bool mine = base + lane < r1 && pca_counted(a.mask, a.cn, (uint32_t)(base + lane));
      const u64 bal = __ballot(mine);  // (wave-uniform: which of these 64 rows count)
      if (q0 == 0) counted += (uint32_t)__popcll(bal);
      const int nb = (int)min((u64)64, r1 - base);
      for (int u = 0; u < nb; ++u) {
        if (!((bal >> u) & 1)) continue;
        const f4* rp = a.rows + (size_t)(base + u) * a.pitch4;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const uint32_t q = q0 + lane + 64 * t;
          if (q < a.pitch4) {
            const f4 v = ld16<true>(rp + q);
            s[t].x += v.x;
            s[t].y += v.y;
            s[t].z += v.z;
            s[t].w += v.w;
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t q = q0 + lane + 64 * t;
      if (q < a.pitch4) a.partial[(size_t)p * a.pitch4 + q] = s[t];
    }
  }
  if (lane == 0) a.partial_count[p] = counted;
}

// mean[i] = (((partial 0 + partial 1) + partial 2) + ...)[i] / (float)count in fp32, one thread per column; zero past the
// dimension and when nothing is counted.  Every thread folds the counters itself; thread 0 writes the count.
PCA_KERNEL __launch_bounds__(256) void moments_mean_kernel(MomentsSumArgs a) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  u64 n = 0;
  for (uint32_t p = 0; p < a.ranges; ++p) n += a.partial_count[p];
  if (i == 0) *a.count = n;
  if (i >= a.mean_len) return;
  float s = 0.f;
  if (i < a.dim && n) {
    const float* part = (const float*)a.partial;
    const size_t pitch = (size_t)a.pitch4 * 4;
    for (uint32_t p = 0; p < a.ranges; ++p) s += part[p * pitch + i];
    s = s / (float)n;
  }
  a.mean[i] = s;
}

struct ScatterArgs {
  const f4* rows;
  const float* cn;
  const uint32_t* mask;
  const f4* mean;   // [dp / 4] quads: what is subtracted while a row is staged (zeros for center = 0)
  float* partial;   // [ranges][dp][dp]
  double* out;      // [dim][dim] (combine)
  uint32_t n_rows, pitch4, dim, dp, nb, side, ranges;
  u64 rows_per_range;  // a multiple of PCA_CHUNK_ROWS
};

// Workgroup = 8 waves = (range blockIdx.x, tile group blockIdx.y).  The range's rows go chunk by chunk (32 rows) through two
// LDS buffers, row-major, only the group's column blocks, the mean subtracted on the way in, uncounted rows and columns past
// the row's end as zeros; the loader's registers run one chunk ahead of the matrix ops.  For the row pair (r, r + 1) of a chunk
// a lane's fragment of column block b is x_{r + (lane >> 5)}[32 b + (lane & 31)]: the A operand of v_mfma_f32_32x32x2_f32
// (A[lane & 31][lane >> 5]) when b = I and its B operand (B[lane >> 5][lane & 31]) when b = J, so tile (I, J) accumulates
// sum_r x_r[32 I + i] x_r[32 J + j] as one fma chain in row order.  A wave holds NT tiles = 16 NT accumulator registers; the
// instance is the smallest NT that holds the launch's fullest wave (host_pca.h: PcaPlan::instance).
// C layout as assign_tile_kernel's: column j = lane & 31, row i = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) for register e.
// NS = staged quads a thread carries per chunk: 8 quads x staged blocks / 16 threads of a row.
template <int NT, int NS>
PCA_KERNEL __launch_bounds__(512) void scatter_tile_kernel(ScatterArgs a) {
  extern __shared__ float lds_f[];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: the wave's tile table stays out of the vector registers)
  const PcaGroup G = pca_group((int)a.nb, (int)a.side, (int)blockIdx.y);
  const int ldw = pca_lds_row(G.staged);
  const u64 r0 = (u64)blockIdx.x * a.rows_per_range, r1 = min((u64)a.n_rows, r0 + a.rows_per_range);
  const uint32_t chunks = r1 > r0 ? (uint32_t)((r1 - r0 + PCA_CHUNK_ROWS - 1) / PCA_CHUNK_ROWS) : 0;

  // this wave's tiles: LDS offsets (floats) of their A and B blocks; cnt of them are real
  const int first = wave * G.per_wave;
  const int cnt = max(0, min(G.per_wave, G.tiles - first));
  int offa[NT], offb[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    int sa = 0, sb = 0;
    if (t < cnt) pca_tile_staged(G, first + t, &sa, &sb);
    offa[t] = sa * 32;
    offb[t] = sb * 32;
  }

  // the loader: thread (srow = tid >> 4, sq = tid & 15) carries quads sq, sq + 16, ... of staged row srow, in two halves of
  // NH quads so that only NH quads wait in registers under the matrix ops: half 0 is fetched at the start of the previous chunk
  // and stored after its first eight row pairs, half 1 is fetched then and stored at its end
  constexpr int NH = NS / 2;
  const uint32_t srow = (uint32_t)tid >> 4, sq = (uint32_t)tid & 15;
  f4 sr[NH];
  uint32_t word = 0;  // which of the staged chunk's 32 rows count (wave-uniform; every wave computes it for itself)
  auto gload = [&](uint32_t c, int half) PCA_INLINE {
    const u64 base = r0 + (u64)c * PCA_CHUNK_ROWS;
    if (half == 0) {
      const bool mine = lane < PCA_CHUNK_ROWS && base + lane < r1 && pca_counted(a.mask, a.cn, (uint32_t)(base + lane));
      word = (uint32_t)__ballot(mine);
    }
    const bool on = (word >> srow) & 1;
    const f4* rp = a.rows + (size_t)(base + srow) * a.pitch4;  // (read only when the row counts: it then lies inside the range)
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      const uint32_t q = sq + 16u * (uint32_t)(half * NH + i);
      f4 v = f4{0.f, 0.f, 0.f, 0.f};
      if ((q >> 3) < (uint32_t)G.staged) {
        const uint32_t gq = (uint32_t)pca_staged_block(G, (int)(q >> 3)) * 8 + (q & 7);  // the quad's place in a stored row
        if (on && gq < a.pitch4) {
          const f4 x = rp[gq];
          const f4 m = a.mean[gq];
          v.x = x.x - m.x;
          v.y = x.y - m.y;
          v.z = x.z - m.z;
          v.w = x.w - m.w;
        }
      }
      sr[i] = v;
    }
  };
  auto lstore = [&](int buf, int half) PCA_INLINE {
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      const uint32_t q = sq + 16u * (uint32_t)(half * NH + i);
      if ((q >> 3) < (uint32_t)G.staged) *(f4*)&lds_f[(buf * PCA_CHUNK_ROWS + srow) * ldw + q * 4] = sr[i];
    }
  };

  f16v acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
  // eight row pairs of a chunk from its LDS buffer
  auto pairs = [&](int buf, int p0) PCA_INLINE {
    const float* B = lds_f + (buf * PCA_CHUNK_ROWS + 2 * p0 + lh) * ldw + l31;
    // (no branch on the wave's real tile count: a spare accumulator repeats the group's first tile and is never written out.
    // One set of 2 NT fragment registers, refilled in place: right after tile t's matrix op has taken its two fragments, the
    // NEXT row pair's fragments of tile t are read into them -- NT matrix ops ahead of their use)
    float fa[NT], fb[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      fa[t] = B[offa[t]];
      fb[t] = B[offb[t]];
    }
#pragma unroll
    for (int p = 0; p < PCA_CHUNK_ROWS / 4; ++p) {
      const float* P = B + 2 * (p + 1) * ldw;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[t], fb[t], acc[t], 0, 0, 0);
        if (p + 1 < PCA_CHUNK_ROWS / 4) {
          fa[t] = P[offa[t]];
          fb[t] = P[offb[t]];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };

  if (chunks) {
    gload(0, 0);
    lstore(0, 0);
    gload(0, 1);
    lstore(0, 1);
  }
  __syncthreads();
  for (uint32_t c = 0; c < chunks; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < chunks;
    if (more) gload(c + 1, 0);  // the next chunk's global loads, in flight under this chunk's matrix ops
    pairs(buf, 0);
    if (more) {
      lstore(buf ^ 1, 0);
      gload(c + 1, 1);
    }
    pairs(buf, PCA_CHUNK_ROWS / 4);
    if (more) lstore(buf ^ 1, 1);
    __syncthreads();
  }

  // the wave's tiles to this range's partial: element (32 I + i, 32 J + j)
  float* part = a.partial + (size_t)blockIdx.x * a.dp * a.dp;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t >= cnt) continue;
    const uint32_t I = (uint32_t)pca_staged_block(G, offa[t] >> 5), J = (uint32_t)pca_staged_block(G, offb[t] >> 5);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const uint32_t i = 32 * I + (e & 3) + 8 * (e >> 2) + 4 * lh, j = 32 * J + l31;
      part[(size_t)i * a.dp + j] = acc[t][e];
    }
  }
}

typedef void (*scatter_tile_fn)(ScatterArgs);
static scatter_tile_fn pick_scatter_tile(int instance) {
  switch (instance) {
    case 1: return scatter_tile_kernel<1, 8>;
    case 2: return scatter_tile_kernel<2, 8>;
    case 4: return scatter_tile_kernel<4, 8>;
    case 6: return scatter_tile_kernel<6, 8>;
    case 8: return scatter_tile_kernel<8, 8>;
    case PCA_WAVE_TILES: return scatter_tile_kernel<PCA_WAVE_TILES, 6>;
    default: return nullptr;
  }
}

// out[i][j] = out[j][i] = ((double)partial 0 + partial 1) + ... in float64 in range order: one thread per element i <= j
PCA_KERNEL __launch_bounds__(256) void scatter_combine_kernel(ScatterArgs a) {
  const u64 total = (u64)a.dim * a.dim;
  for (u64 e = (u64)blockIdx.x * 256 + threadIdx.x; e < total; e += (u64)gridDim.x * 256) {
    const uint32_t i = (uint32_t)(e / a.dim), j = (uint32_t)(e - (u64)i * a.dim);
    if (i > j) continue;
    const size_t at = (size_t)i * a.dp + j, per = (size_t)a.dp * a.dp;
    double s = 0.0;
    for (uint32_t p = 0; p < a.ranges; ++p) s += (double)a.partial[p * per + at];
    a.out[(size_t)i * a.dim + j] = s;
    a.out[(size_t)j * a.dim + i] = s;
  }
}

struct ProjectArgs {
  const f4* rows;
  const float* cn;
  const uint32_t* mask;
  const f4* basis;   // [32][kq] quads: rows >= m and columns >= dim zero
  const f4* offset;  // [kq] quads, zero past the dimension
  float* out;        // [n_rows][m]
  uint32_t n_rows, pitch4, kq, m, num_tiles;  // kq = 8 ceil(dim / 32): quads of the padded dimension dp
};

// Workgroup = 4 waves, tile = 128 stored rows, wave w its rows 32 w .. 32 w + 31.  Operand roles as assign_tile_kernel's: the
// basis vectors are the M operand (A[c][k]), the stored rows the N operand (B[k][row]), so lane (row = lane & 31, half =
// lane >> 5) ends with components (e & 3) + 8 (e >> 2) + 4 half of ITS row: four consecutive components per register quad,
// one 16-byte store each when m is a multiple of 4.  K = the columns, staged in chunks of 32 floats through two LDS buffers
// (rows minus offset; the basis chunk next to them, from L2), the loader one chunk ahead.  MFMA step j of a chunk takes
// columns 2 j and 2 j + 1: the chain runs over ascending columns.
PCA_KERNEL __launch_bounds__(256) void project_tile_kernel(ProjectArgs a) {
  constexpr int BK = PCA_PROJECT_BK, QPC = BK / 4, LD = PCA_PROJECT_LD, TR = PCA_PROJECT_TILE_ROWS;
  constexpr int RPP = 256 / QPC, NA = TR / RPP;  // 32 rows per pass of the 256 threads, 4 passes
  extern __shared__ float lds_f[];
  float* Rs = lds_f;               // [2][TR][LD] stored rows minus offset
  float* Bs = Rs + 2 * TR * LD;    // [2][32][LD] basis
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
  const uint32_t kchunks = a.kq / QPC;
  const uint32_t srow = tid / QPC, squad = tid % QPC;
  if (blockIdx.x >= a.num_tiles) return;

  uint32_t ld_tile = blockIdx.x, ld_kc = 0, ld_on = 0;
  f4 sr[NA], sb;
  auto gload = [&]() PCA_INLINE {
    const uint32_t kq = ld_kc * QPC + squad;
    const uint32_t r0 = ld_tile * TR;
    const f4 o = a.offset[kq];
    if (ld_kc == 0) {  // which of this thread's rows of the tile count: looked up once per tile, not in front of every chunk's loads
      ld_on = 0;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const uint32_t row = r0 + srow + RPP * i;
        if (row < a.n_rows && pca_counted(a.mask, a.cn, row)) ld_on |= 1u << i;
      }
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const uint32_t row = r0 + srow + RPP * i;
      f4 v = f4{0.f, 0.f, 0.f, 0.f};
      // (an uncounted row is staged as zeros and written as zeros; columns past the row's end count as zero)
      if (((ld_on >> i) & 1) && kq < a.pitch4) v = ld16<true>(a.rows + (size_t)row * a.pitch4 + kq);
      v.x -= o.x;
      v.y -= o.y;
      v.z -= o.z;
      v.w -= o.w;
      sr[i] = v;
    }
    sb = a.basis[(size_t)srow * a.kq + kq];
    if (++ld_kc == kchunks) {
      ld_kc = 0;
      if (ld_tile + gridDim.x < a.num_tiles) ld_tile += gridDim.x;  // (past the last tile: it is staged again, never consumed)
    }
  };
  auto lstore = [&](int buf) PCA_INLINE {
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) Rs[(buf * TR + srow + RPP * i) * LD + squad * 4 + e] = sr[i][e];
#pragma unroll
    for (int e = 0; e < 4; ++e) Bs[(buf * 32 + srow) * LD + squad * 4 + e] = sb[e];
  };

  gload();
  lstore(0);
  __syncthreads();
  uint32_t it = 0;
  for (uint32_t t = blockIdx.x; t < a.num_tiles; t += gridDim.x) {
    f16v acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    for (uint32_t kc = 0; kc < kchunks; ++kc, ++it) {
      const int buf = it & 1;
      gload();
      const float* R = Rs + (buf * TR + wave * 32 + l31) * LD + lh;
      const float* Bv = Bs + (buf * 32 + l31) * LD + lh;
#pragma unroll
      for (int j = 0; j < BK / 2; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Bv[2 * j], R[2 * j], acc, 0, 0, 0);
      lstore(buf ^ 1);
      __syncthreads();
    }
    const uint32_t row = t * TR + wave * 32 + l31;
    if (row >= a.n_rows) continue;
    const bool counted = pca_counted(a.mask, a.cn, row);
    float* o = a.out + (size_t)row * a.m;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const uint32_t c0 = 8 * g + 4 * lh;
      f4 v = f4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
      if (!counted) v = f4{0.f, 0.f, 0.f, 0.f};
      if ((a.m & 3) == 0) {
        if (c0 < a.m) *(f4*)(o + c0) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c0 + e < a.m) o[c0 + e] = v[e];
      }
    }
  }
}
