// kernels_seed.h -- k-means++ seeding of the stored rows (wdbx_index_seed_centers): D^2 sampling with
// integer weights, the whole loop of steps on the device.  A step is three kinds of launch:
//   seed_pick_kernel   one workgroup: the step's candidate rows from its draws -- target = mulhi64(draw, W), a workgroup prefix
//                      scan over the sums of the blocks of 1 024 rows, then over the weights of the block the target lands in
//   seed_eval_kernel   the hot path: ONE read of the stored rows against the step's candidate rows, which the workgroup fetches
//                      by row number from the corpus into LDS; every (row, candidate) score has exact_score's bits, becomes an
//                      integer weight (seed_weight, host_seed.h) and is folded into the candidate's 64-bit potential
//   seed_apply_kernel  the winner (smallest potential, ties to the lowest trial), w <- min(w, w_win), the new block sums
// No floating-point atomics and no order dependence anywhere: every sum is an integer sum.
// Part of the single translation unit wdbx_hip.hip (included there, behind kernels_rowblock.h); not a standalone header.

struct SeedArgs {
  const f4* rows;        // [n_rows, pitch4] quads
  const float* cn;       // squared row norms (init: not finite = not eligible)
  const uint32_t* mask;  // optional row filter (init)
  uint32_t* w;           // [n_rows] the minimum over the chosen centres of a row's weight (SEED_W_UNSET before the first)
  uint32_t* dead;        // [blocks * 32] bit r: row r is ineligible, chosen or past the end -- its weight is 0 whatever w says
  u64* sums;             // [blocks] the live rows' weights per block of SEED_BLOCK_ROWS rows
  u64* pot;              // [SEED_MAX_TRIALS] the step's potentials
  uint32_t* cand;        // [SEED_MAX_TRIALS] the step's candidate rows
  u64* out_rows;         // [n_centers]
  u64* out_pot;          // [n_centers]
  const u64* draws;      // [n_centers * n_trials]
  uint32_t* scratch;     // [n_trials][n_rows] every candidate's weights of the step
  uint32_t n_rows, pitch4, blocks, span;
  int n_trials;          // of the call (the draws' stride)
  int step;              // the centre being chosen
  int trials;            // candidates of this step: 1 for the first, n_trials after it
  int j0, n_res;         // eval: the resident chunk, candidates [j0, j0 + n_res)
  int shift;             // L2: the call's shift
};

__device__ __forceinline__ u64 seed_wave_sum(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// exclusive prefix of v over the 256 threads in thread order and the total, through 256 u64 of LDS (Hillis-Steele)
__device__ __forceinline__ u64 seed_wg_scan(u64 v, u64* sc, int tid, u64* total) {
  sc[tid] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const u64 add = tid >= o ? sc[tid - o] : 0ull;
    __syncthreads();
    sc[tid] += add;
    __syncthreads();
  }
  const u64 incl = sc[tid];
  *total = sc[255];
  __syncthreads();  // (sc is free again)
  return incl - v;
}

// every row's weight unset; dead = masked out, a squared norm that is not finite (a removed row is NaN), or past the end
__global__ __launch_bounds__(256) void seed_init_kernel(SeedArgs a) {
  const int lane = threadIdx.x & 63;
  for (uint32_t b = blockIdx.x; b < a.blocks; b += gridDim.x) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t row = b * SEED_BLOCK_ROWS + (uint32_t)i * 256 + threadIdx.x;
      bool ok = false;
      if (row < a.n_rows) {
        ok = row_allowed(a.mask, row) && fabsf(a.cn[row]) < INFINITY;
        a.w[row] = SEED_W_UNSET;
      }
      const u64 bal = __ballot(ok);
      if (lane == 0) {  // (row is a multiple of 64 here)
        a.dead[row >> 5] = ~(uint32_t)bal;
        a.dead[(row >> 5) + 1] = ~(uint32_t)(bal >> 32);
      }
    }
  }
}

// One workgroup.  The sampling weight of a live row is w, or 1 in the first step and when every w is 0 (every eligible row
// coincides with a centre); of a dead row 0.  A trial's target t = mulhi64(draw, W) < W picks the lowest row whose inclusive
// prefix sum exceeds t: thread i owns a contiguous run of blocks, the workgroup scan of the runs' sums finds the run, its owner
// walks to the block, the workgroup scan of the block's 256 groups of 4 rows finds the group, its owner walks to the row.
// Also clears the potentials for the step's eval launches.
__global__ __launch_bounds__(256) void seed_pick_kernel(SeedArgs a) {
  __shared__ u64 sc[256];
  __shared__ u64 hit_rem;
  __shared__ uint32_t hit_block;
  const int tid = threadIdx.x;
  if (tid < SEED_MAX_TRIALS) a.pot[tid] = 0;
  const uint32_t run = (a.blocks + 255) / 256;
  const uint32_t b0 = min((uint32_t)tid * run, a.blocks), b1 = min(b0 + run, a.blocks);
  bool uniform = a.step == 0;
  auto block_sum = [&](uint32_t b) -> u64 {
    if (!uniform) return a.sums[b];
    uint32_t live = 0;
    for (uint32_t wd = 0; wd < SEED_BLOCK_ROWS / 32; ++wd) live += (uint32_t)__popc(~a.dead[b * (SEED_BLOCK_ROWS / 32) + wd]);
    return live;
  };
  u64 mine, excl, W;
  for (;;) {
    mine = 0;
    for (uint32_t b = b0; b < b1; ++b) mine += block_sum(b);
    excl = seed_wg_scan(mine, sc, tid, &W);
    if (uniform || W) break;  // (the same for every thread)
    uniform = true;
  }
  for (int j = 0; j < a.trials; ++j) {
    if (!W) {  // (no live row: the host refuses such a call; nothing is read out of bounds either way)
      if (tid == 0) a.cand[j] = 0;
      continue;
    }
    const u64 t = seed_mulhi64(a.draws[(size_t)a.step * a.n_trials + j], W);
    if (mine && excl <= t && t - excl < mine) {
      u64 rem = t - excl;
      uint32_t b = b0;
      for (; b + 1 < b1; ++b) {
        const u64 v = block_sum(b);
        if (rem < v) break;
        rem -= v;
      }
      hit_block = b;
      hit_rem = rem;
    }
    __syncthreads();
    const uint32_t r0 = hit_block * SEED_BLOCK_ROWS + (uint32_t)tid * 4;
    const u64 rem = hit_rem;
    const uint32_t dw = a.dead[r0 >> 5];
    u64 v[4], s4 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t r = r0 + (uint32_t)i;
      const bool live = r < a.n_rows && !((dw >> (r & 31)) & 1u);
      v[i] = live ? (uniform ? 1ull : (u64)a.w[r]) : 0ull;
      s4 += v[i];
    }
    u64 total;
    const u64 e = seed_wg_scan(s4, sc, tid, &total);
    if (s4 && e <= rem && rem - e < s4) {
      u64 x = rem - e;
      uint32_t pick = r0 + 3;
#pragma unroll
      for (int i = 2; i >= 0; --i) {  // the lowest i whose inclusive prefix exceeds x
        const u64 upto = v[0] + (i >= 1 ? v[1] : 0ull) + (i >= 2 ? v[2] : 0ull);
        if (x < upto) pick = r0 + (uint32_t)i;
      }
      a.cand[j] = pick;
    }
    __syncthreads();  // (hit_block / hit_rem are free again)
  }
}

// The hot path.  Grid: persistent, each of its waves a contiguous span of rows, walked two rows at a time so that one LDS read of
// a candidate quad serves two loaded rows.  The chunk's n_res candidate rows lie in LDS; lane j accumulates quads j, j + 64, ...
// of a loaded row against each candidate with accum<METRIC> in that order and exact_finish closes each chain: exact_score's bits
// with the candidate row as the query (kernels_rowblock.h's frame, the queries in LDS instead of registers).  CB: accumulators
// per loaded row; slots past n_res repeat the last candidate and report nothing.
// Lane b of the first 16 lanes reports candidate b for the first row of the pair, lane 16 + b for the second: the weight, its
// store to the scratch, min(w, w_b) into the lane's own 64-bit sum.  The sums meet by one integer shuffle in the wave, through
// LDS (the candidates' own bytes, behind a barrier) in the workgroup, and leave it as one integer atomicAdd per candidate.
template <int METRIC, int CB>
__global__ __launch_bounds__(256) void seed_eval_kernel(SeedArgs a) {
  extern __shared__ f4 seed_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t pitch4 = a.pitch4;
  for (int c = 0; c < a.n_res; ++c) {
    const f4* src = a.rows + (size_t)a.cand[a.j0 + c] * pitch4;
    for (uint32_t i = threadIdx.x; i < pitch4; i += 256) seed_lds[(size_t)c * pitch4 + i] = src[i];
  }
  __syncthreads();
  const int slot = lane & 15;
  const bool reporter = lane < 32 && slot < a.n_res && slot < CB;
  const uint32_t crow = a.cand[a.j0 + min(slot, a.n_res - 1)];
  uint32_t* const sc = a.scratch + (size_t)(a.j0 + min(slot, a.n_res - 1)) * a.n_rows;
  u64 pot = 0;
  const u64 first = (u64)(blockIdx.x * 4 + wave) * a.span;
  const uint32_t r_end = (uint32_t)min((u64)a.n_rows, first + a.span);
  for (uint32_t r = (uint32_t)min(first, (u64)a.n_rows); r < r_end; r += 2) {
    const bool has1 = r + 1 < r_end;
    const uint32_t r1 = has1 ? r + 1 : r;
    const bool d0 = (a.dead[r >> 5] >> (r & 31)) & 1u;
    const bool d1 = !has1 || ((a.dead[r1 >> 5] >> (r1 & 31)) & 1u);
    f4 acc0[CB], acc1[CB];
#pragma unroll
    for (int b = 0; b < CB; ++b) acc0[b] = acc1[b] = f4{0.f, 0.f, 0.f, 0.f};
    if (!(d0 && d1)) {  // (wave-uniform) a pair of dead rows is not read
      const f4* p0 = a.rows + (size_t)r * pitch4;
      const f4* p1 = a.rows + (size_t)r1 * pitch4;
      for (uint32_t i = (uint32_t)lane; i < pitch4; i += 64) {
        const f4 v0 = ld16<true>(p0 + i), v1 = ld16<true>(p1 + i);
        uint32_t at = i;  // candidate b's quad i: slot min(b, n_res - 1)
#pragma unroll
        for (int b = 0; b < CB; ++b) {
          const f4 c = seed_lds[at];
          acc0[b] = accum<METRIC>(acc0[b], v0, c);
          acc1[b] = accum<METRIC>(acc1[b], v1, c);
          at += b + 1 < a.n_res ? pitch4 : 0u;
        }
      }
    }
    float mine = 0.f;
#pragma unroll
    for (int b = 0; b < CB; ++b) {
      const float s0 = exact_finish<METRIC, 64>(acc0[b]), s1 = exact_finish<METRIC, 64>(acc1[b]);
      if (lane == b) mine = s0;
      if (lane == 16 + b) mine = s1;
    }
    if (reporter && (lane < 16 || has1)) {
      const uint32_t row = lane < 16 ? r : r1;
      const bool dead = lane < 16 ? d0 : d1;
      // a chosen row is dead; the candidate itself weighs 0 by its row number, whatever its score against itself rounds to
      const uint32_t wj = (dead || row == crow) ? 0u : seed_weight(METRIC == WDBX_METRIC_L2, mine, a.shift);
      sc[row] = wj;
      if (!dead) pot += (u64)min(a.w[row], wj);
    }
  }
  pot += __shfl_xor(pot, 16);
  __syncthreads();  // (every wave is done with the candidates: their bytes become the workgroup's 4 x 16 sums)
  u64* const red = (u64*)seed_lds;
  if (lane < 16) red[wave * 16 + lane] = pot;
  __syncthreads();
  if ((int)threadIdx.x < a.n_res) {
    const u64 s = red[threadIdx.x] + red[16 + threadIdx.x] + red[32 + threadIdx.x] + red[48 + threadIdx.x];
    if (s) atomicAdd((unsigned long long*)&a.pot[a.j0 + threadIdx.x], (unsigned long long)s);
  }
}

// The step's winner, then one pass over the weights: w <- min(w, the winner's), the winner dies, a block's live weights are summed.
// Workgroups stride over the blocks; a thread owns 4 consecutive rows (one word of dead bits).
__global__ __launch_bounds__(256) void seed_apply_kernel(SeedArgs a) {
  __shared__ u64 red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int win = 0;
  u64 best = a.pot[0];
  for (int j = 1; j < a.trials; ++j) {
    const u64 p = a.pot[j];
    if (p < best) best = p, win = j;
  }
  const uint32_t wrow = a.cand[win];
  const uint32_t* const sw = a.scratch + (size_t)win * a.n_rows;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.out_rows[a.step] = wrow;
    a.out_pot[a.step] = best;
  }
  for (uint32_t b = blockIdx.x; b < a.blocks; b += gridDim.x) {
    const uint32_t r0 = b * SEED_BLOCK_ROWS + threadIdx.x * 4;
    const uint32_t dw = a.dead[r0 >> 5];
    u64 s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t r = r0 + (uint32_t)i;
      if (r >= a.n_rows) continue;
      const uint32_t v = min(a.w[r], sw[r]);
      a.w[r] = v;
      if (r == wrow) atomicOr(&a.dead[r >> 5], 1u << (r & 31));
      else if (!((dw >> (r & 31)) & 1u)) s += v;
    }
    s = seed_wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) a.sums[b] = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
  }
}

typedef void (*seed_eval_fn)(SeedArgs);

template <int METRIC>
static seed_eval_fn pick_seed_eval_metric(int block) {
  if (block == 1) return seed_eval_kernel<METRIC, 1>;
  if (block == 4) return seed_eval_kernel<METRIC, 4>;
  if (block == 16) return seed_eval_kernel<METRIC, 16>;
  return nullptr;
}

static seed_eval_fn pick_seed_eval(int metric, int block) {
  return metric == WDBX_METRIC_L2 ? pick_seed_eval_metric<WDBX_METRIC_L2>(block) : pick_seed_eval_metric<WDBX_METRIC_COSINE>(block);
}
