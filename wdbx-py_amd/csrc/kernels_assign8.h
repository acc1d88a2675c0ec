// kernels_assign8.h -- the int8 route of nearest-centre assignment (wdbx_index_assign, option assign_i8): a candidate sweep on
// v_mfma_i32_16x16x64_i8 over shadow copy G, then exact scoring of the candidates alone.  Part of the single translation unit
// wdbx_hip.hip (included there, behind kernels_assign.h and kernels_join.h); not a standalone header.
//
//   assign_quant_kernel  the call's prepared centres (assign_prep_kernel) as an i8 operand: signed bytes with one scale PER
//                        CENTRE, in the MFMA fragment order of shadow copy G (g8_offset), so a centre block is copied to LDS as
//                        it lies and a 1 KiB fragment is one conflict-free ds_read_b128 per lane; per centre {s_c, |c|^2}, and
//                        the call-wide maxima of a_c >= s_c |n_c|_2 and b_c >= s_c |delta_c|_2 (integer atomicMax on float
//                        bits).  Unused slots of the last block and centres with a NaN or infinite element: zero bytes and a
//                        NaN scale, which no comparison of the sweep keeps (an infinite centre also sets a_max = +inf: every
//                        row then goes to the listed exact pass).
//   assign_i8_kernel     the sweep.  A workgroup (8 waves) KEEPS a tile of 256 stored rows and walks every centre block; each
//                        wave owns 32 rows of the tile as the N operand (fragments of G from memory straight into a register
//                        ring, no LDS for rows, no barrier in the k loop), the centre block is the M operand, resident in LDS.
//                        In the 16x16 accumulator a lane then holds 4 centres for ONE stored row (row = lane & 15 of half h),
//                        so a row's block maximum is a fold over the lane's registers and two exchanges (lanes ^ 16, ^ 32).
//                        The next centre block is read from L2 into registers before the k loop and stored to the OTHER LDS
//                        buffer behind it: one barrier per (tile, block), none with a single block.  best_T(r) lives in two
//                        registers per lane for the whole walk, so no order of blocks or stale read exists to depend on.
//                        After a block's maximum is folded in, every accumulator with T(c) >= best_T(r) - margin is appended
//                        as (row << 32 | centre) to ONE global buffer, one integer atomic per wave and (tile, block) with hits;
//                        the counter counts past the buffer, the host grows it and sweeps again.  Rows whose bad-row bit is set
//                        append nothing; rows of a group G does not vouch for, or whose margin is not finite, are listed for
//                        assign_exact_kernel's pass over all centres instead.
//   assign_pairs_kernel  the exact pass: a wave takes a run of candidates, scores (stored row, centre as the query) with
//                        exact_score and folds the score into the row's 64-bit key (order-preserving score bits, -0 as +0, then
//                        ~centre) with an integer atomicMax: the lowest index wins equal bits, whatever the arrival order.
//   assign_decode_kernel key -> out_center (no key: -1).
// Plan, route and the inequality: host_assign8.h.  DESIGN.md section 4.20b.  No floating-point atomics anywhere.
#include "host_assign8.h"

struct AssignQuantArgs {
  const float* centres;  // [slots, pitch] prepared (assign_prep_kernel); slots past n_centers may lie past the fp32 buffer's end
  const float* cnorm;    // [n_centers ..] squared norms as prepared
  int8_t* out8;          // [slots8, pitch8] fragment order
  float* par;            // [slots8] s_c (NaN: excluded), then [slots8] |c|^2
  uint32_t* max_bits;    // {a_max, b_max} float bits (zero before the launch)
  uint32_t pitch, dim, pitch8, n_centers, slots8;
};

// one wave per quantised centre slot; group_to_i8g's arithmetic with the centre as a group of its own
__global__ __launch_bounds__(256) void assign_quant_kernel(AssignQuantArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= a.slots8) return;
  const bool used = slot < a.n_centers;
  const float* p = a.centres + (size_t)(used ? slot : 0) * a.pitch;
  float mx = 0.f;
  bool bad = false, inf = false;
  if (used)
    for (uint32_t c = lane; c < a.dim; c += 64) {
      const float v = p[c];
      bad = bad || !(fabsf(v) <= 3.4028235e38f);
      inf = inf || fabsf(v) > 3.4028235e38f;
      mx = fmaxf(mx, fabsf(v));
    }
  bad = __any(bad) || !used;
  inf = __any(inf) && used;
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  const bool vanishing = mx < 1.2e-30f;
  const float s_c = vanishing ? 2.0f * mx : mx / 127.0f;
  const float inv = vanishing ? 0.f : 127.0f / mx;
  float n2 = 0.f, d2 = 0.f;
  for (uint32_t c = lane; c < a.pitch8; c += 64) {
    float x = 0.f, res = 0.f;
    if (!bad && c < a.dim) {
      const float v = p[c];
      x = fminf(fmaxf(rintf(v * inv), -127.f), 127.f);
      res = vanishing ? (mx > 0.f ? 0.5f : 0.f) : v * inv - x;
    }
    a.out8[g8_offset(slot, c, a.pitch8)] = (int8_t)(int)x;
    n2 = fmaf(x, x, n2);
    d2 = fmaf(res, res, d2);
  }
  for (int o = 32; o > 0; o >>= 1) {
    n2 += __shfl_xor(n2, o);
    d2 += __shfl_xor(d2, o);
  }
  if (lane == 0) {
    a.par[slot] = bad ? __uint_as_float(0x7FC00000u) : s_c;
    a.par[a.slots8 + slot] = used ? a.cnorm[slot] : 0.f;
    if (inf) atomicMax(a.max_bits, 0x7F800000u);
    if (!bad) {  // rounded up as the group table's entries are
      atomicMax(a.max_bits, __float_as_uint(s_c * sqrtf(n2) * 1.0002f));
      atomicMax(a.max_bits + 1, __float_as_uint(s_c * (sqrtf(d2) * 1.0002f + 2e-5f * sqrtf((float)a.dim))));
    }
  }
}

struct Assign8Args {
  const int8_t* rows8;       // shadow copy G: fragment-ordered blocks, whole tiles
  const f4* groups;          // {s_g, a_g, b_g, vouch} per 64-row group
  const u64* gbad;           // bad-row bits per group: the handle's table, or the call's (gbad_with_mask_kernel)
  const int8_t* centres8;    // [n_blocks * 32 CT8, pitch8] fragment order (assign_quant_kernel)
  const float* par;          // [slots8] s_c, [slots8] |c|^2
  const uint32_t* max_bits;  // {a_max, b_max}
  uint32_t n_rows, pitch8, num_tiles, n_blocks;
  float gamma, under;
  u64* pairs;                      // [pair_cap] (row << 32 | centre)
  unsigned long long* pair_count;  // counts past pair_cap
  u64 pair_cap;
  u64* list;                       // rows for the listed exact pass, in no order
  uint32_t* list_count;
};

template <int METRIC, int CT8>
__global__ __launch_bounds__(512) void assign_i8_kernel(Assign8Args a) {
  constexpr bool L2 = METRIC == WDBX_METRIC_L2;
  constexpr int BA = 32 * CT8, NJ = 2 * CT8;                    // centres of a block; row groups of 16 centres
  constexpr int MAXP = CT8 == 4 ? 512 : ASSIGN8_MAX_PITCH8;     // bytes of a row this instance serves
  constexpr int PF = BA * MAXP / 16 / 512;                      // 16-byte pieces of the next block a thread carries
  static_assert(CT8 == 4 || CT8 == 2, "centre blocks of 128 and 64");
  extern __shared__ __attribute__((aligned(16))) char lds_a8[];
  const uint32_t pitch8 = a.pitch8;
  const uint32_t blk_bytes = (uint32_t)BA * pitch8;             // one centre block's bytes
  float* const spar = (float*)(lds_a8 + 2 * (size_t)blk_bytes); // [2][2][BA]: per buffer s_c, then |c|^2
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, kb = lane >> 4;
  const uint32_t steps = pitch8 / 64, pieces = blk_bytes / 16;
  const uint32_t slots8 = a.n_blocks * BA;
  if (blockIdx.x >= a.num_tiles) return;
  Assign8Call call;
  call.a_max = __uint_as_float(a.max_bits[0]);
  call.b_max = __uint_as_float(a.max_bits[1]);
  call.gamma = a.gamma;
  call.under = a.under;

  // the next centre block: global -> registers (before a k loop), registers -> the other LDS buffer (behind it)
  i32x4 pf[PF];
  float pfs = 0.f, pfc = 0.f;
  auto fetch = [&](uint32_t blk) {
    const i32x4* src = (const i32x4*)(a.centres8 + (size_t)blk * blk_bytes);
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const uint32_t e = tid + 512u * i;
      pf[i] = src[e < pieces ? e : 0];
    }
    if (tid < BA) {
      pfs = a.par[blk * BA + tid];
      pfc = a.par[slots8 + blk * BA + tid];
    }
  };
  auto stage = [&](uint32_t buf) {
    i32x4* dst = (i32x4*)(lds_a8 + (size_t)buf * blk_bytes);
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const uint32_t e = tid + 512u * i;
      if (e < pieces) dst[e] = pf[i];
    }
    if (tid < BA) {
      spar[buf * 2 * BA + tid] = pfs;
      spar[buf * 2 * BA + BA + tid] = pfc;
    }
  };
  fetch(0);
  stage(0);
  __syncthreads();
  uint32_t cur = 0;  // the LDS buffer that holds the block being computed

  // the row stream: this wave's 32 rows, k-step after k-step, block after block, tile after tile, two k-steps ahead
  uint32_t ld_tile = blockIdx.x, ld_blk = 0, ld_s = 0;
  const size_t wave_bytes = (size_t)32 * pitch8;
  const int8_t* ld_p = a.rows8 + ((size_t)ld_tile * 8 + wave) * wave_bytes + lane * 16;
  i32x4 ring[2][2];
  auto load_next = [&](int j) {
    ring[j][0] = *(const i32x4*)ld_p;
    ring[j][1] = *(const i32x4*)(ld_p + 1024);
    ld_p += 2048;
    if (++ld_s == steps) {
      ld_s = 0;
      if (++ld_blk == a.n_blocks) {
        ld_blk = 0;
        if (ld_tile + gridDim.x < a.num_tiles) ld_tile += gridDim.x;  // past the last tile: re-read it (valid memory, never used)
      }
      ld_p = a.rows8 + ((size_t)ld_tile * 8 + wave) * wave_bytes + lane * 16;
    }
  };
  load_next(0);
  load_next(1);

  for (uint32_t t = blockIdx.x; t < a.num_tiles; t += gridDim.x) {
    // ---- per (tile, wave): the group's scale, its margin, the rows that may be returned ----
    const uint32_t wrow0 = (t * 8 + wave) * 32;
    const uint32_t gidx = __builtin_amdgcn_readfirstlane(wrow0 >> 6);
    const u64 bad64 = *(const __attribute__((address_space(4))) u64*)(a.gbad + gidx);
    const uint32_t wbad = (uint32_t)(bad64 >> (wrow0 & 32u));  // this wave's 32 rows
    const f4 gt = *(const __attribute__((address_space(4))) f4*)(a.groups + gidx);
    const float margin = assign8_margin(L2, Assign8Group{gt.x, gt.y, gt.z}, call);
    const bool listed = assign8_listed(margin, gt.w);  // (wave-uniform)
    // this lane's two rows: wrow0 + 16 h + l15
    const bool ok0 = !((wbad >> l15) & 1u) && !listed, ok1 = !((wbad >> (16 + l15)) & 1u) && !listed;
    float best0 = -INFINITY, best1 = -INFINITY;

    for (uint32_t blk = 0; blk < a.n_blocks; ++blk) {
      const bool more = a.n_blocks > 1;  // (uniform) with one block the resident one serves every tile
      if (more) fetch(blk + 1 == a.n_blocks ? 0 : blk + 1);
      i32x4 acc[NJ][2];  // [centre group][row half]: centre 16 j + 4 kb + i, row 16 h + l15
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j][0] = acc[j][1] = i32x4{0, 0, 0, 0};
      const char* const cb = lds_a8 + (size_t)cur * blk_bytes + lane * 16;
      for (uint32_t s0 = 0; s0 < steps; s0 += 2) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const i32x4 rf0 = ring[jj][0], rf1 = ring[jj][1];
          const char* const cs = cb + (s0 + jj) * 2048u;
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const i32x4 cf = *(const i32x4*)(cs + (uint32_t)(j >> 1) * 32u * pitch8 + (uint32_t)(j & 1) * 1024u);
            acc[j][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(cf, rf0, acc[j][0], 0, 0, 0);
            acc[j][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(cf, rf1, acc[j][1], 0, 0, 0);
          }
          load_next(jj);
        }
      }

      // ---- the block's epilogue: T in place of D, the rows' block maxima, the running best, the candidates ----
      const float* const sp = spar + cur * 2 * BA;
      float m0 = -INFINITY, m1 = -INFINITY;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const f4 sc = *(const f4*)(sp + 16 * j + 4 * kb);
        f4 c2 = {0.f, 0.f, 0.f, 0.f};
        if constexpr (L2) c2 = *(const f4*)(sp + BA + 16 * j + 4 * kb);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float t0 = assign8_T(L2, gt.x, sc[i], acc[j][0][i], c2[i]);
          const float t1 = assign8_T(L2, gt.x, sc[i], acc[j][1][i], c2[i]);
          acc[j][0][i] = __float_as_int(t0);
          acc[j][1][i] = __float_as_int(t1);
          m0 = fmaxf(m0, t0);  // (an excluded centre's T is NaN: fmaxf passes the other operand)
          m1 = fmaxf(m1, t1);
        }
      }
      m0 = fmaxf(m0, __shfl_xor(m0, 16));
      m1 = fmaxf(m1, __shfl_xor(m1, 16));
      m0 = fmaxf(m0, __shfl_xor(m0, 32));
      m1 = fmaxf(m1, __shfl_xor(m1, 32));
      best0 = fmaxf(best0, m0);
      best1 = fmaxf(best1, m1);
      const float thr0 = ok0 ? best0 - margin : INFINITY, thr1 = ok1 ? best1 - margin : INFINITY;  // (+inf: nothing passes)
      u64 bits = 0;  // bit 8 j + 4 h + i
      // (best = -inf -- every centre so far excluded -- gives thr = -inf, which a NaN still fails; an infinite T: its row's
      // margin was not finite, the row is listed)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (__int_as_float(acc[j][0][i]) >= thr0) bits |= 1ull << (8 * j + i);
          if (__int_as_float(acc[j][1][i]) >= thr1) bits |= 1ull << (8 * j + 4 + i);
        }
      if (__any(bits != 0)) {  // (wave-uniform)
        const uint32_t cnt = (uint32_t)__popcll(bits);
        uint32_t incl = cnt;  // inclusive prefix sum over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
          if (lane >= o) incl += v;
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.pair_count, (unsigned long long)total);
        base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), 0) << 32) | (uint32_t)__shfl((int)(uint32_t)base, 0);
        u64 pos = base + (incl - cnt);
        for (u64 w = bits; w; w &= w - 1) {
          const uint32_t b = (uint32_t)__builtin_ctzll(w);
          const uint32_t row = wrow0 + 16 * ((b >> 2) & 1u) + l15, centre = blk * BA + 16 * (b >> 3) + 4 * kb + (b & 3u);
          if (pos < a.pair_cap) a.pairs[pos] = ((u64)row << 32) | centre;
          ++pos;
        }
      }
      if (more) {
        stage(cur ^ 1);   // (the other buffer: every wave left it at the previous barrier)
        __syncthreads();
        cur ^= 1;
      }
    }
    // rows the sweep does not answer for: the listed exact pass takes them against all centres
    wave_append(listed && lane < 32 && !((wbad >> lane) & 1u), (u64)(wrow0 + lane), a.list, a.list_count, a.n_rows, lane);
  }
}

typedef void (*assign_i8_fn)(Assign8Args);
static assign_i8_fn pick_assign_i8(int metric, int ct8) {
  const bool l2 = metric == WDBX_METRIC_L2;
  switch (ct8) {
    case 4: return l2 ? assign_i8_kernel<WDBX_METRIC_L2, 4> : assign_i8_kernel<WDBX_METRIC_COSINE, 4>;
    case 2: return l2 ? assign_i8_kernel<WDBX_METRIC_L2, 2> : assign_i8_kernel<WDBX_METRIC_COSINE, 2>;
    default: return nullptr;
  }
}

// ---- the exact pass over the candidates ----
struct AssignPairsArgs {
  const f4* rows;      // [n_rows, pitch4]
  const f4* centres;   // [n_centers, pitch4] prepared
  const u64* pairs;    // (row << 32 | centre)
  u64 n_pairs;
  u64* keys;           // [n_rows] zero before the launch
  int32_t* out_center; // decode
  uint32_t n_rows, pitch4;
};

// join_filter_kernel's frame: a wave takes runs of up to 64 candidates; lane i keeps candidate i's key
template <int METRIC>
__global__ __launch_bounds__(256) void assign_pairs_kernel(AssignPairsArgs a) {
  const int lane = threadIdx.x & 63;
  const u64 waves = (u64)gridDim.x * 4;
  const u64 per = (a.n_pairs + waves - 1) / waves;
  const u64 C = per < 1 ? 1 : per > 64 ? 64 : per;
  for (u64 c0 = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * C; c0 < a.n_pairs; c0 += waves * C) {
    const uint32_t nloc = (uint32_t)(a.n_pairs - c0 < C ? a.n_pairs - c0 : C);
    u64 key = 0;
    uint32_t mine = 0;
    for (uint32_t i = 0; i < nloc; ++i) {
      const u64 p = a.pairs[c0 + i];
      const uint32_t row = (uint32_t)(p >> 32), centre = (uint32_t)p;
      const float s = exact_score<METRIC>(a.rows + (size_t)row * a.pitch4, a.centres + (size_t)centre * a.pitch4, a.pitch4, (uint32_t)lane);
      if ((uint32_t)lane == i && s == s) {  // (a NaN score is no result)
        key = make_key(s + 0.0f, centre);
        mine = row;
      }
    }
    if (key) atomicMax((unsigned long long*)(a.keys + mine), (unsigned long long)key);
  }
}

__global__ __launch_bounds__(256) void assign_decode_kernel(AssignPairsArgs a) {
  for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < a.n_rows; r += gridDim.x * 256) {
    const u64 key = a.keys[r];
    a.out_center[r] = key ? (int32_t)key_row(key) : -1;
  }
}
// every row's key to "none", before the exact pass
__global__ __launch_bounds__(256) void assign_clear_kernel(AssignPairsArgs a) {
  for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < a.n_rows; r += gridDim.x * 256) a.keys[r] = 0;
}
