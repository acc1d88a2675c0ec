// kernels_join.h -- similarity self-join (wdbx_index_self_join): every pair of stored rows whose exact score reaches a threshold.
// Part of the single translation unit wdbx_hip.hip (included there, in order); not a standalone header.
//
//   join_tile_kernel    the sweep.  BOTH operands are shadow copy G of kernels_tiles8.h (signed bytes, one scale per 64-row
//                       group, MFMA fragment order) on v_mfma_i32_16x16x64_i8:
//     * an ANCHOR BLOCK of 32 * CT8 consecutive rows (128 up to 768 bytes of a row, 64 up to 1536: at most 96 KiB) is copied VERBATIM
//       from G into LDS: a 1 KiB A fragment of G is a valid B fragment as it lies (lane l owns the 16 bytes at 16 l, the same
//       k order on both sides), so there is no quantiser, no swizzle and no fp32 staging, and every B fragment read is one
//       contiguous, conflict-free ds_read_b128 at  lane * 16 + constant;
//     * the CANDIDATE rows stream as in gemm_i8_kernel: 8 waves, each owning 32 rows of a 256-row tile (64 accumulators
//       against 128 anchors), fragments from HBM straight into a register ring, no barrier in the k loop;
//     * the TRIANGLE: the workgroup of anchor block i starts at the tile that holds its own rows and runs to the last one; a
//       hit with row <= anchor is cleared.  Blocks are handed out longest first by an integer ticket (block 0 streams every
//       tile, the last block one), so a persistent grid of one workgroup per CU ends together; the answer does not depend on
//       who took which block: pairs are sorted behind the exact pass;
//     * the EPILOGUE is an integer compare: a wave's 32 rows lie in one 64-row group, a column group of 16 anchors in one
//       anchor group, so per (tile, wave) there are at most 2 thresholds T_AB (join_cut, host_join.h), computed once from the
//       two group-table entries, and the test is D >= T_AB.  L2 adds the two cached norms: one convert and one fma per
//       accumulator (join_l2_keep).  Rows whose bad-row bit is set (removed, past the end, masked out: the call's table) are
//       cleared on both sides before anything is appended;
//     * hits are rare: a wave appends (anchor << 32 | row) to ONE global buffer with one integer atomic per tile with hits
//       (per-lane counts, a wave prefix sum, positions); the counter counts past the buffer, the host grows it and sweeps again.
//   join_filter_kernel  the exact pass, range_filter_kernel's frame: a wave takes a run of candidate pairs, scores (stored row a
//                       as the query, row b) with exact_score, applies the caller's threshold and compacts (anchor, key).
// No floating-point atomics anywhere.
#include "host_join.h"

struct JoinArgs {
  const int8_t* rows8;   // shadow copy G: fragment-ordered blocks, whole tiles
  const f4* groups;      // {s_g, a_g, b_g, vouch} per 64-row group
  const u64* gbad;       // bad-row bits per group: the handle's table, or the call's (gbad_with_mask_kernel)
  const float* cn;       // L2: squared fp32 norm per row
  uint32_t n_rows, pitch8;
  uint32_t num_tiles, num_blocks;
  float thr;
  u64* pairs;                      // [pair_cap] (anchor << 32 | row)
  unsigned long long* pair_count;  // counts past pair_cap
  uint32_t* ticket;                // the next anchor block
  u64 pair_cap;
};

template <int METRIC, int CT8, int PITCH8>
__global__ __launch_bounds__(512) void join_tile_kernel(JoinArgs a) {
  constexpr bool L2 = METRIC == WDBX_METRIC_L2;
  constexpr int BA = 32 * CT8, NJ = 2 * CT8;        // anchors of a block; column groups of 16 anchors
  constexpr int NG = CT8 >= 2 ? CT8 / 2 : 1;        // 64-row groups of an anchor block
  constexpr int RING = PITCH8 == 384 ? 3 : PITCH8 == 768 ? 6 : 2;  // k-steps in flight: a divisor of pitch8 / 64
  static_assert(CT8 == 4 || CT8 == 2, "anchor blocks of 128 and 64 rows (a 256-row block's epilogue does not fit the registers)");
  constexpr int W = NJ < 8 ? NJ : 8;                // anchor fragments in flight
  constexpr int NW = (NJ + 3) / 4;                  // words of a lane's packed hit bits: 8 rows x 4 column groups each
  extern __shared__ __attribute__((aligned(16))) char lds_join[];
  __shared__ uint32_t s_block;
  const uint32_t pitch8 = PITCH8 ? (uint32_t)PITCH8 : a.pitch8;
  float* const an = (float*)(lds_join + (size_t)BA * pitch8);  // [BA] the anchors' norms, taken low (L2)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, kb = lane >> 4;
  const uint32_t steps = pitch8 / 64;
  const size_t blk_bytes = (size_t)32 * pitch8;

  for (;;) {
    // ---- the next anchor block: longest first ----
    if (tid == 0) s_block = atomicAdd(a.ticket, 1u);
    __syncthreads();  // (also: every wave is done with the previous block's fragments)
    const uint32_t blk = __builtin_amdgcn_readfirstlane(s_block);
    if (blk >= a.num_blocks) return;
    {
      const i32x4* src = (const i32x4*)(a.rows8 + (size_t)blk * BA * pitch8);
      for (uint32_t e = tid; e < (uint32_t)BA * (pitch8 / 16); e += 512) ((i32x4*)lds_join)[e] = src[e];
      if constexpr (L2) {
        for (uint32_t r = tid; r < (uint32_t)BA; r += 512) {
          const uint32_t row = blk * BA + r;
          an[r] = join_norm_low(a.cn[row < a.n_rows ? row : a.n_rows - 1]);
        }
      }
    }
    __syncthreads();
    const uint32_t arow0 = blk * BA;     // the block's first anchor
    const uint32_t agrp0 = arow0 >> 6;   // ... and its first group
    const uint32_t t0 = arow0 / G8_ROWS;

    // ---- the candidate stream: this wave's 32 rows of tile after tile, k-step after k-step, RING ahead ----
    uint32_t ld_tile = t0, ld_s = 0;
    const int8_t* ld_p = a.rows8 + ((size_t)ld_tile * 8 + wave) * blk_bytes + lane * 16;
    i32x4 ring[RING][2];
    auto load_next = [&](int j) {
      ring[j][0] = __builtin_nontemporal_load((const i32x4*)ld_p);
      ring[j][1] = __builtin_nontemporal_load((const i32x4*)(ld_p + 1024));
      ld_p += 2048;
      if (++ld_s == steps) {
        ld_s = 0;
        if (ld_tile + 1 < a.num_tiles) ++ld_tile;  // past the last tile: re-read it (valid memory, never used)
        ld_p = a.rows8 + ((size_t)ld_tile * 8 + wave) * blk_bytes + lane * 16;
      }
    };
#pragma unroll
    for (int j = 0; j < RING; ++j) load_next(j);

    // anchor fragment of k-step `step`, column group j: the block lies in LDS as it lies in G
    auto b_base = [&](uint32_t step) -> uint32_t {
      uint32_t addr = (uint32_t)lane * 16 + (PITCH8 ? 0u : step * 2048u);
      asm volatile("" : "+v"(addr));  // (opaque per k-step: the block's fragments must not be hoisted out of the tile loop)
      return addr;
    };
    auto b_read = [&](uint32_t step, int j, uint32_t base) -> i32x4 {
      const uint32_t off = (uint32_t)(j >> 1) * 32u * pitch8 + (uint32_t)(j & 1) * 1024u + (PITCH8 ? step * 2048u : 0u);
      return *(const i32x4*)(lds_join + base + off);
    };
    i32x4 acc[NJ][2];  // [column group][row half]: rows 16 h + 4 kb + i, anchor 16 j + l15
    i32x4 bf[W];
    uint32_t tb = b_base(0);
#pragma unroll
    for (int j = 0; j < W; ++j) bf[j] = b_read(0, j, tb);

    for (uint32_t t = t0; t < a.num_tiles; ++t) {
      auto trip = [&](auto first_tag, uint32_t s0) {
#pragma unroll
        for (int jj = 0; jj < RING; ++jj) {
          const uint32_t sn = s0 + jj + 1 == steps ? 0 : s0 + jj + 1;  // the next k-step (of the next tile at the end)
          const uint32_t tbn = b_base(sn);
          const i32x4 af0 = ring[jj][0], af1 = ring[jj][1];
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            if (decltype(first_tag)::value && jj == 0) {
              const i32x4 zero = {0, 0, 0, 0};
              acc[j][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af0, bf[j % W], zero, 0, 0, 0);
              acc[j][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af1, bf[j % W], zero, 0, 0, 0);
            } else {
              acc[j][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af0, bf[j % W], acc[j][0], 0, 0, 0);
              acc[j][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af1, bf[j % W], acc[j][1], 0, 0, 0);
            }
            if (j + W < NJ) bf[j % W] = b_read(s0 + jj, j + W, tb);
            else bf[j % W] = b_read(sn, j + W - NJ, tbn);
          }
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
          }
          __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);    // VMEM read: the ring's loads stay here
          load_next(jj);
          tb = tbn;
        }
      };
      if constexpr (PITCH8 != 0) {
        trip(std::true_type{}, 0);
#pragma unroll
        for (uint32_t s0 = RING; s0 < (uint32_t)(PITCH8 / 64); s0 += RING) trip(std::false_type{}, s0);
      } else {
        trip(std::true_type{}, 0);
        for (uint32_t s0 = RING; s0 < steps; s0 += RING) trip(std::false_type{}, s0);
      }

      // ---- the tile's epilogue: this wave's 32 rows (one group B) against the block's NG groups A ----
      const uint32_t wrow0 = (t * 8 + wave) * 32;
      const uint32_t gidx = __builtin_amdgcn_readfirstlane(wrow0 >> 6);
      const u64 cbad64 = *(const __attribute__((address_space(4))) u64*)(a.gbad + gidx);
      const uint32_t cbad = (uint32_t)(cbad64 >> (wrow0 & 32u));  // this wave's 32 rows
      if (cbad == 0xFFFFFFFFu) continue;                          // (wave-uniform) none of them may be returned
      const f4 gt = *(const __attribute__((address_space(4))) f4*)(a.groups + gidx);
      JoinCut cut[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const f4 ga = *(const __attribute__((address_space(4))) f4*)(a.groups + agrp0 + g);
        cut[g] = join_cut(L2, a.thr, JoinGroup{ga.x, ga.y, ga.z}, JoinGroup{gt.x, gt.y, gt.z});
      }
      const uint32_t lrow0 = wrow0 + 4 * kb;  // this lane's rows: lrow0 + 16 h + i
      float ub[L2 ? 8 : 1];
      if constexpr (L2) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const uint32_t row = lrow0 + 16 * (r >> 2) + (r & 3);
          ub[r] = join_norm_low(a.cn[row < a.n_rows ? row : a.n_rows - 1]);
        }
      }
      // (L2: col = the threshold of this lane's anchor column of group j, computed where it is used, not kept in NJ registers)
      auto column = [&](int j) -> float { return L2 ? join_l2_col(an[16 * j + l15], cut[j >> 2]) : 0.f; };
      auto test = [&](int j, int r, float col) -> bool {
        if constexpr (L2) return join_l2_keep(acc[j][r >> 2][r & 3], ub[r], cut[j >> 2], col);
        else return acc[j][r >> 2][r & 3] >= cut[j >> 2].T;
      };
      bool hit = false;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if constexpr (L2) {
          const float col = column(j);
#pragma unroll
          for (int r = 0; r < 8; ++r) hit = hit || test(j, r, col);
        } else {
          int m = max(max(acc[j][0][0], acc[j][0][1]), max(acc[j][0][2], acc[j][0][3]));
          m = max(m, max(max(acc[j][1][0], acc[j][1][1]), max(acc[j][1][2], acc[j][1][3])));
          hit = hit || m >= cut[j >> 2].T;
        }
      }
      if (!__any(hit)) continue;  // (wave-uniform) the common case

      // rare: which (anchor, row) of this lane, packed 8 rows x 4 column groups per word; the triangle, the end of the rows
      // and both sides' bad rows are cleared here
      uint32_t pk[NW];
      uint32_t cnt = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) pk[w] = 0;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const uint32_t anchor = arow0 + 16 * j + l15;
        const u64 abad = *(const __attribute__((address_space(4))) u64*)(a.gbad + agrp0 + (j >> 2));
        const bool a_ok = !((abad >> ((16 * j + l15) & 63)) & 1ull);
        const float col = column(j);
        uint32_t bits = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const uint32_t lr = 16 * (r >> 2) + (r & 3);
          const uint32_t row = lrow0 + lr;
          if (test(j, r, col) && row > anchor && row < a.n_rows && !((cbad >> (4 * kb + lr)) & 1u)) bits |= 1u << r;
        }
        if (!a_ok) bits = 0;
        pk[j >> 2] |= bits << (8 * (j & 3));
        cnt += (uint32_t)__builtin_popcount(bits);
      }
      uint32_t incl = cnt;  // inclusive prefix sum over the wave
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, o);
        if (lane >= o) incl += v;
      }
      const uint32_t total = (uint32_t)__shfl((int)incl, 63);
      if (total == 0) continue;  // (the diagonal: only self and mirrored hits)
      unsigned long long base = 0;
      if (lane == 0) base = atomicAdd(a.pair_count, (unsigned long long)total);
      base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), 0) << 32) | (uint32_t)__shfl((int)(uint32_t)base, 0);
      u64 pos = base + (incl - cnt);
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        for (uint32_t word = pk[w]; word; word &= word - 1) {
          const uint32_t b = (uint32_t)__builtin_ctz(word);
          const uint32_t j = 4 * w + (b >> 3), r = b & 7;
          const uint32_t anchor = arow0 + 16 * j + l15, row = lrow0 + 16 * (r >> 2) + (r & 3);
          if (pos < a.pair_cap) a.pairs[pos] = ((u64)anchor << 32) | row;
          ++pos;
        }
      }
    }
  }
}

// ---- instances and launch ----
typedef void (*join_tile_fn)(JoinArgs);
// (No 256-anchor instance: with 128 accumulators the epilogue's hit path does not fit 256 registers without scratch in any form
// that was compiled -- ring 3 or 2, window 8 or 4, compile-time or run-time pitch: 16 to 104 bytes per lane.  DESIGN.md 4.23.)
static join_tile_fn pick_join_tile(int metric, int ct8, uint32_t pitch8) {
  constexpr int C = WDBX_METRIC_COSINE, L = WDBX_METRIC_L2;
  const bool l2 = metric == WDBX_METRIC_L2;
  switch (ct8) {
    case 4:
      if (pitch8 == 384) return l2 ? join_tile_kernel<L, 4, 384> : join_tile_kernel<C, 4, 384>;
      if (pitch8 == 768) return l2 ? join_tile_kernel<L, 4, 768> : join_tile_kernel<C, 4, 768>;
      return l2 ? join_tile_kernel<L, 4, 0> : join_tile_kernel<C, 4, 0>;
    case 2: return l2 ? join_tile_kernel<L, 2, 0> : join_tile_kernel<C, 2, 0>;
    default: return nullptr;
  }
}

// ---- the exact pass ----
struct JoinFilterArgs {
  const f4* rows;          // [n_rows, pitch4] quads
  const u64* pairs;        // (anchor << 32 | row)
  u64 n_pairs;
  const uint32_t* mask;    // optional row filter
  float thr;
  uint32_t pitch4;
  u64* out_keys;           // [cap] (score, row) as make_key
  uint32_t* out_anchor;    // [cap] the key's anchor
  uint32_t* count;
  uint32_t cap;
};

template <int METRIC>
__global__ __launch_bounds__(256) void join_filter_kernel(JoinFilterArgs a) {
  const int lane = threadIdx.x & 63;
  const u64 waves = (u64)gridDim.x * 4;
  const u64 per = (a.n_pairs + waves - 1) / waves;
  const u64 C = per < 1 ? 1 : per > 64 ? 64 : per;  // candidates per wave and trip, as range_filter_kernel spreads them
  for (u64 c0 = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * C; c0 < a.n_pairs; c0 += waves * C) {
    const uint32_t nloc = (uint32_t)(a.n_pairs - c0 < C ? a.n_pairs - c0 : C);
    bool keep = false;
    u64 key = 0;
    uint32_t anchor = 0;
    for (uint32_t i = 0; i < nloc; ++i) {
      const u64 p = a.pairs[c0 + i];
      const uint32_t ar = (uint32_t)(p >> 32), row = (uint32_t)p;
      const float s = exact_score<METRIC>(a.rows + (size_t)row * a.pitch4, a.rows + (size_t)ar * a.pitch4, a.pitch4, (uint32_t)lane);
      if ((uint32_t)lane == i) {
        keep = range_pass<METRIC>(s, a.thr) && ar < row &&
               (!a.mask || (((a.mask[ar >> 5] >> (ar & 31)) & (a.mask[row >> 5] >> (row & 31))) & 1u));
        key = make_key(s + 0.0f, row);
        anchor = ar;
      }
    }
    // wave_append's positions for two arrays: one atomic per wave
    const u64 bal = __ballot(keep);
    if (!bal) continue;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    const int leader = __ffsll((long long)bal) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(a.count, (uint32_t)__popcll(bal));
    base = (uint32_t)__shfl((int)base, leader);
    if (keep && base + rank < a.cap) {
      a.out_keys[base + rank] = key;
      a.out_anchor[base + rank] = anchor;
    }
  }
}
