// host_range_batch.h -- the device-free host side of wdbx_index_range_search_batch: the route decision, the cut of a call's
// queries into tile blocks, the sizes of the block's buffers, and the bookkeeping of the blocks that end on the per-query path.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/range_batch_harness.cpp (plain g++ in the CPU suite,
// tests/test_range_batch_host.py).  No HIP, no kernel types in here.
//
// A block is a run of consecutive queries that share ONE full pass of the int8 tile kernel (gemm_i8_kernel<PHASE 1>): up to
// 256 queries, 128 where the kernel's widest query block is 128 (L2, rows beyond 384 bytes of i8).  The kernel's query block is
// 64 * ct slots wide (ct = 1, 2, 4); the slots behind the block's last query are padded queries (tau = +inf: never a pair).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr int RANGE_BATCH_MAX_BLOCK = 256;          // queries per block at most (the tile kernel's widest query block)
constexpr uint32_t RANGE_PAIR_CAP_DEFAULT = 16384;  // pairs per wave: the floor of the top-k path's sizing (two tiles' worth
                                                    // of "every row of the wave's group for every query")
constexpr uint32_t RANGE_PAIR_CAP_MIN = 64, RANGE_PAIR_CAP_MAX = 1u << 16;
// candidate + result key buffers of a block beyond this many bytes: the block is answered per query instead (64 queries per
// round there, and the fp32 scan past that)
constexpr uint64_t RANGE_BATCH_MAX_KEY_BYTES = 1ull << 30;

// candidates per query a handle keeps room for between calls (8 MiB + 8 MiB of keys per 64 slots); a call that grew past it
// releases its buffers at its end
constexpr uint32_t RANGE_BATCH_KEEP_CAP = 16384;

enum { RANGE_BATCH_NONE = 0, RANGE_BATCH_PER_QUERY = 1, RANGE_BATCH_TILES = 2, RANGE_BATCH_MIXED = 3 };

// what the route looks at (the handle's options and shape; i8_pitch = the rows' i8 image in bytes, 0 = the tiles do not
// serve this shape; shadow_fits = the i8 shadow copy is in place)
struct RangeBatchShape {
  uint64_t n_rows;
  int nq;
  int metric_l2;
  uint32_t i8_pitch;
  int shadow_fits;
  int64_t gemm_bf16, gemm8_variant, gemm_masked, gemm_min_rows, gemm_min_work, min_queries;
  int has_mask;
};

// the batched path's own row test (host_index.h::gemm_eligible without its k and query-count parts): from 2 x gemm_min_rows
// rows always; below, when gemm_min_work is off, from gemm_min_rows; else from queries x rows >= gemm_min_work (0.65 of it
// from gemm_min_rows rows)
static inline bool range_batch_rows_ok(uint64_t n_rows, int nq, int64_t min_rows, int64_t min_work) {
  if ((int64_t)n_rows >= 2 * min_rows) return true;
  if (min_work <= 0) return (int64_t)n_rows >= min_rows;
  const uint64_t work = (int64_t)n_rows >= min_rows ? (uint64_t)min_work * 13 / 20 : (uint64_t)min_work;
  return (uint64_t)nq * n_rows >= work;
}

// queries per block at most: 256, or 128 for L2 and rows beyond 384 bytes of i8; 0 = no tile instance (rows beyond 1536 bytes)
static inline int range_batch_block_queries(int metric_l2, uint32_t i8_pitch) {
  if (!i8_pitch || i8_pitch > 1536u) return 0;
  if (i8_pitch > 768u) return 64;  // (the query block must stay within 96 KiB of LDS)
  return (metric_l2 || i8_pitch > 384u) ? 128 : 256;
}

// true = the tile route
static inline bool range_batch_use_tiles(const RangeBatchShape& s) {
  if (!s.n_rows || s.n_rows >= 0xFFFFFF00ull || s.nq < 1) return false;
  if (s.gemm_bf16 != 3 || s.gemm8_variant != 0 || !s.shadow_fits) return false;
  if (s.has_mask && s.gemm_masked <= 0) return false;
  if (range_batch_block_queries(s.metric_l2, s.i8_pitch) == 0) return false;
  if ((int64_t)s.nq < s.min_queries) return false;
  return range_batch_rows_ok(s.n_rows, s.nq, s.gemm_min_rows, s.gemm_min_work);
}

struct RangeBatchBlock {
  int q0, nv;  // the block's queries [q0, q0 + nv)
  int ct;      // the kernel's query block: 64 * ct slots (1, 2 or 4)
};

// nq queries in order into blocks of at most max_block (64, 128 or 256); forced_ct = option gemm_ct (1, 2, 4; anything else:
// the narrowest query block that holds what is left, as the top-k path cuts)
static inline std::vector<RangeBatchBlock> range_batch_blocks(int nq, int max_block, int forced_ct = 0) {
  std::vector<RangeBatchBlock> out;
  if (nq < 1 || (max_block != 64 && max_block != 128 && max_block != 256)) return out;
  const int max_ct = max_block / 64;
  for (int q0 = 0; q0 < nq;) {
    const int rem = nq - q0;
    int ct = (forced_ct == 1 || forced_ct == 2 || forced_ct == 4) ? forced_ct : rem > 128 ? 4 : rem > 64 ? 2 : 1;
    ct = std::min(ct, max_ct);
    const int nv = std::min(64 * ct, rem);
    out.push_back({q0, nv, ct});
    q0 += nv;
  }
  return out;
}

// pairs per wave: option range_pair_cap (0 = the default), clamped to what the kernel's 32-bit positions and the buffer allow
static inline uint32_t range_batch_pair_cap(int64_t opt) {
  if (opt <= 0) return RANGE_PAIR_CAP_DEFAULT;
  return (uint32_t)std::min<int64_t>(std::max<int64_t>(opt, RANGE_PAIR_CAP_MIN), RANGE_PAIR_CAP_MAX);
}

// the producing waves of a full pass: 8 per workgroup, one workgroup per tile up to one per CU
static inline uint32_t range_batch_waves(uint64_t n_rows, uint32_t cus) {
  const uint64_t tiles = (n_rows + 255) / 256;
  return (uint32_t)std::min<uint64_t>(tiles, cus) * 8u;
}

struct RangeBatchSizes {
  size_t pairs_bytes, pair_count_bytes;  // [waves][pair_cap] u64, [waves] u32
  size_t cand_bytes, keys_bytes;         // [slots][cap] u64 (the scatter addresses every slot's counter), [nv][cap] u64
  size_t count_bytes;                    // candidate counters [256] + the lost flag, u32
  size_t rcnt_bytes, thr_bytes;          // result counters [256] u32; thresholds [256] exact + [256] selection, float
  size_t qb8_bytes, qpar_bytes, tau_bytes;
};
static inline RangeBatchSizes range_batch_sizes(const RangeBatchBlock& b, uint32_t cap, uint32_t pair_cap, uint32_t waves, uint32_t i8_pitch) {
  RangeBatchSizes s;
  const size_t slots = (size_t)64 * b.ct;
  s.pairs_bytes = (size_t)waves * pair_cap * sizeof(uint64_t);
  s.pair_count_bytes = (size_t)waves * sizeof(uint32_t);
  s.cand_bytes = slots * cap * sizeof(uint64_t);
  s.keys_bytes = (size_t)b.nv * cap * sizeof(uint64_t);
  s.count_bytes = ((size_t)RANGE_BATCH_MAX_BLOCK + 1) * sizeof(uint32_t);
  s.rcnt_bytes = (size_t)RANGE_BATCH_MAX_BLOCK * sizeof(uint32_t);
  s.thr_bytes = (size_t)2 * RANGE_BATCH_MAX_BLOCK * sizeof(float);
  s.qb8_bytes = slots * i8_pitch;
  s.qpar_bytes = slots * 4 * sizeof(float);
  s.tau_bytes = slots * sizeof(float);
  return s;
}
// may the candidate buffers of a block of 64 * ct slots grow to cap entries per query?  (no: the block is answered per query)
static inline bool range_batch_cap_fits(const RangeBatchBlock& b, uint64_t cap) {
  return (uint64_t)64 * b.ct * cap * sizeof(uint64_t) <= RANGE_BATCH_MAX_KEY_BYTES;
}

// what a call did, block by block
struct RangeBatchTally {
  int64_t blocks = 0, tile_blocks = 0, fallback_queries = 0, pairs = 0;
  std::vector<uint8_t> per_query;  // [nq] 1 = answered by the per-query path
  void start(int nq) {
    blocks = tile_blocks = fallback_queries = pairs = 0;
    per_query.assign((size_t)(nq > 0 ? nq : 0), 0);
  }
  void tiles(const RangeBatchBlock&, uint64_t kept_pairs) {
    ++blocks;
    ++tile_blocks;
    pairs += (int64_t)kept_pairs;
  }
  // a wave of the block's pass ran out of pair room (or its buffers may not grow): exactly the block's queries
  void lost(const RangeBatchBlock& b, uint64_t kept_pairs) {
    ++blocks;
    pairs += (int64_t)kept_pairs;
    fallback_queries += b.nv;
    for (int q = b.q0; q < b.q0 + b.nv; ++q) per_query[(size_t)q] = 1;
  }
  int path() const {
    if (!blocks) return RANGE_BATCH_NONE;
    if (!fallback_queries) return RANGE_BATCH_TILES;
    return RANGE_BATCH_MIXED;
  }
};
