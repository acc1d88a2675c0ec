// host_multivector_tiles.h -- the device-free host side of the matrix-core scoring route of wdbx_index_search_multivector
// (label_keys_tile_kernel, kernels_multivector_tiles.h): which rounds may take it, the vector blocks of a round, the instance,
// its LDS and its grid.  The rounds themselves stay multivector_plan's (host_multivector.h); the certainty bound's coefficients
// are assign_bound's (host_assign.h, DESIGN.md sections 4.20 and 4.12b).
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/multivector_tiles_harness.cpp (plain g++ in the CPU suite,
// tests/test_multivector_tiles_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "host_assign.h"
#include "host_subset.h"

constexpr int MVT_SPAN = 64;          // positions of the label order one wave owns (= LABEL_SPAN, checked where both are visible)
constexpr int MVT_WAVES = 4;          // waves (spans in flight) of a workgroup
constexpr int MVT_BK = ASSIGN_BK;     // floats of K staged per chunk ...
constexpr int MVT_LD = ASSIGN_LD;     // ... in padded LDS rows, as assign_tile_kernel's
constexpr int MVT_BLOCK_MAX = 128;    // vectors per block at most (vt = 4: 2 * 4 * 16 accumulator registers per lane)
// one workgroup per CU: its four waves' gathered rows alone are 72 KiB, so two never fit a CU's 160 KiB
constexpr size_t MVT_LDS_LIMIT = 160 * 1024;

struct MultivectorTilePlan {
  bool eligible = false;  // metric 0, an instance exists and its LDS fits the limit
  int vt = 0;             // 32-vector MFMA column tiles per block: 1, 2 or 4 (the instance)
  uint32_t block = 0;     // vectors per block = 32 * vt
  uint32_t vblocks = 0;   // grid.y: blocks [b * block, min(vectors, (b + 1) * block)), every vector of the round in exactly one
  int ni = 0;             // row_block_ni of the pitch: the form of the resolve's exact scores (the other half of the instance)
  size_t lds = 0;         // dynamic LDS: two buffers of K-chunks of (4 waves x 64 gathered rows + the block's vectors)
  uint32_t grid = 0;      // grid.x: workgroups along the spans, four spans per trip each
};

static inline int multivector_tile_vt(uint32_t vectors) { return vectors <= 32 ? 1 : vectors <= 64 ? 2 : 4; }

// the LDS bytes do not depend on the pitch: K is walked in chunks of MVT_BK floats whatever the row length
static inline size_t multivector_tile_lds(int vt) {
  return (size_t)2 * (MVT_WAVES * MVT_SPAN + 32 * vt) * MVT_LD * sizeof(float);
}

// vectors of block b of a round
static inline uint32_t multivector_tile_block_count(const MultivectorTilePlan& p, uint32_t vectors, uint32_t b) {
  return std::min<uint32_t>(p.block, vectors - b * p.block);
}

// One round of `vectors` (1 .. MULTIVECTOR_MAX_ROUND) on a handle of `metric` (0 = inner product / cosine; the L2 bound is not
// derived: the row norm varies inside an item) with rows of `pitch` floats and n_spans spans in its label order.  The grid holds
// one workgroup per CU over all vector blocks TOGETHER (what is resident at once) and never more than there are spans to take.
static inline MultivectorTilePlan multivector_tile_plan(int metric, uint32_t vectors, uint32_t pitch, uint32_t n_spans, int cu_count,
                                                        size_t lds_limit = MVT_LDS_LIMIT) {
  MultivectorTilePlan p;
  if (vectors < 1 || pitch < 4 || pitch % 4 || n_spans < 1) return p;
  p.vt = multivector_tile_vt(vectors);
  p.block = 32u * (uint32_t)p.vt;
  p.vblocks = (vectors + p.block - 1) / p.block;
  p.ni = row_block_ni(pitch / 4);
  p.lds = multivector_tile_lds(p.vt);
  const uint64_t want = std::max<uint64_t>(1, (uint64_t)std::max(cu_count, 1) / p.vblocks);
  p.grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, ((uint64_t)n_spans + MVT_WAVES - 1) / MVT_WAVES));
  p.eligible = metric == 0 && p.block <= (uint32_t)MVT_BLOCK_MAX && p.lds <= lds_limit;
  return p;
}

// option multivector_tiles: 0 never, 1 wherever the plan is eligible, -1 a round of at least min_vectors vectors
static inline bool multivector_tile_route(int64_t option, int64_t min_vectors, uint32_t vectors, const MultivectorTilePlan& p) {
  if (!p.eligible || option == 0) return false;
  return option == 1 || (int64_t)vectors >= min_vectors;
}
