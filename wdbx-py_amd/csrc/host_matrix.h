// host_matrix.h -- the device-free host side of wdbx_index_search_matrix: the plan of a distance matrix among listed rows.
// The anchors are the listed rows themselves, so the call is wdbx_index_search_rows' plan with n_ids "queries": route, anchor
// block, grid and a round's scratch are subset_plan's (host_subset.h), called as it is; what is added here is the instance
// (NI, sink) and the rounds.  List validation and the narrowing to 32 bits are subset_validate's.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/matrix_harness.cpp (plain g++ in the CPU suite,
// tests/test_matrix_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>

#include "host_subset.h"

// anchors of one round at most: a round is one scoring launch and one ranking launch (one per anchor on the select route)
constexpr int MATRIX_ROUND_MAX = 256;
// listed rows of one call at most: the anchors are the ranking tail's slots, which are ints
constexpr uint64_t MATRIX_MAX_IDS = (uint64_t)INT_MAX;

struct MatrixPlan {
  SubsetPlan sp;         // route (SUBSET_*: read-only option "last_matrix_path"), qb = anchors per block, round = anchors per
                         // round, blocks = grid.x, P, lds, scratch_u64 of a full round
  int ni = 0;            // row_block_ni of the pitch: the loads per lane of a candidate row and of an anchor
  int mode = 2;          // matrix_kernel's MODE: 0 lists in LDS, 1 lists in registers, 2 a key per (anchor, listed row)
  uint64_t rounds = 0;   // consecutive anchors [r * round, min(n_ids, (r + 1) * round))
  size_t scratch_bytes = 0;  // of the worst (= a full) round
};

// anchors of round r and the list position of its first
static inline uint64_t matrix_round_first(const MatrixPlan& p, uint64_t r) { return r * (uint64_t)p.sp.round; }
static inline int matrix_round_anchors(const MatrixPlan& p, uint64_t n_ids, uint64_t r) {
  return (int)std::min<uint64_t>((uint64_t)p.sp.round, n_ids - matrix_round_first(p, r));
}
// grid.y of a round of b anchors
static inline uint32_t matrix_anchor_blocks(const MatrixPlan& p, int b) { return (uint32_t)((b + p.sp.qb - 1) / p.sp.qb); }

// n_ids <= MATRIX_MAX_IDS (the entry point refuses more).  keys_max / select_min_k / lds_lists: options rows_keys_max,
// select_min_k and lds_lists, as subset_plan takes them.
static inline MatrixPlan matrix_plan(uint64_t n_ids, int k, uint32_t pitch4, int cu_count, int64_t keys_max, int64_t select_min_k,
                                     bool lds_lists) {
  MatrixPlan p;
  p.ni = row_block_ni(pitch4);
  p.sp = subset_plan(n_ids, (int)std::min<uint64_t>(n_ids, MATRIX_MAX_IDS), k, cu_count, keys_max, select_min_k, lds_lists);
  if (p.sp.route == SUBSET_NONE) return p;
  static_assert(MATRIX_ROUND_MAX == 256, "subset_plan's rounds are the rounds of this call");
  p.mode = p.sp.route == SUBSET_LISTS ? (k <= 128 && !lds_lists ? 1 : 0) : 2;
  p.rounds = (n_ids + (uint64_t)p.sp.round - 1) / (uint64_t)p.sp.round;
  p.scratch_bytes = p.sp.scratch_u64 * sizeof(uint64_t);
  return p;
}
