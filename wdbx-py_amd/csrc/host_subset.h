// host_subset.h -- the device-free host side of wdbx_index_search_rows: validation of the caller's row list and its narrowing
// to the 32-bit row numbers the device walks, the choice of the route and of the query block, grid and partial-list sizing.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/subset_harness.cpp (plain g++ in the CPU suite,
// tests/test_search_rows_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>

// loads per lane of a gathered row in every kernel built on kernels_rowblock.h: 2 up to 128 quads, 4 up to 256, 0 = the loop
constexpr int row_block_ni(uint32_t pitch4) { return pitch4 <= 128 ? 2 : pitch4 <= 256 ? 4 : 0; }
// f(std::integral_constant<int, NI>()) for that value: a picker instantiates its kernel with NI = decltype(ni)::value
template <typename F>
static inline auto with_row_block_ni(uint32_t pitch4, F f) {
  switch (row_block_ni(pitch4)) {
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 0>());
  }
}

// The list must be strictly increasing row numbers below n_rows (so every key of the call is unique, which the merges rely
// on, and one pass validates it).  Returns n_ids when the list is valid, else the index of the first offending entry.
// out32 (may be null: validation only) receives the rows narrowed to 32 bits; n_rows is below 2^32 - 256 for every index
// (32-bit row keys), so a valid entry always fits -- an entry at or above 2^32 is out of range like any other.
static inline uint64_t subset_validate(const uint64_t* row_ids, uint64_t n_ids, uint64_t n_rows, uint32_t* out32) {
  uint64_t prev = 0;
  for (uint64_t i = 0; i < n_ids; ++i) {
    const uint64_t r = row_ids[i];
    if (r >= n_rows || r > 0xFFFFFFFFull || (i && r <= prev)) return i;
    if (out32) out32[i] = (uint32_t)r;
    prev = r;
  }
  return n_ids;
}

// Routes of a call (read-only option "last_rows_path"):
//   KEYS    every listed row's key per query into a buffer, ranked by merge_kernel as unsorted candidates (list_len = 1):
//           short lists, whatever k is
//   LISTS   per-workgroup sorted lists of k keys, merged by merge_kernel like the fp32 scan's partial lists
//   SELECT  a key per listed row and query, then the radix-select chain per query: k in the select range on a long list
enum { SUBSET_NONE = 0, SUBSET_KEYS = 1, SUBSET_LISTS = 2, SUBSET_SELECT = 3 };

// keys_max: option rows_keys_max (lists up to this length take KEYS); select_min_k: option select_min_k (0 = never)
static inline int subset_route(uint64_t n_ids, int k, int64_t keys_max, int64_t select_min_k) {
  if (n_ids == 0) return SUBSET_NONE;
  if (keys_max > 0 && n_ids <= (uint64_t)keys_max) return SUBSET_KEYS;
  if (select_min_k > 0 && k >= select_min_k) return SUBSET_SELECT;
  return SUBSET_LISTS;
}

// Queries that share one fetch of a row (one grid row per block of them).  A lone query is the block of one; the key routes
// keep no list, so always 8; with lists: 8 up to k = 64 (one register of keys per query), 4 up to k = 128 (two), 1 beyond
// that (lists in LDS, or in registers when lds_lists keeps k <= 128 there too -- the block of one serves both).
static inline int subset_query_block(int route, int nq, int k, bool lds_lists) {
  if (nq <= 1) return 1;
  if (route != SUBSET_LISTS) return 8;
  if (k > 128 || lds_lists) return 1;
  return k <= 64 ? 8 : 4;
}

struct SubsetPlan {
  int route = SUBSET_NONE;
  int qb = 1;            // queries per query block
  int round = 1;         // queries per round of launches (a multiple of qb unless it is the whole call)
  uint32_t blocks = 1;   // grid.x: workgroups of four waves along the list
  uint32_t P = 0;        // LISTS: partial lists per query (= blocks: the four wave lists are merged in the workgroup)
  size_t lds = 0;        // LISTS: dynamic LDS of the scoring kernel (the lists, or the hand-over area of the register lists)
  size_t scratch_u64 = 0;  // u64s of scratch per round: partial lists (LISTS) or keys (KEYS, SELECT)
};

// dynamic LDS of subset_kernel's list instances: a list of k keys per wave and query of the block (four waves)
static inline size_t subset_lists_lds(int qb, int k) { return (size_t)4 * qb * k * sizeof(uint64_t); }

// cu_count: compute units; the grid holds about two workgroups per CU over all query blocks (eight waves per CU, each with
// several rows' loads in flight) and never more waves than listed rows.  A round's scratch stays within 256 MiB.
static inline SubsetPlan subset_plan(uint64_t n_ids, int nq, int k, int cu_count, int64_t keys_max, int64_t select_min_k,
                                     bool lds_lists) {
  SubsetPlan p;
  p.route = subset_route(n_ids, k, keys_max, select_min_k);
  if (p.route == SUBSET_NONE || nq < 1) return p;
  p.qb = subset_query_block(p.route, nq, k, lds_lists);
  const uint64_t budget = (256ull << 20) / sizeof(uint64_t);
  int round = std::min(nq, 256);
  if (p.route != SUBSET_LISTS) {
    const uint64_t fit = std::max<uint64_t>(1, budget / n_ids);
    if ((uint64_t)round > fit) round = (int)fit;
    if (round < p.qb) p.qb = 1;  // (a key per row for eight queries does not fit: one query at a time)
  }
  if (round < nq) round = std::max(p.qb, round / p.qb * p.qb);
  p.round = round;
  const uint32_t qblocks = (uint32_t)((round + p.qb - 1) / p.qb);
  const uint64_t want = std::max<uint64_t>(1, ((uint64_t)cu_count * 2 + qblocks - 1) / qblocks);
  p.blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (n_ids + 3) / 4));
  if (p.route == SUBSET_LISTS) {
    p.P = p.blocks;
    p.lds = subset_lists_lds(p.qb, k);
    p.scratch_u64 = (size_t)round * k * p.P;
  } else {
    p.scratch_u64 = (size_t)round * n_ids;
  }
  return p;
}
