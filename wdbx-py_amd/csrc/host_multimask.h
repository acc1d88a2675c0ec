// host_multimask.h -- the device-free host side of wdbx_index_search_multimask: where each query of a call with one row mask
// PER QUERY sits in the int8 tile kernel's query blocks.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/multimask_harness.cpp (plain g++ in the CPU suite,
// tests/test_multimask_host.py).  No HIP, no kernel types in here.
//
// The tile kernel's column group j holds the 16 queries 16 j .. 16 j + 15 and is wave-uniform; everything a row mask does in
// that kernel hangs off one wave-uniform word per tile.  So a call may carry several masks as long as ALL 16 QUERIES OF A
// COLUMN GROUP SHARE ONE MASK: the word becomes a scalar per column group.  This header does that placement:
//   * a query's CLASS is its entry of query_mask: -1 (every row) or the index of one of the call's masks;
//   * classes ascend (-1 first), the queries of a class keep the caller's order;
//   * every class is padded to whole column groups: at most 15 pad slots per class (they follow its last query);
//   * column groups are packed, in that order, into blocks of at most block_slots slots (256, or 128 where the kernel's
//     widest query block is 128: L2, long rows); a class larger than a block simply spans blocks.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

constexpr int MULTIMASK_GROUP = 16;  // queries per column group of the int8 tile kernel

struct MultimaskPlan {
  std::vector<int32_t> slot_query;    // [16 * groups] the caller's query in that slot, -1 = a pad slot
  std::vector<int32_t> group_class;   // [groups] the class of the column group's 16 slots
  std::vector<uint32_t> block_group;  // [blocks + 1] first column group of each block, then the number of groups
  std::vector<int32_t> classes;       // the distinct classes of the call, ascending (-1 first when present)
  uint32_t groups() const { return (uint32_t)group_class.size(); }
  uint32_t blocks() const { return block_group.empty() ? 0u : (uint32_t)block_group.size() - 1u; }
};

// false: nq < 1, n_masks < 0, block_slots no positive multiple of 16, or an entry of query_mask outside [-1, n_masks)
// (*bad_query, when given, receives that entry's position; nq for the other refusals).
static inline bool multimask_plan(const int32_t* query_mask, int nq, int n_masks, int block_slots, MultimaskPlan* out, int* bad_query = nullptr) {
  if (bad_query) *bad_query = nq;
  if (!query_mask || !out || nq < 1 || n_masks < 0 || block_slots < MULTIMASK_GROUP || block_slots % MULTIMASK_GROUP) return false;
  // (classes as 0 .. n_masks: class c sits at c + 1)
  std::vector<uint32_t> count((size_t)n_masks + 1, 0u);
  for (int q = 0; q < nq; ++q) {
    const int32_t c = query_mask[q];
    if (c < -1 || c >= n_masks) {
      if (bad_query) *bad_query = q;
      return false;
    }
    ++count[(size_t)(c + 1)];
  }
  out->slot_query.clear();
  out->group_class.clear();
  out->block_group.clear();
  out->classes.clear();
  std::vector<size_t> next((size_t)n_masks + 1, 0);  // the class's next free slot
  size_t slots = 0;
  for (int c = 0; c <= n_masks; ++c) {
    if (!count[(size_t)c]) continue;
    out->classes.push_back(c - 1);
    next[(size_t)c] = slots;
    const size_t g = (count[(size_t)c] + MULTIMASK_GROUP - 1) / MULTIMASK_GROUP;
    out->group_class.insert(out->group_class.end(), g, c - 1);
    slots += g * MULTIMASK_GROUP;
  }
  out->slot_query.assign(slots, -1);
  for (int q = 0; q < nq; ++q) out->slot_query[next[(size_t)(query_mask[q] + 1)]++] = q;  // (stable: caller order inside a class)
  const uint32_t per_block = (uint32_t)(block_slots / MULTIMASK_GROUP), groups = out->groups();
  for (uint32_t g = 0; g < groups; g += per_block) out->block_group.push_back(g);
  out->block_group.push_back(groups);
  return true;
}
