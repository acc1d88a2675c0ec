// host_rowlists.h -- the device-free host side of wdbx_index_search_row_lists: a batched search among listed rows with one
// row list PER QUERY.  The lists come as a CSR pair (every list back to back, offsets) plus query_list[nq]; this header checks
// that pair, decides each list's route, puts the queries in list order and cuts the call into the work items that
// rowlists_kernel (kernels_rowlists.h) runs, one workgroup each.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/rowlists_harness.cpp (plain g++ in the CPU suite,
// tests/test_row_lists_host.py).  No HIP, no kernel types in here.
//
//   * ROUTE of a list: at most keys_max rows (option rows_keys_max) -> the batched pass below; longer, or keys_max = 0 -> its
//     queries go through wdbx_index_search_rows' own code, list by list.  A list no query names has no route.
//   * SLOTS: the queries of the pass ordered by list, the caller's order kept inside a list (stable).  The host permutes the
//     queries into slot order before the upload and the results back after the download.
//   * ROUNDS: consecutive slots, at most 256 of them and at most 256 MiB of keys (slots x stride x 8 bytes, stride = the
//     longest list of the round; a single slot is always allowed).  A round is one scoring and one ranking launch.
//   * QUERY BLOCKS: inside a round the slots of one list are cut into blocks of qb queries (the last may be short); qb = 8,
//     or 1 when no list of the pass has more than one query.  A block never mixes lists.
//   * CHUNKS: a list is cut into chunks of ROWLISTS_CHUNK listed rows (the last may be short).
//   * WORK ITEM: one (chunk, query block) pair.  Items of one chunk are neighbours, so the blocks that share its rows run
//     close together.  An empty list has slots and no items: its keys are never written and its length 0 ranks nothing.
// ROWLISTS_CHUNK = 256: a workgroup is four waves of one row each, so a chunk is 64 rows per wave -- the block's 8 query
// loads are 8 / 256 = 3 % of the row bytes the item reads, and a 100-row list still gives every wave 25 rows.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_subset.h"

constexpr uint32_t ROWLISTS_CHUNK = 256;
constexpr int ROWLISTS_QB = 8;
constexpr uint32_t ROWLISTS_ROUND_SLOTS = 256;
constexpr uint64_t ROWLISTS_ROUND_KEY_BYTES = 256ull << 20;

enum { ROWLISTS_ROUTE_UNUSED = 0, ROWLISTS_ROUTE_PASS = 1, ROWLISTS_ROUTE_FALLBACK = 2 };

// (the kernel reads this struct as it is: five 32-bit words)
struct RowListsItem {
  uint32_t first;   // first entry in the uploaded id array (the pass lists' rows back to back)
  uint32_t n;       // entries of the chunk, 1 .. ROWLISTS_CHUNK
  uint32_t slot;    // first slot of the query block, counted from the round's first slot
  uint32_t nq;      // queries of the block, 1 .. qb
  uint32_t offset;  // the chunk's first entry inside its list: key (slot + b, offset + i) = keys[(slot + b) * stride + offset + i]
};

struct RowListsRound {
  uint32_t slot0 = 0, slots = 0;  // the round's slots [slot0, slot0 + slots)
  size_t item0 = 0, items = 0;    // its work items
  uint64_t stride = 1;            // keys per slot: the longest list of the round, at least 1
};

struct RowListsPlan {
  int qb = 1;
  std::vector<uint8_t> list_route;     // [n_lists] ROWLISTS_ROUTE_*
  std::vector<uint64_t> list_base;     // [n_lists] PASS lists: where the list starts in the uploaded id array
  uint64_t pass_ids = 0;               // entries of the uploaded id array
  std::vector<int32_t> slot_query;     // [slots] the caller's query in that slot
  std::vector<uint32_t> slot_len;      // [slots] the length of its list
  std::vector<int32_t> fallback_lists; // the lists that go through the per-list code, ascending
  std::vector<RowListsItem> items;
  std::vector<RowListsRound> rounds;
  // what last_lists_path reports: 0 nothing launched, 1 the batched pass only, 2 both, 3 list by list only
  int path() const { return fallback_lists.empty() ? (items.empty() ? 0 : 1) : (items.empty() ? 3 : 2); }
};

// The CSR pair and query_list alone (no row is looked at): 0 = fine, else what to refuse, with *where = the offending position.
enum { ROWLISTS_OK = 0, ROWLISTS_BAD_ARG = 1, ROWLISTS_BAD_OFFSET = 2, ROWLISTS_BAD_QUERY = 3 };

static inline int rowlists_check(const uint64_t* list_offsets, int n_lists, const int32_t* query_list, int nq, int64_t* where) {
  if (where) *where = -1;
  if (!list_offsets || !query_list || n_lists < 1 || nq < 1) return ROWLISTS_BAD_ARG;
  if (list_offsets[0] != 0) return where ? (*where = 0, ROWLISTS_BAD_OFFSET) : ROWLISTS_BAD_OFFSET;
  for (int l = 0; l < n_lists; ++l)
    if (list_offsets[l + 1] < list_offsets[l]) return where ? (*where = l + 1, ROWLISTS_BAD_OFFSET) : ROWLISTS_BAD_OFFSET;
  for (int q = 0; q < nq; ++q)
    if (query_list[q] < 0 || query_list[q] >= n_lists) return where ? (*where = q, ROWLISTS_BAD_QUERY) : ROWLISTS_BAD_QUERY;
  return ROWLISTS_OK;
}

// Every list strictly increasing and below n_rows (subset_validate per list).  true = all valid; else *bad_list / *bad_entry
// name the first offending list and its first offending entry.  ids32 (may be null) receives the rows of the PASS lists of
// plan, narrowed, at their list_base.
static inline bool rowlists_validate(const uint64_t* list_rows, const uint64_t* list_offsets, int n_lists, uint64_t n_rows,
                                     const RowListsPlan* plan, uint32_t* ids32, int* bad_list, uint64_t* bad_entry) {
  for (int l = 0; l < n_lists; ++l) {
    const uint64_t len = list_offsets[l + 1] - list_offsets[l];
    uint32_t* out = nullptr;
    if (ids32 && plan && plan->list_route[(size_t)l] == ROWLISTS_ROUTE_PASS) out = ids32 + plan->list_base[(size_t)l];
    const uint64_t bad = subset_validate(list_rows + list_offsets[l], len, n_rows, out);
    if (bad != len) {
      if (bad_list) *bad_list = l;
      if (bad_entry) *bad_entry = bad;
      return false;
    }
  }
  return true;
}

// The pair must have passed rowlists_check.  keys_max: option rows_keys_max.  false: the pass would hold 2^32 or more ids.
static inline bool rowlists_plan(const uint64_t* list_offsets, int n_lists, const int32_t* query_list, int nq, int64_t keys_max,
                                 RowListsPlan* out) {
  RowListsPlan& p = *out;
  p = RowListsPlan();
  std::vector<uint32_t> count((size_t)n_lists, 0u);
  for (int q = 0; q < nq; ++q) ++count[(size_t)query_list[q]];
  p.list_route.assign((size_t)n_lists, ROWLISTS_ROUTE_UNUSED);
  p.list_base.assign((size_t)n_lists, 0);
  std::vector<size_t> next((size_t)n_lists, 0);  // the list's next free slot
  size_t slots = 0;
  uint32_t most = 0;
  for (int l = 0; l < n_lists; ++l) {
    if (!count[(size_t)l]) continue;
    const uint64_t len = list_offsets[l + 1] - list_offsets[l];
    if (keys_max > 0 && len <= (uint64_t)keys_max) {
      p.list_route[(size_t)l] = ROWLISTS_ROUTE_PASS;
      p.list_base[(size_t)l] = p.pass_ids;
      p.pass_ids += len;
      next[(size_t)l] = slots;
      slots += count[(size_t)l];
      most = std::max(most, count[(size_t)l]);
    } else {
      p.list_route[(size_t)l] = ROWLISTS_ROUTE_FALLBACK;
      p.fallback_lists.push_back(l);
    }
  }
  if (p.pass_ids > 0xFFFFFFFFull) return false;
  p.qb = most > 1 ? ROWLISTS_QB : 1;
  p.slot_query.assign(slots, -1);
  p.slot_len.assign(slots, 0u);
  std::vector<int32_t> slot_list(slots, -1);
  for (int q = 0; q < nq; ++q) {  // (stable: caller order inside a list)
    const int l = query_list[q];
    if (p.list_route[(size_t)l] != ROWLISTS_ROUTE_PASS) continue;
    const size_t s = next[(size_t)l]++;
    p.slot_query[s] = q;
    p.slot_len[s] = (uint32_t)(list_offsets[l + 1] - list_offsets[l]);
    slot_list[s] = l;
  }
  const uint64_t budget = ROWLISTS_ROUND_KEY_BYTES / sizeof(uint64_t);
  for (size_t s0 = 0; s0 < slots;) {
    RowListsRound r;
    r.slot0 = (uint32_t)s0;
    r.item0 = p.items.size();
    size_t s1 = s0;
    uint64_t stride = 1;
    while (s1 < slots && s1 - s0 < ROWLISTS_ROUND_SLOTS) {
      const uint64_t st = std::max<uint64_t>(stride, p.slot_len[s1]);
      if (s1 > s0 && (uint64_t)(s1 - s0 + 1) * st > budget) break;
      stride = st;
      ++s1;
    }
    r.slots = (uint32_t)(s1 - s0);
    r.stride = stride;
    // the round's slots list by list: chunk by chunk, every query block of the list
    for (size_t a = s0; a < s1;) {
      size_t b = a;
      while (b < s1 && slot_list[b] == slot_list[a]) ++b;
      const uint32_t len = p.slot_len[a];
      const uint64_t base = p.list_base[(size_t)slot_list[a]];
      for (uint32_t off = 0; off < len; off += ROWLISTS_CHUNK)
        for (size_t s = a; s < b; s += (size_t)p.qb) {
          RowListsItem it;
          it.first = (uint32_t)(base + off);
          it.n = std::min(ROWLISTS_CHUNK, len - off);
          it.slot = (uint32_t)(s - s0);
          it.nq = (uint32_t)std::min<size_t>((size_t)p.qb, b - s);
          it.offset = off;
          p.items.push_back(it);
        }
      a = b;
    }
    r.items = p.items.size() - r.item0;
    p.rounds.push_back(r);
    s0 = s1;
  }
  return true;
}
