// host_update.h -- the device-free side of a write of LISTED rows (wdbx_index_set_rows_at, wdbx_index_remove_rows): the list
// check, how many listed rows lie below each derived copy's coverage, the distinct int8 groups, the upload rounds and the
// launch count.  The list check and the narrowing to 32 bits are subset_validate's (host_subset.h).
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/update_harness.cpp (plain g++ in the CPU suite,
// tests/test_update_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_subset.h"

// bytes of caller rows one upload round carries at most (the scratch block never grows past it)
constexpr uint64_t UPDATE_ROUND_BYTES = 256ull << 20;

// rows [0, x) each derived copy covers; 0 = the copy does not exist (or covers nothing)
struct UpdateCoverage {
  uint64_t cn = 0, bf16 = 0, i8g = 0, u8 = 0, u6 = 0, u42 = 0;
};

struct UpdatePlan {
  uint64_t n = 0;                                  // listed rows
  uint32_t n_cn = 0, n_16 = 0, n_8 = 0, n_6 = 0, n_42 = 0;  // list positions below each per-row copy's coverage
  uint32_t n_refresh = 0;                          // ... the largest of them: positions the refresh launch walks (0: no launch)
  std::vector<uint32_t> groups;                    // distinct 64-row groups of the listed rows below the int8 copy's coverage, increasing
  uint64_t round_rows = 0, rounds = 0;             // scatter rounds: rows per round, how many
  int launches = 0;                                // kernel launches of the call: rounds + (n_refresh > 0) + (groups not empty)
};

// positions of the strictly increasing list whose row lies below `coverage`
static inline uint32_t update_count_below(const uint32_t* ids, uint64_t n, uint64_t coverage) {
  if (coverage > 0xFFFFFFFFull) return (uint32_t)n;
  return (uint32_t)(std::lower_bound(ids, ids + n, (uint32_t)coverage) - ids);
}

// the distinct groups row / 64 of the first n positions of the list, in one pass (the list is sorted)
static inline void update_groups(const uint32_t* ids, uint64_t n, std::vector<uint32_t>* out) {
  out->clear();
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t g = ids[i] / 64;
    if (out->empty() || out->back() != g) out->push_back(g);
  }
}

// rows of one upload round: as many dim-float rows as UPDATE_ROUND_BYTES holds, at least one
static inline uint64_t update_round_rows(uint32_t dim) {
  return std::max<uint64_t>(1, UPDATE_ROUND_BYTES / ((uint64_t)std::max<uint32_t>(dim, 1) * sizeof(float)));
}
static inline uint64_t update_round_first(const UpdatePlan& p, uint64_t round) { return round * p.round_rows; }
static inline uint64_t update_round_count(const UpdatePlan& p, uint64_t round) {
  return std::min(p.round_rows, p.n - update_round_first(p, round));
}

// ids: the validated list, narrowed.  upload: the call carries row data (set_rows_at) and scatters in rounds; a removal
// uploads nothing and scatters in one launch.
static inline UpdatePlan update_plan(const uint32_t* ids, uint64_t n, uint32_t dim, const UpdateCoverage& c, bool upload) {
  UpdatePlan p;
  p.n = n;
  if (!n) return p;
  p.n_cn = update_count_below(ids, n, c.cn);
  p.n_16 = update_count_below(ids, n, c.bf16);
  p.n_8 = update_count_below(ids, n, c.u8);
  p.n_6 = update_count_below(ids, n, c.u6);
  p.n_42 = update_count_below(ids, n, c.u42);
  p.n_refresh = std::max(std::max(std::max(p.n_cn, p.n_16), std::max(p.n_8, p.n_6)), p.n_42);
  update_groups(ids, update_count_below(ids, n, c.i8g), &p.groups);
  p.round_rows = upload ? update_round_rows(dim) : n;
  p.rounds = (n + p.round_rows - 1) / p.round_rows;
  p.launches = (int)p.rounds + (p.n_refresh ? 1 : 0) + (p.groups.empty() ? 0 : 1);
  return p;
}
