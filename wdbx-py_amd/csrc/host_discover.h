// host_discover.h -- the device-free host side of wdbx_index_search_discover (rows ranked by context pairs and a target,
// DESIGN.md section 4.17): validation of the pair offsets, the plan of the scoring pass and of the zone stage (ranking mode,
// grids, rounds within the scratch bound), the staged vectors and their table, the zones an answer needs, and the splice of
// the zone lists into the caller's rows.  The exclusion list is recommend's (recommend_validate_exclude).
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/discover_harness.cpp (plain g++ in the CPU suite,
// tests/test_discover_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "host_recommend.h"

constexpr int DISCOVER_MAX_PAIRS = 32;                      // WDBX_MAX_CONTEXT_PAIRS
constexpr int DISCOVER_ZONE_COUNT = DISCOVER_MAX_PAIRS + 1;  // wins values 0 .. 32 (DISCOVER_ZONES of kernels_discover.h)
constexpr uint64_t DISCOVER_RECORD_BYTES = 9;               // a row's record: the 64-bit key and the wins byte
constexpr uint64_t DISCOVER_SCRATCH_BYTES = RECOMMEND_SCRATCH_BYTES;  // what a round's records, keys or lists may take

// pair_offsets [nq + 1]: [0] == 0, non-decreasing, per query at most DISCOVER_MAX_PAIRS pairs and, in context mode (no
// target), at least one.  true = valid; else *msg names the query and the entry.
static inline bool discover_validate_offsets(const uint64_t* off, int nq, bool target, std::string* msg) {
  char buf[200];
  if (off[0] != 0) {
    snprintf(buf, sizeof buf, "pair_offsets[0] = %llu, must be 0", (unsigned long long)off[0]);
    *msg = buf;
    return false;
  }
  for (int q = 0; q < nq; ++q) {
    if (off[q + 1] < off[q]) {
      snprintf(buf, sizeof buf, "pair_offsets decrease at entry %d (query %d): %llu after %llu", q + 1, q,
               (unsigned long long)off[q + 1], (unsigned long long)off[q]);
      *msg = buf;
      return false;
    }
    const uint64_t pairs = off[q + 1] - off[q];
    if (pairs > (uint64_t)DISCOVER_MAX_PAIRS) {
      snprintf(buf, sizeof buf, "query %d has %llu context pairs, more than %d (pair_offsets entries %d and %d)", q,
               (unsigned long long)pairs, DISCOVER_MAX_PAIRS, q, q + 1);
      *msg = buf;
      return false;
    }
    if (!target && pairs == 0) {
      snprintf(buf, sizeof buf, "query %d has no context pair and the call has no targets (pair_offsets entries %d and %d)", q, q, q + 1);
      *msg = buf;
      return false;
    }
  }
  return true;
}

// passes of the kernel over a loaded row for `pairs` pairs: blocks of 8 vectors, one of 4, one of 2
static inline int discover_pair_blocks(uint64_t pairs) { return (int)(pairs / 4 + (pairs % 4) / 2 + pairs % 2); }

// The scoring pass.  Context mode ranks in the pass itself: the plan is recommend's (mode 0 / 1 / 2, lists or keys as scratch).
// Target mode writes records: `mode` is the ZONE stage's ranking mode, the pass's scratch is DISCOVER_RECORD_BYTES per row and
// query and `round` keeps it within the budget.
struct DiscoverPlan {
  bool target = false;
  int mode = 0;
  int round = 1;            // queries per round of launches (grid.y)
  uint32_t blocks = 1;      // grid.x: workgroups of four waves along the corpus
  uint32_t P = 0;           // context mode, lists: partial lists per query
  size_t lds = 0;           // context mode, lists: dynamic LDS of the scoring kernel
  size_t scratch_u64 = 0;   // context mode: u64s of lists or keys per round
  size_t record_rows = 0;   // target mode: records per round (round * n_rows)
};

static inline DiscoverPlan discover_plan(uint64_t n_rows, int nq, int k, bool target, int cu_count, int64_t select_min_k,
                                         bool lds_lists, uint64_t budget = DISCOVER_SCRATCH_BYTES) {
  DiscoverPlan p;
  p.target = target;
  const RecommendPlan rp = recommend_plan(n_rows, nq, k, cu_count, select_min_k, lds_lists, budget);
  p.mode = rp.mode;
  if (n_rows == 0 || nq < 1) return p;
  if (!target) {
    p.round = rp.round;
    p.blocks = rp.blocks;
    p.P = rp.P;
    p.lds = rp.lds;
    p.scratch_u64 = rp.scratch_u64;
    return p;
  }
  int round = std::min(nq, 256);
  const uint64_t want = std::max<uint64_t>(1, ((uint64_t)cu_count * 8 + round - 1) / round);
  p.blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (n_rows + 3) / 4));
  const uint64_t fit = std::max<uint64_t>(1, budget / (DISCOVER_RECORD_BYTES * n_rows));
  if ((uint64_t)round > fit) round = (int)fit;
  p.round = round;
  p.record_rows = (size_t)round * n_rows;
  return p;
}

// The zone stage for `slots` (query, zone) entries: a lane per row, so a workgroup walks 256 rows at a time; lists of k keys
// per workgroup (modes 0, 1) or a key per row (mode 2) as scratch, `round` entries per launch within the budget.
struct DiscoverZonePlan {
  int round = 1;
  uint32_t blocks = 1;
  uint32_t P = 0;
  size_t lds = 0;
  size_t scratch_u64 = 0;
};

static inline DiscoverZonePlan discover_zone_plan(uint64_t n_rows, int slots, int k, int mode, int cu_count,
                                                  uint64_t budget = DISCOVER_SCRATCH_BYTES) {
  DiscoverZonePlan z;
  if (n_rows == 0 || slots < 1) return z;
  int round = std::min(slots, 256);
  const uint64_t want = std::max<uint64_t>(1, ((uint64_t)cu_count * 8 + round - 1) / round);
  z.blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (n_rows + 255) / 256));
  const uint64_t per_slot = mode == 2 ? n_rows : (uint64_t)k * z.blocks;
  const uint64_t fit = std::max<uint64_t>(1, std::max<uint64_t>(1, budget / sizeof(uint64_t)) / per_slot);
  if ((uint64_t)round > fit) round = (int)fit;
  z.round = round;
  if (mode != 2) {
    z.P = z.blocks;
    z.lds = (size_t)4 * k * sizeof(uint64_t);
  }
  z.scratch_u64 = (size_t)round * per_slot;
  return z;
}

// staged vectors of the call: query q's are [target q?, p0, n0, p1, n1, ...], the queries back to back
static inline uint64_t discover_staged_count(const uint64_t* off, int nq, bool target) { return 2 * off[nq] + (target ? (uint64_t)nq : 0); }

// ... laid out from the caller's arrays (targets [nq, dim] or null, context [2 * off[nq], dim]) into out [staged count, dim]
static inline void discover_stage(const float* targets, const float* context, const uint64_t* off, int nq, int dim, float* out) {
  size_t at = 0;
  for (int q = 0; q < nq; ++q) {
    if (targets) {
      memcpy(out + at * dim, targets + (size_t)q * dim, (size_t)dim * sizeof(float));
      ++at;
    }
    const size_t n = (size_t)(2 * (off[q + 1] - off[q]));
    if (n) memcpy(out + at * dim, context + (size_t)(2 * off[q]) * dim, n * dim * sizeof(float));
    at += n;
  }
}

// the kernel's table for queries [first, first + count): per slot {first staged vector, pairs}
static inline void discover_table(const uint64_t* off, int first, int count, bool target, uint32_t* out) {
  for (int s = 0; s < count; ++s) {
    const int q = first + s;
    out[2 * s] = (uint32_t)(2 * off[q] + (target ? (uint64_t)q : 0));
    out[2 * s + 1] = (uint32_t)(off[q + 1] - off[q]);
  }
}

// One query's zones from its counts [DISCOVER_ZONE_COUNT] (rows with a key per wins value): from the most wins down, the
// non-empty zones until k rows are covered, each with the rows to take from it.
struct DiscoverZone {
  uint32_t zone;
  uint32_t take;
};

static inline std::vector<DiscoverZone> discover_zones(const uint32_t* counts, int k) {
  std::vector<DiscoverZone> z;
  uint64_t left = (uint64_t)k;
  for (int w = DISCOVER_ZONE_COUNT - 1; w >= 0 && left > 0; --w) {
    if (!counts[w]) continue;
    const uint32_t take = (uint32_t)std::min<uint64_t>(counts[w], left);
    z.push_back({(uint32_t)w, take});
    left -= take;
  }
  return z;
}

// Splice: the zone lists zone_idx / zone_score [zone slots, k] are in the order of `zones` (query by query, each query's zones
// from the top down); query q's row is the head (`take` entries) of each of its lists, wins = the zone, then empty slots
// (-1 / 0 / 0).  out_wins may be null.
static inline void discover_splice(const std::vector<std::vector<DiscoverZone>>& zones, const int64_t* zone_idx, const float* zone_score,
                                   int k, int64_t* out_idx, float* out_score, uint8_t* out_wins) {
  size_t slot = 0;
  for (size_t q = 0; q < zones.size(); ++q) {
    const size_t base = q * (size_t)k;
    int at = 0;
    for (const DiscoverZone& z : zones[q]) {
      const size_t zb = slot * (size_t)k;
      for (uint32_t i = 0; i < z.take && at < k; ++i, ++at) {
        out_idx[base + at] = zone_idx[zb + i];
        out_score[base + at] = zone_score[zb + i];
        if (out_wins) out_wins[base + at] = (uint8_t)z.zone;
      }
      ++slot;
    }
    for (; at < k; ++at) {
      out_idx[base + at] = -1;
      out_score[base + at] = 0.0f;
      if (out_wins) out_wins[base + at] = 0;
    }
  }
}
