// host_recommend.h -- the device-free host side of wdbx_index_search_recommend (rows ranked by positive and negative examples):
// validation of the offsets and of the exclusion list, the plan of a pass (ranking mode, grid, rounds within the scratch
// bound), the example table the kernel reads, which queries the favoured pass left short of k, and the splice of the two
// sides' lists into the caller's rows.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/recommend_harness.cpp (plain g++ in the CPU suite,
// tests/test_recommend_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

constexpr int RECOMMEND_MAX_EXAMPLES = 64;         // WDBX_MAX_EXAMPLES
constexpr uint64_t RECOMMEND_MAX_EXCLUDE = 1024;   // WDBX_MAX_EXCLUDE_ROWS
constexpr uint64_t RECOMMEND_SCRATCH_BYTES = 256ull << 20;  // what a round's keys or lists may take (as subset_plan)

// example_offsets [2 * nq + 1]: [0] == 0, non-decreasing, per query at least one positive and at most RECOMMEND_MAX_EXAMPLES
// examples.  true = valid; else *msg names the query and the entry.
static inline bool recommend_validate_offsets(const uint64_t* off, int nq, std::string* msg) {
  char buf[200];
  if (off[0] != 0) {
    snprintf(buf, sizeof buf, "example_offsets[0] = %llu, must be 0", (unsigned long long)off[0]);
    *msg = buf;
    return false;
  }
  for (int i = 0; i < 2 * nq; ++i)
    if (off[i + 1] < off[i]) {
      snprintf(buf, sizeof buf, "example_offsets decrease at entry %d (query %d): %llu after %llu", i + 1, i / 2,
               (unsigned long long)off[i + 1], (unsigned long long)off[i]);
      *msg = buf;
      return false;
    }
  for (int q = 0; q < nq; ++q) {
    const uint64_t pos = off[2 * q + 1] - off[2 * q], all = off[2 * q + 2] - off[2 * q];
    if (pos == 0) {
      snprintf(buf, sizeof buf, "query %d has no positive example (example_offsets entries %d and %d)", q, 2 * q, 2 * q + 1);
      *msg = buf;
      return false;
    }
    if (all > (uint64_t)RECOMMEND_MAX_EXAMPLES) {
      snprintf(buf, sizeof buf, "query %d has %llu examples, more than %d (example_offsets entries %d to %d)", q,
               (unsigned long long)all, RECOMMEND_MAX_EXAMPLES, 2 * q, 2 * q + 2);
      *msg = buf;
      return false;
    }
  }
  return true;
}

// exclude_rows: strictly increasing row numbers below n_rows, at most RECOMMEND_MAX_EXCLUDE of them.  out32 (may be null)
// receives them narrowed to 32 bits (n_rows is below 2^32 - 256 for every index).  true = valid; else *msg names the entry.
static inline bool recommend_validate_exclude(const uint64_t* rows, uint64_t n, uint64_t n_rows, uint32_t* out32, std::string* msg) {
  char buf[200];
  if (n > RECOMMEND_MAX_EXCLUDE) {
    snprintf(buf, sizeof buf, "exclude_rows holds %llu rows, more than %llu", (unsigned long long)n, (unsigned long long)RECOMMEND_MAX_EXCLUDE);
    *msg = buf;
    return false;
  }
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t r = rows[i];
    if (r >= n_rows || r > 0xFFFFFFFFull || (i && r <= rows[i - 1])) {
      snprintf(buf, sizeof buf, "exclude_rows must be strictly increasing row numbers below %llu (entry %llu is %llu)",
               (unsigned long long)n_rows, (unsigned long long)i, (unsigned long long)r);
      *msg = buf;
      return false;
    }
    if (out32) out32[i] = (uint32_t)r;
  }
  return true;
}

// passes of the kernel over a loaded row for `count` examples of one sign: blocks of 8, one of 4, the rest one by one
static inline int recommend_example_blocks(uint64_t count) { return (int)(count / 8 + (count % 8) / 4 + count % 4); }

// Ranking modes (the kernel's MODE): 0 per-wave lists in LDS, 1 register lists (k <= 128), 2 a key per row and the
// radix-select chain (k from option select_min_k on; 0 = never)
static inline int recommend_mode(int k, int64_t select_min_k, bool lds_lists) {
  if (select_min_k > 0 && k >= select_min_k) return 2;
  return (k <= 128 && !lds_lists) ? 1 : 0;
}

struct RecommendPlan {
  int mode = 0;
  int round = 1;           // queries per round of launches (grid.y)
  uint32_t blocks = 1;     // grid.x: workgroups of four waves along the corpus
  uint32_t P = 0;          // lists: partial lists per query (= blocks: the four wave lists are merged in the workgroup)
  size_t lds = 0;          // lists: dynamic LDS of the scoring kernel
  size_t scratch_u64 = 0;  // u64s of scratch per round: partial lists (modes 0, 1) or keys (mode 2)
};

// cu_count: compute units; the grid holds about eight workgroups per CU over the round's queries (the pass streams the whole
// corpus) and never more waves than rows.  budget: bytes a round's scratch may take (RECOMMEND_SCRATCH_BYTES; smaller in tests).
static inline RecommendPlan recommend_plan(uint64_t n_rows, int nq, int k, int cu_count, int64_t select_min_k, bool lds_lists,
                                           uint64_t budget = RECOMMEND_SCRATCH_BYTES) {
  RecommendPlan p;
  p.mode = recommend_mode(k, select_min_k, lds_lists);
  if (n_rows == 0 || nq < 1) return p;
  const uint64_t budget_u64 = std::max<uint64_t>(1, budget / sizeof(uint64_t));
  int round = std::min(nq, 256);
  const uint64_t want = std::max<uint64_t>(1, ((uint64_t)cu_count * 8 + round - 1) / round);
  p.blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (n_rows + 3) / 4));
  const uint64_t per_query = p.mode == 2 ? n_rows : (uint64_t)k * p.blocks;
  const uint64_t fit = std::max<uint64_t>(1, budget_u64 / per_query);
  if ((uint64_t)round > fit) round = (int)fit;
  p.round = round;
  if (p.mode != 2) {
    p.P = p.blocks;
    p.lds = (size_t)4 * k * sizeof(uint64_t);
  }
  p.scratch_u64 = (size_t)round * per_query;
  return p;
}

// the rounds of `items` queries: (first, count), consecutive, each query exactly once
static inline std::vector<std::pair<int, int>> recommend_rounds(int items, int round) {
  std::vector<std::pair<int, int>> r;
  for (int q0 = 0; q0 < items; q0 += std::max(round, 1)) r.push_back({q0, std::min(std::max(round, 1), items - q0)});
  return r;
}

// the kernel's table for the listed queries: per slot {first positive, first negative, end of the negatives}
static inline void recommend_table(const uint64_t* off, const uint32_t* queries, size_t n, uint32_t* out) {
  for (size_t s = 0; s < n; ++s) {
    const uint32_t q = queries[s];
    out[3 * s] = (uint32_t)off[2 * q];
    out[3 * s + 1] = (uint32_t)off[2 * q + 1];
    out[3 * s + 2] = (uint32_t)off[2 * q + 2];
  }
}

// after the favoured pass (fav_idx [nq, k], -1 = empty slot, filled from the front): the queries that fell short of k, in
// order, and by how many
static inline void recommend_short(const int64_t* fav_idx, int nq, int k, std::vector<uint32_t>* short_queries, std::vector<int>* gaps) {
  short_queries->clear();
  gaps->clear();
  for (int q = 0; q < nq; ++q) {
    int have = 0;
    while (have < k && fav_idx[(size_t)q * k + have] >= 0) ++have;
    if (have < k) {
      short_queries->push_back((uint32_t)q);
      gaps->push_back(k - have);
    }
  }
}

// Splice: query q's row is its favoured list, then -- for short query number s -- the head of the disfavoured list
// dis_idx / dis_score [short queries, k], then empty slots (-1 / 0 / 0).  out_side may be null.
static inline void recommend_splice(const int64_t* fav_idx, const float* fav_score, const int64_t* dis_idx, const float* dis_score,
                                    const std::vector<uint32_t>& short_queries, int nq, int k, int64_t* out_idx, float* out_score,
                                    uint8_t* out_side) {
  size_t s = 0;
  for (int q = 0; q < nq; ++q) {
    const size_t base = (size_t)q * k;
    int have = 0;
    for (; have < k && fav_idx[base + have] >= 0; ++have) {
      out_idx[base + have] = fav_idx[base + have];
      out_score[base + have] = fav_score[base + have];
      if (out_side) out_side[base + have] = 1;
    }
    const bool is_short = s < short_queries.size() && short_queries[s] == (uint32_t)q;
    int at = have;
    if (is_short) {
      const size_t db = s * (size_t)k;
      for (int i = 0; at < k && i < k && dis_idx[db + i] >= 0; ++i, ++at) {
        out_idx[base + at] = dis_idx[db + i];
        out_score[base + at] = dis_score[db + i];
        if (out_side) out_side[base + at] = 0;
      }
      ++s;
    }
    for (; at < k; ++at) {
      out_idx[base + at] = -1;
      out_score[base + at] = 0.0f;
      if (out_side) out_side[base + at] = 0;
    }
  }
}
