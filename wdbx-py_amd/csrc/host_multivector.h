// host_multivector.h -- the device-free host side of wdbx_index_search_multivector (late interaction / MaxSim: rank the labels by
// the sum over a query's vectors of each vector's best score among the label's rows): the cut of a call's vectors into rounds,
// the segments of each round, the route, the grids and the scratch sizes.  Included by wdbx_hip.hip (behind host_labels.h, whose
// label order and scratch budget it uses) and, on its own, by tests/host_harness/multivector_harness.cpp (plain g++ in the CPU
// suite, tests/test_multivector_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_labels.h"

constexpr int MULTIVECTOR_MAX_VECTORS = 1024;       // (= WDBX_MAX_QUERY_VECTORS) vectors of one query
constexpr int MULTIVECTOR_MAX_ROUND = 256;          // the largest round (option multivector_round_vectors: 1 .. this, the default)
constexpr int MULTIVECTOR_BLOCK = 8;                // vectors per block of the scoring kernel (label_keys_kernel's QB)
constexpr uint32_t MULTIVECTOR_NO_SLOT = 0xFFFFFFFFu;

// The vectors [v0, v1) of one round that belong to one query (numbered inside the round).  carry_in: the query began in an
// earlier round, the fold goes on from the accumulator; carry_out: it goes on in the next round, the fold is stored and nothing
// is ranked.  A segment that does not carry out is RANKED: it is the `slot`-th ranked segment of its round.  The reduce-and-rank
// kernel reads this struct as it is (five 32-bit words).
struct MultivectorSegment {
  uint32_t query;
  uint32_t v0, v1;
  uint32_t slot;   // MULTIVECTOR_NO_SLOT on a segment that carries out
  uint32_t carry;  // bit 0 = carry_in, bit 1 = carry_out
};
constexpr uint32_t MV_CARRY_IN = 1u, MV_CARRY_OUT = 2u;

struct MultivectorRound {
  uint64_t first = 0;        // its first vector in the call
  uint32_t vectors = 0;      // its vectors (consecutive)
  uint32_t seg0 = 0;         // its segments: [seg0, seg0 + segs) of MultivectorPlan::segments, in vector order
  uint32_t segs = 0;
  uint32_t ranked = 0;       // of them ranked (consecutive queries, the first is ranked_query0)
  uint32_t ranked_query0 = 0;
};

struct MultivectorPlan {
  int qb = 1;                  // vectors per block of the scoring kernel (1 or 8)
  int round_max = 1;           // vectors a round holds at the most
  bool floor = false;          // one vector per round because a single vector's items pass the budget (the scratch may then, too)
  bool select = false;         // k from select_min_k: a key per label and the radix-select chain; else lists + merge
  uint32_t score_blocks = 1;   // scoring grid.x of a full round: workgroups of four waves along the spans
  uint32_t rank_blocks = 1;    // reduce-and-rank grid.x (= partial lists per ranked segment on the list route)
  size_t lds = 0;              // list route: dynamic LDS of the reduce-and-rank kernel
  size_t keys_u64 = 0;         // u64s of item keys of the largest round
  size_t rank_u64 = 0;         // u64s behind them: partial lists (list route) or label keys (select route) of the most ranked segments
  std::vector<MultivectorRound> rounds;
  std::vector<MultivectorSegment> segments;
};

// u64s of ranking scratch one ranked segment takes
static inline uint64_t multivector_rank_u64_per_segment(bool select, uint32_t n_labels, int k, uint32_t rank_blocks) {
  return select ? (uint64_t)n_labels : (uint64_t)k * rank_blocks;
}

// dynamic LDS of multivector_rank_kernel's list instances: a list of k keys per wave (four waves)
static inline size_t multivector_rank_lds(int k) { return (size_t)4 * k * sizeof(uint64_t); }

// scoring grid.x for a round of `vectors`: two workgroups per CU over all vector blocks TOGETHER and never one more (the 8-vector
// instances run two workgroups per CU: with 3 blocks, 171 x 3 = 513 workgroups left one behind a full machine and the round
// took twice its time, profiles/multivector/), four spans per workgroup at least
static inline uint32_t multivector_score_blocks(uint32_t vectors, int qb, uint32_t n_spans, int cu_count) {
  const uint32_t vblocks = (vectors + (uint32_t)qb - 1) / (uint32_t)qb;
  const uint64_t want = std::max<uint64_t>(1, (uint64_t)cu_count * 2 / vblocks);
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, ((uint64_t)n_spans + 3) / 4));
}

// vector_offsets: [nq + 1], [0] == 0, strictly increasing (the caller has checked).  n_items >= n_labels >= 1, n_spans >= 1.
// round_vectors: the option, 1 .. MULTIVECTOR_MAX_ROUND.  A round is charged, per vector, its item keys and one ranked segment's
// scratch (no round ranks more segments than it has vectors), so whatever the queries' lengths a round of round_max vectors fits.
static inline MultivectorPlan multivector_plan(const uint64_t* vector_offsets, int nq, uint32_t n_items, uint32_t n_labels,
                                               uint32_t n_spans, int k, int cu_count, int64_t select_min_k, int64_t round_vectors) {
  MultivectorPlan p;
  const uint64_t total = vector_offsets[nq];
  p.select = select_min_k > 0 && k >= select_min_k;
  // a ranking workgroup takes at least 2048 labels (eight per lane), two workgroups per CU at the most
  p.rank_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)n_labels + 2047) / 2048, (uint64_t)cu_count * 2));
  const uint64_t per_segment = multivector_rank_u64_per_segment(p.select, n_labels, k, p.rank_blocks);
  const uint64_t per_vector = (uint64_t)n_items + per_segment;
  const uint64_t fit = DISTINCT_SCRATCH_BYTES / sizeof(uint64_t) / per_vector;
  p.floor = fit < 1;
  const uint64_t opt = (uint64_t)std::min<int64_t>(std::max<int64_t>(round_vectors, 1), MULTIVECTOR_MAX_ROUND);
  p.round_max = (int)std::max<uint64_t>(1, std::min<uint64_t>(opt, fit));
  p.qb = (p.round_max == 1 || total <= 1) ? 1 : MULTIVECTOR_BLOCK;
  p.lds = p.select ? 0 : multivector_rank_lds(k);
  p.score_blocks = multivector_score_blocks((uint32_t)std::min<uint64_t>(total, (uint64_t)p.round_max), p.qb, n_spans, cu_count);
  int q = 0;  // the query of the next vector
  for (uint64_t first = 0; first < total;) {
    const uint64_t left = total - first;
    uint64_t take = std::min<uint64_t>(left, (uint64_t)p.round_max);
    if (take < left && take >= MULTIVECTOR_BLOCK) take = take / MULTIVECTOR_BLOCK * MULTIVECTOR_BLOCK;  // whole blocks while more follows
    MultivectorRound r;
    r.first = first;
    r.vectors = (uint32_t)take;
    r.seg0 = (uint32_t)p.segments.size();
    for (uint64_t v = first; v < first + take;) {
      while (vector_offsets[q + 1] <= v) ++q;
      const uint64_t end = std::min<uint64_t>(vector_offsets[q + 1], first + take);
      MultivectorSegment s;
      s.query = (uint32_t)q;
      s.v0 = (uint32_t)(v - first);
      s.v1 = (uint32_t)(end - first);
      s.carry = (vector_offsets[q] < first ? MV_CARRY_IN : 0u) | (vector_offsets[q + 1] > first + take ? MV_CARRY_OUT : 0u);
      s.slot = MULTIVECTOR_NO_SLOT;
      if (!(s.carry & MV_CARRY_OUT)) {
        if (!r.ranked) r.ranked_query0 = s.query;
        s.slot = r.ranked++;
      }
      p.segments.push_back(s);
      v = end;
    }
    r.segs = (uint32_t)p.segments.size() - r.seg0;
    p.keys_u64 = std::max<size_t>(p.keys_u64, (size_t)r.vectors * n_items);
    p.rank_u64 = std::max<size_t>(p.rank_u64, (size_t)r.ranked * (size_t)per_segment);
    p.rounds.push_back(r);
    first += take;
  }
  return p;
}
