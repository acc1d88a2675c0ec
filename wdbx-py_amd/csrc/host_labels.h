// host_labels.h -- the device-free host side of wdbx_index_search_distinct: the label order (rows sorted by (label, row), dense
// label numbers, spans, items and their tables), the over-fetch and its host walk, the choice of the route, grid and scratch
// sizing of the full pass.  Included by wdbx_hip.hip and, on its own, by tests/host_harness/labels_harness.cpp (plain g++ in the
// CPU suite, tests/test_distinct_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <unordered_set>
#include <vector>

constexpr uint32_t LABEL_NONE = 0xFFFFFFFFu;  // (= WDBX_LABEL_NONE) the row is a label of its own
constexpr uint32_t LABEL_SPAN = 64;           // positions of the label order one wave walks at a time

// The label order of n rows.  A position is an index into `rows`; a span is LABEL_SPAN consecutive positions (the last may be
// short); an ITEM is a maximal run of one label inside one span -- the unit the scoring kernel writes one key per query for.
// Items are numbered in position order, so a label's items are consecutive and a span's items are consecutive.
struct LabelOrder {
  std::vector<uint32_t> rows;         // [n] every row number, sorted by (label, row); NONE rows last, by row
  std::vector<uint32_t> dense;        // [n] dense label index of each position (each NONE row its own)
  std::vector<uint32_t> span_item0;   // [n_spans + 1] first item of each span; the last entry = n_items
  std::vector<uint32_t> label_item0;  // [n_labels + 1] first item of each label; the last entry = n_items
  std::vector<uint32_t> label_row0;   // [n_labels] smallest row of each label (host only: what a ranked label is reported as)
  uint32_t n_labels = 0, n_items = 0, n_spans = 0;
};

// labels: the first n_set rows' labels (rows behind them are NONE; n_set <= n).  n is below 2^32 - 256 for every index.
static inline void label_order_build(const uint32_t* labels, uint64_t n_set, uint64_t n, LabelOrder* out) {
  LabelOrder& o = *out;
  o = LabelOrder();
  o.rows.resize((size_t)n);
  o.dense.resize((size_t)n);
  std::vector<uint64_t> keyed((size_t)n);
  for (uint64_t r = 0; r < n; ++r) keyed[(size_t)r] = ((uint64_t)(r < n_set ? labels[r] : LABEL_NONE) << 32) | r;
  std::sort(keyed.begin(), keyed.end());
  o.n_spans = (uint32_t)((n + LABEL_SPAN - 1) / LABEL_SPAN);
  o.span_item0.reserve((size_t)o.n_spans + 1);
  uint32_t prev = 0;
  for (uint64_t p = 0; p < n; ++p) {
    const uint32_t lab = (uint32_t)(keyed[(size_t)p] >> 32);
    const bool new_label = p == 0 || lab == LABEL_NONE || lab != prev;
    const bool new_span = p % LABEL_SPAN == 0;
    if (new_label) {
      o.label_item0.push_back(o.n_items);
      o.label_row0.push_back((uint32_t)keyed[(size_t)p]);
      ++o.n_labels;
    }
    if (new_span) o.span_item0.push_back(o.n_items);
    if (new_label || new_span) ++o.n_items;
    o.rows[(size_t)p] = (uint32_t)keyed[(size_t)p];
    o.dense[(size_t)p] = o.n_labels - 1;
    prev = lab;
  }
  o.span_item0.push_back(o.n_items);
  o.label_item0.push_back(o.n_items);
}

// Routes of a call (read-only option "last_distinct_path")
enum { DISTINCT_NONE = 0, DISTINCT_OVERFETCH = 1, DISTINCT_BOTH = 2, DISTINCT_FULL = 3 };

// k' of the over-fetch: min(rows, max_k, overfetch * k); 0 = no over-fetch (option distinct_overfetch <= 0, empty index)
static inline int distinct_overfetch_k(uint64_t n_rows, int k, int64_t overfetch, int max_k) {
  if (overfetch <= 0 || n_rows == 0) return 0;
  const uint64_t want = (uint64_t)std::min<int64_t>(overfetch, max_k) * (uint64_t)k;
  return (int)std::min<uint64_t>(std::min<uint64_t>(n_rows, (uint64_t)max_k), want);
}

// One query's ranked rows idx[0 .. kp) / score[0 .. kp) (row -1 = unused slot, only at the end) -> the first row of each label,
// cut at k, into out_*[0 .. k) (out_label may be null); the rest -1 / 0 / NONE.  labels: the first n_set rows' labels.
// Returns true when the answer is final: k labels found, or the ranking held every eligible row (it has an unused slot, or
// kp reached the row count).
static inline bool distinct_walk(const int64_t* idx, const float* score, int kp, uint64_t n_rows, const uint32_t* labels,
                                 uint64_t n_set, int k, int64_t* out_idx, float* out_score, uint32_t* out_label) {
  std::unordered_set<uint32_t> seen;
  int found = 0, valid = 0;
  for (int i = 0; i < kp && found < k; ++i) {
    if (idx[i] < 0) break;
    ++valid;
    const uint64_t r = (uint64_t)idx[i];
    const uint32_t lab = r < n_set ? labels[r] : LABEL_NONE;
    if (lab != LABEL_NONE && !seen.insert(lab).second) continue;
    out_idx[found] = idx[i];
    out_score[found] = score[i];
    if (out_label) out_label[found] = lab;
    ++found;
  }
  const bool all_seen = found < k && (valid < kp || (uint64_t)kp >= n_rows);
  for (int i = found; i < k; ++i) {
    out_idx[i] = -1;
    out_score[i] = 0.0f;
    if (out_label) out_label[i] = LABEL_NONE;
  }
  return found == k || all_seen;
}

// The full pass: per round of queries one scoring launch (a key per (query, item)), one ranking launch (the best key of each
// label, into per-workgroup top-k lists or a key per label) and the merge launch / the radix-select chains.
struct DistinctPlan {
  int qb = 1;                  // queries per query block of the scoring kernel (1 or 8)
  int round = 1;               // queries per round (a multiple of qb unless it is the whole call)
  bool select = false;         // k from select_min_k: a key per label and the radix-select chain; else lists + merge
  uint32_t score_blocks = 1;   // scoring grid.x: workgroups of four waves along the spans
  uint32_t rank_blocks = 1;    // ranking grid.x (= partial lists per query on the list route)
  size_t lds = 0;              // list route: dynamic LDS of the ranking kernel
  size_t keys_u64 = 0;         // u64s of item keys per round
  size_t rank_u64 = 0;         // u64s behind them: partial lists (list route) or label keys (select route)
};

constexpr uint64_t DISTINCT_SCRATCH_BYTES = 256ull << 20;  // what a round's keys and lists may take (as subset_plan)

// dynamic LDS of label_rank_kernel's list instances: a list of k keys per wave (four waves)
static inline size_t label_rank_lds(int k) { return (size_t)4 * k * sizeof(uint64_t); }

// n_items >= n_labels >= 1, n_spans >= 1.  A label order whose items alone pass the budget for ONE query still runs, a query
// at a time (the scratch is then what one query needs).
static inline DistinctPlan distinct_plan(uint32_t n_items, uint32_t n_labels, uint32_t n_spans, int nq, int k, int cu_count,
                                         int64_t select_min_k) {
  DistinctPlan p;
  p.select = select_min_k > 0 && k >= select_min_k;
  // a ranking workgroup takes at least 2048 labels (eight per lane), two workgroups per CU at the most
  p.rank_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t)n_labels + 2047) / 2048, (uint64_t)cu_count * 2));
  const uint64_t per_query = (uint64_t)n_items + (p.select ? (uint64_t)n_labels : (uint64_t)k * p.rank_blocks);
  const uint64_t fit = std::max<uint64_t>(1, DISTINCT_SCRATCH_BYTES / sizeof(uint64_t) / per_query);
  int round = (int)std::min<uint64_t>((uint64_t)std::min(nq, 256), fit);
  p.qb = nq <= 1 || fit < 8 ? 1 : 8;  // (a key per item for eight queries does not fit: one query at a time)
  if (round < nq) round = std::max(p.qb, round / p.qb * p.qb);
  p.round = round;
  const uint32_t qblocks = (uint32_t)((round + p.qb - 1) / p.qb);
  const uint64_t want = std::max<uint64_t>(1, ((uint64_t)cu_count * 2 + qblocks - 1) / qblocks);
  p.score_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, ((uint64_t)n_spans + 3) / 4));
  p.lds = p.select ? 0 : label_rank_lds(k);
  p.keys_u64 = (size_t)round * n_items;
  p.rank_u64 = (size_t)round * (p.select ? (size_t)n_labels : (size_t)k * p.rank_blocks);
  return p;
}
