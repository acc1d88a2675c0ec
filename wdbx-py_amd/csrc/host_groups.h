// host_groups.h -- the device-free host side of wdbx_index_search_groups / _group_members: where each label's run lies in the
// label order (host_labels.h), the dense label of a label value, the tasks of a call (a segment of a run, or one direct row, per
// workgroup of group_members_kernel) with the table that says which tasks belong to which (query, slot), and the rounds that
// keep a round's partial lists and task table within the scratch budget.  Included by wdbx_hip.hip and, on its own, by
// tests/host_harness/groups_harness.cpp (plain g++ in the CPU suite, tests/test_groups_host.py).  No HIP, no kernel types.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_labels.h"

constexpr int GROUPS_MAX_SIZE = 64;                      // (= WDBX_MAX_GROUP_SIZE) a wave's register list: one key per lane
constexpr int64_t GROUPS_SEGMENT_MIN = 4, GROUPS_SEGMENT_MAX = 65536, GROUPS_SEGMENT_DEFAULT = 2048;
constexpr uint64_t GROUPS_SCRATCH_BYTES = 256ull << 20;  // what a round's partial lists and tables may take (as distinct_plan)

// What ensure_label_order keeps on the host beside label_row0: the first position of each dense label (the last entry = n) and
// how many dense labels carry a label value -- they come first and ascend by value, every NONE row behind them is its own.
struct LabelRuns {
  std::vector<uint32_t> label_pos0;  // [n_labels + 1]
  uint32_t n_labelled = 0;
};

static inline void label_runs_build(const LabelOrder& lo, const uint32_t* labels, uint64_t n_set, LabelRuns* out) {
  LabelRuns& r = *out;
  r = LabelRuns();
  const size_t n = lo.rows.size();
  r.label_pos0.assign((size_t)lo.n_labels + 1, (uint32_t)n);
  for (size_t p = n; p-- > 0;) r.label_pos0[lo.dense[p]] = (uint32_t)p;  // (descending: the first position is written last)
  for (uint32_t d = 0; d < lo.n_labels; ++d) {
    const uint32_t row = lo.label_row0[d];
    if (row >= n_set || labels[row] == LABEL_NONE) break;
    ++r.n_labelled;
  }
}

// the dense label of a label value: binary search over labels[label_row0[d]], d < n_labelled; -1 = the handle holds no such row
static inline int64_t groups_find_label(const uint32_t* labels, const uint32_t* label_row0, uint32_t n_labelled, uint32_t value) {
  if (value == LABEL_NONE) return -1;
  uint32_t lo = 0, hi = n_labelled;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (labels[label_row0[mid]] < value) lo = mid + 1;
    else hi = mid;
  }
  return lo < n_labelled && labels[label_row0[lo]] == value ? (int64_t)lo : -1;
}

// What one (query, slot) ranks: nothing (count 0), the single row `start` (direct), or positions [start, start + count).
struct GroupSlot {
  uint32_t start = 0, count = 0;
  bool direct = false;
};

// slot_row < 0: unused.  slot_label NONE: the row itself.  Else that label's run; a label the handle does not hold ranks nothing.
static inline GroupSlot groups_slot(const uint32_t* labels, const uint32_t* label_row0, const LabelRuns& runs, uint32_t slot_label,
                                    int64_t slot_row) {
  GroupSlot s;
  if (slot_row < 0) return s;
  if (slot_label == LABEL_NONE) {
    s.start = (uint32_t)slot_row;
    s.count = 1;
    s.direct = true;
    return s;
  }
  const int64_t d = groups_find_label(labels, label_row0, runs.n_labelled, slot_label);
  if (d < 0) return s;
  s.start = runs.label_pos0[(size_t)d];
  s.count = runs.label_pos0[(size_t)d + 1] - s.start;
  return s;
}

// One workgroup's work (the device reads this layout: four words)
struct GroupTask {
  uint32_t query;   // query of the call
  uint32_t start;   // first position of the label order, or the row (direct)
  uint32_t count;   // positions (1 for a direct task)
  uint32_t direct;  // 1: `start` is a row number, the label order is not read
};

// slots: [nq * k], slot s belongs to query s / k.  A run is cut into segments of segment_rows positions (the last may be
// short).  slot_task0 [nq * k + 1]: slot s owns tasks [slot_task0[s], slot_task0[s + 1]) -- none for an unused slot.
static inline void groups_tasks(const GroupSlot* slots, size_t n_slots, int k, uint32_t segment_rows, std::vector<GroupTask>* tasks,
                                std::vector<uint64_t>* slot_task0) {
  tasks->clear();
  slot_task0->assign(n_slots + 1, 0);
  for (size_t s = 0; s < n_slots; ++s) {
    (*slot_task0)[s] = tasks->size();
    const GroupSlot& g = slots[s];
    const uint32_t query = (uint32_t)(s / (size_t)k);
    if (g.direct) {
      if (g.count) tasks->push_back(GroupTask{query, g.start, 1u, 1u});
      continue;
    }
    for (uint64_t p = 0; p < g.count; p += segment_rows)
      tasks->push_back(GroupTask{query, (uint32_t)(g.start + p), (uint32_t)std::min<uint64_t>(segment_rows, g.count - p), 0u});
  }
  (*slot_task0)[n_slots] = tasks->size();
}

// A round: slots [slot0, slot1) with all their tasks -- one scoring launch of a workgroup per task (grid.x = tasks; none when
// the round has no task) and one merge launch of a wave per slot (four per workgroup).
struct GroupsRound {
  size_t slot0 = 0, slot1 = 0;
  uint64_t task0 = 0, tasks = 0;
  uint32_t merge_blocks = 0;
};

// bytes of a round: its partial lists (tasks * group_size keys), its tasks and its share of the slot table
static inline uint64_t groups_round_bytes(uint64_t tasks, uint64_t slots, int group_size) {
  return tasks * ((uint64_t)group_size * sizeof(uint64_t) + sizeof(GroupTask)) + (slots + 1) * sizeof(uint64_t);
}

// Consecutive slots are taken while the round stays within the budget; a slot whose tasks alone pass it still runs, as a round
// of its own (the scratch is then what that slot needs).
static inline std::vector<GroupsRound> groups_plan(const std::vector<uint64_t>& slot_task0, int group_size,
                                                   uint64_t budget = GROUPS_SCRATCH_BYTES) {
  std::vector<GroupsRound> rounds;
  const size_t n_slots = slot_task0.empty() ? 0 : slot_task0.size() - 1;
  size_t s0 = 0;
  while (s0 < n_slots) {
    size_t s1 = s0 + 1;
    while (s1 < n_slots && groups_round_bytes(slot_task0[s1 + 1] - slot_task0[s0], s1 + 1 - s0, group_size) <= budget) ++s1;
    GroupsRound r;
    r.slot0 = s0;
    r.slot1 = s1;
    r.task0 = slot_task0[s0];
    r.tasks = slot_task0[s1] - slot_task0[s0];
    r.merge_blocks = (uint32_t)((s1 - s0 + 3) / 4);
    rounds.push_back(r);
    s0 = s1;
  }
  return rounds;
}
