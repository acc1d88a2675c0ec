// Stand-alone driver of wdbx-py_amd/csrc/host_groups.h (the device-free host side of wdbx_index_search_groups) for
// tests/test_groups_host.py: plain g++, once more under -fsanitize=address,undefined.
//   runs    stdin: "n n_set", the n_set labels, then "m" and m label values to look up.  Builds the label order and the runs;
//           prints "n_labels n_labelled", the label_pos0 table, then per looked-up value "dense start count" (dense -1: not held)
//   tasks   argv: k segment_rows; stdin: "n_slots", then per slot "start count direct".  Prints the task count, per task
//           "query start count direct", then the slot_task0 table
//   slots   stdin: "n n_set", the labels, then "m" and m pairs "label row" (row may be -1).  Prints per pair "start count direct"
//   plan    argv: group_size budget; stdin: "n_slots" and the n_slots + 1 entries of slot_task0.  Prints per round
//           "slot0 slot1 task0 tasks merge_blocks bytes"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_groups.h"

static bool read_labels(uint64_t* n, std::vector<uint32_t>* labels) {
  uint64_t n_set;
  if (scanf("%" SCNu64 " %" SCNu64, n, &n_set) != 2 || n_set > *n) return false;
  labels->resize((size_t)n_set);
  for (auto& x : *labels)
    if (scanf("%" SCNu32, &x) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "runs") || !strcmp(argv[1], "slots")) {
    uint64_t n;
    std::vector<uint32_t> labels;
    if (!read_labels(&n, &labels)) return 2;
    LabelOrder lo;
    label_order_build(labels.data(), labels.size(), n, &lo);
    LabelRuns runs;
    label_runs_build(lo, labels.data(), labels.size(), &runs);
    int m;
    if (scanf("%d", &m) != 1) return 2;
    if (!strcmp(argv[1], "runs")) {
      printf("%u %u\n", lo.n_labels, runs.n_labelled);
      for (uint32_t p : runs.label_pos0) printf("%u ", p);
      printf("\n");
      for (int i = 0; i < m; ++i) {
        uint32_t v;
        if (scanf("%" SCNu32, &v) != 1) return 2;
        const int64_t d = groups_find_label(labels.data(), lo.label_row0.data(), runs.n_labelled, v);
        if (d < 0) printf("-1 0 0\n");
        else printf("%" PRId64 " %u %u\n", d, runs.label_pos0[(size_t)d], runs.label_pos0[(size_t)d + 1] - runs.label_pos0[(size_t)d]);
      }
      return 0;
    }
    for (int i = 0; i < m; ++i) {
      uint32_t v;
      int64_t row;
      if (scanf("%" SCNu32 " %" SCNd64, &v, &row) != 2) return 2;
      const GroupSlot s = groups_slot(labels.data(), lo.label_row0.data(), runs, v, row);
      printf("%u %u %d\n", s.start, s.count, (int)s.direct);
    }
    return 0;
  }
  if (!strcmp(argv[1], "tasks") && argc == 4) {
    const int k = atoi(argv[2]);
    const uint32_t seg = (uint32_t)strtoul(argv[3], nullptr, 10);
    size_t n_slots;
    if (scanf("%zu", &n_slots) != 1 || k < 1 || seg < 1) return 2;
    std::vector<GroupSlot> slots(n_slots);
    for (auto& s : slots) {
      int direct;
      if (scanf("%" SCNu32 " %" SCNu32 " %d", &s.start, &s.count, &direct) != 3) return 2;
      s.direct = direct != 0;
    }
    std::vector<GroupTask> tasks;
    std::vector<uint64_t> slot_task0;
    groups_tasks(slots.data(), n_slots, k, seg, &tasks, &slot_task0);
    printf("%zu\n", tasks.size());
    for (const GroupTask& t : tasks) printf("%u %u %u %u\n", t.query, t.start, t.count, t.direct);
    for (uint64_t t : slot_task0) printf("%" PRIu64 " ", t);
    printf("\n");
    return 0;
  }
  if (!strcmp(argv[1], "plan") && argc == 4) {
    const int g = atoi(argv[2]);
    const uint64_t budget = strtoull(argv[3], nullptr, 10);
    size_t n_slots;
    if (scanf("%zu", &n_slots) != 1) return 2;
    std::vector<uint64_t> slot_task0(n_slots + 1);
    for (auto& x : slot_task0)
      if (scanf("%" SCNu64, &x) != 1) return 2;
    for (const GroupsRound& r : groups_plan(slot_task0, g, budget))
      printf("%zu %zu %" PRIu64 " %" PRIu64 " %u %" PRIu64 "\n", r.slot0, r.slot1, r.task0, r.tasks, r.merge_blocks,
             groups_round_bytes(r.tasks, r.slot1 - r.slot0, g));
    return 0;
  }
  return 2;
}
