// Stand-alone driver of wdbx-py_amd/csrc/host_multimask.h for tests/test_multimask_host.py (plain g++, no HIP).
//   multimask_harness <block_slots> <n_masks> < "nq  c_0 c_1 ... c_(nq-1)"
// prints
//   ok <0|1> <bad_query>
//   slots   q q q ...        (-1 = pad)
//   groups  c c c ...        (class per column group)
//   blocks  g g g ...        (first column group of each block, then the number of groups)
//   classes c c ...
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_multimask.h"

template <class T>
static void line(const char* name, const std::vector<T>& v) {
  printf("%s", name);
  for (const T x : v) printf(" %lld", (long long)x);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int block_slots = atoi(argv[1]), n_masks = atoi(argv[2]);
  int nq = 0;
  if (scanf("%d", &nq) != 1) return 2;
  std::vector<int32_t> cls((size_t)(nq > 0 ? nq : 0));
  for (int q = 0; q < nq; ++q) {
    int c;
    if (scanf("%d", &c) != 1) return 2;
    cls[(size_t)q] = c;
  }
  MultimaskPlan plan;
  int bad = -2;
  const bool ok = multimask_plan(cls.data(), nq, n_masks, block_slots, &plan, &bad);
  printf("ok %d %d\n", ok ? 1 : 0, bad);
  if (!ok) return 0;
  line("slots", plan.slot_query);
  line("groups", plan.group_class);
  line("blocks", plan.block_group);
  line("classes", plan.classes);
  return 0;
}
