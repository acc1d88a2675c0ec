// Stand-alone driver of wdbx-py_amd/csrc/host_refine.h for tests/test_refine_launch_host.py (plain g++, no HIP).
// One case per input line, one output line per case:
//   refine_harness < "k cap lds_lists"   -> reg waves n_lds lds raise
// and, first, one line of the header's constants: REFINE_R REFINE_MAX_WAVES REFINE_LDS_BUDGET REFINE_LDS_DEFAULT_LIMIT
#include <cstdio>

#include "host_refine.h"

int main() {
  printf("%d %d %zu %zu\n", REFINE_R, REFINE_MAX_WAVES, REFINE_LDS_BUDGET, REFINE_LDS_DEFAULT_LIMIT);
  int k, lds_lists;
  unsigned cap;
  while (scanf("%d %u %d", &k, &cap, &lds_lists) == 3) {
    const RefineShape s = refine_shape(k, cap, lds_lists != 0);
    printf("%d %d %u %zu %d\n", s.reg ? 1 : 0, s.waves, s.n_lds, s.lds, s.raise ? 1 : 0);
  }
  return feof(stdin) ? 0 : 4;  // (a line that did not parse)
}
