// Stand-alone driver of u42_share_groups (wdbx-py_amd/csrc/host_selection.h) for tests/test_u42_share_host.py (plain g++, no
// HIP).  One case per input line, one output line per case:
//   u42_share_groups_harness < "nv qp"   -> groups first_0 width_0 first_1 width_1 ...
// The arrays handed to the function hold exactly nv entries (heap blocks of their own), so a write behind them is a finding
// of the sanitised build.
#include <cstdio>
#include <vector>

#include "host_selection.h"

int main() {
  unsigned nv, qp;
  while (scanf("%u %u", &nv, &qp) == 2) {
    if (nv < 1 || nv > 4096) return 3;
    std::vector<uint32_t> first(nv), width(nv);
    const uint32_t n = u42_share_groups(nv, qp, first.data(), width.data());
    if (n > nv) return 5;
    printf("%u", n);
    for (uint32_t i = 0; i < n; ++i) printf(" %u %u", first[i], width[i]);
    printf("\n");
  }
  return feof(stdin) ? 0 : 4;  // (a line that did not parse)
}
