// Stand-alone driver of u42_mfma_groups next to u42_share_groups (wdbx-py_amd/csrc/host_selection.h), the way a round plans its
// full passes (enqueue_singles_u6), for tests/test_u42_mfma_host.py (plain g++, no HIP).  One case per input line, one output
// line per case:
//   u42_mfma_groups_harness < "nv min_short qp"   -> mfma_groups covered valu_groups first_0 width_0 first_1 width_1 ...
// The VALU groups' first queries are those of the round (covered + what u42_share_groups returns).  Their arrays hold exactly
// the queries left to them (heap blocks of their own, one entry at least), so a write behind them is a finding of the
// sanitised build.
#include <cstdio>
#include <vector>

#include "host_selection.h"

int main() {
  unsigned nv, min_short, qp;
  while (scanf("%u %u %u", &nv, &min_short, &qp) == 3) {
    if (nv < 1 || nv > 4096) return 3;
    uint32_t covered = ~0u;
    const uint32_t ngm = u42_mfma_groups(nv, min_short, &covered);
    if (covered > nv) return 5;
    const uint32_t rest = nv - covered;
    std::vector<uint32_t> first(rest ? rest : 1), width(rest ? rest : 1);
    const uint32_t n = u42_share_groups(rest, qp, first.data(), width.data());
    if (n > rest) return 6;
    printf("%u %u %u", ngm, covered, n);
    for (uint32_t i = 0; i < n; ++i) printf(" %u %u", covered + first[i], width[i]);
    printf("\n");
  }
  return feof(stdin) ? 0 : 4;  // (a line that did not parse)
}
