// Stand-alone driver of u42_mfma_round_grid next to scan_full_grid (wdbx-py_amd/csrc/host_selection.h): grid.x of the one launch
// that holds all matrix-core groups of a round (enqueue_singles_u6), for tests/test_u42_round_grid_host.py (plain g++, no HIP).
// One case per input line, one output line per case:
//   u42_round_grid_harness < "tiles64 cus wgs_per_cu groups"   -> round_grid full_grid xcds
#include <cstdio>

#include "host_selection.h"

int main() {
  unsigned tiles64, cus, wgs, groups;
  while (scanf("%u %u %u %u", &tiles64, &cus, &wgs, &groups) == 4) {
    if (tiles64 < 1 || cus < 1 || wgs < 1 || groups < 1) return 3;
    printf("%u %u %u\n", u42_mfma_round_grid(tiles64, cus, wgs, groups), scan_full_grid(tiles64, cus, wgs), U42_XCDS);
  }
  return feof(stdin) ? 0 : 4;  // (a line that did not parse)
}
