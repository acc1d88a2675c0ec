// Drives the device-free host side of wdbx_index_assign's int8 route (wdbx-py_amd/csrc/host_assign8.h) for
// tests/test_assign8_host.py: built with plain g++, once as it is and once under -fsanitize=address,undefined.
//   plan  OPT N_ROWS MIN_ROWS PITCH8 SHADOW N_CENTERS CUS MAX_GRID PAIR_CAP
//         -> path why ct8 block n_blocks slots lds tiles grid quant_grid pair_cap covered
//   terms (stdin, one per line: L2 sA aA bA a_max b_max gamma under sc D c2 -- floats as hex)
//         -> per line: T bound margin listed (floats as hex; listed for vouch = 1)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_assign8.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "plan") && argc == 11) {
    const long long opt = atoll(argv[2]);
    const unsigned long long n = strtoull(argv[3], nullptr, 10), min_rows = strtoull(argv[4], nullptr, 10);
    const uint32_t pitch8 = (uint32_t)atoll(argv[5]);
    const int n_centers = atoi(argv[7]);
    const Assign8Why why = assign8_why(opt, n, min_rows, pitch8);
    const Assign8Plan p = assign8_plan(why, atoi(argv[6]) != 0, n, n_centers, pitch8, atoi(argv[8]), strtoull(argv[9], nullptr, 10),
                                       strtoull(argv[10], nullptr, 10));
    // every centre in exactly one block
    int covered = p.path == ASSIGN_PATH_I8;
    if (covered) {
      std::vector<int> seen((size_t)n_centers, 0);
      for (int b = 0; b < p.n_blocks; ++b)
        for (int c = 0; c < assign8_block_count(p, n_centers, b); ++c) ++seen[(size_t)(assign8_block_first(p, b) + c)];
      for (int c = 0; c < n_centers; ++c) covered &= seen[(size_t)c] == 1;
    }
    printf("%d %d %d %d %d %d %zu %u %u %u %llu %d\n", p.path, p.why, p.ct8, p.block, p.n_blocks, p.slots, p.lds, p.tiles, p.grid,
           p.quant_grid, (unsigned long long)p.pair_cap, covered);
    return 0;
  }
  if (!strcmp(argv[1], "terms")) {
    int l2, D;
    float sA, aA, bA, amax, bmax, gamma, under, sc, c2;
    while (scanf("%d %a %a %a %a %a %a %a %a %d %a", &l2, &sA, &aA, &bA, &amax, &bmax, &gamma, &under, &sc, &D, &c2) == 11) {
      const Assign8Group g{sA, aA, bA};
      const Assign8Call c{amax, bmax, gamma, under};
      const float margin = assign8_margin(l2 != 0, g, c);
      printf("%a %a %a %d\n", (double)assign8_T(l2 != 0, sA, sc, D, c2), (double)assign8_bound(l2 != 0, g, c), (double)margin,
             (int)assign8_listed(margin, 1.0f));
    }
    return 0;
  }
  return 2;
}
