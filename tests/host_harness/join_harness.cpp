// join_harness.cpp -- stand-alone driver of wdbx-py_amd/csrc/host_join.h (the plan and the tile test of wdbx_index_self_join) for
// the CPU suite (tests/test_join_host.py): plain g++, no HIP.  Built once plain and once under -fsanitize=address,undefined.
//   plan N_ROWS ELIGIBLE PITCH8 SHADOW CU MAX_GRID PAIR_CAP MIN_ROWS EXACT_MAX -> the JoinPlan's fields, then covered = 1 when
//     the blocks hold every row exactly once, each starts at the tile of its first row and the tile visits add up
//   validate NAN HAVE_OFFSETS CAPACITY HAVE_ROWS HAVE_SCORES -> the JoinCheck value;   limits -> the header's constants
//   keep -> per line of stdin "L2 t sA aA bA sB aB bB D cnA cnB" (floats in any strtof form) one line "1" / "0": the sweep's
//     test of one accumulator, through the functions the kernel's epilogue calls
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host_join.h"

int main(int argc, char** argv) {
  if (argc >= 11 && !strcmp(argv[1], "plan")) {
    const uint64_t n_rows = strtoull(argv[2], nullptr, 10);
    const JoinPlan p = join_plan(n_rows, strtoull(argv[3], nullptr, 10), (uint32_t)atoi(argv[4]), atoi(argv[5]) != 0, atoi(argv[6]),
                                 strtoull(argv[7], nullptr, 10), strtoull(argv[8], nullptr, 10), strtoull(argv[9], nullptr, 10),
                                 strtoull(argv[10], nullptr, 10));
    bool covered = true;
    if (p.path == JOIN_PATH_SWEEP) {
      uint64_t next = 0, visits = 0;
      for (uint32_t i = 0; i < p.blocks; ++i) {
        const uint64_t first = (uint64_t)i * p.block_rows;
        covered = covered && first == next && first < n_rows && join_block_first_tile(p, i) == first / JOIN_TILE_ROWS &&
                  (first + p.block_rows - 1) / JOIN_TILE_ROWS == first / JOIN_TILE_ROWS && join_block_tiles(p, i) >= 1;
        next = first + p.block_rows;
        visits += join_block_tiles(p, i);
      }
      covered = covered && next >= n_rows && next - n_rows < p.block_rows && visits == p.tile_visits && p.lds == join_lds_bytes(p.ct8, (uint32_t)atoi(argv[4]));
    }
    printf("%d %d %d %d %u %u %u %zu %u %" PRIu64 " %" PRIu64 " %d\n", p.path, p.why, p.refused ? 1 : 0, p.ct8, p.block_rows, p.blocks,
           p.tiles, p.lds, p.grid, p.pair_cap, p.tile_visits, covered ? 1 : 0);
    return 0;
  }
  if (argc >= 7 && !strcmp(argv[1], "validate")) {
    printf("%d\n", (int)join_validate(atoi(argv[2]) ? NAN : 0.5f, atoi(argv[3]) != 0, strtoull(argv[4], nullptr, 10), atoi(argv[5]) != 0,
                                      atoi(argv[6]) != 0));
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "limits")) {
    printf("%d %u %zu %" PRIu64 " %" PRIu64 " %" PRId64 " %" PRId64 "\n", JOIN_TILE_ROWS, JOIN_MAX_PITCH8, JOIN_LDS_BLOCK_MAX,
           JOIN_PAIR_BYTES_MAX, JOIN_PAIR_CAP_MIN, JOIN_MIN_ROWS_DEFAULT, JOIN_EXACT_MAX_ROWS_DEFAULT);
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "keep")) {
    int l2, D;
    float t, v[6], cna, cnb;
    while (scanf("%d %f %f %f %f %f %f %f %d %f %f", &l2, &t, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &D, &cna, &cnb) == 11) {
      const JoinCut c = join_cut(l2 != 0, t, JoinGroup{v[0], v[1], v[2]}, JoinGroup{v[3], v[4], v[5]});
      const bool keep = l2 ? join_l2_keep(D, join_norm_low(cnb), c, join_l2_col(join_norm_low(cna), c)) : D >= c.T;
      printf("%d\n", keep ? 1 : 0);
    }
    return 0;
  }
  fprintf(stderr, "usage: join_harness plan | validate | limits | keep ...\n");
  return 1;
}
