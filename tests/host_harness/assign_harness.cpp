// assign_harness.cpp -- stand-alone driver of wdbx-py_amd/csrc/host_assign.h (the plan of wdbx_index_assign) for the CPU suite
// (tests/test_assign_host.py): plain g++, no HIP.  Built once plain and once under -fsanitize=address,undefined.
//
//   assign_harness plan N_ROWS N_CENTERS PITCH CU L2
//     -> "mt block n_blocks slots lds tiles grid prep_grid exact_grid partials sums_grid rows_per_partial centre_bytes aux_bytes
//        partial_bytes covered", covered = 1 when the blocks hold every centre exactly once and the partials every row
//   assign_harness validate N_CENTERS HAVE_CENTERS ANY_OUTPUT   -> the AssignCheck value
//   assign_harness limits   -> "max_centers block_max lds_limit budget tile_rows"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_assign.h"

int main(int argc, char** argv) {
  if (argc >= 7 && !strcmp(argv[1], "plan")) {
    const uint64_t n_rows = strtoull(argv[2], nullptr, 10);
    const int n_centers = atoi(argv[3]);
    const uint32_t pitch = (uint32_t)strtoul(argv[4], nullptr, 10);
    const AssignPlan p = assign_plan(n_rows, n_centers, pitch, atoi(argv[5]), atoi(argv[6]) != 0);
    std::vector<int> seen((size_t)n_centers, 0);
    bool covered = p.slots >= n_centers && p.lds == assign_lds_bytes(p.block);
    for (int b = 0; b < p.n_blocks; ++b) {
      const int first = assign_block_first(p, b), count = assign_block_count(p, n_centers, b);
      covered = covered && count >= 1 && count <= p.block;
      for (int c = first; c < first + count && c < n_centers; ++c) ++seen[(size_t)c];
    }
    for (int s : seen) covered = covered && s == 1;
    covered = covered && (uint64_t)p.partials * p.rows_per_partial >= n_rows &&
              (!n_rows || (uint64_t)(p.partials - 1) * p.rows_per_partial < n_rows);
    printf("%d %d %d %d %zu %u %u %u %u %u %u %" PRIu64 " %zu %zu %zu %d\n", p.mt, p.block, p.n_blocks, p.slots, p.lds, p.tiles,
           p.grid, p.prep_grid, p.exact_grid, p.partials, p.sums_grid, p.rows_per_partial, p.centre_bytes, p.aux_bytes,
           p.partial_bytes, covered ? 1 : 0);
    return 0;
  }
  if (argc >= 5 && !strcmp(argv[1], "validate")) {
    printf("%d\n", (int)assign_validate(atoi(argv[2]), atoi(argv[3]) != 0, atoi(argv[4]) != 0));
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "limits")) {
    printf("%d %d %zu %zu %d\n", ASSIGN_MAX_CENTERS, ASSIGN_BLOCK_MAX, ASSIGN_LDS_LIMIT, ASSIGN_PARTIALS_BUDGET, ASSIGN_TILE_ROWS);
    return 0;
  }
  fprintf(stderr, "usage: assign_harness plan N_ROWS N_CENTERS PITCH CU L2 | validate N_CENTERS HAVE_CENTERS ANY_OUTPUT | limits\n");
  return 1;
}
