// multivector_tiles_harness.cpp -- stand-alone driver of wdbx-py_amd/csrc/host_multivector_tiles.h (the plan of the matrix-core
// scoring route of wdbx_index_search_multivector) for the CPU suite (tests/test_multivector_tiles_host.py): plain g++, no HIP.
// Built once plain and once under -fsanitize=address,undefined.
//
//   multivector_tiles_harness plan METRIC VECTORS PITCH N_SPANS CU
//     -> "eligible vt block vblocks ni lds grid covered", covered = 1 when the blocks hold every vector of the round exactly once
//   multivector_tiles_harness route OPTION MIN_VECTORS METRIC VECTORS PITCH   -> 1 when the round takes the tile route
//   multivector_tiles_harness limits   -> "block_max lds_limit span waves"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_multivector_tiles.h"

int main(int argc, char** argv) {
  if (argc >= 7 && !strcmp(argv[1], "plan")) {
    const uint32_t vectors = (uint32_t)strtoul(argv[3], nullptr, 10);
    const MultivectorTilePlan p = multivector_tile_plan(atoi(argv[2]), vectors, (uint32_t)strtoul(argv[4], nullptr, 10),
                                                        (uint32_t)strtoul(argv[5], nullptr, 10), atoi(argv[6]));
    std::vector<int> seen(vectors, 0);
    bool covered = p.lds == multivector_tile_lds(p.vt);
    for (uint32_t b = 0; b < p.vblocks; ++b) {
      const uint32_t count = multivector_tile_block_count(p, vectors, b);
      covered = covered && count >= 1 && count <= p.block;
      for (uint32_t v = b * p.block; v < b * p.block + count && v < vectors; ++v) ++seen[v];
    }
    for (int s : seen) covered = covered && s == 1;
    printf("%d %d %u %u %d %zu %u %d\n", p.eligible ? 1 : 0, p.vt, p.block, p.vblocks, p.ni, p.lds, p.grid, covered ? 1 : 0);
    return 0;
  }
  if (argc >= 7 && !strcmp(argv[1], "route")) {
    const uint32_t vectors = (uint32_t)strtoul(argv[5], nullptr, 10);
    const MultivectorTilePlan p = multivector_tile_plan(atoi(argv[4]), vectors, (uint32_t)strtoul(argv[6], nullptr, 10), 1000, 256);
    printf("%d\n", multivector_tile_route(atoll(argv[2]), atoll(argv[3]), vectors, p) ? 1 : 0);
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "limits")) {
    printf("%d %zu %d %d\n", MVT_BLOCK_MAX, MVT_LDS_LIMIT, MVT_SPAN, MVT_WAVES);
    return 0;
  }
  fprintf(stderr, "usage: multivector_tiles_harness plan METRIC VECTORS PITCH N_SPANS CU | route OPTION MIN METRIC VECTORS PITCH | limits\n");
  return 1;
}
