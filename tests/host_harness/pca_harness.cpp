// pca_harness.cpp -- stand-alone driver of wdbx-py_amd/csrc/host_pca.h for the CPU suite (tests/test_pca_host.py): plain g++, no
// HIP; built once plain and once under -fsanitize=address,undefined.  `plans` prints one line per dimension, the plan's numbers
// and covered = 1 when every tile of the upper triangle lies in exactly one group and one wave, no wave holds more than its
// instance's tiles, every tile's two column blocks are among its group's staged blocks, the staging fits the instance's loader
// and the ranges hold every row exactly once; `limits` prints the header's constants.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_pca.h"

static bool covered(const PcaPlan& p, uint64_t n_rows, uint32_t pitch) {
  std::vector<int> seen((size_t)p.nb * p.nb, 0);
  bool ok = p.dp == 32 * p.nb && p.groups == pca_group_count(p.nb, p.side) && p.lds == pca_lds_bytes(p.staged);
  ok = ok && p.wave_tiles <= p.instance && p.instance <= PCA_WAVE_TILES && p.staged <= (p.instance <= 8 ? 16 : 12);
  for (int g = 0; g < p.groups; ++g) {
    const PcaGroup G = pca_group(p.nb, p.side, g);
    ok = ok && G.si <= G.sj && G.ni >= 1 && G.nj >= 1 && G.per_wave * PCA_WAVES >= G.tiles && G.staged <= p.staged;
    // what the kernel's loader carries: 32 rows x 8 quads x staged blocks over 512 threads
    ok = ok && PCA_CHUNK_ROWS * 8 * G.staged <= 512 * (p.instance <= 8 ? 8 : 6);
    for (int w = 0; w < PCA_WAVES; ++w)
      for (int q = w * G.per_wave; q < (w + 1) * G.per_wave && q < G.tiles; ++q) {
        int a = -1, b = -1;
        pca_tile_staged(G, q, &a, &b);
        if (a < 0 || a >= G.staged || b < 0 || b >= G.staged) return false;
        const int I = pca_staged_block(G, a), J = pca_staged_block(G, b);
        if (I < 0 || I > J || J >= p.nb) return false;
        ++seen[(size_t)I * p.nb + J];
      }
  }
  for (int i = 0; i < p.nb; ++i)
    for (int j = 0; j < p.nb; ++j) ok = ok && seen[(size_t)i * p.nb + j] == (j >= i ? 1 : 0);
  ok = ok && p.range_rows % PCA_CHUNK_ROWS == 0 && (uint64_t)p.ranges * p.range_rows >= n_rows &&
       (!n_rows || (uint64_t)(p.ranges - 1) * p.range_rows < n_rows);
  ok = ok && p.partial_bytes == (size_t)p.ranges * p.dp * p.dp * sizeof(float);
  ok = ok && (uint64_t)p.sum_ranges * p.sum_rows >= n_rows && (!n_rows || (uint64_t)(p.sum_ranges - 1) * p.sum_rows < n_rows);
  ok = ok && p.sum_bytes == (size_t)p.sum_ranges * (pitch + 1) * sizeof(float) && p.sum_grid == (p.sum_ranges + 3) / 4;
  return ok;
}

int main(int argc, char** argv) {
  if (argc >= 8 && !strcmp(argv[1], "plans")) {
    const int lo = atoi(argv[2]), hi = atoi(argv[3]);
    const uint64_t n_rows = strtoull(argv[4], nullptr, 10);
    for (int dim = lo; dim <= hi; ++dim) {
      const uint32_t pitch = (uint32_t)(dim + 3) / 4 * 4;
      const PcaPlan p = pca_plan(n_rows, dim, pitch, atoi(argv[5]), atoi(argv[6]), atoll(argv[7]), true);
      printf("%d %d %d %d %d %d %d %zu %u %" PRIu64 " %zu %u %" PRIu64 " %d\n", dim, p.nb, p.side, p.groups, p.wave_tiles, p.staged,
             p.instance, p.lds, p.ranges, p.range_rows, p.partial_bytes, p.sum_ranges, p.sum_rows, covered(p, n_rows, pitch) ? 1 : 0);
    }
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "limits")) {
    printf("%d %d %d %d %d %zu %zu\n", PCA_MAX_COMPONENTS, PCA_MAX_DIM, PCA_CHUNK_ROWS, PCA_WAVES, PCA_WAVE_TILES, PCA_LDS_LIMIT,
           PCA_PARTIALS_BUDGET);
    return 0;
  }
  fprintf(stderr, "usage: pca_harness plans DIM_LO DIM_HI N_ROWS CU FORCED_SIDE FORCED_RANGES | limits\n");
  return 1;
}
