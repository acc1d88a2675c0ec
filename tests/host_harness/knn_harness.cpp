// knn_harness.cpp -- stand-alone driver of wdbx-py_amd/csrc/host_knn.h (the plan and the margin of wdbx_index_knn_graph) for the
// CPU suite (tests/test_knn_graph_host.py): plain g++, no HIP.  Built once plain and once under -fsanitize=address,undefined.
//   plan N_ROWS ELIGIBLE K CU SHADOW FINITE [MAX_GRID] -> the KnnPlan's fields, then covered = 1 when the passes hold every row exactly once
//   validate K HAVE_IDX HAVE_SCORE -> the KnnCheck value;   limits -> the header's constants
//   margin DIM L2 CASES SEED WORST -> "violations max_ppm" over CASES pairs of fp32 vectors (WORST: every element a hair under a
//     bf16 rounding midpoint, signs alike, so the operands' errors add up): T from bf16-rounded operands on an fp32 fma chain, S in
//     float64 from the fp32 operands; violations counts |T - S| > b_T, max_ppm is the largest |T - S| / b_T in 1e-6
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "host_knn.h"

static float to_bf16(float x) {  // round to nearest even on the upper 16 bits
  uint32_t u;
  memcpy(&u, &x, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  u &= 0xFFFF0000u;
  memcpy(&x, &u, 4);
  return x;
}

int main(int argc, char** argv) {
  if (argc >= 8 && !strcmp(argv[1], "plan")) {
    const uint64_t n_rows = strtoull(argv[2], nullptr, 10), eligible = strtoull(argv[3], nullptr, 10);
    const KnnPlan p = knn_plan(n_rows, eligible, atoi(argv[4]), atoi(argv[5]), atoi(argv[6]) != 0, atoi(argv[7]) != 0,
                               argc >= 9 ? strtoull(argv[8], nullptr, 10) : 0);
    bool covered = true;
    if (p.path != KNN_PATH_NONE) {
      uint64_t next = 0;
      for (uint32_t i = 0; i < p.passes; ++i) {
        covered = covered && knn_pass_first(p, i) == next && knn_pass_anchors(p, n_rows, i) >= 1;
        next += knn_pass_anchors(p, n_rows, i);
      }
      covered = covered && next == n_rows && p.lds == knn_lds_bytes() && p.cap == knn_list_cap(atoi(argv[4]));
    }
    printf("%d %u %zu %u %u %u %u %u %zu %zu %zu %d\n", p.path, p.cap, p.lds, p.anchor_tiles, p.cand_tiles, p.grid, p.passes,
           p.exact_grid, p.list_bytes, p.count_bytes, p.flag_bytes, covered ? 1 : 0);
    return 0;
  }
  if (argc >= 5 && !strcmp(argv[1], "validate")) {
    printf("%d\n", (int)knn_validate(atoi(argv[2]), atoi(argv[3]) != 0, atoi(argv[4]) != 0));
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "limits")) {
    printf("%d %d %d %zu %zu %" PRIu64 "\n", KNN_MAX_K, KNN_ANCHOR_TILE, KNN_CAND_TILE, KNN_LDS_LIMIT, KNN_SCRATCH_BUDGET,
           KNN_TILE_MIN_ROWS);
    return 0;
  }
  if (argc >= 7 && !strcmp(argv[1], "margin")) {
    const int dim = atoi(argv[2]), cases = atoi(argv[4]);
    const bool l2 = atoi(argv[3]) != 0, worst = atoi(argv[6]) != 0;
    const uint32_t pitch = (uint32_t)(dim + 3) / 4 * 4;
    const KnnBound bound = knn_bound(pitch);
    std::mt19937 rng((uint32_t)atoi(argv[5]));
    std::normal_distribution<float> normal(0.f, 1.f);
    std::uniform_int_distribution<int> expo(-20, 20);
    std::vector<float> a((size_t)dim), c((size_t)dim);
    int violations = 0;
    double worst_ratio = 0;
    for (int t = 0; t < cases; ++t) {
      const float sa = ldexpf(1.f, expo(rng)), sc = ldexpf(1.f, expo(rng));
      const float under = 1.f + 0.00390625f - 9.5367431640625e-07f;  // 1 + 2^-8 - 2^-20: rounds DOWN by almost half a bf16 step
      for (size_t i = 0; i < (size_t)dim; ++i) {
        a[i] = sa * (worst ? under * ldexpf(1.f, expo(rng) / 8) : normal(rng));
        c[i] = sc * (worst ? under * ldexpf(1.f, expo(rng) / 8) : normal(rng));
      }
      float dot = 0.f, an2 = 0.f, cn2 = 0.f;
      double S = 0, cc = 0;
      for (size_t i = 0; i < (size_t)dim; ++i) {
        dot = fmaf(to_bf16(a[i]), to_bf16(c[i]), dot);
        an2 = fmaf(a[i], a[i], an2);
        cn2 = fmaf(c[i], c[i], cn2);
        S += (double)a[i] * (double)c[i];
        cc += (double)c[i] * (double)c[i];
      }
      const double T = l2 ? (double)fmaf(2.0f, dot, -cn2) : (double)dot;
      if (l2) S = 2 * S - cc;
      const double bT = (double)knn_tile_margin(l2, an2, cn2, bound);
      const double err = fabs(T - S);
      if (!(err <= bT)) ++violations;
      if (bT > 0 && err / bT > worst_ratio) worst_ratio = err / bT;
    }
    printf("%d %ld\n", violations, lround(worst_ratio * 1e6));
    return 0;
  }
  fprintf(stderr, "usage: knn_harness plan | validate | limits | margin ...\n");
  return 1;
}
