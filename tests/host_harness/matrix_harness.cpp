// matrix_harness.cpp -- stand-alone driver of wdbx-py_amd/csrc/host_matrix.h (the plan of wdbx_index_search_matrix) for the CPU
// suite (tests/test_matrix_host.py): plain g++, no HIP.  Built once plain and once under -fsanitize=address,undefined.
//
//   matrix_harness plan N_IDS K PITCH4 CU KEYS_MAX SELECT_MIN_K LDS_LISTS
//     -> one line "route qb round blocks P lds scratch_u64 ni mode rounds scratch_bytes", then one line per round
//        "first anchors anchor_blocks" (at most the first and the last 4 rounds when there are more than 8)
//   matrix_harness validate N_ROWS id id ...
//     -> "ok n" or "bad entry": subset_validate, the pass the entry point runs, with the narrowed rows checked against the input
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_matrix.h"

int main(int argc, char** argv) {
  if (argc >= 9 && !strcmp(argv[1], "plan")) {
    const uint64_t n_ids = strtoull(argv[2], nullptr, 10);
    const int k = atoi(argv[3]);
    const uint32_t pitch4 = (uint32_t)strtoul(argv[4], nullptr, 10);
    const int cu = atoi(argv[5]);
    const int64_t keys_max = atoll(argv[6]), select_min_k = atoll(argv[7]);
    const bool lds_lists = atoi(argv[8]) != 0;
    const MatrixPlan p = matrix_plan(n_ids, k, pitch4, cu, keys_max, select_min_k, lds_lists);
    printf("%d %d %d %u %u %zu %zu %d %d %" PRIu64 " %zu\n", p.sp.route, p.sp.qb, p.sp.round, p.sp.blocks, p.sp.P, p.sp.lds,
           p.sp.scratch_u64, p.ni, p.mode, p.rounds, p.scratch_bytes);
    uint64_t covered = 0;
    for (uint64_t r = 0; r < p.rounds; ++r) {
      const uint64_t first = matrix_round_first(p, r);
      const int b = matrix_round_anchors(p, n_ids, r);
      if (first != covered || b < 1 || b > MATRIX_ROUND_MAX) {
        fprintf(stderr, "round %" PRIu64 ": first %" PRIu64 " after %" PRIu64 " anchors, %d anchors\n", r, first, covered, b);
        return 2;
      }
      covered += (uint64_t)b;
      if (p.rounds <= 8 || r < 4 || r + 4 >= p.rounds) printf("%" PRIu64 " %d %u\n", first, b, matrix_anchor_blocks(p, b));
    }
    if (covered != n_ids) {
      fprintf(stderr, "the rounds cover %" PRIu64 " of %" PRIu64 " anchors\n", covered, n_ids);
      return 2;
    }
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "validate")) {
    const uint64_t n_rows = strtoull(argv[2], nullptr, 10);
    std::vector<uint64_t> ids;
    for (int i = 3; i < argc; ++i) ids.push_back(strtoull(argv[i], nullptr, 10));
    std::vector<uint32_t> out(ids.size());
    const uint64_t bad = subset_validate(ids.data(), ids.size(), n_rows, out.data());
    if (bad != ids.size()) {
      printf("bad %" PRIu64 "\n", bad);
      return 0;
    }
    for (size_t i = 0; i < ids.size(); ++i)
      if ((uint64_t)out[i] != ids[i]) return 2;
    printf("ok %zu\n", ids.size());
    return 0;
  }
  fprintf(stderr, "usage: matrix_harness plan N_IDS K PITCH4 CU KEYS_MAX SELECT_MIN_K LDS_LISTS | validate N_ROWS id ...\n");
  return 1;
}
