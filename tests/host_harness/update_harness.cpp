// update_harness.cpp -- stand-alone driver of wdbx-py_amd/csrc/host_update.h (the plan of wdbx_index_set_rows_at /
// wdbx_index_remove_rows) for the CPU suite (tests/test_update_host.py): plain g++, no HIP.  Built once plain and once under
// -fsanitize=address,undefined.
//
//   update_harness plan N_ROWS DIM UPLOAD CN BF16 I8G U8 U6 U42 id id ...
//     -> "bad entry" when the list fails the check (subset_validate, the pass the entry points run), else one line
//        "n n_cn n_16 n_8 n_6 n_42 n_refresh round_rows rounds launches", one line "groups g g ..." and one line per round
//        "first count" (at most the first and the last 4 rounds when there are more than 8)
//   update_harness rounds N DIM
//     -> "round_rows rounds first_of_last count_of_last" of an upload of N rows of DIM floats (no list is built)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_update.h"

int main(int argc, char** argv) {
  if (argc >= 11 && !strcmp(argv[1], "plan")) {
    const uint64_t n_rows = strtoull(argv[2], nullptr, 10);
    const uint32_t dim = (uint32_t)strtoul(argv[3], nullptr, 10);
    const bool upload = atoi(argv[4]) != 0;
    UpdateCoverage c;
    c.cn = strtoull(argv[5], nullptr, 10);
    c.bf16 = strtoull(argv[6], nullptr, 10);
    c.i8g = strtoull(argv[7], nullptr, 10);
    c.u8 = strtoull(argv[8], nullptr, 10);
    c.u6 = strtoull(argv[9], nullptr, 10);
    c.u42 = strtoull(argv[10], nullptr, 10);
    std::vector<uint64_t> ids;
    for (int i = 11; i < argc; ++i) ids.push_back(strtoull(argv[i], nullptr, 10));
    std::vector<uint32_t> ids32(ids.size());
    const uint64_t bad = subset_validate(ids.data(), ids.size(), n_rows, ids32.data());
    if (bad != ids.size()) {
      printf("bad %" PRIu64 "\n", bad);
      return 0;
    }
    const UpdatePlan p = update_plan(ids32.data(), ids32.size(), dim, c, upload);
    printf("%" PRIu64 " %u %u %u %u %u %u %" PRIu64 " %" PRIu64 " %d\n", p.n, p.n_cn, p.n_16, p.n_8, p.n_6, p.n_42, p.n_refresh, p.round_rows,
           p.rounds, p.launches);
    printf("groups");
    for (uint32_t g : p.groups) printf(" %u", g);
    printf("\n");
    uint64_t covered = 0;
    for (uint64_t r = 0; r < p.rounds; ++r) {
      const uint64_t first = update_round_first(p, r), count = update_round_count(p, r);
      if (first != covered || count < 1 || count > p.round_rows) {
        fprintf(stderr, "round %" PRIu64 ": first %" PRIu64 " after %" PRIu64 " rows, %" PRIu64 " rows\n", r, first, covered, count);
        return 2;
      }
      covered += count;
      if (p.rounds <= 8 || r < 4 || r + 4 >= p.rounds) printf("%" PRIu64 " %" PRIu64 "\n", first, count);
    }
    if (covered != p.n) {
      fprintf(stderr, "the rounds cover %" PRIu64 " of %" PRIu64 " rows\n", covered, p.n);
      return 2;
    }
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "rounds")) {
    UpdatePlan p;
    p.n = strtoull(argv[2], nullptr, 10);
    p.round_rows = update_round_rows((uint32_t)strtoul(argv[3], nullptr, 10));
    p.rounds = (p.n + p.round_rows - 1) / p.round_rows;
    const uint64_t last = p.rounds ? p.rounds - 1 : 0;
    printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p.round_rows, p.rounds, p.rounds ? update_round_first(p, last) : 0,
           p.rounds ? update_round_count(p, last) : 0);
    return 0;
  }
  fprintf(stderr, "usage: update_harness plan N_ROWS DIM UPLOAD CN BF16 I8G U8 U6 U42 id ... | rounds N DIM\n");
  return 1;
}
