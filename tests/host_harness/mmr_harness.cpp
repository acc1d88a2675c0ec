// Stand-alone driver of wdbx-py_amd/csrc/host_mmr.h (the device-free host side of wdbx_index_search_mmr) for
// tests/test_mmr_host.py: plain g++, once more under -fsanitize=address,undefined.
//   plan     stdin: lines "pitch4 budget nq m_0 .. m_(nq-1)" -> two lines per case:
//                     n_rounds ni grid-of-the-largest-round (x y z)
//                     per round: q0 nq m_max rows g_floats bytes first_row0 last_row0 last_g0   (the table's ends)
//   check    stdin: lines "nq k fetch_k lambda buffers" (lambda as a C float literal, "nan" for NaN) -> the MmrArg code per line
//   pool     stdin: lines "fetch_k i_0 .. i_(fetch_k-1)" -> the pool size per line
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_mmr.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "plan")) {
    unsigned pitch4;
    unsigned long long budget;
    int nq;
    while (scanf("%u %llu %d", &pitch4, &budget, &nq) == 3) {
      if (nq < 1) return 2;
      std::vector<uint32_t> m((size_t)nq);
      for (auto& x : m)
        if (scanf("%" SCNu32, &x) != 1 || x > (uint32_t)MMR_MAX_POOL) return 2;
      const std::vector<MmrRound> rounds = mmr_plan_rounds(m.data(), nq, pitch4, budget);
      MmrRound big;
      for (const MmrRound& r : rounds)
        if (r.m_max >= big.m_max) big = r;
      const MmrGrid g = mmr_pairs_grid(big);
      printf("%zu %d %u %u %u\n", rounds.size(), mmr_pairs_ni(pitch4), g.x, g.y, g.z);
      std::vector<MmrQuery> table;
      for (const MmrRound& r : rounds) {
        mmr_round_queries(m.data(), r, &table);
        if (table.size() != r.nq) return 3;
        uint64_t bytes = 0;
        for (uint32_t i = 0; i < r.nq; ++i) bytes += mmr_query_bytes(m[r.q0 + i], pitch4);
        printf("%u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %" PRIu64 " ", r.q0, r.nq, r.m_max, r.rows, r.g_floats, bytes,
               table.front().row0, table.back().row0, table.back().g0);
      }
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(argv[1], "check")) {
    int nq, k, fetch_k, buffers;
    char lam[64];
    while (scanf("%d %d %d %63s %d", &nq, &k, &fetch_k, lam, &buffers) == 5) {
      const float lambda = !strcmp(lam, "nan") ? NAN : strtof(lam, nullptr);
      const MmrArg a = mmr_check_args(nq, k, fetch_k, lambda, buffers != 0, 2048);
      if ((a == MMR_ARG_OK) != (mmr_arg_message(a)[0] == 0)) return 3;
      printf("%d\n", (int)a);
    }
    return 0;
  }
  if (!strcmp(argv[1], "pool")) {
    int fetch_k;
    while (scanf("%d", &fetch_k) == 1) {
      if (fetch_k < 1) return 2;
      std::vector<int64_t> idx((size_t)fetch_k);
      for (auto& x : idx)
        if (scanf("%" SCNd64, &x) != 1) return 2;
      printf("%u\n", mmr_pool_size(idx.data(), fetch_k));
    }
    return 0;
  }
  return 2;
}
