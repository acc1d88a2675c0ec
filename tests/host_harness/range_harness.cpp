// Drives the device-free host side of wdbx_index_range_search (wdbx-py_amd/csrc/host_range.h) the way the library does:
// per-query counts -> CSR offsets; when they fit the capacity, the keys go to the row array at their offsets and
// range_sort_decode sorts and decodes them there.  tests/test_range_search.py builds it with g++ and checks the output.
//   stdin:  metric_l2 nq capacity, then nq counts, then sum(counts) keys (decimal u64), query by query
//   stdout: "offsets" o_0 .. o_nq, then (only when o_nq <= capacity) "rows" r..., "scores" float bits (u32)...
//   extra mode "tau qq t": prints the float bits of range_selection_tau_l2(qq, t)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_range.h"

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "tau")) {
    double qq = 0;
    float t = 0;
    if (scanf("%lf %f", &qq, &t) != 2) return 2;
    const float f = range_selection_tau_l2(qq, t);
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    printf("%u\n", u);
    return 0;
  }
  int metric_l2 = 0, nq = 0;
  unsigned long long capacity = 0;
  if (scanf("%d %d %llu", &metric_l2, &nq, &capacity) != 3 || nq < 0) return 2;
  std::vector<uint64_t> counts(nq), offsets(nq + 1, 0);
  for (auto& c : counts)
    if (scanf("%" SCNu64, &c) != 1) return 2;
  // as the library does it: rounds of queries, each continuing the running offset
  const int round = 3;
  for (int q0 = 0; q0 < nq; q0 += round) range_csr_offsets(counts.data() + q0, std::min(round, nq - q0), offsets.data() + q0);
  const uint64_t total = offsets[nq];
  std::vector<uint64_t> keys(total);
  for (auto& k : keys)
    if (scanf("%" SCNu64, &k) != 1) return 2;
  printf("offsets");
  for (uint64_t o : offsets) printf(" %" PRIu64, o);
  printf("\n");
  if (total > capacity) return 0;
  std::vector<int64_t> rows(capacity + 1, -7);  // (the caller's buffers: capacity slots)
  std::vector<float> scores(capacity + 1, -7.0f);
  if (total) memcpy(rows.data(), keys.data(), total * sizeof(uint64_t));
  range_sort_decode(metric_l2, nq, offsets.data(), rows.data(), scores.data());
  printf("rows");
  for (uint64_t i = 0; i < total; ++i) printf(" %" PRId64, rows[i]);
  printf("\nscores");
  for (uint64_t i = 0; i < total; ++i) {
    uint32_t u;
    memcpy(&u, &scores[i], sizeof u);
    printf(" %u", u);
  }
  printf("\n");
  return rows[capacity] == -7 && scores[capacity] == -7.0f ? 0 : 3;  // nothing written past the capacity
}
