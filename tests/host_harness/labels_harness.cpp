// Stand-alone driver of wdbx-py_amd/csrc/host_labels.h (the device-free host side of wdbx_index_search_distinct) for
// tests/test_distinct_host.py: plain g++, once more under -fsanitize=address,undefined.
//   order            stdin: n, n_set, then n_set labels  -> n_labels n_items n_spans / rows / dense / span_item0 / label_item0
//   plan CU SELMIN   stdin: lines "n_items n_labels n_spans nq k"  -> qb round select score_blocks rank_blocks lds keys_u64 rank_u64
//   overfetch        stdin: lines "n_rows k overfetch"  -> k'
//   walk KP NROWS K  stdin: n_set, then n_set labels, then KP (row score) pairs  -> final / rows / scores / labels
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_labels.h"

static void print_u32(const std::vector<uint32_t>& v) {
  for (uint32_t x : v) printf("%u ", x);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "order")) {
    unsigned long long n = 0, n_set = 0;
    if (scanf("%llu %llu", &n, &n_set) != 2 || n_set > n) return 2;
    std::vector<uint32_t> labels((size_t)n_set);
    for (auto& l : labels)
      if (scanf("%" SCNu32, &l) != 1) return 2;
    LabelOrder o;
    label_order_build(labels.data(), n_set, n, &o);
    printf("%u %u %u\n", o.n_labels, o.n_items, o.n_spans);
    print_u32(o.rows);
    print_u32(o.dense);
    print_u32(o.span_item0);
    print_u32(o.label_item0);
    return 0;
  }
  if (!strcmp(argv[1], "plan") && argc == 4) {
    const int cu = atoi(argv[2]);
    const long long sel = atoll(argv[3]);
    unsigned n_items, n_labels, n_spans;
    int nq, k;
    while (scanf("%u %u %u %d %d", &n_items, &n_labels, &n_spans, &nq, &k) == 5) {
      const DistinctPlan p = distinct_plan(n_items, n_labels, n_spans, nq, k, cu, sel);
      printf("%d %d %d %u %u %zu %zu %zu\n", p.qb, p.round, p.select ? 1 : 0, p.score_blocks, p.rank_blocks, p.lds, p.keys_u64, p.rank_u64);
    }
    return 0;
  }
  if (!strcmp(argv[1], "overfetch")) {
    unsigned long long n;
    int k;
    long long of;
    while (scanf("%llu %d %lld", &n, &k, &of) == 3) printf("%d\n", distinct_overfetch_k(n, k, of, 2048));
    return 0;
  }
  if (!strcmp(argv[1], "walk") && argc == 5) {
    const int kp = atoi(argv[2]), k = atoi(argv[4]);
    const unsigned long long n_rows = strtoull(argv[3], nullptr, 10);
    unsigned long long n_set = 0;
    if (scanf("%llu", &n_set) != 1) return 2;
    std::vector<uint32_t> labels((size_t)n_set);
    for (auto& l : labels)
      if (scanf("%" SCNu32, &l) != 1) return 2;
    std::vector<int64_t> idx((size_t)kp);
    std::vector<float> score((size_t)kp);
    for (int i = 0; i < kp; ++i)
      if (scanf("%" SCNd64 " %f", &idx[(size_t)i], &score[(size_t)i]) != 2) return 2;
    std::vector<int64_t> oi((size_t)k);
    std::vector<float> os((size_t)k);
    std::vector<uint32_t> ol((size_t)k);
    const bool fin = distinct_walk(idx.data(), score.data(), kp, n_rows, labels.data(), n_set, k, oi.data(), os.data(), ol.data());
    printf("%d\n", fin ? 1 : 0);
    for (int64_t r : oi) printf("%" PRId64 " ", r);
    printf("\n");
    for (float s : os) printf("%g ", s);
    printf("\n");
    print_u32(ol);
    return 0;
  }
  return 2;
}
