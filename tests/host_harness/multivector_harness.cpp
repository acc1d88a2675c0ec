// Stand-alone driver of wdbx-py_amd/csrc/host_multivector.h (the device-free host side of wdbx_index_search_multivector) for
// tests/test_multivector_host.py: plain g++, once more under -fsanitize=address,undefined.
//   plan CU SELMIN   stdin: lines "n_items n_labels n_spans k round_option nq c_0 .. c_(nq-1)" (c_i = vectors of query i)
//                    -> three lines per case:
//                       qb round_max floor select score_blocks rank_blocks lds keys_u64 rank_u64 n_rounds n_segments
//                       per round:   first vectors seg0 segs ranked ranked_query0
//                       per segment: query v0 v1 slot carry      (slot -1 = the segment carries out)
//   row0             stdin: n, n_set, then n_set labels  -> label_row0 of the label order (the smallest row of each label)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_multivector.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "plan") && argc == 4) {
    const int cu = atoi(argv[2]);
    const long long sel = atoll(argv[3]);
    unsigned n_items, n_labels, n_spans;
    int k, nq;
    long long opt;
    while (scanf("%u %u %u %d %lld %d", &n_items, &n_labels, &n_spans, &k, &opt, &nq) == 6) {
      if (nq < 1) return 2;
      std::vector<uint64_t> off((size_t)nq + 1, 0);
      for (int i = 0; i < nq; ++i) {
        unsigned long long c;
        if (scanf("%llu", &c) != 1 || c < 1) return 2;
        off[(size_t)i + 1] = off[(size_t)i] + c;
      }
      const MultivectorPlan p = multivector_plan(off.data(), nq, n_items, n_labels, n_spans, k, cu, sel, opt);
      printf("%d %d %d %d %u %u %zu %zu %zu %zu %zu\n", p.qb, p.round_max, p.floor ? 1 : 0, p.select ? 1 : 0, p.score_blocks,
             p.rank_blocks, p.lds, p.keys_u64, p.rank_u64, p.rounds.size(), p.segments.size());
      for (const MultivectorRound& r : p.rounds)
        printf("%" PRIu64 " %u %u %u %u %u ", r.first, r.vectors, r.seg0, r.segs, r.ranked, r.ranked_query0);
      printf("\n");
      for (const MultivectorSegment& s : p.segments)
        printf("%u %u %u %lld %u ", s.query, s.v0, s.v1, s.slot == MULTIVECTOR_NO_SLOT ? -1ll : (long long)s.slot, s.carry);
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(argv[1], "row0")) {
    unsigned long long n = 0, n_set = 0;
    if (scanf("%llu %llu", &n, &n_set) != 2 || n_set > n) return 2;
    std::vector<uint32_t> labels((size_t)n_set);
    for (auto& l : labels)
      if (scanf("%" SCNu32, &l) != 1) return 2;
    LabelOrder o;
    label_order_build(labels.data(), n_set, n, &o);
    if (o.label_row0.size() != o.n_labels) return 3;
    for (uint32_t x : o.label_row0) printf("%u ", x);
    printf("\n");
    return 0;
  }
  return 2;
}
