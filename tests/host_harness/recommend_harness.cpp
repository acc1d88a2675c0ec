// Stand-alone driver of wdbx-py_amd/csrc/host_recommend.h (the device-free host side of wdbx_index_search_recommend) for
// tests/test_recommend_host.py: plain g++, once more under -fsanitize=address,undefined.
//   offsets  stdin: lines "nq off_0 .. off_(2 nq)" -> per line "ok" or the refusal's message
//   exclude  stdin: lines "n_rows n r_0 .. r_(n-1)" -> per line "ok r_0 .. r_(n-1)" (narrowed to 32 bits) or the message
//   plan     stdin: lines "n_rows nq k cu_count select_min_k lds_lists budget" -> per line
//                     mode round blocks P lds scratch_u64 example_blocks(k) | first count of every round
//   passes   stdin: "nq k round", then per query two lines "n id .. " : its favoured rows in rank order (any number), then its
//            disfavoured rows in rank order.  Simulates the call: the favoured pass in rounds of `round` queries (each list cut
//            at k, -1 padded), recommend_short, the table of the short queries, the disfavoured pass in rounds of the SHORT
//            queries, recommend_splice.  Scores: 0.5 * id on the favoured side, 0.25 * id on the other.  Prints
//            "short q:gap .." and per query "id:score:side .." (k slots).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_recommend.h"

static bool read_list(std::vector<int64_t>* v) {
  int n;
  if (scanf("%d", &n) != 1 || n < 0) return false;
  v->resize((size_t)n);
  for (auto& x : *v)
    if (scanf("%" SCNd64, &x) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::string msg;
  if (!strcmp(argv[1], "offsets")) {
    int nq;
    while (scanf("%d", &nq) == 1) {
      if (nq < 1) return 2;
      std::vector<uint64_t> off((size_t)2 * nq + 1);
      for (auto& x : off)
        if (scanf("%" SCNu64, &x) != 1) return 2;
      printf("%s\n", recommend_validate_offsets(off.data(), nq, &msg) ? "ok" : msg.c_str());
    }
    return 0;
  }
  if (!strcmp(argv[1], "exclude")) {
    uint64_t n_rows, n;
    while (scanf("%" SCNu64 " %" SCNu64, &n_rows, &n) == 2) {
      std::vector<uint64_t> rows((size_t)n);
      for (auto& x : rows)
        if (scanf("%" SCNu64, &x) != 1) return 2;
      std::vector<uint32_t> out((size_t)std::min<uint64_t>(n, RECOMMEND_MAX_EXCLUDE), 0xFFFFFFFFu);
      if (!recommend_validate_exclude(rows.data(), n, n_rows, out.data(), &msg)) {
        printf("%s\n", msg.c_str());
        continue;
      }
      printf("ok");
      for (uint32_t r : out) printf(" %u", r);
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(argv[1], "plan")) {
    uint64_t n_rows, budget;
    int nq, k, cu, lds_lists;
    long long select_min_k;
    while (scanf("%" SCNu64 " %d %d %d %lld %d %" SCNu64, &n_rows, &nq, &k, &cu, &select_min_k, &lds_lists, &budget) == 7) {
      const RecommendPlan p = recommend_plan(n_rows, nq, k, cu, select_min_k, lds_lists != 0, budget);
      printf("%d %d %u %u %zu %zu %d |", p.mode, p.round, p.blocks, p.P, p.lds, p.scratch_u64, recommend_example_blocks((uint64_t)k));
      for (const auto& r : recommend_rounds(nq, p.round)) printf(" %d %d", r.first, r.second);
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(argv[1], "passes")) {
    int nq, k, round;
    if (scanf("%d %d %d", &nq, &k, &round) != 3 || nq < 1 || k < 1 || round < 1) return 2;
    std::vector<std::vector<int64_t>> fav((size_t)nq), dis((size_t)nq);
    std::vector<uint64_t> off((size_t)2 * nq + 1, 0);
    for (int q = 0; q < nq; ++q) {
      if (!read_list(&fav[(size_t)q]) || !read_list(&dis[(size_t)q])) return 2;
      off[(size_t)2 * q + 1] = off[(size_t)2 * q] + 1 + (uint64_t)q % 3;
      off[(size_t)2 * q + 2] = off[(size_t)2 * q + 1] + (uint64_t)q % 2;
    }
    const size_t elems = (size_t)nq * k;
    std::vector<int64_t> fav_idx(elems, -7), out_idx(elems, -7);
    std::vector<float> fav_score(elems, -7.f), out_score(elems, -7.f);
    std::vector<uint8_t> out_side(elems, 7), seen((size_t)nq, 0);
    auto fill = [&](const std::vector<int64_t>& list, float scale, int64_t* idx, float* score) {
      for (int i = 0; i < k; ++i) {
        const bool have = (size_t)i < list.size();
        idx[i] = have ? list[(size_t)i] : -1;
        score[i] = have ? scale * (float)list[(size_t)i] : 0.0f;
      }
    };
    for (const auto& r : recommend_rounds(nq, round))
      for (int q = r.first; q < r.first + r.second; ++q) {
        if (seen[(size_t)q]++) return 3;  // (each query exactly once)
        fill(fav[(size_t)q], 0.5f, &fav_idx[(size_t)q * k], &fav_score[(size_t)q * k]);
      }
    for (uint8_t s : seen)
      if (s != 1) return 3;
    std::vector<uint32_t> short_queries;
    std::vector<int> gaps;
    recommend_short(fav_idx.data(), nq, k, &short_queries, &gaps);
    const size_t ns = short_queries.size();
    std::vector<uint32_t> table(ns * 3);
    recommend_table(off.data(), short_queries.data(), ns, table.data());
    std::vector<int64_t> dis_idx(ns * k, -7);
    std::vector<float> dis_score(ns * k, -7.f);
    for (const auto& r : recommend_rounds((int)ns, round))
      for (int s = r.first; s < r.first + r.second; ++s) {
        const uint32_t q = short_queries[(size_t)s];
        if (table[(size_t)3 * s] != off[(size_t)2 * q] || table[(size_t)3 * s + 1] != off[(size_t)2 * q + 1] ||
            table[(size_t)3 * s + 2] != off[(size_t)2 * q + 2])
          return 4;  // (the slot's table entry is its query's)
        fill(dis[q], 0.25f, &dis_idx[(size_t)s * k], &dis_score[(size_t)s * k]);
      }
    recommend_splice(fav_idx.data(), fav_score.data(), dis_idx.data(), dis_score.data(), short_queries, nq, k, out_idx.data(),
                     out_score.data(), out_side.data());
    printf("short");
    for (size_t s = 0; s < ns; ++s) printf(" %u:%d", short_queries[s], gaps[s]);
    printf("\n");
    for (int q = 0; q < nq; ++q) {
      for (int i = 0; i < k; ++i)
        printf("%s%" PRId64 ":%g:%d", i ? " " : "", out_idx[(size_t)q * k + i], (double)out_score[(size_t)q * k + i],
               (int)out_side[(size_t)q * k + i]);
      printf("\n");
    }
    // a second splice without out_side must write the same rows
    std::vector<int64_t> idx2(elems, -7);
    std::vector<float> score2(elems, -7.f);
    recommend_splice(fav_idx.data(), fav_score.data(), dis_idx.data(), dis_score.data(), short_queries, nq, k, idx2.data(),
                     score2.data(), nullptr);
    return idx2 == out_idx && score2 == out_score ? 0 : 5;
  }
  return 2;
}
