// Stand-alone driver of wdbx-py_amd/csrc/host_discover.h (the device-free host side of wdbx_index_search_discover) for
// tests/test_discover_host.py: plain g++, once more under -fsanitize=address,undefined.
//   offsets  stdin: lines "target nq off_0 .. off_nq" -> per line "ok" or the refusal's message
//   plan     stdin: lines "n_rows nq k target cu_count select_min_k lds_lists budget" -> per line
//                     mode round blocks P lds scratch_u64 record_rows pair_blocks(k) | first count of every round
//   zplan    stdin: lines "n_rows slots k mode cu_count budget" -> per line round blocks P lds scratch_u64 | first count ..
//   zones    stdin: lines "k c_0 .. c_32" -> per line "zone:take .." from the top down
//   stage    stdin: "target nq dim off_0 .. off_nq": targets are rows of 100 + q, context vector v rows of 1000 + v -> the
//            staged vectors' first elements on one line, then the table "first:pairs .." of all queries
//   call     stdin: "nq k round", then per query 33 counts.  Simulates target mode: rounds of `round` queries, per round the
//            zones of its queries, a zone list per (query, zone) slot (k slots: rows 1000 * q + 10 * zone + i for i < count,
//            score 0.5 * row, -1 / 0 beyond), discover_splice into the caller's rows.  Prints "slots N" and per query
//            "id:score:wins .." (k slots).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_discover.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::string msg;
  if (!strcmp(argv[1], "offsets")) {
    int target, nq;
    while (scanf("%d %d", &target, &nq) == 2) {
      if (nq < 1) return 2;
      std::vector<uint64_t> off((size_t)nq + 1);
      for (auto& x : off)
        if (scanf("%" SCNu64, &x) != 1) return 2;
      printf("%s\n", discover_validate_offsets(off.data(), nq, target != 0, &msg) ? "ok" : msg.c_str());
    }
    return 0;
  }
  if (!strcmp(argv[1], "plan")) {
    uint64_t n_rows, budget;
    int nq, k, target, cu, lds_lists;
    long long select_min_k;
    while (scanf("%" SCNu64 " %d %d %d %d %lld %d %" SCNu64, &n_rows, &nq, &k, &target, &cu, &select_min_k, &lds_lists, &budget) == 8) {
      const DiscoverPlan p = discover_plan(n_rows, nq, k, target != 0, cu, select_min_k, lds_lists != 0, budget);
      printf("%d %d %u %u %zu %zu %zu %d |", p.mode, p.round, p.blocks, p.P, p.lds, p.scratch_u64, p.record_rows,
             discover_pair_blocks((uint64_t)k));
      for (const auto& r : recommend_rounds(nq, p.round)) printf(" %d %d", r.first, r.second);
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(argv[1], "zplan")) {
    uint64_t n_rows, budget;
    int slots, k, mode, cu;
    while (scanf("%" SCNu64 " %d %d %d %d %" SCNu64, &n_rows, &slots, &k, &mode, &cu, &budget) == 6) {
      const DiscoverZonePlan z = discover_zone_plan(n_rows, slots, k, mode, cu, budget);
      printf("%d %u %u %zu %zu |", z.round, z.blocks, z.P, z.lds, z.scratch_u64);
      for (const auto& r : recommend_rounds(slots, z.round)) printf(" %d %d", r.first, r.second);
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(argv[1], "zones")) {
    int k;
    while (scanf("%d", &k) == 1) {
      uint32_t counts[DISCOVER_ZONE_COUNT];
      for (auto& c : counts)
        if (scanf("%u", &c) != 1) return 2;
      const std::vector<DiscoverZone> z = discover_zones(counts, k);
      for (size_t i = 0; i < z.size(); ++i) printf("%s%u:%u", i ? " " : "", z[i].zone, z[i].take);
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(argv[1], "stage")) {
    int target, nq, dim;
    if (scanf("%d %d %d", &target, &nq, &dim) != 3 || nq < 1 || dim < 1) return 2;
    std::vector<uint64_t> off((size_t)nq + 1);
    for (auto& x : off)
      if (scanf("%" SCNu64, &x) != 1) return 2;
    if (!discover_validate_offsets(off.data(), nq, target != 0, &msg)) return 2;
    std::vector<float> targets((size_t)nq * dim), context((size_t)(2 * off[(size_t)nq]) * dim);
    for (int q = 0; q < nq; ++q)
      for (int d = 0; d < dim; ++d) targets[(size_t)q * dim + d] = 100.0f + (float)q;
    for (size_t v = 0; v < 2 * off[(size_t)nq]; ++v)
      for (int d = 0; d < dim; ++d) context[v * dim + d] = 1000.0f + (float)v;
    const uint64_t staged = discover_staged_count(off.data(), nq, target != 0);
    std::vector<float> out((size_t)staged * dim, -1.0f);
    discover_stage(target ? targets.data() : nullptr, context.data(), off.data(), nq, dim, out.data());
    for (uint64_t v = 0; v < staged; ++v) {
      for (int d = 1; d < dim; ++d)
        if (out[(size_t)v * dim + d] != out[(size_t)v * dim]) return 3;  // (whole vectors were copied)
      printf("%s%g", v ? " " : "", (double)out[(size_t)v * dim]);
    }
    printf("\n");
    std::vector<uint32_t> table((size_t)nq * 2), part(2);
    discover_table(off.data(), 0, nq, target != 0, table.data());
    for (int q = 0; q < nq; ++q) {
      discover_table(off.data(), q, 1, target != 0, part.data());
      if (part[0] != table[(size_t)2 * q] || part[1] != table[(size_t)2 * q + 1]) return 4;  // (a round's table is a slice)
      printf("%s%u:%u", q ? " " : "", table[(size_t)2 * q], table[(size_t)2 * q + 1]);
    }
    printf("\n");
    return 0;
  }
  if (!strcmp(argv[1], "call")) {
    int nq, k, round;
    if (scanf("%d %d %d", &nq, &k, &round) != 3 || nq < 1 || k < 1 || round < 1) return 2;
    std::vector<uint32_t> counts((size_t)nq * DISCOVER_ZONE_COUNT);
    for (auto& c : counts)
      if (scanf("%u", &c) != 1) return 2;
    const size_t elems = (size_t)nq * k;
    std::vector<int64_t> out_idx(elems, -7), idx2(elems, -7);
    std::vector<float> out_score(elems, -7.f), score2(elems, -7.f);
    std::vector<uint8_t> out_wins(elems, 7), seen((size_t)nq, 0);
    size_t total = 0;
    for (const auto& r : recommend_rounds(nq, round)) {
      std::vector<std::vector<DiscoverZone>> zones((size_t)r.second);
      std::vector<int64_t> z_idx;
      std::vector<float> z_score;
      for (int s = 0; s < r.second; ++s) {
        const int q = r.first + s;
        if (seen[(size_t)q]++) return 3;  // (each query exactly once)
        zones[(size_t)s] = discover_zones(&counts[(size_t)q * DISCOVER_ZONE_COUNT], k);
        for (const DiscoverZone& z : zones[(size_t)s]) {
          const uint32_t have = counts[(size_t)q * DISCOVER_ZONE_COUNT + z.zone];
          for (int i = 0; i < k; ++i) {
            const int64_t row = 1000 * q + 10 * (int64_t)z.zone + i;
            z_idx.push_back((uint32_t)i < have ? row : -1);
            z_score.push_back((uint32_t)i < have ? 0.5f * (float)row : 0.0f);
          }
          ++total;
        }
      }
      const size_t o = (size_t)r.first * k;
      discover_splice(zones, z_idx.data(), z_score.data(), k, &out_idx[o], &out_score[o], &out_wins[o]);
      discover_splice(zones, z_idx.data(), z_score.data(), k, &idx2[o], &score2[o], nullptr);
    }
    for (uint8_t s : seen)
      if (s != 1) return 3;
    printf("slots %zu\n", total);
    for (int q = 0; q < nq; ++q) {
      for (int i = 0; i < k; ++i)
        printf("%s%" PRId64 ":%g:%d", i ? " " : "", out_idx[(size_t)q * k + i], (double)out_score[(size_t)q * k + i],
               (int)out_wins[(size_t)q * k + i]);
      printf("\n");
    }
    return idx2 == out_idx && score2 == out_score ? 0 : 5;  // (a splice without out_wins writes the same rows)
  }
  return 2;
}
