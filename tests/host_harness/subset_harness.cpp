// Drives the device-free host side of wdbx_index_search_rows (wdbx-py_amd/csrc/host_subset.h): validation and narrowing of a
// row list, and the route / query block / grid / scratch sizing.  tests/test_search_rows_host.py builds it with g++ (plain, and
// with -fsanitize=address,undefined) and checks the output.
//   "validate n_rows n_ids id..."   -> "first_bad <index>" (n_ids = valid) then "rows r..." (the narrowed list) when valid
//   "validate_big n_rows first n"   -> the same for the list first, first + 1, ... (n entries) without printing the rows
//   "plan cu keys_max select_min_k lds_lists", stdin: lines "n_ids nq k" -> per line "route qb round blocks P lds scratch_u64"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_subset.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "validate") && argc >= 4) {
    const uint64_t n_rows = strtoull(argv[2], nullptr, 10), n_ids = strtoull(argv[3], nullptr, 10);
    if ((uint64_t)argc != 4 + n_ids) return 2;
    // exact-size heap blocks: a read or write past either end is the sanitizer's to find
    std::vector<uint64_t> ids(n_ids);
    std::vector<uint32_t> out(n_ids);
    for (uint64_t i = 0; i < n_ids; ++i) ids[i] = strtoull(argv[4 + i], nullptr, 10);
    const uint64_t bad = subset_validate(ids.data(), n_ids, n_rows, out.data());
    const uint64_t bad_only = subset_validate(ids.data(), n_ids, n_rows, nullptr);
    if (bad != bad_only) return 3;
    printf("first_bad %" PRIu64 "\n", bad);
    if (bad == n_ids) {
      printf("rows");
      for (uint32_t r : out) printf(" %u", r);
      printf("\n");
    }
    return 0;
  }
  if (!strcmp(argv[1], "validate_big") && argc == 5) {
    const uint64_t n_rows = strtoull(argv[2], nullptr, 10), first = strtoull(argv[3], nullptr, 10), n = strtoull(argv[4], nullptr, 10);
    std::vector<uint64_t> ids(n);
    std::vector<uint32_t> out(n);
    for (uint64_t i = 0; i < n; ++i) ids[i] = first + i;
    const uint64_t bad = subset_validate(ids.data(), n, n_rows, out.data());
    printf("first_bad %" PRIu64 "\n", bad);
    for (uint64_t i = 0; i < bad; ++i)
      if ((uint64_t)out[i] != ids[i]) return 3;
    return 0;
  }
  if (!strcmp(argv[1], "plan") && argc == 6) {
    unsigned long long n_ids = 0;
    int nq = 0, k = 0;
    while (scanf("%llu %d %d", &n_ids, &nq, &k) == 3) {
      const SubsetPlan p = subset_plan(n_ids, nq, k, atoi(argv[2]), atoll(argv[3]), atoll(argv[4]), atoi(argv[5]) != 0);
      printf("%d %d %d %u %u %zu %zu\n", p.route, p.qb, p.round, p.blocks, p.P, p.lds, p.scratch_u64);
    }
    return 0;
  }
  return 2;
}
