// Drives the device-free host side of wdbx_index_search_row_lists (wdbx-py_amd/csrc/host_rowlists.h): the check of the CSR
// pair, the validation of the lists, and the plan (routes, slots, rounds, query blocks, work items).
// tests/test_row_lists_host.py builds it with g++ (plain, and with -fsanitize=address,undefined) and checks the output.
//   "check", stdin: "n_lists nq", the n_lists + 1 offsets, the nq list numbers -> "check <code> <where>"
//   "validate n_rows", stdin: "n_lists", the offsets, every row -> "valid" or "bad <list> <entry>"
//   "plan keys_max", stdin: "n_lists nq", the offsets, the list numbers -> the plan, one record per line:
//       "plan <qb> <path> <pass_ids> <slots>", "routes r...", "bases b...", "slot_query q...", "slot_len n...",
//       "round <slot0> <slots> <item0> <items> <stride>" per round, "item <first> <n> <slot> <nq> <offset>" per item
//   A plan is also run through rowlists_validate with rows 0, 1, ... per list, narrowing into an exact-size block.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_rowlists.h"

static bool read_u64(uint64_t* v) {
  unsigned long long x = 0;
  if (scanf("%llu", &x) != 1) return false;
  *v = x;
  return true;
}

static bool read_pair(int n_lists, int nq, std::vector<uint64_t>* offsets, std::vector<int32_t>* which) {
  // exact-size heap blocks: a read past either end is the sanitizer's to find
  offsets->resize((size_t)n_lists + 1);
  which->resize((size_t)nq);
  for (uint64_t& o : *offsets)
    if (!read_u64(&o)) return false;
  for (int32_t& w : *which) {
    long long x = 0;
    if (scanf("%lld", &x) != 1) return false;
    w = (int32_t)x;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "check") && argc == 2) {
    int n_lists = 0, nq = 0;
    if (scanf("%d %d", &n_lists, &nq) != 2 || n_lists < 0 || nq < 0) return 2;
    std::vector<uint64_t> offsets;
    std::vector<int32_t> which;
    if (!read_pair(n_lists, nq, &offsets, &which)) return 2;
    int64_t where = -7;
    const int code = rowlists_check(offsets.data(), n_lists, which.data(), nq, &where);
    if (code != rowlists_check(offsets.data(), n_lists, which.data(), nq, nullptr)) return 3;
    printf("check %d %" PRId64 "\n", code, where);
    return 0;
  }
  if (!strcmp(argv[1], "validate") && argc == 3) {
    const uint64_t n_rows = strtoull(argv[2], nullptr, 10);
    int n_lists = 0;
    if (scanf("%d", &n_lists) != 1 || n_lists < 1) return 2;
    std::vector<uint64_t> offsets((size_t)n_lists + 1);
    for (uint64_t& o : offsets)
      if (!read_u64(&o)) return 2;
    std::vector<uint64_t> rows((size_t)offsets.back());
    for (uint64_t& r : rows)
      if (!read_u64(&r)) return 2;
    int bad_list = -1;
    uint64_t bad_entry = 0;
    if (rowlists_validate(rows.data(), offsets.data(), n_lists, n_rows, nullptr, nullptr, &bad_list, &bad_entry))
      printf("valid\n");
    else
      printf("bad %d %" PRIu64 "\n", bad_list, bad_entry);
    return 0;
  }
  if (!strcmp(argv[1], "plan") && argc == 3) {
    const int64_t keys_max = atoll(argv[2]);
    int n_lists = 0, nq = 0;
    if (scanf("%d %d", &n_lists, &nq) != 2 || n_lists < 1 || nq < 1) return 2;
    std::vector<uint64_t> offsets;
    std::vector<int32_t> which;
    if (!read_pair(n_lists, nq, &offsets, &which)) return 2;
    if (rowlists_check(offsets.data(), n_lists, which.data(), nq, nullptr) != ROWLISTS_OK) return 2;
    RowListsPlan p;
    if (!rowlists_plan(offsets.data(), n_lists, which.data(), nq, keys_max, &p)) {
      printf("refused\n");
      return 0;
    }
    // every list holds rows 0, 1, ...: valid for an index of as many rows as the longest list
    std::vector<uint64_t> rows((size_t)offsets.back());
    uint64_t longest = 0;
    for (int l = 0; l < n_lists; ++l) {
      for (uint64_t i = offsets[l]; i < offsets[l + 1]; ++i) rows[i] = i - offsets[l];
      longest = std::max(longest, offsets[l + 1] - offsets[l]);
    }
    std::vector<uint32_t> ids32((size_t)p.pass_ids);
    int bad_list = -1;
    uint64_t bad_entry = 0;
    if (!rowlists_validate(rows.data(), offsets.data(), n_lists, longest, &p, ids32.data(), &bad_list, &bad_entry)) return 3;
    for (int l = 0; l < n_lists; ++l)
      if (p.list_route[(size_t)l] == ROWLISTS_ROUTE_PASS)
        for (uint64_t i = 0; i < offsets[l + 1] - offsets[l]; ++i)
          if (ids32[(size_t)(p.list_base[(size_t)l] + i)] != (uint32_t)i) return 3;
    printf("plan %d %d %" PRIu64 " %zu\n", p.qb, p.path(), p.pass_ids, p.slot_query.size());
    printf("routes");
    for (uint8_t r : p.list_route) printf(" %d", (int)r);
    printf("\nbases");
    for (uint64_t b : p.list_base) printf(" %" PRIu64, b);
    printf("\nslot_query");
    for (int32_t q : p.slot_query) printf(" %d", q);
    printf("\nslot_len");
    for (uint32_t n : p.slot_len) printf(" %u", n);
    printf("\n");
    for (const RowListsRound& r : p.rounds) printf("round %u %u %zu %zu %" PRIu64 "\n", r.slot0, r.slots, r.item0, r.items, r.stride);
    for (const RowListsItem& it : p.items) printf("item %u %u %u %u %u\n", it.first, it.n, it.slot, it.nq, it.offset);
    return 0;
  }
  return 2;
}
