// copies_harness.cpp -- stand-alone driver of wdbx-py_amd/csrc/host_copies.h (the coverage of one derived copy of the rows, its
// transitions and the decision whether its allocations may stay) for the CPU suite (tests/test_copies_host.py): plain g++, no
// HIP.  Built once plain and once under -fsanitize=address,undefined.
//
//   copies_harness overlap ROWS GRANULE FIRST END
//     -> "first end" of the part of rows [FIRST, END) a copy of ROWS rows holds, or "empty"
//   copies_harness drive GRANULE op op ...
//     one coverage, starting at 0 rows, through the ops e<n> (extended_to n), c<m> (cut at first moved row m), r (reset),
//     = (nothing) and ?<n> (covers n): one line per op, the rows covered after it -- for ?<n>, "yes" or "no"
//   copies_harness room SHAPE_CHANGED PART_TOO_SMALL REFUSED_HERE
//     -> "kept", "fresh" or "no room"
//   copies_harness life REMEMBERS step step ...
//     a copy whose parts are always too small, asked for room at the capacities f<cap> (the allocation fails) and s<cap> (it
//     succeeds): one line per step, the decision before the allocation is tried
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host_copies.h"

static const char* room_name(int room) { return room == SHADOW_KEPT ? "kept" : room == SHADOW_FRESH ? "fresh" : "no room"; }

int main(int argc, char** argv) {
  if (argc == 6 && !strcmp(argv[1], "overlap")) {
    CopyCoverage c;
    c.rows = strtoull(argv[2], nullptr, 10);
    c.granule = (uint32_t)strtoul(argv[3], nullptr, 10);
    const RowRange r = c.overlap(strtoull(argv[4], nullptr, 10), strtoull(argv[5], nullptr, 10));
    if (r.empty())
      printf("empty\n");
    else
      printf("%" PRIu64 " %" PRIu64 "\n", r.first, r.end);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "drive")) {
    CopyCoverage c;
    c.granule = (uint32_t)strtoul(argv[2], nullptr, 10);
    for (int i = 3; i < argc; ++i) {
      const uint64_t v = argv[i][0] ? strtoull(argv[i] + 1, nullptr, 10) : 0;
      switch (argv[i][0]) {
        case 'e': c.extended_to(v); break;
        case 'c': c.cut(v); break;
        case 'r': c.reset(); break;
        case '=': break;
        case '?': printf("%s\n", c.covers(v) ? "yes" : "no"); continue;
        default: fprintf(stderr, "unknown op %s\n", argv[i]); return 1;
      }
      printf("%" PRIu64 "\n", c.rows);
    }
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "room")) {
    printf("%s\n", room_name(copy_room_decision(atoi(argv[2]) != 0, atoi(argv[3]) != 0, atoi(argv[4]) != 0)));
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "life")) {
    CopyCoverage c;
    c.remembers = atoi(argv[2]) != 0;
    for (int i = 3; i < argc; ++i) {
      const uint64_t cap = argv[i][0] ? strtoull(argv[i] + 1, nullptr, 10) : 0;
      const int room = copy_room_decision(false, true, c.refused_at(cap));
      if (room == SHADOW_FRESH && argv[i][0] == 'f') c.refuse_at(cap);
      printf("%s\n", room_name(room));
    }
    return 0;
  }
  fprintf(stderr, "usage: copies_harness overlap ROWS GRANULE FIRST END | drive GRANULE op ... | room S P R | life REMEMBERS step ...\n");
  return 1;
}
