// Stand-alone driver of wdbx-py_amd/csrc/host_selection.h for tests/test_selection_plan_host.py (plain g++, no HIP).
// One mode per run, one case per input line, one output line per case:
//   selection_harness sample  < "n_rows tile_rows rw k div_option k_scaled factor"
//       -> div tiles sample_tiles stride bounds expect cap
//   selection_harness masked  < "n_rows tile_rows rw k div_option allowed"      (k_scaled = 1, factor = 32: the int8 tiles)
//       -> base_sample_tiles masked_sample_tiles stride bounds expect cap
//   selection_harness pairs   < "expect nwaves"     -> pair_cap
//   selection_harness gib     < "n_rows u8_pitch"   -> 0 | 1
#include <cstdio>
#include <cstring>

#include "host_selection.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  unsigned long long n, allowed, expect;
  unsigned tile_rows, rw, factor, nwaves, pitch;
  long long div_opt;
  int k, k_scaled;
  if (!strcmp(argv[1], "sample")) {
    while (scanf("%llu %u %u %d %lld %d %u", &n, &tile_rows, &rw, &k, &div_opt, &k_scaled, &factor) == 7) {
      const uint32_t div = selection_div(div_opt, k, k_scaled != 0);
      const SelectionSample s = selection_sample(n, tile_rows, rw, k, div);
      printf("%u %u %u %u %u %llu %u\n", div, s.tiles, s.sample_tiles, s.stride, s.bounds, (unsigned long long)s.expect,
             selection_cap(s.expect, factor));
    }
  } else if (!strcmp(argv[1], "masked")) {
    while (scanf("%llu %u %u %d %lld %llu", &n, &tile_rows, &rw, &k, &div_opt, &allowed) == 6) {
      const SelectionSample base = selection_sample(n, tile_rows, rw, k, selection_div(div_opt, k, true));
      const uint32_t grown = selection_sample_masked(base.sample_tiles, base.tiles, rw, k, n, allowed);
      const SelectionSample s = selection_of(base.tiles, grown, rw, k);
      if (s.sample_tiles != grown) return 3;  // (the masked sample comes back clamped)
      printf("%u %u %u %u %llu %u\n", base.sample_tiles, s.sample_tiles, s.stride, s.bounds, (unsigned long long)s.expect,
             selection_cap(s.expect, 32));
    }
  } else if (!strcmp(argv[1], "pairs")) {
    while (scanf("%llu %u", &expect, &nwaves) == 2) printf("%u\n", selection_pair_cap(expect, nwaves));
  } else if (!strcmp(argv[1], "gib")) {
    while (scanf("%llu %u", &n, &pitch) == 2) printf("%d\n", shadow_over_1gib(n, pitch) ? 1 : 0);
  } else {
    return 2;
  }
  return feof(stdin) ? 0 : 4;  // (a line that did not parse)
}
