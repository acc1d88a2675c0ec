// Stand-alone driver of wdbx-py_amd/csrc/host_scan_plan.h for tests/test_scan_plan_host.py (plain g++, no HIP).
// One mode per run, one case per input line, one output line per case:
//   scan_plan_harness form    < "pitch4 lanes generic force_ragged"  -> L QPL ragged generic passes_in_flight lds_extra
//   scan_plan_harness listed  < "pitch4"                             -> L lds_extra          (the generic / listed lane count)
//   scan_plan_harness has     < "L QPL"                              -> 0 | 1                (scan_has_instance)
//   scan_plan_harness range   < "pitch4"                             -> P NI
//   scan_plan_harness plan    < "n_rows L k select lds_lists lds_extra cu_count per_cu opt_blocks wg_merge blocked"
//       -> mode groups max_blocks blocks partial_lists chunk lds_bytes needs_attribute
#include <cstdio>
#include <cstring>

#include "host_scan_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  int pitch4, generic, force_ragged, L, qpl, k, select, lds_lists, per_cu, wg_merge, blocked;
  long long lanes, opt_blocks;
  unsigned long long n, lds_extra;
  unsigned cu_count, p4;
  if (!strcmp(argv[1], "form")) {
    while (scanf("%d %lld %d %d", &pitch4, &lanes, &generic, &force_ragged) == 4) {
      const ScanForm f = scan_form(pitch4, lanes, generic != 0, force_ragged != 0);
      printf("%d %d %d %d %d %zu\n", f.L, f.QPL, f.ragged ? 1 : 0, f.generic ? 1 : 0, f.generic ? 1 : scan_passes_in_flight(f.QPL),
             scan_lds_extra(f.generic, pitch4));
    }
  } else if (!strcmp(argv[1], "listed")) {
    while (scanf("%d", &pitch4) == 1) {
      const ScanForm f = scan_generic_form(pitch4);
      if (!f.generic || f.ragged || f.QPL != 0 || f.L != scan_generic_lanes(pitch4)) return 3;
      printf("%d %zu\n", f.L, scan_lds_extra(true, pitch4));
    }
  } else if (!strcmp(argv[1], "has")) {
    while (scanf("%d %d", &L, &qpl) == 2) printf("%d\n", scan_has_instance(L, qpl) ? 1 : 0);
  } else if (!strcmp(argv[1], "range")) {
    while (scanf("%u", &p4) == 1) {
      const RangeForm f = range_scan_form(p4);
      printf("%d %d\n", f.P, f.NI);
    }
  } else if (!strcmp(argv[1], "plan")) {
    while (scanf("%llu %d %d %d %d %llu %u %d %lld %d %d", &n, &L, &k, &select, &lds_lists, &lds_extra, &cu_count, &per_cu, &opt_blocks,
                 &wg_merge, &blocked) == 11) {
      const uint32_t groups = scan_groups(n, L);
      const uint32_t blocks = scan_blocks(cu_count, per_cu, opt_blocks, groups);
      const size_t lds = scan_lds_bytes(select != 0, k, (size_t)lds_extra);
      printf("%d %u %u %u %u %u %zu %d\n", scan_list_mode(select != 0, k, lds_lists != 0), groups, scan_max_blocks(groups), blocks,
             scan_partial_lists(wg_merge != 0, blocks), scan_chunk(blocked != 0, groups, blocks), lds,
             scan_lds_needs_attribute(lds) ? 1 : 0);
    }
  } else {
    return 2;
  }
  return feof(stdin) ? 0 : 4;  // (a line that did not parse)
}
