// Drives the device-free host side of wdbx_index_seed_centers (wdbx-py_amd/csrc/host_seed.h) for tests/test_seed_host.py:
// built with plain g++, once as it is and once under -fsanitize=address,undefined.
//   weight   L2 SCORE(hex float) SHIFT            -> the weight
//   shift    MAX_NORM2(hex float)                 -> the shift
//   mulhi    DRAW W (decimal 64-bit)              -> the target
//   validate N_CENTERS N_TRIALS HAVE_DRAWS HAVE_ROWS -> the check
//   plan     N_ROWS N_CENTERS N_TRIALS PITCH CUS MAX_RESIDENT
//            -> fits resident passes lds eval_grid span blocks apply_grid state_bytes scratch_bytes ordered
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host_seed.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "weight") && argc == 5) return printf("%u\n", seed_weight(atoi(argv[2]) != 0, strtof(argv[3], nullptr), atoi(argv[4]))) < 0;
  if (!strcmp(argv[1], "shift") && argc == 3) return printf("%d\n", seed_shift(strtof(argv[2], nullptr))) < 0;
  if (!strcmp(argv[1], "mulhi") && argc == 4)
    return printf("%llu\n", (unsigned long long)seed_mulhi64(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10))) < 0;
  if (!strcmp(argv[1], "validate") && argc == 6)
    return printf("%d\n", (int)seed_validate(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]) != 0, atoi(argv[5]) != 0)) < 0;
  if (!strcmp(argv[1], "plan") && argc == 8) {
    const SeedPlan p = seed_plan(strtoull(argv[2], nullptr, 10), atoi(argv[3]), atoi(argv[4]), (uint32_t)atoll(argv[5]), atoi(argv[6]),
                                 strtoull(argv[7], nullptr, 10));
    // the regions of the state allocation follow one another without overlap, each aligned for its type
    const int ordered = p.off_dead <= p.off_sums && p.off_sums <= p.off_pot && p.off_pot < p.off_cand && p.off_cand < p.off_rows &&
                        p.off_rows <= p.off_outpot && p.off_outpot <= p.off_draws && p.off_draws <= p.state_bytes &&
                        p.off_sums % 8 == 0 && p.off_rows % 8 == 0 && p.off_dead % 4 == 0;
    printf("%d %u %u %zu %u %u %u %u %zu %zu %d\n", (int)p.fits, p.resident, p.passes, p.lds, p.eval_grid, p.span, p.blocks, p.apply_grid,
           p.state_bytes, p.scratch_bytes, ordered);
    return 0;
  }
  return 2;
}
