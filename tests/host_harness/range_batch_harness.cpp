// Stand-alone driver of wdbx-py_amd/csrc/host_range_batch.h for tests/test_range_batch_host.py (plain g++, no HIP).
//   range_batch_harness route  <n_rows> <nq> <l2> <i8_pitch> <shadow_fits> <gemm_bf16> <gemm8_variant> <gemm_masked>
//                              <gemm_min_rows> <gemm_min_work> <min_queries> <has_mask>      -> "tiles <0|1> block <queries per block>"
//   range_batch_harness blocks <nq> <max_block> <forced_ct>                                  -> one "q0 nv ct" line per block
//   range_batch_harness sizes  <nv> <ct> <cap> <pair_cap_option> <n_rows> <cus> <i8_pitch>   -> "name value" lines
//   range_batch_harness tally  <nq> <max_block> <lost block> <lost block> ...                -> path, counts, the per-query flags
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_range_batch.h"

static long long num(char** argv, int i) { return atoll(argv[i]); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "route") && argc == 14) {
    RangeBatchShape s = {};
    s.n_rows = (uint64_t)num(argv, 2);
    s.nq = (int)num(argv, 3);
    s.metric_l2 = (int)num(argv, 4);
    s.i8_pitch = (uint32_t)num(argv, 5);
    s.shadow_fits = (int)num(argv, 6);
    s.gemm_bf16 = num(argv, 7);
    s.gemm8_variant = num(argv, 8);
    s.gemm_masked = num(argv, 9);
    s.gemm_min_rows = num(argv, 10);
    s.gemm_min_work = num(argv, 11);
    s.min_queries = num(argv, 12);
    s.has_mask = (int)num(argv, 13);
    printf("tiles %d block %d\n", range_batch_use_tiles(s) ? 1 : 0, range_batch_block_queries(s.metric_l2, s.i8_pitch));
    return 0;
  }
  if (!strcmp(argv[1], "blocks") && argc == 5) {
    for (const RangeBatchBlock& b : range_batch_blocks((int)num(argv, 2), (int)num(argv, 3), (int)num(argv, 4)))
      printf("%d %d %d\n", b.q0, b.nv, b.ct);
    return 0;
  }
  if (!strcmp(argv[1], "sizes") && argc == 9) {
    const RangeBatchBlock b = {0, (int)num(argv, 2), (int)num(argv, 3)};
    const uint32_t cap = (uint32_t)num(argv, 4), pair_cap = range_batch_pair_cap(num(argv, 5));
    const uint32_t waves = range_batch_waves((uint64_t)num(argv, 6), (uint32_t)num(argv, 7));
    const RangeBatchSizes s = range_batch_sizes(b, cap, pair_cap, waves, (uint32_t)num(argv, 8));
    printf("pair_cap %u\nwaves %u\npairs %zu\npair_count %zu\ncand %zu\nkeys %zu\ncount %zu\nrcnt %zu\nthr %zu\nqb8 %zu\nqpar %zu\ntau %zu\nfits %d\n",
           pair_cap, waves, s.pairs_bytes, s.pair_count_bytes, s.cand_bytes, s.keys_bytes, s.count_bytes, s.rcnt_bytes, s.thr_bytes,
           s.qb8_bytes, s.qpar_bytes, s.tau_bytes, range_batch_cap_fits(b, cap) ? 1 : 0);
    return 0;
  }
  if (!strcmp(argv[1], "tally") && argc >= 4) {
    const int nq = (int)num(argv, 2);
    const std::vector<RangeBatchBlock> blocks = range_batch_blocks(nq, (int)num(argv, 3), 0);
    std::vector<char> is_lost(blocks.size(), 0);
    for (int i = 4; i < argc; ++i) {
      const long long b = num(argv, i);
      if (b < 0 || b >= (long long)blocks.size()) return 2;
      is_lost[(size_t)b] = 1;
    }
    RangeBatchTally t;
    t.start(nq);
    for (size_t b = 0; b < blocks.size(); ++b) {
      if (is_lost[b]) t.lost(blocks[b], 7);
      else t.tiles(blocks[b], 100);
    }
    printf("path %d blocks %lld tile_blocks %lld fallback %lld pairs %lld\nflags", t.path(), (long long)t.blocks, (long long)t.tile_blocks,
           (long long)t.fallback_queries, (long long)t.pairs);
    for (const uint8_t f : t.per_query) printf(" %d", (int)f);
    printf("\n");
    return 0;
  }
  return 2;
}
