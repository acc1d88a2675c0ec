// host_selection.h -- the device-free plan of the selection rounds: how many tiles a top-k query samples, at what stride, and
// how many candidates its buffers hold.  One rule for the four paths that answer a query by sample -> threshold -> full pass ->
// fp32 re-scoring -> final top-k (host_index.h): the legacy fp32 / bf16 tiles, the int8 tiles, the u8 rounds and the u6 rounds.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/selection_harness.cpp (plain g++ in the CPU suite,
// tests/test_selection_plan_host.py).  No HIP, no kernel types in here.
//
// A path names four numbers: the rows of a sampled tile, the lower bounds a tile reports per query (rw), the divisor rule
// and the capacity factor.  Everything is 32-bit arithmetic on tile counts (row counts stay below 2^32 - 256) except the
// expected candidates and the capacities, which are taken in 64 bits and clamped.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

// sampled fraction 1 / div: option gemm_sample_div when set; else 32, or (k_scaled: every path whose selection scores carry
// an error margin that multiplies the candidates -- all but the exact fp32 tiles) a larger sample for a larger k
static inline uint32_t selection_div(int64_t opt_sample_div, int k, bool k_scaled) {
  if (opt_sample_div > 0) return (uint32_t)opt_sample_div;
  return k_scaled ? std::min(32u, std::max(4u, 1024u / (uint32_t)k)) : 32u;
}

struct SelectionSample {
  uint32_t tiles;         // tiles of tile_rows rows that hold the corpus
  uint32_t sample_tiles;  // how many of them the sample pass visits: tiles 0, stride, 2 stride, ...
  uint32_t stride;
  uint32_t bounds;        // lower bounds per query the sample reports (rw per tile); fewer than k = the corpus is too small
  uint64_t expect;        // rows expected above the threshold: k * (tiles / sample_tiles + 1)
};

// ... for a sample of sample_tiles of the tiles (clamped to [1, tiles])
static inline SelectionSample selection_of(uint32_t tiles, uint32_t sample_tiles, uint32_t rw, int k) {
  SelectionSample s;
  s.tiles = tiles;
  s.sample_tiles = std::max<uint32_t>(1, std::min(sample_tiles, tiles));
  s.stride = tiles / s.sample_tiles;
  s.bounds = rw * s.sample_tiles;
  s.expect = (uint64_t)k * (tiles / s.sample_tiles + 1);
  return s;
}

// the sample of a call without a row mask: a fraction 1 / div of the tiles, at least the tiles that report 8 k bounds
static inline SelectionSample selection_sample(uint64_t n_rows, uint32_t tile_rows, uint32_t rw, int k, uint32_t div) {
  const uint32_t tiles = (uint32_t)((n_rows + tile_rows - 1) / tile_rows);
  return selection_of(tiles, std::max<uint32_t>(tiles / div, (8u * k + rw - 1) / rw), rw, k);
}

// the sampled tiles of a call (or, with a mask per query, of one block) whose mask allows `allowed` of the n_rows rows (never
// more than n_rows: the allowed rows are counted up to the last row); base_sample_tiles = selection_sample()'s
static inline uint32_t selection_sample_masked(uint32_t base_sample_tiles, uint32_t tiles, uint32_t rw, int k, uint64_t n_rows,
                                               uint64_t allowed) {
  uint32_t sample_tiles = base_sample_tiles;
  // (a mask of at most 16 384 rows: the candidate buffers hold ALL of them, so tau = -inf is answered from the candidates and
  // a larger sample would buy nothing: the sample stays what an unmasked call takes)
  if (allowed > 16384) {
    // A row mask that allows a fraction f of the rows: only blocks holding an allowed row vouch, and each for the best of its
    // ~32 f allowed rows.  tau is then the k-th best of ~(sampled rows) x f rows and the full pass keeps ~k x rows / (sampled
    // rows) of the allowed ones: the candidates per query do not grow with 1 / f, but the VOUCHING blocks shrink -- a fraction
    // 1 - (1 - f)^32 of the sampled ones.  So the sample grows by 1 / f, up to 8 x (a quarter of the corpus at the default
    // 1 / 32: beyond that the sample pass would cost what the full pass does), and further only while fewer than 8 k sampled
    // blocks are expected to vouch; clamped to all tiles.  Fewer than k vouching blocks leave tau = -inf: every allowed row is a
    // candidate, what does not fit is repaired by the masked fp32 scan.  
    const double f = n_rows ? (double)allowed / (double)n_rows : 0.0;
    if (f > 0.0) {
      const double pv = 1.0 - std::pow(1.0 - std::min(f, 1.0), 32.0);
      const double scaled = (double)sample_tiles * std::min(1.0 / f, 8.0), vouch = (8.0 * k) / (rw * std::max(pv, 1e-9));
      sample_tiles = (uint32_t)std::min<double>(std::ceil(std::max(scaled, vouch)), (double)tiles);
    }
  }
  return std::max<uint32_t>(1, std::min(sample_tiles, tiles));
}

// candidate keys per query: factor x the expected rows (the path's margin: how loose its bounds are), at least 4096, at most 2^22
static inline uint32_t selection_cap(uint64_t expect, uint32_t factor) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(4096, expect * factor), 1u << 22);
}

// the int8 tiles' per-wave (query, row) pair lists: 4 x the share one of nwaves waves expects of a full query block, at least
// 16384 pairs (two tiles' worth of "every row of the wave's group is a candidate for every query", so a few outlier groups do
// not turn the call into per-query repairs), at most 2^16
constexpr uint32_t SELECTION_BLOCK_QUERIES = 256;  // the widest query block of the tile kernels
static inline uint32_t selection_pair_cap(uint64_t expect, uint32_t nwaves) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(16384, (uint64_t)SELECTION_BLOCK_QUERIES * expect * 16 / nwaves), 1u << 16);
}

// The split planes' full passes of a round (kernels_scan42.h): up to qp (1, 2 or 4) consecutive queries share one read of the
// four-bit plane.  The round's nv queries go as nv / qp groups of qp; what is left goes as one group of 2 and / or one lone
// query (5 at qp = 4: {0 .. 3} {4}; 7: {0 .. 3} {4, 5} {6}) -- no dummy query is scanned, at most two groups are narrower than
// qp.  first[i], width[i]: group i's first query and its number of queries (a width the kernel has an instance for); both hold
// nv entries at least.  Returns the number of groups.
static inline uint32_t u42_share_groups(uint32_t nv, uint32_t qp, uint32_t* first, uint32_t* width) {
  uint32_t n = 0, at = 0;
  for (uint32_t w = qp >= 4 ? 4 : qp >= 2 ? 2 : 1; w >= 1; w /= 2)
    for (; nv - at >= w; at += w) first[n] = at, width[n++] = w;
  return n;
}

// The split planes' full passes on the matrix cores (scan_u42_mfma_kernel): 16 consecutive queries of the round per group.  The
// round's nv queries go as nv / 16 full groups from query 0; a remainder of at least min_short queries goes as one short group
// behind them (its absent columns are never written); a smaller remainder is left to u42_share_groups.  Returns the number of
// groups; *covered = the queries they take, [0, *covered) of the round: the VALU groups start there.
constexpr uint32_t U42_MFMA_GROUP = 16;
static inline uint32_t u42_mfma_groups(uint32_t nv, uint32_t min_short, uint32_t* covered) {
  const uint32_t full = nv / U42_MFMA_GROUP, rest = nv % U42_MFMA_GROUP;
  const bool tail = rest > 0 && rest >= min_short;
  *covered = full * U42_MFMA_GROUP + (tail ? rest : 0u);
  return full + (tail ? 1u : 0u);
}

// "the u8 shadow exceeds 1 GiB": the size from which a pass per launch is the rule (u8_pitch bytes per row).  The u6 and u42
// scans are taken by size above it, a round's passes go out as one grid up to it.
static inline bool shadow_over_1gib(uint64_t n_rows, uint32_t u8_pitch) { return n_rows * u8_pitch > (1ull << 30); }
