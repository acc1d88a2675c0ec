// host_mmr.h -- the device-free host side of wdbx_index_search_mmr (maximal marginal relevance: a diversified top-k picked
// greedily from the pool of the fetch_k best rows): the argument checks, the pool of a query, the cut of a call's queries into
// rounds that keep the gathered rows and the similarity squares within the scratch budget, the grids and the instance picker
// of the pairs kernel.  Included by wdbx_hip.hip (behind host_labels.h, whose scratch budget it uses) and, on its own, by
// tests/host_harness/mmr_harness.cpp (plain g++ in the CPU suite, tests/test_mmr_host.py).  No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_labels.h"
#include "host_subset.h"

constexpr int MMR_MAX_POOL = 2048;        // (= WDBX_MAX_K) candidates of one query; 8 per thread of the selection workgroup
constexpr int MMR_BLOCK = 8;              // candidate columns one wave scores a fetched row against (mmr_pairs_kernel's QB)
constexpr uint32_t MMR_CHUNK_ROWS = 64;   // candidate rows per workgroup of the pairs kernel: 16 per wave
constexpr uint32_t MMR_MAX_ROUND = 32768;  // queries of one round at the most (grid.z of the pairs kernel)
constexpr int64_t MMR_SCRATCH_MIB_MAX = (int64_t)(DISTINCT_SCRATCH_BYTES >> 20);  // option mmr_scratch_mib: 1 .. this, the default

// One query of a round as the kernels read it (four 32-bit words): its m candidates are rows [row0, row0 + m) of the round's
// gathered rows (and of its candidate and relevance tables), its similarity square is m x m floats from float g0 of the round's G.
struct MmrQuery {
  uint32_t row0;
  uint32_t m;
  uint64_t g0;
};

struct MmrRound {
  uint32_t q0 = 0, nq = 0;   // its queries: [q0, q0 + nq) of the call, consecutive
  uint32_t m_max = 0;        // the largest pool among them
  uint64_t rows = 0;         // sum of m: gathered rows
  uint64_t g_floats = 0;     // sum of m^2: floats of G
};

// The refusals that need no handle.  0 = fine; else which argument is at fault (mmr_arg_message names it).
enum MmrArg { MMR_ARG_OK = 0, MMR_ARG_NQ, MMR_ARG_K, MMR_ARG_FETCH_K, MMR_ARG_LAMBDA, MMR_ARG_BUFFER };

static inline MmrArg mmr_check_args(int nq, int k, int fetch_k, float lambda, bool buffers, int max_k) {
  if (nq < 1) return MMR_ARG_NQ;
  if (k < 1 || k > max_k) return MMR_ARG_K;
  if (fetch_k < k || fetch_k > max_k) return MMR_ARG_FETCH_K;
  if (!(lambda >= 0.0f && lambda <= 1.0f)) return MMR_ARG_LAMBDA;  // (a NaN fails both comparisons)
  if (!buffers) return MMR_ARG_BUFFER;
  return MMR_ARG_OK;
}

static inline const char* mmr_arg_message(MmrArg a) {
  switch (a) {
    case MMR_ARG_NQ: return "nq below 1";
    case MMR_ARG_K: return "k outside [1, WDBX_MAX_K]";
    case MMR_ARG_FETCH_K: return "fetch_k outside [k, WDBX_MAX_K]";
    case MMR_ARG_LAMBDA: return "lambda is NaN or outside [0, 1]";
    case MMR_ARG_BUFFER: return "null buffer";
    default: return "";
  }
}

// the pool of one query: the leading slots of its top-fetch_k answer that hold a row (the ranking is dense: -1 slots trail)
static inline uint32_t mmr_pool_size(const int64_t* idx, int fetch_k) {
  uint32_t m = 0;
  while (m < (uint32_t)fetch_k && idx[m] >= 0) ++m;
  return m;
}

// bytes of round scratch one query takes: its gathered rows and its similarity square
static inline uint64_t mmr_query_bytes(uint32_t m, uint32_t pitch4) {
  return (uint64_t)m * pitch4 * 16 + (uint64_t)m * m * sizeof(float);
}

// m: [nq] pool sizes (each <= MMR_MAX_POOL; 0 = the query has no candidate and costs nothing).  Rounds of consecutive queries, as
// many as keep the sum of mmr_query_bytes within budget (MMR_MAX_ROUND at the most); a query that passes the budget alone is a round of its own.
static inline std::vector<MmrRound> mmr_plan_rounds(const uint32_t* m, int nq, uint32_t pitch4, uint64_t budget) {
  std::vector<MmrRound> rounds;
  uint64_t bytes = 0;
  MmrRound r;
  for (int q = 0; q < nq; ++q) {
    const uint64_t b = mmr_query_bytes(m[q], pitch4);
    if (r.nq && (bytes + b > budget || r.nq == MMR_MAX_ROUND)) {
      rounds.push_back(r);
      r = MmrRound();
      r.q0 = (uint32_t)q;
      bytes = 0;
    }
    ++r.nq;
    r.m_max = std::max(r.m_max, m[q]);
    r.rows += m[q];
    r.g_floats += (uint64_t)m[q] * m[q];
    bytes += b;
  }
  if (r.nq) rounds.push_back(r);
  return rounds;
}

// the table of a round's queries, in order
static inline void mmr_round_queries(const uint32_t* m, const MmrRound& r, std::vector<MmrQuery>* out) {
  out->clear();
  uint32_t row0 = 0;
  uint64_t g0 = 0;
  for (uint32_t i = 0; i < r.nq; ++i) {
    const uint32_t mi = m[r.q0 + i];
    out->push_back(MmrQuery{row0, mi, g0});
    row0 += mi;
    g0 += (uint64_t)mi * mi;
  }
}

static inline int mmr_pairs_ni(uint32_t pitch4) { return row_block_ni(pitch4); }  // (the pairs kernel's loads per lane: the shared ladder)

// grid of the pairs kernel for a round: x = chunks of MMR_CHUNK_ROWS candidate rows, y = blocks of MMR_BLOCK candidate columns
// (both of the round's largest pool: a workgroup past its query's pool returns at once), z = the round's queries
struct MmrGrid {
  uint32_t x, y, z;
};
static inline MmrGrid mmr_pairs_grid(const MmrRound& r) {
  return MmrGrid{(r.m_max + MMR_CHUNK_ROWS - 1) / MMR_CHUNK_ROWS, (r.m_max + (uint32_t)MMR_BLOCK - 1) / (uint32_t)MMR_BLOCK, r.nq};
}

// workgroups of the gather for a round: four rows per workgroup at a time, a few trips on large rounds
static inline uint32_t mmr_gather_grid(uint64_t rows) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((rows + 3) / 4, 16384)); }
