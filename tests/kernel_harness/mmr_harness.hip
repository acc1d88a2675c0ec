// mmr_harness.hip -- test-only launcher of the two kernels of wdbx_index_search_mmr ALONE (tests/mmr_harness.py,
// tests/test_gpu_mmr_kernels.py): mmr_pairs_kernel and mmr_select_kernel.
//
// Built from the very headers libwdbx_hip.so is built from, in wdbx_hip.hip's order: kernels_common.h, kernels_aux.h (exact_finish
// next to accum), host_subset.h (row_block_ni), host_mmr.h (the query table, the grids), kernels_rowblock.h (the pairs kernel's
// frame: exact_score_block) and kernels_mmr.h.  The pairs
// instance comes from pick_mmr_pairs, its grid from mmr_pairs_grid.  This file defines no kernel of its own.  Each entry point
// takes HOST pointers with their lengths: copy in, launch on the null stream, synchronise, copy out; it returns the HIP error
// code, or -1 when the arguments would make a kernel read or write outside the uploaded arrays (checked here, before anything
// is launched).  Output arrays are copied IN as well, so a word the kernel leaves alone comes back as the caller put it.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "wdbx_hip.h"

typedef unsigned long long u64;
typedef float f4 __attribute__((ext_vector_type(4)));

#include "kernels_common.h"
#include "kernels_aux.h"
#include "host_subset.h"
#include "host_mmr.h"
#include "kernels_rowblock.h"
#include "kernels_mmr.h"
static_assert(MMR_MAX_POOL == WDBX_MAX_K, "a pool is a top-k answer");
static_assert(sizeof(MmrQuery) == 4 * sizeof(uint32_t), "the query table is four 32-bit words per query");

namespace {

struct Bufs {
  void* p[16];
  int n = 0;
  hipError_t err = hipSuccess;
  void* up(const void* host, size_t bytes) {
    if (!host || err != hipSuccess) return nullptr;
    void* d = nullptr;
    err = hipMalloc(&d, std::max<size_t>(bytes, 16));
    if (err != hipSuccess) return nullptr;
    p[n++] = d;
    if (bytes) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    return d;
  }
  void down(void* host, const void* dev, size_t bytes) {
    if (host && dev && bytes && err == hipSuccess) err = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
  }
  ~Bufs() {
    for (int i = 0; i < n; ++i) (void)hipFree(p[i]);
  }
};

int finish(Bufs& b) {
  if (b.err != hipSuccess) (void)hipGetLastError();
  return (int)b.err;
}

// every query's rows inside [0, n_rows), its square inside [0, n_g), its pool no larger than a selection workgroup holds;
// the largest pool comes back
bool table_ok(const MmrQuery* qs, uint32_t nq, uint64_t n_rows, uint64_t n_g, uint32_t* m_max) {
  *m_max = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    if (qs[q].m > (uint32_t)MMR_MAX_POOL) return false;
    if ((uint64_t)qs[q].row0 + qs[q].m > n_rows) return false;
    if (qs[q].g0 > n_g || (uint64_t)qs[q].m * qs[q].m > n_g - qs[q].g0) return false;
    *m_max = std::max(*m_max, qs[q].m);
  }
  return true;
}

}  // namespace

extern "C" {

// mmr_pairs_kernel<metric, MMR_BLOCK, NI(pitch4)> over the table's queries.  rows: [n_rows, pitch4] quads (the gathered
// candidates), table: [nq] of four 32-bit words (row0, m, g0 low, g0 high), G: [n_g] floats.
int mmr_pairs(int metric, const float* rows, uint64_t n_rows, uint32_t pitch4, const uint32_t* table, uint32_t nq, float* G,
              uint64_t n_g) {
  if (!rows || !table || !G || n_rows < 1 || pitch4 < 1 || nq < 1 || nq > MMR_MAX_ROUND) return -1;
  const MmrQuery* qs = (const MmrQuery*)table;
  MmrRound r;
  r.nq = nq;
  if (!table_ok(qs, nq, n_rows, n_g, &r.m_max) || r.m_max < 1) return -1;
  const mmr_pairs_fn fn = pick_mmr_pairs(metric, pitch4);
  if (!fn) return -1;
  Bufs b;
  MmrPairsArgs a = {};
  a.rows = (const f4*)b.up(rows, (size_t)n_rows * pitch4 * sizeof(f4));
  a.qs = (const MmrQuery*)b.up(qs, (size_t)nq * sizeof(MmrQuery));
  a.G = (float*)b.up(G, (size_t)n_g * sizeof(float));
  a.pitch4 = pitch4;
  if (b.err != hipSuccess) return finish(b);
  const MmrGrid g = mmr_pairs_grid(r);
  hipLaunchKernelGGL(fn, dim3(g.x, g.y, g.z), dim3(256), 0, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(G, a.G, (size_t)n_g * sizeof(float));
  return finish(b);
}

// mmr_select_kernel, one workgroup per query of the table.  G: [n_g] floats, cand / rel: [n_cand], out_*: [n_out] >= nq * k
// (out_mmr may be null).
int mmr_select(const uint32_t* table, uint32_t nq, const float* G, uint64_t n_g, const u64* cand, const float* rel, uint64_t n_cand,
               int64_t* out_idx, float* out_score, float* out_mmr, uint64_t n_out, float lambda, int k, int negate) {
  if (!table || !G || !cand || !rel || !out_idx || !out_score || nq < 1 || k < 1 || k > WDBX_MAX_K) return -1;
  if ((uint64_t)nq * k > n_out) return -1;
  const MmrQuery* qs = (const MmrQuery*)table;
  uint32_t m_max;
  if (!table_ok(qs, nq, n_cand, n_g, &m_max)) return -1;
  Bufs b;
  MmrSelectArgs a = {};
  a.qs = (const MmrQuery*)b.up(qs, (size_t)nq * sizeof(MmrQuery));
  a.G = (const float*)b.up(G, (size_t)n_g * sizeof(float));
  a.cand = (const u64*)b.up(cand, (size_t)n_cand * sizeof(u64));
  a.rel = (const float*)b.up(rel, (size_t)n_cand * sizeof(float));
  a.out_idx = (int64_t*)b.up(out_idx, (size_t)n_out * sizeof(int64_t));
  a.out_score = (float*)b.up(out_score, (size_t)n_out * sizeof(float));
  a.out_mmr = (float*)b.up(out_mmr, (size_t)n_out * sizeof(float));
  a.lambda = lambda;
  a.k = k;
  a.negate = negate;
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(mmr_select_kernel, dim3(nq), dim3(256), 0, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out_idx, a.out_idx, (size_t)n_out * sizeof(int64_t));
  b.down(out_score, a.out_score, (size_t)n_out * sizeof(float));
  b.down(out_mmr, a.out_mmr, (size_t)n_out * sizeof(float));
  return finish(b);
}

}  // extern "C"
