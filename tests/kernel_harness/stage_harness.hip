// stage_harness.hip -- test-only launcher of the int8 batch stages AROUND the tile kernel, each alone (tests/stage_harness.py,
// tests/test_gpu_stage_kernels.py): scatter_pairs_kernel, refine_pairs_kernel and mark_lost_kernel (the pair scatter, the
// second selection stage and the overflow marks of the batched calls), place_queries_kernel and pad_tau_kernel (the slots of
// a call with one mask per query), range_batch_bound_kernel (kernels_range_batch.h), gather_rows_kernel and
// normalize_rows_kernel (kernels_aux.h).
//
// Built from the very headers libwdbx_hip.so is built from; this file defines no kernel of its own.  The refine launch goes
// through refine_launch_for / enqueue_refine (kernels_tiles8.h, host_refine.h): what host_index.h launches.  The other
// grids are the expressions the library's launch sites hold.  Built by `make -C wdbx-py_amd/csrc all` as
// tests/kernel_harness/libstage_harness.so.
//
// Each entry point takes HOST pointers, each with its length: copy in, launch on the null stream, synchronise, copy out.
// Output arrays are copied IN as well, so a slot the kernel leaves alone comes back with whatever the caller put there.
// It returns the HIP error code, or -1 -- before anything is launched -- when the arguments would let a kernel read or write
// outside the uploaded arrays.  The checks follow the kernels' real extents.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "wdbx_hip.h"

typedef unsigned long long u64;
typedef float f4 __attribute__((ext_vector_type(4)));

#include "kernels_common.h"
#include "kernels_merge_select.h"
#include "kernels_tiles8.h"
#include "kernels_aux.h"
#include "kernels_range_batch.h"

namespace {

// device buffers of one call: freed when the call returns, whichever way
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

int sync_and_check(Bufs& b) {
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  b.err = hipDeviceSynchronize();
  return finish(b);
}

}  // namespace

extern "C" {

uint32_t stage_scatter_lists() { return (uint32_t)SCATTER_LISTS; }
uint32_t stage_refine_r() { return (uint32_t)REFINE_R; }
uint32_t stage_kth_low_bit() { return (uint32_t)KTH_LOW_BIT; }
float stage_range_batch_gamma() { return RANGE_BATCH_GAMMA; }

// scatter_pairs_kernel, grid (nlists + SCATTER_LISTS - 1) / SCATTER_LISTS as the library launches it.  pairs: [pairs_len] >=
// nlists * pair_cap; pair_count: [nlists]; cand: [cand_len]; count: [count_len]; lost: [lost_len >= 1] (word 0 is the flag).
// A pair's query byte q takes part when it lies in the first min(pair_count[w], pair_cap) pairs of its list: then
// q < count_len and (q + 1) * cap <= cand_len.
int stage_scatter(const u64* pairs, uint64_t pairs_len, const uint32_t* pair_count, uint32_t nlists, uint32_t pair_cap, u64* cand,
                  uint64_t cand_len, uint32_t* count, uint64_t count_len, uint32_t cap, uint32_t* lost, uint64_t lost_len) {
  if (!pairs || !pair_count || !cand || !count || !lost || lost_len < 1) return -1;
  if (nlists < 1 || nlists > (1u << 16) || pair_cap < 1 || pair_cap > (1u << 16) || cap < 1) return -1;
  if (pairs_len < (uint64_t)nlists * pair_cap) return -1;
  for (uint32_t w = 0; w < nlists; ++w) {
    const uint32_t have = std::min(pair_count[w], pair_cap);
    for (uint32_t i = 0; i < have; ++i) {
      const uint64_t q = (pairs[(size_t)w * pair_cap + i] >> 32) & 255u;
      if (q >= count_len || (q + 1) * cap > cand_len) return -1;
    }
  }
  Bufs b;
  const u64* d_pairs = (const u64*)b.up(pairs, (size_t)pairs_len * sizeof(u64));
  const uint32_t* d_pc = (const uint32_t*)b.up(pair_count, (size_t)nlists * sizeof(uint32_t));
  u64* d_cand = (u64*)b.up(cand, (size_t)cand_len * sizeof(u64));
  uint32_t* d_count = (uint32_t*)b.up(count, (size_t)count_len * sizeof(uint32_t));
  uint32_t* d_lost = (uint32_t*)b.up(lost, (size_t)lost_len * sizeof(uint32_t));
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(scatter_pairs_kernel, dim3((nlists + SCATTER_LISTS - 1) / SCATTER_LISTS), dim3(1024), 0, nullptr, d_pairs, d_pc, nlists,
                     pair_cap, d_cand, d_count, cap, d_lost);
  if (sync_and_check(b)) return (int)b.err;
  b.down(cand, d_cand, (size_t)cand_len * sizeof(u64));
  b.down(count, d_count, (size_t)count_len * sizeof(uint32_t));
  b.down(lost, d_lost, (size_t)lost_len * sizeof(uint32_t));
  return finish(b);
}

// the launch shape refine_shape gives: out = {reg, waves, n_lds, lds bytes, raise}
int stage_refine_shape(int k, uint32_t cap, int lds_lists, uint64_t* out) {
  if (k < 1 || k > WDBX_MAX_K || !out) return -1;
  const RefineShape s = refine_shape(k, cap, lds_lists != 0);
  out[0] = s.reg;
  out[1] = (uint64_t)s.waves;
  out[2] = s.n_lds;
  out[3] = s.lds;
  out[4] = s.raise;
  return 0;
}

// refine_pairs_kernel through refine_launch_for / enqueue_refine, one workgroup per query.  n_lds_override: 0 = the shape's
// n_lds; else a smaller one (a list longer than it takes the wave-list branch -- the LDS bytes stay the shape's, which hold
// the waves' lists whatever n_lds is).  cand: [cand_len] >= nq * cap; count: [nq]; groups: [n_groups][4]; gbad: [gbad_len];
// cn: [cn_len] (L2) or null; qpar: [qpar_len >= nq][4].  A query the kernel works on (k < count[q] <= cap) has every entry's
// row inside the tables: row >> 6 < n_groups and < gbad_len, row < cn_len for L2.  (Lanes past the end of a list fetch row 0.)
int stage_refine(int metric, int k, int lds_lists, uint32_t n_lds_override, u64* cand, uint64_t cand_len, uint32_t* count, uint32_t nq,
                 uint32_t cap, const float* groups, uint64_t n_groups, const u64* gbad, uint64_t gbad_len, const float* cn, uint64_t cn_len,
                 const float* qpar, uint64_t qpar_len) {
  if (!cand || !count || !groups || !gbad || !qpar) return -1;
  if (metric != WDBX_METRIC_COSINE && metric != WDBX_METRIC_L2) return -1;
  const bool l2 = metric == WDBX_METRIC_L2;
  if (l2 && !cn) return -1;
  if (k < 1 || k > WDBX_MAX_K || nq < 1 || nq > 65536 || cap < 1) return -1;
  if (cand_len < (uint64_t)nq * cap || qpar_len < nq) return -1;
  if (n_groups < 1 || gbad_len < 1 || (l2 && cn_len < 1)) return -1;
  const RefineShape shape = refine_shape(k, cap, lds_lists != 0);
  if (n_lds_override > shape.n_lds) return -1;
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t n = count[q];
    if (n > cap || n <= (uint32_t)k) continue;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t row = ~(uint32_t)cand[(size_t)q * cap + i];
      const uint64_t g = row >> 6;
      if (g >= n_groups || g >= gbad_len || (l2 && row >= cn_len)) return -1;
    }
  }
  Bufs b;
  RefineArgs r = {};
  r.cand = (u64*)b.up(cand, (size_t)cand_len * sizeof(u64));
  r.count = (uint32_t*)b.up(count, (size_t)nq * sizeof(uint32_t));
  r.cap = cap;
  r.groups = (const f4*)b.up(groups, (size_t)n_groups * sizeof(f4));
  r.gbad = (const u64*)b.up(gbad, (size_t)gbad_len * sizeof(u64));
  r.cn = (const float*)b.up(cn, (size_t)cn_len * sizeof(float));
  r.qpar = (const f4*)b.up(qpar, (size_t)qpar_len * sizeof(f4));
  r.k = k;
  if (b.err != hipSuccess) return finish(b);
  RefineLaunch rl;
  if ((b.err = refine_launch_for(metric, k, cap, lds_lists != 0, &rl)) != hipSuccess) return finish(b);
  r.n_lds = n_lds_override ? n_lds_override : rl.shape.n_lds;
  if ((b.err = enqueue_refine(nullptr, rl, r, (int)nq)) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(cand, r.cand, (size_t)cand_len * sizeof(u64));
  b.down(count, r.count, (size_t)nq * sizeof(uint32_t));
  return finish(b);
}

// mark_lost_kernel, one workgroup of `threads` (0: the library's 256).  count: [count_len >= nq]; lost: one word or null;
// over_list: [over_len >= nq + 1] or null.
int stage_mark_lost(uint32_t* count, uint64_t count_len, uint32_t nq, const uint32_t* lost, uint32_t cap, uint32_t* over_list,
                    uint64_t over_len, uint32_t threads) {
  if (!count || nq > count_len) return -1;
  if (over_list && over_len < (uint64_t)nq + 1) return -1;
  if (!threads) threads = 256;
  if (threads % 64 != 0 || threads > 1024) return -1;
  Bufs b;
  uint32_t* d_count = (uint32_t*)b.up(count, (size_t)count_len * sizeof(uint32_t));
  const uint32_t* d_lost = (const uint32_t*)b.up(lost, sizeof(uint32_t));
  uint32_t* d_over = (uint32_t*)b.up(over_list, (size_t)over_len * sizeof(uint32_t));
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(mark_lost_kernel, dim3(1), dim3(threads), 0, nullptr, d_count, nq, d_lost, cap, d_over);
  if (sync_and_check(b)) return (int)b.err;
  b.down(count, d_count, (size_t)count_len * sizeof(uint32_t));
  b.down(over_list, d_over, (size_t)over_len * sizeof(uint32_t));
  return finish(b);
}

// place_queries_kernel, grid (slots * pitch4 + 255) / 256.  q: [q_rows][pitch4 * 4]; slot_query: [slots], each < q_rows
// (negative: a pad); out: [out_len] float4s >= slots * pitch4.
int stage_place_queries(const float* q, uint64_t q_rows, const int32_t* slot_query, uint32_t pitch4, uint32_t slots, float* out,
                        uint64_t out_len) {
  if (!q || !slot_query || !out || pitch4 < 1 || slots < 1 || q_rows < 1) return -1;
  if ((uint64_t)slots * pitch4 >= (1ull << 31) || out_len < (uint64_t)slots * pitch4) return -1;
  for (uint32_t s = 0; s < slots; ++s)
    if (slot_query[s] >= 0 && (uint64_t)slot_query[s] >= q_rows) return -1;
  Bufs b;
  const f4* d_q = (const f4*)b.up(q, (size_t)q_rows * pitch4 * sizeof(f4));
  const int32_t* d_sq = (const int32_t*)b.up(slot_query, (size_t)slots * sizeof(int32_t));
  f4* d_out = (f4*)b.up(out, (size_t)out_len * sizeof(f4));
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(place_queries_kernel, dim3((slots * pitch4 + 255) / 256), dim3(256), 0, nullptr, d_q, d_sq, pitch4, slots, d_out);
  if (sync_and_check(b)) return (int)b.err;
  b.down(out, d_out, (size_t)out_len * sizeof(f4));
  return finish(b);
}

// pad_tau_kernel, grid (slots + 255) / 256.  tau: [tau_len >= slots]; slot_query: [slots].
int stage_pad_tau(float* tau, uint64_t tau_len, const int32_t* slot_query, uint32_t slots) {
  if (!tau || !slot_query || slots < 1 || tau_len < slots) return -1;
  Bufs b;
  float* d_tau = (float*)b.up(tau, (size_t)tau_len * sizeof(float));
  const int32_t* d_sq = (const int32_t*)b.up(slot_query, (size_t)slots * sizeof(int32_t));
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(pad_tau_kernel, dim3((slots + 255) / 256), dim3(256), 0, nullptr, d_tau, d_sq, slots);
  if (sync_and_check(b)) return (int)b.err;
  b.down(tau, d_tau, (size_t)tau_len * sizeof(float));
  return finish(b);
}

// range_batch_bound_kernel, grid range_batch_bound_grid(gbn).  qpar: [qpar_len >= gbn][4]; tau_in: [tau_in_len >= nv];
// tau: [tau_len >= gbn]; result_count: [rc_len >= gbn].
int stage_range_batch_bound(uint32_t nv, uint32_t gbn, float* qpar, uint64_t qpar_len, const float* tau_in, uint64_t tau_in_len, float* tau,
                            uint64_t tau_len, uint32_t* result_count, uint64_t rc_len) {
  if (!qpar || !tau_in || !tau || !result_count || gbn < 1 || gbn > 65536 || nv > gbn) return -1;
  if (qpar_len < gbn || tau_in_len < nv || tau_len < gbn || rc_len < gbn) return -1;
  Bufs b;
  f4* d_qpar = (f4*)b.up(qpar, (size_t)qpar_len * sizeof(f4));
  const float* d_in = (const float*)b.up(tau_in, (size_t)tau_in_len * sizeof(float));
  float* d_tau = (float*)b.up(tau, (size_t)tau_len * sizeof(float));
  uint32_t* d_rc = (uint32_t*)b.up(result_count, (size_t)rc_len * sizeof(uint32_t));
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(range_batch_bound_kernel, dim3(range_batch_bound_grid(gbn)), dim3(256), 0, nullptr, nv, gbn, d_qpar, d_in, d_tau, d_rc);
  if (sync_and_check(b)) return (int)b.err;
  b.down(qpar, d_qpar, (size_t)qpar_len * sizeof(f4));
  b.down(tau, d_tau, (size_t)tau_len * sizeof(float));
  b.down(result_count, d_rc, (size_t)rc_len * sizeof(uint32_t));
  return finish(b);
}

// gather_rows_kernel, grid `grid` or the library's min((n + 3) / 4, 65536).  rows: [n_rows][pitch4 * 4]; src: [n], each
// < n_rows; dst: [dst_rows >= n][pitch4 * 4].
int stage_gather_rows(const float* rows, uint64_t n_rows, uint32_t pitch4, const u64* src, uint64_t n, float* dst, uint64_t dst_rows,
                      uint32_t grid) {
  if (!rows || !src || !dst || pitch4 < 1 || n < 1 || n_rows < 1 || dst_rows < n || grid > 65536) return -1;
  for (uint64_t i = 0; i < n; ++i)
    if (src[i] >= n_rows) return -1;
  Bufs b;
  const f4* d_rows = (const f4*)b.up(rows, (size_t)n_rows * pitch4 * sizeof(f4));
  const u64* d_src = (const u64*)b.up(src, (size_t)n * sizeof(u64));
  f4* d_dst = (f4*)b.up(dst, (size_t)dst_rows * pitch4 * sizeof(f4));
  if (b.err != hipSuccess) return finish(b);
  if (!grid) grid = (uint32_t)std::min<uint64_t>((n + 3) / 4, 65536);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(256), 0, nullptr, d_rows, pitch4, d_src, (u64)n, d_dst);
  if (sync_and_check(b)) return (int)b.err;
  b.down(dst, d_dst, (size_t)dst_rows * pitch4 * sizeof(f4));
  return finish(b);
}

// normalize_rows_kernel, grid `grid` or the library's min((n + 3) / 4, 65536).  rows: [have_rows >= n][pitch].
int stage_normalize_rows(float* rows, uint64_t have_rows, uint64_t n, uint32_t pitch, uint32_t grid) {
  if (!rows || pitch < 1 || n < 1 || have_rows < n || grid > 65536) return -1;
  Bufs b;
  float* d_rows = (float*)b.up(rows, (size_t)have_rows * pitch * sizeof(float));
  if (b.err != hipSuccess) return finish(b);
  if (!grid) grid = (uint32_t)std::min<uint64_t>((n + 3) / 4, 65536);
  hipLaunchKernelGGL(normalize_rows_kernel, dim3(grid), dim3(256), 0, nullptr, d_rows, (u64)n, pitch);
  if (sync_and_check(b)) return (int)b.err;
  b.down(rows, d_rows, (size_t)have_rows * pitch * sizeof(float));
  return finish(b);
}

}  // extern "C"
