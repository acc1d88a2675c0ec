// rank_harness.hip -- test-only launcher of the library's ranking kernels (tests/rank_harness.py, tests/test_gpu_rank_kernels.py).
//
// Built from the very headers libwdbx_hip.so is built from: kernels_common.h and kernels_merge_select.h are included below, and
// every launch goes through the host helpers that live next to the kernels there (merge_launch_for / enqueue_merge,
// enqueue_kth, radix_select_grid / enqueue_radix_select / enqueue_sort_out), so the instance, the workgroup size and the LDS
// are the product's.  This file defines no kernel of its own.  Each entry point takes HOST pointers: copy in, launch on the
// null stream, synchronise, copy out; it returns the HIP error code, or -1 when the arguments would make a kernel read or
// write outside the uploaded arrays (checked here, before anything is launched).  Output arrays are copied IN as well, so a
// query the kernel skips comes back with whatever the caller put there.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "wdbx_hip.h"

typedef unsigned long long u64;
typedef float f4 __attribute__((ext_vector_type(4)));

#include "kernels_common.h"
#include "kernels_merge_select.h"

namespace {

// device buffers of one call: freed when the call returns, whichever way
struct Bufs {
  void* p[16];
  int n = 0;
  hipError_t err = hipSuccess;
  // a device copy of host[0 .. bytes) (null stays null)
  void* up(const void* host, size_t bytes) {
    if (!host || err != hipSuccess) return nullptr;
    void* d = nullptr;
    err = hipMalloc(&d, std::max<size_t>(bytes, 8));
    if (err != hipSuccess) return nullptr;
    p[n++] = d;
    if (bytes) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    return d;
  }
  void* zeros(size_t bytes) {
    if (err != hipSuccess) return nullptr;
    void* d = nullptr;
    err = hipMalloc(&d, std::max<size_t>(bytes, 8));
    if (err != hipSuccess) return nullptr;
    p[n++] = d;
    err = hipMemset(d, 0, std::max<size_t>(bytes, 8));
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

}  // namespace

extern "C" {

// the scalar fields of MergeArgs (the pointers are the arguments of rank_merge)
struct RankMerge {
  uint64_t q_stride, i_stride, p_stride;
  uint32_t P;
  int32_t list_len, k, metric;
  uint32_t row_base;
  int64_t idx_base;
  uint32_t over_cap;
  int32_t no_fast;
};

// what merge_launch_for chooses for k: waves per workgroup, bytes of dynamic LDS, 1 = the register-list instance
int rank_merge_geometry(int k, int lds_lists, int* waves, uint64_t* lds, int* reg) {
  if (k < 1 || k > WDBX_MAX_K) return -1;
  MergeLaunch ml;
  const hipError_t e = merge_launch_for(k, lds_lists != 0, &ml);
  if (e != hipSuccess) return (int)e;
  *waves = ml.waves;
  *lds = ml.lds;
  *reg = ml.fn == merge_kernel<true> ? 1 : 0;
  return 0;
}

// nq queries in one launch.  in[0 .. n_in); P_dev, only_if_over: [nq] or null; out_keys, out_idx, out_score: [nq, k] or null;
// out_kth, over_out: [nq] or null.
int rank_merge(const RankMerge* d, int lds_lists, int nq, const u64* in, uint64_t n_in, const uint32_t* P_dev,
               const uint32_t* only_if_over, u64* out_keys, int64_t* out_idx, float* out_score, float* out_kth, uint32_t* over_out) {
  if (!d || !in || nq < 1 || d->k < 1 || d->k > WDBX_MAX_K || d->list_len < 1) return -1;
  if (d->P && (uint64_t)(nq - 1) * d->q_stride + (uint64_t)(d->P - 1) * d->p_stride + (uint64_t)(d->list_len - 1) * d->i_stride >= n_in)
    return -1;  // (the kernel clamps P_dev to P: the last entry of the last list of the last query is the furthest read)
  Bufs b;
  const size_t nk = (size_t)nq * d->k;
  MergeArgs m = {};
  m.in = (const u64*)b.up(in, n_in * sizeof(u64));
  m.q_stride = d->q_stride;
  m.i_stride = d->i_stride;
  m.p_stride = d->p_stride;
  m.P = d->P;
  m.P_dev = (const uint32_t*)b.up(P_dev, (size_t)nq * sizeof(uint32_t));
  m.list_len = d->list_len;
  m.k = d->k;
  m.metric = d->metric;
  m.row_base = d->row_base;
  m.idx_base = d->idx_base;
  m.out_keys = (u64*)b.up(out_keys, nk * sizeof(u64));
  m.out_idx = (int64_t*)b.up(out_idx, nk * sizeof(int64_t));
  m.out_score = (float*)b.up(out_score, nk * sizeof(float));
  m.out_kth = (float*)b.up(out_kth, (size_t)nq * sizeof(float));
  m.only_if_over = (const uint32_t*)b.up(only_if_over, (size_t)nq * sizeof(uint32_t));
  m.over_cap = d->over_cap;
  m.over_out = (uint32_t*)b.up(over_out, (size_t)nq * sizeof(uint32_t));
  m.no_fast = d->no_fast;
  if (b.err != hipSuccess) return finish(b);
  MergeLaunch ml;
  if ((b.err = merge_launch_for(m.k, lds_lists != 0, &ml)) != hipSuccess) return finish(b);
  if ((b.err = enqueue_merge(nullptr, ml, m, nq)) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out_keys, m.out_keys, nk * sizeof(u64));
  b.down(out_idx, m.out_idx, nk * sizeof(int64_t));
  b.down(out_score, m.out_score, nk * sizeof(float));
  b.down(out_kth, m.out_kth, (size_t)nq * sizeof(float));
  b.down(over_out, m.over_out, (size_t)nq * sizeof(uint32_t));
  return finish(b);
}

// kth_score_kernel: query q reads keys[q * q_stride .. + n); out_kth: [nq]
int rank_kth(const u64* keys, uint64_t n_keys, uint32_t n, uint64_t q_stride, int nq, int k, float* out_kth) {
  if (!keys || !out_kth || nq < 1 || k < 1 || n < 1 || n > (uint32_t)KTH_R * 1024) return -1;
  if ((uint64_t)(nq - 1) * q_stride + n > n_keys) return -1;
  Bufs b;
  KthArgs a = {(const u64*)b.up(keys, n_keys * sizeof(u64)), q_stride, n, k, (float*)b.up(out_kth, (size_t)nq * sizeof(float))};
  if (b.err != hipSuccess) return finish(b);
  if ((b.err = enqueue_kth(nullptr, a, nq)) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out_kth, a.out_kth, (size_t)nq * sizeof(float));
  return finish(b);
}

// The radix select chain of one query: init, 8 x (hist, pick), compact, sort_out, k-th value.
//   src_mode 0: the chain reads keys[0 .. n) (src == null; alt unused).
//   src_mode 1: select_source_kernel chooses on the device, from *count against cap, between the candidates keys[0 .. *count)
//               (count <= cap; n = the buffer's size >= cap) and the dump alt[0 .. n_alt); the chain is handed alt / n_alt
//               as fixed arguments, as the library hands it the dump, and must ignore them.
//   grid 0: radix_select_grid(rows the chain may read, the device's CUs); else that many workgroups.
// out_keys, out_idx, out_score: [k]; out_kth: [1]; out_total, out_count: the state's total and out_count afterwards.
int rank_select(const u64* keys, uint64_t n, const u64* alt, uint64_t n_alt, int src_mode, uint32_t count, uint32_t cap, int k,
                int metric, uint32_t row_base, int64_t idx_base, uint32_t grid, u64* out_keys, int64_t* out_idx, float* out_score,
                float* out_kth, uint32_t* out_total, uint32_t* out_count) {
  if (k < 1 || k > WDBX_MAX_K || !out_keys || !out_idx || !out_score || !out_kth || !out_total || !out_count) return -1;
  if (src_mode == 0 ? (!keys && n) : (src_mode != 1 || !keys || !alt || cap > n || n_alt < 1)) return -1;
  Bufs b;
  int dev = 0, cus = 0;
  if ((b.err = hipGetDevice(&dev)) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return finish(b);
  const u64* d_keys = (const u64*)b.up(keys ? keys : (const u64*)&n, n * sizeof(u64));
  const u64* d_alt = src_mode ? (const u64*)b.up(alt, n_alt * sizeof(u64)) : nullptr;
  SelectState* st = (SelectState*)b.zeros(sizeof(SelectState));
  u64* sel = (u64*)b.zeros((size_t)WDBX_MAX_K * sizeof(u64));
  SelectSrc* src = nullptr;
  if (src_mode) {
    src = (SelectSrc*)b.zeros(sizeof(SelectSrc));
    const uint32_t* d_count = (const uint32_t*)b.up(&count, sizeof(count));
    if (b.err != hipSuccess) return finish(b);
    hipLaunchKernelGGL(select_source_kernel, dim3(1), dim3(64), 0, nullptr, src, d_count, cap, d_keys, d_alt, (u64)n_alt);
    b.err = hipGetLastError();
  }
  MergeArgs m = {};
  m.k = k;
  m.metric = metric;
  m.row_base = row_base;
  m.idx_base = idx_base;
  m.out_keys = (u64*)b.up(out_keys, (size_t)k * sizeof(u64));
  m.out_idx = (int64_t*)b.up(out_idx, (size_t)k * sizeof(int64_t));
  m.out_score = (float*)b.up(out_score, (size_t)k * sizeof(float));
  float* d_kth = (float*)b.up(out_kth, sizeof(float));
  if (b.err != hipSuccess) return finish(b);
  const uint64_t rows = src_mode ? std::max<uint64_t>(n_alt, cap) : n;
  if (!grid) grid = std::max<uint32_t>(1, radix_select_grid(rows, cus));
  const u64* fixed = src_mode ? d_alt : d_keys;
  const u64 fixed_n = src_mode ? n_alt : n;
  if ((b.err = enqueue_radix_select(nullptr, fixed, fixed_n, src, st, sel, (uint32_t)k, grid)) != hipSuccess) return finish(b);
  if ((b.err = enqueue_sort_out(nullptr, sel, st, m)) != hipSuccess) return finish(b);
  hipLaunchKernelGGL(select_kth_value_kernel, dim3(1), dim3(64), 0, nullptr, (const SelectState*)st, (uint32_t)k, d_kth);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out_keys, m.out_keys, (size_t)k * sizeof(u64));
  b.down(out_idx, m.out_idx, (size_t)k * sizeof(int64_t));
  b.down(out_score, m.out_score, (size_t)k * sizeof(float));
  b.down(out_kth, d_kth, sizeof(float));
  SelectState h;
  b.down(&h, st, sizeof(SelectState));
  if (b.err == hipSuccess) {
    *out_total = h.total;
    *out_count = h.out_count;
  }
  return finish(b);
}

}  // extern "C"
