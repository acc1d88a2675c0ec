// u42_mfma_harness.hip -- a launcher of the split planes' matrix-core pass ALONE (tests/u42_mfma_harness.py,
// tests/test_gpu_u42_mfma.py): u42_query_i16_kernel over the launch's queries, then one launch of scan_u42_mfma_kernel with grid
// (grid_x, ceil(nq / 16)) on planes, thresholds and a capacity the caller hands it.  The planes come from
// tests/u42_share_harness.py (rows_to_u42_kernel).
//
// The kernels are the library's own: this file includes the headers wdbx_hip.hip includes and owns no device code.  The scan
// instance is chosen by the picker that lives next to the kernel (pick_scan42_mfma).  Built by `make -C wdbx-py_amd/csrc all`
// as tests/kernel_harness/libu42_mfma_harness.so.
//
// The entry point checks its arguments against the sizes of the arrays it uploads and returns -1 on a refusal, a HIP error
// code on a failed call, 0 otherwise.
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
#include "kernels_scan8.h"
#include "kernels_scan6.h"
#include "kernels_scan42.h"

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

}  // namespace

extern "C" {

// 1 where scan_u42_mfma_kernel has an instance for rows of `units` 32-element units
int u42m_has_instance(uint32_t units) { return u42_mfma_has_instance(units) ? 1 : 0; }

// u42_query_i16_kernel over ceil(nq / 16) * 16 queries (the last group's absent columns included), then one launch of the
// instance for `units` with grid (grid_x, ceil(nq / 16)).  hcodes: [ceil(n_rows / 64)][units][64][4] dwords (h_dwords of them);
// sa4: [n_rows][2]; lrec: [n_rows][lpitch] dwords; queries: [nq][qpitch]; tau: [nq]; cand: [cand_len] >= nq * cap keys; count,
// survivors: [nq]; surv_p: [nq][n_rows] dwords; qb: [ceil(nq / 16)][u42_mfma_group_dwords(units)] dwords (qb_dwords of them); qc:
// [ceil(nq / 16) * 16][8] dwords.
int u42m_scan(uint32_t n_rows, uint32_t units, uint32_t qpitch, uint32_t nq, uint32_t cap, uint32_t grid_x, const uint32_t* hcodes,
              uint64_t h_dwords, const float* sa4, const uint32_t* lrec, uint64_t l_dwords, const float* queries, const float* tau,
              u64* cand, uint64_t cand_len, uint32_t* count, uint32_t* survivors, uint32_t* surv_p, uint32_t* qb, uint64_t qb_dwords,
              uint32_t* qc) {
  if (!hcodes || !sa4 || !lrec || !queries || !tau || !cand || !count || !survivors || !surv_p || !qb || !qc) return -1;
  if (n_rows < 1 || n_rows > (1u << 20) || units < 1 || nq < 1 || cap < 1 || grid_x < 1 || grid_x > 65535 || nq > 1024) return -1;
  if ((uint64_t)units * 32 > qpitch || (uint64_t)nq * cap > cand_len) return -1;
  const scan42_mfma_fn fn = pick_scan42_mfma(units);
  if (!fn) return -1;
  static_assert(sizeof(U42QConst) == 32, "the tests read eight dwords per query");
  const uint32_t tiles64 = (n_rows + 63) / 64, lpitch = u42_lpitch(units);
  const uint32_t groups = (nq + U42_MFMA_QUERIES - 1) / U42_MFMA_QUERIES;
  if (h_dwords != (uint64_t)tiles64 * units * 256 || l_dwords != (uint64_t)n_rows * lpitch) return -1;
  if (qb_dwords != (uint64_t)groups * u42_mfma_group_dwords(units)) return -1;
  Bufs b;
  Scan42MfmaArgs m = {};
  Scan42Args& a = m.a;
  a.hcodes = (const uint32_t*)b.up(hcodes, (size_t)h_dwords * 4);
  a.sa4 = (const f2v*)b.up(sa4, (size_t)n_rows * sizeof(f2v));
  a.lrec = (const uint32_t*)b.up(lrec, (size_t)l_dwords * 4);
  a.query = (const float*)b.up(queries, (size_t)nq * qpitch * sizeof(float));
  a.n_rows = n_rows;
  a.units = units;
  a.qpitch = qpitch;
  a.lpitch = lpitch;
  a.tau = (const float*)b.up(tau, (size_t)nq * sizeof(float));
  a.cand = (u64*)b.up(cand, (size_t)cand_len * sizeof(u64));
  a.count = (uint32_t*)b.up(count, (size_t)nq * sizeof(uint32_t));
  a.survivors = (uint32_t*)b.up(survivors, (size_t)nq * sizeof(uint32_t));
  a.cap = cap;
  uint32_t* d_qb = (uint32_t*)b.up(qb, (size_t)qb_dwords * 4);
  U42QConst* d_qc = (U42QConst*)b.up(qc, (size_t)groups * U42_MFMA_QUERIES * sizeof(U42QConst));
  m.qb = d_qb;
  m.qc = d_qc;
  m.nq = nq;
  m.surv_p = (uint32_t*)b.up(surv_p, (size_t)nq * n_rows * 4);
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(u42_query_i16_kernel, dim3(groups * U42_MFMA_QUERIES), dim3(64), 0, nullptr, a.query, qpitch, units, nq, d_qb, d_qc);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(grid_x, groups), dim3(256), 0, nullptr, m);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(cand, a.cand, (size_t)cand_len * sizeof(u64));
  b.down(count, a.count, (size_t)nq * sizeof(uint32_t));
  b.down(survivors, a.survivors, (size_t)nq * sizeof(uint32_t));
  b.down(surv_p, m.surv_p, (size_t)nq * n_rows * 4);
  b.down(qb, d_qb, (size_t)qb_dwords * 4);
  b.down(qc, d_qc, (size_t)groups * U42_MFMA_QUERIES * sizeof(U42QConst));
  return finish(b);
}

}  // extern "C"
