// u42_share_harness.hip -- a launcher of the split planes' full pass with QP queries per read ALONE (tests/u42_share_harness.py,
// tests/test_gpu_u42_share.py): rows_to_u42_kernel makes the planes, then one launch of scan_u42_kernel<UC, QP> with grid
// (grid_x, nq / QP) on planes, thresholds and a capacity the caller hands it.  QP = 1 is the lone pass the shared ones are
// compared with.
//
// The kernels are the library's own: this file includes the headers wdbx_hip.hip includes and owns no device code.  The scan
// instance is chosen by the picker that lives next to the kernel (u42_unit_chunk / pick_scan42).  Built by
// `make -C wdbx-py_amd/csrc all` as tests/kernel_harness/libu42_share_harness.so.
//
// Every entry point checks its arguments against the sizes of the arrays it uploads and returns -1 on a refusal, a HIP error
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

// rows_to_u42_kernel over all n rows of rows[n][pitch], pitch a multiple of 32.
// hcodes: [ceil(n / 64)][pitch / 32][64][4] dwords; sa4: [n][2]; lrec: [n][lpitch] dwords.
int u42sh_quantise(const float* rows, uint64_t n, uint32_t dim, uint32_t pitch, uint32_t* hcodes, float* sa4, uint32_t* lrec) {
  if (!rows || !hcodes || !sa4 || !lrec || n < 1 || n > (1u << 24) || dim < 1 || dim > pitch || pitch % 32 != 0) return -1;
  const uint32_t units = pitch / 32, lpitch = u42_lpitch(units);
  const size_t tiles = (size_t)((n + 63) / 64);
  const size_t h_bytes = tiles * units * 1024, l_bytes = (size_t)n * lpitch * 4;
  Bufs b;
  const float* d_rows = (const float*)b.up(rows, (size_t)n * pitch * sizeof(float));
  uint32_t* d_h = (uint32_t*)b.up(hcodes, h_bytes);
  f2v* d_sa4 = (f2v*)b.up(sa4, (size_t)n * sizeof(f2v));
  uint32_t* d_l = (uint32_t*)b.up(lrec, l_bytes);
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(rows_to_u42_kernel, dim3(std::max<uint32_t>(1, rows_to_u42_grid(n))), dim3(256), 0, nullptr, d_rows, (u64)0, (u64)n,
                     dim, pitch, units, d_h, d_sa4, d_l, lpitch);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(hcodes, d_h, h_bytes);
  b.down(sa4, d_sa4, (size_t)n * sizeof(f2v));
  b.down(lrec, d_l, l_bytes);
  return finish(b);
}

// One launch of scan_u42_kernel<UC, qp> with grid (grid_x, nq / qp): qp = 1, 2 or 4 and divides nq.  hcodes:
// [ceil(n_rows / 64)][units][64][4] dwords (h_dwords of them); sa4: [n_rows][2]; lrec: [n_rows][lpitch] dwords; queries:
// [nq][qpitch]; tau: [nq]; cand: [cand_len] >= nq * cap keys; count, survivors: [nq].
int u42sh_scan(uint32_t n_rows, uint32_t units, uint32_t qpitch, uint32_t nq, uint32_t qp, uint32_t cap, uint32_t grid_x,
               const uint32_t* hcodes, uint64_t h_dwords, const float* sa4, const uint32_t* lrec, uint64_t l_dwords, const float* queries,
               const float* tau, u64* cand, uint64_t cand_len, uint32_t* count, uint32_t* survivors) {
  if (!hcodes || !sa4 || !lrec || !queries || !tau || !cand || !count || !survivors) return -1;
  if (n_rows < 1 || units < 1 || nq < 1 || cap < 1 || grid_x < 1 || grid_x > 65535 || nq > 65535) return -1;
  if ((qp != 1 && qp != 2 && qp != 4) || nq % qp != 0) return -1;
  if ((uint64_t)units * 32 > qpitch || (uint64_t)nq * cap > cand_len) return -1;
  const scan42_fn fn = pick_scan42(u42_unit_chunk(units), (int)qp);
  if (!fn) return -1;
  const uint32_t tiles64 = (n_rows + 63) / 64, lpitch = u42_lpitch(units);
  if (h_dwords != (uint64_t)tiles64 * units * 256 || l_dwords != (uint64_t)n_rows * lpitch) return -1;
  Bufs b;
  Scan42Args a = {};
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
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(grid_x, nq / qp), dim3(256), 0, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(cand, a.cand, (size_t)cand_len * sizeof(u64));
  b.down(count, a.count, (size_t)nq * sizeof(uint32_t));
  b.down(survivors, a.survivors, (size_t)nq * sizeof(uint32_t));
  return finish(b);
}

}  // extern "C"
