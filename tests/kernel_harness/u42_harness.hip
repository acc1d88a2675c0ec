// u42_harness.hip -- a launcher of the split six-bit planes' kernels ALONE (tests/u42_harness.py,
// tests/test_gpu_u42_kernels.py): rows_to_u42_kernel next to rows_to_u6_kernel (the same rows, so that a6 can be compared
// with the u6 shadow's a bit for bit) and one launch of scan_u42_kernel on planes, thresholds and a grid the caller hands it.
//
// The kernels are the library's own: this file includes the headers wdbx_hip.hip includes and owns no device code.  The scan
// instance is chosen by the picker that lives next to the kernel (u42_unit_chunk / pick_scan42), the record pitch by
// u42_lpitch.  Built by `make -C wdbx-py_amd/csrc all` as tests/kernel_harness/libu42_harness.so.
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

int u42h_unit_chunk(uint32_t units) { return u42_unit_chunk(units); }
uint32_t u42h_lpitch(uint32_t units) { return u42_lpitch(units); }

// rows_to_u42_kernel and rows_to_u6_kernel over rows [r0, n) of rows[n_alloc][pitch], pitch a multiple of 32.
// hcodes: [ceil(n_alloc / 64)][pitch / 32][64][4] dwords; sa4: [n_alloc][2]; lrec: [n_alloc][lpitch] dwords;
// codes6: [ceil(n_alloc / 64)][pitch / 16][64][3] dwords; sa6: [n_alloc][2].  grid 0: rows_to_u42_grid(n - r0).
int u42h_quantise(const float* rows, uint64_t n_alloc, uint64_t r0, uint64_t n, uint32_t dim, uint32_t pitch, uint32_t grid,
                  uint32_t* hcodes, float* sa4, uint32_t* lrec, uint32_t* codes6, float* sa6) {
  if (!rows || !hcodes || !sa4 || !lrec || !codes6 || !sa6 || n > n_alloc || r0 > n || dim < 1 || dim > pitch || pitch % 32 != 0)
    return -1;
  const uint32_t units = pitch / 32, lpitch = u42_lpitch(units);
  const size_t tiles = (size_t)((n_alloc + 63) / 64);
  const size_t h_bytes = tiles * units * 1024, l_bytes = (size_t)n_alloc * lpitch * 4, c6_bytes = tiles * units * 2 * 768;
  Bufs b;
  const float* d_rows = (const float*)b.up(rows, (size_t)n_alloc * pitch * sizeof(float));
  uint32_t* d_h = (uint32_t*)b.up(hcodes, h_bytes);
  f2v* d_sa4 = (f2v*)b.up(sa4, (size_t)n_alloc * sizeof(f2v));
  uint32_t* d_l = (uint32_t*)b.up(lrec, l_bytes);
  uint32_t* d_c6 = (uint32_t*)b.up(codes6, c6_bytes);
  f2v* d_sa6 = (f2v*)b.up(sa6, (size_t)n_alloc * sizeof(f2v));
  if (b.err != hipSuccess) return finish(b);
  if (!grid) grid = std::max<uint32_t>(1, rows_to_u42_grid(n - r0));
  hipLaunchKernelGGL(rows_to_u42_kernel, dim3(grid), dim3(256), 0, nullptr, d_rows, (u64)r0, (u64)n, dim, pitch, units, d_h, d_sa4, d_l,
                     lpitch);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  hipLaunchKernelGGL(rows_to_u6_kernel, dim3(grid), dim3(256), 0, nullptr, d_rows, (u64)r0, (u64)n, dim, pitch, units * 2, d_c6, d_sa6);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(hcodes, d_h, h_bytes);
  b.down(sa4, d_sa4, (size_t)n_alloc * sizeof(f2v));
  b.down(lrec, d_l, l_bytes);
  b.down(codes6, d_c6, c6_bytes);
  b.down(sa6, d_sa6, (size_t)n_alloc * sizeof(f2v));
  return finish(b);
}

// One launch of scan_u42_kernel with grid (grid_x, nq).  hcodes: [ceil(n_rows / 64)][units][64][4] dwords (h_dwords of them);
// sa4: [n_rows][2]; lrec: [n_rows][lpitch] dwords; queries: [nq][qpitch]; tau: [nq]; cand: [cand_len] >= nq * cap keys;
// count, survivors: [nq].
int u42h_scan(uint32_t n_rows, uint32_t units, uint32_t qpitch, uint32_t nq, uint32_t cap, uint32_t grid_x, const uint32_t* hcodes,
              uint64_t h_dwords, const float* sa4, const uint32_t* lrec, uint64_t l_dwords, const float* queries, const float* tau,
              u64* cand, uint64_t cand_len, uint32_t* count, uint32_t* survivors) {
  if (!hcodes || !sa4 || !lrec || !queries || !tau || !cand || !count || !survivors) return -1;
  if (n_rows < 1 || units < 1 || nq < 1 || cap < 1 || grid_x < 1 || grid_x > 65535 || nq > 65535) return -1;
  if ((uint64_t)units * 32 > qpitch || (uint64_t)nq * cap > cand_len) return -1;
  const scan42_fn fn = pick_scan42(u42_unit_chunk(units));
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
  hipLaunchKernelGGL(fn, dim3(grid_x, nq), dim3(256), 0, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(cand, a.cand, (size_t)cand_len * sizeof(u64));
  b.down(count, a.count, (size_t)nq * sizeof(uint32_t));
  b.down(survivors, a.survivors, (size_t)nq * sizeof(uint32_t));
  return finish(b);
}

}  // extern "C"
