// u42_convert_harness.hip -- the split six-bit planes' converts ALONE (tests/u42_convert_harness.py,
// tests/test_gpu_u42_convert.py): u42_unpack8 and u42_rem4 of kernels_scan42.h on dwords the caller hands it, one thread per
// dword, the floats written out as they come.
//
// The helpers are the library's own: this file includes the headers wdbx_hip.hip includes; its two kernels only call them
// and store what they return.  Built by `make -C wdbx-py_amd/csrc all` as tests/kernel_harness/libu42_convert_harness.so,
// with the library's flags (the same denormal mode).
//
// Every entry point returns -1 on a refusal, a HIP error code on a failed call, 0 otherwise.
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

// out[8 i + e] = element e of dword i of the h plane (e = b from the low nibble of byte b, 4 + b from its high nibble)
__global__ void u42c_nibbles_kernel(const uint32_t* in, uint32_t n, float* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f2v f[4];
  u42_unpack8(in[i], f);
  for (int k = 0; k < 4; ++k) out[8 * i + 2 * k] = f[k].x, out[8 * i + 2 * k + 1] = f[k].y;
}

// out[16 i + 4 j + b] = element 4 j + b of dword i of an l record (bits [8 b + 2 j, 8 b + 2 j + 1])
__global__ void u42c_remainders_kernel(const uint32_t* in, uint32_t n, float* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int j = 0; j < 4; ++j) {
    f2v lo, hi;
    u42_rem4(in[i], j, lo, hi);
    float* o = out + 16 * i + 4 * j;
    o[0] = lo.x, o[1] = lo.y, o[2] = hi.x, o[3] = hi.y;
  }
}

int run(void (*kernel)(const uint32_t*, uint32_t, float*), const uint32_t* in, uint32_t n, float* out, uint32_t per) {
  if (!in || !out || n < 1 || n > (1u << 20)) return -1;
  uint32_t* d_in = nullptr;
  float* d_out = nullptr;
  hipError_t e = hipMalloc((void**)&d_in, (size_t)n * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, (size_t)n * per * 4);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_out, out, (size_t)n * per * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, d_in, n, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * per * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) (void)hipGetLastError();
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return (int)e;
}

}  // namespace

extern "C" {

// in: [n] dwords; out: [n][8] floats (what the caller put there stays where the kernel writes nothing)
int u42c_nibbles(const uint32_t* in, uint32_t n, float* out) { return run(u42c_nibbles_kernel, in, n, out, 8); }
// in: [n] dwords; out: [n][16] floats
int u42c_remainders(const uint32_t* in, uint32_t n, float* out) { return run(u42c_remainders_kernel, in, n, out, 16); }

}  // extern "C"
