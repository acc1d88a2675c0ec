// matrix_harness.hip -- test-only launcher of matrix_kernel ALONE (tests/matrix_harness.py, tests/test_gpu_matrix_kernels.py):
// one round of anchors of a distance matrix among listed rows, in its three modes.
//
// Built from the very headers libwdbx_hip.so is built from, in wdbx_hip.hip's order: kernels_common.h, kernels_aux.h,
// host_subset.h (row_block_ni), kernels_rowblock.h and kernels_matrix.h.  The instance comes from pick_matrix.  This file
// defines no kernel of its own.  The entry point takes HOST pointers with their lengths: copy in, launch on the null stream,
// synchronise, copy out; it returns the HIP error code, or -1 when the arguments would make the kernel read or write outside
// the uploaded arrays (checked here, before anything is launched).  The output array is copied IN as well, with `guard` extra
// words in front of and behind it on the device, so a word the kernel leaves alone comes back as the caller put it.

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
#include "kernels_rowblock.h"
#include "kernels_matrix.h"

extern "C" {

// matrix_kernel<metric, qb, NI(pitch4), mode> for the anchors at list positions [first, first + na) of ids, over all n_ids
// listed rows, with `blocks` workgroups along the list.  rows: [n_rows, pitch4] quads; ids: [n_ids] strictly increasing, below
// n_rows.  out: [guard + n_out + guard] u64s, the kernel's array holds na * k * blocks (modes 0, 1) or na * n_ids (mode 2) keys.
int matrix_pass(int metric, int mode, int qb, const float* rows, uint32_t n_rows, uint32_t pitch4, const uint32_t* ids, uint32_t n_ids,
                uint32_t first, uint32_t na, int k, uint32_t blocks, u64* out, uint64_t n_out, uint64_t guard) {
  if (!rows || !ids || !out || n_rows < 1 || pitch4 < 1 || n_ids < 1 || na < 1 || blocks < 1 || blocks > 65535) return -1;
  if (mode < 0 || mode > 2 || k < 1 || k > WDBX_MAX_K || (mode == 1 && k > 128) || qb < 1) return -1;
  if ((uint64_t)first + na > n_ids || (na + (uint32_t)qb - 1) / (uint32_t)qb > 65535) return -1;
  for (uint32_t i = 0; i < n_ids; ++i)
    if (ids[i] >= n_rows || (i && ids[i] <= ids[i - 1])) return -1;
  const uint64_t need = mode == 2 ? (uint64_t)na * n_ids : (uint64_t)na * k * blocks;
  if (need != n_out) return -1;
  const matrix_fn fn = pick_matrix(metric, mode, qb, pitch4);
  if (!fn) return -1;
  const size_t lds = mode == 2 ? 0 : (size_t)4 * qb * k * sizeof(u64);
  const size_t out_bytes = (size_t)(n_out + 2 * guard) * sizeof(u64);
  f4* d_rows = nullptr;
  uint32_t* d_ids = nullptr;
  u64* d_out = nullptr;
  hipError_t err = hipMalloc((void**)&d_rows, (size_t)n_rows * pitch4 * sizeof(f4));
  if (err == hipSuccess) err = hipMalloc((void**)&d_ids, (size_t)n_ids * sizeof(uint32_t));
  if (err == hipSuccess) err = hipMalloc((void**)&d_out, out_bytes);
  if (err == hipSuccess) err = hipMemcpy(d_rows, rows, (size_t)n_rows * pitch4 * sizeof(f4), hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(d_ids, ids, (size_t)n_ids * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(d_out, out, out_bytes, hipMemcpyHostToDevice);
  if (err == hipSuccess && lds >= 64 * 1024) err = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err == hipSuccess) {
    MatrixArgs a = {};
    a.rows = d_rows;
    a.ids = d_ids;
    a.out = d_out + guard;
    a.key_stride = n_ids;
    a.n_ids = n_ids;
    a.pitch4 = pitch4;
    a.first = first;
    a.na = na;
    a.k = k;
    hipLaunchKernelGGL(fn, dim3(blocks, (na + (uint32_t)qb - 1) / (uint32_t)qb), dim3(256), lds, nullptr, a);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost);
  if (err != hipSuccess) (void)hipGetLastError();
  (void)hipFree(d_rows);
  (void)hipFree(d_ids);
  (void)hipFree(d_out);
  return (int)err;
}

}  // extern "C"
