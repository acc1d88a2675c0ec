// recommend_harness.hip -- test-only launcher of recommend_kernel ALONE (tests/recommend_harness.py,
// tests/test_gpu_recommend_kernels.py): both sides, all three ranking modes.
//
// Built from the very headers libwdbx_hip.so is built from, in wdbx_hip.hip's order: kernels_common.h, kernels_aux.h
// (exact_finish next to accum), host_subset.h (row_block_ni), host_recommend.h, kernels_rowblock.h (the kernel's frame:
// exact_score_block, the mask bit) and kernels_recommend.h.  The instance
// comes from pick_recommend.  This file defines no kernel of its own.  The entry point takes HOST pointers with their lengths:
// copy in, launch on the null stream, synchronise, copy out; it returns the HIP error code, or -1 when the arguments would
// make the kernel read or write outside the uploaded arrays (checked here, before anything is launched).  The output array is
// copied IN as well, with `guard` extra words in front of and behind it on the device, so a word the kernel leaves alone --
// the guards included -- comes back as the caller put it.

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
#include "host_recommend.h"
#include "kernels_rowblock.h"
#include "kernels_recommend.h"
static_assert(RECOMMEND_MAX_EXAMPLES == WDBX_MAX_EXAMPLES && RECOMMEND_MAX_EXCLUDE == WDBX_MAX_EXCLUDE_ROWS, "the plan's limits are the header's");

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

// recommend_kernel<metric, NI(pitch4), mode> for nq queries over n_rows rows with `blocks` workgroups along the corpus.
// rows: [n_rows, pitch4] quads; examples: [n_examples, pitch4] quads; table: [nq][3]; mask: null or ceil(n_rows / 32) words
// (n_mask_words of them); exclude: [n_exclude].  out: [guard + n_out + guard] u64s; the kernel's array starts at out + guard and
// holds nq * k * blocks (modes 0, 1) or nq * n_rows (mode 2) keys.
int recommend_pass(int metric, int mode, int side, const float* rows, uint32_t n_rows, uint32_t pitch4, const float* examples,
                   uint32_t n_examples, const uint32_t* table, uint32_t nq, const uint32_t* mask, uint64_t n_mask_words,
                   const uint32_t* exclude, uint32_t n_exclude, int k, uint32_t blocks, u64* out, uint64_t n_out, uint64_t guard) {
  if (!rows || !examples || !table || !out || n_rows < 1 || pitch4 < 1 || nq < 1 || nq > 65535 || blocks < 1 || blocks > 65535) return -1;
  if (mode < 0 || mode > 2 || k < 1 || k > WDBX_MAX_K || (mode == 1 && k > 128)) return -1;
  if (mask && n_mask_words < ((uint64_t)n_rows + 31) / 32) return -1;
  if (n_exclude && !exclude) return -1;
  for (uint32_t i = 0; i < n_exclude; ++i)
    if (exclude[i] >= n_rows || (i && exclude[i] <= exclude[i - 1])) return -1;
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t* t = table + (size_t)q * 3;
    if (t[0] > t[1] || t[1] > t[2] || t[2] > n_examples) return -1;
  }
  const uint64_t need = mode == 2 ? (uint64_t)nq * n_rows : (uint64_t)nq * k * blocks;
  if (need != n_out) return -1;
  const recommend_fn fn = pick_recommend(metric, mode, pitch4);
  if (!fn) return -1;
  const size_t lds = mode == 2 ? 0 : (size_t)4 * k * sizeof(u64);
  Bufs b;
  RecommendArgs a = {};
  a.rows = (const f4*)b.up(rows, (size_t)n_rows * pitch4 * sizeof(f4));
  a.examples = (const f4*)b.up(examples, (size_t)n_examples * pitch4 * sizeof(f4));
  a.table = (const uint32_t*)b.up(table, (size_t)nq * 3 * sizeof(uint32_t));
  a.mask = (const uint32_t*)b.up(mask, (size_t)n_mask_words * sizeof(uint32_t));
  a.exclude = (const uint32_t*)b.up(exclude, (size_t)n_exclude * sizeof(uint32_t));
  u64* d_out = (u64*)b.up(out, (size_t)(n_out + 2 * guard) * sizeof(u64));
  a.out = d_out ? d_out + guard : nullptr;
  a.key_stride = n_rows;
  a.n_exclude = n_exclude;
  a.n_rows = n_rows;
  a.pitch4 = pitch4;
  a.k = k;
  a.side = side;
  if (b.err != hipSuccess) return finish(b);
  if (lds >= 64 * 1024) b.err = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(blocks, nq), dim3(256), lds, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, d_out, (size_t)(n_out + 2 * guard) * sizeof(u64));
  return finish(b);
}

}  // extern "C"
