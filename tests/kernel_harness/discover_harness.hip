// discover_harness.hip -- test-only launcher of discover_kernel and discover_zone_kernel ALONE (tests/discover_harness.py,
// tests/test_gpu_discover_kernels.py): the scoring pass in its four modes and the zone stage in its three.
//
// Built from the very headers libwdbx_hip.so is built from, in wdbx_hip.hip's order: kernels_common.h, kernels_aux.h,
// host_subset.h (row_block_ni), host_discover.h (with host_recommend.h), kernels_rowblock.h, kernels_recommend.h (the
// exclusion-list search) and kernels_discover.h.  The instances come from pick_discover / pick_discover_zone.  This file
// defines no kernel of its own.  The entry points take HOST pointers with their lengths: copy in, launch on the null stream,
// synchronise, copy out; they return the HIP error code, or -1 when the arguments would make a kernel read or write outside
// the uploaded arrays (checked here, before anything is launched).  Every output array is copied IN as well, the key array
// with `guard` extra words in front of and behind it on the device, so a word the kernel leaves alone comes back as the caller
// put it.  The caller stages the vectors itself: a table entry may start anywhere in them.

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
#include "host_discover.h"
#include "kernels_rowblock.h"
#include "kernels_recommend.h"
#include "kernels_discover.h"
static_assert(DISCOVER_MAX_PAIRS == WDBX_MAX_CONTEXT_PAIRS && DISCOVER_ZONES == DISCOVER_ZONE_COUNT, "the plan's limits are the header's and the kernel's");

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

// discover_kernel<metric, NI(pitch4), mode> for nq queries over n_rows rows with `blocks` workgroups along the corpus.
// rows: [n_rows, pitch4] quads; vectors: [n_vectors, pitch4] quads; table: [nq][2] {first staged vector, pairs} (mode 3: the
// first staged vector is the target); mask: null or ceil(n_rows / 32) words; exclude: [n_exclude].  out: [guard + n_out +
// guard] u64s, the kernel's array holds nq * k * blocks (modes 0, 1) or nq * n_rows (modes 2, 3) keys.  Mode 3 only: wins
// [guard + nq * n_rows + guard] bytes and counts [nq * 33] words, which the kernel adds to.
int discover_pass(int metric, int mode, const float* rows, uint32_t n_rows, uint32_t pitch4, const float* vectors, uint32_t n_vectors,
                  const uint32_t* table, uint32_t nq, const uint32_t* mask, uint64_t n_mask_words, const uint32_t* exclude,
                  uint32_t n_exclude, int k, uint32_t blocks, u64* out, uint64_t n_out, uint8_t* wins, uint32_t* counts, uint64_t guard) {
  if (!rows || !vectors || !table || !out || n_rows < 1 || pitch4 < 1 || nq < 1 || nq > 65535 || blocks < 1 || blocks > 65535) return -1;
  if (mode < 0 || mode > 3 || k < 1 || k > WDBX_MAX_K || (mode == 1 && k > 128)) return -1;
  if (mode == 3 && (!wins || !counts)) return -1;
  if (mask && n_mask_words < ((uint64_t)n_rows + 31) / 32) return -1;
  if (n_exclude && !exclude) return -1;
  for (uint32_t i = 0; i < n_exclude; ++i)
    if (exclude[i] >= n_rows || (i && exclude[i] <= exclude[i - 1])) return -1;
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t* t = table + (size_t)q * 2;
    if (t[1] > (uint32_t)DISCOVER_MAX_PAIRS || (uint64_t)t[0] + 2 * t[1] + (mode == 3 ? 1 : 0) > n_vectors) return -1;
  }
  const bool per_row = mode >= 2;
  const uint64_t need = per_row ? (uint64_t)nq * n_rows : (uint64_t)nq * k * blocks;
  if (need != n_out) return -1;
  const discover_fn fn = pick_discover(metric, mode, pitch4);
  if (!fn) return -1;
  const size_t lds = per_row ? 0 : (size_t)4 * k * sizeof(u64);
  Bufs b;
  DiscoverArgs a = {};
  a.rows = (const f4*)b.up(rows, (size_t)n_rows * pitch4 * sizeof(f4));
  a.vectors = (const f4*)b.up(vectors, (size_t)n_vectors * pitch4 * sizeof(f4));
  a.table = (const uint32_t*)b.up(table, (size_t)nq * 2 * sizeof(uint32_t));
  a.mask = (const uint32_t*)b.up(mask, (size_t)n_mask_words * sizeof(uint32_t));
  a.exclude = (const uint32_t*)b.up(exclude, (size_t)n_exclude * sizeof(uint32_t));
  u64* d_out = (u64*)b.up(out, (size_t)(n_out + 2 * guard) * sizeof(u64));
  uint8_t* d_wins = mode == 3 ? (uint8_t*)b.up(wins, (size_t)(n_out + 2 * guard)) : nullptr;
  uint32_t* d_counts = mode == 3 ? (uint32_t*)b.up(counts, (size_t)nq * DISCOVER_ZONES * sizeof(uint32_t)) : nullptr;
  a.out = d_out ? d_out + guard : nullptr;
  a.wins = d_wins ? d_wins + guard : nullptr;
  a.counts = d_counts;
  a.key_stride = n_rows;
  a.n_exclude = n_exclude;
  a.n_rows = n_rows;
  a.pitch4 = pitch4;
  a.k = k;
  if (b.err != hipSuccess) return finish(b);
  if (lds >= 64 * 1024) b.err = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(blocks, nq), dim3(256), lds, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, d_out, (size_t)(n_out + 2 * guard) * sizeof(u64));
  if (mode == 3) {
    b.down(wins, d_wins, (size_t)(n_out + 2 * guard));
    b.down(counts, d_counts, (size_t)nq * DISCOVER_ZONES * sizeof(uint32_t));
  }
  return finish(b);
}

// discover_zone_kernel<mode> for n_entries (query slot, zone) entries over records of n_slots query slots with n_rows rows each.
// out: [guard + n_out + guard] u64s, n_out = n_entries * k * blocks (modes 0, 1) or n_entries * n_rows (mode 2).
int discover_zone_pass(int mode, const u64* rec_key, const uint8_t* rec_wins, uint32_t n_slots, uint32_t n_rows, const uint32_t* table,
                       uint32_t n_entries, int k, uint32_t blocks, u64* out, uint64_t n_out, uint64_t guard) {
  if (!rec_key || !rec_wins || !table || !out || n_slots < 1 || n_rows < 1 || n_entries < 1 || n_entries > 65535 || blocks < 1 ||
      blocks > 65535)
    return -1;
  if (mode < 0 || mode > 2 || k < 1 || k > WDBX_MAX_K || (mode == 1 && k > 128)) return -1;
  for (uint32_t e = 0; e < n_entries; ++e)
    if (table[2 * e] >= n_slots) return -1;
  const uint64_t need = mode == 2 ? (uint64_t)n_entries * n_rows : (uint64_t)n_entries * k * blocks;
  if (need != n_out) return -1;
  const discover_zone_fn fn = pick_discover_zone(mode);
  if (!fn) return -1;
  const size_t lds = mode == 2 ? 0 : (size_t)4 * k * sizeof(u64);
  Bufs b;
  DiscoverZoneArgs a = {};
  a.rec_key = (const u64*)b.up(rec_key, (size_t)n_slots * n_rows * sizeof(u64));
  a.rec_wins = (const uint8_t*)b.up(rec_wins, (size_t)n_slots * n_rows);
  a.table = (const uint32_t*)b.up(table, (size_t)n_entries * 2 * sizeof(uint32_t));
  u64* d_out = (u64*)b.up(out, (size_t)(n_out + 2 * guard) * sizeof(u64));
  a.out = d_out ? d_out + guard : nullptr;
  a.rec_stride = n_rows;
  a.n_rows = n_rows;
  a.k = k;
  if (b.err != hipSuccess) return finish(b);
  if (lds >= 64 * 1024) b.err = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(blocks, n_entries), dim3(256), lds, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, d_out, (size_t)(n_out + 2 * guard) * sizeof(u64));
  return finish(b);
}

}  // extern "C"
