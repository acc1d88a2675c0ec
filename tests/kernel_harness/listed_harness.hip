// listed_harness.hip -- test-only launcher of the listed-row, label and multi-vector kernels ALONE (tests/listed_harness.py,
// tests/test_gpu_listed_kernels.py): subset_kernel, rowlists_kernel, label_keys_kernel, label_rank_kernel and
// multivector_rank_kernel.
//
// Built from the very headers libwdbx_hip.so is built from, in wdbx_hip.hip's order: kernels_common.h, kernels_aux.h (for
// exact_finish next to accum; its own kernels need nothing else), the device-free host headers of the four calls (the structs
// the kernels read and the sizes of their dynamic LDS: subset_lists_lds, label_rank_lds, multivector_rank_lds), kernels_rowblock.h
// (the frame of the first three kernels; its loads per lane come from host_subset.h's row_block_ni) and the four kernel headers.  The instance of every launch comes from the pickers that live next to the kernels (pick_subset,
// pick_rowlists, pick_label_keys, pick_label_rank, pick_multivector_rank); a null picker result returns -1.  This file defines
// no kernel of its own.  Each entry point takes HOST pointers with their lengths, an explicit grid.x and the scalar fields of
// the kernel's argument struct: copy in, launch on the null stream, synchronise, copy out; it returns the HIP error code, or
// -1 when the arguments would make the kernel read or write outside the uploaded arrays (checked here, before anything is
// launched).  Output arrays are copied IN as well, so a word the kernel leaves alone comes back with whatever the caller put
// there.

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
#include "host_rowlists.h"
#include "host_labels.h"
#include "host_multivector.h"
#include "kernels_rowblock.h"
#include "kernels_subset.h"
#include "kernels_rowlists.h"
#include "kernels_labels.h"
static_assert(LABEL_SPAN_DEV == LABEL_SPAN, "the kernels walk the spans the host built");
#include "kernels_multivector.h"

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

// the host's rule for every instance with lists in dynamic LDS
hipError_t allow_lds(const void* fn, size_t lds) {
  if (lds < 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

bool ids_below(const uint32_t* ids, uint64_t n, uint64_t n_rows) {
  for (uint64_t i = 0; i < n; ++i)
    if (ids[i] >= n_rows) return false;
  return true;
}

// mode 0 / 1: lists of k keys, register lists up to 128; mode 2: no k
bool list_k_ok(int mode, int k) {
  if (mode == 2) return true;
  return k >= 1 && k <= WDBX_MAX_K && (mode != 1 || k <= 128);
}

// label_item0[0 .. n_labels] is a non-decreasing table that starts at 0; returns false when it is not
bool item_table_ok(const uint32_t* t, uint64_t entries) {
  if (!t || entries < 2 || t[0] != 0) return false;
  for (uint64_t i = 1; i < entries; ++i)
    if (t[i] < t[i - 1]) return false;
  return true;
}

}  // namespace

extern "C" {

// subset_kernel<metric, qb, NI(pitch4), mode>, grid (grid_x, ceil(nq / qb)).  rows: [n_rows, pitch4] quads, queries: [nq,
// pitch4] quads, ids: [n_ids], out: [n_out] (lists: nq * k * grid_x words are the kernel's; keys: (nq - 1) * key_stride + n_ids).
int listed_subset(int metric, int mode, int qb, const float* rows, uint64_t n_rows, uint32_t pitch4, const float* queries,
                  uint32_t nq, const uint32_t* ids, uint32_t n_ids, u64* out, uint64_t n_out, uint64_t key_stride, int k,
                  uint32_t grid_x) {
  if (!rows || !queries || !ids || !out || n_rows < 1 || pitch4 < 1 || nq < 1 || n_ids < 1 || grid_x < 1 || qb < 1) return -1;
  if (mode < 0 || mode > 2 || !list_k_ok(mode, k)) return -1;
  if (!ids_below(ids, n_ids, n_rows)) return -1;
  if (mode == 2 ? (key_stride < n_ids || (uint64_t)(nq - 1) * key_stride + n_ids > n_out) : (uint64_t)nq * k * grid_x > n_out) return -1;
  const subset_fn fn = pick_subset(metric, mode, qb, pitch4);
  if (!fn) return -1;
  Bufs b;
  SubsetArgs a = {};
  a.rows = (const f4*)b.up(rows, (size_t)n_rows * pitch4 * sizeof(f4));
  a.queries = (const f4*)b.up(queries, (size_t)nq * pitch4 * sizeof(f4));
  a.ids = (const uint32_t*)b.up(ids, (size_t)n_ids * sizeof(uint32_t));
  a.out = (u64*)b.up(out, (size_t)n_out * sizeof(u64));
  a.key_stride = key_stride;
  a.n_ids = n_ids;
  a.pitch4 = pitch4;
  a.nq = nq;
  a.k = k;
  if (b.err != hipSuccess) return finish(b);
  const size_t lds = mode == 2 ? 0 : subset_lists_lds(qb, k);
  if ((b.err = allow_lds((const void*)fn, lds)) != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(grid_x, (nq + (uint32_t)qb - 1) / (uint32_t)qb), dim3(256), lds, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, a.out, (size_t)n_out * sizeof(u64));
  return finish(b);
}

// rowlists_kernel<metric, qb, NI(pitch4)>, one workgroup per item: grid_x = the first grid_x of the n_items items.
// queries: [n_slots, pitch4] quads, ids: [n_ids] (the lists back to back), items: [n_items] of five 32-bit words, keys: [n_keys].
int listed_rowlists(int metric, int qb, const float* rows, uint64_t n_rows, uint32_t pitch4, const float* queries,
                    uint32_t n_slots, const uint32_t* ids, uint64_t n_ids, const uint32_t* items, uint32_t n_items, u64* keys,
                    uint64_t n_keys, uint64_t stride, uint32_t grid_x) {
  if (!rows || !queries || !ids || !items || !keys || n_rows < 1 || pitch4 < 1 || n_slots < 1 || qb < 1) return -1;
  if (grid_x < 1 || grid_x > n_items) return -1;
  static_assert(sizeof(RowListsItem) == 5 * sizeof(uint32_t), "the items are five 32-bit words");
  const RowListsItem* it = (const RowListsItem*)items;
  for (uint32_t i = 0; i < n_items; ++i) {
    if (it[i].n < 1 || it[i].nq < 1 || it[i].nq > (uint32_t)qb) return -1;
    if ((uint64_t)it[i].first + it[i].n > n_ids || (uint64_t)it[i].offset + it[i].n > stride) return -1;
    if ((uint64_t)it[i].slot + it[i].nq > n_slots) return -1;
    if (((uint64_t)it[i].slot + it[i].nq - 1) * stride + it[i].offset + it[i].n > n_keys) return -1;
    if (!ids_below(ids + it[i].first, it[i].n, n_rows)) return -1;
  }
  const rowlists_fn fn = pick_rowlists(metric, qb, pitch4);
  if (!fn) return -1;
  Bufs b;
  RowListsArgs a = {};
  a.rows = (const f4*)b.up(rows, (size_t)n_rows * pitch4 * sizeof(f4));
  a.queries = (const f4*)b.up(queries, (size_t)n_slots * pitch4 * sizeof(f4));
  a.ids = (const uint32_t*)b.up(ids, (size_t)n_ids * sizeof(uint32_t));
  a.items = (const RowListsItem*)b.up(items, (size_t)n_items * sizeof(RowListsItem));
  a.keys = (u64*)b.up(keys, (size_t)n_keys * sizeof(u64));
  a.stride = stride;
  a.pitch4 = pitch4;
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(grid_x), dim3(256), 0, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(keys, a.keys, (size_t)n_keys * sizeof(u64));
  return finish(b);
}

// label_keys_kernel<metric, qb, NI(pitch4)>, grid (grid_x, ceil(nq / qb)).  order, dense: [n]; span_item0: [span_entries] =
// ceil(n / 64) + 1 entries, span s holding exactly the runs of dense inside it; mask: null or [mask_words] >= ceil(n_rows / 32);
// keys: [n_keys], (nq - 1) * key_stride + n_items of them the kernel's.
int listed_label_keys(int metric, int qb, const float* rows, uint64_t n_rows, uint32_t pitch4, const float* queries, uint32_t nq,
                      const uint32_t* order, const uint32_t* dense, uint32_t n, const uint32_t* span_item0, uint64_t span_entries,
                      const uint32_t* mask, uint64_t mask_words, u64* keys, uint64_t n_keys, uint64_t key_stride, uint32_t grid_x) {
  if (!rows || !queries || !order || !dense || !span_item0 || !keys || n_rows < 1 || pitch4 < 1 || nq < 1 || n < 1 || grid_x < 1 || qb < 1)
    return -1;
  const uint32_t n_spans = (uint32_t)(((uint64_t)n + LABEL_SPAN - 1) / LABEL_SPAN);
  if (span_entries != (uint64_t)n_spans + 1 || span_item0[0] != 0) return -1;
  if (!ids_below(order, n, n_rows)) return -1;
  for (uint32_t s = 0; s < n_spans; ++s) {  // the items a wave writes for span s: one per run of dense inside it
    const uint32_t p0 = s * LABEL_SPAN, p1 = (uint32_t)std::min<uint64_t>((uint64_t)p0 + LABEL_SPAN, n);
    uint32_t runs = 1;
    for (uint32_t p = p0 + 1; p < p1; ++p) runs += dense[p] != dense[p - 1];
    if (span_item0[s + 1] < span_item0[s] || span_item0[s + 1] - span_item0[s] != runs) return -1;
  }
  const uint64_t n_items = span_item0[n_spans];
  if (key_stride < n_items || (uint64_t)(nq - 1) * key_stride + n_items > n_keys) return -1;
  if (mask && mask_words < (n_rows + 31) / 32) return -1;
  const label_keys_fn fn = pick_label_keys(metric, qb, pitch4);
  if (!fn) return -1;
  Bufs b;
  LabelKeysArgs a = {};
  a.rows = (const f4*)b.up(rows, (size_t)n_rows * pitch4 * sizeof(f4));
  a.queries = (const f4*)b.up(queries, (size_t)nq * pitch4 * sizeof(f4));
  a.order = (const uint32_t*)b.up(order, (size_t)n * sizeof(uint32_t));
  a.dense = (const uint32_t*)b.up(dense, (size_t)n * sizeof(uint32_t));
  a.span_item0 = (const uint32_t*)b.up(span_item0, (size_t)span_entries * sizeof(uint32_t));
  a.mask = (const uint32_t*)b.up(mask, (size_t)mask_words * sizeof(uint32_t));
  a.keys = (u64*)b.up(keys, (size_t)n_keys * sizeof(u64));
  a.key_stride = key_stride;
  a.n = n;
  a.n_spans = n_spans;
  a.pitch4 = pitch4;
  a.nq = nq;
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(grid_x, (nq + (uint32_t)qb - 1) / (uint32_t)qb), dim3(256), 0, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(keys, a.keys, (size_t)n_keys * sizeof(u64));
  return finish(b);
}

// label_rank_kernel<mode>, grid (grid_x, nq).  keys: [n_keys] item keys, query q at q * key_stride; label_item0: [n_labels + 1];
// out: [n_out] (lists: nq * k * grid_x words are the kernel's; keys: nq * n_labels).
int listed_label_rank(int mode, const u64* keys, uint64_t n_keys, uint64_t key_stride, uint32_t nq, const uint32_t* label_item0,
                      uint32_t n_labels, u64* out, uint64_t n_out, int k, uint32_t grid_x) {
  if (!keys || !out || nq < 1 || n_labels < 1 || grid_x < 1 || mode < 0 || mode > 2 || !list_k_ok(mode, k)) return -1;
  if (!item_table_ok(label_item0, (uint64_t)n_labels + 1)) return -1;
  const uint64_t n_items = label_item0[n_labels];
  if (key_stride < n_items || (uint64_t)(nq - 1) * key_stride + n_items > n_keys) return -1;
  if ((mode == 2 ? (uint64_t)nq * n_labels : (uint64_t)nq * k * grid_x) > n_out) return -1;
  const label_rank_fn fn = pick_label_rank(mode);
  if (!fn) return -1;
  Bufs b;
  LabelRankArgs a = {};
  a.keys = (const u64*)b.up(keys, (size_t)n_keys * sizeof(u64));
  a.key_stride = key_stride;
  a.label_item0 = (const uint32_t*)b.up(label_item0, ((size_t)n_labels + 1) * sizeof(uint32_t));
  a.n_labels = n_labels;
  a.out = (u64*)b.up(out, (size_t)n_out * sizeof(u64));
  a.k = k;
  if (b.err != hipSuccess) return finish(b);
  const size_t lds = mode == 2 ? 0 : label_rank_lds(k);
  if ((b.err = allow_lds((const void*)fn, lds)) != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(grid_x, nq), dim3(256), lds, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, a.out, (size_t)n_out * sizeof(u64));
  return finish(b);
}

// multivector_rank_kernel<mode>, grid (grid_x, n_segs).  keys: [n_keys] item keys, vector v of the round at v * key_stride,
// key_rows vectors uploaded; segs: [n_segs] of five 32-bit words; acc: null or [n_acc] >= n_labels; out: [n_out] (lists: slot s
// at s * k * grid_x; keys: slot s at s * n_labels).  Refused: two segments of one launch of which one reads acc and another
// writes it, two that write it, two ranked segments with one slot.
int listed_multivector_rank(int mode, const u64* keys, uint64_t n_keys, uint64_t key_stride, uint32_t key_rows,
                            const uint32_t* label_item0, uint32_t n_labels, const uint32_t* segs, uint32_t n_segs, float* acc,
                            uint64_t n_acc, u64* out, uint64_t n_out, int k, uint32_t grid_x) {
  if (!keys || !segs || !out || key_rows < 1 || n_labels < 1 || n_segs < 1 || grid_x < 1 || mode < 0 || mode > 2 || !list_k_ok(mode, k))
    return -1;
  if (!item_table_ok(label_item0, (uint64_t)n_labels + 1)) return -1;
  const uint64_t n_items = label_item0[n_labels];
  if (key_stride < n_items || (uint64_t)(key_rows - 1) * key_stride + n_items > n_keys) return -1;
  static_assert(sizeof(MultivectorSegment) == 5 * sizeof(uint32_t), "the segments are five 32-bit words");
  const MultivectorSegment* sg = (const MultivectorSegment*)segs;
  const uint64_t per_slot = mode == 2 ? (uint64_t)n_labels : (uint64_t)k * grid_x;
  int readers = 0, writers = 0, both = 0;
  for (uint32_t i = 0; i < n_segs; ++i) {
    if (sg[i].v0 >= sg[i].v1 || sg[i].v1 > key_rows) return -1;
    const bool in = sg[i].carry & MV_CARRY_IN, outw = sg[i].carry & MV_CARRY_OUT;
    readers += in;
    writers += outw;
    both += in && outw;
    if ((in || outw) && (!acc || n_acc < n_labels)) return -1;
    if (!outw) {
      if (((uint64_t)sg[i].slot + 1) * per_slot > n_out) return -1;
      for (uint32_t j = 0; j < i; ++j)
        if (!(sg[j].carry & MV_CARRY_OUT) && sg[j].slot == sg[i].slot) return -1;
    }
  }
  if (writers > 1 || (writers == 1 && readers > both)) return -1;
  const multivector_rank_fn fn = pick_multivector_rank(mode);
  if (!fn) return -1;
  Bufs b;
  MultivectorRankArgs a = {};
  a.keys = (const u64*)b.up(keys, (size_t)n_keys * sizeof(u64));
  a.key_stride = key_stride;
  a.label_item0 = (const uint32_t*)b.up(label_item0, ((size_t)n_labels + 1) * sizeof(uint32_t));
  a.n_labels = n_labels;
  a.segs = (const MultivectorSegment*)b.up(segs, (size_t)n_segs * sizeof(MultivectorSegment));
  a.acc = (float*)b.up(acc, (size_t)n_acc * sizeof(float));
  a.out = (u64*)b.up(out, (size_t)n_out * sizeof(u64));
  a.k = k;
  if (b.err != hipSuccess) return finish(b);
  const size_t lds = mode == 2 ? 0 : multivector_rank_lds(k);
  if ((b.err = allow_lds((const void*)fn, lds)) != hipSuccess) return finish(b);
  hipLaunchKernelGGL(fn, dim3(grid_x, n_segs), dim3(256), lds, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(acc, a.acc, (size_t)n_acc * sizeof(float));
  b.down(out, a.out, (size_t)n_out * sizeof(u64));
  return finish(b);
}

}  // extern "C"
