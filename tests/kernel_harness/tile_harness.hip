// tile_harness.hip -- test-only launcher of the int8 tile kernel ALONE (tests/tile_harness.py, tests/test_gpu_tile_kernels.py):
// gemm_i8_kernel in both phases and the two small kernels that feed its arguments, gbad_with_mask_kernel and
// group_ref_kernel, on bytes, tables and thresholds the caller hands it.
//
// Built from the very headers libwdbx_hip.so is built from; this file defines no kernel of its own.  The instance, its
// ring, its LDS bytes and the launch itself come from the helpers that live behind the kernel in kernels_tiles8.h
// (gemm8_launch_of / gemm8_prepare / gemm8_grid / enqueue_gemm8: what host_index.h::launch_gemm8 calls), so every instance
// the pickers can return is instantiated here.  Built by `make -C wdbx-py_amd/csrc all` as
// tests/kernel_harness/libtile_harness.so.
//
// Each entry point takes HOST pointers, each with its length: copy in, launch on the null stream, synchronise, copy out.
// Output arrays are copied IN as well, so a slot the kernel leaves alone comes back with whatever the caller put there.
// It returns the HIP error code, or -1 -- before anything is launched -- when the arguments would let a kernel read or write
// outside the uploaded arrays.  The checks follow the kernel's real extents (tile_check below).

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

hipError_t device_cus(uint32_t* cus) {
  int dev = 0, n = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
  *cus = (uint32_t)std::max(n, 1);
  return e;
}

}  // namespace

extern "C" {

// the scalar arguments of one tile launch
struct TileCall {
  int32_t ct;       // query blocks of 64 * ct: 1, 2, 4
  int32_t metric;   // WDBX_METRIC_COSINE (inner product) or WDBX_METRIC_L2
  int32_t masked;   // PHASE 1: the MASKED instance (gbad = the call's bad-row table)
  int32_t multi;    // a mask per query: gbad = n_classes tables of n_class_groups entries, class_row per column group
  int32_t variant;  // option gemm8_variant: 0 / 14, 12, 13
  uint32_t n_rows, pitch8, num_tiles, tile_stride;
  uint32_t grid;    // 0: the library's rule, gemm8_grid(num_tiles, cus)
  uint32_t cus;     // ... for this CU count (0: the device's)
  uint32_t pair_cap;
  uint32_t n_classes;
  uint64_t n_class_groups;
  uint8_t class_row[16];
};

}  // extern "C"

namespace {

bool variant_ok(int v) { return v == 0 || v == 12 || v == 13 || v == 14; }

// What both phases read: false = a launch with these arguments could leave the uploaded arrays.
//   rows8: the loader reads whole tiles, the last one tile (num_tiles - 1) * tile_stride (also when it re-reads "past the end")
//   groups, gbad: one entry per 64 rows, up to the second half of the last tile's last wave
//   cn: [n_rows], index clamped to n_rows - 1 (so n_rows >= 1 for L2)
//   qb8: [64 ct][pitch8], qpar: [64 ct]
bool tile_check(const TileCall* d, int phase, const Gemm8Launch& l, uint64_t rows8_bytes, uint64_t n_groups, uint64_t cn_len,
                bool have_gbad, uint64_t gbad_len, uint64_t qb8_bytes, uint64_t qpar_len) {
  if (d->ct != 1 && d->ct != 2 && d->ct != 4) return false;
  const bool l2 = d->metric == WDBX_METRIC_L2;
  if (d->pitch8 < 128 || d->pitch8 % 128 != 0 || (uint64_t)64 * d->ct * d->pitch8 > (uint64_t)G8_LDS_B_MAX) return false;
  if (!l.fn || l.ring < 1 || (d->pitch8 / 64) % (uint32_t)l.ring != 0) return false;
  if (d->num_tiles < 1 || d->tile_stride < 1) return false;
  const uint64_t last_tile = (uint64_t)(d->num_tiles - 1) * d->tile_stride;
  const uint64_t rows_covered = (last_tile + 1) * G8_ROWS;
  if (rows_covered >= (1ull << 32)) return false;  // (the kernel's row numbers are 32 bits)
  if (rows8_bytes < rows_covered * d->pitch8) return false;
  const uint64_t last_group = (((last_tile * 8 + 7) * 32) >> 6);
  if (n_groups <= last_group) return false;
  if (d->n_rows > rows_covered) return false;
  if (l2 && (d->n_rows < 1 || cn_len < d->n_rows)) return false;
  const uint64_t gbn = (uint64_t)64 * d->ct;
  if (qb8_bytes < gbn * d->pitch8 || qpar_len < gbn) return false;
  if (d->multi) {
    if (!have_gbad || d->n_classes < 1 || d->n_classes > 256 || d->n_class_groups <= last_group) return false;
    if (gbad_len < (uint64_t)d->n_classes * d->n_class_groups) return false;
    for (int j = 0; j < 4 * d->ct; ++j)  // 2 CT8 column groups
      if (d->class_row[j] >= d->n_classes) return false;
  } else if (phase == 0 || d->masked) {
    if (!have_gbad || gbad_len <= last_group) return false;
  }
  return true;
}

uint32_t tile_grid(const TileCall* d, uint32_t cus) { return d->grid ? d->grid : gemm8_grid(d->num_tiles, cus); }

void fill_args(Gemm8Args& g, const TileCall* d) {
  g.n_rows = d->n_rows;
  g.pitch8 = d->pitch8;
  g.num_tiles = d->num_tiles;
  g.tile_stride = d->tile_stride;
  if (d->multi) {
    g.n_class_groups = d->n_class_groups;
    memcpy(g.class_row, d->class_row, sizeof(g.class_row));
  }
}

}  // namespace

extern "C" {

uint32_t tile_lds_b_max() { return (uint32_t)G8_LDS_B_MAX; }
uint32_t tile_pair_d_unknown() { return PAIR_D_UNKNOWN; }

// 1: the library has the instance of these arguments (then *ring = the k-steps in flight it was compiled with, *lds = the
// dynamic LDS bytes of its launch); 0: it has none; -1: not a question the pickers answer
int tile_instance(int phase, int ct, uint32_t pitch8, int l2, int masked, int multi, int variant, int* ring, uint64_t* lds) {
  if ((phase != 0 && phase != 1) || (ct != 1 && ct != 2 && ct != 4) || pitch8 < 128 || pitch8 % 128 != 0 || !variant_ok(variant)) return -1;
  const int metric = l2 ? WDBX_METRIC_L2 : WDBX_METRIC_COSINE;
  const Gemm8Launch l = phase == 0 ? gemm8_launch_of<0>(ct, pitch8, metric, false, multi != 0, variant)
                                   : gemm8_launch_of<1>(ct, pitch8, metric, masked != 0, multi != 0, variant);
  if (ring) *ring = l.ring;
  if (lds) *lds = l.lds;
  return l.fn ? 1 : 0;
}

// PHASE 0.  rows8: the fragment-ordered bytes; groups: [n_groups][4]; cn: [cn_len] (L2) or null; gbad: [gbad_len]; qb8:
// [64 ct][pitch8]; qpar: [64 ct][4]; halfmax: [halfmax_len] >= 64 ct * 8 * num_tiles (what lies behind is the caller's guard).
int tile_phase0(const TileCall* d, const int8_t* rows8, uint64_t rows8_bytes, const float* groups, uint64_t n_groups, const float* cn,
                uint64_t cn_len, const u64* gbad, uint64_t gbad_len, const int8_t* qb8, uint64_t qb8_bytes, const float* qpar,
                uint64_t qpar_len, u64* halfmax, uint64_t halfmax_len) {
  if (!d || !rows8 || !groups || !qb8 || !qpar || !halfmax || d->masked || !variant_ok(d->variant)) return -1;
  if (d->metric != WDBX_METRIC_COSINE && d->metric != WDBX_METRIC_L2) return -1;
  if (d->metric == WDBX_METRIC_L2 && !cn) return -1;
  const Gemm8Launch l = gemm8_launch_of<0>(d->ct, d->pitch8, d->metric, false, d->multi != 0, d->variant);
  if (!tile_check(d, 0, l, rows8_bytes, n_groups, cn_len, gbad != nullptr, gbad_len, qb8_bytes, qpar_len)) return -1;
  if (halfmax_len < (uint64_t)64 * d->ct * 8 * d->num_tiles) return -1;
  if (d->grid > 4096) return -1;
  uint32_t cus = d->cus;  // (asked of the device only when the caller names neither a grid nor a CU count)
  if (!d->grid && !cus) {
    const hipError_t e = device_cus(&cus);
    if (e != hipSuccess) return (int)e;
  }
  Bufs b;
  Gemm8Args g = {};
  g.rows8 = (const int8_t*)b.up(rows8, (size_t)rows8_bytes);
  g.groups = (const f4*)b.up(groups, (size_t)n_groups * sizeof(f4));
  g.cn = (const float*)b.up(cn, (size_t)cn_len * sizeof(float));
  g.gbad = (const u64*)b.up(gbad, (size_t)gbad_len * sizeof(u64));
  g.qb8 = (const int8_t*)b.up(qb8, (size_t)qb8_bytes);
  g.qpar = (const f4*)b.up(qpar, (size_t)qpar_len * sizeof(f4));
  g.halfmax = (u64*)b.up(halfmax, (size_t)halfmax_len * sizeof(u64));
  fill_args(g, d);
  if (b.err != hipSuccess) return finish(b);
  if ((b.err = gemm8_prepare(l)) != hipSuccess) return finish(b);
  if ((b.err = enqueue_gemm8(nullptr, l, g, tile_grid(d, cus))) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(halfmax, g.halfmax, (size_t)halfmax_len * sizeof(u64));
  return finish(b);
}

// PHASE 1.  As above, and gref: [gref_len >= 2]; tau: [64 ct]; pairs: [pairs_len] >= grid * 8 * pair_cap (what lies behind
// is the caller's guard); pair_count: [pair_count_len] >= grid * 8.  gbad may be null unless masked or multi.
int tile_phase1(const TileCall* d, const int8_t* rows8, uint64_t rows8_bytes, const float* groups, uint64_t n_groups, const float* cn,
                uint64_t cn_len, const float* gref, uint64_t gref_len, const u64* gbad, uint64_t gbad_len, const int8_t* qb8,
                uint64_t qb8_bytes, const float* qpar, uint64_t qpar_len, const float* tau, uint64_t tau_len, u64* pairs,
                uint64_t pairs_len, uint32_t* pair_count, uint64_t pair_count_len) {
  if (!d || !rows8 || !groups || !qb8 || !qpar || !gref || !tau || !pairs || !pair_count || !variant_ok(d->variant)) return -1;
  if (d->metric != WDBX_METRIC_COSINE && d->metric != WDBX_METRIC_L2) return -1;
  if (d->metric == WDBX_METRIC_L2 && !cn) return -1;
  if (d->masked && d->multi) return -1;
  const Gemm8Launch l = gemm8_launch_of<1>(d->ct, d->pitch8, d->metric, d->masked != 0, d->multi != 0, d->variant);
  if (!tile_check(d, 1, l, rows8_bytes, n_groups, cn_len, gbad != nullptr, gbad_len, qb8_bytes, qpar_len)) return -1;
  if (gref_len < 2 || tau_len < (uint64_t)64 * d->ct || d->pair_cap < 1 || d->grid > 4096) return -1;
  uint32_t cus = d->cus;
  if (!d->grid && !cus) {
    const hipError_t e = device_cus(&cus);
    if (e != hipSuccess) return (int)e;
  }
  const uint32_t grid = tile_grid(d, cus);
  if (pairs_len < (uint64_t)grid * 8 * d->pair_cap || pair_count_len < (uint64_t)grid * 8) return -1;
  Bufs b;
  Gemm8Args g = {};
  g.rows8 = (const int8_t*)b.up(rows8, (size_t)rows8_bytes);
  g.groups = (const f4*)b.up(groups, (size_t)n_groups * sizeof(f4));
  g.cn = (const float*)b.up(cn, (size_t)cn_len * sizeof(float));
  g.gref = (const float*)b.up(gref, (size_t)gref_len * sizeof(float));
  g.gbad = (const u64*)b.up(gbad, (size_t)gbad_len * sizeof(u64));
  g.qb8 = (const int8_t*)b.up(qb8, (size_t)qb8_bytes);
  g.qpar = (const f4*)b.up(qpar, (size_t)qpar_len * sizeof(f4));
  g.tau = (const float*)b.up(tau, (size_t)tau_len * sizeof(float));
  g.pairs = (u64*)b.up(pairs, (size_t)pairs_len * sizeof(u64));
  g.pair_count = (uint32_t*)b.up(pair_count, (size_t)pair_count_len * sizeof(uint32_t));
  g.pair_cap = d->pair_cap;
  fill_args(g, d);
  if (b.err != hipSuccess) return finish(b);
  if ((b.err = gemm8_prepare(l)) != hipSuccess) return finish(b);
  if ((b.err = enqueue_gemm8(nullptr, l, g, grid)) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(pairs, g.pairs, (size_t)pairs_len * sizeof(u64));
  b.down(pair_count, g.pair_count, (size_t)pair_count_len * sizeof(uint32_t));
  return finish(b);
}

// gbad_with_mask_kernel, grid (grid_x or gbad_with_mask_grid(n_groups), n_classes).  gbad: [n_groups]; mask: [mask_len] words
// (null: every class is the one without a mask); class_mask: [n_classes] or null (then n_classes = 1: the one mask, row 0);
// call_bad: [call_bad_len] >= n_classes * n_groups.
int tile_gbad_with_mask(const u64* gbad, uint64_t n_groups, const uint32_t* mask, uint64_t mask_len, uint64_t mask_words,
                        uint64_t mask_stride, const int32_t* class_mask, uint32_t n_classes, u64* call_bad, uint64_t call_bad_len,
                        uint32_t grid_x) {
  if (!gbad || !call_bad || n_groups < 1 || n_classes < 1 || n_classes > 1024 || grid_x > 4096) return -1;
  if (call_bad_len < (uint64_t)n_classes * n_groups || mask_words > (1ull << 40) || mask_stride > (1ull << 40)) return -1;
  if (!class_mask) {
    if (n_classes != 1 || !mask || mask_len < mask_words) return -1;
  } else {
    for (uint32_t y = 0; y < n_classes; ++y)
      if (class_mask[y] >= 0 && (!mask || (uint64_t)class_mask[y] * mask_stride + mask_words > mask_len)) return -1;
  }
  Bufs b;
  const u64* d_gbad = (const u64*)b.up(gbad, (size_t)n_groups * sizeof(u64));
  const uint32_t* d_mask = (const uint32_t*)b.up(mask, (size_t)mask_len * sizeof(uint32_t));
  const int32_t* d_class = (const int32_t*)b.up(class_mask, (size_t)n_classes * sizeof(int32_t));
  u64* d_out = (u64*)b.up(call_bad, (size_t)call_bad_len * sizeof(u64));
  if (b.err != hipSuccess) return finish(b);
  if (!grid_x) grid_x = std::max<uint32_t>(1, gbad_with_mask_grid(n_groups));
  hipLaunchKernelGGL(gbad_with_mask_kernel, dim3(grid_x, n_classes), dim3(256), 0, nullptr, d_gbad, d_mask, (u64)mask_words, (u64)n_groups,
                     d_out, (u64)mask_stride, d_class);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(call_bad, d_out, (size_t)call_bad_len * sizeof(u64));
  return finish(b);
}

// group_ref_kernel, both passes as the host enqueues them: the 8 words {a_ref, b_ref, sum a, sum b, count, -, -, -} zeroed,
// pass 0, pass 1 (grid_x or group_ref_grid(n_groups) workgroups each).  groups: [n_groups][4]; ref: [8] words out.
int tile_group_ref(const float* groups, uint64_t n_groups, uint32_t grid_x, uint32_t* ref) {
  if (!groups || !ref || n_groups < 1 || grid_x > 4096) return -1;
  Bufs b;
  const f4* d_groups = (const f4*)b.up(groups, (size_t)n_groups * sizeof(f4));
  float* d_ref = (float*)b.up(ref, 8 * sizeof(float));
  if (b.err != hipSuccess) return finish(b);
  if ((b.err = hipMemsetAsync(d_ref, 0, 8 * sizeof(float), nullptr)) != hipSuccess) return finish(b);
  if (!grid_x) grid_x = std::max<uint32_t>(1, group_ref_grid(n_groups));
  for (int pass = 0; pass < 2; ++pass)
    hipLaunchKernelGGL(group_ref_kernel, dim3(grid_x), dim3(256), 0, nullptr, d_groups, (u64)n_groups, d_ref, (uint32_t*)(d_ref + 4), pass);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(ref, d_ref, 8 * sizeof(float));
  return finish(b);
}

}  // extern "C"
