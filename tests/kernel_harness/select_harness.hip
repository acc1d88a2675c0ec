// select_harness.hip -- test-only launcher of the library's selection kernels (tests/select_harness.py,
// tests/test_gpu_select_kernels.py): the u8 / u6 / i8 quantisers, the row norms, the u8 and u6 selection scans, the exact
// re-scoring and the cut behind it.
//
// Built from the very headers libwdbx_hip.so is built from (kernels_common.h, kernels_merge_select.h, kernels_scan8.h,
// kernels_scan6.h, kernels_tiles.h and kernels_tiles8.h -- for the two i8 quantisers of the tile path; the tile kernels are
// templates and are not instantiated here --, kernels_aux.h are included below); the instance of every launch is chosen by
// the pickers that live next to the kernels there (scan8_shape / pick_scan8 / pick_scan8_sample4, u6_unit_chunk /
// pick_scan6) and the grids by the helpers next to them (rows_to_u8_grid, rows_to_u6_grid, row_sqnorm_grid,
// rows_to_i8g_grid, queries_to_i8_grid, scan_sample_grid, scan_full_grid).  This file
// defines no kernel of its own.  Each entry point takes HOST pointers: copy in, launch on the null stream, synchronise, copy
// out; it returns the HIP error code, or -1 when the arguments would make a kernel read or write outside the uploaded arrays
// (checked here, before anything is launched).  Output arrays are copied IN as well, so a slot the kernel leaves alone
// comes back with whatever the caller put there.  Every array comes with its length: the checks are against those.

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
#include "kernels_tiles.h"
#include "kernels_tiles8.h"
#include "kernels_aux.h"

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

hipError_t device_cus(uint32_t* cus) {
  int dev = 0, n = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
  *cus = (uint32_t)std::max(n, 1);
  return e;
}

}  // namespace

extern "C" {

// the instantiated u8 row shape that serves `dim` (scan8_shape): 16-byte pieces per row, lanes per row, loads per lane;
// sample4: 1 when scan8_sample4_kernel has an instance of it.  -1: none.
int sel_scan8_shape(uint32_t dim, uint32_t* pieces, int* L, int* QPL, int* sample4) {
  const Scan8Shape* sh = scan8_shape(dim);
  if (!sh) return -1;
  *pieces = sh->pieces;
  *L = sh->L;
  *QPL = sh->QPL;
  *sample4 = pick_scan8_sample4<WDBX_METRIC_COSINE>(sh->L, sh->QPL) ? 1 : 0;
  return 0;
}

// units in flight per wave of the u6 scans for rows of `units` 16-element units (u6_unit_chunk); 0 = no instance
int sel_u6_unit_chunk(uint32_t units) { return u6_unit_chunk(units); }

uint32_t sel_u6_cut_seg() { return U6_CUT_SEG; }

// rows_to_u8_kernel over rows [r0, n) of rows[n_alloc][pitch]; out: [n_alloc][pitch8] bytes, scale: [n_alloc].
// grid 0: rows_to_u8_grid(n - r0).
int sel_rows_to_u8(const float* rows, uint64_t n_alloc, uint64_t r0, uint64_t n, uint32_t dim, uint32_t pitch, uint32_t pitch8,
                   uint32_t grid, uint8_t* out, float* scale) {
  if (!rows || !out || !scale || n > n_alloc || r0 > n || dim < 1 || dim > pitch || pitch8 < 1) return -1;
  Bufs b;
  const float* d_rows = (const float*)b.up(rows, (size_t)n_alloc * pitch * sizeof(float));
  uint8_t* d_out = (uint8_t*)b.up(out, (size_t)n_alloc * pitch8);
  float* d_scale = (float*)b.up(scale, (size_t)n_alloc * sizeof(float));
  if (b.err != hipSuccess) return finish(b);
  if (!grid) grid = std::max<uint32_t>(1, rows_to_u8_grid(n - r0));
  hipLaunchKernelGGL(rows_to_u8_kernel, dim3(grid), dim3(256), 0, nullptr, d_rows, (u64)r0, (u64)n, dim, pitch, d_out, pitch8, d_scale);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, d_out, (size_t)n_alloc * pitch8);
  b.down(scale, d_scale, (size_t)n_alloc * sizeof(float));
  return finish(b);
}

// rows_to_u6_kernel over rows [r0, n); units = pitch / 16; codes: [ceil(n_alloc / 64)][units][64][3] dwords, sa: [n_alloc][2].
// grid 0: rows_to_u6_grid(n - r0).
int sel_rows_to_u6(const float* rows, uint64_t n_alloc, uint64_t r0, uint64_t n, uint32_t dim, uint32_t pitch, uint32_t grid,
                   uint32_t* codes, float* sa) {
  if (!rows || !codes || !sa || n > n_alloc || r0 > n || dim < 1 || dim > pitch || pitch % 16 != 0) return -1;
  const uint32_t units = pitch / 16;
  const size_t code_bytes = (size_t)((n_alloc + 63) / 64) * units * 768;
  Bufs b;
  const float* d_rows = (const float*)b.up(rows, (size_t)n_alloc * pitch * sizeof(float));
  uint32_t* d_codes = (uint32_t*)b.up(codes, code_bytes);
  f2v* d_sa = (f2v*)b.up(sa, (size_t)n_alloc * sizeof(f2v));
  if (b.err != hipSuccess) return finish(b);
  if (!grid) grid = std::max<uint32_t>(1, rows_to_u6_grid(n - r0));
  hipLaunchKernelGGL(rows_to_u6_kernel, dim3(grid), dim3(256), 0, nullptr, d_rows, (u64)r0, (u64)n, dim, pitch, units, d_codes, d_sa);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(codes, d_codes, code_bytes);
  b.down(sa, d_sa, (size_t)n_alloc * sizeof(f2v));
  return finish(b);
}

// row_sqnorm_kernel over rows [r0, n); cn: [n_alloc]; stats: the three statistics words (copied in and out) or null.
int sel_row_sqnorm(const float* rows, uint64_t n_alloc, uint64_t r0, uint64_t n, uint32_t pitch, uint32_t grid, float* cn,
                   uint32_t* stats) {
  if (!rows || !cn || n > n_alloc || r0 > n || pitch < 4 || pitch % 4 != 0) return -1;
  Bufs b;
  const float* d_rows = (const float*)b.up(rows, (size_t)n_alloc * pitch * sizeof(float));
  float* d_cn = (float*)b.up(cn, (size_t)n_alloc * sizeof(float));
  uint32_t* d_stats = (uint32_t*)b.up(stats, 3 * sizeof(uint32_t));
  if (b.err != hipSuccess) return finish(b);
  if (!grid) grid = std::max<uint32_t>(1, row_sqnorm_grid(n - r0));
  hipLaunchKernelGGL(row_sqnorm_kernel, dim3(grid), dim3(256), 0, nullptr, d_rows, (u64)r0, (u64)n, pitch, d_cn, d_stats);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(cn, d_cn, (size_t)n_alloc * sizeof(float));
  b.down(stats, d_stats, 3 * sizeof(uint32_t));
  return finish(b);
}

// byte offset of (row, col) in the fragment-ordered i8 shadow (g8_offset), for the tests' numpy restatement of the layout
uint64_t sel_g8_offset(uint64_t r, uint32_t col, uint32_t pitch8) { return (uint64_t)g8_offset((u64)r, col, pitch8); }

// rows_to_i8g_kernel over the 64-row groups [g0, g1) of rows[n_alloc][pitch], of which the first n_rows exist; out: [g1 * 64 *
// pitch8] signed bytes in the kernel's fragment order (pitch8 a multiple of 64, >= dim); groups: [g1][4]; gbad: [g1].
// grid 0: rows_to_i8g_grid(g1 - g0).
int sel_rows_to_i8g(const float* rows, uint64_t n_alloc, uint64_t g0, uint64_t g1, uint64_t n_rows, uint32_t dim, uint32_t pitch,
                    uint32_t pitch8, uint32_t grid, int8_t* out, float* groups, u64* gbad) {
  if (!rows || !out || !groups || !gbad || n_rows > n_alloc || n_alloc < 1 || g0 > g1 || g1 < 1 || dim < 1 || dim > pitch) return -1;
  if (pitch8 < dim || pitch8 % 64 != 0) return -1;
  Bufs b;
  const size_t out_bytes = (size_t)g1 * 64 * pitch8;
  const float* d_rows = (const float*)b.up(rows, (size_t)n_alloc * pitch * sizeof(float));
  int8_t* d_out = (int8_t*)b.up(out, out_bytes);
  f4* d_groups = (f4*)b.up(groups, (size_t)g1 * sizeof(f4));
  u64* d_gbad = (u64*)b.up(gbad, (size_t)g1 * sizeof(u64));
  if (b.err != hipSuccess) return finish(b);
  if (!grid) grid = std::max<uint32_t>(1, rows_to_i8g_grid(g1 - g0));
  hipLaunchKernelGGL(rows_to_i8g_kernel, dim3(grid), dim3(256), 0, nullptr, d_rows, (u64)g0, (u64)g1, (u64)n_rows, dim, pitch, d_out,
                     pitch8, d_groups, d_gbad);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, d_out, out_bytes);
  b.down(groups, d_groups, (size_t)g1 * sizeof(f4));
  b.down(gbad, d_gbad, (size_t)g1 * sizeof(u64));
  return finish(b);
}

// queries_to_i8_kernel for a block of gbn queries of which the first nv exist: q: [nv][pitch]; out: [gbn][pitch8] signed
// bytes; qpar: [gbn][4]; tau_init, count_zero: [gbn]; lost_zero: [1].  grid 0: queries_to_i8_grid(gbn).
int sel_queries_to_i8(const float* q, uint32_t nv, uint32_t gbn, uint32_t dim, uint32_t pitch, uint32_t pitch8, uint32_t grid,
                      int8_t* out, float* qpar, float* tau_init, uint32_t* count_zero, uint32_t* lost_zero) {
  if (!q || !out || !qpar || !tau_init || !count_zero || !lost_zero || nv < 1 || nv > gbn || dim < 1 || dim > pitch || pitch8 < 1) return -1;
  Bufs b;
  const float* d_q = (const float*)b.up(q, (size_t)nv * pitch * sizeof(float));
  int8_t* d_out = (int8_t*)b.up(out, (size_t)gbn * pitch8);
  f4* d_qpar = (f4*)b.up(qpar, (size_t)gbn * sizeof(f4));
  float* d_tau = (float*)b.up(tau_init, (size_t)gbn * sizeof(float));
  uint32_t* d_count = (uint32_t*)b.up(count_zero, (size_t)gbn * sizeof(uint32_t));
  uint32_t* d_lost = (uint32_t*)b.up(lost_zero, sizeof(uint32_t));
  if (b.err != hipSuccess) return finish(b);
  if (!grid) grid = std::max<uint32_t>(1, queries_to_i8_grid(gbn));
  hipLaunchKernelGGL(queries_to_i8_kernel, dim3(grid), dim3(256), 0, nullptr, d_q, dim, pitch, nv, d_out, pitch8, gbn, d_qpar, d_tau,
                     d_count, d_lost);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, d_out, (size_t)gbn * pitch8);
  b.down(qpar, d_qpar, (size_t)gbn * sizeof(f4));
  b.down(tau_init, d_tau, (size_t)gbn * sizeof(float));
  b.down(count_zero, d_count, (size_t)gbn * sizeof(uint32_t));
  b.down(lost_zero, d_lost, sizeof(uint32_t));
  return finish(b);
}

// the scalar arguments of one u8 scan launch
struct SelScan8 {
  int32_t phase;   // 0, 1, 2 = scan8_kernel<PHASE>; 3 = scan8_sample4_kernel
  int32_t metric;
  uint32_t n_rows, dim;  // dim chooses the instance (scan8_shape); the shadow's rows are pieces * 16 bytes
  uint32_t qquads;       // quads per query in `queries`
  uint32_t nq;           // grid.y (sample4: queries of the launch)
  uint32_t num_tiles, tile_stride, sample_nt;  // sample passes
  uint32_t tau_n;        // > 0: the in-kernel threshold from tau_keys[0 .. tau_n) (one query)
  int32_t tau_k;
  uint32_t cap;
  uint32_t grid_x;       // 0: the library's (scan_sample_grid / scan_full_grid at 2 workgroups per CU)
};

// shadow: [n_rows][pieces * 16] bytes; scale: [n_rows]; cn: [n_rows] (L2) or null; queries: [nq][qquads * 4]; mask:
// [ceil(n_rows / 32)] or null; tau: [nq] or null; tau_keys: [tau_n] or null; halfmax: [halfmax_len] (sample passes:
// >= nq * num_tiles * 4); cand: [cand_len] (full passes: >= nq * cap; what lies behind is the caller's guard); count: [nq].
int sel_scan8(const SelScan8* d, const uint8_t* shadow, uint64_t shadow_bytes, const float* scale, const float* cn,
              const float* queries, const uint32_t* mask, const float* tau, const u64* tau_keys, u64* halfmax, uint64_t halfmax_len,
              u64* cand, uint64_t cand_len, uint32_t* count) {
  if (!d || !shadow || !scale || !queries || !count || d->n_rows < 1 || d->nq < 1 || d->qquads < 1) return -1;
  if (d->phase < 0 || d->phase > 3 || (d->metric != WDBX_METRIC_COSINE && d->metric != WDBX_METRIC_L2)) return -1;
  const bool l2 = d->metric == WDBX_METRIC_L2, sample = d->phase == 0 || d->phase == 3;
  if (l2 && !cn) return -1;
  const Scan8Shape* sh = scan8_shape(d->dim);
  if (!sh || shadow_bytes != (uint64_t)d->n_rows * sh->pieces * 16) return -1;
  scan8_fn fn = nullptr;
  switch (d->phase) {
    case 0: fn = l2 ? pick_scan8<0, WDBX_METRIC_L2>(sh->L, sh->QPL) : pick_scan8<0, WDBX_METRIC_COSINE>(sh->L, sh->QPL); break;
    case 1: fn = l2 ? pick_scan8<1, WDBX_METRIC_L2>(sh->L, sh->QPL) : pick_scan8<1, WDBX_METRIC_COSINE>(sh->L, sh->QPL); break;
    case 2: fn = l2 ? pick_scan8<2, WDBX_METRIC_L2>(sh->L, sh->QPL) : pick_scan8<2, WDBX_METRIC_COSINE>(sh->L, sh->QPL); break;
    case 3: fn = l2 ? pick_scan8_sample4<WDBX_METRIC_L2>(sh->L, sh->QPL) : pick_scan8_sample4<WDBX_METRIC_COSINE>(sh->L, sh->QPL); break;
  }
  if (!fn) return -1;
  uint32_t ngroups = 0;
  if (sample) {
    // (rows past the end are clamped by the kernel; the group's first row must not wrap around 2^32)
    if (!halfmax || d->num_tiles < 1 || d->tile_stride < 1 || (uint64_t)d->num_tiles * d->tile_stride * 256 >= (1ull << 32)) return -1;
    ngroups = d->num_tiles * 4;
    if ((uint64_t)d->nq * ngroups > halfmax_len) return -1;
  } else {
    if (!cand || d->cap < 1 || (uint64_t)d->nq * d->cap > cand_len) return -1;
    if (d->phase == 1 && d->tau_n) {
      if (!tau_keys || d->tau_n > 1024 || d->tau_k < 1 || d->nq != 1) return -1;  // (the keys are one query's)
    } else if (!tau) {
      return -1;
    }
  }
  Bufs b;
  uint32_t cus = 1;
  if ((b.err = device_cus(&cus)) != hipSuccess) return finish(b);
  Scan8Args a = {};
  a.rows8 = (const u4v*)b.up(shadow, shadow_bytes);
  a.scale = (const float*)b.up(scale, (size_t)d->n_rows * sizeof(float));
  a.cn = (const float*)b.up(cn, (size_t)d->n_rows * sizeof(float));
  a.query = (const f4*)b.up(queries, (size_t)d->nq * d->qquads * sizeof(f4));
  a.mask = (const uint32_t*)b.up(mask, (size_t)((d->n_rows + 31) / 32) * sizeof(uint32_t));
  a.n_rows = d->n_rows;
  a.pieces = sh->pieces;
  a.qquads = d->qquads;
  a.halfmax = (u64*)b.up(halfmax, (size_t)halfmax_len * sizeof(u64));
  a.num_tiles = d->num_tiles;
  a.tile_stride = d->tile_stride;
  a.sample_nt = d->sample_nt;
  a.tau = (const float*)b.up(tau, (size_t)d->nq * sizeof(float));
  if (d->phase == 1 && d->tau_n) {
    a.tau_keys = (const u64*)b.up(tau_keys, (size_t)d->tau_n * sizeof(u64));
    a.tau_n = d->tau_n;
    a.tau_k = d->tau_k;
  }
  a.cand = (u64*)b.up(cand, (size_t)cand_len * sizeof(u64));
  a.count = (uint32_t*)b.up(count, (size_t)d->nq * sizeof(uint32_t));
  a.cap = d->cap;
  a.nq = d->nq;
  if (b.err != hipSuccess) return finish(b);
  uint32_t gx = d->grid_x, gy = d->nq;
  if (sample) {
    if (!gx) gx = scan_sample_grid(ngroups, cus);
    if (d->phase == 3) {
      const uint32_t qn = sh->QPL >= 3 ? 3 : 4;
      gy = (d->nq + qn - 1) / qn;
    }
  } else if (!gx) {
    const uint32_t R = 64u / (uint32_t)sh->L;
    gx = scan_full_grid((d->n_rows + R - 1) / R, cus, 2);
  }
  hipLaunchKernelGGL(fn, dim3(gx, gy), dim3(256), 0, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(halfmax, a.halfmax, (size_t)halfmax_len * sizeof(u64));
  b.down(cand, a.cand, (size_t)cand_len * sizeof(u64));
  b.down(count, a.count, (size_t)d->nq * sizeof(uint32_t));
  return finish(b);
}

// the scalar arguments of one u6 scan launch
struct SelScan6 {
  int32_t sample;  // 1: scan8_u6_sample_kernel, 0: scan8_u6_kernel
  uint32_t n_rows, units, qpitch;
  uint32_t nq;     // sample: queries of the launch; full pass: grid.y
  uint32_t num_tiles, tile_stride;
  uint32_t cap;
  uint32_t grid_x;  // 0: the library's
};

// codes: [ceil(n_rows / 64)][units][64][3] dwords (code_dwords of them); sa: [n_rows][2]; queries: [nq][qpitch]; tau: [nq]
// (full pass); halfmax: [halfmax_len] (sample: >= nq * num_tiles * 4); cand: [cand_len] (full pass: >= nq * cap);
// count, count2: [nq].
int sel_scan6(const SelScan6* d, const uint32_t* codes, uint64_t code_dwords, const float* sa, const float* queries, const float* tau,
              u64* halfmax, uint64_t halfmax_len, u64* cand, uint64_t cand_len, uint32_t* count, uint32_t* count2) {
  if (!d || !codes || !sa || !queries || !count || d->n_rows < 1 || d->nq < 1 || d->units < 1) return -1;
  if ((uint64_t)d->units * 16 > d->qpitch) return -1;
  const int uc = u6_unit_chunk(d->units);
  scan6_fn fn = uc ? pick_scan6(uc, d->sample != 0) : nullptr;
  if (!fn) return -1;
  const uint32_t tiles64 = (d->n_rows + 63) / 64;
  if (code_dwords != (uint64_t)tiles64 * d->units * 192) return -1;
  uint32_t ngroups = 0;
  if (d->sample) {
    if (!halfmax || !count2 || d->num_tiles < 1 || d->tile_stride < 1 || (uint64_t)d->num_tiles * d->tile_stride * 256 >= (1ull << 32))
      return -1;
    ngroups = d->num_tiles * 4;
    if ((uint64_t)d->nq * ngroups > halfmax_len) return -1;
  } else if (!cand || !tau || d->cap < 1 || (uint64_t)d->nq * d->cap > cand_len) {
    return -1;
  }
  Bufs b;
  uint32_t cus = 1;
  if ((b.err = device_cus(&cus)) != hipSuccess) return finish(b);
  Scan6Args a = {};
  a.codes = (const uint32_t*)b.up(codes, (size_t)code_dwords * sizeof(uint32_t));
  a.sa = (const f2v*)b.up(sa, (size_t)d->n_rows * sizeof(f2v));
  a.query = (const float*)b.up(queries, (size_t)d->nq * d->qpitch * sizeof(float));
  a.n_rows = d->n_rows;
  a.units = d->units;
  a.qpitch = d->qpitch;
  a.halfmax = (u64*)b.up(halfmax, (size_t)halfmax_len * sizeof(u64));
  a.num_tiles = d->num_tiles;
  a.tile_stride = d->tile_stride;
  a.nq = d->nq;
  a.tau = (const float*)b.up(tau, (size_t)d->nq * sizeof(float));
  a.cand = (u64*)b.up(cand, (size_t)cand_len * sizeof(u64));
  a.count = (uint32_t*)b.up(count, (size_t)d->nq * sizeof(uint32_t));
  a.count2 = (uint32_t*)b.up(count2, (size_t)d->nq * sizeof(uint32_t));
  a.cap = d->cap;
  if (b.err != hipSuccess) return finish(b);
  uint32_t gx = d->grid_x;
  if (!gx) gx = d->sample ? scan_sample_grid(ngroups, cus) : scan_full_grid(tiles64, cus, 2);
  const uint32_t gy = d->sample ? (d->nq + 3) / 4 : d->nq;
  hipLaunchKernelGGL(fn, dim3(gx, gy), dim3(256), 0, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(halfmax, a.halfmax, (size_t)halfmax_len * sizeof(u64));
  b.down(cand, a.cand, (size_t)cand_len * sizeof(u64));
  b.down(count, a.count, (size_t)d->nq * sizeof(uint32_t));
  b.down(count2, a.count2, (size_t)d->nq * sizeof(uint32_t));
  return finish(b);
}

// rescore_kernel<metric> as the library launches it (grid (256, nq)): rows: [n_rows][pitch4 * 4]; queries: [nq][pitch4 * 4];
// cand: [cand_len] >= nq * cap keys, re-scored in place; count: [nq].  Every key the kernel will read must name a row < n_rows.
int sel_rescore(int metric, const float* rows, uint64_t n_rows, uint32_t pitch4, const float* queries, uint32_t nq, u64* cand,
                uint64_t cand_len, const uint32_t* count, uint32_t cap, uint32_t grid_x) {
  if (!rows || !queries || !cand || !count || n_rows < 1 || pitch4 < 1 || nq < 1 || cap < 1 || (uint64_t)nq * cap > cand_len) return -1;
  if (metric != WDBX_METRIC_COSINE && metric != WDBX_METRIC_L2) return -1;
  for (uint32_t q = 0; q < nq; ++q)
    for (uint32_t j = 0; j < std::min(count[q], cap); ++j)
      if ((uint64_t)(~(uint32_t)(cand[(size_t)q * cap + j] & 0xFFFFFFFFull)) >= n_rows) return -1;
  Bufs b;
  const f4* d_rows = (const f4*)b.up(rows, (size_t)n_rows * pitch4 * sizeof(f4));
  const f4* d_q = (const f4*)b.up(queries, (size_t)nq * pitch4 * sizeof(f4));
  u64* d_cand = (u64*)b.up(cand, (size_t)cand_len * sizeof(u64));
  const uint32_t* d_count = (const uint32_t*)b.up(count, (size_t)nq * sizeof(uint32_t));
  if (b.err != hipSuccess) return finish(b);
  const dim3 grid(grid_x ? grid_x : 256, nq);
  if (metric == WDBX_METRIC_L2)
    hipLaunchKernelGGL(rescore_kernel<WDBX_METRIC_L2>, grid, dim3(256), 0, nullptr, d_rows, pitch4, d_q, d_cand, d_count, cap,
                       (u64*)nullptr, (uint32_t*)nullptr);
  else
    hipLaunchKernelGGL(rescore_kernel<WDBX_METRIC_COSINE>, grid, dim3(256), 0, nullptr, d_rows, pitch4, d_q, d_cand, d_count, cap,
                       (u64*)nullptr, (uint32_t*)nullptr);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(cand, d_cand, (size_t)cand_len * sizeof(u64));
  return finish(b);
}

// u6_cut_kernel as the library launches it (grid (ceil(cap / U6_CUT_SEG), nq)): cand: [nq][cap]; count: [nq]; out: [out_len]
// >= nq * cap2 (what lies behind is the caller's guard); count2: [nq], copied in (the library's sample pass zeroes it).
int sel_u6_cut(const u64* cand, const uint32_t* count, uint32_t cap, int k, uint32_t nq, u64* out, uint64_t out_len, uint32_t* count2,
               uint32_t cap2) {
  if (!cand || !count || !out || !count2 || cap < 1 || cap2 < 1 || nq < 1 || k < 1 || (uint64_t)nq * cap2 > out_len) return -1;
  Bufs b;
  const u64* d_cand = (const u64*)b.up(cand, (size_t)nq * cap * sizeof(u64));
  const uint32_t* d_count = (const uint32_t*)b.up(count, (size_t)nq * sizeof(uint32_t));
  u64* d_out = (u64*)b.up(out, (size_t)out_len * sizeof(u64));
  uint32_t* d_count2 = (uint32_t*)b.up(count2, (size_t)nq * sizeof(uint32_t));
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(u6_cut_kernel, dim3((cap + U6_CUT_SEG - 1) / U6_CUT_SEG, nq), dim3(1024), 0, nullptr, d_cand, d_count, cap, k,
                     d_out, d_count2, cap2);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, d_out, (size_t)out_len * sizeof(u64));
  b.down(count2, d_count2, (size_t)nq * sizeof(uint32_t));
  return finish(b);
}

}  // extern "C"
