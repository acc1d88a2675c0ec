// gemm_harness.hip -- test-only launcher of the fp32 and bf16 tile kernels ALONE (tests/gemm_harness.py,
// tests/test_gpu_gemm_kernels.py): gemm_topk_kernel and gemm_bf16w8_kernel (on fp32 rows and on the bf16 shadow copy) in
// both phases, the two conversions rows_to_bf16_kernel / queries_to_bf16_kernel, and the small kernels of kernels_aux.h
// that make the tiles' selection sound: cn_stats_kernel, group_max_kernel, query_norm_kernel, tau_margin_kernel.
//
// Built from the very headers libwdbx_hip.so is built from; this file defines no kernel of its own.  The instance, its LDS
// bytes, its K-tail form, its workgroup size and the grid come from the helpers that live behind the kernels in
// kernels_tiles.h (gemm_launch_of / gemm_prepare / gemm_grid / enqueue_gemm: what host_index.h::launch_gemm_ct calls), so
// every instance the picker can return is instantiated here.  Built by `make -C wdbx-py_amd/csrc all` as
// tests/kernel_harness/libgemm_harness.so.
//
// Each entry point takes HOST pointers, each with its length: copy in, launch on the null stream, synchronise, copy out.
// Output arrays are copied IN as well, so a slot the kernel leaves alone comes back with whatever the caller put there.
// It returns the HIP error code, or -1 -- before anything is launched -- when the arguments would let a kernel read or write
// outside the uploaded arrays.  The checks follow the kernels' real extents (gemm_check below).

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
#include "kernels_tiles.h"
#include "kernels_aux.h"

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

GemmLaunch launch_of(int phase, int family, int ct, int metric, bool groupb, uint32_t pitch4) {
  return phase == 0 ? gemm_launch_of<0>(family, ct, metric, groupb, pitch4) : gemm_launch_of<1>(family, ct, metric, groupb, pitch4);
}

bool question_ok(int phase, int family, int ct, int metric, uint32_t pitch4) {
  return (phase == 0 || phase == 1) && (family == GEMM_FP32 || family == GEMM_BF16 || family == GEMM_BF16_SHADOW) &&
         (ct == 1 || ct == 2 || ct == 4) && (metric == WDBX_METRIC_COSINE || metric == WDBX_METRIC_L2) && pitch4 >= 1;
}

}  // namespace

extern "C" {

// the scalar arguments of one tile launch
struct GemmCall {
  int32_t phase;    // 0: halfmax, 1: cand / count
  int32_t family;   // GEMM_FP32, GEMM_BF16, GEMM_BF16_SHADOW
  int32_t ct;       // query blocks of 64 * ct: 1, 2, 4
  int32_t metric;   // WDBX_METRIC_COSINE (inner product) or WDBX_METRIC_L2
  int32_t groupb;   // the GROUPB instance: gmax, qn, eps, gam, floor_abs, under_abs are used
  uint32_t n_rows;
  uint32_t pitch4;  // 16-byte pieces per row: fp32 quads, or (shadow) groups of 8 bf16
  uint32_t num_tiles, tile_stride;
  uint32_t grid;    // 0: the library's rule, gemm_grid(launch, num_tiles, cus)
  uint32_t cus;     // ... for this CU count (0: the device's)
  uint32_t cap;
  uint32_t qb_pitch16;
  uint32_t live;
  float eps, gam, floor_abs, under_abs;
};

uint32_t gemm_tile_pad_rows() { return (uint32_t)TILE_PAD_ROWS; }
uint32_t gemm_rows_per_tile(int family) { return gemm_tile_rows(family); }

// 1: the library has the instance of these arguments (then *lds = the dynamic LDS bytes of its launch, *threads its
// workgroup size, *ktail whether it is the K-tail form, *per_cu the workgroups per CU of the grid rule); 0: it has none;
// -1: not a question the picker answers
int gemm_instance(int phase, int family, int ct, int metric, int groupb, uint32_t pitch4, uint64_t* lds, uint32_t* threads, int* ktail,
                  uint32_t* per_cu, uint64_t* fn_id) {
  if (!question_ok(phase, family, ct, metric, pitch4)) return -1;
  const GemmLaunch l = launch_of(phase, family, ct, metric, groupb != 0, pitch4);
  if (lds) *lds = l.lds;
  if (threads) *threads = l.threads;
  if (ktail) *ktail = l.ktail ? 1 : 0;
  if (per_cu) *per_cu = l.per_cu;
  if (fn_id) *fn_id = (uint64_t)(uintptr_t)l.fn;  // (an identity only: equal for equal instances)
  return l.fn ? 1 : 0;
}

uint32_t gemm_grid_rule(int phase, int family, int ct, int metric, int groupb, uint32_t pitch4, uint32_t num_tiles, uint32_t cus) {
  if (!question_ok(phase, family, ct, metric, pitch4)) return 0;
  return gemm_grid(launch_of(phase, family, ct, metric, groupb != 0, pitch4), num_tiles, cus);
}

// One tile launch.  Lengths are in elements of the named type.
//   rows:    fp32 tiles: [n_rows][pitch4] quads (rows past the end are clamped to the last row);
//            bf16 tiles: whole tiles of 256 rows up to tile (num_tiles - 1) * tile_stride are READ without clamping (the
//            loader re-reads that tile "past the end" as well), at most TILE_PAD_ROWS rows past n_rows as in the library
//   queries: fp32 tiles: [64 ct][pitch4] quads;  qb16: bf16 tiles: [64 ct][qb_pitch16 * 8] bf16, qb_pitch16 >= the K extent
//            the kernel walks (a pair of chunks)
//   cn: [n_rows] (L2), gmax: [ceil(n_rows / 64)], qn: [64 ct] (GROUPB), both indices clamped to the last row
//   PHASE 0: halfmax [64 ct][RW * num_tiles] (what lies behind is the caller's guard)
//   PHASE 1: tau [64 ct], cand [64 ct][cap] (+ guard), count [64 ct] (+ guard)
int gemm_tiles(const GemmCall* d, const void* rows, uint64_t rows_bytes, const float* queries, uint64_t queries_len, const uint16_t* qb16,
               uint64_t qb16_len, const float* cn, uint64_t cn_len, const float* gmax, uint64_t gmax_len, const float* qn, uint64_t qn_len,
               const float* tau, uint64_t tau_len, u64* halfmax, uint64_t halfmax_len, u64* cand, uint64_t cand_len, uint32_t* count,
               uint64_t count_len) {
  if (!d || !rows || !question_ok(d->phase, d->family, d->ct, d->metric, d->pitch4)) return -1;
  const bool fp32 = d->family == GEMM_FP32, shadow = d->family == GEMM_BF16_SHADOW, l2 = d->metric == WDBX_METRIC_L2;
  const GemmLaunch l = launch_of(d->phase, d->family, d->ct, d->metric, d->groupb != 0, d->pitch4);
  if (!l.fn) return -1;
  if (d->n_rows < 1 || d->num_tiles < 1 || d->tile_stride < 1 || d->grid > 4096 || d->pitch4 > (1u << 16)) return -1;
  // the form without a K tail reads whole chunks (fp32: 8 pieces, bf16: pairs of chunks of 8 pieces)
  if (!l.ktail && d->pitch4 % (fp32 ? 8u : 16u) != 0) return -1;
  const uint64_t gbn = (uint64_t)64 * d->ct, tile_rows = gemm_tile_rows(d->family), rw = tile_rows / 64;
  const uint64_t last_tile = (uint64_t)(d->num_tiles - 1) * d->tile_stride;
  const uint64_t rows_covered = (last_tile + 1) * tile_rows;
  if (rows_covered >= (1ull << 32)) return -1;  // (the kernels' row numbers are 32 bits)
  if (fp32) {
    if (rows_bytes < (uint64_t)d->n_rows * d->pitch4 * 16) return -1;
    if (!queries || queries_len < gbn * d->pitch4 * 4) return -1;
  } else {
    if (rows_covered > (uint64_t)d->n_rows + TILE_PAD_ROWS) return -1;
    if (rows_bytes < rows_covered * d->pitch4 * 16) return -1;
    const uint64_t kchunks = (((uint64_t)d->pitch4 + 7) / 8 + 1) / 2 * 2, ppr = shadow ? 8 : 4;
    if (!qb16 || d->qb_pitch16 < kchunks * ppr || qb16_len < gbn * d->qb_pitch16 * 8) return -1;
  }
  if (l2 && (!cn || cn_len < d->n_rows)) return -1;
  if (d->groupb && (!gmax || !qn || gmax_len < ((uint64_t)d->n_rows + 63) / 64 || qn_len < gbn)) return -1;
  if (d->phase == 0) {
    if (!halfmax || halfmax_len < gbn * rw * d->num_tiles) return -1;
  } else {
    if (!tau || !cand || !count || tau_len < gbn || count_len < gbn || cand_len < gbn * d->cap) return -1;
  }
  uint32_t cus = d->cus;  // (asked of the device only when the caller names neither a grid nor a CU count)
  if (!d->grid && !cus) {
    const hipError_t e = device_cus(&cus);
    if (e != hipSuccess) return (int)e;
  }
  const uint32_t grid = d->grid ? d->grid : gemm_grid(l, d->num_tiles, cus);
  if (grid < 1) return -1;
  Bufs b;
  GemmArgs g = {};
  g.rows = (const f4*)b.up(rows, (size_t)rows_bytes);
  g.queries = (const f4*)b.up(fp32 ? queries : nullptr, (size_t)queries_len * sizeof(float));
  g.qb16 = b.up(fp32 ? nullptr : qb16, (size_t)qb16_len * 2);
  g.qb_pitch16 = d->qb_pitch16;
  g.n_rows = d->n_rows;
  g.pitch4 = d->pitch4;
  g.num_tiles = d->num_tiles;
  g.tile_stride = d->tile_stride;
  g.live = d->live;
  g.cn = (const float*)b.up(l2 ? cn : nullptr, (size_t)cn_len * sizeof(float));
  if (d->groupb) {
    g.gmax = (const float*)b.up(gmax, (size_t)gmax_len * sizeof(float));
    g.qn = (const float*)b.up(qn, (size_t)qn_len * sizeof(float));
    g.eps = d->eps;
    g.gam = d->gam;
    g.floor_abs = d->floor_abs;
    g.under_abs = d->under_abs;
  }
  if (d->phase == 0) {
    g.halfmax = (u64*)b.up(halfmax, (size_t)halfmax_len * sizeof(u64));
  } else {
    g.tau = (const float*)b.up(tau, (size_t)tau_len * sizeof(float));
    g.cand = (u64*)b.up(cand, (size_t)cand_len * sizeof(u64));
    g.count = (uint32_t*)b.up(count, (size_t)count_len * sizeof(uint32_t));
    g.cap = d->cap;
  }
  if (b.err != hipSuccess) return finish(b);
  if ((b.err = gemm_prepare(l)) != hipSuccess) return finish(b);
  if ((b.err = enqueue_gemm(nullptr, l, g, grid)) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  if (d->phase == 0) {
    b.down(halfmax, g.halfmax, (size_t)halfmax_len * sizeof(u64));
  } else {
    b.down(cand, g.cand, (size_t)cand_len * sizeof(u64));
    b.down(count, g.count, (size_t)count_len * sizeof(uint32_t));
  }
  return finish(b);
}

// rows_to_bf16_kernel over rows [r0, n).  rows: [rows_len] >= n * pitch floats; out: [out_len] >= n * pitch16 bf16 (+ guard);
// grid 0: the library's rule.
int gemm_rows_to_bf16(const float* rows, uint64_t rows_len, uint64_t r0, uint64_t n, uint32_t pitch, uint16_t* out, uint64_t out_len,
                      uint32_t pitch16, uint32_t grid) {
  if (!rows || !out || r0 > n || n >= (1ull << 32) || pitch < 1 || pitch16 < 8 || pitch16 % 8 != 0 || pitch > pitch16 || grid > 4096) return -1;
  if (rows_len < n * pitch || out_len < n * pitch16) return -1;
  Bufs b;
  const float* d_rows = (const float*)b.up(rows, (size_t)rows_len * sizeof(float));
  __bf16* d_out = (__bf16*)b.up(out, (size_t)out_len * 2);
  if (b.err != hipSuccess) return finish(b);
  const u64 pieces = (n - r0) * (pitch16 / 8);
  if (!grid) grid = (uint32_t)std::max<u64>(1, std::min<u64>((pieces + 255) / 256, 1u << 20));
  hipLaunchKernelGGL(rows_to_bf16_kernel, dim3(grid), dim3(256), 0, nullptr, d_rows, (u64)r0, (u64)n, pitch, d_out, pitch16);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, d_out, (size_t)out_len * 2);
  return finish(b);
}

// queries_to_bf16_kernel.  q: [q_len] >= nv * pitch floats; out: [out_len] >= blocks * gbn * kpad bf16 (+ guard); grid 0: the
// library's rule (one thread per element).
int gemm_queries_to_bf16(const float* q, uint64_t q_len, uint32_t pitch, uint32_t nv, uint16_t* out, uint64_t out_len, uint32_t kpad,
                         uint32_t gbn, uint32_t live, uint32_t blocks, uint32_t grid) {
  if (!q || !out || pitch < 1 || kpad < 1 || gbn < 1 || live < 1 || blocks < 1 || grid > 4096) return -1;
  const uint64_t total = (uint64_t)blocks * gbn * kpad;
  if (total >= (1ull << 31) || out_len < total || q_len < (uint64_t)nv * pitch) return -1;
  Bufs b;
  const float* d_q = (const float*)b.up(q, (size_t)q_len * sizeof(float));
  __bf16* d_out = (__bf16*)b.up(out, (size_t)out_len * 2);
  if (b.err != hipSuccess) return finish(b);
  if (!grid) grid = (uint32_t)((total + 255) / 256);
  hipLaunchKernelGGL(queries_to_bf16_kernel, dim3(grid), dim3(256), 0, nullptr, d_q, pitch, nv, d_out, kpad, gbn, live, blocks);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out, d_out, (size_t)out_len * 2);
  return finish(b);
}

// cn_stats_kernel over cn[0 .. n); stats: [stats_len >= 3] words the caller zeroed; grid 0: the library's rule.
int gemm_cn_stats(const float* cn, uint64_t cn_len, uint64_t n, uint32_t* stats, uint64_t stats_len, uint32_t grid) {
  if (!cn || !stats || n < 1 || cn_len < n || stats_len < 3 || grid > 4096) return -1;
  Bufs b;
  const float* d_cn = (const float*)b.up(cn, (size_t)cn_len * sizeof(float));
  uint32_t* d_stats = (uint32_t*)b.up(stats, (size_t)stats_len * sizeof(uint32_t));
  if (b.err != hipSuccess) return finish(b);
  if (!grid) grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(cn_stats_kernel, dim3(grid), dim3(256), 0, nullptr, d_cn, (u64)n, d_stats);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(stats, d_stats, (size_t)stats_len * sizeof(uint32_t));
  return finish(b);
}

// group_max_kernel.  gmax: [gmax_len] >= ceil(n / 64) (+ guard); grid 0: the library's rule.
int gemm_group_max(const float* cn, uint64_t cn_len, uint64_t n, float* gmax, uint64_t gmax_len, uint32_t grid) {
  if (!cn || !gmax || n < 1 || cn_len < n || gmax_len < (n + 63) / 64 || grid > 4096) return -1;
  Bufs b;
  const float* d_cn = (const float*)b.up(cn, (size_t)cn_len * sizeof(float));
  float* d_gmax = (float*)b.up(gmax, (size_t)gmax_len * sizeof(float));
  if (b.err != hipSuccess) return finish(b);
  if (!grid) grid = (uint32_t)std::min<uint64_t>(((n + 63) / 64 + 255) / 256, 4096);
  hipLaunchKernelGGL(group_max_kernel, dim3(grid), dim3(256), 0, nullptr, d_cn, (u64)n, d_gmax);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(gmax, d_gmax, (size_t)gmax_len * sizeof(float));
  return finish(b);
}

// query_norm_kernel, gbn workgroups of one wave.  queries: [q_len] >= nv * pitch; qn: [qn_len] >= gbn (+ guard).
int gemm_query_norm(const float* queries, uint64_t q_len, uint32_t pitch, int nv, int gbn, float* qn, uint64_t qn_len) {
  if (!queries || !qn || pitch < 1 || nv < 0 || gbn < 1 || gbn > 4096 || nv > gbn || q_len < (uint64_t)nv * pitch || qn_len < (uint64_t)gbn) return -1;
  Bufs b;
  const float* d_q = (const float*)b.up(queries, (size_t)q_len * sizeof(float));
  float* d_qn = (float*)b.up(qn, (size_t)qn_len * sizeof(float));
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(query_norm_kernel, dim3(gbn), dim3(64), 0, nullptr, d_q, pitch, nv, gbn, d_qn);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(qn, d_qn, (size_t)qn_len * sizeof(float));
  return finish(b);
}

// tau_margin_kernel, nv workgroups of one wave.  tau: [tau_len] >= nv (+ guard); queries: [q_len] >= nv * pitch.
int gemm_tau_margin(float* tau, uint64_t tau_len, const float* queries, uint64_t q_len, uint32_t pitch, int nv, uint32_t cn_max_bits, int metric,
                    int bf16, float floor_abs, float under_abs) {
  if (!tau || !queries || pitch < 1 || nv < 1 || nv > 4096 || tau_len < (uint64_t)nv || q_len < (uint64_t)nv * pitch) return -1;
  if (metric != WDBX_METRIC_COSINE && metric != WDBX_METRIC_L2) return -1;
  Bufs b;
  float* d_tau = (float*)b.up(tau, (size_t)tau_len * sizeof(float));
  const float* d_q = (const float*)b.up(queries, (size_t)q_len * sizeof(float));
  const uint32_t* d_bits = (const uint32_t*)b.up(&cn_max_bits, sizeof(uint32_t));
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(tau_margin_kernel, dim3(nv), dim3(64), 0, nullptr, d_tau, d_q, pitch, nv, d_bits, metric, bf16, floor_abs, under_abs);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(tau, d_tau, (size_t)tau_len * sizeof(float));
  return finish(b);
}

}  // extern "C"
