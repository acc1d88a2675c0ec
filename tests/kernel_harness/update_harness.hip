// update_harness.hip -- test-only launcher of the kernels behind wdbx_index_set_rows_at / wdbx_index_remove_rows
// (tests/update_harness.py, tests/test_gpu_update_kernels.py): the scatter, the fused refresh and the int8 group-list form of
// kernels_update.h next to the range quantisers they share their per-row functions with.
//
// Built from the very headers libwdbx_hip.so is built from; the plan of a list-form run is host_update.h's update_plan, the
// grids are the helpers' next to the kernels.  This file defines no kernel of its own.  The one entry point takes HOST
// pointers: copy in, launch on the null stream, synchronise, copy out; it returns the HIP error code, or -1 when the arguments
// would make a kernel read or write outside the uploaded arrays (checked here, before anything is launched).  Every array is
// copied IN as well as out, with the byte length the caller states (room for guard cells behind it included), so a cell no
// kernel touches comes back with whatever the caller put there.
//
//   mode 0  the list form: update_scatter_kernel (rounds of `round_rows` rows), update_refresh_kernel, rows_to_i8g_list_kernel
//   mode 1  what wdbx_index_set_rows does once per listed row: the row copied to its place (pads zero), normalize_rows_kernel
//           over that row when asked, then every range quantiser over [r, r + 1) where r lies below the copy's coverage and
//           rows_to_i8g_kernel over the row's group
//   mode 2  no write of rows: every range quantiser over [0, coverage) of the rows as given

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "wdbx_hip.h"

typedef unsigned long long u64;
typedef float f4 __attribute__((ext_vector_type(4)));

#include "host_update.h"
#include "kernels_common.h"
#include "kernels_merge_select.h"
#include "kernels_tiles.h"
#include "kernels_scan8.h"
#include "kernels_scan6.h"
#include "kernels_scan42.h"
#include "kernels_tiles8.h"
#include "kernels_aux.h"
#include "kernels_update.h"

namespace {

struct Bufs {
  void* p[24];
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

// One run.  n_rows stored rows of `pitch` floats; cov_*: rows [0, cov) each copy covers (0: the copy is absent and its
// arrays may be null).  *_bytes: what the caller allocated for each array.  Copies' layouts are the library's: u6 / u42 in
// 64-row tiles, the int8 rows in fragment order.
struct UpdCase {
  uint32_t dim, pitch, pitch16, pitch8, pitch8g, normalize;
  uint64_t n_rows, round_rows;  // round_rows: rows per scatter round of mode 0 (0: update_plan's)
  uint64_t cov_cn, cov_16, cov_8, cov_6, cov_42, cov_g;
  uint64_t rows_bytes, cn_bytes, r16_bytes, r8_bytes, s8_bytes, c6_bytes, sa6_bytes, h42_bytes, sa42_bytes, l42_bytes, r8g_bytes,
      grp_bytes, gbad_bytes;
};

// list: n strictly increasing rows below n_rows; src: [n, dim] or null (the rows become NaN tombstones).  launches_out (may be
// null): mode 0's launch count as update_plan states it.
int upd_run(int mode, const UpdCase* c, const uint32_t* list, uint64_t n, const float* src, float* rows, float* cn, uint16_t* r16,
            uint8_t* r8, float* s8, uint32_t* c6, float* sa6, uint32_t* h42, float* sa42, uint32_t* l42, int8_t* r8g, float* grp,
            u64* gbad, int* launches_out) {
  if (!c || !rows || mode < 0 || mode > 2 || c->dim < 1 || c->dim > c->pitch || c->pitch % 4 != 0 || c->n_rows < 1) return -1;
  if (n && !list) return -1;
  for (uint64_t i = 0; i < n; ++i)
    if (list[i] >= c->n_rows || (i && list[i] <= list[i - 1])) return -1;
  const uint64_t N = c->n_rows, tiles = (N + 63) / 64;
  const uint32_t units6 = c->pitch / 16, units42 = c->pitch / 32, lpitch = u42_lpitch(units42);
  if (std::max({c->cov_cn, c->cov_16, c->cov_8, c->cov_6, c->cov_42, c->cov_g}) > N) return -1;
  if (c->rows_bytes < N * c->pitch * sizeof(float)) return -1;
  if (c->cov_cn && (!cn || c->cn_bytes < N * sizeof(float))) return -1;
  if (c->cov_16 && (!r16 || c->pitch16 < c->pitch || c->pitch16 % 8 != 0 || c->r16_bytes < N * c->pitch16 * 2)) return -1;
  if (c->cov_8 && (!r8 || !s8 || c->pitch8 < 1 || c->r8_bytes < N * c->pitch8 || c->s8_bytes < N * sizeof(float))) return -1;
  if (c->cov_6 && (!c6 || !sa6 || c->pitch % 16 != 0 || c->c6_bytes < tiles * units6 * 768 || c->sa6_bytes < N * 8)) return -1;
  if (c->cov_42 && (!h42 || !sa42 || !l42 || c->pitch % 32 != 0 || c->h42_bytes < tiles * units42 * 1024 || c->sa42_bytes < N * 8 ||
                    c->l42_bytes < N * lpitch * 4))
    return -1;
  // (the group kernels write whole groups up to the end of the last listed row's group: zero rows past n_rows)
  if (c->cov_g && (!r8g || !grp || !gbad || c->pitch8g < c->dim || c->pitch8g % 64 != 0 || c->r8g_bytes < tiles * 64 * c->pitch8g ||
                   c->grp_bytes < tiles * 16 || c->gbad_bytes < tiles * 8))
    return -1;
  Bufs b;
  float* d_rows = (float*)b.up(rows, c->rows_bytes);
  float* d_cn = c->cov_cn ? (float*)b.up(cn, c->cn_bytes) : nullptr;
  __bf16* d_r16 = c->cov_16 ? (__bf16*)b.up(r16, c->r16_bytes) : nullptr;
  uint8_t* d_r8 = c->cov_8 ? (uint8_t*)b.up(r8, c->r8_bytes) : nullptr;
  float* d_s8 = c->cov_8 ? (float*)b.up(s8, c->s8_bytes) : nullptr;
  uint32_t* d_c6 = c->cov_6 ? (uint32_t*)b.up(c6, c->c6_bytes) : nullptr;
  f2v* d_sa6 = c->cov_6 ? (f2v*)b.up(sa6, c->sa6_bytes) : nullptr;
  uint32_t* d_h42 = c->cov_42 ? (uint32_t*)b.up(h42, c->h42_bytes) : nullptr;
  f2v* d_sa42 = c->cov_42 ? (f2v*)b.up(sa42, c->sa42_bytes) : nullptr;
  uint32_t* d_l42 = c->cov_42 ? (uint32_t*)b.up(l42, c->l42_bytes) : nullptr;
  int8_t* d_r8g = c->cov_g ? (int8_t*)b.up(r8g, c->r8g_bytes) : nullptr;
  f4* d_grp = c->cov_g ? (f4*)b.up(grp, c->grp_bytes) : nullptr;
  u64* d_gbad = c->cov_g ? (u64*)b.up(gbad, c->gbad_bytes) : nullptr;
  if (b.err != hipSuccess) return finish(b);

  // the range quantisers over [r0, r1) clipped to each copy's coverage (modes 1 and 2)
  auto range_forms = [&](u64 r0, u64 r1) -> hipError_t {
    if (r0 < c->cov_cn) {
      const u64 e = std::min<u64>(r1, c->cov_cn);
      hipLaunchKernelGGL(row_sqnorm_kernel, dim3(std::max(1u, row_sqnorm_grid(e - r0))), dim3(256), 0, nullptr, (const float*)d_rows, r0, e,
                         c->pitch, d_cn, (uint32_t*)nullptr);
    }
    if (r0 < c->cov_16) {
      const u64 e = std::min<u64>(r1, c->cov_16), pieces = (e - r0) * (c->pitch16 / 8);
      hipLaunchKernelGGL(rows_to_bf16_kernel, dim3((uint32_t)std::min<u64>((pieces + 255) / 256, 1u << 20)), dim3(256), 0, nullptr,
                         (const float*)d_rows, r0, e, c->pitch, d_r16, c->pitch16);
    }
    if (r0 < c->cov_g) {
      const u64 e = std::min<u64>(r1, c->cov_g), g0 = r0 / 64, g1 = (e + 63) / 64;
      hipLaunchKernelGGL(rows_to_i8g_kernel, dim3(rows_to_i8g_grid(g1 - g0)), dim3(256), 0, nullptr, (const float*)d_rows, g0, g1, (u64)N,
                         c->dim, c->pitch, d_r8g, c->pitch8g, d_grp, d_gbad);
    }
    if (r0 < c->cov_8) {
      const u64 e = std::min<u64>(r1, c->cov_8);
      hipLaunchKernelGGL(rows_to_u8_kernel, dim3(rows_to_u8_grid(e - r0)), dim3(256), 0, nullptr, (const float*)d_rows, r0, e, c->dim,
                         c->pitch, d_r8, c->pitch8, d_s8);
    }
    if (r0 < c->cov_6) {
      const u64 e = std::min<u64>(r1, c->cov_6);
      hipLaunchKernelGGL(rows_to_u6_kernel, dim3(rows_to_u6_grid(e - r0)), dim3(256), 0, nullptr, (const float*)d_rows, r0, e, c->dim,
                         c->pitch, units6, d_c6, d_sa6);
    }
    if (r0 < c->cov_42) {
      const u64 e = std::min<u64>(r1, c->cov_42);
      hipLaunchKernelGGL(rows_to_u42_kernel, dim3(rows_to_u42_grid(e - r0)), dim3(256), 0, nullptr, (const float*)d_rows, r0, e, c->dim,
                         c->pitch, units42, d_h42, d_sa42, d_l42, lpitch);
    }
    return hipGetLastError();
  };

  if (mode == 0 && n) {
    UpdateCoverage cov;
    cov.cn = c->cov_cn, cov.bf16 = c->cov_16, cov.i8g = c->cov_g, cov.u8 = c->cov_8, cov.u6 = c->cov_6, cov.u42 = c->cov_42;
    UpdatePlan p = update_plan(list, n, c->dim, cov, src != nullptr);
    if (c->round_rows && src) {
      p.round_rows = c->round_rows;
      p.rounds = (n + p.round_rows - 1) / p.round_rows;
      p.launches = (int)p.rounds + (p.n_refresh ? 1 : 0) + (p.groups.empty() ? 0 : 1);
    }
    if (launches_out) *launches_out = p.launches;
    std::vector<uint32_t> both(list, list + n);
    both.insert(both.end(), p.groups.begin(), p.groups.end());
    const uint32_t* d_list = (const uint32_t*)b.up(both.data(), both.size() * sizeof(uint32_t));
    float* d_src = src ? (float*)b.up(src, (size_t)n * c->dim * sizeof(float)) : nullptr;
    if (b.err != hipSuccess) return finish(b);
    for (uint64_t round = 0; round < p.rounds; ++round) {
      const uint64_t i0 = update_round_first(p, round), cnt = update_round_count(p, round);
      hipLaunchKernelGGL(update_scatter_kernel, dim3(update_rows_grid(cnt)), dim3(256), 0, nullptr,
                         d_src ? (const float*)(d_src + (size_t)i0 * c->dim) : (const float*)nullptr, d_list, (u64)i0, (u64)cnt, c->dim, c->pitch,
                         d_rows, (int)c->normalize);
    }
    if (p.n_refresh) {
      UpdateArgs a = {};
      a.rows = d_rows, a.list = d_list, a.dim = c->dim, a.pitch = c->pitch;
      a.n_cn = p.n_cn, a.n_16 = p.n_16, a.n_8 = p.n_8, a.n_6 = p.n_6, a.n_42 = p.n_42;
      a.cn = d_cn, a.rows16 = d_r16, a.pitch16 = c->pitch16, a.rows8 = d_r8, a.pitch8 = c->pitch8, a.scale8 = d_s8;
      a.units6 = units6, a.codes6 = d_c6, a.sa6 = d_sa6;
      a.units42 = units42, a.lpitch42 = lpitch, a.h42 = d_h42, a.sa42 = d_sa42, a.lrec42 = d_l42;
      hipLaunchKernelGGL(update_refresh_kernel, dim3(update_rows_grid(p.n_refresh)), dim3(256), 0, nullptr, a);
    }
    if (!p.groups.empty())
      hipLaunchKernelGGL(rows_to_i8g_list_kernel, dim3(rows_to_i8g_list_grid(p.groups.size())), dim3(256), 0, nullptr, (const float*)d_rows,
                         d_list + n, (u64)p.groups.size(), (u64)N, c->dim, c->pitch, d_r8g, c->pitch8g, d_grp, d_gbad);
    b.err = hipGetLastError();
  } else if (mode == 1) {
    std::vector<float> padded(c->pitch);
    for (uint64_t i = 0; i < n && b.err == hipSuccess; ++i) {
      const u64 r = list[i];
      for (uint32_t e = 0; e < c->pitch; ++e) padded[e] = e < c->dim ? (src ? src[i * c->dim + e] : NAN) : 0.f;
      b.err = hipMemcpy(d_rows + r * c->pitch, padded.data(), c->pitch * sizeof(float), hipMemcpyHostToDevice);
      if (b.err != hipSuccess) break;
      if (c->normalize) hipLaunchKernelGGL(normalize_rows_kernel, dim3(1), dim3(256), 0, nullptr, d_rows + r * c->pitch, (u64)1, c->pitch);
      b.err = range_forms(r, r + 1);
    }
  } else if (mode == 2) {
    b.err = range_forms(0, N);
  }
  if (b.err != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(rows, d_rows, c->rows_bytes);
  b.down(cn, d_cn, c->cn_bytes);
  b.down(r16, d_r16, c->r16_bytes);
  b.down(r8, d_r8, c->r8_bytes);
  b.down(s8, d_s8, c->s8_bytes);
  b.down(c6, d_c6, c->c6_bytes);
  b.down(sa6, d_sa6, c->sa6_bytes);
  b.down(h42, d_h42, c->h42_bytes);
  b.down(sa42, d_sa42, c->sa42_bytes);
  b.down(l42, d_l42, c->l42_bytes);
  b.down(r8g, d_r8g, c->r8g_bytes);
  b.down(grp, d_grp, c->grp_bytes);
  b.down(gbad, d_gbad, c->gbad_bytes);
  return finish(b);
}

}  // extern "C"
