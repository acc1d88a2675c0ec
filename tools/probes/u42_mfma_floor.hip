// Probe: what one launch of scan_u42_mfma_kernel costs when (almost) nothing survives -- the pass's own floor of loads, MFMAs
// and compares -- and, with a finite threshold, at a chosen share of survivors and candidates.
// Random plane bytes, s = 1 and a4 = `a4` for every row, random l records with a6 = 0, 16 random unit queries, every threshold
// = `tau` (default +inf: no row survives, only the h plane and {s, a4} are read).  With random h the four-bit estimate w4 of a
// unit query is about normal with mean -0.5 sum q and deviation 18.4, so tau = 61.7 and a4 = 17.3 let about 0.8 % of the (row,
// query) pairs survive and 0.04 % become candidates, the shares of the headline corpus (profiles/u42_mfma/README.md).
// The kernels are the library's own: this file includes the headers wdbx_hip.hip includes and owns no device code.
// Prints one JSON line: ms per launch (mean and minimum of `launches` timed one by one with an event pair), survivors and
// candidates per query of one launch.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I wdbx-py_amd/csrc tools/probes/u42_mfma_floor.hip -o tools/probes/bin/u42_mfma_floor
//   usage: u42_mfma_floor [rows = 10000000] [workgroups per CU = 2] [tau = inf] [a4 = 0] [launches = 20]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "wdbx_hip.h"

typedef unsigned long long u64;
typedef float f4 __attribute__((ext_vector_type(4)));

#include "kernels_common.h"
#include "kernels_merge_select.h"
#include "kernels_scan8.h"
#include "kernels_scan6.h"
#include "kernels_scan42.h"

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); \
      return 1;                                                                    \
    }                                                                              \
  } while (0)

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static inline u64 rng() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

int main(int argc, char** argv) {
  const uint32_t n_rows = argc > 1 ? (uint32_t)atol(argv[1]) : 10000000u;
  const uint32_t wgs = argc > 2 ? (uint32_t)atoi(argv[2]) : 2u;
  const float tau = argc > 3 ? (float)atof(argv[3]) : INFINITY;
  const float a4 = argc > 4 ? (float)atof(argv[4]) : 0.f;
  const int launches = argc > 5 ? atoi(argv[5]) : 20;
  const uint32_t units = U42_MFMA_MAX_UNITS, nq = U42_MFMA_QUERIES, cap = 65536, qpitch = units * 32;
  if (n_rows < 1 || n_rows > (1u << 24) || wgs < 1 || wgs > 8 || launches < 1 || launches > 1000) {
    fprintf(stderr, "arguments out of range\n");
    return 2;
  }
  const scan42_mfma_fn fn = pick_scan42_mfma(units);
  if (!fn) return 2;
  const uint32_t tiles64 = (n_rows + 63) / 64, lpitch = u42_lpitch(units);
  const size_t h_dwords = (size_t)tiles64 * units * 256, l_dwords = (size_t)n_rows * lpitch;

  std::vector<u64> h(h_dwords / 2);
  for (auto& v : h) v = rng();
  std::vector<f2v> sa(n_rows, f2v{1.0f, a4});
  std::vector<uint32_t> l(l_dwords);
  for (size_t r = 0; r < n_rows; ++r) {
    uint32_t* rec = l.data() + r * lpitch;
    for (uint32_t i = 0; i < units * 2; ++i) rec[i] = (uint32_t)rng();
    for (uint32_t i = units * 2; i < lpitch; ++i) rec[i] = 0u;  // (a6 = 0)
  }
  std::vector<float> q((size_t)nq * qpitch), taus(nq, tau);
  for (uint32_t j = 0; j < nq; ++j) {
    double ss = 0;
    float* v = q.data() + (size_t)j * qpitch;
    for (uint32_t i = 0; i < qpitch; ++i) {
      v[i] = (float)((double)(rng() >> 11) * 0x1p-53 - 0.5);
      ss += (double)v[i] * v[i];
    }
    for (uint32_t i = 0; i < qpitch; ++i) v[i] = (float)(v[i] / sqrt(ss));
  }

  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  Scan42MfmaArgs m = {};
  Scan42Args& a = m.a;
  void *d_h, *d_sa, *d_l, *d_q, *d_tau, *d_cand, *d_count, *d_surv, *d_qb, *d_qc;
  CK(hipMalloc(&d_h, h_dwords * 4));
  CK(hipMalloc(&d_sa, (size_t)n_rows * sizeof(f2v)));
  CK(hipMalloc(&d_l, l_dwords * 4));
  CK(hipMalloc(&d_q, q.size() * 4));
  CK(hipMalloc(&d_tau, nq * 4));
  CK(hipMalloc(&d_cand, (size_t)nq * cap * sizeof(u64)));
  CK(hipMalloc(&d_count, nq * 4));
  CK(hipMalloc(&d_surv, nq * 4));
  CK(hipMalloc(&d_qb, (size_t)u42_mfma_group_dwords(units) * 4));
  CK(hipMalloc(&d_qc, nq * sizeof(U42QConst)));
  CK(hipMemcpy(d_h, h.data(), h_dwords * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_sa, sa.data(), (size_t)n_rows * sizeof(f2v), hipMemcpyHostToDevice));
  CK(hipMemcpy(d_l, l.data(), l_dwords * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_q, q.data(), q.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_tau, taus.data(), nq * 4, hipMemcpyHostToDevice));
  a.hcodes = (const uint32_t*)d_h;
  a.sa4 = (const f2v*)d_sa;
  a.lrec = (const uint32_t*)d_l;
  a.query = (const float*)d_q;
  a.n_rows = n_rows;
  a.units = units;
  a.qpitch = qpitch;
  a.lpitch = lpitch;
  a.tau = (const float*)d_tau;
  a.cand = (u64*)d_cand;
  a.count = (uint32_t*)d_count;
  a.survivors = (uint32_t*)d_surv;
  a.cap = cap;
  m.qb = (const uint32_t*)d_qb;
  m.qc = (const U42QConst*)d_qc;
  m.nq = nq;
  m.surv_p = nullptr;
  hipLaunchKernelGGL(u42_query_i16_kernel, dim3(nq), dim3(64), 0, nullptr, a.query, qpitch, units, nq, (uint32_t*)d_qb, (U42QConst*)d_qc);
  CK(hipGetLastError());
  const uint32_t grid = scan_full_grid(tiles64, (uint32_t)prop.multiProcessorCount, wgs);
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  double sum = 0, best = 1e30;
  std::vector<uint32_t> count(nq), surv(nq);
  for (int it = -3; it < launches; ++it) {  // (three launches to warm up)
    CK(hipMemset(d_count, 0, nq * 4));
    CK(hipMemset(d_surv, 0, nq * 4));
    CK(hipEventRecord(e0, nullptr));
    hipLaunchKernelGGL(fn, dim3(grid, 1), dim3(256), 0, nullptr, m);
    CK(hipGetLastError());
    CK(hipEventRecord(e1, nullptr));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (it >= 0) sum += ms, best = std::min(best, (double)ms);
  }
  CK(hipMemcpy(count.data(), d_count, nq * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(surv.data(), d_surv, nq * 4, hipMemcpyDeviceToHost));
  double cs = 0, ss = 0;
  for (uint32_t j = 0; j < nq; ++j) cs += count[j], ss += surv[j];
  const double bytes = (double)h_dwords * 4 + (double)n_rows * 8;
  printf("{\"probe\": \"u42_mfma_floor\", \"rows\": %u, \"units\": %u, \"wgs_per_cu\": %u, \"grid\": %u, \"tau\": %g, \"a4\": %g, "
         "\"launches\": %d, \"ms_mean\": %.4f, \"ms_min\": %.4f, \"plane_bytes\": %.0f, \"plane_TBps_at_mean\": %.3f, "
         "\"survivors_per_query\": %.1f, \"candidates_per_query\": %.1f}\n",
         n_rows, units, wgs, grid, (double)tau, (double)a4, launches, sum / launches, best, bytes, bytes / (sum / launches * 1e-3) / 1e12,
         ss / nq, cs / nq);
  return 0;
}
