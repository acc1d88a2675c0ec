// host_range.h -- the device-free host side of wdbx_index_range_search: CSR offsets from the per-query counts, the per-query
// sort of the downloaded keys and their decoding, and the L2 selection threshold.  Included by wdbx_hip.hip and, on its own,
// by tests/host_harness/range_harness.cpp (plain g++ in the CPU suite, tests/test_range_search.py).
// No HIP, no kernel types in here.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>

// counts[0 .. n) -> offsets[1 .. n] given offsets[0] (the running total before these queries: the library fills the offsets
// round by round); returns offsets[n]
static inline uint64_t range_csr_offsets(const uint64_t* counts, int n, uint64_t* offsets) {
  for (int i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + counts[i];
  return offsets[n];
}

// the score of a key as make_key (kernels_common.h) encoded it: (orderable float bits << 32) | ~row
static inline float range_key_score(uint64_t key) {
  const uint32_t ord = (uint32_t)(key >> 32);
  const uint32_t u = (ord & 0x80000000u) ? (ord ^ 0x80000000u) : ~ord;
  float s;
  memcpy(&s, &u, sizeof s);
  return s;
}
static inline int64_t range_key_row(uint64_t key) { return (int64_t)(uint32_t)~(uint32_t)(key & 0xFFFFFFFFull); }

// Every query's keys sit unsorted at [offsets[q], offsets[q + 1]) of rows_keys (the caller's row array, int64 = a u64 slot
// each): sorted descending = (score descending, row ascending) -- for L2 the keys hold negated distances, so (distance
// ascending, row ascending) -- then decoded in place into rows, and scores (L2: the positive squared distance).
static inline void range_sort_decode(int metric_l2, int nq, const uint64_t* offsets, int64_t* rows_keys, float* scores) {
  uint64_t* keys = reinterpret_cast<uint64_t*>(rows_keys);
  for (int q = 0; q < nq; ++q) std::sort(keys + offsets[q], keys + offsets[q + 1], std::greater<uint64_t>());
  const uint64_t total = offsets[nq];
  for (uint64_t i = 0; i < total; ++i) {
    const uint64_t key = keys[i];
    float s = range_key_score(key);
    if (metric_l2) s = -s + 0.0f;
    scores[i] = s;
    rows_keys[i] = range_key_row(key);
  }
}

// L2: the selection scan keeps a row when 2 c.q - |c|^2 (plus its bound) reaches tau; a squared distance d <= t is
// |q|^2 - d >= |q|^2 - t.  The exact pass computes d in fp32 with a relative error below 2e-6 up to 4096 dimensions, so a row
// it finds at d_fp32 <= t has a real d <= t (1 + 2e-6): tau = |q|^2 - t - 1e-5 |t|, rounded down to a float.  qq = |q|^2 in
// double.  +inf threshold: everything; -inf: nothing but the rows whose bound is NaN (the exact pass drops them).
static inline float range_selection_tau_l2(double qq, float t) {
  if (std::isinf(t)) return t > 0 ? -INFINITY : INFINITY;
  const double tau = qq - (double)t - 1e-5 * std::fabs((double)t);
  float f = (float)tau;
  if ((double)f > tau) f = std::nextafter(f, -INFINITY);
  return f;
}
