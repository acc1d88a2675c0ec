// host_calls.h -- the device-free plumbing the blocking entry points share: the allowed rows of a host mask, the padded copy
// of a call's queries, the host ranking of a lone query's keys, and the class-by-class fallback of the calls that carry one
// mask or one row list per query.
// Included by wdbx_hip.hip and, on its own, by tests/host_harness/calls_harness.cpp (plain g++ in the CPU suite,
// tests/test_host_calls.py).  No HIP, no kernel types in here.  Keys are decoded by range_key_row / range_key_score
// (host_range.h).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>

#include "host_range.h"

// how many of n_rows rows a mask allows (uint32 words, bit r % 32 of word r / 32 = row r; ceil(n_rows / 32) words are read):
// bits past the last row do not count
static inline uint64_t mask_allowed_rows(const uint32_t* mask_words, uint64_t n_rows) {
  const size_t words = (size_t)((n_rows + 31) / 32);
  if (!words) return 0;
  uint64_t allowed = 0;
  for (size_t w = 0; w + 1 < words; ++w) allowed += (uint64_t)__builtin_popcount(mask_words[w]);
  const uint32_t tail = (uint32_t)(n_rows & 31);
  return allowed + (uint64_t)__builtin_popcount(mask_words[words - 1] & (tail ? (1u << tail) - 1u : ~0u));
}

// nq queries of dim floats to dst at a pitch of `pitch` floats, the padding zeroed; with an index table, query q of dst is
// query index[q] of src (entries may repeat)
static inline void pad_queries(float* dst, size_t pitch, const float* src, size_t dim, size_t nq, const int32_t* index = nullptr) {
  if (pitch == dim && !index) {
    memcpy(dst, src, nq * dim * sizeof(float));
    return;
  }
  if (pitch != dim) memset(dst, 0, nq * pitch * sizeof(float));
  for (size_t q = 0; q < nq; ++q) memcpy(dst + q * pitch, src + (index ? (size_t)index[q] : q) * dim, dim * sizeof(float));
}

// cnt unsorted keys -> the k best in key order = (score descending, row ascending), decoded; a zero key (a NaN score) is
// never a result; L2 keys hold negated distances; the slots behind the last result are -1 / 0.0
static inline void rank_keys_host(const uint64_t* keys_in, size_t cnt, int k, bool l2, int64_t* out_idx, float* out_score) {
  std::vector<uint64_t> keys(keys_in, keys_in + cnt);
  const size_t kk = std::min<size_t>((size_t)k, cnt);
  if (kk < cnt) std::nth_element(keys.begin(), keys.begin() + kk, keys.end(), std::greater<uint64_t>());  // O(n) ...
  std::sort(keys.begin(), keys.begin() + kk, std::greater<uint64_t>());                                   // ... + k log k
  size_t o = 0;
  for (; o < kk && keys[o]; ++o) {
    const float s = range_key_score(keys[o]);
    out_idx[o] = range_key_row(keys[o]);
    out_score[o] = l2 ? -s + 0.0f : s;
  }
  for (; o < (size_t)k; ++o) {
    out_idx[o] = -1;
    out_score[o] = 0.0f;
  }
}

// A call answered class by class through an older call: for every entry c of classes, in that order, the queries q with
// class_of[q] == c are gathered in the caller's order, call(c, n_members, q, idx, score) answers them into [n_members, k]
// arrays, and the answers go back to the members' rows of out_idx / out_score.  A class without members is skipped; the
// first non-zero status of call ends the loop and is returned.
template <class Call>
static inline int for_each_class(int nq, int dim, int k, const float* queries, const int32_t* class_of, const std::vector<int32_t>& classes,
                                 int64_t* out_idx, float* out_score, Call&& call) {
  std::vector<float> cq, cs;
  std::vector<int64_t> ci;
  std::vector<int32_t> members;
  for (const int32_t c : classes) {
    members.clear();
    for (int q = 0; q < nq; ++q)
      if (class_of[q] == c) members.push_back(q);
    if (members.empty()) continue;
    const size_t nm = members.size();
    cq.resize(nm * (size_t)dim);
    ci.resize(nm * (size_t)k);
    cs.resize(nm * (size_t)k);
    pad_queries(cq.data(), (size_t)dim, queries, (size_t)dim, nm, members.data());
    const int rc = call(c, (int)nm, (const float*)cq.data(), ci.data(), cs.data());
    if (rc) return rc;
    for (size_t i = 0; i < nm; ++i) {
      memcpy(out_idx + (size_t)members[i] * k, &ci[i * k], (size_t)k * sizeof(int64_t));
      memcpy(out_score + (size_t)members[i] * k, &cs[i * k], (size_t)k * sizeof(float));
    }
  }
  return 0;
}
