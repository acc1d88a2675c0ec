// Stand-alone driver of wdbx-py_amd/csrc/host_calls.h for tests/test_host_calls.py (plain g++, no HIP).  Every mode reads
// its cases from standard input as whitespace-separated unsigned integers (floats travel as their bit patterns, signed
// values with an offset the mode names) and prints one line per result.
//   calls_harness mask     cases "n_rows n_words w ..."                          -> "allowed"
//   calls_harness pad      cases "dim pitch nq n_src n_index i ... bits ..."     -> the nq * pitch destination words (bits)
//   calls_harness rank     cases "cnt k l2 key ..."                              -> "row bits" per slot, row + 1 printed
//   calls_harness classes  one case "nq dim k fail_class+1 fail_code n_classes c+1 ... class_of+1 ... query bits ..."
//                          -> "call c+1 n q bits ..." per callback, "rc r", then "out idx+7 bits ..." per query
// The buffers handed to the header are heap allocations of exactly the size the call may touch: the sanitized build of the
// test sees every read or write past them.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_calls.h"

static bool next(uint64_t* v) { return scanf("%" SCNu64, v) == 1; }
static uint64_t must() {
  uint64_t v = 0;
  if (!next(&v)) exit(2);
  return v;
}
static float as_float(uint64_t bits) {
  const uint32_t u = (uint32_t)bits;
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}
static uint32_t as_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}

static int run_mask() {
  uint64_t n_rows;
  while (next(&n_rows)) {
    std::vector<uint32_t> words((size_t)must());
    for (uint32_t& w : words) w = (uint32_t)must();
    printf("%" PRIu64 "\n", mask_allowed_rows(words.data(), n_rows));
  }
  return 0;
}

static int run_pad() {
  uint64_t dim;
  while (next(&dim)) {
    const size_t pitch = (size_t)must(), nq = (size_t)must(), n_src = (size_t)must();
    std::vector<int32_t> index((size_t)must());
    for (int32_t& i : index) i = (int32_t)must();
    std::vector<float> src(n_src * dim);
    for (float& f : src) f = as_float(must());
    std::vector<float> dst(nq * pitch);
    memset(dst.data(), 0xFF, dst.size() * sizeof(float));  // (whatever the padding held before)
    pad_queries(dst.data(), pitch, src.data(), (size_t)dim, nq, index.empty() ? nullptr : index.data());
    for (const float f : dst) printf("%u ", as_bits(f));
    printf("\n");
  }
  return 0;
}

static int run_rank() {
  uint64_t cnt;
  while (next(&cnt)) {
    const int k = (int)must();
    const bool l2 = must() != 0;
    std::vector<uint64_t> keys((size_t)cnt);
    for (uint64_t& key : keys) key = must();
    std::vector<int64_t> idx((size_t)k, 99);
    std::vector<float> score((size_t)k, 99.0f);
    rank_keys_host(keys.data(), keys.size(), k, l2, idx.data(), score.data());
    for (int i = 0; i < k; ++i) printf("%lld %u ", (long long)idx[(size_t)i] + 1, as_bits(score[(size_t)i]));
    printf("\n");
  }
  return 0;
}

static int run_classes() {
  const int nq = (int)must(), dim = (int)must(), k = (int)must();
  const int32_t fail_class = (int32_t)must() - 1;
  const int fail_code = (int)must();
  std::vector<int32_t> classes((size_t)must());
  for (int32_t& c : classes) c = (int32_t)must() - 1;
  std::vector<int32_t> class_of((size_t)nq);
  for (int32_t& c : class_of) c = (int32_t)must() - 1;
  std::vector<float> queries((size_t)nq * dim);
  for (float& f : queries) f = as_float(must());
  std::vector<int64_t> out_idx((size_t)nq * k, -7);
  std::vector<float> out_score((size_t)nq * k, -7.0f);
  // the callback answers member i, slot j with idx = 1000 * (first value of its query) + 10 * (class + 1) + j and
  // score = (second value of its query) + j + class / 2
  const int rc = for_each_class(nq, dim, k, queries.data(), class_of.data(), classes, out_idx.data(), out_score.data(),
                                [&](int32_t c, int n, const float* q, int64_t* idx, float* score) {
                                  printf("call %d %d", (int)c + 1, n);
                                  for (int i = 0; i < n * dim; ++i) printf(" %u", as_bits(q[i]));
                                  printf("\n");
                                  if (c == fail_class) return fail_code;
                                  for (int i = 0; i < n; ++i)
                                    for (int j = 0; j < k; ++j) {
                                      idx[i * k + j] = (int64_t)(1000.0f * q[i * dim]) + 10 * (c + 1) + j;
                                      score[i * k + j] = q[i * dim + 1] + (float)j + 0.5f * (float)c;
                                    }
                                  return 0;
                                });
  printf("rc %d\n", rc);
  for (int q = 0; q < nq; ++q) {
    printf("out");
    for (int j = 0; j < k; ++j) printf(" %lld %u", (long long)out_idx[(size_t)q * k + j] + 7, as_bits(out_score[(size_t)q * k + j]));
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string mode = argv[1];
  if (mode == "mask") return run_mask();
  if (mode == "pad") return run_pad();
  if (mode == "rank") return run_rank();
  if (mode == "classes") return run_classes();
  return 2;
}
