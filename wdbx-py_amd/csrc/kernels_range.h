// kernels_range.h -- exact range search: every row whose fp32 score reaches a per-query threshold.
// Part of the single translation unit wdbx_hip.hip (included there, in order); not a standalone header.
//
// The output of a range query is not bounded by any k, so nothing here keeps a list: rows (or candidates) that pass are
// appended to a per-query key buffer, staged per wave (WaveStage, kernels_common.h: one atomicAdd per 64 keys; the filter,
// whose wave holds up to 64 candidates at once, with wave_append), and the counter keeps counting past the buffer, so the
// host learns the exact size and grows it.  Every score that decides or is returned comes from
// exact_score (kernels_aux.h), rescore_kernel's arithmetic, so the answer does not depend on which path selected the rows.
//   fp32 path   range_scan_kernel: every row scored exactly, survivors appended.
//   u8 path     scan8_kernel<PHASE 2> (kernels_scan8.h) keeps every row whose quantisation upper bound reaches the threshold,
//               range_filter_kernel scores those exactly and compacts the survivors.
// A pass: cosine / inner product score >= thr[q]; L2 squared distance <= thr[q]; a NaN score never passes.

struct RangeArgs {
  const f4* rows;        // [n_rows, pitch4] quads
  const f4* queries;     // [nq, pitch4]
  const float* thr;      // [nq] the caller's thresholds (distances for L2)
  const uint32_t* mask;  // optional row filter, bit r = row r may be returned
  uint32_t n_rows, pitch4;
  u64* out;              // [nq][cap] keys (score, row) as make_key
  uint32_t* count;       // [nq] exact number of passing rows
  uint32_t cap;
  // range_filter_kernel: the candidates of the selection scan
  const u64* cand;
  const uint32_t* cand_count;
  uint32_t cand_cap;
};

template <int METRIC>
__device__ __forceinline__ bool range_pass(float s, float thr) {
  if constexpr (METRIC == WDBX_METRIC_L2)
    return s == s && -s <= thr;  // (s = -distance exactly)
  else
    return s == s && s >= thr;
}

// one query per blockIdx.y; P lanes per row (64 / P rows per wave pass), U passes scored at once (with NI > 0 the loads of
// all of them are in flight together).  grid.x workgroups stride over the row groups.
template <int METRIC, int P, int NI>
__global__ __launch_bounds__(256) void range_scan_kernel(RangeArgs a) {
  constexpr int R = 64 / P;
  constexpr int U = NI == 0 ? 1 : NI >= 3 ? 2 : 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t j = (uint32_t)(lane % P), g = (uint32_t)(lane / P);
  const uint32_t q = blockIdx.y;
  const f4* qp = a.queries + (size_t)q * a.pitch4;
  const float thr = a.thr[q];
  u64* out = a.out + (size_t)q * a.cap;
  uint32_t* count = a.count + q;
  const uint32_t last_row = a.n_rows - 1;
  const uint32_t groups = (a.n_rows + R - 1) / R;
  const uint32_t W = gridDim.x * 4;
  __shared__ u64 stage[4][128];
  WaveStage st = {stage[wave], 0u};
  for (uint32_t cur = blockIdx.x * 4 + wave; cur < groups; cur += U * W) {
    float s[U];
    uint32_t row[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t grp = cur + (uint32_t)u * W;
      row[u] = grp < groups ? grp * R + g : 0xFFFFFFFFu;
      const uint32_t rc = min(row[u], last_row);
      s[u] = exact_score<METRIC, P, NI, true>(a.rows + (size_t)rc * a.pitch4, qp, a.pitch4, j);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool keep = j == 0 && row[u] <= last_row && range_pass<METRIC>(s[u], thr) &&
                        (!a.mask || ((a.mask[row[u] >> 5] >> (row[u] & 31)) & 1u));
      st.push(keep, make_key(s[u] + 0.0f, row[u] <= last_row ? row[u] : 0u), out, count, a.cap, lane);
    }
  }
  st.finish(out, count, a.cap, lane);
}

// the selection scan's candidates of query blockIdx.y: exact scores (one wave per candidate, rescore_kernel's layout), the
// passing ones compacted into out.  A wave takes a run of C consecutive candidates, C = the candidates per wave of the grid
// (1 .. 64): few candidates spread over all waves (latency), many go 64 to a wave (one append per 64).
template <int METRIC>
__global__ __launch_bounds__(256) void range_filter_kernel(RangeArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t q = blockIdx.y;
  const uint32_t have = min(a.cand_count[q], a.cand_cap);
  const uint32_t waves = gridDim.x * 4;
  const uint32_t C = max(1u, min(64u, (have + waves - 1) / waves));
  const u64* cand = a.cand + (size_t)q * a.cand_cap;
  const f4* qp = a.queries + (size_t)q * a.pitch4;
  const float thr = a.thr[q];
  u64* out = a.out + (size_t)q * a.cap;
  for (uint32_t c0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * C; c0 < have; c0 += waves * C) {
    const uint32_t nloc = min(C, have - c0);
    bool keep = false;
    u64 key = 0;
    for (uint32_t i = 0; i < nloc; ++i) {
      const uint32_t row = key_row(cand[c0 + i]);
      const float s = exact_score<METRIC>(a.rows + (size_t)row * a.pitch4, qp, a.pitch4, (uint32_t)lane);
      if ((uint32_t)lane == i) {
        keep = range_pass<METRIC>(s, thr);
        key = make_key(s + 0.0f, row);
      }
    }
    wave_append(keep, key, out, a.count + q, a.cap, lane);
  }
}

// the instance of a form (host_scan_plan.h: range_scan_form): host-side picker, shared by the range search (wdbx_hip.hip) and
// the tests' launcher (tests/kernel_harness/scan_harness.hip).  null: the form names no instance
typedef void (*range_fn)(RangeArgs);
template <int METRIC>
static range_fn pick_range_scan_form(int P, int NI) {
  if (P == 64) {
    switch (NI) {
      case 0: return range_scan_kernel<METRIC, 64, 0>;
      case 1: return range_scan_kernel<METRIC, 64, 1>;
      case 2: return range_scan_kernel<METRIC, 64, 2>;
      case 3: return range_scan_kernel<METRIC, 64, 3>;
      case 4: return range_scan_kernel<METRIC, 64, 4>;
      default: return nullptr;
    }
  }
  if (NI != 1) return nullptr;
  switch (P) {
    case 1: return range_scan_kernel<METRIC, 1, 1>;
    case 2: return range_scan_kernel<METRIC, 2, 1>;
    case 4: return range_scan_kernel<METRIC, 4, 1>;
    case 8: return range_scan_kernel<METRIC, 8, 1>;
    case 16: return range_scan_kernel<METRIC, 16, 1>;
    case 32: return range_scan_kernel<METRIC, 32, 1>;
    default: return nullptr;
  }
}

template <int METRIC>
static range_fn pick_range_scan(uint32_t pitch4) {
  const RangeForm f = range_scan_form(pitch4);
  return pick_range_scan_form<METRIC>(f.P, f.NI);
}
