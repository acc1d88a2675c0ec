// kernels_multivector.h -- the reduction and ranking of wdbx_index_search_multivector (late interaction / MaxSim): label_keys_kernel
// (kernels_labels.h) has scored a round of vectors and left one key per (vector, item); multivector_rank_kernel takes, per
// segment of the round (host_multivector.h: the vectors of one query inside the round), each label's best key of every vector,
// folds their scores in fp32 in the caller's vector order and ranks the labels by that sum.  Plain stores, one writer per key and
// per accumulator entry: no atomics, no memset, answers bit-identical from run to run.
// Part of the single translation unit wdbx_hip.hip (included there, in order); not a standalone header.

struct MultivectorRankArgs {
  const u64* keys;                  // [round's vectors][key_stride] item keys of the round
  uint64_t key_stride;
  const uint32_t* label_item0;      // [n_labels + 1] first item of each label
  uint32_t n_labels;
  const MultivectorSegment* segs;   // the segments grid y walks (blockIdx.y = index in here)
  float* acc;                       // [n_labels] the fold of the one query that is cut by a round boundary; NaN = dead label
  u64* out;                         // lists: [ranked segments][k][P] as the fp32 scan's partial lists; keys: [ranked segments][n_labels]
  int k;
};

// MODE 0: a sorted list of k keys per wave in LDS, 1: in registers (k <= 128), 2: no list, every label's key goes to
// out[slot][label] (ranked by the radix-select chain).  Grid: x = workgroups along the labels (a lane per label, 64 labels per
// wave and trip, as label_rank_kernel), y = segments.  A lane starts from the accumulator (carry_in) or +0.0f and, vector by
// vector in the segment's order, takes the maximum over its label's consecutive items of that vector's key column -- lanes read
// neighbouring items, 8 bytes per item and vector; four vectors' columns are in flight at a time, the fold stays in order -- and
// adds its score; a zero maximum (no eligible row for that vector) makes the sum NaN for good.  A carry_out segment stores the
// sum and ends (the whole workgroup: the flag is uniform over the grid row).  Any other forms make_key(sum, label position), 0
// for a NaN sum, and ranks as label_rank_kernel does.  The host never puts a segment that reads acc and another one that writes
// it in one launch.
template <int MODE>
__global__ __launch_bounds__(256) void multivector_rank_kernel(MultivectorRankArgs a) {
  constexpr bool REG = MODE == 1;
  constexpr int VU = 4;
  extern __shared__ u64 lds_lists[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const MultivectorSegment seg = a.segs[blockIdx.y];
  const bool carry_in = seg.carry & MV_CARRY_IN, carry_out = seg.carry & MV_CARRY_OUT;
  TopList<REG> top;
  u64 thr = 0;
  if constexpr (MODE != 2) top.init(lds_lists + (size_t)wave * a.k, a.k, lane);
  for (uint32_t l0 = (blockIdx.x * 4 + wave) * 64; l0 < a.n_labels; l0 += gridDim.x * 256) {
    const uint32_t l = l0 + (uint32_t)lane;
    u64 key = 0;
    if (l < a.n_labels) {
      const uint32_t i0 = a.label_item0[l], i1 = a.label_item0[l + 1];
      float sum = carry_in ? a.acc[l] : 0.0f;
      for (uint32_t v = seg.v0; v < seg.v1; v += VU) {
        u64 best[VU];
#pragma unroll
        for (int u = 0; u < VU; ++u) best[u] = 0;
        for (uint32_t i = i0; i < i1; ++i) {
#pragma unroll
          for (int u = 0; u < VU; ++u)  // (past the segment's end: its last vector again, dropped below)
            best[u] = max(best[u], a.keys[(size_t)min(v + (uint32_t)u, seg.v1 - 1) * a.key_stride + i]);
        }
#pragma unroll
        for (int u = 0; u < VU; ++u)
          if (v + (uint32_t)u < seg.v1) sum = best[u] ? sum + key_score(best[u]) : __builtin_nanf("");
      }
      if (carry_out)
        a.acc[l] = sum;
      else
        key = sum == sum ? make_key(sum, l) : 0ull;  // a NaN sum is never a result
    }
    if (carry_out) continue;
    if constexpr (MODE == 2) {
      if (l < a.n_labels) a.out[(size_t)seg.slot * a.n_labels + l] = key;
    } else {
      thr = top.offer(key, key > thr, thr, lane);
    }
  }
  if (carry_out) return;
  if constexpr (MODE != 2) {
    if constexpr (REG) top.store(lds_lists + (size_t)wave * a.k, 1, lane);
    __syncthreads();
    if (wave == 0) {
      const u64* other = lds_lists + (size_t)lane * a.k;  // (lanes 1 .. 3: the other waves' lists)
      walk_lists<REG>([&](int ptr) { return other[ptr]; }, lane >= 1 && lane < 4, a.k, top, thr, lane);
      top.store(a.out + (size_t)seg.slot * a.k * gridDim.x + blockIdx.x, gridDim.x, lane);
    }
  }
}

typedef void (*multivector_rank_fn)(MultivectorRankArgs);

static multivector_rank_fn pick_multivector_rank(int mode) {
  return mode == 0 ? multivector_rank_kernel<0> : mode == 1 ? multivector_rank_kernel<1> : multivector_rank_kernel<2>;
}
