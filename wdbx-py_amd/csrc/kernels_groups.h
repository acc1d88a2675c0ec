// kernels_groups.h -- stage 2 of wdbx_index_search_groups (the best group_size rows of each chosen label): group_members_kernel
// walks one task -- a segment of a label's run in the label order (host_labels.h), or one direct row -- and writes the sorted
// best keys of its rows; group_merge_kernel merges the sorted lists of each (query, slot) and writes rows, scores and the count.
// Plain stores, one writer per key and per output word: no atomics, answers bit-identical from run to run.
// Part of the single translation unit wdbx_hip.hip (included there, in order); not a standalone header.

constexpr int GROUPS_MAX_SIZE_DEV = 64;  // (= GROUPS_MAX_SIZE, host_groups.h; checked where both are visible)

struct GroupTaskDev {  // (= GroupTask, host_groups.h)
  uint32_t query, start, count, direct;
};

struct GroupMembersArgs {
  const f4* rows;             // [n_rows, pitch4] quads
  const f4* queries;          // [nq, pitch4] the call's queries
  const uint32_t* order;      // [n] row of each position of the label order (not read by direct tasks; may be null without any run)
  const uint32_t* mask;       // optional row filter: bit r set = row r may be returned
  const GroupTaskDev* tasks;  // the round's tasks, one per workgroup
  u64* partial;               // [tasks][g] sorted keys of each task, zeros behind the members
  uint32_t pitch4;
  int g;                      // group size, 1 .. 64
};

// Grid: x = the round's tasks.  Wave w of the workgroup takes positions w, w + 4, ... of the task, U rows' loads in flight (as
// label_keys_kernel).  A row's score is exact_score_block's (kernels_rowblock.h): rescore_kernel's arithmetic bit for bit, wave-
// uniform, so is its key; a masked-out row (tested on the wave-uniform row, before the scoring) and a NaN score give no key.
// Each wave keeps its g best keys in registers (one per lane); wave 0 merges the four lists as subset_kernel does.
template <int METRIC, int NI>
__global__ __launch_bounds__(256) void group_members_kernel(GroupMembersArgs a) {
  constexpr int U = row_block_u(NI), NR = row_block_nr(NI);
  __shared__ u64 lists[4 * GROUPS_MAX_SIZE_DEV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t j = (uint32_t)lane;
  const GroupTaskDev t = a.tasks[blockIdx.x];
  const f4* qp[1];
  f4 q[1][NR];
  qp[0] = a.queries + (size_t)t.query * a.pitch4;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    q[0][i] = f4{0.f, 0.f, 0.f, 0.f};
    if (NI > 0 && j + (uint32_t)i * 64 < a.pitch4) q[0][i] = qp[0][j + (uint32_t)i * 64];
  }
  TopList<true> top;
  top.init(nullptr, a.g, lane);
  u64 thr = 0;
  for (uint32_t cur = (uint32_t)wave; cur < t.count; cur += U * 4) {
    f4 c[U][NR];
    uint32_t row[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t pos = min(cur + (uint32_t)u * 4, t.count - 1);  // (past the task's end: its last position again, dropped below)
      row[u] = t.direct ? t.start : a.order[t.start + pos];
      const f4* cp = a.rows + (size_t)row[u] * a.pitch4;
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        c[u][i] = f4{0.f, 0.f, 0.f, 0.f};
        if (NI > 0 && j + (uint32_t)i * 64 < a.pitch4) c[u][i] = ld16<true>(cp + j + (uint32_t)i * 64);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (cur + (uint32_t)u * 4 >= t.count) break;  // (wave-uniform)
      if (!row_allowed(a.mask, row[u])) continue;  // (wave-uniform)
      float s[1];
      exact_score_block<METRIC, 1, NI>(c[u], a.rows + (size_t)row[u] * a.pitch4, q, qp, a.pitch4, j, s);
      const u64 key = readlane64(row_key(s[0], row[u]), 0);
      if (key > thr) thr = top.insert(key, lane);
    }
  }
  top.store(lists + wave * GROUPS_MAX_SIZE_DEV, 1, lane);
  __syncthreads();
  if (wave == 0) {
    const u64* other = lists + lane * GROUPS_MAX_SIZE_DEV;  // (lanes 1 .. 3: the other waves' lists)
    walk_lists<true>([&](int ptr) { return other[ptr]; }, lane >= 1 && lane < 4, a.g, top, thr, lane);
    top.store(a.partial + (size_t)blockIdx.x * a.g, 1, lane);
  }
}

typedef void (*group_members_fn)(GroupMembersArgs);

static group_members_fn pick_group_members(int metric, uint32_t pitch4) {
  return with_row_block_ni(pitch4, [&](auto ni) -> group_members_fn {
    constexpr int NI = decltype(ni)::value;
    return metric == WDBX_METRIC_L2 ? group_members_kernel<WDBX_METRIC_L2, NI> : group_members_kernel<WDBX_METRIC_COSINE, NI>;
  });
}

struct GroupMergeArgs {
  const u64* partial;         // [tasks][g] the round's sorted lists
  const u64* slot_task0;      // the round's slots: slot s owns the call's tasks [slot_task0[s], slot_task0[s + 1])
  uint64_t task_base;         // the call's task number of the round's first list
  uint32_t n_slots;           // slots of the round
  int g;
  int64_t* out_idx;           // [n_slots][g]
  float* out_score;           // [n_slots][g]
  int32_t* out_count;         // [n_slots]
};

// Grid: x = workgroups of four waves, a wave per (query, slot).  The slot's lists are walked 64 at a time (a lane per list)
// into one register list; a key becomes (row, score in the caller's units) exactly as merge_kernel converts it.  Every member
// slot and the count are written: a slot without tasks or without any eligible row gets -1 / 0 and count 0.
template <int METRIC>
__global__ __launch_bounds__(256) void group_merge_kernel(GroupMergeArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t s = blockIdx.x * 4 + (uint32_t)wave;
  if (s >= a.n_slots) return;  // (wave-uniform; no barrier in this kernel)
  const u64 t0 = a.slot_task0[s] - a.task_base, t1 = a.slot_task0[s + 1] - a.task_base;
  TopList<true> top;
  top.init(nullptr, a.g, lane);
  u64 thr = 0;
  for (u64 base = t0; base < t1; base += 64) {
    const bool owns = base + (u64)lane < t1;
    const u64* mine = a.partial + (size_t)(owns ? base + (u64)lane : t0) * a.g;
    thr = walk_lists<true>([&](int ptr) { return mine[ptr]; }, owns, a.g, top, thr, lane);
  }
  const u64 key = top.reg;
  const bool member = lane < a.g && key != 0;
  if (lane < a.g) {
    float sc = key_score(key);
    if (METRIC == WDBX_METRIC_L2) sc = -sc + 0.0f;
    a.out_idx[(size_t)s * a.g + lane] = member ? (int64_t)key_row(key) : -1;
    a.out_score[(size_t)s * a.g + lane] = member ? sc : 0.0f;
  }
  const int count = __popcll(__ballot(member));
  if (lane == 0) a.out_count[s] = count;
}

typedef void (*group_merge_fn)(GroupMergeArgs);

static group_merge_fn pick_group_merge(int metric) {
  return metric == WDBX_METRIC_L2 ? group_merge_kernel<WDBX_METRIC_L2> : group_merge_kernel<WDBX_METRIC_COSINE>;
}
