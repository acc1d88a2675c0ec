// groups_harness.hip -- test-only launcher of group_members_kernel and group_merge_kernel ALONE (tests/groups_harness.py,
// tests/test_gpu_groups_kernels.py).
//
// Built from the very headers libwdbx_hip.so is built from, in wdbx_hip.hip's order: kernels_common.h, kernels_aux.h
// (exact_finish next to accum), host_subset.h (row_block_ni), host_groups.h, kernels_rowblock.h (the members kernel's frame:
// exact_score_block, the key rule, the mask bit) and kernels_groups.h.  The instances come
// from pick_group_members / pick_group_merge.  This file defines no kernel of its own.  The entry points take HOST pointers
// with their lengths: copy in, launch on the null stream, synchronise, copy out; they return the HIP error code, or -1 when the
// arguments would make a kernel read or write outside the uploaded arrays (checked here, before anything is launched).  Output
// arrays are copied IN as well, with `guard` extra words in front of and behind them on the device, so a word a kernel leaves
// alone -- the guards included -- comes back as the caller put it.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "wdbx_hip.h"

typedef unsigned long long u64;
typedef float f4 __attribute__((ext_vector_type(4)));

#include "kernels_common.h"
#include "kernels_aux.h"
#include "host_subset.h"
#include "host_groups.h"
#include "kernels_rowblock.h"
#include "kernels_groups.h"
static_assert(GROUPS_MAX_SIZE_DEV == GROUPS_MAX_SIZE && GROUPS_MAX_SIZE == WDBX_MAX_GROUP_SIZE, "a wave's register list holds a group");
static_assert(sizeof(GroupTaskDev) == sizeof(GroupTask) && sizeof(GroupTask) == 16, "the device reads the host's tasks");

namespace {

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

}  // namespace

extern "C" {

// group_members_kernel<metric, NI(pitch4)> over n_tasks tasks ([n_tasks][4] words: query, start, count, direct).
// rows: [n_rows, pitch4] quads; queries: [nq, pitch4] quads; order: [n_order] row numbers; mask: null or n_mask_words words.
// partial: [guard + n_tasks * g + guard] u64s; the kernel's array starts at partial + guard.
int groups_members(int metric, const float* rows, uint32_t n_rows, uint32_t pitch4, const float* queries, uint32_t nq,
                   const uint32_t* order, uint32_t n_order, const uint32_t* mask, uint64_t n_mask_words, const uint32_t* tasks,
                   uint32_t n_tasks, int g, u64* partial, uint64_t guard) {
  if (!rows || !queries || !order || !tasks || !partial || n_rows < 1 || pitch4 < 1 || nq < 1 || n_order < 1 || n_tasks < 1) return -1;
  if (g < 1 || g > WDBX_MAX_GROUP_SIZE) return -1;
  if (mask && n_mask_words < ((uint64_t)n_rows + 31) / 32) return -1;
  for (uint32_t i = 0; i < n_order; ++i)
    if (order[i] >= n_rows) return -1;
  for (uint32_t t = 0; t < n_tasks; ++t) {
    const uint32_t* w = tasks + (size_t)t * 4;
    if (w[0] >= nq || w[2] < 1 || w[3] > 1) return -1;
    if (w[3] ? (w[1] >= n_rows || w[2] != 1) : (w[1] >= n_order || w[2] > n_order - w[1])) return -1;
  }
  Bufs b;
  GroupMembersArgs a = {};
  a.rows = (const f4*)b.up(rows, (size_t)n_rows * pitch4 * sizeof(f4));
  a.queries = (const f4*)b.up(queries, (size_t)nq * pitch4 * sizeof(f4));
  a.order = (const uint32_t*)b.up(order, (size_t)n_order * sizeof(uint32_t));
  a.mask = (const uint32_t*)b.up(mask, (size_t)n_mask_words * sizeof(uint32_t));
  a.tasks = (const GroupTaskDev*)b.up(tasks, (size_t)n_tasks * sizeof(GroupTaskDev));
  const size_t n_out = (size_t)n_tasks * g;
  u64* d_out = (u64*)b.up(partial, (n_out + 2 * guard) * sizeof(u64));
  a.partial = d_out ? d_out + guard : nullptr;
  a.pitch4 = pitch4;
  a.g = g;
  if (b.err != hipSuccess) return finish(b);
  hipLaunchKernelGGL(pick_group_members(metric, pitch4), dim3(n_tasks), dim3(256), 0, nullptr, a);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(partial, d_out, (n_out + 2 * guard) * sizeof(u64));
  return finish(b);
}

// group_merge_kernel<metric> over n_slots slots.  partial: [n_lists][g] sorted keys; slot_task0: [n_slots + 1], non-decreasing,
// slot_task0[0] >= task_base, the last entry - task_base <= n_lists.  out_idx / out_score: [guard + n_slots * g + guard];
// out_count: [guard + n_slots + guard].
int groups_merge(int metric, const u64* partial, uint64_t n_lists, const u64* slot_task0, uint64_t task_base, uint32_t n_slots, int g,
                 int64_t* out_idx, float* out_score, int32_t* out_count, uint64_t guard) {
  if (!partial || !slot_task0 || !out_idx || !out_score || !out_count || n_slots < 1 || g < 1 || g > WDBX_MAX_GROUP_SIZE) return -1;
  if (slot_task0[0] < task_base) return -1;
  for (uint32_t s = 0; s < n_slots; ++s)
    if (slot_task0[s + 1] < slot_task0[s]) return -1;
  if (slot_task0[n_slots] - task_base > n_lists) return -1;
  Bufs b;
  GroupMergeArgs m = {};
  m.partial = (const u64*)b.up(partial, std::max<size_t>((size_t)n_lists, 1) * g * sizeof(u64));
  m.slot_task0 = (const u64*)b.up(slot_task0, ((size_t)n_slots + 1) * sizeof(u64));
  const size_t n_out = (size_t)n_slots * g;
  int64_t* d_idx = (int64_t*)b.up(out_idx, (n_out + 2 * guard) * sizeof(int64_t));
  float* d_score = (float*)b.up(out_score, (n_out + 2 * guard) * sizeof(float));
  int32_t* d_count = (int32_t*)b.up(out_count, ((size_t)n_slots + 2 * guard) * sizeof(int32_t));
  if (b.err != hipSuccess) return finish(b);
  m.task_base = task_base;
  m.n_slots = n_slots;
  m.g = g;
  m.out_idx = d_idx + guard;
  m.out_score = d_score + guard;
  m.out_count = d_count + guard;
  hipLaunchKernelGGL(pick_group_merge(metric), dim3((n_slots + 3) / 4), dim3(256), 0, nullptr, m);
  if ((b.err = hipGetLastError()) != hipSuccess) return finish(b);
  if ((b.err = hipDeviceSynchronize()) != hipSuccess) return finish(b);
  b.down(out_idx, d_idx, (n_out + 2 * guard) * sizeof(int64_t));
  b.down(out_score, d_score, (n_out + 2 * guard) * sizeof(float));
  b.down(out_count, d_count, ((size_t)n_slots + 2 * guard) * sizeof(int32_t));
  return finish(b);
}

}  // extern "C"
