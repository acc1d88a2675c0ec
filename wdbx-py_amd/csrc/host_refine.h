// host_refine.h -- the device-free launch shape of the second selection stage (refine_pairs_kernel, kernels_tiles8.h): which
// instance, how many waves, how many candidates per query the dynamic LDS holds and how many bytes of it the launch asks for.
// Included by kernels_tiles8.h (refine_launch_for / enqueue_refine behind the kernel: what host_index.h and the tests' kernel
// harness tests/kernel_harness/stage_harness.hip both launch through) and, on its own, by tests/host_harness/refine_harness.cpp
// (plain g++ in the CPU suite, tests/test_refine_launch_host.py).  No HIP, no kernel types in here.
//
// The rule.  The kernel's dynamic LDS serves one of two layouts per query:
//   n <= n_lds   one upper bound (4 bytes) per candidate; the lower bounds stay in registers, REFINE_R per thread
//   n >  n_lds   one TopList of k keys (8 bytes each) per wave plus the final list: (waves + 1) * k keys
// and the launch asks for the larger of the two.  Both stay within REFINE_LDS_BUDGET = 128 KiB, the budget of the merge
// kernels (merge_waves_for, kernels_merge_select.h), so that the kernel's static LDS fits under the 160 KiB of a CU as well:
// the workgroup runs 16 waves while 17 lists of k keys fit the budget (k <= 963) and fewer from there on, down to 7 waves at
// k = 2048 -- the kernel takes its wave count from blockDim.x in both layouts (the threshold search, the list walk and the
// compaction loop all stride by it), so a smaller workgroup is the same computation in more trips.  n_lds shrinks with the
// workgroup (REFINE_R entries per thread), so a query of more than REFINE_R * threads candidates takes the wave lists.
// A request above 64 KiB (k >= 482) needs the function's dynamic LDS limit raised first: RefineShape::raise.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

constexpr int REFINE_R = 8;                            // lower bounds a thread keeps in registers (n <= n_lds)
constexpr int REFINE_MAX_WAVES = 16;                   // __launch_bounds__(1024); s_wcnt of the compaction
constexpr size_t REFINE_LDS_BUDGET = 128 * 1024;       // = the merge kernels'
constexpr size_t REFINE_LDS_DEFAULT_LIMIT = 64 * 1024; // what a function may ask for without raising its limit

struct RefineShape {
  bool reg;        // the waves' lists in registers (k <= 128 unless option lds_lists) -- the REG instance
  int waves;       // of 64 threads
  uint32_t n_lds;  // RefineArgs::n_lds
  size_t lds;      // dynamic LDS bytes of the launch
  bool raise;      // lds is above the default limit: hipFuncAttributeMaxDynamicSharedMemorySize first
};

// waves whose k-key lists, plus the final one, fit the budget: merge_waves_for's rule
static inline int refine_waves_for(int k) {
  const int nw = (int)(REFINE_LDS_BUDGET / ((size_t)std::max(k, 1) * sizeof(uint64_t))) - 1;
  return std::max(1, std::min(REFINE_MAX_WAVES, nw));
}

// k in 1 .. WDBX_MAX_K (2048); cap = candidates a query's buffer holds
static inline RefineShape refine_shape(int k, uint32_t cap, bool lds_lists) {
  RefineShape s;
  s.reg = k <= 128 && !lds_lists;
  s.waves = refine_waves_for(k);
  s.n_lds = std::min<uint32_t>(cap, (uint32_t)REFINE_R * 64u * (uint32_t)s.waves);
  s.lds = std::max((size_t)s.n_lds * 4, (size_t)(s.waves + 1) * (size_t)k * sizeof(uint64_t));
  s.raise = s.lds > REFINE_LDS_DEFAULT_LIMIT;
  return s;
}
