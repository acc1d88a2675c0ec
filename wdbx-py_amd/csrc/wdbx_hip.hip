// wdbx_hip.hip -- MI355X (gfx950, CDNA4) implementation of the WDBX vector_search hot path.
//
// What the reference does on this path (paths under /root/reference):
//   FaissIndex.search   wdbx/core/indexing.py:983-1030  exact inner product of one unit query against
//                                                        every stored unit row, k best descending
//   FaissIndex.add      indexing.py:858-905, :921-968    rows normalised (:851-856) and appended
//   VectorStore.search  wdbx/core/vector_store.py:323-345 per-shard top-`limit`, concatenate, sort, cut
// Here: the corpus lives row-major fp32 in HBM (plus optional reduced-precision shadow copies used only to
// select candidates); every query makes one streaming pass; a small kernel merges partial lists or ranks the
// exactly re-scored candidates; across GPUs the per-shard lists are all-gathered with RCCL and merged again.
//
// One translation unit, in parts (included below in this order):
//   kernels_common.h        64-bit ordering keys, per-wave top-k list, lane-group reductions
//   kernels_scan.h          scan_kernel<L,QPL,METRIC,NT,MODE,RAGGED>, scan_kernel_generic: the fp32 scan of one
//                           query (HBM-bound, 16-byte non-temporal loads straight into VGPRs, query in VGPRs, DPP
//                           tree, per-wave threshold top-k; MODE 2: key per row for the radix select)
//   kernels_merge_select.h  merge_kernel<REG> (P lists -> 1; also thresholds and candidate top-k), radix select
//   kernels_tiles.h         batched queries on the matrix cores: gemm_topk_kernel (exact fp32 MFMA tiles),
//                           gemm_bf16w8_kernel (bf16 SELECTION tiles over the fp32 rows or the bf16 shadow copy),
//                           their epilogue (sampled maxima / candidate append), rows/queries -> bf16
//   kernels_scan8.h         scan8_kernel: single-query SELECTION scan over the u8 shadow copy (default path of
//                           single queries), rows -> u8 + scales, query norms
//   kernels_aux.h           row norms, threshold margins, rescore_kernel (exact fp32 scores of the candidates),
//                           synthetic fill / normalise, read probes
//   kernels_scan6.h         scan8_u6_kernel: the same selection over the six-bit u6 shadow copy with a stored residual norm per
//                           row (rounds of single queries on large shards), its quantiser and the cut behind the re-scoring
//   kernels_scan42.h        scan_u42_kernel: that scan's full pass over the same codes split in two planes -- every row's top four
//                           bits, the low two bits only of the rows the four-bit bound cannot rule out; its quantiser
//   kernels_range.h         range search: range_scan_kernel (fp32, every row scored exactly), range_filter_kernel (exact
//                           scores of the u8 selection's candidates); wave-aggregated appends, no k
//   host_refine.h           the device-free launch shape of refine_pairs_kernel (included by kernels_tiles8.h): instance, waves,
//                           n_lds and dynamic LDS bytes within 128 KiB for every k
//   kernels_range_batch.h   range_batch_bound_kernel: the selection thresholds and the widened bound of a block of range queries in
//                           front of the int8 tiles' full pass (wdbx_index_range_search_batch)
//   host_range_batch.h      that call's route, its blocks of up to 256 queries, buffer sizes and per-query fallback bookkeeping
//   kernels_rowblock.h      the frame of the six kernels that score gathered fp32 rows against a block of queries in registers:
//                           rows in flight, exact_score_block, the key rule, the mask bit
//   kernels_subset.h        subset_kernel: exact scores of LISTED rows (wdbx_index_search_rows), a block of queries per fetched
//                           row, per-workgroup top-k lists or a key per listed row
//   kernels_matrix.h        matrix_kernel: the distance matrix among listed rows (wdbx_index_search_matrix): subset_kernel with the
//                           listed rows themselves as the queries, read where they lie, each one's own list position left out
//   host_matrix.h           that call's plan: subset_plan's route, anchor block and grid, the instance and the rounds
//   kernels_rowlists.h      rowlists_kernel: the same scores for a call with one row list PER QUERY (wdbx_index_search_row_lists),
//                           one workgroup per (chunk of a list, block of its queries) work item of host_rowlists.h
//   kernels_labels.h        label_keys_kernel, label_rank_kernel: the full pass of wdbx_index_search_distinct (at most one row per
//                           label): the best key of each label run inside a span of the label order, then of each label, ranked
//   host_labels.h           the label order of a handle (rows sorted by (label, row), items, tables), the over-fetch's host walk, the
//                           full pass's rounds, grids and scratch
//   kernels_multivector.h   multivector_rank_kernel: the reduction and ranking of wdbx_index_search_multivector (late interaction): per
//                           label the sum over a query's vectors of the vector's best key score, the labels ranked by that sum
//   host_multivector.h      the rounds and segments of that call's vectors, its route, grids and scratch
//   kernels_mmr.h           mmr_pairs_kernel, mmr_select_kernel: wdbx_index_search_mmr (maximal marginal relevance) behind its pool -- the
//                           similarity square of a query's gathered candidates and the greedy selection over it
//   host_mmr.h              that call's argument checks, pools, rounds and grids
//   kernels_recommend.h     recommend_kernel: the pass of wdbx_index_search_recommend over the whole corpus -- every row scored against
//                           a query's positive and negative examples, the scores folded into one key per side
//   host_recommend.h        that call's offset and exclusion checks, plan, short queries and the splice of the two sides
//   kernels_discover.h      discover_kernel, discover_zone_kernel: wdbx_index_search_discover -- every row scored against a query's
//                           context pairs (and target), folded per pair into a loss key or a (target key, wins) record; the zones'
//                           ranking from the records
//   host_discover.h         that call's offset checks, plans of the pass and of the zone stage, staged vectors, zones and splice
//   kernels_groups.h        group_members_kernel, group_merge_kernel: stage 2 of wdbx_index_search_groups -- the best group_size rows of
//                           each chosen label, scored along the label's run of the label order, and the merge of a run's segments
//   host_groups.h           the runs of the label order, the dense label of a label value, that call's tasks, slot table and rounds
//   kernels_update.h        update_scatter_kernel, update_refresh_kernel, rows_to_i8g_list_kernel: wdbx_index_set_rows_at /
//                           wdbx_index_remove_rows -- a call's rows to their listed places (or the NaN tombstone), then every derived
//                           copy of exactly those rows through the per-row functions the range quantisers call
//   host_update.h           that call's coverage counts, distinct int8 groups, upload rounds and launch count
//   host_multimask.h        a call with one row mask per query: the placement of its queries in the int8 tiles' query blocks
//   host_selection.h        the plan of the selection rounds: sampled tiles, stride, candidate and pair capacities of the tile paths and
//                           the u8 / u6 rounds, the masked sample's growth, the 1 GiB shadow rule
//   host_calls.h            what the blocking entry points share, device-free: allowed rows of a mask, padded query copies, the host
//                           ranking of a lone query's keys, the class-by-class fallback loop
//   host_index.h            the handle, kernel choice, the enqueue functions of every search path, and what the blocking entry
//                           points share on the device side: query upload, result buffers and download, mask scope and check
//   host_group.h            the in-process shard group: per-shard host threads, exchange (RCCL all-gather / device copies), merge
// The selection paths never decide a result: they keep every row whose score could reach the true k-th best
// under a rigorous error bound, and the kept rows are re-scored in fp32 from the fp32 rows.
//
// Ordering everywhere is one total order on 64-bit keys:
//   key = (orderable(score) << 32) | ~row      (bigger key = better; 0 = empty slot)
// so "score descending, row ascending" is a single unsigned compare, ties are deterministic and a
// merged multi-shard result equals the single-shard result bit for bit.

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <functional>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "wdbx_hip.h"

typedef unsigned long long u64;
typedef float f4 __attribute__((ext_vector_type(4)));

// error plumbing (g_err, fail), the exception barrier (WDBX_CATCH), the shard dispatcher, ordered locks, grow bookkeeping and
// the option table lookup live in host_dispatch.h: the device-free slice of the host side, which the CPU suite also builds
// with plain g++ under -fsanitize=thread / address,undefined (tests/test_host_dispatch_sanitizers.py)
#include "host_dispatch.h"
#include "host_range.h"  // (device-free as well: CSR offsets, per-query sort and decoding of a range search's keys)
#include "host_range_batch.h"  // (device-free as well: route, blocks, buffer sizes and fallback bookkeeping of a batched range search)
#include "host_calls.h"  // (device-free as well: mask popcount, padded query copies, host ranking of keys, class-by-class loop)
#include "host_subset.h"  // (device-free as well: row-list validation, route and grid sizing of a search among listed rows)
#include "host_matrix.h"  // (device-free as well: route, anchor block, instance and rounds of a distance matrix among listed rows)
#include "host_multimask.h"  // (device-free as well: where the queries of a call with a mask per query sit in the tile blocks)
#include "host_selection.h"  // (device-free as well: the sample, stride and capacities of the selection rounds)
#include "host_scan_plan.h"  // (device-free as well: the fp32 scan and range forms of a pitch, grid / list / chunk / LDS numbers of a scan)
#include "host_labels.h"  // (device-free as well: label order, items, over-fetch walk, rounds and scratch of a distinct search)
#include "host_multivector.h"  // (device-free as well: rounds, segments, route and scratch of a multi-vector search)
#include "host_rowlists.h"  // (device-free as well: slots, rounds, query blocks and work items of a call with a row list per query)
#include "host_mmr.h"  // (device-free as well: argument checks, pools, rounds and grids of an MMR search)
#include "host_recommend.h"  // (device-free as well: offsets, exclusion list, plan, short queries and splice of a recommend search)
#include "host_discover.h"  // (device-free as well: pair offsets, plans, staged vectors, zones and splice of a discovery search)
#include "host_groups.h"  // (device-free as well: label runs, dense label lookup, tasks, slot table and rounds of a groups search)
#include "host_update.h"  // (device-free as well: coverage counts, distinct int8 groups, rounds and launch count of a write of listed rows)

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      (void)hipGetLastError(); /* (the runtime's "last error" is sticky: a failed allocation must not fail the next launch check) */ \
      int c_ = (e_ == hipErrorOutOfMemory) ? WDBX_E_NOMEM                                    \
               : (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? WDBX_E_NODEVICE   \
                                                                         : WDBX_E_HIP;       \
      return fail(c_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    }                                                                                        \
  } while (0)

#define NCCL_TRY(expr)                                                                        \
  do {                                                                                        \
    ncclResult_t r_ = (expr);                                                                 \
    if (r_ != ncclSuccess)                                                                    \
      return fail(WDBX_E_RCCL, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
  } while (0)

#include "kernels_common.h"
#include "kernels_scan.h"
#include "kernels_merge_select.h"
#include "kernels_tiles.h"
#include "kernels_scan8.h"
#include "kernels_scan6.h"
#include "kernels_scan42.h"
#include "kernels_tiles8.h"
#include "kernels_aux.h"
#include "kernels_range.h"
#include "kernels_range_batch.h"
#include "kernels_rowblock.h"
#include "kernels_subset.h"
#include "kernels_matrix.h"
#include "kernels_rowlists.h"
#include "kernels_labels.h"
static_assert(LABEL_SPAN_DEV == LABEL_SPAN, "the kernels walk the spans the host built");
#include "kernels_multivector.h"
static_assert(MULTIVECTOR_MAX_VECTORS == WDBX_MAX_QUERY_VECTORS, "the plan's limit is the header's");
#include "kernels_mmr.h"
static_assert(MMR_MAX_POOL == WDBX_MAX_K, "a pool is a top-k answer");
#include "kernels_recommend.h"
static_assert(RECOMMEND_MAX_EXAMPLES == WDBX_MAX_EXAMPLES && RECOMMEND_MAX_EXCLUDE == WDBX_MAX_EXCLUDE_ROWS, "the plan's limits are the header's");
#include "kernels_discover.h"
static_assert(DISCOVER_MAX_PAIRS == WDBX_MAX_CONTEXT_PAIRS && DISCOVER_ZONES == DISCOVER_ZONE_COUNT, "the plan's limits are the header's and the kernel's");
#include "kernels_groups.h"
static_assert(GROUPS_MAX_SIZE_DEV == GROUPS_MAX_SIZE && GROUPS_MAX_SIZE == WDBX_MAX_GROUP_SIZE, "a wave's register list holds a group");
static_assert(sizeof(GroupTaskDev) == sizeof(GroupTask) && sizeof(GroupTask) == 16, "the device reads the host's tasks");
#include "kernels_update.h"
#include "host_index.h"
#include "host_group.h"

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static int drain(EventPool& pool, uint64_t* count, double* ms);

// every device allocation the handle holds: the fp32 rows, each shadow copy with its tables, and the scratch buffers
static uint64_t device_bytes_resident(const wdbx_index* ix) { return ix->bufs.total_bytes(); }

extern "C" {

int wdbx_hip_version(void) { return WDBX_HIP_ABI_VERSION; }

const char* wdbx_last_error(void) { return g_err.c_str(); }

int wdbx_device_count(int* out_count) try {
  if (!out_count) return fail(WDBX_E_INVALID, "out_count is null");
  *out_count = 0;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(WDBX_E_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  *out_count = n;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_create(int device_id, int dim, int metric, uint64_t capacity_rows, wdbx_index** out) try {
  if (!out) return fail(WDBX_E_INVALID, "out is null");
  *out = nullptr;
  if (dim < 1 || dim > (1 << 20)) return fail(WDBX_E_INVALID, "dim=%d outside [1, 2^20]", dim);
  if (metric != WDBX_METRIC_COSINE && metric != WDBX_METRIC_L2) return fail(WDBX_E_INVALID, "metric=%d unknown", metric);
  int ndev = 0;
  int rc = wdbx_device_count(&ndev);
  if (rc) return rc;
  if (ndev < 1) return fail(WDBX_E_NODEVICE, "no HIP device visible: the WDBX HIP backend needs an AMD GPU");
  if (device_id < 0 || device_id >= ndev) return fail(WDBX_E_NODEVICE, "device_id=%d but %d device(s) visible", device_id, ndev);
  wdbx_index* ix = new (std::nothrow) wdbx_index();
  if (!ix) return fail(WDBX_E_NOMEM, "host allocation failed");
  ix->device = device_id;
  ix->dim = dim;
  ix->pitch = (dim + 3) / 4 * 4;
  ix->metric = metric;
  DeviceGuard g(device_id);
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, device_id);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete ix;
    return fail(WDBX_E_HIP, "device setup failed: %s", hipGetErrorString(e));
  }
  ix->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  const char* env;
  if ((env = getenv("WDBX_HIP_SCAN_LANES"))) ix->opt_lanes = atoll(env);
  if ((env = getenv("WDBX_HIP_SCAN_BLOCKS"))) ix->opt_blocks = atoll(env);
  if ((env = getenv("WDBX_HIP_SCAN_NT"))) ix->opt_nt = atoll(env);
  if ((env = getenv("WDBX_HIP_SCAN_BLOCKED"))) ix->opt_blocked = atoll(env);
  rc = reserve_locked(ix, std::max<uint64_t>(capacity_rows, 1));
  if (rc) {
    (void)hipStreamDestroy(ix->stream);
    delete ix;
    return rc;
  }
  *out = ix;
  return WDBX_OK;
} WDBX_CATCH

void wdbx_index_destroy(wdbx_index* ix) try {
  if (!ix) return;
  {
    std::unique_lock<std::mutex> lk(ix->mu);
    // (blocking searches that wait for their event outside the mutex still read their staging slot afterwards)
    ix->slots.wait_all_free(lk);
    DeviceGuard g(ix->device);
    (void)hipStreamSynchronize(ix->stream);
    if (ix->comm) (void)ncclCommDestroy(ix->comm);
    for (hipEvent_t e : ix->scan_ev.ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : ix->merge_ev.ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : ix->gemm_ev.ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : ix->sample_ev.ev) (void)hipEventDestroy(e);
    ix->bufs.release_all();
    if (ix->h_stage) (void)hipHostFree(ix->h_stage);
    for (hipEvent_t e : ix->slot_done)
      if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(ix->stream);
  }
  delete ix;
} WDBX_CATCH_VOID

int wdbx_index_dim(const wdbx_index* ix) { return ix ? ix->dim : 0; }
int wdbx_index_row_pitch(const wdbx_index* ix) { return ix ? ix->pitch : 0; }

int wdbx_index_size(wdbx_index* ix, uint64_t* out_rows) try {
  if (!ix || !out_rows) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  *out_rows = ix->n;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_capacity(wdbx_index* ix, uint64_t* out_rows) try {
  if (!ix || !out_rows) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  *out_rows = ix->cap;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_reserve(wdbx_index* ix, uint64_t capacity_rows) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  return reserve_locked(ix, capacity_rows);
} WDBX_CATCH

int wdbx_index_clear(wdbx_index* ix) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  ix->n = 0;
  ix->cn_rows = 0;
  ix->cn_stats_dirty = false;
  ix->shadow_rows = 0;
  ix->shadow8_rows = 0;
  ix->shadow6_rows = 0;
  ix->shadow42_rows = 0;
  ix->shadowg_rows = 0;
  ix->shadowg_tail_n = ~0ull;
  ix->labels.clear();  // (back to "no label was ever set")
  ix->lab_valid = false;
  return WDBX_OK;
} WDBX_CATCH

static int ensure_room(wdbx_index* ix, uint64_t extra) {
  const uint64_t need = ix->n + extra;
  if (need <= ix->cap) return WDBX_OK;
  return reserve_locked(ix, std::max(need, ix->cap + ix->cap / 2));
}

int wdbx_index_add(wdbx_index* ix, const float* rows, uint64_t n, int normalize, uint64_t* first_row_out) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (n && !rows) return fail(WDBX_E_INVALID, "rows is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  if (first_row_out) *first_row_out = ix->n;
  if (!n) return WDBX_OK;
  int rc = ensure_room(ix, n);
  if (rc) return rc;
  rc = upload_rows(ix, ix->n, rows, n, normalize);
  if (rc) return rc;
  ix->n += n;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_set_rows(wdbx_index* ix, uint64_t first_row, const float* rows, uint64_t n, int normalize) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (n && !rows) return fail(WDBX_E_INVALID, "rows is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (first_row > ix->n || n > ix->n - first_row)
    return fail(WDBX_E_INVALID, "rows [%llu, +%llu) outside the %llu stored rows", (u64)first_row, (u64)n, (u64)ix->n);
  if (!n) return WDBX_OK;
  DeviceGuard g(ix->device);
  return upload_rows(ix, first_row, rows, n, normalize);
} WDBX_CATCH

// the two writes of listed rows: rows == nullptr is the removal
static int update_listed(wdbx_index* ix, const uint64_t* row_ids, uint64_t n, const float* rows, int normalize) {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (n && !row_ids) return fail(WDBX_E_INVALID, "row_ids is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  std::vector<uint32_t> ids32((size_t)n);
  const uint64_t bad = subset_validate(row_ids, n, ix->n, ids32.data());
  if (bad != n)
    return fail(WDBX_E_INVALID, "row_ids must be strictly increasing row numbers below %llu (entry %llu)", (u64)ix->n, (u64)bad);
  DeviceGuard g(ix->device);
  return update_rows_at(ix, ids32.data(), n, rows, normalize);
}

int wdbx_index_set_rows_at(wdbx_index* ix, const uint64_t* row_ids, uint64_t n, const float* rows, int normalize) try {
  if (n && !rows) return fail(WDBX_E_INVALID, "rows is null");
  return update_listed(ix, row_ids, n, rows, normalize);
} WDBX_CATCH

int wdbx_index_remove_rows(wdbx_index* ix, const uint64_t* row_ids, uint64_t n) try {
  return update_listed(ix, row_ids, n, nullptr, 0);
} WDBX_CATCH

int wdbx_index_get_rows(wdbx_index* ix, uint64_t first_row, uint64_t n, float* out_rows) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (n && !out_rows) return fail(WDBX_E_INVALID, "out_rows is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (first_row > ix->n || n > ix->n - first_row)
    return fail(WDBX_E_INVALID, "rows [%llu, +%llu) outside the %llu stored rows", (u64)first_row, (u64)n, (u64)ix->n);
  if (!n) return WDBX_OK;
  DeviceGuard g(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  const float* src = ix->d_rows + (size_t)first_row * ix->pitch;
  if (ix->pitch == ix->dim)
    HIP_TRY(hipMemcpy(out_rows, src, (size_t)n * ix->dim * sizeof(float), hipMemcpyDeviceToHost));
  else
    HIP_TRY(hipMemcpy2D(out_rows, (size_t)ix->dim * sizeof(float), src, (size_t)ix->pitch * sizeof(float),
                        (size_t)ix->dim * sizeof(float), n, hipMemcpyDeviceToHost));
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_fill_synthetic(wdbx_index* ix, uint64_t seed, uint64_t counter_row0, uint64_t n, int normalize,
                              uint64_t* first_row_out) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  if (first_row_out) *first_row_out = ix->n;
  if (!n) return WDBX_OK;
  int rc = ensure_room(ix, n);
  if (rc) return rc;
  rc = launch_fill(ix, ix->d_rows + (size_t)ix->n * ix->pitch, seed, counter_row0, n, normalize);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ix->stream));
  ix->n += n;
  return WDBX_OK;
} WDBX_CATCH

// Keep exactly the rows src_rows[0 .. n_keep) (strictly increasing), moved down to rows 0 .. n_keep - 1 in that order:
// the compaction behind HipFlatIndex.optimize() (the reference's rebuild hook, indexing.py:1124-1149).  In place, chunk by
// chunk through a scratch buffer: the sources of a later chunk all lie at or behind that chunk's own destination rows, so
// writing an earlier chunk cannot overwrite them.  Derived copies (norms, shadows) are kept up to the first moved row and
// rebuilt lazily behind it.
int wdbx_index_compact(wdbx_index* ix, const uint64_t* src_rows, uint64_t n_keep) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (n_keep && !src_rows) return fail(WDBX_E_INVALID, "src_rows is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (n_keep > ix->n) return fail(WDBX_E_INVALID, "%llu rows to keep of %llu stored", (u64)n_keep, (u64)ix->n);
  uint64_t first_moved = n_keep;
  for (uint64_t i = 0; i < n_keep; ++i) {
    if (src_rows[i] >= ix->n || (i && src_rows[i] <= src_rows[i - 1]))
      return fail(WDBX_E_INVALID, "src_rows must be strictly increasing row numbers below %llu (entry %llu)", (u64)ix->n, (u64)i);
    if (first_moved == n_keep && src_rows[i] != i) first_moved = i;
  }
  DeviceGuard g(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  if (first_moved < n_keep) {
    const uint64_t chunk = std::max<uint64_t>(1024, (256ull << 20) / ((uint64_t)ix->pitch * sizeof(float)));  // 256 MiB of rows at a time
    DevBuf<float> d_tmp;  // (locals: freed on every way out)
    DevBuf<u64> d_src;
    const uint64_t c_max = std::min(chunk, n_keep - first_moved);
    const int rc = d_tmp.grow((size_t)c_max * ix->pitch * sizeof(float));
    if (rc) return rc;
    hipError_t e = d_src.try_grow((size_t)c_max * sizeof(u64)) ? hipSuccess : hipErrorOutOfMemory;
    for (uint64_t i0 = first_moved; e == hipSuccess && i0 < n_keep; i0 += chunk) {
      const uint64_t c = std::min(chunk, n_keep - i0);
      e = hipMemcpyAsync(d_src, src_rows + i0, (size_t)c * sizeof(u64), hipMemcpyHostToDevice, ix->stream);
      if (e != hipSuccess) break;
      hipLaunchKernelGGL(gather_rows_kernel, dim3((uint32_t)std::min<uint64_t>((c + 3) / 4, 65536)), dim3(256), 0, ix->stream,
                         (const f4*)ix->d_rows.p, (uint32_t)(ix->pitch / 4), (const u64*)d_src, (u64)c, (f4*)d_tmp.p);
      e = hipGetLastError();
      if (e == hipSuccess)
        e = hipMemcpyAsync(ix->d_rows + (size_t)i0 * ix->pitch, d_tmp, (size_t)c * ix->pitch * sizeof(float), hipMemcpyDeviceToDevice,
                           ix->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);  // (the host list and the scratch are reused by the next chunk)
    }
    if (e != hipSuccess) return fail(WDBX_E_HIP, "compaction failed: %s (the rows behind row %llu are undefined)", hipGetErrorString(e), (u64)first_moved);
  }
  if (!ix->labels.empty()) {  // the labels move with their rows (src_rows is increasing: in place, front to back)
    ix->labels.resize((size_t)ix->n, WDBX_LABEL_NONE);
    for (uint64_t i = first_moved; i < n_keep; ++i) ix->labels[(size_t)i] = ix->labels[(size_t)src_rows[i]];
    ix->labels.resize((size_t)n_keep);
  }
  ix->lab_valid = false;
  ix->n = n_keep;
  ix->cn_rows = std::min(ix->cn_rows, first_moved);
  ix->shadow_rows = std::min(ix->shadow_rows, first_moved);
  ix->shadow8_rows = std::min(ix->shadow8_rows, first_moved);
  ix->shadow6_rows = std::min(ix->shadow6_rows, first_moved);
  ix->shadow42_rows = std::min(ix->shadow42_rows, first_moved);
  ix->shadowg_rows = std::min(ix->shadowg_rows, first_moved / 64 * 64);  // (whole 64-row groups: a group's scale depends on all its rows)
  ix->shadowg_tail_n = ~0ull;  // the groups behind the new last row still describe dropped rows: rewritten by the next batch
  ix->cn_stats_dirty = true;  // the running maximum / sum still hold the dropped rows' norms
  ix->gmax_valid = false;
  return WDBX_OK;
} WDBX_CATCH

// mask_word_count: how many words the caller's mask holds (checked against the row count under the handle's lock: a mask built
// before a concurrent add is refused instead of over-read); ~0 = the caller vouches for ceil(rows / 32) words
// held: the caller already holds the handle's mutex through this lock and keeps it (a call that answers in several steps,
// wdbx_index_search_multimask's class-by-class route): the call then never lets go of it -- no staging slot, no narrow wait.
static int search_host(wdbx_index* ix, const float* queries, int nq, int k, int normalize_queries,
                       const uint32_t* mask_words, uint64_t mask_word_count, int64_t* out_idx, float* out_score,
                       std::unique_lock<std::mutex>* held = nullptr) {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 0) return fail(WDBX_E_INVALID, "nq=%d", nq);
  if (nq == 0) return WDBX_OK;
  if (!queries || !out_idx || !out_score) return fail(WDBX_E_INVALID, "null buffer");
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  // The handle's mutex covers everything that touches the handle's state: buffer growth, the enqueue of the call's whole
  // chain of launches, option reads.  It does NOT cover the wait for the GPU when the call's queries and results live in a
  // staging slot of its own (small calls: mapped host memory the kernels read and write directly) -- the next caller on
  // another thread enqueues behind this call on the stream while this one waits for its event, so N threads calling one
  // handle (the reference's 4-worker pools per index, indexing.py:692, :1045-1048) pipeline instead of taking turns at
  // wall-clock latency.  Scratch buffers are shared by consecutive calls: the stream runs them in order.
  std::unique_lock<std::mutex> own;
  if (!held) own = std::unique_lock<std::mutex>(ix->mu);
  std::unique_lock<std::mutex>& lk = held ? *held : own;
  DeviceGuard g(ix->device);
  MaskScope scope(ix);  // the mask applies to this call only (such a call keeps the mutex to its end: d_mask is one buffer)
  int rc;
  const size_t elems = (size_t)nq * k;
  const size_t q_bytes = (size_t)nq * ix->pitch * sizeof(float);
  constexpr size_t STAGE_Q = 256 << 10, STAGE_IDX = 256 << 10, STAGE_SCORE = 128 << 10;
  constexpr size_t SLOT_BYTES = STAGE_Q + STAGE_IDX + STAGE_SCORE + 256;
  // a staging slot of its own for a small call.  Callers beyond STAGE_SLOTS in flight wait for one with the mutex RELEASED,
  // so the slot is taken FIRST, before this call has changed anything in the handle (a row mask set before the wait would
  // be seen by the calls that run meanwhile), and everything the decision rests on is looked at again after a wait.
  struct SlotHold {
    wdbx_index* ix;
    std::unique_lock<std::mutex>* lk;
    int slot = -1;
    ~SlotHold() {
      // (a call that kept the mutex -- a masked one -- keeps it until its mask is reset too: give_back leaves it as it is)
      if (slot >= 0) ix->slots.give_back(slot, *lk);
    }
  } hold{ix, &lk};
  bool gemm, zero_copy;
  for (;;) {
    // (a row mask: one masked pass over the int8 tiles when they are what would run; per-query masked scans otherwise)
    gemm = gemm_eligible(ix, nq, k) && (!(mask_words && ix->n) || masked_tiles_ready(ix, k));
    zero_copy = ix->opt_zero_copy && !gemm && !held && q_bytes <= STAGE_Q && elems * sizeof(int64_t) <= STAGE_IDX;
    if (zero_copy && !ix->h_stage) {
      void* hp = nullptr;
      void* dp = nullptr;
      // (coherent whatever HIP_HOST_COHERENT says)
      bool ok = hipHostMalloc(&hp, STAGE_SLOTS * SLOT_BYTES, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
                hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess;
      for (int s = 0; ok && s < STAGE_SLOTS; ++s) ok = hipEventCreateWithFlags(&ix->slot_done[s], hipEventDisableTiming) == hipSuccess;
      if (ok) {
        ix->h_stage = (char*)hp;
        ix->h_stage_dev = (char*)dp;
      } else {
        for (int s = 0; s < STAGE_SLOTS; ++s)
          if (ix->slot_done[s]) {
            (void)hipEventDestroy(ix->slot_done[s]);
            ix->slot_done[s] = nullptr;
          }
        if (hp) (void)hipHostFree(hp);
        (void)hipGetLastError();
        ix->opt_zero_copy = 0;  // not available here: use the copy path from now on
        zero_copy = false;
      }
    }
    if (!zero_copy || hold.slot >= 0) break;
    if ((hold.slot = ix->slots.try_take()) >= 0) break;  // (taken without a wait: nothing can have changed)
    ix->slots.wait(lk);  // mutex released while waiting: decide again afterwards
  }
  if (mask_words && ix->n && ((rc = check_mask_words(ix->n, mask_word_count)) || (rc = scope.set(mask_words)))) return rc;
  if (!gemm) ix->last_batch_masked = 0;  // (what the last_batch_* options describe is the last call, whatever it ran)
  char* const hs = zero_copy ? ix->h_stage + (size_t)hold.slot * SLOT_BYTES : nullptr;      // this call's slot, host view
  char* const ds = zero_copy ? ix->h_stage_dev + (size_t)hold.slot * SLOT_BYTES : nullptr;  // ... and device view
  // wait for this call's launches: with a slot and no row mask, by its own event with the mutex RELEASED
  const bool narrow = zero_copy && !ix->active_mask;
  auto wait_for_gpu = [&]() -> int {
    if (narrow) {
      HIP_TRY(hipEventRecord(ix->slot_done[hold.slot], ix->stream));
      lk.unlock();
      HIP_TRY(hipEventSynchronize(ix->slot_done[hold.slot]));
    } else {
      HIP_TRY(hipStreamSynchronize(ix->stream));
    }
    return WDBX_OK;
  };
  // ... or, when the call's last kernel reports into a word of the slot (merge_signal_done): the event still marks the call on
  // the stream; the wait itself is a poll of the word, which the kernel wrote behind its results (wait_done_word)
  auto wait_polled = [&](volatile uint32_t* word, uint32_t seq) -> int {
    HIP_TRY(hipEventRecord(ix->slot_done[hold.slot], ix->stream));
    hipEvent_t ev = ix->slot_done[hold.slot];
    lk.unlock();
    return wait_done_word(word, seq, ev);
  };
  bool poll_tail = false;  // a small batch whose single merge launch took the signal: the common tail below polls
  uint32_t poll_seq = 0;
  float* dq;
  int64_t* doidx;
  float* doscore;
  if (zero_copy) {
    pad_queries((float*)hs, (size_t)ix->pitch, queries, (size_t)ix->dim, (size_t)nq);
    dq = (float*)ds;
    doidx = (int64_t*)(ds + STAGE_Q);
    doscore = (float*)(ds + STAGE_Q + STAGE_IDX);
    if (normalize_queries && ix->metric == WDBX_METRIC_COSINE && (rc = launch_normalize(ix, dq, nq))) return rc;
  } else {
    if ((rc = ensure_out(ix, elems)) || (rc = upload_queries(ix, queries, (uint64_t)nq, normalize_queries))) return rc;
    dq = ix->d_q;
    doidx = ix->d_oidx;
    doscore = ix->d_oscore;
  }
  if (gemm) {
    rc = enqueue_search_gemm(ix, dq, nq, k, doidx, doscore);
    if (rc) return rc;
    std::vector<uint32_t> counts(nq);
    HIP_TRY(hipMemcpyAsync(counts.data(), ix->d_count, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    // a query whose candidate buffer overflowed has been re-run exactly by the conditional repair launches queued behind
    // its block (enqueue_batch_repair); shapes without a device-side repair are re-run here
    for (int q = 0; q < nq && !ix->last_batch_repaired; ++q)
      if (counts[q] > ix->last_batch_cap &&
          (rc = enqueue_exact_rerun(ix, dq + (size_t)q * ix->pitch, k, doidx + (size_t)q * k, doscore + (size_t)q * k)))
        return rc;
  } else {
    // Lone query through mapped memory: the u8 selection scan skips its queued repair launches and its final merge --
    // the re-scored candidates' keys and their count land in the call's slot and THIS thread ranks them after its wait
    // (an overflowed candidate buffer is repaired then, too); on small shards the threshold is taken inside the full pass.
    // 3 dependent launches instead of 5 (7 with the repairs).
    volatile uint32_t* const over = zero_copy ? (volatile uint32_t*)(hs + STAGE_Q + STAGE_IDX + STAGE_SCORE) : nullptr;
    const bool defer = zero_copy && nq == 1 && !use_select(ix, k);
    uint32_t done_seq = 0;
    if (defer) {
      over[0] = 0;
      over[1] = 0;
      over[2] = 0;
      ix->defer_flag_dev = (uint32_t*)(ds + STAGE_Q + STAGE_IDX + STAGE_SCORE);
      if (narrow && ix->opt_poll_done) {  // the chain's last kernel reports into over[2]; this thread polls it (wait_for_lone)
        if (++ix->lone_seq == 0) ++ix->lone_seq;
        done_seq = ix->lone_seq;
        ix->done_flag_dev = ix->defer_flag_dev + 2;
        ix->done_seq = done_seq;
        ix->done_signals = 0;
      }
      if (ix->opt_lone_host_select) {
        ix->lone_keys_dev = (u64*)(ds + STAGE_Q);
        ix->lone_count_dev = ix->defer_flag_dev + 1;
        ix->lone_cap_max = (uint32_t)((STAGE_IDX + STAGE_SCORE) / sizeof(u64));
      }
    }
    // a small batch (one round of up to 32 queries) on the plain fp32 scan ends in ONE merge launch of nq workgroups: the same
    // completion word, written by the last of them (a ticket)
    const bool batch_poll = !defer && narrow && nq > 1 && nq <= 32 && ix->opt_poll_done && !use_select(ix, k);
    if (batch_poll) {
      if (!ix->d_ticket) {
        if ((rc = ix->d_ticket.grow(sizeof(uint32_t)))) return rc;
        HIP_TRY(hipMemsetAsync(ix->d_ticket, 0, sizeof(uint32_t), ix->stream));
      }
      over[2] = 0;
      if (++ix->lone_seq == 0) ++ix->lone_seq;
      done_seq = ix->lone_seq;
      ix->done_flag_dev = (uint32_t*)(ds + STAGE_Q + STAGE_IDX + STAGE_SCORE) + 2;
      ix->done_seq = done_seq;
      ix->done_signals = 0;
    }
    ix->lone_used = false;
    rc = enqueue_search(ix, dq, nq, k, doidx, doscore, SEARCH_FINAL);
    ix->defer_flag_dev = nullptr;
    ix->lone_keys_dev = nullptr;
    ix->lone_count_dev = nullptr;
    // exactly one launch took the completion signal -- a final merge_kernel -- and it is the chain's last kernel on the plain
    // fp32 scan (0) and on the u8 scan (2) when its candidates are ranked on the device; the u8 scan's usual lone form ends in
    // rescore_kernel (hundreds of waves each storing one key: a host-visibility fence per storing wave costs more than the
    // runtime's path) and the bf16 single-query path (1) queues repair launches behind its merge: event wait as before
    const bool poll = ix->done_flag_dev && ix->done_signals == 1 &&
                      (ix->last_single_path == 0 || (ix->last_single_path == 2 && !batch_poll));  // (a u8 ROUND queues repairs behind its merge)
    ix->done_flag_dev = nullptr;
    if (rc) return rc;
    if (poll && batch_poll) {
      poll_tail = true;
      poll_seq = done_seq;
    }
    if (defer) {
      const bool lone_used = ix->lone_used;         // (handle state: read before the mutex may go)
      const uint32_t cap = ix->last_batch_cap;
      const int metric = ix->metric;
      if (poll) {
        if ((rc = wait_polled(over + 2, done_seq))) return rc;
      } else if ((rc = wait_for_gpu())) return rc;
      bool repair = false;
      if (lone_used) {
        const uint32_t cnt = over[1];
        if (cnt > cap) {
          repair = true;
        } else {  // the exact keys of the kept rows: the k largest, in key order = (score descending, row ascending)
          rank_keys_host((const uint64_t*)(hs + STAGE_Q), cnt, k, metric == WDBX_METRIC_L2, out_idx, out_score);
          return WDBX_OK;
        }
      } else if (over[0]) {
        repair = true;
      }
      if (repair) {  // (rare: back under the mutex, the exact scan into the same slot)
        if (!lk.owns_lock()) lk.lock();
        if ((rc = enqueue_exact_rerun(ix, dq, k, doidx, doscore))) return rc;  // (a lone query: nq = 1)
        HIP_TRY(hipStreamSynchronize(ix->stream));
      }
      memcpy(out_idx, hs + STAGE_Q, elems * sizeof(int64_t));
      memcpy(out_score, hs + STAGE_Q + STAGE_IDX, elems * sizeof(float));
      return WDBX_OK;
    }
  }
  if (zero_copy) {
    if (poll_tail) {
      if ((rc = wait_polled((volatile uint32_t*)(hs + STAGE_Q + STAGE_IDX + STAGE_SCORE) + 2, poll_seq))) return rc;
    } else if ((rc = wait_for_gpu())) return rc;
    memcpy(out_idx, hs + STAGE_Q, elems * sizeof(int64_t));
    memcpy(out_score, hs + STAGE_Q + STAGE_IDX, elems * sizeof(float));
  } else if ((rc = download_results(ix, elems, out_idx, out_score))) {
    return rc;
  }
  return WDBX_OK;
}

int wdbx_index_search(wdbx_index* ix, const float* queries, int nq, int k, int normalize_queries, int64_t* out_idx,
                      float* out_score) try {
  return search_host(ix, queries, nq, k, normalize_queries, nullptr, 0, out_idx, out_score);
} WDBX_CATCH

int wdbx_index_search_masked(wdbx_index* ix, const float* queries, int nq, int k, int normalize_queries,
                             const uint32_t* mask_words, int64_t* out_idx, float* out_score) try {
  if (!mask_words) return fail(WDBX_E_INVALID, "mask_words is null");
  return search_host(ix, queries, nq, k, normalize_queries, mask_words, ~0ull, out_idx, out_score);
} WDBX_CATCH

int wdbx_index_search_masked_n(wdbx_index* ix, const float* queries, int nq, int k, int normalize_queries,
                               const uint32_t* mask_words, uint64_t mask_word_count, int64_t* out_idx, float* out_score) try {
  if (!mask_words) return fail(WDBX_E_INVALID, "mask_words is null");
  return search_host(ix, queries, nq, k, normalize_queries, mask_words, mask_word_count, out_idx, out_score);
} WDBX_CATCH

// ---- one row mask PER QUERY in one batched call (host_multimask.h) ---------------------------
// query_mask[i] = which of the call's masks query i reads, or -1 (every row).  When the int8 tiles are what a masked batch
// would run (masked_tiles_ready) the whole call is one tile pass per block of up to 256 placed queries, whatever the number
// of masks: the queries are placed so that a column group of 16 shares one mask, each class of the call gets its bad-row
// table, and the kernels read the table row of the column group at hand.  Otherwise every class goes through the call that
// existed before (wdbx_index_search_masked_n; wdbx_index_search for the class without a mask) and the answers are scattered
// back.  Results in the caller's order either way.  The call holds the handle's mutex to its end on both routes (the masks,
// the placed queries and the tables are the handle's; the class-by-class calls run under the lock this call took).
int wdbx_index_search_multimask(wdbx_index* ix, const float* queries, int nq, int k, int normalize_queries,
                                const uint32_t* const* mask_words, const uint64_t* mask_word_counts, int n_masks,
                                const int32_t* query_mask, int64_t* out_idx, float* out_score) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 1) return fail(WDBX_E_INVALID, "nq=%d", nq);
  if (!queries || !out_idx || !out_score || !query_mask) return fail(WDBX_E_INVALID, "null buffer");
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  if (n_masks < 0 || n_masks > WDBX_MAX_CALL_MASKS) return fail(WDBX_E_INVALID, "n_masks=%d outside [0, %d]", n_masks, WDBX_MAX_CALL_MASKS);
  if (n_masks && (!mask_words || !mask_word_counts)) return fail(WDBX_E_INVALID, "null mask list");
  for (int m = 0; m < n_masks; ++m)
    if (!mask_words[m]) return fail(WDBX_E_INVALID, "mask %d is null", m);
  for (int q = 0; q < nq; ++q)
    if (query_mask[q] < -1 || query_mask[q] >= n_masks)
      return fail(WDBX_E_INVALID, "query_mask[%d]=%d outside [-1, %d)", q, (int)query_mask[q], n_masks);
  std::unique_lock<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  const size_t words = (size_t)((ix->n + 31) / 32);
  int rc;
  for (int m = 0; m < n_masks && ix->n; ++m)
    if ((rc = check_mask_words(ix->n, mask_word_counts[m], ("row mask " + std::to_string(m)).c_str()))) return rc;
  const bool l2 = ix->metric == WDBX_METRIC_L2;
  ix->last_batch_masked = 0;
  const bool tiles = ix->n && ix->n < 0xFFFFFF00ull && gemm_eligible(ix, nq, k) && masked_tiles_ready(ix, k);
  if (!tiles) {
    // class by class through the calls that existed before, in the caller's order inside a class; the lock stays held
    std::vector<int32_t> classes((size_t)n_masks + 1);
    for (int c = -1; c < n_masks; ++c) classes[(size_t)(c + 1)] = c;
    return for_each_class(nq, ix->dim, k, queries, query_mask, classes, out_idx, out_score,
                          [&](int32_t c, int nm, const float* cq, int64_t* ci, float* cs) {
                            return search_host(ix, cq, nm, k, normalize_queries, c < 0 ? nullptr : mask_words[c],
                                               c < 0 ? 0 : mask_word_counts[c], ci, cs, &lk);
                          });
  }
  // ---- the tile route ----
  const int forced = (ix->opt_gemm_ct == 1 || ix->opt_gemm_ct == 2 || ix->opt_gemm_ct == 4) ? (int)ix->opt_gemm_ct : 4;
  const int max_ct = std::min(forced, l2 ? std::min(2, i8g_max_ct(ix)) : i8g_max_ct(ix));
  MultimaskPlan plan;
  if (!multimask_plan(query_mask, nq, n_masks, 64 * max_ct, &plan)) return fail(WDBX_E_INVALID, "query_mask cannot be placed");
  const size_t slots = plan.slot_query.size(), rows = plan.classes.size();
  // the classes' masks (class row r at r * stride words; the class without a mask has none), their allowed rows counted on
  // the host copies as set_active_mask does, and the row -> mask table of the bad-row kernel
  const size_t stride = (words + 63) / 64 * 64;
  std::vector<uint64_t> allowed(rows, ix->n);
  std::vector<int32_t> class_mask(rows, -1);
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t off_q = 0, off_slot = up(slots * ix->pitch * sizeof(float)), off_cm = off_slot + up(slots * sizeof(int32_t)),
               off_masks = off_cm + up(rows * sizeof(int32_t)), total = off_masks + rows * stride * sizeof(uint32_t);
  if ((rc = ix->d_mm.grow(total))) return rc;
  float* const d_slots_q = (float*)(ix->d_mm + off_q);
  int32_t* const d_slot_query = (int32_t*)(ix->d_mm + off_slot);
  int32_t* const d_class_mask = (int32_t*)(ix->d_mm + off_cm);
  uint32_t* const d_masks = (uint32_t*)(ix->d_mm + off_masks);
  for (size_t r = 0; r < rows; ++r) {
    const int c = plan.classes[r];
    if (c < 0) continue;
    class_mask[r] = (int32_t)r;
    const uint32_t* mw = mask_words[c];
    HIP_TRY(hipMemcpyAsync(d_masks + r * stride, mw, words * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
    allowed[r] = mask_allowed_rows(mw, ix->n);
  }
  HIP_TRY(hipMemcpyAsync(d_slot_query, plan.slot_query.data(), slots * sizeof(int32_t), hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(hipMemcpyAsync(d_class_mask, class_mask.data(), rows * sizeof(int32_t), hipMemcpyHostToDevice, ix->stream));
  // the queries as in search_host, then into their slots
  if ((rc = ensure_out(ix, slots * (size_t)k)) || (rc = upload_queries(ix, queries, (uint64_t)nq, normalize_queries))) return rc;
  const uint32_t pitch4 = (uint32_t)(ix->pitch / 4);
  hipLaunchKernelGGL(place_queries_kernel, dim3((uint32_t)((slots * pitch4 + 255) / 256)), dim3(256), 0, ix->stream, (const f4*)ix->d_q.p,
                     (const int32_t*)d_slot_query, pitch4, (uint32_t)slots, (f4*)d_slots_q);
  HIP_TRY(hipGetLastError());
  ix->last_batch_repaired = false;
  MultiCall mc = {&plan, d_slot_query, d_masks, stride, d_class_mask, allowed.data()};
  MaskScope scope(ix, true);  // (the repair launches set the class's mask for their own duration; nothing outlives the call)
  if ((rc = enqueue_search_gemm8(ix, d_slots_q, (int)slots, k, ix->d_oidx, ix->d_oscore, SEARCH_FINAL, nullptr, &mc))) return rc;
  // what wdbx_index_batch_status reports: the caller's queries
  ix->last_batch_nq = (uint32_t)nq;
  ix->last_batch_slot.assign((size_t)nq, 0);
  for (size_t s2 = 0; s2 < slots; ++s2)
    if (plan.slot_query[s2] >= 0) ix->last_batch_slot[(size_t)plan.slot_query[s2]] = (int32_t)s2;
  std::vector<uint32_t> counts(slots);
  HIP_TRY(hipMemcpyAsync(counts.data(), ix->d_count, slots * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  // shapes without a device-side repair (option batch_repair = 0, partial lists beyond 256 MiB): the overflowed queries are
  // re-run here on the fp32 scan, each with its class's mask
  for (size_t s2 = 0; s2 < slots && !ix->last_batch_repaired; ++s2)
    if (plan.slot_query[s2] >= 0 && counts[s2] > ix->last_batch_cap) {
      const int c = plan.group_class[s2 / MULTIMASK_GROUP];
      const size_t r = (size_t)(std::lower_bound(plan.classes.begin(), plan.classes.end(), c) - plan.classes.begin());
      ix->active_mask = c < 0 ? nullptr : d_masks + r * stride;
      ix->mask_allowed = allowed[r];
      rc = enqueue_exact_rerun(ix, d_slots_q + s2 * ix->pitch, k, ix->d_oidx + s2 * k, ix->d_oscore + s2 * k);
      ix->active_mask = nullptr;
      if (rc) return rc;
    }
  return download_results(ix, plan.slot_query, k, out_idx, out_score);
} WDBX_CATCH

// ---- search among listed rows (kernels_subset.h, host_subset.h) -------------------------------------
// The whole call holds the handle's mutex (like a masked search: the list buffer is the handle's).  The list is validated
// and narrowed under the lock (row numbers are checked against the row count a concurrent add cannot change meanwhile), goes
// to the device once, and the queries are served in rounds (subset_plan): subset_kernel, then the ranking tail
// (enqueue_rank_tail, host_index.h).  The scoring launches are bracketed as scan launches.
// held: the caller already holds the handle's mutex and keeps it (wdbx_index_search_row_lists' list-by-list route), as in search_host.
static int search_rows_host(wdbx_index* ix, const float* queries, int nq, int k, int normalize_queries, const uint64_t* row_ids,
                            uint64_t n_ids, int64_t* out_idx, float* out_score, bool held = false) {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 1) return fail(WDBX_E_INVALID, "nq=%d", nq);
  if (!queries || !out_idx || !out_score) return fail(WDBX_E_INVALID, "null buffer");
  if (n_ids && !row_ids) return fail(WDBX_E_INVALID, "row_ids is null");
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  std::unique_lock<std::mutex> lk;
  if (!held) lk = std::unique_lock<std::mutex>(ix->mu);
  if (ix->n >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "shard holds too many rows for 32-bit row keys");
  if (n_ids > ix->n) return fail(WDBX_E_INVALID, "%llu listed rows of %llu stored", (u64)n_ids, (u64)ix->n);
  std::vector<uint32_t> ids32((size_t)n_ids);
  const uint64_t bad = subset_validate(row_ids, n_ids, ix->n, ids32.data());
  if (bad != n_ids)
    return fail(WDBX_E_INVALID, "row_ids must be strictly increasing row numbers below %llu (entry %llu)", (u64)ix->n, (u64)bad);
  const size_t elems = (size_t)nq * k;
  const SubsetPlan sp = subset_plan(n_ids, nq, k, ix->cu_count, ix->opt_rows_keys_max, ix->opt_select_min_k, ix->opt_lds_lists != 0);
  ix->last_rows_path = sp.route;
  if (sp.route == SUBSET_NONE) {  // nothing listed: every slot empty, as wdbx_index_search leaves them
    for (size_t i = 0; i < elems; ++i) {
      out_idx[i] = -1;
      out_score[i] = 0.0f;
    }
    return WDBX_OK;
  }
  DeviceGuard g(ix->device);
  int rc;
  if ((rc = ensure_out(ix, elems))) return rc;
  if ((rc = ix->d_sub_ids.grow((size_t)n_ids * sizeof(uint32_t)))) return rc;
  const bool lists = sp.route == SUBSET_LISTS;
  const RankSource::Form form = lists ? RankSource::LISTS : sp.route == SUBSET_SELECT ? RankSource::SELECT : RankSource::KEYS;
  if ((rc = grow_rank_scratch(ix, form, sp.scratch_u64))) return rc;
  if ((rc = upload_queries(ix, queries, (uint64_t)nq, normalize_queries))) return rc;
  HIP_TRY(hipMemcpyAsync(ix->d_sub_ids, ids32.data(), (size_t)n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));

  const uint32_t pitch4 = (uint32_t)ix->pitch / 4;
  const bool reg = k <= 128 && !ix->opt_lds_lists;
  const int mode = lists ? (reg ? 1 : 0) : 2;
  const subset_fn fn = pick_subset(ix->metric, mode, sp.qb, pitch4);
  if (!fn) return fail(WDBX_E_STATE, "no listed-rows instance for mode %d with %d queries per block", mode, sp.qb);
  const size_t lds = lists ? sp.lds : 0;
  if (lds >= 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int q0 = 0; q0 < nq; q0 += sp.round) {
    const int b = std::min(sp.round, nq - q0);
    SubsetArgs a = {};
    a.rows = (const f4*)ix->d_rows.p;
    a.queries = (const f4*)(ix->d_q + (size_t)q0 * ix->pitch);
    a.ids = ix->d_sub_ids;
    a.out = lists ? ix->d_partials : ix->d_sub_keys;
    a.key_stride = n_ids;
    a.n_ids = (uint32_t)n_ids;
    a.pitch4 = pitch4;
    a.nq = (uint32_t)b;
    a.k = k;
    const uint32_t qblocks = (uint32_t)((b + sp.qb - 1) / sp.qb);
    if ((rc = record(ix->scan_ev, ix->profile, ix->stream, true))) return rc;
    hipLaunchKernelGGL(fn, dim3(sp.blocks, qblocks), dim3(256), lds, ix->stream, a);
    HIP_TRY(hipGetLastError());
    if ((rc = record(ix->scan_ev, ix->profile, ix->stream, false))) return rc;
    const RankSource src = lists ? RankSource{form, ix->d_partials, sp.P, nullptr} : RankSource{form, ix->d_sub_keys, n_ids, nullptr};
    if ((rc = enqueue_rank_tail(ix, src, q0, b, k, ix->metric))) return rc;
  }
  return download_results(ix, elems, out_idx, out_score);
}

int wdbx_index_search_rows(wdbx_index* ix, const float* queries, int nq, int k, int normalize_queries, const uint64_t* row_ids,
                           uint64_t n_ids, int64_t* out_idx, float* out_score) try {
  return search_rows_host(ix, queries, nq, k, normalize_queries, row_ids, n_ids, out_idx, out_score);
} WDBX_CATCH

// ---- distance matrix among listed rows (kernels_matrix.h, host_matrix.h) --------------------
// wdbx_index_search_rows with the listed rows themselves as the queries.  The whole call holds the handle's mutex.  Under it the
// list is validated and narrowed by the pass wdbx_index_search_rows uses and goes to the device once; nothing else goes up: the
// anchors are read from the corpus through the list.  Every round of consecutive anchors (matrix_plan) is one matrix_kernel
// launch, bracketed as a scan launch, and the ranking tail writing from the round's first slot on; one download at the end.
int wdbx_index_search_matrix(wdbx_index* ix, const uint64_t* row_ids, uint64_t n_ids, int k, int64_t* out_idx, float* out_score) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  if (n_ids && (!row_ids || !out_idx || !out_score)) return fail(WDBX_E_INVALID, "null buffer");
  std::unique_lock<std::mutex> lk(ix->mu);
  if (ix->n >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "shard holds too many rows for 32-bit row keys");
  if (n_ids > ix->n) return fail(WDBX_E_INVALID, "%llu listed rows of %llu stored", (u64)n_ids, (u64)ix->n);
  if (n_ids > MATRIX_MAX_IDS) return fail(WDBX_E_INVALID, "%llu listed rows in one call: at most 2^31 - 1", (u64)n_ids);
  std::vector<uint32_t> ids32((size_t)n_ids);
  const uint64_t bad = subset_validate(row_ids, n_ids, ix->n, ids32.data());
  if (bad != n_ids)
    return fail(WDBX_E_INVALID, "row_ids must be strictly increasing row numbers below %llu (entry %llu)", (u64)ix->n, (u64)bad);
  const uint32_t pitch4 = (uint32_t)ix->pitch / 4;
  const MatrixPlan mp = matrix_plan(n_ids, k, pitch4, ix->cu_count, ix->opt_rows_keys_max, ix->opt_select_min_k, ix->opt_lds_lists != 0);
  ix->last_matrix_path = mp.sp.route;
  ix->last_matrix_rounds = (int64_t)mp.rounds;
  if (mp.sp.route == SUBSET_NONE) return WDBX_OK;  // (nothing listed: nothing to write, nothing launched)
  const size_t elems = (size_t)n_ids * k;
  DeviceGuard g(ix->device);
  int rc;
  if ((rc = ensure_out(ix, elems))) return rc;
  if ((rc = ix->d_sub_ids.grow((size_t)n_ids * sizeof(uint32_t)))) return rc;
  const bool lists = mp.sp.route == SUBSET_LISTS;
  const RankSource::Form form = lists ? RankSource::LISTS : mp.sp.route == SUBSET_SELECT ? RankSource::SELECT : RankSource::KEYS;
  if ((rc = grow_rank_scratch(ix, form, mp.sp.scratch_u64))) return rc;
  HIP_TRY(hipMemcpyAsync(ix->d_sub_ids, ids32.data(), (size_t)n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
  const matrix_fn fn = pick_matrix(ix->metric, mp.mode, mp.sp.qb, pitch4);
  if (!fn) return fail(WDBX_E_STATE, "no distance-matrix instance for mode %d with %d anchors per block", mp.mode, mp.sp.qb);
  const size_t lds = lists ? mp.sp.lds : 0;
  for (uint64_t r = 0; r < mp.rounds; ++r) {
    const uint64_t first = matrix_round_first(mp, r);
    const int b = matrix_round_anchors(mp, n_ids, r);
    MatrixArgs a = {};
    a.rows = (const f4*)ix->d_rows.p;
    a.ids = ix->d_sub_ids;
    a.out = lists ? ix->d_partials : ix->d_sub_keys;
    a.key_stride = n_ids;
    a.n_ids = (uint32_t)n_ids;
    a.pitch4 = pitch4;
    a.first = (uint32_t)first;
    a.na = (uint32_t)b;
    a.k = k;
    if ((rc = launch_bracketed(ix, ix->scan_ev, fn, dim3(mp.sp.blocks, matrix_anchor_blocks(mp, b)), lds, a))) return rc;
    const RankSource src = lists ? RankSource{form, ix->d_partials, mp.sp.P, nullptr} : RankSource{form, ix->d_sub_keys, n_ids, nullptr};
    if ((rc = enqueue_rank_tail(ix, src, (int)first, b, k, ix->metric))) return rc;
  }
  return download_results(ix, elems, out_idx, out_score);
} WDBX_CATCH

// ---- one row list PER QUERY in one batched call (host_rowlists.h, kernels_rowlists.h) --------
// The whole call holds the handle's mutex.  Under it: the CSR pair and every list are checked, the plan is made, the pass
// lists' rows, the work items, the slots' list lengths and the queries (in slot order) go to the device once, and every round
// is one rowlists_kernel launch (bracketed as a scan launch) and one merge_kernel launch over the slots' keys as unsorted
// candidates with the slot's list length as its count.  One download, then the results go back to the caller's order.  The
// queries of lists beyond rows_keys_max then run list by list through search_rows_host under the same lock.
int wdbx_index_search_row_lists(wdbx_index* ix, const float* queries, int nq, int k, int normalize_queries, const uint64_t* list_rows,
                                const uint64_t* list_offsets, int n_lists, const int32_t* query_list, int64_t* out_idx,
                                float* out_score) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 1) return fail(WDBX_E_INVALID, "nq=%d", nq);
  if (n_lists < 1) return fail(WDBX_E_INVALID, "n_lists=%d: every query needs a list", n_lists);
  if (!queries || !out_idx || !out_score || !list_offsets || !query_list) return fail(WDBX_E_INVALID, "null buffer");
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  int64_t where = -1;
  switch (rowlists_check(list_offsets, n_lists, query_list, nq, &where)) {
    case ROWLISTS_OK: break;
    case ROWLISTS_BAD_OFFSET:
      return where == 0 ? fail(WDBX_E_INVALID, "list_offsets[0]=%llu, not 0", (u64)list_offsets[0])
                        : fail(WDBX_E_INVALID, "list_offsets[%lld]=%llu below list_offsets[%lld]=%llu", (long long)where,
                               (u64)list_offsets[where], (long long)where - 1, (u64)list_offsets[where - 1]);
    case ROWLISTS_BAD_QUERY:
      return fail(WDBX_E_INVALID, "query_list[%lld]=%d outside [0, %d)", (long long)where, (int)query_list[where], n_lists);
    default: return fail(WDBX_E_INVALID, "bad list arguments");
  }
  if (list_offsets[n_lists] && !list_rows) return fail(WDBX_E_INVALID, "list_rows is null");
  std::unique_lock<std::mutex> lk(ix->mu);
  if (ix->n >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "shard holds too many rows for 32-bit row keys");
  RowListsPlan plan;
  if (!rowlists_plan(list_offsets, n_lists, query_list, nq, ix->opt_rows_keys_max, &plan))
    return fail(WDBX_E_INVALID, "%llu listed rows in one call: at most 2^32 - 1", (u64)plan.pass_ids);
  std::vector<uint32_t> ids32((size_t)plan.pass_ids);
  int bad_list = -1;
  uint64_t bad_entry = 0;
  if (!rowlists_validate(list_rows, list_offsets, n_lists, ix->n, &plan, ids32.data(), &bad_list, &bad_entry))
    return fail(WDBX_E_INVALID, "list %d must hold strictly increasing row numbers below %llu (entry %llu)", bad_list, (u64)ix->n,
                (u64)bad_entry);
  ix->last_lists_path = plan.path();
  ix->last_lists_items = (int64_t)plan.items.size();
  ix->last_lists_rounds = plan.items.empty() ? 0 : (int64_t)plan.rounds.size();
  const size_t slots = plan.slot_query.size();
  if (plan.items.empty()) {  // (only empty lists on the pass: every slot empty, as wdbx_index_search_rows leaves them)
    for (size_t s = 0; s < slots; ++s)
      for (int i = 0; i < k; ++i) {
        out_idx[(size_t)plan.slot_query[s] * k + i] = -1;
        out_score[(size_t)plan.slot_query[s] * k + i] = 0.0f;
      }
  } else {
    DeviceGuard g(ix->device);
    int rc;
    if ((rc = ensure_out(ix, slots * (size_t)k))) return rc;
    size_t key_u64 = 0;
    for (const RowListsRound& r : plan.rounds) key_u64 = std::max(key_u64, (size_t)r.slots * (size_t)r.stride);
    const size_t items_bytes = (plan.items.size() * sizeof(RowListsItem) + 255) / 256 * 256;
    if ((rc = ix->d_sub_ids.grow((size_t)plan.pass_ids * sizeof(uint32_t)))) return rc;
    if ((rc = ix->d_sub_keys.grow(key_u64 * sizeof(u64)))) return rc;
    if ((rc = ix->d_rl.grow(items_bytes + slots * sizeof(uint32_t)))) return rc;
    const RowListsItem* const d_items = (const RowListsItem*)ix->d_rl.p;
    const uint32_t* const d_len = (const uint32_t*)(ix->d_rl + items_bytes);
    // the queries in slot order, padded to the row pitch (host side: one upload whatever the order)
    std::vector<float> hq(slots * (size_t)ix->pitch);
    pad_queries(hq.data(), (size_t)ix->pitch, queries, (size_t)ix->dim, slots, plan.slot_query.data());
    if ((rc = upload_queries(ix, hq.data(), slots, normalize_queries, ix->pitch))) return rc;
    HIP_TRY(hipMemcpyAsync(ix->d_sub_ids, ids32.data(), (size_t)plan.pass_ids * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipMemcpyAsync(ix->d_rl, plan.items.data(), plan.items.size() * sizeof(RowListsItem), hipMemcpyHostToDevice, ix->stream));
    HIP_TRY(hipMemcpyAsync(ix->d_rl + items_bytes, plan.slot_len.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
    const uint32_t pitch4 = (uint32_t)ix->pitch / 4;
    const rowlists_fn fn = pick_rowlists(ix->metric, plan.qb, pitch4);
    if (!fn) return fail(WDBX_E_STATE, "no row-lists instance with %d queries per block", plan.qb);
    for (const RowListsRound& r : plan.rounds) {
      if (r.items) {  // (a round of empty lists only scores nothing; the ranking below still empties its slots)
        if (r.items > 0x7FFFFFFFull) return fail(WDBX_E_INVALID, "%zu work items in one round", r.items);
        RowListsArgs a = {};
        a.rows = (const f4*)ix->d_rows.p;
        a.queries = (const f4*)(ix->d_q + (size_t)r.slot0 * ix->pitch);
        a.ids = ix->d_sub_ids;
        a.items = d_items + r.item0;
        a.keys = ix->d_sub_keys;
        a.stride = r.stride;
        a.pitch4 = pitch4;
        if ((rc = launch_bracketed(ix, ix->scan_ev, fn, dim3((uint32_t)r.items), 0, a))) return rc;
      }
      const RankSource src = {RankSource::KEYS, ix->d_sub_keys, r.stride, d_len + r.slot0};
      if ((rc = enqueue_rank_tail(ix, src, (int)r.slot0, (int)r.slots, k, ix->metric))) return rc;
    }
    if ((rc = download_results(ix, plan.slot_query, k, out_idx, out_score))) return rc;
  }
  // the longer lists (each has queries: rowlists_plan), each with its queries in the caller's order, through the call that
  // existed before; the lock stays held
  return for_each_class(nq, ix->dim, k, queries, query_list, plan.fallback_lists, out_idx, out_score,
                        [&](int32_t l, int nm, const float* cq, int64_t* ci, float* cs) {
                          return search_rows_host(ix, cq, nm, k, normalize_queries, list_rows + list_offsets[l],
                                                  list_offsets[l + 1] - list_offsets[l], ci, cs, true);
                        });
} WDBX_CATCH

// ---- distinct search: at most one row per label (host_labels.h, kernels_labels.h) -------------
int wdbx_index_set_labels(wdbx_index* ix, uint64_t first_row, uint64_t n, const uint32_t* labels) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (n && !labels) return fail(WDBX_E_INVALID, "labels is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (first_row > ix->n || n > ix->n - first_row)
    return fail(WDBX_E_INVALID, "rows [%llu, +%llu) outside the %llu stored rows", (u64)first_row, (u64)n, (u64)ix->n);
  if (!n) return WDBX_OK;
  ix->labels.resize((size_t)ix->n, WDBX_LABEL_NONE);  // (rows added since the last call start as NONE)
  std::copy(labels, labels + n, ix->labels.begin() + (size_t)first_row);
  ix->lab_valid = false;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_get_labels(wdbx_index* ix, uint64_t first_row, uint64_t n, uint32_t* out_labels) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (n && !out_labels) return fail(WDBX_E_INVALID, "out_labels is null");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (first_row > ix->n || n > ix->n - first_row)
    return fail(WDBX_E_INVALID, "rows [%llu, +%llu) outside the %llu stored rows", (u64)first_row, (u64)n, (u64)ix->n);
  for (uint64_t i = 0; i < n; ++i)
    out_labels[i] = first_row + i < ix->labels.size() ? ix->labels[(size_t)(first_row + i)] : WDBX_LABEL_NONE;
  return WDBX_OK;
} WDBX_CATCH

// the device copy of the label order, for the labels and the row count as they are now (under the handle's mutex)
static int ensure_label_order(wdbx_index* ix) {
  if (ix->lab_valid && ix->lab_n == ix->n) return WDBX_OK;
  LabelOrder lo;
  label_order_build(ix->labels.data(), std::min<uint64_t>(ix->labels.size(), ix->n), ix->n, &lo);
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t rows_b = (size_t)ix->n * sizeof(uint32_t);
  const size_t off_dense = up(rows_b), off_span = off_dense + up(rows_b),
               off_label = off_span + up(lo.span_item0.size() * sizeof(uint32_t)),
               total = off_label + lo.label_item0.size() * sizeof(uint32_t);
  ix->lab_valid = false;
  int rc = ix->d_lab.grow(total);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(ix->d_lab, lo.rows.data(), rows_b, hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(hipMemcpyAsync(ix->d_lab + off_dense, lo.dense.data(), rows_b, hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(hipMemcpyAsync(ix->d_lab + off_span, lo.span_item0.data(), lo.span_item0.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(hipMemcpyAsync(ix->d_lab + off_label, lo.label_item0.data(), lo.label_item0.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));  // (the host tables go away with this call)
  ix->lab_off_dense = off_dense;
  ix->lab_off_span = off_span;
  ix->lab_off_label = off_label;
  ix->lab_items = lo.n_items;
  ix->lab_labels = lo.n_labels;
  ix->lab_spans = lo.n_spans;
  label_runs_build(lo, ix->labels.data(), std::min<uint64_t>(ix->labels.size(), ix->n), &ix->lab_runs);
  ix->lab_row0 = std::move(lo.label_row0);
  ix->lab_n = ix->n;
  ix->lab_valid = true;
  return WDBX_OK;
}

// what the label calls (distinct, multi-vector) share: label_keys_kernel's arguments for nq queries from first_query on, ...
static LabelKeysArgs label_keys_args(const wdbx_index* ix, uint64_t first_query, uint32_t nq, uint32_t pitch4) {
  LabelKeysArgs a = {};
  a.rows = (const f4*)ix->d_rows.p;
  a.queries = (const f4*)(ix->d_q + (size_t)first_query * ix->pitch);
  a.order = (const uint32_t*)ix->d_lab.p;
  a.dense = (const uint32_t*)(ix->d_lab + ix->lab_off_dense);
  a.span_item0 = (const uint32_t*)(ix->d_lab + ix->lab_off_span);
  a.mask = ix->active_mask;
  a.keys = ix->d_sub_keys;
  a.key_stride = ix->lab_items;
  a.n = (uint32_t)ix->n;
  a.n_spans = ix->lab_spans;
  a.pitch4 = pitch4;
  a.nq = nq;
  return a;
}

// ... their scratch: the item keys in d_sub_keys and behind them, on the select route, a key per label; else the partial lists
static int grow_label_scratch(wdbx_index* ix, bool select, size_t keys_u64, size_t rank_u64) {
  if (select) return grow_rank_scratch(ix, RankSource::SELECT, keys_u64 + rank_u64);
  const int rc = ix->d_sub_keys.grow(keys_u64 * sizeof(u64));
  return rc ? rc : grow_rank_scratch(ix, RankSource::LISTS, rank_u64);
}

// ... and what their ranking launch leaves to the tail
static RankSource label_rank_source(const wdbx_index* ix, bool select, size_t keys_u64, uint32_t rank_blocks) {
  return select ? RankSource{RankSource::SELECT, ix->d_sub_keys + keys_u64, ix->lab_labels, nullptr}
                : RankSource{RankSource::LISTS, ix->d_partials, rank_blocks, nullptr};
}

// The full pass for nq host queries, under the handle's mutex, on a non-empty index: per round (distinct_plan) label_keys_kernel
// (bracketed as a scan launch), label_rank_kernel (a merge launch) and the ranking tail over its partial lists or label keys
// (enqueue_rank_tail, host_index.h).  No memset: every item key, list entry and label key is written.
static int distinct_full_pass(wdbx_index* ix, const float* queries, int nq, int k, int normalize_queries, const uint32_t* mask_words,
                              int64_t* out_idx, float* out_score) {
  int rc;
  if ((rc = ensure_label_order(ix))) return rc;
  ix->last_distinct_items = ix->lab_items;
  ix->last_distinct_labels = ix->lab_labels;
  const DistinctPlan dp = distinct_plan(ix->lab_items, ix->lab_labels, ix->lab_spans, nq, k, ix->cu_count, ix->opt_select_min_k);
  const size_t elems = (size_t)nq * k;
  if ((rc = ensure_out(ix, elems))) return rc;
  if ((rc = grow_label_scratch(ix, dp.select, dp.keys_u64, dp.rank_u64))) return rc;
  if ((rc = upload_queries(ix, queries, (uint64_t)nq, normalize_queries))) return rc;
  MaskScope scope(ix);
  if (mask_words && (rc = scope.set(mask_words))) return rc;
  const uint32_t pitch4 = (uint32_t)ix->pitch / 4;
  const label_keys_fn kfn = pick_label_keys(ix->metric, dp.qb, pitch4);
  if (!kfn) return fail(WDBX_E_STATE, "no label-keys instance with %d queries per block", dp.qb);
  const bool reg = k <= 128 && !ix->opt_lds_lists;
  const label_rank_fn rfn = pick_label_rank(dp.select ? 2 : (reg ? 1 : 0));
  if (dp.lds >= 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)rfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dp.lds));
  for (int q0 = 0; q0 < nq; q0 += dp.round) {
    const int b = std::min(dp.round, nq - q0);
    const uint32_t qblocks = (uint32_t)((b + dp.qb - 1) / dp.qb);
    if ((rc = launch_bracketed(ix, ix->scan_ev, kfn, dim3(dp.score_blocks, qblocks), 0, label_keys_args(ix, (uint64_t)q0, (uint32_t)b, pitch4))))
      return rc;
    LabelRankArgs r = {};
    r.keys = ix->d_sub_keys;
    r.key_stride = ix->lab_items;
    r.label_item0 = (const uint32_t*)(ix->d_lab + ix->lab_off_label);
    r.n_labels = ix->lab_labels;
    r.out = dp.select ? ix->d_sub_keys + dp.keys_u64 : ix->d_partials;
    r.k = k;
    if ((rc = record(ix->merge_ev, ix->profile, ix->stream, true))) return rc;
    hipLaunchKernelGGL(rfn, dim3(dp.rank_blocks, (uint32_t)b), dim3(256), dp.lds, ix->stream, r);
    HIP_TRY(hipGetLastError());
    if ((rc = record(ix->merge_ev, ix->profile, ix->stream, false))) return rc;
    if ((rc = enqueue_rank_tail(ix, label_rank_source(ix, dp.select, dp.keys_u64, dp.rank_blocks), q0, b, k, ix->metric))) return rc;
  }
  return download_results(ix, elems, out_idx, out_score);
}

// The distinct search under the handle's mutex (lk holds it; the device is set; nq, k and the buffers are checked): what
// wdbx_index_search_distinct answers and stage 1 of wdbx_index_search_groups.
static int distinct_locked(wdbx_index* ix, const float* queries, int nq, int k, int normalize_queries, const uint32_t* mask_words,
                           uint64_t mask_word_count, int64_t* out_idx, float* out_score, uint32_t* out_label,
                           std::unique_lock<std::mutex>& lk) {
  int rc;
  const size_t elems = (size_t)nq * k;
  ix->last_distinct_path = DISTINCT_NONE;
  ix->last_distinct_items = ix->last_distinct_labels = ix->last_distinct_short = 0;
  if (ix->n == 0) {  // every slot empty, as wdbx_index_search leaves them
    for (size_t i = 0; i < elems; ++i) {
      out_idx[i] = -1;
      out_score[i] = 0.0f;
      if (out_label) out_label[i] = WDBX_LABEL_NONE;
    }
    return WDBX_OK;
  }
  if (mask_words && (rc = check_mask_words(ix->n, mask_word_count))) return rc;
  if (ix->n >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "shard holds too many rows for 32-bit row keys");
  const uint32_t* const labels = ix->labels.data();
  const uint64_t n_set = std::min<uint64_t>(ix->labels.size(), ix->n);
  if (ix->labels.empty()) {  // no label was ever set: every row its own label, the ordinary search IS the answer
    if ((rc = search_host(ix, queries, nq, k, normalize_queries, mask_words, mask_word_count, out_idx, out_score, &lk))) return rc;
    if (out_label) std::fill(out_label, out_label + elems, WDBX_LABEL_NONE);
    ix->last_distinct_path = DISTINCT_OVERFETCH;
    return WDBX_OK;
  }
  // the over-fetch: the ordinary top-k', walked per query; the queries whose walk is not final are short
  const int kp = distinct_overfetch_k(ix->n, k, ix->opt_distinct_overfetch, WDBX_MAX_K);
  std::vector<int> short_q;
  if (kp) {
    std::vector<int64_t> fi((size_t)nq * kp);
    std::vector<float> fs((size_t)nq * kp);
    if ((rc = search_host(ix, queries, nq, kp, normalize_queries, mask_words, mask_word_count, fi.data(), fs.data(), &lk))) return rc;
    for (int q = 0; q < nq; ++q)
      if (!distinct_walk(fi.data() + (size_t)q * kp, fs.data() + (size_t)q * kp, kp, ix->n, labels, n_set, k, out_idx + (size_t)q * k,
                         out_score + (size_t)q * k, out_label ? out_label + (size_t)q * k : nullptr))
        short_q.push_back(q);
    if (short_q.empty()) {
      ix->last_distinct_path = DISTINCT_OVERFETCH;
      return WDBX_OK;
    }
  } else {
    short_q.resize((size_t)nq);
    for (int q = 0; q < nq; ++q) short_q[(size_t)q] = q;
  }
  ix->last_distinct_short = (int64_t)short_q.size();
  // the full pass for the short queries, gathered; their slots are overwritten
  const int ns = (int)short_q.size();
  std::vector<float> sq;
  const float* fq = queries;
  if (ns < nq) {
    sq.resize((size_t)ns * ix->dim);
    for (int i = 0; i < ns; ++i) memcpy(sq.data() + (size_t)i * ix->dim, queries + (size_t)short_q[(size_t)i] * ix->dim, (size_t)ix->dim * sizeof(float));
    fq = sq.data();
  }
  std::vector<int64_t> ri((size_t)ns * k);
  std::vector<float> rs((size_t)ns * k);
  if ((rc = distinct_full_pass(ix, fq, ns, k, normalize_queries, mask_words, ri.data(), rs.data()))) return rc;
  for (int i = 0; i < ns; ++i) {
    const size_t o = (size_t)short_q[(size_t)i] * k;
    for (int s = 0; s < k; ++s) {
      const int64_t r = ri[(size_t)i * k + s];
      out_idx[o + s] = r;
      out_score[o + s] = rs[(size_t)i * k + s];
      if (out_label) out_label[o + s] = (r >= 0 && (uint64_t)r < n_set) ? labels[r] : WDBX_LABEL_NONE;
    }
  }
  ix->last_distinct_path = kp ? DISTINCT_BOTH : DISTINCT_FULL;
  return WDBX_OK;
}

int wdbx_index_search_distinct(wdbx_index* ix, const float* queries, int nq, int k, int normalize_queries, const uint32_t* mask_words,
                               uint64_t mask_word_count, int64_t* out_idx, float* out_score, uint32_t* out_label) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 1) return fail(WDBX_E_INVALID, "nq=%d", nq);
  if (!queries || !out_idx || !out_score) return fail(WDBX_E_INVALID, "null buffer");
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  std::unique_lock<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  return distinct_locked(ix, queries, nq, k, normalize_queries, mask_words, mask_word_count, out_idx, out_score, out_label, lk);
} WDBX_CATCH

// ---- search groups: the best group_size rows of each of the k best labels (host_groups.h, kernels_groups.h, DESIGN.md
// section 4.16) ----
// Stage 2 under the handle's mutex, on a non-empty index: slots [nq * k] say what each (query, slot) ranks.  The task table is
// built on the host (groups_tasks) and served in rounds (groups_plan): per round group_members_kernel with a workgroup per task
// (bracketed as a scan launch; none when the round has no task), then group_merge_kernel with a wave per slot, which writes
// every member slot and count of the round -- no memset.  One download at the end.  out_count may be null.
static int group_members_pass(wdbx_index* ix, const float* queries, int nq, int k, int g, int normalize_queries,
                              const uint32_t* mask_words, const std::vector<GroupSlot>& slots, int64_t* out_idx, float* out_score,
                              int32_t* out_count) {
  int rc;
  std::vector<GroupTask> tasks;
  std::vector<uint64_t> slot_task0;
  groups_tasks(slots.data(), slots.size(), k, (uint32_t)ix->opt_groups_segment_rows, &tasks, &slot_task0);
  const std::vector<GroupsRound> rounds = groups_plan(slot_task0, g);
  const size_t n_slots = slots.size(), elems = n_slots * (size_t)g;
  uint64_t max_tasks = 1;
  for (const GroupsRound& r : rounds) max_tasks = std::max(max_tasks, r.tasks);
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t off_tasks = up((n_slots + 1) * sizeof(uint64_t)), off_count = off_tasks + up((size_t)max_tasks * sizeof(GroupTask));
  if ((rc = ensure_out(ix, elems))) return rc;
  if ((rc = ix->d_partials.grow((size_t)max_tasks * g * sizeof(u64)))) return rc;
  if ((rc = ix->d_grp.grow(off_count + n_slots * sizeof(int32_t)))) return rc;
  if ((rc = upload_queries(ix, queries, (uint64_t)nq, normalize_queries))) return rc;
  MaskScope scope(ix);
  if (mask_words && (rc = scope.set(mask_words))) return rc;
  u64* const d_slot_task0 = (u64*)ix->d_grp.p;
  GroupTaskDev* const d_tasks = (GroupTaskDev*)(ix->d_grp + off_tasks);
  int32_t* const d_count = (int32_t*)(ix->d_grp + off_count);
  HIP_TRY(hipMemcpyAsync(d_slot_task0, slot_task0.data(), (n_slots + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ix->stream));
  const uint32_t pitch4 = (uint32_t)ix->pitch / 4;
  const group_members_fn mfn = pick_group_members(ix->metric, pitch4);
  const group_merge_fn gfn = pick_group_merge(ix->metric);
  for (const GroupsRound& r : rounds) {
    if (r.tasks) {
      HIP_TRY(hipMemcpyAsync(d_tasks, tasks.data() + r.task0, (size_t)r.tasks * sizeof(GroupTask), hipMemcpyHostToDevice, ix->stream));
      GroupMembersArgs a = {};
      a.rows = (const f4*)ix->d_rows.p;
      a.queries = (const f4*)ix->d_q.p;
      a.order = ix->lab_valid ? (const uint32_t*)ix->d_lab.p : nullptr;
      a.mask = ix->active_mask;
      a.tasks = d_tasks;
      a.partial = ix->d_partials;
      a.pitch4 = pitch4;
      a.g = g;
      if ((rc = launch_bracketed(ix, ix->scan_ev, mfn, dim3((uint32_t)r.tasks), 0, a))) return rc;
    }
    GroupMergeArgs m = {};
    m.partial = ix->d_partials;
    m.slot_task0 = d_slot_task0 + r.slot0;
    m.task_base = r.task0;
    m.n_slots = (uint32_t)(r.slot1 - r.slot0);
    m.g = g;
    m.out_idx = ix->d_oidx + r.slot0 * (size_t)g;
    m.out_score = ix->d_oscore + r.slot0 * (size_t)g;
    m.out_count = d_count + r.slot0;
    if ((rc = launch_bracketed(ix, ix->merge_ev, gfn, dim3(r.merge_blocks), 0, m))) return rc;
  }
  ix->last_groups_path = 1;
  ix->last_groups_tasks = (int64_t)tasks.size();
  ix->last_groups_rounds = (int64_t)rounds.size();
  if (out_count) HIP_TRY(hipMemcpyAsync(out_count, d_count, n_slots * sizeof(int32_t), hipMemcpyDeviceToHost, ix->stream));
  return download_results(ix, elems, out_idx, out_score);
}

// what every (query, slot) of a call ranks, from its label and row (under the handle's mutex; builds the label order when a
// slot names a label and the handle has labels)
static int group_slots(wdbx_index* ix, const uint32_t* slot_labels, const int64_t* slot_rows, size_t n_slots, std::vector<GroupSlot>* slots) {
  int rc;
  bool any_label = false;
  for (size_t s = 0; s < n_slots && !any_label; ++s) any_label = slot_rows[s] >= 0 && slot_labels[s] != WDBX_LABEL_NONE;
  static const LabelRuns no_runs;
  const bool use = any_label && !ix->labels.empty();
  if (use && (rc = ensure_label_order(ix))) return rc;
  const LabelRuns& runs = use ? ix->lab_runs : no_runs;
  slots->resize(n_slots);
  for (size_t s = 0; s < n_slots; ++s) (*slots)[s] = groups_slot(ix->labels.data(), ix->lab_row0.data(), runs, slot_labels[s], slot_rows[s]);
  return WDBX_OK;
}

static int groups_check(const wdbx_index* ix, const float* queries, int nq, int k, int group_size, const void* out_idx, const void* out_score) {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 1) return fail(WDBX_E_INVALID, "nq=%d", nq);
  if (!queries || !out_idx || !out_score) return fail(WDBX_E_INVALID, "null buffer");
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  if (group_size < 1 || group_size > WDBX_MAX_GROUP_SIZE)
    return fail(WDBX_E_INVALID, "group_size=%d outside [1, %d]", group_size, WDBX_MAX_GROUP_SIZE);
  return WDBX_OK;
}

int wdbx_index_search_groups(wdbx_index* ix, const float* queries, int nq, int k, int group_size, int normalize_queries,
                             const uint32_t* mask_words, uint64_t mask_word_count, int64_t* out_idx, float* out_score,
                             uint32_t* out_label, int32_t* out_count) try {
  int rc;
  if ((rc = groups_check(ix, queries, nq, k, group_size, out_idx, out_score))) return rc;
  std::unique_lock<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  ix->last_groups_path = 0;
  ix->last_groups_tasks = ix->last_groups_rounds = 0;
  const size_t n_slots = (size_t)nq * k;
  // stage 1: the distinct search, through the steps its public entry runs
  std::vector<int64_t> d_idx(n_slots);
  std::vector<float> d_score(n_slots);
  std::vector<uint32_t> d_label(n_slots);
  if ((rc = distinct_locked(ix, queries, nq, k, normalize_queries, mask_words, mask_word_count, d_idx.data(), d_score.data(), d_label.data(), lk)))
    return rc;
  if (out_label) std::copy(d_label.begin(), d_label.end(), out_label);
  if (ix->n == 0) {  // every slot empty, nothing launched
    std::fill(out_idx, out_idx + n_slots * (size_t)group_size, (int64_t)-1);
    std::fill(out_score, out_score + n_slots * (size_t)group_size, 0.0f);
    if (out_count) std::fill(out_count, out_count + n_slots, 0);
    return WDBX_OK;
  }
  std::vector<GroupSlot> slots;
  if ((rc = group_slots(ix, d_label.data(), d_idx.data(), n_slots, &slots))) return rc;
  return group_members_pass(ix, queries, nq, k, group_size, normalize_queries, mask_words, slots, out_idx, out_score, out_count);
} WDBX_CATCH

int wdbx_index_search_group_members(wdbx_index* ix, const float* queries, int nq, int k, int group_size, int normalize_queries,
                                    const uint32_t* mask_words, uint64_t mask_word_count, const uint32_t* slot_labels,
                                    const int64_t* slot_rows, int64_t* out_idx, float* out_score, int32_t* out_count) try {
  int rc;
  if ((rc = groups_check(ix, queries, nq, k, group_size, out_idx, out_score))) return rc;
  if (!slot_labels || !slot_rows) return fail(WDBX_E_INVALID, "null slot buffer");
  std::unique_lock<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  ix->last_groups_path = 0;
  ix->last_groups_tasks = ix->last_groups_rounds = 0;
  const size_t n_slots = (size_t)nq * k;
  for (size_t s = 0; s < n_slots; ++s)
    if (slot_rows[s] >= 0 && (uint64_t)slot_rows[s] >= ix->n)
      return fail(WDBX_E_INVALID, "slot %llu: row %lld of %llu stored rows", (u64)s, (long long)slot_rows[s], (u64)ix->n);
  if (ix->n == 0) {  // (every slot is unused then)
    std::fill(out_idx, out_idx + n_slots * (size_t)group_size, (int64_t)-1);
    std::fill(out_score, out_score + n_slots * (size_t)group_size, 0.0f);
    if (out_count) std::fill(out_count, out_count + n_slots, 0);
    return WDBX_OK;
  }
  if (mask_words && (rc = check_mask_words(ix->n, mask_word_count))) return rc;
  if (ix->n >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "shard holds too many rows for 32-bit row keys");
  std::vector<GroupSlot> slots;
  if ((rc = group_slots(ix, slot_labels, slot_rows, n_slots, &slots))) return rc;
  return group_members_pass(ix, queries, nq, k, group_size, normalize_queries, mask_words, slots, out_idx, out_score, out_count);
} WDBX_CATCH

// ---- multi-vector search: labels ranked by the sum of per-vector best scores (host_multivector.h, kernels_multivector.h,
// DESIGN.md section 4.12) ----
// Under the handle's mutex to its end.  Per round of vectors (multivector_plan): label_keys_kernel with the round's vectors as
// its queries (bracketed as a scan launch), multivector_rank_kernel over the round's segments and, for the segments that end a
// query, merge_kernel over their partial lists or per query the radix-select chain over its label keys (bracketed as merge
// launches).  No memset: every item key, accumulator entry, list entry and label key that is read has been written.
int wdbx_index_search_multivector(wdbx_index* ix, const float* vectors, const uint64_t* vector_offsets, int nq, int k,
                                  int normalize_queries, const uint32_t* mask_words, uint64_t mask_word_count, int64_t* out_idx,
                                  float* out_score, uint32_t* out_label) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 1) return fail(WDBX_E_INVALID, "nq=%d", nq);
  if (!vectors || !vector_offsets || !out_idx || !out_score) return fail(WDBX_E_INVALID, "null buffer");
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  if (vector_offsets[0] != 0) return fail(WDBX_E_INVALID, "vector_offsets[0]=%llu, not 0", (u64)vector_offsets[0]);
  for (int q = 0; q < nq; ++q) {
    if (vector_offsets[q + 1] <= vector_offsets[q]) return fail(WDBX_E_INVALID, "query %d has no vector", q);
    if (vector_offsets[q + 1] - vector_offsets[q] > WDBX_MAX_QUERY_VECTORS)
      return fail(WDBX_E_INVALID, "query %d has %llu vectors, more than %d", q, (u64)(vector_offsets[q + 1] - vector_offsets[q]), WDBX_MAX_QUERY_VECTORS);
  }
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  int rc;
  const size_t elems = (size_t)nq * k;
  ix->last_multivector_rounds = ix->last_multivector_vectors = ix->last_multivector_labels = 0;
  if (ix->n == 0) {  // every slot empty, nothing launched
    for (size_t i = 0; i < elems; ++i) {
      out_idx[i] = -1;
      out_score[i] = 0.0f;
      if (out_label) out_label[i] = WDBX_LABEL_NONE;
    }
    return WDBX_OK;
  }
  if (mask_words && (rc = check_mask_words(ix->n, mask_word_count))) return rc;
  if (ix->n >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "shard holds too many rows for 32-bit row keys");
  if ((rc = ensure_label_order(ix))) return rc;
  const uint64_t total = vector_offsets[nq];
  const MultivectorPlan mp = multivector_plan(vector_offsets, nq, ix->lab_items, ix->lab_labels, ix->lab_spans, k, ix->cu_count,
                                              ix->opt_select_min_k, ix->opt_multivector_round_vectors);
  if ((rc = ensure_out(ix, elems))) return rc;
  if ((rc = grow_label_scratch(ix, mp.select, mp.keys_u64, mp.rank_u64))) return rc;
  const size_t acc_bytes = ((size_t)ix->lab_labels * sizeof(float) + 255) / 256 * 256;
  const size_t seg_bytes = mp.segments.size() * sizeof(MultivectorSegment);
  if ((rc = ix->d_mv.grow(acc_bytes + seg_bytes))) return rc;
  const MultivectorSegment* const d_segs = (const MultivectorSegment*)(ix->d_mv + acc_bytes);
  HIP_TRY(hipMemcpyAsync(ix->d_mv + acc_bytes, mp.segments.data(), seg_bytes, hipMemcpyHostToDevice, ix->stream));
  if ((rc = upload_queries(ix, vectors, total, normalize_queries))) return rc;
  MaskScope scope(ix);
  if (mask_words && (rc = scope.set(mask_words))) return rc;
  const uint32_t pitch4 = (uint32_t)ix->pitch / 4;
  const label_keys_fn kfn = pick_label_keys(ix->metric, mp.qb, pitch4);
  if (!kfn) return fail(WDBX_E_STATE, "no label-keys instance with %d vectors per block", mp.qb);
  const bool reg = k <= 128 && !ix->opt_lds_lists;
  const multivector_rank_fn rfn = pick_multivector_rank(mp.select ? 2 : (reg ? 1 : 0));
  if (mp.lds >= 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)rfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mp.lds));
  for (const MultivectorRound& r : mp.rounds) {
    const uint32_t vblocks = (r.vectors + (uint32_t)mp.qb - 1) / (uint32_t)mp.qb;
    const uint32_t sblocks = r.vectors == (uint32_t)mp.round_max ? mp.score_blocks
                                                                 : multivector_score_blocks(r.vectors, mp.qb, ix->lab_spans, ix->cu_count);
    if ((rc = launch_bracketed(ix, ix->scan_ev, kfn, dim3(sblocks, vblocks), 0, label_keys_args(ix, r.first, r.vectors, pitch4)))) return rc;
    MultivectorRankArgs m = {};
    m.keys = ix->d_sub_keys;
    m.key_stride = ix->lab_items;
    m.label_item0 = (const uint32_t*)(ix->d_lab + ix->lab_off_label);
    m.n_labels = ix->lab_labels;
    m.acc = (float*)ix->d_mv.p;
    m.out = mp.select ? ix->d_sub_keys + mp.keys_u64 : ix->d_partials;
    m.k = k;
    // a first segment that reads the accumulator and a LAST one that writes it must not share a launch: the writer goes second
    const MultivectorSegment& s_first = mp.segments[r.seg0];
    const MultivectorSegment& s_last = mp.segments[r.seg0 + r.segs - 1];
    const bool split = r.segs > 1 && (s_first.carry & MV_CARRY_IN) && (s_last.carry & MV_CARRY_OUT);
    if ((rc = record(ix->merge_ev, ix->profile, ix->stream, true))) return rc;
    m.segs = d_segs + r.seg0;
    hipLaunchKernelGGL(rfn, dim3(mp.rank_blocks, r.segs - (split ? 1u : 0u)), dim3(256), mp.lds, ix->stream, m);
    HIP_TRY(hipGetLastError());
    if (split) {
      m.segs = d_segs + r.seg0 + r.segs - 1;
      hipLaunchKernelGGL(rfn, dim3(mp.rank_blocks, 1), dim3(256), mp.lds, ix->stream, m);
      HIP_TRY(hipGetLastError());
    }
    if ((rc = record(ix->merge_ev, ix->profile, ix->stream, false))) return rc;
    if (!r.ranked) continue;
    const RankSource src = label_rank_source(ix, mp.select, mp.keys_u64, mp.rank_blocks);
    if ((rc = enqueue_rank_tail(ix, src, (int)r.ranked_query0, (int)r.ranked, k, ix->metric))) return rc;
  }
  if ((rc = download_results(ix, elems, out_idx, out_score))) return rc;
  // label positions -> (smallest row of the label, its stored label)
  const uint64_t n_set = std::min<uint64_t>(ix->labels.size(), ix->n);
  for (size_t i = 0; i < elems; ++i) {
    uint32_t lab = WDBX_LABEL_NONE;
    if (out_idx[i] >= 0) {
      const uint32_t row = ix->lab_row0[(size_t)out_idx[i]];
      out_idx[i] = (int64_t)row;
      if (row < n_set) lab = ix->labels[row];
    }
    if (out_label) out_label[i] = lab;
  }
  ix->last_multivector_rounds = (int64_t)mp.rounds.size();
  ix->last_multivector_vectors = (int64_t)total;
  ix->last_multivector_labels = ix->lab_labels;
  return WDBX_OK;
} WDBX_CATCH

// ---- MMR search: a diversified top-k picked greedily from the pool of the best rows (host_mmr.h, kernels_mmr.h, DESIGN.md
// section 4.14) ----
// Under the handle's mutex to its end.  The pool is the ordinary search for k' = fetch_k (search_host under the lock this call
// took, as the distinct search's over-fetch); its row numbers and scores come back to the host, where the pools are measured and
// the rounds planned (mmr_plan_rounds), and go up again per round as the gather's list and the relevance table.  Per round:
// gather_rows_kernel into the round's contiguous rows, mmr_pairs_kernel (bracketed as a scan launch), mmr_select_kernel
// (bracketed as a merge launch).  No memset: every word of G that is read and every output slot has been written.
int wdbx_index_search_mmr(wdbx_index* ix, const float* queries, int nq, int k, int fetch_k, float lambda, int normalize_queries,
                          const uint32_t* mask_words, uint64_t mask_word_count, int64_t* out_idx, float* out_score,
                          float* out_mmr) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  const MmrArg bad = mmr_check_args(nq, k, fetch_k, lambda, queries && out_idx && out_score, WDBX_MAX_K);
  if (bad != MMR_ARG_OK) return fail(WDBX_E_INVALID, "%s (nq=%d k=%d fetch_k=%d lambda=%g)", mmr_arg_message(bad), nq, k, fetch_k, (double)lambda);
  std::unique_lock<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  int rc;
  const size_t elems = (size_t)nq * k;
  ix->last_mmr_path = 0;
  ix->last_mmr_rounds = ix->last_mmr_candidates = 0;
  if (ix->n == 0) {  // every slot empty, nothing launched
    for (size_t i = 0; i < elems; ++i) {
      out_idx[i] = -1;
      out_score[i] = 0.0f;
      if (out_mmr) out_mmr[i] = 0.0f;
    }
    return WDBX_OK;
  }
  if (mask_words && (rc = check_mask_words(ix->n, mask_word_count))) return rc;
  // the pool: the exact top-fetch_k, on the host
  std::vector<int64_t> fi((size_t)nq * fetch_k);
  std::vector<float> fs((size_t)nq * fetch_k);
  if ((rc = search_host(ix, queries, nq, fetch_k, normalize_queries, mask_words, mask_word_count, fi.data(), fs.data(), &lk))) return rc;
  const bool l2 = ix->metric == WDBX_METRIC_L2;
  const uint32_t pitch4 = (uint32_t)ix->pitch / 4;
  std::vector<uint32_t> m((size_t)nq);
  uint64_t total = 0;
  for (int q = 0; q < nq; ++q) total += m[(size_t)q] = mmr_pool_size(fi.data() + (size_t)q * fetch_k, fetch_k);
  const std::vector<MmrRound> rounds = mmr_plan_rounds(m.data(), nq, pitch4, (uint64_t)ix->opt_mmr_scratch_mib << 20);
  // the largest round's layout: table | candidates | relevance | values | rows | G, each part on a 256-byte boundary
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  size_t max_nq = 0, max_rows = 0, max_g = 0;
  for (const MmrRound& r : rounds) {
    max_nq = std::max<size_t>(max_nq, r.nq);
    max_rows = std::max<size_t>(max_rows, (size_t)r.rows);
    max_g = std::max<size_t>(max_g, (size_t)r.g_floats);
  }
  const size_t off_cand = up(max_nq * sizeof(MmrQuery)), off_rel = off_cand + up(max_rows * sizeof(u64)),
               off_val = off_rel + up(max_rows * sizeof(float)), off_rows = off_val + up(max_nq * (size_t)k * sizeof(float)),
               off_g = off_rows + up(max_rows * (size_t)pitch4 * sizeof(f4)), need = off_g + up(max_g * sizeof(float));
  if ((rc = ix->d_mmr.grow(need))) return rc;
  if ((rc = ensure_out(ix, max_nq * (size_t)k))) return rc;
  const mmr_pairs_fn pfn = pick_mmr_pairs(ix->metric, pitch4);
  std::vector<MmrQuery> table;
  std::vector<u64> cand;
  std::vector<float> rel;
  for (const MmrRound& r : rounds) {
    mmr_round_queries(m.data(), r, &table);
    cand.clear();
    rel.clear();
    for (uint32_t i = 0; i < r.nq; ++i) {
      const size_t at = (size_t)(r.q0 + i) * fetch_k;
      for (uint32_t c = 0; c < m[r.q0 + i]; ++c) {
        cand.push_back((u64)fi[at + c]);
        rel.push_back(l2 ? -fs[at + c] : fs[at + c]);
      }
    }
    const MmrQuery* const d_table = (const MmrQuery*)ix->d_mmr.p;
    u64* const d_cand = (u64*)(ix->d_mmr + off_cand);
    float* const d_rel = (float*)(ix->d_mmr + off_rel);
    float* const d_val = (float*)(ix->d_mmr + off_val);
    f4* const d_gathered = (f4*)(ix->d_mmr + off_rows);
    float* const d_g = (float*)(ix->d_mmr + off_g);
    HIP_TRY(hipMemcpyAsync(ix->d_mmr, table.data(), table.size() * sizeof(MmrQuery), hipMemcpyHostToDevice, ix->stream));
    if (r.rows) {
      HIP_TRY(hipMemcpyAsync(d_cand, cand.data(), cand.size() * sizeof(u64), hipMemcpyHostToDevice, ix->stream));
      HIP_TRY(hipMemcpyAsync(d_rel, rel.data(), rel.size() * sizeof(float), hipMemcpyHostToDevice, ix->stream));
      if ((rc = record(ix->scan_ev, ix->profile, ix->stream, true))) return rc;
      hipLaunchKernelGGL(gather_rows_kernel, dim3(mmr_gather_grid(r.rows)), dim3(256), 0, ix->stream, (const f4*)ix->d_rows.p, pitch4,
                         (const u64*)d_cand, (u64)r.rows, d_gathered);
      HIP_TRY(hipGetLastError());
      MmrPairsArgs pa = {};
      pa.rows = d_gathered;
      pa.qs = d_table;
      pa.G = d_g;
      pa.pitch4 = pitch4;
      const MmrGrid pg = mmr_pairs_grid(r);
      hipLaunchKernelGGL(pfn, dim3(pg.x, pg.y, pg.z), dim3(256), 0, ix->stream, pa);
      HIP_TRY(hipGetLastError());
      if ((rc = record(ix->scan_ev, ix->profile, ix->stream, false, 2))) return rc;
    }
    MmrSelectArgs sa = {};
    sa.qs = d_table;
    sa.G = d_g;
    sa.cand = d_cand;
    sa.rel = d_rel;
    sa.out_idx = ix->d_oidx;
    sa.out_score = ix->d_oscore;
    sa.out_mmr = d_val;
    sa.lambda = lambda;
    sa.k = k;
    sa.negate = l2 ? 1 : 0;
    if ((rc = launch_bracketed(ix, ix->merge_ev, mmr_select_kernel, dim3(r.nq), 0, sa))) return rc;
    const size_t o = (size_t)r.q0 * k, e = (size_t)r.nq * k;
    if (out_mmr) HIP_TRY(hipMemcpyAsync(out_mmr + o, d_val, e * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
    if ((rc = download_results(ix, e, out_idx + o, out_score + o))) return rc;  // (waits: the host tables are rebuilt for the next round)
  }
  ix->last_mmr_path = 1;
  ix->last_mmr_rounds = (int64_t)rounds.size();
  ix->last_mmr_candidates = (int64_t)total;
  return WDBX_OK;
} WDBX_CATCH

// ---- recommend search: rows ranked by positive and negative examples (host_recommend.h, kernels_recommend.h, DESIGN.md
// section 4.15) ----------------------------------------------------------------------------------------------------------
// The whole call holds the handle's mutex.  The offsets need no lock; the mask's length and the exclusion list are checked
// against the row count under it.  Then recommend_locked (host_index.h): the favoured pass for all queries, the disfavoured
// pass for the short ones, the splice.
int wdbx_index_search_recommend(wdbx_index* ix, const float* examples, const uint64_t* example_offsets, int nq, int k,
                                int normalize_examples, const uint32_t* mask_words, uint64_t mask_word_count,
                                const uint64_t* exclude_rows, uint64_t n_exclude, int64_t* out_idx, float* out_score,
                                uint8_t* out_side) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 1) return fail(WDBX_E_INVALID, "nq=%d", nq);
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  if (!examples || !example_offsets || !out_idx || !out_score) return fail(WDBX_E_INVALID, "null buffer");
  if (n_exclude && !exclude_rows) return fail(WDBX_E_INVALID, "exclude_rows is null");
  std::string msg;
  if (!recommend_validate_offsets(example_offsets, nq, &msg)) return fail(WDBX_E_INVALID, "%s", msg.c_str());
  std::unique_lock<std::mutex> lk(ix->mu);
  if (ix->n >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "shard holds too many rows for 32-bit row keys");
  if (mask_words) {
    const int rc = check_mask_words(ix->n, mask_word_count);
    if (rc) return rc;
  }
  std::vector<uint32_t> exclude32((size_t)std::min<uint64_t>(n_exclude, RECOMMEND_MAX_EXCLUDE));
  if (!recommend_validate_exclude(exclude_rows, n_exclude, ix->n, exclude32.data(), &msg)) return fail(WDBX_E_INVALID, "%s", msg.c_str());
  ix->last_recommend_path = 0;
  ix->last_recommend_short = 0;
  if (ix->n == 0) {  // every slot empty, nothing launched
    for (size_t i = 0; i < (size_t)nq * k; ++i) {
      out_idx[i] = -1;
      out_score[i] = 0.0f;
      if (out_side) out_side[i] = 0;
    }
    return WDBX_OK;
  }
  DeviceGuard g(ix->device);
  MaskScope scope(ix);
  return recommend_locked(ix, examples, example_offsets, nq, k, normalize_examples, mask_words, exclude32, scope, out_idx, out_score,
                          out_side);
} WDBX_CATCH

// ---- discovery search: rows ranked by context pairs and a target (host_discover.h, kernels_discover.h, DESIGN.md section
// 4.17) ------------------------------------------------------------------------------------------------------------------
// The whole call holds the handle's mutex.  The offsets need no lock; the mask's length and the exclusion list are checked
// against the row count under it.  Then discover_locked (host_index.h).
int wdbx_index_search_discover(wdbx_index* ix, const float* targets, const float* context, const uint64_t* pair_offsets, int nq, int k,
                               int normalize_vectors, const uint32_t* mask_words, uint64_t mask_word_count,
                               const uint64_t* exclude_rows, uint64_t n_exclude, int64_t* out_idx, float* out_score,
                               uint8_t* out_wins) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 1) return fail(WDBX_E_INVALID, "nq=%d", nq);
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  if (!pair_offsets || !out_idx || !out_score) return fail(WDBX_E_INVALID, "null buffer");
  if (n_exclude && !exclude_rows) return fail(WDBX_E_INVALID, "exclude_rows is null");
  std::string msg;
  if (!discover_validate_offsets(pair_offsets, nq, targets != nullptr, &msg)) return fail(WDBX_E_INVALID, "%s", msg.c_str());
  if (pair_offsets[nq] && !context) return fail(WDBX_E_INVALID, "null buffer: context");
  std::unique_lock<std::mutex> lk(ix->mu);
  if (ix->n >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "shard holds too many rows for 32-bit row keys");
  if (mask_words) {
    const int rc = check_mask_words(ix->n, mask_word_count);
    if (rc) return rc;
  }
  std::vector<uint32_t> exclude32((size_t)std::min<uint64_t>(n_exclude, RECOMMEND_MAX_EXCLUDE));
  if (!recommend_validate_exclude(exclude_rows, n_exclude, ix->n, exclude32.data(), &msg)) return fail(WDBX_E_INVALID, "%s", msg.c_str());
  ix->last_discover_path = 0;
  ix->last_discover_zone_slots = 0;
  if (ix->n == 0) {  // every slot empty, nothing launched
    for (size_t i = 0; i < (size_t)nq * k; ++i) {
      out_idx[i] = -1;
      out_score[i] = 0.0f;
      if (out_wins) out_wins[i] = 0;
    }
    return WDBX_OK;
  }
  DeviceGuard g(ix->device);
  MaskScope scope(ix);
  return discover_locked(ix, targets, context, pair_offsets, nq, k, normalize_vectors, mask_words, exclude32, scope, out_idx, out_score,
                         out_wins);
} WDBX_CATCH

// ---- range search (range_u8_eligible: host_index.h; pick_range_scan: kernels_range.h) --------------
// The whole call holds the handle's mutex (like a masked search: the key buffers are the handle's).  Per round of up to 64
// queries: [u8 path: memset counters, scan8_kernel<PHASE 2> -> candidates] -> memset, range_filter_kernel / range_scan_kernel
// -> result keys; one synchronisation reads both counters.  A counter past its buffer (the counters count on) grows that
// buffer to the exact count and the overflowed stage runs again -- once: the same inputs give the same count (a candidate
// overflow reruns the filter too, whose input was cut).  Then the keys go to the caller's row array at their CSR offsets and
// range_sort_decode (host_range.h) sorts and decodes them there.
// (the argument checks and the body under the lock are functions of their own: wdbx_index_range_search_batch makes the same
// checks and runs the same rounds for the queries its tile blocks do not answer, under the lock IT took)
static int range_check_args(wdbx_index* ix, const float* queries, int nq, const float* thresholds, uint64_t capacity,
                            uint64_t* out_offsets, int64_t* out_rows, float* out_scores) {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 1) return fail(WDBX_E_INVALID, "nq=%d", nq);
  if (!queries || !thresholds || !out_offsets) return fail(WDBX_E_INVALID, "null buffer");
  if (capacity && (!out_rows || !out_scores)) return fail(WDBX_E_INVALID, "capacity %llu without result buffers", (u64)capacity);
  for (int q = 0; q < nq; ++q)
    if (thresholds[q] != thresholds[q]) return fail(WDBX_E_INVALID, "threshold of query %d is NaN", q);
  return WDBX_OK;
}
static int range_search_locked(wdbx_index* ix, const float* queries, int nq, const float* thresholds, int normalize_queries,
                               const uint32_t* mask_words, uint64_t mask_word_count, uint64_t capacity, uint64_t* out_offsets,
                               int64_t* out_rows, float* out_scores) {
  MaskScope scope(ix);
  int rc;
  out_offsets[0] = 0;
  if (ix->n == 0) {
    for (int q = 0; q < nq; ++q) out_offsets[q + 1] = 0;
    return WDBX_OK;
  }
  if (mask_words && ((rc = check_mask_words(ix->n, mask_word_count)) || (rc = scope.set(mask_words)))) return rc;
  if ((rc = upload_queries(ix, queries, (uint64_t)nq, normalize_queries))) return rc;
  const bool l2 = ix->metric == WDBX_METRIC_L2;
  const bool u8 = range_u8_eligible(ix) && prepare_u8_shadow(ix);
  if (u8 && l2 && (rc = ensure_row_norms(ix))) return rc;
  ix->last_range_path = u8 ? 2 : 0;
  constexpr int ROUND = 64;
  if ((rc = ix->d_rcnt.grow(2 * ROUND * sizeof(uint32_t)))) return rc;
  if ((rc = ix->d_rthr.grow(2 * ROUND * sizeof(float)))) return rc;
  const uint32_t pitch4 = (uint32_t)ix->pitch / 4;
  const Scan8Shape* sh = u8 ? scan8_shape((uint32_t)ix->dim) : nullptr;
  const scan8_fn f2 = !u8 ? nullptr : l2 ? pick_scan8<2, WDBX_METRIC_L2>(sh->L, sh->QPL) : pick_scan8<2, WDBX_METRIC_COSINE>(sh->L, sh->QPL);
  if (u8 && !f2) return fail(WDBX_E_STATE, "no u8 range instance for %d lanes x %d loads", sh->L, sh->QPL);
  const range_fn fscan = l2 ? pick_range_scan<WDBX_METRIC_L2>(pitch4) : pick_range_scan<WDBX_METRIC_COSINE>(pitch4);
  const range_fn ffilter = l2 ? range_filter_kernel<WDBX_METRIC_L2> : range_filter_kernel<WDBX_METRIC_COSINE>;
  std::vector<float> hthr(2 * ROUND);
  std::vector<uint32_t> hcnt(2 * ROUND);
  std::vector<uint64_t> cnt(ROUND);

  for (int q0 = 0; q0 < nq; q0 += ROUND) {
    const int nv = std::min(ROUND, nq - q0);
    const float* dq = ix->d_q + (size_t)q0 * ix->pitch;
    for (int i = 0; i < nv; ++i) {
      const float t = thresholds[q0 + i];
      hthr[i] = t;
      if (l2) {
        double qq = 0.0;
        for (int c = 0; c < ix->dim; ++c) qq += (double)queries[(size_t)(q0 + i) * ix->dim + c] * queries[(size_t)(q0 + i) * ix->dim + c];
        hthr[ROUND + i] = range_selection_tau_l2(qq, t);
      } else {
        hthr[ROUND + i] = t;  // (the rounding of the exact pass is added to the bound inside the scan)
      }
    }
    HIP_TRY(hipMemcpyAsync(ix->d_rthr, hthr.data(), 2 * ROUND * sizeof(float), hipMemcpyHostToDevice, ix->stream));
    auto enqueue_select = [&]() -> int {  // u8 path: the candidates
      const uint32_t cap = ix->range_cand_cap;
      int rc2 = ix->d_rcand.grow((size_t)nv * cap * sizeof(u64));
      if (rc2) return rc2;
      HIP_TRY(hipMemsetAsync(ix->d_rcnt, 0, (size_t)nv * sizeof(uint32_t), ix->stream));
      Scan8Args a = {};
      a.rows8 = (const u4v*)ix->d_rows8.p;
      a.scale = ix->d_scale8;
      a.cn = ix->d_cn;
      a.query = (const f4*)dq;
      a.mask = ix->active_mask;
      a.n_rows = (uint32_t)ix->n;
      a.pieces = sh->pieces;
      a.qquads = pitch4;
      a.tau = ix->d_rthr + ROUND;
      a.cand = ix->d_rcand;
      a.count = ix->d_rcnt;
      a.cap = cap;
      const uint32_t groups1 = (uint32_t)((ix->n + (64 / sh->L) - 1) / (64 / sh->L));
      const uint32_t grid1 = std::min<uint32_t>((groups1 + 3) / 4, (uint32_t)ix->cu_count * 2);
      if ((rc2 = record(ix->scan_ev, ix->profile, ix->stream, true))) return rc2;
      hipLaunchKernelGGL(f2, dim3(grid1, nv), dim3(256), 0, ix->stream, a);
      HIP_TRY(hipGetLastError());
      return record(ix->scan_ev, ix->profile, ix->stream, false, (uint32_t)nv);
    };
    auto enqueue_out = [&]() -> int {  // the exact pass: result keys
      const uint32_t cap = u8 ? ix->range_cand_cap : ix->range_out_cap;  // (u8: results <= candidates, never past the buffer)
      int rc2 = ix->d_rkeys.grow((size_t)nv * cap * sizeof(u64));
      if (rc2) return rc2;
      HIP_TRY(hipMemsetAsync(ix->d_rcnt + ROUND, 0, (size_t)nv * sizeof(uint32_t), ix->stream));
      RangeArgs r = {};
      r.rows = (const f4*)ix->d_rows.p;
      r.queries = (const f4*)dq;
      r.thr = ix->d_rthr;
      r.mask = ix->active_mask;
      r.n_rows = (uint32_t)ix->n;
      r.pitch4 = pitch4;
      r.out = ix->d_rkeys;
      r.count = ix->d_rcnt + ROUND;
      r.cap = cap;
      r.cand = ix->d_rcand;
      r.cand_count = ix->d_rcnt;
      r.cand_cap = ix->range_cand_cap;
      EventPool& ev = u8 ? ix->merge_ev : ix->scan_ev;
      if ((rc2 = record(ev, ix->profile, ix->stream, true))) return rc2;
      if (u8) {
        hipLaunchKernelGGL(ffilter, dim3((uint32_t)ix->cu_count * 8, nv), dim3(256), 0, ix->stream, r);
      } else {
        uint32_t P = 1;  // (lanes per row, as pick_range_scan chose them)
        while (P < pitch4 && P < 64) P <<= 1;
        const uint64_t groups = (ix->n + (64 / P) - 1) / (64 / P);
        const uint32_t grid = (uint32_t)std::min<uint64_t>((groups + 3) / 4, (uint64_t)ix->cu_count * 8);
        hipLaunchKernelGGL(fscan, dim3(grid, nv), dim3(256), 0, ix->stream, r);
      }
      HIP_TRY(hipGetLastError());
      return record(ev, ix->profile, ix->stream, false, (uint32_t)nv);
    };
    auto read_counts = [&]() -> int {
      HIP_TRY(hipMemcpyAsync(hcnt.data(), ix->d_rcnt, 2 * ROUND * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
      HIP_TRY(hipStreamSynchronize(ix->stream));
      return WDBX_OK;
    };
    auto max_of = [&](int base) {
      uint32_t m = 0;
      for (int i = 0; i < nv; ++i) m = std::max(m, hcnt[base + i]);
      return m;
    };
    if (u8 && (rc = enqueue_select())) return rc;
    if ((rc = enqueue_out()) || (rc = read_counts())) return rc;
    if (u8 && max_of(0) > ix->range_cand_cap) {  // candidates past their buffer: grow to the exact count, select + filter again
      ix->range_cand_cap = max_of(0);
      if ((rc = enqueue_select()) || (rc = enqueue_out()) || (rc = read_counts())) return rc;
      if (max_of(0) > ix->range_cand_cap) return fail(WDBX_E_STATE, "range search: candidate count changed between two passes");
    }
    if (!u8 && max_of(ROUND) > ix->range_out_cap) {  // results past their buffer: grow, the scan again
      ix->range_out_cap = max_of(ROUND);
      if ((rc = enqueue_out()) || (rc = read_counts())) return rc;
      if (max_of(ROUND) > ix->range_out_cap) return fail(WDBX_E_STATE, "range search: result count changed between two passes");
    }
    for (int i = 0; i < nv; ++i) cnt[i] = hcnt[ROUND + i];
    const uint64_t total = range_csr_offsets(cnt.data(), nv, out_offsets + q0);
    if (total <= capacity) {  // the keys, straight into the caller's row array at their offsets (u64 slots)
      const uint32_t cap = u8 ? ix->range_cand_cap : ix->range_out_cap;
      for (int i = 0; i < nv; ++i)
        if (cnt[i])
          HIP_TRY(hipMemcpyAsync(out_rows + out_offsets[q0 + i], ix->d_rkeys + (size_t)i * cap, cnt[i] * sizeof(u64),
                                 hipMemcpyDeviceToHost, ix->stream));
      HIP_TRY(hipStreamSynchronize(ix->stream));
    }
  }
  if (out_offsets[nq] <= capacity) range_sort_decode(l2 ? 1 : 0, nq, out_offsets, out_rows, out_scores);
  return WDBX_OK;
}

static int range_search_host(wdbx_index* ix, const float* queries, int nq, const float* thresholds, int normalize_queries,
                             const uint32_t* mask_words, uint64_t mask_word_count, uint64_t capacity, uint64_t* out_offsets,
                             int64_t* out_rows, float* out_scores) {
  const int rc = range_check_args(ix, queries, nq, thresholds, capacity, out_offsets, out_rows, out_scores);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  return range_search_locked(ix, queries, nq, thresholds, normalize_queries, mask_words, mask_word_count, capacity, out_offsets,
                             out_rows, out_scores);
}

int wdbx_index_range_search(wdbx_index* ix, const float* queries, int nq, const float* thresholds, int normalize_queries,
                            const uint32_t* mask_words, uint64_t mask_word_count, uint64_t capacity, uint64_t* out_offsets,
                            int64_t* out_rows, float* out_scores) try {
  return range_search_host(ix, queries, nq, thresholds, normalize_queries, mask_words, mask_word_count, capacity, out_offsets,
                           out_rows, out_scores);
} WDBX_CATCH

// ---- batched range search (host_range_batch.h, kernels_range_batch.h) ------------------------
// One full pass of the int8 tiles per block of up to 256 queries instead of one u8 scan per query.  Per block, all on the
// handle's stream: queries_to_i8_kernel -> range_batch_bound_kernel (tau per query, the bound widened by the exact pass's own
// rounding, result counters zeroed) -> gemm_i8_kernel<PHASE 1> -> scatter_pairs_kernel -> range_filter_kernel; one
// synchronisation reads the candidate counters, the lost flag and the result counters.  A candidate counter past its buffer
// grows the buffers to the exact count and runs scatter + filter again, once.  A wave that ran out of pair room (nobody knows
// which query lost pairs) sends the block's queries through range_search_locked: the per-query rounds, under this call's lock.
// The whole call holds the handle's mutex.
// staged_q0: the caller's query that sits first in d_q (the queries are staged again, from the next block on, after a block
// that went through the per-query rounds)
static int range_batch_block(wdbx_index* ix, const RangeBatchBlock& b, int staged_q0, const float* queries, const float* thresholds,
                             const u64* gbad, uint32_t pair_cap, uint32_t nwaves, std::vector<uint32_t>& hcand, std::vector<uint32_t>& hres,
                             bool* lost) {
  int rc;
  const bool l2 = ix->metric == WDBX_METRIC_L2, masked = ix->active_mask != nullptr;
  const int gbn = 64 * b.ct, nv = b.nv;
  const uint32_t pitch8 = ix->pitch8g, pitch4 = (uint32_t)ix->pitch / 4;
  const uint32_t tiles = (uint32_t)((ix->n + G8_ROWS - 1) / G8_ROWS);
  const float* qsrc = ix->d_q + (size_t)(b.q0 - staged_q0) * ix->pitch;
  constexpr int MB = RANGE_BATCH_MAX_BLOCK;
  const RangeBatchSizes sz = range_batch_sizes(b, ix->range_batch_cap, pair_cap, nwaves, pitch8);
  if ((rc = ix->d_qb8.grow(sz.qb8_bytes))) return rc;
  if ((rc = ix->d_qpar.grow(sz.qpar_bytes))) return rc;
  if ((rc = ix->d_tau.grow(sz.tau_bytes))) return rc;
  if ((rc = ix->d_count.grow(sz.count_bytes))) return rc;
  if ((rc = ix->d_pairs.grow(sz.pairs_bytes))) return rc;
  if ((rc = ix->d_pair_count.grow(sz.pair_count_bytes))) return rc;
  if ((rc = ix->d_rcnt.grow(sz.rcnt_bytes))) return rc;
  if ((rc = ix->d_rthr.grow(sz.thr_bytes))) return rc;
  uint32_t* const d_lost = ix->d_count + MB;
  // the exact thresholds [0, 256) and the selection thresholds [256, 512)
  std::vector<float> hthr(2 * MB, INFINITY);
  for (int i = 0; i < nv; ++i) {
    const float t = thresholds[b.q0 + i];
    hthr[i] = t;
    if (l2) {
      const float* qv = queries + (size_t)(b.q0 + i) * ix->dim;
      double qq = 0.0;
      for (int c = 0; c < ix->dim; ++c) qq += (double)qv[c] * qv[c];
      hthr[MB + i] = range_selection_tau_l2(qq, t);
    } else {
      hthr[MB + i] = t;  // (the rounding of the exact pass widens the bound: range_batch_bound_kernel)
    }
  }
  HIP_TRY(hipMemcpyAsync(ix->d_rthr, hthr.data(), 2 * MB * sizeof(float), hipMemcpyHostToDevice, ix->stream));
  hipLaunchKernelGGL(queries_to_i8_kernel, dim3(queries_to_i8_grid((uint32_t)gbn)), dim3(256), 0, ix->stream, qsrc, (uint32_t)ix->dim,
                     (uint32_t)ix->pitch, (uint32_t)nv, ix->d_qb8, pitch8, (uint32_t)gbn, ix->d_qpar, ix->d_tau, ix->d_count, d_lost);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(range_batch_bound_kernel, dim3(range_batch_bound_grid((uint32_t)gbn)), dim3(256), 0, ix->stream, (uint32_t)nv,
                     (uint32_t)gbn, ix->d_qpar, (const float*)(ix->d_rthr + MB), ix->d_tau, ix->d_rcnt);
  HIP_TRY(hipGetLastError());
  Gemm8Args g = {};
  g.rows8 = ix->d_rows8g;
  g.groups = ix->d_groups8;
  g.cn = ix->d_cn;
  g.gbad = gbad;
  g.gref = ix->d_gref8;
  g.qb8 = ix->d_qb8;
  g.qpar = ix->d_qpar;
  g.n_rows = (uint32_t)ix->n;
  g.pitch8 = pitch8;
  g.num_tiles = tiles;
  g.tile_stride = 1;
  g.tau = ix->d_tau;
  g.pairs = ix->d_pairs;
  g.pair_count = ix->d_pair_count;
  g.pair_cap = pair_cap;
  if ((rc = launch_gemm8<1>(ix, g, b.ct, masked, false))) return rc;
  const range_fn ffilter = l2 ? range_filter_kernel<WDBX_METRIC_L2> : range_filter_kernel<WDBX_METRIC_COSINE>;
  // pairs -> per-query candidates -> result keys; the counters are zero on entry (the block's first two kernels, or the memsets
  // of the second run)
  auto enqueue_gather = [&]() -> int {
    const uint32_t cap = ix->range_batch_cap;
    const RangeBatchSizes s2 = range_batch_sizes(b, cap, pair_cap, nwaves, pitch8);
    int rc2;
    if ((rc2 = ix->d_cand.grow(s2.cand_bytes))) return rc2;
    if ((rc2 = ix->d_rkeys.grow(s2.keys_bytes))) return rc2;
    hipLaunchKernelGGL(scatter_pairs_kernel, dim3((nwaves + SCATTER_LISTS - 1) / SCATTER_LISTS), dim3(1024), 0, ix->stream,
                       (const u64*)ix->d_pairs, (const uint32_t*)ix->d_pair_count, nwaves, pair_cap, ix->d_cand, ix->d_count, cap, d_lost);
    HIP_TRY(hipGetLastError());
    RangeArgs r = {};
    r.rows = (const f4*)ix->d_rows.p;
    r.queries = (const f4*)qsrc;
    r.thr = ix->d_rthr;
    r.n_rows = (uint32_t)ix->n;
    r.pitch4 = pitch4;
    r.out = ix->d_rkeys;
    r.count = ix->d_rcnt;
    r.cap = cap;  // (results <= candidates: never past the buffer)
    r.cand = ix->d_cand;
    r.cand_count = ix->d_count;
    r.cand_cap = cap;
    if ((rc2 = record(ix->merge_ev, ix->profile, ix->stream, true))) return rc2;
    // (up to 256 queries share the device: about 32 workgroups per CU over all of them, at least 8 per query)
    const uint32_t fgrid = std::min<uint32_t>((uint32_t)ix->cu_count * 8, std::max<uint32_t>(8, (uint32_t)ix->cu_count * 32 / (uint32_t)nv));
    hipLaunchKernelGGL(ffilter, dim3(fgrid, nv), dim3(256), 0, ix->stream, r);
    HIP_TRY(hipGetLastError());
    if ((rc2 = record(ix->merge_ev, ix->profile, ix->stream, false, (uint32_t)nv))) return rc2;
    HIP_TRY(hipMemcpyAsync(hcand.data(), ix->d_count, (MB + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipMemcpyAsync(hres.data(), ix->d_rcnt, MB * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return WDBX_OK;
  };
  if ((rc = enqueue_gather())) return rc;
  *lost = hcand[MB] != 0;
  if (*lost) return WDBX_OK;
  uint32_t most = 0;
  for (int i = 0; i < nv; ++i) most = std::max(most, hcand[i]);
  if (most > ix->range_batch_cap) {  // candidates past their buffers: grow to the exact count, scatter + filter again
    if (!range_batch_cap_fits(b, most)) {
      *lost = true;  // (buffers this large for 256 queries at once: the per-query rounds instead)
      return WDBX_OK;
    }
    ix->range_batch_cap = most;
    const std::vector<uint32_t> first(hcand.begin(), hcand.begin() + nv);
    HIP_TRY(hipMemsetAsync(ix->d_count, 0, (size_t)gbn * sizeof(uint32_t), ix->stream));
    HIP_TRY(hipMemsetAsync(ix->d_rcnt, 0, (size_t)gbn * sizeof(uint32_t), ix->stream));
    if ((rc = enqueue_gather())) return rc;
    // (the same pairs scattered again: every query's count must be what the first run counted)
    if (hcand[MB] || !std::equal(first.begin(), first.end(), hcand.begin()))
      return fail(WDBX_E_STATE, "batched range search: candidate count changed between two passes");
  }
  return WDBX_OK;
}

int wdbx_index_range_search_batch(wdbx_index* ix, const float* queries, int nq, const float* thresholds, int normalize_queries,
                                  const uint32_t* mask_words, uint64_t mask_word_count, uint64_t capacity, uint64_t* out_offsets,
                                  int64_t* out_rows, float* out_scores) try {
  int rc = range_check_args(ix, queries, nq, thresholds, capacity, out_offsets, out_rows, out_scores);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  ix->last_range_batch_path = RANGE_BATCH_NONE;
  ix->last_range_batch_blocks = ix->last_range_batch_pairs = ix->last_range_batch_fallback = 0;
  out_offsets[0] = 0;
  if (ix->n == 0) {
    for (int q = 0; q < nq; ++q) out_offsets[q + 1] = 0;
    return WDBX_OK;
  }
  if (mask_words && (rc = check_mask_words(ix->n, mask_word_count))) return rc;
  const bool l2 = ix->metric == WDBX_METRIC_L2;
  RangeBatchShape shape = {};
  shape.n_rows = ix->n;
  shape.nq = nq;
  shape.metric_l2 = l2 ? 1 : 0;
  shape.i8_pitch = i8_tiles_shape_ok(ix) ? i8g_pitch(ix) : 0u;
  shape.shadow_fits = 1;
  shape.gemm_bf16 = ix->opt_gemm_bf16;
  shape.gemm8_variant = ix->opt_gemm8_variant;
  shape.gemm_masked = ix->opt_gemm_masked;
  shape.gemm_min_rows = ix->opt_gemm_min_rows;
  shape.gemm_min_work = ix->opt_gemm_min_work;
  shape.min_queries = ix->opt_range_batch_min_queries;
  shape.has_mask = mask_words ? 1 : 0;
  // (the shadow copy is built only when everything else says tiles: a per-query call must not allocate it)
  const bool tiles = range_batch_use_tiles(shape) && prepare_i8g_shadow(ix);
  if (!tiles) {
    ix->last_range_batch_path = RANGE_BATCH_PER_QUERY;
    ix->last_range_batch_fallback = nq;
    return range_search_locked(ix, queries, nq, thresholds, normalize_queries, mask_words, mask_word_count, capacity, out_offsets,
                               out_rows, out_scores);
  }
  if (l2 && (rc = ensure_row_norms(ix))) return rc;
  if ((rc = ensure_group_ref(ix))) return rc;
  const std::vector<RangeBatchBlock> blocks =
      range_batch_blocks(nq, range_batch_block_queries(shape.metric_l2, shape.i8_pitch), (int)ix->opt_gemm_ct);
  const uint32_t pair_cap = range_batch_pair_cap(ix->opt_range_pair_cap);
  const uint32_t nwaves = range_batch_waves(ix->n, (uint32_t)ix->cu_count);
  RangeBatchTally tally;
  tally.start(nq);
  std::vector<uint32_t> hcand(RANGE_BATCH_MAX_BLOCK + 1), hres(RANGE_BATCH_MAX_BLOCK);
  std::vector<uint64_t> cnt(RANGE_BATCH_MAX_BLOCK), sub_offsets(RANGE_BATCH_MAX_BLOCK + 1);
  MaskScope scope(ix);
  // The call's queries sit in d_q from query staged_q0 on, its mask in d_mask and its bad-row table in d_call_bad.  A block
  // answered by the per-query rounds overwrites d_q with its own queries and clears active_mask (the mask's words and the
  // table stay what they are): only the queries BEHIND that block are staged again, and the mask is re-armed.
  if (mask_words && (rc = scope.set(mask_words))) return rc;
  if ((rc = upload_queries(ix, queries, (uint64_t)nq, normalize_queries))) return rc;
  int staged_q0 = 0;
  bool staged = true;
  const u64* gbad = ix->d_gbad8;
  if (mask_words) {  // this call's bad-row table: removed rows, rows past the end, rows the mask leaves out
    const u64 ngroups = ix->d_groups8.bytes / sizeof(f4);
    if ((rc = ix->d_call_bad.grow((size_t)ngroups * sizeof(u64)))) return rc;
    hipLaunchKernelGGL(gbad_with_mask_kernel, dim3(gbad_with_mask_grid(ngroups), 1), dim3(256), 0, ix->stream, (const u64*)ix->d_gbad8,
                       (const uint32_t*)ix->active_mask, (u64)((ix->n + 31) / 32), ngroups, ix->d_call_bad, (u64)0, (const int32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    gbad = ix->d_call_bad;
  }
  for (const RangeBatchBlock& b : blocks) {
    if (!staged) {
      if ((rc = upload_queries(ix, queries + (size_t)b.q0 * ix->dim, (uint64_t)(nq - b.q0), normalize_queries))) return rc;
      staged_q0 = b.q0;
      if (mask_words) {
        ix->active_mask = ix->d_mask;
        scope.armed = true;
      }
      staged = true;
    }
    bool lost = false;
    if ((rc = range_batch_block(ix, b, staged_q0, queries, thresholds, gbad, pair_cap, nwaves, hcand, hres, &lost))) return rc;
    uint64_t kept = 0;
    for (int i = 0; i < b.nv; ++i) kept += hcand[i];
    const uint64_t base = out_offsets[b.q0];
    if (lost) {  // every query of the block through the per-query rounds; its results land sorted and decoded
      tally.lost(b, kept);
      const uint64_t room = capacity > base ? capacity - base : 0;
      if ((rc = range_search_locked(ix, queries + (size_t)b.q0 * ix->dim, b.nv, thresholds + b.q0, normalize_queries, mask_words,
                                    mask_word_count, room, sub_offsets.data(), room ? out_rows + base : nullptr,
                                    room ? out_scores + base : nullptr)))
        return rc;
      for (int i = 0; i < b.nv; ++i) out_offsets[b.q0 + i + 1] = base + sub_offsets[i + 1];
      staged = false;
      continue;
    }
    tally.tiles(b, kept);
    for (int i = 0; i < b.nv; ++i) cnt[i] = hres[i];
    const uint64_t total = range_csr_offsets(cnt.data(), b.nv, out_offsets + b.q0);
    if (total <= capacity) {  // the keys, straight into the caller's row array at their offsets (u64 slots)
      for (int i = 0; i < b.nv; ++i)
        if (cnt[i])
          HIP_TRY(hipMemcpyAsync(out_rows + out_offsets[b.q0 + i], ix->d_rkeys + (size_t)i * ix->range_batch_cap, cnt[i] * sizeof(u64),
                                 hipMemcpyDeviceToHost, ix->stream));
      HIP_TRY(hipStreamSynchronize(ix->stream));
    }
  }
  if (out_offsets[nq] <= capacity) {  // sort and decode the tile blocks' keys (a per-query block's are done)
    for (const RangeBatchBlock& b : blocks) {
      if (tally.per_query[(size_t)b.q0]) continue;
      const uint64_t base = out_offsets[b.q0];
      for (int i = 0; i <= b.nv; ++i) sub_offsets[i] = out_offsets[b.q0 + i] - base;
      if (sub_offsets[b.nv]) range_sort_decode(l2 ? 1 : 0, b.nv, sub_offsets.data(), out_rows + base, out_scores + base);
    }
  }
  // One query with very many hits must not pin gigabytes for the handle's life, nor size every later block's 256 buffers by
  // it: beyond RANGE_BATCH_KEEP_CAP candidates per query the grown buffers are released and the next call starts from that
  // capacity again (and regrows, once, if it meets such a query).
  if (ix->range_batch_cap > RANGE_BATCH_KEEP_CAP) {
    ix->range_batch_cap = RANGE_BATCH_KEEP_CAP;
    HIP_TRY(hipStreamSynchronize(ix->stream));
    if ((rc = ix->d_cand.release()) || (rc = ix->d_rkeys.release())) return rc;
  }
  ix->last_range_batch_path = tally.path();
  ix->last_range_batch_blocks = tally.blocks;
  ix->last_range_batch_pairs = tally.pairs;
  ix->last_range_batch_fallback = tally.fallback_queries;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_device_alloc(wdbx_index* ix, uint64_t bytes, void** out_dev_ptr) try {
  if (!ix || !out_dev_ptr) return fail(WDBX_E_INVALID, "null argument");
  *out_dev_ptr = nullptr;
  DeviceGuard g(ix->device);
  HIP_TRY(hipMalloc(out_dev_ptr, bytes ? bytes : 1));
  return WDBX_OK;
} WDBX_CATCH

int wdbx_device_free(wdbx_index* ix, void* dev_ptr) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (!dev_ptr) return WDBX_OK;
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  HIP_TRY(hipFree(dev_ptr));
  return WDBX_OK;
} WDBX_CATCH

int wdbx_device_upload(wdbx_index* ix, void* dev_dst, const void* host_src, uint64_t bytes) try {
  if (!ix || (bytes && (!dev_dst || !host_src))) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  HIP_TRY(hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return WDBX_OK;
} WDBX_CATCH

int wdbx_device_download(wdbx_index* ix, void* host_dst, const void* dev_src, uint64_t bytes) try {
  if (!ix || (bytes && (!host_dst || !dev_src))) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  HIP_TRY(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return WDBX_OK;
} WDBX_CATCH

int wdbx_device_fill_synthetic(wdbx_index* ix, float* dev_dst, uint64_t seed, uint64_t counter_row0, uint64_t n,
                               int normalize) try {
  if (!ix || (n && !dev_dst)) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  int rc = launch_fill(ix, dev_dst, seed, counter_row0, n, normalize);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_search_device(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx,
                             float* d_out_score) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  return enqueue_search(ix, d_queries, nq, k, d_out_idx, d_out_score, SEARCH_FINAL);
} WDBX_CATCH

int wdbx_index_search_sharded_device(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx,
                                     float* d_out_score) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  return enqueue_search(ix, d_queries, nq, k, d_out_idx, d_out_score, SEARCH_SHARDED);
} WDBX_CATCH

int wdbx_index_search_sharded_batch_device(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx,
                                           float* d_out_score) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  if (!gemm_eligible(ix, std::max(nq, (int)ix->opt_gemm_min_nq), k))
    return fail(WDBX_E_STATE, "batched MFMA path needs >= %lld rows and k*1024 <= rows on every rank",
                (long long)ix->opt_gemm_min_rows);
  return enqueue_search_gemm(ix, d_queries, nq, k, d_out_idx, d_out_score, SEARCH_SHARDED);
} WDBX_CATCH

int wdbx_index_search_batch_device(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx,
                                   float* d_out_score) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  if (!gemm_eligible(ix, std::max(nq, (int)ix->opt_gemm_min_nq), k))
    return fail(WDBX_E_STATE, "batched MFMA path needs >= %lld rows and k*1024 <= rows", (long long)ix->opt_gemm_min_rows);
  return enqueue_search_gemm(ix, d_queries, nq, k, d_out_idx, d_out_score);
} WDBX_CATCH

// wdbx_index_search_batch_device with a row mask from the host (uint32 words, bit r % 32 of word r / 32 = row r may be
// returned; mask_word_count >= ceil(rows / 32) or the call is refused): one masked pass over the int8 tiles when they are what
// would run (option last_batch_masked = 1), the masked per-query paths otherwise.  The mask is copied before the call
// returns and applies to this call only; the results are device-resident and ordered on the handle's stream as for the
// unmasked call; wdbx_index_batch_status describes the call when it ran the masked pass (after the per-query fall-back: that
// path's last round, as after wdbx_index_search_device).
int wdbx_index_search_batch_masked_device(wdbx_index* ix, const float* d_queries, int nq, int k, const uint32_t* mask_words,
                                          uint64_t mask_word_count, int64_t* d_out_idx, float* d_out_score) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (!mask_words) return fail(WDBX_E_INVALID, "mask_words is null");
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  if (!gemm_eligible(ix, std::max(nq, (int)ix->opt_gemm_min_nq), k))
    return fail(WDBX_E_STATE, "batched MFMA path needs >= %lld rows and k*1024 <= rows", (long long)ix->opt_gemm_min_rows);
  int rc;
  if ((rc = check_mask_words(ix->n, mask_word_count))) return rc;
  MaskScope scope(ix);
  const bool tiles = masked_tiles_ready(ix, k);
  if ((rc = scope.set(mask_words))) return rc;
  if (tiles) return enqueue_search_gemm(ix, d_queries, nq, k, d_out_idx, d_out_score);
  ix->last_batch_masked = false;
  return enqueue_search(ix, d_queries, nq, k, d_out_idx, d_out_score, SEARCH_FINAL);
} WDBX_CATCH

int wdbx_index_batch_status(wdbx_index* ix, uint32_t* out_counts, int nq, uint32_t* out_capacity, int* out_overflowed) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  if (nq < 0 || (uint32_t)nq > ix->last_batch_nq) return fail(WDBX_E_INVALID, "nq=%d but the last batch had %u queries", nq, ix->last_batch_nq);
  std::vector<uint32_t> counts((size_t)std::max(nq, 1));
  if (ix->last_batch_masked == 2) {  // a mask per query: the counters are per slot; reported in the caller's query order
    std::vector<uint32_t> slots(ix->last_batch_slot.empty() ? 0 : (size_t)*std::max_element(ix->last_batch_slot.begin(), ix->last_batch_slot.end()) + 1);
    if (!slots.empty()) HIP_TRY(hipMemcpyAsync(slots.data(), ix->d_count, slots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    for (int q = 0; q < nq; ++q) counts[(size_t)q] = slots[(size_t)ix->last_batch_slot[(size_t)q]];
  } else if (nq) {
    HIP_TRY(hipMemcpyAsync(counts.data(), ix->d_count, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
  }
  HIP_TRY(hipStreamSynchronize(ix->stream));
  int over = 0;
  for (int q = 0; q < nq; ++q) {
    if (counts[q] > ix->last_batch_cap) ++over;
    if (out_counts) out_counts[q] = counts[q];
  }
  if (out_capacity) *out_capacity = ix->last_batch_cap;
  if (out_overflowed) *out_overflowed = over;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_profile_read_gemm(wdbx_index* ix, uint64_t* launches, double* ms_total) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return drain(ix->gemm_ev, launches, ms_total);
} WDBX_CATCH

int wdbx_index_profile_read_sample(wdbx_index* ix, uint64_t* launches, double* ms_total) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return drain(ix->sample_ev, launches, ms_total);
} WDBX_CATCH

int wdbx_index_synchronize(wdbx_index* ix) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return WDBX_OK;
} WDBX_CATCH

int wdbx_comm_unique_id(void* out_128_bytes) try {
  if (!out_128_bytes) return fail(WDBX_E_INVALID, "null argument");
  static_assert(sizeof(ncclUniqueId) <= WDBX_UNIQUE_ID_BYTES, "unique id larger than the ABI slot");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  memset(out_128_bytes, 0, WDBX_UNIQUE_ID_BYTES);
  memcpy(out_128_bytes, &id, sizeof id);
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_comm_init(wdbx_index* ix, int nranks, int rank, const void* unique_id_128_bytes,
                         uint64_t global_row_base) try {
  if (!ix || !unique_id_128_bytes) return fail(WDBX_E_INVALID, "null argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(WDBX_E_INVALID, "rank %d of %d", rank, nranks);
  if (global_row_base >= 0xFFFFFFFFull) return fail(WDBX_E_INVALID, "global row base exceeds 32-bit row keys");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (ix->comm) return fail(WDBX_E_STATE, "communicator already initialised");
  DeviceGuard g(ix->device);
  ncclUniqueId id;
  memcpy(&id, unique_id_128_bytes, sizeof id);
  NCCL_TRY(ncclCommInitRank(&ix->comm, nranks, id, rank));
  ix->nranks = nranks;
  ix->rank = rank;
  ix->row_base = global_row_base;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_comm_destroy(wdbx_index* ix) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->comm) return WDBX_OK;
  DeviceGuard g(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  NCCL_TRY(ncclCommDestroy(ix->comm));
  ix->comm = nullptr;
  ix->nranks = 1;
  ix->rank = 0;
  ix->row_base = 0;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_comm_info(wdbx_index* ix, int* out_nranks, int* out_rank, uint64_t* out_row_base) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  int n = 0, r = -1;
  if (ix->comm) {  // what RCCL itself says about the communicator, not what the host side asked for
    NCCL_TRY(ncclCommCount(ix->comm, &n));
    NCCL_TRY(ncclCommUserRank(ix->comm, &r));
  }
  if (out_nranks) *out_nranks = n;
  if (out_rank) *out_rank = r;
  if (out_row_base) *out_row_base = ix->row_base;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_comm_set_row_base(wdbx_index* ix, uint64_t global_row_base) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  if (global_row_base >= 0xFFFFFFFFull) return fail(WDBX_E_INVALID, "global row base exceeds 32-bit row keys");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->comm) return fail(WDBX_E_STATE, "no communicator on this handle");
  DeviceGuard g(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  ix->row_base = global_row_base;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_probe_read(wdbx_index* ix, int nontemporal, int blocks, int reps, double* out_ms_per_pass) try {
  if (!ix || !out_ms_per_pass) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  if (!ix->n) return fail(WDBX_E_STATE, "empty index");
  int rc = ix->d_tau.grow((size_t)GB_N * sizeof(float));
  if (rc) return rc;
  const u64 quads = (u64)ix->n * (u64)(ix->pitch / 4);
  const uint32_t grid = blocks > 0 ? (uint32_t)blocks : (uint32_t)ix->cu_count * 8;
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  reps = std::max(1, reps);
  for (int i = -2; i < reps; ++i) {
    if (i == 0) HIP_TRY(hipEventRecord(e0, ix->stream));
    if (nontemporal)
      hipLaunchKernelGGL(probe_read_kernel<true>, dim3(grid), dim3(256), 0, ix->stream, (const f4*)ix->d_rows.p, quads, ix->d_tau);
    else
      hipLaunchKernelGGL(probe_read_kernel<false>, dim3(grid), dim3(256), 0, ix->stream, (const f4*)ix->d_rows.p, quads, ix->d_tau);
  }
  HIP_TRY(hipEventRecord(e1, ix->stream));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *out_ms_per_pass = ms / reps;
  return WDBX_OK;
} WDBX_CATCH


// ------------------------------------------------------------------------------------------------
// in-process shard group (host_group.h): S shards driven by one process, one host thread per shard -- the reference's
// VectorStore(num_shards=S) shape (vector_store.py:111-134, :323-345)
// ------------------------------------------------------------------------------------------------
int wdbx_group_create(const int* device_ids, int n, int dim, int metric, uint64_t cap_per_shard, wdbx_group** out) try {
  if (!out) return fail(WDBX_E_INVALID, "out is null");
  *out = nullptr;
  if (!device_ids || n < 1 || n > 64) return fail(WDBX_E_INVALID, "need 1..64 device ids");
  if (cap_per_shard < 1 || cap_per_shard * (uint64_t)n >= 0xFFFFFF00ull)
    return fail(WDBX_E_INVALID, "cap_per_shard * shards must stay below 2^32 rows");
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j)
      if (device_ids[i] == device_ids[j]) return fail(WDBX_E_INVALID, "device %d listed twice (RCCL needs one rank per device)", device_ids[i]);
  wdbx_group* g = new (std::nothrow) wdbx_group();
  if (!g) return fail(WDBX_E_NOMEM, "host allocation failed");
  g->cap_per_shard = cap_per_shard;
  g->dim = dim;
  g->metric = metric;
  g->sh = std::vector<GroupShard>((size_t)n);  // (in place: a shard's buffers do not move)
  int rc = WDBX_OK;
  for (int i = 0; i < n && rc == WDBX_OK; ++i) {
    rc = wdbx_index_create(device_ids[i], dim, metric, cap_per_shard, &g->sh[i].ix);
    if (rc == WDBX_OK) g->sh[i].ix->row_base = (uint64_t)i * cap_per_shard;
  }
  if (rc == WDBX_OK) rc = group_finish_setup(g, 0);
  if (rc != WDBX_OK) {
    const std::string keep = g_err;
    group_free(g);
    g_err = keep;
    return rc;
  }
  *out = g;
  return WDBX_OK;
} WDBX_CATCH

// A group over EXISTING shard handles (the facade's one index per shard, vector_store.py:111-134): the handles stay
// owned by the caller and keep growing through wdbx_index_add; the group adds the exchange (RCCL communicators from
// ncclCommInitAll when every shard has its own device, device copies otherwise) and gives shard s the row numbers
// [s * stride, (s + 1) * stride) in merged results, stride = (2^32 - 256) / n.  Shard order = row order, so ties come
// back in the order of the reference's stable sort over its shard loop (vector_store.py:323-330).
int wdbx_group_attach_ex(wdbx_index* const* shards, int n, int exchange_mode, wdbx_group** out) try {
  if (!out) return fail(WDBX_E_INVALID, "out is null");
  *out = nullptr;
  if (!shards || n < 1 || n > 64) return fail(WDBX_E_INVALID, "need 1..64 shard handles");
  if (exchange_mode < 0 || exchange_mode > 2) return fail(WDBX_E_INVALID, "exchange_mode=%d (0 auto, 1 RCCL, 2 device copies)", exchange_mode);
  for (int i = 0; i < n; ++i) {
    if (!shards[i]) return fail(WDBX_E_INVALID, "shard %d is null", i);
    if (shards[i]->dim != shards[0]->dim || shards[i]->metric != shards[0]->metric)
      return fail(WDBX_E_INVALID, "shard %d differs from shard 0 in dim or metric", i);
    if (shards[i]->comm) return fail(WDBX_E_STATE, "shard %d already belongs to a per-rank communicator", i);
    for (int j = 0; j < i; ++j)
      if (shards[i] == shards[j]) return fail(WDBX_E_INVALID, "shard handle %d listed twice", i);
  }
  wdbx_group* g = new (std::nothrow) wdbx_group();
  if (!g) return fail(WDBX_E_NOMEM, "host allocation failed");
  g->owns_shards = false;
  g->dim = shards[0]->dim;
  g->metric = shards[0]->metric;
  g->cap_per_shard = 0xFFFFFF00ull / (uint64_t)n;
  g->sh = std::vector<GroupShard>((size_t)n);
  for (int i = 0; i < n; ++i) g->sh[i].ix = shards[i];
  int rc = group_finish_setup(g, exchange_mode);
  if (rc != WDBX_OK) {
    const std::string keep = g_err;
    group_free(g);
    g_err = keep;
    return rc;
  }
  for (int i = 0; i < n; ++i) {
    std::lock_guard<std::mutex> li(shards[i]->mu);
    shards[i]->row_base = (uint64_t)i * g->cap_per_shard;
  }
  *out = g;
  return WDBX_OK;
} WDBX_CATCH

int wdbx_group_attach(wdbx_index* const* shards, int n, wdbx_group** out) try {
  return wdbx_group_attach_ex(shards, n, 0, out);
} WDBX_CATCH

void wdbx_group_destroy(wdbx_group* g) try {
  if (!g) return;
  group_free(g);
} WDBX_CATCH_VOID

int wdbx_group_info(wdbx_group* g, int* out_shards, int* out_rccl_nranks, uint64_t* out_row_stride) try {
  if (!g) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(g->mu);
  int n = 0;  // what RCCL itself says; 0 = the group exchanges by device copies
  if (g->exchange == GROUP_EXCHANGE_RCCL && g->sh[0].comm) NCCL_TRY(ncclCommCount(g->sh[0].comm, &n));
  if (out_shards) *out_shards = (int)g->sh.size();
  if (out_rccl_nranks) *out_rccl_nranks = n;
  if (out_row_stride) *out_row_stride = g->cap_per_shard;
  return WDBX_OK;
} WDBX_CATCH

// counters of the group (names: "exchanges" = exchange + merge steps enqueued so far, one per chunk of a call; "dispatches" =
// jobs handed to the shards' threads; "unusable" = 1 after a failed collective aborted the communicators)
int wdbx_group_stat(wdbx_group* g, const char* name, int64_t* value) try {
  if (!g || !name || !value) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(g->mu);
  if (!strcmp(name, "exchanges")) return *value = (int64_t)g->exchanges, WDBX_OK;
  if (!strcmp(name, "dispatches")) return *value = (int64_t)g->disp.dispatches, WDBX_OK;
  if (!strcmp(name, "unusable")) return *value = g->unusable ? 1 : 0, WDBX_OK;
  return fail(WDBX_E_INVALID, "unknown group statistic '%s'", name);
} WDBX_CATCH

int wdbx_group_size(wdbx_group* g, uint64_t* out_rows) try {
  if (!g || !out_rows) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(g->mu);
  uint64_t total = 0;
  for (GroupShard& s : g->sh) {
    std::lock_guard<std::mutex> li(s.ix->mu);
    total += s.ix->n;
  }
  *out_rows = total;
  return WDBX_OK;
} WDBX_CATCH

// append rows; they fill shard 0 up to cap_per_shard, then shard 1, ... (contiguous global rows)
int wdbx_group_add(wdbx_group* g, const float* rows, uint64_t n, int normalize, uint64_t* first_row_out) try {
  if (!g) return fail(WDBX_E_INVALID, "null handle");
  if (n && !rows) return fail(WDBX_E_INVALID, "rows is null");
  std::lock_guard<std::mutex> lk(g->mu);
  if (!g->owns_shards) return fail(WDBX_E_STATE, "an attached group does not place rows: add them to the shard handles");
  uint64_t total = 0;
  for (GroupShard& s : g->sh) total += s.ix->n;
  if (total + n > g->cap_per_shard * g->sh.size())
    return fail(WDBX_E_INVALID, "group is full: %llu + %llu rows > %llu", (u64)total, (u64)n, (u64)(g->cap_per_shard * g->sh.size()));
  if (first_row_out) *first_row_out = total;
  uint64_t done = 0;
  while (done < n) {
    const size_t s = (size_t)((total + done) / g->cap_per_shard);
    wdbx_index* ix = g->sh[s].ix;
    const uint64_t room = g->cap_per_shard - ix->n, take = std::min(room, n - done);
    int rc = wdbx_index_add(ix, rows + (size_t)done * g->dim, take, normalize, nullptr);
    if (rc) return rc;
    done += take;
  }
  return WDBX_OK;
} WDBX_CATCH

// global row number of each shard's first row (default: shard * stride, or shard * cap_per_shard for owned groups); a
// caller that placed contiguous row ranges itself (bench.py) gives the ranges' first rows
int wdbx_group_set_row_bases(wdbx_group* g, const uint64_t* bases, int n) try {
  if (!g || !bases) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(g->mu);
  if (n != (int)g->sh.size()) return fail(WDBX_E_INVALID, "%d bases for %d shards", n, (int)g->sh.size());
  for (int i = 0; i < n; ++i)
    if (bases[i] >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "row base %llu exceeds 32-bit row keys", (u64)bases[i]);
  GroupLocks locks(g);
  for (int i = 0; i < n; ++i) {
    DeviceGuard dg(g->sh[i].ix->device);
    HIP_TRY(hipStreamSynchronize(g->sh[i].ix->stream));
    g->sh[i].ix->row_base = bases[i];
  }
  return WDBX_OK;
} WDBX_CATCH

// ---- resident queries: the group's own query buffer on every shard's device ----
int wdbx_group_queries_upload(wdbx_group* g, const float* queries, int nq, int normalize_queries) try {
  if (!g) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 1 || !queries) return fail(WDBX_E_INVALID, "need at least one query");
  std::lock_guard<std::mutex> lk(g->mu);
  GroupLocks locks(g);
  return group_load_queries(g, queries, 0, 0, nq, normalize_queries);
} WDBX_CATCH

int wdbx_group_queries_synthetic(wdbx_group* g, uint64_t seed, uint64_t counter_row0, int nq, int normalize) try {
  if (!g) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 1) return fail(WDBX_E_INVALID, "need at least one query");
  std::lock_guard<std::mutex> lk(g->mu);
  GroupLocks locks(g);
  return group_load_queries(g, nullptr, seed, counter_row0, nq, normalize);
} WDBX_CATCH

// asynchronous: enqueue the search of resident queries [first, first + nq) on every shard, the exchange and the merge
int wdbx_group_search_resident(wdbx_group* g, int first_query, int nq, int k, int k_out) try {
  if (!g) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 0) return fail(WDBX_E_INVALID, "nq=%d", nq);
  std::lock_guard<std::mutex> lk(g->mu);
  GroupLocks locks(g);
  const int rc = group_enqueue_search(g, first_query, nq, k, k_out, false, false);
  return rc ? group_fail_drained(g, rc) : rc;
} WDBX_CATCH

int wdbx_group_synchronize(wdbx_group* g) try {
  if (!g) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(g->mu);
  for (GroupShard& s : g->sh) {
    DeviceGuard dg(s.ix->device);
    HIP_TRY(hipStreamSynchronize(s.ix->stream));
  }
  return WDBX_OK;
} WDBX_CATCH

// results [nq, k_out] of the most recent search (blocking: waits for the root shard's stream)
int wdbx_group_results(wdbx_group* g, int nq, int k_out, int64_t* out_idx, float* out_score) try {
  if (!g || !out_idx || !out_score) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(g->mu);
  if (nq < 0 || nq > g->last_nq || k_out != g->last_k_out)
    return fail(WDBX_E_INVALID, "the last search left [%d, %d] results, [%d, %d] asked for", g->last_nq, g->last_k_out, nq, k_out);
  if (!nq) return WDBX_OK;
  wdbx_index* root = g->sh[0].ix;
  DeviceGuard dg(root->device);
  const size_t elems = (size_t)nq * k_out;
  HIP_TRY(hipMemcpyAsync(out_idx, g->d_oidx, elems * sizeof(int64_t), hipMemcpyDeviceToHost, root->stream));
  HIP_TRY(hipMemcpyAsync(out_score, g->d_oscore, elems * sizeof(float), hipMemcpyDeviceToHost, root->stream));
  HIP_TRY(hipStreamSynchronize(root->stream));
  return WDBX_OK;
} WDBX_CATCH

static int group_search_host(wdbx_group* g, const float* queries, int nq, int k, int k_out, int normalize_queries,
                             const uint32_t* const* masks, const uint64_t* mask_word_counts, int64_t* out_idx, float* out_score);

// every shard's top-k, merged into the k_out best of their union (k <= k_out <= shards * k): k_out = k is the plain
// search; k_out = shards * k returns the whole merged candidate list the reference's VectorStore.search sorts before
// its threshold / metadata post-filter / cut (vector_store.py:323-345).  out_idx / out_score are [nq, k_out].  Blocking.
int wdbx_group_search_merged(wdbx_group* g, const float* queries, int nq, int k, int k_out, int normalize_queries,
                             int64_t* out_idx, float* out_score) try {
  return group_search_host(g, queries, nq, k, k_out, normalize_queries, nullptr, nullptr, out_idx, out_score);
} WDBX_CATCH

// the same with a row filter per shard (metadata push-down through the group: vector_store.py:337-342 only post-filters):
// mask_words[s] = shard s's mask (uint32 words, bit r % 32 of word r / 32 = row r may be returned, ceil(rows / 32) words) or
// null for "every row of that shard"
int wdbx_group_search_merged_masked(wdbx_group* g, const float* queries, int nq, int k, int k_out, int normalize_queries,
                                    const uint32_t* const* mask_words, int64_t* out_idx, float* out_score) try {
  if (!mask_words) return fail(WDBX_E_INVALID, "mask_words is null");
  return group_search_host(g, queries, nq, k, k_out, normalize_queries, mask_words, nullptr, out_idx, out_score);
} WDBX_CATCH

// ... and with the number of words each mask holds (mask_word_counts[s]; ignored for a null mask): a mask shorter than
// ceil(rows of shard s / 32) words -- built before a concurrent add -- is refused under the locks instead of over-read
int wdbx_group_search_merged_masked_n(wdbx_group* g, const float* queries, int nq, int k, int k_out, int normalize_queries,
                                      const uint32_t* const* mask_words, const uint64_t* mask_word_counts, int64_t* out_idx,
                                      float* out_score) try {
  if (!mask_words || !mask_word_counts) return fail(WDBX_E_INVALID, "mask_words / mask_word_counts is null");
  return group_search_host(g, queries, nq, k, k_out, normalize_queries, mask_words, mask_word_counts, out_idx, out_score);
} WDBX_CATCH

static int group_search_host(wdbx_group* g, const float* queries, int nq, int k, int k_out, int normalize_queries,
                             const uint32_t* const* masks, const uint64_t* mask_word_counts, int64_t* out_idx, float* out_score) {
  if (!g) return fail(WDBX_E_INVALID, "null handle");
  if (nq < 0) return fail(WDBX_E_INVALID, "nq=%d", nq);
  if (nq == 0) return WDBX_OK;
  if (!queries || !out_idx || !out_score) return fail(WDBX_E_INVALID, "null buffer");
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  std::lock_guard<std::mutex> lk(g->mu);
  GroupLocks locks(g);  // held until the results are on the host: the shards' own callers wait, as on any busy handle
  int rc;
  if (masks && mask_word_counts)
    for (size_t s = 0; s < g->sh.size(); ++s)
      if (masks[s] && (rc = check_mask_words(g->sh[s].ix->n, mask_word_counts[s], ("shard " + std::to_string(s) + ": row mask").c_str())))
        return rc;
  wdbx_index* root = g->sh[0].ix;
  const size_t elems = (size_t)nq * k_out, pitch = (size_t)root->pitch, dim = (size_t)root->dim;
  // small calls (the facade's lone queries): queries and results through mapped host memory, no memcpy calls at all
  const bool cosine_norm = normalize_queries && root->metric == WDBX_METRIC_COSINE;
  if (g->h_stage && !cosine_norm && (size_t)nq * pitch * sizeof(float) <= GROUP_STAGE_Q && elems * sizeof(int64_t) <= GROUP_STAGE_IDX) {
    pad_queries((float*)g->h_stage, pitch, queries, dim, (size_t)nq);
    // a lone query: no repair launches are queued (two per shard); each shard leaves an overflow word instead, and the rare
    // call that finds one set is run again with the repairs in place
    volatile uint32_t* const flags = (volatile uint32_t*)(g->h_stage + GROUP_STAGE_Q + GROUP_STAGE_IDX + GROUP_STAGE_SCORE);
    const bool defer = nq == 1 && !use_select(root, k) && g->sh.size() <= 64;
    if (defer)
      for (size_t s = 0; s < g->sh.size(); ++s) flags[s] = 0;
    // (a failed enqueue: the shards that did enqueue still read the staged query and write keys, flags and results into the
    // staging area the next call reuses -- wait for them before returning the error)
    // a lone query: the group's final merge (one workgroup on the root's stream, behind the exchange and so behind every
    // shard's local stage) writes a sequence number behind its results and this thread polls it, as wdbx_index_search does
    uint32_t done_seq = 0;
    const bool poll = defer && root->opt_poll_done && g->sh[0].stage_dev;
    if (poll) {
      DeviceGuard dgr(root->device);
      if (!g->done_ev) HIP_TRY(hipEventCreateWithFlags(&g->done_ev, hipEventDisableTiming));
      if (++g->lone_seq == 0) ++g->lone_seq;
      done_seq = g->lone_seq;
      flags[64] = 0;
      root->done_flag_dev = (uint32_t*)(g->sh[0].stage_dev + GROUP_STAGE_Q + GROUP_STAGE_IDX + GROUP_STAGE_SCORE) + 64;
      root->done_seq = done_seq;
      root->done_signals = 0;
    }
    rc = group_enqueue_search(g, 0, nq, k, k_out, true, true, masks, defer);
    const bool polled = poll && root->done_signals == 1;
    root->done_flag_dev = nullptr;
    if (rc) return group_fail_drained(g, rc);
    DeviceGuard dg(root->device);
    // (the root stream's merge depends on every shard's local stage through the exchange: when it has drained, no
    // device reads the staged queries any more and the results are in host memory)
    if (polled) {
      HIP_TRY(hipEventRecord(g->done_ev, root->stream));
      if ((rc = wait_done_word(flags + 64, done_seq, g->done_ev))) return rc;
    } else {
      HIP_TRY(hipStreamSynchronize(root->stream));
    }
    if (defer) {
      bool over = false;
      for (size_t s = 0; s < g->sh.size(); ++s) over = over || flags[s] != 0;
      if (over) {
        if ((rc = group_enqueue_search(g, 0, nq, k, k_out, true, true, masks, false))) return group_fail_drained(g, rc);
        HIP_TRY(hipStreamSynchronize(root->stream));
      }
    }
    memcpy(out_idx, g->h_stage + GROUP_STAGE_Q, elems * sizeof(int64_t));
    memcpy(out_score, g->h_stage + GROUP_STAGE_Q + GROUP_STAGE_IDX, elems * sizeof(float));
    return WDBX_OK;
  }
  if ((rc = group_load_queries(g, queries, 0, 0, nq, normalize_queries))) return group_fail_drained(g, rc);  // (the caller's query buffer)
  if ((rc = group_enqueue_search(g, 0, nq, k, k_out, false, true, masks))) return group_fail_drained(g, rc);
  DeviceGuard dg(root->device);
  HIP_TRY(hipMemcpyAsync(out_idx, g->d_oidx, elems * sizeof(int64_t), hipMemcpyDeviceToHost, root->stream));
  HIP_TRY(hipMemcpyAsync(out_score, g->d_oscore, elems * sizeof(float), hipMemcpyDeviceToHost, root->stream));
  // (the root stream's merge depends on every shard's local stage through the exchange: when it has drained, the
  // caller's query buffer is no longer read by any device)
  HIP_TRY(hipStreamSynchronize(root->stream));
  return WDBX_OK;
}

// blocking search over all shards (k_out = k)
int wdbx_group_search(wdbx_group* g, const float* queries, int nq, int k, int normalize_queries, int64_t* out_idx,
                      float* out_score) try {
  return wdbx_group_search_merged(g, queries, nq, k, k, normalize_queries, out_idx, out_score);
} WDBX_CATCH

// host-level all-gather of small buffers through a handle's per-rank communicator (launcher-side plumbing of a
// torch-free multi-process run: barrier, max-reduction of a time, result cross-checks)
int wdbx_index_comm_allgather_host(wdbx_index* ix, const void* send, void* recv, uint64_t bytes) try {
  if (!ix || !send || !recv || !bytes) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  if (!ix->comm) return fail(WDBX_E_STATE, "no communicator on this handle");
  DeviceGuard g(ix->device);
  int rc = ix->d_gathered.grow((size_t)(ix->nranks + 1) * bytes);
  if (rc) return rc;
  char* base = (char*)ix->d_gathered.p;
  HIP_TRY(hipMemcpyAsync(base, send, bytes, hipMemcpyHostToDevice, ix->stream));
  NCCL_TRY(ncclAllGather(base, base + bytes, bytes, ncclUint8, ix->comm, ix->stream));
  HIP_TRY(hipMemcpyAsync(recv, base + bytes, (size_t)ix->nranks * bytes, hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_profile(wdbx_index* ix, int enable) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  ix->profile = enable != 0;
  return WDBX_OK;
} WDBX_CATCH

static int drain(EventPool& pool, uint64_t* count, double* ms) {
  double total = 0;
  uint64_t launches = 0;
  for (size_t i = 0; i + 1 < pool.used; i += 2) {
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, pool.ev[i], pool.ev[i + 1]));
    total += t;
    launches += pool.launches[i / 2];
  }
  if (count) *count = launches;
  if (ms) *ms = total;
  pool.used = 0;
  return WDBX_OK;
}

int wdbx_index_profile_read(wdbx_index* ix, uint64_t* scan_launches, double* scan_ms_total, uint64_t* merge_launches,
                            double* merge_ms_total) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  DeviceGuard g(ix->device);
  HIP_TRY(hipStreamSynchronize(ix->stream));
  int rc = drain(ix->scan_ev, scan_launches, scan_ms_total);
  if (rc) return rc;
  return drain(ix->merge_ev, merge_launches, merge_ms_total);
} WDBX_CATCH

static const OptionDesc<wdbx_index> kOptions[] = {
    {"scan_lanes", &wdbx_index::opt_lanes},
    {"scan_blocks", &wdbx_index::opt_blocks},
    {"scan_nt", &wdbx_index::opt_nt},
    {"scan_blocked", &wdbx_index::opt_blocked},
    {"scan_generic", &wdbx_index::opt_generic},
    {"exchange_batch", &wdbx_index::opt_batch},
    {"lds_lists", &wdbx_index::opt_lds_lists},
    {"merge_fast", &wdbx_index::opt_merge_fast},
    {"poll_done", &wdbx_index::opt_poll_done},
    {"scan_one_grid", &wdbx_index::opt_scan_one_grid},
    {"zero_copy", &wdbx_index::opt_zero_copy},
    {"lone_host_select", &wdbx_index::opt_lone_host_select},
    {"wg_merge", &wdbx_index::opt_wg_merge},
    {"gemm_ct", &wdbx_index::opt_gemm_ct},
    {"gemm_l2", &wdbx_index::opt_gemm_l2},
    {"gemm_l2_i8", &wdbx_index::opt_gemm_l2_i8},
    {"gemm_bf16", &wdbx_index::opt_gemm_bf16},
    {"gemm8_variant", &wdbx_index::opt_gemm8_variant},
    {"gemm8_refine", &wdbx_index::opt_gemm8_refine},
    {"scan8_sample4", &wdbx_index::opt_scan8_sample4},
    {"scan_shadow", &wdbx_index::opt_scan_shadow},
    {"scan8_wgs", &wdbx_index::opt_scan8_wgs},
    {"scan8_per_query", &wdbx_index::opt_scan8_per_query},
    {"scan_u6", &wdbx_index::opt_scan_u6},
    {"scan_u6_cap", &wdbx_index::opt_scan_u6_cap},
    {"scan_u42", &wdbx_index::opt_scan_u42},
    {"scan_u42_share", &wdbx_index::opt_scan_u42_share},
    {"scan_u42_mfma", &wdbx_index::opt_scan_u42_mfma},
    {"batch_repair", &wdbx_index::opt_batch_repair},
    {"single_min_rows", &wdbx_index::opt_single_min_rows},
    {"range_min_rows", &wdbx_index::opt_range_min_rows},
    {"group_bounds", &wdbx_index::opt_group_bounds},
    {"scan_force_ragged", &wdbx_index::opt_force_ragged},
    {"select_min_k", &wdbx_index::opt_select_min_k},
    {"gemm_min_queries", &wdbx_index::opt_gemm_min_nq},
    {"gemm_min_rows", &wdbx_index::opt_gemm_min_rows},
    {"gemm_min_work", &wdbx_index::opt_gemm_min_work},
    {"gemm_sample_div", &wdbx_index::opt_gemm_sample_div},
    {"gemm_masked", &wdbx_index::opt_gemm_masked},
    {"rows_keys_max", &wdbx_index::opt_rows_keys_max},
    {"distinct_overfetch", &wdbx_index::opt_distinct_overfetch},
    {"multivector_round_vectors", &wdbx_index::opt_multivector_round_vectors},
    {"range_batch_min_queries", &wdbx_index::opt_range_batch_min_queries},
    {"range_pair_cap", &wdbx_index::opt_range_pair_cap},
    {"mmr_scratch_mib", &wdbx_index::opt_mmr_scratch_mib},
    {"groups_segment_rows", &wdbx_index::opt_groups_segment_rows},
};

static int64_t* option_slot(wdbx_index* ix, const char* name) { return find_option(ix, kOptions, name); }

int wdbx_index_set_option(wdbx_index* ix, const char* name, int64_t value) try {
  if (!ix) return fail(WDBX_E_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(ix->mu);
  int64_t* slot = option_slot(ix, name);
  if (!slot) return fail(WDBX_E_INVALID, "unknown option '%s'", name ? name : "(null)");
  if (slot == &ix->opt_gemm8_variant && value != 0 && value != 12 && value != 13 && value != 14)
    return fail(WDBX_E_INVALID, "gemm8_variant %lld: 0 (= 14), 12 and 13 are the forms the library has", (long long)value);
  if (slot == &ix->opt_multivector_round_vectors && (value < 1 || value > MULTIVECTOR_MAX_ROUND))
    return fail(WDBX_E_INVALID, "multivector_round_vectors %lld outside [1, %d]", (long long)value, MULTIVECTOR_MAX_ROUND);
  if (slot == &ix->opt_range_pair_cap && value != 0 && (value < (int64_t)RANGE_PAIR_CAP_MIN || value > (int64_t)RANGE_PAIR_CAP_MAX))
    return fail(WDBX_E_INVALID, "range_pair_cap %lld: 0 (the default sizing) or [%u, %u] pairs per wave", (long long)value,
                RANGE_PAIR_CAP_MIN, RANGE_PAIR_CAP_MAX);
  if (slot == &ix->opt_mmr_scratch_mib && (value < 1 || value > MMR_SCRATCH_MIB_MAX))
    return fail(WDBX_E_INVALID, "mmr_scratch_mib %lld outside [1, %lld]", (long long)value, (long long)MMR_SCRATCH_MIB_MAX);
  if (slot == &ix->opt_groups_segment_rows && (value < GROUPS_SEGMENT_MIN || value > GROUPS_SEGMENT_MAX))
    return fail(WDBX_E_INVALID, "groups_segment_rows %lld outside [%lld, %lld]", (long long)value, (long long)GROUPS_SEGMENT_MIN,
                (long long)GROUPS_SEGMENT_MAX);
  if (slot == &ix->opt_scan_u42_share && value != -1 && value != 1 && value != 2 && value != 4)
    return fail(WDBX_E_INVALID, "scan_u42_share %lld: -1 (the default), 1, 2 or 4 queries per read", (long long)value);
  if (slot == &ix->opt_scan_u42_mfma && value != -1 && value != 0 && value != 1)
    return fail(WDBX_E_INVALID, "scan_u42_mfma %lld: -1 (the default), 0 or 1", (long long)value);
  *slot = value;
  if (!strcmp(name, "group_bounds")) ix->gmax_valid = false;  // re-decide (and rebuild the group maxima) at the next batch
  return WDBX_OK;
} WDBX_CATCH

int wdbx_index_get_option(wdbx_index* ix, const char* name, int64_t* value) try {
  if (!ix || !value) return fail(WDBX_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(ix->mu);
  // read-only state of the batched path
  if (name && !strcmp(name, "last_gemm_family")) return *value = ix->last_gemm_mode, WDBX_OK;
  if (name && !strcmp(name, "shadow_rows")) return *value = (int64_t)ix->shadow_rows, WDBX_OK;
  if (name && !strcmp(name, "shadow_bytes")) return *value = (int64_t)ix->d_rows16.bytes, WDBX_OK;
  if (name && !strcmp(name, "shadow8_rows")) return *value = (int64_t)ix->shadow8_rows, WDBX_OK;
  if (name && !strcmp(name, "shadow8_bytes")) return *value = (int64_t)(ix->d_rows8.bytes + ix->d_scale8.bytes), WDBX_OK;
  if (name && !strcmp(name, "shadowg_rows")) return *value = (int64_t)ix->shadowg_rows, WDBX_OK;
  if (name && !strcmp(name, "shadowg_bytes")) return *value = (int64_t)(ix->d_rows8g.bytes + ix->d_groups8.bytes), WDBX_OK;
  if (name && !strcmp(name, "last_single_path")) return *value = ix->last_single_path, WDBX_OK;
  if (name && !strcmp(name, "last_single_u6")) return *value = ix->last_single_u6, WDBX_OK;
  if (name && (!strcmp(name, "u6_candidates_sum") || !strcmp(name, "u6_candidates_max"))) {
    // the u6 scan's candidate counts of the last round (batch_status reports the cut's short lists); waits for the stream
    const uint32_t nq = ix->last_single_u6 ? std::min<uint32_t>(ix->last_batch_nq, 64) : 0;
    std::vector<uint32_t> c(std::max<uint32_t>(nq, 1), 0u);
    DeviceGuard g(ix->device);
    if (nq) HIP_TRY(hipMemcpyAsync(c.data(), ix->d_count6, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    int64_t sum = 0, mx = 0;
    for (uint32_t v : c) sum += v, mx = std::max<int64_t>(mx, v);
    return *value = name[14] == 's' ? sum : mx, WDBX_OK;
  }
  if (name && !strcmp(name, "last_single_u42")) return *value = ix->last_single_u42, WDBX_OK;
  if (name && !strcmp(name, "last_u42_share")) return *value = ix->last_u42_share, WDBX_OK;
  if (name && !strcmp(name, "last_u42_mfma_groups")) return *value = ix->last_u42_mfma_groups, WDBX_OK;
  if (name && !strcmp(name, "u42_survivors_sum")) {
    // rows that passed the four-bit bound in the last round's full passes; waits for the stream
    const uint32_t nq = ix->last_single_u42 ? std::min<uint32_t>(ix->last_batch_nq, 64) : 0;
    std::vector<uint32_t> c(std::max<uint32_t>(nq, 1), 0u);
    DeviceGuard g(ix->device);
    if (nq) HIP_TRY(hipMemcpyAsync(c.data(), ix->d_count42, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    int64_t sum = 0;
    for (uint32_t v : c) sum += v;
    return *value = sum, WDBX_OK;
  }
  if (name && !strcmp(name, "shadow42_rows")) return *value = (int64_t)ix->shadow42_rows, WDBX_OK;
  if (name && !strcmp(name, "shadow42_bytes")) return *value = (int64_t)ix->d_rows42.bytes, WDBX_OK;
  if (name && !strcmp(name, "shadow6_rows")) return *value = (int64_t)ix->shadow6_rows, WDBX_OK;
  if (name && !strcmp(name, "shadow6_bytes")) return *value = (int64_t)ix->d_rows6.bytes, WDBX_OK;
  if (name && !strcmp(name, "last_range_path")) return *value = ix->last_range_path, WDBX_OK;
  if (name && !strcmp(name, "last_range_batch_path")) return *value = ix->last_range_batch_path, WDBX_OK;
  if (name && !strcmp(name, "last_range_batch_blocks")) return *value = ix->last_range_batch_blocks, WDBX_OK;
  if (name && !strcmp(name, "last_range_batch_pairs")) return *value = ix->last_range_batch_pairs, WDBX_OK;
  if (name && !strcmp(name, "last_range_batch_fallback_queries")) return *value = ix->last_range_batch_fallback, WDBX_OK;
  if (name && !strcmp(name, "last_rows_path")) return *value = ix->last_rows_path, WDBX_OK;
  if (name && !strcmp(name, "last_matrix_path")) return *value = ix->last_matrix_path, WDBX_OK;
  if (name && !strcmp(name, "last_matrix_rounds")) return *value = ix->last_matrix_rounds, WDBX_OK;
  if (name && !strcmp(name, "last_update_launches")) return *value = ix->last_update_launches, WDBX_OK;
  if (name && !strcmp(name, "last_lists_path")) return *value = ix->last_lists_path, WDBX_OK;
  if (name && !strcmp(name, "last_lists_items")) return *value = ix->last_lists_items, WDBX_OK;
  if (name && !strcmp(name, "last_lists_rounds")) return *value = ix->last_lists_rounds, WDBX_OK;
  if (name && !strcmp(name, "last_distinct_path")) return *value = ix->last_distinct_path, WDBX_OK;
  if (name && !strcmp(name, "last_distinct_items")) return *value = ix->last_distinct_items, WDBX_OK;
  if (name && !strcmp(name, "last_distinct_labels")) return *value = ix->last_distinct_labels, WDBX_OK;
  if (name && !strcmp(name, "last_distinct_short")) return *value = ix->last_distinct_short, WDBX_OK;
  if (name && !strcmp(name, "last_multivector_rounds")) return *value = ix->last_multivector_rounds, WDBX_OK;
  if (name && !strcmp(name, "last_multivector_vectors")) return *value = ix->last_multivector_vectors, WDBX_OK;
  if (name && !strcmp(name, "last_multivector_labels")) return *value = ix->last_multivector_labels, WDBX_OK;
  if (name && !strcmp(name, "last_mmr_path")) return *value = ix->last_mmr_path, WDBX_OK;
  if (name && !strcmp(name, "last_recommend_path")) return *value = ix->last_recommend_path, WDBX_OK;
  if (name && !strcmp(name, "last_recommend_short")) return *value = ix->last_recommend_short, WDBX_OK;
  if (name && !strcmp(name, "last_discover_path")) return *value = ix->last_discover_path, WDBX_OK;
  if (name && !strcmp(name, "last_discover_zone_slots")) return *value = ix->last_discover_zone_slots, WDBX_OK;
  if (name && !strcmp(name, "last_groups_path")) return *value = ix->last_groups_path, WDBX_OK;
  if (name && !strcmp(name, "last_groups_tasks")) return *value = ix->last_groups_tasks, WDBX_OK;
  if (name && !strcmp(name, "last_groups_rounds")) return *value = ix->last_groups_rounds, WDBX_OK;
  if (name && !strcmp(name, "last_mmr_rounds")) return *value = ix->last_mmr_rounds, WDBX_OK;
  if (name && !strcmp(name, "last_mmr_candidates")) return *value = ix->last_mmr_candidates, WDBX_OK;
  if (name && !strcmp(name, "last_sample_qn")) return *value = ix->last_sample_qn, WDBX_OK;
  if (name && !strcmp(name, "last_batch_repaired")) return *value = ix->last_batch_repaired ? 1 : 0, WDBX_OK;
  if (name && !strcmp(name, "last_batch_masked")) return *value = ix->last_batch_masked, WDBX_OK;
  // (the last tile call with a mask per query: its classes and tile blocks; 0 after any other call)
  if (name && !strcmp(name, "last_batch_mask_classes")) return *value = ix->last_batch_masked == 2 ? (int64_t)ix->last_batch_classes : 0, WDBX_OK;
  if (name && !strcmp(name, "last_batch_blocks")) return *value = ix->last_batch_masked == 2 ? (int64_t)ix->last_batch_blocks : 0, WDBX_OK;
  if (name && !strcmp(name, "last_batch_allowed_rows")) return *value = (int64_t)ix->last_batch_allowed, WDBX_OK;
  if (name && !strcmp(name, "group_bounds_active")) return *value = ix->group_bounds ? 1 : 0, WDBX_OK;
  if (name && !strcmp(name, "exchanges")) return *value = (int64_t)ix->exchanges, WDBX_OK;
  if (name && !strcmp(name, "device_bytes_resident")) return *value = (int64_t)device_bytes_resident(ix), WDBX_OK;
  int64_t* slot = option_slot(ix, name);
  if (!slot) return fail(WDBX_E_INVALID, "unknown option '%s'", name ? name : "(null)");
  *value = *slot;
  return WDBX_OK;
} WDBX_CATCH

}  // extern "C"
