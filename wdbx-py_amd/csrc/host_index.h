// host_index.h -- host side: the handle, kernel choice and the enqueue functions of every search path.
// Part of the single translation unit wdbx_hip.hip (included there, in order); not a standalone header.

// ------------------------------------------------------------------------------------------------
// host side: the handle
// ------------------------------------------------------------------------------------------------
struct EventPool {
  std::vector<hipEvent_t> ev;        // pairs
  std::vector<uint32_t> launches;    // kernel launches bracketed by each pair (back-to-back launches of ONE kernel share a pair:
  size_t used = 0;                   //  an event record between two kernels costs ~10 us of idle stream)
};

constexpr int STAGE_SLOTS = 4;

// Device memory of the handle and of the shard group: every allocation is a DevBuf member of its owner (bookkeeping:
// host_dispatch.h), allocated and freed here and nowhere else.
struct HipMem {
  static int alloc(void** p, size_t bytes) {
    HIP_TRY(hipMalloc(p, bytes));
    return WDBX_OK;
  }
  static int release(void* p) {
    HIP_TRY(hipFree(p));
    return WDBX_OK;
  }
};
using DevBufs = BufList<HipMem>;
template <class T>
using DevBuf = Buf<T, HipMem>;

struct wdbx_index {
  DevBufs bufs;  // (first: the DevBuf members below link themselves in; option "device_bytes_resident" is its total)
  int device = 0, dim = 0, pitch = 0, metric = 0;
  int cu_count = 256;
  uint64_t n = 0, cap = 0;
  DevBuf<float> d_rows{&bufs};
  hipStream_t stream = nullptr;
  std::mutex mu;
  // scratch (grown on demand, reused)
  DevBuf<u64> d_partials{&bufs};
  DevBuf<u64> d_local_keys{&bufs};
  DevBuf<u64> d_gathered{&bufs};
  DevBuf<float> d_q{&bufs};
  DevBuf<int64_t> d_oidx{&bufs};
  DevBuf<float> d_oscore{&bufs};
  // communicator
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  uint64_t row_base = 0;
  uint64_t exchanges = 0;  // all-gather + merge steps this handle has enqueued (read-only option "exchanges")
  // pinned, device-mapped staging for small blocking searches: the kernels read the query from and
  // write the result to host memory directly (no memcpy calls on the latency path)
  char* h_stage = nullptr;
  char* h_stage_dev = nullptr;
  // STAGE_SLOTS staging blocks: a small blocking call owns one from its enqueue to the moment it has read its results, and
  // waits for the GPU on the slot's event with the handle's mutex released (search_host)
  SlotPool<4> slots;   // (host_dispatch.h; = STAGE_SLOTS)
  hipEvent_t slot_done[4] = {nullptr, nullptr, nullptr, nullptr};
  DevBuf<u64> d_dump{&bufs};  // one key per row (large-k select)
  DevBuf<u64> d_sel{&bufs};
  DevBuf<SelectState> d_state{&bufs};
  DevBuf<uint32_t> d_mask{&bufs};
  const uint32_t* active_mask = nullptr;  // set only for the duration of a masked search (under the mutex)
  uint64_t mask_allowed = 0;              // ... and how many of the rows it allows (popcount of the host mask: set_active_mask)
  // the int8 tiles' bad-row table of ONE masked batch: d_gbad8 | ~mask (gbad_with_mask_kernel); d_gbad8 itself never changes
  DevBuf<u64> d_call_bad{&bufs};
  int last_batch_masked = 0;              // the last batch ran the masked tile pass (1), or the pass with a mask per query (2)
  // a call with one row mask per query (wdbx_index_search_multimask): its queries in slot order, the slots' queries, its masks
  // and the classes' mask numbers in one scratch allocation; what the last such tile call looked like
  DevBuf<char> d_mm{&bufs};
  uint32_t last_batch_classes = 0, last_batch_blocks = 0;
  std::vector<int32_t> last_batch_slot;   // ... and the slot of each of the caller's queries (wdbx_index_batch_status)
  uint64_t last_batch_allowed = 0;        // ... over this many allowed rows
  // batched (GEMM) path scratch
  DevBuf<float> d_qblock{&bufs};
  DevBuf<u64> d_halfmax{&bufs};
  DevBuf<float> d_tau{&bufs};
  DevBuf<u64> d_cand{&bufs};
  DevBuf<uint32_t> d_count{&bufs};
  uint32_t last_batch_nq = 0, last_batch_cap = 0;
  bool last_batch_repaired = false;  // the last batch's overflowed queries were repaired on the device (conditional launches)
  DevBuf<void> d_qb16{&bufs};  // bf16 tiles: the query block as bf16
  DevBuf<float> d_cn{&bufs};  // L2 / bf16 batched path: squared row norms for rows [0, cn_rows), and their maximum
  uint64_t cn_rows = 0;
  DevBuf<void> d_rows16{&bufs};  // bf16 shadow copy of rows [0, shadow_rows), row pitch pitch16 elements (zero padded)
  uint64_t shadow_rows = 0;
  uint32_t pitch16 = 0;
  int last_gemm_mode = 0;  // tile kernel family the last batch ran on (GEMM_FP32 / GEMM_BF16 / GEMM_BF16_SHADOW)
  DevBuf<uint8_t> d_rows8{&bufs};  // u8 shadow copy of rows [0, shadow8_rows) for the single-query selection scan, pitch8 bytes
  DevBuf<float> d_scale8{&bufs};   // its per-row scales
  DevBuf<float> d_gmax{&bufs};     // largest squared row norm per 64-row group (selection bounds of the tile kernels)
  DevBuf<float> d_qn{&bufs};       // |q| per query of a block
  bool gmax_valid = false;
  bool cn_stats_dirty = false; // cached norms were refreshed in place: recompute their statistics before deciding
  bool group_bounds = false;   // per-group bounds (norms vary a lot) or one global bound (they do not: cheaper epilogue)
  DevBuf<void> d_selsrc{&bufs};    // device-side SelectSrc of the large-k selection epilogue
  uint64_t shadow8_rows = 0;
  uint32_t pitch8 = 0;
  uint64_t u8_no_room_cap = ~0ull;  // capacity at which the u8 shadow last failed to allocate
  // u6 shadow copy of rows [0, shadow6_rows) for rounds of single queries (kernels_scan6.h): ONE allocation, the six-bit codes
  // in 64-row tiles of units6 units followed by the per-row {s, a} pairs
  DevBuf<uint32_t> d_rows6{&bufs};
  uint64_t shadow6_rows = 0, rows6_tiles = 0;
  uint32_t units6 = 0;
  uint64_t u6_no_room_cap = ~0ull;
  DevBuf<uint32_t> d_count6{&bufs};  // its candidate counters (d_count holds the cut's: what the repair launches look at)
  int last_single_u6 = 0;      // 1: the last single-query search selected on the u6 shadow (last_single_path stays 2)
  // the u6 codes once more in two planes (kernels_scan42.h): ONE allocation, the h plane in 64-row tiles of units42 units,
  // the per-row {s, a4} pairs, the l records of lpitch42 dwords per row
  DevBuf<uint32_t> d_rows42{&bufs};
  uint64_t shadow42_rows = 0, rows42_tiles = 0;
  uint32_t units42 = 0;
  uint64_t u42_no_room_cap = ~0ull;
  DevBuf<uint32_t> d_count42{&bufs};  // rows that passed the four-bit bound, per query of the last round
  int last_single_u42 = 0;     // 1: the last u6 round's full passes ran over the split planes
  int last_u42_share = 0;      // ... the widest group of queries that shared one read of the four-bit plane in the last call (0: none ran)
  DevBuf<uint32_t> d_q16{&bufs};   // the round's 16-bit queries as matrix operands, then its U42QConst (u42_query_i16_kernel)
  int last_u42_mfma_groups = 0;  // ... the groups of 16 whose full pass ran on the matrix cores in the last call
  uint32_t* defer_flag_dev = nullptr;  // non-null during a blocking call that repairs overflow itself (mapped host word)
  // a lone blocking call through a staging slot: the LAST kernel of its chain writes done_seq into done_flag_dev (a mapped
  // host word of the slot) and the caller polls that word instead of waiting on the runtime; done_signals counts the launches
  // that took the signal (exactly one, or the caller waits on its event as before)
  uint32_t* done_flag_dev = nullptr;
  uint32_t done_seq = 0, lone_seq = 0;
  int done_signals = 0;
  DevBuf<uint32_t> d_ticket{&bufs};        // merge_kernel's workgroup ticket for that signal when a small batch is merged (zero between launches)
  // a lone blocking query whose final top-k the HOST takes (search_host): the re-scored candidates' keys and their count go
  // to these mapped host locations and no final merge is launched; lone_cap_max = keys the host area holds
  u64* lone_keys_dev = nullptr;
  uint32_t* lone_count_dev = nullptr;
  uint32_t lone_cap_max = 0;
  bool lone_used = false;              // set by the enqueue when it took that form
  int last_single_path = 0;    // 0 fp32 scan, 1 bf16 tiles, 2 u8 scan (what the last single-query search ran on)
  int last_sample_qn = 1;      // queries per workgroup of the last u8 sample launch (1, 3 or 4: scan8_sample4_kernel)
  DevBuf<uint32_t> d_cnmax{&bufs};
  // group-scaled i8 shadow copy of the rows for the int8 tiles (kernels_tiles8.h): rows [0, shadowg_rows) quantised
  DevBuf<int8_t> d_rows8g{&bufs};
  DevBuf<f4> d_groups8{&bufs};       // per 64-row group {s_g, a_g, b_g, vouch}
  DevBuf<uint32_t> d_over_list{&bufs};  // {n, q_0 ..}: the overflowed queries of a batch block, for its repair scan (mark_lost_kernel)
  DevBuf<float> d_gref8{&bufs};      // {a_ref, b_ref, sum a, sum b} + a counter: the prefilter epilogue's ordinary-group bounds
  bool gref_valid = false;       // (recomputed when the group table changed)
  DevBuf<u64> d_gbad8{&bufs};        // per 64-row group: bits of the rows that hold a NaN (removed rows) or lie past the end
  uint64_t shadowg_rows = 0;
  uint64_t shadowg_tail_n = ~0ull;  // the row count for which the groups behind the last row (to the end of its 256-row tile) were last written
  uint32_t pitch8g = 0;
  uint64_t i8g_no_room_cap = ~0ull;
  DevBuf<int8_t> d_qb8{&bufs};       // the query block as i8
  DevBuf<f4> d_qpar{&bufs};          // its per-query parameters
  DevBuf<u64> d_pairs{&bufs};        // the tile waves' candidate (query, row) pairs and how many each wave produced
  DevBuf<uint32_t> d_pair_count{&bufs};
  // range search (wdbx_index_range_search): per-query key buffers of the selection candidates and of the results, their
  // counters ([0, 64) candidates, [64, 128) results) and thresholds ([0, 64) exact, [64, 128) selection scale); the per-query
  // capacities grow to the exact count after an overflow and stay there
  DevBuf<u64> d_rcand{&bufs};
  DevBuf<u64> d_rkeys{&bufs};
  DevBuf<uint32_t> d_rcnt{&bufs};
  DevBuf<float> d_rthr{&bufs};
  uint32_t range_cand_cap = 16384, range_out_cap = 16384;
  int last_range_path = 0;     // 0 fp32 range scan, 2 u8 selection scan + exact filter (what the last range search ran on)
  // batched range search (wdbx_index_range_search_batch): its candidates live in d_cand, its pairs in d_pairs, its result keys,
  // counters and thresholds in the buffers above ([0, 256) each); what the last call did (host_range_batch.h)
  // candidates per query of a block: grows to the exact count after an overflow and stays there up to RANGE_BATCH_KEEP_CAP
  // (host_range_batch.h); a call that grew past that releases d_cand / d_rkeys at its end and falls back to it
  uint32_t range_batch_cap = 1024;
  int last_range_batch_path = 0;
  int64_t last_range_batch_blocks = 0, last_range_batch_pairs = 0, last_range_batch_fallback = 0;
  // search among listed rows (wdbx_index_search_rows): the device copy of the call's row list and, on the key routes, one key
  // per listed row and query of a round; the partial lists of the list route live in d_partials
  DevBuf<uint32_t> d_sub_ids{&bufs};
  DevBuf<u64> d_sub_keys{&bufs};
  int last_rows_path = 0;      // 0 nothing launched (empty list), 1 keys + merge, 2 lists + merge, 3 keys + radix select
  // distance matrix among listed rows (wdbx_index_search_matrix): list, keys and lists live where the listed-row search keeps them
  int last_matrix_path = 0;    // as last_rows_path
  int64_t last_matrix_rounds = 0;
  // one row list per query (wdbx_index_search_row_lists): the call's work items, then its slots' list lengths; the lists' rows
  // and the round's keys live in d_sub_ids / d_sub_keys
  DevBuf<char> d_rl{&bufs};
  int last_lists_path = 0;     // 0 nothing launched, 1 the batched pass only, 2 both, 3 list by list only
  int64_t last_lists_items = 0, last_lists_rounds = 0;
  // distinct search (wdbx_index_search_distinct): the labels of rows [0, labels.size()) on the host (rows behind them are
  // WDBX_LABEL_NONE; empty = no label was ever set) and the device copy of the label order (host_labels.h) in one allocation:
  // rows | dense label of each position | first item of each span | first item of each label.  Rebuilt by the next full pass
  // after a label change (lab_valid) or a row-count change (lab_n).  The pass's keys live in d_sub_keys, its lists in d_partials.
  std::vector<uint32_t> labels;
  DevBuf<char> d_lab{&bufs};
  bool lab_valid = false;
  uint64_t lab_n = 0;
  uint32_t lab_items = 0, lab_labels = 0, lab_spans = 0;
  size_t lab_off_dense = 0, lab_off_span = 0, lab_off_label = 0;
  int last_distinct_path = 0;  // 0 nothing launched, 1 over-fetch alone, 2 over-fetch + full pass for the short queries, 3 full pass
  int64_t last_distinct_items = 0, last_distinct_labels = 0, last_distinct_short = 0;
  // multi-vector search (wdbx_index_search_multivector): the smallest row of each label of that label order, on the host (what a
  // ranked label position is reported as), and one allocation of the call's state: the fp32 accumulator of the query a round
  // boundary cuts, [lab_labels], then the segments of every round (host_multivector.h).  Keys and lists as the distinct search.
  std::vector<uint32_t> lab_row0;
  DevBuf<char> d_mv{&bufs};
  int64_t last_multivector_rounds = 0, last_multivector_vectors = 0, last_multivector_labels = 0;
  // MMR search (wdbx_index_search_mmr): one allocation of the largest round's state (host_mmr.h): the query table | the candidates'
  // row numbers | their relevance | the picks' values | the gathered rows | the similarity squares
  DevBuf<char> d_mmr{&bufs};
  int last_mmr_path = 0;  // 0 nothing launched, 1 ran
  int64_t last_mmr_rounds = 0, last_mmr_candidates = 0;
  // recommend search (wdbx_index_search_recommend): one allocation of the call's tables (host_recommend.h): the example table of
  // every query | that of the short queries | the exclusion list.  The examples live in d_q, keys in d_sub_keys, lists in d_partials.
  DevBuf<char> d_rec{&bufs};
  int last_recommend_path = 0;  // 0 nothing launched, 1 favoured pass only, 2 both passes
  int64_t last_recommend_short = 0;
  // discovery search (wdbx_index_search_discover): one allocation of a round's state (host_discover.h): target mode's records (keys |
  // wins) | the zones' counts | the query table | the zone table | the exclusion list.  Vectors in d_q, keys in d_sub_keys, lists
  // in d_partials.
  DevBuf<char> d_disc{&bufs};
  int last_discover_path = 0;  // 0 nothing launched, 1 context mode, 2 target mode
  int64_t last_discover_zone_slots = 0;
  // search groups (wdbx_index_search_groups / _group_members): where each dense label's run lies in the label order, on the host
  // (host_groups.h; rebuilt with the label order), and one allocation of a call's tables: the slot table | the round's tasks |
  // the slots' counts.  Queries in d_q, partial lists in d_partials, members in d_oidx / d_oscore.
  LabelRuns lab_runs;
  DevBuf<char> d_grp{&bufs};
  int last_groups_path = 0;  // 0 nothing launched, 1 ran
  int64_t last_groups_tasks = 0, last_groups_rounds = 0;
  // writes of listed rows (wdbx_index_set_rows_at / wdbx_index_remove_rows, host_update.h): the call's row list followed by its
  // distinct int8 groups, and the block of caller rows one scatter round carries; kernel launches of the last such call
  DevBuf<uint32_t> d_upd_list{&bufs};
  DevBuf<float> d_upd_rows{&bufs};
  int64_t last_update_launches = 0;
  // profiling
  bool profile = false;
  EventPool scan_ev, merge_ev, gemm_ev, sample_ev;
  // options
  int64_t opt_lanes = 0, opt_blocks = 0, opt_nt = 1, opt_blocked = 0, opt_batch = 32, opt_generic = 0;
  int64_t opt_group_bounds = -1, opt_single_min_rows = 131072, opt_scan8_wgs = -1, opt_scan8_per_query = -1,
          opt_batch_repair = 1, opt_scan_shadow = 2, opt_gemm_bf16 = 3, opt_gemm8_variant = 0,
          opt_gemm8_refine = 1, opt_scan8_sample4 = 1, opt_gemm_l2 = 1, opt_gemm_l2_i8 = 1, opt_force_ragged = 0,
          opt_gemm_ct = 0, opt_wg_merge = 1, opt_zero_copy = 1, opt_lone_host_select = 1, opt_lds_lists = 0,
          opt_merge_fast = 1, opt_poll_done = 1, opt_scan_one_grid = 1, opt_select_min_k = 200, opt_gemm_min_nq = 4, opt_gemm_min_rows = 65536, opt_gemm_min_work = 800000,
          opt_gemm_sample_div = 0, opt_range_min_rows = 131072, opt_scan_u6 = -1, opt_scan_u6_cap = 0, opt_scan_u42 = -1, opt_scan_u42_share = -1, opt_scan_u42_mfma = -1, opt_gemm_masked = 1, opt_rows_keys_max = 8192, opt_distinct_overfetch = 4,
          opt_multivector_round_vectors = 256, opt_range_batch_min_queries = 4, opt_range_pair_cap = 0,
          opt_mmr_scratch_mib = MMR_SCRATCH_MIB_MAX, opt_groups_segment_rows = GROUPS_SEGMENT_DEFAULT;
};

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// A call's row mask (uint32 words, bit r % 32 of word r / 32 = row r may be returned; the caller has checked that it holds
// ceil(rows / 32) words): to the handle's one mask buffer, behind the stream's earlier work.  The caller keeps the handle's
// mutex and resets active_mask at the end of the call.  The allowed rows are counted here, on the host copy (bits past the
// last row do not count): the batched dispatch sizes its sample by them without asking the device.
static int set_active_mask(wdbx_index* ix, const uint32_t* mask_words) {
  const size_t words = (size_t)((ix->n + 31) / 32);
  int rc = ix->d_mask.grow(words * sizeof(uint32_t));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(ix->d_mask, mask_words, words * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
  ix->mask_allowed = mask_allowed_rows(mask_words, ix->n);
  ix->active_mask = ix->d_mask;
  return WDBX_OK;
}

// ... and the reset: a row mask applies to one call (one enqueue of the shard group) only.  armed from the start where the
// call sets a mask in every case, or by set() where it may return before it has changed the handle.
struct MaskScope {
  wdbx_index* ix;
  bool armed;
  explicit MaskScope(wdbx_index* ix_, bool armed_ = false) : ix(ix_), armed(armed_) {}
  ~MaskScope() {
    if (armed) ix->active_mask = nullptr;
  }
  int set(const uint32_t* mask_words) {
    armed = true;
    return set_active_mask(ix, mask_words);
  }
};

// the one check of a mask's length against the row count (under the handle's lock: a mask built before a concurrent add is
// refused instead of over-read); label says whose mask: "row mask", "row mask 3", "shard 2: row mask"
static int check_mask_words(uint64_t n_rows, uint64_t mask_word_count, const char* label = "row mask") {
  const uint64_t words = (n_rows + 31) / 32;
  if (mask_word_count >= words) return WDBX_OK;
  return fail(WDBX_E_INVALID, "%s of %llu words for %llu rows (%llu words needed)", label, (u64)mask_word_count, (u64)n_rows, (u64)words);
}

// n host rows of src_pitch floats (their first dim floats count) to dst at the row pitch, behind the stream's earlier work: one
// copy when the pitches agree, else the padding is zeroed first
static int copy_padded(wdbx_index* ix, float* dst, const float* src, uint64_t n, int src_pitch) {
  const size_t bytes = (size_t)n * ix->pitch * sizeof(float);
  if (src_pitch == ix->pitch) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ix->stream));
  } else {
    HIP_TRY(hipMemsetAsync(dst, 0, bytes, ix->stream));
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)ix->pitch * sizeof(float), src, (size_t)src_pitch * sizeof(float), (size_t)ix->dim * sizeof(float), n,
                             hipMemcpyHostToDevice, ix->stream));
  }
  return WDBX_OK;
}

// the result buffers of the blocking calls, for at least elems results (contents never preserved)
static int ensure_out(wdbx_index* ix, size_t elems) {
  const int rc = ix->d_oidx.grow(elems * sizeof(int64_t));
  return rc ? rc : ix->d_oscore.grow(elems * sizeof(float));
}

// Wait for a lone call's completion word (mapped host memory; the chain's last kernel writes seq behind its results,
// merge_signal_done): a poll of the word -- 5 us less than the runtime's completion path (profiles/r04/poll/) -- with a look at
// the event the caller recorded behind the chain every 4 096 spins, which is how a failed launch would surface.
static inline int wait_done_word(volatile uint32_t* word, uint32_t seq, hipEvent_t ev) {
  for (uint32_t spins = 1;; ++spins) {
    if (*word == seq) break;
    if ((spins & 0xFFFu) == 0) {
      const hipError_t e = hipEventQuery(ev);
      if (e == hipSuccess) break;  // (the kernel has ended: its stores are visible)
      if (e != hipErrorNotReady) HIP_TRY(hipEventSynchronize(ev));
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);  // (the results are read after the word, not before)
  return WDBX_OK;
}

// ---- scan dispatch ------------------------------------------------------------------------------
struct ScanChoice {
  scan_fn fn = nullptr;
  int L = 8;
  bool generic = false;
  size_t lds_extra = 0;  // bytes beyond the 4 lists
};

static bool use_select(const wdbx_index* ix, int k) { return ix->opt_select_min_k > 0 && k >= ix->opt_select_min_k; }

static ScanChoice scan_choice_of(const ScanForm& f, scan_fn fn, int pitch4) {
  ScanChoice c;
  c.fn = fn;
  c.L = f.L;
  c.generic = f.generic;
  c.lds_extra = scan_lds_extra(f.generic, pitch4);
  return c;
}

// the handle's scan kernel at this k: the form by the shape rule (host_scan_plan.h: scan_form), the instance by the pickers next
// to the kernels (kernels_scan.h)
static ScanChoice choose_scan(const wdbx_index* ix, int k) {
  const int reg = scan_list_mode(use_select(ix, k), k, ix->opt_lds_lists != 0);
  const int pitch4 = ix->pitch / 4;
  ScanForm f = scan_form(pitch4, ix->opt_lanes, ix->opt_generic != 0, ix->opt_force_ragged != 0);
  scan_fn fn = pick_scan_form(f, ix->metric, ix->opt_nt != 0, reg);
  if (!fn) {  // (scan_has_instance and pick_specialised disagree: the generic kernel serves any pitch)
    f = scan_generic_form(pitch4);
    fn = pick_scan_form(f, ix->metric, false, reg);
  }
  return scan_choice_of(f, fn, pitch4);
}

struct LaunchPlan {
  ScanChoice sc;
  uint32_t blocks = 0, P = 0, groups = 0, chunk = 0;
  bool wg_merge = false;
  size_t lds = 0;
};

// listed: the plan of the listed repair scan (scan_kernel_listed, generic body) instead of the handle's own scan kernel
static int plan_scan(wdbx_index* ix, int k, LaunchPlan* out, bool listed = false) {
  LaunchPlan lp;
  if (listed) {
    const int pitch4 = ix->pitch / 4;
    const ScanForm f = scan_generic_form(pitch4);
    lp.sc = scan_choice_of(f, pick_listed(f.L, ix->metric, scan_list_mode(false, k, ix->opt_lds_lists != 0)), pitch4);
  } else {
    lp.sc = choose_scan(ix, k);
  }
  lp.groups = scan_groups(ix->n, lp.sc.L);
  lp.lds = scan_lds_bytes(use_select(ix, k), k, lp.sc.lds_extra);
  if (scan_lds_needs_attribute(lp.lds))
    HIP_TRY(hipFuncSetAttribute((const void*)lp.sc.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lp.lds));
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)lp.sc.fn, 256, lp.lds));
  if (per_cu < 1) return fail(WDBX_E_INVALID, "scan kernel does not fit a CU at k=%d (LDS %zu B)", k, lp.lds);
  lp.blocks = scan_blocks((uint32_t)ix->cu_count, per_cu, ix->opt_blocks, lp.groups);
  lp.wg_merge = ix->opt_wg_merge != 0;
  lp.P = scan_partial_lists(lp.wg_merge, lp.blocks);
  lp.chunk = scan_chunk(ix->opt_blocked != 0, lp.groups, lp.blocks);
  *out = lp;
  return WDBX_OK;
}

static int record(EventPool& pool, bool enabled, hipStream_t s, bool start, uint32_t launches = 1) {
  if (!enabled) return WDBX_OK;
  if (start) {
    if (pool.used + 2 > pool.ev.size()) {
      if (pool.ev.size() >= 2 * 65536) return WDBX_OK;  // pool exhausted: stop sampling
      for (int i = 0; i < 2; ++i) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        pool.ev.push_back(e);
      }
      pool.launches.resize(pool.ev.size() / 2, 1);
    }
    HIP_TRY(hipEventRecord(pool.ev[pool.used], s));
  } else if (pool.used + 2 <= pool.ev.size()) {
    HIP_TRY(hipEventRecord(pool.ev[pool.used + 1], s));
    pool.launches[pool.used / 2] = launches;
    pool.used += 2;
  }
  return WDBX_OK;
}

static int launch_merge(wdbx_index* ix, const MergeArgs& m_in, int nq) {
  MergeArgs m = m_in;
  m.no_fast = ix->opt_merge_fast ? 0 : 1;
  if (ix->done_flag_dev && (nq == 1 || ix->d_ticket) && (m.out_idx || m.out_score) && !m.only_if_over) {  // the call's final ranking
    m.done_flag = ix->done_flag_dev;
    m.done_seq = ix->done_seq;
    m.done_ticket = ix->d_ticket;
    ++ix->done_signals;
  }
  MergeLaunch ml;  // (waves, LDS, instance: kernels_merge_select.h)
  HIP_TRY(merge_launch_for(m.k, ix->opt_lds_lists != 0, &ml));
  int rc = record(ix->merge_ev, ix->profile, ix->stream, true);
  if (rc) return rc;
  HIP_TRY(enqueue_merge(ix->stream, ml, m, nq));
  return record(ix->merge_ev, ix->profile, ix->stream, false);
}

// ---- what the listed-row, label and corpus calls share ------------------------------------------------
// One launch of 256-thread workgroups between the two records of `pool`; a kernel whose dynamic LDS passes 64 KiB gets its limit
// raised first -- a runtime call on EVERY such launch, so a site that launches in a loop of rounds with lists in LDS raises the
// limit once before the loop and keeps its bracket written out (wdbx_index_search_matrix passes its lists' LDS and reaches the raise
// only with k = WDBX_MAX_K lists in LDS, once per round of 256 anchors; every other caller passes lds = 0);
// so does a site that launches twice inside one bracket or counts more than one launch per bracket.
template <typename Fn, typename Args>
static int launch_bracketed(wdbx_index* ix, EventPool& pool, Fn fn, dim3 grid, size_t lds, const Args& a) {
  if (lds >= 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int rc = record(pool, ix->profile, ix->stream, true);
  if (rc) return rc;
  hipLaunchKernelGGL(fn, grid, dim3(256), lds, ix->stream, a);
  HIP_TRY(hipGetLastError());
  return record(pool, ix->profile, ix->stream, false);
}

// What a round's scoring launch left to rank, slot after slot:
//   LISTS   n partial lists of k sorted keys per slot ([slot][k][n]) -> one merge launch
//   SELECT  n keys per slot -> per slot the radix-select chain and the sort of its k keys, inside one merge bracket each
//   KEYS    n keys per slot, ranked as unsorted candidates by one merge launch; P_dev (optional): each slot's own count
struct RankSource {
  enum Form { LISTS, SELECT, KEYS } form;
  const u64* in;
  uint64_t n;
  const uint32_t* P_dev;
};

// the scratch of a round: partial lists, or keys and -- on the select route only -- the chain's state
static int grow_rank_scratch(wdbx_index* ix, RankSource::Form form, size_t scratch_u64) {
  int rc;
  if (form == RankSource::LISTS) return ix->d_partials.grow(scratch_u64 * sizeof(u64));
  if ((rc = ix->d_sub_keys.grow(scratch_u64 * sizeof(u64))) || form == RankSource::KEYS) return rc;
  if ((rc = ix->d_sel.grow((size_t)WDBX_MAX_K * sizeof(u64)))) return rc;
  return ix->d_state.grow(sizeof(SelectState));
}

// The ranking tail of `b` slots: their best k into d_oidx / d_oscore from slot `first` on.  metric: what converts a key's value
// to the caller's score (recommend's disfavoured side passes the other metric, discovery's context mode cosine).
static int enqueue_rank_tail(wdbx_index* ix, const RankSource& src, int first, int b, int k, int metric) {
  int rc;
  MergeArgs m = {};
  m.k = k;
  m.metric = metric;
  if (src.form == RankSource::SELECT) {
    const uint32_t sgrid = radix_select_grid(src.n, ix->cu_count);
    for (int q = 0; q < b; ++q) {
      if ((rc = record(ix->merge_ev, ix->profile, ix->stream, true))) return rc;
      HIP_TRY(enqueue_radix_select(ix->stream, src.in + (size_t)q * src.n, (u64)src.n, nullptr, (SelectState*)ix->d_state,
                                   (u64*)ix->d_sel, (uint32_t)k, sgrid));
      m.out_idx = ix->d_oidx + (size_t)(first + q) * k;
      m.out_score = ix->d_oscore + (size_t)(first + q) * k;
      HIP_TRY(enqueue_sort_out(ix->stream, (const u64*)ix->d_sel, (const SelectState*)ix->d_state, m));
      if ((rc = record(ix->merge_ev, ix->profile, ix->stream, false))) return rc;
    }
    return WDBX_OK;
  }
  const bool lists = src.form == RankSource::LISTS;
  m.in = src.in;
  m.q_stride = lists ? (uint64_t)k * src.n : src.n;
  m.i_stride = lists ? src.n : 0;
  m.p_stride = 1;
  m.P = (uint32_t)src.n;
  m.P_dev = src.P_dev;
  m.list_len = lists ? k : 1;
  m.out_idx = ix->d_oidx + (size_t)first * k;
  m.out_score = ix->d_oscore + (size_t)first * k;
  return launch_merge(ix, m, b);
}

// ---- the steps the selection rounds share (their plan: host_selection.h) ------------------------------------------
static_assert(SELECTION_BLOCK_QUERIES == GB_N, "host_selection.h sizes the pair lists for the widest query block");

// The thresholds of nv queries from their sampled lower bounds in d_halfmax (`bounds` per query) into d_tau: the k-th largest
// bound, a rigorous lower bound of each query's true k-th best score.  allow_kth: by kth_score_kernel where the bounds fit it
// (at most 2^-15 relative below the k-th largest), else -- and always on the legacy tiles -- by the list merge.
static int enqueue_sample_threshold(wdbx_index* ix, uint32_t bounds, int k, int nv, bool allow_kth) {
  int rc;
  if (allow_kth && bounds <= (uint32_t)KTH_R * 1024 && !ix->opt_lds_lists) {
    KthArgs ka = {ix->d_halfmax, (u64)bounds, bounds, k, ix->d_tau};
    if ((rc = record(ix->merge_ev, ix->profile, ix->stream, true))) return rc;
    HIP_TRY(enqueue_kth(ix->stream, ka, nv));
    return record(ix->merge_ev, ix->profile, ix->stream, false);
  }
  MergeArgs m = {};
  m.in = ix->d_halfmax;
  m.q_stride = bounds;
  m.i_stride = 0;
  m.p_stride = 1;
  m.P = bounds;
  m.list_len = 1;
  m.k = k;
  m.metric = ix->metric;
  m.out_kth = ix->d_tau;
  return launch_merge(ix, m, nv);
}

// The final ranking of a round: per query the best k of its d_count[q] (at most cap) re-scored keys at in + q * cap.
static MergeArgs final_topk_args(const wdbx_index* ix, const u64* in, uint32_t cap, const uint32_t* d_count, int k) {
  MergeArgs f = {};
  f.in = in;
  f.q_stride = cap;
  f.i_stride = 0;
  f.p_stride = 1;
  f.P = cap;
  f.P_dev = d_count;
  f.list_len = 1;
  f.k = k;
  f.metric = ix->metric;
  return f;
}

// ... and where it goes, for the queries from q0 on: keys with global rows for the caller's own exchange (keys_out), this
// shard's lists with global rows for the exchange that follows (sharded), or the results themselves
static void final_topk_output(const wdbx_index* ix, MergeArgs* f, u64* keys_out, bool sharded, int64_t* d_out_idx, float* d_out_score,
                              int q0, int k) {
  if (keys_out) {
    f->row_base = (uint32_t)ix->row_base;
    f->out_keys = keys_out + (size_t)q0 * k;
  } else if (sharded) {
    f->row_base = (uint32_t)ix->row_base;
    f->out_keys = ix->d_local_keys;
  } else {
    f->out_idx = d_out_idx + (size_t)q0 * k;
    f->out_score = d_out_score + (size_t)q0 * k;
  }
}

// The life cycle of a shadow copy's allocations (u8: codes and scales; i8 groups: rows, table and bad-row bits; bf16, u6, u42: one
// each).  SHADOW_KEPT: the shape is the same and every part is large enough, nothing was done.  Else the parts are released,
// *shadow_rows restarts at 0 and they are allocated anew: SHADOW_FRESH, or SHADOW_NO_ROOM (= 0) with every part released and
// the capacity remembered in *no_room_cap so that the next calls at this capacity do not try again.
enum { SHADOW_NO_ROOM = 0, SHADOW_KEPT = 1, SHADOW_FRESH = 2 };
struct ShadowPart {
  BufBase<HipMem>* buf;
  size_t need;
};
static int shadow_room(wdbx_index* ix, bool shape_changed, std::initializer_list<ShadowPart> parts, uint64_t* shadow_rows,
                       uint64_t* no_room_cap) {
  bool stale = shape_changed;
  for (const ShadowPart& s : parts) stale = stale || s.buf->bytes < s.need;
  if (!stale) return SHADOW_KEPT;
  if (*no_room_cap == ix->cap) return SHADOW_NO_ROOM;
  for (const ShadowPart& s : parts) (void)s.buf->release();
  *shadow_rows = 0;
  for (const ShadowPart& s : parts) {
    if (s.buf->try_grow(s.need)) continue;
    for (const ShadowPart& r : parts) (void)r.buf->release();
    *no_room_cap = ix->cap;
    return SHADOW_NO_ROOM;
  }
  return SHADOW_FRESH;
}

// all-gather this rank's key lists [b, k] (global rows) and merge the nranks lists per query
static int exchange_and_merge(wdbx_index* ix, int b, int k, int64_t* d_out_idx, float* d_out_score) {
  int rc = ix->d_gathered.grow((size_t)ix->nranks * b * k * sizeof(u64));
  if (rc) return rc;
  // per-shard records [b, k] -> [nranks, b, k] on every rank (tiny: latency-bound)
  NCCL_TRY(ncclAllGather(ix->d_local_keys, ix->d_gathered, (size_t)b * k, ncclUint64, ix->comm, ix->stream));
  ++ix->exchanges;
  MergeArgs m = {};
  m.list_len = k;
  m.in = ix->d_gathered;
  m.q_stride = (uint64_t)k;
  m.i_stride = 1;
  m.p_stride = (uint64_t)b * k;
  m.P = (uint32_t)ix->nranks;
  m.k = k;
  m.metric = ix->metric;
  m.out_idx = d_out_idx;
  m.out_score = d_out_score;
  return launch_merge(ix, m, b);
}

// Enqueue nq searches.  Caller holds the handle's mutex and has made its device current.
// mode: 0 = final results of this shard alone; 1 = per-rank shard group (all-gather through the
// handle's communicator + second merge); 2 = only this shard's key list (global rows) into keys_dst [nq, k] (a buffer
// of the caller, who runs the exchange: the in-process shard group, host_group.h) or, without one, d_local_keys
enum { SEARCH_FINAL = 0, SEARCH_SHARDED = 1, SEARCH_LOCAL_KEYS = 2 };

static int enqueue_search_gemm(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx, float* d_out_score,
                               int mode, int count_slot, u64* keys_out);
struct MultiCall;
static int enqueue_search_gemm8(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx, float* d_out_score, int mode,
                                u64* keys_out, const MultiCall* mc = nullptr);
static bool shadow_single_eligible(const wdbx_index* ix, int k, int nq_call);
static bool u8_single_eligible(const wdbx_index* ix, int k, int nq_call);
static int enqueue_singles_u8(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx, float* d_out_score,
                              u64* keys_out, bool candidates_only = false);
static bool prepare_u8_shadow(wdbx_index* ix);
static bool u6_single_eligible(const wdbx_index* ix, int k, int nq_call);
static bool prepare_u6_shadow(wdbx_index* ix);
static int enqueue_singles_u6(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx, float* d_out_score,
                              u64* keys_out, bool u42);
static bool u42_single_eligible(const wdbx_index* ix);
static bool prepare_u42_shadow(wdbx_index* ix);

static int enqueue_search(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx,
                          float* d_out_score, int mode, u64* keys_dst = nullptr) {
  const bool keys_only = mode == SEARCH_LOCAL_KEYS;
  const bool sharded = mode != SEARCH_FINAL;  // the local stage ends in keys with global rows
  if (nq <= 0) return WDBX_OK;
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  if (!d_queries || (!keys_only && (!d_out_idx || !d_out_score))) return fail(WDBX_E_INVALID, "null device buffer");
  if (mode == SEARCH_SHARDED && !ix->comm) return fail(WDBX_E_STATE, "sharded search before wdbx_index_comm_init");
  if (ix->n >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "shard holds too many rows for 32-bit row keys");

  const int batch = keys_only ? nq : (int)std::max<int64_t>(1, std::min<int64_t>(ix->opt_batch, 1024));
  int rc;
  if (ix->n == 0 && !keys_dst) {
    // empty shard: every local list is empty (the reference returns [] at indexing.py:998)
    rc = ix->d_local_keys.grow((size_t)batch * k * sizeof(u64));
    if (rc) return rc;
  }
  LaunchPlan lp;
  const bool select = ix->n && use_select(ix, k);
  if (ix->n) {
    rc = plan_scan(ix, k, &lp);
    if (rc) return rc;
    if (select) {
      if ((rc = ix->d_dump.grow((size_t)ix->n * sizeof(u64)))) return rc;
      if ((rc = ix->d_sel.grow((size_t)WDBX_MAX_K * sizeof(u64)))) return rc;
      if ((rc = ix->d_state.grow(sizeof(SelectState)))) return rc;
    } else {
      rc = ix->d_partials.grow((size_t)batch * k * lp.P * sizeof(u64));
      if (rc) return rc;
    }
  }
  // SEARCH_SHARDED: the rounds of `batch` queries keep their size (the small kernels around the scans are shared per round),
  // but the all-gather + merge are issued once per EXCHANGE CHUNK of up to 1024 queries: an all-gather costs ~0.2 ms of
  // stream time whatever it carries (measured with one rank: 87.8 vs 81.0 us per query at 1.25 M rows when issued per 32)
  const int xch = keys_only ? nq : batch * std::max(1, 1024 / batch);
  if (sharded) {
    if (!keys_dst) {
      rc = ix->d_local_keys.grow((size_t)std::min(xch, std::max(nq, batch)) * k * sizeof(u64));
      if (rc) return rc;
    }
    if (!keys_only) {
      rc = ix->d_gathered.grow((size_t)ix->nranks * std::min(xch, std::max(nq, batch)) * k * sizeof(u64));
      if (rc) return rc;
    }
  }

  u64* const lbase = keys_dst ? keys_dst : ix->d_local_keys;  // (keys_only: one batch, so offsets within it are offsets in keys_dst)
  ix->last_u42_share = 0;
  ix->last_u42_mfma_groups = 0;
  for (int q0 = 0; q0 < nq; q0 += batch) {
    const int b = std::min(batch, nq - q0);
    u64* const lkeys = lbase ? lbase + (size_t)(q0 % xch) * k : nullptr;  // this round's lists inside the exchange chunk
    if (select) {
      // large k: per query  scan (key per row) -> radix select -> compact -> sort
      const uint32_t sgrid_rows = radix_select_grid(ix->n, ix->cu_count);
      // On the u8 selection scan the chain below ranks the query's re-scored CANDIDATES; the key-per-row fp32 scan
      // is then only the conditional repair of an overflowed candidate buffer, and a device-side descriptor picks
      // which of the two the chain reads.
      const bool u8 = u8_single_eligible(ix, k, nq) && prepare_u8_shadow(ix);  // (also for the in-process group's local stage)
      ix->last_single_path = u8 ? 2 : 0;
      ix->last_single_u6 = 0;
      ix->last_single_u42 = 0;
      SelectSrc* src = nullptr;
      if (u8) {
        if ((rc = ix->d_count.grow(((size_t)batch + 2 * GB_N) * sizeof(uint32_t)))) return rc;
        if ((rc = ix->d_selsrc.grow(sizeof(SelectSrc)))) return rc;
        src = (SelectSrc*)ix->d_selsrc.p;
      }
      for (int q = 0; q < b; ++q) {
        ScanArgs sa = {};
        if (u8) {
          rc = enqueue_singles_u8(ix, d_queries + (size_t)(q0 + q) * ix->pitch, 1, k, nullptr, nullptr, nullptr, true);
          if (rc) return rc;
          sa.only_if_over = ix->d_count;
          sa.over_cap = ix->last_batch_cap;
        }
        sa.rows = (const f4*)ix->d_rows.p;
        sa.query = (const f4*)(d_queries + (size_t)(q0 + q) * ix->pitch);
        sa.partials = ix->d_dump;
        sa.mask = ix->active_mask;
        sa.n_rows = (uint32_t)ix->n;
        sa.pitch4 = (uint32_t)(ix->pitch / 4);
        sa.groups = lp.groups;
        sa.chunk = lp.chunk;
        sa.k = k;
        sa.wg_merge = lp.wg_merge ? 1 : 0;
        if (!u8 && (rc = record(ix->scan_ev, ix->profile, ix->stream, true))) return rc;
        hipLaunchKernelGGL(lp.sc.fn, dim3(lp.blocks), dim3(256), lp.lds, ix->stream, sa);
        HIP_TRY(hipGetLastError());
        if (!u8 && (rc = record(ix->scan_ev, ix->profile, ix->stream, false))) return rc;
        if ((rc = record(ix->merge_ev, ix->profile, ix->stream, true))) return rc;
        // (on the selection scan the chain's grid is sized for the candidate buffer; the rare repair walks the N keys
        // with the same, smaller grid)
        const uint32_t sgrid = u8 ? std::min<uint32_t>(sgrid_rows, (ix->last_batch_cap + 255) / 256) : sgrid_rows;
        if (u8)
          hipLaunchKernelGGL(select_source_kernel, dim3(1), dim3(64), 0, ix->stream, src, (const uint32_t*)ix->d_count,
                             ix->last_batch_cap, (const u64*)ix->d_cand, (const u64*)ix->d_dump, (u64)ix->n);
        HIP_TRY(enqueue_radix_select(ix->stream, (const u64*)ix->d_dump, (u64)ix->n, (const SelectSrc*)src, (SelectState*)ix->d_state,
                                     (u64*)ix->d_sel, (uint32_t)k, sgrid));
        MergeArgs m = {};
        m.k = k;
        m.metric = ix->metric;
        m.row_base = (uint32_t)ix->row_base;
        m.out_keys = sharded ? lkeys + (size_t)q * k : nullptr;
        m.out_idx = sharded ? nullptr : d_out_idx + (size_t)(q0 + q) * k;
        m.out_score = sharded ? nullptr : d_out_score + (size_t)(q0 + q) * k;
        HIP_TRY(enqueue_sort_out(ix->stream, (const u64*)ix->d_sel, (const SelectState*)ix->d_state, m));
        if ((rc = record(ix->merge_ev, ix->profile, ix->stream, false))) return rc;
      }
    } else if (ix->n) {
      // Single queries on a reduced-precision shadow copy: each query makes ITS OWN selection pass (threshold from
      // a sample, every row whose score could reach it under a rigorous error bound becomes a candidate, the
      // candidates are re-scored in fp32 from the fp32 rows).  Preferred: the u8 scan (a quarter of the fp32 bytes,
      // query kept in fp32, per-row bounds, honours row masks); else the bf16 tile kernel with one live column
      // (half the bytes).  The fp32 scan and its merge still follow, but as REPAIR launches that return at once
      // unless that query's candidate buffer overflowed (massive near-duplicates) -- the result is exact either
      // way, without a host round trip (a blocking caller with one query does the check itself: defer_flag_dev).
      const bool u8 = u8_single_eligible(ix, k, nq) && prepare_u8_shadow(ix);  // (also for the in-process group's local stage)
      const bool shadow = u8 || (!keys_only && shadow_single_eligible(ix, k, nq));
      ix->last_single_path = u8 ? 2 : shadow ? 1 : 0;
      // rounds on a large shard select on the six-bit shadow instead (0.76 of the u8 bytes per pass; kernels_scan6.h)
      const bool u6 = u8 && u6_single_eligible(ix, k, nq) && prepare_u6_shadow(ix);
      ix->last_single_u6 = u6 ? 1 : 0;
      // ... and make the full passes over the split planes where those serve the shape (0.68 of the u6 bytes; kernels_scan42.h)
      const bool u42 = u6 && u42_single_eligible(ix) && prepare_u42_shadow(ix);
      ix->last_single_u42 = u42 ? 1 : 0;
      if (shadow) {
        if ((rc = ix->d_count.grow(((size_t)batch + 2 * GB_N) * sizeof(uint32_t)))) return rc;
        if (u6)
          rc = enqueue_singles_u6(ix, d_queries + (size_t)q0 * ix->pitch, b, k, d_out_idx ? d_out_idx + (size_t)q0 * k : nullptr,
                                  d_out_score ? d_out_score + (size_t)q0 * k : nullptr, sharded ? lkeys : nullptr, u42);
        else if (u8)  // the u8 selection scan: a quarter of the fp32 bytes per query
          rc = enqueue_singles_u8(ix, d_queries + (size_t)q0 * ix->pitch, b, k, d_out_idx ? d_out_idx + (size_t)q0 * k : nullptr,
                                  d_out_score ? d_out_score + (size_t)q0 * k : nullptr, sharded ? lkeys : nullptr);
        else     // the bf16 tile kernel with one live column: half the fp32 bytes
          rc = enqueue_search_gemm(ix, d_queries + (size_t)q0 * ix->pitch, b, k, d_out_idx + (size_t)q0 * k,
                                   d_out_score + (size_t)q0 * k, SEARCH_FINAL, 0, sharded ? lkeys : nullptr);
        if (rc) return rc;
      }
      if (u8 && ix->defer_flag_dev) continue;  // the blocking caller repairs an overflow after its synchronisation
      // shadow paths: the fp32 scans below are REPAIR launches (they return at once unless the query's candidate buffer
      // overflowed), so the round's b of them go out as ONE grid of b rows (4.4 us per empty launch otherwise);
      // fp32 path: one timed launch per query -- or, for a round of several queries over a corpus of at most 1 GiB, ONE grid
      // with a row per query (blockIdx.y, as the repair launches): every query still makes its own pass over all rows, but the
      // passes run side by side out of the caches and the launches' fixed ~9 us are paid once per round, not per query
      // (10 k rows: 8 queries 90 -> 3x us, profiles/r04/small_batch/).  Larger corpora: a launch per query, as the u8 scan
      // does beyond 1 GiB (two passes streaming different regions at once cost more than the gaps between launches)
      const bool one_grid = !shadow && b > 1 && ix->opt_scan_one_grid && (uint64_t)ix->n * ix->pitch * sizeof(float) <= (1ull << 30);
      for (int q = 0; q < ((shadow || one_grid) ? 1 : b); ++q) {
        ScanArgs sa = {};
        if (shadow) {
          sa.only_if_over = ix->d_count + q;
          sa.over_cap = ix->last_batch_cap;
        }
        if (shadow || one_grid) sa.y_partials = (uint32_t)((size_t)k * lp.P);
        sa.rows = (const f4*)ix->d_rows.p;
        sa.query = (const f4*)(d_queries + (size_t)(q0 + q) * ix->pitch);
        sa.partials = ix->d_partials + (size_t)q * k * lp.P;
        sa.mask = ix->active_mask;
        sa.n_rows = (uint32_t)ix->n;
        sa.pitch4 = (uint32_t)(ix->pitch / 4);
        sa.groups = lp.groups;
        sa.chunk = lp.chunk;
        sa.k = k;
        sa.wg_merge = lp.wg_merge ? 1 : 0;
        // (repair launches are not timed: they would read as scans of zero length)
        rc = shadow ? WDBX_OK : record(ix->scan_ev, ix->profile, ix->stream, true);
        if (rc) return rc;
        hipLaunchKernelGGL(lp.sc.fn, dim3(lp.blocks, (shadow || one_grid) ? b : 1), dim3(256), lp.lds, ix->stream, sa);
        HIP_TRY(hipGetLastError());
        rc = shadow ? WDBX_OK : record(ix->scan_ev, ix->profile, ix->stream, false, one_grid ? (uint32_t)b : 1u);
        if (rc) return rc;
      }
      MergeArgs m = {};
      if (shadow) {
        m.only_if_over = ix->d_count;
        m.over_cap = ix->last_batch_cap;
      }
      m.list_len = k;
      m.in = ix->d_partials;
      m.q_stride = (uint64_t)k * lp.P;
      m.i_stride = lp.P;
      m.p_stride = 1;
      m.P = lp.P;
      m.k = k;
      m.metric = ix->metric;
      m.row_base = (uint32_t)ix->row_base;
      m.idx_base = 0;
      m.out_keys = sharded ? lkeys : nullptr;
      m.out_idx = sharded ? nullptr : d_out_idx + (size_t)q0 * k;
      m.out_score = sharded ? nullptr : d_out_score + (size_t)q0 * k;
      rc = launch_merge(ix, m, b);
      if (rc) return rc;
    } else if (sharded) {
      HIP_TRY(hipMemsetAsync(lkeys, 0, (size_t)b * k * sizeof(u64), ix->stream));
    } else {
      // no rows: idx = -1 (all bits set), score = 0
      HIP_TRY(hipMemsetAsync(d_out_idx + (size_t)q0 * k, 0xFF, (size_t)b * k * sizeof(int64_t), ix->stream));
      HIP_TRY(hipMemsetAsync(d_out_score + (size_t)q0 * k, 0, (size_t)b * k * sizeof(float), ix->stream));
    }
    if (mode == SEARCH_SHARDED && ((q0 + b) % xch == 0 || q0 + b == nq)) {  // the chunk is complete: exchange it
      const int c0 = q0 / xch * xch, c = q0 + b - c0;
      rc = exchange_and_merge(ix, c, k, d_out_idx + (size_t)c0 * k, d_out_score + (size_t)c0 * k);
      if (rc) return rc;
    }
  }
  return WDBX_OK;
}


// The conditional repair of a batched block (the device-side form of what wdbx_index_search does on the host): for each
// of the block's nv queries whose candidate counter exceeds the capacity -- its selection result may be incomplete -- the
// exact fp32 scan + merge, as ONE grid of nv rows that returns at once for every other query (4 us when nothing
// overflowed).  Writes the same outputs the block's final merge wrote.  *done = false when this shape has no device-side
// repair (k in the radix-select range, or partial lists beyond 256 MiB): the caller then leaves it to the host, as before.
static int enqueue_batch_repair(wdbx_index* ix, const float* qsrc, int nv, int k, uint32_t* d_count_block, uint32_t cap,
                                int64_t* out_idx, float* out_score, u64* out_keys, bool* done, const uint32_t* d_lost = nullptr) {
  *done = false;
  int rc;
  LaunchPlan lp;
  bool go = ix->n && !use_select(ix, k) && ix->opt_batch_repair;
  size_t need = 0;
  if (go) {
    if ((rc = plan_scan(ix, k, &lp, true))) return rc;
    need = (size_t)nv * k * lp.P * sizeof(u64);
    if (need > ((size_t)256 << 20)) go = false;
  }
  if (go && (rc = ix->d_over_list.grow((GB_N + 1) * sizeof(uint32_t)))) return rc;
  // (after the exact passes consumed the buffers) a lost pair marks every query of the BLOCK as overflowed -- nobody knows
  // which of them lost a candidate; and the overflowed queries are listed for the repair scan
  if (go || d_lost) {
    hipLaunchKernelGGL(mark_lost_kernel, dim3(1), dim3(256), 0, ix->stream, d_count_block, (uint32_t)nv, d_lost, cap,
                       go ? ix->d_over_list : (uint32_t*)nullptr);
    HIP_TRY(hipGetLastError());
  }
  if (!go) return WDBX_OK;
  if ((rc = ix->d_partials.grow(need))) return rc;
  ScanArgs sa = {};
  sa.over_list = ix->d_over_list;
  sa.y_partials = (uint32_t)((size_t)k * lp.P);
  sa.rows = (const f4*)ix->d_rows.p;
  sa.query = (const f4*)qsrc;
  sa.partials = ix->d_partials;
  sa.mask = ix->active_mask;  // (a masked batch: its overflowed queries are repaired by the masked scan)
  sa.n_rows = (uint32_t)ix->n;
  sa.pitch4 = (uint32_t)(ix->pitch / 4);
  sa.groups = lp.groups;
  sa.chunk = lp.chunk;
  sa.k = k;
  sa.wg_merge = lp.wg_merge ? 1 : 0;
  // a few grid rows share the listed queries (none listed: the grid returns at once)
  hipLaunchKernelGGL(lp.sc.fn, dim3(lp.blocks, std::min(nv, 4)), dim3(256), lp.lds, ix->stream, sa);
  HIP_TRY(hipGetLastError());
  MergeArgs m = {};
  m.only_if_over = d_count_block;
  m.over_cap = cap;
  m.list_len = k;
  m.in = ix->d_partials;
  m.q_stride = (uint64_t)k * lp.P;
  m.i_stride = lp.P;
  m.p_stride = 1;
  m.P = lp.P;
  m.k = k;
  m.metric = ix->metric;
  m.row_base = (uint32_t)ix->row_base;
  m.out_keys = out_keys;
  m.out_idx = out_idx;
  m.out_score = out_score;
  if ((rc = launch_merge(ix, m, nv))) return rc;
  *done = true;
  return WDBX_OK;
}

// ---- batched queries on the MFMA path ----------------------------------------------------------
static bool i8_tiles_eligible(const wdbx_index* ix);
static bool gemm_eligible(const wdbx_index* ix, int nq, int k) {
  if (ix->metric == WDBX_METRIC_L2 && !ix->opt_gemm_l2) return false;
  // From how many queries a call shares ONE pass: gemm_min_queries (4).  On the i8 tiles a small batch costs little more
  // than one scan (10 M x 384: 0.71 ms for up to 16 queries against 0.60 ms per single query), so on large shards two
  // coalesced callers already share a pass -- unless the option was raised to keep batching off.
  int64_t min_nq = ix->opt_gemm_min_nq;
  if (min_nq > 2 && min_nq <= 4 && ix->n >= 3000000 && ix->i8g_no_room_cap != ix->cap && i8_tiles_eligible(ix)) min_nq = 2;
  if (nq < min_nq || (uint64_t)k * 8 * GB_M > ix->n) return false;
  if ((int64_t)ix->n >= 2 * ix->opt_gemm_min_rows) return true;
  // Below 2 x gemm_min_rows the alternative is the fp32 scan with a round's queries as one grid, whose cost grows with
  // queries x rows (0.2-0.25 ns each; cheaper per row on the larger corpora) while a matrix-core batch costs its ~130-180 us of
  // launches whatever it holds: the tiles from queries x rows >= gemm_min_work below gemm_min_rows (measured, d = 384: 21 k rows
  // from 36 queries, 40 k from 18, 60 k from 12) and from 0.65 of it between gemm_min_rows and twice that (70 k rows from 8
  // queries, 100 k from 6): profiles/r04/small_batch/
  if (ix->opt_gemm_min_work <= 0) return (int64_t)ix->n >= ix->opt_gemm_min_rows;
  const uint64_t work = (int64_t)ix->n >= ix->opt_gemm_min_rows ? (uint64_t)ix->opt_gemm_min_work * 13 / 20 : (uint64_t)ix->opt_gemm_min_work;
  return (uint64_t)nq * ix->n >= work;
}

// single queries take the shadow selection pipeline (see enqueue_search) when the bf16 shadow is in use, no row
// mask is active (the tiles do not read masks) and k is served by the list kernels (the repair launch)
// rows from which a selection path pays: its 6 launches pipeline behind each other when a call carries several
// queries, but a lone query waits for each of them (measured, d = 384: 65 k rows 60 vs 41 us, equal at 262 k)
static inline int64_t selection_min_rows(const wdbx_index* ix, int nq_call) {
  return nq_call > 1 ? ix->opt_gemm_min_rows : std::max(ix->opt_gemm_min_rows, ix->opt_single_min_rows);
}

static bool shadow_single_eligible(const wdbx_index* ix, int k, int nq_call) {
  if (ix->opt_scan_shadow <= 0 || ix->opt_gemm_bf16 < 2 || ix->active_mask || use_select(ix, k)) return false;
  if (ix->metric == WDBX_METRIC_L2 && !ix->opt_gemm_l2) return false;
  // the shadow pads rows to 128 elements: for short rows it is no smaller than the fp32 rows (d = 32: twice
  // the bytes, measured 0.54x; d = 64: 0.98x; d = 100: 1.4x) -- worth it from 0.8 of the fp32 bytes down
  const uint64_t pitch16 = ((uint64_t)ix->pitch + 127) / 128 * 128;
  if (pitch16 * 2 * 10 > (uint64_t)ix->pitch * 4 * 8) return false;
  return (int64_t)ix->n >= selection_min_rows(ix, nq_call) && (uint64_t)k * 8 * GB_M <= ix->n;
}

// ---- single queries on the u8 selection scan ---------------------------------------------------
static bool u8_single_eligible(const wdbx_index* ix, int k, int nq_call) {
  if (ix->opt_scan_shadow < 2) return false;  // (row masks and k >= 200 are served by the u8 scan too)
  const Scan8Shape* sh = scan8_shape((uint32_t)ix->dim);
  // worth it from 0.6 of the fp32 bytes down (d = 32 would read as many bytes as the fp32 row)
  if (!sh || (uint64_t)sh->pieces * 16 * 10 > (uint64_t)ix->pitch * 4 * 6) return false;
  return (int64_t)ix->n >= selection_min_rows(ix, nq_call) && (uint64_t)k * 8 * GB_M <= ix->n;
}

// Allocates / refreshes the u8 shadow and its scales for the rows added or overwritten since the last search.
// false = no room for it on the device (remembered per capacity): the caller stays on the other paths.
static bool prepare_u8_shadow(wdbx_index* ix) {
  const Scan8Shape* sh = scan8_shape((uint32_t)ix->dim);
  if (!sh) return false;
  const uint32_t pitch8 = sh->pieces * 16;
  const size_t need = ((size_t)ix->cap + TILE_PAD_ROWS) * pitch8, need_s = ((size_t)ix->cap + TILE_PAD_ROWS) * sizeof(float);
  if (!shadow_room(ix, ix->pitch8 != pitch8, {{&ix->d_rows8, need}, {&ix->d_scale8, need_s}},
                   &ix->shadow8_rows, &ix->u8_no_room_cap))
    return false;
  ix->pitch8 = pitch8;
  if (ix->shadow8_rows < ix->n) {
    const uint32_t blocks = rows_to_u8_grid(ix->n - ix->shadow8_rows);
    hipLaunchKernelGGL(rows_to_u8_kernel, dim3(blocks), dim3(256), 0, ix->stream, (const float*)ix->d_rows, (u64)ix->shadow8_rows,
                       (u64)ix->n, (uint32_t)ix->dim, (uint32_t)ix->pitch, ix->d_rows8, pitch8, ix->d_scale8);
    if (hipGetLastError() != hipSuccess) return false;
    ix->shadow8_rows = ix->n;
  }
  return true;
}

// ---- range search (wdbx_index_range_search) -------------------------------------------------------
// the u8 selection applies as for a lone top-k query (u8_single_eligible's shape and size rules; k plays no part)
static bool range_u8_eligible(const wdbx_index* ix) {
  if (ix->opt_scan_shadow < 2) return false;
  const Scan8Shape* sh = scan8_shape((uint32_t)ix->dim);
  if (!sh || (uint64_t)sh->pieces * 16 * 10 > (uint64_t)ix->pitch * 4 * 6) return false;
  return (int64_t)ix->n >= ix->opt_range_min_rows;
}

// squared fp32 norms of the rows added since they were last computed (the L2 selection paths' |c|^2 term), and their
// running maximum / sum / count
static int ensure_row_norms(wdbx_index* ix) {
  int rc;
  if ((rc = ix->d_cnmax.grow(4 * sizeof(uint32_t)))) return rc;
  if (ix->d_cn.bytes < (size_t)ix->n * sizeof(float)) {
    if ((rc = ix->d_cn.grow((size_t)ix->cap * sizeof(float)))) return rc;
    ix->cn_rows = 0;
  }
  if (ix->cn_rows == 0) HIP_TRY(hipMemsetAsync(ix->d_cnmax, 0, 4 * sizeof(uint32_t), ix->stream));
  if (ix->cn_rows < ix->n) {
    const uint32_t blocks = row_sqnorm_grid(ix->n - ix->cn_rows);
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3(blocks), dim3(256), 0, ix->stream, (const float*)ix->d_rows, (u64)ix->cn_rows,
                       (u64)ix->n, (uint32_t)ix->pitch, ix->d_cn, ix->d_cnmax);
    HIP_TRY(hipGetLastError());
    ix->cn_rows = ix->n;
    ix->gmax_valid = false;
  }
  return WDBX_OK;
}

// nq single queries, each with its own sample pass + full pass over the u8 shadow; thresholds, re-scoring and
// the final top-k run once per round of 32 queries.  Candidate counters at d_count[0 .. nq) (sized by the caller).
// candidates_only (k >= 200, one query per call): thresholds by radix select, no final top-k -- the re-scored
// candidates stay in d_cand[0 .. d_count[0]) for the caller's select chain.
static int enqueue_singles_u8(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx, float* d_out_score,
                              u64* keys_out, bool candidates_only) {
  const Scan8Shape* sh = scan8_shape((uint32_t)ix->dim);
  if (!sh) return fail(WDBX_E_STATE, "no u8 scan instance for dim %d", ix->dim);
  const bool l2 = ix->metric == WDBX_METRIC_L2;
  const uint32_t pitch8 = sh->pieces * 16;
  int rc;
  if (ix->d_rows8.bytes < ((size_t)ix->cap + TILE_PAD_ROWS) * pitch8 || ix->pitch8 != pitch8 || ix->shadow8_rows < ix->n)
    return fail(WDBX_E_STATE, "u8 shadow not prepared");
  if (l2 && (rc = ensure_row_norms(ix))) return rc;  // squared fp32 norms of the rows (the 2 w - |c|^2 form)
  // the plan (host_selection.h): sampled 256-row tiles of 4 groups of 64 rows each, as on the tile path; a larger sample for
  // a larger k; 32 x the expected rows as candidates
  const SelectionSample s = selection_sample(ix->n, 256, 4, k, selection_div(ix->opt_gemm_sample_div, k, true));
  const uint32_t sample_tiles = s.sample_tiles, stride = s.stride, ngroups = s.bounds;
  if (ngroups < (uint32_t)k) return fail(WDBX_E_STATE, "corpus too small for the selection scan at k=%d", k);
  const uint32_t cap = selection_cap(s.expect, 32);
  constexpr int ROUND = 64;  // queries per round at most (the caller hands over `exchange_batch` = 32 queries at a time by default)
  if ((rc = ix->d_halfmax.grow((size_t)ROUND * ngroups * sizeof(u64)))) return rc;
  if ((rc = ix->d_tau.grow((size_t)GB_N * sizeof(float)))) return rc;
  if ((rc = ix->d_cand.grow((size_t)ROUND * cap * sizeof(u64)))) return rc;
  if (ix->d_count.bytes < ((size_t)nq + GB_N) * sizeof(uint32_t)) return fail(WDBX_E_STATE, "candidate counters not sized by the caller");
  ix->last_batch_nq = (uint32_t)nq;  // (the sample launch resets each query's candidate counter)
  ix->last_batch_cap = cap;
  scan8_fn f0 = l2 ? pick_scan8<0, WDBX_METRIC_L2>(sh->L, sh->QPL) : pick_scan8<0, WDBX_METRIC_COSINE>(sh->L, sh->QPL);
  scan8_fn f1 = l2 ? pick_scan8<1, WDBX_METRIC_L2>(sh->L, sh->QPL) : pick_scan8<1, WDBX_METRIC_COSINE>(sh->L, sh->QPL);
  if (!f0 || !f1) return fail(WDBX_E_STATE, "no u8 scan instance for %d lanes x %d loads", sh->L, sh->QPL);
  const uint32_t R = 64u / (uint32_t)sh->L;
  const uint32_t groups1 = (uint32_t)((ix->n + R - 1) / R);
  // workgroups per CU in the full pass's grid (2 fit at once: 8 waves per CU).  Shards of about 1 - 2.7 M rows at d = 384 -- the
  // strong-scaling shard sizes of 4 and 8 GPUs: a round's passes go out as one grid there -- take 6: with three times as many,
  // shorter workgroups per pass the tail of one query's pass overlaps the start of the next one's instead of the two resident
  // workgroups of every CU walking through prologue and tail in step (1.25 M rows 12 545 -> 12 782 q/s, 2.5 M 6 246 -> 6 512;
  // 400 k rows lose with more than 2, 5 M and 10 M rows do not care: profiles/r04/small_shard/summary.txt).  -1 = by size.
  const bool over_1gib = shadow_over_1gib(ix->n, pitch8);
  const int64_t wgs_auto = (nq > 1 && (uint64_t)ix->n * pitch8 >= (400ull << 20) && !over_1gib) ? 6 : 2;  // (measured on rounds)
  const uint32_t wgs = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(ix->opt_scan8_wgs > 0 ? ix->opt_scan8_wgs : wgs_auto, 8));
  const uint32_t grid1 = scan_full_grid(groups1, (uint32_t)ix->cu_count, wgs);
  const uint32_t grid0 = scan_sample_grid(ngroups, (uint32_t)ix->cu_count);
  const size_t pitch4 = ix->pitch / 4;

  for (int q0 = 0; q0 < nq; q0 += ROUND) {
    const int nv = std::min(ROUND, nq - q0);
    const float* qsrc = d_queries + (size_t)q0 * ix->pitch;
    Scan8Args a = {};
    a.rows8 = (const u4v*)ix->d_rows8.p;
    a.scale = ix->d_scale8;
    a.cn = ix->d_cn;
    a.n_rows = (uint32_t)ix->n;
    a.mask = ix->active_mask;
    a.pieces = sh->pieces;
    a.qquads = (uint32_t)pitch4;
    a.num_tiles = sample_tiles;
    a.tile_stride = stride;
    a.sample_nt = (uint64_t)ngroups * 64 * (pitch8 + 4) > (48ull << 20);  // beyond ~48 MB the sample does not stay cached
    a.cap = cap;
    // phase 0, all queries of the round in one launch: maxima of the lower bounds over the sampled groups
    a.query = (const f4*)qsrc;
    a.halfmax = ix->d_halfmax;
    a.count = ix->d_count + q0;
    if ((rc = record(ix->sample_ev, ix->profile, ix->stream, true))) return rc;
    // a sample too large for the L2s (non-temporal loads) is read once per four (QPL = 3: three) queries of the round
    // (scan8_sample4_kernel).  Measured per round of 32 queries: 10 M x 384 top-10 (121 MB per query, served by the Infinity
    // Cache) 560 -> 363 us; 10 M x 768 L2 top-100 (772 MB per query, from HBM) about 3.9 -> 1.6 ms = 755 -> 797 q/s.
    scan8_fn f04 = ((a.sample_nt || ix->opt_scan8_sample4 == 2) && nv >= 4 && ix->opt_scan8_sample4)  // (2: also on a small sample, for tests)
                       ? (l2 ? pick_scan8_sample4<WDBX_METRIC_L2>(sh->L, sh->QPL) : pick_scan8_sample4<WDBX_METRIC_COSINE>(sh->L, sh->QPL))
                       : nullptr;
    ix->last_sample_qn = 1;
    if (f04) {
      const int qn = sh->QPL >= 3 ? 3 : 4;
      ix->last_sample_qn = qn;
      a.nq = (uint32_t)nv;
      hipLaunchKernelGGL(f04, dim3(grid0, (nv + qn - 1) / qn), dim3(256), 0, ix->stream, a);
    } else {
      hipLaunchKernelGGL(f0, dim3(grid0, nv), dim3(256), 0, ix->stream, a);
    }
    HIP_TRY(hipGetLastError());
    if ((rc = record(ix->sample_ev, ix->profile, ix->stream, false))) return rc;
    // a lone blocking query whose final top-k the host takes (3 dependent launches instead of 5): possible when its
    // candidate buffer fits the mapped host area; the threshold is then taken inside phase 1 when the sample is small
    const bool lone = ix->lone_keys_dev && nq == 1 && !candidates_only && !keys_out && cap <= ix->lone_cap_max;
    // (the in-kernel threshold also serves a lone query of the asynchronous entry points and of the shard group's local stage)
    const bool tau_in_kernel = nq == 1 && !candidates_only && k <= 128 && ngroups <= 1024 && ix->opt_lone_host_select;
    if (tau_in_kernel) {
      // (phase 1 takes the k-th largest sampled lower bound itself)
    } else if (candidates_only) {  // large k: the k-th largest sampled lower bound by radix select (the list kernels are insert-bound)
      if (nv != 1) return fail(WDBX_E_STATE, "large-k selection runs one query per call");
      if ((rc = ix->d_state.grow(sizeof(SelectState)))) return rc;
      const uint32_t hgrid = std::min<uint32_t>((ngroups + 255) / 256, (uint32_t)ix->cu_count * 4);
      HIP_TRY(enqueue_radix_select(ix->stream, (const u64*)ix->d_halfmax, (u64)ngroups, nullptr, (SelectState*)ix->d_state, nullptr,
                                   (uint32_t)k, hgrid));
      hipLaunchKernelGGL(select_kth_value_kernel, dim3(1), dim3(64), 0, ix->stream, (const SelectState*)ix->d_state, (uint32_t)k,
                         ix->d_tau);
      HIP_TRY(hipGetLastError());
    } else if ((rc = enqueue_sample_threshold(ix, ngroups, k, nv, true))) {
      return rc;
    }
    // phase 1: every row whose upper bound reaches the threshold.  Every query makes its own pass over all rows; the
    // round's passes go out as ONE grid on small shards (grid.y = query: no launch gaps, ramps and tails overlap; option
    // scan8_per_query: -1 by size, 0 always one grid, 1 a launch per query).  One event pair around them: the profile
    // reports elapsed / passes.
    if ((rc = record(ix->gemm_ev, ix->profile, ix->stream, true))) return rc;
    a.query = (const f4*)qsrc;
    a.tau = ix->d_tau;
    a.cand = ix->d_cand;
    a.count = ix->d_count + q0;
    if (tau_in_kernel) {
      a.tau_keys = ix->d_halfmax;
      a.tau_n = ngroups;
      a.tau_k = k;
    }
    // (measured, d = 384: 1.25 M rows 84.5 vs 86.9 us per pass in one grid; 10 M rows 603 vs 591 us -- two passes streaming
    // different regions at once cost more there than the gaps between launches.  -1 = by size: one grid up to 1 GiB of shadow)
    const bool one_grid = ix->opt_scan8_per_query == 0 || (ix->opt_scan8_per_query < 0 && !over_1gib);
    if (one_grid && nv > 1) {
      hipLaunchKernelGGL(f1, dim3(grid1, nv), dim3(256), 0, ix->stream, a);
      HIP_TRY(hipGetLastError());
    } else {
      for (int i = 0; i < nv; ++i) {
        a.query = (const f4*)(qsrc + (size_t)i * ix->pitch);
        a.tau = ix->d_tau + i;
        a.cand = ix->d_cand + (size_t)i * cap;
        a.count = ix->d_count + q0 + i;
        hipLaunchKernelGGL(f1, dim3(grid1), dim3(256), 0, ix->stream, a);
        HIP_TRY(hipGetLastError());
      }
    }
    if ((rc = record(ix->gemm_ev, ix->profile, ix->stream, false, (uint32_t)nv))) return rc;
    // exact fp32 scores for the candidates, from the fp32 rows
    hipLaunchKernelGGL(l2 ? rescore_kernel<WDBX_METRIC_L2> : rescore_kernel<WDBX_METRIC_COSINE>, dim3(256, nv), dim3(256), 0,
                       ix->stream, (const f4*)ix->d_rows.p, (uint32_t)pitch4, (const f4*)qsrc, ix->d_cand,
                       (const uint32_t*)(ix->d_count + q0), cap, lone ? ix->lone_keys_dev : (u64*)nullptr,
                       lone ? ix->lone_count_dev : (uint32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    if (candidates_only) continue;  // the caller's select chain ranks them
    if (lone) {  // the host ranks the keys after its synchronisation
      ix->lone_used = true;
      continue;
    }
    MergeArgs f = final_topk_args(ix, ix->d_cand, cap, ix->d_count + q0, k);
    f.over_out = ix->defer_flag_dev ? ix->defer_flag_dev + q0 : nullptr;
    final_topk_output(ix, &f, keys_out, false, d_out_idx, d_out_score, q0, k);
    if ((rc = launch_merge(ix, f, nv))) return rc;
  }
  return WDBX_OK;
}

// ---- rounds of single queries on the u6 selection scan (kernels_scan6.h) ---------------------------------------
// Where the u8 scan is eligible AND: inner product / cosine, k <= 32, no row mask, a call of several queries (a lone query
// keeps the u8 scan's short chain), rows of whole 16-element units.  Option scan_u6: -1 = shards whose u8 shadow exceeds
// 1 GiB (where a pass per launch is the rule and the bytes of a pass are the step), 0 = never, 1 = wherever eligible.
static bool u6_single_eligible(const wdbx_index* ix, int k, int nq_call) {
  if (ix->opt_scan_u6 == 0 || ix->metric == WDBX_METRIC_L2 || ix->active_mask || k > 32 || nq_call < 2) return false;
  if (ix->pitch % 16 != 0 || ix->pitch > 4096 || !u6_unit_chunk((uint32_t)ix->pitch / 16)) return false;
  const Scan8Shape* sh = scan8_shape((uint32_t)ix->dim);
  if (ix->opt_scan_u6 < 0 && (!sh || !shadow_over_1gib(ix->n, sh->pieces * 16))) return false;
  return true;
}

// the three parts of the split planes' allocation, and their quantiser over rows [first, end)
static inline f2v* u42_sa4(const wdbx_index* ix) { return (f2v*)(ix->d_rows42 + (size_t)ix->rows42_tiles * ix->units42 * 256); }
static inline uint32_t* u42_lrec(const wdbx_index* ix) { return (uint32_t*)(u42_sa4(ix) + (size_t)ix->rows42_tiles * 64); }
static hipError_t launch_rows_to_u42(wdbx_index* ix, uint64_t first, uint64_t end) {
  hipLaunchKernelGGL(rows_to_u42_kernel, dim3(rows_to_u42_grid(end - first)), dim3(256), 0, ix->stream, (const float*)ix->d_rows, (u64)first,
                     (u64)end, (uint32_t)ix->dim, (uint32_t)ix->pitch, ix->units42, ix->d_rows42, u42_sa4(ix), u42_lrec(ix),
                     u42_lpitch(ix->units42));
  return hipGetLastError();
}

// Allocates / refreshes the u6 shadow for the rows added since the last search that took this path (the life cycle of
// prepare_u8_shadow).  false = no room on the device (remembered per capacity): the caller stays on the u8 scan.
static bool prepare_u6_shadow(wdbx_index* ix) {
  const uint32_t units = (uint32_t)ix->pitch / 16;
  const uint64_t tiles = ((uint64_t)ix->cap + 63) / 64;
  const size_t need = (size_t)tiles * units * 768 + (size_t)tiles * 64 * sizeof(f2v);
  if (!shadow_room(ix, ix->units6 != units || ix->rows6_tiles != tiles, {{&ix->d_rows6, need}}, &ix->shadow6_rows,
                   &ix->u6_no_room_cap))
    return false;
  ix->units6 = units;
  ix->rows6_tiles = tiles;
  if (ix->shadow6_rows < ix->n) {
    const uint32_t blocks = rows_to_u6_grid(ix->n - ix->shadow6_rows);
    hipLaunchKernelGGL(rows_to_u6_kernel, dim3(blocks), dim3(256), 0, ix->stream, (const float*)ix->d_rows, (u64)ix->shadow6_rows,
                       (u64)ix->n, (uint32_t)ix->dim, (uint32_t)ix->pitch, units, ix->d_rows6,
                       (f2v*)(ix->d_rows6 + (size_t)ix->rows6_tiles * units * 192));
    if (hipGetLastError() != hipSuccess) return false;
    ix->shadow6_rows = ix->n;
  }
  return true;
}

// The split planes behind a u6 round (kernels_scan42.h): rows of whole 32-element units.  Option scan_u42: -1 = where the u6
// scan is taken by its size rule (the u8 shadow exceeds 1 GiB), 0 = never, 1 = wherever the u6 scan is taken.
static bool u42_single_eligible(const wdbx_index* ix) {
  if (ix->opt_scan_u42 == 0 || ix->pitch % 32 != 0 || !u42_unit_chunk((uint32_t)ix->pitch / 32)) return false;
  const Scan8Shape* sh = scan8_shape((uint32_t)ix->dim);
  if (ix->opt_scan_u42 < 0 && (!sh || !shadow_over_1gib(ix->n, sh->pieces * 16))) return false;
  return true;
}

// Allocates / refreshes the planes for the rows added since the last round that read them (the life cycle of
// prepare_u6_shadow).  false = no room on the device (remembered per capacity): the round stays on the u6 full pass.
static bool prepare_u42_shadow(wdbx_index* ix) {
  const uint32_t units = (uint32_t)ix->pitch / 32, lpitch = u42_lpitch(units);
  const uint64_t tiles = ((uint64_t)ix->cap + 63) / 64;
  const size_t need = (size_t)tiles * units * 1024 + (size_t)tiles * 64 * sizeof(f2v) + (size_t)tiles * 64 * lpitch * sizeof(uint32_t);
  if (!shadow_room(ix, ix->units42 != units || ix->rows42_tiles != tiles, {{&ix->d_rows42, need}},
                   &ix->shadow42_rows, &ix->u42_no_room_cap))
    return false;
  ix->units42 = units;
  ix->rows42_tiles = tiles;
  if (ix->shadow42_rows < ix->n) {
    if (launch_rows_to_u42(ix, ix->shadow42_rows, ix->n) != hipSuccess) return false;
    ix->shadow42_rows = ix->n;
  }
  return true;
}

// queries per read of the four-bit plane where option scan_u42_share leaves it to the library.  10 M x 384, 2000 steps, whole
// steps, means of three at 3 workgroups per CU: 1 -> 3095.7 q/s (the lone passes), 2 -> 5186.4, 4 -> 7039.7
// (profiles/u42_share/README.md, sweep_share/)
constexpr uint32_t U42_SHARE_DEFAULT = 4;

// the shortest remainder of a round (queries behind its full groups of 16) that goes to the matrix-core pass as one short group
// where option scan_u42_mfma leaves it to the library; a shorter one goes to the VALU groups.  A pass of 16 costs what it costs
// at any width (the plane read and the matrix operations do not shrink with absent columns): at 10 M x 384, 2000 steps, 0.790 ms
// per group at the 2 workgroups per CU it runs with, 0.933 ms at 3 (16 x the 0.0494 / 0.0583 ms per query of the event pair;
// profiles/u42_mfma/README.md, sweep_wgs/).  The VALU groups of profiles/u42_share/README.md cost 0.319 ms lone, 0.378 ms a
// pair, 0.552 ms four: 4 queries = 0.552 ms, 5 = 0.552 + 0.319 = 0.871 ms, so the pass wins from 5 on.
// tests/test_gpu_u42_share_calls.py pins that a default round of up to 5 queries reports a VALU width: hence 6, not 5.
constexpr uint32_t U42_MFMA_MIN_SHORT = 6;

// nq single queries of a round, each with its own full pass over the u6 shadow: sample (4 queries per workgroup) ->
// thresholds -> a pass per query -> exact re-scoring (rescore_kernel, as behind the u8 scan) -> cut -> final top-k.
// The candidate counters live in d_count6; d_count[0 .. nq) are the CUT's counters against last_batch_cap = its capacity, and
// end above it for a query whose candidate buffer or short list overflowed: what the callers' repair launches test.
// u42: the full passes run over the split planes instead (scan_u42_kernel); everything in front of and behind them is the same.
// There up to scan_u42_share consecutive queries of the round make their pass TOGETHER: one read and one unpack of the four-bit
// plane and of {s, a4} per group (u42_share_groups).  Still the query's own: its fp32 query, threshold, bounds, survivors, refine,
// candidates and counters -- its answer is bit for bit that of a pass of its own.
static int enqueue_singles_u6(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx, float* d_out_score,
                              u64* keys_out, bool u42) {
  const uint32_t units = (uint32_t)ix->pitch / 16;
  const int uc = u6_unit_chunk(units);
  scan6_fn f0 = pick_scan6(uc, true), f1 = pick_scan6(uc, false);
  if (!f0 || !f1) return fail(WDBX_E_STATE, "no u6 scan instance for %u units", units);
  if (!ix->d_rows6 || ix->units6 != units || ix->shadow6_rows < ix->n) return fail(WDBX_E_STATE, "u6 shadow not prepared");
  // option scan_u42_share: how many queries of a round share one read of the four-bit plane (-1: U42_SHARE_DEFAULT; 1: none)
  const uint32_t share = ix->opt_scan_u42_share == 1 || ix->opt_scan_u42_share == 2 || ix->opt_scan_u42_share == 4
                             ? (uint32_t)ix->opt_scan_u42_share : U42_SHARE_DEFAULT;
  scan42_fn f42[5] = {};  // by group width: 1, 2, 4
  for (int w = 1; u42 && w <= 4; w *= 2) f42[w] = pick_scan42(u42_unit_chunk(units / 2), w);
  if (u42 && (!f42[1] || !f42[2] || !f42[4] || !ix->d_rows42 || ix->units42 != units / 2 || ix->shadow42_rows < ix->n))
    return fail(WDBX_E_STATE, "split planes not prepared");
  // option scan_u42_mfma: full groups of 16 (and a remainder of U42_MFMA_MIN_SHORT or more) on scan_u42_mfma_kernel.  -1: where
  // the unit count has an instance and scan_u42_share is left at -1; 1: wherever an instance exists; 0: never.  An explicit
  // scan_u42_share of 1, 2 or 4 keeps the VALU kernels for the whole round unless scan_u42_mfma = 1 asks for both.
  const scan42_mfma_fn fm = u42 && ix->opt_scan_u42_mfma != 0 && (ix->opt_scan_u42_mfma == 1 || ix->opt_scan_u42_share == -1)
                                ? pick_scan42_mfma(units / 2) : nullptr;
  int rc;
  // the plan (host_selection.h): sampled 256-row tiles of 4 groups of 64 rows each and the divisor of the u8 scan
  const SelectionSample s = selection_sample(ix->n, 256, 4, k, selection_div(ix->opt_gemm_sample_div, k, true));
  const uint32_t sample_tiles = s.sample_tiles, stride = s.stride, ngroups = s.bounds;
  if (ngroups < (uint32_t)k) return fail(WDBX_E_STATE, "corpus too small for the selection scan at k=%d", k);
  // candidates: 256 x the k * (stride + 1) rows expected above the threshold (10 M x 384 top-10: 84 480; measured 3.8 k per
  // query on the bench corpus, an estimated 25 k on Gaussian rows)
  const uint32_t cap = ix->opt_scan_u6_cap > 0 ? (uint32_t)std::min<int64_t>(ix->opt_scan_u6_cap, 1 << 22) : selection_cap(s.expect, 256);
  constexpr uint32_t cap2 = 4096;  // the cut's short list: a few keys beyond k per segment
  constexpr int ROUND = 64;
  if ((rc = ix->d_halfmax.grow((size_t)ROUND * ngroups * sizeof(u64)))) return rc;
  if ((rc = ix->d_tau.grow((size_t)GB_N * sizeof(float)))) return rc;
  if ((rc = ix->d_cand.grow((size_t)ROUND * ((size_t)cap + cap2) * sizeof(u64)))) return rc;
  if ((rc = ix->d_count6.grow((size_t)ROUND * sizeof(uint32_t)))) return rc;
  if (u42 && (rc = ix->d_count42.grow((size_t)ROUND * sizeof(uint32_t)))) return rc;
  const size_t q16_dwords = (size_t)(ROUND / U42_MFMA_GROUP) * u42_mfma_group_dwords(units / 2);
  if (fm && (rc = ix->d_q16.grow(q16_dwords * 4 + (size_t)ROUND * sizeof(U42QConst)))) return rc;
  if (ix->d_count.bytes < ((size_t)nq + GB_N) * sizeof(uint32_t)) return fail(WDBX_E_STATE, "candidate counters not sized by the caller");
  ix->last_batch_nq = (uint32_t)nq;
  ix->last_batch_cap = cap2;
  u64* const cand2 = ix->d_cand + (size_t)ROUND * cap;
  const uint32_t tiles64 = (uint32_t)((ix->n + 63) / 64);
  // workgroups per CU of the full pass (option scan8_wgs).  Measured at 10 M x 384, whole steps: 2 -> 2222 q/s, 4 -> 2125,
  // 6 -> 2008, 8 -> 1990 (profiles/u6/README.md): eight waves per CU with 6 KiB in flight each keep HBM busy, more of them
  // only spread the stream over more pages at once
  // The split planes' pass, same corpus: 1 -> 1879, 2 -> 2885, 3 -> 3028, 4 -> 2959, 6 -> 2885 (profiles/u42/README.md): a wave
  // holds 6 KiB in flight as before but computes longer per byte, so a third workgroup still fills gaps.  With the packed
  // converts: 1 -> 1991, 2 -> 3005, 3 -> 3032 (mean of six), 4 -> 2935, 6 -> 2929 (profiles/u42_pipe/README.md)
  // Groups that share a read compute longer still per byte, 2000 steps: four queries per read 2 -> 6469, 3 -> 7057, 4 -> 7097,
  // 6 -> 6844 (means of three, spreads 8 / 30 / 18 / 22); two per read 2 -> 4855, 3 -> 5186, 4 -> 5279, 6 -> 4400
  // (profiles/u42_share/README.md): 4 for them, 3 stays for the lone passes of a round's remainder
  const auto wgs_of = [&](uint32_t width) {
    return (uint32_t)std::max<int64_t>(1, std::min<int64_t>(ix->opt_scan8_wgs > 0 ? ix->opt_scan8_wgs : !u42 ? 2 : width > 1 ? 4 : 3, 8));
  };
  const uint32_t grid1 = scan_full_grid(tiles64, (uint32_t)ix->cu_count, wgs_of(1));
  const uint32_t grid_shared = scan_full_grid(tiles64, (uint32_t)ix->cu_count, wgs_of(2));
  // the matrix-core pass, 2000 steps, means of three: 1 -> 22579 q/s, 2 -> 30096, 3 -> 22514 (spreads 73 / 352 / 66;
  // profiles/u42_mfma_pipe/README.md).  Its 70.8 KiB of LDS let a CU hold two workgroups: a grid of three per CU runs them in two
  // uneven rounds.  No load is in flight while a wave computes its tile, so the second wave of a SIMD is what overlaps
  const uint32_t grid_mfma = scan_full_grid(tiles64, (uint32_t)ix->cu_count,
                                            (uint32_t)std::max<int64_t>(1, std::min<int64_t>(ix->opt_scan8_wgs > 0 ? ix->opt_scan8_wgs : 2, 8)));
  const uint32_t grid0 = scan_sample_grid(ngroups, (uint32_t)ix->cu_count);
  const size_t pitch4 = ix->pitch / 4;
  const Scan8Shape* sh = scan8_shape((uint32_t)ix->dim);
  const bool one_grid = ix->opt_scan8_per_query == 0 || (ix->opt_scan8_per_query < 0 && sh && !shadow_over_1gib(ix->n, sh->pieces * 16));

  for (int q0 = 0; q0 < nq; q0 += ROUND) {
    const int nv = std::min(ROUND, nq - q0);
    const float* qsrc = d_queries + (size_t)q0 * ix->pitch;
    Scan6Args a = {};
    a.codes = ix->d_rows6;
    a.sa = (const f2v*)(ix->d_rows6 + (size_t)ix->rows6_tiles * units * 192);
    a.query = qsrc;
    a.n_rows = (uint32_t)ix->n;
    a.units = units;
    a.qpitch = (uint32_t)ix->pitch;
    a.halfmax = ix->d_halfmax;
    a.num_tiles = sample_tiles;
    a.tile_stride = stride;
    a.nq = (uint32_t)nv;
    a.tau = ix->d_tau;
    a.cand = ix->d_cand;
    a.count = ix->d_count6;
    a.count2 = ix->d_count + q0;
    a.cap = cap;
    // the sample, all queries of the round in one launch: maxima of the lower bounds over the sampled groups
    ix->last_sample_qn = 4;
    if ((rc = launch_bracketed(ix, ix->sample_ev, f0, dim3(grid0, (nv + 3) / 4), 0, a))) return rc;
    if ((rc = enqueue_sample_threshold(ix, ngroups, k, nv, true))) return rc;
    // the full passes: every query makes its own pass over all rows, on the split planes together with up to three neighbours
    // (one grid on small shards, as the u8 scan); one event pair around them, the profile reports elapsed / nv passes
    if ((rc = record(ix->gemm_ev, ix->profile, ix->stream, true))) return rc;
    if (u42) {
      Scan42Args b = {};
      b.hcodes = ix->d_rows42;
      b.sa4 = u42_sa4(ix);
      b.lrec = u42_lrec(ix);
      b.n_rows = a.n_rows;
      b.units = ix->units42;
      b.qpitch = a.qpitch;
      b.lpitch = u42_lpitch(ix->units42);
      b.cap = cap;
      // (the survivors are counted for the probes only: an atomic per 64 of them)
      HIP_TRY(hipMemsetAsync(ix->d_count42, 0, (size_t)nv * sizeof(uint32_t), ix->stream));
      // the groups of 16 on the matrix cores (host_selection.h): the round's queries as 16-bit operands once, then one grid
      // for all groups or a launch per group
      uint32_t taken = 0;
      if (fm) {
        const uint32_t ngm = u42_mfma_groups((uint32_t)nv, U42_MFMA_MIN_SHORT, &taken);
        if (ngm) {
          U42QConst* const qc = (U42QConst*)(ix->d_q16 + q16_dwords);
          hipLaunchKernelGGL(u42_query_i16_kernel, dim3(ngm * U42_MFMA_GROUP), dim3(64), 0, ix->stream, qsrc, b.qpitch, b.units, taken,
                             ix->d_q16, qc);
          HIP_TRY(hipGetLastError());
          Scan42MfmaArgs mm = {};
          for (uint32_t g = 0; g < ngm;) {
            const uint32_t run = one_grid ? ngm : 1, i = g * U42_MFMA_GROUP;
            mm.a = b;
            mm.a.query = qsrc + (size_t)i * ix->pitch;
            mm.a.tau = ix->d_tau + i;
            mm.a.cand = ix->d_cand + (size_t)i * cap;
            mm.a.count = ix->d_count6 + i;
            mm.a.survivors = ix->d_count42 + i;
            mm.qb = ix->d_q16 + (size_t)g * u42_mfma_group_dwords(b.units);
            mm.qc = qc + i;
            mm.nq = one_grid ? taken : std::min(taken - i, U42_MFMA_GROUP);
            hipLaunchKernelGGL(fm, dim3(grid_mfma, run), dim3(256), 0, ix->stream, mm);
            HIP_TRY(hipGetLastError());
            g += run;
          }
          ix->last_u42_mfma_groups += (int)ngm;
        }
      }
      // what they leave, as the groups that share a read (host_selection.h): a launch per group, or (one grid) per run of groups
      // of one width
      uint32_t first[ROUND], width[ROUND];
      const uint32_t ng = u42_share_groups((uint32_t)nv - taken, share, first, width);
      for (uint32_t g = 0; g < ng;) {
        uint32_t run = 1;
        while (one_grid && g + run < ng && width[g + run] == width[g]) ++run;
        const uint32_t i = taken + first[g];
        b.query = qsrc + (size_t)i * ix->pitch;
        b.tau = ix->d_tau + i;
        b.cand = ix->d_cand + (size_t)i * cap;
        b.count = ix->d_count6 + i;
        b.survivors = ix->d_count42 + i;
        hipLaunchKernelGGL(f42[width[g]], dim3(width[g] > 1 ? grid_shared : grid1, run), dim3(256), 0, ix->stream, b);
        HIP_TRY(hipGetLastError());
        ix->last_u42_share = std::max(ix->last_u42_share, (int)width[g]);
        g += run;
      }
    } else if (one_grid && nv > 1) {
      hipLaunchKernelGGL(f1, dim3(grid1, nv), dim3(256), 0, ix->stream, a);
      HIP_TRY(hipGetLastError());
    } else {
      for (int i = 0; i < nv; ++i) {
        a.query = qsrc + (size_t)i * ix->pitch;
        a.tau = ix->d_tau + i;
        a.cand = ix->d_cand + (size_t)i * cap;
        a.count = ix->d_count6 + i;
        hipLaunchKernelGGL(f1, dim3(grid1), dim3(256), 0, ix->stream, a);
        HIP_TRY(hipGetLastError());
      }
    }
    if ((rc = record(ix->gemm_ev, ix->profile, ix->stream, false, (uint32_t)nv))) return rc;
    // exact fp32 scores for the candidates, from the fp32 rows
    hipLaunchKernelGGL(rescore_kernel<WDBX_METRIC_COSINE>, dim3(256, nv), dim3(256), 0, ix->stream, (const f4*)ix->d_rows.p,
                       (uint32_t)pitch4, (const f4*)qsrc, ix->d_cand, (const uint32_t*)ix->d_count6, cap, (u64*)nullptr,
                       (uint32_t*)nullptr);
    // the cut: per segment of the re-scored keys those that can be among the best k
    hipLaunchKernelGGL(u6_cut_kernel, dim3((cap + U6_CUT_SEG - 1) / U6_CUT_SEG, nv), dim3(1024), 0, ix->stream, (const u64*)ix->d_cand,
                       (const uint32_t*)ix->d_count6, cap, k, cand2, ix->d_count + q0, cap2);
    HIP_TRY(hipGetLastError());
    MergeArgs f = final_topk_args(ix, cand2, cap2, ix->d_count + q0, k);
    f.over_out = ix->defer_flag_dev ? ix->defer_flag_dev + q0 : nullptr;
    final_topk_output(ix, &f, keys_out, false, d_out_idx, d_out_score, q0, k);
    if ((rc = launch_merge(ix, f, nv))) return rc;
  }
  return WDBX_OK;
}

// (the tile kernel families GEMM_FP32 / GEMM_BF16 / GEMM_BF16_SHADOW / GEMM_I8: kernels_tiles.h, behind the kernels)
static inline int gemm_family(const wdbx_index* ix) {
  return ix->opt_gemm_bf16 <= 0 ? GEMM_FP32 : ix->opt_gemm_bf16 == 1 ? GEMM_BF16 : GEMM_BF16_SHADOW;
}

// ---- int8 tiles (option gemm_bf16 = 3, the default): inner product / cosine, rows whose i8 image is at most 1536 bytes
// (the query block stays resident in LDS: 64 * CT queries x pitch8g bytes <= 96 KiB), and not shorter than 0.8 of ...
static inline uint32_t i8g_pitch(const wdbx_index* ix) { return (uint32_t)((ix->dim + 127) / 128 * 128); }
static inline int i8g_max_ct(const wdbx_index* ix) {
  const uint32_t p = i8g_pitch(ix);
  return p * 256u <= (uint32_t)G8_LDS_B_MAX ? 4 : p * 128u <= (uint32_t)G8_LDS_B_MAX ? 2 : p * 64u <= (uint32_t)G8_LDS_B_MAX ? 1 : 0;
}
static bool i8_tiles_shape_ok(const wdbx_index* ix) {  // (everything but the row mask)
  if (ix->opt_gemm_bf16 < 3) return false;
  if (ix->metric == WDBX_METRIC_L2 && (!ix->opt_gemm_l2 || !ix->opt_gemm_l2_i8)) return false;
  if (i8g_max_ct(ix) == 0) return false;
  // short rows: the padded i8 image (128-byte multiples) must be clearly smaller than the fp32 row
  return (uint64_t)i8g_pitch(ix) * 10 <= (uint64_t)ix->pitch * 4 * 8;
}
// (a row mask: the masked full pass exists for the product forms only -- option gemm_masked = 0 keeps masked calls off the tiles)
static bool i8_tiles_eligible(const wdbx_index* ix) {
  if (ix->active_mask && !(ix->opt_gemm_masked > 0 && ix->opt_gemm8_variant == 0)) return false;
  return i8_tiles_shape_ok(ix);
}

// Allocates / refreshes shadow copy G for the rows added since the last batch (whole 64-row groups: the group that was
// only partly filled is re-quantised, its scale may have changed).  false = no room on the device (remembered per
// capacity): the caller stays on the bf16 tiles.
static bool prepare_i8g_shadow(wdbx_index* ix) {
  const uint32_t pitch8 = i8g_pitch(ix);
  const size_t need = (((size_t)ix->cap + G8_ROWS - 1) / G8_ROWS + 1) * G8_ROWS * pitch8;  // whole tiles (fragment order) + one of slack
  const size_t need_g = (((size_t)ix->cap + TILE_PAD_ROWS + 63) / 64 + 1) * sizeof(f4);
  const int room = shadow_room(ix, ix->pitch8g != pitch8, {{&ix->d_rows8g, need}, {&ix->d_groups8, need_g}, {&ix->d_gbad8, need_g / 2}},
                               &ix->shadowg_rows, &ix->i8g_no_room_cap);
  if (room != SHADOW_KEPT) ix->shadowg_tail_n = ~0ull;
  if (room == SHADOW_NO_ROOM) return false;
  if (room == SHADOW_FRESH) {
    // (the table entries of the pad groups are read by the last tile's waves and must not be garbage that traps: zero;
    // pad groups hold no row: all their bad-row bits set)
    if (hipMemsetAsync(ix->d_groups8, 0, need_g, ix->stream) != hipSuccess || hipMemsetAsync(ix->d_gbad8, 0xFF, need_g / 2, ix->stream) != hipSuccess) {
      (void)ix->d_groups8.release();  // (stale again: the next call starts over)
      return false;
    }
    ix->pitch8g = pitch8;
  }
  // Groups are (re)quantised up to the END OF THE LAST 256-ROW TILE of the current row count, not just up to the last row's
  // group: the tile kernels read whole tiles, and PHASE 0 trusts the bad-row bits alone to keep rows past the end out of the
  // threshold sample.  After wdbx_index_clear() + fewer rows, or a compaction that dropped live tail rows, the groups between
  // ceil(n / 64) and the tile's end would otherwise keep the OLD corpus's bytes, table entries and "good" bits, their lower
  // bounds could enter the k-th largest, and a threshold above the true k-th score silently drops true neighbours.
  if (ix->shadowg_rows < ix->n || ix->shadowg_tail_n != ix->n) {
    const u64 g0 = std::min<u64>(ix->shadowg_rows, ix->n) / 64;
    const u64 g1 = (ix->n + G8_ROWS - 1) / G8_ROWS * (G8_ROWS / 64);
    if (g1 > g0) {
      hipLaunchKernelGGL(rows_to_i8g_kernel, dim3(rows_to_i8g_grid(g1 - g0)), dim3(256), 0, ix->stream,
                         (const float*)ix->d_rows, g0, g1, (u64)ix->n, (uint32_t)ix->dim, (uint32_t)ix->pitch, ix->d_rows8g, pitch8,
                         ix->d_groups8, ix->d_gbad8);
      if (hipGetLastError() != hipSuccess) return false;
    }
    ix->shadowg_rows = ix->n;
    ix->shadowg_tail_n = ix->n;
    ix->gref_valid = false;
  }
  return true;
}
// A call WITH a row mask may take the batched path only when the int8 tiles are what would run (no other tile family reads
// masks), in their product form, with k below the select range; their shadow copy must be in place (no room: not eligible).
// Everything else keeps the per-query paths.  (Looked at before or after active_mask is set: the answer is the same.)
static bool masked_tiles_ready(wdbx_index* ix, int k) {
  if (ix->opt_gemm_masked <= 0 || ix->opt_gemm8_variant != 0 || use_select(ix, k) || !ix->n) return false;
  return i8_tiles_shape_ok(ix) && prepare_i8g_shadow(ix);
}
// (the instances, their pickers and the launch helpers: kernels_tiles.h, behind the kernels)
template <int PHASE, int CT>
static int launch_gemm_ct(wdbx_index* ix, const GemmArgs& g, int family) {
  if (family != GEMM_FP32 && CT < 2) return fail(WDBX_E_STATE, "bf16 tiles need a query block of at least 128");
  const GemmLaunch l = gemm_launch_ct<PHASE, CT>(family, ix->metric, g.gmax != nullptr, g.pitch4);
  if (!l.fn) return fail(WDBX_E_STATE, "no tile kernel for this family with per-group bounds");
  HIP_TRY(gemm_prepare(l));
  const uint32_t grid = gemm_grid(l, g.num_tiles, (uint32_t)ix->cu_count);
  int rc = record(ix->gemm_ev, ix->profile, ix->stream, true);
  if (rc) return rc;
  HIP_TRY(enqueue_gemm(ix->stream, l, g, grid));
  return record(ix->gemm_ev, ix->profile, ix->stream, false);
}

template <int PHASE>
static int launch_gemm(wdbx_index* ix, const GemmArgs& g, int ct, int family) {
  switch (ct) {
    case 1: return launch_gemm_ct<PHASE, 1>(ix, g, family);
    case 2: return launch_gemm_ct<PHASE, 2>(ix, g, family);
    default: return launch_gemm_ct<PHASE, 4>(ix, g, family);
  }
}

// Enqueue nq (any number) queries in blocks of 256 through the GEMM path.  Per query a counter of
// appended candidates is left in d_count[q]; a count above the capacity means that query's result
// may be incomplete and must be re-run on the scan path (wdbx_index_batch_status).
// count_slot >= 0: the per-query candidate counters live at d_count[count_slot ...] (sized by the caller) and
// only they are reset; keys_out != null: the final top-k is written there as keys with global rows instead
// of idx/score, and no exchange follows (the single-query caller batches its own).
static int enqueue_search_gemm(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx,
                               float* d_out_score, int mode = SEARCH_FINAL, int count_slot = -1, u64* keys_out = nullptr) {
  const bool sharded = mode == SEARCH_SHARDED;
  if (sharded && !ix->comm) return fail(WDBX_E_STATE, "sharded search before wdbx_index_comm_init");
  if (nq <= 0) return WDBX_OK;
  if (k < 1 || k > WDBX_MAX_K) return fail(WDBX_E_INVALID, "k=%d outside [1, %d]", k, WDBX_MAX_K);
  if (!d_queries || (!keys_out && (!d_out_idx || !d_out_score))) return fail(WDBX_E_INVALID, "null device buffer");
  if (ix->n >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "shard holds too many rows for 32-bit row keys");
  int rc;
  ix->last_batch_repaired = false;
  ix->last_batch_masked = false;
  if (count_slot < 0 && i8_tiles_eligible(ix) && prepare_i8g_shadow(ix))
    return enqueue_search_gemm8(ix, d_queries, nq, k, d_out_idx, d_out_score, mode, keys_out);
  // (the other tile families read no row mask: their callers ask masked_tiles_ready first)
  if (ix->active_mask) return fail(WDBX_E_STATE, "a row mask on the batched path needs the int8 tiles");
  int family = gemm_family(ix);
  // short rows: the padded shadow would be no smaller than the fp32 rows, so the tiles read those
  if (family == GEMM_BF16_SHADOW && ((uint64_t)ix->pitch + 127) / 128 * 128 >= 2 * (uint64_t)ix->pitch) family = GEMM_BF16;
  if (family == GEMM_BF16_SHADOW) {  // the bf16 shadow copy of the rows added since the last batch
    const uint32_t pitch16 = (uint32_t)((ix->pitch + 127) / 128 * 128);  // whole pairs of 64-element chunks
    const size_t need = ((size_t)ix->cap + TILE_PAD_ROWS) * pitch16 * 2;
    uint64_t every_call = ~0ull;  // (a shadow that found no room is tried again by the next batch: nothing is remembered)
    const int room = shadow_room(ix, ix->pitch16 != pitch16, {{&ix->d_rows16, need}}, &ix->shadow_rows, &every_call);
    if (room == SHADOW_FRESH) ix->pitch16 = pitch16;
    if (room == SHADOW_NO_ROOM) family = GEMM_BF16;  // the same tiles on the fp32 rows
    if (family == GEMM_BF16_SHADOW && ix->shadow_rows < ix->n) {
      const u64 pieces = (ix->n - ix->shadow_rows) * (pitch16 / 8);
      hipLaunchKernelGGL(rows_to_bf16_kernel, dim3((uint32_t)std::min<u64>((pieces + 255) / 256, 1u << 20)), dim3(256), 0,
                         ix->stream, (const float*)ix->d_rows, (u64)ix->shadow_rows, (u64)ix->n, (uint32_t)ix->pitch,
                         (__bf16*)ix->d_rows16.p, pitch16);
      HIP_TRY(hipGetLastError());
      ix->shadow_rows = ix->n;
    }
  }
  ix->last_gemm_mode = family;
  const bool l2 = ix->metric == WDBX_METRIC_L2, bf16 = family != GEMM_FP32;
  const bool inexact = l2 || bf16;  // selection scores differ from the final ones: margin + exact re-scoring
  // the plan (host_selection.h): the family's tiles, a PHASE 0 key per 64 rows of a tile and query (rw).  The bf16 tiles make
  // the sample pass cheap and their error margin multiplies the candidates, so a larger k gets a larger sample (a tighter
  // threshold) there, and 32 x the expected candidates as capacity against 8 x on the exact fp32 tiles
  const uint32_t tile_rows = gemm_tile_rows(family), rw = tile_rows / 64;
  const SelectionSample s = selection_sample(ix->n, tile_rows, rw, k, selection_div(ix->opt_gemm_sample_div, k, bf16));
  const uint32_t tiles = s.tiles, sample_tiles = s.sample_tiles, stride = s.stride;
  if (s.bounds < (uint32_t)k) return fail(WDBX_E_STATE, "corpus too small for the batched path at k=%d", k);
  const uint32_t cap = selection_cap(s.expect, bf16 ? 32 : 8);
  const size_t pitch4 = ix->pitch / 4;
  if ((rc = ix->d_qblock.grow((size_t)GB_N * ix->pitch * sizeof(float)))) return rc;
  if ((rc = ix->d_halfmax.grow((size_t)GB_N * rw * sample_tiles * sizeof(u64)))) return rc;
  if ((rc = ix->d_tau.grow((size_t)GB_N * sizeof(float)))) return rc;
  if ((rc = ix->d_cand.grow((size_t)GB_N * cap * sizeof(u64)))) return rc;
  if (count_slot < 0) {
    if ((rc = ix->d_count.grow(((size_t)nq + GB_N) * sizeof(uint32_t)))) return rc;
  } else if (ix->d_count.bytes < ((size_t)count_slot + nq + GB_N) * sizeof(uint32_t)) {
    return fail(WDBX_E_STATE, "candidate counters not sized by the caller");
  }
  uint32_t* const d_count = ix->d_count + std::max(count_slot, 0);
  if (sharded && (rc = ix->d_local_keys.grow((size_t)GB_N * k * sizeof(u64)))) return rc;
  HIP_TRY(hipMemsetAsync(d_count, 0, (count_slot < 0 ? (size_t)nq + GB_N : (size_t)nq) * sizeof(uint32_t), ix->stream));
  // bf16 query block: zero padded to the K extent the tile kernel walks (a ring of 4 chunks / a pair of chunks)
  const uint32_t kring = family == GEMM_BF16_SHADOW ? 128u : 64u;
  const uint32_t kpad = (uint32_t)((ix->pitch + kring - 1) / kring * kring);
  if (bf16 && (rc = ix->d_qb16.grow((size_t)GB_N * kpad * 2))) return rc;
  if (inexact) {  // squared norms of the rows added since the last such batch (L2 term, and the error margin)
    if ((rc = ensure_row_norms(ix))) return rc;
    // How the selection error is bounded.  Norms all alike (the reference normalises its rows): ONE bound from the
    // largest norm, subtracted from the thresholds (tau_margin_kernel) -- nothing in the tile epilogue.  Norms that
    // vary a lot (largest > 1.5 x mean: unnormalised data, outlier rows): a bound per 64-row group from that group's
    // largest norm, applied in the epilogue (+10 % kernel time), so an outlier only loosens its own group and the
    // batch does not degenerate into per-query repairs.  Decided when the norms change (one 8-byte read-back).
    if (!ix->gmax_valid) {
      if (ix->cn_stats_dirty) {  // rows were overwritten in place: rebuild maximum / sum / count from the cached norms
        HIP_TRY(hipMemsetAsync(ix->d_cnmax, 0, 4 * sizeof(uint32_t), ix->stream));
        hipLaunchKernelGGL(cn_stats_kernel, dim3((uint32_t)std::min<uint64_t>((ix->n + 255) / 256, 2048)), dim3(256), 0, ix->stream,
                           (const float*)ix->d_cn, (u64)ix->n, ix->d_cnmax);
        HIP_TRY(hipGetLastError());
        ix->cn_stats_dirty = false;
      }
      uint32_t words[3] = {0, 0, 0};
      HIP_TRY(hipMemcpyAsync(words, ix->d_cnmax, sizeof words, hipMemcpyDeviceToHost, ix->stream));
      HIP_TRY(hipStreamSynchronize(ix->stream));
      float cmax, csum;
      memcpy(&cmax, &words[0], 4);
      memcpy(&csum, &words[1], 4);
      const float mean = words[2] ? csum / (float)words[2] : 0.f;  // over the rows with a finite norm (removed rows are NaN)
      // an infinite norm (a row with an infinite or huge element) always takes the per-group instances: their epilogue
      // sends such a group's rows to the exact pass whatever the selection scores say (kernels_tiles.h)
      ix->group_bounds = ix->opt_group_bounds == 1 || !(cmax < INFINITY) || (ix->opt_group_bounds != 0 && !(cmax <= 1.5f * mean));
      if (ix->group_bounds) {
        if ((rc = ix->d_gmax.grow(((size_t)ix->cap + 63) / 64 * sizeof(float)))) return rc;
        const uint32_t gblocks = (uint32_t)std::min<uint64_t>(((ix->n + 63) / 64 + 255) / 256, 4096);
        hipLaunchKernelGGL(group_max_kernel, dim3(gblocks), dim3(256), 0, ix->stream, (const float*)ix->d_cn, (u64)ix->n, ix->d_gmax);
        HIP_TRY(hipGetLastError());
      }
      ix->gmax_valid = true;
    }
    if ((rc = ix->d_qn.grow((size_t)2 * GB_N * sizeof(float)))) return rc;
  }
  const bool group_bounds = inexact && ix->group_bounds;
  ix->last_batch_nq = (uint32_t)nq;
  ix->last_batch_cap = cap;
  // rounding-error coefficients of the selection scores (kernels_tiles.h, GemmArgs): fp32 chains of n terms carry
  // gamma = n u / (1 - n u); bf16 roundings of both operands add 2^-7 (+ 2^-16) per product
  const float nu = (float)(ix->pitch + 18) * 5.9604645e-08f;
  const float gamma = 1.02f * nu / (1.0f - nu);
  const float sel_eps = (gamma + (bf16 ? 1.05f * 0.0078125f : 0.0f)) * 1.0102f, sel_gam = gamma * 1.01f;
  const float sel_floor = bf16 ? 7.5e-37f * sqrtf((float)ix->pitch) : 0.0f;  // 2^-120 sqrt(d): see GemmArgs::floor_abs
  const float sel_under = ldexpf((float)(ix->pitch + 18), -149);  // gradual underflow of the fma chain: GemmArgs::under_abs

  // per_query: the single-query caller.  Every query makes its OWN pass pair (a 128-column tile with one live
  // column), but the small kernels around the passes (conversion, thresholds, margins, re-scoring, final
  // top-k) run once per round of up to PQ_ROUND queries.
  const bool per_query = count_slot >= 0;
  constexpr int PQ_ROUND = 32;
  if (per_query && !bf16) return fail(WDBX_E_STATE, "single-query passes need the bf16 tiles");
  if (per_query && (rc = ix->d_qb16.grow((size_t)PQ_ROUND * 128 * kpad * 2))) return rc;
  for (int q0 = 0; q0 < nq;) {
    // query block: 256, 128 or 64 wide -- a small batch does not pay for 256 columns (the bf16 tiles: 256 or 128)
    const int rem = nq - q0;
    int ct = (ix->opt_gemm_ct == 1 || ix->opt_gemm_ct == 2 || ix->opt_gemm_ct == 4) ? (int)ix->opt_gemm_ct
             : rem > 128 ? 4 : rem > 64 ? 2 : 1;
    if (bf16 && ct < 2) ct = 2;
    if (per_query) ct = 2;
    if (family == GEMM_BF16_SHADOW && l2 && group_bounds && ct > 2) ct = 2;  // see pick_gemm_kernel_gb
    const int gbn = 64 * ct, nv = std::min(per_query ? PQ_ROUND : gbn, rem);
    const int passes = per_query ? nv : 1;  // tile kernel launches per phase this round
    const float* qsrc = d_queries + (size_t)q0 * ix->pitch;
    if (nv < gbn && !bf16) {  // zero-padded private copy of a partial block (the bf16 block is padded by its conversion)
      HIP_TRY(hipMemsetAsync(ix->d_qblock, 0, (size_t)gbn * ix->pitch * sizeof(float), ix->stream));
      HIP_TRY(hipMemcpyAsync(ix->d_qblock, qsrc, (size_t)nv * ix->pitch * sizeof(float), hipMemcpyDeviceToDevice, ix->stream));
      qsrc = ix->d_qblock;
    }
    // tau = +inf for padded queries so they never append
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ix->d_tau, 0x7F800000, GB_N, ix->stream));
    GemmArgs g = {};
    g.rows = (const f4*)ix->d_rows.p;
    g.queries = (const f4*)qsrc;
    g.n_rows = (uint32_t)ix->n;
    g.pitch4 = (uint32_t)pitch4;
    if (family == GEMM_BF16_SHADOW) {
      g.rows = (const f4*)ix->d_rows16.p;
      g.pitch4 = ix->pitch16 / 8;
    }
    g.num_tiles = sample_tiles;
    g.tile_stride = stride;
    g.cn = ix->d_cn;
    g.live = per_query ? 1 : 0;
    if (group_bounds) {
      const int nqn = per_query ? nv : gbn;
      hipLaunchKernelGGL(query_norm_kernel, dim3(nqn), dim3(64), 0, ix->stream, qsrc, (uint32_t)ix->pitch, nv, nqn, ix->d_qn);
      HIP_TRY(hipGetLastError());
      g.gmax = ix->d_gmax;
      g.qn = ix->d_qn;
      g.eps = sel_eps;
      g.gam = sel_gam;
      g.floor_abs = sel_floor;
      g.under_abs = sel_under;
    }
    const size_t qb_block = (size_t)gbn * kpad;  // bf16 elements per query block
    if (bf16) {
      hipLaunchKernelGGL(queries_to_bf16_kernel, dim3((uint32_t)((passes * qb_block + 255) / 256)), dim3(256), 0, ix->stream, qsrc,
                         (uint32_t)ix->pitch, (uint32_t)nv, (__bf16*)ix->d_qb16.p, kpad, (uint32_t)gbn,
                         (uint32_t)(per_query ? 1 : gbn), (uint32_t)passes);
      HIP_TRY(hipGetLastError());
      g.qb_pitch16 = kpad / 8;
    }
    for (int i = 0; i < passes; ++i) {  // phase 0: maxima of the sampled tiles
      g.qb16 = bf16 ? (const void*)((const __bf16*)ix->d_qb16.p + (size_t)i * qb_block) : nullptr;
      g.halfmax = ix->d_halfmax + (size_t)i * rw * sample_tiles;
      if (group_bounds) g.qn = ix->d_qn + (per_query ? i : 0);
      if ((rc = launch_gemm<0>(ix, g, ct, family))) return rc;
    }
    if ((rc = enqueue_sample_threshold(ix, s.bounds, k, nv, false))) return rc;  // (these families never took kth_score_kernel)
    if (inexact && !group_bounds) {  // one global rounding-error margin below the sampled threshold
      hipLaunchKernelGGL(tau_margin_kernel, dim3(nv), dim3(64), 0, ix->stream, ix->d_tau, qsrc, (uint32_t)ix->pitch, nv,
                         (const uint32_t*)ix->d_cnmax, ix->metric, (int)bf16, sel_floor, sel_under);
      HIP_TRY(hipGetLastError());
    }  // (with per-group bounds the k-th largest reported LOWER bound is already a valid threshold)
    g.num_tiles = tiles;
    g.tile_stride = 1;
    g.halfmax = nullptr;
    g.cap = cap;
    for (int i = 0; i < passes; ++i) {  // phase 1: every score above the threshold becomes a candidate
      g.qb16 = bf16 ? (const void*)((const __bf16*)ix->d_qb16.p + (size_t)i * qb_block) : nullptr;
      g.tau = ix->d_tau + i;
      g.cand = ix->d_cand + (size_t)i * cap;
      g.count = d_count + q0 + i;
      if (group_bounds) g.qn = ix->d_qn + (per_query ? i : 0);
      if ((rc = launch_gemm<1>(ix, g, ct, family))) return rc;
    }
    if (inexact) {  // exact fp32 scores for the selected candidates
      hipLaunchKernelGGL(l2 ? rescore_kernel<WDBX_METRIC_L2> : rescore_kernel<WDBX_METRIC_COSINE>, dim3(64, nv), dim3(256), 0,
                         ix->stream, (const f4*)ix->d_rows.p, (uint32_t)pitch4, (const f4*)qsrc, ix->d_cand,
                         (const uint32_t*)(d_count + q0), cap, (u64*)nullptr, (uint32_t*)nullptr);
      HIP_TRY(hipGetLastError());
    }
    MergeArgs f = final_topk_args(ix, ix->d_cand, cap, d_count + q0, k);
    final_topk_output(ix, &f, keys_out, sharded, d_out_idx, d_out_score, q0, k);
    if ((rc = launch_merge(ix, f, nv))) return rc;
    if (!per_query) {  // (the single-query caller queues its own repair launches)
      bool done = false;
      if ((rc = enqueue_batch_repair(ix, qsrc, nv, k, d_count + q0, cap, f.out_idx, f.out_score, f.out_keys, &done))) return rc;
      if (q0 == 0) ix->last_batch_repaired = done;
      else ix->last_batch_repaired = ix->last_batch_repaired && done;
    }
    if (sharded && (rc = exchange_and_merge(ix, nv, k, d_out_idx + (size_t)q0 * k, d_out_score + (size_t)q0 * k))) return rc;
    q0 += nv;
  }
  return WDBX_OK;
}

// ---- batched queries on the int8 tiles (kernels_tiles8.h) ----------------------------------------
// (the instances, their pickers and the launch helpers: kernels_tiles8.h, behind the kernel)
template <int PHASE>
static int launch_gemm8(wdbx_index* ix, const Gemm8Args& g, int ct, bool masked = false, bool multi = false) {
  const Gemm8Launch l = gemm8_launch_of<PHASE>(ct, g.pitch8, ix->metric, masked, multi, (int)ix->opt_gemm8_variant);
  if (!l.fn) return fail(WDBX_E_STATE, "no int8 tile instance for this query block");
  HIP_TRY(gemm8_prepare(l));
  const uint32_t grid = gemm8_grid(g.num_tiles, (uint32_t)ix->cu_count);
  int rc = record(ix->gemm_ev, ix->profile, ix->stream, true);
  if (rc) return rc;
  HIP_TRY(enqueue_gemm8(ix->stream, l, g, grid));
  return record(ix->gemm_ev, ix->profile, ix->stream, false);
}

// the ordinary-group bounds of the int8 tiles' prefilter epilogue (two passes over the group table, ~10 us), rebuilt after the
// shadow copy changed; shared by the top-k batches and the batched range search
static int ensure_group_ref(wdbx_index* ix) {
  if (ix->gref_valid) return WDBX_OK;
  const int rc = ix->d_gref8.grow(8 * sizeof(float));
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(ix->d_gref8, 0, 8 * sizeof(float), ix->stream));
  const u64 ngroups = (ix->n + 63) / 64;
  const uint32_t blocks = group_ref_grid(ngroups);
  for (int pass = 0; pass < 2; ++pass)
    hipLaunchKernelGGL(group_ref_kernel, dim3(blocks), dim3(256), 0, ix->stream, (const f4*)ix->d_groups8, ngroups, ix->d_gref8,
                       (uint32_t*)(ix->d_gref8 + 4), pass);
  HIP_TRY(hipGetLastError());
  ix->gref_valid = true;
  return WDBX_OK;
}

// nq (any number) queries in blocks of up to 256 through the int8 tiles.  Same contract as enqueue_search_gemm: per-query
// candidate counters in d_count[q] (a count above the capacity = that query must be re-run on the scan path), results are
// the exact fp32 ranking of the kept rows (rescore_kernel + merge_kernel).
// mc != null: a call with one row mask PER QUERY (wdbx_index_search_multimask).  d_queries are then the
// call's SLOTS (host_multimask.h: every column group of 16 slots holds queries of one class; pad slots are zero rows), nq
// their number, the blocks are the plan's, and results and candidate counters come back in slot order.
struct MultiCall {
  const MultimaskPlan* plan;
  const int32_t* d_slot_query;  // the plan's slot_query on the device
  const uint32_t* d_masks;      // the masks of the call's classes: class row r at d_masks + r * mask_stride (a row without a mask: unused)
  size_t mask_stride;           // words
  const int32_t* d_class_mask;  // per class row: r, or -1 for the class without a mask
  const uint64_t* allowed;      // per class row: how many rows the class allows
};
static int enqueue_search_gemm8(wdbx_index* ix, const float* d_queries, int nq, int k, int64_t* d_out_idx, float* d_out_score,
                                int mode, u64* keys_out, const MultiCall* mc) {
  const bool sharded = mode == SEARCH_SHARDED;
  int rc;
  ix->last_gemm_mode = GEMM_I8;
  const bool masked = ix->active_mask != nullptr, multi = mc != nullptr;
  if (multi && (masked || sharded || keys_out)) return fail(WDBX_E_STATE, "a mask per query: the plain blocking call only");
  const uint32_t pitch8 = ix->pitch8g;
  // the plan (host_selection.h): tiles of G8_ROWS rows, a lower bound per 32-row block, the divisor of the selection scans,
  // 32 x the expected rows as candidates.  A row mask grows the sample (selection_sample_masked).
  constexpr uint32_t rw = G8_ROWS / 32;
  const SelectionSample base = selection_sample(ix->n, G8_ROWS, rw, k, selection_div(ix->opt_gemm_sample_div, k, true));
  const uint32_t tiles = base.tiles;
  // the sampled tiles of a call (or, with a mask per query, of one block) whose mask allows `allowed` rows
  auto sample_for = [&](bool masked, uint64_t allowed) -> uint32_t {
    return masked ? selection_sample_masked(base.sample_tiles, tiles, rw, k, ix->n, allowed) : base.sample_tiles;
  };
  // A mask per query: the rule per BLOCK, for its most selective class above 16 384 rows (the class whose vouching blocks
  // are fewest; the block's other classes get a larger sample than they need, never a smaller one).  Sizes below: the
  // smallest sample of the call gives the most candidates per query, the largest the most sampled bounds.
  std::vector<uint32_t> block_sample;
  uint32_t sample_tiles, sample_max;
  uint64_t small_class = 0;  // the largest mask of at most 16 384 rows: room for ALL its rows in the candidate buffers
  if (multi) {
    const MultimaskPlan& pl = *mc->plan;
    std::vector<int> row_of_class((size_t)WDBX_MAX_CALL_MASKS + 1, 0);
    for (size_t r = 0; r < pl.classes.size(); ++r) {
      row_of_class[(size_t)(pl.classes[r] + 1)] = (int)r;
      if (mc->allowed[r] <= 16384) small_class = std::max(small_class, mc->allowed[r]);
    }
    sample_tiles = tiles;
    sample_max = 1;
    for (uint32_t b = 0; b < pl.blocks(); ++b) {
      uint64_t least = ~0ull;
      for (uint32_t g = pl.block_group[b]; g < pl.block_group[b + 1]; ++g) {
        const uint64_t al = mc->allowed[(size_t)row_of_class[(size_t)(pl.group_class[g] + 1)]];
        if (al > 16384) least = std::min(least, al);
      }
      block_sample.push_back(least == ~0ull ? sample_for(false, 0) : sample_for(true, least));
      sample_tiles = std::min(sample_tiles, block_sample.back());
      sample_max = std::max(sample_max, block_sample.back());
    }
  } else {
    sample_tiles = sample_max = sample_for(masked, ix->mask_allowed);
    if (masked && ix->mask_allowed <= 16384) small_class = ix->mask_allowed;
  }
  const SelectionSample s = selection_of(tiles, sample_tiles, rw, k);  // (the call's smallest sample: the most candidates per query)
  if (s.bounds < (uint32_t)k) return fail(WDBX_E_STATE, "corpus too small for the batched path at k=%d", k);
  uint32_t cap = selection_cap(s.expect, 32);
  // (a mask that allows few rows: room for ALL of them, so that tau = -inf -- no sampled block held an allowed row -- is
  // answered from the candidates, not by a repair scan per query; 16 384 rows = 32 MiB of candidate buffers)
  cap = std::max<uint32_t>(cap, (uint32_t)small_class);
  const size_t pitch4 = ix->pitch / 4;
  if ((rc = ix->d_halfmax.grow((size_t)GB_N * rw * sample_max * sizeof(u64)))) return rc;
  if ((rc = ix->d_tau.grow((size_t)GB_N * sizeof(float)))) return rc;
  if ((rc = ix->d_cand.grow((size_t)GB_N * cap * sizeof(u64)))) return rc;
  // (+ 1 word behind the counters: "a wave's pair list overflowed" -- see scatter_pairs_kernel)
  if ((rc = ix->d_count.grow(((size_t)nq + GB_N + 1) * sizeof(uint32_t)))) return rc;
  uint32_t* const d_lost = ix->d_count + nq + GB_N;
  if ((rc = ix->d_qb8.grow((size_t)GB_N * pitch8))) return rc;
  if ((rc = ix->d_qpar.grow((size_t)GB_N * sizeof(f4)))) return rc;
  // per-wave candidate pair lists of the full pass: room for 4x the expected share of a wave, at least 2048 pairs
  const uint32_t nwaves = std::min<uint32_t>(tiles, (uint32_t)ix->cu_count) * 8;
  const uint32_t pair_cap = selection_pair_cap(s.expect, nwaves);
  if ((rc = ix->d_pairs.grow((size_t)nwaves * pair_cap * sizeof(u64)))) return rc;
  if ((rc = ix->d_pair_count.grow((size_t)nwaves * sizeof(uint32_t)))) return rc;
  if (sharded && (rc = ix->d_local_keys.grow((size_t)GB_N * k * sizeof(u64)))) return rc;
  // (the counters of every block, tau and the lost flag are initialised by the block's queries_to_i8_kernel: no memsets)
  ix->last_batch_nq = (uint32_t)nq;
  ix->last_batch_cap = cap;
  ix->last_batch_masked = multi ? 2 : masked ? 1 : 0;
  ix->last_batch_allowed = masked ? ix->mask_allowed : ix->n;
  ix->last_batch_classes = multi ? (uint32_t)mc->plan->classes.size() : 0u;
  ix->last_batch_blocks = multi ? mc->plan->blocks() : 0u;
  const u64* gbad = ix->d_gbad8;
  const u64 ngroups = ix->d_groups8.bytes / sizeof(f4);  // (d_gbad8's entries: to the end of the last tile + the pad groups)
  if (masked || multi) {  // this call's bad-row table(s): one launch over the whole group table (8 bytes per 64 rows), no synchronisation
    const uint32_t rows = multi ? (uint32_t)mc->plan->classes.size() : 1u;
    if ((rc = ix->d_call_bad.grow((size_t)rows * ngroups * sizeof(u64)))) return rc;
    hipLaunchKernelGGL(gbad_with_mask_kernel, dim3(gbad_with_mask_grid(ngroups), rows), dim3(256), 0, ix->stream, (const u64*)ix->d_gbad8,
                       multi ? mc->d_masks : ix->active_mask, (u64)((ix->n + 31) / 32), ngroups, ix->d_call_bad,
                       (u64)(multi ? mc->mask_stride : 0), multi ? mc->d_class_mask : (const int32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    gbad = ix->d_call_bad;
  }
  const bool l2 = ix->metric == WDBX_METRIC_L2;
  if (l2 && (rc = ensure_row_norms(ix))) return rc;
  if ((rc = ensure_group_ref(ix))) return rc;
  const int max_ct = l2 ? std::min(2, i8g_max_ct(ix)) : i8g_max_ct(ix);  // (L2: query blocks of at most 128)
  // the class runs of a block with a mask per query: {first slot in the block, slots, class row} -- what reads ONE mask per
  // launch (the second selection stage, the repair scan) is launched per run
  struct ClassRun {
    int s0, n, row;
  };
  std::vector<ClassRun> runs;
  uint32_t mblock = 0;
  for (int q0 = 0; q0 < nq; ++mblock) {
    // (a mask per query: the plan's block -- its slots are whole column groups and fit the widest query block)
    const int rem = multi ? (int)(mc->plan->block_group[mblock + 1] - mc->plan->block_group[mblock]) * MULTIMASK_GROUP : nq - q0;
    int ct = (ix->opt_gemm_ct == 1 || ix->opt_gemm_ct == 2 || ix->opt_gemm_ct == 4) ? (int)ix->opt_gemm_ct : rem > 128 ? 4 : rem > 64 ? 2 : 1;
    ct = std::min(ct, max_ct);
    const int gbn = 64 * ct, nv = std::min(gbn, rem);
    if (multi && nv != rem) return fail(WDBX_E_STATE, "a block of %d slots for query blocks of %d", rem, gbn);
    const float* qsrc = d_queries + (size_t)q0 * ix->pitch;
    const uint32_t stride = tiles / (multi ? block_sample[mblock] : sample_tiles);
    if (multi) sample_tiles = block_sample[mblock];
    hipLaunchKernelGGL(queries_to_i8_kernel, dim3(queries_to_i8_grid((uint32_t)gbn)), dim3(256), 0, ix->stream, qsrc, (uint32_t)ix->dim,
                       (uint32_t)ix->pitch, (uint32_t)nv, ix->d_qb8, pitch8, (uint32_t)gbn, ix->d_qpar, ix->d_tau, ix->d_count + q0, d_lost);
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
    g.num_tiles = sample_tiles;
    g.tile_stride = stride;
    g.halfmax = ix->d_halfmax;
    if (multi) {
      const MultimaskPlan& pl = *mc->plan;
      g.n_class_groups = ngroups;
      runs.clear();
      for (uint32_t gi = pl.block_group[mblock]; gi < pl.block_group[mblock + 1]; ++gi) {
        const int j = (int)(gi - pl.block_group[mblock]);
        const int row = (int)(std::lower_bound(pl.classes.begin(), pl.classes.end(), pl.group_class[gi]) - pl.classes.begin());
        g.class_row[j] = (uint8_t)row;  // (column groups behind the block's last: row 0, all their queries padded)
        if (!runs.empty() && runs.back().row == row) runs.back().n += MULTIMASK_GROUP;
        else runs.push_back({j * MULTIMASK_GROUP, MULTIMASK_GROUP, row});
      }
    }
    if ((rc = launch_gemm8<0>(ix, g, ct, false, multi))) return rc;
    // the k-th largest of the groups' LOWER bounds: a valid threshold by itself (no margin)
    if ((rc = enqueue_sample_threshold(ix, rw * sample_tiles, k, nv, true))) return rc;
    if (multi) {  // the pad slots inside the block are padded queries
      hipLaunchKernelGGL(pad_tau_kernel, dim3((nv + 255) / 256), dim3(256), 0, ix->stream, ix->d_tau, mc->d_slot_query + q0, (uint32_t)nv);
      HIP_TRY(hipGetLastError());
    }
    g.num_tiles = tiles;
    g.tile_stride = 1;
    g.halfmax = nullptr;
    g.tau = ix->d_tau;
    g.pairs = ix->d_pairs;
    g.pair_count = ix->d_pair_count;
    g.pair_cap = pair_cap;
    if ((rc = launch_gemm8<1>(ix, g, ct, masked, multi))) return rc;
    hipLaunchKernelGGL(scatter_pairs_kernel, dim3((nwaves + SCATTER_LISTS - 1) / SCATTER_LISTS), dim3(1024), 0, ix->stream,
                       (const u64*)ix->d_pairs, (const uint32_t*)ix->d_pair_count, nwaves, pair_cap, ix->d_cand, ix->d_count + q0, cap,
                       d_lost);
    HIP_TRY(hipGetLastError());
    if (ix->opt_gemm8_refine) {
      // second selection stage (refine_pairs_kernel): the pairs' own integer dot products turn into per-row bounds, and the
      // rows that cannot be among the k best are dropped before the exact pass gathers any fp32 row
      RefineArgs r = {};
      r.cand = ix->d_cand;
      r.count = ix->d_count + q0;
      r.cap = cap;
      r.groups = ix->d_groups8;
      r.gbad = gbad;
      r.cn = ix->d_cn;
      r.qpar = ix->d_qpar;
      r.k = k;
      // (instance, waves, n_lds and LDS bytes: refine_launch_for -- within 128 KiB of LDS whatever k is, host_refine.h)
      RefineLaunch rl;
      HIP_TRY(refine_launch_for(l2 ? WDBX_METRIC_L2 : WDBX_METRIC_COSINE, k, cap, ix->opt_lds_lists != 0, &rl));
      r.n_lds = rl.shape.n_lds;
      if (multi) {  // (one workgroup per query, one bad-row table per launch: a launch per class run, its class's table)
        for (const ClassRun& cr : runs) {
          RefineArgs rr = r;
          rr.cand = r.cand + (size_t)cr.s0 * cap;
          rr.count = r.count + cr.s0;
          rr.qpar = r.qpar + cr.s0;
          rr.gbad = gbad + (size_t)cr.row * ngroups;
          HIP_TRY(enqueue_refine(ix->stream, rl, rr, cr.n));
        }
      } else {
        HIP_TRY(enqueue_refine(ix->stream, rl, r, nv));
      }
    }
    // exact fp32 scores of the kept rows (L2: the direct form sum (c - q)^2)
    hipLaunchKernelGGL(l2 ? rescore_kernel<WDBX_METRIC_L2> : rescore_kernel<WDBX_METRIC_COSINE>, dim3(64, nv), dim3(256), 0, ix->stream,
                       (const f4*)ix->d_rows.p, (uint32_t)pitch4, (const f4*)qsrc, ix->d_cand, (const uint32_t*)(ix->d_count + q0), cap,
                       (u64*)nullptr, (uint32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    MergeArgs f = final_topk_args(ix, ix->d_cand, cap, ix->d_count + q0, k);
    final_topk_output(ix, &f, keys_out, sharded, d_out_idx, d_out_score, q0, k);
    if ((rc = launch_merge(ix, f, nv))) return rc;
    if (multi) {
      // an overflowed query is repaired by the scan with ITS mask: the repair launches per class run, each with its class's
      // mask as the scan's (a run of the class without a mask: none)
      bool done = true;
      for (const ClassRun& cr : runs) {
        bool d1 = false;
        ix->active_mask = mc->d_class_mask && mc->plan->classes[(size_t)cr.row] >= 0 ? mc->d_masks + (size_t)cr.row * mc->mask_stride : nullptr;
        rc = enqueue_batch_repair(ix, qsrc + (size_t)cr.s0 * ix->pitch, cr.n, k, ix->d_count + q0 + cr.s0, cap, f.out_idx + (size_t)cr.s0 * k,
                                  f.out_score + (size_t)cr.s0 * k, nullptr, &d1, d_lost);
        ix->active_mask = nullptr;
        if (rc) return rc;
        done = done && d1;
      }
      ix->last_batch_repaired = q0 == 0 ? done : (ix->last_batch_repaired && done);
    } else {  // (marks the block's queries overflowed if a wave lost pairs, then the conditional repair launches)
      bool done = false;
      if ((rc = enqueue_batch_repair(ix, qsrc, nv, k, ix->d_count + q0, cap, f.out_idx, f.out_score, f.out_keys, &done, d_lost))) return rc;
      if (q0 == 0) ix->last_batch_repaired = done;
      else ix->last_batch_repaired = ix->last_batch_repaired && done;
    }
    if (sharded && (rc = exchange_and_merge(ix, nv, k, d_out_idx + (size_t)q0 * k, d_out_score + (size_t)q0 * k))) return rc;
    q0 += nv;
  }
  return WDBX_OK;
}

static int launch_normalize(wdbx_index* ix, float* d, uint64_t n) {
  if (!n) return WDBX_OK;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 3) / 4, 65536);
  hipLaunchKernelGGL(normalize_rows_kernel, dim3(blocks), dim3(256), 0, ix->stream, d, (u64)n, (uint32_t)ix->pitch);
  HIP_TRY(hipGetLastError());
  return WDBX_OK;
}

static int launch_fill(wdbx_index* ix, float* d, uint64_t seed, uint64_t row0, uint64_t n, int normalize) {
  if (!n) return WDBX_OK;
  const uint64_t total = n * (uint64_t)ix->pitch;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(fill_synthetic_kernel, dim3(blocks), dim3(256), 0, ix->stream, d, (u64)n, (uint32_t)ix->dim,
                     (uint32_t)ix->pitch, (u64)seed, (u64)row0);
  HIP_TRY(hipGetLastError());
  if (normalize) return launch_normalize(ix, d, n);
  return WDBX_OK;
}

static int reserve_locked(wdbx_index* ix, uint64_t cap) {
  if (cap <= ix->cap) return WDBX_OK;
  if (cap >= 0xFFFFFF00ull) return fail(WDBX_E_INVALID, "capacity %llu exceeds the 2^32 - 256 rows one shard can number", (u64)cap);
  // (+ TILE_PAD_ROWS rows of slack: the 8-wave tile kernels read whole 256-row tiles and mask rows past the end)
  const size_t bytes = ((size_t)cap + TILE_PAD_ROWS) * ix->pitch * sizeof(float);
  DevBuf<float> nd;  // (frees itself unless the handle adopts it)
  int rc = nd.grow(bytes);
  if (rc) return rc;
  if (ix->n) {
    hipError_t e = hipMemcpyAsync(nd, ix->d_rows, (size_t)ix->n * ix->pitch * sizeof(float), hipMemcpyDeviceToDevice,
                                  ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess) return fail(WDBX_E_HIP, "row copy during reserve failed: %s", hipGetErrorString(e));
  }
  rc = ix->d_rows.adopt(nd);
  ix->cap = cap;
  return rc;
}

static int upload_rows(wdbx_index* ix, uint64_t first, const float* rows, uint64_t n, int normalize) {
  float* dst = ix->d_rows + (size_t)first * ix->pitch;
  int rc = copy_padded(ix, dst, rows, n, ix->dim);
  if (rc) return rc;
  if (normalize && (rc = launch_normalize(ix, dst, n))) return rc;
  // Derived copies (cached norms, bf16 and u8 shadows) of OVERWRITTEN rows are refreshed right here, for exactly
  // those rows: an update in the middle of a large corpus must not invalidate everything behind it.  Rows appended
  // past what a copy covers are picked up lazily by the next search, as before.
  const uint64_t end = first + n;
  if (first < ix->cn_rows && ix->d_cn) {
    const uint64_t e = std::min(end, ix->cn_rows);
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3(row_sqnorm_grid(e - first)), dim3(256), 0, ix->stream,
                       (const float*)ix->d_rows, (u64)first, (u64)e, (uint32_t)ix->pitch, ix->d_cn, (uint32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    ix->gmax_valid = false;
    ix->cn_stats_dirty = true;  // the running maximum / sum would keep the overwritten rows' old norms
  }
  if (first < ix->shadow_rows && ix->d_rows16) {
    const uint64_t e = std::min(end, ix->shadow_rows);
    const u64 pieces = (e - first) * (ix->pitch16 / 8);
    hipLaunchKernelGGL(rows_to_bf16_kernel, dim3((uint32_t)std::min<u64>((pieces + 255) / 256, 1u << 20)), dim3(256), 0, ix->stream,
                       (const float*)ix->d_rows, (u64)first, (u64)e, (uint32_t)ix->pitch, (__bf16*)ix->d_rows16.p, ix->pitch16);
    HIP_TRY(hipGetLastError());
  }
  if (first < ix->shadowg_rows && ix->d_rows8g) {  // whole groups: a group's scale depends on all of its rows
    const uint64_t e = std::min(end, ix->shadowg_rows);
    const u64 g0 = first / 64, g1 = (e + 63) / 64;
    hipLaunchKernelGGL(rows_to_i8g_kernel, dim3(rows_to_i8g_grid(g1 - g0)), dim3(256), 0, ix->stream,
                       (const float*)ix->d_rows, g0, g1, (u64)std::max<uint64_t>(ix->n, end), (uint32_t)ix->dim, (uint32_t)ix->pitch,
                       ix->d_rows8g, ix->pitch8g, ix->d_groups8, ix->d_gbad8);
    HIP_TRY(hipGetLastError());
    ix->gref_valid = false;
  }
  if (first < ix->shadow8_rows && ix->d_rows8) {
    const uint64_t e = std::min(end, ix->shadow8_rows);
    hipLaunchKernelGGL(rows_to_u8_kernel, dim3(rows_to_u8_grid(e - first)), dim3(256), 0, ix->stream,
                       (const float*)ix->d_rows, (u64)first, (u64)e, (uint32_t)ix->dim, (uint32_t)ix->pitch, ix->d_rows8, ix->pitch8,
                       ix->d_scale8);
    HIP_TRY(hipGetLastError());
  }
  if (first < ix->shadow6_rows && ix->d_rows6) {
    const uint64_t e = std::min(end, ix->shadow6_rows);
    hipLaunchKernelGGL(rows_to_u6_kernel, dim3(rows_to_u6_grid(e - first)), dim3(256), 0, ix->stream,
                       (const float*)ix->d_rows, (u64)first, (u64)e, (uint32_t)ix->dim, (uint32_t)ix->pitch, ix->units6, ix->d_rows6,
                       (f2v*)(ix->d_rows6 + (size_t)ix->rows6_tiles * ix->units6 * 192));
    HIP_TRY(hipGetLastError());
  }
  if (first < ix->shadow42_rows && ix->d_rows42) HIP_TRY(launch_rows_to_u42(ix, first, std::min(end, ix->shadow42_rows)));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return WDBX_OK;
}

// ---- writes of listed rows (kernels_update.h, host_update.h) ------------------------------------------------------------
// ids: the call's validated list (strictly increasing, below ix->n), narrowed.  rows: [n, dim] in list order, or null for a
// removal (the scatter writes the NaN tombstone and nothing is uploaded).  What upload_rows does for a range, for the listed
// rows: the rows to their places (in rounds of UPDATE_ROUND_BYTES of caller rows), then every derived copy for exactly the
// listed rows it covers -- one refresh launch for the per-row copies, one for the int8 groups the list touches.  The number of
// launches does not depend on n beyond the rounds (read-only option "last_update_launches").  Returns when the device is done.
constexpr size_t UPDATE_KEEP_BYTES = 16u << 20;  // a larger block of caller rows is released at the end of its call
static int update_rows_at(wdbx_index* ix, const uint32_t* ids, uint64_t n, const float* rows, int normalize) {
  UpdateCoverage cov;
  cov.cn = ix->d_cn ? ix->cn_rows : 0;
  cov.bf16 = ix->d_rows16 ? ix->shadow_rows : 0;
  cov.i8g = ix->d_rows8g ? ix->shadowg_rows : 0;
  cov.u8 = ix->d_rows8 ? ix->shadow8_rows : 0;
  cov.u6 = ix->d_rows6 ? ix->shadow6_rows : 0;
  cov.u42 = ix->d_rows42 ? ix->shadow42_rows : 0;
  const UpdatePlan p = update_plan(ids, n, (uint32_t)ix->dim, cov, rows != nullptr);
  ix->last_update_launches = p.launches;
  if (!n) return WDBX_OK;
  int rc = ix->d_upd_list.grow((size_t)(n + p.groups.size()) * sizeof(uint32_t));
  if (rc) return rc;
  const uint32_t* d_list = ix->d_upd_list;
  const uint32_t* d_groups = d_list + n;
  HIP_TRY(hipMemcpyAsync(ix->d_upd_list, ids, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
  if (!p.groups.empty())
    HIP_TRY(hipMemcpyAsync(ix->d_upd_list + n, p.groups.data(), p.groups.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
  if (rows && (rc = ix->d_upd_rows.grow((size_t)std::min<uint64_t>(n, p.round_rows) * ix->dim * sizeof(float)))) return rc;
  for (uint64_t round = 0; round < p.rounds; ++round) {
    const uint64_t i0 = update_round_first(p, round), c = update_round_count(p, round);
    if (rows)  // (stream order keeps this copy behind the scatter that read the block's previous contents)
      HIP_TRY(hipMemcpyAsync(ix->d_upd_rows, rows + (size_t)i0 * ix->dim, (size_t)c * ix->dim * sizeof(float), hipMemcpyHostToDevice, ix->stream));
    hipLaunchKernelGGL(update_scatter_kernel, dim3(update_rows_grid(c)), dim3(256), 0, ix->stream,
                       rows ? (const float*)ix->d_upd_rows : (const float*)nullptr, d_list, (u64)i0, (u64)c, (uint32_t)ix->dim, (uint32_t)ix->pitch,
                       (float*)ix->d_rows, normalize);
    HIP_TRY(hipGetLastError());
  }
  // the validity flags upload_rows drops for an overwritten row of the same copies
  if (p.n_cn) {
    ix->gmax_valid = false;
    ix->cn_stats_dirty = true;
  }
  if (p.n_refresh) {
    UpdateArgs a = {};
    a.rows = ix->d_rows;
    a.list = d_list;
    a.dim = (uint32_t)ix->dim;
    a.pitch = (uint32_t)ix->pitch;
    a.n_cn = p.n_cn, a.n_16 = p.n_16, a.n_8 = p.n_8, a.n_6 = p.n_6, a.n_42 = p.n_42;
    a.cn = ix->d_cn;
    a.rows16 = (__bf16*)ix->d_rows16.p;
    a.pitch16 = ix->pitch16;
    a.rows8 = ix->d_rows8;
    a.pitch8 = ix->pitch8;
    a.scale8 = ix->d_scale8;
    if (p.n_6) {
      a.units6 = ix->units6;
      a.codes6 = ix->d_rows6;
      a.sa6 = (f2v*)(ix->d_rows6 + (size_t)ix->rows6_tiles * ix->units6 * 192);
    }
    if (p.n_42) {
      a.units42 = ix->units42;
      a.lpitch42 = u42_lpitch(ix->units42);
      a.h42 = ix->d_rows42;
      a.sa42 = u42_sa4(ix);
      a.lrec42 = u42_lrec(ix);
    }
    hipLaunchKernelGGL(update_refresh_kernel, dim3(update_rows_grid(p.n_refresh)), dim3(256), 0, ix->stream, a);
    HIP_TRY(hipGetLastError());
  }
  if (!p.groups.empty()) {  // whole groups: a group's scale depends on all of its rows
    hipLaunchKernelGGL(rows_to_i8g_list_kernel, dim3(rows_to_i8g_list_grid(p.groups.size())), dim3(256), 0, ix->stream,
                       (const float*)ix->d_rows, d_groups, (u64)p.groups.size(), (u64)ix->n, (uint32_t)ix->dim, (uint32_t)ix->pitch,
                       ix->d_rows8g, ix->pitch8g, ix->d_groups8, ix->d_gbad8);
    HIP_TRY(hipGetLastError());
    ix->gref_valid = false;
  }
  HIP_TRY(hipStreamSynchronize(ix->stream));  // (ids, the plan's groups and the caller's rows are free again)
  if (ix->d_upd_rows.bytes > UPDATE_KEEP_BYTES) return ix->d_upd_rows.release();
  return WDBX_OK;
}

// ---- what the blocking entry points share (wdbx_hip.hip) ------------------------------------------------------------
// nq of the caller's queries (src_pitch floats apart, 0 = dim) into d_q at the row pitch, normalised for cosine when asked
static int upload_queries(wdbx_index* ix, const float* queries, uint64_t nq, int normalize_queries, int src_pitch = 0) {
  int rc = ix->d_q.grow((size_t)nq * ix->pitch * sizeof(float));
  if (rc || (rc = copy_padded(ix, ix->d_q, queries, nq, src_pitch ? src_pitch : ix->dim))) return rc;
  if (normalize_queries && ix->metric == WDBX_METRIC_COSINE) return launch_normalize(ix, ix->d_q, nq);
  return WDBX_OK;
}

// the first elems results of d_oidx / d_oscore to the host; returns when they are there
static int download_results(wdbx_index* ix, size_t elems, int64_t* out_idx, float* out_score) {
  HIP_TRY(hipMemcpyAsync(out_idx, ix->d_oidx, elems * sizeof(int64_t), hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipMemcpyAsync(out_score, ix->d_oscore, elems * sizeof(float), hipMemcpyDeviceToHost, ix->stream));
  HIP_TRY(hipStreamSynchronize(ix->stream));
  return WDBX_OK;
}

// ... of a call that placed its queries in slots: slot s holds the k results of the caller's query slot_query[s] (-1: a pad)
static int download_results(wdbx_index* ix, const std::vector<int32_t>& slot_query, int k, int64_t* out_idx, float* out_score) {
  const size_t slots = slot_query.size();
  std::vector<int64_t> h_idx(slots * (size_t)k);
  std::vector<float> h_score(slots * (size_t)k);
  const int rc = download_results(ix, slots * (size_t)k, h_idx.data(), h_score.data());
  if (rc) return rc;
  for (size_t s = 0; s < slots; ++s) {
    const int32_t q = slot_query[s];
    if (q < 0) continue;
    memcpy(out_idx + (size_t)q * k, &h_idx[s * k], (size_t)k * sizeof(int64_t));
    memcpy(out_score + (size_t)q * k, &h_score[s * k], (size_t)k * sizeof(float));
  }
  return WDBX_OK;
}

// one query whose candidate buffer overflowed, again: straight to the fp32 scan (the selection would overflow again)
static int enqueue_exact_rerun(wdbx_index* ix, const float* dq, int k, int64_t* out_idx, float* out_score) {
  const int64_t keep = ix->opt_scan_shadow;
  ix->opt_scan_shadow = 0;
  const int rc = enqueue_search(ix, dq, 1, k, out_idx, out_score, SEARCH_FINAL);
  ix->opt_scan_shadow = keep;
  return rc;
}

// ---- recommend search (kernels_recommend.h, host_recommend.h): one side's pass for `slots` queries ------------------------
// d_table holds the slots' example table, the examples are in d_q, the mask (if any) is the active one.  Rounds of rp.round
// slots: recommend_kernel (bracketed as a scan launch), then the ranking tail (enqueue_rank_tail).  Results: d_oidx / d_oscore
// [slots, k].  The disfavoured side's key value is -n in the ranking domain, so the tail converts it with the OTHER metric's
// sign: out_score is n in the caller's units.
static RankSource corpus_rank_source(const wdbx_index* ix, bool lists, uint32_t P) {  // (a corpus pass: P lists, or a key per row)
  return lists ? RankSource{RankSource::LISTS, ix->d_partials, P, nullptr} : RankSource{RankSource::SELECT, ix->d_sub_keys, ix->n, nullptr};
}

static int enqueue_recommend_pass(wdbx_index* ix, const RecommendPlan& rp, const uint32_t* d_table, int slots, int k, int side,
                                  const uint32_t* d_exclude, uint32_t n_exclude) {
  const uint32_t pitch4 = (uint32_t)ix->pitch / 4;
  const recommend_fn fn = pick_recommend(ix->metric, rp.mode, pitch4);
  if (!fn) return fail(WDBX_E_STATE, "no recommend instance for mode %d", rp.mode);
  const bool lists = rp.mode != 2;
  const size_t lds = lists ? rp.lds : 0;
  if (lds >= 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  int rc;
  for (const std::pair<int, int>& r : recommend_rounds(slots, rp.round)) {
    const int q0 = r.first, b = r.second;
    RecommendArgs a = {};
    a.rows = (const f4*)ix->d_rows.p;
    a.examples = (const f4*)ix->d_q.p;
    a.table = d_table + (size_t)q0 * 3;
    a.mask = ix->active_mask;
    a.exclude = d_exclude;
    a.out = lists ? ix->d_partials : ix->d_sub_keys;
    a.key_stride = ix->n;
    a.n_exclude = n_exclude;
    a.n_rows = (uint32_t)ix->n;
    a.pitch4 = pitch4;
    a.k = k;
    a.side = side;
    if ((rc = record(ix->scan_ev, ix->profile, ix->stream, true))) return rc;
    hipLaunchKernelGGL(fn, dim3(rp.blocks, (uint32_t)b), dim3(256), lds, ix->stream, a);
    HIP_TRY(hipGetLastError());
    if ((rc = record(ix->scan_ev, ix->profile, ix->stream, false))) return rc;
    const int metric = side ? ix->metric : (ix->metric == WDBX_METRIC_L2 ? WDBX_METRIC_COSINE : WDBX_METRIC_L2);
    if ((rc = enqueue_rank_tail(ix, corpus_rank_source(ix, lists, rp.P), q0, b, k, metric))) return rc;
  }
  return WDBX_OK;
}

// The call under the handle's lock (the caller holds it, has checked the arguments that need no lock, and resets the mask):
//   1. the favoured pass for all queries;  2. the disfavoured pass for the queries that came back short of k only;
//   3. the splice (host_recommend.h).
static int recommend_locked(wdbx_index* ix, const float* examples, const uint64_t* off, int nq, int k, int normalize_examples,
                            const uint32_t* mask_words, const std::vector<uint32_t>& exclude32, MaskScope& scope, int64_t* out_idx,
                            float* out_score, uint8_t* out_side) {
  const size_t elems = (size_t)nq * k;
  const RecommendPlan rp = recommend_plan(ix->n, nq, k, ix->cu_count, ix->opt_select_min_k, ix->opt_lds_lists != 0);
  int rc;
  if ((rc = ensure_out(ix, elems))) return rc;
  const size_t n_ex = exclude32.size();
  const size_t tab_words = (size_t)nq * 3;
  if ((rc = ix->d_rec.grow((2 * tab_words + std::max<size_t>(n_ex, 1)) * sizeof(uint32_t)))) return rc;
  uint32_t* d_tab = (uint32_t*)ix->d_rec.p;
  uint32_t* d_tab_short = d_tab + tab_words;
  uint32_t* d_exclude = d_tab_short + tab_words;
  if ((rc = grow_rank_scratch(ix, rp.mode != 2 ? RankSource::LISTS : RankSource::SELECT, rp.scratch_u64))) return rc;
  if ((rc = upload_queries(ix, examples, off[2 * nq], normalize_examples))) return rc;
  if (mask_words && (rc = scope.set(mask_words))) return rc;
  std::vector<uint32_t> all((size_t)nq), tab(tab_words);
  for (int q = 0; q < nq; ++q) all[(size_t)q] = (uint32_t)q;
  recommend_table(off, all.data(), all.size(), tab.data());
  HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab_words * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
  if (n_ex) HIP_TRY(hipMemcpyAsync(d_exclude, exclude32.data(), n_ex * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
  if ((rc = enqueue_recommend_pass(ix, rp, d_tab, nq, k, 1, d_exclude, (uint32_t)n_ex))) return rc;
  std::vector<int64_t> fav_idx(elems), dis_idx;
  std::vector<float> fav_score(elems), dis_score;
  if ((rc = download_results(ix, elems, fav_idx.data(), fav_score.data()))) return rc;
  ix->last_recommend_path = 1;
  std::vector<uint32_t> short_queries;
  std::vector<int> gaps;
  recommend_short(fav_idx.data(), nq, k, &short_queries, &gaps);
  if (!short_queries.empty()) {
    const int ns = (int)short_queries.size();
    std::vector<uint32_t> tab_short((size_t)ns * 3);
    recommend_table(off, short_queries.data(), short_queries.size(), tab_short.data());
    HIP_TRY(hipMemcpyAsync(d_tab_short, tab_short.data(), tab_short.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
    const RecommendPlan rs = recommend_plan(ix->n, ns, k, ix->cu_count, ix->opt_select_min_k, ix->opt_lds_lists != 0);
    // (fewer queries: a wider grid, so longer partial lists per query; the mode is the first pass's: it goes by k alone)
    if ((rc = grow_rank_scratch(ix, rs.mode != 2 ? RankSource::LISTS : RankSource::SELECT, rs.scratch_u64))) return rc;
    if ((rc = enqueue_recommend_pass(ix, rs, d_tab_short, ns, k, 0, d_exclude, (uint32_t)n_ex))) return rc;
    dis_idx.resize((size_t)ns * k);
    dis_score.resize((size_t)ns * k);
    if ((rc = download_results(ix, (size_t)ns * k, dis_idx.data(), dis_score.data()))) return rc;
    ix->last_recommend_path = 2;
    ix->last_recommend_short = ns;
  }
  recommend_splice(fav_idx.data(), fav_score.data(), dis_idx.data(), dis_score.data(), short_queries, nq, k, out_idx, out_score, out_side);
  return WDBX_OK;
}

// ---- discovery search (kernels_discover.h, host_discover.h) -----------------------------------------------------------------
// The call under the handle's lock (the caller holds it, has checked the arguments that need no lock, and resets the mask).
// Context mode (no targets): per round the scoring pass ranks by the loss and the tail follows; the loss is a ranking-domain
// value for either metric, so the tail never applies the L2 sign.  Target mode, per round of queries:
//   1. the scoring pass writes every row's record and the zones' counts;  2. one small download of the counts;
//   3. the zones each query needs (discover_zones), one zone launch per round of (query, zone) slots and its tail;
//   4. the splice (host_discover.h).
static int discover_locked(wdbx_index* ix, const float* targets, const float* context, const uint64_t* off, int nq, int k,
                           int normalize_vectors, const uint32_t* mask_words, const std::vector<uint32_t>& exclude32, MaskScope& scope,
                           int64_t* out_idx, float* out_score, uint8_t* out_wins) {
  const bool target = targets != nullptr;
  const uint32_t pitch4 = (uint32_t)ix->pitch / 4;
  const DiscoverPlan dp = discover_plan(ix->n, nq, k, target, ix->cu_count, ix->opt_select_min_k, ix->opt_lds_lists != 0);
  const bool lists = dp.mode != 2;
  const discover_fn fn = pick_discover(ix->metric, target ? 3 : dp.mode, pitch4);
  if (!fn) return fail(WDBX_E_STATE, "no discover instance for mode %d", dp.mode);
  int rc;
  // the round's state: records (keys | wins) | counts | query table | zone table | exclusion list
  const size_t n_ex = exclude32.size();
  const size_t key_bytes = dp.record_rows * sizeof(u64);
  const size_t counts_at = (key_bytes + dp.record_rows + 7) / 8 * 8;
  const size_t counts_words = target ? (size_t)dp.round * DISCOVER_ZONES : 0;
  const size_t qtab_at = counts_at + counts_words * sizeof(uint32_t);
  const size_t ztab_at = qtab_at + (size_t)nq * 2 * sizeof(uint32_t);
  const size_t ztab_words = counts_words * 2;
  const size_t ex_at = ztab_at + ztab_words * sizeof(uint32_t);
  if ((rc = ix->d_disc.grow(ex_at + std::max<size_t>(n_ex, 1) * sizeof(uint32_t)))) return rc;
  u64* d_rec_key = (u64*)ix->d_disc.p;
  uint8_t* d_rec_wins = (uint8_t*)(ix->d_disc + key_bytes);
  uint32_t* d_counts = (uint32_t*)(ix->d_disc + counts_at);
  uint32_t* d_qtab = (uint32_t*)(ix->d_disc + qtab_at);
  uint32_t* d_ztab = (uint32_t*)(ix->d_disc + ztab_at);
  uint32_t* d_exclude = (uint32_t*)(ix->d_disc + ex_at);
  const RankSource::Form form = lists ? RankSource::LISTS : RankSource::SELECT;
  if (!target && (rc = grow_rank_scratch(ix, form, dp.scratch_u64))) return rc;
  if ((rc = ensure_out(ix, (size_t)nq * k))) return rc;
  // the staged vectors: context mode's are the caller's array as it is
  const uint64_t staged = discover_staged_count(off, nq, target);
  std::vector<float> stage;
  if (target) {
    stage.resize((size_t)staged * ix->dim);
    discover_stage(targets, context, off, nq, ix->dim, stage.data());
  }
  if ((rc = upload_queries(ix, target ? stage.data() : context, staged, normalize_vectors))) return rc;
  if (mask_words && (rc = scope.set(mask_words))) return rc;
  std::vector<uint32_t> qtab((size_t)nq * 2);
  discover_table(off, 0, nq, target, qtab.data());
  HIP_TRY(hipMemcpyAsync(d_qtab, qtab.data(), qtab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
  if (n_ex) HIP_TRY(hipMemcpyAsync(d_exclude, exclude32.data(), n_ex * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
  const size_t lds = (!target && lists) ? dp.lds : 0;
  if (lds >= 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ix->last_discover_path = target ? 2 : 1;
  for (const std::pair<int, int>& r : recommend_rounds(nq, dp.round)) {
    const int q0 = r.first, b = r.second;
    DiscoverArgs a = {};
    a.rows = (const f4*)ix->d_rows.p;
    a.vectors = (const f4*)ix->d_q.p;
    a.table = d_qtab + (size_t)q0 * 2;
    a.mask = ix->active_mask;
    a.exclude = d_exclude;
    a.out = target ? d_rec_key : (lists ? ix->d_partials : ix->d_sub_keys);
    a.wins = d_rec_wins;
    a.counts = d_counts;
    a.key_stride = ix->n;
    a.n_exclude = (uint32_t)n_ex;
    a.n_rows = (uint32_t)ix->n;
    a.pitch4 = pitch4;
    a.k = k;
    if (target) HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)b * DISCOVER_ZONES * sizeof(uint32_t), ix->stream));
    if ((rc = record(ix->scan_ev, ix->profile, ix->stream, true))) return rc;
    hipLaunchKernelGGL(fn, dim3(dp.blocks, (uint32_t)b), dim3(256), lds, ix->stream, a);
    HIP_TRY(hipGetLastError());
    if ((rc = record(ix->scan_ev, ix->profile, ix->stream, false))) return rc;
    if (!target) {
      if ((rc = enqueue_rank_tail(ix, corpus_rank_source(ix, lists, dp.P), q0, b, k, WDBX_METRIC_COSINE))) return rc;
      continue;
    }
    std::vector<uint32_t> counts((size_t)b * DISCOVER_ZONES);
    HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    std::vector<std::vector<DiscoverZone>> zones((size_t)b);
    std::vector<uint32_t> ztab;
    for (int q = 0; q < b; ++q) {
      zones[(size_t)q] = discover_zones(&counts[(size_t)q * DISCOVER_ZONES], k);
      for (const DiscoverZone& z : zones[(size_t)q]) {
        ztab.push_back((uint32_t)q);
        ztab.push_back(z.zone);
      }
    }
    const int zslots = (int)(ztab.size() / 2);
    std::vector<int64_t> z_idx((size_t)zslots * k);
    std::vector<float> z_score((size_t)zslots * k);
    if (zslots) {
      const DiscoverZonePlan zp = discover_zone_plan(ix->n, zslots, k, dp.mode, ix->cu_count);
      const discover_zone_fn zfn = pick_discover_zone(dp.mode);
      if (!zfn) return fail(WDBX_E_STATE, "no discover zone instance for mode %d", dp.mode);
      if ((rc = grow_rank_scratch(ix, form, zp.scratch_u64))) return rc;
      if ((rc = ensure_out(ix, (size_t)zslots * k))) return rc;
      if (zp.lds >= 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)zfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)zp.lds));
      HIP_TRY(hipMemcpyAsync(d_ztab, ztab.data(), ztab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ix->stream));
      for (const std::pair<int, int>& zr : recommend_rounds(zslots, zp.round)) {
        DiscoverZoneArgs za = {};
        za.rec_key = d_rec_key;
        za.rec_wins = d_rec_wins;
        za.table = d_ztab + (size_t)zr.first * 2;
        za.out = lists ? ix->d_partials : ix->d_sub_keys;
        za.rec_stride = ix->n;
        za.n_rows = (uint32_t)ix->n;
        za.k = k;
        if ((rc = record(ix->merge_ev, ix->profile, ix->stream, true))) return rc;
        hipLaunchKernelGGL(zfn, dim3(zp.blocks, (uint32_t)zr.second), dim3(256), zp.lds, ix->stream, za);
        HIP_TRY(hipGetLastError());
        if ((rc = record(ix->merge_ev, ix->profile, ix->stream, false))) return rc;
        if ((rc = enqueue_rank_tail(ix, corpus_rank_source(ix, lists, zp.P), zr.first, zr.second, k, ix->metric))) return rc;
      }
      if ((rc = download_results(ix, (size_t)zslots * k, z_idx.data(), z_score.data()))) return rc;
      ix->last_discover_zone_slots += zslots;
    }
    discover_splice(zones, z_idx.data(), z_score.data(), k, out_idx + (size_t)q0 * k, out_score + (size_t)q0 * k,
                    out_wins ? out_wins + (size_t)q0 * k : nullptr);
  }
  if (!target) {
    if ((rc = download_results(ix, (size_t)nq * k, out_idx, out_score))) return rc;
    if (out_wins) memset(out_wins, 0, (size_t)nq * k);
  }
  return WDBX_OK;
}
