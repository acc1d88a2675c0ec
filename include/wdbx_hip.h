/*
 * wdbx_hip.h -- C ABI of the MI355X-native WDBX vector_search hot path.
 *
 * One shared library (libwdbx_hip.so, built from wdbx-py_amd/csrc/wdbx_hip.hip for
 * gfx950) replaces what the reference reaches through third-party native code on
 * the path WDBX.vector_search -> VectorStore.search -> VectorIndex.search:
 *
 *   reference interface (paths under /root/reference)            replaced by
 *   ------------------------------------------------------------------------------
 *   faiss.IndexFlatIP(dim)            wdbx/core/indexing.py:717   wdbx_index_create
 *   faiss.index_cpu_to_gpu(res,0,ix)  indexing.py:741-748         wdbx_index_create(device_id)
 *   index.add(rows[n,d])              indexing.py:890, :950       wdbx_index_add
 *   _normalize_vector at add          indexing.py:851-856,886,939 wdbx_index_add(normalize=1)
 *   hnswlib replace_vector            indexing.py:374, :431, :552 wdbx_index_set_rows
 *   index.search(q[1,d], k)           indexing.py:1013 (and :490) wdbx_index_search
 *   faiss IndexFlat range_search      (never reached: the reference  wdbx_index_range_search
 *                                      post-filters a top-k, vector_store.py:337-342)
 *   self.next_index / index.ntotal    indexing.py:998, :1005      wdbx_index_size
 *   _create_index() on clear          indexing.py:1098            wdbx_index_clear
 *   per-shard loop + list.sort merge  vector_store.py:323-345     wdbx_index_search_sharded_device
 *                                                                 (RCCL all-gather + merge)
 *
 * Conventions
 *   - every function returns 0 (WDBX_OK) or a negative WDBX_E_* code and never
 *     throws; wdbx_last_error() gives the calling thread's last message.
 *   - host buffers are caller-owned and only read/written during the call; device
 *     memory, streams and events are owned by the library.
 *   - rows are fp32, row-major [n, dim].  In HBM a row occupies
 *     wdbx_index_row_pitch() floats (dim rounded up to a multiple of 4, zero padded).
 *   - metric 0 = cosine as the reference does it: inner product over rows that
 *     were unit-normalised at add time; the query is normalised by the caller or
 *     with normalize_queries=1.  metric 1 = squared L2 (extension).
 *   - result order is total and deterministic: (score descending, row ascending)
 *     for cosine, (distance ascending, row ascending) for L2; unused result slots
 *     hold row -1 (like faiss, indexing.py:1023).  Rows whose score is NaN are
 *     never returned.
 *   - thread-safety: any thread may call into one handle (the reference calls search from
 *     4-worker pools, indexing.py:692, :1045-1048).  A handle mutex serialises everything that
 *     touches the handle's state, i.e. the ENQUEUE of a call's launches; a small blocking search
 *     (queries and results in one of 4 mapped staging slots) waits for the GPU on its own event
 *     with the mutex released, so concurrent callers pipeline on the handle's stream instead of
 *     taking turns at wall-clock latency.  Calls with a row mask, batched calls and ingest keep
 *     the mutex to their end.
 */
#ifndef WDBX_HIP_H
#define WDBX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WDBX_HIP_ABI_VERSION 1

#define WDBX_OK 0
#define WDBX_E_INVALID (-1)   /* bad argument */
#define WDBX_E_HIP (-2)       /* HIP runtime error (message has the hipError string) */
#define WDBX_E_NOMEM (-3)     /* device or host allocation failed */
#define WDBX_E_NODEVICE (-4)  /* no usable GPU */
#define WDBX_E_RCCL (-5)      /* RCCL error */
#define WDBX_E_STATE (-6)     /* call not valid in the handle's state */

#define WDBX_METRIC_COSINE 0
#define WDBX_METRIC_L2 1

#define WDBX_MAX_K 2048 /* largest k one search accepts */

typedef struct wdbx_index wdbx_index;

/* ---- library ---------------------------------------------------------------- */
int wdbx_hip_version(void);
const char* wdbx_last_error(void);
int wdbx_device_count(int* out_count);

/* ---- one shard = one flat index resident in one GPU's HBM -------------------- */
int wdbx_index_create(int device_id, int dim, int metric, uint64_t capacity_rows, wdbx_index** out);
void wdbx_index_destroy(wdbx_index* idx);
int wdbx_index_dim(const wdbx_index* idx);
int wdbx_index_row_pitch(const wdbx_index* idx); /* floats per stored row */
int wdbx_index_size(wdbx_index* idx, uint64_t* out_rows);
int wdbx_index_capacity(wdbx_index* idx, uint64_t* out_rows);
int wdbx_index_reserve(wdbx_index* idx, uint64_t capacity_rows); /* grow (copies rows device-to-device) */
int wdbx_index_clear(wdbx_index* idx);

/* append n host rows [n, dim]; normalize!=0 unit-normalises each row on the device
 * (a zero row stays zero, indexing.py:853-856); *first_row_out = index of the first
 * appended row (rows are numbered in append order, as faiss/next_index do). */
int wdbx_index_add(wdbx_index* idx, const float* rows, uint64_t n, int normalize, uint64_t* first_row_out);
/* overwrite stored rows [first_row, first_row+n) (replace_vector / zero-on-remove) */
int wdbx_index_set_rows(wdbx_index* idx, uint64_t first_row, const float* rows, uint64_t n, int normalize);
/* Batch upsert and delete of LISTED rows (the write side of batch_store / delete): overwrite the stored rows row_ids[0 .. n)
 * with rows[n, dim] (in the order of row_ids), or turn them into removed rows, in one call.
 *   row_ids is strictly increasing and every row lies below the index size; a list that is not strictly increasing, a row at
 *   or past the size, or a null pointer with n > 0 is WDBX_E_INVALID (wdbx_index_search_rows' rule for its list) and nothing
 *   is written.  n == 0 is a no-op that returns WDBX_OK.
 *   wdbx_index_remove_rows writes the NaN tombstone a removed row holds (quiet NaN in every element: never a result on any
 *   path); it uploads no row data, the kernel writes the NaN.
 * Contract.  After the call the fp32 rows are exactly what wdbx_index_set_rows called once per listed row with the same
 * normalize (for a removal: with a row of NaN) would have left, and every derived copy that exists -- cached norms, bf16, the
 * int8 groups with their scales and bad-row words, u8 and its scales, u6, the two u42 planes and their records -- is the same
 * bit for bit: both forms run the same per-row device functions.  (One exception below a copy's horizon only: an int8 group
 * that the copy's coverage cuts is quantised from the group's rows as they are at the end of the call, not as they were when
 * its last covered row was written; the rows behind the coverage are re-quantised by the lazy pick-up in both cases.)  Rows
 * past a copy's coverage stay for the lazy pick-up of the next search, as with wdbx_index_set_rows, and the same validity flags
 * fall (group maxima, norm statistics, group reference bounds).  Labels are left alone.  No other entry point changes.
 * Cost.  One upload of the list and one of the rows (in rounds of at most 256 MiB), then per round one scatter launch, one
 * launch that refreshes every per-row copy of the listed rows and one for the int8 groups the list touches: the number of
 * launches does not depend on n beyond the rounds (get_option "last_update_launches").  Both calls hold the handle's mutex
 * and return when the device is done, as wdbx_index_set_rows does. */
int wdbx_index_set_rows_at(wdbx_index* idx, const uint64_t* row_ids, uint64_t n, const float* rows, int normalize);
int wdbx_index_remove_rows(wdbx_index* idx, const uint64_t* row_ids, uint64_t n);
/* keep exactly the stored rows src_rows[0 .. n_keep) (strictly increasing row numbers), moved down to rows
 * 0 .. n_keep - 1 in that order; everything else is dropped.  The compaction behind the backend's optimize()
 * (the reference rebuilds its index there, indexing.py:1124-1149): removed rows are NaN tombstones that every scan
 * still streams.  Row order is preserved; shadow copies are rebuilt lazily from the first moved row on. */
int wdbx_index_compact(wdbx_index* idx, const uint64_t* src_rows, uint64_t n_keep);
/* read stored rows back (as stored, i.e. after normalisation) into out_rows[n, dim] */
int wdbx_index_get_rows(wdbx_index* idx, uint64_t first_row, uint64_t n, float* out_rows);
/* append n synthetic rows generated on the device: element (r, c) of counter row
 * r = counter_row0 + i is ((splitmix64(seed ^ (r*dim + c)) >> 40) - 2^23) * 2^-23
 * (BASELINE.md section 3); optional unit normalisation. */
int wdbx_index_fill_synthetic(wdbx_index* idx, uint64_t seed, uint64_t counter_row0, uint64_t n,
                              int normalize, uint64_t* first_row_out);

/* blocking search of nq host queries [nq, dim]: out_idx[nq, k] (row or -1),
 * out_score[nq, k] (inner product, or squared distance for L2).
 * Every result is the exact fp32 ranking.  How a single query is answered (option "scan_shadow"):
 *   2 (default) a selection scan over a u8 SHADOW COPY of the rows (per-row scales; +25 % device memory, built and
 *               refreshed lazily) keeps every row whose score could reach the k-th best under a rigorous
 *               quantisation bound; the kept rows are re-scored in fp32 from the fp32 rows.  Applies from
 *               65 536 rows (131 072 for a call with a single query), dim 54 ... 4096, any k, with or without a row
 *               mask; an overflowing candidate buffer is repaired on the device by the fp32 scan.
 *   1           the same selection on the bf16 tile kernel over the bf16 shadow (k < 200, no masks)
 *   0           the fp32 scan kernel
 * From "gemm_min_queries" (4) queries per call the batched path below answers them in one pass. */
int wdbx_index_search(wdbx_index* idx, const float* queries, int nq, int k, int normalize_queries,
                      int64_t* out_idx, float* out_score);

/* same with a row filter (metadata push-down; the reference only post-filters,
 * vector_store.py:337-342): bit r of mask_words (uint32 words, bit r%32 of word r/32,
 * ceil(size/32) words, host memory) says whether row r may be returned.  The result is the exact
 * top-k of the allowed rows. */
int wdbx_index_search_masked(wdbx_index* idx, const float* queries, int nq, int k, int normalize_queries,
                             const uint32_t* mask_words, int64_t* out_idx, float* out_score);
/* the same, with the number of words the mask holds: checked against the row count UNDER the handle's lock, so a mask
 * built before a concurrent add (the reference mutates its indices from pool threads, indexing.py:381-383, :407) is
 * refused with WDBX_E_INVALID instead of over-read.  What the Python binding calls. */
int wdbx_index_search_masked_n(wdbx_index* idx, const float* queries, int nq, int k, int normalize_queries,
                               const uint32_t* mask_words, uint64_t mask_word_count, int64_t* out_idx, float* out_score);

/* ---- one row mask PER QUERY in one batched call ------------------------------- */
/* The workload row masks exist for is one filter per tenant, user or language: a batch whose queries do not share a mask.
 * mask_words[0 .. n_masks) are masks in the format of wdbx_index_search_masked_n (mask_word_counts[m] words each, checked
 * against the row count under the handle's lock), query_mask[i] says which of them query i reads, -1 = every row.  Blocking,
 * host buffers.
 *   Results: in the CALLER'S query order; format, order, -1 slots and NaN handling as wdbx_index_search_masked_n.  Query i's
 *   answer is the exact fp32 top-k of the rows its mask allows, bit-identical to wdbx_index_search_masked_n called with that
 *   query alone and its mask (wdbx_index_search for a -1 query) -- except for queries whose candidate buffer overflowed: they
 *   are repaired by the fp32 scan with THEIR mask and carry its scores (same ids, scores up to 1 ulp apart), as repaired
 *   queries of every batch do.
 *   WDBX_E_INVALID: n_masks outside [0, WDBX_MAX_CALL_MASKS], a query_mask entry outside [-1, n_masks), a mask shorter than
 *   ceil(rows / 32) words, a null mask pointer, k outside [1, WDBX_MAX_K], nq < 1.  n_masks == 0 with every entry -1 is the
 *   unmasked batch.
 *   Route: when the int8 tiles are what a masked batch would run (gemm_bf16 = 3, gemm8_variant = 0, k below the select range,
 *   option gemm_masked, enough queries and rows for the batched path) the call is ONE tile pass per block of up to 256 placed
 *   queries (128 for L2 and rows beyond 384 bytes of i8), whatever the number of masks: the queries are sorted by mask, each
 *   mask's queries padded to whole column groups of 16, and the kernels read the mask word of the column group at hand
 *   (get_option "last_batch_masked" == 2, "last_batch_mask_classes" = distinct masks the call used, the maskless class
 *   included, "last_batch_blocks" = tile blocks it ran; wdbx_index_batch_status reports its counts in the caller's query
 *   order).  Otherwise every distinct mask's queries go through wdbx_index_search_masked_n (wdbx_index_search for -1) and
 *   the answers are scattered back.  Exact either way.
 *   The call holds the handle's mutex to its end.  Nothing of a call's masks stays valid in the handle. */
#define WDBX_MAX_CALL_MASKS 64
int wdbx_index_search_multimask(wdbx_index* idx, const float* queries, int nq, int k, int normalize_queries,
                                const uint32_t* const* mask_words, const uint64_t* mask_word_counts, int n_masks,
                                const int32_t* query_mask, /* [nq]: index into mask_words, or -1 = every row */
                                int64_t* out_idx, float* out_score);

/* ---- search among listed rows: the exact top-k of an explicit row list -------- */
/* The exact fp32 top-k of the rows row_ids[0 .. n_ids) (host memory, the index's own row numbers) for each of nq host
 * queries [nq, dim]: what a selective `filter=` (vector_store.py:337-342 post-filters a top-k instead) or "rank these
 * candidates" costs when only the listed rows are read -- n_ids rows per block of queries, not the shard.  Blocking.
 *   Results: the format and order of wdbx_index_search -- (score descending, row ascending), L2 (distance ascending, row
 *   ascending) with positive squared distances; unused slots hold row -1 and score 0 (fewer than k listed rows, n_ids == 0).
 *   A row whose score is NaN (removed rows, rows with a NaN element) is never returned.
 *   Scores: exactly the arithmetic of the candidates' re-scoring on every other path (rescore_kernel), so a listed row's
 *   score is bit-identical to what wdbx_index_search, the masked calls and wdbx_index_range_search return for it.
 *   row_ids must be STRICTLY INCREASING and below the row count, checked under the handle's lock (a list built before a
 *   concurrent add stays valid: row numbers do not move); anything else is WDBX_E_INVALID, as are k outside
 *   [1, WDBX_MAX_K] and nq < 1.  n_ids may be 0 (every slot -1) and as large as the index.
 *   Every fetched row is scored against a block of queries (8 up to k = 64, 4 up to k = 128, else 1; a lone query is the
 *   block of one).  Routes (get_option "last_rows_path"): 1 = lists of at most option "rows_keys_max" rows (default 8192):
 *   a key per listed row and query, ranked by the merge kernel; 2 = per-workgroup top-k lists merged like the fp32 scan's;
 *   3 = k from option "select_min_k" on a longer list: a key per listed row, then the radix-select chain per query;
 *   0 = nothing launched (empty list).  The scoring launches count as scan launches in wdbx_index_profile_read.
 *   The call holds the handle's mutex to its end.  Nothing of a call's list stays valid in the handle. */
int wdbx_index_search_rows(wdbx_index* idx, const float* queries, int nq, int k, int normalize_queries,
                           const uint64_t* row_ids, uint64_t n_ids, int64_t* out_idx, float* out_score);

/* ---- distance matrix among listed rows: each listed row's nearest among the others ---- */
/* For every listed row row_ids[i] (host memory, the index's own row numbers) the exact fp32 top-k of the listed rows OTHER
 * THAN row_ids[i] itself: what clustering, a UMAP / t-SNE layout or a near-duplicate report reads from a sample of stored
 * vectors.  out_idx / out_score are host buffers [n_ids, k]; line i belongs to row_ids[i].  Blocking.
 *   The query of line i is the STORED row row_ids[i], as stored (cosine rows were normalised when they were added; nothing is
 *   normalised again), read on the device where it lies: no vector crosses the bus in either direction.
 *   Self is the same list position, which is the same row number; it is left out by position, not by score.  Another listed
 *   row holding an equal vector is a neighbour like any other.
 *   Results: format, order, -1 / 0 unused slots and NaN handling as wdbx_index_search_rows; a candidate whose score is NaN is
 *   never returned.  An anchor that was removed or holds a NaN has every slot -1.  With k >= n_ids a line has at most
 *   n_ids - 1 results.
 *   Scores: exact_score_block's arithmetic.  Line i is bit-identical, ids and score bits, to wdbx_index_search_rows called
 *   with the query wdbx_index_get_rows(row_ids[i]), normalize_queries = 0 and the list with entry i removed.  The answer is
 *   bit-identical from run to run and does not depend on how the anchors fall into rounds.
 *   WDBX_E_INVALID: a list that is not strictly increasing or reaches the row count (checked under the handle's lock by the
 *   pass wdbx_index_search_rows uses; the message names the entry), k outside [1, WDBX_MAX_K], a null buffer with n_ids > 0,
 *   more than 2^31 - 1 listed rows.  n_ids == 0 is WDBX_OK and launches nothing.  A refused call leaves the handle usable.
 *   Routes and anchor blocks are wdbx_index_search_rows' with the listed rows as its queries (get_option "last_matrix_path":
 *   0 = nothing launched, 1 = a key per (anchor, listed row) ranked by the merge kernel, 2 = per-workgroup top-k lists, 3 = keys
 *   and the radix-select chain per anchor; options "rows_keys_max" and "select_min_k" decide as they do there).  The anchors
 *   run in rounds of at most 256 consecutive list positions (get_option "last_matrix_rounds"), each one scoring launch --
 *   counted as a scan launch in wdbx_index_profile_read -- and one ranking launch (one per anchor on route 3) -- counted as
 *   merge launches; a round's scratch stays within 256 MiB.
 *   The call holds the handle's mutex to its end.  Nothing of the call's list stays valid in the handle. */
int wdbx_index_search_matrix(wdbx_index* idx, const uint64_t* row_ids, uint64_t n_ids, int k,
                             int64_t* out_idx /* [n_ids, k] */, float* out_score /* [n_ids, k] */);

/* ---- search among listed rows, one row list PER QUERY in one batched call ------ */
/* What wdbx_index_search_rows answers for one list, for a batch whose queries each name their own list (a rerank stage's
 * candidates, a selective filter per tenant): query i is ranked among the rows of list query_list[i].  The lists come back to
 * back in list_rows with list_offsets[l] .. list_offsets[l + 1] bounding list l.  Blocking, host buffers.
 *   Results in the caller's query order; format, order, -1 / 0 unused slots and NaN handling as wdbx_index_search_rows.
 *   Query i's ids and scores are bit-identical to wdbx_index_search_rows called with that query alone and its list.
 *   Several queries may name one list (they share every fetch of its rows, 8 queries at a time); a list may be empty (every
 *   slot of its queries -1); a list no query names is still checked.
 *   WDBX_E_INVALID: a list that is not strictly increasing or reaches the row count (checked under the handle's lock; the
 *   message names the list and the entry), list_offsets[0] != 0 or decreasing offsets, a query_list entry outside
 *   [0, n_lists) (there is no "-1 = every row": a whole-shard query is not a list), n_lists < 1, nq < 1, k outside
 *   [1, WDBX_MAX_K], a null buffer.  A refused call leaves the handle usable.
 *   Routes: the queries of lists of at most option "rows_keys_max" rows run in rounds of up to 256 queries, each round one
 *   scoring launch (one workgroup per chunk of 256 listed rows and block of queries; counted as a scan launch in
 *   wdbx_index_profile_read) and one merge launch; the queries of a longer list -- all of them with rows_keys_max = 0 -- go
 *   through wdbx_index_search_rows' own routes, list by list, under the lock the call already holds.  Exact either way.
 *   get_option: "last_lists_path" 0 = nothing launched, 1 = the batched pass only, 2 = both, 3 = list by list only;
 *   "last_lists_items" the work items of the call; "last_lists_rounds" its rounds.
 *   The call holds the handle's mutex to its end.  Nothing of a call's lists stays valid in the handle. */
int wdbx_index_search_row_lists(wdbx_index* idx, const float* queries, int nq, int k, int normalize_queries,
                                const uint64_t* list_rows,     /* every list back to back */
                                const uint64_t* list_offsets,  /* [n_lists + 1], list_offsets[0] == 0, non-decreasing */
                                int n_lists,
                                const int32_t* query_list,     /* [nq]: which list query i is ranked in */
                                int64_t* out_idx, float* out_score);

/* ---- distinct search: exact top-k with at most one row per label --------------- */
/* A label is any 32-bit value a caller attaches to a row (a document id for a corpus of chunks; Qdrant's search groups,
 * Elasticsearch's collapse and Milvus' grouping search answer the same question, the reference has nothing: it cuts a top-k
 * of rows, vector_store.py:323-345).  Labels need not be dense and the rows of one label need not be adjacent.  Rows added by
 * wdbx_index_add / wdbx_index_fill_synthetic start as WDBX_LABEL_NONE: each such row is a label of its own.
 * wdbx_index_set_rows leaves labels alone, wdbx_index_compact moves them with their rows, wdbx_index_clear drops them,
 * wdbx_index_reserve keeps them.  A range reaching past the row count is WDBX_E_INVALID (checked under the handle's lock).
 * The handle keeps the labels on the host and, built at the next distinct search after any label or row-count change, a
 * device-resident label order (every row sorted by (label, row), the dense label index of each position, the item tables of
 * the kernels); it counts in get_option "device_bytes_resident". */
#define WDBX_LABEL_NONE 0xFFFFFFFFu /* the row is a label of its own */
int wdbx_index_set_labels(wdbx_index* idx, uint64_t first_row, uint64_t n, const uint32_t* labels);
int wdbx_index_get_labels(wdbx_index* idx, uint64_t first_row, uint64_t n, uint32_t* out_labels);

/* For each of nq host queries [nq, dim]: take every live row the mask allows (mask_words NULL = every row; else
 * mask_word_count words, at least ceil(rows / 32)) whose score is not NaN, rank them by (score descending, row ascending) --
 * L2: (distance ascending, row ascending), positive squared distances --, keep the FIRST row of each label, cut at k.
 * Blocking, host buffers.  Unused slots hold row -1, score 0 and label WDBX_LABEL_NONE; out_label (may be NULL) receives each
 * slot's stored label.  A handle on which no label was ever set answers exactly as wdbx_index_search (or
 * wdbx_index_search_masked_n with a mask) does, bit for bit, whatever the options say (path 1).
 *   WDBX_E_INVALID: k outside [1, WDBX_MAX_K], nq < 1, a null query or result buffer, a mask shorter than ceil(rows / 32)
 *   words -- the conditions of wdbx_index_search_masked_n.  A refused call leaves the handle usable.
 *   Routes (get_option "last_distinct_path"): 0 = nothing launched (empty index, every slot -1); 1 = the over-fetch alone
 *   answered every query; 2 = the over-fetch, then the full pass for the queries that fell short; 3 = the full pass for all.
 *   Over-fetch (option "distinct_overfetch", default 4, 0 = never): the ordinary search -- the entry wdbx_index_search /
 *   _masked_n use -- for k' = min(rows, WDBX_MAX_K, distinct_overfetch * k), walked per query on the host keeping the first row
 *   of each label.  A query whose walk finds k labels, or whose k' reached every eligible row, is finished: exact, because
 *   any row outside the top-k' ranks below all of them.
 *   Full pass: waves walk spans of 64 positions of the label order, score each fetched row once against a block of up to 8
 *   queries and keep the best key per (query, label run inside the span); a second kernel takes the best key of each label
 *   and ranks the labels (per-workgroup top-k lists and the merge kernel below option "select_min_k", a key per label and
 *   the radix-select chain from it).  Every key has exactly one writer: answers are bit-identical from run to run.  Rounds of at
 *   most 256 queries keep their scratch within 256 MiB.  The scoring launches count as scan launches in
 *   wdbx_index_profile_read.
 *   Scores: a slot answered by the over-fetch (every slot on path 1; on path 2 the slots of the queries that did not fall
 *   short) carries the score wdbx_index_search returned for that row; a slot answered by the full pass (every slot on path 3;
 *   on path 2 the slots of the short queries) carries rescore_kernel's arithmetic, bit-identical to wdbx_index_search_rows
 *   and wdbx_index_range_search for the same row.  The rows are the same either way.
 *   get_option, read-only: "last_distinct_items" / "last_distinct_labels" the items and labels of the label order the call
 *   used (0 when it was not needed), "last_distinct_short" the queries the full pass served.
 *   The call holds the handle's mutex to its end. */
int wdbx_index_search_distinct(wdbx_index* idx, const float* queries, int nq, int k, int normalize_queries,
                               const uint32_t* mask_words, uint64_t mask_word_count, /* NULL = every row */
                               int64_t* out_idx, float* out_score, uint32_t* out_label /* may be NULL */);

/* ---- search groups: the k best labels, each with its best group_size rows ------- */
/* wdbx_index_search_distinct with a group size (Qdrant's search groups with group_size, Elasticsearch's collapse with
 * inner_hits, Milvus' grouping search with group_size; the reference has nothing): "ten documents, each with its three best
 * chunks".  Blocking, host buffers, both metrics.
 * Groups: the groups of query i, their order and out_label are what wdbx_index_search_distinct returns for the same queries, k,
 *   mask and options -- stage 1 runs the very steps of that call, so option "distinct_overfetch" and the read-only
 *   "last_distinct_*" options keep their meaning for it.  A WDBX_LABEL_NONE row is a group of its own; on a handle without labels
 *   every row is one.
 * Members: slot s of query i holds the first group_size eligible rows of that label -- eligible: live, allowed by the mask
 *   (mask_words NULL = every row; else mask_word_count words, at least ceil(rows / 32)), with a score that is not NaN -- ranked
 *   by (score descending, row ascending), L2 by (distance ascending, row ascending).  Every member's score is computed in
 *   rescore_kernel's arithmetic: bit-identical to what wdbx_index_search_rows and wdbx_index_range_search return for that row
 *   and query; -0 comes back as +0 and L2 scores are positive squared distances.  out_idx / out_score are
 *   [nq, k, group_size]; out_label (may be NULL) and out_count (may be NULL; the members found, 1 .. group_size) are [nq, k].
 *   Unused member slots hold -1 / 0; unused group slots hold -1 / 0 / WDBX_LABEL_NONE / count 0.  An empty index gives every
 *   slot -1 and launches nothing.
 *   With group_size = 1 out_idx[., ., 0] and out_label equal the distinct search's, with one exception: where two rows of one
 *   label score within an ulp of each other and the distinct search answered from its over-fetch (whose scan may sum in its
 *   own lane order), member 0 -- always the label's best row in rescore_kernel's arithmetic -- may be the other of the two.
 *   Answers are bit-identical from run to run (every key and every output word has one writer) and do not depend on option
 *   "groups_segment_rows" or on the rounds.
 * Stage 2: the rows of a label lie contiguous in the device-resident label order (above).  The host finds each winner's run,
 *   cuts it into tasks of at most "groups_segment_rows" positions (option, default 2048, range 4 .. 65536, anything else is
 *   WDBX_E_INVALID) -- an unlabelled winner is one direct row -- and per round (partial lists and task table within 256 MiB; a
 *   slot that passes it alone still runs) launches one scoring kernel (a workgroup per task, a register list of group_size keys
 *   per wave; counted as a scan launch in wdbx_index_profile_read) and one merge kernel (a wave per slot merges the slot's
 *   sorted lists and writes members, scores and count).  One download.
 *   get_option, read-only: "last_groups_path" 0 = nothing launched, 1 = ran; "last_groups_tasks"; "last_groups_rounds".
 *   WDBX_E_INVALID, the handle stays usable: nq < 1, k outside [1, WDBX_MAX_K], group_size outside
 *   [1, WDBX_MAX_GROUP_SIZE], a null query / out_idx / out_score, a mask shorter than ceil(rows / 32) words (checked under the
 *   handle's lock), 2^32 - 256 rows or more (the distinct search's condition).
 *   The call holds the handle's mutex to its end and leaves nothing valid in the handle. */
#define WDBX_MAX_GROUP_SIZE 64
int wdbx_index_search_groups(wdbx_index* idx, const float* queries, int nq, int k, int group_size, int normalize_queries,
                             const uint32_t* mask_words, uint64_t mask_word_count, /* NULL = every row */
                             int64_t* out_idx, float* out_score,                   /* [nq, k, group_size] */
                             uint32_t* out_label, int32_t* out_count /* [nq, k]; each may be NULL */);

/* Stage 2 alone, on the caller's slots (what a store of several shards needs: a label of the global top-k is in the top-k of
 * the shard that holds its best row, its other rows may lie on shards where it did not make the top-k).  slot_labels /
 * slot_rows are [nq, k]: slot_rows < 0 = the slot is unused (-1 / 0, count 0); slot_labels == WDBX_LABEL_NONE = the group is
 * the single row slot_rows (eligibility still applies); any other label = that label's rows on this handle, whatever
 * slot_rows (>= 0) says -- a label this handle does not hold gives count 0, not an error.  Members, scores, counts, options and
 * refusals as wdbx_index_search_groups; also WDBX_E_INVALID: a null slot_labels / slot_rows, a slot_rows at or past the row
 * count (checked under the lock). */
int wdbx_index_search_group_members(wdbx_index* idx, const float* queries, int nq, int k, int group_size, int normalize_queries,
                                    const uint32_t* mask_words, uint64_t mask_word_count, /* NULL = every row */
                                    const uint32_t* slot_labels, const int64_t* slot_rows, /* [nq, k] */
                                    int64_t* out_idx, float* out_score,                    /* [nq, k, group_size] */
                                    int32_t* out_count /* [nq, k]; may be NULL */);

/* ---- multi-vector search: labels ranked by the sum of per-vector best scores ---- */
/* Late interaction / MaxSim (ColBERT, Qdrant's multivector, Vespa; the reference has nothing): a document is stored as many
 * rows under one label (wdbx_index_set_labels), a query is itself several vectors, and
 *     score(query, label) = sum over the query's vectors t of ( best score of t among the label's rows ).
 * Query i's vectors are rows vector_offsets[i] .. vector_offsets[i + 1] - 1 of `vectors`.  Blocking, host buffers; the call
 * holds the handle's mutex to its end and nothing of it stays valid in the handle.
 *   Eligible row: a live row the mask allows (mask_words NULL = every row; else mask_word_count words, at least
 *   ceil(rows / 32)) whose score against vector t is not NaN -- the conditions of wdbx_index_search_distinct.
 *   Per-vector best m(t, L): the best score of t among label L's eligible rows (L2: the smallest squared distance): the score
 *   part of the maximum of the rows' (score, row) keys, exactly as the distinct search's full pass forms it.  A row's score
 *   here is bit-identical to wdbx_index_search_rows and wdbx_index_range_search for the same row and vector.
 *   Label score S(L): the fp32 left fold ((+0.0f + m(t0, L)) + m(t0 + 1, L)) + ... in the caller's vector order, plain adds
 *   in the ranking domain (L2 adds the negated distances; out_score is the positive sum of squared distances).
 *   Never returned: a label without an eligible row for SOME vector of the query, and a label whose sum is NaN (inf + -inf).
 *   A row labelled WDBX_LABEL_NONE is a label of its own; on a handle without any labels every row is one (the same path).
 *   Order: (S descending, position of the label in the label order ascending) -- L2: (sum ascending, same tie rule).  The
 *   label order is stored label value ascending, then the unlabelled rows by row number.  Total and deterministic: every key
 *   and every accumulator entry has one writer, answers are bit-identical from run to run.
 *   Outputs [nq, k]: out_idx the label's SMALLEST row number (unique per label; what names an unlabelled row), out_label
 *   (may be NULL) its stored label, out_score S.  Unused slots hold -1 / 0 / WDBX_LABEL_NONE.  An empty index: every slot
 *   -1, nothing launched.  normalize_queries normalises each vector on its own.
 *   WDBX_E_INVALID: nq < 1, k outside [1, WDBX_MAX_K], a null buffer, vector_offsets[0] != 0, a query with no vector or with
 *   more than WDBX_MAX_QUERY_VECTORS, a mask shorter than ceil(rows / 32) words (checked under the handle's lock).  A refused
 *   call leaves the handle usable.
 *   Rounds: the call's vectors are cut into rounds of consecutive vectors, at most option "multivector_round_vectors"
 *   (default 256, 1 .. 256; anything else is WDBX_E_INVALID) and at most what keeps a round's item keys and ranking scratch
 *   within 256 MiB (one vector per round when one vector's keys alone pass that).  A round may hold several queries and may
 *   cut a query in two: the one fp32 accumulator per label of the handle carries its fold into the next round (a dead label
 *   is NaN in it).  Per round: the distinct search's scoring kernel with the round's vectors as its queries (every fetched
 *   row scored once per block of 8 vectors; counted as scan launches in wdbx_index_profile_read), then one reduce-and-rank
 *   kernel (per-workgroup top-k lists and the merge kernel below option "select_min_k", a key per label and the radix-select
 *   chain from it).  The answer does not depend on the rounds.
 *   get_option, read-only: "last_multivector_rounds", "last_multivector_vectors", "last_multivector_labels" (0 after a call
 *   on an empty index). */
#define WDBX_MAX_QUERY_VECTORS 1024
int wdbx_index_search_multivector(wdbx_index* idx,
                                  const float* vectors,           /* [vector_offsets[nq], dim]: the queries' vectors back to back */
                                  const uint64_t* vector_offsets, /* [nq + 1], [0] == 0, strictly increasing */
                                  int nq, int k, int normalize_queries,
                                  const uint32_t* mask_words, uint64_t mask_word_count, /* NULL = every row */
                                  int64_t* out_idx, float* out_score, uint32_t* out_label /* [nq, k]; out_label may be NULL */);

/* ---- MMR search: a diversified top-k picked from the pool of the best rows ------ */
/* Maximal marginal relevance (LangChain's max_marginal_relevance_search on every vector store; Qdrant, Milvus, Weaviate and
 * Vespa ship it or a rerank stage for it; the reference has nothing: it cuts a top-k of rows, vector_store.py:323-345, and a
 * distinct search only removes rows of one label): each of nq host queries [nq, dim] gets k rows picked greedily from its
 * fetch_k best, every pick trading relevance against similarity to the rows already picked.  Blocking, host buffers; the
 * call holds the handle's mutex to its end and nothing of it stays valid in the handle.  Both metrics.
 *   Pool: query i's candidates are the exact top-fetch_k of the rows the mask allows (mask_words NULL = every row; else
 *   mask_word_count words, at least ceil(rows / 32)): the answer of wdbx_index_search / wdbx_index_search_masked_n for
 *   k' = fetch_k, reached through the internal entry those calls (and the distinct search's over-fetch) use.  Position
 *   0 .. m - 1 is that ranking; rel_i is the returned score in the ranking domain (L2: the negated squared distance); m may be
 *   below fetch_k (few eligible rows, -1 slots).  A NaN-scored row is never a candidate, as everywhere else.
 *   Similarity: G[i][j] is the score of candidate row i with candidate row j's STORED row as the query, in exact_score's
 *   arithmetic (lane order, fma chain, fold and xor tree as every exact score of this library), in the ranking domain.  So
 *   G[i][j] is bit-identical to what wdbx_index_search_rows returns for row i with wdbx_index_get_rows(row j) as the query
 *   (L2: negated), and G[i][j] == G[j][i] bit for bit: the products commute and the order of summation depends on the element
 *   index only.  (A NaN similarity is NaN both ways; its sign and payload are not specified, and the selection ignores it.)
 *   Selection: greedy, in fp32, no contraction -- every (x) and (-) below is ONE correctly rounded fp32 operation, never an
 *   fma.  Pick 0 is position 0, its value lambda (x) rel_0.  Every candidate starts with maxsim_i = -inf; after each pick p,
 *   maxsim_i = fmaxf(maxsim_i, G[p][i]), a NaN similarity ignored.  The next pick is the unpicked candidate with the largest
 *       v_i = (lambda (x) rel_i) (-) ((1.0f (-) lambda) (x) maxsim_i);
 *   ties (-0 and +0 are one value) go to the smaller position; a NaN v_i ranks below every non-NaN value, NaN values among
 *   themselves by position.  Selection stops after min(k, m) picks.
 *   Outputs [nq, k], in pick order: out_idx the row, out_score the row's relevance exactly as wdbx_index_search returned it
 *   (L2: the positive squared distance), out_mmr (may be NULL) the value the pick won with.  Unused slots hold -1 / 0 / 0.  An
 *   empty index: every slot -1, nothing launched.
 *   Consequences: with lambda == 1.0f on finite rows the answer equals the first k columns of wdbx_index_search(.., fetch_k),
 *   ids and score bits.  Answers are bit-identical from run to run: every word of G, every maxsim and every output slot has
 *   one writer.
 *   WDBX_E_INVALID: nq < 1, k outside [1, WDBX_MAX_K], fetch_k outside [k, WDBX_MAX_K], lambda NaN or outside [0, 1], a null
 *   query or result buffer, a mask shorter than ceil(rows / 32) words (checked under the handle's lock).  A refused call leaves
 *   the handle usable.
 *   Rounds: the pool's row numbers come back to the host with the pool (as the distinct search's over-fetch hands them to its
 *   host walk) and go up again as the gather's list.  A round holds as many consecutive queries as keep their gathered rows
 *   ([sum m, row pitch]) and similarity squares (m x m floats each) within option "mmr_scratch_mib" MiB (default and largest
 *   256, smallest 1; anything else is WDBX_E_INVALID); a query that passes it alone is a round of its own.  Per round: the
 *   gather, one launch of the pairs kernel (one wave per candidate row, scored against blocks of 8 candidate columns), one
 *   launch of the selection kernel (one workgroup per query).  The answer does not depend on the rounds.
 *   get_option, read-only: "last_mmr_path" 0 nothing launched, 1 ran; "last_mmr_rounds" the rounds of the last call;
 *   "last_mmr_candidates" the sum of m over the call's queries. */
int wdbx_index_search_mmr(wdbx_index* idx, const float* queries, int nq, int k, int fetch_k, float lambda,
                          int normalize_queries,
                          const uint32_t* mask_words, uint64_t mask_word_count, /* NULL = every row */
                          int64_t* out_idx, float* out_score, float* out_mmr /* [nq, k]; out_mmr may be NULL */);

/* ---- recommend search: rank rows by positive and negative examples ("more like these, less like those") ---------------
 * Each of nq queries is a set of example vectors, positives and negatives; every eligible row is scored against all of them
 * in one pass over the corpus and ranked by the fold below.  Blocking, host buffers; the call holds the handle's mutex to
 * its end and nothing of it stays valid in the handle.  Both metrics.
 *   Examples: examples is [example_offsets[2 * nq], dim], back to back; example_offsets is [2 * nq + 1], [0] == 0,
 *   non-decreasing: query i's positives are [off[2i], off[2i + 1]), its negatives [off[2i + 1], off[2i + 2]).  At least one
 *   positive and at most WDBX_MAX_EXAMPLES examples per query.  normalize_examples as normalize_queries elsewhere.
 *   Scores and eligibility: r(row, e) is the score of row with example e as the query, in the ranking domain (L2: the
 *   negated squared distance), in exact_score's arithmetic (lane order, fma chain, fold and xor tree as every exact score of
 *   this library): bit-identical to what wdbx_index_search_rows and wdbx_index_range_search return for that row and that
 *   vector.  An eligible row is a live row that the mask allows (mask_words NULL = every row; else mask_word_count words, at
 *   least ceil(rows / 32)) and that is not in exclude_rows (strictly increasing row numbers, at most WDBX_MAX_EXCLUDE_ROWS;
 *   NULL / 0 = none).  A row with a NaN r for any example of the query is never returned.
 *   The fold: p = max r over the query's positives, n = max r over its negatives, or -inf when there are none.  A row is
 *   FAVOURED when p > n; otherwise, ties included, it is DISFAVOURED.
 *   Order: every favoured row ranks before every disfavoured row.  Favoured rows by (p descending, row ascending);
 *   disfavoured rows by (n ascending, row ascending) -- the row farthest from its nearest negative first; the key value is
 *   (-n) + 0.0f.  This is the order of Qdrant's current best_score strategy without its sigmoid, which is monotone and in fp32
 *   would only create ties.  Each query's answer is cut at k.
 *   Outputs [nq, k]: out_idx the row; out_score the value the row was ranked by in the caller's units -- p for favoured, n
 *   for disfavoured (L2: the positive squared distance to the nearest positive or negative; -0 comes back as +0, as
 *   everywhere); out_side (may be NULL) 1 for favoured, 0 for disfavoured.  Unused slots hold -1 / 0 / 0.  An empty index:
 *   every slot -1, nothing launched.
 *   Consequences: one positive and no negatives gives ids and score bits equal to the exact top-k of that vector in
 *   exact_score's arithmetic, i.e. to the head of wdbx_index_range_search or to wdbx_index_search_rows over every row
 *   (wdbx_index_search may sum a row in its scan's own lane order: the same ids unless two scores lie within an ulp, but not
 *   necessarily the same score bits).  A negative equal to a positive makes every row disfavoured.  Answers are bit-identical from run to run: every list slot and every
 *   key has one writer.  The answer does not depend on how the examples are cut into blocks (a maximum), nor on the rounds.
 *   WDBX_E_INVALID: nq < 1, k outside [1, WDBX_MAX_K], a null buffer, a query with no positive example or with more than
 *   WDBX_MAX_EXAMPLES examples, offsets that decrease or example_offsets[0] != 0, a mask shorter than ceil(rows / 32) words,
 *   exclude_rows that is not strictly increasing, reaches the row count or is longer than WDBX_MAX_EXCLUDE_ROWS (the mask and
 *   exclude_rows are checked under the handle's lock).  A refused call leaves the handle usable.
 *   Passes: the 64-bit key has no spare bit for the side, so there are two: the favoured pass for all queries (favoured rows
 *   emit make_key(p + 0.0f, row), all others 0), then the disfavoured pass for the queries that came back short of k only
 *   (disfavoured rows emit make_key((-n) + 0.0f, row)); the host splices the two lists.  Each pass fetches every row once per
 *   query (one wave per row, examples in blocks of up to 8) and ranks as the listed-row paths do: per-workgroup lists merged
 *   by the merge kernel, or from select_min_k on a key per row and the radix-select chain, in rounds whose keys stay within
 *   256 MiB.  The exclusion list lives on the device at its own size.  The scoring launches count as scan launches in
 *   wdbx_index_profile_read.
 *   get_option, read-only: "last_recommend_path" 0 nothing launched, 1 favoured pass only, 2 both passes;
 *   "last_recommend_short" the queries the second pass served. */
#define WDBX_MAX_EXAMPLES 64        /* positives + negatives of one query */
#define WDBX_MAX_EXCLUDE_ROWS 1024
int wdbx_index_search_recommend(wdbx_index* idx,
                                const float* examples,           /* [example_offsets[2 * nq], dim], back to back */
                                const uint64_t* example_offsets, /* [2 * nq + 1] */
                                int nq, int k, int normalize_examples,
                                const uint32_t* mask_words, uint64_t mask_word_count, /* NULL = every row */
                                const uint64_t* exclude_rows, uint64_t n_exclude,     /* strictly increasing; may be NULL / 0 */
                                int64_t* out_idx, float* out_score, uint8_t* out_side /* [nq, k]; out_side may be NULL */);

/* ---- discovery search: rank rows by context pairs and a target ---------------------------------------------------------
 * Each of nq queries is a list of context PAIRS (positive, negative) and, when targets is not NULL, a target vector.  A pair
 * splits the space into the side nearer its positive and the side nearer its negative.  Every eligible row is scored against
 * all of a query's vectors in one pass over the corpus and ranked by the per-pair fold below.  Blocking, host buffers; the
 * call holds the handle's mutex to its end and nothing of it stays valid in the handle.  Both metrics.
 *   Vectors: targets is [nq, dim], or NULL = context search for every query.  context is [2 * pair_offsets[nq], dim]: pair i
 *   is vectors 2i (positive) and 2i + 1 (negative).  pair_offsets is [nq + 1], [0] == 0, non-decreasing: query q's pairs are
 *   [off[q], off[q + 1]).  normalize_vectors as normalize_queries elsewhere, for the targets and the context alike.
 *   Scores and eligibility: r(row, v) is the score of row with vector v as the query, in the ranking domain (L2: the negated
 *   squared distance), in exact_score's arithmetic: bit-identical to what wdbx_index_search_rows and
 *   wdbx_index_range_search return for that row and that vector.  Eligible rows, the mask and exclude_rows are exactly those
 *   of wdbx_index_search_recommend.  A row is never returned if any r for it is NaN, or if any r(p_i) - r(n_i) is NaN
 *   (inf - inf).
 *   Target mode (targets != NULL): 0 to WDBX_MAX_CONTEXT_PAIRS pairs per query.  wins = #{i : r(p_i) > r(n_i)}; a tie is not
 *   a win.  t = r(target) + 0.0f.  Order: (wins descending, t descending, row ascending), cut at k.  out_score is t in the
 *   caller's units (L2: the positive squared distance), out_wins the row's wins.  With zero pairs the ids and score bits
 *   equal wdbx_index_search_recommend with one positive and no negative.
 *   Context mode (targets == NULL): every query needs at least one pair.  loss = sum over i of fminf(r(p_i) - r(n_i), 0.0f),
 *   accumulated in fp32 from 0.0f in pair order (no multiply: nothing to contract).  Order: (loss + 0.0f descending, row
 *   ascending): rows on the right side of every pair all have loss 0 and come out in row order.  out_score is the loss as
 *   computed: <= 0, in the ranking domain, no unit conversion for either metric.  out_wins slots are 0.
 *   Outputs [nq, k]; out_wins may be NULL.  Unused slots hold -1 / 0 / 0.  An empty index: every slot -1, nothing launched.
 *   Answers are bit-identical from run to run and do not depend on how the vectors are cut into blocks (the loss terms are
 *   added in pair order whatever the cut, and a pair never straddles a block) nor on the rounds: every record, list slot and
 *   key has one writer, and the only atomics add integers.
 *   WDBX_E_INVALID: nq < 1, k outside [1, WDBX_MAX_K], a null buffer (context may be NULL only when the call has no pair at
 *   all), pair_offsets[0] != 0 or decreasing offsets, more than WDBX_MAX_CONTEXT_PAIRS pairs in a query, a context-mode query
 *   with no pair, and recommend's mask and exclusion errors (checked under the handle's lock).  A refused call leaves the
 *   handle usable.
 *   Stages: a query's vectors are staged as [target?, p0, n0, p1, n1, ...] and go through exact_score_block in blocks of 8,
 *   4 and 2 (the target: a block of one), one wave per row.  Context mode ranks in the pass itself, as recommend does
 *   (per-workgroup lists and the merge kernel, or from select_min_k on a key per row and the radix-select chain), with
 *   make_key(loss + 0.0f, row).  Target mode needs two levels and the 64-bit key has no spare bit, so the pass -- ONE read of
 *   the corpus per query, however many wins values the answer spans -- writes a record per row, make_key(t, row) (0 when the
 *   row is ineligible or NaN) and the wins byte, and counts the rows per wins value ("zone").  The host downloads the counts,
 *   picks per query the zones from the top down that cover k, and a second kernel ranks each (query, zone) slot from the 9
 *   bytes per row of the records with the same list or select modes; the host splices the zones' lists.  Rounds keep the
 *   records, keys or lists within 256 MiB.  The scoring launches count as scan launches in wdbx_index_profile_read, the zone
 *   launches as merge launches.
 *   get_option, read-only: "last_discover_path" 0 nothing launched, 1 context mode, 2 target mode;
 *   "last_discover_zone_slots" the (query, zone) slots the second stage ranked. */
#define WDBX_MAX_CONTEXT_PAIRS 32
int wdbx_index_search_discover(wdbx_index* idx,
                               const float* targets,           /* [nq, dim], or NULL = context search for every query */
                               const float* context,           /* [2 * pair_offsets[nq], dim]: pair i is vectors 2i (positive), 2i + 1 (negative) */
                               const uint64_t* pair_offsets,   /* [nq + 1], [0] == 0, non-decreasing: query q's pairs are [off[q], off[q + 1]) */
                               int nq, int k, int normalize_vectors,
                               const uint32_t* mask_words, uint64_t mask_word_count, /* NULL = every row */
                               const uint64_t* exclude_rows, uint64_t n_exclude,     /* strictly increasing; may be NULL / 0 */
                               int64_t* out_idx, float* out_score, uint8_t* out_wins /* [nq, k]; out_wins may be NULL */);

/* ---- range search: every row within a similarity, no k ----------------------- */
/* every row whose score reaches thresholds[q] (cosine/IP: score >= t; L2: squared distance <= t), exact fp32,
 * per query sorted like wdbx_index_search; replaces faiss' IndexFlat range_search, which the reference never reaches
 * (it only post-filters a top-k, vector_store.py:337-342).  out_offsets[nq + 1] always receives the true counts
 * (CSR: query i's results are [out_offsets[i], out_offsets[i+1])).  out_rows / out_scores hold the results only when
 * out_offsets[nq] <= capacity (otherwise the call still returns WDBX_OK, their first `capacity` slots may have been used as
 * scratch, and the caller retries with capacity = out_offsets[nq]; capacity 0 = count only).  mask_words may be NULL (then
 * mask_word_count is ignored); a mask is checked against the row count under the handle's lock, as in
 * wdbx_index_search_masked_n.
 *   Result set: the live rows (passing the mask) whose fp32 score reaches the threshold; a NaN score never does (removed
 *   rows, rows with a NaN element).  A NaN threshold is WDBX_E_INVALID; +-inf are allowed (-inf on cosine: every non-NaN row).
 *   Scores: computed with exactly the arithmetic of the candidates' re-scoring on the top-k paths, whichever path selects
 *   the rows -- bit-identical to what wdbx_index_search returns for the same rows where that takes the u8 selection scan.
 *   L2 scores are the positive squared distances.
 *   Order: (score descending, row ascending) for cosine, (distance ascending, row ascending) for L2.
 *   Paths: from option "range_min_rows" (131 072) rows, with scan_shadow = 2 and a row shape the u8 selection scan serves,
 *   a selection scan over the u8 shadow keeps every row whose quantisation upper bound reaches the threshold and the kept
 *   rows are scored exactly; otherwise every row is scored exactly in fp32 (get_option "last_range_path": 2 / 0).
 *   The call holds the handle's mutex to its end.  Nothing of a call's results stays in the handle. */
int wdbx_index_range_search(wdbx_index* idx, const float* queries, int nq, const float* thresholds,
                            int normalize_queries, const uint32_t* mask_words, uint64_t mask_word_count,
                            uint64_t capacity, uint64_t* out_offsets, int64_t* out_rows, float* out_scores);

/* ---- batched range search: one int8 tile pass per block of queries ------------ */
/* wdbx_index_range_search for a BATCH of queries (near-duplicate detection, threshold retrieval for a page of items, cluster
 * assignment): the same arguments, the same contract, word for word -- CSR offsets always true, the capacity retry rule,
 * count-only with capacity 0, result set, order, NaN handling, +-inf thresholds, refusals, the handle's mutex held to the end.
 * For every query the rows, their order and the bits of every score equal what wdbx_index_range_search returns for that
 * query alone.
 *   Route (get_option "last_range_batch_path": 0 = nothing launched, an empty index; 1 = the per-query path only; 2 = tiles
 *   only; 3 = tiles, with some blocks answered per query).  The tile route is taken when the int8 tiles would serve a batch
 *   (gemm_bf16 = 3, gemm8_variant = 0, an i8 row image of at most 1536 bytes, the shadow copy fits; with a mask also
 *   gemm_masked), the row count passes the batched path's own row test (gemm_min_rows / gemm_min_work, as for top-k) and nq is
 *   at least option "range_batch_min_queries" (default 4).  Otherwise the call runs wdbx_index_range_search's rounds
 *   unchanged, under the same lock.
 *   Tile route: blocks of up to 256 consecutive queries (128 for L2 and rows beyond 384 bytes of i8, 64 beyond 768).  Per
 *   block the queries are quantised, their selection thresholds and a bound widened by the exact pass's own rounding are
 *   set, ONE full pass of the int8 tile kernel keeps every (query, row) pair whose rigorous upper bound reaches the query's
 *   threshold (with a mask: the masked instances, the mask's rows removed before pairs are appended), the pairs are sorted by
 *   query and the exact pass of wdbx_index_range_search scores and filters them.  The tile launches count as gemm launches in
 *   wdbx_index_profile_read_gemm.  No sample, no second selection stage.
 *   Two overflows, both exact: a query's candidates past their buffer grow it to the exact count and the gather runs again,
 *   once (a count that changes between the two runs is WDBX_E_STATE); a wave of the tile pass that ran out of pair room sends
 *   every query of ITS block through the per-query path ("last_range_batch_fallback_queries" counts them; a -inf cosine
 *   threshold in a batch ends here by design).  Option "range_pair_cap": pairs per wave, 0 = the default sizing (16 384),
 *   else 64 .. 65 536 (anything else is WDBX_E_INVALID).
 *   get_option, read-only: "last_range_batch_blocks" the blocks of the last call, "last_range_batch_pairs" the pairs its tile
 *   passes kept. */
int wdbx_index_range_search_batch(wdbx_index* idx, const float* queries, int nq, const float* thresholds,
                                  int normalize_queries, const uint32_t* mask_words, uint64_t mask_word_count,
                                  uint64_t capacity, uint64_t* out_offsets, int64_t* out_rows, float* out_scores);

/* ---- device-resident path (inputs already in HBM; asynchronous) -------------- */
int wdbx_device_alloc(wdbx_index* idx, uint64_t bytes, void** out_dev_ptr);
int wdbx_device_free(wdbx_index* idx, void* dev_ptr);
int wdbx_device_upload(wdbx_index* idx, void* dev_dst, const void* host_src, uint64_t bytes);   /* blocking */
int wdbx_device_download(wdbx_index* idx, void* host_dst, const void* dev_src, uint64_t bytes); /* blocking */
/* fill a device query buffer [nq, row_pitch] with synthetic (optionally normalised) queries */
int wdbx_device_fill_synthetic(wdbx_index* idx, float* dev_dst, uint64_t seed, uint64_t counter_row0,
                               uint64_t n, int normalize);
/* enqueue nq single-query scans on the handle's stream and return at once.
 * d_queries is [nq, row_pitch] (zero padded beyond dim), d_out_idx [nq,k], d_out_score [nq,k]. */
int wdbx_index_search_device(wdbx_index* idx, const float* d_queries, int nq, int k,
                             int64_t* d_out_idx, float* d_out_score);
int wdbx_index_synchronize(wdbx_index* idx);

/* ---- batched queries (extension: the reference is single-query; BASELINE config 4) -- */
/* nq queries share ONE pass over the corpus, in blocks of up to 256 queries: a matrix-core pass computes
 * rows . queries^T tile by tile with a fused threshold filter, then a per-query top-k of the survivors.
 * Results are the exact fp32 ranking in every mode.  Tile family, option "gemm_bf16" (read back what the last batch
 * ran on with get_option("last_gemm_family")):
 *   3 (default) int8 tiles (v_mfma_i32_16x16x64_i8) over a GROUP-SCALED i8 SHADOW COPY of the rows (one scale per 64
 *               rows, stored in MFMA fragment order; +25 % device memory, built and refreshed lazily), only to SELECT
 *               candidates under a rigorous per-(group, query) quantisation bound; every candidate is re-scored in
 *               fp32 from the fp32 rows.  Cosine / inner product and (since round 3) L2, rows whose i8 image is at
 *               most 1536 bytes; other shapes and a shadow that does not fit fall to 2.
 *   2           bf16 tiles (v_mfma_f32_32x32x16_bf16) over a bf16 shadow copy (+50 % device memory), selection only,
 *               rigorous rounding-error margin, fp32 re-scoring.  Falls back to 1 when the shadow does not fit.
 *   1           the same bf16 selection reading the fp32 rows (no extra memory, twice the bytes per pass)
 *   0           exact fp32 MFMA tiles (v_mfma_f32_32x32x2_f32), no re-scoring for cosine
 * L2 selects by 2 c.q - |c|^2 on the pass and re-scores with the direct form.  wdbx_index_search() takes
 * this path by itself for nq >= 4 (2 on shards of 3 M rows and more) on corpora >= 65536 rows.  Asynchronous like
 * wdbx_index_search_device. */
int wdbx_index_search_batch_device(wdbx_index* idx, const float* d_queries, int nq, int k,
                                   int64_t* d_out_idx, float* d_out_score);
/* The same with a row mask from the HOST (uint32 words, bit r % 32 of word r / 32 = row r may be returned;
 * mask_word_count >= ceil(rows / 32) or WDBX_E_INVALID): the filter push-down of wdbx_index_search_masked for a whole
 * batch.  When the int8 tiles are what would run (gemm_bf16 = 3, gemm8_variant = 0, k below the select range; option
 * gemm_masked, default 1) the batch is ONE masked pass: the mask becomes the call's bad-row table, masked-out rows neither
 * vouch for the sampled threshold nor enter the candidate lists, and the sample grows with 1 / (allowed fraction)
 * (get_option "last_batch_masked" == 1, "last_batch_allowed_rows").  Otherwise the queries take the masked per-query
 * paths.  Exact either way.  The mask is copied before the call returns and applies to this call only.
 * wdbx_index_batch_status describes this call when it ran the masked pass (last_batch_masked == 1); after the per-query
 * fall-back it describes that path's last round of queries, as after wdbx_index_search_device.
 * wdbx_index_search_masked / _masked_n and the group's masked calls take the same pass from gemm_min_queries queries on. */
int wdbx_index_search_batch_masked_device(wdbx_index* idx, const float* d_queries, int nq, int k,
                                          const uint32_t* mask_words, uint64_t mask_word_count,
                                          int64_t* d_out_idx, float* d_out_score);
/* synchronises; per query the number of candidates the filter kept (out_counts[nq], may be null),
 * the buffer capacity, and how many queries exceeded it.  Since round 3 such queries are re-run exactly ON THE DEVICE by
 * conditional launches queued behind their block (get_option "last_batch_repaired" == 1; option "batch_repair"): the
 * results are exact either way and the count only tells how many needed it.  Shapes without a device-side repair (k in
 * the radix-select range) leave it to the caller as before (wdbx_index_search() does it by itself). */
int wdbx_index_batch_status(wdbx_index* idx, uint32_t* out_counts, int nq, uint32_t* out_capacity,
                            int* out_overflowed);
int wdbx_index_profile_read_gemm(wdbx_index* idx, uint64_t* launches, double* ms_total);
/* the sample launches of the single-query selection scan (one launch per round of up to 32 queries) */
int wdbx_index_profile_read_sample(wdbx_index* idx, uint64_t* launches, double* ms_total);

/* ---- shards across GPUs: one process per GPU, RCCL over xGMI ----------------- */
#define WDBX_UNIQUE_ID_BYTES 128
int wdbx_comm_unique_id(void* out_128_bytes); /* rank 0 creates, the host side distributes */
/* join the shard group; global_row_base = number of rows held by lower ranks
 * (contiguous row ranges, so the merged order equals the single-shard order). */
int wdbx_index_comm_init(wdbx_index* idx, int nranks, int rank, const void* unique_id_128_bytes,
                         uint64_t global_row_base);
int wdbx_index_comm_destroy(wdbx_index* idx);
/* what RCCL reports for the handle's communicator (ncclCommCount / ncclCommUserRank; 0 / -1 without one) and the
 * handle's global row base -- evidence for a scaling run that the exchange really spans N ranks */
int wdbx_index_comm_info(wdbx_index* idx, int* out_nranks, int* out_rank, uint64_t* out_row_base);
/* re-base this rank's rows (after the shard was cleared and refilled with another row range) without tearing the
 * communicator down */
int wdbx_index_comm_set_row_base(wdbx_index* idx, uint64_t global_row_base);
/* as wdbx_index_search_device, but every rank scans its own shard, the per-shard
 * (row, score) records are all-gathered with RCCL and merged on every rank:
 * identical global results on all ranks; rows are global row numbers. */
int wdbx_index_search_sharded_device(wdbx_index* idx, const float* d_queries, int nq, int k,
                                     int64_t* d_out_idx, float* d_out_score);
/* the same exchange around the batched MFMA path (every rank must call it with the same nq, k; every
 * rank's shard must be eligible: cosine, >= 65536 rows).  wdbx_index_batch_status reports this rank's
 * candidate overflow as for the unsharded call. */
int wdbx_index_search_sharded_batch_device(wdbx_index* idx, const float* d_queries, int nq, int k,
                                           int64_t* d_out_idx, float* d_out_score);
/* host-level all-gather of `bytes` bytes per rank through the handle's communicator (recv: nranks * bytes, rank order):
 * the launcher-side plumbing of a multi-process run without any other transport -- barrier, max-reduction of a time,
 * result cross-checks.  Blocking. */
int wdbx_index_comm_allgather_host(wdbx_index* idx, const void* send, void* recv, uint64_t bytes);

/* ---- shards across GPUs in ONE process (the reference's VectorStore(num_shards=S) shape,
 *      vector_store.py:111-134, :323-345): S flat indices, contiguous row ranges (global row r lives in shard
 *      r / cap_per_shard).  Every shard's launches are enqueued by the shard's own persistent host thread; the per-shard
 *      (row, score) key lists are exchanged with ONE ncclAllGather per shard (communicators from ncclCommInitAll) and
 *      merged on the first shard's device.  Shards that share a device cannot be RCCL ranks: such a group exchanges
 *      by device-to-device copies instead (same results; wdbx_group_info reports 0 RCCL ranks). ---- */
typedef struct wdbx_group wdbx_group;
int wdbx_group_create(const int* device_ids, int n, int dim, int metric, uint64_t cap_per_shard, wdbx_group** out);
void wdbx_group_destroy(wdbx_group* grp);
/* append rows: they fill shard 0 up to cap_per_shard, then shard 1, ... ; *first_row_out = global row */
int wdbx_group_add(wdbx_group* grp, const float* rows, uint64_t n, int normalize, uint64_t* first_row_out);
int wdbx_group_size(wdbx_group* grp, uint64_t* out_rows);
/* blocking: every shard scans its rows, per-shard (row, score) key lists are exchanged and merged on the first
 * shard's device; out_idx holds global rows.  Identical to a single-shard search. */
int wdbx_group_search(wdbx_group* grp, const float* queries, int nq, int k, int normalize_queries,
                      int64_t* out_idx, float* out_score);
/* The same fan-out over EXISTING shard handles -- the reference's VectorStore keeps one index object per shard
 * (vector_store.py:111-134) and loops over them (:323-327): the handles stay owned by the caller and keep growing
 * through wdbx_index_add; the group only adds the exchange.  In merged results shard s owns the row numbers
 * [s * stride, (s + 1) * stride), stride = (2^32 - 256) / n (wdbx_group_info): row = stride * shard + local row, and ties
 * come back in shard order = the order of the reference's stable sort (:330); wdbx_group_set_row_bases replaces that
 * numbering.  wdbx_group_add is not valid on such a group; wdbx_group_destroy leaves the handles alive.  While a group
 * call enqueues it holds every shard's handle mutex, and it works on buffers of its own, so the shards' own callers
 * (wdbx_index_search on the same handles from other threads) can run concurrently with it.
 * exchange_mode: 0 = RCCL when every shard has its own device and the communicators come up, device copies otherwise
 * (also: environment WDBX_GROUP_EXCHANGE=rccl|copy); 1 = RCCL or fail; 2 = device copies. */
int wdbx_group_attach(wdbx_index* const* shards, int n, wdbx_group** out);
int wdbx_group_attach_ex(wdbx_index* const* shards, int n, int exchange_mode, wdbx_group** out);
/* *out_rccl_nranks: what ncclCommCount says about the group's communicator; 0 = the group exchanges by device copies */
int wdbx_group_info(wdbx_group* grp, int* out_shards, int* out_rccl_nranks, uint64_t* out_row_stride);
/* counters of the group: "exchanges" = exchange (all-gather / device copies) + merge steps enqueued so far -- a call is cut
 * into chunks and each chunk has ONE, so a caller can say how many a timed region held; "dispatches" = jobs handed to the
 * shards' threads; "unusable" = 1 after a failed collective made the group abort its communicators */
int wdbx_group_stat(wdbx_group* grp, const char* name, int64_t* value);
/* global row number of each shard's first row (a caller that placed contiguous row ranges itself) */
int wdbx_group_set_row_bases(wdbx_group* grp, const uint64_t* bases, int n);
/* every shard's top-k, exchanged and merged into the k_out best of their union, k <= k_out <= min(shards * k,
 * WDBX_MAX_K); out_idx / out_score are [nq, k_out].  k_out = shards * k is the whole candidate list the reference sorts
 * before its threshold / metadata post-filter / cut (vector_store.py:329-345), so a post-filtered query sees exactly
 * the candidates the reference would.  Blocking. */
int wdbx_group_search_merged(wdbx_group* grp, const float* queries, int nq, int k, int k_out, int normalize_queries,
                             int64_t* out_idx, float* out_score);
/* the same with a row filter per shard (metadata push-down, SURVEY 8f row 2, through the group): mask_words[s] = shard s's
 * mask as in wdbx_index_search_masked (ceil(rows of that shard / 32) uint32 words, host memory), or null = every row */
int wdbx_group_search_merged_masked(wdbx_group* grp, const float* queries, int nq, int k, int k_out, int normalize_queries,
                                    const uint32_t* const* mask_words, int64_t* out_idx, float* out_score);
/* the same, with mask_word_counts[s] = words held by mask_words[s] (ignored for a null mask): a short mask is refused under
 * the group's locks (vector_store.py:337-342 filters a list that cannot change under it; a pushed-down mask can go stale) */
int wdbx_group_search_merged_masked_n(wdbx_group* grp, const float* queries, int nq, int k, int k_out, int normalize_queries,
                                      const uint32_t* const* mask_words, const uint64_t* mask_word_counts, int64_t* out_idx,
                                      float* out_score);
/* (wdbx_group_search_merged answers a call that carries enough queries -- 4 on shards of >= 65536 rows -- with ONE batched
 * matrix-core pass per shard, as wdbx_index_search does; the resident form below makes one scan per query on every shard,
 * as wdbx_index_search_device does.)
 * device-resident form (inputs already in HBM; asynchronous): queries are placed once in the group's query buffer on
 * EVERY shard's device (from the host, or generated there like wdbx_device_fill_synthetic); search_resident enqueues the
 * search of queries [first_query, first_query + nq) on all shards + exchange + merge and returns; the results [nq, k_out]
 * of the most recent search stay on the first shard's device until wdbx_group_results copies them out. */
int wdbx_group_queries_upload(wdbx_group* grp, const float* queries, int nq, int normalize_queries);
int wdbx_group_queries_synthetic(wdbx_group* grp, uint64_t seed, uint64_t counter_row0, int nq, int normalize);
int wdbx_group_search_resident(wdbx_group* grp, int first_query, int nq, int k, int k_out);
int wdbx_group_synchronize(wdbx_group* grp);
int wdbx_group_results(wdbx_group* grp, int nq, int k_out, int64_t* out_idx, float* out_score);

/* ---- measurement ------------------------------------------------------------- */
/* enable!=0: bracket every scan-kernel launch with HIP events on the handle's stream */
int wdbx_index_profile(wdbx_index* idx, int enable);
/* synchronises, then reports and resets: number of scan launches measured and their
 * summed duration (ms); likewise for the merge kernels. */
int wdbx_index_profile_read(wdbx_index* idx, uint64_t* scan_launches, double* scan_ms_total,
                            uint64_t* merge_launches, double* merge_ms_total);
/* measurement aid: time `reps` plain streaming reads of the stored rows (16 B per lane, no
 * arithmetic, no top-k) -- the read ceiling on this device that the scan kernel is compared with */
int wdbx_index_probe_read(wdbx_index* idx, int nontemporal, int blocks, int reps, double* out_ms_per_pass);
/* tuning knobs (name/value); unknown names return WDBX_E_INVALID.  Settable: scan_lanes, scan_blocks, scan_nt,
 * scan_blocked, scan_generic, scan_force_ragged, exchange_batch, lds_lists, merge_fast (1: merges whose keys fit the registers are ranked there, default; 0: always the list walk), scan_one_grid (1: a round of several queries on the fp32 scan over a corpus of at most 1 GiB is one grid with a row per query, default; 0: a launch per query), poll_done (1: a blocking call of up to 32 queries whose chain ends in a final merge polls a word that kernel writes into the mapped staging slot, default; 0: always waits on its event), zero_copy, wg_merge, select_min_k,
 * scan_shadow (2 u8 selection scan / 1 bf16 tiles / 0 fp32 scan; range search: 2 u8 selection, below 2 the fp32 range scan), scan8_wgs, single_min_rows,
 * range_min_rows (rows from which a range search takes the u8 selection scan, default 131 072), gemm_bf16 (tile family
 * 3/2/1/0 as above), gemm_ct, gemm_l2, gemm_l2_i8, gemm8_variant (the i8 tiles' full-pass epilogue, for A/B: 0 = 14 the product form, 12, 13; any other value returns WDBX_E_INVALID), gemm8_refine (1: second selection stage of the i8 tiles, default), batch_repair, scan8_per_query, scan8_sample4 (1: a round's sample pass serves 3-4 queries per workgroup when the sample is too large for the L2s; 2: always; 0: never), gemm_min_queries, gemm_min_rows, gemm_min_work (below gemm_min_rows: the tiles from queries x rows >= this, default 800000; 0: never), gemm_sample_div, gemm_masked (1: a masked call with enough queries is one masked pass over the int8 tiles, default; 0: masked per-query scans), group_bounds, rows_keys_max (wdbx_index_search_rows: lists of at most this many rows are ranked from one key per listed row, default 8192; 0: never),
 * scan_u42_mfma (the split planes' full passes of a round on the matrix cores, 16 queries per read of the four-bit plane: -1 where the row's unit count has an instance (d from 257 to 384) and scan_u42_share is -1, default; 0: never; 1: wherever an instance exists; any other value returns WDBX_E_INVALID.  Answers are bit-identical at every setting).
 * get_option also answers the read-only names: last_u42_mfma_groups (the groups of 16 queries whose full pass ran on the matrix cores in the last call), last_gemm_family (0/1/2/3: what the last batch ran on),
 * last_single_path (0 fp32 scan / 1 bf16 tiles / 2 u8 selection scan), last_range_path (0 fp32 range scan / 2 u8 selection + exact filter), last_rows_path (the route of the last wdbx_index_search_rows: 0 nothing launched / 1 keys + merge / 2 lists + merge / 3 keys + radix select), last_sample_qn (queries per workgroup of the last u8 sample launch: 1, 3 or 4), last_batch_repaired, last_batch_masked (1: the last batch ran the masked tile pass), last_batch_allowed_rows (the rows its mask allowed), shadow_rows + shadow_bytes (bf16 copy),
 * shadow8_rows + shadow8_bytes (u8 copy), shadowg_rows + shadowg_bytes (group-scaled i8 copy), group_bounds_active,
 * exchanges (all-gather + merge steps this handle's per-rank communicator has enqueued), device_bytes_resident (every device
 * allocation of the handle: fp32 rows, shadow copies and their tables, scratch). */
int wdbx_index_set_option(wdbx_index* idx, const char* name, int64_t value);
int wdbx_index_get_option(wdbx_index* idx, const char* name, int64_t* value);

#ifdef __cplusplus
}
#endif
#endif /* WDBX_HIP_H */
