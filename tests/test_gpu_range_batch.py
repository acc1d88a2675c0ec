"""Batched range search on the MI355X (wdbx_index_range_search_batch and its public forms): one int8 tile pass per block of
queries.  The reference of every comparison is wdbx_index_range_search on the SAME handle (or an int64 brute force), never
the new entry point; every comparison is ``==`` on the CSR offsets, the rows and the bit patterns of the scores.

Corpora come from ``fill_synthetic`` and are read back.  ``gemm_min_rows = 16384`` as tests/test_gpu_multimask.py sets it, and
``gemm_min_work = 0`` (the row rule alone: at 20 011 rows the work rule of the top-k path, queries x rows >= 520 000, would keep
the batches of 4 and 17 queries off the tiles) let 20 011 rows -- no multiple of 256, 64 or 32 -- reach the tile route."""
import asyncio
import ctypes as C
import shutil
import tempfile

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

N = 20_011
E_INVALID = -1
NQ_MAX = 300


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


def _open(native, n, d, l2=False, normalize=True):
    ix = native.NativeIndex(d, metric=native.METRIC_L2 if l2 else native.METRIC_COSINE, capacity_rows=max(n, 1))
    if n:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=normalize)
    ix.set_option("gemm_min_rows", 16384)
    ix.set_option("gemm_min_work", 0)
    ix.set_option("single_min_rows", 0)
    return ix


_SHARED = {}


def _corpus(native, d, l2=False):
    """One index per shape, shared by the tests that do not write rows or options, and per query of a fixed set of 300 the
    scores wdbx_index_search returns for its 1000 best rows: what the thresholds are taken from."""
    key = (d, l2)
    if key not in _SHARED:
        ix = _open(native, N, d, l2)
        queries = _queries(NQ_MAX, d)
        _, scores = ix.search(queries, 1000)
        _SHARED[key] = (ix, queries, scores)
    return _SHARED[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for ix, _, _ in _SHARED.values():
        ix.close()
    _SHARED.clear()


def _queries(nq, d, offset=0):
    return O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, offset, nq, d))


def _thresholds(scores, l2):
    """per query from its own top-k scores: 0, 1, ~10 and ~1000 hits, and nothing at all (+inf; L2: -inf), in turn"""
    none = -np.inf if l2 else np.inf
    out = np.empty(len(scores), np.float32)
    for i, s in enumerate(scores):
        kind = i % 5
        out[i] = (np.nextafter(s[0], np.float32(none)) if kind == 0 else s[0] if kind == 1 else s[9] if kind == 2
                  else s[999] if kind == 3 else none)
    return out


def _same(got, ref, what=""):
    assert np.array_equal(got[0], ref[0]), (what, "offsets", got[0][:8], ref[0][:8])
    assert np.array_equal(got[1], ref[1]), (what, "rows")
    assert np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32)), (what, "score bits")


def _compare(ix, queries, thresholds, mask_words=None, path=2, what=""):
    ref = ix.range_search(queries, thresholds, mask_words=mask_words)
    got = ix.range_search_batch(queries, thresholds, mask_words=mask_words)
    _same(got, ref, what)
    if path is not None:
        assert ix.get_option("last_range_batch_path") == path, (what, ix.get_option("last_range_batch_path"))
    return got


def _raw(native, ix, entry, queries, thresholds, capacity, mask=None, mask_words=None):
    q = np.ascontiguousarray(queries, np.float32)
    t = np.ascontiguousarray(thresholds, np.float32)
    nq = len(q)
    off = np.full(nq + 1, 0xDEAD, np.uint64)
    rows = np.empty(max(capacity, 1), np.int64)
    scores = np.empty(max(capacity, 1), np.float32)
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = getattr(ix._lib, entry)(ix._h, q.ctypes.data_as(f32p), nq, t.ctypes.data_as(f32p), 0,
                                 None if mask is None else mask.ctypes.data_as(u32p),
                                 0 if mask is None else (len(mask) if mask_words is None else mask_words), capacity,
                                 off.ctypes.data_as(C.POINTER(C.c_uint64)), rows.ctypes.data_as(C.POINTER(C.c_int64)),
                                 scores.ctypes.data_as(f32p))
    return rc, off.astype(np.int64), rows, scores


# ---- 1. shapes and batch sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [4, 17, 256, 300])
@pytest.mark.parametrize("d,l2", [(384, False), (384, True), (100, False), (100, True)],
                         ids=["d384-cosine", "d384-l2", "d100-cosine", "d100-l2"])
def test_batches_equal_the_per_query_call(native, d, l2, nq):
    ix, queries, scores = _corpus(native, d, l2)
    t = _thresholds(scores[:nq], l2)
    ix.profile(True)
    ix.profile_read_gemm()
    off, _, _ = _compare(ix, queries[:nq], t, what=f"d={d} l2={l2} nq={nq}")
    block = 128 if l2 else 256
    blocks = -(-nq // block)
    assert ix.get_option("last_range_batch_blocks") == blocks
    assert ix.get_option("last_range_batch_fallback_queries") == 0
    assert ix.profile_read_gemm()["gemm_launches"] == blocks  # one tile pass per block, counted as a gemm launch
    ix.profile(False)
    counts = np.diff(off)
    assert ix.get_option("last_range_batch_pairs") >= counts.sum()
    # the thresholds do what they were chosen for: 0, 1, ~10, ~1000 hits and nothing, within one batch
    for i in range(nq):
        kind, c = i % 5, counts[i]
        # (a search score may sit an ulp from the range score of the same row where the search took another scoring kernel)
        assert (c == 0 if kind == 4 else c <= 1 if kind == 0 else c <= 3 if kind == 1 else 5 <= c <= 20 if kind == 2
                else 900 <= c <= 1100), (i, kind, c)


def test_d768_runs_blocks_of_128(native):
    ix, queries, scores = _corpus(native, 768)
    nq = 130
    _compare(ix, queries[:nq], _thresholds(scores[:nq], False), what="d=768")
    assert ix.get_option("last_range_batch_blocks") == 2


def test_three_queries_take_the_per_query_path(native):
    ix, queries, scores = _corpus(native, 384)
    q3, t3 = queries[1:4], _thresholds(scores[:4], False)[1:4]  # 1, ~10 and ~1000 hits
    _compare(ix, q3, t3, path=1)
    assert ix.get_option("last_range_batch_fallback_queries") == 3 and ix.get_option("last_range_batch_blocks") == 0
    ix.set_option("range_batch_min_queries", 3)
    try:
        _compare(ix, q3, t3, path=2)
    finally:
        ix.set_option("range_batch_min_queries", 4)


# ---- 2. counts and retries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l2", [False, True], ids=["cosine", "l2"])
def test_count_only_and_too_small_capacity_agree_with_the_full_call(native, l2):
    ix, queries, scores = _corpus(native, 384, l2)
    nq = 40
    q, t = queries[:nq], _thresholds(scores[:nq], l2)
    ref = ix.range_search(q, t)
    total = int(ref[0][-1])
    assert total > 8000
    for capacity in (0, 100, total - 1):
        rc, off, _, _ = _raw(native, ix, "wdbx_index_range_search_batch", q, t, capacity)
        assert rc == 0 and np.array_equal(off, ref[0]), capacity
        assert ix.get_option("last_range_batch_path") == 2
    rc, off, rows, sc = _raw(native, ix, "wdbx_index_range_search_batch", q, t, total)  # the retry with the exact total
    assert rc == 0
    _same((off, rows[:total], sc[:total]), ref, "exact capacity")


def test_capacity_rules_across_blocks_and_through_a_lost_block(native):
    """300 queries are two blocks: the running total, a later block that no longer fits, the per-block sort and decode -- and,
    with pair lists of 64, the same through blocks answered by the per-query rounds (their room is what the earlier blocks left)"""
    ix, queries, scores = _corpus(native, 384)
    q, t = queries, _thresholds(scores, False)
    ref = ix.range_search(q, t)
    total, first_block = int(ref[0][-1]), int(ref[0][256])
    assert 0 < first_block < total
    try:
        for pair_cap, path in ((0, 2), (64, 3)):
            ix.set_option("range_pair_cap", pair_cap)
            for capacity in (0, 100, first_block, first_block + 1, total - 1):  # (the first block fits, the second does not)
                rc, off, _, _ = _raw(native, ix, "wdbx_index_range_search_batch", q, t, capacity)
                assert rc == 0 and np.array_equal(off, ref[0]), (pair_cap, capacity)
                assert ix.get_option("last_range_batch_path") == path and ix.get_option("last_range_batch_blocks") == 2
            rc, off, rows, sc = _raw(native, ix, "wdbx_index_range_search_batch", q, t, total)
            assert rc == 0
            _same((off, rows[:total], sc[:total]), ref, f"exact capacity, pair lists of {pair_cap}")
    finally:
        ix.set_option("range_pair_cap", 0)


def test_the_default_work_rule_routes_by_queries_times_rows(native):
    """gemm_min_work at its default (800 000; 0.65 of it from gemm_min_rows rows): 300 x 20 011 passes it, 17 x 20 011 does not"""
    ix, queries, scores = _corpus(native, 384)
    t = _thresholds(scores, False)
    ix.set_option("gemm_min_work", 800000)
    try:
        _compare(ix, queries, t, path=2, what="300 queries under the work rule")
        assert ix.get_option("last_range_batch_blocks") == 2
        _compare(ix, queries[:17], t[:17], path=1, what="17 queries under the work rule")
    finally:
        ix.set_option("gemm_min_work", 0)


# ---- 3. ties at the threshold ----------------------------------------------------------------------------------------------
def test_forty_copies_at_the_threshold_all_come_back_in_row_order(native):
    d = 384
    queries = _queries(8, d, 40)
    with _open(native, N, d) as ix:
        idx, _ = ix.search(queries[:1], 1)
        best = ix.get_rows(int(idx[0, 0]), 1)
        copies = np.unique(np.concatenate([np.arange(5000, 5032), [0, 255, 256, 12_345, 19_999, 20_000, N - 2, N - 1]]))
        assert len(copies) == 40
        for r in copies:
            ix.set_rows(int(r), best)
        _, s = ix.search(queries[:1], 1)
        _, _, first = ix.range_search(queries[:1], s[0, 0] - np.float32(1e-3))
        t = np.full(8, first[0], np.float32)  # exactly the score the range search returns for the copies
        off, rows, scores = _compare(ix, queries, t, what="ties")
        mine = rows[off[0]:off[1]]
        at_t = mine[scores[off[0]:off[1]].view(np.uint32) == t[:1].view(np.uint32)[0]]
        assert set(copies.tolist()) <= set(at_t.tolist()) and np.all(np.diff(at_t) > 0)


# ---- 4. masks, removed rows, NaN / inf -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,l2", [(384, False), (100, True)], ids=["d384-cosine", "d100-l2"])
def test_masks(native, d, l2):
    ix, queries, scores = _corpus(native, d, l2)
    nq = 40
    t = _thresholds(scores[:nq], l2)
    rng = np.random.default_rng(3)
    for name, allowed in (("5 %", rng.random(N) < 0.05), ("every second row", np.arange(N) % 2 == 0)):
        words = native.pack_row_mask(allowed)
        got = _compare(ix, queries[:nq], t, mask_words=words, what=name)
        assert np.all(allowed[got[1]]) and got[0][-1] > 0
        # bits set past the last row change nothing
        words2 = words.copy()
        words2[-1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
        _same(ix.range_search_batch(queries[:nq], t, mask_words=words2), got, name + ", bits past the end")


def test_a_short_mask_is_refused_and_the_handle_stays_usable(native):
    ix, queries, scores = _corpus(native, 384)
    t = _thresholds(scores[:8], False)
    words = native.pack_row_mask(np.ones(N, bool))
    rc, _, _, _ = _raw(native, ix, "wdbx_index_range_search_batch", queries[:8], t, 0, mask=words, mask_words=len(words) - 1)
    assert rc == E_INVALID
    rc, _, _, _ = _raw(native, ix, "wdbx_index_range_search_batch", queries[:8], np.full(8, np.nan, np.float32), 0)
    assert rc == E_INVALID
    _compare(ix, queries[:8], t, what="after the refusals")
    _compare(ix, queries[:8], t, mask_words=words, what="a full mask")


@pytest.mark.parametrize("l2", [False, True], ids=["cosine", "l2"])
def test_removed_rows_and_an_infinite_element(native, l2):
    d = 100
    queries = _queries(24, d, 7)
    with _open(native, N, d, l2) as ix:
        _, s = ix.search(queries, 1000)
        t = _thresholds(s, l2)
        idx, _ = ix.search(queries, 3)
        last_tile = N // 256 * 256
        dead = np.unique(np.concatenate([idx.ravel(), [0, 63, 64, last_tile, last_tile + 1, N - 2, N - 1]]))  # best rows, the last tile's rows and its end
        for r in dead:
            ix.set_rows(int(r), np.full((1, d), np.nan, np.float32))
        inf_row = ix.get_rows(777, 1)
        inf_row[0, 3] = np.inf
        ix.set_rows(777, inf_row)  # its 64-row group cannot be quantised: all of it goes to the exact pass
        off, rows, scores = _compare(ix, queries, t, what="tombstones")
        assert not np.any(np.isin(rows, dead)) and not np.any(np.isnan(scores))
        # +inf as a threshold: only a score of +inf reaches it (cosine: the infinite row, where the query's element is positive)
        t_inf = np.full(24, -np.inf if l2 else np.inf, np.float32)
        off, rows, _ = _compare(ix, queries, t_inf, what="infinite thresholds")
        assert set(rows.tolist()) <= {777}
        words = native.pack_row_mask(np.arange(N) % 3 != 0)
        _compare(ix, queries, t, mask_words=words, what="tombstones under a mask")


# ---- 5. an integer corpus: the result set independent of any library path --------------------------------------------------
@pytest.mark.parametrize("l2", [False, True], ids=["inner-product", "l2"])
def test_integer_corpus_against_int64(native, l2):
    d, nq = 100, 20
    rng = np.random.default_rng(12)
    rows = rng.integers(-3, 4, size=(N, d)).astype(np.float32)
    rows[5::97] *= 8  # (unnormalised on purpose: norms differ inside the 64-row groups)
    queries = rng.integers(-4, 5, size=(nq, d)).astype(np.float32)
    with _open(native, 0, d, l2) as ix:
        ix.add(rows)
        r64, q64 = rows.astype(np.int64), queries.astype(np.int64)
        exact = ((r64[None, :, :] - q64[:, None, :]) ** 2).sum(axis=2) if l2 else q64 @ r64.T  # [nq, N], exact in fp32 too
        assert np.abs(exact).max() < 2 ** 24
        srt = np.sort(exact, axis=1)
        t = np.array([(srt[i, [0, 9, 99, 999][i % 4]] if l2 else srt[i, -1 - [0, 9, 99, 999][i % 4]]) for i in range(nq)], np.float32)
        off, got_rows, got_scores = _compare(ix, queries, t, what="integers")
        for i in range(nq):
            hit = np.flatnonzero(exact[i] <= t[i]) if l2 else np.flatnonzero(exact[i] >= t[i])
            key = exact[i, hit] if l2 else -exact[i, hit]
            want = hit[np.lexsort((hit, key))]
            assert np.array_equal(got_rows[off[i]:off[i + 1]], want), i
            assert np.array_equal(got_scores[off[i]:off[i + 1]], exact[i, want].astype(np.float32)), i


# ---- 6. the two overflows --------------------------------------------------------------------------------------------------
def test_a_full_pair_list_sends_its_block_through_the_per_query_path(native):
    d = 384
    with _open(native, N, d) as ix:
        queries = _queries(NQ_MAX, d)
        _, s = ix.search(queries, 1000)
        t = s[:, 999].copy()  # ~1000 hits each
        with pytest.raises(native.HipBackendError):
            ix.set_option("range_pair_cap", 63)
        ix.set_option("range_pair_cap", 64)
        off, _, _ = _compare(ix, queries, t, path=3, what="pair lists of 64")
        assert ix.get_option("last_range_batch_fallback_queries") > 0 and ix.get_option("last_range_batch_blocks") == 2
        assert np.all(np.diff(off) >= 990)  # (a search score may sit an ulp from the range score)
        # -inf cosine queries in a batch of 8 return every non-NaN row: through the per-query path where the pair lists fill (three
        # such queries are 96 pairs per wave of 32 rows, against lists of 64), and from the tiles with the default lists (20 010
        # pairs per query spread over the waves fit them: the candidate buffers grow instead)
        ix.set_rows(100, np.full((1, d), np.nan, np.float32))
        for cap, path, everything in ((64, 3, [1, 5, 6]), (0, 2, [5])):
            t8 = s[:8, 9].copy()
            t8[everything] = -np.inf
            ix.set_option("range_pair_cap", cap)
            off, rows, _ = _compare(ix, queries[:8], t8, path=path, what="-inf in a batch")
            for i in everything:
                assert off[i + 1] - off[i] == N - 1 and 100 not in rows[off[i]:off[i + 1]]
            assert ix.get_option("last_range_batch_fallback_queries") == (8 if cap else 0)


def test_candidate_buffers_grow_to_the_exact_count(native):
    d = 384
    with _open(native, N, d) as ix:
        queries = _queries(16, d, 500)
        _, s = ix.search(queries, 2000)
        _compare(ix, queries, s[:, 0].copy(), what="tiny results")  # one hit each: the buffers stay at their first size
        # ~5000 hits for one query: a threshold between the 2000th score and 0 by the rows' own scores
        all_scores = ix.get_rows(0, N) @ queries[3]
        t = s[:, 4].copy()
        t[3] = np.sort(all_scores)[-5000]
        off, _, _ = _compare(ix, queries, t, what="one query with ~5000 hits")
        assert 4900 <= off[4] - off[3] <= 5100
        _compare(ix, queries, t, what="again, the buffers grown")


# ---- 7. per-query fallbacks, the empty index -------------------------------------------------------------------------------
def test_other_tile_families_and_small_indexes_answer_per_query(native):
    d = 384
    with _open(native, N, d) as ix:
        queries = _queries(12, d, 30)
        _, s = ix.search(queries, 10)
        t = s[:, 9].copy()
        for option, value, back in (("gemm_bf16", 2, 3), ("gemm8_variant", 13, 0)):
            ix.set_option(option, value)
            _compare(ix, queries, t, path=1, what=option)
            ix.set_option(option, back)
        ix.set_option("gemm_masked", 0)
        _compare(ix, queries, t, mask_words=native.pack_row_mask(np.arange(N) % 2 == 0), path=1, what="gemm_masked = 0")
        _compare(ix, queries, t, path=2, what="gemm_masked = 0, no mask")
    with _open(native, 1000, d) as ix:
        _, s = ix.search(queries, 10)
        _compare(ix, queries, s[:, 9].copy(), path=1, what="1 000 rows")


def test_empty_index(native):
    with _open(native, 0, 100) as ix:
        off, rows, scores = ix.range_search_batch(_queries(6, 100), 0.5)
        assert off.tolist() == [0] * 7 and len(rows) == 0 and len(scores) == 0
        assert ix.get_option("last_range_batch_path") == 0 and ix.get_option("last_range_batch_blocks") == 0


# ---- 8. the public layers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 2])
def test_store_and_rest_equal_search_range_per_query(shards):
    from wdbx_amd import WDBX, api

    d, n = 16, 600
    temp_dir = tempfile.mkdtemp()
    w = WDBX(vector_dimension=d, num_shards=shards, data_dir=temp_dir, enable_plugins=False,
             config={"WDBX_VECTOR_STORE_SAVE_IMMEDIATELY": False})
    try:
        asyncio.run(w.initialize())
        rng = np.random.default_rng(5)
        vectors = {f"v{i}": rng.standard_normal(d).astype(np.float32).tolist() for i in range(n)}
        meta = {f"v{i}": {"lang": "en" if i % 3 == 0 else "de"} for i in range(n)}
        assert w.vector_store.batch_store(vectors, meta) == n
        queries = rng.standard_normal((9, d)).astype(np.float32).tolist()
        thresholds = [0.9, 0.5, 0.3, 0.1, 0.0, -1.5, 0.4, 0.2, 0.6]
        for kw in ({}, {"filter_metadata": {"lang": "en"}}, {"filter_metadata": {"lang": "en"}, "prefilter": True},
                   {"max_results": 7}):
            got = w.vector_store.search_range_batch(queries, thresholds, **kw)
            assert len(got) == 9 and len(got[5]) == (7 if "max_results" in kw else n // 3 if kw else n)
            for q, t, res in zip(queries, thresholds, got):
                assert res == w.vector_store.search_range(q, t, **kw)
        assert w.vector_search_range_batch(queries, 0.3) == [w.vector_search_range(q, 0.3) for q in queries]
        body = {"query_vectors": queries, "thresholds": thresholds, "filter_metadata": {"lang": "de"}, "max_results": 50}
        out = asyncio.run(api.range_search_batch_endpoint(w, body))
        for q, t, res in zip(queries, thresholds, out["results"]):
            one = asyncio.run(api.range_search_endpoint(w, {"query_vector": q, "threshold": t, "filter_metadata": {"lang": "de"},
                                                           "max_results": 50}))
            assert res == one["results"]
    finally:
        asyncio.run(w.shutdown())
        shutil.rmtree(temp_dir, ignore_errors=True)
