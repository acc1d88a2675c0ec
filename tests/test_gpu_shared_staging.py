"""The blocking entry points share one query upload, one pair of result buffers and one mask scope (host_index.h:
upload_queries, ensure_out, download_results, MaskScope).  So: every entry point in turn on ONE handle, in an order in which
the buffers grow, are reused by a smaller call, and are used by another entry point than the one that sized them -- each
answer equal to a numpy float64 brute force, ids and scores, on integer data where every fp32 score is exact and ties
resolve by row number (as tests/test_gpu_search_rows.py does).  And a mask that is too short is refused by every call that
takes one, with the handle usable right afterwards."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


def _case(native, d, n, metric):
    """n rows and 64 queries with integer elements in {-2 .. 2}, un-normalised, and the float64 score of every pair"""
    rng = np.random.default_rng(7 * d + n + metric)
    rows = rng.integers(-2, 3, size=(n, d)).astype(np.float64)
    queries = rng.integers(-2, 3, size=(64, d)).astype(np.float64)
    if metric == COS:
        score = queries @ rows.T
    else:
        score = ((queries[:, None, :] - rows[None, :, :]) ** 2).sum(axis=2)
    ix = native.NativeIndex(d, metric, 0, capacity_rows=n)
    ix.add(rows.astype(np.float32), normalize=False)
    return ix, queries.astype(np.float32), score, rng


def _order(s, ids, metric):
    """(score descending, row ascending); L2: (distance ascending, row ascending)"""
    return np.lexsort((ids, -s if metric == COS else s))


def _topk(score, metric, q0, allowed, k):
    """allowed: per query of the call, the row numbers (ascending) it may return; unused slots -1 / 0.0"""
    e_idx = np.full((len(allowed), k), -1, np.int64)
    e_score = np.zeros((len(allowed), k), np.float32)
    for i, ids in enumerate(allowed):
        s = score[q0 + i, ids]
        order = _order(s, ids, metric)[:k]
        e_idx[i, : len(order)] = ids[order]
        e_score[i, : len(order)] = s[order]
    return e_idx, e_score


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d,n,long_list", [(54, 3000, 2000), (16, 500, 400)])  # pitch 56: the padded copy; pitch == dim: the plain one
def test_every_entry_point_in_turn_on_one_handle(native, d, n, long_list, metric):
    ix, queries, score, rng = _case(native, d, n, metric)
    every = np.arange(n)
    try:
        # 1. the smallest call
        first = ix.search(queries[:1], 1)
        _same(first, _topk(score, metric, 0, [every], 1), "search 1 x 1")
        # 2. a mask per query, 3 masks and the unmasked class: class by class on a shard this small, the buffers grow
        allowed = [np.flatnonzero(rng.random(n) < p) for p in (0.5, 0.1, 0.01)]
        masks = [native.pack_row_mask(np.isin(every, a)) for a in allowed]
        which = rng.integers(-1, 3, 40)
        which[:4] = [-1, 0, 1, 2]
        got = ix.search_multimask(queries[:40], 50, masks, which)
        assert ix.get_option("last_batch_masked") == 0
        _same(got, _topk(score, metric, 0, [every if c < 0 else allowed[c] for c in which], 50), "multimask 40 x 50")
        # 3. a row list per query: the batched pass for the short lists, list by list for the long one
        lists = [np.empty(0, np.int64), np.array([n - 1]), np.sort(rng.choice(n, 7, replace=False)),
                 np.sort(rng.choice(n, long_list, replace=False))]
        query_list = np.array([0, 1, 2, 3, 3, 2, 1, 0, 3])
        ix.set_option("rows_keys_max", 64)
        got = ix.search_row_lists(queries[:9], 5, lists, query_list)
        assert ix.get_option("last_lists_path") == 2
        _same(got, _topk(score, metric, 0, [lists[l] for l in query_list], 5), "row lists 9 x 5")
        # 4. listed rows, the largest result so far
        ids = np.sort(rng.choice(n, 500, replace=False))
        got = ix.search_rows(queries[:33], 128, ids)
        _same(got, _topk(score, metric, 0, [ids] * 33, 128), "rows 33 x 128")
        # 5. a range search under a mask: the threshold is the 30th best allowed score of each query (ties come along)
        mask_rows = allowed[0]
        thr = np.array([score[q, mask_rows][_order(score[q, mask_rows], mask_rows, metric)[29]] for q in range(3)], np.float32)
        offsets, r_rows, r_scores = ix.range_search(queries[:3], thr, mask_words=masks[0])
        for q in range(3):
            s = score[q, mask_rows]
            keep = s >= thr[q] if metric == COS else s <= thr[q]
            order = _order(s[keep], mask_rows[keep], metric)
            assert 30 <= keep.sum() < 200, keep.sum()
            assert np.array_equal(r_rows[offsets[q]:offsets[q + 1]], mask_rows[keep][order]), ("range", q)
            assert np.array_equal(r_scores[offsets[q]:offsets[q + 1]], s[keep][order].astype(np.float32)), ("range", q)
        # 6. one mask for the call, small again
        got = ix.search(queries[:2], 3, mask_words=masks[1])
        _same(got, _topk(score, metric, 0, [allowed[1]] * 2, 3), "masked 2 x 3")
        # 7. the first call again
        again = ix.search(queries[:1], 1)
        _same(again, first, "search 1 x 1 again")
    finally:
        ix.close()


@pytest.mark.parametrize("metric", [COS, L2])
def test_a_short_mask_is_refused_and_leaves_the_handle_usable(native, metric):
    d, n = 54, 3000
    ix, queries, score, rng = _case(native, d, n, metric)
    every = np.arange(n)
    try:
        allowed = np.flatnonzero(rng.random(n) < 0.3)
        mask = native.pack_row_mask(np.isin(every, allowed))
        short = mask.size - 1
        f32p, i64p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        q = np.ascontiguousarray(queries[:2])
        idx, sc = np.empty((2, 3), np.int64), np.empty((2, 3), np.float32)
        want = _topk(score, metric, 0, [allowed] * 2, 3)
        lib, h = ix._lib, ix._h

        def refused(rc):
            assert rc == -1 and b"row mask" in lib.wdbx_last_error(), (rc, lib.wdbx_last_error())
            # (had the refused call left its mask on the handle, this unmasked search would be filtered by it)
            _same(ix.search(q, 3), _topk(score, metric, 0, [every] * 2, 3), "unmasked after a refusal")
            _same(ix.search(q, 3, mask_words=mask), want, "masked after a refusal")

        refused(lib.wdbx_index_search_masked_n(h, q.ctypes.data_as(f32p), 2, 3, 0, mask.ctypes.data_as(u32p), short,
                                               idx.ctypes.data_as(i64p), sc.ctypes.data_as(f32p)))
        ptrs = (u32p * 1)(mask.ctypes.data_as(u32p))
        counts = (C.c_uint64 * 1)(short)
        which = np.array([0, -1], np.int32)
        refused(lib.wdbx_index_search_multimask(h, q.ctypes.data_as(f32p), 2, 3, 0, ptrs, counts, 1,
                                                which.ctypes.data_as(C.POINTER(C.c_int32)), idx.ctypes.data_as(i64p),
                                                sc.ctypes.data_as(f32p)))
        thr = np.full(2, 1e9 if metric == L2 else -1e9, np.float32)
        offsets, r_rows, r_scores = np.zeros(3, np.uint64), np.empty(2 * n, np.int64), np.empty(2 * n, np.float32)
        refused(lib.wdbx_index_range_search(h, q.ctypes.data_as(f32p), 2, thr.ctypes.data_as(f32p), 0, mask.ctypes.data_as(u32p),
                                            short, 2 * n, offsets.ctypes.data_as(u64p), r_rows.ctypes.data_as(i64p),
                                            r_scores.ctypes.data_as(f32p)))
        off, rr, _ = ix.range_search(q, thr, mask_words=mask)  # every allowed row, twice
        assert off.tolist() == [0, len(allowed), 2 * len(allowed)] and np.array_equal(np.sort(rr[: len(allowed)]), allowed)
    finally:
        ix.close()
