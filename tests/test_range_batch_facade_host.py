"""Batched range search, host side (no GPU): ``VectorStore.search_range_batch``, the facade and the REST endpoint.  The shard
is a stub that scores a small corpus exactly in numpy and honours row masks the way the library does; it records every call,
so the tests see ONE call per shard for the whole batch.  The reference of every comparison is ``search_range`` per query."""
import asyncio
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from wdbx_amd import api
from wdbx_amd.config import WDBXConfig
from wdbx_amd.vector_store import VectorStore
from wdbx_amd.wdbx import WDBX

D, N = 4, 90


def _pack(allowed):
    bits = np.zeros((len(allowed) + 31) // 32 * 32, bool)
    bits[: len(allowed)] = allowed
    return np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).ravel()


def _unpack(words, n):
    return ((words[np.arange(n) // 32] >> (np.arange(n) % 32).astype(np.uint32)) & 1).astype(bool)


class _Shard:
    """An exact shard over ``rows`` with ids ``v<first + row>``."""

    def __init__(self, rows, first):
        self.rows, self.first = rows, first
        self.next_index = len(rows)
        self.calls = []  # (kind, number of queries, masked)
        self.thread_pool = None
        self.swallow_errors = False

    def _range(self, q, t, row_mask):
        s = self.rows @ np.asarray(q, np.float32)
        allowed = np.ones(len(s), bool) if row_mask is None else _unpack(row_mask, len(s))
        order = [r for r in np.lexsort((np.arange(len(s)), -s)) if allowed[r] and s[r] >= np.float32(t)]
        return [(f"v{self.first + r}", float(s[r])) for r in order]

    def range_search(self, q, threshold, row_mask=None):
        self.calls.append(("single", 1, row_mask is not None))
        return self._range(q, threshold, row_mask)

    def range_search_batch(self, queries, thresholds, row_mask=None):
        thresholds = np.broadcast_to(np.asarray(thresholds, np.float64), (len(queries),))
        self.calls.append(("batch", len(queries), row_mask is not None))
        return [self._range(q, t, row_mask) for q, t in zip(queries, thresholds)]

    def row_mask_for(self, predicate):
        return _pack(np.array([predicate(f"v{self.first + r}") for r in range(len(self.rows))]))


def _store(shards):
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((N, D)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    cut = [0, N] if shards == 1 else [0, 40, N]
    vs = VectorStore.__new__(VectorStore)
    vs.indices = [_Shard(rows[a:b], a) for a, b in zip(cut, cut[1:])]
    vs.metadata = {f"v{r}": {"lang": "en" if r % 3 == 0 else "de"} for r in range(N)}
    vs.vector_dim = D
    vs.config = WDBXConfig({})
    vs._mask_cache, vs._meta_version = {}, 0
    vs._pending, vs._drain_task = [], None
    vs._group = False
    vs._sync_lock, vs._sync_pending, vs._sync_busy, vs._sync_coalesce, vs._sync_last_batch = threading.Lock(), [], False, False, 0
    vs._group_lock, vs._group_verified, vs._group_path, vs.last_search_path = threading.Lock(), False, "copy_group", ""
    vs.thread_pool = ThreadPoolExecutor(max_workers=4)
    vs._shard_pool = ThreadPoolExecutor(max_workers=2)
    return vs


@pytest.fixture(params=[1, 2], ids=["one shard", "two shards"])
def store(request):
    return _store(request.param)


def _queries(n, seed=3):
    q = np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _calls(store):
    return [c for ix in store.indices for c in ix.calls]


def _reset(store):
    for ix in store.indices:
        ix.calls.clear()


def test_scalar_threshold_is_one_call_per_shard_and_equals_search_range(store):
    queries = _queries(7)
    got = store.search_range_batch(queries, 0.4)
    assert _calls(store) == [("batch", 7, False)] * len(store.indices)
    assert len(got) == 7 and any(got)
    for q, res in zip(queries, got):
        assert res == store.search_range(q, 0.4)


def test_one_threshold_per_query(store):
    queries = _queries(5)
    thresholds = [0.9, -1.0, 0.2, 0.5, 2.0]
    got = store.search_range_batch(queries, thresholds)
    for q, t, res in zip(queries, thresholds, got):
        assert res == store.search_range(q, t)
    assert len(got[1]) == N and got[4] == []
    # merged per query over the shards: best first, ties and order as merge_range leaves them
    assert all(a[1] >= b[1] for res in got for a, b in zip(res, res[1:]))


def test_filter_travels_as_the_mask_under_prefilter_and_is_post_filtered_without(store):
    queries, flt = _queries(6), {"lang": "en"}
    pushed = store.search_range_batch(queries, 0.1, filter_metadata=flt, prefilter=True)
    assert _calls(store) == [("batch", 6, True)] * len(store.indices)
    _reset(store)
    posted = store.search_range_batch(queries, 0.1, filter_metadata=flt)
    assert _calls(store) == [("batch", 6, False)] * len(store.indices)
    assert pushed == posted and any(pushed)
    for q, res in zip(queries, pushed):
        assert res == store.search_range(q, 0.1, filter_metadata=flt, prefilter=True)
        assert all(r[2]["lang"] == "en" for r in res)
    _reset(store)
    store.config = WDBXConfig({"FILTER_PUSHDOWN": True})
    assert store.search_range_batch(queries, 0.1, filter_metadata=flt) == pushed
    assert _calls(store) == [("batch", 6, True)] * len(store.indices)


def test_max_results_cuts_each_query(store):
    queries = _queries(4)
    got = store.search_range_batch(queries, -1.0, max_results=5)
    assert [len(r) for r in got] == [5] * 4
    for q, res in zip(queries, got):
        assert res == store.search_range(q, -1.0, max_results=5)
    assert store.search_range_batch(queries, -1.0, max_results=0) == [[]] * 4


def test_refusals_and_the_empty_batch(store):
    assert store.search_range_batch([], 0.5) == []
    with pytest.raises(ValueError):
        store.search_range_batch(_queries(3), [0.1, 0.2])
    with pytest.raises(ValueError):
        store.search_range_batch(_queries(2), [0.1, float("nan")])
    with pytest.raises(ValueError):
        store.search_range_batch([[1.0, 2.0]], 0.5)
    assert _calls(store) == []


def test_async_form(store):
    queries = _queries(3)
    got = asyncio.run(store.search_range_batch_async(queries.tolist(), [0.3, 0.4, 0.5]))
    assert got == store.search_range_batch(queries, [0.3, 0.4, 0.5])


class _W:
    """the facade's two methods over a stub store (WDBX itself needs a device)"""

    def __init__(self, store):
        self.vector_store, self.vector_dim = store, D

    _check_dim = WDBX._check_dim
    vector_search_range_batch = WDBX.vector_search_range_batch
    vector_search_range_batch_async = WDBX.vector_search_range_batch_async


def test_facade_passes_through(store):
    w, queries = _W(store), _queries(3)
    assert w.vector_search_range_batch(queries.tolist(), 0.3, max_results=4) == store.search_range_batch(queries, 0.3, max_results=4)
    with pytest.raises(ValueError):
        w.vector_search_range_batch([[1.0]], 0.3)


def test_rest_endpoint(store):
    w, queries = _W(store), _queries(3)
    body = {"query_vectors": queries.tolist(), "thresholds": [0.2, 0.5, 0.9], "filter_metadata": {"lang": "de"}, "max_results": 6}
    out = asyncio.run(api.range_search_batch_endpoint(w, body))
    want = store.search_range_batch(queries, [0.2, 0.5, 0.9], filter_metadata={"lang": "de"}, max_results=6)
    assert [[r["vector_id"] for r in res] for res in out["results"]] == [[r[0] for r in res] for res in want]
    assert [[r["similarity"] for r in res] for res in out["results"]] == [[r[1] for r in res] for res in want]
    one = asyncio.run(api.range_search_batch_endpoint(w, {"query_vectors": queries.tolist(), "threshold": 0.5}))
    assert [[r["vector_id"] for r in res] for res in one["results"]] == [[r[0] for r in res] for res in store.search_range_batch(queries, 0.5)]
    assert asyncio.run(api.range_search_batch_endpoint(w, {"query_vectors": [], "threshold": 0.5})) == {"results": []}
    for bad in ([1, 2], {"threshold": 0.5}, {"query_vectors": queries.tolist()},
                dict(body, threshold=0.5), dict(body, thresholds=[0.1]), dict(body, thresholds=[0.1, "x", 0.2]),
                dict(body, thresholds=[0.1, float("nan"), 0.2]), dict(body, thresholds=0.5),
                {"query_vectors": queries.tolist(), "threshold": True}, dict(body, filter_metadata=[1]),
                dict(body, max_results=-1), dict(body, max_results=1.5), dict(body, query_vectors=[[1.0, "a"]])):
        with pytest.raises(ValueError):
            asyncio.run(api.range_search_batch_endpoint(w, bad))
