"""Filter push-down for batches, host side (no GPU): ``VectorStore.search_batch(prefilter=)``, the REST field, and the
async coalescer batching callers that share one pushed-down filter.  The shard is a stub that ranks a small corpus exactly
in numpy and honours a row mask the way the library does (only rows whose bit is set compete); it records every call."""
import asyncio
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from wdbx_amd import api
from wdbx_amd.config import WDBXConfig
from wdbx_amd.vector_store import VectorStore

D, N = 4, 60


def _pack(allowed):
    bits = np.zeros((len(allowed) + 31) // 32 * 32, bool)
    bits[: len(allowed)] = allowed
    return np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).ravel()


def _unpack(words, n):
    return ((words[np.arange(n) // 32] >> (np.arange(n) % 32).astype(np.uint32)) & 1).astype(bool)


class _Shard:
    """An exact shard over ``rows`` with ids ``v<row>``."""

    def __init__(self, rows):
        self.rows = rows
        self.next_index = len(rows)
        self.calls = []  # (kind, number of queries, mask as a tuple of allowed rows or None)
        self.thread_pool = None
        self.swallow_errors = False

    def _rank(self, q, limit, row_mask):
        s = self.rows @ np.asarray(q, np.float32)
        allowed = np.ones(len(s), bool) if row_mask is None else _unpack(row_mask, len(s))
        order = [r for r in np.lexsort((np.arange(len(s)), -s)) if allowed[r]]
        return [(f"v{r}", float(s[r])) for r in order[:limit]]

    @staticmethod
    def _key(row_mask):
        return None if row_mask is None else tuple(np.nonzero(_unpack(row_mask, N))[0].tolist())

    def search(self, q, limit=10, row_mask=None):
        self.calls.append(("single", 1, self._key(row_mask)))
        return self._rank(q, limit, row_mask)

    def search_batch(self, queries, limit=10, row_mask=None):
        self.calls.append(("batch", len(queries), self._key(row_mask)))
        return [self._rank(q, limit, row_mask) for q in queries]

    def row_mask_for(self, predicate):
        return _pack(np.array([predicate(f"v{r}") for r in range(len(self.rows))]))


@pytest.fixture()
def store():
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((N, D)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    vs = VectorStore.__new__(VectorStore)
    vs.indices = [_Shard(rows)]
    # one row in six is "en", one in ten "de": a post-filter of a top-5 under-returns
    vs.metadata = {f"v{r}": {"lang": "en" if r % 6 == 0 else "de" if r % 10 == 1 else "xx"} for r in range(N)}
    vs.vector_dim = D
    vs.config = WDBXConfig({})
    vs._mask_cache, vs._meta_version = {}, 0
    vs._pending, vs._drain_task = [], None
    vs._group = False
    vs._sync_lock, vs._sync_pending, vs._sync_busy, vs._sync_coalesce, vs._sync_last_batch = threading.Lock(), [], False, False, 0
    vs._group_lock, vs._group_verified, vs._group_path, vs.last_search_path = threading.Lock(), False, "copy_group", ""
    vs.thread_pool = ThreadPoolExecutor(max_workers=4)
    vs._shard_pool = ThreadPoolExecutor(max_workers=1)
    vs.rows = rows
    return vs


def _queries(n, seed=3):
    q = np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def test_prefilter_returns_a_full_limit_where_the_post_filter_under_returns(store):
    queries, flt, limit = _queries(6), {"lang": "en"}, 5
    post = store.search_batch(queries, limit=limit, filter_metadata=flt)
    assert any(len(r) < limit for r in post), "the corpus is meant to make the post-filter under-return"
    pushed = store.search_batch(queries, limit=limit, filter_metadata=flt, prefilter=True)
    en = [r for r in range(N) if r % 6 == 0]
    for q, res in zip(queries, pushed):
        assert len(res) == limit and all(meta == {"lang": "en"} for _, _, meta in res)
        s = store.rows[en] @ q
        want = [f"v{en[i]}" for i in np.lexsort((np.arange(len(en)), -s))[:limit]]
        assert [vid for vid, _, _ in res] == want
        assert res == store.search(q, limit=limit, filter_metadata=flt, prefilter=True)
    # ONE batched call with the filter's mask reached the shard
    batched = [c for c in store.indices[0].calls if c[0] == "batch" and c[2] is not None]
    assert batched == [("batch", 6, tuple(en))]


def test_default_and_prefilter_false_keep_todays_output(store):
    queries, flt, limit = _queries(5, seed=4), {"lang": "en"}, 5
    today = [store._merge([store.indices[0]._rank(q, limit, None)], limit, 0.0, flt) for q in queries]
    assert store.search_batch(queries, limit=limit, filter_metadata=flt) == today
    assert store.search_batch(queries, limit=limit, filter_metadata=flt, prefilter=False) == today
    assert all(c[2] is None for c in store.indices[0].calls)  # no mask ever reached the shard
    # without a filter prefilter=True changes nothing either
    assert store.search_batch(queries, limit=limit, prefilter=True) == store.search_batch(queries, limit=limit)
    # config FILTER_PUSHDOWN is the default of prefilter=None, as in search()
    store.config = WDBXConfig({"FILTER_PUSHDOWN": True})
    assert store.search_batch(queries, limit=limit, filter_metadata=flt) == \
        store.search_batch(queries, limit=limit, filter_metadata=flt, prefilter=True)
    assert store.search_batch(queries, limit=limit, filter_metadata=flt, prefilter=False) == today


class _Facade:
    def __init__(self):
        self.seen = []

    def vector_search_batch(self, queries, limit=10, threshold=0.0, filter_metadata=None, **kw):
        self.seen.append((len(queries), limit, filter_metadata, kw))
        return [[("a", 0.5, {})] for _ in queries]


def test_rest_batch_endpoint_parses_prefilter():
    w = _Facade()
    body = {"query_vectors": [[0.0, 1.0], [1.0, 0.0]], "limit": 3, "filter_metadata": {"lang": "en"}}
    out = asyncio.run(api.search_batch_endpoint(w, dict(body, prefilter=True)))
    assert out == {"results": [[{"vector_id": "a", "similarity": 0.5, "metadata": {}}]] * 2}
    asyncio.run(api.search_batch_endpoint(w, dict(body, prefilter=False)))
    asyncio.run(api.search_batch_endpoint(w, body))
    asyncio.run(api.search_batch_endpoint(w, dict(body, prefilter=None)))
    assert [s[3] for s in w.seen] == [{"prefilter": True}, {"prefilter": False}, {}, {}]
    for bad in ("yes", 1, [True]):
        with pytest.raises(ValueError):
            asyncio.run(api.search_batch_endpoint(w, dict(body, prefilter=bad)))


def test_wdbx_facade_passes_prefilter_on():
    from wdbx_amd.wdbx import WDBX

    w = WDBX.__new__(WDBX)
    w.vector_dim = D

    class _Store:
        def search_batch(self, queries, **kw):
            return kw

    w.vector_store = _Store()
    assert w.vector_search_batch([[0.0] * D], limit=3, filter_metadata={"a": 1}, prefilter=True) == \
        {"limit": 3, "threshold": 0.0, "filter_metadata": {"a": 1}, "prefilter": True}
    assert w.vector_search_batch([[0.0] * D])["prefilter"] is None


def test_async_callers_with_the_same_filter_share_one_masked_batch(store):
    queries = _queries(6, seed=5)
    en, de = {"lang": "en"}, {"lang": "de"}

    async def many(filters):
        return await asyncio.gather(*[store.search_async(q.tolist(), limit=4, filter_metadata=f, prefilter=True)
                                      for q, f in zip(queries, filters)])

    got = asyncio.run(many([en] * 6))
    calls = store.indices[0].calls
    en_rows = tuple(r for r in range(N) if r % 6 == 0)
    assert calls == [("batch", 6, en_rows)], calls
    for q, res in zip(queries, got):
        assert res == store.search(q, limit=4, filter_metadata=en, prefilter=True)
    # different filters do not share a call, and neither masks the other's rows
    del calls[:]
    got = asyncio.run(many([en, de, en, de, en, None]))
    de_rows = tuple(r for r in range(N) if r % 10 == 1)
    assert sorted(calls, key=str) == sorted([("batch", 3, en_rows), ("batch", 2, de_rows), ("single", 1, None)], key=str), calls
    for q, f, res in zip(queries, [en, de, en, de, en, None], got):
        assert res == store.search(q, limit=4, filter_metadata=f, prefilter=True)
