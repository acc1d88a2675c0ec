"""One filter PER QUERY in a batch, host side (no GPU): ``VectorStore.search_batch(filter_metadata=[...])``, the facade and
the REST field.  The shard is a stub that ranks a small corpus exactly in numpy and honours row masks the way the library
does; it records every call, so the tests see that push-down makes ONE call per shard whatever the number of filters."""
import asyncio
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from wdbx_amd import api
from wdbx_amd.config import WDBXConfig
from wdbx_amd.indexing import RowList
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
        self.calls = []  # (kind, number of queries, number of masks)
        self.thread_pool = None
        self.swallow_errors = False
        self.supports_row_masks = True

    def _rank(self, q, limit, row_mask):
        s = self.rows @ np.asarray(q, np.float32)
        if isinstance(row_mask, RowList):
            allowed = np.zeros(len(s), bool)
            allowed[row_mask.rows.astype(np.int64)] = True
        else:
            allowed = np.ones(len(s), bool) if row_mask is None else _unpack(row_mask, len(s))
        order = [r for r in np.lexsort((np.arange(len(s)), -s)) if allowed[r]]
        return [(f"v{r}", float(s[r])) for r in order[:limit]]

    def search(self, q, limit=10, row_mask=None):
        self.calls.append(("single", 1, 0 if row_mask is None else 1))
        return self._rank(q, limit, row_mask)

    def search_batch(self, queries, limit=10, row_mask=None, row_masks=None, mask_of_query=None):
        if row_masks is not None:
            assert row_mask is None and len(mask_of_query) == len(queries)
            assert len(row_masks) <= 64 and all(-1 <= c < len(row_masks) for c in mask_of_query)  # what the library accepts
            self.calls.append(("multimask", len(queries), len(row_masks)))
            return [self._rank(q, limit, None if c < 0 else row_masks[c]) for q, c in zip(queries, mask_of_query)]
        self.calls.append(("batch", len(queries), 0 if row_mask is None else 1))
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


FILTERS = [{"lang": "en"}, None, {"lang": "de"}, {"lang": "en"}, {"lang": "xx"}, {}, {"lang": "de"}]


def test_pushed_down_list_is_one_call_and_equals_per_query_search(store):
    queries, limit = _queries(len(FILTERS)), 5
    got = store.search_batch(queries, limit=limit, filter_metadata=FILTERS, prefilter=True)
    assert store.indices[0].calls == [("multimask", len(FILTERS), 3)]  # three distinct filters, one call
    for q, flt, res in zip(queries, FILTERS, got):
        assert res == store.search(q, limit=limit, filter_metadata=flt, prefilter=True)
        assert all(r[2]["lang"] == flt["lang"] for r in res if flt)
    assert all(len(r) == limit for r in got)


def test_list_without_pushdown_post_filters_each_query_by_its_own_filter(store):
    queries, limit = _queries(len(FILTERS)), 5
    got = store.search_batch(queries, limit=limit, filter_metadata=FILTERS)
    assert store.indices[0].calls == [("batch", len(FILTERS), 0)]
    for q, flt, res in zip(queries, FILTERS, got):
        assert res == store.search(q, limit=limit, filter_metadata=flt)
    assert any(len(r) < limit for r in got), "the corpus is meant to make the post-filter under-return"


def test_dict_and_none_forms_are_unchanged(store):
    queries = _queries(4)
    store.search_batch(queries, limit=5, filter_metadata={"lang": "en"}, prefilter=True)
    store.search_batch(queries, limit=5)
    assert store.indices[0].calls == [("batch", 4, 1), ("batch", 4, 0)]


def test_a_list_of_nones_makes_no_masks(store):
    queries = _queries(3)
    assert store.search_batch(queries, limit=5, filter_metadata=[None] * 3, prefilter=True) == store.search_batch(queries, limit=5)
    assert store.indices[0].calls == [("batch", 3, 0), ("batch", 3, 0)]


def test_a_shard_with_a_row_list_keeps_one_call_per_filter(store):
    store.config = WDBXConfig({"FILTER_GATHER_MAX_ROWS": 8})  # "de" matches 6 rows: it travels as its rows
    queries, limit = _queries(len(FILTERS)), 5
    got = store.search_batch(queries, limit=limit, filter_metadata=FILTERS, prefilter=True)
    kinds = [c[0] for c in store.indices[0].calls]
    assert "multimask" not in kinds and kinds.count("batch") == 4  # none, en, de, xx
    for q, flt, res in zip(queries, FILTERS, got):
        assert res == store.search(q, limit=limit, filter_metadata=flt, prefilter=True)


def test_wrong_list_length_raises(store):
    with pytest.raises(ValueError):
        store.search_batch(_queries(3), limit=5, filter_metadata=[None, None], prefilter=True)
    with pytest.raises(ValueError):
        store.search_batch(_queries(3), limit=5, filter_metadata=[None] * 4)


def test_rest_batch_endpoint_passes_the_list_through(store):
    class _W:
        def vector_search_batch(self, queries, limit, threshold, flt, **extra):
            return store.search_batch(np.asarray(queries, np.float32), limit=limit, threshold=threshold, filter_metadata=flt, **extra)

    queries = _queries(3)
    body = {"query_vectors": queries.tolist(), "limit": 4, "filter_metadata": [{"lang": "en"}, None, {"lang": "de"}], "prefilter": True}
    out = asyncio.run(api.search_batch_endpoint(_W(), body))
    assert [len(r) for r in out["results"]] == [4, 4, 4]
    assert all(r["metadata"]["lang"] == "en" for r in out["results"][0]) and all(r["metadata"]["lang"] == "de" for r in out["results"][2])
    with pytest.raises(ValueError):
        asyncio.run(api.search_batch_endpoint(_W(), dict(body, filter_metadata=[None])))
    with pytest.raises(ValueError):
        asyncio.run(api.search_batch_endpoint(_W(), dict(body, filter_metadata=[1, 2, 3])))


def test_more_than_64_distinct_filters_go_in_groups_of_64(store):
    """One filter per user: 150 distinct filters in one batch.  The library takes 64 masks per call, so the shard sees three
    calls (64 + 64 + 22 filters; the queries without a filter ride with the first) and every answer is the per-query one."""
    store.metadata = {f"v{r}": {"user": r % 150} for r in range(N)}
    filters = [{"user": u} for u in range(150)] + [None, {"user": 3}, None]
    queries, limit = _queries(len(filters)), 3
    got = store.search_batch(queries, limit=limit, filter_metadata=filters, prefilter=True)
    assert store.indices[0].calls == [("multimask", 64 + 3, 64), ("multimask", 64, 64), ("multimask", 22, 22)]
    for q, flt, res in zip(queries, filters, got):
        assert res == store.search(q, limit=limit, filter_metadata=flt, prefilter=True)
        assert all(r[2]["user"] == flt["user"] for r in res if flt)


MIXED = [{"lang": "en"}, {"lang": "de"}, {"lang": "en"}, {"lang": "xx"}, {"lang": "de"}, {"lang": "xx"}]


def _six_async(store, queries):
    async def run():
        return await asyncio.gather(*[store.search_async(q.tolist(), limit=4, filter_metadata=f, prefilter=True)
                                      for q, f in zip(queries, MIXED)])
    return asyncio.run(run())


def test_async_coalesce_filters_is_one_multimask_call_with_the_one_at_a_time_answers(store):
    assert WDBXConfig({}).get("ASYNC_COALESCE_FILTERS") is False
    queries = _queries(6, seed=8)
    store.config = WDBXConfig({"ASYNC_COALESCE_FILTERS": True})
    got = _six_async(store, queries)
    assert store.indices[0].calls == [("multimask", 6, 3)]
    for q, f, res in zip(queries, MIXED, got):
        assert res == store.search(q, limit=4, filter_metadata=f, prefilter=True)


def test_async_default_keeps_one_call_per_filter(store):
    _six_async(store, _queries(6, seed=8))
    assert sorted(store.indices[0].calls) == [("batch", 2, 1)] * 3


def test_async_coalesce_filters_needs_the_method_on_every_index(store):
    store.config = WDBXConfig({"ASYNC_COALESCE_FILTERS": True})
    store.indices[0].supports_row_masks = False
    _six_async(store, _queries(6, seed=8))
    assert sorted(store.indices[0].calls) == [("batch", 2, 1)] * 3
