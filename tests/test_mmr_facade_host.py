"""MMR search, host side of the facade (no GPU): ``VectorStore.search_mmr`` over a stub shard that answers the call as the
library defines it, in numpy float32 -- pick order and relevance scores come back, ``fetch_k`` defaults to 4 * limit, two
shards are refused with the reason, a filter always travels as the row mask, the threshold cut, the REST field, and the
``_async`` forms agree with the blocking ones."""
import asyncio
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mmr_harness as MH
from wdbx_amd import api
from wdbx_amd.config import WDBXConfig
from wdbx_amd.vector_store import VectorStore

D, N = 8, 90


def _pack(allowed):
    bits = np.zeros((len(allowed) + 31) // 32 * 32, bool)
    bits[: len(allowed)] = allowed
    return np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).ravel()


def _unpack(words, n):
    return ((words[np.arange(n) // 32] >> (np.arange(n) % 32).astype(np.uint32)) & 1).astype(bool)


def _mmr(rows, allowed, q, limit, fetch_k, lam):
    """[(row, relevance, value)] in pick order: the pool by (score descending, row), the float32 loop of tests/mmr_harness.py"""
    s = (rows @ np.asarray(q, np.float32)).astype(np.float32)
    ids = np.flatnonzero(allowed)
    pool = ids[np.lexsort((ids, -s[ids]))][:fetch_k]
    c = rows[pool]
    pos, val = MH.greedy_f32(s[pool], (c @ c.T).astype(np.float32), lam, limit)
    return [(int(pool[p]), float(s[pool[p]]), float(v)) for p, v in zip(pos, val)]


class _Shard:
    def __init__(self, rows, tag):
        self.rows, self.tag = rows, tag
        self.next_index = len(rows)
        self.calls = []  # (limit, fetch_k, lambda, mask given)
        self.swallow_errors = False

    def _id(self, r):
        return f"{self.tag}v{r}"

    def search_mmr(self, q, limit=10, fetch_k=None, lambda_mult=0.5, mask=None):
        assert mask is None or mask.dtype == np.uint32
        assert isinstance(q, np.ndarray) and q.shape == (D,)
        self.calls.append((limit, fetch_k, lambda_mult, mask is not None))
        allowed = np.ones(len(self.rows), bool) if mask is None else _unpack(mask, len(self.rows))
        pool = min(2048, 4 * limit) if fetch_k is None else fetch_k
        return [(self._id(r), s, v) for r, s, v in _mmr(self.rows, allowed, q, limit, pool, lambda_mult)]

    def row_mask_for(self, predicate):
        return _pack(np.array([predicate(self._id(r)) for r in range(len(self.rows))]))


def _store(tags=("a",)):
    rng = np.random.default_rng(12)
    vs = VectorStore.__new__(VectorStore)
    vs.indices = []
    vs.metadata = {}
    vs.vectors = {}
    vs._bulk_id_shard, vs._bulk_ranges = {}, []
    vs._label_ids = {}
    vs.config = WDBXConfig({})
    for tag in tags:
        rows = rng.standard_normal((N, D)).astype(np.float32)
        rows[40:50] = rows[3] + 0.01 * rng.standard_normal((10, D)).astype(np.float32)  # ten near-duplicates of row 3
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        vs.indices.append(_Shard(rows, tag))
        for r in range(N):
            vs.metadata[f"{tag}v{r}"] = {"lang": "en" if r % 5 else "de"}
            vs._bulk_id_shard[f"{tag}v{r}"] = len(vs.indices) - 1
    vs.num_shards = len(tags)
    vs.vector_dim = D
    vs._mask_cache, vs._meta_version = {}, 0
    vs._pending, vs._drain_task = [], None
    vs._group = False
    vs._sync_lock, vs._sync_pending, vs._sync_busy, vs._sync_coalesce, vs._sync_last_batch = threading.Lock(), [], False, False, 0
    vs._group_lock, vs._group_verified, vs._group_path, vs.last_search_path = threading.Lock(), False, "copy_group", ""
    vs.thread_pool = ThreadPoolExecutor(max_workers=4)
    vs._shard_pool = ThreadPoolExecutor(max_workers=2)
    return vs


@pytest.fixture()
def store():
    return _store()


def _query(store):
    q = store.indices[0].rows[3] + np.float32(0.3) * np.random.default_rng(5).standard_normal(D).astype(np.float32)
    return (q / np.linalg.norm(q)).astype(np.float32)


def _brute(store, q, limit, fetch_k, lam, threshold=0.0, flt=None):
    ix = store.indices[0]
    allowed = np.array([not flt or all(store.metadata[ix._id(r)].get(k) == v for k, v in flt.items()) for r in range(N)])
    picks = _mmr(ix.rows, allowed, q, limit, fetch_k, lam)
    return [(ix._id(r), s) for r, s, _ in picks if not (threshold > 0 and s < threshold)][:limit]


def _same(got, want, store):
    assert [(g[0], g[1]) for g in got] == want
    assert all(g[2] == store.metadata[g[0]] for g in got)


@pytest.mark.parametrize("limit,fetch_k,lam", [(1, None, 0.5), (5, None, 0.5), (5, 40, 0.25), (10, 10, 0.0), (10, 90, 1.0)])
def test_picks_come_back_in_pick_order_with_relevance_scores(store, limit, fetch_k, lam):
    q = _query(store)
    got = store.search_mmr(q.tolist(), limit=limit, fetch_k=fetch_k, lambda_mult=lam)
    _same(got, _brute(store, q, limit, min(2048, 4 * limit) if fetch_k is None else fetch_k, lam), store)
    assert store.indices[0].calls[-1] == (limit, fetch_k, lam, False)
    assert asyncio.run(store.search_mmr_async(q.tolist(), limit=limit, fetch_k=fetch_k, lambda_mult=lam)) == got


def test_the_answer_is_diversified(store):
    q = _query(store)
    plain = store.search_mmr(q.tolist(), limit=5, fetch_k=40, lambda_mult=1.0)
    dups = {f"av{r}" for r in [3, *range(40, 50)]}
    assert {g[0] for g in plain} <= dups                               # relevance alone: the duplicates
    mixed = store.search_mmr(q.tolist(), limit=5, fetch_k=40, lambda_mult=0.5)
    assert mixed[0] == plain[0] and len({g[0] for g in mixed} - dups) >= 3
    assert [g[1] for g in plain] == sorted((g[1] for g in plain), reverse=True)
    assert [g[1] for g in mixed] != sorted((g[1] for g in mixed), reverse=True)  # pick order, not score order


def test_two_shards_are_refused_with_the_reason():
    vs = _store(tags=("a", "b"))
    q = _query(vs)
    with pytest.raises(ValueError, match=r"one shard.*both rows on one device.*do not compose"):
        vs.search_mmr(q.tolist(), limit=5)
    with pytest.raises(ValueError, match="one shard"):
        asyncio.run(vs.search_mmr_async(q.tolist(), limit=5))
    assert all(ix.calls == [] for ix in vs.indices)


def test_bad_arguments_are_refused(store):
    q = _query(store).tolist()
    with pytest.raises(ValueError, match="dimension"):
        store.search_mmr(q + [0.0], limit=5)
    for lam in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="lambda_mult"):
            store.search_mmr(q, limit=5, lambda_mult=lam)
    with pytest.raises(ValueError, match="fetch_k"):
        store.search_mmr(q, limit=5, fetch_k=4)
    assert store.indices[0].calls == []


def test_a_filter_always_travels_as_the_mask(store):
    q = _query(store)
    flt = {"lang": "de"}
    got = store.search_mmr(q.tolist(), limit=6, fetch_k=12, lambda_mult=0.5, filter_metadata=flt)
    assert store.indices[0].calls == [(6, 12, 0.5, True)]  # whatever FILTER_PUSHDOWN says (default False)
    _same(got, _brute(store, q, 6, 12, 0.5, flt=flt), store)
    assert len(got) == 6 and all(g[2]["lang"] == "de" for g in got)
    assert asyncio.run(store.search_mmr_async(q.tolist(), limit=6, fetch_k=12, lambda_mult=0.5, filter_metadata=flt)) == got


def test_threshold_cuts_by_relevance(store):
    q = _query(store)
    full = store.search_mmr(q.tolist(), limit=10, fetch_k=40, lambda_mult=0.5)
    scores = sorted(g[1] for g in full)
    t = (scores[4] + scores[5]) / 2
    assert t > 0
    cut = store.search_mmr(q.tolist(), limit=10, fetch_k=40, lambda_mult=0.5, threshold=t)
    assert cut == [g for g in full if g[1] >= t] and len(cut) == 5
    _same(cut, _brute(store, q, 10, 40, 0.5, threshold=t), store)
    assert store.search_mmr(q.tolist(), limit=10, fetch_k=40, lambda_mult=0.5, threshold=0.0) == full
    assert store.search_mmr(q.tolist(), limit=10, fetch_k=40, lambda_mult=0.5, threshold=100.0) == []


def test_rest_field(store):
    class _W:
        async def vector_search_async(self, query, limit, threshold, flt):
            return [("plain", 1.0, {})]

        async def vector_search_mmr_async(self, query, limit, fetch_k, lambda_mult, threshold, flt):
            return await store.search_mmr_async(query, limit=limit, fetch_k=fetch_k, lambda_mult=lambda_mult, threshold=threshold,
                                                filter_metadata=flt)

    q = _query(store)
    body = {"query_vector": q.tolist(), "limit": 5, "filter_metadata": {"lang": "en"}, "mmr": {"lambda": 0.25, "fetch_k": 40}}
    res = asyncio.run(api.search_endpoint(_W(), body))["results"]
    want = _brute(store, q, 5, 40, 0.25, flt={"lang": "en"})
    assert [(r["vector_id"], r["similarity"]) for r in res] == want
    assert store.indices[0].calls[-1] == (5, 40, 0.25, True)
    # the members are optional: lambda 0.5, fetch_k left to the store
    asyncio.run(api.search_endpoint(_W(), dict(body, mmr={})))
    assert store.indices[0].calls[-1] == (5, None, 0.5, True)
    # absent or null: the plain search
    assert asyncio.run(api.search_endpoint(_W(), {"query_vector": q.tolist()}))["results"][0]["vector_id"] == "plain"
    assert asyncio.run(api.search_endpoint(_W(), {"query_vector": q.tolist(), "mmr": None}))["results"][0]["vector_id"] == "plain"
    for bad in (True, 0.5, [], {"lambda": 2}, {"lambda": "x"}, {"lambda": True}, {"fetch_k": 4}, {"fetch_k": 1.5}, {"k": 3}):
        with pytest.raises(ValueError):
            asyncio.run(api.search_endpoint(_W(), dict(body, mmr=bad)))
    with pytest.raises(ValueError, match="query_vector alone"):
        asyncio.run(api.search_endpoint(_W(), dict(body, distinct=True)))
    with pytest.raises(ValueError, match="query_vector alone"):
        asyncio.run(api.search_endpoint(_W(), dict(body, query_vectors=[q.tolist()])))
