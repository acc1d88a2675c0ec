"""Recommend search, host side of the facade (no GPU): ``VectorStore.recommend`` over stub shards that answer the call as the
library defines it, in numpy float32 -- id examples are resolved with ``get`` and excluded on the shard that holds them, the
cross-shard merge order, a filter always travels as the row masks, ``average_vector`` goes through the plain search, the REST
body, and the ``_async`` forms agree with the blocking ones."""
import asyncio
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from wdbx_amd import api
from wdbx_amd.config import WDBXConfig
from wdbx_amd.vector_store import VectorStore

D, N = 8, 60
_F32 = np.float32


def _pack(allowed):
    bits = np.zeros((len(allowed) + 31) // 32 * 32, bool)
    bits[: len(allowed)] = allowed
    return np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).ravel()


def _unpack(words, n):
    return ((words[np.arange(n) // 32] >> (np.arange(n) % 32).astype(np.uint32)) & 1).astype(bool)


def _fold(rows, allowed, pos, neg):
    """[(row, score, side)] of every allowed row, favoured first by (p descending, row), then the others by (n ascending, row)"""
    p = np.max(np.stack([rows @ v for v in pos]), axis=0).astype(_F32)
    n = np.max(np.stack([rows @ v for v in neg]), axis=0).astype(_F32) if len(neg) else np.full(len(rows), -np.inf, _F32)
    ids = np.flatnonzero(allowed)
    fav = [r for r in ids if p[r] > n[r]]
    dis = [r for r in ids if not p[r] > n[r]]
    fav.sort(key=lambda r: (-p[r], r))
    dis.sort(key=lambda r: (n[r], r))
    return [(int(r), float(p[r]), 1) for r in fav] + [(int(r), float(n[r]), 0) for r in dis]


class _Shard:
    def __init__(self, rows, tag):
        self.rows, self.tag = rows, tag
        self.next_index = len(rows)
        self.calls = []  # (positives, negatives, limit, mask given, sorted exclude ids)
        self.swallow_errors = False

    def _id(self, r):
        return f"{self.tag}v{r}"

    def _row_of(self, vector_id):  # (the store's own get asks the shard for an id it does not hold in memory)
        tail = vector_id[len(self.tag) + 1:]
        return int(tail) if vector_id.startswith(self.tag + "v") and tail.isdigit() and int(tail) < len(self.rows) else None

    def recommend(self, positives, negatives=(), limit=10, mask=None, exclude_ids=()):
        assert mask is None or mask.dtype == np.uint32
        assert all(isinstance(v, np.ndarray) and v.shape == (D,) for v in list(positives) + list(negatives))
        self.calls.append((len(positives), len(negatives), limit, mask is not None, sorted(exclude_ids)))
        allowed = np.ones(len(self.rows), bool) if mask is None else _unpack(mask, len(self.rows))
        for vid in exclude_ids:
            assert vid.startswith(self.tag + "v")  # (only the ids this shard holds)
            allowed[int(vid[len(self.tag) + 1:])] = False
        return [(self._id(r), s, side) for r, s, side in _fold(self.rows, allowed, positives, negatives)[:limit]]

    def row_mask_for(self, predicate):
        return _pack(np.array([predicate(self._id(r)) for r in range(len(self.rows))]))


def _store(tags=("a",)):
    rng = np.random.default_rng(21)
    vs = VectorStore.__new__(VectorStore)
    vs.indices = []
    vs.metadata = {}
    vs.vectors = {}
    vs._bulk_id_shard, vs._bulk_ranges = {}, []
    vs._label_ids = {}
    vs.config = WDBXConfig({})
    for tag in tags:
        rows = rng.standard_normal((N, D)).astype(_F32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        vs.indices.append(_Shard(rows, tag))
        for r in range(N):
            vs.metadata[f"{tag}v{r}"] = {"lang": "en" if r % 3 else "de"}
            vs._bulk_id_shard[f"{tag}v{r}"] = len(vs.indices) - 1
            vs.vectors[f"{tag}v{r}"] = rows[r]
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


def _brute(store, pos, neg, limit, exclude=(), flt=None):
    """the merge from the definition over ALL shards' rows: favoured by (score descending, shard, row), then n ascending"""
    fav, dis = [], []
    for s, ix in enumerate(store.indices):
        allowed = np.array([ix._id(r) not in exclude and (not flt or all(store.metadata[ix._id(r)].get(k) == v for k, v in flt.items()))
                            for r in range(N)])
        for r, score, side in _fold(ix.rows, allowed, pos, neg):
            (fav if side else dis).append((score, s, r, ix._id(r)))
    fav.sort(key=lambda t: (-t[0], t[1], t[2]))
    dis.sort(key=lambda t: (t[0], t[1], t[2]))
    return [(vid, score, 1) for score, _, _, vid in fav][:limit] + [(vid, score, 0) for score, _, _, vid in dis][:max(0, limit - len(fav))]


def _vec(rng):
    v = rng.standard_normal(D).astype(_F32)
    return v / np.linalg.norm(v)


@pytest.mark.parametrize("tags", [("a",), ("a", "b"), ("a", "b", "c")])
@pytest.mark.parametrize("limit", [1, 7, 200])
def test_ids_are_resolved_excluded_per_shard_and_the_merge_is_ordered(tags, limit):
    store = _store(tags)
    rng = np.random.default_rng(len(tags) * 10 + limit)
    last = tags[-1]
    positive = ["av3", _vec(rng).tolist(), f"{last}v7"]
    negative = [f"{last}v11", _vec(rng).tolist()]
    pos = [store.indices[0].rows[3], np.asarray(positive[1], _F32), store.indices[-1].rows[7]]
    neg = [store.indices[-1].rows[11], np.asarray(negative[1], _F32)]
    got = store.recommend(positive, negative, limit=limit, with_side=True)
    want = _brute(store, pos, neg, limit, exclude={"av3", f"{last}v7", f"{last}v11"})
    assert [(g[0], g[1], g[3]) for g in got] == want
    assert all(g[2] == store.metadata[g[0]] for g in got)
    assert not {g[0] for g in got} & {"av3", f"{last}v7", f"{last}v11"}
    for s, ix in enumerate(store.indices):
        held = sorted(v for v in ("av3", f"{last}v7", f"{last}v11") if v.startswith(ix.tag + "v"))
        assert ix.calls == [(3, 2, limit, False, held)]
    sides = [g[3] for g in got]
    assert sides == sorted(sides, reverse=True)  # (every favoured result before every disfavoured one)
    plain = store.recommend(positive, negative, limit=limit)
    assert plain == [g[:3] for g in got]
    assert asyncio.run(store.recommend_async(positive, negative, limit=limit, with_side=True)) == got


def test_a_negative_equal_to_the_positive_disfavours_everything():
    store = _store(("a", "b"))
    v = _vec(np.random.default_rng(2)).tolist()
    got = store.recommend([v], [v], limit=9, with_side=True)
    assert len(got) == 9 and all(g[3] == 0 for g in got)
    assert [g[1] for g in got] == sorted(g[1] for g in got)  # (n ascending: farthest from the negative first)


def test_a_filter_always_travels_as_the_masks():
    store = _store(("a", "b"))
    rng = np.random.default_rng(3)
    v, w = _vec(rng), _vec(rng)
    flt = {"lang": "de"}
    got = store.recommend([v.tolist()], [w.tolist()], limit=12, filter_metadata=flt, with_side=True)
    assert all(ix.calls == [(1, 1, 12, True, [])] for ix in store.indices)  # whatever FILTER_PUSHDOWN says (default False)
    assert [(g[0], g[1], g[3]) for g in got] == _brute(store, [v], [w], 12, flt=flt)
    assert len(got) == 12 and all(g[2]["lang"] == "de" for g in got)


def test_bad_arguments_are_refused():
    store = _store()
    v = _vec(np.random.default_rng(4)).tolist()
    with pytest.raises(ValueError, match="at least one positive"):
        store.recommend([], [v])
    with pytest.raises(ValueError, match=r"positive\[1\].*no stored vector has the id 'nope'"):
        store.recommend([v, "nope"])
    with pytest.raises(ValueError, match=r"negative\[0\].*dimension"):
        store.recommend([v], [v + [0.0]])
    with pytest.raises(ValueError, match="strategy"):
        store.recommend([v], strategy="sum_scores")
    with pytest.raises(ValueError, match="65 examples, at most 64"):
        store.recommend([v] * 33, [v] * 32)
    assert store.indices[0].calls == []


def test_average_vector_goes_through_the_plain_search():
    store = _store(("a", "b"))
    rng = np.random.default_rng(5)
    seen = []

    def search(query_vector, limit=10, threshold=0.0, filter_metadata=None, prefilter=None):
        seen.append((np.asarray(query_vector, _F32), limit, threshold, filter_metadata, prefilter))
        return [("av5", 0.9, {}), ("x1", 0.8, {}), ("bv2", 0.7, {}), ("x2", 0.6, {}), ("x3", 0.5, {}), ("x4", 0.4, {})]

    store.search = search
    v, w = _vec(rng), _vec(rng)
    got = store.recommend(["av5", v.tolist()], ["bv2", w.tolist()], limit=3, strategy="average_vector", with_side=True)
    assert got == [("x1", 0.8, {}, 1), ("x2", 0.6, {}, 1), ("x3", 0.5, {}, 1)]  # (the id examples dropped, then the cut)
    (q, limit, threshold, flt, prefilter), = seen
    avg_p = np.mean(np.stack([store.indices[0].rows[5], v]), axis=0, dtype=_F32)
    avg_n = np.mean(np.stack([store.indices[1].rows[2], w]), axis=0, dtype=_F32)
    assert np.array_equal(q, avg_p + (avg_p - avg_n)) and (limit, threshold, flt, prefilter) == (3 + 2, 0.0, None, None)
    assert all(ix.calls == [] for ix in store.indices)
    store.recommend([v.tolist()], limit=2, strategy="average_vector", filter_metadata={"lang": "en"})
    q, limit, _, flt, prefilter = seen[-1]
    assert np.array_equal(q, v) and (limit, flt, prefilter) == (2, {"lang": "en"}, True)  # (the filter as the row masks)


def test_rest_body():
    store = _store(("a", "b"))

    class _W:
        async def vector_recommend_async(self, positive, negative=None, limit=10, strategy="best_score", filter_metadata=None,
                                         with_side=False):
            return await store.recommend_async(positive, negative, limit=limit, strategy=strategy, filter_metadata=filter_metadata,
                                               with_side=with_side)

    v = _vec(np.random.default_rng(6))
    body = {"positive": ["av3", v.tolist()], "negative": ["bv4"], "limit": 5, "filter_metadata": {"lang": "en"}}
    res = asyncio.run(api.recommend_endpoint(_W(), body))["results"]
    want = _brute(store, [store.indices[0].rows[3], v], [store.indices[1].rows[4]], 5, exclude={"av3", "bv4"}, flt={"lang": "en"})
    assert [(r["vector_id"], r["similarity"], r["side"]) for r in res] == want
    assert all(r["metadata"] == store.metadata[r["vector_id"]] for r in res)
    # negative, limit, strategy and the filter are optional; null means the default
    res = asyncio.run(api.recommend_endpoint(_W(), {"positive": [v.tolist()], "negative": None, "limit": None, "strategy": None}))
    assert len(res["results"]) == 10 and store.indices[0].calls[-1] == (1, 0, 10, False, [])
    for bad in ({}, {"positive": []}, {"positive": "av3"}, {"positive": [["x"]]}, {"positive": [True]},
                dict(body, negative="bv4"), dict(body, limit="5"), dict(body, limit=True), dict(body, strategy="sum"),
                dict(body, filter_metadata=[1])):
        with pytest.raises(ValueError):
            asyncio.run(api.recommend_endpoint(_W(), bad))
    with pytest.raises(ValueError):
        asyncio.run(api.recommend_endpoint(_W(), [1]))
