"""Discovery search, host side of the facade (no GPU): ``VectorStore.discover`` over stub shards that answer the call as the
library defines it, in numpy float32 -- ids and raw vectors mixed in the target and the pairs, ids resolved with ``get`` and
excluded on the shard that holds them, the cross-shard merge order of both modes, a filter always travels as the row masks,
the REST body, and the ``_async`` forms agree with the blocking ones."""
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


def _fold(rows, allowed, target, pairs):
    """[(row, score, wins)] of every allowed row in the contract's order: (wins descending, target score descending, row) with a
    target, (loss descending, row) without"""
    wins = np.zeros(len(rows), int)
    loss = np.zeros(len(rows), _F32)
    for p, n in pairs:
        rp, rn = (rows @ p).astype(_F32), (rows @ n).astype(_F32)
        wins += rp > rn
        loss = (loss + np.fmin(rp - rn, _F32(0))).astype(_F32)
    ids = [int(r) for r in np.flatnonzero(allowed)]
    if target is None:
        ids.sort(key=lambda r: (-loss[r], r))
        return [(r, float(loss[r]), 0) for r in ids]
    t = (rows @ target).astype(_F32)
    ids.sort(key=lambda r: (-wins[r], -t[r], r))
    return [(r, float(t[r]), int(wins[r])) for r in ids]


class _Shard:
    def __init__(self, rows, tag):
        self.rows, self.tag = rows, tag
        self.next_index = len(rows)
        self.calls = []  # (target given, pairs, limit, mask given, sorted exclude ids)
        self.swallow_errors = False

    def _id(self, r):
        return f"{self.tag}v{r}"

    def _row_of(self, vector_id):  # (the store's own get asks the shard for an id it does not hold in memory)
        tail = vector_id[len(self.tag) + 1:]
        return int(tail) if vector_id.startswith(self.tag + "v") and tail.isdigit() and int(tail) < len(self.rows) else None

    def discover(self, target, pairs, limit=10, mask=None, exclude_ids=()):
        assert mask is None or mask.dtype == np.uint32
        flat = [v for pair in pairs for v in pair] + ([] if target is None else [target])
        assert all(isinstance(v, np.ndarray) and v.shape == (D,) for v in flat)
        self.calls.append((target is not None, len(pairs), limit, mask is not None, sorted(exclude_ids)))
        allowed = np.ones(len(self.rows), bool) if mask is None else _unpack(mask, len(self.rows))
        for vid in exclude_ids:
            assert vid.startswith(self.tag + "v")  # (only the ids this shard holds)
            allowed[int(vid[len(self.tag) + 1:])] = False
        return [(self._id(r), s, w) for r, s, w in _fold(self.rows, allowed, target, pairs)[:limit]]

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


def _brute(store, target, pairs, limit, exclude=(), flt=None):
    """the merge from the definition over ALL shards' rows: (wins descending, score descending, shard, row)"""
    every = []
    for s, ix in enumerate(store.indices):
        allowed = np.array([ix._id(r) not in exclude and (not flt or all(store.metadata[ix._id(r)].get(k) == v for k, v in flt.items()))
                            for r in range(N)])
        every += [(-wins, -score, s, r, ix._id(r)) for r, score, wins in _fold(ix.rows, allowed, target, pairs)]
    every.sort()
    return [(vid, -neg_score, -neg_wins) for neg_wins, neg_score, _, _, vid in every][:limit]


def _vec(rng):
    v = rng.standard_normal(D).astype(_F32)
    return v / np.linalg.norm(v)


@pytest.mark.parametrize("tags", [("a",), ("a", "b"), ("a", "b", "c")])
@pytest.mark.parametrize("limit", [1, 7, 200])
@pytest.mark.parametrize("with_target", [True, False])
def test_ids_are_resolved_excluded_per_shard_and_the_merge_is_ordered(tags, limit, with_target):
    store = _store(tags)
    rng = np.random.default_rng(len(tags) * 10 + limit)
    last = tags[-1]
    raw = [_vec(rng) for _ in range(3)]
    context = [("av3", raw[0].tolist()), (raw[1].tolist(), f"{last}v11"), {"positive": f"{last}v7", "negative": "av5"}]
    pairs = [(store.indices[0].rows[3], raw[0]), (raw[1], store.indices[-1].rows[11]),
             (store.indices[-1].rows[7], store.indices[0].rows[5])]
    ids = {"av3", f"{last}v11", f"{last}v7", "av5"}
    target, tvec = None, None
    if with_target:
        target, tvec = ("av9", store.indices[0].rows[9]) if limit != 7 else (raw[2].tolist(), raw[2])
        if limit != 7:
            ids.add("av9")
    got = store.discover(target, context, limit=limit, with_wins=True)
    want = _brute(store, tvec, pairs, limit, exclude=ids)
    assert [(g[0], g[1], g[3]) for g in got] == want
    assert all(g[2] == store.metadata[g[0]] for g in got)
    assert not {g[0] for g in got} & ids
    for ix in store.indices:
        held = sorted(v for v in ids if v.startswith(ix.tag + "v"))
        assert ix.calls == [(with_target, 3, limit, False, held)]
    wins = [g[3] for g in got]
    assert wins == sorted(wins, reverse=True)
    if not with_target:
        assert all(g[3] == 0 and g[1] <= 0 for g in got)
        assert [g[1] for g in got] == sorted((g[1] for g in got), reverse=True)  # (loss descending)
    assert store.discover(target, context, limit=limit) == [g[:3] for g in got]
    assert asyncio.run(store.discover_async(target, context, limit=limit, with_wins=True)) == got


def test_two_shards_equal_one_shard_of_the_same_rows():
    """the merged answer of two shards is the single shard's answer, up to the ids' shard tags"""
    two = _store(("a", "b"))
    one = _store(("a",))
    one.indices[0].rows = np.concatenate([ix.rows for ix in two.indices])
    one.indices[0].next_index = 2 * N
    rng = np.random.default_rng(7)
    pairs = [(_vec(rng).tolist(), _vec(rng).tolist()) for _ in range(3)]
    t = _vec(rng).tolist()
    name = lambda vid: int(vid[2:]) + (N if vid[0] == "b" else 0)  # noqa: E731
    for target in (t, None):
        got = two.discover(target, pairs, limit=25, with_wins=True)
        ref = one.indices[0].discover(None if target is None else np.asarray(target, _F32),
                                      [(np.asarray(p, _F32), np.asarray(n, _F32)) for p, n in pairs], 25)
        assert [(name(g[0]), g[1], g[3]) for g in got] == [(int(vid[2:]), s, w) for vid, s, w in ref]


def test_a_filter_always_travels_as_the_masks():
    store = _store(("a", "b"))
    rng = np.random.default_rng(3)
    v, w, t = _vec(rng), _vec(rng), _vec(rng)
    flt = {"lang": "de"}
    got = store.discover(t.tolist(), [(v.tolist(), w.tolist())], limit=12, filter_metadata=flt, with_wins=True)
    assert all(ix.calls == [(True, 1, 12, True, [])] for ix in store.indices)  # whatever FILTER_PUSHDOWN says (default False)
    assert [(g[0], g[1], g[3]) for g in got] == _brute(store, t, [(v, w)], 12, flt=flt)
    assert len(got) == 12 and all(g[2]["lang"] == "de" for g in got)


def test_bad_arguments_are_refused():
    store = _store()
    v = _vec(np.random.default_rng(4)).tolist()
    with pytest.raises(ValueError, match="a target or at least one context pair"):
        store.discover(None, [])
    with pytest.raises(ValueError, match=r"context\[1\].*no stored vector has the id 'nope'"):
        store.discover(v, [(v, v), (v, "nope")])
    with pytest.raises(ValueError, match=r"target\[0\].*dimension"):
        store.discover(v + [0.0], [(v, v)])
    with pytest.raises(ValueError, match=r"context\[0\]: a pair"):
        store.discover(v, [(v, v, v)])
    with pytest.raises(ValueError, match="33 context pairs, at most 32"):
        store.discover(v, [(v, v)] * 33)
    assert store.indices[0].calls == []
    assert store.discover(v, [(v, v)], limit=0) == []


def test_rest_body():
    store = _store(("a", "b"))

    class _W:
        async def vector_discover_async(self, target=None, context=(), limit=10, filter_metadata=None, with_wins=False):
            return await store.discover_async(target, context, limit=limit, filter_metadata=filter_metadata, with_wins=with_wins)

    rng = np.random.default_rng(6)
    v, w = _vec(rng), _vec(rng)
    body = {"target": v.tolist(), "context": [{"positive": "av3", "negative": w.tolist()}, ["bv4", "av8"]], "limit": 5,
            "filter_metadata": {"lang": "en"}}
    res = asyncio.run(api.discover_endpoint(_W(), body))["results"]
    pairs = [(store.indices[0].rows[3], w), (store.indices[1].rows[4], store.indices[0].rows[8])]
    want = _brute(store, v, pairs, 5, exclude={"av3", "bv4", "av8"}, flt={"lang": "en"})
    assert [(r["vector_id"], r["similarity"], r["wins"]) for r in res] == want
    assert all(r["metadata"] == store.metadata[r["vector_id"]] for r in res)
    # a context search: no target (absent or null); limit and the filter are optional, null means the default
    res = asyncio.run(api.discover_endpoint(_W(), {"target": None, "context": body["context"], "limit": None}))["results"]
    assert [(r["vector_id"], r["similarity"], r["wins"]) for r in res] == _brute(store, None, pairs, 10, exclude={"av3", "bv4", "av8"})
    assert store.indices[0].calls[-1] == (False, 2, 10, False, ["av3", "av8"])
    res = asyncio.run(api.discover_endpoint(_W(), {"target": "av1"}))["results"]
    assert len(res) == 10 and store.indices[0].calls[-1] == (True, 0, 10, False, ["av1"])
    for bad in ({}, {"context": []}, {"target": [["x"]]}, {"target": True}, dict(body, context="av3"), dict(body, context=[["av3"]]),
                dict(body, context=[{"positive": "av3"}]), dict(body, limit="5"), dict(body, limit=True),
                dict(body, filter_metadata=[1])):
        with pytest.raises(ValueError):
            asyncio.run(api.discover_endpoint(_W(), bad))
    with pytest.raises(ValueError):
        asyncio.run(api.discover_endpoint(_W(), [1]))
