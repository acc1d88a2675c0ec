"""Distinct search, host side of the facade (no GPU): ``VectorStore.search_distinct`` over two stub shards that rank a small
corpus exactly in numpy and keep the labels they are given -- label interning across shards, the cross-shard dedupe and its
order (ties across shards included), the threshold, relabelling through ``update_metadata``, a filter always travelling as the
row mask, the REST field, and config ``DISTINCT_KEY=None``."""
import asyncio
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from wdbx_amd import _native, api
from wdbx_amd.config import WDBXConfig
from wdbx_amd.vector_store import VectorStore

D, N = 4, 60
NONE = _native.LABEL_NONE


def _pack(allowed):
    bits = np.zeros((len(allowed) + 31) // 32 * 32, bool)
    bits[: len(allowed)] = allowed
    return np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).ravel()


def _unpack(words, n):
    return ((words[np.arange(n) // 32] >> (np.arange(n) % 32).astype(np.uint32)) & 1).astype(bool)


class _Shard:
    """An exact shard over ``rows`` with ids ``<tag>v<row>`` that answers the distinct search as the library defines it."""

    def __init__(self, rows, tag):
        self.rows, self.tag = rows, tag
        self.next_index = len(rows)
        self.labels = np.full(len(rows), NONE, np.uint64)
        self.calls = []  # (kind, mask given)
        self.swallow_errors = False

    def _id(self, r):
        return f"{self.tag}v{r}"

    def _row_of(self, vid):
        head = self.tag + "v"
        if isinstance(vid, str) and vid.startswith(head) and vid[len(head):].isdigit() and int(vid[len(head):]) < len(self.rows):
            return int(vid[len(head):])
        return None

    def set_labels(self, vector_ids, labels):
        for vid, lab in zip(vector_ids, labels):
            assert 0 <= int(lab) <= NONE
            r = self._row_of(vid)
            if r is not None:
                self.labels[r] = int(lab)

    def _ranked(self, q, mask):
        s = self.rows @ np.asarray(q, np.float32)
        allowed = np.ones(len(s), bool) if mask is None else _unpack(mask, len(s))
        return s, [r for r in np.lexsort((np.arange(len(s)), -s)) if allowed[r]]

    def search_distinct(self, q, limit=10, mask=None):
        assert mask is None or mask.dtype == np.uint32
        self.calls.append(("distinct", mask is not None))
        s, order = self._ranked(q, mask)
        seen, out = set(), []
        for r in order:
            lab = int(self.labels[r])
            if lab != NONE:
                if lab in seen:
                    continue
                seen.add(lab)
            out.append((self._id(r), float(s[r]), lab))
            if len(out) == limit:
                break
        return out

    def search(self, q, limit=10, row_mask=None):
        self.calls.append(("single", row_mask is not None))
        s, order = self._ranked(q, row_mask)
        return [(self._id(r), float(s[r])) for r in order[:limit]]

    def row_mask_for(self, predicate):
        return _pack(np.array([predicate(self._id(r)) for r in range(len(self.rows))]))

    def add(self, vid, vec):
        assert self._row_of(vid) is not None  # (the stub's rows are fixed: storing names one of them)

    def batch_add(self, vecs):
        for vid in vecs:
            self.add(vid, None)


def _doc(tag, r):
    """documents span both shards: chunk (tag, r) belongs to document r % 12; every 10th row has no document"""
    return None if r % 10 == 9 else f"doc{r % 12}"


def _store(distinct_key="doc", label=True):
    rng = np.random.default_rng(11)
    vs = VectorStore.__new__(VectorStore)
    vs.indices = []
    vs.metadata = {}
    vs.vectors = {}
    vs._bulk_id_shard, vs._bulk_ranges = {}, []
    vs._label_ids = {}
    vs.config = WDBXConfig({"DISTINCT_KEY": distinct_key})
    for tag in ("a", "b"):
        rows = rng.standard_normal((N, D)).astype(np.float32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        vs.indices.append(_Shard(rows, tag))
        for r in range(N):
            doc = _doc(tag, r)
            vs.metadata[f"{tag}v{r}"] = {"lang": "en" if r % 5 else "de", **({"doc": doc} if doc else {})}
            vs._bulk_id_shard[f"{tag}v{r}"] = len(vs.indices) - 1
    vs.num_shards = 2
    vs.vector_dim = D
    vs._mask_cache, vs._meta_version = {}, 0
    vs._pending, vs._drain_task = [], None
    vs._group = False
    vs._sync_lock, vs._sync_pending, vs._sync_busy, vs._sync_coalesce, vs._sync_last_batch = threading.Lock(), [], False, False, 0
    vs._group_lock, vs._group_verified, vs._group_path, vs.last_search_path = threading.Lock(), False, "copy_group", ""
    vs.thread_pool = ThreadPoolExecutor(max_workers=4)
    vs._shard_pool = ThreadPoolExecutor(max_workers=2)
    if label:
        vs._push_labels(vs.metadata)  # (what loading a store does)
    return vs


@pytest.fixture()
def store():
    return _store()


def _query(seed=3):
    q = np.random.default_rng(seed).standard_normal(D).astype(np.float32)
    return q / np.linalg.norm(q)


def _brute(store, q, limit, threshold=0.0, flt=None):
    """every vector of both shards by (score descending, shard, row), the first of each document kept"""
    rows = []
    for shard, ix in enumerate(store.indices):
        s = ix.rows @ q
        rows += [(-float(s[r]), shard, r, ix._id(r)) for r in range(N)]
    seen, out = set(), []
    for neg, _, _, vid in sorted(rows):
        meta = store.metadata[vid]
        if flt and any(meta.get(k) != v for k, v in flt.items()):
            continue
        if threshold > 0 and -neg < threshold:
            break
        doc = meta.get("doc")
        if doc is not None:
            key = doc if isinstance(doc, (str, int)) else repr(doc)
            if key in seen:
                continue
            seen.add(key)
        out.append((vid, -neg))
        if len(out) == limit:
            break
    return out


def _same(got, want, store):
    assert [(g[0], g[1]) for g in got] == [(vid, pytest.approx(s, abs=1e-6)) for vid, s in want]
    assert all(g[2] == store.metadata[g[0]] for g in got)


def test_interning_is_one_table_for_all_shards(store):
    a, b = store.indices
    for r in range(N):
        if _doc("a", r) is None:
            assert a.labels[r] == NONE and b.labels[r] == NONE
        else:
            assert a.labels[r] == b.labels[r] != NONE          # the same document, the same label in both shards
            assert a.labels[r] == a.labels[r % 12] or r % 12 == 9
    assert len(store._label_ids) == 12                          # dense: one label per document
    assert sorted(store._label_ids.values()) == list(range(12))


def test_unhashable_values_are_interned_by_their_json_text(store):
    store.update_metadata("av0", {"doc": ["x", 1]})
    store.update_metadata("bv5", {"doc": ["x", 1]})
    store.update_metadata("bv6", {"doc": {"k": [2]}})
    a, b = store.indices
    assert a.labels[0] == b.labels[5] != NONE and b.labels[6] not in (NONE, a.labels[0])
    assert store._label_of({"doc": ["x", 1]}) == a.labels[0] and store._label_of({"other": 1}) == NONE


@pytest.mark.parametrize("limit", [1, 5, 12, 30])
def test_cross_shard_dedupe_and_order(store, limit):
    for seed in range(5):
        q = _query(seed)
        got = store.search_distinct(q.tolist(), limit=limit)
        _same(got, _brute(store, q, limit), store)
        docs = [g[2]["doc"] for g in got if "doc" in g[2]]
        assert len(docs) == len(set(docs))
    # every shard was asked once, for its own top-`limit` labels, without a mask
    assert all(ix.calls == [("distinct", False)] * 5 for ix in store.indices)
    # 12 documents + 6 unlabelled rows per shard: 24 results at the most
    assert len(store.search_distinct(_query().tolist(), limit=30)) == 24


def test_a_label_whose_best_rows_tie_across_shards_goes_to_the_lower_shard(store):
    a, b = store.indices
    q = np.full(D, 0.5, np.float32)            # (unit length, and every product and sum below is exact)
    a.rows[31] = b.rows[7] = q                 # document 7: the query itself in both shards, nothing scores higher
    got = store.search_distinct(q.tolist(), limit=24)
    hits = [g for g in got if g[2].get("doc") == "doc7"]
    assert len(hits) == 1 and hits[0][0] == "av31"  # (score, shard, row): shard a before shard b
    _same(got, _brute(store, q, 24), store)
    # two UNLABELLED rows with one score both stay, shard a first
    b.rows[9] = a.rows[9]
    got = store.search_distinct(q.tolist(), limit=24)
    ids = [g[0] for g in got]
    assert "av9" in ids and "bv9" in ids and ids.index("av9") + 1 == ids.index("bv9")
    _same(got, _brute(store, q, 24), store)


def test_threshold_is_applied_as_in_search(store):
    q = _query()
    full = store.search_distinct(q.tolist(), limit=24)
    t = (full[5][1] + full[6][1]) / 2
    cut = store.search_distinct(q.tolist(), limit=24, threshold=t)
    assert cut == full[:6]
    _same(cut, _brute(store, q, 24, threshold=t), store)
    assert store.search_distinct(q.tolist(), limit=24, threshold=0.0) == full    # 0 (and below) = no threshold, as search
    assert store.search_distinct(q.tolist(), limit=24, threshold=-1.0) == full
    assert store.search_distinct(q.tolist(), limit=24, threshold=2.0) == []


def test_update_metadata_relabels(store):
    q = _query()
    first = store.search_distinct(q.tolist(), limit=5)
    top, second = first[0][0], first[1][0]
    assert "doc" in store.metadata[top] and "doc" in store.metadata[second]
    # the best hit joins the second hit's document: the second hit disappears behind it
    assert store.update_metadata(top, dict(store.metadata[top], doc=store.metadata[second]["doc"]))
    got = store.search_distinct(q.tolist(), limit=5)
    assert got[0][0] == top and second not in [g[0] for g in got]
    _same(got, _brute(store, q, 5), store)
    # ... and leaves every document: it stands for itself, the second hit is back
    assert store.update_metadata(top, {"lang": "en"})
    shard = store.indices[0 if top.startswith("a") else 1]
    assert shard.labels[shard._row_of(top)] == NONE
    got = store.search_distinct(q.tolist(), limit=5)
    assert [g[0] for g in got[:2]] == [top, second]
    _same(got, _brute(store, q, 5), store)
    assert asyncio.run(store.update_metadata_async(top, {"doc": "brand new"}))
    assert shard.labels[shard._row_of(top)] == store._label_ids["brand new"]
    assert store.update_metadata("nobody", {"doc": "x"}) is False


def test_store_and_batch_store_push_labels():
    vs = _store(label=False)
    assert all((ix.labels == NONE).all() for ix in vs.indices)
    vs.store("av3", [0.0] * D, {"doc": "d1"})
    vs.batch_store({"bv4": [0.0] * D, "av5": [0.0] * D}, {"bv4": {"doc": "d1"}, "av5": {"doc": "d2"}})
    a, b = vs.indices
    assert a.labels[3] == b.labels[4] == vs._label_ids["d1"] and a.labels[5] == vs._label_ids["d2"]
    assert (a.labels != NONE).sum() == 2 and (b.labels != NONE).sum() == 1


def test_a_filter_always_travels_as_the_mask(store):
    q = _query()
    flt = {"lang": "de"}
    got = store.search_distinct(q.tolist(), limit=10, filter_metadata=flt)
    assert all(ix.calls == [("distinct", True)] for ix in store.indices)  # whatever FILTER_PUSHDOWN says (default False)
    assert got and all(g[2]["lang"] == "de" for g in got)
    _same(got, _brute(store, q, 10, flt=flt), store)
    # a document whose best chunk does not match is shown by its best MATCHING chunk, not dropped
    plain = {g[2].get("doc"): g[0] for g in store.search_distinct(q.tolist(), limit=24)}
    moved = [g for g in got if "doc" in g[2] and plain[g[2]["doc"]] != g[0]]
    assert moved
    assert asyncio.run(store.search_distinct_async(q.tolist(), limit=10, filter_metadata=flt)) == got


def test_rest_field(store):
    class _W:
        async def vector_search_async(self, query, limit, threshold, flt):
            return [("plain", 1.0, {})]

        async def vector_search_distinct_async(self, query, limit, threshold, flt):
            return await store.search_distinct_async(query, limit=limit, threshold=threshold, filter_metadata=flt)

    q = _query()
    body = {"query_vector": q.tolist(), "limit": 5, "distinct": True, "filter_metadata": {"lang": "en"}}
    res = asyncio.run(api.search_endpoint(_W(), body))["results"]
    assert [r["vector_id"] for r in res] == [vid for vid, _ in _brute(store, q, 5, flt={"lang": "en"})]
    for off in (False, None):
        assert asyncio.run(api.search_endpoint(_W(), dict(body, distinct=off)))["results"][0]["vector_id"] == "plain"
    assert asyncio.run(api.search_endpoint(_W(), {"query_vector": q.tolist()}))["results"][0]["vector_id"] == "plain"
    for bad in ("yes", 1, []):
        with pytest.raises(ValueError):
            asyncio.run(api.search_endpoint(_W(), dict(body, distinct=bad)))


def test_without_distinct_key_the_call_says_so_and_nothing_else_changes():
    vs = _store(distinct_key=None)
    assert all((ix.labels == NONE).all() for ix in vs.indices) and vs._label_ids == {}
    with pytest.raises(ValueError, match="DISTINCT_KEY"):
        vs.search_distinct(_query().tolist(), limit=5)
    with pytest.raises(ValueError, match="DISTINCT_KEY"):
        asyncio.run(vs.search_distinct_async(_query().tolist(), limit=5))
    # storing, updating and searching go on as before, and no shard hears of labels
    vs.store("av3", [0.0] * D, {"doc": "d1"})
    vs.update_metadata("av4", {"doc": "d1"})
    res = vs.search(_query().tolist(), limit=3)
    assert len(res) == 3 and all(kind == "single" for ix in vs.indices for kind, _ in ix.calls)
    assert all((ix.labels == NONE).all() for ix in vs.indices) and vs._label_ids == {}
    assert WDBXConfig({}).get("DISTINCT_KEY") is None
