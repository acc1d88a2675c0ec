"""Multi-vector search, host side of the facade (no GPU): ``VectorStore.search_multivector`` over a stub shard that ranks a
small corpus by late interaction exactly in numpy and keeps the labels it is given -- config ``DISTINCT_KEY`` is required, two
shards are refused with the reason, a filter always travels as the row mask, the threshold cut, the REST field."""
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


def _maxsim(rows, labels, allowed, vectors):
    """[(first row of the label, fp32 sum folded in vector order, label)] in (sum descending, label order) -- labelled rows by
    label value, then every NONE row by row number; a label without an allowed row is absent"""
    groups = {}
    for r in range(len(rows)):
        groups.setdefault((0, int(labels[r]), 0) if labels[r] != NONE else (1, 0, r), []).append(r)
    out = []
    for pos, key in enumerate(sorted(groups)):
        live = [r for r in groups[key] if allowed[r]]
        if not live:
            continue
        total = np.float32(0.0)
        for v in vectors:
            total = np.float32(total + np.max(rows[live] @ np.asarray(v, np.float32)))
        out.append((-float(total), pos, groups[key][0], int(labels[groups[key][0]])))
    return [(first, -neg, lab) for neg, _, first, lab in sorted(out)]


class _Shard:
    """An exact shard over ``rows`` with ids ``<tag>v<row>`` that answers the multi-vector search as the library defines it."""

    def __init__(self, rows, tag):
        self.rows, self.tag = rows, tag
        self.next_index = len(rows)
        self.labels = np.full(len(rows), NONE, np.uint64)
        self.calls = []  # (kind, vectors, mask given)
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
            r = self._row_of(vid)
            if r is not None:
                self.labels[r] = int(lab)

    def search_multivector(self, vectors, limit=10, mask=None):
        assert mask is None or mask.dtype == np.uint32
        assert all(isinstance(v, np.ndarray) and v.shape == (D,) for v in vectors)
        self.calls.append(("multivector", len(vectors), mask is not None))
        allowed = np.ones(len(self.rows), bool) if mask is None else _unpack(mask, len(self.rows))
        return [(self._id(r), s, lab) for r, s, lab in _maxsim(self.rows, self.labels, allowed, vectors)[:limit]]

    def search(self, q, limit=10, row_mask=None):
        self.calls.append(("single", 1, row_mask is not None))
        s = self.rows @ np.asarray(q, np.float32)
        return [(self._id(r), float(s[r])) for r in np.lexsort((np.arange(len(s)), -s))[:limit]]

    def row_mask_for(self, predicate):
        return _pack(np.array([predicate(self._id(r)) for r in range(len(self.rows))]))


def _doc(r):
    """documents of five chunks, scattered; every 10th row has no document"""
    return None if r % 10 == 9 else f"doc{r % 12}"


def _store(distinct_key="doc", tags=("a",)):
    rng = np.random.default_rng(11)
    vs = VectorStore.__new__(VectorStore)
    vs.indices = []
    vs.metadata = {}
    vs.vectors = {}
    vs._bulk_id_shard, vs._bulk_ranges = {}, []
    vs._label_ids = {}
    vs.config = WDBXConfig({"DISTINCT_KEY": distinct_key})
    for tag in tags:
        rows = rng.standard_normal((N, D)).astype(np.float32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        vs.indices.append(_Shard(rows, tag))
        for r in range(N):
            doc = _doc(r)
            vs.metadata[f"{tag}v{r}"] = {"lang": "en" if r % 5 else "de", **({"doc": doc} if doc else {})}
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
    vs._push_labels(vs.metadata)  # (what loading a store does)
    return vs


@pytest.fixture()
def store():
    return _store()


def _queries(n=3, seed=3):
    q = np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _brute(store, qs, limit, threshold=0.0, flt=None):
    """documents by the metadata alone (no labels): (representative id, sum)"""
    ix = store.indices[0]
    docs = {}
    for r in range(N):
        meta = store.metadata[ix._id(r)]
        docs.setdefault(meta.get("doc", ("none", r)), []).append(r)
    out = []
    for key, members in docs.items():
        live = [r for r in members if not flt or all(store.metadata[ix._id(r)].get(k) == v for k, v in flt.items())]
        if not live:
            continue
        total = np.float32(0.0)
        for q in qs:
            total = np.float32(total + np.max(ix.rows[live] @ q))
        out.append((-float(total), members[0]))
    out = [(ix._id(r), -neg) for neg, r in sorted(out) if not (threshold > 0 and -neg < threshold)]
    return out[:limit]


def _same(got, want, store):
    assert [(g[0], g[1]) for g in got] == [(vid, pytest.approx(s, abs=1e-6)) for vid, s in want]
    assert all(g[2] == store.metadata[g[0]] for g in got)


@pytest.mark.parametrize("limit", [1, 5, 12, 30])
def test_documents_are_ranked_by_the_sum_of_per_vector_maxima(store, limit):
    for seed in range(4):
        qs = _queries(1 + seed, seed)
        got = store.search_multivector(qs.tolist(), limit=limit)
        _same(got, _brute(store, qs, limit), store)
        assert store.indices[0].calls[-1] == ("multivector", 1 + seed, False)
    # 12 documents + 6 unlabelled rows: 18 results at the most, each document once, shown by its first stored vector
    full = store.search_multivector(_queries().tolist(), limit=30)
    assert len(full) == 18 and len({g[0] for g in full}) == 18
    firsts = {}
    for r in range(N):
        if _doc(r) is not None:
            firsts.setdefault(_doc(r), f"av{r}")
    assert {g[0] for g in full if "doc" in g[2]} == set(firsts.values()) and firsts["doc9"] == "av21"


def test_distinct_key_is_required():
    vs = _store(distinct_key=None)
    with pytest.raises(ValueError, match="DISTINCT_KEY"):
        vs.search_multivector(_queries().tolist(), limit=5)
    with pytest.raises(ValueError, match="DISTINCT_KEY"):
        asyncio.run(vs.search_multivector_async(_queries().tolist(), limit=5))
    assert vs.indices[0].calls == []


def test_two_shards_are_refused_with_the_reason():
    vs = _store(tags=("a", "b"))
    with pytest.raises(ValueError, match=r"one shard.*hash of their id.*do not compose"):
        vs.search_multivector(_queries().tolist(), limit=5)
    with pytest.raises(ValueError, match="one shard"):
        asyncio.run(vs.search_multivector_async(_queries().tolist(), limit=5))
    assert all(ix.calls == [] for ix in vs.indices)


def test_bad_queries_are_refused(store):
    with pytest.raises(ValueError, match="empty"):
        store.search_multivector([], limit=5)
    with pytest.raises(ValueError, match="dimension"):
        store.search_multivector([[0.0] * D, [0.0] * (D + 1)], limit=5)


def test_a_filter_always_travels_as_the_mask(store):
    qs = _queries(4)
    flt = {"lang": "de"}
    got = store.search_multivector(qs.tolist(), limit=10, filter_metadata=flt)
    assert store.indices[0].calls == [("multivector", 4, True)]  # whatever FILTER_PUSHDOWN says (default False)
    _same(got, _brute(store, qs, 10, flt=flt), store)
    # only matching vectors stand for their document: its sum changes, and a document without a match is gone
    plain = dict((g[0], g[1]) for g in store.search_multivector(qs.tolist(), limit=30))
    assert got and len(got) < len(plain) and any(plain[g[0]] != g[1] for g in got)
    assert asyncio.run(store.search_multivector_async(qs.tolist(), limit=10, filter_metadata=flt)) == got


def test_threshold_is_applied_as_in_search(store):
    qs = _queries(3)
    full = store.search_multivector(qs.tolist(), limit=18)
    assert full[5][1] > full[6][1] > 0
    t = (full[5][1] + full[6][1]) / 2
    cut = store.search_multivector(qs.tolist(), limit=18, threshold=t)
    assert cut == full[:6]
    _same(cut, _brute(store, qs, 18, threshold=t), store)
    assert store.search_multivector(qs.tolist(), limit=18, threshold=0.0) == full    # 0 (and below) = no threshold, as search
    assert store.search_multivector(qs.tolist(), limit=18, threshold=-1.0) == full
    assert store.search_multivector(qs.tolist(), limit=18, threshold=100.0) == []


def test_rest_field(store):
    class _W:
        async def vector_search_async(self, query, limit, threshold, flt):
            return [("plain", 1.0, {})]

        async def vector_search_multivector_async(self, queries, limit, threshold, flt):
            return await store.search_multivector_async(queries, limit=limit, threshold=threshold, filter_metadata=flt)

    qs = _queries(3)
    body = {"query_vectors": qs.tolist(), "limit": 5, "filter_metadata": {"lang": "en"}}
    res = asyncio.run(api.search_endpoint(_W(), body))["results"]
    want = _brute(store, qs, 5, flt={"lang": "en"})
    assert [r["vector_id"] for r in res] == [vid for vid, _ in want]
    assert [r["similarity"] for r in res] == [pytest.approx(s, abs=1e-6) for _, s in want]
    # absent or null: the plain search
    assert asyncio.run(api.search_endpoint(_W(), {"query_vector": qs[0].tolist()}))["results"][0]["vector_id"] == "plain"
    assert asyncio.run(api.search_endpoint(_W(), {"query_vector": qs[0].tolist(), "query_vectors": None}))["results"][0]["vector_id"] == "plain"
    for bad in ("yes", 1, [], [1.0, 2.0], [[1.0, "x"]], [[1.0], 2.0]):
        with pytest.raises(ValueError):
            asyncio.run(api.search_endpoint(_W(), dict(body, query_vectors=bad)))
    with pytest.raises(ValueError, match="stands alone"):
        asyncio.run(api.search_endpoint(_W(), dict(body, query_vector=qs[0].tolist())))
    with pytest.raises(ValueError, match="stands alone"):
        asyncio.run(api.search_endpoint(_W(), dict(body, distinct=True)))
