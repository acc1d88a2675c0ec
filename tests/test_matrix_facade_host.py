"""Distance matrix, host side of the facade (no GPU): ``VectorStore.search_matrix`` and the pairs / offsets forms over stub
shards that answer the two library calls as the header defines them, in numpy float32 -- the sample (seed, filter, explicit
ids, MATRIX_MAX_SAMPLE), the multi-shard composition against one shard holding every row, what crosses between shards, the
two result formats, the REST bodies and the ``_async`` forms."""
import asyncio
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from wdbx_amd import api
from wdbx_amd.config import WDBXConfig
from wdbx_amd.vector_store import VectorStore
from wdbx_amd.wdbx import WDBX

D, N = 8, 40
_F32 = np.float32


def _pack(allowed):
    bits = np.zeros((len(allowed) + 31) // 32 * 32, bool)
    bits[: len(allowed)] = allowed
    return np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).ravel()


def _rank(rows, query, among, limit):
    """[(row, score)] of the rows `among`, (score descending, row ascending), in float32"""
    s = (rows[among] @ query).astype(_F32)
    order = np.lexsort((among, -s))[:limit]
    return [(int(among[i]), float(s[i])) for i in order]


class _Shard:
    metric = 0  # cosine

    def __init__(self, rows, tag):
        self.rows, self.tag = rows, tag
        self.next_index = len(rows)
        self.matrix_calls, self.among_calls = [], []
        self.swallow_errors = False

    def _id(self, r):
        return f"{self.tag}v{r}"

    def _row_of(self, vector_id):
        tail = vector_id[len(self.tag) + 1:]
        return int(tail) if vector_id.startswith(self.tag + "v") and tail.isdigit() and int(tail) < len(self.rows) else None

    def _rows_of(self, ids):
        return np.array(sorted({self._row_of(v) for v in ids} - {None}), np.int64)

    def row_mask_for(self, predicate):
        return _pack(np.array([predicate(self._id(r)) for r in range(len(self.rows))]))

    def mapped_ids(self, mask_words=None):
        rows = range(len(self.rows))
        return [self._id(r) for r in rows if mask_words is None or (int(mask_words[r >> 5]) >> (r & 31)) & 1]

    def stored_vectors(self, ids):
        rows = self._rows_of(ids)
        return [self._id(r) for r in rows], self.rows[rows].copy()

    def search_matrix(self, ids, limit=10):
        rows = self._rows_of(ids)
        self.matrix_calls.append((sorted(ids), limit))
        return [(self._id(a), [(self._id(r), s) for r, s in _rank(self.rows, self.rows[a], rows[rows != a], limit)]) for a in rows]

    def search_batch_among(self, queries, ids, limit=10, normalize=True):
        assert isinstance(queries, np.ndarray) and queries.dtype == _F32 and queries.shape[1] == D
        rows = self._rows_of(ids)
        self.among_calls.append((queries.copy(), sorted(ids), limit, normalize))
        return [[(self._id(r), s) for r, s in _rank(self.rows, q, rows, limit)] for q in queries]


def _store(tags=("a",), seed=21):
    """N rows per shard with integer elements: every dot product is exact in float32 and no row scores two others the same, so
    tie order across shards cannot decide"""
    rng = np.random.default_rng(seed)
    vs = VectorStore.__new__(VectorStore)
    vs.indices, vs.metadata, vs.vectors = [], {}, {}
    vs._bulk_id_shard, vs._bulk_ranges, vs._label_ids = {}, [], {}
    vs.config = WDBXConfig({})
    every = _distinct_rows(rng, N * len(tags))
    for t, tag in enumerate(tags):
        rows = every[t * N:(t + 1) * N]
        vs.indices.append(_Shard(rows, tag))
        for r in range(N):
            vs.metadata[f"{tag}v{r}"] = {"lang": "en" if r % 3 else "de"}
            vs._bulk_id_shard[f"{tag}v{r}"] = t
            vs.vectors[f"{tag}v{r}"] = rows[r]
    vs.num_shards, vs.vector_dim = len(tags), D
    vs._mask_cache, vs._meta_version = {}, 0
    vs._pending, vs._drain_task, vs._group = [], None, False
    vs._sync_lock, vs._sync_pending, vs._sync_busy, vs._sync_coalesce, vs._sync_last_batch = threading.Lock(), [], False, False, 0
    vs._group_lock, vs._group_verified, vs._group_path, vs.last_search_path = threading.Lock(), False, "copy_group", ""
    vs.thread_pool = ThreadPoolExecutor(max_workers=4)
    vs._shard_pool = ThreadPoolExecutor(max_workers=2)
    return vs


def _distinct_rows(rng, n):
    """integer rows (every dot product below 2^24: exact in float32) such that no row scores two other rows the same (drawn
    until that holds)"""
    for _ in range(200):
        rows = rng.integers(-1000, 1001, size=(n, D)).astype(_F32)
        g = (rows.astype(np.int64) @ rows.astype(np.int64).T)
        np.fill_diagonal(g, np.iinfo(np.int64).min)
        if all(len(np.unique(line)) == n for line in g):
            return rows
    raise AssertionError("no fixture with distinct scores")


def _wdbx(store):
    w = WDBX.__new__(WDBX)
    w.vector_store = store
    return w


def _one_shard_of(store):
    one = _store(("a",))
    one.indices[0].rows = np.concatenate([ix.rows for ix in store.indices])
    one.indices[0].next_index = len(one.indices[0].rows)
    return one


def _global(vid):  # a multi-shard id as the row of the one shard that holds everything
    return "abc".index(vid[0]) * N + int(vid[2:])


def test_the_sample_is_deterministic_under_a_seed_and_honours_the_filter():
    store = _store(("a", "b"))
    a = store.search_matrix(sample=12, limit=2, seed=5)
    b = store.search_matrix(sample=12, limit=2, seed=5)
    c = store.search_matrix(sample=12, limit=2, seed=6)
    assert a == b and len(a) == 12
    assert [x[0] for x in a] == sorted(x[0] for x in a) and [x[0] for x in a] != [x[0] for x in c]
    de = store.search_matrix(sample=9, limit=3, filter_metadata={"lang": "de"}, seed=1)
    assert len(de) == 9
    for anchor, res in de:
        assert store.metadata[anchor]["lang"] == "de" and len(res) == 3
        assert all(store.metadata[v]["lang"] == "de" and v != anchor for v, _ in res)
    # a sample larger than the matches is all of them; explicit ids are the sample (unknown ones ignored, repeats once)
    assert len(store.search_matrix(sample=1000, limit=1, filter_metadata={"lang": "de"})) == 2 * len(range(0, N, 3))
    got = store.search_matrix(sample=1, limit=5, vector_ids=["bv3", "av1", "nope", "av1", "av9"])
    assert [x[0] for x in got] == ["av1", "av9", "bv3"] and all(len(res) == 2 for _, res in got)
    assert store.search_matrix(sample=0) == [] and store.search_matrix(vector_ids=[]) == []
    assert store.search_matrix(sample=3, limit=0, seed=1) == [(x[0], []) for x in store.search_matrix(sample=3, limit=1, seed=1)]
    with pytest.raises(ValueError):
        store.search_matrix(sample=-1)


def test_matrix_max_sample_is_enforced():
    store = _store(("a", "b"))
    assert WDBXConfig({}).get("MATRIX_MAX_SAMPLE") == 10000
    store.config.set("MATRIX_MAX_SAMPLE", 10)
    assert len(store.search_matrix(sample=10, seed=1)) == 10
    with pytest.raises(ValueError, match="MATRIX_MAX_SAMPLE"):
        store.search_matrix(sample=11, seed=1)
    with pytest.raises(ValueError, match="MATRIX_MAX_SAMPLE"):
        store.search_matrix(vector_ids=[f"av{r}" for r in range(11)])


@pytest.mark.parametrize("tags", [("a", "b"), ("a", "b", "c")])
@pytest.mark.parametrize("limit", [1, 4, 200])
def test_several_shards_equal_one_shard_holding_all_rows(tags, limit):
    store = _store(tags)
    one = _one_shard_of(store)
    got = store.search_matrix(sample=25, limit=limit, seed=3)
    sample = [a for a, _ in got]
    assert len(sample) == 25 and len({a[0] for a in sample}) == len(tags)
    ref = one.indices[0].search_matrix([f"av{_global(a)}" for a in sample], limit)
    want = {int(a[2:]): [(int(v[2:]), s) for v, s in res] for a, res in ref}
    for anchor, res in got:
        assert [(_global(v), s) for v, s in res] == want[_global(anchor)], anchor
        assert len(res) == min(limit, 24)


def test_what_crosses_between_shards():
    store = _store(("a", "b", "c"))
    ids = ["av1", "av5", "bv2", "bv7", "bv9"]  # (shard c holds no sampled row: it is never asked)
    store.search_matrix(limit=3, vector_ids=ids)
    a, b, c = store.indices
    assert a.matrix_calls == [(["av1", "av5"], 3)] and b.matrix_calls == [(["bv2", "bv7", "bv9"], 3)]
    assert c.matrix_calls == [] and c.among_calls == []
    # every shard is asked once by every OTHER shard's anchors: the raw stored vectors, normalize off, its own part of the sample
    (q, listed, limit, normalize), = a.among_calls
    assert (q == b.rows[[2, 7, 9]]).all() and listed == ["av1", "av5"] and limit == 3 and normalize is False
    (q, listed, limit, normalize), = b.among_calls
    assert (q == a.rows[[1, 5]]).all() and listed == ["bv2", "bv7", "bv9"] and normalize is False
    # one shard: one call, nothing crosses
    single = _store(("a",))
    single.search_matrix(sample=7, seed=2)
    assert len(single.indices[0].matrix_calls) == 1 and single.indices[0].among_calls == []


def test_pairs_and_offsets_agree_and_async_equals_blocking():
    store = _store(("a", "b"))
    w = _wdbx(store)
    args = dict(sample=10, limit=3, filter_metadata={"lang": "en"}, seed=4)
    lines = store.search_matrix(**args)
    pairs = w.vector_search_matrix_pairs(**args)
    off = w.vector_search_matrix_offsets(**args)
    assert pairs == [{"a": a, "b": v, "score": s} for a, res in lines for v, s in res] and len(pairs) == 30
    assert off["ids"] == [a for a, _ in lines]
    assert len(off["offsets_row"]) == len(off["offsets_col"]) == len(off["scores"]) == len(pairs)
    back = [{"a": off["ids"][r], "b": off["ids"][c], "score": s} for r, c, s in zip(off["offsets_row"], off["offsets_col"], off["scores"])]
    assert back == pairs
    assert off["offsets_row"] == sorted(off["offsets_row"])  # anchor-major
    assert asyncio.run(store.search_matrix_async(**args)) == lines
    assert asyncio.run(w.vector_search_matrix_pairs_async(**args)) == pairs
    assert asyncio.run(w.vector_search_matrix_offsets_async(**args)) == off
    # L2: the facade reports positive squared distances, nearest first
    for ix in store.indices:
        ix.metric = 1
    l2 = w.vector_search_matrix_pairs(**args)
    assert [p["score"] for p in l2] == [-p["score"] for p in pairs]


def test_rest_bodies():
    store = _store(("a", "b"))
    w = _wdbx(store)
    body = {"sample": 6, "limit": 2, "filter": {"lang": "de"}, "seed": 9}
    want = w.vector_search_matrix_pairs(sample=6, limit=2, filter_metadata={"lang": "de"}, seed=9)
    assert asyncio.run(api.search_matrix_pairs_endpoint(w, body)) == {"pairs": want}
    assert asyncio.run(api.search_matrix_offsets_endpoint(w, body)) == w.vector_search_matrix_offsets(
        sample=6, limit=2, filter_metadata={"lang": "de"}, seed=9)
    ids = ["av1", "bv2", "bv3"]
    got = asyncio.run(api.search_matrix_pairs_endpoint(w, {"vector_ids": ids, "limit": None, "sample": None, "filter": None}))
    assert got == {"pairs": w.vector_search_matrix_pairs(vector_ids=ids)} and len(got["pairs"]) == 6
    assert len(asyncio.run(api.search_matrix_offsets_endpoint(w, {"seed": 1}))["ids"]) == 10  # the defaults: 10 x 3
    for bad in ([1], {"sample": "6"}, {"sample": True}, {"sample": -1}, {"limit": 2.5}, {"filter": [1]}, {"vector_ids": "av1"},
                {"vector_ids": [1]}, {"seed": "x"}):
        with pytest.raises(ValueError):
            asyncio.run(api.search_matrix_pairs_endpoint(w, bad))
        with pytest.raises(ValueError):
            asyncio.run(api.search_matrix_offsets_endpoint(w, bad))
