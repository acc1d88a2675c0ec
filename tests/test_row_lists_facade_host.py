"""One id list PER QUERY in a batch, host side (no GPU): ``VectorStore.search_batch_among_each``, the config
``FILTER_GATHER_PER_QUERY`` route of a batch with a filter per query, and the REST field ``vector_id_lists``.  The shards are
stubs that rank a small corpus exactly in numpy; they run the real ``HipFlatIndex.search_batch_among_each`` on top of a
numpy ``search_row_lists_raw`` and record every call."""
import asyncio
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from wdbx_amd import api
from wdbx_amd.config import WDBXConfig
from wdbx_amd.indexing import HipFlatIndex, RowList
from wdbx_amd.vector_store import VectorStore

D, N = 4, 60


def _pack(allowed):
    bits = np.zeros((len(allowed) + 31) // 32 * 32, bool)
    bits[: len(allowed)] = allowed
    return np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).ravel()


def _unpack(words, n):
    return ((words[np.arange(n) // 32] >> (np.arange(n) % 32).astype(np.uint32)) & 1).astype(bool)


class _Shard:
    """An exact shard over ``rows`` with ids ``<tag>v<row>``."""
    supports_row_lists = True
    search_batch_among_each = HipFlatIndex.search_batch_among_each  # the real method, over the stub's raw call

    def __init__(self, rows, tag):
        self.rows, self.tag = rows, tag
        self.next_index = len(rows)
        self.calls = []  # (kind, number of queries, number of masks or lists)
        self.thread_pool = None
        self.swallow_errors = False
        self.supports_row_masks = True
        self.rows_searches = 0

    def _id(self, r):
        return f"{self.tag}v{r}"

    def _row_of(self, vid):
        head = self.tag + "v"
        if isinstance(vid, str) and vid.startswith(head) and vid[len(head):].isdigit() and int(vid[len(head):]) < len(self.rows):
            return int(vid[len(head):])
        return None

    def rows_of(self, ids):
        rows = {r for r in (self._row_of(i) for i in ids) if r is not None}
        return np.fromiter(sorted(rows), dtype=np.uint64, count=len(rows))

    def _order(self, q, allowed):
        s = self.rows @ np.asarray(q, np.float32)
        return s, [r for r in np.lexsort((np.arange(len(s)), -s)) if allowed[r]]

    def _rank(self, q, limit, row_mask):
        n = len(self.rows)
        if isinstance(row_mask, RowList):
            allowed = np.zeros(n, bool)
            allowed[row_mask.rows.astype(np.int64)] = True
        else:
            allowed = np.ones(n, bool) if row_mask is None else _unpack(row_mask, n)
        s, order = self._order(q, allowed)
        return [(self._id(r), float(s[r])) for r in order[:limit]]

    def _map(self, idx_row, score_row):
        return [(self._id(int(r)), float(s)) for r, s in zip(idx_row, score_row) if r != -1]

    def search_rows_raw(self, queries, limit, rows):
        self.calls.append(("rows", len(queries), 1))
        return self.search_row_lists_raw(queries, limit, [rows], [0] * len(queries), record=False)

    def search_row_lists_raw(self, queries, limit, lists, list_of_query, record=True):
        assert len(list_of_query) == len(queries) and all(0 <= c < len(lists) for c in list_of_query)
        for rows in lists:  # what the library accepts
            assert rows.dtype == np.uint64 and np.all(np.diff(rows.astype(np.int64)) > 0) and all(r < len(self.rows) for r in rows)
        if record:
            self.calls.append(("row_lists", len(queries), len(lists)))
        if not any(len(r) for r in lists):
            return None
        self.rows_searches += 1
        idx = np.full((len(queries), limit), -1, np.int64)
        score = np.zeros((len(queries), limit), np.float32)
        for i, (q, c) in enumerate(zip(queries, list_of_query)):
            allowed = np.zeros(len(self.rows), bool)
            allowed[lists[c].astype(np.int64)] = True
            s, order = self._order(q, allowed)
            idx[i, : len(order[:limit])] = order[:limit]
            score[i, : len(order[:limit])] = s[order[:limit]]
        return idx, score

    def search_batch_among(self, queries, ids, limit=10):
        raw = self.search_rows_raw(queries, limit, self.rows_of(ids))
        return [[] for _ in queries] if raw is None else [self._map(i, s) for i, s in zip(*raw)]

    def search(self, q, limit=10, row_mask=None):
        self.calls.append(("single", 1, 0 if row_mask is None else 1))
        return self._rank(q, limit, row_mask)

    def search_batch(self, queries, limit=10, row_mask=None, row_masks=None, mask_of_query=None):
        if row_masks is not None:
            assert row_mask is None and len(mask_of_query) == len(queries)
            assert len(row_masks) <= 64 and all(-1 <= c < len(row_masks) for c in mask_of_query)
            assert not any(isinstance(m, RowList) for m in row_masks)  # a row list is no mask
            self.calls.append(("multimask", len(queries), len(row_masks)))
            return [self._rank(q, limit, None if c < 0 else row_masks[c]) for q, c in zip(queries, mask_of_query)]
        self.calls.append(("batch", len(queries), 0 if row_mask is None else 1))
        return [self._rank(q, limit, row_mask) for q in queries]

    def row_mask_for(self, predicate):
        return _pack(np.array([predicate(self._id(r)) for r in range(len(self.rows))]))


def _lang(r):
    return "en" if r % 6 == 0 else "de" if r % 10 == 1 else "xx"


@pytest.fixture()
def store():
    rng = np.random.default_rng(11)
    vs = VectorStore.__new__(VectorStore)
    vs.indices = []
    vs.metadata = {}
    vs._bulk_id_shard, vs._bulk_ranges = {}, []
    for tag in ("a", "b"):
        rows = rng.standard_normal((N, D)).astype(np.float32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        vs.indices.append(_Shard(rows, tag))
        for r in range(N):
            vs.metadata[f"{tag}v{r}"] = {"lang": _lang(r)}
            vs._bulk_id_shard[f"{tag}v{r}"] = len(vs.indices) - 1
    vs.num_shards = 2
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


def _queries(n, seed=3):
    q = np.random.default_rng(seed).standard_normal((n, D)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _calls(store):
    return [ix.calls for ix in store.indices]


def _clear(store):
    for ix in store.indices:
        ix.calls.clear()


ID_LISTS = [
    ["av3", "bv7", "av50", "bv0", "av9"],                     # both shards, any order
    ["bv7", "av3", "av3", "bv7", "av50", "bv0", "av9"],       # the same vectors, other order, repeats
    ["av1", "nobody", "av2", "bv999", "zv3"],                 # unknown ids; shard a only
    [],                                                       # an empty list
    [f"bv{r}" for r in range(N)],                             # shard b only, all of it
    ["nobody"],                                               # only unknown ids
]


def test_among_each_is_one_call_per_shard_and_equals_the_per_query_call(store):
    queries, limit = _queries(len(ID_LISTS)), 4
    got = store.search_batch_among_each(queries, ID_LISTS, limit=limit)
    # one call per shard for the whole batch; lists 0 and 1 name the same rows and share one list (with the empty one: 3, 3)
    assert _calls(store) == [[("row_lists", len(ID_LISTS), 3)], [("row_lists", len(ID_LISTS), 3)]]
    for q, ids, res in zip(queries, ID_LISTS, got):
        assert res == store.search_among(q, ids, limit=limit)
        assert {r[0] for r in res} <= set(ids)
    assert got[0] == [(v, s, store.metadata[v]) for v, s, _ in got[0]] and len(got[0]) == 4
    assert got[3] == [] and got[5] == [] and len(got[2]) == 2 and len(got[4]) == limit
    assert store.last_search_path == "threads"


def test_among_each_threshold_and_single_shard_work(store):
    queries = _queries(2, seed=5)
    lists = [["av1", "av2", "av3"], ["av4", "av5"]]
    got = store.search_batch_among_each(queries, lists, limit=3, threshold=0.1)
    assert _calls(store) == [[("row_lists", 2, 2)], []]  # shard b holds none of the ids: no call
    for q, ids, res in zip(queries, lists, got):
        assert res == store.search_among(q, ids, limit=3, threshold=0.1)
        assert all(r[1] >= 0.1 for r in res)
    assert store.search_batch_among_each(queries, [[], ["nobody"]], limit=3) == [[], []]
    assert store.search_batch_among_each(np.empty((0, D), np.float32), [], limit=3) == []


def test_among_each_wrong_length_raises(store):
    with pytest.raises(ValueError):
        store.search_batch_among_each(_queries(3), [["av1"], ["av2"]], limit=3)
    with pytest.raises(ValueError):
        store.search_batch_among_each(_queries(1), [["av1"], ["av2"]], limit=3)
    with pytest.raises(ValueError):
        store.search_batch_among_each(np.zeros((2, D + 1), np.float32), [[], []], limit=3)
    with pytest.raises(ValueError):
        store.indices[0].search_batch_among_each(_queries(3), [["av1"]], limit=3)


FILTERS = [{"lang": "en"}, None, {"lang": "de"}, {"lang": "en"}, {"lang": "xx"}, {}, {"lang": "de"}, {"lang": "en"}]


def _filtered(store, config):
    store.config = WDBXConfig(config)
    store._mask_cache = {}
    _clear(store)
    return store.search_batch(_queries(len(FILTERS)), limit=5, filter_metadata=FILTERS, prefilter=True)


def test_filter_gather_per_query_on_off_and_without_the_attribute(store):
    # "en" matches 10 rows of a shard, "de" 6, "xx" 44: with 12 gathered rows en and de travel as their rows
    off = _filtered(store, {"FILTER_GATHER_MAX_ROWS": 12})
    for calls in _calls(store):  # off: one call per filter, as before (none, en, de, xx)
        assert [c[0] for c in calls] == ["batch"] * 4
    on = _filtered(store, {"FILTER_GATHER_MAX_ROWS": 12, "FILTER_GATHER_PER_QUERY": True})
    for calls in _calls(store):  # on: the five en / de queries in one call with two lists, the other three with xx's mask
        assert calls == [("row_lists", 5, 2), ("multimask", 3, 1)]
    assert on == off
    for q, flt, res in zip(_queries(len(FILTERS)), FILTERS, on):
        assert res == store.search(q, limit=5, filter_metadata=flt, prefilter=True)
        assert all(r[2]["lang"] == flt["lang"] for r in res if flt)
    # every filter as its rows: the unfiltered queries still need the shard
    on_all = _filtered(store, {"FILTER_GATHER_MAX_ROWS": 50, "FILTER_GATHER_PER_QUERY": True})
    for calls in _calls(store):
        assert calls == [("row_lists", 6, 3), ("batch", 2, 0)]
    assert on_all == off
    # an index without the attribute keeps one call per filter
    store.indices[1].supports_row_lists = False
    mixed = _filtered(store, {"FILTER_GATHER_MAX_ROWS": 12, "FILTER_GATHER_PER_QUERY": True})
    assert _calls(store)[0] == [("row_lists", 5, 2), ("multimask", 3, 1)]
    assert [c[0] for c in _calls(store)[1]] == ["batch"] * 4
    assert mixed == off
    # no filter travels as its rows: the multimask call, whatever the switch says
    _filtered(store, {"FILTER_GATHER_MAX_ROWS": 0, "FILTER_GATHER_PER_QUERY": True})
    assert _calls(store) == [[("multimask", len(FILTERS), 3)]] * 2


def test_rest_batch_endpoint_takes_vector_id_lists(store):
    class _W:
        def vector_search_batch_among_each(self, queries, lists, limit, threshold):
            return store.search_batch_among_each(np.asarray(queries, np.float32), lists, limit=limit, threshold=threshold)

        def vector_search_batch(self, *a, **k):
            raise AssertionError("the listed form does not go through vector_search_batch")

    queries = _queries(3)
    lists = [["av3", "bv7", "av50"], [], ["bv1", "bv2", "nobody"]]
    body = {"query_vectors": queries.tolist(), "limit": 2, "vector_id_lists": lists}
    out = asyncio.run(api.search_batch_endpoint(_W(), body))
    assert [len(r) for r in out["results"]] == [2, 0, 2]
    want = store.search_batch_among_each(queries, lists, limit=2)
    assert [[(r["vector_id"], r["similarity"], r["metadata"]) for r in res] for res in out["results"]] == want
    for bad in (lists[:2], lists + [[]], "av3", [["av3"], "bv7", []], [[1], [], []]):
        with pytest.raises(ValueError):
            asyncio.run(api.search_batch_endpoint(_W(), dict(body, vector_id_lists=bad)))
    with pytest.raises(ValueError):
        asyncio.run(api.search_batch_endpoint(_W(), dict(body, filter_metadata={"lang": "en"})))
