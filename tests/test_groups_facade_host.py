"""Search groups, host side of the facade (no GPU): ``VectorStore.search_groups`` over stub shards that rank a small corpus
exactly in numpy -- one shard (one ``search_groups`` call) and three shards (``search_distinct`` everywhere, the global labels,
``group_members`` everywhere, the members merged by (score descending, shard, position)): a label split over three shards, a
label that only one shard holds, an unlabelled winner, ties across shards, the threshold, a filter always travelling as the row
mask, the facade's group keys, the REST field and config ``DISTINCT_KEY=None``."""
import asyncio
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_distinct_facade_host import D, N, NONE, _query, _Shard
from wdbx_amd import api
from wdbx_amd.config import WDBXConfig
from wdbx_amd.vector_store import VectorStore
from wdbx_amd.wdbx import WDBX


class _GShard(_Shard):
    """... that also answers the two group calls as the library defines them"""

    def _members(self, s, order, label, vid, g):
        if label != NONE:
            rows = [r for r in order if int(self.labels[r]) == label]
        else:
            row = self._row_of(vid)
            rows = [r for r in order if r == row]
        return [(self._id(r), float(s[r])) for r in rows[:g]]

    def search_groups(self, q, limit=10, group_size=3, mask=None):
        assert mask is None or mask.dtype == np.uint32
        top = _Shard.search_distinct(self, q, limit, mask)
        self.calls[-1] = ("groups", mask is not None)
        s, order = self._ranked(q, mask)
        return [(label, self._members(s, order, label, vid, group_size)) for vid, _, label in top]

    def group_members(self, q, groups, group_size=3, mask=None):
        assert mask is None or mask.dtype == np.uint32
        self.calls.append(("members", mask is not None))
        s, order = self._ranked(q, mask)
        return [self._members(s, order, label, vid, group_size) for label, vid in groups]


def _doc(tag, r):
    """documents span the shards: chunk (tag, r) belongs to document r % 12; every 10th row has none; "solo" lives in shard b"""
    if r % 10 == 9:
        return None
    if tag == "b" and r in (3, 4, 5):
        return "solo"
    return f"doc{r % 12}"


def _store(tags=("a", "b", "c"), distinct_key="doc"):
    rng = np.random.default_rng(23)
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
        vs.indices.append(_GShard(rows, tag))
        for r in range(N):
            doc = _doc(tag, r)
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
    vs._shard_pool = ThreadPoolExecutor(max_workers=3)
    vs._push_labels(vs.metadata)
    return vs


def _brute(store, q, limit, g, threshold=0.0, flt=None):
    """every vector of every shard by (score descending, shard, row): the groups in the order of their first vector, cut at
    limit; each group's first g vectors; then the threshold"""
    rows = []
    for shard, ix in enumerate(store.indices):
        s = ix.rows @ q
        rows += [(-float(s[r]), shard, r, ix._id(r)) for r in range(N)]
    groups, at = [], {}
    for neg, _, _, vid in sorted(rows):
        meta = store.metadata[vid]
        if flt and any(meta.get(k) != v for k, v in flt.items()):
            continue
        key = meta.get("doc", vid)
        if key not in at:
            if len(groups) == limit:
                continue
            at[key] = len(groups)
            groups.append((key, []))
        if len(groups[at[key]][1]) < g:
            groups[at[key]][1].append((vid, -neg))
    out = []
    for key, hits in groups:
        hits = [h for h in hits if not (threshold > 0 and h[1] < threshold)]
        if hits:
            out.append((key, hits))
    return out


def _same(got, want, store):
    """got: the store's [(label, [(vid, score, metadata)])]"""
    assert len(got) == len(want)
    for (label, hits), (key, w_hits) in zip(got, want):
        assert [(h[0], h[1]) for h in hits] == [(vid, pytest.approx(s, abs=1e-6)) for vid, s in w_hits]
        assert all(h[2] == store.metadata[h[0]] for h in hits)
        assert label == (store._label_ids[key] if key in store._label_ids else NONE)


@pytest.mark.parametrize("g", [1, 3, 7])
@pytest.mark.parametrize("limit", [1, 5, 13, 40])
def test_three_shards_equal_the_brute_force(limit, g):
    store = _store()
    for seed in range(4):
        q = _query(seed)
        _same(store.search_groups(q.tolist(), limit=limit, group_size=g), _brute(store, q, limit, g), store)
    # every shard: one distinct call and one members call per search, no mask
    assert all(ix.calls == [("distinct", False), ("members", False)] * 4 for ix in store.indices)


def test_one_shard_is_one_groups_call():
    store = _store(tags=("a",))
    q = _query()
    got = store.search_groups(q.tolist(), limit=6, group_size=3)
    _same(got, _brute(store, q, 6, 3), store)
    assert store.indices[0].calls == [("groups", False)]
    assert asyncio.run(store.search_groups_async(q.tolist(), limit=6, group_size=3)) == got


def test_a_label_split_over_three_shards_and_a_label_one_shard_holds():
    store = _store()
    a, b, c = store.indices
    q = np.full(D, 0.5, np.float32)  # (unit length; every product and sum below is exact)
    # document 2: its best row in shard c, the next two in shard a (a tie), one more in shard b; its other rows score lowest
    for ix in store.indices:
        for r in range(2, N, 12):
            if r % 10 != 9 and not (ix is b and r in (3, 4, 5)):
                ix.rows[r] = -q
    c.rows[2] = q
    a.rows[14] = a.rows[26] = q * np.float32(0.5)
    b.rows[38] = q * np.float32(0.25)
    got = store.search_groups(q.tolist(), limit=40, group_size=4)
    assert got[0][0] == store._label_ids["doc2"] and [h[0] for h in got[0][1]] == ["cv2", "av14", "av26", "bv38"]
    # "solo": only shard b holds it -- the other shards answer its slot with nothing
    solo = [hits for label, hits in got if label == store._label_ids["solo"]]
    assert len(solo) == 1 and len(solo[0]) == 3 and all(h[0] in ("bv3", "bv4", "bv5") for h in solo[0])
    _same(got, _brute(store, q, 40, 4), store)


def test_an_unlabelled_winner_is_a_group_of_its_own():
    store = _store()
    a, b, c = store.indices
    q = np.full(D, 0.5, np.float32)
    b.rows[19] = q  # row 19 carries no document
    got = store.search_groups(q.tolist(), limit=4, group_size=5)
    assert got[0][0] == NONE and [h[0] for h in got[0][1]] == ["bv19"]
    _same(got, _brute(store, q, 4, 5), store)


def test_ties_are_broken_by_shard_then_position():
    store = _store()
    a, b, c = store.indices
    q = np.full(D, 0.5, np.float32)
    c.rows[7] = b.rows[7] = a.rows[31] = a.rows[19 + 12] = q  # document 7 in all three shards with one score (a: row 31)
    b.rows[43] = q                                            # ... and a second row of it in shard b
    got = store.search_groups(q.tolist(), limit=2, group_size=4)
    assert [h[0] for h in got[0][1]] == ["av31", "bv7", "bv43", "cv7"]
    _same(got, _brute(store, q, 2, 4), store)


def test_threshold_drops_members_and_whole_groups():
    store = _store()
    q = _query()
    full = store.search_groups(q.tolist(), limit=10, group_size=4)
    best = sorted(hits[0][1] for _, hits in full)
    t = (best[4] + best[5]) / 2  # five of the ten groups have no member that reaches it
    cut = store.search_groups(q.tolist(), limit=10, group_size=4, threshold=t)
    assert cut == [(label, [h for h in hits if h[1] >= t]) for label, hits in full if hits[0][1] >= t]
    assert len(cut) == 5 and any(len(c[1]) < len(f[1]) for c in cut for f in full if f[0] == c[0] != NONE)
    _same(cut, _brute(store, q, 10, 4, threshold=t), store)
    assert store.search_groups(q.tolist(), limit=10, group_size=4, threshold=-1.0) == full
    assert store.search_groups(q.tolist(), limit=10, group_size=4, threshold=2.0) == []


def test_a_filter_always_travels_as_the_mask():
    store = _store()
    q = _query()
    flt = {"lang": "de"}
    got = store.search_groups(q.tolist(), limit=8, group_size=3, filter_metadata=flt)
    assert all(ix.calls == [("distinct", True), ("members", True)] for ix in store.indices)
    assert got and all(h[2]["lang"] == "de" for _, hits in got for h in hits)
    _same(got, _brute(store, q, 8, 3, flt=flt), store)
    one = _store(tags=("a",))
    _same(one.search_groups(q.tolist(), limit=8, group_size=3, filter_metadata=flt), _brute(one, q, 8, 3, flt=flt), one)
    assert one.indices[0].calls == [("groups", True)]


def _facade(store):
    w = WDBX.__new__(WDBX)
    w.vector_store = store
    w.vector_dimension = D
    return w


def test_facade_keys_and_rest_shapes():
    store = _store()
    w = _facade(store)
    w._check_dim = lambda v: None
    q = _query()
    want = _brute(store, q, 6, 2)
    groups = w.vector_search_groups(q.tolist(), limit=6, group_size=2)
    assert [g["key"] for g in groups] == [key for key, _ in want]  # the DISTINCT_KEY value, or the vector id without one
    assert [[h[0] for h in g["hits"]] for g in groups] == [[vid for vid, _ in hits] for _, hits in want]
    assert asyncio.run(w.vector_search_groups_async(q.tolist(), limit=6, group_size=2)) == groups
    body = {"query_vector": q.tolist(), "limit": 6, "group_size": 2}
    res = asyncio.run(api.search_endpoint(w, body))
    assert set(res) == {"groups"} and [g["key"] for g in res["groups"]] == [key for key, _ in want]
    for g, (_, hits) in zip(res["groups"], want):
        assert set(g) == {"key", "hits"}
        assert [set(h) for h in g["hits"]] == [{"vector_id", "similarity", "metadata"}] * len(hits)
        assert [h["vector_id"] for h in g["hits"]] == [vid for vid, _ in hits]
    # with "distinct": true as well: the same groups; null = no groups
    assert asyncio.run(api.search_endpoint(w, dict(body, distinct=True))) == res

    class _Plain:
        async def vector_search_async(self, query, limit, threshold, flt):
            return [("plain", 1.0, {})]

        async def vector_search_distinct_async(self, query, limit, threshold, flt):
            return [("distinct", 1.0, {})]

    assert asyncio.run(api.search_endpoint(_Plain(), dict(body, group_size=None)))["results"][0]["vector_id"] == "plain"
    assert asyncio.run(api.search_endpoint(_Plain(), {"query_vector": q.tolist(), "distinct": True}))["results"][0]["vector_id"] == "distinct"
    for bad in (0, -1, True, "3", 2.0, []):
        with pytest.raises(ValueError, match="group_size"):
            asyncio.run(api.search_endpoint(w, dict(body, group_size=bad)))
    for extra in ({"mmr": {"lambda": 0.5}}, {"query_vectors": [q.tolist()]}):
        with pytest.raises(ValueError, match="group_size"):
            asyncio.run(api.search_endpoint(w, dict(body, **extra)))


def test_without_distinct_key_the_call_says_so():
    vs = _store(distinct_key=None)
    with pytest.raises(ValueError, match="DISTINCT_KEY"):
        vs.search_groups(_query().tolist(), limit=5)
    with pytest.raises(ValueError, match="DISTINCT_KEY"):
        asyncio.run(vs.search_groups_async(_query().tolist(), limit=5))
    w = _facade(vs)
    w._check_dim = lambda v: None
    with pytest.raises(ValueError, match="DISTINCT_KEY"):
        w.vector_search_groups(_query().tolist(), limit=5)
    with pytest.raises(ValueError, match="group_size"):
        _store().search_groups(_query().tolist(), limit=5, group_size=0)
