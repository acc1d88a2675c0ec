"""Batch upsert and delete, host side of the facade (no GPU): ``HipFlatIndex`` over a recording stand-in of the native handle
-- a ``batch_add`` that mixes new and stored ids issues ONE native update call, ``remove_many`` one removal, a failing native
call restores the id maps -- and ``VectorStore.delete_many`` / ``delete_by_filter`` over recording shards: ids split by shard,
one call per shard, metadata gone, the cached row masks rebuilt, one save per call.  The REST handler's shapes."""
import asyncio
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from wdbx_amd import _native, api
from wdbx_amd.config import WDBXConfig
from wdbx_amd.indexing import HipFlatIndex
from wdbx_amd.vector_store import VectorStore, fnv1a_64

D = 8
_F32 = np.float32


class _Native:
    """Records the write calls of the native handle; rows live in a numpy array."""

    def __init__(self, fail_on=()):
        self.rows = np.zeros((0, D), _F32)
        self.calls = []
        self.fail_on = set(fail_on)

    def _note(self, name, *what):
        self.calls.append((name,) + what)
        if name in self.fail_on:
            raise _native.HipBackendError(-5, f"{name} failed")

    def add(self, rows, normalize=False):
        rows = np.atleast_2d(np.asarray(rows, _F32))
        self._note("add", len(rows))
        first = len(self.rows)
        self.rows = np.concatenate([self.rows, rows])
        return first

    def set_rows(self, first_row, rows, normalize=False):
        rows = np.atleast_2d(np.asarray(rows, _F32))
        self._note("set_rows", int(first_row), len(rows))
        self.rows[first_row:first_row + len(rows)] = rows

    def set_rows_at(self, rows_idx, rows, normalize=False):
        idx = [int(r) for r in rows_idx]
        assert idx == sorted(set(idx)) and all(0 <= r < len(self.rows) for r in idx)  # the C ABI's rule
        self._note("set_rows_at", tuple(idx))
        self.rows[idx] = np.asarray(rows, _F32)

    def remove_rows(self, rows_idx):
        idx = [int(r) for r in rows_idx]
        assert idx == sorted(set(idx)) and all(0 <= r < len(self.rows) for r in idx)
        self._note("remove_rows", tuple(idx))
        self.rows[idx] = np.nan


def _index(fail_on=(), swallow=False):
    ix = HipFlatIndex.__new__(HipFlatIndex)
    ix._native = _Native(fail_on)
    ix.vector_dim, ix.metric = D, _native.METRIC_COSINE
    ix.id_to_index, ix.index_to_id, ix.next_index = {}, {}, 0
    ix._implicit, ix._implicit_removed, ix._dirty_rows = [], set(), set()
    ix._ingest_lock = threading.RLock()
    ix.swallow_errors = swallow
    ix._unsaved_adds, ix.autosave_rows, ix._implicit_key = 0, 0, None
    return ix


def _vec(seed):
    return np.random.default_rng(seed).standard_normal(D).astype(_F32)


def _unit(v):
    return v / np.sqrt(v.dot(v))


def test_batch_add_sends_the_stored_ids_in_one_update_call():
    ix = _index()
    assert ix.batch_add({f"v{i}": _vec(i) for i in range(6)})
    assert ix._native.calls == [("add", 6)]
    ix._native.calls.clear()
    # stored ids out of row order, new ids in between
    batch = {"v4": _vec(104), "n0": _vec(200), "v1": _vec(101), "n1": _vec(201), "v5": _vec(105)}
    assert ix.batch_add(batch)
    assert ix._native.calls == [("set_rows_at", (1, 4, 5)), ("add", 2)]
    assert ix._dirty_rows == {1, 4, 5}
    assert (ix.id_to_index["n0"], ix.id_to_index["n1"], ix.next_index) == (6, 7, 8)
    # the same rows the per-id path leaves
    twin = _index()
    twin.batch_add({f"v{i}": _vec(i) for i in range(6)})
    for vid, v in batch.items():
        twin.add(vid, v)
    assert np.array_equal(ix._native.rows, twin._native.rows) and ix.id_to_index == twin.id_to_index
    assert np.array_equal(ix._native.rows[4], _unit(_vec(104)))
    # only stored ids: no append at all; only new ids: no update call
    ix._native.calls.clear()
    ix.batch_add({"v0": _vec(300), "n1": _vec(301)})
    ix.batch_add({"n9": _vec(302)})
    assert ix._native.calls == [("set_rows_at", (0, 7)), ("add", 1)]


def test_batch_add_errors_are_handled_as_before():
    ix = _index(fail_on=("set_rows_at",))
    ix._native.fail_on.clear()
    ix.batch_add({"a": _vec(1), "b": _vec(2)})
    ix._native.fail_on.add("set_rows_at")
    with pytest.raises(_native.HipBackendError):
        ix.batch_add({"a": _vec(3), "c": _vec(4)})
    assert "c" not in ix.id_to_index and ix._dirty_rows == set()
    ix.swallow_errors = True
    assert ix.batch_add({"a": _vec(3)}) is False
    with pytest.raises(ValueError):
        _index().batch_add({"a": np.zeros(D + 1, _F32)})


def test_remove_many_is_one_native_call_and_counts_the_present_ids():
    ix = _index()
    ix.batch_add({f"v{i}": _vec(i) for i in range(8)})
    ix._native.calls.clear()
    assert ix.remove_many(["v6", "nope", "v2", "v6", "v3"]) == 3
    assert ix._native.calls == [("remove_rows", (2, 3, 6))]
    assert all(v not in ix.id_to_index for v in ("v2", "v3", "v6")) and all(r not in ix.index_to_id for r in (2, 3, 6))
    assert ix._dirty_rows == {2, 3, 6} and ix.size() == 5
    assert np.isnan(ix._native.rows[[2, 3, 6]]).all() and not np.isnan(ix._native.rows[[0, 1, 4, 5, 7]]).any()
    assert ix.remove_many(["v2", "nope"]) == 0 and ix.remove_many([]) == 0
    assert len(ix._native.calls) == 1                        # nothing present: no native call
    # implicit (bulk) ids are unmapped through the removed-row set
    ix._implicit.append((8, 4, "row_", 0))
    ix._native.add(np.zeros((4, D), _F32))
    ix.next_index = 12
    ix._native.calls.clear()
    assert ix.remove_many(["row_1", "v0", "row_3"]) == 3
    assert ix._native.calls == [("remove_rows", (0, 9, 11))] and ix._implicit_removed == {9, 11}
    assert ix._row_of("row_1") is None and ix._row_of("row_2") == 10


def test_remove_many_restores_the_maps_when_the_native_call_fails():
    ix = _index()
    ix.batch_add({f"v{i}": _vec(i) for i in range(4)})
    ix._implicit.append((4, 2, "row_", 0))
    ix._native.add(np.zeros((2, D), _F32))
    ix.next_index = 6
    before = (dict(ix.id_to_index), dict(ix.index_to_id))
    ix._native.fail_on.add("remove_rows")
    with pytest.raises(_native.HipBackendError):
        ix.remove_many(["v1", "row_0", "v3"])
    assert (ix.id_to_index, ix.index_to_id) == before and ix._implicit_removed == set() and ix._dirty_rows == set()
    ix.swallow_errors = True
    assert ix.remove_many(["v1", "row_0"]) == 0
    assert (ix.id_to_index, ix.index_to_id) == before and ix._implicit_removed == set()


# ---- the store over recording shards --------------------------------------------------------------------------------
class _Shard:
    def __init__(self):
        self.ids = {}     # id -> row
        self.next_index = 0
        self.calls = []
        self.swallow_errors = False

    def put(self, vector_id):
        self.ids[vector_id] = self.next_index
        self.next_index += 1

    def _row_of(self, vector_id):
        return self.ids.get(vector_id)

    def remove_many(self, vector_ids):
        self.calls.append(("remove_many", sorted(vector_ids)))
        return sum(self.ids.pop(v, None) is not None for v in vector_ids)

    def remove(self, vector_id):
        self.calls.append(("remove", vector_id))
        return self.ids.pop(vector_id, None) is not None

    def row_mask_for(self, predicate):
        allowed = np.zeros(self.next_index, bool)
        for vid, row in self.ids.items():
            allowed[row] = predicate(vid)
        return allowed


def _store(shards=2, n=40, save_immediately=False):
    vs = VectorStore.__new__(VectorStore)
    vs.indices = [_Shard() for _ in range(shards)]
    vs.num_shards = shards
    vs.metadata, vs.vectors = {}, {}
    vs._bulk_id_shard, vs._bulk_ranges = {}, []
    vs._label_ids = {}
    vs.config = WDBXConfig({"VECTOR_STORE_SAVE_IMMEDIATELY": save_immediately})
    vs.vector_dim = D
    vs._mask_cache, vs._meta_version = {}, 0
    vs.thread_pool = ThreadPoolExecutor(max_workers=2)
    vs.saves = 0

    def save_now():
        vs.saves += 1
    vs._save_now = save_now
    for i in range(n):
        vid = f"v{i}"
        vs.vectors[vid] = _vec(i)
        vs.metadata[vid] = {"lang": "de" if i % 4 == 0 else "en", "n": i}
        vs.indices[fnv1a_64(vid) % shards].put(vid)
    return vs


def test_delete_many_splits_by_shard_one_call_each():
    vs = _store(save_immediately=True)
    gone = [f"v{i}" for i in (3, 7, 8, 20, 21, 39)]
    assert vs.delete_many(gone + ["nope", "v3"]) == 6
    by_shard = [sorted(v for v in gone if fnv1a_64(v) % 2 == s) for s in range(2)]
    assert [ix.calls for ix in vs.indices] == [[("remove_many", ids)] if ids else [] for ids in by_shard]
    assert all(v not in vs.metadata and v not in vs.vectors for v in gone) and len(vs.metadata) == 34
    assert vs._meta_version == 1 and vs.saves == 1           # once per call, not once per id
    assert vs.delete_many(["nope"]) == 0 and vs.delete_many(gone) == 0 and vs.delete_many([]) == 0
    assert vs.saves == 1 and sum(len(ix.calls) for ix in vs.indices) == sum(bool(ids) for ids in by_shard)
    # what the single delete leaves for the same ids
    twin = _store(save_immediately=True)
    for v in gone:
        assert twin.delete(v)
    assert twin.metadata == vs.metadata and sorted(twin.vectors) == sorted(vs.vectors)
    assert [ix.ids for ix in twin.indices] == [ix.ids for ix in vs.indices] and twin.saves == 6


def test_delete_by_filter_counts_drops_metadata_and_rebuilds_the_masks():
    vs = _store()
    flt = {"lang": "de"}
    masks = vs._row_masks(flt)
    assert sum(int(m.sum()) for m in masks) == 10
    assert vs._row_masks(flt) is masks                       # cached
    assert vs.delete_by_filter(flt) == 10
    assert all(m["lang"] == "en" for m in vs.metadata.values()) and len(vs.vectors) == 30
    assert sum(len(ix.calls) for ix in vs.indices) <= 2 and vs.saves == 0
    fresh = vs._row_masks(flt)
    assert fresh is not masks and sum(int(m.sum()) for m in fresh) == 0
    assert vs.delete_by_filter(flt) == 0 and vs.delete_by_filter({}) == 0 and len(vs.vectors) == 30
    assert asyncio.run(vs.delete_by_filter_async({"n": 1})) == 1
    assert asyncio.run(vs.delete_many_async(["v2", "v2", "zzz"])) == 1


class _Wdbx:
    def __init__(self):
        self.calls = []

    async def delete_vectors_async(self, ids):
        self.calls.append(("ids", ids))
        return len(ids)

    async def delete_by_filter_async(self, flt):
        self.calls.append(("filter", flt))
        return 7


def test_rest_handler_shapes():
    w = _Wdbx()
    assert asyncio.run(api.delete_vectors_endpoint(w, {"vector_ids": ["a", "b"]})) == {"deleted": 2}
    assert asyncio.run(api.delete_vectors_endpoint(w, {"vector_ids": []})) == {"deleted": 0}
    assert asyncio.run(api.delete_vectors_endpoint(w, {"filter_metadata": {"lang": "de"}, "vector_ids": None})) == {"deleted": 7}
    assert w.calls == [("ids", ["a", "b"]), ("ids", []), ("filter", {"lang": "de"})]
    for body in ([], {}, {"vector_ids": ["a"], "filter_metadata": {"x": 1}}, {"vector_ids": "a"}, {"vector_ids": [1]},
                 {"filter_metadata": {}}, {"filter_metadata": ["lang"]}):
        with pytest.raises(ValueError):
            asyncio.run(api.delete_vectors_endpoint(w, body))
    assert len(w.calls) == 3
