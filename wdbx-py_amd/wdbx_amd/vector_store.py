"""Shard fan-out, merge, threshold, metadata post-filter (reference:
wdbx/core/vector_store.py:22-815).  Same constructor, methods and result shapes;
every shard is a ``HipFlatIndex`` living in one GPU's HBM.

Differences a maintainer should know (all documented in INTEGRATION.md):
* the object is callable -- ``wdbx.vector_store(vector, metadata)`` works although
  ``wdbx.vector_store`` is this object (the reference's method/attribute clash,
  wdbx.py:120 vs :241, makes that call raise ``TypeError``);
* shard placement is a deterministic FNV-1a hash of the id instead of Python's
  salted ``hash`` (vector_store.py:178-190), so it survives a restart;
* ``index_type`` is "hip" only;
* the fan-out of ``search`` over several shards can be ONE call into the library: every shard's launches are enqueued by
  its own host thread, the per-shard (row, score) lists are exchanged (RCCL all-gather over xGMI with one shard per GPU,
  device copies when shards share a GPU) and merged on the device (``wdbx_group_search_merged``) -- the reference's
  loop + ``list.sort`` (vector_store.py:323-345) with the same candidate set and the same order (``HIP_GROUP_SEARCH``).
  Row masks of a pushed-down filter travel with the call (one mask per shard).
"""

from __future__ import annotations

import array
import asyncio
import json
import logging
import os
import pickle
import random
import threading
import time
import uuid
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .config import WDBXConfig
from .indexing import HipFlatIndex, RowList

logger = logging.getLogger(__name__)

Result = Tuple[str, float, Dict[str, Any]]


def fnv1a_64(text: str) -> int:
    h = 0xCBF29CE484222325
    for b in text.encode("utf-8"):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def matches_filter(metadata: Dict[str, Any], filter_metadata: Dict[str, Any]) -> bool:
    """Metadata predicate with the reference's grammar (vector_store.py:414-463):
    equality, or a ``{"$op": arg}`` dict of which only the first key counts;
    ``$gt $lt $gte $lte $in`` fail on a missing key, ``$nin`` and
    ``$exists: False`` pass on it, unknown operators are ignored."""
    for key, wanted in filter_metadata.items():
        if isinstance(wanted, dict) and list(wanted.keys())[0].startswith("$"):
            op = list(wanted.keys())[0]
            arg = wanted[op]
            have = key in metadata
            val = metadata.get(key)
            if op == "$exists":
                ok = have if arg else not have
            elif op == "$nin":
                ok = not (have and val in arg)
            elif op == "$in":
                ok = have and val in arg
            elif op == "$gt":
                ok = have and not (val <= arg)
            elif op == "$lt":
                ok = have and not (val >= arg)
            elif op == "$gte":
                ok = have and not (val < arg)
            elif op == "$lte":
                ok = have and not (val > arg)
            else:
                ok = True
            if not ok:
                return False
        elif key not in metadata or metadata[key] != wanted:
            return False
    return True


def _as_query(query_vector) -> np.ndarray:
    """list -> float32 array (vector_store.py:321 ``np.array(query_vector, dtype=np.float32)``): for a plain list of Python
    numbers ``array('f')`` makes the same double -> float casts in two thirds of the time; anything else goes the numpy way."""
    if type(query_vector) is list:
        try:
            return np.frombuffer(array.array("f", query_vector), dtype=np.float32)
        except (TypeError, OverflowError):
            pass
    return np.array(query_vector, dtype=np.float32)


def merge_range(shard_results, metadata: Dict[str, Any], filter_metadata: Optional[Dict[str, Any]] = None,
                max_results: Optional[int] = None) -> List[Result]:
    """The merge of a range search (``VectorStore.search_range``): the shards' [(id, score)] lists concatenated in shard
    order, stable-sorted by score descending (as ``_merge``: ties keep shard order, then each shard's own order), the
    metadata post-filter, then the cut to ``max_results`` (None = all); metadata attached."""
    merged: List[Tuple[str, float]] = []
    for results in shard_results:
        merged.extend(results)
    merged.sort(key=lambda r: r[1], reverse=True)
    if filter_metadata:
        merged = [r for r in merged if matches_filter(metadata.get(r[0], {}), filter_metadata)]
    if max_results is not None:
        merged = merged[: max(0, int(max_results))]
    return [(vid, score, metadata.get(vid, {})) for vid, score in merged]


class _SyncRequest:
    """One synchronous caller waiting in ``VectorStore._search_coalesced``.  ``gate`` is a plain lock used as a one-shot
    signal (created held; the server releases it): a tenth of the cost of ``threading.Event`` under the GIL."""
    __slots__ = ("query", "limit", "threshold", "flt", "gate", "result", "error", "promoted")

    def __init__(self, query, limit, threshold, flt):
        self.query, self.limit, self.threshold, self.flt = query, limit, threshold, flt
        self.gate = threading.Lock()
        self.gate.acquire()
        self.result = None
        self.error = None
        self.promoted = False


class VectorStore:
    _sync_coalesce = False  # (instances switch it on in __init__ from SYNC_COALESCE, once the queue and its lock exist)

    def __init__(
        self,
        vector_dim: int,
        data_dir: Path,
        num_shards: int = 1,
        use_gpu: bool = False,
        index_type: str = "hip",
        config: Optional[WDBXConfig] = None,
    ):
        self.vector_dim = vector_dim
        self.data_dir = Path(data_dir)
        self.num_shards = num_shards
        self.use_gpu = use_gpu
        self.index_type = index_type
        self.config = config or WDBXConfig({})

        self.vectors: Dict[str, np.ndarray] = {}
        self.metadata: Dict[str, Dict[str, Any]] = {}
        self.indices: List[HipFlatIndex] = []
        self._mask_cache: Dict[str, Any] = {}
        self._meta_version = 0
        self._pending: List[Any] = []      # coalescing queue of search_async (one event loop)
        self._drain_task = None
        # coalescing of SYNCHRONOUS callers on several threads (the reference's per-index pools call search from 4 workers,
        # indexing.py:692, :1045-1048): whoever arrives while a search is in flight queues up, and the next leader answers the
        # whole queue with ONE batched pass per shard (see _search_coalesced)
        self._sync_lock = threading.Lock()
        self._sync_pending: List[Any] = []
        self._sync_busy = False
        self._sync_last_batch = 0
        self._group_verified = False       # an RCCL group is checked once against the per-shard path before it is trusted
        self._sync_coalesce = bool(self.config.get("SYNC_COALESCE", True))
        # bulk-ingested rows: (prefix, first_label, count, shard) ranges with implicit ids, and the
        # shard of explicitly named bulk rows (placed by row range, not by hash)
        self._bulk_ranges: List[Tuple[str, int, int, int]] = []
        self._bulk_id_shard: Dict[str, int] = {}
        # distinct search (config DISTINCT_KEY): the values of that metadata field interned into 32-bit labels, ONE table for the
        # whole store so that the shards agree on a value's label
        self._label_ids: Dict[Any, int] = {}
        self._bulk_rows = 0        # labels handed out to implicit-id bulk rows so far (the next label)
        # shard group (one library call per search, RCCL merge): created lazily, None = not tried, False = unavailable
        self._group: Any = None
        self._group_lock = threading.Lock()  # (the group is built lazily by whichever searching thread comes first)
        self.last_search_path = ""  # "rccl_group" / "copy_group" / "threads": which fan-out served the last search (diagnostics)
        self._group_path = "rccl_group"

        self.thread_pool = ThreadPoolExecutor(
            max_workers=self.config.get("VECTOR_STORE_THREADS", os.cpu_count() or 4))
        # the per-shard calls of one fan-out run on a pool of their own: a fan-out that is itself running on
        # ``thread_pool`` (search_async) must never wait for workers of the pool it occupies (with
        # VECTOR_STORE_THREADS=1 and two shards that is a deadlock on the first call)
        self._shard_pool = ThreadPoolExecutor(max_workers=max(1, num_shards), thread_name_prefix="wdbx-shard")
        self._create_dirs()
        self._init_indices()
        self._load_data()
        logger.info("VectorStore initialized with %d vectors, %d shards, index_type=%s", self.count(),
                    self.num_shards, self.index_type)

    # ---- construction ----
    def _create_dirs(self) -> None:
        for sub in ["vectors", "metadata", "indices"] + [f"shard_{s}" for s in range(self.num_shards)]:
            (self.data_dir / sub).mkdir(parents=True, exist_ok=True)

    def _devices(self) -> List[int]:
        wanted = self.config.get("HIP_DEVICES")
        if wanted:
            return [int(d) for d in wanted]
        n = _native.device_count()
        if n < 1:
            raise _native.HipBackendError(-4, "no HIP device visible: the WDBX HIP backend needs an AMD GPU")
        return list(range(n))

    def _init_indices(self) -> None:
        if self.index_type not in ("hip", "hip_flat"):
            raise ValueError(f"Unsupported index type: {self.index_type}")
        devices = self._devices()
        self.indices = []
        for shard in range(self.num_shards):
            self.indices.append(HipFlatIndex(
                vector_dim=self.vector_dim,
                index_path=self.data_dir / f"shard_{shard}" / "index",
                use_gpu=self.use_gpu,
                config=self.config,
                device_id=devices[shard % len(devices)],
            ))

    def _load_data(self) -> None:
        meta_path = self.data_dir / "metadata" / "metadata.json"
        if meta_path.exists():
            try:
                with open(meta_path, "r") as f:
                    self.metadata = json.load(f)
            except Exception as e:
                logger.error("Error loading metadata: %s", e)
        bulk_path = self.data_dir / "metadata" / "bulk.json"
        if bulk_path.exists():
            try:
                with open(bulk_path, "r") as f:
                    b = json.load(f)
                self._bulk_ranges = [tuple(r) for r in b.get("ranges", [])]
                self._bulk_id_shard = {k: int(v) for k, v in b.get("id_shard", {}).items()}
                self._bulk_rows = int(b.get("rows", 0))
            except Exception as e:
                logger.error("Error loading bulk table: %s", e)
        vec_path = self.data_dir / "vectors" / "vectors.pickle"
        if vec_path.exists():
            try:
                with open(vec_path, "rb") as f:
                    self.vectors = pickle.load(f)
            except Exception as e:
                logger.error("Error loading vectors: %s", e)
        self._reconcile()
        self._push_labels(self.metadata)

    def _reconcile(self) -> None:
        """Make the tables loaded above agree with what the shards' own files brought back into HBM (they are saved
        at different moments; after an unclean exit the index files can be older than vectors.pickle / bulk.json):
        every id of the id -> vector table that its shard does not hold is added again, and bulk ranges / bulk ids
        that no shard holds any more are dropped (their rows existed only in HBM)."""
        missing: Dict[int, Dict[str, np.ndarray]] = {}
        for vid, vec in self.vectors.items():
            shard = self._get_shard_for_id(vid)
            if self.indices[shard]._row_of(vid) is None:
                missing.setdefault(shard, {})[vid] = vec
        for shard, vecs in missing.items():
            logger.warning("shard %d: re-adding %d vectors its index files did not hold", shard, len(vecs))
            self.indices[shard].batch_add(vecs)
        # a bulk range survives if its shard still holds at least one run of its labels (a compaction splits a range
        # into the runs of its surviving rows, indexing.py ``optimize``)
        def held(prefix, label0, count, shard):
            return any(p == prefix and l0 < label0 + count and label0 < l0 + c for _, c, p, l0 in self.indices[shard]._implicit)

        kept = [r for r in self._bulk_ranges if held(*r)]
        if len(kept) != len(self._bulk_ranges):
            logger.warning("dropping %d bulk ranges that no shard holds any more", len(self._bulk_ranges) - len(kept))
            self._bulk_ranges = kept
        gone = [vid for vid, s in self._bulk_id_shard.items() if self.indices[s]._row_of(vid) is None]
        for vid in gone:
            del self._bulk_id_shard[vid]
        if gone:
            logger.warning("dropping %d bulk ids that no shard holds any more", len(gone))

    # ---- labels of the distinct search ----
    def _label_of(self, metadata: Optional[Dict[str, Any]]) -> int:
        """The 32-bit label of a vector with this metadata: its DISTINCT_KEY value interned store-wide (an unhashable value
        by its JSON text); LABEL_NONE when the key is missing."""
        key = self.config.get("DISTINCT_KEY")
        if key is None or not isinstance(metadata, dict) or key not in metadata:
            return _native.LABEL_NONE
        value = metadata[key]
        try:
            hash(value)
        except TypeError:
            value = ("json", json.dumps(value, sort_keys=True, default=str))
        label = self._label_ids.get(value)
        if label is None:
            label = len(self._label_ids)
            if label >= _native.LABEL_NONE:
                raise OverflowError("more distinct values than 32-bit labels")
            self._label_ids[value] = label
        return label

    def _push_labels(self, vector_ids) -> None:
        """Label the named vectors in their shards from their current metadata (nothing without DISTINCT_KEY)."""
        if self.config.get("DISTINCT_KEY") is None:
            return
        per_shard: Dict[int, Tuple[List[str], List[int]]] = {}
        for vid in vector_ids:
            ids, labels = per_shard.setdefault(self._get_shard_for_id(vid), ([], []))
            ids.append(vid)
            labels.append(self._label_of(self.metadata.get(vid)))
        for shard, (ids, labels) in per_shard.items():
            self.indices[shard].set_labels(ids, labels)

    def _save_metadata(self) -> None:
        try:
            with open(self.data_dir / "metadata" / "metadata.json", "w") as f:
                json.dump(self.metadata, f)
            with open(self.data_dir / "metadata" / "bulk.json", "w") as f:
                json.dump({"ranges": self._bulk_ranges, "id_shard": self._bulk_id_shard, "rows": self._bulk_rows}, f)
        except Exception as e:
            logger.error("Error saving metadata: %s", e)

    def _save_vectors(self) -> None:
        try:
            with open(self.data_dir / "vectors" / "vectors.pickle", "wb") as f:
                pickle.dump(self.vectors, f)
        except Exception as e:
            logger.error("Error saving vectors: %s", e)

    def _save_indices(self) -> None:
        for ix in self.indices:
            if ix.unsaved():
                ix.save()

    def _save_now(self) -> None:
        """Everything durable at once (VECTOR_STORE_SAVE_IMMEDIATELY, shutdown, clear): the shards' rows first -- an
        incremental append, indexing.py -- then the tables that refer to them."""
        self._save_indices()
        self._save_metadata()
        self._save_vectors()

    def _get_shard_for_id(self, vector_id: str) -> int:
        shard = self._bulk_id_shard.get(vector_id)
        if shard is not None:
            return shard
        for prefix, label0, count, s in self._bulk_ranges:
            if vector_id.startswith(prefix):
                tail = vector_id[len(prefix):]
                if tail.isdigit() and label0 <= int(tail) < label0 + count:
                    return s
        return fnv1a_64(vector_id) % self.num_shards

    def _is_bulk(self, vector_id: str) -> bool:
        return vector_id not in self.vectors and self.indices[self._get_shard_for_id(vector_id)]._row_of(
            vector_id) is not None

    def bulk_store(self, rows, ids: Optional[Sequence[str]] = None,
                   metadata: Optional[Dict[str, Dict[str, Any]]] = None, id_prefix: str = "row_",
                   exact_normalize: bool = False, persist: Optional[bool] = None) -> int:
        """Bulk ingest of an ``[N, d]`` float32 array (the reference's per-vector
        ``batch_store`` builds N Python arrays and dict entries, vector_store.py:720-763).
        Rows are placed in CONTIGUOUS ranges (row r -> shard r // ceil(N/S)), one host-to-HBM copy
        per shard, normalised on the device; with ``ids=None`` they get implicit ids
        ``f"{id_prefix}{n}"`` (n counts bulk rows of this store) and cost no per-row host memory.
        The original vectors are not retained on the host: ``get`` returns the stored (normalised)
        row read back from HBM.  Bulk rows are written to the shards' files by ``shutdown`` (or at once with
        ``persist=True`` / VECTOR_STORE_SAVE_IMMEDIATELY); ranges that were never saved are dropped when the store is
        reopened (``_reconcile``)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.vector_dim:
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {rows.shape}")
        n = rows.shape[0]
        if ids is not None and len(ids) != n:
            raise ValueError("len(ids) != number of rows")
        per = -(-n // self.num_shards) if n else 0
        for s in range(self.num_shards):
            b, e = min(s * per, n), min((s + 1) * per, n)
            if e <= b:
                continue
            label0 = self._bulk_rows + b
            if ids is None:
                self.indices[s].add_rows(None, rows[b:e], id_prefix=id_prefix, first_label=label0,
                                         exact_normalize=exact_normalize)
                self._bulk_ranges.append((id_prefix, label0, e - b, s))
            else:
                self.indices[s].add_rows(list(ids[b:e]), rows[b:e], exact_normalize=exact_normalize)
                for vid in ids[b:e]:
                    self._bulk_id_shard[vid] = s
        self._bulk_rows += n
        for vid, meta in (metadata or {}).items():
            self.metadata[vid] = meta
        self._push_labels(metadata or {})
        self._meta_version += 1
        if persist or (persist is None and self.config.get("VECTOR_STORE_SAVE_IMMEDIATELY", False)):
            self._save_now()
        return n

    def bulk_store_synthetic(self, n: int, seed: int, counter_row0: int = 0, id_prefix: str = "row_") -> int:
        """Benchmark / test corpora of BASELINE.md section 3 generated ON THE DEVICE (``wdbx_index_fill_synthetic``:
        element (r, c) = ((splitmix64(seed ^ (r * d + c)) >> 40) - 2^23) * 2^-23, rows unit-normalised for cosine),
        placed like ``bulk_store`` (contiguous ranges, implicit ids ``f"{id_prefix}{label}"``)."""
        per = -(-n // self.num_shards) if n else 0
        for s in range(self.num_shards):
            b, e = min(s * per, n), min((s + 1) * per, n)
            if e <= b:
                continue
            label0 = self._bulk_rows + b
            self.indices[s].add_synthetic_rows(seed, counter_row0 + b, e - b, id_prefix=id_prefix, first_label=label0)
            self._bulk_ranges.append((id_prefix, label0, e - b, s))
        self._bulk_rows += n
        self._meta_version += 1
        return n

    async def initialize(self):
        await asyncio.gather(*[ix.initialize() for ix in self.indices])

    async def shutdown(self):
        self._save_now()
        if self._group:
            self._group.close()
        self._group = False
        await asyncio.gather(*[ix.shutdown() for ix in self.indices])
        self.thread_pool.shutdown()
        self._shard_pool.shutdown()

    # ---- the facade's ``vector_store(vector, metadata, id)`` (wdbx.py:241-270) ----
    def _check_dim(self, vector: Sequence[float]) -> None:
        if len(vector) != self.vector_dim:
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {len(vector)}")

    def __call__(self, vector: List[float], metadata: Optional[Dict[str, Any]] = None,
                 id: Optional[str] = None) -> str:
        self._check_dim(vector)
        vector_id = id or str(uuid.uuid4())
        self.store(vector_id, vector, metadata)
        return vector_id

    # ---- ingest ----
    def _remember(self, vector_id: str, vector, metadata) -> np.ndarray:
        vec = np.array(vector, dtype=np.float32)
        self.vectors[vector_id] = vec
        self.metadata[vector_id] = metadata or {}
        self._meta_version += 1
        return vec

    def store(self, vector_id: str, vector: List[float], metadata: Optional[Dict[str, Any]] = None) -> bool:
        try:
            vec = self._remember(vector_id, vector, metadata)
            self.indices[self._get_shard_for_id(vector_id)].add(vector_id, vec)
            self._push_labels([vector_id])
            if self.config.get("VECTOR_STORE_SAVE_IMMEDIATELY", False):
                self._save_now()
            return True
        except Exception as e:
            logger.error("Error storing vector: %s", e)
            return False

    async def store_async(self, vector_id: str, vector: List[float],
                          metadata: Optional[Dict[str, Any]] = None) -> bool:
        try:
            vec = self._remember(vector_id, vector, metadata)
            await self.indices[self._get_shard_for_id(vector_id)].add_async(vector_id, vec)
            self._push_labels([vector_id])
            if self.config.get("VECTOR_STORE_SAVE_IMMEDIATELY", False):
                await asyncio.get_event_loop().run_in_executor(self.thread_pool, self._save_now)
            return True
        except Exception as e:
            logger.error("Error storing vector asynchronously: %s", e)
            return False

    def _group_by_shard(self, vectors, metadata) -> Dict[int, Dict[str, np.ndarray]]:
        metadata = metadata or {}
        groups: Dict[int, Dict[str, np.ndarray]] = {}
        for vector_id, vector in vectors.items():
            vec = self._remember(vector_id, vector, metadata.get(vector_id, {}))
            groups.setdefault(self._get_shard_for_id(vector_id), {})[vector_id] = vec
        return groups

    def batch_store(self, vectors: Dict[str, List[float]],
                    metadata: Optional[Dict[str, Dict[str, Any]]] = None) -> int:
        for shard, vecs in self._group_by_shard(vectors, metadata).items():
            self.indices[shard].batch_add(vecs)
        self._push_labels(vectors)
        if self.config.get("VECTOR_STORE_SAVE_IMMEDIATELY", False):
            self._save_now()
        return len(vectors)

    async def batch_store_async(self, vectors: Dict[str, List[float]],
                                metadata: Optional[Dict[str, Dict[str, Any]]] = None) -> int:
        groups = self._group_by_shard(vectors, metadata)
        if groups:
            await asyncio.gather(*[self.indices[s].batch_add_async(v) for s, v in groups.items()])
        self._push_labels(vectors)
        if self.config.get("VECTOR_STORE_SAVE_IMMEDIATELY", False):
            await asyncio.get_event_loop().run_in_executor(self.thread_pool, self._save_now)
        return len(vectors)

    # ---- search ----
    def _matches_filter(self, vector_id: str, filter_metadata: Dict[str, Any]) -> bool:
        return matches_filter(self.metadata.get(vector_id, {}), filter_metadata)

    def _merge(self, shard_results, limit: int, threshold: float,
               filter_metadata: Optional[Dict[str, Any]]) -> List[Result]:
        """vector_store.py:323-351: shard order concat, stable sort by score
        descending, ``threshold > 0`` keeps ``score >= threshold``, metadata
        post-filter, cut to ``limit``, attach metadata."""
        merged: List[Tuple[str, float]] = []
        for results in shard_results:
            merged.extend(results)
        merged.sort(key=lambda r: r[1], reverse=True)
        if threshold > 0:
            merged = [r for r in merged if r[1] >= threshold]
        if filter_metadata:
            merged = [r for r in merged if self._matches_filter(r[0], filter_metadata)]
        return [(vid, score, self.metadata.get(vid, {})) for vid, score in merged[:limit]]

    def _row_masks(self, filter_metadata: Dict[str, Any]):
        """Per-shard row masks of the metadata filter (push-down), cached until the
        store changes."""
        key = self._mask_key(filter_metadata)
        version = (sum(ix.next_index for ix in self.indices), len(self.metadata), self._meta_version)
        cache = self._mask_cache
        if cache.get("version") != version:
            cache.clear()
            cache["version"] = version
        if key not in cache:
            cache[key] = [ix.row_mask_for(lambda vid: self._matches_filter(vid, filter_metadata))
                          for ix in self.indices]
        return cache[key]

    # ---- fan-out over the shards ----
    def _shard_group(self):
        """The in-library shard group (``wdbx_group_attach`` over this store's per-shard handles): every shard's
        launches enqueued by its own host thread inside ONE library call, the per-shard lists exchanged by RCCL
        all-gather (one shard per GPU) or by device copies (shards sharing a GPU), merged on the device.
        ``HIP_GROUP_SEARCH``: "auto" (default) and True = on for any layout of several shards; "always" = also for a single
        shard; False = off.  A group whose exchange is RCCL (one shard per GPU) is VERIFIED on its first query against the
        per-shard calls + Python merge (``_fan_out``): a differing answer or an error switches it off for this store with one
        log line (tools/preflight_multigpu.py and tests/test_gpu_parity.py::test_rccl_group_over_distinct_devices_* exercise
        the same exchange stage by stage).  Any failure to build it (e.g. RCCL initialisation) is logged once and the
        per-shard calls stay in use."""
        if self._group is not None:
            return self._group or None
        with self._group_lock:
            if self._group is not None:
                return self._group or None
            devices = [ix.device_id for ix in self.indices]
            mode = self.config.get("HIP_GROUP_SEARCH", "auto")
            wanted = mode == "always" or ((mode is True or mode == "auto") and len(self.indices) > 1)
            group: Any = False
            if wanted:
                try:
                    group = _native.NativeGroup.attach([ix._native for ix in self.indices])
                    info = group.info()
                    self._group_stride = info["row_stride"]
                    self._group_path = "rccl_group" if info["rccl_nranks"] > 0 else "copy_group"
                except Exception as e:
                    logger.warning("shard group unavailable, searching shard by shard: %s", e)
                    group = False
            self._group = group
        return self._group or None

    def _group_search(self, queries: np.ndarray, limit: int, keep_all: bool,
                      masks=None) -> Optional[List[List[Tuple[str, float]]]]:
        """One library call for all shards; returns, per query, the merged per-shard candidate list best first
        (the top ``limit`` of it, or with ``keep_all`` the whole union of the shards' top-``limit`` lists, which is what
        the reference's threshold / post-filter see) -- or None when the group cannot serve this call."""
        group = self._shard_group()
        if group is None:
            return None
        shards = len(self.indices)
        if int(limit) > _native.MAX_K:
            return None  # (the per-shard path returns up to MAX_K per shard and merges them: same answer only there)
        k = min(int(limit), max(ix.next_index for ix in self.indices))
        if k <= 0:
            return [[] for _ in range(queries.shape[0])]
        k_out = min(shards * k, sum(min(k, ix.next_index) for ix in self.indices)) if keep_all else k
        k_out = max(k_out, k)
        if k_out > _native.MAX_K:
            return None
        try:
            prepared = np.stack([self.indices[0]._prepare(q) for q in queries])
            idx, score = group.search_merged(prepared, k, k_out, mask_words=masks)
        except Exception as e:
            logger.error("Error searching the shard group: %s", e)
            if all(ix.swallow_errors for ix in self.indices):
                return [[] for _ in range(queries.shape[0])]
            raise
        stride = self._group_stride
        cosine = self.indices[0].metric == _native.METRIC_COSINE
        out = []
        for irow, srow in zip(idx.tolist(), score.tolist()):
            res = []
            for g, sc in zip(irow, srow):
                if g == -1:
                    continue
                res.append((self.indices[g // stride]._id_of(g % stride), float(sc if cosine else -sc)))
            out.append(res)
        return out

    def _fan_out(self, query: np.ndarray, limit: int, masks, post_filtered: bool) -> List[List[Tuple[str, float]]]:
        """Per-shard candidate lists of one query, in shard order (or ONE already merged list from the shard group:
        the stable sort of ``_merge`` leaves it as it is)."""
        # (a pushed-down filter travels with the call: every shard applies its own row mask inside its scan)
        # (a shard that answers from a row list is not a group call: the group knows masks only)
        merged = None if self._has_lists(masks) else self._group_search(
            query[None, :], limit, keep_all=post_filtered, masks=None if all(m is None for m in masks) else masks)
        if merged is not None and self._group_path == "rccl_group" and not self._group_verified:
            merged = self._verify_group_once(query, limit, masks, post_filtered, merged)
        if merged is not None:
            self.last_search_path = self._group_path
            return merged
        self.last_search_path = "threads"
        return self._per_shard(query, limit, masks)

    def _verify_group_once(self, query, limit, masks, post_filtered, merged):
        """First query through an RCCL group: the same query through the per-shard calls, merged as the reference does; ids
        must agree.  On a mismatch the group is closed and the store stays on the per-shard path."""
        per_shard = self._per_shard(query, limit, masks)
        flat = [r for res in per_shard for r in res]
        flat.sort(key=lambda r: r[1], reverse=True)
        want = [vid for vid, _ in flat[: len(merged[0])]]
        got = [vid for vid, _ in merged[0]]
        if got == want:
            self._group_verified = True
            return merged
        logger.error("shard group (RCCL exchange) disagrees with the per-shard path on its first query (%s vs %s): "
                     "switched off for this store", got[:5], want[:5])
        with self._group_lock:
            try:
                if self._group:
                    self._group.close()
            finally:
                self._group = False
        return None

    def _per_shard(self, query: np.ndarray, limit: int, masks) -> List[List[Tuple[str, float]]]:
        if len(self.indices) > 1:
            # the reference loops over its shards one after the other (vector_store.py:325-327); here every
            # shard is a GPU-resident index behind a GIL-releasing call, so the fan-out runs concurrently
            # (one worker per shard) and the results are gathered in shard order -- same answer
            return list(self._shard_pool.map(lambda a: a[0].search(query, limit=limit, row_mask=a[1]),
                                             zip(self.indices, masks)))
        return [ix.search(query, limit=limit, row_mask=m) for ix, m in zip(self.indices, masks)]

    def _masks_for(self, filter_metadata, prefilter: Optional[bool], gather: bool = False):
        """Per shard what a pushed-down filter travels as: None (no push-down), the row mask, or -- ``gather`` (the top-k
        searches) with config ``FILTER_GATHER_MAX_ROWS`` > 0 -- a ``RowList`` for a shard in which the filter matches at
        most that many rows: that shard answers through the search among listed rows, at the cost of those rows."""
        if prefilter is None:
            prefilter = bool(self.config.get("FILTER_PUSHDOWN", False))
        if not (prefilter and filter_metadata):
            return [None] * len(self.indices)
        masks = self._row_masks(filter_metadata)
        gmax = int(self.config.get("FILTER_GATHER_MAX_ROWS", 0) or 0) if gather else 0
        if gmax <= 0:
            return masks
        # (cached next to the masks, under the same version: _row_masks has just cleared the cache if the store changed)
        key = ("rows", self._mask_key(filter_metadata), gmax)
        cache = self._mask_cache
        if key not in cache:
            out = []
            for ix, words in zip(self.indices, masks):
                bits = np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")
                rows = np.flatnonzero(bits[: ix.next_index])
                out.append(RowList(rows.astype(np.uint64)) if rows.size <= gmax else words)
            cache[key] = out
        return cache[key]

    @staticmethod
    def _has_lists(masks) -> bool:
        return masks is not None and any(isinstance(m, RowList) for m in masks)

    @staticmethod
    def _mask_key(filter_metadata) -> str:
        """The ``_mask_cache`` key of a pushed-down filter: callers with the same key share one set of row masks."""
        return json.dumps(filter_metadata, sort_keys=False, default=str)

    def search(self, query_vector: List[float], limit: int = 10, threshold: float = 0.0,
               filter_metadata: Optional[Dict[str, Any]] = None, prefilter: Optional[bool] = None) -> List[Result]:
        """``prefilter=True`` (or config ``FILTER_PUSHDOWN``) evaluates the metadata filter BEFORE the
        scan, so a filtered query returns a full ``limit`` whenever enough rows match; the default keeps
        the reference's post-filter (vector_store.py:337-342), which can under-return."""
        query = _as_query(query_vector)
        masks = self._masks_for(filter_metadata, prefilter, gather=True)
        if self._sync_coalesce and all(m is None for m in masks) and query.shape == (self.vector_dim,):
            return self._search_coalesced(query, int(limit), threshold, filter_metadata)
        shard_results = self._fan_out(query, limit, masks, post_filtered=bool(filter_metadata))
        return self._merge(shard_results, limit, threshold, filter_metadata)

    # ---- synchronous callers on several threads: leader / follower coalescing ----
    def _search_coalesced(self, query: np.ndarray, limit: int, threshold: float, flt) -> List[Result]:
        """The reference serves ``search`` from thread pools (indexing.py:692, :1045-1048); N threads calling a GPU-resident
        index one query at a time would be N serial corpus scans behind the handle's mutex.  Instead: a caller that finds no
        search in flight becomes the LEADER and runs at once (a lone caller pays a lock and a list append: nothing waits for
        company).  Callers that arrive meanwhile queue up; when the leader is done it hands over to the first of them, which
        answers EVERYTHING queued by then -- itself included -- with ONE batched pass per shard (the matrix-core kernels from
        4 queries up, per-query scans inside one call below that) and wakes the others.  Each caller keeps its own limit,
        threshold and filter; a shard's top-kmax list cut to ``limit`` is its top-``limit`` list, so the answers are those of
        one-at-a-time calls (config ``SYNC_COALESCE=False`` restores them)."""
        req = _SyncRequest(query, limit, threshold, flt)
        with self._sync_lock:
            self._sync_pending.append(req)
            lead = not self._sync_busy
            if lead:
                self._sync_busy = True
        if not lead:
            req.gate.acquire()            # woken by the leader that served (or promoted) this request
            if not req.promoted:
                return self._sync_finish(req)
        # leader: everything queued so far, own request included.  A PROMOTED leader (so: callers are contending) first gives
        # the callers of the batch that has just been answered a moment to come back -- they are re-entering search() right
        # now, and a batch taken this instant would hold one or two queries where a few microseconds later it holds them all
        # (a first leader never waits: a lone caller is served at once)
        batch: List[Any] = []
        try:
            if req.promoted and self._sync_last_batch > 2:
                want, deadline = self._sync_last_batch - 1, time.perf_counter() + 40e-6
                while len(self._sync_pending) < want and time.perf_counter() < deadline:
                    time.sleep(0)         # (yields the GIL to the callers on their way in)
            with self._sync_lock:
                batch, self._sync_pending = self._sync_pending, []
            self._sync_last_batch = len(batch)
            self._serve_sync_batch(batch)
        except BaseException as e:  # every waiter of this batch sees the failure
            for r in batch:
                if r.result is None and r.error is None:
                    r.error = e if isinstance(e, Exception) else RuntimeError(str(e))
            if not batch or not isinstance(e, Exception):
                raise
        finally:
            # whatever happened above (an interrupt in the wait included), leadership is handed on or given up: a leader that
            # left with _sync_busy still set would park every later caller for ever
            with self._sync_lock:
                if self._sync_pending:
                    nxt = self._sync_pending[0]
                    nxt.promoted = True
                    nxt.gate.release()
                else:
                    self._sync_busy = False
            for r in batch:
                if r is not req:
                    r.gate.release()
        return self._sync_finish(req)

    @staticmethod
    def _sync_finish(req) -> List[Result]:
        if req.error is not None:
            raise req.error
        return req.result

    def _serve_sync_batch(self, batch) -> None:
        if len(batch) == 1:
            r = batch[0]
            res = self._fan_out(r.query, r.limit, [None] * len(self.indices), bool(r.flt))
            r.result = self._merge(res, r.limit, r.threshold, r.flt)
            return
        kmax = max(r.limit for r in batch)
        queries = np.stack([r.query for r in batch])
        merged = None
        if all(r.limit == kmax for r in batch) and self._shard_group() is not None and (
                self._group_path != "rccl_group" or self._group_verified):
            merged = self._group_search(queries, kmax, keep_all=any(bool(r.flt) for r in batch))
        if merged is not None:
            self.last_search_path = self._group_path
            for m, r in zip(merged, batch):
                r.result = self._merge([m], r.limit, r.threshold, r.flt)
            return
        self.last_search_path = "threads"
        raw_capable = all(hasattr(ix, "search_batch_raw") for ix in self.indices)
        if raw_capable:
            if len(self.indices) > 1:
                raws = list(self._shard_pool.map(lambda ix: ix.search_batch_raw(queries, limit=kmax), self.indices))
            else:
                raws = [self.indices[0].search_batch_raw(queries, limit=kmax)]
            # (the leader maps and merges for everybody before it wakes anybody: the callers then come back together, and the
            # next batch is as large as this one -- with the tails on the callers' own threads the arrivals spread out and the
            # batches shrank: 11.7 k vs 14.5 k q/s from 8 threads on 1 M rows)
            for i, r in enumerate(batch):
                lists = [[] if raw is None else ix._map(raw[0][i][: r.limit], raw[1][i][: r.limit])
                         for ix, raw in zip(self.indices, raws)]
                r.result = self._merge(lists, r.limit, r.threshold, r.flt)
            return
        if len(self.indices) > 1:
            per_shard = list(self._shard_pool.map(lambda ix: ix.search_batch(queries, limit=kmax), self.indices))
        else:
            per_shard = [self.indices[0].search_batch(queries, limit=kmax)]
        for i, r in enumerate(batch):
            r.result = self._merge([res[i][: r.limit] for res in per_shard], r.limit, r.threshold, r.flt)

    async def search_async(self, query_vector: List[float], limit: int = 10, threshold: float = 0.0,
                           filter_metadata: Optional[Dict[str, Any]] = None,
                           prefilter: Optional[bool] = None) -> List[Result]:
        """Same contract as the reference (vector_store.py:355-412).  Concurrent callers on one event
        loop are COALESCED: whatever is queued while the previous batch runs is answered by one
        batched pass per shard (the matrix-core kernels from 4 queries up) instead of one corpus scan
        per caller.  No waiting window: a lone caller is served at once, exactly as before.  Every
        shard is still asked for each query's own top-``limit``; results are the exact ones
        (config ``ASYNC_COALESCE=False`` restores one call per query).  ``prefilter`` / FILTER_PUSHDOWN as in
        ``search``: waiting callers that push down the SAME filter (the same ``_mask_cache`` key) share one masked batched
        call -- one masked matrix-core pass per shard; callers with different filters are served in separate calls, unless
        config ``ASYNC_COALESCE_FILTERS`` (default False) is on: then all waiting push-down callers with equal ``limit`` go in
        ONE call per shard with a row mask per query (``wdbx_index_search_multimask``)."""
        query = np.array(query_vector, dtype=np.float32)
        if query.shape != (self.vector_dim,):
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {query.shape}")
        loop = asyncio.get_running_loop()
        masks = self._masks_for(filter_metadata, prefilter, gather=True)
        pushed = any(m is not None for m in masks)
        if not self.config.get("ASYNC_COALESCE", True):
            shard_results = await loop.run_in_executor(self.thread_pool, self._fan_out, query, limit, masks,
                                                       bool(filter_metadata))
            return self._merge(shard_results, limit, threshold, filter_metadata)
        fut = loop.create_future()
        self._pending.append((query, int(limit), threshold, filter_metadata, fut,
                              self._mask_key(filter_metadata) if pushed else None))
        if self._drain_task is None or self._drain_task.done():
            self._drain_task = loop.create_task(self._drain_pending())
        return await fut

    async def _drain_pending(self) -> None:
        loop = asyncio.get_running_loop()
        nomask = [None] * len(self.indices)
        while self._pending:
            taken, self._pending = self._pending, []
            jobs = []
            if self.config.get("ASYNC_COALESCE_FILTERS", False) and all(
                    getattr(ix, "supports_row_masks", False) for ix in self.indices):
                # push-down callers with equal limit and DIFFERENT filters: one call per shard with a mask per query
                by_limit: Dict[int, List[Any]] = {}
                rest = []
                for b in taken:
                    (rest if b[5] is None else by_limit.setdefault(b[1], [])).append(b)
                for group in by_limit.values():
                    if len({b[5] for b in group}) > 1:
                        jobs.append(self._drain_filters(loop, [b[:5] for b in group]))
                    else:
                        rest.extend(group)
                taken = rest
            # callers that push down the same filter share one masked call; the others (no mask) share the unmasked one
            by_mask: Dict[Any, List[Any]] = {}
            for b in taken:
                by_mask.setdefault(b[5], []).append(b)
            # (the groups run side by side, as such callers did when each went to the pool alone; a group's masks are taken
            # NOW, once, not when its first caller queued: the store may have changed since)
            await asyncio.gather(*jobs, *[
                self._drain_batch(loop, [b[:5] for b in batch], None if key is None else batch[0][3], nomask)
                for key, batch in by_mask.items()])

    async def _drain_filters(self, loop, batch) -> None:
        """One coalesced batch of ``search_async`` callers that push down different filters with one ``limit``."""
        try:
            queries = np.stack([b[0] for b in batch])
            per_shard = await loop.run_in_executor(self.thread_pool, self._per_shard_filters, queries, batch[0][1],
                                                   [b[3] for b in batch])
            for i, (_, limit, threshold, flt, fut) in enumerate(batch):
                if not fut.done():
                    fut.set_result(self._merge([res[i] for res in per_shard], limit, threshold, flt))
        except Exception as e:  # deliver the failure to every waiter of this batch
            for b in batch:
                if not b[4].done():
                    b[4].set_exception(e)

    async def _drain_batch(self, loop, batch, pushed_filter, nomask) -> None:
        """One coalesced batch of ``search_async`` callers; ``pushed_filter``: the filter they all push down, or None."""
        try:
            masks = None if pushed_filter is None else self._masks_for(pushed_filter, True, gather=True)
            if len(batch) == 1:
                query, limit, threshold, flt, fut = batch[0]
                res = await loop.run_in_executor(self.thread_pool, self._fan_out, query, limit, masks or nomask, bool(flt))
                if not fut.done():
                    fut.set_result(self._merge(res, limit, threshold, flt))
                return
            kmax = max(b[1] for b in batch)
            queries = np.stack([b[0] for b in batch])
            if all(b[1] == kmax for b in batch) and not self._has_lists(masks) and self._shard_group() is not None:
                # same limit everywhere: ONE group call answers the whole batch (a caller with a filter needs the
                # union of the shards' lists, as in ``search``)
                keep_all = any(bool(b[3]) for b in batch)
                merged = await loop.run_in_executor(self.thread_pool, self._group_search, queries, kmax, keep_all, masks)
                if merged is not None:
                    self.last_search_path = self._group_path
                    for m, (_, limit, threshold, flt, fut) in zip(merged, batch):
                        if not fut.done():
                            fut.set_result(self._merge([m], limit, threshold, flt))
                    return
            if masks is None:
                per_shard = await asyncio.gather(*[
                    loop.run_in_executor(ix.thread_pool, ix.search_batch, queries, kmax) for ix in self.indices])
            else:  # every shard's own row mask travels with its batched call
                per_shard = await asyncio.gather(*[
                    loop.run_in_executor(ix.thread_pool, ix.search_batch, queries, kmax, m)
                    for ix, m in zip(self.indices, masks)])
            for i, (_, limit, threshold, flt, fut) in enumerate(batch):
                if not fut.done():
                    # a shard's top-kmax list cut to `limit` IS its top-`limit` list
                    fut.set_result(self._merge([res[i][:limit] for res in per_shard], limit, threshold, flt))
        except Exception as e:  # deliver the failure to every waiter of this batch
            for b in batch:
                if not b[4].done():
                    b[4].set_exception(e)

    def _search_batch_filters(self, queries: np.ndarray, limit: int, threshold: float, filters,
                              prefilter: Optional[bool]) -> List[List[Result]]:
        """``search_batch`` with one filter (or None) PER QUERY.  With push-down every shard gets the distinct filters' row
        masks and the per-query index in ONE call (one pass over the int8 tiles for all filters together); a shard for which
        some filter travels as a ``RowList`` keeps one call per filter -- or, with config ``FILTER_GATHER_PER_QUERY``, sends those
        queries in one call with a row list per query and the others in the call with a mask per query.  Without push-down every query's top-``limit`` is
        post-filtered by its own filter.  Shard by shard: the shard group takes no per-query masks."""
        if len(filters) != queries.shape[0]:
            raise ValueError(f"filter_metadata lists {len(filters)} filters for {queries.shape[0]} queries")
        if prefilter is None:
            prefilter = bool(self.config.get("FILTER_PUSHDOWN", False))
        self.last_search_path = "threads"
        nq = queries.shape[0]
        if not nq:
            return []
        if not (prefilter and any(filters)):
            if len(self.indices) > 1:
                per_shard = list(self._shard_pool.map(lambda ix: ix.search_batch(queries, limit=limit), self.indices))
            else:
                per_shard = [ix.search_batch(queries, limit=limit) for ix in self.indices]
            return [self._merge([res[q] for res in per_shard], limit, threshold, filters[q] or None) for q in range(nq)]
        per_shard = self._per_shard_filters(queries, limit, filters)
        return [self._merge([res[q] for res in per_shard], limit, threshold, filters[q] or None) for q in range(nq)]

    def _per_shard_filters(self, queries: np.ndarray, limit: int, filters) -> List[Any]:
        """Every shard's top-``limit`` lists of a batch whose query i pushes down ``filters[i]`` (None: no filter)."""
        nq = queries.shape[0]
        # the distinct filters (by mask-cache key) and which of them every query pushes down (-1: none)
        keys: Dict[str, int] = {}
        distinct: List[Any] = []
        which = []
        for flt in filters:
            if not flt:
                which.append(-1)
                continue
            key = self._mask_key(flt)
            if key not in keys:
                keys[key] = len(distinct)
                distinct.append(flt)
            which.append(keys[key])
        per_filter = [self._masks_for(flt, True, gather=True) for flt in distinct]  # [filter][shard]

        cmax = _native.MAX_CALL_MASKS  # masks one library call takes: more distinct filters go in groups of that many

        per_query = bool(self.config.get("FILTER_GATHER_PER_QUERY", False))

        def masked(ix, members, masks, which):
            """``members`` (queries of the batch) with row masks only: one call per group of at most cmax masks."""
            if len(masks) <= cmax:
                return ix.search_batch(queries[members], limit=limit, row_masks=masks, mask_of_query=which)
            out: Dict[int, Any] = {}
            # (the queries without a filter travel with the first group)
            for c0 in range(0, len(masks), cmax):
                part = [i for i, c in enumerate(which) if c0 <= c < c0 + cmax or (c0 == 0 and c < 0)]
                res = ix.search_batch(queries[[members[i] for i in part]], limit=limit, row_masks=masks[c0:c0 + cmax],
                                      mask_of_query=[which[i] - c0 if which[i] >= 0 else -1 for i in part])
                out.update(zip(part, res))
            return [out[i] for i in range(len(members))]

        def one(s):
            ix, masks = self.indices[s], [pf[s] for pf in per_filter]
            if not any(isinstance(m, RowList) for m in masks) and len(masks) <= cmax:
                return ix.search_batch(queries, limit=limit, row_masks=masks, mask_of_query=which)
            out: List[Any] = [None] * nq
            if not any(isinstance(m, RowList) for m in masks):
                # (the queries without a filter travel with the first group)
                for c0 in range(0, len(masks), cmax):
                    members = [q for q in range(nq) if c0 <= which[q] < c0 + cmax or (c0 == 0 and which[q] < 0)]
                    res = ix.search_batch(queries[members], limit=limit, row_masks=masks[c0:c0 + cmax],
                                          mask_of_query=[which[q] - c0 if which[q] >= 0 else -1 for q in members])
                    for q, r in zip(members, res):
                        out[q] = r
                return out
            if per_query and getattr(ix, "supports_row_lists", False):
                # FILTER_GATHER_PER_QUERY: the queries whose filter travels as its rows in ONE call with a list per query,
                # the others (row masks, no filter) in the call with a mask per query; scattered back into query order
                listed = [q for q in range(nq) if which[q] >= 0 and isinstance(masks[which[q]], RowList)]
                used = sorted({which[q] for q in listed})
                at = {c: i for i, c in enumerate(used)}
                raw = ix.search_row_lists_raw(queries[listed], limit, [masks[c].rows for c in used],
                                              [at[which[q]] for q in listed])
                res = [[] for _ in listed] if raw is None else [ix._map(i, sc) for i, sc in zip(*raw)]
                for q, r in zip(listed, res):
                    out[q] = r
                rest = [q for q in range(nq) if out[q] is None]
                if rest:
                    kept = [c for c, m in enumerate(masks) if not isinstance(m, RowList)]
                    at = {c: i for i, c in enumerate(kept)}
                    if any(which[q] >= 0 for q in rest):
                        res = masked(ix, rest, [masks[c] for c in kept], [at[which[q]] if which[q] >= 0 else -1 for q in rest])
                    else:
                        res = ix.search_batch(queries[rest], limit=limit)
                    for q, r in zip(rest, res):
                        out[q] = r
                return out
            # (a filter that travels as its rows: one call per filter, as before)
            for c in sorted(set(which)):
                members = [q for q in range(nq) if which[q] == c]
                res = ix.search_batch(queries[members], limit=limit, row_mask=None if c < 0 else masks[c])
                for q, r in zip(members, res):
                    out[q] = r
            return out
        shards = range(len(self.indices))
        return list(self._shard_pool.map(one, shards)) if len(self.indices) > 1 else [one(0)]

    def search_batch(self, queries, limit: int = 10, threshold: float = 0.0,
                     filter_metadata=None, prefilter: Optional[bool] = None) -> List[List[Result]]:
        """Extension: one corpus pass per shard for a whole query batch -- through the shard group when there is
        one (every shard runs its matrix-core pass, or per-query scans for a few queries, inside ONE library call, the
        lists are exchanged and merged on the device), else shard by shard on the shard pool.  ``prefilter`` / FILTER_PUSHDOWN
        as in ``search``: the filter's row masks travel with the call (one MASKED matrix-core pass per shard), so every query
        returns a full ``limit`` whenever enough rows match; the default post-filters the top-``limit`` as before.
        ``filter_metadata`` may be a LIST holding one filter or ``None`` per query (any other length raises ``ValueError``):
        with push-down every shard still makes one call, with the distinct filters' masks and the per-query index."""
        queries = np.asarray(queries, dtype=np.float32)
        if queries.ndim != 2 or queries.shape[1] != self.vector_dim:
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {queries.shape}")
        if isinstance(filter_metadata, (list, tuple)):
            return self._search_batch_filters(queries, int(limit), threshold, list(filter_metadata), prefilter)
        masks = self._masks_for(filter_metadata, prefilter, gather=True)
        pushed = any(m is not None for m in masks)
        if queries.shape[0] and not self._has_lists(masks):
            merged = self._group_search(queries, limit, keep_all=bool(filter_metadata), masks=masks if pushed else None)
            if merged is not None:
                self.last_search_path = self._group_path
                return [self._merge([m], limit, threshold, filter_metadata) for m in merged]
        self.last_search_path = "threads"
        if pushed:
            def one(a):
                return a[0].search_batch(queries, limit=limit, row_mask=a[1])
            pairs = list(zip(self.indices, masks))
            per_shard = list(self._shard_pool.map(one, pairs)) if len(pairs) > 1 else [one(pairs[0])]
        elif len(self.indices) > 1:  # shards run concurrently (GIL-releasing calls), gathered in shard order
            per_shard = list(self._shard_pool.map(lambda ix: ix.search_batch(queries, limit=limit), self.indices))
        else:
            per_shard = [ix.search_batch(queries, limit=limit) for ix in self.indices]
        return [self._merge([res[q] for res in per_shard], limit, threshold, filter_metadata)
                for q in range(queries.shape[0])]

    # ---- search among listed ids (extension: the exact top-k of an explicit list of vectors) ----
    def _ids_by_shard(self, vector_ids) -> List[List[str]]:
        per: List[List[str]] = [[] for _ in self.indices]
        for vid in vector_ids:
            per[self._get_shard_for_id(vid)].append(vid)
        return per

    def search_batch_among(self, queries, vector_ids, limit: int = 10, threshold: float = 0.0) -> List[List[Result]]:
        """Per query the best ``limit`` among the vectors named by ``vector_ids`` only -- "rank these candidates", or a filter
        evaluated elsewhere -- with the merge semantics of ``search`` (threshold, cut, metadata attached).  Ids may come in
        any order and repeat; unknown and deleted ids are ignored; an empty list gives empty results.  The ids are split by
        shard and every shard holding some scores ITS listed rows exactly (the library's search among listed rows: the cost
        follows the list, not the shard), on the shard pool; no shard group, no coalescing."""
        queries = np.asarray(queries, dtype=np.float32)
        if queries.ndim != 2 or queries.shape[1] != self.vector_dim:
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {queries.shape}")
        self.last_search_path = "threads"
        if queries.shape[0] == 0:
            return []
        work = [(ix, ids) for ix, ids in zip(self.indices, self._ids_by_shard(vector_ids)) if ids]
        if not work:
            return [[] for _ in range(queries.shape[0])]

        def one(a):
            return a[0].search_batch_among(queries, a[1], limit=limit)
        per_shard = list(self._shard_pool.map(one, work)) if len(work) > 1 else [one(work[0])]
        return [self._merge([res[q] for res in per_shard], limit, threshold, None) for q in range(queries.shape[0])]

    def search_batch_among_each(self, queries, vector_id_lists, limit: int = 10, threshold: float = 0.0) -> List[List[Result]]:
        """``search_batch_among`` with one id list PER QUERY (``vector_id_lists[i]`` is query i's; any other length raises
        ``ValueError``): a rerank stage's candidates, a filter evaluated elsewhere per tenant.  Every query's ids are split
        by shard, and every shard holding some answers ALL its queries in one library call with a row list per query
        (``wdbx_index_search_row_lists``), on the shard pool; merged per query as ``search`` merges."""
        queries = np.asarray(queries, dtype=np.float32)
        if queries.ndim != 2 or queries.shape[1] != self.vector_dim:
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {queries.shape}")
        vector_id_lists = list(vector_id_lists)
        if len(vector_id_lists) != queries.shape[0]:
            raise ValueError(f"vector_id_lists holds {len(vector_id_lists)} lists for {queries.shape[0]} queries")
        self.last_search_path = "threads"
        nq = queries.shape[0]
        if nq == 0:
            return []
        split = [self._ids_by_shard(ids) for ids in vector_id_lists]  # [query][shard]
        work = [s for s in range(len(self.indices)) if any(split[q][s] for q in range(nq))]
        if not work:
            return [[] for _ in range(nq)]

        def one(s):
            return self.indices[s].search_batch_among_each(queries, [split[q][s] for q in range(nq)], limit=limit)
        per_shard = list(self._shard_pool.map(one, work)) if len(work) > 1 else [one(work[0])]
        return [self._merge([res[q] for res in per_shard], limit, threshold, None) for q in range(nq)]

    def search_among(self, query_vector: List[float], vector_ids, limit: int = 10, threshold: float = 0.0) -> List[Result]:
        query = _as_query(query_vector)
        if query.shape != (self.vector_dim,):
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {query.shape}")
        return self.search_batch_among(query[None, :], vector_ids, limit=limit, threshold=threshold)[0]

    async def search_among_async(self, query_vector: List[float], vector_ids, limit: int = 10,
                                 threshold: float = 0.0) -> List[Result]:
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(self.thread_pool, lambda: self.search_among(
            query_vector, vector_ids, limit=limit, threshold=threshold))

    # ---- distinct search (extension: at most one result per value of the metadata field DISTINCT_KEY) ----
    def search_distinct(self, query_vector: List[float], limit: int = 10, threshold: float = 0.0,
                        filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        """The best ``limit`` vectors with at most ONE per value of the metadata field named by config ``DISTINCT_KEY`` (ten
        documents, each by its best chunk, instead of the ten best chunks); a vector without the field stands for itself.
        Exact: every shard answers its own top-``limit`` labels (``wdbx_index_search_distinct``) -- a label in the global
        top-``limit`` is in the top-``limit`` of the shard that holds its best row --, the union keeps the best row of each
        label, ordered by (score descending, shard, row) and cut at ``limit``.  ``filter_metadata`` always travels as the
        shards' row masks (a post-filter could drop a label whose best row does not match); ``threshold`` as in
        ``search``."""
        if self.config.get("DISTINCT_KEY") is None:
            raise ValueError("search_distinct needs config DISTINCT_KEY: the metadata field whose values label the vectors")
        query = _as_query(query_vector)
        if query.shape != (self.vector_dim,):
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {query.shape}")
        masks = self._row_masks(filter_metadata) if filter_metadata else [None] * len(self.indices)
        work = list(zip(self.indices, masks))
        one = lambda a: a[0].search_distinct(query, limit, mask=a[1])  # noqa: E731
        per_shard = list(self._shard_pool.map(one, work)) if len(work) > 1 else [one(work[0])]
        # (a shard's list is ordered by (score descending, row ascending): the position stands for the row among equal scores)
        ranked = sorted(((-score, shard, pos, vid, label) for shard, res in enumerate(per_shard)
                         for pos, (vid, score, label) in enumerate(res)), key=lambda t: t[:3])
        seen, out = set(), []
        for neg, _, _, vid, label in ranked:
            if threshold > 0 and -neg < threshold:
                break
            if label != _native.LABEL_NONE:
                if label in seen:
                    continue
                seen.add(label)
            out.append((vid, -neg, self.metadata.get(vid, {})))
            if len(out) >= limit:
                break
        return out

    async def search_distinct_async(self, query_vector: List[float], limit: int = 10, threshold: float = 0.0,
                                    filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(self.thread_pool, lambda: self.search_distinct(
            query_vector, limit=limit, threshold=threshold, filter_metadata=filter_metadata))

    # ---- search groups (extension: the best values of DISTINCT_KEY, each with its best group_size vectors) ----
    def search_groups(self, query_vector: List[float], limit: int = 10, group_size: int = 3, threshold: float = 0.0,
                      filter_metadata: Optional[Dict[str, Any]] = None) -> List[Tuple[int, List[Result]]]:
        """``search_distinct`` with a group size: the best ``limit`` values of the metadata field named by config
        ``DISTINCT_KEY``, each with its best ``group_size`` vectors (ten documents, each with its three best chunks); a
        vector without the field is a group of its own.  Returns ``[(label, [(vector_id, score, metadata), ...])]``, groups
        and members best first.  One shard: one ``wdbx_index_search_groups`` call.  Several shards: every shard answers
        ``search_distinct``, the merge of ``search_distinct`` picks the global labels, every shard then answers
        ``group_members`` for them (a label's other rows may lie on shards where it did not make the top-``limit``), and
        each label's members are merged by (score descending, shard, position) and cut at ``group_size``.
        ``filter_metadata`` always travels as the shards' row masks.  ``threshold`` drops the groups whose best member is
        below it, and the members below it."""
        if self.config.get("DISTINCT_KEY") is None:
            raise ValueError("search_groups needs config DISTINCT_KEY: the metadata field whose values label the vectors")
        if int(group_size) < 1:
            raise ValueError(f"group_size must be at least 1, got {group_size}")
        query = _as_query(query_vector)
        if query.shape != (self.vector_dim,):
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {query.shape}")
        masks = self._row_masks(filter_metadata) if filter_metadata else [None] * len(self.indices)
        work = list(zip(self.indices, masks))
        if len(work) == 1:
            groups = work[0][0].search_groups(query, limit, group_size, mask=work[0][1])
        else:
            one = lambda a: a[0].search_distinct(query, limit, mask=a[1])  # noqa: E731
            per_shard = list(self._shard_pool.map(one, work))
            ranked = sorted(((-score, shard, pos, vid, label) for shard, res in enumerate(per_shard)
                             for pos, (vid, score, label) in enumerate(res)), key=lambda t: t[:3])
            seen, chosen = set(), []
            for _, _, _, vid, label in ranked:
                if label != _native.LABEL_NONE:
                    if label in seen:
                        continue
                    seen.add(label)
                chosen.append((label, vid))
                if len(chosen) >= limit:
                    break
            two = lambda a: a[0].group_members(query, chosen, group_size, mask=a[1])  # noqa: E731
            members = list(self._shard_pool.map(two, work))  # [shard][group] -> [(vid, score)]
            groups = []
            for gi, (label, _) in enumerate(chosen):
                merged = sorted(((-score, shard, pos, vid) for shard, res in enumerate(members)
                                 for pos, (vid, score) in enumerate(res[gi])), key=lambda t: t[:3])
                groups.append((label, [(vid, -neg) for neg, _, _, vid in merged[:int(group_size)]]))
        out = []
        for label, hits in groups:
            if threshold > 0:
                hits = [(vid, score) for vid, score in hits if score >= threshold]
            if hits:
                out.append((label, [(vid, score, self.metadata.get(vid, {})) for vid, score in hits]))
        return out

    async def search_groups_async(self, query_vector: List[float], limit: int = 10, group_size: int = 3, threshold: float = 0.0,
                                  filter_metadata: Optional[Dict[str, Any]] = None) -> List[Tuple[int, List[Result]]]:
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(self.thread_pool, lambda: self.search_groups(
            query_vector, limit=limit, group_size=group_size, threshold=threshold, filter_metadata=filter_metadata))

    # ---- multi-vector search (extension: late interaction over the documents DISTINCT_KEY names) ----
    def search_multivector(self, query_vectors: List[List[float]], limit: int = 10, threshold: float = 0.0,
                           filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        """Late interaction (MaxSim): the query is SEVERAL vectors, a document is every vector that shares a value of the
        metadata field named by config ``DISTINCT_KEY`` (a vector without the field is a document of its own), and a
        document's score is the sum over the query's vectors of that vector's best score among the document's vectors.
        Returns the best ``limit`` documents as ``(vector_id, score, metadata)`` of each document's representative (its
        first stored vector).  ``filter_metadata`` always travels as the row mask: only matching vectors stand for their
        document.  ``threshold`` as in ``search``, on the summed score.  One shard only: vectors are placed by the hash of
        their id, so a document's vectors lie in several shards, and per-vector maxima do not compose from per-shard
        rankings."""
        if self.config.get("DISTINCT_KEY") is None:
            raise ValueError("search_multivector needs config DISTINCT_KEY: the metadata field whose values name the documents")
        if len(self.indices) != 1:
            raise ValueError(
                f"search_multivector needs a store of one shard, this one has {len(self.indices)}: vectors are placed by the hash "
                "of their id, so a document's vectors lie in several shards, and a document's per-vector maxima (and their sum) "
                "do not compose from per-shard rankings")
        queries = [_as_query(v) for v in query_vectors]
        if not queries:
            raise ValueError("query_vectors is empty")
        for q in queries:
            if q.shape != (self.vector_dim,):
                raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {q.shape}")
        mask = self._row_masks(filter_metadata)[0] if filter_metadata else None
        out = []
        for vid, score, _ in self.indices[0].search_multivector(queries, limit, mask=mask):
            if threshold > 0 and score < threshold:
                break
            out.append((vid, score, self.metadata.get(vid, {})))
        return out[:limit]

    async def search_multivector_async(self, query_vectors: List[List[float]], limit: int = 10, threshold: float = 0.0,
                                       filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(self.thread_pool, lambda: self.search_multivector(
            query_vectors, limit=limit, threshold=threshold, filter_metadata=filter_metadata))

    # ---- MMR search (extension: a diversified top-limit picked from the pool of the best vectors) ----
    def search_mmr(self, query_vector: List[float], limit: int = 10, fetch_k: Optional[int] = None, lambda_mult: float = 0.5,
                   threshold: float = 0.0, filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        """Maximal marginal relevance: ``limit`` vectors picked greedily from the ``fetch_k`` best (default
        ``min(WDBX_MAX_K, 4 * limit)``), each pick the candidate with the largest ``lambda_mult * relevance - (1 -
        lambda_mult) * (its largest similarity to a vector already picked)`` -- ten near-identical chunks no longer fill the
        answer.  Returned in PICK order as ``(vector_id, score, metadata)``, scores as ``search`` returns them.
        ``filter_metadata`` always travels as the row mask, so the pool holds matching vectors only; ``threshold`` drops the
        picks whose relevance is below it, as in ``search``.  One shard only: the pairwise similarities need both rows on
        one device, and a pick depends on every earlier pick, so per-shard answers do not compose; cross-shard MMR is out of
        scope."""
        if len(self.indices) != 1:
            raise ValueError(
                f"search_mmr needs a store of one shard, this one has {len(self.indices)}: the similarity of two candidates "
                "needs both rows on one device, and per-shard selections do not compose")
        query = _as_query(query_vector)
        if query.shape != (self.vector_dim,):
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {query.shape}")
        if not 0.0 <= float(lambda_mult) <= 1.0:
            raise ValueError(f"lambda_mult must lie in [0, 1], got {lambda_mult}")
        if fetch_k is not None and int(fetch_k) < int(limit):
            raise ValueError(f"fetch_k={fetch_k} is below limit={limit}")
        mask = self._row_masks(filter_metadata)[0] if filter_metadata else None
        out = []
        for vid, score, _ in self.indices[0].search_mmr(query, limit, fetch_k=fetch_k, lambda_mult=lambda_mult, mask=mask):
            if threshold > 0 and score < threshold:
                continue  # (pick order is not score order: a later pick may still pass)
            out.append((vid, score, self.metadata.get(vid, {})))
        return out[:limit]

    async def search_mmr_async(self, query_vector: List[float], limit: int = 10, fetch_k: Optional[int] = None,
                               lambda_mult: float = 0.5, threshold: float = 0.0,
                               filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(self.thread_pool, lambda: self.search_mmr(
            query_vector, limit=limit, fetch_k=fetch_k, lambda_mult=lambda_mult, threshold=threshold,
            filter_metadata=filter_metadata))

    # ---- recommend search (extension: rank by positive and negative examples) ----
    def _resolve_examples(self, examples, what: str):
        """Examples are stored vector ids or raw vectors: ``(vectors, ids)``, the ids resolved with :meth:`get`."""
        vectors, ids = [], []
        for i, e in enumerate(examples or ()):
            if isinstance(e, str):
                got = self.get(e)
                if got is None:
                    raise ValueError(f"{what}[{i}]: no stored vector has the id {e!r}")
                ids.append(e)
                e = got[0]
            v = _as_query(e)
            if v.shape != (self.vector_dim,):
                raise ValueError(f"{what}[{i}]: vector dimension mismatch: expected {self.vector_dim}, got {v.shape}")
            vectors.append(v)
        return vectors, ids

    def recommend(self, positive, negative=None, limit: int = 10, strategy: str = "best_score",
                  filter_metadata: Optional[Dict[str, Any]] = None, with_side: bool = False) -> List[tuple]:
        """"More like these, less like those": ``positive`` and ``negative`` are lists whose items are stored vector ids or
        raw vectors; every example that is an id never comes back.  ``strategy="best_score"`` (Qdrant's, without its
        sigmoid): per vector ``p`` is its best score over the positives and ``n`` over the negatives; vectors with ``p > n``
        (favoured) come first by ``p`` descending, the others follow by ``n`` ascending.  The fold is per vector, so any
        number of shards serves: every shard returns its own top-``limit`` (``wdbx_index_search_recommend``, the id examples
        excluded on the shard that holds them), the merge takes favoured results by (score descending, shard, position),
        then disfavoured ones by (``n`` ascending, shard, position), cut at ``limit``.  ``strategy="average_vector"`` needs
        no pass of its own: the query is ``avg(pos) + (avg(pos) - avg(neg))`` through :meth:`search` with ``limit`` + the
        number of id examples, which are then dropped.  ``filter_metadata`` always travels as the row masks.  Returns
        ``(vector_id, score, metadata)``, with ``side`` (1 favoured, 0 disfavoured; always 1 for ``average_vector``) appended
        when ``with_side`` is set."""
        if strategy not in ("best_score", "average_vector"):
            raise ValueError(f'strategy must be "best_score" or "average_vector", got {strategy!r}')
        pos, pos_ids = self._resolve_examples(positive, "positive")
        neg, neg_ids = self._resolve_examples(negative, "negative")
        if not pos:
            raise ValueError("recommend needs at least one positive example")
        if len(pos) + len(neg) > _native.MAX_EXAMPLES:
            raise ValueError(f"{len(pos) + len(neg)} examples, at most {_native.MAX_EXAMPLES} are served")
        example_ids = set(pos_ids) | set(neg_ids)
        if limit <= 0:
            return []
        if strategy == "average_vector":
            avg = np.mean(np.stack(pos), axis=0, dtype=np.float32)
            query = avg + (avg - np.mean(np.stack(neg), axis=0, dtype=np.float32)) if neg else avg
            found = self.search(query.tolist(), limit=limit + len(example_ids), threshold=0.0, filter_metadata=filter_metadata,
                                **({"prefilter": True} if filter_metadata else {}))
            out = [(vid, score, meta) + ((1,) if with_side else ()) for vid, score, meta in found if vid not in example_ids]
            return out[:limit]
        masks = self._row_masks(filter_metadata) if filter_metadata else [None] * len(self.indices)
        by_shard = [[] for _ in self.indices]
        for vid in example_ids:
            by_shard[self._get_shard_for_id(vid)].append(vid)
        work = list(zip(self.indices, masks, by_shard))
        one = lambda a: a[0].recommend(pos, neg, limit, mask=a[1], exclude_ids=a[2])  # noqa: E731
        per_shard = list(self._shard_pool.map(one, work)) if len(work) > 1 else [one(work[0])]
        # (a shard's list is favoured first by (p descending, row), then disfavoured by (n ascending, row): within a side the
        # position stands for the row among equal scores)
        ranked = sorted(((0, -score, shard, at) if side else (1, score, shard, at), vid, score, side)
                        for shard, res in enumerate(per_shard) for at, (vid, score, side) in enumerate(res))
        return [(vid, score, self.metadata.get(vid, {})) + ((side,) if with_side else ()) for _, vid, score, side in ranked[:limit]]

    async def recommend_async(self, positive, negative=None, limit: int = 10, strategy: str = "best_score",
                              filter_metadata: Optional[Dict[str, Any]] = None, with_side: bool = False) -> List[tuple]:
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(self.thread_pool, lambda: self.recommend(
            positive, negative, limit=limit, strategy=strategy, filter_metadata=filter_metadata, with_side=with_side))

    # ---- discovery search (extension: rank by context pairs and a target) ----
    def discover(self, target=None, context=(), limit: int = 10, filter_metadata: Optional[Dict[str, Any]] = None,
                 with_wins: bool = False) -> List[tuple]:
        """Discovery: ``context`` is a list of (positive, negative) pairs and ``target`` an optional vector; the target and
        every pair element are each a stored vector id or a raw vector, and every one that is an id never comes back.  A
        pair is won by a vector that scores higher against its positive than against its negative.  With a target, vectors
        rank by (pairs won descending, target score descending); without one (context search, at least one pair) by the
        loss, the sum over the pairs of ``min(score(positive) - score(negative), 0)``, descending: vectors on the right side
        of every pair have loss 0.  The fold is per vector, so any number of shards serves: every shard gets the same
        vectors and returns its own top-``limit`` (``wdbx_index_search_discover``, the id examples excluded on the shard that
        holds them); the merge takes (wins descending, score descending, shard, position) with a target and (loss
        descending, shard, position) without.  ``filter_metadata`` always travels as the row masks.  Returns ``(vector_id,
        score, metadata)`` -- the score is the target's, or the loss -- with the pairs won appended when ``with_wins`` is
        set (0 in a context search)."""
        pairs, ids = [], []
        for i, pair in enumerate(context or ()):
            if isinstance(pair, dict):
                pair = (pair.get("positive"), pair.get("negative"))
            if isinstance(pair, (str, bytes)) or len(pair) != 2:
                raise ValueError(f"context[{i}]: a pair (positive, negative) is needed")
            vs, got = self._resolve_examples(list(pair), f"context[{i}]")
            pairs.append((vs[0], vs[1]))
            ids += got
        tgt = None
        if target is not None:
            vs, got = self._resolve_examples([target], "target")
            tgt = vs[0]
            ids += got
        if tgt is None and not pairs:
            raise ValueError("discover needs a target or at least one context pair")
        if len(pairs) > _native.MAX_CONTEXT_PAIRS:
            raise ValueError(f"{len(pairs)} context pairs, at most {_native.MAX_CONTEXT_PAIRS} are served")
        if limit <= 0:
            return []
        masks = self._row_masks(filter_metadata) if filter_metadata else [None] * len(self.indices)
        by_shard = [[] for _ in self.indices]
        for vid in set(ids):
            by_shard[self._get_shard_for_id(vid)].append(vid)
        work = list(zip(self.indices, masks, by_shard))
        one = lambda a: a[0].discover(tgt, pairs, limit, mask=a[1], exclude_ids=a[2])  # noqa: E731
        per_shard = list(self._shard_pool.map(one, work)) if len(work) > 1 else [one(work[0])]
        # (a shard's list is already in the order below with the row last: the position stands for the row among equals)
        ranked = sorted(((-wins, -score, shard, at), vid, score, wins)
                        for shard, res in enumerate(per_shard) for at, (vid, score, wins) in enumerate(res))
        return [(vid, score, self.metadata.get(vid, {})) + ((wins,) if with_wins else ()) for _, vid, score, wins in ranked[:limit]]

    async def discover_async(self, target=None, context=(), limit: int = 10, filter_metadata: Optional[Dict[str, Any]] = None,
                             with_wins: bool = False) -> List[tuple]:
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(self.thread_pool, lambda: self.discover(
            target, context, limit=limit, filter_metadata=filter_metadata, with_wins=with_wins))

    # ---- distance matrix (extension: each sampled vector's nearest among the sample) ----
    def _matrix_sample(self, sample: int, filter_metadata, vector_ids, seed) -> List[str]:
        """The sampled ids, sorted: the explicit ``vector_ids`` (known ones, once each), else ``sample`` of the ids the filter
        matches -- the evaluation ``_row_masks`` caches -- or of every id, drawn by ``random.Random(seed)`` from the sorted ids."""
        if vector_ids is not None:
            chosen = sorted({vid for vid in vector_ids if self._known(vid)})
        else:
            if isinstance(sample, bool) or not isinstance(sample, int) or sample < 0:
                raise ValueError("sample must be a non-negative integer")
            masks = self._row_masks(filter_metadata) if filter_metadata else [None] * len(self.indices)
            pool = sorted(vid for ix, mask in zip(self.indices, masks) for vid in ix.mapped_ids(mask))
            chosen = sorted(random.Random(seed).sample(pool, min(sample, len(pool))))
        cap = int(self.config.get("MATRIX_MAX_SAMPLE", 10000))
        if len(chosen) > cap:
            raise ValueError(f"a distance matrix over {len(chosen)} vectors: MATRIX_MAX_SAMPLE allows {cap}")
        return chosen

    def search_matrix(self, sample: int = 10, limit: int = 3, filter_metadata: Optional[Dict[str, Any]] = None,
                      vector_ids=None, seed=None) -> List[Tuple[str, List[Tuple[str, float]]]]:
        """Distance matrix: for every sampled vector its ``limit`` nearest among the OTHER sampled vectors, the stored vector
        being the query -- ``[(id, [(neighbour id, score), ...]), ...]`` in sorted id order, what clustering, a 2-D layout or
        a near-duplicate report reads.  The sample is ``vector_ids`` when given (unknown and deleted ids are ignored), else
        ``sample`` of the vectors ``filter_metadata`` matches (of all vectors without one), drawn by
        ``random.Random(seed)``: with a seed the same store gives the same sample.  More than ``MATRIX_MAX_SAMPLE``
        sampled vectors is a ``ValueError``.  A vector is never its own neighbour; another vector equal to it is one.
        One shard: one library call (``wdbx_index_search_matrix``), no vector leaves the device.  Several shards: every shard
        answers its own sampled rows that way; its anchors' stored vectors are read once and go, as they are (nothing is
        normalised again), to every other shard holding sampled rows, which ranks them among ITS part of the sample
        (``wdbx_index_search_rows``); per anchor the parts are merged in ``_merge``'s order and cut to ``limit``.  Both
        calls return the same score bits, so the merged lines are what one shard holding everything would return (up to
        the order of exactly tied scores).  On the shard pool; never through the shard group."""
        chosen = self._matrix_sample(sample, filter_metadata, vector_ids, seed)
        self.last_search_path = "threads"
        if not chosen:
            return []
        if limit <= 0:
            return [(vid, []) for vid in chosen]
        per = self._ids_by_shard(chosen)
        work = [s for s, ids in enumerate(per) if ids]
        own = list(self._shard_pool.map(lambda s: self.indices[s].search_matrix(per[s], limit), work)) if len(work) > 1 \
            else [self.indices[work[0]].search_matrix(per[work[0]], limit)]
        parts: Dict[str, List[List[Tuple[str, float]]]] = {}  # anchor -> its lists, in shard order
        if len(work) == 1:
            parts = {anchor: [res] for anchor, res in own[0]}
        else:
            stored = list(self._shard_pool.map(lambda s: self.indices[s].stored_vectors(per[s]), work))
            cross = [(a, b) for a in range(len(work)) for b in range(len(work)) if a != b and len(stored[a][0])]

            def one(ab):  # shard work[a]'s anchors among shard work[b]'s part of the sample
                a, b = ab
                return self.indices[work[b]].search_batch_among(stored[a][1], per[work[b]], limit=limit, normalize=False)
            answers = dict(zip(cross, self._shard_pool.map(one, cross)))
            for a in range(len(work)):
                mine = dict(own[a])
                for at, anchor in enumerate(stored[a][0]):
                    parts[anchor] = [mine.get(anchor, []) if b == a else answers[(a, b)][at] for b in range(len(work))]
        return [(anchor, [(vid, score) for vid, score, _ in self._merge(parts[anchor], limit, 0.0, None)])
                for anchor in chosen if anchor in parts]

    async def search_matrix_async(self, sample: int = 10, limit: int = 3, filter_metadata: Optional[Dict[str, Any]] = None,
                                  vector_ids=None, seed=None) -> List[Tuple[str, List[Tuple[str, float]]]]:
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(self.thread_pool, lambda: self.search_matrix(
            sample, limit, filter_metadata=filter_metadata, vector_ids=vector_ids, seed=seed))

    # ---- range search (extension: every vector within a similarity, no limit) ----
    def search_range(self, query_vector: List[float], threshold: float,
                     filter_metadata: Optional[Dict[str, Any]] = None, prefilter: Optional[bool] = None,
                     max_results: Optional[int] = None) -> List[Result]:
        """Every stored vector whose score reaches ``threshold`` (``score >= threshold`` in the scores ``search`` returns:
        cosine similarity, for L2 the negated squared distance), best first, cut to ``max_results`` only after sorting and
        filtering (None = all).  Unlike ``search(limit, threshold)``, which ranks a top-``limit`` and then drops what is
        below the threshold, nothing is lost to a limit.  Each shard answers with the library's range search (on the shard
        pool, gathered in shard order); no shard group and no coalescing.  ``prefilter`` / FILTER_PUSHDOWN as in
        ``search``: without ``max_results`` the pushed-down filter and the post-filter give the same list."""
        query = _as_query(query_vector)
        if query.shape != (self.vector_dim,):
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {query.shape}")
        masks = self._masks_for(filter_metadata, prefilter)
        if len(self.indices) > 1:
            shard_results = list(self._shard_pool.map(lambda a: a[0].range_search(query, threshold, row_mask=a[1]),
                                                      zip(self.indices, masks)))
        else:
            shard_results = [ix.range_search(query, threshold, row_mask=m) for ix, m in zip(self.indices, masks)]
        return merge_range(shard_results, self.metadata, filter_metadata, max_results)

    async def search_range_async(self, query_vector: List[float], threshold: float,
                                 filter_metadata: Optional[Dict[str, Any]] = None, prefilter: Optional[bool] = None,
                                 max_results: Optional[int] = None) -> List[Result]:
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(self.thread_pool, lambda: self.search_range(
            query_vector, threshold, filter_metadata=filter_metadata, prefilter=prefilter, max_results=max_results))

    def search_range_batch(self, query_vectors: List[List[float]], thresholds,
                           filter_metadata: Optional[Dict[str, Any]] = None, prefilter: Optional[bool] = None,
                           max_results: Optional[int] = None) -> List[List[Result]]:
        """``search_range`` for a batch of queries: one result list per query, each exactly what ``search_range`` returns for
        that query (near-duplicate detection, threshold retrieval for a page of items, cluster assignment).  ``thresholds``
        is a scalar or one per query.  One call per shard for the whole batch (the library's batched range search: one int8
        tile pass per block of up to 256 queries), then ``merge_range`` per query over the shards.  ONE filter for the
        batch: the row mask of every shard's call when ``prefilter`` / FILTER_PUSHDOWN says so, else the post-filter of
        ``search_range``; ``max_results`` cuts each query's list."""
        queries = [_as_query(v) for v in query_vectors]
        for q in queries:
            if q.shape != (self.vector_dim,):
                raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {q.shape}")
        nq = len(queries)
        t = np.asarray(thresholds, dtype=np.float64)
        if t.ndim > 1 or (t.ndim == 1 and t.shape[0] != nq):
            raise ValueError(f"thresholds: a scalar or one per query ({nq}), got shape {t.shape}")
        if np.isnan(t).any():
            raise ValueError("threshold is NaN")
        if nq == 0:
            return []
        t = np.ascontiguousarray(np.broadcast_to(t, (nq,)))
        batch = np.stack(queries)
        masks = self._masks_for(filter_metadata, prefilter)
        if len(self.indices) > 1:
            per_shard = list(self._shard_pool.map(lambda a: a[0].range_search_batch(batch, t, row_mask=a[1]),
                                                  zip(self.indices, masks)))
        else:
            per_shard = [ix.range_search_batch(batch, t, row_mask=m) for ix, m in zip(self.indices, masks)]
        return [merge_range([shard[i] for shard in per_shard], self.metadata, filter_metadata, max_results)
                for i in range(nq)]

    async def search_range_batch_async(self, query_vectors: List[List[float]], thresholds,
                                       filter_metadata: Optional[Dict[str, Any]] = None, prefilter: Optional[bool] = None,
                                       max_results: Optional[int] = None) -> List[List[Result]]:
        loop = asyncio.get_running_loop()
        return await loop.run_in_executor(self.thread_pool, lambda: self.search_range_batch(
            query_vectors, thresholds, filter_metadata=filter_metadata, prefilter=prefilter, max_results=max_results))

    # ---- row management ----
    def _known(self, vector_id: str) -> bool:
        return vector_id in self.vectors or self._is_bulk(vector_id)

    def _forget(self, vector_id: str) -> None:
        self.vectors.pop(vector_id, None)
        self.metadata.pop(vector_id, None)
        self._bulk_id_shard.pop(vector_id, None)
        self._meta_version += 1  # cached push-down masks name rows by position: rebuild them

    def delete(self, vector_id: str) -> bool:
        if not self._known(vector_id):
            return False
        self.indices[self._get_shard_for_id(vector_id)].remove(vector_id)
        self._forget(vector_id)
        if self.config.get("VECTOR_STORE_SAVE_IMMEDIATELY", False):
            self._save_now()
        return True

    async def delete_async(self, vector_id: str) -> bool:
        if not self._known(vector_id):
            return False
        await self.indices[self._get_shard_for_id(vector_id)].remove_async(vector_id)
        self._forget(vector_id)
        if self.config.get("VECTOR_STORE_SAVE_IMMEDIATELY", False):
            await asyncio.get_event_loop().run_in_executor(self.thread_pool, self._save_now)
        return True

    def delete_many(self, vector_ids) -> int:
        """``delete`` for many ids: the ids split by shard, ONE native removal per shard (``HipFlatIndex.remove_many``), the
        bookkeeping of ``delete`` once per call.  Unknown ids are skipped; returns how many were present."""
        by_shard: Dict[int, List[str]] = {}
        seen = set()
        for vector_id in vector_ids:
            if vector_id in seen or not self._known(vector_id):
                continue
            seen.add(vector_id)
            by_shard.setdefault(self._get_shard_for_id(vector_id), []).append(vector_id)
        if not seen:
            return 0
        for shard, ids in by_shard.items():
            self.indices[shard].remove_many(ids)
        for vector_id in seen:
            self.vectors.pop(vector_id, None)
            self.metadata.pop(vector_id, None)
            self._bulk_id_shard.pop(vector_id, None)
        self._meta_version += 1  # cached push-down masks name rows by position: rebuild them
        if self.config.get("VECTOR_STORE_SAVE_IMMEDIATELY", False):
            self._save_now()
        return len(seen)

    async def delete_many_async(self, vector_ids) -> int:
        ids = list(vector_ids)
        return await asyncio.get_event_loop().run_in_executor(self.thread_pool, self.delete_many, ids)

    def delete_by_filter(self, filter_metadata: Dict[str, Any]) -> int:
        """Delete every stored id whose metadata matches ``filter_metadata`` (the matcher of the filtered searches, evaluated
        on the host); an empty filter deletes nothing.  Returns how many ids were deleted."""
        if not filter_metadata:
            return 0
        return self.delete_many([vid for vid in list(self.metadata) if self._matches_filter(vid, filter_metadata)])

    async def delete_by_filter_async(self, filter_metadata: Dict[str, Any]) -> int:
        return await asyncio.get_event_loop().run_in_executor(self.thread_pool, self.delete_by_filter, filter_metadata)

    def _set_metadata(self, vector_id: str, metadata: Dict[str, Any]) -> bool:
        if not self._known(vector_id):
            return False
        self.metadata[vector_id] = metadata
        self._meta_version += 1
        self._push_labels([vector_id])
        return True

    def update_metadata(self, vector_id: str, metadata: Dict[str, Any]) -> bool:
        if not self._set_metadata(vector_id, metadata):
            return False
        if self.config.get("VECTOR_STORE_SAVE_IMMEDIATELY", False):
            self._save_metadata()
        return True

    async def update_metadata_async(self, vector_id: str, metadata: Dict[str, Any]) -> bool:
        if not self._set_metadata(vector_id, metadata):
            return False
        if self.config.get("VECTOR_STORE_SAVE_IMMEDIATELY", False):
            await asyncio.get_event_loop().run_in_executor(self.thread_pool, self._save_metadata)
        return True

    def get(self, vector_id: str) -> Optional[Tuple[List[float], Dict[str, Any]]]:
        if vector_id not in self.vectors:
            ix = self.indices[self._get_shard_for_id(vector_id)]
            row = ix._row_of(vector_id)
            if row is None:
                return None
            return ix._native.get_rows(row, 1)[0].tolist(), self.metadata.get(vector_id, {})
        return self.vectors[vector_id].tolist(), self.metadata.get(vector_id, {})

    async def get_async(self, vector_id: str) -> Optional[Tuple[List[float], Dict[str, Any]]]:
        return self.get(vector_id)

    def count(self) -> int:
        """Rows that still have an id, over all shards (explicit ids + implicit bulk rows - removed ones): what a search
        can return.  Equals the reference's ``len(self.vectors)`` (vector_store.py:651) for per-vector ingest."""
        return sum(ix.size() for ix in self.indices)

    def _forget_bulk(self) -> None:
        self._bulk_ranges, self._bulk_id_shard, self._bulk_rows = [], {}, 0
        self._meta_version += 1

    def clear(self) -> int:
        removed = self.count()
        for ix in self.indices:
            ix.clear()
        self.vectors, self.metadata = {}, {}
        self._forget_bulk()
        self._save_now()
        return removed

    async def clear_async(self) -> int:
        removed = self.count()
        await asyncio.gather(*[ix.clear_async() for ix in self.indices])
        self.vectors, self.metadata = {}, {}
        self._forget_bulk()
        await asyncio.get_event_loop().run_in_executor(self.thread_pool, self._save_now)
        return removed

    def get_stats(self) -> Dict[str, Any]:
        return {
            "vector_count": self.count(),
            "metadata_count": len(self.metadata),
            "index_type": self.index_type,
            "num_shards": self.num_shards,
            "vector_dim": self.vector_dim,
            "use_gpu": self.use_gpu,
            "indices": [{"shard": i, "type": self.index_type, "size": ix.size(), "stats": ix.get_stats()}
                        for i, ix in enumerate(self.indices)],
        }

    def _after_optimize(self) -> None:
        self._meta_version += 1  # cached push-down masks name rows by position: rebuild them
        self._mask_cache.clear()

    def optimize(self) -> bool:
        """vector_store.py:696-713: every shard's ``optimize`` (here: compaction of removed rows, indexing.py)."""
        ok = all([ix.optimize() for ix in self.indices])
        self._after_optimize()
        return ok

    async def optimize_async(self) -> bool:
        res = await asyncio.gather(*[ix.optimize_async() for ix in self.indices])
        self._after_optimize()
        return all(res)
