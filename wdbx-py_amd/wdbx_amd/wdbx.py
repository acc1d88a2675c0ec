"""The ``WDBX`` facade for the hot path (reference: wdbx/core/wdbx.py:21-502):
constructor signature, ``initialize/shutdown``, ``vector_store[_async]``,
``vector_search[_async]``, row management and ``get_stats`` keep the reference's
names, arguments, return shapes and error text.  Plugins and the TCP
``ShardManager`` are out of scope; ``enable_plugins`` /
``enable_distributed`` are accepted and recorded only."""

from __future__ import annotations

import logging
import uuid
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

from . import _native
from .config import WDBXConfig
from .vector_store import VectorStore

logger = logging.getLogger(__name__)

Result = Tuple[str, float, Dict[str, Any]]


class WDBX:
    def __init__(
        self,
        vector_dimension: int = 384,
        num_shards: int = 1,
        data_dir: str = "./wdbx_data",
        config: Optional[Dict[str, Any]] = None,
        enable_plugins: bool = True,
        enable_distributed: bool = False,
        enable_gpu: bool = False,
        log_level: str = "INFO",
    ):
        """Same signature and defaults as the reference (wdbx.py:36-46).  ``enable_gpu`` is plumbed to the store and
        its indices exactly as there (:124); this backend always runs on the GPU -- see ``HipFlatIndex.__init__`` for
        what the flag means here (recorded, reported in ``get_stats`` as given, one warning when it is False)."""
        level = getattr(logging, log_level.upper(), None)
        if not isinstance(level, int):
            raise ValueError(f"Invalid log level: {log_level}")
        if not logging.getLogger().handlers:
            logging.basicConfig(level=level, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s",
                                datefmt="%Y-%m-%d %H:%M:%S")
        self.vector_dim = vector_dimension
        self.num_shards = num_shards
        self.data_dir = Path(data_dir)
        self.config = WDBXConfig(config or {})
        self.enable_plugins = enable_plugins
        self.enable_distributed = enable_distributed
        self.enable_gpu = enable_gpu
        self.data_dir.mkdir(parents=True, exist_ok=True)

        # ``vector_store`` is the store object AND the store call (see VectorStore.__call__)
        self.vector_store = VectorStore(
            vector_dim=self.vector_dim,
            data_dir=self.data_dir,
            num_shards=self.num_shards,
            use_gpu=self.enable_gpu,
            index_type=self.config.get("INDEX_TYPE", "hip"),
            config=self.config,
        )
        self.plugins: Dict[str, Any] = {}
        self.shard_manager = None
        logger.info("WDBX initialized successfully with vector_dim=%d, num_shards=%d", self.vector_dim,
                    self.num_shards)

    @property
    def version(self) -> str:
        from . import __version__

        return __version__

    async def initialize(self):
        await self.vector_store.initialize()

    async def shutdown(self):
        await self.vector_store.shutdown()

    # ---- plugin registry (callers of the path; kept so embedding providers can register) ----
    def get_plugin(self, plugin_name: str):
        if not self.enable_plugins:
            return None
        return self.plugins.get(plugin_name)

    def register_plugin(self, plugin) -> bool:
        if not self.enable_plugins or plugin.name in self.plugins:
            return False
        self.plugins[plugin.name] = plugin
        return True

    # ---- store ----
    def _check_dim(self, vector) -> None:
        if len(vector) != self.vector_dim:
            raise ValueError(f"Vector dimension mismatch: expected {self.vector_dim}, got {len(vector)}")

    async def vector_store_async(self, vector: List[float], metadata: Optional[Dict[str, Any]] = None,
                                 id: Optional[str] = None) -> str:
        self._check_dim(vector)
        vector_id = id or str(uuid.uuid4())
        await self.vector_store.store_async(vector_id, vector, metadata)
        return vector_id

    # ---- search ----
    def vector_search(self, query_vector: List[float], limit: int = 10, threshold: float = 0.0,
                      filter_metadata: Optional[Dict[str, Any]] = None,
                      prefilter: Optional[bool] = None) -> List[Result]:
        self._check_dim(query_vector)
        return self.vector_store.search(query_vector, limit=limit, threshold=threshold,
                                        filter_metadata=filter_metadata, prefilter=prefilter)

    async def vector_search_async(self, query_vector: List[float], limit: int = 10, threshold: float = 0.0,
                                  filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        self._check_dim(query_vector)
        return await self.vector_store.search_async(query_vector, limit=limit, threshold=threshold,
                                                    filter_metadata=filter_metadata)

    def vector_search_batch(self, query_vectors, limit: int = 10, threshold: float = 0.0,
                            filter_metadata=None, prefilter: Optional[bool] = None) -> List[List[Result]]:
        """Extension: several queries at once (the reference is single-query).  ``prefilter`` as in
        ``vector_search``: the metadata filter is pushed down into the batched pass.  ``filter_metadata``: one filter for
        the batch, or a LIST with one filter or ``None`` per query (``VectorStore.search_batch``)."""
        for q in query_vectors:
            self._check_dim(q)
        return self.vector_store.search_batch(query_vectors, limit=limit, threshold=threshold,
                                              filter_metadata=filter_metadata, prefilter=prefilter)

    def vector_search_among(self, query_vector: List[float], vector_ids, limit: int = 10,
                            threshold: float = 0.0) -> List[Result]:
        """Extension: the best ``limit`` among the vectors named by ``vector_ids`` only (re-ranking a candidate list, a filter
        evaluated elsewhere); unknown and deleted ids are ignored.  Costs what the listed vectors cost, not the store."""
        self._check_dim(query_vector)
        return self.vector_store.search_among(query_vector, vector_ids, limit=limit, threshold=threshold)

    def vector_search_batch_among(self, query_vectors, vector_ids, limit: int = 10,
                                  threshold: float = 0.0) -> List[List[Result]]:
        for q in query_vectors:
            self._check_dim(q)
        return self.vector_store.search_batch_among(query_vectors, vector_ids, limit=limit, threshold=threshold)

    def vector_search_batch_among_each(self, query_vectors, vector_id_lists, limit: int = 10,
                                       threshold: float = 0.0) -> List[List[Result]]:
        """Extension: ``vector_search_among`` for a batch whose queries each bring THEIR OWN id list (``vector_id_lists[i]``
        is query i's; another length raises ``ValueError``), one library call per shard for the whole batch."""
        for q in query_vectors:
            self._check_dim(q)
        return self.vector_store.search_batch_among_each(query_vectors, vector_id_lists, limit=limit, threshold=threshold)

    async def vector_search_among_async(self, query_vector: List[float], vector_ids, limit: int = 10,
                                        threshold: float = 0.0) -> List[Result]:
        self._check_dim(query_vector)
        return await self.vector_store.search_among_async(query_vector, vector_ids, limit=limit, threshold=threshold)

    def vector_search_distinct(self, query_vector: List[float], limit: int = 10, threshold: float = 0.0,
                               filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        """Extension: the best ``limit`` vectors with at most one per value of the metadata field named by config
        ``DISTINCT_KEY`` (search groups / collapse: ten documents, each by its best chunk).  Exact; a filter is pushed down."""
        self._check_dim(query_vector)
        return self.vector_store.search_distinct(query_vector, limit=limit, threshold=threshold,
                                                 filter_metadata=filter_metadata)

    async def vector_search_distinct_async(self, query_vector: List[float], limit: int = 10, threshold: float = 0.0,
                                           filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        self._check_dim(query_vector)
        return await self.vector_store.search_distinct_async(query_vector, limit=limit, threshold=threshold,
                                                             filter_metadata=filter_metadata)

    def _render_groups(self, groups) -> List[Dict[str, Any]]:
        key = self.vector_store.config.get("DISTINCT_KEY")
        out = []
        for _, hits in groups:
            meta = hits[0][2]
            out.append({"key": meta[key] if isinstance(meta, dict) and key in meta else hits[0][0], "hits": hits})
        return out

    def vector_search_groups(self, query_vector: List[float], limit: int = 10, group_size: int = 3, threshold: float = 0.0,
                             filter_metadata: Optional[Dict[str, Any]] = None) -> List[Dict[str, Any]]:
        """Extension: ``vector_search_distinct`` with a group size -- the best ``limit`` values of the metadata field named
        by config ``DISTINCT_KEY``, each with its best ``group_size`` vectors (ten documents, each with its three best
        chunks).  Each group is ``{"key": <the DISTINCT_KEY value, or the vector id of a vector without the field>, "hits":
        [(vector_id, score, metadata), ...]}``, groups and hits best first.  Exact; a filter is pushed down."""
        self._check_dim(query_vector)
        return self._render_groups(self.vector_store.search_groups(query_vector, limit=limit, group_size=group_size,
                                                                   threshold=threshold, filter_metadata=filter_metadata))

    async def vector_search_groups_async(self, query_vector: List[float], limit: int = 10, group_size: int = 3,
                                         threshold: float = 0.0,
                                         filter_metadata: Optional[Dict[str, Any]] = None) -> List[Dict[str, Any]]:
        self._check_dim(query_vector)
        return self._render_groups(await self.vector_store.search_groups_async(
            query_vector, limit=limit, group_size=group_size, threshold=threshold, filter_metadata=filter_metadata))

    def vector_search_multivector(self, query_vectors: List[List[float]], limit: int = 10, threshold: float = 0.0,
                                  filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        """Extension: late interaction (MaxSim).  The query is several vectors; the documents named by config ``DISTINCT_KEY``
        are ranked by the sum over the query's vectors of each vector's best score among the document's vectors.  Exact; a
        filter is pushed down; a store of one shard only (``VectorStore.search_multivector`` says why)."""
        for v in query_vectors:
            self._check_dim(v)
        return self.vector_store.search_multivector(query_vectors, limit=limit, threshold=threshold,
                                                    filter_metadata=filter_metadata)

    async def vector_search_multivector_async(self, query_vectors: List[List[float]], limit: int = 10, threshold: float = 0.0,
                                              filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        for v in query_vectors:
            self._check_dim(v)
        return await self.vector_store.search_multivector_async(query_vectors, limit=limit, threshold=threshold,
                                                                filter_metadata=filter_metadata)

    def vector_search_mmr(self, query_vector: List[float], limit: int = 10, fetch_k: Optional[int] = None,
                          lambda_mult: float = 0.5, threshold: float = 0.0,
                          filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        """Extension: maximal marginal relevance.  ``limit`` vectors picked greedily from the ``fetch_k`` best (default
        ``min(2048, 4 * limit)``), trading relevance (weight ``lambda_mult``) against similarity to the vectors already
        picked; returned in pick order.  A filter is pushed down; a store of one shard only (``VectorStore.search_mmr`` says
        why)."""
        self._check_dim(query_vector)
        return self.vector_store.search_mmr(query_vector, limit=limit, fetch_k=fetch_k, lambda_mult=lambda_mult,
                                            threshold=threshold, filter_metadata=filter_metadata)

    async def vector_search_mmr_async(self, query_vector: List[float], limit: int = 10, fetch_k: Optional[int] = None,
                                      lambda_mult: float = 0.5, threshold: float = 0.0,
                                      filter_metadata: Optional[Dict[str, Any]] = None) -> List[Result]:
        self._check_dim(query_vector)
        return await self.vector_store.search_mmr_async(query_vector, limit=limit, fetch_k=fetch_k, lambda_mult=lambda_mult,
                                                        threshold=threshold, filter_metadata=filter_metadata)

    def vector_recommend(self, positive, negative=None, limit: int = 10, strategy: str = "best_score",
                         filter_metadata: Optional[Dict[str, Any]] = None, with_side: bool = False) -> List[tuple]:
        """Extension: "more like these, less like those".  ``positive`` / ``negative``: lists of stored vector ids or raw
        vectors; id examples never come back.  ``strategy="best_score"``: vectors nearer to their best positive than to
        their best negative first, by that positive's score; the others follow, the one farthest from its nearest negative
        first.  ``"average_vector"``: one plain search with ``avg(pos) + (avg(pos) - avg(neg))``.  A filter is pushed down;
        any number of shards.  ``(vector_id, score, metadata)``, with ``side`` appended when ``with_side`` is set
        (``VectorStore.recommend`` states the order)."""
        return self.vector_store.recommend(positive, negative, limit=limit, strategy=strategy,
                                           filter_metadata=filter_metadata, with_side=with_side)

    async def vector_recommend_async(self, positive, negative=None, limit: int = 10, strategy: str = "best_score",
                                     filter_metadata: Optional[Dict[str, Any]] = None, with_side: bool = False) -> List[tuple]:
        return await self.vector_store.recommend_async(positive, negative, limit=limit, strategy=strategy,
                                                       filter_metadata=filter_metadata, with_side=with_side)

    def vector_discover(self, target=None, context=(), limit: int = 10, filter_metadata: Optional[Dict[str, Any]] = None,
                        with_wins: bool = False) -> List[tuple]:
        """Extension: discovery.  ``context``: (positive, negative) pairs, ``target``: an optional vector; each a stored
        vector id or a raw vector, and ids never come back.  With a target: vectors on the right side of the most pairs
        first, by the target's score within equal wins.  Without: context search, vectors by how far they sit on the wrong
        side of any pair (0 = on the right side of all).  A filter is pushed down; any number of shards.  ``(vector_id,
        score, metadata)``, with the pairs won appended when ``with_wins`` is set (``VectorStore.discover`` states the
        order)."""
        return self.vector_store.discover(target, context, limit=limit, filter_metadata=filter_metadata, with_wins=with_wins)

    async def vector_discover_async(self, target=None, context=(), limit: int = 10,
                                    filter_metadata: Optional[Dict[str, Any]] = None, with_wins: bool = False) -> List[tuple]:
        return await self.vector_store.discover_async(target, context, limit=limit, filter_metadata=filter_metadata,
                                                      with_wins=with_wins)

    def _matrix_lines(self, lines):
        """a distance matrix's lines with the scores as reported: cosine similarity, for L2 the positive squared distance"""
        if self.vector_store.indices[0].metric == _native.METRIC_COSINE:
            return lines
        return [(anchor, [(vid, -score) for vid, score in res]) for anchor, res in lines]

    @staticmethod
    def _matrix_pairs(lines) -> List[Dict[str, Any]]:
        return [{"a": anchor, "b": vid, "score": score} for anchor, res in lines for vid, score in res]

    @staticmethod
    def _matrix_offsets(lines) -> Dict[str, List[Any]]:
        ids = [anchor for anchor, _ in lines]
        at = {vid: i for i, vid in enumerate(ids)}
        cells = [(at[anchor], at[vid], score) for anchor, res in lines for vid, score in res]
        return {"offsets_row": [c[0] for c in cells], "offsets_col": [c[1] for c in cells], "scores": [c[2] for c in cells],
                "ids": ids}

    def vector_search_matrix_pairs(self, sample: int = 10, limit: int = 3, filter_metadata: Optional[Dict[str, Any]] = None,
                                   vector_ids=None, seed=None) -> List[Dict[str, Any]]:
        """Extension: distance matrix.  A sample of the stored vectors -- ``vector_ids``, else ``sample`` of those
        ``filter_metadata`` matches, drawn with ``seed`` -- and for each its ``limit`` nearest among the OTHER sampled
        vectors: ``[{"a": id, "b": id, "score": s}, ...]``, anchor-major (anchors in sorted id order), each anchor's
        neighbours nearest first.  Scores are cosine similarities, for L2 the positive squared distances.  Any number of
        shards (``VectorStore.search_matrix`` states how)."""
        return self._matrix_pairs(self._matrix_lines(self.vector_store.search_matrix(
            sample, limit, filter_metadata=filter_metadata, vector_ids=vector_ids, seed=seed)))

    async def vector_search_matrix_pairs_async(self, sample: int = 10, limit: int = 3,
                                               filter_metadata: Optional[Dict[str, Any]] = None, vector_ids=None,
                                               seed=None) -> List[Dict[str, Any]]:
        return self._matrix_pairs(self._matrix_lines(await self.vector_store.search_matrix_async(
            sample, limit, filter_metadata=filter_metadata, vector_ids=vector_ids, seed=seed)))

    def vector_search_matrix_offsets(self, sample: int = 10, limit: int = 3, filter_metadata: Optional[Dict[str, Any]] = None,
                                     vector_ids=None, seed=None) -> Dict[str, List[Any]]:
        """``vector_search_matrix_pairs`` as a sparse matrix: ``{"offsets_row": [...], "offsets_col": [...], "scores": [...],
        "ids": [...]}`` -- cell i says that ``ids[offsets_col[i]]`` is a neighbour of ``ids[offsets_row[i]]`` with
        ``scores[i]``; the cells are in the order of the pairs."""
        return self._matrix_offsets(self._matrix_lines(self.vector_store.search_matrix(
            sample, limit, filter_metadata=filter_metadata, vector_ids=vector_ids, seed=seed)))

    async def vector_search_matrix_offsets_async(self, sample: int = 10, limit: int = 3,
                                                 filter_metadata: Optional[Dict[str, Any]] = None, vector_ids=None,
                                                 seed=None) -> Dict[str, List[Any]]:
        return self._matrix_offsets(self._matrix_lines(await self.vector_store.search_matrix_async(
            sample, limit, filter_metadata=filter_metadata, vector_ids=vector_ids, seed=seed)))

    def vector_search_range(self, query_vector: List[float], threshold: float,
                            filter_metadata: Optional[Dict[str, Any]] = None, prefilter: Optional[bool] = None,
                            max_results: Optional[int] = None) -> List[Result]:
        """Extension: EVERY stored vector whose score reaches ``threshold`` (cosine similarity; for L2 the negated squared
        distance), best first, with no top-k limit in between (``vector_search(limit, threshold)`` thresholds a top-``limit``
        and silently drops the rest).  ``max_results`` cuts the sorted, filtered list (None = all)."""
        self._check_dim(query_vector)
        return self.vector_store.search_range(query_vector, threshold, filter_metadata=filter_metadata,
                                              prefilter=prefilter, max_results=max_results)

    async def vector_search_range_async(self, query_vector: List[float], threshold: float,
                                        filter_metadata: Optional[Dict[str, Any]] = None, prefilter: Optional[bool] = None,
                                        max_results: Optional[int] = None) -> List[Result]:
        self._check_dim(query_vector)
        return await self.vector_store.search_range_async(query_vector, threshold, filter_metadata=filter_metadata,
                                                          prefilter=prefilter, max_results=max_results)

    def vector_search_range_batch(self, query_vectors: List[List[float]], thresholds,
                                  filter_metadata: Optional[Dict[str, Any]] = None, prefilter: Optional[bool] = None,
                                  max_results: Optional[int] = None) -> List[List[Result]]:
        """Extension: ``vector_search_range`` for a batch of queries -- one list per query, each exactly what
        ``vector_search_range`` returns for it; ``thresholds`` a scalar or one per query; one filter for the batch."""
        for v in query_vectors:
            self._check_dim(v)
        return self.vector_store.search_range_batch(query_vectors, thresholds, filter_metadata=filter_metadata,
                                                    prefilter=prefilter, max_results=max_results)

    async def vector_search_range_batch_async(self, query_vectors: List[List[float]], thresholds,
                                              filter_metadata: Optional[Dict[str, Any]] = None,
                                              prefilter: Optional[bool] = None,
                                              max_results: Optional[int] = None) -> List[List[Result]]:
        for v in query_vectors:
            self._check_dim(v)
        return await self.vector_store.search_range_batch_async(query_vectors, thresholds, filter_metadata=filter_metadata,
                                                                prefilter=prefilter, max_results=max_results)

    # ---- row management ----
    def delete_vector(self, vector_id: str) -> bool:
        return self.vector_store.delete(vector_id)

    async def delete_vector_async(self, vector_id: str) -> bool:
        return await self.vector_store.delete_async(vector_id)

    def delete_vectors(self, vector_ids: List[str]) -> int:
        """Extension: delete many ids in one call (one native removal per shard); returns how many were stored."""
        return self.vector_store.delete_many(vector_ids)

    async def delete_vectors_async(self, vector_ids: List[str]) -> int:
        return await self.vector_store.delete_many_async(vector_ids)

    def delete_by_filter(self, filter_metadata: Dict[str, Any]) -> int:
        """Extension: delete every id whose metadata matches the filter; returns how many were deleted."""
        return self.vector_store.delete_by_filter(filter_metadata)

    async def delete_by_filter_async(self, filter_metadata: Dict[str, Any]) -> int:
        return await self.vector_store.delete_by_filter_async(filter_metadata)

    def update_metadata(self, vector_id: str, metadata: Dict[str, Any]) -> bool:
        return self.vector_store.update_metadata(vector_id, metadata)

    async def update_metadata_async(self, vector_id: str, metadata: Dict[str, Any]) -> bool:
        return await self.vector_store.update_metadata_async(vector_id, metadata)

    def get_vector(self, vector_id: str):
        return self.vector_store.get(vector_id)

    async def get_vector_async(self, vector_id: str):
        return await self.vector_store.get_async(vector_id)

    def count_vectors(self) -> int:
        return self.vector_store.count()

    def clear(self) -> int:
        return self.vector_store.clear()

    async def clear_async(self) -> int:
        return await self.vector_store.clear_async()

    def get_stats(self) -> Dict[str, Any]:
        stats = {
            "version": self.version,
            "vector_dimension": self.vector_dim,
            "num_shards": self.num_shards,
            "total_vectors": self.count_vectors(),
            "plugins_enabled": self.enable_plugins,
            "plugins_loaded": len(self.plugins) if self.enable_plugins else 0,
            "distributed_enabled": self.enable_distributed,
            "gpu_enabled": self.enable_gpu,
        }
        stats.update(self.vector_store.get_stats())
        return stats
