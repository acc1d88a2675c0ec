"""Framework-free handlers of the reference's REST search route.

The reference serves ``POST /api/v1/vectors/search`` with FastAPI (wdbx/api/server.py:141-152, :353-364): a
``SearchModel`` body (:109-113, :321-325) is passed to ``wdbx.vector_search_async`` and the hits come back as
``{"results": [{"vector_id", "similarity", "metadata"}]}``.  The HTTP shell (uvicorn, auth, CORS) is control plane and
out of scope; these two coroutines are what a route function calls, with the same request and response shapes and the
same validation outcome (a malformed body is a 422 there; here a ``ValueError`` the caller maps to it):

    @router.post("/vectors/search")
    async def search_vectors(body: dict):
        return await search_endpoint(wdbx, body)

``range_search_endpoint`` answers "every vector within this similarity" (no limit; the extension the reference lacks).
``range_search_batch_endpoint`` is its batch form: many range queries in one request, one call per shard.
``search_batch_endpoint`` is the batch form the reference lacks: many queries in one request, answered by
one batched pass per shard (``vector_search_batch``).  Concurrent single requests need no batch route: they are
coalesced at ``VectorStore.search_async`` (what the reference's server produces, api/server.py:143).
"""

from __future__ import annotations

from typing import Any, Dict, List, Optional

_FIELDS = ("query_vector", "limit", "threshold", "filter_metadata")


def _parse_common(payload: Dict[str, Any], filter_list: bool = False):
    if not isinstance(payload, dict):
        raise ValueError("request body must be an object")
    limit = payload.get("limit", 10)
    threshold = payload.get("threshold", 0.0)
    flt = payload.get("filter_metadata")
    limit = 10 if limit is None else limit        # Optional[int] = 10 (server.py:111): null means the default
    threshold = 0.0 if threshold is None else threshold
    if isinstance(limit, bool) or not isinstance(limit, int):
        raise ValueError("limit must be an integer")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
        raise ValueError("threshold must be a number")
    if filter_list and isinstance(flt, list):  # the batch form: one filter (an object or null) per query
        if not all(f is None or isinstance(f, dict) for f in flt):
            raise ValueError("filter_metadata must be an object, or a list of objects and nulls")
    elif flt is not None and not isinstance(flt, dict):
        raise ValueError("filter_metadata must be an object")
    return limit, float(threshold), flt


def _vector(v: Any, what: str) -> List[float]:
    if not isinstance(v, (list, tuple)) or not all(isinstance(x, (int, float)) and not isinstance(x, bool) for x in v):
        raise ValueError(f"{what} must be a list of numbers")
    return [float(x) for x in v]


def _render(results) -> Dict[str, Any]:
    return {"results": [{"vector_id": vid, "similarity": sim, "metadata": meta} for vid, sim, meta in results]}


async def search_endpoint(wdbx, payload: Dict[str, Any]) -> Dict[str, Any]:
    """``POST /api/v1/vectors/search`` (server.py:141-152): body ``{"query_vector": [...], "limit": 10, "threshold": 0.0,
    "filter_metadata": null}`` -> ``{"results": [{"vector_id", "similarity", "metadata"}, ...]}``.  ``"distinct": true``
    (extension; absent, null or false = the plain search): at most one result per value of the store's ``DISTINCT_KEY``
    metadata field (``wdbx.vector_search_distinct_async``).  ``"query_vectors": [[...], ...]`` (extension, in place of
    ``query_vector``): a query of several vectors, the documents ranked by late interaction
    (``wdbx.vector_search_multivector_async``); not together with ``query_vector`` or ``distinct``.  ``"mmr": {"lambda": 0.5,
    "fetch_k": 40}`` (extension; absent or null = the plain search; both members optional, ``lambda`` in [0, 1], ``fetch_k``
    an integer >= ``limit`` or null): the results are picked by maximal marginal relevance from the ``fetch_k`` best and come
    in pick order (``wdbx.vector_search_mmr_async``); not together with ``distinct`` or ``query_vectors``.  ``"group_size": n``
    (extension; an integer >= 1; absent or null = no groups): the best ``limit`` values of ``DISTINCT_KEY``, each with its
    best ``n`` vectors (``wdbx.vector_search_groups_async``); the response is ``{"groups": [{"key", "hits": [{"vector_id",
    "similarity", "metadata"}, ...]}, ...]}``; with or without ``"distinct": true``, not together with ``mmr`` or
    ``query_vectors``."""
    limit, threshold, flt = _parse_common(payload)
    group_size = payload.get("group_size")
    if group_size is not None:
        if isinstance(group_size, bool) or not isinstance(group_size, int) or group_size < 1:
            raise ValueError("group_size must be an integer >= 1, or null")
        if payload.get("mmr") is not None or payload.get("query_vectors") is not None:
            raise ValueError("group_size goes with query_vector alone: neither mmr nor query_vectors")
    mmr = payload.get("mmr")
    if mmr is not None:
        if not isinstance(mmr, dict) or set(mmr) - {"lambda", "fetch_k"}:
            raise ValueError('mmr must be an object with the members "lambda" and "fetch_k"')
        if payload.get("distinct") or payload.get("query_vectors") is not None:
            raise ValueError("mmr goes with query_vector alone: neither distinct nor query_vectors")
        lam = mmr.get("lambda", 0.5)
        lam = 0.5 if lam is None else lam
        if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0.0 <= lam <= 1.0:
            raise ValueError("mmr.lambda must be a number in [0, 1]")
        fetch_k = mmr.get("fetch_k")
        if fetch_k is not None and (isinstance(fetch_k, bool) or not isinstance(fetch_k, int) or fetch_k < limit):
            raise ValueError("mmr.fetch_k must be an integer >= limit, or null")
        if "query_vector" not in payload:
            raise ValueError("query_vector is required")
        query = _vector(payload["query_vector"], "query_vector")
        return _render(await wdbx.vector_search_mmr_async(query, limit, fetch_k, float(lam), threshold, flt))
    if payload.get("query_vectors") is not None:
        if "query_vector" in payload or payload.get("distinct"):
            raise ValueError("query_vectors stands alone: neither query_vector nor distinct goes with it")
        vectors = payload["query_vectors"]
        if not isinstance(vectors, (list, tuple)) or not vectors:
            raise ValueError("query_vectors must be a non-empty list of vectors")
        queries = [_vector(v, f"query_vectors[{i}]") for i, v in enumerate(vectors)]
        return _render(await wdbx.vector_search_multivector_async(queries, limit, threshold, flt))
    if "query_vector" not in payload:
        raise ValueError("query_vector is required")
    query = _vector(payload["query_vector"], "query_vector")
    distinct = payload.get("distinct")
    if distinct is not None and not isinstance(distinct, bool):
        raise ValueError("distinct must be true, false or null")
    if group_size is not None:
        groups = await wdbx.vector_search_groups_async(query, limit, group_size, threshold, flt)
        return {"groups": [{"key": g["key"], "hits": _render(g["hits"])["results"]} for g in groups]}
    if distinct:
        return _render(await wdbx.vector_search_distinct_async(query, limit, threshold, flt))
    return _render(await wdbx.vector_search_async(query, limit, threshold, flt))


async def search_batch_endpoint(wdbx, payload: Dict[str, Any]) -> Dict[str, Any]:
    """Batch form (extension): body ``{"query_vectors": [[...], ...], "limit", "threshold", "filter_metadata",
    "prefilter"}`` -> ``{"results": [<one search_endpoint result list per query>]}``.  One batched matrix-core pass per
    shard.  ``prefilter`` (true / false; absent or null = the store's ``FILTER_PUSHDOWN``): push the metadata filter down
    into that pass, so every query returns a full ``limit`` whenever enough rows match.  ``filter_metadata`` may be a LIST
    with one filter (an object or null) per query; any other length is refused.  ``vector_id_lists`` (a list with one list
    of vector ids per query; any other length is refused; not together with ``filter_metadata``): every query is ranked
    among ITS listed vectors only (``vector_search_batch_among_each``), one call per shard for the whole batch."""
    import asyncio

    limit, threshold, flt = _parse_common(payload, filter_list=True)
    if "query_vectors" not in payload or not isinstance(payload["query_vectors"], (list, tuple)):
        raise ValueError("query_vectors is required and must be a list of vectors")
    queries = [_vector(v, f"query_vectors[{i}]") for i, v in enumerate(payload["query_vectors"])]
    if isinstance(flt, list) and len(flt) != len(queries):
        raise ValueError(f"filter_metadata lists {len(flt)} filters for {len(queries)} queries")
    id_lists = payload.get("vector_id_lists")
    if id_lists is not None:
        if not isinstance(id_lists, (list, tuple)) or not all(
                isinstance(ids, (list, tuple)) and all(isinstance(i, str) for i in ids) for ids in id_lists):
            raise ValueError("vector_id_lists must be a list of lists of vector ids")
        if len(id_lists) != len(queries):
            raise ValueError(f"vector_id_lists holds {len(id_lists)} lists for {len(queries)} queries")
        if flt is not None:
            raise ValueError("vector_id_lists and filter_metadata exclude each other")
    if not queries:
        return {"results": []}
    loop = asyncio.get_running_loop()
    if id_lists is not None:
        per_query = await loop.run_in_executor(None, lambda: wdbx.vector_search_batch_among_each(
            queries, [list(ids) for ids in id_lists], limit, threshold))
        return {"results": [_render(r)["results"] for r in per_query]}
    prefilter = payload.get("prefilter")
    if prefilter is not None and not isinstance(prefilter, bool):
        raise ValueError("prefilter must be true, false or null")
    extra = {} if prefilter is None else {"prefilter": prefilter}  # (absent / null: the facade's own default)
    per_query = await loop.run_in_executor(None, lambda: wdbx.vector_search_batch(queries, limit, threshold, flt, **extra))
    return {"results": [_render(r)["results"] for r in per_query]}


async def recommend_endpoint(wdbx, payload: Dict[str, Any]) -> Dict[str, Any]:
    """Recommend form (extension): body ``{"positive": [...], "negative": [...], "limit": 10, "strategy": "best_score",
    "filter_metadata": null}`` -> the ``search_endpoint`` response shape with a ``"side"`` member per result (1: nearer to a
    positive than to any negative, 0: not) (``wdbx.vector_recommend_async``).  The items of ``positive`` (at least one) and
    ``negative`` (absent or null = none) are stored vector ids (strings) or vectors (lists of numbers); ``strategy`` is
    ``"best_score"`` (absent or null) or ``"average_vector"``."""
    if not isinstance(payload, dict):
        raise ValueError("request body must be an object")
    limit = payload.get("limit", 10)
    limit = 10 if limit is None else limit
    if isinstance(limit, bool) or not isinstance(limit, int):
        raise ValueError("limit must be an integer")
    flt = payload.get("filter_metadata")
    if flt is not None and not isinstance(flt, dict):
        raise ValueError("filter_metadata must be an object")
    strategy = payload.get("strategy")
    strategy = "best_score" if strategy is None else strategy
    if strategy not in ("best_score", "average_vector"):
        raise ValueError('strategy must be "best_score" or "average_vector"')

    def examples(name: str, required: bool):
        items = payload.get(name)
        if items is None and not required:
            return []
        if not isinstance(items, (list, tuple)) or (required and not items):
            raise ValueError(f"{name} must be a {'non-empty ' if required else ''}list of vector ids and vectors")
        return [e if isinstance(e, str) else _vector(e, f"{name}[{i}]") for i, e in enumerate(items)]

    positive, negative = examples("positive", True), examples("negative", False)
    found = await wdbx.vector_recommend_async(positive, negative, limit=limit, strategy=strategy, filter_metadata=flt,
                                              with_side=True)
    return {"results": [{"vector_id": vid, "similarity": sim, "metadata": meta, "side": side} for vid, sim, meta, side in found]}


async def discover_endpoint(wdbx, payload: Dict[str, Any]) -> Dict[str, Any]:
    """Discovery form (extension): body ``{"target": ..., "context": [{"positive": ..., "negative": ...}, ...], "limit": 10,
    "filter_metadata": null}`` -> the ``search_endpoint`` response shape with a ``"wins"`` member per result, the context
    pairs the vector is on the right side of (``wdbx.vector_discover_async``).  ``target`` (absent or null = context search,
    then ``similarity`` is the loss, <= 0, and ``wins`` 0) and the members of every pair are stored vector ids (strings) or
    vectors (lists of numbers); a pair may also be a two-item list [positive, negative]."""
    if not isinstance(payload, dict):
        raise ValueError("request body must be an object")
    limit = payload.get("limit", 10)
    limit = 10 if limit is None else limit
    if isinstance(limit, bool) or not isinstance(limit, int):
        raise ValueError("limit must be an integer")
    flt = payload.get("filter_metadata")
    if flt is not None and not isinstance(flt, dict):
        raise ValueError("filter_metadata must be an object")

    def example(e, name: str):
        return e if isinstance(e, str) else _vector(e, name)

    target = payload.get("target")
    target = None if target is None else example(target, "target")
    items = payload.get("context")
    items = [] if items is None else items
    if not isinstance(items, (list, tuple)):
        raise ValueError("context must be a list of pairs")
    context = []
    for i, pair in enumerate(items):
        if isinstance(pair, dict) and "positive" in pair and "negative" in pair:
            pair = (pair["positive"], pair["negative"])
        if not isinstance(pair, (list, tuple)) or len(pair) != 2:
            raise ValueError(f"context[{i}] must be an object with positive and negative, or a list of the two")
        context.append((example(pair[0], f"context[{i}].positive"), example(pair[1], f"context[{i}].negative")))
    if target is None and not context:
        raise ValueError("target or a non-empty context is required")
    found = await wdbx.vector_discover_async(target, context, limit=limit, filter_metadata=flt, with_wins=True)
    return {"results": [{"vector_id": vid, "similarity": sim, "metadata": meta, "wins": wins} for vid, sim, meta, wins in found]}


def _matrix_arguments(payload) -> Dict[str, Any]:
    """the body of the two distance-matrix forms: ``{"sample": 10, "limit": 3, "filter": null, "vector_ids": null, "seed": null}``"""
    if not isinstance(payload, dict):
        raise ValueError("request body must be an object")

    def integer(name, default, optional=False):
        value = payload.get(name)
        if value is None:
            return default
        if isinstance(value, bool) or not isinstance(value, int) or (value < 0 and not optional):
            raise ValueError(f"{name} must be a{'n' if optional else ' non-negative'} integer")
        return value

    flt = payload.get("filter")
    if flt is not None and not isinstance(flt, dict):
        raise ValueError("filter must be an object")
    vector_ids = payload.get("vector_ids")
    if vector_ids is not None and (not isinstance(vector_ids, (list, tuple)) or not all(isinstance(v, str) for v in vector_ids)):
        raise ValueError("vector_ids must be a list of vector ids")
    return {"sample": integer("sample", 10), "limit": integer("limit", 3), "filter_metadata": flt, "vector_ids": vector_ids,
            "seed": integer("seed", None, optional=True)}


async def search_matrix_pairs_endpoint(wdbx, payload: Dict[str, Any]) -> Dict[str, Any]:
    """Distance-matrix form (extension), as pairs: body ``{"sample": 10, "limit": 3, "filter": null, "vector_ids": null,
    "seed": null}`` -> ``{"pairs": [{"a": id, "b": id, "score": s}, ...]}`` (``wdbx.vector_search_matrix_pairs_async``): for each
    sampled vector its ``limit`` nearest among the other sampled vectors.  ``vector_ids`` names the sample itself; else
    ``sample`` vectors are drawn from those ``filter`` matches, reproducibly with ``seed``."""
    return {"pairs": await wdbx.vector_search_matrix_pairs_async(**_matrix_arguments(payload))}


async def search_matrix_offsets_endpoint(wdbx, payload: Dict[str, Any]) -> Dict[str, Any]:
    """Distance-matrix form (extension), as a sparse matrix: the body of ``search_matrix_pairs_endpoint`` ->
    ``{"offsets_row": [...], "offsets_col": [...], "scores": [...], "ids": [...]}`` (``wdbx.vector_search_matrix_offsets_async``);
    rows and columns are positions in ``ids``."""
    return await wdbx.vector_search_matrix_offsets_async(**_matrix_arguments(payload))


async def delete_vectors_endpoint(wdbx, payload: Dict[str, Any]) -> Dict[str, Any]:
    """Batch delete (extension): body ``{"vector_ids": ["a", "b"]}`` or ``{"filter_metadata": {...}}`` -- exactly one of the
    two -- -> ``{"deleted": n}``, the number of ids that were stored (``wdbx.delete_vectors_async`` /
    ``wdbx.delete_by_filter_async``): one removal per shard, whatever the number of ids.  An empty filter is refused: it
    would match everything."""
    if not isinstance(payload, dict):
        raise ValueError("request body must be an object")
    vector_ids, flt = payload.get("vector_ids"), payload.get("filter_metadata")
    if (vector_ids is None) == (flt is None):
        raise ValueError("exactly one of vector_ids and filter_metadata must be given")
    if vector_ids is not None:
        if not isinstance(vector_ids, (list, tuple)) or not all(isinstance(v, str) for v in vector_ids):
            raise ValueError("vector_ids must be a list of vector ids")
        return {"deleted": await wdbx.delete_vectors_async(list(vector_ids))}
    if not isinstance(flt, dict) or not flt:
        raise ValueError("filter_metadata must be a non-empty object")
    return {"deleted": await wdbx.delete_by_filter_async(flt)}


async def range_search_endpoint(wdbx, payload: Dict[str, Any]) -> Dict[str, Any]:
    """Range form (extension): body ``{"query_vector": [...], "threshold": 0.8, "filter_metadata": null,
    "max_results": null}`` -> the ``search_endpoint`` response shape with EVERY vector whose similarity reaches
    ``threshold`` (``wdbx.vector_search_range_async``), best first; ``max_results`` (null = all) cuts after sorting."""
    if not isinstance(payload, dict):
        raise ValueError("request body must be an object")
    if "query_vector" not in payload:
        raise ValueError("query_vector is required")
    if "threshold" not in payload:
        raise ValueError("threshold is required")
    threshold = payload["threshold"]
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or threshold != threshold:
        raise ValueError("threshold must be a number")
    flt = payload.get("filter_metadata")
    if flt is not None and not isinstance(flt, dict):
        raise ValueError("filter_metadata must be an object")
    max_results = payload.get("max_results")
    if max_results is not None and (isinstance(max_results, bool) or not isinstance(max_results, int) or max_results < 0):
        raise ValueError("max_results must be a non-negative integer or null")
    query = _vector(payload["query_vector"], "query_vector")
    return _render(await wdbx.vector_search_range_async(query, float(threshold), filter_metadata=flt,
                                                        max_results=max_results))


async def range_search_batch_endpoint(wdbx, payload: Dict[str, Any]) -> Dict[str, Any]:
    """Batched range form (extension): body ``{"query_vectors": [[...], ...], "threshold": 0.8 | "thresholds": [...],
    "filter_metadata": null, "max_results": null}`` -> ``{"results": [<one range_search_endpoint result list per query>]}``
    (``wdbx.vector_search_range_batch_async``).  ``threshold`` serves every query, ``thresholds`` holds one per query (any
    other length is refused); exactly one of the two.  One filter for the batch; ``max_results`` cuts each query's list."""
    if not isinstance(payload, dict):
        raise ValueError("request body must be an object")
    if "query_vectors" not in payload or not isinstance(payload["query_vectors"], (list, tuple)):
        raise ValueError("query_vectors is required and must be a list of vectors")
    queries = [_vector(v, f"query_vectors[{i}]") for i, v in enumerate(payload["query_vectors"])]

    def number(x):
        return not isinstance(x, bool) and isinstance(x, (int, float)) and x == x

    if ("threshold" in payload) == ("thresholds" in payload):
        raise ValueError("exactly one of threshold and thresholds is required")
    if "threshold" in payload:
        if not number(payload["threshold"]):
            raise ValueError("threshold must be a number")
        thresholds = [float(payload["threshold"])] * len(queries)
    else:
        thresholds = payload["thresholds"]
        if not isinstance(thresholds, (list, tuple)) or not all(number(x) for x in thresholds):
            raise ValueError("thresholds must be a list of numbers")
        if len(thresholds) != len(queries):
            raise ValueError(f"thresholds holds {len(thresholds)} values for {len(queries)} queries")
        thresholds = [float(x) for x in thresholds]
    flt = payload.get("filter_metadata")
    if flt is not None and not isinstance(flt, dict):
        raise ValueError("filter_metadata must be an object")
    max_results = payload.get("max_results")
    if max_results is not None and (isinstance(max_results, bool) or not isinstance(max_results, int) or max_results < 0):
        raise ValueError("max_results must be a non-negative integer or null")
    if not queries:
        return {"results": []}
    per_query = await wdbx.vector_search_range_batch_async(queries, thresholds, filter_metadata=flt, max_results=max_results)
    return {"results": [_render(r)["results"] for r in per_query]}
