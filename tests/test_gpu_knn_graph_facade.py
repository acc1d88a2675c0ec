"""The k-NN graph through the facade on the MI355X: ``WDBX.vector_knn_graph`` on a few hundred stored vectors with string ids
and a metadata filter equals, id for id, the composition through ``vector_search_among`` over the filter's matches without the
anchor; the ``_async`` form agrees; two shards raise; ``GRAPH_MAX_ROWS`` refuses."""
import asyncio

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

D, N, K = 16, 400, 5


def test_facade_filter_async_shards_and_row_limit(tmp_path):
    from wdbx_amd import WDBX

    raw = O.synth_rows(O.SEED_CORPUS, 0, N, D).astype(np.float32)
    ids = [f"doc-{i:03d}" for i in range(N)]
    meta = {v: {"lang": "en" if i % 3 else "de"} for i, v in enumerate(ids)}
    one = WDBX(vector_dimension=D, num_shards=1, data_dir=str(tmp_path / "graph1"), enable_plugins=False)
    one.vector_store.bulk_store(raw, ids=ids, metadata=meta)
    for flt in (None, {"lang": "de"}):
        members = [v for v in ids if flt is None or meta[v]["lang"] == "de"]
        graph = one.vector_knn_graph(k=K, filter_metadata=flt)
        assert sorted(graph) == members
        for anchor in members:
            others = [v for v in members if v != anchor]
            want = one.vector_search_among(one.get_vector(anchor)[0], others, limit=K)
            assert [v for v, _ in graph[anchor]] == [r[0] for r in want], anchor
            assert np.allclose([s for _, s in graph[anchor]], [r[1] for r in want], rtol=0, atol=2e-6)
        assert asyncio.run(one.vector_knn_graph_async(k=K, filter_metadata=flt)) == graph
    one.vector_store.config.set("GRAPH_MAX_ROWS", N - 1)
    with pytest.raises(ValueError, match="GRAPH_MAX_ROWS"):
        one.vector_knn_graph(k=K)
    two = WDBX(vector_dimension=D, num_shards=2, data_dir=str(tmp_path / "graph2"), enable_plugins=False)
    two.vector_store.bulk_store(raw, ids=ids, metadata=meta)
    with pytest.raises(ValueError, match="one shard"):
        two.vector_knn_graph(k=K)
