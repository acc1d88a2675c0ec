"""The similarity self-join through the facade on the MI355X: ``WDBX.vector_similar_pairs`` on a clustered store with string
ids and a metadata filter names exactly the pairs a float64 ranking of the stored vectors names (away from the threshold by more
than fp32 rounding), each once, lower row first; the filter travels as the mask; the ``_async`` form agrees; ``max_pairs`` cuts;
two shards raise; ``JOIN_MAX_ROWS`` refuses."""
import asyncio

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, N, THR = 16, 1100, 0.97


def test_facade_ids_filter_async_cut_shards_and_row_limit(tmp_path):
    from wdbx_amd import WDBX

    rng = np.random.default_rng(77)
    centres = rng.standard_normal((N // 5, D))
    raw = (centres[np.arange(N) % len(centres)] + rng.uniform(0.02, 0.3, (N, 1)) * rng.standard_normal((N, D))).astype(np.float32)
    ids = [f"doc-{i:04d}" for i in range(N)]
    meta = {v: {"lang": "en" if i % 3 else "de"} for i, v in enumerate(ids)}
    one = WDBX(vector_dimension=D, num_shards=1, data_dir=str(tmp_path / "join1"), enable_plugins=False)
    one.vector_store.bulk_store(raw, ids=ids, metadata=meta)
    x = np.stack([np.asarray(one.get_vector(v)[0], np.float64) for v in ids])
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    sim = x @ x.T
    for flt in (None, {"lang": "de"}):
        member = np.array([flt is None or meta[v]["lang"] == "de" for v in ids])
        pairs = one.vector_similar_pairs(THR, filter_metadata=flt)
        rows = [(ids.index(a), ids.index(b)) for a, b, _ in pairs]
        assert len(set(rows)) == len(rows) > 0 and all(a < b and member[a] and member[b] for a, b in rows)
        assert [a for a, _ in rows] == sorted(a for a, _ in rows)  # segment order: by the lower row
        assert np.allclose([s for _, _, s in pairs], [sim[a, b] for a, b in rows], rtol=0, atol=5e-6)
        both = member[:, None] & member[None, :] & np.triu(np.ones((N, N), bool), 1)
        have = np.zeros((N, N), bool)
        have[tuple(np.array(rows).T)] = True
        assert have[both & (sim >= THR + 5e-6)].all() and not have[~both | (sim < THR - 5e-6)].any()
        assert asyncio.run(one.vector_similar_pairs_async(THR, filter_metadata=flt)) == pairs
        assert one.vector_similar_pairs(THR, filter_metadata=flt, max_pairs=7) == pairs[:7]
    one.vector_store.config.set("JOIN_MAX_ROWS", N - 1)
    with pytest.raises(ValueError, match="JOIN_MAX_ROWS"):
        one.vector_similar_pairs(THR)
    two = WDBX(vector_dimension=D, num_shards=2, data_dir=str(tmp_path / "join2"), enable_plugins=False)
    two.vector_store.bulk_store(raw, ids=ids, metadata=meta)
    with pytest.raises(ValueError, match="one shard"):
        two.vector_similar_pairs(THR)
