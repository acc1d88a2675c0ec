"""Batch upsert and delete through the facade on the MI355X: ``batch_store`` over a mix of new and stored ids leaves the search
answers the per-id path leaves; ``delete_vectors`` / ``delete_by_filter`` return the right counts, drop metadata, keep deleted
ids out of a ``prefilter=True`` search (the cached row masks are rebuilt), and survive save and reload; the REST handler."""
import asyncio

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

D, N = 32, 600


def _bits(results):
    return [(vid, np.float32(score).view(np.uint32).item()) for vid, score, _ in results]


def _open(path, shards):
    from wdbx_amd import WDBX

    return WDBX(vector_dimension=D, num_shards=shards, data_dir=str(path), enable_plugins=False)


@pytest.mark.parametrize("shards", [1, 2])
def test_batch_store_and_batch_delete(tmp_path, shards):
    from wdbx_amd import api

    raw = O.synth_rows(O.SEED_CORPUS, 0, N, D).astype(np.float32)
    fresh = O.synth_rows(O.SEED_CORPUS, N, 200, D).astype(np.float32)
    queries = O.synth_rows(O.SEED_QUERY, 0, 6, D).astype(np.float32)
    meta = {f"v{i}": {"lang": "de" if i % 5 == 0 else "en", "n": i} for i in range(N + 100)}
    one, per_id = _open(tmp_path / "batch", shards), _open(tmp_path / "single", shards)
    for w in (one, per_id):
        w.vector_store.batch_store({f"v{i}": raw[i].tolist() for i in range(N)}, {f"v{i}": meta[f"v{i}"] for i in range(N)})
        w.vector_search(queries[0].tolist(), limit=5)          # (the copies of the default route exist before the update)
    # 100 stored ids get new vectors, 100 new ids arrive, in one call / one id at a time
    update = {f"v{i}": fresh[j].tolist() for j, i in enumerate(range(250, 350))}
    update.update({f"v{N + j}": fresh[100 + j].tolist() for j in range(100)})
    update_meta = {vid: meta[vid] for vid in update}
    one.vector_store.batch_store(update, update_meta)
    for vid, vec in update.items():
        per_id.vector_store.store(vid, vec, update_meta[vid])
    assert one.count_vectors() == per_id.count_vectors() == N + 100
    for q in queries:
        for kwargs in (dict(limit=10), dict(limit=10, filter_metadata={"lang": "de"}, prefilter=True)):
            assert _bits(one.vector_search(q.tolist(), **kwargs)) == _bits(per_id.vector_search(q.tolist(), **kwargs))
    # an updated id answers with its new vector
    top = one.vector_search(fresh[3].tolist(), limit=1)
    assert top[0][0] == "v253" and top[0][1] > 0.9999

    # ---- delete by ids
    flt = {"lang": "de"}
    before = one.vector_search(queries[1].tolist(), limit=10, filter_metadata=flt, prefilter=True)   # (caches the masks)
    gone = [vid for vid, _, _ in before[:4]] + ["v7", "v7", "never-stored"]
    assert one.delete_vectors(gone) == 5
    for vid in gone:
        assert per_id.delete_vector(vid) in (True, False)
    assert one.count_vectors() == per_id.count_vectors() == N + 95
    after = one.vector_search(queries[1].tolist(), limit=10, filter_metadata=flt, prefilter=True)
    assert not {vid for vid, _, _ in after} & set(gone)
    assert _bits(after) == _bits(per_id.vector_search(queries[1].tolist(), limit=10, filter_metadata=flt, prefilter=True))
    assert all(one.get_vector(vid) is None and vid not in one.vector_store.metadata for vid in gone)
    for q in queries:
        assert _bits(one.vector_search(q.tolist(), limit=10)) == _bits(per_id.vector_search(q.tolist(), limit=10))

    # ---- delete by filter, the async form and the REST handler
    n_de = sum(1 for m in one.vector_store.metadata.values() if m["lang"] == "de")
    assert n_de > 100 and one.delete_by_filter(flt) == n_de
    assert one.delete_by_filter(flt) == 0
    assert one.vector_search(queries[2].tolist(), limit=10, filter_metadata=flt, prefilter=True) == []
    assert all(m["lang"] == "en" for _, _, m in one.vector_search(queries[2].tolist(), limit=50))
    assert asyncio.run(one.delete_vectors_async(["v1", "v2", "v1"])) == 2
    assert asyncio.run(one.delete_by_filter_async({"n": 3})) == 1
    assert asyncio.run(api.delete_vectors_endpoint(one, {"vector_ids": ["v4", "v4", "nope"]})) == {"deleted": 1}
    assert asyncio.run(api.delete_vectors_endpoint(one, {"filter_metadata": {"n": 6}})) == {"deleted": 1}
    left = one.count_vectors()
    assert left == N + 95 - n_de - 5
    want = [_bits(one.vector_search(q.tolist(), limit=10)) for q in queries]

    # ---- save, reload
    asyncio.run(one.shutdown())
    asyncio.run(per_id.shutdown())
    again = _open(tmp_path / "batch", shards)
    asyncio.run(again.initialize())
    assert again.count_vectors() == left
    assert [_bits(again.vector_search(q.tolist(), limit=10)) for q in queries] == want
    assert again.get_vector("v1") is None and again.get_vector("v253") is not None
    asyncio.run(again.shutdown())
