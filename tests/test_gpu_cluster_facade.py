"""Nearest-centre assignment and k-means through the facade on the MI355X: ``WDBX.vector_cluster`` recovers three well-separated
blobs on one shard and on two, equals a numpy Lloyd run from the same initial ids, never worsens its inertia, repeats itself
bit for bit; ``WDBX.vector_assign`` with a metadata filter answers for the matching ids only."""
import asyncio
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, N, K = 8, 300, 3


def _blob(i):
    return (i // 7) % 3


def _lloyd(unit, first, max_iter=25, tol=1e-4):
    """Spherical Lloyd in float64 from the rows ``first``: (centres, labels, iterations)."""
    centers, previous = unit[first].copy(), None
    for it in range(1, max_iter + 1):
        labels = (unit @ centers.T).argmax(1)
        counts = np.bincount(labels, minlength=K)
        moved = centers.copy()
        for c in range(K):
            if counts[c]:
                moved[c] = unit[labels == c].sum(0) / counts[c]
        moved /= np.linalg.norm(moved, axis=1, keepdims=True)
        shift = np.linalg.norm(moved - centers, axis=1).max()
        settled = previous is not None and np.array_equal(counts, previous) and shift < tol
        centers, previous = moved, counts
        if settled:
            break
    return centers, (unit @ centers.T).argmax(1), it


@pytest.mark.parametrize("shards", [1, 2])
def test_cluster_recovers_blobs_and_assign_follows_the_filter(tmp_path, shards):
    from wdbx_amd import WDBX

    rng = np.random.default_rng(3)
    blob = np.array([_blob(i) for i in range(N)])
    raw = (np.eye(D, dtype=np.float32)[blob] + 0.05 * rng.standard_normal((N, D))).astype(np.float32)
    meta = {f"row_{i}": {"lang": "en" if i % 2 else "de"} for i in range(N)}
    w = WDBX(vector_dimension=D, num_shards=shards, data_dir=str(tmp_path / f"cluster{shards}"), enable_plugins=False)
    w.vector_store.bulk_store(raw, metadata=meta)
    ids = sorted(meta)
    first = [int(v[4:]) for v in random.Random(1).sample(ids, K)]
    assert sorted(blob[first]) == [0, 1, 2]  # (the seed's initial ids lie in three blobs: Lloyd then has one fixed point)

    res = w.vector_cluster(K, seed=1)
    labels = np.array([res["assignments"][f"row_{i}"] for i in range(N)])
    assert len(res["assignments"]) == N and len(set(zip(blob.tolist(), labels.tolist()))) == K  # a permutation of the blobs
    assert res["counts"] == np.bincount(labels, minlength=K).tolist() and res["centers"].shape == (K, D)
    unit = raw.astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    centers, want, iterations = _lloyd(unit, first)
    assert np.array_equal(labels, want) and res["iterations"] == iterations
    assert np.allclose(res["centers"], centers, atol=1e-5, rtol=0)
    assert abs(res["inertia"] - (unit @ centers.T).max(1).sum()) < 1e-3
    # the inertia (a sum of similarities: larger is tighter) never gets worse from one iteration to the next
    steps = [w.vector_cluster(K, max_iter=m, seed=1)["inertia"] for m in (0, 1, 2)]
    assert steps[0] <= steps[1] + 1e-4 and steps[1] <= steps[2] + 1e-4 and steps[2] == res["inertia"]
    # two runs, and the async form: the same bits
    for again in (w.vector_cluster(K, seed=1), asyncio.run(w.vector_cluster_async(K, seed=1))):
        assert again["assignments"] == res["assignments"] and again["inertia"] == res["inertia"]
        assert again["centers"].tobytes() == res["centers"].tobytes() and again["counts"] == res["counts"]

    everyone = w.vector_assign(res["centers"])
    assert {v: c for v, (c, _) in everyone.items()} == res["assignments"]
    german = w.vector_assign(res["centers"], filter_metadata={"lang": "de"})
    assert sorted(german) == [v for v in ids if meta[v]["lang"] == "de"]
    assert all(german[v] == everyone[v] for v in german)
    assert asyncio.run(w.vector_assign_async(res["centers"], filter_metadata={"lang": "de"})) == german
    for v, (c, s) in list(everyone.items())[:20]:
        assert abs(s - float(unit[int(v[4:])] @ centers[c])) < 1e-5
