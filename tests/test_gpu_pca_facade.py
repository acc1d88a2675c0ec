"""PCA through the facade on the MI355X (``WDBX.vector_pca`` / ``vector_reduce``): the decomposition is numpy's of the natively
returned scatter matrix, one shard and two shards agree within the bounds of their chains, the coordinates are
``wdbx_index_project``'s, and a filter travels as row masks."""
import asyncio

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, M = 600, 40, 5
U = 2.0 ** -24


def _planted():
    """Three strong directions (scales 5, 3, 2) in a random rotation, plus noise of scale 0.1 in the other 37."""
    rng = np.random.default_rng(11)
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    z = rng.standard_normal((N, D)) * np.concatenate([[5.0, 3.0, 2.0], np.full(D - 3, 0.1)])
    return (z @ q.T).astype(np.float32)


def _store(tmp_path, shards):
    from wdbx_amd import WDBX

    meta = {f"row_{i}": {"lang": "en" if i % 3 else "de"} for i in range(N)}
    w = WDBX(vector_dimension=D, num_shards=shards, data_dir=str(tmp_path / f"pca{shards}"), enable_plugins=False)
    w.vector_store.bulk_store(_planted(), metadata=meta)
    return w


def _shard_moments(ix):
    """A shard's moments and the bounds of tests/test_gpu_moments.py for them, about the exact float64 moments of its stored rows:
    the chain bound, 2 u more for the rounding of the staged fp32 subtraction (1.001: |a| about the fp32 mean, not the exact
    one), and n e e^T for a mean off by e <= the mean bound."""
    got, nat = ix.moments(), ix._native
    L, P = nat.get_option("last_moments_range_rows"), nat.get_option("last_moments_partials")
    Ls, Ps = nat.get_option("last_moments_sum_rows"), nat.get_option("last_moments_sum_partials")
    x = nat.get_rows(0, nat.size()).astype(np.float64)
    a = np.abs(x - x.mean(axis=0))
    mean_bound = (Ls + Ps + 2) * U * np.abs(x).sum(axis=0) / len(x)
    bound = 1.001 * ((L + 6) * U + P * 2.0 ** -53) * (a.T @ a) + len(x) * np.outer(mean_bound, mean_bound)
    return got, bound, mean_bound


def test_components_are_eigh_of_the_native_scatter_and_shards_agree(tmp_path):
    from wdbx_amd.vector_store import VectorStore

    w1, w2 = _store(tmp_path, 1), _store(tmp_path, 2)
    fit = w1.vector_pca(M)
    got, bound1, _ = _shard_moments(w1.vector_store.indices[0])
    assert fit["count"] == got["count"] == N
    # the same function on the same input: no tolerance
    values, vectors = np.linalg.eigh(got["scatter"] / (N - 1))
    order = np.argsort(values)[::-1][:M]
    comps = vectors[:, order].T
    comps = comps * np.where(comps[np.arange(M), np.argmax(np.abs(comps), axis=1)] < 0, -1.0, 1.0)[:, None]
    assert np.array_equal(fit["components"], comps) and np.array_equal(fit["explained_variance"], values[order])
    assert np.array_equal(fit["explained_variance_ratio"], values[order] / values.sum())
    assert np.array_equal(fit["mean"], got["mean"].astype(np.float64))
    assert np.max(np.abs(fit["components"] @ fit["components"].T - np.eye(M))) < 1e-12
    # the planted spectrum (the rows are stored normalised, which scales all directions alike: 2^2 against 0.1^2 after the third)
    assert fit["explained_variance_ratio"][:3].sum() > 0.9 and fit["explained_variance"][3] < 0.1 * fit["explained_variance"][2]
    again = asyncio.run(w1.vector_pca_async(M))
    assert all(np.array_equal(fit[k], again[k]) for k in ("mean", "components", "explained_variance"))

    # two shards: each side within its bounds of its rows' exact scatter; the means' errors enter the merge through d d^T
    parts = [_shard_moments(ix) for ix in w2.vector_store.indices]
    n2, mean2, scatter2 = VectorStore.merge_moments([(p[0]["count"], p[0]["mean"], p[0]["scatter"]) for p in parts])
    (ga, ba, ma), (gb, bb, mb) = parts
    delta, off = np.abs(gb["mean"].astype(np.float64) - ga["mean"]), ma + mb
    cross = ga["count"] * gb["count"] / N * (np.outer(delta, off) + np.outer(off, delta) + np.outer(off, off))
    assert n2 == N and sorted(p[0]["count"] for p in parts) != [0, N]
    err = np.abs(scatter2 - got["scatter"])
    print(f"one shard against two: scatter err/bound {np.max(err / (bound1 + ba + bb + cross)):.3f}")
    assert np.all(err <= bound1 + ba + bb + cross)
    fit2 = w2.vector_pca(M)
    assert fit2["count"] == N and np.array_equal(fit2["mean"], mean2)


@pytest.mark.parametrize("shards", [1, 2])
def test_reduce_returns_the_matching_ids_with_projects_coordinates(tmp_path, shards):
    w = _store(tmp_path, shards)
    vs = w.vector_store
    flt = {"lang": "en"}
    fit = w.vector_pca(2, filter_metadata=flt)
    assert fit["count"] == sum(1 for i in range(N) if i % 3)
    coords = w.vector_reduce(2, filter_metadata=flt)
    assert sorted(coords) == sorted(f"row_{i}" for i in range(N) if i % 3)
    basis, offset = fit["components"].astype(np.float32), fit["mean"].astype(np.float32)
    for ix, mask in zip(vs.indices, vs._row_masks(flt)):
        res = ix.project(basis, offset=offset, mask=mask)
        raw = ix._native.project(basis, offset=offset, mask=mask)
        assert np.array_equal(res["coords"], raw[res["rows"]]) and len(res["ids"]) == len(res["rows"])
        assert all(coords[vid] == row.tolist() for vid, row in zip(res["ids"], res["coords"]))
    assert w.vector_reduce(components=fit["components"], mean=fit["mean"], filter_metadata=flt) == coords
    assert asyncio.run(w.vector_reduce_async(2, filter_metadata=flt)) == coords
    nothing = {"lang": "fr"}
    assert w.vector_pca(2, filter_metadata=nothing)["count"] == 0 and w.vector_reduce(2, filter_metadata=nothing) == {}
