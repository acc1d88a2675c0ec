"""k-means++ initialisation through the facade on the MI355X: ``WDBX.vector_cluster(init="k-means++")`` gives the same bits
twice, starts from the rows ``seed_centers`` returns for the same draws, agrees with its ``_async`` form, raises on two shards
and on an unknown ``init``; the default stays ``init="random"``."""
import asyncio
import random

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

D, N, K, SEED = 16, 400, 6, 1234


def test_kmeanspp_init_is_reproducible_starts_from_the_seeded_rows_and_refuses_two_shards(tmp_path):
    from wdbx_amd import WDBX

    raw = O.synth_rows(O.SEED_CORPUS, 0, N, D).astype(np.float32)
    ids = [f"doc-{i:03d}" for i in range(N)]
    one = WDBX(vector_dimension=D, num_shards=1, data_dir=str(tmp_path / "seed1"), enable_plugins=False)
    one.vector_store.bulk_store(raw, ids=ids)
    first = one.vector_cluster(K, seed=SEED, init="k-means++")
    again = one.vector_cluster(K, seed=SEED, init="k-means++")
    assert first["centers"].tobytes() == again["centers"].tobytes() and first["assignments"] == again["assignments"]
    assert first["inertia"] == again["inertia"] and sum(first["counts"]) == N
    assert asyncio.run(one.vector_cluster_async(K, seed=SEED, init="k-means++"))["centers"].tobytes() == first["centers"].tobytes()
    # the initial centres (max_iter=0: no Lloyd step) are the stored vectors of the rows seed_centers returns for the same draws
    trials = 2 + int(np.log(K))
    rng = random.Random(SEED)
    draws = np.array([rng.getrandbits(64) for _ in range(K * trials)], dtype=np.uint64)
    picked = one.vector_store.indices[0].seed_centers(K, draws, trials)
    start = one.vector_cluster(K, seed=SEED, init="k-means++", max_iter=0)["centers"]
    assert len(set(picked["ids"])) == K
    stored = np.stack([one.get_vector(v)[0] for v in picked["ids"]]).astype(np.float64)
    assert np.array_equal(start, (stored / np.linalg.norm(stored, axis=1)[:, None]).astype(np.float32))  # (cluster's own unit())
    # the default is init="random", and explicit n_trials reaches the library
    assert one.vector_cluster(K, seed=SEED, max_iter=2)["centers"].tobytes() == one.vector_cluster(K, seed=SEED, max_iter=2, init="random")["centers"].tobytes()
    assert one.vector_cluster(K, seed=SEED, init="k-means++", n_trials=1, max_iter=0)["centers"].shape == (K, D)
    with pytest.raises(ValueError, match="n_trials"):
        one.vector_cluster(K, seed=SEED, init="k-means++", n_trials=17)
    with pytest.raises(ValueError, match="init"):
        one.vector_cluster(K, seed=SEED, init="farthest")
    two = WDBX(vector_dimension=D, num_shards=2, data_dir=str(tmp_path / "seed2"), enable_plugins=False)
    two.vector_store.bulk_store(raw, ids=ids)
    with pytest.raises(ValueError, match="one shard"):
        two.vector_cluster(K, seed=SEED, init="k-means++")
