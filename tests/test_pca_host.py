"""Device PCA, the parts that need no GPU: the device-free plan of wdbx_index_moments / wdbx_index_project
(wdbx-py_amd/csrc/host_pca.h) driven by tests/host_harness/pca_harness.cpp -- built once plain and once under
-fsanitize=address,undefined -- and ``VectorStore.pca``'s merge of per-shard moments over a stub of the shards."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
INC = ROOT / "wdbx-py_amd" / "csrc"
HARNESS = ROOT / "tests" / "host_harness" / "pca_harness.cpp"
NAMES = ("dim", "nb", "side", "groups", "wave_tiles", "staged", "instance", "lds", "ranges", "range_rows", "partial_bytes",
         "sum_ranges", "sum_rows", "covered")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("pca_" + request.param) / "pca_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return [list(map(int, line.split())) for line in p.stdout.splitlines()]
    return run


@pytest.mark.parametrize("forced_side", [0, 1, 2, 5])
def test_every_tile_in_one_group_and_one_wave_within_registers_lds_and_scratch(harness, forced_side):
    (max_m, max_dim, chunk, waves, wave_tiles, lds_limit, budget), = harness("limits")
    assert (max_m, max_dim, chunk, waves, wave_tiles, budget) == (32, 4096, 32, 8, 10, 256 << 20) and lds_limit <= 160 * 1024
    configs = ((1, 0), (5000, 7), (10_000_000, 0), (100_000_000, 0), (100_000_000, 1 << 20))
    # (the tiles do not depend on the rows: a forced group side is walked with the largest corpus only)
    for n_rows, forced_ranges in (configs if forced_side == 0 else configs[3:4]):
        plans = [dict(zip(NAMES, line)) for line in harness("plans", 4, 4096, n_rows, 256, forced_side, forced_ranges)]
        assert [p["dim"] for p in plans] == list(range(4, 4097))
        for p in plans:
            assert p["covered"] == 1, p  # exactly one group and wave per tile, staged blocks cover the tiles' reads, ranges the rows
            assert p["nb"] == -(-p["dim"] // 32) and p["groups"] == (lambda s: s * (s + 1) // 2)(-(-p["nb"] // p["side"]))
            assert 1 <= p["wave_tiles"] <= p["instance"] <= wave_tiles and 0 < p["lds"] <= lds_limit
            assert p["partial_bytes"] <= budget and 1 <= p["ranges"] <= max(1, -(-n_rows // chunk))
            assert p["range_rows"] % chunk == 0 and 1 <= p["sum_ranges"] <= max(n_rows, 1)
            if forced_side:
                assert p["side"] == min(forced_side, p["nb"])
            if forced_ranges == 7:
                assert p["ranges"] == min(7, budget // (4 * (32 * p["nb"]) ** 2)) and p["sum_ranges"] == 7
    one = dict(zip(NAMES, harness("plans", 384, 384, 10_000_000, 256, 0, 0)[0]))
    assert (one["groups"], one["wave_tiles"], one["instance"], one["ranges"]) == (1, 10, 10, 256)  # d = 384: the whole triangle, 10 tiles a wave


class _StubShard:
    """``HipFlatIndex.moments`` of a shard that holds ``rows``: float64 moments of its own rows (None when it is empty)."""

    def __init__(self, rows):
        self.rows = rows

    def moments(self, mask=None, center=True):
        if not len(self.rows):
            return None
        x = self.rows.astype(np.float64)
        a = x - x.mean(axis=0)
        return {"count": len(x), "mean": x.mean(axis=0), "scatter": a.T @ a}


def test_the_store_merges_the_shards_moments_like_one_covariance():
    """Three shards of unequal counts, one empty, with different means (the dd^T term carries most of the variance).  Bound: both
    sides are float64 sums of n products of centred values of magnitude at most 2 M (M = max |x|), each within (n + 16) 2^-53 of
    n (2 M)^2 under any summation order (16: the merge's handful of roundings of such terms).  Twice that, over n - 1."""
    from wdbx_amd.vector_store import VectorStore

    rng = np.random.default_rng(5)
    d, counts = 9, (37, 0, 100)
    parts = [rng.standard_normal((c, d)) * (1 + s) + 3.0 * s for s, c in enumerate(counts)]
    vs = VectorStore.__new__(VectorStore)
    vs.vector_dim, vs.indices = d, [_StubShard(p) for p in parts]
    vs._shard_pool = type("Pool", (), {"map": staticmethod(lambda f, work: map(f, work))})()
    out = vs.pca(d)
    x = np.concatenate(parts)
    n, big = len(x), float(np.max(np.abs(x)))
    bound = 2 * (n + 16) * 2.0 ** -53 * n * (2 * big) ** 2 / (n - 1)
    cov = np.cov(x, rowvar=False)
    assert out["count"] == n and np.max(np.abs(out["mean"] - x.mean(axis=0))) <= 8 * 2.0 ** -53 * big
    merged = VectorStore.merge_moments([(r["count"], r["mean"], r["scatter"]) for r in (s.moments() for s in vs.indices) if r])
    assert np.max(np.abs(merged[2] / (n - 1) - cov)) <= bound
    # the decomposition is of that matrix: descending variances, orthonormal components signed by their largest entry
    assert np.all(np.diff(out["explained_variance"]) <= 0) and abs(out["explained_variance_ratio"].sum() - 1) < 1e-12
    assert np.max(np.abs(out["components"] @ out["components"].T - np.eye(d))) < 1e-12
    assert np.all(out["components"][np.arange(d), np.argmax(np.abs(out["components"]), axis=1)] > 0)
