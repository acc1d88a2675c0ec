"""Nearest-centre assignment on the MI355X through ``_native`` (``wdbx_index_assign``): centre and score bit for bit against the
library's own exact path (``wdbx_index_search_rows`` with the centres as queries), against float64 at shapes that path cannot
reach, the ambiguous path forced, the edges of the contract, and the per-centre sums."""
import numpy as np
import pytest

from wdbx_amd import _native

pytestmark = pytest.mark.gpu

COSINE, L2 = _native.METRIC_COSINE, _native.METRIC_L2


@pytest.fixture(scope="module")
def block():
    """The largest centre block of host_assign.h's plan, as the library reports it: the blocks of a call with the most centres."""
    with _native.NativeIndex(4, capacity_rows=1) as ix:
        ix.add(np.ones((1, 4), np.float32))
        ix.assign(np.ones((_native.MAX_CENTERS, 4), np.float32), want=("center",))
        return _native.MAX_CENTERS // ix.get_option("last_assign_center_blocks")


def _gauss(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _expected(ix, centers, n, mask=None):
    """(centre, score) per row from search_rows: every row listed, k = n, one query per centre."""
    idx, score = ix.search_rows(centers, n, np.arange(n, dtype=np.uint64))
    k = centers.shape[0]
    rank = np.full((k, n), -np.inf, np.float32)
    raw = np.zeros((k, n), np.float32)
    for c in range(k):
        ok = idx[c] >= 0
        raw[c, idx[c][ok]] = score[c][ok]
        rank[c, idx[c][ok]] = score[c][ok] if ix.metric == COSINE else -score[c][ok]
    best = rank.argmax(0)  # (the first of equal values: the lowest centre)
    none = rank.max(0) == -np.inf
    if mask is not None:
        none |= ~mask
    return np.where(none, -1, best).astype(np.int32), np.where(none, 0, raw[best, np.arange(n)]).astype(np.float32)


def _same(got, want):
    center, score = want
    assert np.array_equal(got["center"], center), np.flatnonzero(got["center"] != center)[:10]
    assert np.array_equal(got["score"].view(np.uint32), score.view(np.uint32))


@pytest.mark.parametrize("metric", [COSINE, L2])
@pytest.mark.parametrize("n", [1, 127, 129, 1500])
@pytest.mark.parametrize("dim", [4, 100, 384])
def test_centre_and_score_equal_the_exact_path_bit_for_bit(metric, n, dim, block):
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        ix.add(_gauss(n + dim, n, dim), normalize=metric == COSINE)
        for k in (1, 2, 33, block + 1):  # (the last: just above one centre block)
            centers = _gauss(1000 + k, k, dim)
            if metric == COSINE:
                centers /= np.linalg.norm(centers, axis=1, keepdims=True)
            got = ix.assign(centers, want=("center", "score"))
            _same(got, _expected(ix, centers, n))
            assert ix.get_option("last_assign_center_blocks") == -(-k // block)


@pytest.mark.parametrize("metric", [COSINE, L2])
@pytest.mark.parametrize("n, dim, k", [(20000, 384, 257), (5000, 770, 1024)])
def test_against_float64_where_the_exact_path_cannot_reach(metric, n, dim, k):
    rows, centers = _gauss(1, n, dim), _gauss(2, k, dim)
    if metric == COSINE:
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        ix.add(rows)
        got = ix.assign(centers, want=("center",))["center"]
        share = ix.get_option("last_assign_ambiguous") / n
    r64, c64 = rows.astype(np.float64), centers.astype(np.float64)
    dots = r64 @ c64.T
    nr, nc = np.linalg.norm(r64, axis=1), np.linalg.norm(c64, axis=1)
    if metric == COSINE:
        value, b = dots, 1.02 * (dim + 18) * 2.0 ** -24 * nr[:, None] * nc[None, :]
    else:
        value = -(nr[:, None] ** 2 - 2 * dots + nc[None, :] ** 2)
        b = 1.02 * (dim + 18) * 2.0 ** -24 * (nr[:, None] + nc[None, :]) ** 2
    assert got.min() >= 0 and got.max() < k
    at = np.arange(n)
    assert np.all(value[at, got] >= value.max(1) - 2 * b[at, got])
    wrong = float(np.mean(got != value.argmax(1)))
    print(f"metric {metric} {n}x{dim} K={k}: not the float64 argmax {wrong:.4%}, ambiguous rows {share:.4%}")
    assert wrong <= 0.05


@pytest.mark.parametrize("metric", [COSINE, L2])
def test_the_ambiguous_path_forced(metric):
    n, dim = 300, 100
    centers = _gauss(5, 5, dim)
    centers[1] = centers[0]
    centers[1, 17] = np.nextafter(centers[0, 17], np.float32(np.inf))  # one ulp in one element
    centers[3] = centers[2]                                            # an exact duplicate pair
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        ix.add(_gauss(6, n, dim))
        got = ix.assign(centers, want=("center", "score"))
        assert ix.get_option("last_assign_ambiguous") > 0
        _same(got, _expected(ix, centers, n))
    assert not np.any(got["center"] == 3) and np.any(got["center"] == 2)


@pytest.mark.parametrize("metric", [COSINE, L2])
def test_edges(metric):
    n, dim = 200, 20
    rows = _gauss(7, n, dim)
    rows[7, 3] = np.nan   # a NaN element
    rows[9] = 0.0         # a zero row
    centers = _gauss(8, 6, dim)
    centers[1, 0] = np.nan
    allowed = np.ones(n, bool)
    allowed[11] = False
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        ix.add(rows)
        ix.remove_rows([5])
        mask = _native.pack_row_mask(allowed)
        got = ix.assign(centers, mask=mask, want=("center", "score"))
        _same(got, _expected(ix, centers, n, mask=allowed))
        for r in (5, 7, 11):
            assert got["center"][r] == -1 and got["score"][r] == 0
        assert not np.any(got["center"] == 1)
        norms = np.where(np.isnan(centers).any(1), np.inf, (centers.astype(np.float64) ** 2).sum(1))
        assert got["center"][9] == (0 if metric == COSINE else int(norms.argmin()))
        for bad in (dict(centers=centers, mask=mask[:-1]), dict(centers=centers[:0]),
                    dict(centers=np.zeros((_native.MAX_CENTERS + 1, dim), np.float32))):
            with pytest.raises(_native.HipBackendError) as e:
                ix.assign(**bad)
            assert e.value.code == -1
            _same(ix.assign(centers, mask=mask, want=("center", "score")), (got["center"], got["score"]))
        with pytest.raises(_native.HipBackendError) as e:
            ix.assign(centers, want=())
        assert e.value.code == -1


@pytest.mark.parametrize("metric", [COSINE, L2])
def test_sums_and_counts(metric):
    n, dim, k = 1500, 100, 33
    rows = _gauss(9, n, dim)
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        ix.add(rows, normalize=metric == COSINE)
        stored = ix.get_rows(0, n).astype(np.float64)
        centers = _gauss(10, k, dim)
        got = ix.assign(centers, normalize=True, want=("center", "sums", "counts"))
        partials = ix.get_option("last_assign_partials")
        again = ix.assign(centers, normalize=True, want=("center", "sums", "counts"))
    counts = np.bincount(got["center"], minlength=k)
    assert got["center"].min() >= 0 and np.array_equal(got["counts"], counts) and partials >= 1
    for c in range(k):
        mine = stored[got["center"] == c]
        bound = (max(counts[c] - 1, 0) + partials) * 2.0 ** -24 * np.abs(mine).sum(0)
        assert np.all(np.abs(got["sums"][c] - mine.sum(0)) <= bound), c
    assert np.array_equal(got["sums"].view(np.uint32), again["sums"].view(np.uint32))
    assert np.array_equal(got["counts"], again["counts"]) and np.array_equal(got["center"], again["center"])
