"""The int8 route of nearest-centre assignment on the MI355X (option ``assign_i8 = 1``: assign_i8_kernel's candidate sweep, then
assign_pairs_kernel's exact scores): centre and score bit for bit against ``wdbx_index_search_rows`` with the centres as queries
and against the fp32 route on the same handle, near-tied centres, the candidate buffer overflowed, the edges of the contract,
the per-centre sums, and float64 at a shape the exact path cannot reach."""
import numpy as np
import pytest

from wdbx_amd import _native

pytestmark = pytest.mark.gpu

COSINE, L2 = _native.METRIC_COSINE, _native.METRIC_L2
METRICS = pytest.mark.parametrize("metric", [COSINE, L2])
I8 = 2


def _gauss(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _expected(ix, centers, n):
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
    return np.where(none, -1, best).astype(np.int32), np.where(none, 0, raw[best, np.arange(n)]).astype(np.float32)


def _same(got, want):
    center, score = want
    assert np.array_equal(got["center"], center), np.flatnonzero(got["center"] != center)[:10]
    assert np.array_equal(got["score"].view(np.uint32), score.view(np.uint32))


def _swept(ix, centers, **kw):
    """One call forced onto the int8 route."""
    ix.set_option("assign_i8", 1)
    got = ix.assign(centers, want=kw.pop("want", ("center", "score")), **kw)
    assert ix.get_option("last_assign_path") == I8
    return got


@METRICS
@pytest.mark.parametrize("n", [1, 255, 257, 1500])  # one row, either side of the 256-row tile, a ragged last tile
@pytest.mark.parametrize("dim", [100, 384, 770])    # one k-step pair, the common case, a padded image with blocks of 64 centres
def test_centre_and_score_equal_the_exact_path_bit_for_bit(metric, n, dim):
    block = 128 if -(-dim // 128) * 128 <= 512 else 64
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        ix.add(_gauss(n + dim, n, dim), normalize=metric == COSINE)
        for k in (1, 33, block + 1, 600):
            centers = _gauss(1000 + k, k, dim)
            if metric == COSINE:
                centers = _unit(centers)
            _same(_swept(ix, centers), _expected(ix, centers, n))
            assert ix.get_option("last_assign_center_blocks") == -(-k // block) and ix.get_option("last_assign_pairs") >= n


@METRICS
def test_candidates_decide_between_near_tied_centres(metric):
    n, dim, k = 1500, 384, 40
    centers = _unit(_gauss(5, k, dim))
    centers[1] = centers[0]
    centers[1, 17] = np.nextafter(centers[0, 17], np.float32(np.inf))  # one ulp in one element
    centers[3] = centers[2]                                            # an exact duplicate pair
    centers[5] = centers[4]
    centers[5, 9] += np.float32(1e-4) * np.abs(centers[4]).max()       # below the i8 resolution (max / 127)
    rows = centers[np.arange(n) % k] + np.float32(0.02) * _gauss(6, n, dim)
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        ix.add(rows, normalize=metric == COSINE)
        got = _swept(ix, centers)
        assert ix.get_option("last_assign_pairs") > n  # some row had more than one candidate
        _same(got, _expected(ix, centers, n))
    assert not np.any(got["center"] == 3) and np.any(got["center"] == 2)


@METRICS
@pytest.mark.parametrize("grid", [1, 3])
def test_an_overflowed_candidate_buffer_and_a_small_grid_change_nothing(metric, grid):
    n, dim, k = 1500, 100, 200
    centers = _gauss(11, k, dim)
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        ix.add(_gauss(12, n, dim), normalize=metric == COSINE)
        want = _swept(ix, centers)
        assert ix.get_option("last_assign_sweeps") == 1
        ix.set_option("assign_pair_cap", 64)
        ix.set_option("assign_max_grid", grid)
        got = _swept(ix, centers)
        assert ix.get_option("last_assign_sweeps") == 2 and ix.get_option("last_assign_pairs") > 64
        _same(got, (want["center"], want["score"]))


@METRICS
def test_edges(metric):
    n, dim = 200, 48  # (the shortest rows with an i8 image are 40 floats)
    rows = _gauss(7, n, dim)
    rows[7, 3] = np.nan    # a NaN element
    rows[9] = 0.0          # a zero row
    rows[13, 2] = np.inf   # an infinite element: its group goes to the listed exact pass
    centers = _gauss(8, 6, dim)
    centers[1, 0] = np.nan
    allowed = np.ones(n, bool)
    allowed[11] = False
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        ix.add(rows)
        ix.remove_rows([5])
        mask = _native.pack_row_mask(allowed)
        ix.set_option("assign_i8", 0)
        want = ix.assign(centers, mask=mask, want=("center", "score"))
        assert ix.get_option("last_assign_path") == 1
        got = _swept(ix, centers, mask=mask)
        _same(got, (want["center"], want["score"]))
        assert ix.get_option("last_assign_ambiguous") >= 1 and not np.any(got["center"] == 1)
        for r in (5, 7, 11):
            assert got["center"][r] == -1 and got["score"][r] == 0
        ix.set_rows_at([20], -centers[2:3])  # a replaced row is assigned from its new contents
        got = _swept(ix, centers, mask=mask)
        ix.set_option("assign_i8", 0)
        want = ix.assign(centers, mask=mask, want=("center", "score"))
        _same(got, (want["center"], want["score"]))
        assert got["center"][20] != 2
        for bad in (-2, 2):
            with pytest.raises(_native.HipBackendError) as e:
                ix.set_option("assign_i8", bad)
            assert e.value.code == -1


@METRICS
def test_sums_and_counts_equal_the_fp32_routes(metric):
    n, dim, k = 1500, 100, 33
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        ix.add(_gauss(9, n, dim), normalize=metric == COSINE)
        centers = _gauss(10, k, dim)
        ix.set_option("assign_i8", 0)
        want = ix.assign(centers, normalize=True, want=("center", "sums", "counts"))
        got = _swept(ix, centers, normalize=True, want=("center", "sums", "counts"))
    assert np.array_equal(got["center"], want["center"]) and np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(got["sums"].view(np.uint32), want["sums"].view(np.uint32))


@METRICS
def test_against_float64_where_the_exact_path_cannot_reach(metric):
    n, dim, k = 20000, 384, 257
    rows, centers = _gauss(1, n, dim), _gauss(2, k, dim)
    if metric == COSINE:
        rows, centers = _unit(rows), _unit(centers)
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        ix.add(rows)
        got = _swept(ix, centers, want=("center",))["center"]
        per_row = ix.get_option("last_assign_pairs") / n
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
    print(f"metric {metric} {n}x{dim} K={k}: {per_row:.2f} candidates per row")
