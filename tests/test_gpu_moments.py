"""Moments of the stored rows on the MI355X through ``_native`` (``wdbx_index_moments``): count, fp32 mean and the float64
scatter matrix of the matrix-core pass against numpy float64 of the rows read back with ``get_rows`` -- bit for bit where the
arithmetic is exact, within bounds derived from the chain lengths the library reports otherwise."""
import numpy as np
import pytest

from wdbx_amd import _native

pytestmark = pytest.mark.gpu

COSINE, L2 = _native.METRIC_COSINE, _native.METRIC_L2
# dim -> (metric, forced blocks per group side, expected tile groups): less than a block; two ragged blocks; 3 blocks forced to 2
# a side (two diagonal groups and an off-diagonal one); the whole triangle in one group; 25 blocks = 4 super-rows by the plan
SHAPES = {4: (L2, 0, 1), 33: (COSINE, 0, 1), 96: (L2, 2, 3), 384: (COSINE, 0, 1), 800: (L2, 0, 10)}


def _fill(ix, rows, spoil):
    """The rows in; with ``spoil`` some removed, one with a NaN and one with an infinite element, and a mask.  Returns the
    mask words and the counted rows as stored."""
    n = len(rows)
    allowed = np.ones(n, bool)
    if spoil:
        rows = rows.copy()
        rows[17, 1], rows[40, 0] = np.nan, np.inf
        allowed[np.random.default_rng(n).random(n) < 0.3] = False
    ix.add(rows, normalize=ix.metric == COSINE)
    if spoil:
        ix.remove_rows([5, 64, n - 1])
    stored = ix.get_rows(0, n)
    counted = allowed & np.isfinite(stored).all(axis=1)
    return (_native.pack_row_mask(allowed) if spoil else None), stored[counted]


@pytest.mark.parametrize("n", [1, 63, 5000])
@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_mean_and_scatter_within_the_chain_bounds(dim, n):
    """Scatter, per element: a range's partial is one fp32 fma chain over its L rows (uncounted rows and the padding add exact
    zeros), so it is within gamma_L sum |a_ri a_rj| of the exact sum of the staged a = x (-) mean, gamma_L = L u / (1 - L u) <=
    (L + 4) u for every L here (L^2 u < 4), u = 2^-24; the fp32 -> float64 conversions are exact and the fold of P partials
    adds at most P 2^-53 of the same sum.  a is recomputed here from the RETURNED mean with numpy's fp32 subtraction, the
    staging's own.  Mean: a range's column sum is a chain of at most Ls - 1 fp32 additions, the fold of Ps sums Ps - 1 more,
    the division one (the count converts exactly below 2^24): (Ls + Ps + 2) u sum |x_ri| / n covers them with the second-order
    terms."""
    metric, side, groups = SHAPES[dim]
    rows = np.random.default_rng(dim + n).standard_normal((n, dim)).astype(np.float32) + np.float32(0.25)
    with _native.NativeIndex(dim, metric=metric, capacity_rows=n) as ix:
        mask, x = _fill(ix, rows, spoil=n == 5000)
        ix.set_option("moments_tiles_per_group", side)
        for partials in ((0, 1, 7, 1000) if n == 5000 else (0,)):  # (1000: more than the 157 chunks of 32 rows)
            ix.set_option("moments_partials", partials)
            got = ix.moments(center=True, mask=mask)
            again = ix.moments(center=True, mask=mask)
            L, P = ix.get_option("last_moments_range_rows"), ix.get_option("last_moments_partials")
            Ls, Ps = ix.get_option("last_moments_sum_rows"), ix.get_option("last_moments_sum_partials")
            assert ix.get_option("last_moments_tile_groups") == groups and ix.get_option("last_moments_launches") == 4
            assert (P == partials if partials in (1, 7) else 1 <= P <= -(-n // 32)) and L % 32 == 0 and (P - 1) * L < n <= P * L
            assert partials != 1000 or P > 7  # (cut to what the chunks and 256 MiB of partials allow)
            assert got["count"] == len(x)
            x64 = x.astype(np.float64)
            mean_err = np.abs(got["mean"].astype(np.float64) - x64.mean(axis=0))
            mean_bound = (Ls + Ps + 2) * 2.0 ** -24 * np.abs(x64).sum(axis=0) / len(x)
            a = (x - got["mean"][None, :]).astype(np.float64)  # (fp32 subtraction, then exact)
            err = np.abs(got["scatter"] - a.T @ a)
            bound = ((L + 4) * 2.0 ** -24 + P * 2.0 ** -53) * (np.abs(a).T @ np.abs(a))
            print(f"{n}x{dim} partials {P}x{L}: scatter err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
                  f"mean err/bound {np.max(mean_err / np.maximum(mean_bound, 1e-300)):.3f}")
            assert np.all(mean_err <= mean_bound)
            assert np.all(err <= bound)
            assert np.array_equal(got["scatter"].view(np.uint64), got["scatter"].T.copy().view(np.uint64))
            assert np.array_equal(got["scatter"].view(np.uint64), again["scatter"].view(np.uint64))
            assert np.array_equal(got["mean"].view(np.uint32), again["mean"].view(np.uint32))


@pytest.mark.parametrize("dim, n", [(33, 63), (96, 5000), (384, 5000), (800, 1500)])
def test_small_integer_rows_are_exact(dim, n):
    """center = 0 on rows of integers in [-8, 8]: every fp32 product and every partial sum is an integer below 2^24."""
    side = SHAPES[dim][1]
    rows = np.random.default_rng(dim).integers(-8, 9, (n, dim)).astype(np.float32)
    with _native.NativeIndex(dim, metric=L2, capacity_rows=n) as ix:
        mask, x = _fill(ix, rows, spoil=n >= 1500)
        ix.set_option("moments_tiles_per_group", side)
        for partials in (0, 7):
            ix.set_option("moments_partials", partials)
            got = ix.moments(center=False, mask=mask)
            xi = x.astype(np.int64)
            assert got["count"] == len(x)
            assert np.array_equal(got["scatter"], (xi.T @ xi).astype(np.float64))
            assert np.array_equal(got["mean"], xi.sum(axis=0).astype(np.float32) / np.float32(len(x)))


def test_many_equal_rows_of_dimension_three():
    row = np.array([3, -2, 5], np.float32)
    with _native.NativeIndex(3, metric=L2, capacity_rows=1000) as ix:
        ix.add(np.tile(row, (1000, 1)))
        got = ix.moments(center=True)
        assert got["count"] == 1000 and np.array_equal(got["mean"], row) and not got["scatter"].any()
        assert np.array_equal(ix.moments(center=False)["scatter"], 1000.0 * np.outer(row, row))


def test_nothing_counted_and_the_refused_calls_leave_the_handle_usable():
    n, dim = 100, 20
    rows = np.random.default_rng(3).standard_normal((n, dim)).astype(np.float32)
    with _native.NativeIndex(dim, metric=L2, capacity_rows=n) as ix:
        ix.add(rows)
        got = ix.moments(center=True, mask=_native.pack_row_mask(np.zeros(n, bool)))
        assert got["count"] == 0 and not got["mean"].any() and not got["scatter"].any()
        assert ix.get_option("last_moments_launches") == 2 and ix.get_option("last_moments_partials") == 0  # (no scatter launch)
        with pytest.raises(_native.HipBackendError):
            ix.moments(center=2)
        with pytest.raises(_native.HipBackendError):
            ix.moments(mask=np.zeros(3, np.uint32))  # 4 words needed
        assert ix._lib.wdbx_index_moments(ix._h, 1, None, 0, None, None, None) != 0  # every output null
        idx, _ = ix.search(rows[7], 1)
        assert idx[0, 0] == 7
        assert ix.moments(want=("mean",))["count"] == n
    with _native.NativeIndex(4100, metric=L2, capacity_rows=1) as big:
        big.add(np.ones((1, 4100), np.float32))
        with pytest.raises(_native.HipBackendError):
            big.moments(want=("scatter",))
        assert big.moments(want=("mean",))["count"] == 1
