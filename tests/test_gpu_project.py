"""Projection of the stored rows on the MI355X through ``_native`` (``wdbx_index_project``): every row's coordinates on up to
32 directions against numpy -- bit for bit on small integers, within the chain's bound on floats -- zeros for uncounted rows,
nothing written behind the output."""
import ctypes as C

import numpy as np
import pytest

from wdbx_amd import _native

pytestmark = pytest.mark.gpu

DIMS = [4, 33, 96, 384, 800]  # less than a block of 32 columns, two ragged blocks, whole blocks, the flagship, 25 blocks
MS = [1, 2, 31, 32]           # scalar stores (1, 2, 31) and 16-byte stores (32); one and both lane halves


def _index(rows, n):
    """The rows in (the callers' 2 989: 24 tiles of 128, the last one ragged), some removed, a NaN and an infinite element, a
    mask.  Returns the index, the mask words and which rows count."""
    rows = rows.copy()
    rows[17, 1], rows[40, 0] = np.nan, np.inf
    allowed = np.ones(n, bool)
    allowed[np.random.default_rng(n).random(n) < 0.3] = False
    ix = _native.NativeIndex(rows.shape[1], metric=_native.METRIC_L2, capacity_rows=n)
    ix.add(rows)
    ix.remove_rows([5, 64, n - 1])
    counted = allowed & np.isfinite(ix.get_rows(0, n)).all(axis=1)
    return ix, _native.pack_row_mask(allowed), counted


@pytest.mark.parametrize("dim", DIMS)
def test_coordinates_exact_on_integers_and_within_the_chain_bound_on_floats(dim):
    """out[r][c] is one fp32 fma chain over the dp = 32 ceil(dim / 32) staged columns of x (-) offset (the padding adds exact
    zeros): within gamma_dp sum_i |x_i (-) o_i| |b_ci| of the exact sum of those fp32 differences, gamma_dp <= (dp + 2) 2^-24."""
    n, rng = 2989, np.random.default_rng(dim)
    ints = rng.integers(-8, 9, (n, dim)).astype(np.float32)
    floats = rng.standard_normal((n, dim)).astype(np.float32)
    dp = 32 * -(-dim // 32)
    for rows, basis_all, offset in ((ints, rng.integers(-4, 5, (32, dim)).astype(np.float32), rng.integers(-3, 4, dim).astype(np.float32)),
                                    (floats, rng.standard_normal((32, dim)).astype(np.float32), rng.standard_normal(dim).astype(np.float32))):
        ix, mask, counted = _index(rows, n)
        with ix:
            x = ix.get_rows(0, n)[counted]
            for m in MS:
                basis = basis_all[:m]
                got = ix.project(basis, offset=offset, mask=mask)
                assert got.shape == (n, m) and not got[~counted].any()  # uncounted rows: all zeros
                a = (x - offset[None, :]).astype(np.float64)             # (fp32 subtraction, then exact)
                want = a @ basis.astype(np.float64).T
                if rows is ints:  # |sum| <= 800 * 11 * 4 < 2^24: every product and partial sum exact
                    assert np.array_equal(got[counted], want.astype(np.float32))
                else:
                    bound = (dp + 2) * 2.0 ** -24 * (np.abs(a) @ np.abs(basis.astype(np.float64)).T)
                    err = np.abs(got[counted] - want)
                    print(f"dim {dim} m {m}: err/bound {np.max(err / bound):.3f}")
                    assert np.all(err <= bound)


def test_more_tiles_than_resident_workgroups():
    """782 tiles of two K chunks: more than the 768 resident workgroups of 256 CUs, so the loader's cursor crosses a tile boundary."""
    n, dim = 100_003, 33
    rng = np.random.default_rng(9)
    rows, basis = rng.integers(-8, 9, (n, dim)).astype(np.float32), rng.integers(-4, 5, (4, dim)).astype(np.float32)
    with _native.NativeIndex(dim, metric=_native.METRIC_L2, capacity_rows=n) as ix:
        ix.add(rows)
        assert np.array_equal(ix.project(basis), rows @ basis.T)


def test_guard_word_and_the_refused_calls():
    n, dim, m = 300, 33, 31
    rows = np.random.default_rng(1).standard_normal((n, dim)).astype(np.float32)
    with _native.NativeIndex(dim, metric=_native.METRIC_COSINE, capacity_rows=n) as ix:
        ix.add(rows, normalize=True)
        basis = np.ones((m, dim), np.float32)
        buf = np.full(n * m + 1, np.float32(-7.5))  # the output and one guard word behind it
        f32p = C.POINTER(C.c_float)
        assert ix._lib.wdbx_index_project(ix._h, basis.ctypes.data_as(f32p), m, None, None, 0, buf.ctypes.data_as(f32p)) == 0
        assert buf[-1] == np.float32(-7.5) and np.array_equal(buf[:-1].reshape(n, m), ix.project(basis))
        for bad in (0, 33):
            with pytest.raises(_native.HipBackendError):
                ix.project(np.ones((bad, dim), np.float32))
        with pytest.raises(_native.HipBackendError):
            ix.project(basis, mask=np.zeros(3, np.uint32))  # 10 words needed
        assert ix._lib.wdbx_index_project(ix._h, None, 2, None, None, 0, buf.ctypes.data_as(f32p)) != 0
        idx, _ = ix.search(rows[7], 1, normalize_queries=True)
        assert idx[0, 0] == 7
