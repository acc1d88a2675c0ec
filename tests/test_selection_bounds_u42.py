"""CPU check of the two error bounds the split six-bit scan relies on (kernels_scan42.h).

The six-bit code of the u6 shadow, u = rint(c / s) + 32, is stored as u = 4 h + l.  The first stage of scan_u42_kernel sees
only h and forms  w4 = s (4 sum h_i q_i - 30.5 sum q_i)  with  a4 >= |c - s (4 h + 1.5 - 32)|_2;  the refine adds
Q = sum l_i q_i and forms  w6 = s ((4 P + Q) - 32 sum q_i)  with  a6 = the u6 shadow's a.  The scan relies on
    |w4 - c.q| <= m4 = a4 |q|_2 (1 + 1e-5) + 6e-6 (dimp + 8) s |q|_1 (1 + 1e-5)
    |w6 - c.q| <= m6 = a6 |q|_2 (1 + 1e-5) + 6e-6 (dimp + 8) s |q|_1 (1 + 1e-5)
These tests restate the quantiser and both bounds in numpy (float32 arithmetic, the kernels' formulas) and check them against
float64: zero violations allowed.
"""
import numpy as np
import pytest

from test_selection_bounds import _datasets
from test_selection_bounds_u6 import _queries, quantise_u6

F32, F64 = np.float32, np.float64


def dimp_of(d):
    return (d + 31) // 32 * 32


def quantise_u42(rows):
    """kernels_scan42.h::rows_to_u42_kernel: (h, l, s, a4, a6) per row.  The codes, s and a6 ARE quantise_u6's; a4 is the
    residual against 4 h - 30.5 by the same arithmetic (fmaf(-s, 4 h - 30.5, x) has ONE rounding), over the row's own
    elements.  NaN / inf rows: {s, a4} = {-1, 0} / {NaN, 0} and a6 = 0, as on the u6 shadow."""
    rows = rows.astype(F32)
    d = rows.shape[1]
    u, s, a6 = quantise_u6(rows)
    h, l = (u >> 2).astype(np.uint8), (u & 3).astype(np.uint8)
    finite = np.isfinite(rows).all(axis=1)
    x = np.where(finite[:, None], rows, F32(0))
    mx = np.max(np.abs(x), axis=1).astype(F32)
    vanishing = mx < F32(1.2e-30)
    safe = np.where(vanishing, F32(1), mx)
    s_raw = np.where(vanishing, F32(0), safe / F32(31.0)).astype(F32)
    inv = np.where(vanishing, F32(0), F32(31.0) / safe).astype(F32)
    k4 = (F32(4.0) * h.astype(F32) - F32(30.5)).astype(F32)
    resid = (x.astype(F64) - s_raw.astype(F64)[:, None] * k4.astype(F64)).astype(F32)
    rho = (resid * inv[:, None]).astype(F32)
    rr = (rho * rho).astype(F32).sum(axis=1, dtype=F32)
    a4 = (s_raw * (np.sqrt(rr, dtype=F32) * F32(1.0005) + F32(1e-4))).astype(F32)
    a4 = np.where(vanishing, mx * (np.sqrt(F32(d)) + F32(1.0)), a4).astype(F32)
    a4 = np.where(finite, a4, F32(0)).astype(F32)
    return h, l, s, a4, a6


def query_sums(q):
    """kernels_scan6.h::u6_query_sums: sum q, |q|_1 and |q|_2 rounded up."""
    q = q.astype(F32)
    q1 = F32(np.abs(q).sum(dtype=F32)) * F32(1.0 + 1e-5)
    q2 = np.sqrt((q * q).sum(dtype=F32), dtype=F32) * F32(1.0 + 1e-5) + F32(1e-37)
    return q.sum(dtype=F32), q1, q2


def u42_first(h, s, q):
    """the first stage: P = sum h_i q_i and w4 = s (4 P - 30.5 sum q), float32 accumulation"""
    q = q.astype(F32)
    p = (h.astype(F32) * q[None, :]).sum(axis=1, dtype=F32)
    w4 = (s * (F32(4.0) * p - F32(30.5) * q.sum(dtype=F32))).astype(F32)
    return p, w4


def u42_refine(p, l, s, q):
    """the refine: Q = sum l_i q_i and w6 = s ((4 P + Q) - 32 sum q)"""
    q = q.astype(F32)
    qq = (l.astype(F32) * q[None, :]).sum(axis=1, dtype=F32)
    return (s * ((F32(4.0) * p + qq).astype(F32) - F32(32.0) * q.sum(dtype=F32))).astype(F32)


def u42_bound(s, a, q, dimp):
    """m4 (a = a4) or m6 (a = a6): a |q|_2 + s * 6e-6 (dimp + 8) |q|_1"""
    _, q1, q2 = query_sums(q)
    round1 = F32(6e-6) * F32(dimp + 8) * q1
    return (a * q2 + s * round1).astype(F32)


def _families(rng, n, d):
    """in the order of importance: uniform elements normalised (the bench corpus), Gaussian, lognormal-scaled, one-hot,
    vanishing magnitude; then the adversarial families of the u8 / u6 bounds tests"""
    uni = rng.random((n, d)) * 2.0 - 1.0
    yield "uniform_normalised", uni / np.linalg.norm(uni, axis=1, keepdims=True)
    yield "gaussian", rng.standard_normal((n, d))
    yield "lognormal_scaled", rng.standard_normal((n, d)) * rng.lognormal(0, 1.5, size=(n, 1))
    hot = np.zeros((n, d))
    hot[np.arange(n), rng.integers(0, d, n)] = rng.standard_normal(n)
    yield "one_hot", hot
    yield "vanishing", 1e-33 * rng.standard_normal((n, d))
    yield from _datasets(rng, n, d)


@pytest.mark.parametrize("d", [32, 96, 384, 416, 768])
def test_u42_bounds_hold(d):
    rng = np.random.default_rng(4200 + d)
    n, dimp = 300, dimp_of(d)
    for name, rows in _families(rng, n, d):
        rows = rows.astype(F32)
        h, l, s, a4, a6 = quantise_u42(rows)
        assert h.max() <= 15 and l.max() <= 3, (d, name)
        for qname, q in _queries(rng, d):
            exact = rows.astype(F64) @ q.astype(F32).astype(F64)
            p, w4 = u42_first(h, s, q)
            slack4 = u42_bound(s, a4, q, dimp).astype(F64) - np.abs(w4.astype(F64) - exact)
            assert np.all(slack4 >= 0), ("m4", d, qname, name, float(slack4.min()))
            w6 = u42_refine(p, l, s, q)
            slack6 = u42_bound(s, a6, q, dimp).astype(F64) - np.abs(w6.astype(F64) - exact)
            assert np.all(slack6 >= 0), ("m6", d, qname, name, float(slack6.min()))


@pytest.mark.parametrize("d", [32, 96, 384, 416, 768])
def test_planes_are_the_u6_code_and_a6_is_the_u6_a(d):
    rng = np.random.default_rng(4300 + d)
    for name, rows in _families(rng, 200, d):
        rows = rows.astype(F32)
        u, s6, a = quantise_u6(rows)
        h, l, s, a4, a6 = quantise_u42(rows)
        assert np.array_equal(4 * h.astype(np.int64) + l, u), (d, name)
        assert np.array_equal(a6.view(np.uint32), a.view(np.uint32)) and np.array_equal(s.view(np.uint32), s6.view(np.uint32)), (d, name)


def test_stored_residuals_cover_the_real_ones():
    """a4 >= |c - s (4 h - 30.5)|_2 and a6 >= |c - s (u - 32)|_2 in float64 (the Cauchy-Schwarz steps need nothing else)"""
    rng = np.random.default_rng(44)
    for d in (32, 96, 416):
        for name, rows in _families(rng, 200, d):
            rows = rows.astype(F32)
            h, l, s, a4, a6 = quantise_u42(rows)
            c, s64 = rows.astype(F64), s.astype(F64)[:, None]
            real4 = np.linalg.norm(c - s64 * (4.0 * h - 30.5), axis=1)
            real6 = np.linalg.norm(c - s64 * (4.0 * h + l - 32.0), axis=1)
            assert np.all(a4.astype(F64) >= real4), (d, name)
            assert np.all(a6.astype(F64) >= real6), (d, name)


def test_the_four_bit_bound_is_wider_but_not_by_much():
    """on dense unit rows a4 is the residual of a grid four times as coarse: about 4 a6 (what decides the survivor share)"""
    rng = np.random.default_rng(45)
    uni = rng.random((2000, 384)) * 2.0 - 1.0
    _, _, _, a4, a6 = quantise_u42((uni / np.linalg.norm(uni, axis=1, keepdims=True)).astype(F32))
    ratio = np.median(a4 / a6)
    assert 3.5 < ratio < 4.5, ratio
