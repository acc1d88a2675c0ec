"""CPU check of the error bound the six-bit selection scan relies on (kernels_scan6.h).

The u6 shadow keeps per row 6-bit codes u = round(c / s) + 32, s = max|c| / 31, and a >= |c - s (u - 32)|_2, the norm of the
row's actual quantisation residual rounded up.  The scan forms w = s (sum u_i q_i - 32 sum q_i) in fp32 and relies on
    |w - c.q| <= m = a |q|_2 (1 + 1e-5) + 6e-6 (dimp + 8) s |q|_1 (1 + 1e-5)
These tests restate the quantiser and the bound in numpy (float32 arithmetic, the kernels' formulas) and check them against
float64 on the row families of test_selection_bounds.py: zero violations allowed.
"""
import numpy as np
import pytest

from test_selection_bounds import _datasets


def quantise_u6(rows):
    """kernels_scan6.h::rows_to_u6_kernel: codes, s and a per row (float32; fmaf(-s, k, x) has ONE rounding).  A row with a
    NaN element: {-1, 0}, a row with an infinite element (and no NaN): {NaN, 0}; both all codes 32."""
    rows = rows.astype(np.float32)
    d = rows.shape[1]
    has_nan = np.isnan(rows).any(axis=1)
    finite = np.isfinite(rows).all(axis=1)
    rows = np.where(finite[:, None], rows, np.float32(0))
    mx = np.max(np.abs(rows), axis=1).astype(np.float32)
    vanishing = mx < np.float32(1.2e-30)                      # 31 / max would overflow: every code 32, s = 0, a = max (sqrt(d) + 1)
    safe = np.where(vanishing, np.float32(1), mx)
    s = np.where(vanishing, np.float32(0), safe / np.float32(31.0)).astype(np.float32)
    inv = np.where(vanishing, np.float32(0), np.float32(31.0) / safe).astype(np.float32)
    x = np.where(vanishing[:, None], np.float32(0), rows)
    k = np.clip(np.rint((x * inv[:, None]).astype(np.float32)), -31, 31).astype(np.float32)
    resid = (x.astype(np.float64) - s.astype(np.float64)[:, None] * k.astype(np.float64)).astype(np.float32)
    rho = (resid * inv[:, None]).astype(np.float32)
    rr = (rho * rho).astype(np.float32).sum(axis=1, dtype=np.float32)
    a = (s * (np.sqrt(rr, dtype=np.float32) * np.float32(1.0005) + np.float32(1e-4))).astype(np.float32)
    a = np.where(vanishing, mx * (np.sqrt(np.float32(d)) + np.float32(1.0)), a).astype(np.float32)
    s = np.where(has_nan, np.float32(-1.0), np.where(finite, s, np.float32(np.nan))).astype(np.float32)
    a = np.where(finite, a, np.float32(0)).astype(np.float32)
    return (k + 32).astype(np.uint8), s, a


def u6_score(u, s, q):
    """kernels_scan6.h::scan8_u6_kernel: w = s * (sum u_i q_i - 32 sum q_i), float32 accumulation."""
    q = q.astype(np.float32)
    dot = (u.astype(np.float32) * q[None, :]).sum(axis=1, dtype=np.float32)
    return (s * (dot - np.float32(32.0) * q.sum(dtype=np.float32))).astype(np.float32)


def u6_bound(s, a, q, dimp):
    """kernels_scan6.h::u6_query_sums + the kernels' m."""
    q = q.astype(np.float32)
    q1 = np.float32(np.abs(q).sum(dtype=np.float32)) * np.float32(1.0 + 1e-5)
    q2 = np.sqrt((q * q).sum(dtype=np.float32), dtype=np.float32) * np.float32(1.0 + 1e-5) + np.float32(1e-37)
    round1 = np.float32(6e-6) * np.float32(dimp + 8) * q1
    return (a * q2 + s * round1).astype(np.float32)


def _queries(rng, d):
    return (("normal", rng.standard_normal(d)), ("ones", np.ones(d)), ("alternating", (-1.0) ** np.arange(d)),
            ("one_hot", np.eye(d)[3]), ("huge", 1e6 * rng.standard_normal(d)), ("heavy_tail", rng.standard_t(1.5, size=d)))


@pytest.mark.parametrize("d", [96, 128, 384, 400, 768, 4096])
def test_u6_row_bound_holds(d):
    rng = np.random.default_rng(600 + d)
    n = 400
    for qname, q in _queries(rng, d):
        for name, rows in _datasets(rng, n, d):
            rows = rows.astype(np.float32)
            u, s, a = quantise_u6(rows)
            assert u.min() >= 1 and u.max() <= 63, (d, name)
            w = u6_score(u, s, q).astype(np.float64)
            exact = rows.astype(np.float64) @ q.astype(np.float32).astype(np.float64)
            m = u6_bound(s, a, q, d).astype(np.float64)
            slack = m - np.abs(w - exact)
            assert np.all(slack >= 0), (d, qname, name, float(slack.min()), float(m.max()))


def test_u6_stored_residual_covers_the_real_one():
    """a >= |c - s k|_2 in float64, on every family (the Cauchy-Schwarz step needs nothing else of the quantiser)."""
    rng = np.random.default_rng(66)
    for d in (96, 384, 4096):
        for name, rows in _datasets(rng, 300, d):
            rows = rows.astype(np.float32)
            u, s, a = quantise_u6(rows)
            real = np.linalg.norm(rows.astype(np.float64) - s.astype(np.float64)[:, None] * (u.astype(np.float64) - 32.0), axis=1)
            assert np.all(a.astype(np.float64) >= real), (d, name, float((a - real).min()))


def test_u6_code_packing_round_trips():
    """The unit layout of the shadow: dword t byte b = code 4t+b | bits [2t, 2t+1] of code 12+b << 6; the kernel's extraction."""
    rng = np.random.default_rng(6)
    codes = rng.integers(1, 64, size=(1000, 16)).astype(np.uint32)
    dw = np.zeros((1000, 3), np.uint32)
    for t in range(3):
        for b in range(4):
            dw[:, t] |= (codes[:, 4 * t + b] | (((codes[:, 12 + b] >> (2 * t)) & 3) << 6)) << (8 * b)
    out = np.zeros_like(codes)
    for t in range(3):
        lo = dw[:, t] & 0x3F3F3F3F
        for b in range(4):
            out[:, 4 * t + b] = (lo >> (8 * b)) & 0xFF
    hi = ((dw[:, 0] >> 6) & 0x03030303) | ((dw[:, 1] >> 4) & 0x0C0C0C0C) | ((dw[:, 2] >> 2) & 0x30303030)
    for b in range(4):
        out[:, 12 + b] = (hi >> (8 * b)) & 0xFF
    assert np.array_equal(out, codes)


def test_u6_bound_is_tighter_than_the_linf_l1_form():
    """On dense unit rows the stored-residual bound is clearly below 0.51 s |q|_1 at the same 6 bits (what makes 6 bits pay)."""
    rng = np.random.default_rng(7)
    d = 384
    rows = rng.standard_normal((2000, d)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    q = rng.standard_normal(d).astype(np.float32)
    q /= np.linalg.norm(q)
    _, s, a = quantise_u6(rows)
    m = u6_bound(s, a, q, d)
    linf = np.float32(0.51) * s * np.float32(np.abs(q).sum())
    assert np.median(m) < 0.8 * np.median(linf)
