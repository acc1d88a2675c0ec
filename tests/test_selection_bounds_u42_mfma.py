"""CPU check of the bounds the matrix-core full pass of the split planes relies on (kernels_scan42.h).

The query is a 16-bit fixed-point number, Q_i = rint(q_i / delta) = 256 H_i + L_i with delta a power of two, and the first stage
is the exact integer sum P_int = sum h_i Q_i.  With P^ = delta float(P_int) the pass relies on
    |w4 - c.q| <= m4' = a4 |q|_2 (1 + 1e-5) + s round1',   w4 = s (4 P^ - 30.5 sum q)
    |w6 - c.q| <= m6' = a6 |q|_2 (1 + 1e-5) + s round1',   w6 = s ((4 P^ + sum l_i q_i) - 32 sum q)
    round1' = 6e-6 (dimp + 8) |q|_1 (1 + 1e-5) + dimp 2^-138 + 60 sqrt(dimp) e2 (1 + 1e-5),   e2 >= |q - delta Q|_2
These tests restate the query quantiser and both bounds in numpy (tests/u42_mfma_model.py: float32 arithmetic, the kernels'
formulas) and check them against float64: zero violations allowed.

Queries of magnitude 1e-30 and 1e30 lie outside [2^-44, 2^64) and are MARKED under this design: they take no part in the
integer sum and every row is their candidate, so there is no bound to violate; test_marked_queries asserts that they are
marked and that their operand bytes are zero.  The bound check runs the magnitudes just inside the limits instead
(small_in_range, large_in_range)."""
import numpy as np
import pytest

import u42_mfma_model as M
from test_selection_bounds_u42 import quantise_u42

F32, F64 = np.float32, np.float64
DIMS = [288, 320, 352, 384]  # 9 to 12 units: every instanced row (a short last chunk of one, two, three units and the full one)


def _rows(rng, n, d):
    uni = rng.random((n, d)) * 2.0 - 1.0
    yield "uniform_normalised", uni / np.linalg.norm(uni, axis=1, keepdims=True)
    yield "gaussian", rng.standard_normal((n, d))
    yield "scaled", rng.standard_normal((n, d)) * rng.lognormal(0, 1.5, size=(n, 1))
    yield "all_15", np.ones((n, d)) * rng.lognormal(0, 1.0, size=(n, 1))     # every code 63: h = 15, l = 3
    yield "all_0", -np.ones((n, d)) * rng.lognormal(0, 1.0, size=(n, 1))


def _queries(rng, d):
    g = rng.standard_normal(d)
    dom = 1e-4 * rng.standard_normal(d)
    dom[5] = 3.0
    hot = np.zeros(d)
    hot[7] = -1.0
    yield "gaussian", g
    yield "unit", g / np.linalg.norm(g)
    yield "ones", np.ones(d)
    yield "one_dominant", dom
    yield "one_hot", hot
    yield "at_32512", np.where(np.arange(d) % 2 == 0, 32512.0, -32511.5) * 2.0 ** -10
    yield "small_in_range", g * 2.0 ** -42 / np.abs(g).max() * 1.5
    yield "large_in_range", g * 2.0 ** 62 / np.abs(g).max()
    yield "zero", np.zeros(d)


@pytest.mark.parametrize("d", DIMS)
def test_query_quantiser(d):
    rng = np.random.default_rng(4600 + d)
    for name, q in _queries(rng, d):
        q = q.astype(F32)
        qq = M.quantise_query(q)
        assert not qq["marked"], name
        Q, H, L = qq["Q"].astype(np.int64), qq["H"].astype(np.int64), qq["L"].astype(np.int64)
        assert np.array_equal(256 * H + L, Q), name
        assert H.min() >= -128 and H.max() <= 127 and L.min() >= -128 and L.max() <= 127, name
        assert np.abs(Q).max() <= M.QMAX, name
        delta = F64(qq["delta"])
        assert np.log2(delta) == np.round(np.log2(delta)), name
        if name == "zero":
            assert delta == 1.0 and not Q.any() and qq["e2"] == 0
            continue
        assert np.abs(Q).max() > M.QMAX // 2, name   # (the smallest such power of two)
        real = np.linalg.norm(q.astype(F64) - delta * Q)
        assert F64(qq["e2"]) >= real, (name, float(qq["e2"]), real)
        assert F64(qq["e2"]) <= 1.001 * real + delta * 2e-20, (name, float(qq["e2"]), real)
        assert np.isfinite(qq["e2"]) and (qq["e2"] == 0 or qq["e2"] >= 2.0 ** -126), name


def test_marked_queries():
    rng = np.random.default_rng(46)
    g = rng.standard_normal(384)
    for name, q in (("1e-30", g * 1e-30), ("1e30", g * 1e30), ("nan", np.where(np.arange(384) == 3, np.nan, g)),
                    ("inf", np.where(np.arange(384) == 9, np.inf, g)), ("below_2^-44", g / np.abs(g).max() * 2.0 ** -44.01),
                    ("at_2^64", g / np.abs(g).max() * 2.0 ** 64)):
        qq = M.quantise_query(q.astype(F32))
        assert qq["marked"] and not qq["Q"].any(), name
    for name, q in (("at_2^-44", g / np.abs(g).max() * 2.0 ** -44), ("below_2^64", g / np.abs(g).max() * 2.0 ** 63.99)):
        assert not M.quantise_query(q.astype(F32))["marked"], name


def test_p_int_stays_in_int32_at_the_largest_instance():
    assert 15 * M.QMAX * M.MAX_DIMP < 2 ** 31
    assert 256 * (15 * 127 * M.MAX_DIMP) + 15 * 128 * M.MAX_DIMP < 2 ** 31   # 256 Dh + Dl term by term
    h = np.full((1, M.MAX_DIMP), 15, np.uint8)
    for sign in (1, -1):
        p4, p_int = M.p_bits(h, np.full(M.MAX_DIMP, sign * M.QMAX, np.int32), F32(2.0 ** -9))
        assert p_int[0] == sign * 15 * M.QMAX * M.MAX_DIMP


@pytest.mark.parametrize("d", DIMS)
def test_u42_mfma_bounds_hold(d):
    rng = np.random.default_rng(4700 + d)
    n = 300
    for name, rows in _rows(rng, n, d):
        rows = rows.astype(F32)
        h, l, s, a4, a6 = quantise_u42(rows)
        if name == "all_15":
            assert (h == 15).all()
        for qname, q in _queries(rng, d):
            q = q.astype(F32)
            qq = M.quantise_query(q)
            kc = M.query_consts(q, qq)
            exact = rows.astype(F64) @ q.astype(F64)
            p4, p_int = M.p_bits(h, qq["Q"], kc["dp"])
            # the carried value is the exact integer sum times a power of two, rounded once
            assert np.array_equal(p4, (p_int.astype(F64) * F64(kc["dp"])).astype(F32))
            w4, m4 = M.first_stage(p4, s, a4, kc)
            ok4 = ~np.isfinite(m4.astype(F64) + w4.astype(F64)) | (np.abs(w4.astype(F64) - exact) <= m4.astype(F64))
            assert ok4.all(), ("m4'", d, qname, name, int((~ok4).sum()))
            w6, m6 = M.refine(p4, l, s, a6, q, kc)
            ok6 = ~np.isfinite(m6.astype(F64) + w6.astype(F64)) | (np.abs(w6.astype(F64) - exact) <= m6.astype(F64))
            assert ok6.all(), ("m6'", d, qname, name, int((~ok6).sum()))


def test_the_query_term_is_small_on_unit_queries():
    """the estimate behind the design: on a unit query at d = 384 the addend 60 sqrt(dimp) e2 is far below a4 |q|_2 of a dense
    unit row (a4 about 4 s sqrt(d / 12), s = max|c| / 31)"""
    rng = np.random.default_rng(48)
    g = rng.standard_normal(384)
    q = (g / np.linalg.norm(g)).astype(F32)
    qq = M.quantise_query(q)
    rows = rng.random((200, 384)) * 2 - 1
    rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(F32)
    _, _, s, a4, _ = quantise_u42(rows)
    term = 60.0 * np.sqrt(384.0) * F64(qq["e2"]) * s.astype(F64)
    assert np.all(term < 0.05 * a4.astype(F64))
