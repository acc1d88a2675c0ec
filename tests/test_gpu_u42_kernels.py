"""The split six-bit planes' kernels ALONE on the MI355X (kernels_scan42.h), launched by tests/kernel_harness/u42_harness.hip:
the quantiser against its numpy restatement and against rows_to_u6_kernel on the same rows, and the full pass -- first stage,
dense refine, candidate stage -- against float64 on planes, thresholds and grids chosen here.

The full pass runs with gridDim.x of 1 and 3 over 10 000 rows, so every wave walks at least 13 tiles, carries survivors from
tile to tile and refines several times inside its loop; through the service (tests/test_gpu_u42_scan.py, 40 000 rows) no wave
ever sees a second tile."""
import numpy as np
import pytest

import select_harness as S
import u42_harness as H
from test_selection_bounds_u42 import dimp_of, quantise_u42, query_sums, u42_bound, u42_first, u42_refine

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64


def _unit(a):
    n = np.linalg.norm(a, axis=1, keepdims=True)
    return (a / np.where(n > 0, n, 1)).astype(F32)


def _pad(x, width, value=0):
    out = np.full((x.shape[0], width), value, x.dtype)
    out[:, :x.shape[1]] = x
    return out


# --------------------------------------------------------------------------- #
# layouts (CPU)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("units", [1, 3, 13])
def test_plane_layouts_round_trip(units):
    rng = np.random.default_rng(units)
    n = 130
    h = rng.integers(0, 16, size=(n, units * 32)).astype(np.uint8)
    l = rng.integers(0, 4, size=(n, units * 32)).astype(np.uint8)
    a6 = rng.random(n).astype(F32)
    dw = H.pack_h(h)
    assert dw.shape == (3, units, 64, 4) and np.array_equal(H.unpack_h(dw, n), h)
    # row r of tile t, unit u: the 16 bytes at dword offset ((t * units + u) * 64 + r) * 4
    flat = dw.reshape(-1)
    r, u = 77, units - 1
    at = ((1 * units + u) * 64 + (r - 64)) * 4
    assert (flat[at] & 0xF) == h[r, u * 32] and ((flat[at + 3] >> 28) & 0xF) == h[r, u * 32 + 31]
    rec = H.pack_l(l, a6)
    assert rec.shape == (n, H.lpitch_py(units)) and rec.shape[1] % 32 == 0 and rec.shape[1] >= units * 2 + 1
    l2, a_bits = H.unpack_l(rec, units)
    assert np.array_equal(l2, l) and np.array_equal(a_bits, a6.view(U32))
    assert (rec[5, 0] & 3) == l[5, 0] and ((rec[5, 0] >> 2) & 3) == l[5, 4] and ((rec[5, 0] >> 8) & 3) == l[5, 1]


def test_unit_chunks():
    assert [H.unit_chunk_py(u) for u in (0, 1, 3, 4, 5, 6, 12, 13, 24, 128)] == [0, 4, 4, 4, 6, 6, 6, 8, 8, 8]


# --------------------------------------------------------------------------- #
# the quantiser
# --------------------------------------------------------------------------- #
def _quant_corpus(rng, n, d):
    rows = rng.standard_normal((n, d)).astype(F32)
    rows[::3] = _unit(rng.random((len(rows[::3]), d)) * 2 - 1)
    rows[1::7] *= F32(1e-33)                 # vanishing magnitude
    if n > 10:
        rows[4, d // 2] = np.nan
        rows[5, 1] = np.inf
        rows[6, :] = 0
        rows[7] = 0
        rows[7, d - 1] = -3.0                # one-hot
    return rows


def _check_quantiser(out, rows, d, lo, hi):
    """rows [lo, hi) of the harness output against the restatement and against the u6 kernel's output"""
    n_alloc, dimp = len(rows), dimp_of(d)
    units = dimp // 32
    h_ref, l_ref, s_ref, a4_ref, _ = quantise_u42(rows[:, :d])
    h = H.unpack_h(out["h"], n_alloc)[lo:hi]
    l, a6_bits = H.unpack_l(out["lrec"], units)
    l, a6_bits = l[lo:hi], a6_bits[lo:hi]
    sa4, sa6 = out["sa4"][lo:hi], out["sa6"][lo:hi]
    assert np.array_equal(h[:, :d], h_ref[lo:hi]) and np.array_equal(l[:, :d], l_ref[lo:hi]), "planes against the restatement"
    assert (h[:, d:] == 8).all() and (l[:, d:] == 0).all(), "a padding element is not the zero point"
    u6 = S.unpack_u6(out["codes6"], n_alloc)[lo:hi]
    assert np.array_equal(4 * h.astype(np.int64) + l, u6), "4 h + l is not the u6 kernel's code"
    assert np.array_equal(sa4[:, 0], sa6[:, 0]), "s differs from the u6 kernel's"
    assert np.array_equal(a6_bits, sa6[:, 1]), "a6 differs from the u6 kernel's a"
    cls = S.row_class(rows[lo:hi, :d])
    fin = cls == 0
    assert np.array_equal(sa4[fin, 0], s_ref[lo:hi].view(U32)[fin]), "s bits against the restatement"
    assert (sa4[cls == 1, 0] == F32(-1.0).view(U32)).all() and (sa4[cls == 1, 1] == 0).all()
    assert np.isnan(sa4[cls == 2, 0].copy().view(F32)).all() and (sa4[cls == 2, 1] == 0).all()
    # a4: SAFE against the float64 residual, and the documented number: (1.0005 |r4|_2 + 1e-4 s) within gamma(dimp + 16)
    # (check_u6_quantiser's form and reasoning, tests/test_gpu_select_kernels.py)
    a4 = sa4[:, 1].copy().view(F32).astype(F64)[fin]
    s64 = sa4[:, 0].copy().view(F32).astype(F64)[fin]
    c = rows[lo:hi, :d][fin].astype(F64)
    real = np.linalg.norm(c - s64[:, None] * (4.0 * h[fin][:, :d] - 30.5), axis=1)
    assert np.all(a4 >= real), "SAFETY: a4 below the real residual norm"
    mx = np.abs(rows[lo:hi, :d][fin]).max(axis=1)
    van = mx < F32(1.2e-30)
    g = S.gamma(dimp + 16)
    form = 1.0005 * real + 1e-4 * s64
    assert np.all(a4[~van] <= form[~van] * (1 + g)) and np.all(a4[~van] >= form[~van] * (1 - g) - 1e-11 * s64[~van]), "a4 is not its documented form"
    want = (mx[van].astype(F32) * (np.sqrt(F32(d)) + F32(1.0))).astype(F64)
    assert np.all(np.abs(a4[van] - want) <= 4 * S.U * want + 2.0 ** -149), "a4 of a vanishing row"
    ref = a4_ref[lo:hi].astype(F64)[fin]
    assert np.all(np.abs(a4 - ref) <= 2 * g * ref + 2.0 ** -149), "a4 against the restatement"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4161])
@pytest.mark.parametrize("d", [93, 416])
def test_rows_to_u42_kernel_matches_its_restatement(n, d):
    rng = np.random.default_rng(1000 * d + n)
    rows = _pad(_quant_corpus(rng, n, d), dimp_of(d))
    out = H.quantise(rows, d)
    _check_quantiser(out, rows, d, 0, n)
    # incremental builds: rows outside [r0, n1) keep the sentinels, the rows inside are the same whatever the grid
    units = dimp_of(d) // 32
    per_row = out["h"].transpose(0, 2, 1, 3).reshape(-1, units, 4)
    for r0, n1, grid in ((min(5, n - 1), n, 0), (n // 2, max(n // 2, n - 3), 1), (min(63, n - 1), min(66, n), 7)):
        o2 = H.quantise(rows, d, r0=r0, n=n1, grid=grid)
        pr2 = o2["h"].transpose(0, 2, 1, 3).reshape(-1, units, 4)
        assert np.array_equal(pr2[r0:n1], per_row[r0:n1]) and np.array_equal(o2["sa4"][r0:n1], out["sa4"][r0:n1])
        assert np.array_equal(o2["lrec"][r0:n1, :units * 2 + 1], out["lrec"][r0:n1, :units * 2 + 1])
        assert (pr2[:r0] == S.SENT_U32).all() and (pr2[n1:] == S.SENT_U32).all()
        assert (o2["sa4"][:r0] == S.SENT_F32).all() and (o2["sa4"][n1:] == S.SENT_F32).all()
        assert (o2["lrec"][:r0] == S.SENT_U32).all() and (o2["lrec"][n1:] == S.SENT_U32).all()


# --------------------------------------------------------------------------- #
# the full pass
# --------------------------------------------------------------------------- #
N_PASS = 10_000
_PASS = {}


def _pass_case(d):
    """10 000 rows, planes packed from the restatement, one query, float64 truth and the float64 forms of both stages --
    computed once per dimension and shared, never modified"""
    if d not in _PASS:
        rng = np.random.default_rng(42 + d)
        rows = _unit(rng.standard_normal((N_PASS, d)))
        rows[100, 3] = np.nan               # never a candidate
        rows[200, 5] = np.inf               # always one, with a +inf key
        rows[300] *= F32(1e-33)
        q = _unit(rng.standard_normal((1, d)))[0]
        dimp = dimp_of(d)
        h, l, s, a4, a6 = quantise_u42(rows)
        cls = S.row_class(rows)
        truth = S.scores64(rows, q)
        qq = q.astype(F64)
        s64 = s.astype(F64)
        p64 = h.astype(F64) @ qq
        w4_64 = s64 * (4.0 * p64 - 30.5 * qq.sum())
        w6_64 = s64 * (4.0 * p64 + l.astype(F64) @ qq - 32.0 * qq.sum())
        rnd = 6e-6 * (dimp + 8) * s64 * np.abs(qq).sum()
        m4_64 = a4.astype(F64) * (np.sqrt((qq * qq).sum()) + 1e-37) + rnd
        m6_64 = a6.astype(F64) * (np.sqrt((qq * qq).sum()) + 1e-37) + rnd
        # the fp32 restatement of what the kernel compares
        p, w4 = u42_first(h, s, q)
        up4 = (w4 + u42_bound(s, a4, q, dimp)).astype(F32)
        up6 = (u42_refine(p, l, s, q) + u42_bound(s, a6, q, dimp)).astype(F32)
        fin = cls == 0
        # the documented bounds hold on these inputs (the premise of the selection property)
        assert np.all(np.abs(w4_64[fin] - truth[fin]) <= m4_64[fin]) and np.all(np.abs(w6_64[fin] - truth[fin]) <= m6_64[fin])
        _PASS[d] = dict(rows=rows, q=q, dimp=dimp, cls=cls, truth=truth, w6_64=w6_64, m6_64=m6_64, rnd=rnd, up4=up4, up6=up6,
                        h=H.pack_h(_pad(h, dimp, 8)), lrec=H.pack_l(_pad(l, dimp), a6), sa4=np.stack([s, a4], axis=1).astype(F32))
    return _PASS[d]


def _taus(c):
    """-inf; a value that leaves under 64 survivors in all; a value with about 15 % survivors"""
    fin = c["cls"] == 0
    up4 = np.sort(c["up4"][fin])[::-1]
    return [("all", F32(-np.inf), None), ("few", F32(up4[40]), (30, 63)), ("15 %", F32(up4[int(0.15 * N_PASS)]), (0.13 * N_PASS, 0.17 * N_PASS))]


def _sets(c, t):
    """rows the pass MUST keep (float64 score reaches t, or an infinite element) and MAY keep (float64 w6 + 1.001 m6 + 1e-30
    reaches t)"""
    cls = c["cls"]
    with np.errstate(invalid="ignore"):
        must = (cls == 2) | ((cls == 0) & (c["truth"] >= t))
        may = (cls == 2) | ((cls == 0) & (c["w6_64"] + 1.001 * c["m6_64"] + 1e-30 >= t))
    return must, may


@pytest.mark.parametrize("d", [96, 384])
def test_the_restatement_satisfies_the_selection_property(d):
    """CPU: on the inputs of the GPU test the fp32 restatement keeps every row it must and no row it may not"""
    c = _pass_case(d)
    for name, t, _ in _taus(c):
        must, may = _sets(c, t)
        with np.errstate(invalid="ignore"):
            kept = (c["cls"] != 1) & ~(c["up4"] < t) & ~(c["up6"] < t)
        assert not (must & ~kept).any() and not (kept & ~may).any(), (d, name)


@pytest.mark.gpu
@pytest.mark.parametrize("grid_x", [1, 3])
@pytest.mark.parametrize("d", [96, 384])
def test_full_pass_keeps_what_it_must_and_nothing_it_may_not(d, grid_x):
    c = _pass_case(d)
    cap = N_PASS + 64
    for name, t, surv_range in _taus(c):
        r = H.scan(c["h"], c["sa4"], c["lrec"], c["q"][None, :] if d == c["dimp"] else _pad(c["q"][None, :], c["dimp"]), N_PASS,
                   np.array([t], F32), cap, grid_x)
        assert (r["guard"] == S.SENT_KEY).all()
        count, surv = int(r["count"][0]), int(r["survivors"][0])
        print(f"d={d} grid_x={grid_x} tau {name}: survivors {surv}, candidates {count}")
        keys = r["cand"][0, :count]
        rows = S.key_row(keys).astype(np.int64)
        assert rows.size == np.unique(rows).size and (rows.size == 0 or rows.max() < N_PASS)
        assert (r["cand"][0, count:] == S.SENT_KEY).all()
        must, may = _sets(c, t)
        kept = np.zeros(N_PASS, bool)
        kept[rows] = True
        assert not (must & ~kept).any(), ("SAFETY", name, np.flatnonzero(must & ~kept)[:8])
        assert not (kept & ~may).any(), ("TIGHTNESS", name, np.flatnonzero(kept & ~may)[:8])
        assert surv >= count
        if name == "all":
            assert count == surv == int((c["cls"] != 1).sum())
        else:
            assert surv_range[0] <= surv <= surv_range[1], (name, surv)
        # the keys carry w6 within the rounding term of m6 (+inf for the row with an infinite element)
        w = S.ord2f(S.key_ord(keys)).astype(F64)
        fin = c["cls"][rows] == 0
        assert np.all(np.isposinf(w[~fin]))
        assert np.all(np.abs(w[fin] - c["w6_64"][rows[fin]]) <= c["rnd"][rows[fin]] * (1 + S.M_SLACK) + 1e-45)


@pytest.mark.gpu
def test_full_pass_overflow_counts_on():
    """cap = 256 and tau = -inf: the counter ends at the exact total, the first cap keys are valid, nothing behind them is touched"""
    c = _pass_case(96)
    for grid_x in (1, 3):
        r = H.scan(c["h"], c["sa4"], c["lrec"], c["q"][None, :], N_PASS, np.array([-np.inf], F32), 256, grid_x)
        assert (r["guard"] == S.SENT_KEY).all()
        assert int(r["count"][0]) == int((c["cls"] != 1).sum()) > 256
        rows = S.key_row(r["cand"][0]).astype(np.int64)
        assert rows.size == np.unique(rows).size == 256 and rows.max() < N_PASS and not (c["cls"][rows] == 1).any()
        w = S.ord2f(S.key_ord(r["cand"][0])).astype(F64)
        fin = c["cls"][rows] == 0
        assert np.all(np.abs(w[fin] - c["w6_64"][rows[fin]]) <= c["rnd"][rows[fin]] * (1 + S.M_SLACK) + 1e-45)


@pytest.mark.gpu
def test_one_grid_of_several_queries():
    """grid.y = query: each row of the grid has its own threshold, buffer and counters"""
    c = _pass_case(96)
    taus = [t for _, t, _ in _taus(c)]
    one = [H.scan(c["h"], c["sa4"], c["lrec"], c["q"][None, :], N_PASS, np.array([t], F32), N_PASS, 3) for t in taus]
    r = H.scan(c["h"], c["sa4"], c["lrec"], np.repeat(c["q"][None, :], 3, axis=0), N_PASS, np.array(taus, F32), N_PASS, 3)
    for i in range(3):
        n = int(one[i]["count"][0])
        assert int(r["count"][i]) == n and int(r["survivors"][i]) == int(one[i]["survivors"][0])
        assert np.array_equal(np.sort(r["cand"][i, :n]), np.sort(one[i]["cand"][0, :n]))


@pytest.mark.gpu
def test_pickers_match_their_restatement():
    lib = H.load()
    for units in (0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 24, 25, 128):
        assert lib.u42h_unit_chunk(units) == H.unit_chunk_py(units)
        assert lib.u42h_lpitch(units) == H.lpitch_py(units)
