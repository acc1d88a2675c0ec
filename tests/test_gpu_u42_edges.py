"""The edges of scan_u42_kernel's walk over tiles and chunks on the MI355X (kernels_scan42.h), launched by
tests/kernel_harness/u42_harness.hip.

The shapes are the smallest at which the walk can go wrong:
  d = 32 (1 unit: one short chunk per tile), 160 (5 units: a chunk of 6 with one unit missing), 416 (13 units = 8 + 5);
  n = 1, 64, 65 and 64 * 4 * grid_x + 1 (one wave owns two tiles, the others one or none), grid_x = 1 and 2;
  130 rows against -inf: every row survives, the waves' lists refine at 64, 64 and 2;
  a query of magnitude 1e-36: every partial sum of the scaled products is an fp32 subnormal (the kernel keeps denormals).
Each launch is held against the float64 sets of tests/test_gpu_u42_kernels.py: must-keep <= kept <= may-keep, survivors >=
candidates, nothing written behind a buffer."""
import numpy as np
import pytest

import select_harness as S
import u42_harness as H
from test_selection_bounds_u42 import dimp_of, quantise_u42, u42_bound, u42_first

F32, F64 = np.float32, np.float64
_CASES = {}


def _case(n, d, qscale=1.0):
    """n unit rows of d elements (one of vanishing magnitude from 64 rows on), planes packed from the restatement, one query,
    float64 truth and the float64 form of the refine -- computed once per shape and shared, never modified"""
    if (n, d, qscale) not in _CASES:
        rng = np.random.default_rng(7919 * d + n)
        rows = rng.standard_normal((n, d))
        rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(F32)
        if n >= 64:
            rows[37] *= F32(1e-33)
        q = rng.standard_normal(d)
        q = (q / np.linalg.norm(q) * qscale).astype(F32)
        dimp = dimp_of(d)
        h, l, s, a4, a6 = quantise_u42(rows)
        cls = S.row_class(rows)
        assert (cls == 0).all()
        qq, s64 = q.astype(F64), s.astype(F64)
        truth = S.scores64(rows, q)
        p64 = h.astype(F64) @ qq
        w6_64 = s64 * (4.0 * p64 + l.astype(F64) @ qq - 32.0 * qq.sum())
        rnd = 6e-6 * (dimp + 8) * s64 * np.abs(qq).sum()
        m6_64 = a6.astype(F64) * (np.sqrt((qq * qq).sum()) + 1e-37) + rnd
        assert np.all(np.abs(w6_64 - truth) <= m6_64)  # (the premise of the selection property)
        _, w4 = u42_first(h, s, q)
        up4 = (w4 + u42_bound(s, a4, q, dimp)).astype(F32)

        def pad(x, value=0):
            out = np.full((n, dimp), value, x.dtype)
            out[:, :d] = x
            return out

        qp = np.zeros((1, dimp), F32)
        qp[0, :d] = q
        _CASES[(n, d, qscale)] = dict(q=qp, truth=truth, w6_64=w6_64, m6_64=m6_64, rnd=rnd, up4=up4, h=H.pack_h(pad(h, 8)),
                              lrec=H.pack_l(pad(l), a6), sa4=np.stack([s, a4], axis=1).astype(F32))
    return _CASES[(n, d, qscale)]


def _check(c, n, t, grid_x):
    """one launch against the float64 sets; -> (survivors, candidates)"""
    cap = n + 64
    r = H.scan(c["h"], c["sa4"], c["lrec"], c["q"], n, np.array([t], F32), cap, grid_x)
    assert (r["guard"] == S.SENT_KEY).all()
    count, surv = int(r["count"][0]), int(r["survivors"][0])
    keys = r["cand"][0, :count]
    rows = S.key_row(keys).astype(np.int64)
    assert rows.size == np.unique(rows).size and (rows.size == 0 or rows.max() < n)
    assert (r["cand"][0, count:] == S.SENT_KEY).all()
    must = c["truth"] >= t
    may = c["w6_64"] + 1.001 * c["m6_64"] + 1e-30 >= t
    kept = np.zeros(n, bool)
    kept[rows] = True
    assert not (must & ~kept).any(), ("SAFETY", np.flatnonzero(must & ~kept)[:8])
    assert not (kept & ~may).any(), ("TIGHTNESS", np.flatnonzero(kept & ~may)[:8])
    assert surv >= count
    w = S.ord2f(S.key_ord(keys)).astype(F64)
    assert np.all(np.abs(w - c["w6_64"][rows]) <= c["rnd"][rows] * (1 + S.M_SLACK) + 1e-45)
    return surv, count


@pytest.mark.gpu
@pytest.mark.parametrize("grid_x", [1, 2])
@pytest.mark.parametrize("d", [32, 160, 416])
def test_full_pass_at_the_edges_of_tiles_and_chunks(d, grid_x):
    for n in (1, 64, 65, 64 * 4 * grid_x + 1):
        c = _case(n, d)
        up4 = np.sort(c["up4"])
        # every row; about half of them by the four-bit bound; none
        for name, t in (("all", F32(-np.inf)), ("half", up4[n // 2]), ("none", F32(np.inf))):
            surv, count = _check(c, n, t, grid_x)
            print(f"d={d} grid_x={grid_x} n={n} tau {name}: survivors {surv}, candidates {count}")
            if name == "all":
                assert surv == count == n
            elif name == "none":
                assert surv == count == 0


@pytest.mark.gpu
@pytest.mark.parametrize("d", [160, 416])
def test_every_row_survives_three_tiles_of_one_workgroup(d):
    """130 rows, one workgroup: the waves' lists fill to 64, 64 and 2 -- two refine inside the tile loop, one behind it"""
    n = 130
    surv, count = _check(_case(n, d), n, F32(-np.inf), 1)
    assert surv == count == n


@pytest.mark.gpu
@pytest.mark.parametrize("d", [160, 416])
def test_a_query_whose_partial_sums_are_all_subnormal(d):
    """|q|_2 = 1e-36: the products h_i 2^-9 q_i are below 2^-126, so every fma of the pass and of the refine rounds in the
    subnormal range -- the case the rounding term's dimp 2^-138 is for, and it needs the kernel to keep fp32 denormals.
    Against -inf every row comes back with its w6, which must lie within the rounding term of the float64 value; a pass
    that flushed would carry P = Q = 0 and miss it by orders of magnitude.  (Finite thresholds are left out: the squares
    of such a query underflow in u6_query_sums, which is the u6 scan's own limit and not this kernel's.)"""
    n = 257
    c = _case(n, d, 1e-36)
    assert np.abs(c["q"]).max() * 15 * 2.0 ** -9 < 2.0 ** -126
    # the check below can tell: without P and Q the keys would be off by far more than the allowance
    assert np.median(np.abs(c["w6_64"] + c["sa4"][:, 0].astype(F64) * 32.0 * c["q"].astype(F64).sum())) > 100 * c["rnd"].max()
    surv, count = _check(c, n, F32(-np.inf), 1)
    assert surv == count == n
