"""The selection test of the batched range search (kernels_range_batch.h), restated in numpy / float64
after tests/test_selection_bounds.py: rows and queries are quantised as the kernels do, the thresholds and the widened bound
are what the library hands to gemm_i8_kernel<PHASE 1>, and EVERY row the exact pass could accept must pass the tile test:

  cosine / inner product   a row is covered when its fp32 score, emulated in exact_score's summation order (kernels_aux.h: fmas
                           per lane and component, (x + y) + (z + w), six butterfly adds), reaches t -- or when its float64
                           score plus the documented term gamma |c|_2 |q|_2 (gamma = 2e-6) does;
  L2                       ... when its emulated fp32 squared distance is <= t, or its float64 distance is <= t (1 + 2e-6)
                           (the relative error range_selection_tau_l2 documents for that sum).

Rows: unit rows, unnormalised rows with norms 1e-3 .. 1e3 inside one 64-row group, a row with an outlier element, rows near
the query, and copies of one row scaled by 1 + j 2^-23 (j = -3 .. 3), whose scores sit within a few ulps of a threshold taken
from the middle copy, on both sides.  No case is left out: every (dimension, metric, query, threshold) asserts."""
import numpy as np
import pytest

from test_selection_bounds import _fma32, quantise_i8_groups, quantise_i8_query

f32 = np.float32
GAMMA = f32(2e-6)  # kernels_range_batch.h::RANGE_BATCH_GAMMA


def exact_score(rows, q, l2):
    """kernels_aux.h::exact_score for every row at once: lane j of 64 owns the quads j, j + 64, ...; float32 throughout."""
    n, d = rows.shape
    quads = -(-d // 4)
    iters = -(-quads // 64)
    c = np.zeros((n, iters * 64 * 4), f32)
    c[:, :d] = rows
    qq = np.zeros(iters * 64 * 4, f32)
    qq[:d] = q
    c = c.reshape(n, iters, 64, 4)
    qq = qq.reshape(iters, 64, 4)
    acc = np.zeros((n, 64, 4), f32)
    for it in range(iters):
        if l2:
            diff = (c[:, it] - qq[it]).astype(f32)
            acc = _fma32(diff, diff, acc)
        else:
            acc = _fma32(c[:, it], qq[it], acc)
    s = ((acc[:, :, 0] + acc[:, :, 1]).astype(f32) + (acc[:, :, 2] + acc[:, :, 3]).astype(f32)).astype(f32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, lanes ^ o]).astype(f32)
    return s[:, 0]  # (L2: the positive squared distance; the kernel negates it)


def selection_tau_l2(qq, t):
    """host_range.h::range_selection_tau_l2"""
    if np.isinf(t):
        return f32(-np.inf) if t > 0 else f32(np.inf)
    tau = float(qq) - float(t) - 1e-5 * abs(float(t))
    f = f32(tau)
    if float(f) > tau:
        f = np.nextafter(f, f32(-np.inf))
    return f


def tile_keeps(D, s_g, a_g, b_g, cn, s_q, E, M, tau, l2):
    """range_batch_bound_kernel, then gemm_i8_kernel<PHASE 1>'s fp32 chain (the exact epilogue; the prefilter in front of it is
    never stricter: tests/test_selection_bounds.py).  True = the pair is appended."""
    G = f32(GAMMA * f32(M) * f32(1.000001))
    up = f32(1.0) + f32(1.1920929e-7)  # (the kernel takes both sums one ulp up)
    E = f32(f32(f32(E) + f32(G * f32(1.000001))) * up)
    M = f32(f32(f32(M) + f32(G * f32(1.000001))) * up)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        tau = f32(min(f32(tau), f32(1e38) * (f32(s_q) if s_q > 0 else f32(1.0))))
        if l2:
            tau = f32(f32(0.5) * tau)
        if not tau < np.inf:
            return np.zeros(len(D), bool)  # a padded query: never a pair
        w = f32(1.0) / f32(s_q) if s_q > 0 else f32(1.0)
        A = f32(tau * w)
        A1 = f32(A - f32(2e-6) * np.abs(A))
        E1, M1 = f32(f32(E * w) * f32(1.000003)), f32(f32(M * w) * f32(1.000003))
        inv = (f32(1.0) / s_g.astype(f32)).astype(f32)
        inv = np.where(np.isfinite(inv), inv, f32(2.0 ** 60))
        T = _fma32(-(b_g.astype(f32) * inv).astype(f32), M1, _fma32(-(a_g.astype(f32) * inv).astype(f32), E1, _fma32(inv, A1, f32(-1.0))))
        Df = D.astype(f32)
        if l2:
            u = (f32(0.5) * cn * f32(0.9999) * inv).astype(f32)
            f = (_fma32(-u, f32(w * f32(0.999997)), Df) + f32(2e-6) * np.abs(Df)).astype(f32)
            return ~(f < T)
        return ~(Df < T)


def corpus(rng, d, q):
    n = 320
    rows = rng.standard_normal((n, d))
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    # one 64-row group (and a half) of unnormalised rows: norms 1e-3 .. 1e3 next to each other
    norms = np.logspace(-3, 3, 96)
    rng.shuffle(norms)
    rows[96:192] *= norms[:, None]
    # an outlier element: the group's scale is that element's, every other row of the group quantises coarsely
    rows[200, 5 % d] = 40.0
    # rows near the query (high scores), some of them unnormalised
    qn = q / np.linalg.norm(q)
    rows[256:320] = qn + 0.05 * rng.standard_normal((64, d))
    rows[300:320] *= np.logspace(-3, 3, 20)[:, None]
    rows = rows.astype(f32)
    # copies of one row a few ulps apart: their scores straddle a threshold taken from the middle copy
    for base, at in ((270, 240), (120, 20)):
        for j in range(-3, 4):
            rows[at + 3 + j] = (rows[base] * f32(1.0 + j * 2.0 ** -23)).astype(f32)
    return rows


QUERIES = ("unit", "long", "short", "one_hot")


def query(rng, d, kind):
    q = rng.standard_normal(d)
    q /= np.linalg.norm(q)
    if kind == "long":
        q *= 37.5
    elif kind == "short":
        q *= 3e-3
    elif kind == "one_hot":
        q = np.zeros(d)
        q[d // 3] = 1.0
    return q.astype(f32)


@pytest.mark.parametrize("l2", [False, True], ids=["cosine", "l2"])
@pytest.mark.parametrize("d", [54, 100, 384, 768, 4096])
def test_every_row_the_exact_pass_accepts_passes_the_widened_tile_test(d, l2):
    rng = np.random.default_rng(1300 + d + (7 if l2 else 0))
    for kind in QUERIES:
        q = query(rng, d, kind)
        rows = corpus(rng, d, q)
        n = len(rows)
        m, s_q, E, M = quantise_i8_query(q)
        nr, s_g, a_g, b_g = quantise_i8_groups(rows)
        D = nr.astype(np.int64) @ m.astype(np.int64)
        cn = (rows ** 2).sum(axis=1, dtype=f32)  # row_sqnorm_kernel
        s32 = exact_score(rows, q, l2)
        r64, q64 = rows.astype(np.float64), q.astype(np.float64)
        qq = float(q64 @ q64)
        if l2:
            s64 = ((r64 - q64) ** 2).sum(axis=1)
            # the relative error the L2 threshold documents covers the emulated sum (else the emulation, or the claim, is off)
            assert np.all(np.abs(s32.astype(np.float64) - s64) <= 2e-6 * s64), (d, kind)
        else:
            s64 = r64 @ q64
            gterm = float(GAMMA) * np.linalg.norm(r64, axis=1) * np.sqrt(qq)
            # the documented gamma bounds the emulated sum's error
            assert np.all(np.abs(s32.astype(np.float64) - s64) <= gterm), (d, kind)
        order = np.sort(s32)
        best, worst = (order[0], order[-1]) if l2 else (order[-1], order[0])
        step_out = f32(-np.inf) if l2 else f32(np.inf)  # one ulp beyond the best score: nothing is covered
        thresholds = [s32[243], s32[23], np.nextafter(s32[243], step_out), np.nextafter(s32[243], -step_out), best,
                      np.nextafter(best, step_out), order[n // 2], order[n // 4], order[3 * n // 4], worst, f32(0.0),
                      f32(np.inf), f32(-np.inf), f32(3e38), f32(-3e38)]
        for t in thresholds:
            t = f32(t)
            if l2:
                covered = (s32 <= t) | (s64 <= float(t) * (1 + 2e-6))
                tau = selection_tau_l2(qq, t)
            else:
                with np.errstate(invalid="ignore"):
                    covered = (s32 >= t) | (s64 + gterm >= float(t))
                tau = t
            kept = tile_keeps(D, s_g, a_g, b_g, cn, s_q, E, M, tau, l2)
            missed = np.flatnonzero(covered & ~kept)
            assert missed.size == 0, (d, "l2" if l2 else "cosine", kind, float(t), missed[:8].tolist(),
                                      s32[missed[:8]].tolist())
        # the straddling copies really sit within a few ulps of their threshold, on both sides: ulps of the score for the row
        # near the query, of |c| |q| for the row whose products cancel (and of the distance for L2)
        for mid in (243, 23):
            near = s32[mid - 3:mid + 4]
            scale = np.abs(s32[mid]) if (l2 or mid == 243) else f32(np.linalg.norm(r64[mid]) * np.sqrt(qq))
            assert np.all(np.abs(near - s32[mid]) <= 16 * np.spacing(f32(scale))), (d, kind, mid)
            if mid == 243 and not l2:
                assert near.min() < s32[mid] < near.max(), (d, kind)


def test_the_widened_bound_still_selects():
    """unit rows, unit query: a threshold at the 10th best score keeps a small part of the corpus, not all of it"""
    rng = np.random.default_rng(5)
    d, n = 384, 4096
    q = query(rng, d, "unit")
    rows = rng.standard_normal((n, d))
    rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(f32)
    m, s_q, E, M = quantise_i8_query(q)
    nr, s_g, a_g, b_g = quantise_i8_groups(rows)
    D = nr.astype(np.int64) @ m.astype(np.int64)
    s32 = exact_score(rows, q, False)
    t = np.sort(s32)[-10]
    kept = tile_keeps(D, s_g, a_g, b_g, None, s_q, E, M, t, False)
    assert np.all(kept[s32 >= t]) and 10 <= kept.sum() < n // 8
