"""The checkers of the fp32 / bf16 tile tests must be able to fail (CPU): tests/gemm_harness.py's numpy models of the documented
behaviour -- C layout, wave groups, keep rule, cap, pad rows, group bounds, bf16 rounding -- pass the very checker functions
the GPU tests use, and every deliberately wrong model is rejected by them."""
import numpy as np
import pytest

import gemm_harness as G

METRICS = (G.METRIC_COSINE, G.METRIC_L2)
_F32, _U32, _U64 = np.float32, np.uint32, np.uint64
D = 52  # 13 quads: a K tail on both families


def _setup(family, metric, seed=0, ct=2):
    """Five whole tiles and a partial one (one full wave group, one partial), integer corpus, nv below the block."""
    rng = np.random.default_rng(seed)
    T = G.tile_rows(family)
    n, gbn = 5 * T + 64 + 37, 64 * ct
    nv = gbn - 5
    rows, q = G.int_corpus(rng, n, D, nv)
    rows[3] = 0.0
    rows[7] = q[0]
    rows[11, 5] = np.nan
    qb = np.zeros((gbn, D), _F32)
    qb[:nv] = q
    cn = G.sqnorm32(rows)
    covered = 6 * T
    full = np.full((covered, D), 1e30, _F32)  # the pad rows a bf16 tile reads: huge
    full[:n] = rows
    return rng, n, gbn, nv, rows, qb, cn, full


def _scores(full, qb, metric, cn, n, **kw):
    cnf = np.zeros(len(full), _F32)
    cnf[:n] = cn
    with np.errstate(over="ignore", invalid="ignore"):
        return G.ieee_scores(full, qb, metric, cnf, **kw)[0].astype(_F32)


def _dump(S, n, family, gbn, nv, mutant=None, tau=None, cap=None, bound=None, ginf=None):
    cap = n + 3 if cap is None else cap
    cand = np.full(gbn * cap + G.GUARD, G.SENT_KEY, _U64)
    count = np.full(gbn + G.GUARD, G.SENT_U32, _U32)
    count[:gbn] = 0
    if tau is None:
        tau = np.full(gbn, np.inf, _F32)
        tau[:nv] = -np.inf
    return G.model_phase1(S, n, family, 6, 1, 0, tau, cap, cand, count, bound=bound, ginf=ginf, mutant=mutant) + (cap,)


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("metric", METRICS)
def test_the_dump_model_passes_and_wrong_models_are_rejected(family, metric):
    _, n, gbn, nv, rows, qb, cn, full = _setup(family, metric)
    S = _scores(full, qb, metric, cn, n)
    cand, count, cap = _dump(S, n, family, gbn, nv)
    assert G.check_dump(cand, count, gbn, cap, n, nv, exact=S) == 0.0
    # float form of the same check: value = the scores, a band of zero
    G.check_dump(cand, count, gbn, cap, n, nv, value=S.astype(np.float64), band=np.zeros(S.shape))
    # a dropped K-tail quad
    bad = _scores(full, qb, metric, cn, n, drop_last_quad=True)
    cand, count, cap = _dump(bad, n, family, gbn, nv)
    with pytest.raises(AssertionError):
        G.check_dump(cand, count, gbn, cap, n, nv, exact=S)
    # a row off by the 4 (lane >> 5) term; a pad row let through
    for mutant in ("no_lane_half", "pad_row"):
        cand, count, cap = _dump(S, n, family, gbn, nv, mutant=mutant)
        with pytest.raises(AssertionError):
            G.check_dump(cand, count, gbn, cap, n, nv, exact=S)
    # a padded column that counts, a write into the guard, a NaN row let through
    cand, count, cap = _dump(S, n, family, gbn, nv)
    count[nv] = 1
    with pytest.raises(AssertionError):
        G.check_dump(cand, count, gbn, cap, n, nv, exact=S)
    cand, count, cap = _dump(S, n, family, gbn, nv)
    cand[gbn * cap + 1] = 0
    with pytest.raises(AssertionError):
        G.check_dump(cand, count, gbn, cap, n, nv, exact=S)
    cand, count, cap = _dump(np.where(np.isnan(S), _F32(0), S), n, family, gbn, nv)
    with pytest.raises(AssertionError):
        G.check_dump(cand, count, gbn, cap, n, nv, exact=S)
    # live = 1 with tau = -inf in every column (a single-query pass sees the other queries' thresholds): only the gate keeps
    # the idle columns silent, whether their queries are zero or not
    blank_c, blank_n = np.full(gbn * cap + G.GUARD, G.SENT_KEY, _U64), np.concatenate([np.zeros(gbn, _U32), np.full(G.GUARD, G.SENT_U32, _U32)])
    low = np.full(gbn, -np.inf, _F32)
    for Sq in (S, np.where(np.arange(gbn) == 0, S, _F32(0.0)).astype(_F32)):
        G.check_dump(*G.model_phase1(Sq, n, family, 6, 1, 1, low, cap, blank_c, blank_n), gbn, cap, n, 1, exact=S)
        with pytest.raises(AssertionError):
            G.check_dump(*G.model_phase1(Sq, n, family, 6, 1, 1, low, cap, blank_c, blank_n, mutant="no_live_gate"), gbn, cap, n, 1, exact=S)


def _want(S, n, tau, gbn, bound=None):
    R = np.arange(n)
    out = []
    for q in range(gbn):
        with np.errstate(invalid="ignore"):
            cut = _F32(tau[q]) if bound is None else (_F32(tau[q]) - bound[R >> 6, q]).astype(_F32)
            keep = S[:n, q] >= cut
        out.append(G.make_keys(G.f2ord(S[:n, q][keep] + _F32(0.0)), R[keep]))
    return out


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("metric", METRICS)
def test_the_keep_model_passes_and_wrong_models_are_rejected(family, metric):
    _, n, gbn, nv, rows, qb, cn, full = _setup(family, metric, 1)
    S = _scores(full, qb, metric, cn, n)
    tau = np.full(gbn, np.inf, _F32)
    for q in range(nv):  # ON a row's score: the 30th best, full of ties on integers
        tau[q] = np.sort(S[:n, q][~np.isnan(S[:n, q])])[-30]
    want = _want(S, n, tau, gbn)
    assert all(w.size >= 30 for w in want[:nv]) and all(w.size == 0 for w in want[nv:])
    for cap in (n, 7):
        cand, count, _ = _dump(S, n, family, gbn, nv, tau=tau, cap=cap)
        G.check_keep(cand, count, gbn, cap, want)
    # > for >= at the threshold; a pad row let through (tau below the pad rows' huge scores); a write at pos >= cap
    cand, count, _ = _dump(S, n, family, gbn, nv, tau=tau, cap=n, mutant="gt_for_ge")
    with pytest.raises(AssertionError):
        G.check_keep(cand, count, gbn, n, want)
    if family != G.FP32 and metric == G.METRIC_COSINE:
        assert (S[n:, :nv] > tau[:nv]).any()
        cand, count, _ = _dump(S, n, family, gbn, nv, tau=tau, cap=n, mutant="pad_row")
        with pytest.raises(AssertionError):
            G.check_keep(cand, count, gbn, n, want)
    cand, count, _ = _dump(S, n, family, gbn, nv, tau=tau, cap=7, mutant="past_cap")
    with pytest.raises(AssertionError):
        G.check_keep(cand, count, gbn, 7, want)
    # a count clamped to cap
    cand, count, _ = _dump(S, n, family, gbn, nv, tau=tau, cap=7)
    count[:gbn] = np.minimum(count[:gbn], 7)
    with pytest.raises(AssertionError):
        G.check_keep(cand, count, gbn, 7, want)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_the_phase0_model_passes_and_wrong_models_are_rejected(family):
    metric = G.METRIC_COSINE
    _, n, gbn, nv, rows, qb, cn, full = _setup(family, metric, 2)
    S = _scores(full, qb, metric, cn, n)
    RW = G.wave_groups(family)
    blank = np.full(gbn * RW * 6 + G.GUARD, G.SENT_KEY, _U64)
    got = G.model_phase0(S, n, family, 6, 1, 0, blank)
    # an independent statement of the same: the maximum of each 64-row group's scores below n_rows
    hm = got[:gbn * RW * 6].reshape(gbn, RW * 6)
    for ht in range(RW * 6):
        lo, hi = ht * 64, min(ht * 64 + 64, n)
        for q in (0, nv - 1, nv):
            if lo >= n:
                assert hm[q, ht] == 0
                continue
            m = np.nanmax(S[lo:hi, q])
            assert hm[q, ht] == G.make_keys(G.f2ord(_F32(m) + _F32(0.0)), [ht])[0]
    assert (hm[:, (n + 63) // 64:] == 0).all()
    assert family == G.FP32 or (n + 63) // 64 < RW * 6  # the 256-row tiles: wave groups wholly past the end
    G.check_halfmax(got, got)
    for mutant in ("no_lane_half", "pad_row"):
        with pytest.raises(AssertionError):
            G.check_halfmax(G.model_phase0(S, n, family, 6, 1, 0, blank, mutant=mutant), got)
    # live = 1: the other columns keep what they held
    one = G.model_phase0(S, n, family, 6, 1, 1, blank)
    assert (one[RW * 6:] == _U64(G.SENT_KEY)).all() and np.array_equal(one[:RW * 6], got[:RW * 6])
    with pytest.raises(AssertionError):
        G.check_halfmax(got, one)
    # tile_stride 2: tile t starts at row 2 t T
    two = G.model_phase0(S, n, family, 3, 2, 0, np.full(gbn * RW * 3 + G.GUARD, G.SENT_KEY, _U64))
    h2 = two[:gbn * RW * 3].reshape(gbn, RW * 3)
    assert np.array_equal(G.key_ord(h2[:, RW:2 * RW]), G.key_ord(hm[:, 2 * RW:3 * RW]))


@pytest.mark.parametrize("metric", METRICS)
def test_the_bound_model_and_its_checker(metric):
    family = G.BF16
    rng, n, gbn, nv, rows, qb, cn, full = _setup(family, metric, 3)
    rows = (rows * rng.uniform(0.5, 2.0, rows.shape)).astype(_F32)
    rows[64:128] *= 100.0  # one group 100 x the rest
    rows[11, 5] = 1.0
    cn = G.sqnorm32(rows)
    q = (qb[:nv] * rng.uniform(0.5, 2.0, (nv, D))).astype(_F32)
    truth, _ = G.ieee_scores(rows, q, metric, cn)
    # what the bf16 tiles compute, up to fp32 summation: the products of the rounded operands
    v, _ = G.ieee_scores(G.bf16_to_f32(G.to_bf16_sel(rows)), G.bf16_to_f32(G.to_bf16_sel(q)), metric, cn)
    eps, gam, fl = G.lib_sel(D, True)
    gmax, qn = G.group_max(cn, n), G.query_norm_mirror(q, nv, nv)
    b = G.group_bound(gmax, qn, eps, gam, fl, metric)
    bc = G.group_bound(gmax, qn, eps, gam, fl, metric, contract=True)
    assert np.abs(b.astype(np.float64) - bc).max() <= 2.0 ** -22 * np.abs(b).max()
    R = np.arange(n) >> 6
    ratio = G.check_bounds(v, np.minimum(b, bc)[R], truth)
    assert 0 < ratio <= 1
    with pytest.raises(AssertionError):  # a bound that is too small
        G.check_bounds(v, G.group_bound(gmax, qn, eps * _F32(ratio * 0.4), gam * _F32(0.1), fl, metric)[R], truth)
    # the float32 mirror is independent of contraction when eps, gam, floor_abs are powers of two
    p = (2.0 ** -7, 2.0 ** -18, 2.0 ** -10)
    assert np.array_equal(G.group_bound(gmax, qn, *p, metric), G.group_bound(gmax, qn, *p, metric, contract=True))
    # the absolute underflow term: added once to every bound, the same bits in both forms
    bu = G.group_bound(gmax, qn, *p, metric, under_abs=2.0 ** -6)
    assert np.array_equal(bu, G.group_bound(gmax, qn, *p, metric, contract=True, under_abs=2.0 ** -6))
    two = 2.0 if metric == G.METRIC_L2 else 1.0
    assert (bu > G.group_bound(gmax, qn, *p, metric)).all() and np.abs(bu - G.group_bound(gmax, qn, *p, metric) - two * 2.0 ** -6).max() < 1e-3
    assert float(G.lib_under(64)) == 82 * 2.0 ** -149
    # PHASE 1 with the bound: exactly score >= tau - bound; a halved bound is rejected
    S = np.zeros((6 * 256, nv + 5), _F32)
    S[:n, :nv] = v.astype(_F32)
    bb = np.zeros((len(gmax), nv + 5), _F32)
    bb[:, :nv] = G.group_bound(gmax, qn, *p, metric)
    tau = np.full(nv + 5, np.inf, _F32)
    tau[:nv] = np.sort(S[:n, :nv], axis=0)[-20]
    want = _want(S, n, tau, gbn, bb)
    cand, count, _ = _dump(S, n, family, gbn, nv, tau=tau, cap=n, bound=bb)
    G.check_keep(cand, count, gbn, n, want)
    half = G.group_bound(gmax, qn, *p, metric, mutant="bound_halved")
    bb2 = np.zeros_like(bb)
    bb2[:, :nv] = half
    cand, count, _ = _dump(S, n, family, gbn, nv, tau=tau, cap=n, bound=bb2)
    with pytest.raises(AssertionError):
        G.check_keep(cand, count, gbn, n, want)
    # a group with an infinite gmax: all its rows, +inf keys, finite thresholds only
    ginf = np.zeros(len(gmax), bool)
    ginf[2] = True
    cand, count, _ = _dump(S, n, family, gbn, nv, tau=tau, cap=n, bound=bb, ginf=ginf)
    c, cnt = G.check_guards(cand, count, gbn, n)
    for qq in (0, nv - 1):
        have = c[qq, :cnt[qq]]
        inf = have[G.key_ord(have) == G.f2ord(G.INF32)[0]]
        assert np.array_equal(np.sort(G.key_row(inf)), np.arange(128, 192))
    assert (cnt[nv:] == 0).all()


def test_dump_values_and_the_directed_roundings():
    _, n, gbn, nv, rows, qb, cn, full = _setup(G.FP32, G.METRIC_COSINE, 6)
    S = _scores(full, qb, G.METRIC_COSINE, cn, n)
    cand, count, cap = _dump(S, n, G.FP32, gbn, nv)
    v = G.dump_values(cand, count, gbn, cap, n, nv)
    assert np.array_equal(np.isnan(v), np.isnan(S[:n, :nv])) and np.array_equal(np.nan_to_num(v), np.nan_to_num(S[:n, :nv].astype(np.float64)))
    x = np.array([1.0, 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0 - 2.0 ** -30, 2.0 ** -149, 2.0 ** -151, 0.0])
    assert G.f32_down(x).tolist() == [1.0, 1.0, 1.0 - 2.0 ** -24, -1.0 - 2.0 ** -23, 2.0 ** -149, 0.0, 0.0]
    assert G.f32_up(x).tolist() == [1.0, 1.0 + 2.0 ** -23, 1.0, -1.0, 2.0 ** -149, 2.0 ** -149, 0.0]


def test_fmaf_rounds_once():
    rng = np.random.default_rng(4)
    a, b, c = (rng.standard_normal(20000).astype(_F32) for _ in range(3))
    from fractions import Fraction

    got = G.fmaf(a, b, c)
    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], _F32(-np.inf)), np.nextafter(got[i], _F32(np.inf))
        assert abs(exact - Fraction(float(got[i]))) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi))))
    # 1 + 2^-60 rounds to 1
    one = G.fmaf(np.array([2.0 ** -30], _F32), np.array([2.0 ** -30], _F32), np.array([1.0], _F32))
    assert one[0] == _F32(1.0)
    up = G.fmaf(np.array([1.0 + 2.0 ** -23], _F32), np.array([2.0 ** -24 * (1 + 2.0 ** -20)], _F32), np.array([1.0], _F32))
    # (1 + 2^-23) 2^-24 (1 + 2^-20) + 1 = 1 + 2^-24 + (a little): above the tie -> 1 + 2^-23
    assert up[0] == _F32(1.0 + 2.0 ** -23)


def test_the_bf16_model_and_its_checker():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, (1 + 2.0 ** -8) * (1 - 2.0 ** -20), 1.0 + 2.0 ** -8 + 2.0 ** -20,
                  3.39e38, 3.4028235e38, -3.4e38, np.inf, -np.inf, np.nan, -0.0, 1e-40, -1e-45, 3.3895313892515355e38], _F32)
    bits = G.to_bf16_sel(x)
    back = G.bf16_to_f32(bits)
    assert back[0] == 1.0 and back[1] == 1.0 and back[2] == _F32(1.0 + 2.0 ** -6)  # ties to even, both ways
    assert back[3] == 1.0 and back[4] == _F32(1.0 + 2.0 ** -7)
    assert back[5] == G.BF16_MAX and back[6] == G.BF16_MAX and back[7] == -G.BF16_MAX and back[14] == G.BF16_MAX  # the clamp
    assert back[8] == np.inf and back[9] == -np.inf and np.isnan(back[10])
    assert bits[11] == 0x8000 and np.signbit(back[13])
    fin = np.isfinite(x) & (np.abs(x) > 1e-37)
    assert (np.abs(back[fin].astype(np.float64) - x[fin]) <= 2.0 ** -8 * np.abs(x[fin].astype(np.float64))).all()
    G.check_bf16(bits, bits)
    with pytest.raises(AssertionError):  # truncation for round-to-nearest-even
        G.check_bf16(G.to_bf16_sel(x, "truncate"), bits)
    with pytest.raises(AssertionError):  # a +inf from a clamped finite value
        G.check_bf16(G.to_bf16_sel(x, "no_clamp"), bits)
    assert np.isinf(G.bf16_to_f32(G.to_bf16_sel(x, "no_clamp"))[6])
    lost = bits.copy()
    lost[10] = 0x7F80
    with pytest.raises(AssertionError):  # a NaN that became an infinity
        G.check_bf16(lost, bits)
    # the conversions' layouts
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((10, 12)).astype(_F32)
    out = np.full((12, 16), G.SENT_U16, np.uint16)
    m = G.rows_to_bf16_model(rows, 3, 10, 16, out)
    assert (m[:3] == G.SENT_U16).all() and (m[10:] == G.SENT_U16).all() and (m[3:10, 12:] == 0).all()
    assert np.array_equal(m[3:10, :12], G.to_bf16_sel(rows[3:10]))
    q = rng.standard_normal((3, 12)).astype(_F32)
    one = G.queries_to_bf16_model(q, 3, 64, 128, 128, 1)
    assert np.array_equal(one[0, :3, :12], G.to_bf16_sel(q)) and not one[0, 3:].any() and not one[0, :, 12:].any()
    per = G.queries_to_bf16_model(q, 3, 64, 128, 1, 3)
    assert all(np.array_equal(per[b, 0, :12], G.to_bf16_sel(q[b])) and not per[b, 1:].any() for b in range(3))


def test_the_layout_and_the_picker_restatements():
    # every row of a 64-row wave group exactly once
    R = G.walk_rows(G.BF16, 2, 1)
    assert np.array_equal(np.sort(R.ravel()), np.arange(512)) and R.shape == (2, 4, 2, 2, 16)
    assert np.array_equal(np.sort(G.walk_rows(G.FP32, 3, 2)[1].ravel()), np.arange(256, 384))
    # a register group: the lane half's 16 rows of a 32-row block
    assert sorted(R[0, 0, 0, 1]) == [4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23, 28, 29, 30, 31]
    for row in (0, 5, 31, 77, 200):
        blk, lh, pos = G.register_group_of(row)
        t, rem = divmod(blk, 256)
        assert R[t, rem // 64, (rem % 64) // 32, lh, pos] == row
    count = 0
    for family in G.FAMILIES:
        for ct in (1, 2, 4):
            for metric in METRICS:
                for groupb in (0, 1):
                    count += (1 if family == G.SHADOW else 2) * G.has_instance_py(family, ct, metric, groupb)  # (no K tail on the shadow)
    assert count == 41  # 18 fp32 + 16 bf16 + 7 shadow
    assert G.ktail_py(G.FP32, 13) and not G.ktail_py(G.FP32, 16) and G.ktail_py(G.BF16, 8) and not G.ktail_py(G.SHADOW, 16)
    assert G.kchunks_bf16(8) == 2 and G.kchunks_bf16(5) == 2 and G.kchunks_bf16(21) == 4 and G.kchunks_bf16(32) == 4
    assert G.qb_pitch16_py(G.BF16, 32) == 8 and G.qb_pitch16_py(G.SHADOW, 100) == 16 and G.qb_pitch16_py(G.SHADOW, 200) == 32
    assert float(G.lib_gamma(64)) == pytest.approx(1.02 * 82 * 2.0 ** -24, rel=1e-5)
