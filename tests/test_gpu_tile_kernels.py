"""The int8 tile kernel by itself: gemm_i8_kernel (kernels_tiles8.h) in both phases, gbad_with_mask_kernel and
group_ref_kernel, launched by tests/kernel_harness/tile_harness.hip on bytes, tables and thresholds built here.

A selection kernel fails silently: behind the tiles sit the exact re-score and the repair scan, and on
random vectors the k-th score is well separated, so a wrong swizzle for one parity of pitch8 / 128, a row index off by a
fragment half, a slack of the wrong sign or a bad-row bit read from the wrong half of its word lose one row on one query in
a million.  Here every integer dot product is compared bit for bit with the int64 product of the very bytes uploaded, and
the thresholds sit on the rows' own upper bounds.

Shapes: 5 tiles of 256 rows, n_rows = 5 * 256 - 37 (the last 32-row block and the last group are partial; the rows behind the
end hold random bytes, not zeros); grids 1, 2 and 5 (a workgroup walks several tiles, the ring crosses tile boundaries, the
loader re-reads its last tile); pitch8 128 .. 1536 (run-time rings 2, 4, 6, both compile-time pitches, both parities of
pitch8 / 128); every query block that fits, full and with 5 padded queries.  The quantisers clamp to [-127, 127]
(rows_to_i8g_kernel, queries_to_i8_kernel), so -128 is on neither side.

The tolerances are derived in tests/tile_harness.py's docstring from the constants the kernel documents.  Tightness has no
statement where the slack is not finite (a group with a_g = +inf, a query with E = +inf): with the special tables below these
are 1 group of 20 and 1 query in 59 or more, under 8 % of the entries (asserted on the CPU); safety is checked on all of them.

The CPU half (no marker) feeds the same checkers the numpy restatement (accepted on every family) and six deliberately
wrong restatements (each rejected)."""
import zlib
from functools import lru_cache

import numpy as np
import pytest

import tile_harness as T
from tile_harness import COS, L2, Tile

I8, U32, U64, F32, F64 = np.int8, np.uint32, np.uint64, np.float32, np.float64
TILES = 5
N_ROWS = TILES * 256 - 37
N_ALLOC = TILES * 256
N_GROUPS = N_ALLOC // 64 + 2  # (two pad groups behind, as the library's table has)
SPECIAL_SHARE = 0.08


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


# --------------------------------------------------------------------------- #
# inputs (built once per pitch, never changed)
# --------------------------------------------------------------------------- #
@lru_cache(maxsize=None)
def _bytes(pitch8):
    """rows [1280, pitch8], queries [256, pitch8] int8 and their int64 dot products.  Random bytes in [-127, 127]; every 8th row
    and query a pattern whose value depends on (row, column), so that any permutation of fragments, pieces or rows changes D;
    full-scale rows / queries of +127 and -127; zero rows (group 5 whole: the all-zero group of the special tables) and zero
    queries (3 and 6: the zero query and the E = +inf query; 9: zero bytes under ordinary parameters, every D = 0, so that a
    sampled score is minus the error term itself).  pitch8 >= 768: rows 40 .. 43 against query 4 give D = 2^23 - 1,
    2^23, -(2^23 - 1), -2^23."""
    rng = _rng("bytes", pitch8)
    rows = rng.integers(-127, 128, size=(N_ALLOC, pitch8)).astype(I8)
    q8 = rng.integers(-127, 128, size=(256, pitch8)).astype(I8)
    r, c = np.meshgrid(np.arange(N_ALLOC), np.arange(pitch8), indexing="ij")
    pat = ((r * 31 + c * 17 + (r ^ c)) % 255 - 127).astype(I8)
    rows[3::8] = pat[3::8]
    q8[5::8] = pat[5:256:8]
    rows[5], rows[6], rows[7] = 127, -127, 0
    rows[320:384] = 0
    q8[1], q8[2], q8[3], q8[6], q8[9] = 127, -127, 0, 0, 0
    if pitch8 >= 768:
        base = np.zeros(pitch8, I8)
        base[:521] = 127
        rows[40], rows[41] = base, base
        rows[40, 521], rows[41, 521] = 3, 4
        rows[42], rows[43] = -rows[40], -rows[41]
        q8[4] = 0
        q8[4, :520], q8[4, 520], q8[4, 521] = 127, 12, 1
    rows.setflags(write=False)
    q8.setflags(write=False)
    D = T.dots(rows, q8)
    if pitch8 >= 768:
        assert D[40:44, 4].tolist() == [2 ** 23 - 1, 2 ** 23, -(2 ** 23 - 1), -2 ** 23]
        assert abs(int(D[5, 1])) >= 2 ** 23
    return rows, q8, D


def _tables(pitch8, gbn, nv, special):
    """A plausible group table and query parameters (the magnitudes the quantisers produce for vectors of norm about 1 with
    pitch8 elements).  special: group 3 holds an infinite row (a_g = +inf, vouch 0), group 5 is all zero (s_g = a_g = b_g = 0),
    group 7 does not vouch, query 3 is the zero query, query 6 has E = +inf."""
    rng = _rng("tables", pitch8, gbn)
    s_g = (rng.uniform(0.5, 1.5, N_GROUPS) * 0.01).astype(F32)
    groups = np.stack([s_g, s_g * F32(70 * np.sqrt(pitch8)) * rng.uniform(0.9, 1.1, N_GROUPS).astype(F32),
                       s_g * F32(np.sqrt(pitch8 / 12)) * rng.uniform(0.9, 1.1, N_GROUPS).astype(F32), np.ones(N_GROUPS, F32)], axis=1).astype(F32)
    s_q = (rng.uniform(0.5, 1.5, gbn) * 0.008).astype(F32)
    qpar = np.stack([s_q, s_q * F32(np.sqrt(pitch8 / 12)) * rng.uniform(0.9, 1.1, gbn).astype(F32),
                     s_q * F32(70 * np.sqrt(pitch8)) * rng.uniform(0.9, 1.1, gbn).astype(F32), F32(1) / s_q], axis=1).astype(F32)
    if special:
        groups[3] = [groups[3, 0], np.inf, groups[3, 2], 0.0]
        groups[5] = [0.0, 0.0, 0.0, 1.0]
        groups[7, 3] = 0.0
        qpar[3] = 0.0
        qpar[6] = [0.0, np.inf, 0.0, 0.0]
    qpar[nv:] = 0.0
    return groups, qpar


def _end_bad():
    """the table's own bits: rows past the end"""
    g = np.zeros(N_GROUPS, U64)
    for r in range(N_ROWS, N_GROUPS * 64):
        g[r >> 6] |= U64(1) << U64(r & 63)
    return g


def _gbad(seed, share=0.2):
    """rows past the end, `share` of the others at random, rows 64 .. 95 (one whole wave: the LOW half of group 1 only) and rows
    160 .. 191 (the HIGH half of group 2 only)"""
    rng = _rng("gbad", seed)
    g = _end_bad()
    for r in np.flatnonzero(rng.random(N_ROWS) < share):
        g[r >> 6] |= U64(1) << U64(r & 63)
    g[1] = U64(0x00000000FFFFFFFF)
    g[2] = U64(0xFFFFFFFF00000000)
    return g


def _cn(rows, groups):
    """|c|^2 of the rows the bytes stand for; row 10: a NaN norm (a removed row), row 11: a norm that overflowed"""
    s = groups[np.arange(N_ROWS) >> 6, 0].astype(F64)
    cn = (s * s * (rows[:N_ROWS].astype(F64) ** 2).sum(axis=1)).astype(F32)
    cn[10], cn[11] = np.nan, np.inf
    return cn


def _case(pitch8, ct, metric=COS, partial=False, special=False, **kw):
    rows, q8, D = _bytes(pitch8)
    gbn = 64 * ct
    nv = gbn - 5 if partial else gbn
    groups, qpar = _tables(pitch8, gbn, nv, special)
    q = np.array(q8[:gbn])
    q[nv:] = 0
    tau = np.full(gbn, -np.inf, F32)
    tau[nv:] = np.inf
    t = Tile(ct=ct, pitch8=pitch8, rows=rows, q8=q, groups=groups, qpar=qpar, n_rows=N_ROWS, nv=nv, metric=metric, tau=tau,
             cn=_cn(rows, groups) if metric == L2 else None, **kw)
    Dq = np.array(D[:, :gbn])
    Dq[:, nv:] = 0
    return t, Dq


def _thresholds(t, D, shift=0, top=False):
    """tau per real query, by kind (query + shift) % 8, from the float64 upper bounds of the query's rows: the fp32 value of a
    chosen row's bound, its fp32 neighbours above and below, the median (the densest cluster), +0, -0, -inf, the fp32 value just below the largest (one row on the threshold, every other below).
    top: every query selective (the prefilter decides per 32 rows x 16 queries, and one query with a low threshold sends the whole
    column group to the exact epilogue): the fp32 value of the (1 + query % 6)-th largest bound or its neighbour below."""
    rng = _rng("tau", t.pitch8, t.ct, t.metric, shift)
    g = np.arange(N_ROWS) >> 6
    tau = t.tau.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(t.nv):
            ub = t.groups[g, 0].astype(F64) * F64(t.qpar[q, 0]) * D[:N_ROWS, q] + t.groups[g, 1].astype(F64) * F64(t.qpar[q, 1]) + \
                 t.groups[g, 2].astype(F64) * F64(t.qpar[q, 2])
            if t.metric == L2:
                ub = 2.0 * ub - t.cn.astype(F64)
            fin = np.flatnonzero(np.isfinite(ub))
            kind = (q + shift) % 8
            if top:
                v = F32(np.sort(ub[fin])[-min(len(fin), 1 + q % 6)])
                tau[q] = v if kind & 1 else np.nextafter(v, F32(-np.inf))
                continue
            if not len(fin):
                tau[q] = [0.0, -np.inf][kind & 1]
                continue
            pick = F32(ub[rng.choice(fin)])
            tau[q] = [pick, np.nextafter(pick, F32(np.inf)), np.nextafter(pick, F32(-np.inf)), F32(np.median(ub[fin])), F32(0.0), F32(-0.0),
                      F32(-np.inf), np.nextafter(F32(ub[fin].max()), F32(-np.inf))][kind]
    assert np.isfinite(tau[:t.nv]).sum() >= t.nv // 2
    return tau


def _exact_set(t, phase=1):
    live = np.zeros((N_ALLOC, t.gbn), bool)
    live[:N_ROWS, :t.nv] = True
    if t.masked or t.multi:
        live &= ~T.bad_matrix(t, phase)
    return live


# (phase 1 form) -> the Tile fields that select it; every instance pick_gemm8<1> can return
FORMS = {
    "pre_block": dict(),
    "exact13": dict(variant=13),
    "masked": dict(masked=True),
    "multi": dict(multi=True),
    "l2": dict(metric=L2),
    "l2_masked": dict(metric=L2, masked=True),
    "l2_multi": dict(metric=L2, multi=True),
}
CLASS_ROW = (2, 0, 1, 1, 0, 2, 2, 1, 0, 0, 1, 2, 1, 2, 0, 1)


def _form_case(form, pitch8, ct, partial=False, special=False, grid=1, **kw):
    f = dict(FORMS[form])
    if f.get("masked"):
        f["gbad"] = _gbad(("m", pitch8))
    if f.get("multi"):
        f["gbad"] = np.stack([_gbad(("c0", pitch8), 0.1), _end_bad(), _gbad(("c2", pitch8), 0.6)])
        f["class_row"] = CLASS_ROW
    f.update(kw)
    return _case(pitch8, ct, partial=partial, special=special, grid=grid, **f)


def _exact_cases():
    out = []
    i = 0
    for pitch8 in T.PITCHES:
        for ct in (1, 2, 4):
            for form, f in FORMS.items():
                if not T.fits(ct, pitch8, f.get("metric", COS)):
                    continue
                out.append(pytest.param(form, pitch8, ct, (1, 2, 5)[i % 3], bool(i & 1), id=f"{form}-p{pitch8}-ct{ct}-g{(1, 2, 5)[i % 3]}-{'partial' if i & 1 else 'full'}"))
                i += 1
    out.append(pytest.param("pre_group12", 384, 4, 2, True, id="pre_group12-p384-ct4-g2-partial"))
    return out


def _run_exact(run, form, pitch8, ct, grid, partial):
    if form == "pre_group12":
        t, D = _case(pitch8, ct, partial=partial, grid=grid, variant=12)
    else:
        t, D = _form_case(form, pitch8, ct, partial=partial, grid=grid)
    T.check_pairs(t, run(t), D, exact_set=_exact_set(t))


KEEP_CASES = [("pre_block", 128, 4, 5), ("pre_block", 256, 2, 2), ("pre_block", 384, 4, 1), ("exact13", 384, 1, 2), ("pre_block", 640, 2, 1),
              ("masked", 768, 2, 5), ("multi", 1152, 1, 2), ("pre_block", 1536, 1, 1), ("l2", 128, 2, 2), ("l2", 384, 2, 5), ("l2_masked", 768, 1, 1),
              ("l2_multi", 256, 1, 2)]


def _run_keep(run, form, pitch8, ct, grid, shift):
    t, D = _form_case(form, pitch8, ct, partial=True, special=True, grid=grid)
    t.tau = _thresholds(t, D, shift)
    kept = T.check_pairs(t, run(t), D)
    skipped = T.check_keep(t, kept, D)
    assert skipped <= SPECIAL_SHARE, skipped
    # special groups and queries, stated directly: the a_g = +inf group is kept whole for every real query with a threshold
    real = np.flatnonzero(t.tau[:t.nv] < np.inf)
    live = _exact_set(t)
    assert (kept[192:256][:, real] == live[192:256][:, real]).all()
    # the E = +inf query keeps every row its class allows (but a NaN norm's)
    ok = np.ones(N_ALLOC, bool)
    if t.metric == L2:
        ok[10] = False
    assert (kept[ok, 6] == live[ok, 6]).all()
    # the all-zero group: all rows or none, per query
    z = kept[320:384][live[320:384].any(axis=1)]
    assert ((z == z[:1]) | ~live[320:384][live[320:384].any(axis=1)]).all()
    return kept


def _gref_variants(t):
    """gref under which the groups are all ordinary / some over a_ref only / some over b_ref only"""
    a, b = np.sort(t.groups[np.isfinite(t.groups[:, 1]), 1]), np.sort(t.groups[:, 2])
    return [np.array([a[-1], b[-1]], F32), np.array([a[len(a) // 2], b[-1]], F32), np.array([a[-1], b[len(b) // 2]], F32)]


def _uniform(t):
    """every group with the same a_g and b_g, and these as a_ref, b_ref: the prefilter's threshold is then the exact one but for
    its own 4e-6, so a prefilter a little too strict loses the rows that sit on tau"""
    g = t.groups.copy()
    g[:, 1], g[:, 2] = g[:, 1].max(), g[:, 2].max()
    return T.replace(t, groups=g, gref=np.array([g[0, 1], g[0, 2]], F32))


def _run_prefilter_equal(run, pitch8, ct, grid):
    t, D = _case(pitch8, ct, partial=True, special=True, grid=grid)
    t.tau = _thresholds(t, D, 1)
    want = T.check_pairs(t, run(T.replace(t, variant=13)), D)
    assert want.any() and not want[:N_ROWS, :t.nv].all()
    variants = (0, 12) if (ct, pitch8) == (4, 384) else (0,)
    for gref in _gref_variants(t):
        for variant in variants:
            got = T.check_pairs(t, run(T.replace(t, variant=variant, gref=gref)), D)
            assert (got == want).all(), (variant, gref, np.argwhere(got != want)[:4])
    t, D = _case(pitch8, ct, partial=True, grid=grid)
    t = _uniform(t)
    t.tau = _thresholds(t, D, 2, top=True)
    want = T.check_pairs(t, run(T.replace(t, variant=13)), D)
    T.check_keep(t, want, D)
    for variant in variants:
        got = T.check_pairs(t, run(T.replace(t, variant=variant)), D)
        assert (got == want).all(), (variant, "uniform", np.argwhere(got != want)[:4])


def _phase0_case(pitch8, ct, metric, stride, multi=False, seed=0):
    kw = dict(num_tiles=3, tile_stride=stride, special=True, partial=True, metric=metric)
    if multi:
        t, D = _case(pitch8, ct, multi=True, class_row=CLASS_ROW, gbad=np.stack([_gbad(("p0", seed), 0.1), _end_bad(), _gbad(("p2", seed), 0.6)]), **kw)
    else:
        t, D = _case(pitch8, ct, gbad=_gbad(("p", seed), 0.3), **kw)
        # query 0's single best row of block 0 is bad: the next best row vouches
        best = int(np.argmax(D[:32, 0]))
        g = t.gbad.copy()
        g[0] |= U64(1) << U64(best)
        t.gbad = g
    if stride == 1:  # the first three tiles alone: a corpus that ends inside them (the harness wants n_rows within the tiles it is given)
        t.n_rows = 3 * 256 - 37
        g = np.atleast_2d(t.gbad).copy()
        for r in range(t.n_rows, 3 * 256):
            g[:, r >> 6] |= U64(1) << U64(r & 63)
        t.gbad = g if multi else g[0]
        if metric == L2:
            t.cn = t.cn[:t.n_rows]
    return t, D


PHASE0_CASES = [(128, 4, COS, 1, False), (384, 4, COS, 2, False), (256, 2, COS, 2, True), (768, 2, COS, 1, False), (1536, 1, COS, 2, False),
                (640, 2, L2, 2, False), (384, 1, L2, 1, True), (768, 2, L2, 2, False)]


# --------------------------------------------------------------------------- #
# CPU half: the checkers accept the restatement and reject the wrong ones
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("form,pitch8,ct,grid,partial", [p for p in _exact_cases() if p.values[1] in (128, 384, 640)])
def test_checker_accepts_restated_dot_products(form, pitch8, ct, grid, partial):
    _run_exact(T.restate_phase1, form, pitch8, ct, grid, partial)


@pytest.mark.parametrize("form,pitch8,ct,grid", KEEP_CASES)
@pytest.mark.parametrize("shift", [0, 3])
def test_checker_accepts_restated_keep_rule(form, pitch8, ct, grid, shift):
    kept = _run_keep(T.restate_phase1, form, pitch8, ct, grid, shift)
    assert kept.any() and not kept[:N_ROWS].all()


def test_checker_accepts_restated_prefilter():
    _run_prefilter_equal(T.restate_phase1, 384, 4, 2)
    _run_prefilter_equal(T.restate_phase1, 256, 1, 5)


@pytest.mark.parametrize("pitch8,ct,metric,stride,multi", PHASE0_CASES)
def test_checker_accepts_restated_phase0(pitch8, ct, metric, stride, multi):
    t, D = _phase0_case(pitch8, ct, metric, stride, multi)
    out = T.restate_phase0(t)
    T.check_halfmax(t, out, D)
    assert (out["halfmax"] == 0).any() and (out["halfmax"] != 0).any()


def test_checker_rejects_wrong_restatements():
    # a swapped row half, the other parity's swizzle key: the dot products no longer belong to the (row, query) of the pair
    for bug, pitch8 in (("row_half", 128), ("swizzle_parity", 128), ("swizzle_parity", 256), ("swizzle_parity", 384)):
        t, D = _case(pitch8, 1, grid=2)
        with pytest.raises(AssertionError, match="D24 differs"):
            T.check_pairs(t, T.restate_phase1(t, bug), D, exact_set=_exact_set(t))
    # + 1 in place of - 1 in T: rows sitting on the threshold are dropped
    t, D = _case(128, 2, partial=True, grid=2, variant=13)
    t.tau = _thresholds(t, D, 0)
    T.check_keep(t, T.check_pairs(t, T.restate_phase1(t), D), D)
    with pytest.raises(AssertionError, match="were dropped"):
        T.check_keep(t, T.check_pairs(t, T.restate_phase1(t, "slack_sign"), D), D)
    # a prefilter stricter than the exact test
    t = T.replace(_uniform(t), variant=0)
    t.tau = _thresholds(t, D, 0, top=True)
    T.check_keep(t, T.check_pairs(t, T.restate_phase1(t), D), D)
    with pytest.raises(AssertionError, match="were dropped"):
        T.check_keep(t, T.check_pairs(t, T.restate_phase1(t, "pre_strict"), D), D)
    # the wave's bad-row bits from the other half of the word, full pass and sample pass
    t, D = _form_case("masked", 128, 1, grid=2)
    with pytest.raises(AssertionError, match="a bad row was emitted"):
        T.check_pairs(t, T.restate_phase1(t, "bad_shift"), D, exact_set=_exact_set(t))
    t, D = _phase0_case(128, 1, COS, 1)
    with pytest.raises(AssertionError):
        T.check_halfmax(t, T.restate_phase0(t, "bad_shift"), D)
    # tile_stride ignored in the group index
    t, D = _phase0_case(128, 1, COS, 2)
    with pytest.raises(AssertionError):
        T.check_halfmax(t, T.restate_phase0(t, "stride_ignored"), D)
    # ... and a kept set one row too generous fails tightness
    t, D = _case(128, 1, grid=1, variant=13)
    t.tau = _thresholds(t, D, 0)
    kept = T.check_pairs(t, T.restate_phase1(t), D)
    _, may_not, _ = T.keep_rule(t, D)
    assert may_not.any()
    kept[tuple(np.argwhere(may_not)[0])] = True
    with pytest.raises(AssertionError, match="further below tau"):
        T.check_keep(t, kept, D)


def test_ring_rule_covers_the_shapes():
    rings = {(ct, p): T.ring_rule(ct, p) for p in T.PITCHES for ct in (1, 2, 4) if T.fits(ct, p)}
    assert set(rings.values()) == {2, 3, 4, 6}
    assert {(p // 128) & 1 for p in T.PITCHES} == {0, 1}
    assert all((p // 64) % r == 0 for (ct, p), r in rings.items())


def test_small_kernel_restatements():
    gbad = _gbad("small")
    mask = _rng("mask").integers(0, 2 ** 32, size=2 * 41, dtype=np.uint64).astype(U32)
    out = T.gbad_with_mask_py(gbad, mask, 39, 41, [1, -1, 0])
    assert (out[1] == gbad).all()
    assert (out[0][20:] == U64(0xFFFFFFFFFFFFFFFF)).all()          # groups past the mask's end: every row bad
    assert out[0][19] >> U64(32) == U64(0xFFFFFFFF)                 # the odd word count: the last group's high half reads as zero
    assert (out[0][:19] == (gbad[:19] | ~(mask[41:41 + 38:2].astype(U64) | (mask[42:42 + 38:2].astype(U64) << U64(32))))).all()


# --------------------------------------------------------------------------- #
# GPU half
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
def test_instances_rings_and_refusals():
    assert T.load().tile_lds_b_max() == T.LDS_B_MAX and T.load().tile_pair_d_unknown() == T.PAIR_D_UNKNOWN
    for p in T.PITCHES:
        for ct in (1, 2, 4):
            for l2 in (False, True):
                for masked, multi in ((False, False), (True, False), (False, True)):
                    for phase in (0, 1):
                        has, ring, lds = T.instance(phase, ct, p, l2, masked, multi)
                        assert has == (not (l2 and ct == 4))
                        assert ring == T.ring_rule(ct, p) and lds == 64 * ct * p + 64 * ct * 16
    with pytest.raises(ValueError):
        T.instance(1, 3, 128)
    # refused before anything is launched: too short a pairs array, a query block beyond the LDS, a pitch off the 128 grid,
    # a row count beyond the tiles, a group table one entry short, a class row beyond the tables
    t, _ = _case(128, 1, grid=2)
    with pytest.raises(ValueError):
        T.phase1(t, short=T.GUARD + 1)
    for bad in (T.replace(t, ct=4, pitch8=768), T.replace(t, pitch8=192), T.replace(t, n_rows=N_ALLOC + 1), T.replace(t, groups=t.groups[:19]),
                T.replace(t, multi=True, gbad=np.stack([_end_bad()] * 2), class_row=(0, 1, 2, 0) + (0,) * 12), T.replace(t, masked=True, gbad=None)):
        with pytest.raises(ValueError):
            T.phase1(bad)
    with pytest.raises(ValueError):
        T.phase0(T.replace(t, gbad=_end_bad(), num_tiles=3, tile_stride=3))


@pytest.mark.gpu
@pytest.mark.parametrize("form,pitch8,ct,grid,partial", _exact_cases())
def test_dot_products_bit_exact(form, pitch8, ct, grid, partial):
    """tau = -inf: every row < n_rows of every real query exactly once (minus the bad rows of a masked / multi instance), D24 =
    the int64 dot product or PAIR_D_UNKNOWN from 2^23 on, pair_count exact per wave, padded queries and rows past the end
    never: for every instance the picker returns."""
    _run_exact(T.phase1, form, pitch8, ct, grid, partial)


@pytest.mark.gpu
@pytest.mark.parametrize("form,pitch8,ct,grid", KEEP_CASES)
@pytest.mark.parametrize("shift", [0, 3])
def test_keep_rule(form, pitch8, ct, grid, shift):
    """Thresholds on the rows' own upper bounds: safety on every entry, tightness within the derived slack (tile_harness
    docstring), the special groups and queries, bad rows absent far above tau."""
    _run_keep(T.phase1, form, pitch8, ct, grid, shift)


@pytest.mark.gpu
@pytest.mark.parametrize("pitch8,ct,grid", [(384, 4, 2), (256, 1, 5), (768, 2, 1), (1152, 1, 2)])
def test_prefilter_forms_equal_exact(pitch8, ct, grid):
    _run_prefilter_equal(T.phase1, pitch8, ct, grid)


@pytest.mark.gpu
@pytest.mark.parametrize("pitch8,ct,metric,stride,multi", PHASE0_CASES)
def test_phase0(pitch8, ct, metric, stride, multi):
    t, D = _phase0_case(pitch8, ct, metric, stride, multi)
    for grid in (1, 2):
        T.check_halfmax(t, T.phase0(T.replace(t, grid=grid)), D)


@pytest.mark.gpu
def test_pair_lists_overflow_and_library_grid():
    t, D = _form_case("masked", 384, 2, partial=True, grid=5, pair_cap=100)
    out = T.phase1(t)
    T.check_pairs(t, out, D, exact_set=_exact_set(t))
    assert (out["count"] > 100).any() and out["count"][2] == 0  # (rows 64 .. 95, tile 0's wave 2: all 32 rows bad)
    # grid 0: the library's rule, one workgroup per CU up to the tiles
    t, D = _case(256, 1, grid=3)
    T.check_pairs(t, T.phase1(t, cus=3, grid=0), D, exact_set=_exact_set(t))


@pytest.mark.gpu
def test_gbad_with_mask_kernel():
    rng = _rng("gbadmask")
    gbad = _gbad("k")
    n_groups = len(gbad)
    words = (N_ROWS + 31) // 32  # 39: odd
    stride = 41
    mask = rng.integers(0, 2 ** 32, size=3 * stride, dtype=np.uint64).astype(U32)  # (bits set past the last row included)
    for class_mask, grid_x in ((None, 0), ([1, -1, 0, 2], 0), ([2, 2, -1], 3)):
        got, guard = T.gbad_with_mask(gbad, mask, words, stride, class_mask, grid_x)
        assert (got == T.gbad_with_mask_py(gbad, mask, words, stride, class_mask)).all()
        assert (guard == T.SENT_KEY).all()
        assert ((got & _end_bad()[None, :]) == _end_bad()[None, :]).all()  # rows past the end stay bad whatever the mask says
    got, _ = T.gbad_with_mask(gbad, None, 0, 0, [-1, -1])
    assert (got == gbad[None, :]).all() and n_groups == N_GROUPS


@pytest.mark.gpu
def test_group_ref_kernel():
    rng = _rng("gref")
    for name in ("ordinary", "mixed", "none_finite"):
        g, _ = _tables(384, 64, 64, False)
        g = np.tile(g, (40, 1))[:777]
        g[:, 1:3] *= rng.uniform(0.8, 1.2, size=(len(g), 2)).astype(F32)
        if name != "ordinary":
            g[5, 1] *= 3          # outliers: over 1.5 x the mean
            g[6, 2] *= 3
            g[7, 1] = np.inf      # an infinite row
            g[8] = 0              # a pad group
            g[9, 1] = np.nan
        if name == "none_finite":
            g[:, 1] = np.inf
        ref = T.group_ref(g, grid_x=0 if name != "mixed" else 2)
        aref, bref, sa, sb, cnt, ordinary, edge = T.group_ref_py(g)
        assert not edge.any()
        assert ref[4] == cnt and (ref[5:] == 0).all()
        assert ref[0] == aref.view(U32) and ref[1] == bref.view(U32)       # maxima: bit-exact
        # sums: cnt fp32 additions in any order
        f = ref[:4].view(F32)
        assert abs(float(f[2]) - sa) <= T.U * cnt * sa * 1.01 + 1e-30 and abs(float(f[3]) - sb) <= T.U * cnt * sb * 1.01 + 1e-30
        if name == "none_finite":
            assert cnt == 0 and (ref[:4] == 0).all()
        if name == "mixed":
            assert not ordinary[5:10].any() and ordinary.any() and not ordinary[np.isfinite(g[:, 1]) & (g[:, 0] > 0)].all()
