"""The fp32 and bf16 tile kernels alone (kernels_tiles.h), launched by tests/kernel_harness/gemm_harness.hip with the instances
the library's own picker returns: 41 per phase (18 fp32, 16 bf16 on fp32 rows, 7 on the bf16 shadow), their two conversions and
the small kernels of kernels_aux.h behind their margins.

Shapes: five whole tiles and a partial one (5 T + 64 + 37 rows, T = 128 / 256), grid 2 (a workgroup walks three tiles) and
once per case the library's grid; fp32 widths of 3, 8, 13, 16 quads, bf16 widths of 5, 8, 16, 21, 32 quads, shadow rows of
dim 100, 128, 200; nv = 64 CT - 5 queries.  The rows the bf16 tiles read behind n_rows are poisoned (NaN, +inf, huge).

INTEGER corpora ([-4, 4]: exact in bf16, sums far below 2^24): every key must EQUAL the int64 reference.  They hold a zero
row, the query itself, single NaN rows, +inf elements, one whole wave group of NaN rows and (at the widest width) a partial
last group whose rows below n_rows are all NaN.  FLOAT corpora against float64 inside the library's own documented bounds,
nothing added: fp32 tiles gamma sum |c_i q_i| + under_abs (L2: gamma (2 sum |c_i q_i| + cn) + 2 under_abs), gamma = 1.02 nu /
(1 - nu), nu = (pitch + 18) 2^-24 as tau_margin_kernel computes it, under_abs = (pitch + 18) 2^-149; bf16 tiles eps_dot |c||q|
+ floor_abs (|c| + |q|) + under_abs, eps_dot = gamma + 1.05 2^-7, floor_abs = 7.5e-37 sqrt(pitch) (L2, v = 2 dot - cn: twice
that + gamma cn, the form GemmArgs documents).

Idle and padded columns hold ZERO queries, as the library's conversions leave them: a column whose threshold is +inf is only
safe from a +inf score because 0 * inf is NaN.  live = 1 runs with tau = -inf in EVERY column (the library hands such a pass
the other queries' finite thresholds), once with the idle columns' queries left in place.

Worst |error| / bound measured on an MI355X (test_float_corpora_stay_inside_the_documented_bounds prints them), over the
corpora normal / midpoint / denormal / clamp:
  bf16 tiles on fp32 rows, inner product 0.334 / 0.946 / 0.354 / 0.369, L2 0.334 / 0.946 / 0.354 / 0.346
  bf16 tiles on the shadow,  inner product 0.137 / 0.946 / 0.146 / 0.190, L2 0.137 / 0.946 / 0.146 / 0.136
  fp32 tiles,                inner product 0.133 / 0.188 / 0.133 / 0.108, L2 0.090 / 0.191 / 0.100 / 0.073
  per-group bounds (one group 100 x the rest): fp32 L2 0.033, bf16 0.232, shadow 0.119
No ratio exceeds 1: the fp32 tiles round once per term and the bf16 bound holds on gfx950.

under_abs is what these tests found.  The denormal corpus holds rows that are denormal throughout; their scores are denormal,
and gradual underflow rounds every fma there to a multiple of 2^-149 whatever its operands.  Against the purely relative
bound the fp32 tiles had until then (gamma alone) they came out one unit off: 1.7e-45 against a band of 1.5e-45, a ratio of
1.13.  The library's bounds now carry the absolute term (tau_margin_kernel, the per-group bound, sel_under), for every family:
the bf16 tiles accumulate in fp32 as well."""
import numpy as np
import pytest

import gemm_harness as G

pytestmark = pytest.mark.gpu

_F32, _F64, _U16, _U32, _U64 = np.float32, np.float64, np.uint16, np.uint32, np.uint64
COS, L2 = G.METRIC_COSINE, G.METRIC_L2
METRICS = (COS, L2)
WIDTHS = {G.FP32: (3, 8, 13, 16), G.BF16: (5, 8, 16, 21, 32), G.SHADOW: (100, 128, 200)}  # quads; shadow: dims
POISON = {"nan": (np.nan, 0x7FC0), "inf": (np.inf, 0x7F80), "huge": (3.0e38, 0x7F7F)}
P2 = dict(eps=2.0 ** -7, gam=2.0 ** -18, floor_abs=2.0 ** -10, under_abs=2.0 ** -6)  # powers of two: the float32 mirror has one reading

COMBOS = [(f, ct, m, gb) for f in G.FAMILIES for ct in (1, 2, 4) for m in METRICS for gb in (0, 1) if G.has_instance_py(f, ct, m, gb)]
IDS = [f"{G.FAMILY_NAME[f]}-ct{ct}-{'l2' if m else 'ip'}{'-gb' if gb else ''}" for f, ct, m, gb in COMBOS]
COVERED = set()  # the picker's instance (its function's identity) of every tile launch of this session


class Case:
    """One corpus on one family and width, in the form its tile kernel reads."""

    def __init__(self, family, width, ct, rows, q, poison="nan", nv=None):
        self.family, self.ct = family, ct
        self.T, self.RW, self.gbn = G.tile_rows(family), G.wave_groups(family), 64 * ct
        self.n, self.d = rows.shape
        self.pitch = self.d  # floats per fp32 row (a multiple of 4)
        self.rows, self.nv = rows, len(q) if nv is None else nv
        self.qblock = np.zeros((self.gbn, self.d), _F32)
        self.qblock[:self.nv] = q[:self.nv]
        self.tiles = (self.n + self.T - 1) // self.T
        covered = self.tiles * self.T
        self.cn = G.sqnorm32(rows)
        self.qb16 = None
        self.qb_pitch16 = 0
        if family == G.FP32:
            self.pitch4, self.dev_rows = self.d // 4, rows
        elif family == G.BF16:
            self.pitch4 = self.d // 4
            self.dev_rows = np.full((covered, self.d), POISON[poison][0], _F32)
            self.dev_rows[:self.n] = rows
        else:
            pitch16 = (self.d + 127) // 128 * 128
            self.pitch4 = pitch16 // 8
            self.dev_rows = np.full((covered, pitch16), POISON[poison][1], _U16)
            self.dev_rows[:self.n] = 0
            self.dev_rows[:self.n, :self.d] = G.to_bf16_sel(rows)
        if family != G.FP32:
            self.qb_pitch16 = G.qb_pitch16_py(family, self.pitch)
            self.qb16 = np.zeros((self.gbn, self.qb_pitch16 * 8), _U16)
            self.qb16[:, :self.d] = G.to_bf16_sel(self.qblock)

    def single(self):
        """The same case with one live query in column 0, the other columns zero (the library's single-query block)."""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.qblock = np.zeros_like(self.qblock)
        c.qblock[0] = self.qblock[0]
        if self.qb16 is not None:
            c.qb16 = np.zeros_like(self.qb16)
            c.qb16[0] = self.qb16[0]
        return c

    def run(self, phase, metric, groupb=None, grid=2, live=0, tau=None, cap=0, num_tiles=None, tile_stride=1, cn=None):
        num_tiles = self.tiles if num_tiles is None else num_tiles
        kw = {} if groupb is None else groupb
        out = G.tiles(phase, self.family, self.ct, metric, self.dev_rows, self.n, self.pitch4, num_tiles, tile_stride, grid=grid,
                      queries=self.qblock if self.family == G.FP32 else None, qb16=self.qb16, qb_pitch16=self.qb_pitch16,
                      cn=(self.cn if cn is None else cn) if metric == L2 else None, live=live, tau=tau, cap=cap, **kw)
        COVERED.add(G.instance(phase, self.family, self.ct, metric, groupb is not None, self.pitch4)["fn"])
        return out

    def scores(self, metric, q=None):
        """float64 reference [n, gbn] and sum |c_i q_i|."""
        return G.ieee_scores(self.rows, self.qblock if q is None else q, metric, self.cn)

    def groupb(self, params=P2, gmax=None):
        cn = np.where(np.isfinite(self.cn), self.cn, _F32(0.0))
        gmax = G.group_max(cn, self.n) if gmax is None else gmax
        qn = G.query_norm_mirror(self.qblock, self.nv, self.gbn)
        return dict(gmax=gmax, qn=qn, **params)


def _dims(family, width):
    return width if family == G.SHADOW else 4 * width


def _rows_of(family):
    return 5 * G.tile_rows(family) + 64 + 37


def _nan_group(family):
    """The wave group of the integer corpora whose rows ALL score NaN: the second of tile 2, visited at tile_stride 1 and 2."""
    return 2 * G.wave_groups(family) + 1


def _int_case(family, width, ct, seed, poison="nan", specials=True, infs=True, nan_tail=False):
    rng = np.random.default_rng(seed)
    n, d, nv = _rows_of(family), _dims(family, width), 64 * ct - 5
    rows, q = G.int_corpus(rng, n, d, nv)
    if specials:
        rows[1] = 0.0
        rows[5] = q[0]
        rows[70, d // 2] = np.nan
        rows[n - 1, d - 1] = np.nan  # the last row: what clamped loads re-read
        g = _nan_group(family)
        rows[64 * g:64 * g + 64, 1] = np.nan  # a whole wave group of NaN scores
        if nan_tail:
            rows[n - 37:, 2] = np.nan  # the partial last group: every row that survives the n_rows test scores NaN
        if infs:
            rows[200, d - 1] = np.inf
            rows[n - 40, 0] = np.inf
    return Case(family, width, ct, rows, q, poison)


def _tau_dump(c, live=0):
    """tau = -inf for the live queries.  live = 0: +inf for the padded slots, as the library leaves them.  live > 0: -inf for
    EVERY column -- the library hands a single-query pass the other queries' finite thresholds (tau = d_tau + i), so only the
    kernel's own `live` gate keeps the idle columns from appending."""
    tau = np.full(c.gbn, -np.inf, _F32)
    if live == 0:
        tau[c.nv:] = np.inf
    return tau


def _p2_bound(gbk, metric):
    return G.group_bound(gbk["gmax"], gbk["qn"], P2["eps"], P2["gam"], P2["floor_abs"], metric, under_abs=P2["under_abs"])


def _all_instances():
    """Every instance the picker returns over the tests' widths: fn -> (phase, family, ct, metric, groupb, ktail)."""
    ids = {}
    for phase in (0, 1):
        for family, ct, metric, gb in COMBOS:
            for width in WIDTHS[family]:
                p4 = width if family != G.SHADOW else (width + 127) // 128 * 128 // 8
                inst = G.instance(phase, family, ct, metric, gb, p4)
                ids[inst["fn"]] = (phase, G.FAMILY_NAME[family], ct, metric, gb, inst["ktail"])
    return ids


def test_the_picker_returns_41_instances_per_phase_and_refuses_the_rest():
    ids = set()
    for phase in (0, 1):
        have = 0
        for family in G.FAMILIES:
            for ct in (1, 2, 4):
                for metric in METRICS:
                    for groupb in (0, 1):
                        for width in WIDTHS[family]:
                            p4 = width if family != G.SHADOW else (width + 127) // 128 * 128 // 8
                            inst = G.instance(phase, family, ct, metric, groupb, p4)
                            assert (inst is not None) == G.has_instance_py(family, ct, metric, groupb), (phase, family, ct, metric, groupb)
                            if inst is None:
                                continue
                            assert inst["ktail"] == G.ktail_py(family, p4) and inst["lds"] == G.lds_bytes_py(family, ct)
                            assert inst["per_cu"] == G.per_cu_py(family, ct) and inst["threads"] == (256 if family == G.FP32 else 512)
                            if inst["fn"] not in ids:
                                ids.add(inst["fn"])
                                have += 1
                            assert G.grid_rule(phase, family, ct, metric, groupb, p4, 1000, 256) == min(1000, 256 * inst["per_cu"])
                            assert G.grid_rule(phase, family, ct, metric, groupb, p4, 3, 256) == 3
        assert have == 41, have
    assert len(ids) == 82
    # refused: bf16 with CT = 1, fp32 cosine with group bounds, shadow L2 with group bounds at CT = 4
    assert G.instance(1, G.BF16, 1, COS, 0, 16) is None and G.instance(0, G.SHADOW, 1, L2, 0, 16) is None
    assert G.instance(1, G.FP32, 4, COS, 1, 8) is None and G.instance(0, G.SHADOW, 4, L2, 1, 16) is None
    assert G.instance(1, G.SHADOW, 2, L2, 1, 16) is not None and G.instance(1, G.SHADOW, 4, COS, 1, 16) is not None
    assert len(COMBOS) == 24 and set(_all_instances()) == ids  # what the last test of this file expects to have been launched


@pytest.mark.parametrize("combo", COMBOS, ids=IDS)
def test_dump_and_phase0_on_integer_corpora(combo):
    """(a) PHASE 1 with tau = -inf and cap >= n_rows: every key equals the int64 reference; NaN rows absent; padded and idle
    columns untouched; guards intact; poisoned pad rows change nothing.  (c) PHASE 0 with tile_stride 1 and 2, live 0 and 1."""
    family, ct, metric, gb = combo
    for wi, width in enumerate(WIDTHS[family]):
        poisons = ("nan",) if family == G.FP32 else (("nan", "inf", "huge") if wi < 2 else (("nan", "inf", "huge")[wi % 3],))
        nan_tail = wi == len(WIDTHS[family]) - 1
        for pi, poison in enumerate(poisons):
            c = _int_case(family, width, ct, 100 + width, poison, nan_tail=nan_tail)
            gbk = dict(c.groupb(), under_abs=P2["under_abs"]) if gb else None
            exact = c.scores(metric)[0].astype(_F32)
            g = _nan_group(family)
            assert np.isnan(exact[64 * g:64 * g + 64, :c.nv]).all() and (not nan_tail or np.isnan(exact[c.n - 37:, :c.nv]).all())
            cap = c.n + 3
            for grid, live in ((2, 0), (0, 0), (2, 1)) if pi == 0 else ((2, 0),):
                # live = 1: the idle columns hold zero queries (score 0 >= their tau of -inf: only the gate stops them)
                cc = c if live == 0 else c.single()
                cand, count = cc.run(1, metric, gbk, grid=grid, live=live, tau=_tau_dump(c, live), cap=cap)
                G.check_dump(cand, count, c.gbn, cap, c.n, c.nv if live == 0 else 1, exact=exact)
            if pi == 0 and wi == 0:
                # live = 1 with the idle columns' queries left in place and tau = -inf throughout.  (No infinite element
                # here: inf >= inf holds, and an idle column is safe from a +inf score only because its query is zero.)
                f = _int_case(family, width, ct, 100 + width, poison, infs=False)
                fgb = dict(f.groupb(), under_abs=P2["under_abs"]) if gb else None
                cand, count = f.run(1, metric, fgb, grid=2, live=1, tau=_tau_dump(f, 1), cap=cap)
                G.check_dump(cand, count, f.gbn, cap, f.n, 1, exact=f.scores(metric)[0].astype(_F32))
            if pi > 0 and wi > 0:
                continue
            bound = _p2_bound(gbk, metric) if gb else None
            S = np.zeros((c.tiles * c.T, c.gbn), _F32)
            S[:c.n] = exact
            for stride, live in ((1, 0), (2, 0), (1, 1)):
                nt = (c.tiles + stride - 1) // stride
                blank = np.full(c.gbn * c.RW * nt + G.GUARD, G.SENT_KEY, _U64)
                cc = c if live == 0 else c.single()
                got = cc.run(0, metric, gbk, grid=2, live=live, num_tiles=nt, tile_stride=stride)
                want = G.model_phase0(S, c.n, family, nt, stride, live, blank, bound=bound)
                hm = want[:c.gbn * c.RW * nt].reshape(c.gbn, -1)
                cols = c.nv if live == 0 else 1
                # key 0: the group that is NaN throughout, the partial last group whose surviving rows are all NaN
                assert (hm[:cols, (g // c.RW // stride) * c.RW + g % c.RW] == 0).all() and (hm[:cols, :g % c.RW] != 0).all()
                if nan_tail and stride == 1:
                    assert (hm[:cols, (c.n - 1) // 64] == 0).all() and (hm[:cols, (c.n - 1) // 64 - 1] != 0).all()
                G.check_halfmax(got, want)


@pytest.mark.parametrize("combo", COMBOS, ids=IDS)
def test_keep_rule_cap_and_the_maximum_of_16_shortcut(combo):
    """(b) thresholds ON rows' scores, different per column, +inf for padded slots; cap overflow; columns 0 .. 15: exactly one
    row of one 16-row register group qualifies, at position p for column p -- every other register group has none."""
    family, ct, metric, gb = combo
    width = WIDTHS[family][0] if family != G.FP32 else 13
    c = _int_case(family, width, ct, 7, specials=False)
    rows, q = c.rows.copy(), c.qblock[:c.nv]
    planted = [64 + 4 + (p & 3) + 8 * (p >> 2) for p in range(16)]
    assert all(G.register_group_of(r) == (64, 1, p) for p, r in enumerate(planted))
    for p, r in enumerate(planted):
        rows[r] = q[p] if metric == L2 else np.where(q[p] >= 0, 4.0, -4.0)
    rows[300, 0] = np.nan
    c = Case(family, width, ct, rows, q)
    gbk = dict(c.groupb(), under_abs=P2["under_abs"]) if gb else None
    S = c.scores(metric)[0].astype(_F32)
    bound = _p2_bound(gbk, metric) if gb else np.zeros((1 << 10, c.gbn), _F32)
    tau = np.full(c.gbn, np.inf, _F32)
    R = np.arange(c.n)
    for col in range(c.nv):
        s = np.sort(S[:, col][~np.isnan(S[:, col])])
        tau[col] = s[-1] if col < 16 else s[-(20 + col % 23)]
        if col < 16:  # the cut, not the threshold, sits on the planted row's score
            tau[col] = tau[col] + bound[planted[col] >> 6, col]
    want = []
    for col in range(c.gbn):
        with np.errstate(invalid="ignore"):
            keep = S[:, col] >= (tau[col] - bound[R >> 6, col]).astype(_F32)
        want.append(G.make_keys(G.f2ord(S[keep, col] + _F32(0.0)), R[keep]))
    if not gb:
        for p in range(16):
            assert G.key_row(want[p]).tolist() == [planted[p]], (p, G.key_row(want[p]))
    assert max(w.size for w in want) > 7 and all(w.size == 0 for w in want[c.nv:])
    for cap in (c.n, 7):
        cand, count = c.run(1, metric, gbk, grid=2, tau=tau, cap=cap)
        G.check_keep(cand, count, c.gbn, cap, want)


def _float_corpora(rng, n, d, nv):
    """name -> (rows, q): normal values; same-sign rows parallel to the query with every element just below a bf16 rounding
    midpoint; elements in the fp32 denormal range (single elements, and rows that are denormal throughout, whose scores are
    denormal themselves); one element above the bf16 maximum."""
    out = {}
    rows, q = rng.standard_normal((n, d)).astype(_F32), rng.standard_normal((nv, d)).astype(_F32)
    out["normal"] = (rows, q)
    mid = _F32((1 + 2.0 ** -8) * (1 - 2.0 ** -20))
    e = rng.integers(-3, 4, (n, 1))
    out["midpoint"] = ((mid * 2.0 ** e * np.ones((n, d))).astype(_F32), (mid * 2.0 ** rng.integers(-2, 3, (nv, 1)) * np.ones((nv, d))).astype(_F32))
    r2, q2 = rows.copy(), q.copy()  # (the queries stay normal: a product of two denormals is below fp32 altogether)
    r2[::3] *= _F32(1e-39)  # denormal throughout: the SCORES are denormal, which only an absolute term can bound
    r2[1::7, ::2] *= _F32(1e-41)
    out["denormal"] = (r2, q2)
    r3, q3 = (rows * _F32(1e-3)).astype(_F32), (q * _F32(1e-3)).astype(_F32)
    r3[::4, 1] = _F32(3.4e38)
    q3[::3, 2] = _F32(-3.39e38)
    out["clamp"] = (r3, q3)
    return out


def _band(c, metric, bf16):
    """(value, band) [n, gbn]: the library's documented bound of the selection score."""
    v, sab = c.scores(metric)
    g, un = _F64(G.lib_gamma(c.pitch)), _F64(G.lib_under(c.pitch))
    cn = c.cn.astype(_F64)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        if not bf16:
            return v, g * sab + un if metric == COS else g * (2.0 * sab + cn) + 2.0 * un
        nc = np.sqrt((c.rows.astype(_F64) ** 2).sum(axis=1))[:, None]
        nq = np.sqrt((c.qblock.astype(_F64) ** 2).sum(axis=1))[None, :]
        b = _F64(G.lib_eps_dot(c.pitch, True)) * nc * nq + _F64(G.lib_sel(c.pitch, True)[2]) * (nc + nq) + un
        return v, b if metric == COS else 2.0 * b + g * cn


@pytest.mark.parametrize("family", G.FAMILIES, ids=[G.FAMILY_NAME[f] for f in G.FAMILIES])
@pytest.mark.parametrize("metric", METRICS, ids=["ip", "l2"])
def test_float_corpora_stay_inside_the_documented_bounds(family, metric):
    """(a) float corpora against float64, inside the library's own bounds and nothing more; and tau_margin_kernel's margin is
    at least twice the largest error observed, for every live query.  (The margin is not looked at on the clamp corpus: its
    rows beyond the bf16 maximum have an infinite squared norm, the statistic the global margin is computed from, and the
    library takes the per-group bounds for such data.)"""
    ct = 2
    worst = {}
    for width in WIDTHS[family]:
        rng = np.random.default_rng(500 + width)
        n, d, nv = _rows_of(family), _dims(family, width), 64 * ct - 5
        for name, (rows, q) in _float_corpora(rng, n, d, nv).items():
            c = Case(family, width, ct, rows, q, "huge")
            value, band = _band(c, metric, family != G.FP32)
            cap = c.n + 3
            cand, count = c.run(1, metric, None, grid=2, tau=_tau_dump(c), cap=cap)
            r = G.check_dump(cand, count, c.gbn, cap, c.n, c.nv, value=value, band=band)
            worst[name] = max(worst.get(name, 0.0), r)
            # the global margin: >= twice the largest error of any row against this query
            if np.isfinite(c.cn).all() and np.isfinite(value[:, :c.nv]).all():
                fl = G.lib_sel(c.pitch, family != G.FP32)[2]
                after = G.tau_margin(np.zeros(c.nv, _F32), c.qblock[:c.nv], c.nv, c.cn.max(), metric, family != G.FP32, fl, G.lib_under(c.pitch))
                err = np.abs(G.dump_values(cand, count, c.gbn, cap, c.n, c.nv) - value[:, :c.nv]).max(axis=0)
                assert (-after.astype(_F64) >= 2.0 * err).all(), (name, np.flatnonzero(-after.astype(_F64) < 2.0 * err)[:4])
            else:
                assert name == "clamp"
    print(f"\nworst |error| / bound, {G.FAMILY_NAME[family]} {'l2' if metric else 'ip'}: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("combo", [cb for cb in COMBOS if cb[3]], ids=[i for cb, i in zip(COMBOS, IDS) if cb[3]])
def test_group_bounds(combo):
    """(d) a group whose gmax is +inf: PHASE 1 appends every row of it with a +inf key for the columns with a finite threshold
    only, PHASE 0 reports 0 for it; on a float corpus with one group 100 x the rest, score -+ bound brackets the float64 score
    (PHASE 0's reported lower bounds stay below the group's best true score)."""
    family, ct, metric, _ = combo
    width = WIDTHS[family][1]
    c = _int_case(family, width, ct, 11, specials=False)
    gbk = dict(c.groupb(), under_abs=P2["under_abs"])
    gbk["gmax"] = gbk["gmax"].copy()
    gbk["gmax"][3] = np.inf
    exact = c.scores(metric)[0].astype(_F32)
    bound = _p2_bound(gbk, metric)
    tau = np.full(c.gbn, np.inf, _F32)
    tau[:c.nv] = np.sort(exact[:, :c.nv], axis=0)[-25]
    S = np.zeros((c.tiles * c.T, c.gbn), _F32)
    S[:c.n] = exact
    cap = c.n
    blank_c = np.full(c.gbn * cap + G.GUARD, G.SENT_KEY, _U64)
    blank_n = np.concatenate([np.zeros(c.gbn, _U32), np.full(G.GUARD, G.SENT_U32, _U32)])
    ginf = ~(gbk["gmax"] < np.inf)
    mc, mn = G.model_phase1(S, c.n, family, c.tiles, 1, 0, tau, cap, blank_c, blank_n, bound=bound, ginf=ginf)
    want = [G.split_cand(mc, mn, c.gbn, cap)[0][col, :mn[col]] for col in range(c.gbn)]
    assert all((G.key_ord(w) == G.f2ord(G.INF32)[0]).sum() == 64 for w in want[:c.nv]) and all(w.size == 0 for w in want[c.nv:])
    cand, count = c.run(1, metric, gbk, grid=2, tau=tau, cap=cap)
    G.check_keep(cand, count, c.gbn, cap, want)
    blank = np.full(c.gbn * c.RW * c.tiles + G.GUARD, G.SENT_KEY, _U64)
    got = c.run(0, metric, gbk, grid=2)
    wanth = G.model_phase0(S, c.n, family, c.tiles, 1, 0, blank, bound=bound)
    assert (wanth[:c.gbn * c.RW * c.tiles].reshape(c.gbn, -1)[:c.nv, 3] == 0).all()
    G.check_halfmax(got, wanth)
    # float corpus, one group 100 x the rest, the library's own coefficients
    rng = np.random.default_rng(12)
    rows, q = rng.standard_normal((c.n, c.d)).astype(_F32), rng.standard_normal((c.nv, c.d)).astype(_F32)
    rows[128:192] *= _F32(100.0)
    f = Case(family, width, ct, rows, q)
    bf16 = family != G.FP32
    eps, gam, fl = G.lib_sel(f.pitch, bf16)
    cn = f.cn
    gmax = G.group_max_dev(cn, f.n)[:(f.n + 63) // 64]
    qn = G.query_norm(f.qblock, f.nv, f.gbn)[:f.gbn]
    un = G.lib_under(f.pitch)
    lib = dict(gmax=gmax, qn=qn, eps=eps, gam=gam, floor_abs=fl, under_abs=un)
    truth = f.scores(metric)[0]
    cap = f.n + 3
    cand, count = f.run(1, metric, lib, grid=2, tau=_tau_dump(f), cap=cap)
    G.check_guards(cand, count, f.gbn, cap)
    b = np.minimum(G.group_bound(gmax, qn, eps, gam, fl, metric, under_abs=un), G.group_bound(gmax, qn, eps, gam, fl, metric, contract=True, under_abs=un))
    v = G.dump_values(cand, count, f.gbn, cap, f.n, f.nv)
    assert not np.isnan(v).any()
    ratio = G.check_bounds(v, b[np.arange(f.n) >> 6][:, :f.nv], truth[:, :f.nv])
    print(f"\ngroup bounds {IDS[COMBOS.index(combo)]}: worst |error| / bound {ratio:.4f}")
    # PHASE 0 reports lower bounds of each group's best true score
    hm = f.run(0, metric, lib, grid=2)[:f.gbn * f.RW * f.tiles].reshape(f.gbn, -1)
    for g in range((f.n + 63) // 64):
        best = truth[g * 64:min(g * 64 + 64, f.n), :f.nv].max(axis=0)
        assert (G.ord2f(G.key_ord(hm[:f.nv, g])).astype(_F64) <= best).all(), g


def test_conversions_are_bit_equal_to_round_to_nearest_even_with_the_clamp():
    """(e) rows_to_bf16_kernel and queries_to_bf16_kernel."""
    rng = np.random.default_rng(20)
    n, pitch, pitch16 = 300, 100, 128
    rows = (rng.standard_normal((n, pitch)) * 10.0 ** rng.integers(-3, 4, (n, pitch))).astype(_F32)
    rows[0, :12] = [3.39e38, 3.4028235e38, -3.4e38, np.inf, -np.inf, np.nan, -0.0, 1e-40, -1e-45, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.3895314e38]
    rows[7] = rows[0]
    rows[n - 1, pitch - 12:] = rows[0, :12]
    mid = (1 + 2.0 ** -8 * rng.integers(0, 2, (n, 8)) * 2 + 2.0 ** -8).astype(_F32)  # exact ties: to even
    rows[:, 20:28] = mid
    blank = np.full((n + 4, pitch16), G.SENT_U16, _U16)
    for r0, grid in ((0, 0), (7, 1), (n, 1), (n - 1, 3)):
        got = G.rows_to_bf16(rows, r0, n, pitch16, blank, grid)
        G.check_bf16(got, G.rows_to_bf16_model(rows, r0, n, pitch16, blank))
    q = rows[:130].copy()
    for nv, kpad, gbn, live, blocks, grid in ((123, 128, 128, 128, 1, 0), (3, 128, 128, 1, 3, 0), (130, 64, 256, 256, 1, 2), (3, 192, 128, 1, 3, 1)):
        got = G.queries_to_bf16(q, nv, kpad, gbn, live, blocks, grid)
        assert (got[blocks * gbn * kpad:] == G.SENT_U16).all()
        G.check_bf16(got[:blocks * gbn * kpad].reshape(blocks, gbn, kpad), G.queries_to_bf16_model(q, nv, kpad, gbn, live, blocks))


def test_the_small_kernels_behind_the_margins():
    """(e) cn_stats_kernel, group_max_kernel, query_norm_kernel, tau_margin_kernel."""
    rng = np.random.default_rng(21)
    for n in (1, 64, 640, 1381, 5000):
        cn = (rng.standard_normal(n) ** 2 * 50).astype(_F32)
        if n > 100:
            cn[3], cn[70], cn[n - 1], cn[200] = np.nan, np.inf, np.nan, 1e9
            cn[128:192] = np.nan  # a group of removed rows
        for grid in (0, 1):
            st = G.cn_stats(cn, n, grid)
            assert st[3] == G.SENT_U32
            assert st[0:1].view(_F32)[0] == np.nanmax(cn)
            fin = cn[cn < np.inf]
            assert st[2] == fin.size
            s64 = fin.astype(_F64).sum()
            assert abs(_F64(st[1:2].view(_F32)[0]) - s64) <= G.gamma(max(n, 2)) * s64
            gm = G.group_max_dev(cn, n, grid)
            groups = (n + 63) // 64
            assert np.array_equal(gm[:groups], G.group_max(cn, n)) and (gm[groups:].view(_U32) == G.SENT_F32_BITS).all()
    for d in (12, 52, 128, 200):
        nv, gbn = 59, 64
        q = (rng.standard_normal((nv, d)) * 10.0 ** rng.integers(-2, 3, (nv, 1))).astype(_F32)
        qn = G.query_norm(q, nv, gbn)
        true = np.sqrt((q.astype(_F64) ** 2).sum(axis=1))
        mirror = G.query_norm_mirror(q, nv, gbn)
        assert (qn[:nv].astype(_F64) >= true).all() and (qn[nv:gbn] == 0).all() and (qn[gbn:].view(_U32) == G.SENT_F32_BITS).all()
        assert (np.abs(qn[:nv].astype(_F64) - mirror[:nv]) <= G.gamma(d) * mirror[:nv]).all()
        qq = q.copy()
        qq[5, 1] = np.nan
        for metric in METRICS:
            for bf16 in (0, 1):
                fl, un = G.lib_sel(d, bf16)[2], G.lib_under(d)
                cmax = _F32(37.5)
                tau = rng.standard_normal(nv + 4).astype(_F32)
                tau[2] = -np.inf
                got = G.tau_margin(tau, qq, nv, cmax, metric, bf16, fl, un)
                assert got[2] == -np.inf and got[5] == -np.inf and np.array_equal(got[nv:], tau[nv:])
                # The mirror is the kernel's float32 arithmetic as a function of s = sum q^2, monotone in s, and the device's s
                # is within gamma(d) of the exact sum: tau - margin lies between the mirror's answers at s (1 + gamma(d)) and
                # s (1 - gamma(d)).  Apart from gamma: the compiler may fuse the kernel's two multiply-add pairs (2 eps cq +
                # gamma cmax, margin 1.01 + floor term), each then rounds once where the mirror rounds twice -- 2^-24 of the
                # margin each, 2^-23 together -- and the bounds of tau - margin are rounded outwards to float32.
                s = (qq.astype(_F64) ** 2).sum(axis=1)
                fin = np.isfinite(s) & (tau[:nv] > -np.inf)
                m_hi = G.tau_margin_mirror(tau[:nv], G.f32_up(s * (1.0 + G.gamma(d))), cmax, d, metric, bf16, fl, un)[1].astype(_F64)
                m_lo = G.tau_margin_mirror(tau[:nv], G.f32_down(s * (1.0 - G.gamma(d))), cmax, d, metric, bf16, fl, un)[1].astype(_F64)
                lo = G.f32_down(tau[:nv].astype(_F64)[fin] - m_hi[fin] * (1.0 + 2.0 ** -23))
                hi = G.f32_up(tau[:nv].astype(_F64)[fin] - m_lo[fin] * (1.0 - 2.0 ** -23))
                assert fin.sum() == nv - 2 and (m_lo[fin] > 0).all()
                assert ((lo <= got[:nv][fin]) & (got[:nv][fin] <= hi)).all(), (d, metric, bf16)


@pytest.mark.parametrize("family", G.FAMILIES, ids=[G.FAMILY_NAME[f] for f in G.FAMILIES])
@pytest.mark.parametrize("metric", METRICS, ids=["ip", "l2"])
@pytest.mark.parametrize("bounds", ["global", "groups"])
def test_the_two_phases_together_lose_no_true_neighbour(family, metric, bounds):
    """(f) PHASE 0 -> the k-th largest key on the host -> tau_margin_kernel (global margin) -> PHASE 1 with cap = n_rows:
    every row whose float64 score reaches the float64 k-th best is among the candidates."""
    if bounds == "groups" and not G.has_instance_py(family, 2, metric, 1):
        assert family == G.FP32 and metric == COS  # exact scores: nothing to bound
        return
    ct, k = 2, 10
    width = WIDTHS[family][2]
    bf16 = family != G.FP32
    for outlier in (False, True):
        rng = np.random.default_rng(30 + outlier)
        n, d, nv = _rows_of(G.BF16), _dims(family, width), 64 * ct - 5
        rows, q = rng.standard_normal((n, d)).astype(_F32), rng.standard_normal((nv, d)).astype(_F32)
        if outlier:
            rows[256:320] *= _F32(1000.0)
        c = Case(family, width, ct, rows, q)
        eps, gam, fl = G.lib_sel(c.pitch, bf16)
        un = G.lib_under(c.pitch)
        gbk = dict(gmax=G.group_max_dev(c.cn, c.n)[:(c.n + 63) // 64], qn=G.query_norm(c.qblock, c.nv, c.gbn)[:c.gbn], eps=eps, gam=gam,
                   floor_abs=fl, under_abs=un) if bounds == "groups" else None
        hm = c.run(0, metric, gbk, grid=2)[:c.gbn * c.RW * c.tiles].reshape(c.gbn, -1)
        kth = np.sort(hm, axis=1)[:, -k]
        assert (kth[:c.nv] != 0).all()
        tau = np.full(c.gbn, np.inf, _F32)
        tau[:c.nv] = G.ord2f(G.key_ord(kth[:c.nv]))
        if bounds == "global" and (bf16 or metric == L2):
            tau[:c.nv] = G.tau_margin(tau[:c.nv], c.qblock[:c.nv], c.nv, c.cn.max(), metric, bf16, fl, un)
        cand, count = c.run(1, metric, gbk, grid=2, tau=tau, cap=c.n)
        cb, cnt = G.check_guards(cand, count, c.gbn, c.n)
        truth = c.scores(metric)[0]
        if metric == L2:  # the true ranking value: 2 c.q - |c|^2 with the float64 norm
            truth = 2.0 * (c.rows.astype(_F64) @ c.qblock.astype(_F64).T) - (c.rows.astype(_F64) ** 2).sum(axis=1)[:, None]
        elif not bf16 and bounds == "global":
            # fp32 inner product: no margin, the tiles' own fp32 scores ARE the ranking -- the reference is their k-th best
            dump = c.run(1, metric, None, grid=2, tau=_tau_dump(c), cap=c.n)
            truth = G.dump_values(*dump, c.gbn, c.n, c.n, c.nv)
            assert not np.isnan(truth).any()
        for col in range(c.nv):
            need = np.flatnonzero(truth[:, col] >= np.sort(truth[:, col])[-k])
            have = G.key_row(cb[col, :cnt[col]])
            assert np.isin(need, have).all(), (col, outlier, np.setdiff1d(need, have))
            assert cnt[col] <= c.n


def test_the_harness_refuses_what_would_leave_the_arrays():
    c = _int_case(G.BF16, 8, 2, 1)
    tau = _tau_dump(c)
    ok = dict(queries=None, qb16=c.qb16, qb_pitch16=c.qb_pitch16, tau=tau, cap=c.n)
    G.tiles(1, G.BF16, 2, COS, c.dev_rows, c.n, c.pitch4, c.tiles, grid=2, **ok)
    with pytest.raises(ValueError):  # the bf16 tiles read whole tiles: rows short of the last tile's end
        G.tiles(1, G.BF16, 2, COS, c.dev_rows[:c.n], c.n, c.pitch4, c.tiles, grid=2, **ok)
    with pytest.raises(ValueError):  # a tile beyond the pad rows
        G.tiles(1, G.BF16, 2, COS, c.dev_rows, c.n, c.pitch4, c.tiles + 1, grid=2, **ok)
    with pytest.raises(ValueError):  # tile_stride: the last tile read is (num_tiles - 1) * stride
        G.tiles(1, G.BF16, 2, COS, c.dev_rows, c.n, c.pitch4, c.tiles, tile_stride=2, grid=2, **ok)
    with pytest.raises(ValueError):  # the query block's pitch short of the pair of chunks the kernel walks
        G.tiles(1, G.BF16, 2, COS, c.dev_rows, c.n, c.pitch4, c.tiles, grid=2, **dict(ok, qb_pitch16=4))
    with pytest.raises(ValueError):  # fewer than 64 CT query rows
        G.tiles(1, G.BF16, 2, COS, c.dev_rows, c.n, c.pitch4, c.tiles, grid=2, **dict(ok, qb16=c.qb16[:100]))
    with pytest.raises(ValueError):  # cand shorter than [64 CT][cap]
        G.tiles(1, G.BF16, 2, COS, c.dev_rows, c.n, c.pitch4, c.tiles, grid=2, cand_len=c.gbn * c.n - 1, **ok)
    with pytest.raises(ValueError):  # halfmax shorter than [64 CT][RW num_tiles]
        G.tiles(0, G.BF16, 2, COS, c.dev_rows, c.n, c.pitch4, c.tiles, grid=2, qb16=c.qb16, qb_pitch16=c.qb_pitch16,
                halfmax_len=c.gbn * c.RW * c.tiles - 1)
    with pytest.raises(ValueError):  # L2 without cn[n_rows]
        G.tiles(1, G.BF16, 2, L2, c.dev_rows, c.n, c.pitch4, c.tiles, grid=2, cn=c.cn[:-1], **ok)
    with pytest.raises(ValueError):  # group bounds without gmax[ceil(n_rows / 64)]
        G.tiles(1, G.BF16, 2, COS, c.dev_rows, c.n, c.pitch4, c.tiles, grid=2, gmax=np.zeros(c.n // 64, _F32), qn=np.zeros(c.gbn, _F32), **ok)
    with pytest.raises(ValueError):  # n_rows == 0
        G.tiles(1, G.BF16, 2, COS, c.dev_rows, 0, c.pitch4, 1, grid=2, **ok)
    with pytest.raises(ValueError):  # no instance: bf16 tiles with CT = 1
        G.tiles(1, G.BF16, 1, COS, c.dev_rows, c.n, c.pitch4, c.tiles, grid=2, **ok)
    with pytest.raises(ValueError):  # the shadow has no K tail: its pitch is whole chunk pairs
        G.tiles(1, G.SHADOW, 2, COS, c.dev_rows, c.n, 8, c.tiles, grid=2, **ok)
    f = _int_case(G.FP32, 13, 1, 2)
    with pytest.raises(ValueError):  # fp32 tiles: fewer than n_rows rows
        G.tiles(1, G.FP32, 1, COS, f.dev_rows[:-1], f.n, f.pitch4, f.tiles, grid=2, queries=f.qblock, tau=_tau_dump(f), cap=f.n)
    with pytest.raises(ValueError):
        G.tiles(1, G.FP32, 1, COS, f.dev_rows, f.n, f.pitch4, f.tiles, grid=2, queries=f.qblock[:-1], tau=_tau_dump(f), cap=f.n)
    with pytest.raises(ValueError):
        G.rows_to_bf16(np.zeros((4, 8), _F32), 0, 5, 8, np.zeros((5, 8), _U16))
    with pytest.raises(ValueError):
        G.queries_to_bf16(np.zeros((4, 8), _F32), 5, 64, 128, 128, 1)
    with pytest.raises(ValueError):
        G.group_max_dev(np.zeros(100, _F32), 100, gmax_len=1)


def test_zz_every_instance_the_picker_can_return_was_launched():
    """Runs last and needs the whole file to have run before it: a returned instance that no case launched fails this test."""
    want = _all_instances()
    assert len(want) == 82
    assert COVERED >= set(want), ("tile instances not launched in this session", sorted(want[fn] for fn in set(want) - COVERED))
    print(f"\ntile instances launched: {len(COVERED & set(want))} of 82 (41 per phase: 18 fp32, 16 bf16, 7 shadow)")
