"""ctypes loader of tests/kernel_harness/libgemm_harness.so (built by ``make -C wdbx-py_amd/csrc all``), numpy restatements
of what kernels_tiles.h documents for the fp32 and bf16 tile kernels, and the property checkers of
tests/test_gpu_gemm_kernels.py.

The harness launches the library's own ``gemm_topk_kernel`` / ``gemm_bf16w8_kernel`` instance (taken from the picker behind
the kernels), ``rows_to_bf16_kernel``, ``queries_to_bf16_kernel``, ``cn_stats_kernel``, ``group_max_kernel``,
``query_norm_kernel`` and ``tau_margin_kernel`` on arrays the caller hands it.

Restated here: the 32x32 C layout (query = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)), tiles of 64 RW rows and
their wave groups, ``to_bf16_sel`` (round to nearest even, a finite value never becomes infinite, NaN and infinities are
kept), the layouts of the two conversions, the keys, and the float32 arithmetic of the GROUPB bound, of
``tau_margin_kernel`` and of ``query_norm_kernel``.

The checkers are plain numpy and never look at the code under test.  tests/test_gemm_checkers.py feeds them the models of
this file on the CPU, and a list of deliberately wrong models that they must reject."""
import ctypes as C
from pathlib import Path

import numpy as np

from rank_harness import METRIC_COSINE, METRIC_L2, f2ord, key_ord, key_row, make_keys, ord2f  # noqa: F401  (re-exported)
from select_harness import GUARD, SENT_KEY, SENT_U32, gamma  # noqa: F401  (re-exported)

ROOT = Path(__file__).resolve().parent.parent
LIBRARY = ROOT / "tests" / "kernel_harness" / "libgemm_harness.so"

_U16, _U32, _U64, _F32, _F64, _I64 = np.uint16, np.uint32, np.uint64, np.float32, np.float64, np.int64
FP32, BF16, SHADOW = 0, 1, 2  # the GEMM_* families of kernels_tiles.h
FAMILIES = (FP32, BF16, SHADOW)
FAMILY_NAME = {FP32: "fp32", BF16: "bf16", SHADOW: "shadow"}
TILE_PAD_ROWS = 256
SENT_U16 = 0xABAB
SENT_F32_BITS = 0x7FC12345
INF32 = _F32(np.inf)


def tile_rows(family):
    return 128 if family == FP32 else 256


def wave_groups(family):
    """RW: 64-row wave groups per tile."""
    return tile_rows(family) // 64


# --------------------------------------------------------------------------- #
# the picker, restated (the GPU suite compares it with what the library answers)
# --------------------------------------------------------------------------- #
def ktail_py(family, pitch4):
    return family != SHADOW and pitch4 % (8 if family == FP32 else 16) != 0


def has_instance_py(family, ct, metric, groupb):
    if family != FP32 and ct < 2:
        return False  # the bf16 tiles need a query block of at least 128
    if family == FP32 and groupb and metric == METRIC_COSINE:
        return False  # exact inner-product tiles: nothing to bound
    if family == SHADOW and groupb and metric == METRIC_L2 and ct == 4:
        return False  # does not fit the register file
    return True


def lds_bytes_py(family, ct):
    if family == FP32:
        return (2 * 128 + 2 * 64 * ct) * 36 * 4 + 4 * 64 * 4
    bk = 64 if family == SHADOW else 32
    return (2 * 256 + 2 * 64 * ct) * (bk * 2 + 16) + 8 * 64 * 4


def per_cu_py(family, ct):
    return 1 if family != FP32 or ct == 4 else 2


def kchunks_bf16(pitch4):
    """Chunks of 8 pieces the 8-wave tile walks per row: rounded up to a pair."""
    return ((pitch4 + 7) // 8 + 1) // 2 * 2


def qb_pitch16_py(family, pitch):
    """The library's bf16 query block pitch in 16-byte pieces for fp32 rows of `pitch` floats."""
    ring = 128 if family == SHADOW else 64
    return (pitch + ring - 1) // ring * ring // 8


# --------------------------------------------------------------------------- #
# float32 arithmetic, restated
# --------------------------------------------------------------------------- #
def fmaf(a, b, c):
    """round_f32(a * b + c) with ONE rounding, for float32 arrays: the product is exact in float64, the sum is rounded to odd
    there (TwoSum), so the final rounding to float32 sees the exact value's side of every tie."""
    a, b, c = (np.asarray(x, _F32).astype(_F64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = np.atleast_1d(s).view(np.int64).copy()
        fix = np.atleast_1d(np.isfinite(s) & (err != 0) & ((bits & 1) == 0))
        up = np.atleast_1d((err > 0) == (s > 0))  # away from zero when the lost part has the sum's sign
        bits = np.where(fix, np.where(up, bits + 1, bits - 1), bits)
        return bits.view(_F64).reshape(np.shape(s)).astype(_F32)


def lib_gamma(pitch):
    """gamma as tau_margin_kernel and enqueue_search_gemm compute it, in float32: 1.02 nu / (1 - nu), nu = (pitch + 18) u."""
    nu = _F32(pitch + 18) * _F32(5.9604645e-08)
    return _F32(1.02) * nu / (_F32(1.0) - nu)


def lib_eps_dot(pitch, bf16):
    """tau_margin_kernel's eps_dot."""
    return lib_gamma(pitch) + (_F32(1.05) * _F32(0.0078125) if bf16 else _F32(0.0))


def lib_under(pitch):
    """sel_under of enqueue_search_gemm: (pitch + 18) 2^-149, the absolute error that gradual underflow adds to a dot product
    (an fma whose result is denormal rounds to a multiple of 2^-149)."""
    return _F32(np.ldexp(_F64(pitch + 18), -149))


def lib_sel(pitch, bf16):
    """(sel_eps, sel_gam, sel_floor) of enqueue_search_gemm."""
    g = lib_gamma(pitch)
    return ((g + (_F32(1.05) * _F32(0.0078125) if bf16 else _F32(0.0))) * _F32(1.0102), g * _F32(1.01),
            _F32(7.5e-37) * np.sqrt(_F32(pitch)) if bf16 else _F32(0.0))


def group_bound(gmax, qn, eps, gam, floor_abs, metric, contract=False, mutant=None, under_abs=0.0):
    """bound[g, q] of the GROUPB epilogue in float32: fmaf(bscale, qn[q], bconst), bscale = two (eps sqrt(g) + floor_abs),
    bconst = ([gam g] + two floor_abs sqrt(g)) + two under_abs.  contract: the two sums as fused multiply-adds (what a
    compiler may make of them); with eps, gam and floor_abs powers of two both forms give the same bits (two under_abs is
    exact, so the last sum rounds once either way)."""
    g = np.asarray(gmax, _F32)
    eps, gam, fl, un = _F32(eps), _F32(gam), _F32(floor_abs), _F32(under_abs)
    l2 = metric == METRIC_L2
    two = _F32(2.0 if l2 else 1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        sg = np.sqrt(g)
        if contract:
            bscale = two * fmaf(np.full_like(sg, eps), sg, np.full_like(sg, fl))
            bconst = fmaf(np.full_like(sg, two * fl), sg, gam * g if l2 else np.zeros_like(g))
        else:
            bscale = two * (eps * sg + fl)
            bconst = (gam * g if l2 else np.zeros_like(g)) + two * fl * sg
        bconst = bconst + two * un
        out = fmaf(bscale[:, None], np.asarray(qn, _F32)[None, :], bconst[:, None])
    if mutant == "bound_halved":
        out = out * _F32(0.5)
    return out


def query_norm_mirror(q, nv, gbn):
    """qn of query_norm_kernel up to the order of its sum: sqrtf(sum q^2) * 1.0001f in float32 (the sum in float64, rounded
    once), 0 for the padded queries."""
    q = np.asarray(q, _F32)
    out = np.zeros(gbn, _F32)
    s = (q[:nv].astype(_F64) ** 2).sum(axis=1).astype(_F32)
    out[:nv] = np.sqrt(s) * _F32(1.0001)
    return out


def tau_margin_mirror(tau, s, cmax, pitch, metric, bf16, floor_abs, under_abs=0.0):
    """tau_margin_kernel in float32 given s = the device's sum q^2 (float32).  Every step is monotone in s."""
    tau, s, cmax, fl = np.asarray(tau, _F32).copy(), np.asarray(s, _F32), _F32(cmax), _F32(floor_abs)
    g = lib_gamma(pitch)
    eps_dot = g + (_F32(1.05) * _F32(0.0078125) if bf16 else _F32(0.0))
    l2 = metric == METRIC_L2
    with np.errstate(invalid="ignore", over="ignore"):
        cq = np.sqrt(cmax * s) * _F32(1.0001)
        margin = _F32(2.0) * (_F32(2.0) * eps_dot * cq + g * cmax) if l2 else _F32(2.0) * eps_dot * cq
        margin = margin * _F32(1.01) + _F32(2.0) * _F32(2.0 if l2 else 1.0) * fl * (np.sqrt(cmax) + np.sqrt(s))
        margin = margin + _F32(2.0) * _F32(2.0 if l2 else 1.0) * _F32(under_abs)
        margin = np.where(np.isnan(margin), INF32, margin).astype(_F32)
        return np.where(tau > -INF32, tau - margin, tau).astype(_F32), margin


# --------------------------------------------------------------------------- #
# bf16
# --------------------------------------------------------------------------- #
BF16_MAX = _F32(3.3895313892515355e38)


def to_bf16_sel(x, mutant=None):
    """float32 -> bf16 bit patterns: round to nearest even; a finite value beyond the largest finite bf16 is clamped to it;
    NaN stays NaN (quiet), infinities stay infinite."""
    x = np.asarray(x, _F32)
    if mutant != "no_clamp":
        with np.errstate(invalid="ignore"):
            x = np.where(np.isfinite(x), np.clip(x, -BF16_MAX, BF16_MAX), x).astype(_F32)
    u = x.view(_U32).astype(_U64)
    if mutant == "truncate":
        r = u >> _U64(16)
    else:
        r = (u + _U64(0x7FFF) + ((u >> _U64(16)) & _U64(1))) >> _U64(16)
    r = np.where(np.isnan(x), (u >> _U64(16)) | _U64(0x40), r)
    return r.astype(_U16)


def bf16_to_f32(bits):
    return (np.asarray(bits, _U16).astype(_U32) << _U32(16)).view(_F32)


def rows_to_bf16_model(rows, r0, n, pitch16, out, mutant=None):
    """rows [n, pitch] -> out [*, pitch16] bf16 bits: rows r0 .. n - 1 converted and zero padded, the others untouched."""
    out = out.copy()
    pitch = rows.shape[1]
    out[r0:n, :pitch] = to_bf16_sel(rows[r0:n], mutant)
    out[r0:n, pitch:] = 0
    return out


def queries_to_bf16_model(q, nv, kpad, gbn, live, blocks, mutant=None):
    """-> [blocks, gbn, kpad] bf16 bits: block b holds queries b live .. b live + live - 1 in its first rows, zeros elsewhere."""
    q = np.asarray(q, _F32)
    pitch = q.shape[1]
    out = np.zeros((blocks, gbn, kpad), _U16)
    for b in range(blocks):
        for r in range(min(live, gbn)):
            src = b * live + r
            if src < nv:
                out[b, r, :min(pitch, kpad)] = to_bf16_sel(q[src, :kpad], mutant)
    return out


def check_bf16(got, want):
    """Bit-equal bf16 arrays; where the model holds a NaN any NaN will do."""
    got, want = np.asarray(got, _U16), np.asarray(want, _U16)
    assert got.shape == want.shape
    nan_w = ((want & 0x7F80) == 0x7F80) & ((want & 0x7F) != 0)
    nan_g = ((got & 0x7F80) == 0x7F80) & ((got & 0x7F) != 0)
    assert np.array_equal(nan_w, nan_g), "a NaN appeared or was lost in the bf16 conversion"
    bad = np.flatnonzero((got != want).ravel() & ~nan_w.ravel())
    assert bad.size == 0, ("bf16 bits differ from round-to-nearest-even with the finite clamp", bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


# --------------------------------------------------------------------------- #
# corpora and truth
# --------------------------------------------------------------------------- #
def int_corpus(rng, n, d, nq):
    """Small integers in [-4, 4] as fp32: exact in bf16, every partial sum far below 2^24."""
    assert d <= 3200
    return rng.integers(-4, 5, (n, d)).astype(_F32), rng.integers(-4, 5, (nq, d)).astype(_F32)


def ieee_scores(rows, q, metric, cn=None, drop_last_quad=False):
    """[n, nq] float64: c.q (cosine) or 2 c.q - cn (L2) with IEEE's answers on infinities and NaNs (inf * 0 = NaN), from the
    fp32 operands; and S = sum |c_i q_i|.  drop_last_quad: the wrong model that forgets a row's last four elements."""
    r, qq = np.asarray(rows, _F32).astype(_F64), np.asarray(q, _F32).astype(_F64)
    if drop_last_quad:
        r, qq = r[:, :-4], qq[:, :-4]
    odd = ~np.isfinite(r).all(axis=1)
    fin = np.where(odd[:, None], 0.0, r)
    with np.errstate(invalid="ignore", over="ignore"):
        dot, sab = fin @ qq.T, np.abs(fin) @ np.abs(qq).T
        for i in np.flatnonzero(odd):
            dot[i] = (r[i][None, :] * qq).sum(axis=1)
            sab[i] = np.abs(r[i][None, :] * qq).sum(axis=1)
        if metric == METRIC_L2:
            dot = 2.0 * dot - np.asarray(cn, _F32).astype(_F64)[:, None]
    return dot, sab


def sqnorm32(rows):
    """Squared norms as float32 (exact on the integer corpus)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(rows, _F32).astype(_F64) ** 2).sum(axis=1).astype(_F32)


def group_max(cn, n):
    """gmax of group_max_kernel: fmaxf from 0 over the group's norms (NaN skipped)."""
    groups = (n + 63) // 64
    pad = np.full(groups * 64, -1.0, _F32)
    pad[:n] = cn[:n]
    with np.errstate(invalid="ignore"):
        return np.fmax(np.fmax.reduce(pad.reshape(groups, 64), axis=1), _F32(0.0)).astype(_F32)


# --------------------------------------------------------------------------- #
# the documented layout and epilogue
# --------------------------------------------------------------------------- #
def c_layout_row(r, lane, mutant=None):
    """Row inside a 32-row block of accumulator register r of a lane (32x32 MFMA C layout); its query is lane & 31."""
    return (r & 3) + 8 * (r >> 2) + (0 if mutant == "no_lane_half" else 4 * (lane >> 5))


def walk_rows(family, num_tiles, tile_stride, mutant=None):
    """[num_tiles, RW, 2, 2, 16] row numbers: tile, wave group rh, row tile rt, lane half lh, register r."""
    T, RW = tile_rows(family), wave_groups(family)
    t, rh, rt, lh, r = np.meshgrid(np.arange(num_tiles), np.arange(RW), np.arange(2), np.arange(2), np.arange(16), indexing="ij")
    return t * tile_stride * T + rh * 64 + rt * 32 + c_layout_row(r, lh * 32, mutant)


def register_group_of(row):
    """(first row of the 32-row block, lane half, position among the 16 registers) of a row."""
    blk, o = row - row % 32, row % 32
    lh = (o >> 2) & 1
    return blk, lh, (o & 3) + 4 * (o >> 3)


def model_phase0(S, n_rows, family, num_tiles, tile_stride, live, halfmax, bound=None, mutant=None):
    """PHASE 0 on selection scores S [rows covered, gbn] float32 -> halfmax [gbn, RW num_tiles] (copied, live columns written):
    make_key(max over the wave group's rows < n_rows - bound, ht), 0 when that is -inf or NaN."""
    RW = wave_groups(family)
    gbn = S.shape[1]
    flat = halfmax.copy()
    out = flat[:gbn * RW * num_tiles].reshape(gbn, RW * num_tiles)  # (a view: what lies behind is the guard)
    R = walk_rows(family, num_tiles, tile_stride, mutant)
    cols = np.arange(gbn) if live == 0 else np.arange(min(live, gbn))
    for t in range(num_tiles):
        for rh in range(RW):
            rows = R[t, rh].ravel()
            v = S[np.minimum(rows, S.shape[0] - 1)].astype(_F32)
            if mutant != "pad_row":
                v = np.where((rows < n_rows)[:, None], v, -INF32)
            with np.errstate(invalid="ignore"):
                m = np.fmax.reduce(np.vstack([np.full((1, gbn), -INF32), v]), axis=0).astype(_F32)
                if bound is not None:
                    g = min(t * tile_stride * tile_rows(family) + rh * 64, n_rows - 1) >> 6
                    m = (m - bound[g]).astype(_F32)
            m = np.where(np.isnan(m), -INF32, m)
            ht = t * RW + rh
            keys = np.where(m == -INF32, _U64(0), make_keys(f2ord(m + _F32(0.0)), np.full(gbn, ht)))
            out[cols, ht] = keys[cols]
    return flat


def model_phase1(S, n_rows, family, num_tiles, tile_stride, live, tau, cap, cand, count, bound=None, ginf=None, mutant=None):
    """PHASE 1 -> (cand, count) copies: every row < n_rows with S >= tau - bound appended in walk order (the device's order is
    arbitrary), count keeps counting past cap.  ginf [groups] marks the groups whose gmax is infinite: all their rows are
    appended with +inf keys for the columns with a finite threshold.  cand is flat: [gbn * cap] + guard."""
    gbn = S.shape[1]
    cand, count = cand.copy(), count.copy()
    R = walk_rows(family, num_tiles, tile_stride, mutant).ravel()
    grp = np.minimum(R - R % 64, n_rows - 1) >> 6
    V = S[np.minimum(R, S.shape[0] - 1)].astype(_F32)
    inside = np.ones_like(R, bool) if mutant == "pad_row" else R < n_rows
    for q in range(gbn):
        thr = _F32(tau[q]) if (live == 0 or q < live or mutant == "no_live_gate") else INF32
        with np.errstate(invalid="ignore"):
            cut = np.full(R.shape, thr, _F32) if bound is None else (thr - bound[grp, q]).astype(_F32)
            keep = ((V[:, q] > cut) if mutant == "gt_for_ge" else (V[:, q] >= cut)) & inside
        keys = make_keys(f2ord(V[:, q] + _F32(0.0)), R)
        if ginf is not None:
            gi = np.asarray(ginf, bool)[grp]
            keep = np.where(gi, inside & bool(thr < INF32), keep)
            keys = np.where(gi, make_keys(f2ord(np.full(R.shape, INF32)), R), keys)
        idx = np.flatnonzero(keep)
        for pos, i in enumerate(idx):
            if pos < cap or (mutant == "past_cap" and q * cap + pos < cand.size):
                cand[q * cap + pos] = keys[i]
        count[q] += idx.size
    return cand, count


# --------------------------------------------------------------------------- #
# checkers
# --------------------------------------------------------------------------- #
def split_cand(cand, count, gbn, cap):
    """(cand [gbn, cap], its guard, count [gbn], its guard) of the flat arrays a launch returns."""
    return cand[:gbn * cap].reshape(gbn, cap), cand[gbn * cap:], count[:gbn], count[gbn:]


def check_guards(cand, count, gbn, cap):
    c, cg, n, ng = split_cand(cand, count, gbn, cap)
    assert (cg == _U64(SENT_KEY)).all(), "a candidate was written behind the last query's buffer"
    assert (ng == _U32(SENT_U32)).all(), "a counter behind the block was written"
    for q in range(gbn):
        assert (c[q, min(int(n[q]), cap):] == _U64(SENT_KEY)).all(), ("a slot at or behind the count was written", q)
    return c, n


def check_dump(cand, count, gbn, cap, n_rows, live_cols, exact=None, value=None, band=None):
    """A PHASE 1 launch with tau = -inf for the live columns and cap >= n_rows.  Column q < live_cols holds one key per row
    below n_rows whose score is not NaN, each row once; the scores EQUAL exact[:, q] (float32 values, integer corpora) or lie
    within band[:, q] of value[:, q] (an infinite value: equal).  Every other column has count 0 and an untouched buffer.
    -> the worst |error| / band of the launch (0 for exact corpora)."""
    c, n = check_guards(cand, count, gbn, cap)
    assert (n[live_cols:] == 0).all(), "a padded or idle column counted a candidate"
    worst = 0.0
    ref = exact if exact is not None else value
    for q in range(live_cols):
        have = c[q, :int(n[q])]
        rows = key_row(have).astype(_I64)
        assert rows.size == np.unique(rows).size, ("a row was appended twice", q)
        assert (rows < n_rows).all(), ("a row at or beyond n_rows was appended", q, rows[rows >= n_rows][:4])
        want = np.flatnonzero(~np.isnan(ref[:n_rows, q]))
        assert np.array_equal(np.sort(rows), want), ("the rows of the dump are not the rows with a score", q,
                                                     np.setxor1d(rows, want)[:8])
        got = ord2f(key_ord(have)).astype(_F64)
        if exact is not None:
            bad = np.flatnonzero(have != make_keys(f2ord(exact[rows, q].astype(_F32) + _F32(0.0)), rows))
            assert bad.size == 0, ("scores differ from the integer reference", q, rows[bad[:4]], got[bad[:4]], exact[rows[bad[:4]], q])
        else:
            v, b = value[rows, q], band[rows, q]
            inf = np.isinf(v)
            assert np.array_equal(got[inf], v[inf]), ("an infinite score came out finite or with the other sign", q)
            err = np.abs(got[~inf] - v[~inf])
            assert np.isfinite(got[~inf]).all(), ("a finite score came out infinite", q)
            over = err > b[~inf]
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(err > 0, err / b[~inf], 0.0)
            worst = max(worst, float(ratio.max(initial=0.0)))
            assert not over.any(), ("a score outside the documented band", q, rows[~inf][over][:4], err[over][:4], b[~inf][over][:4])
            assert not (np.signbit(got) & (got == 0)).any(), "a negative zero in a key"
    return worst


def dump_values(cand, count, gbn, cap, n_rows, cols):
    """[n_rows, cols] float64: the score each row came out with in a PHASE 1 launch, NaN for a row that is absent."""
    c, n = split_cand(cand, count, gbn, cap)[::2]
    v = np.full((n_rows, cols), np.nan)
    for q in range(cols):
        keys = c[q, :min(int(n[q]), cap)]
        v[key_row(keys).astype(_I64), q] = ord2f(key_ord(keys))
    return v


def f32_down(x):
    """The largest float32 <= x (float64 array)."""
    x = np.asarray(x, _F64)
    y = x.astype(_F32)
    return np.where(y.astype(_F64) > x, np.nextafter(y, -INF32), y).astype(_F32)


def f32_up(x):
    """The smallest float32 >= x (float64 array)."""
    x = np.asarray(x, _F64)
    y = x.astype(_F32)
    return np.where(y.astype(_F64) < x, np.nextafter(y, INF32), y).astype(_F32)


def check_keep(cand, count, gbn, cap, want):
    """A PHASE 1 launch with thresholds.  want[q] = the keys that must be kept.  count is the size of that set whatever cap
    is; the buffer holds that set, or -- past cap -- cap distinct members of it; nothing at or behind min(count, cap)."""
    c, n = check_guards(cand, count, gbn, cap)
    for q in range(gbn):
        w = np.asarray(want[q], _U64)
        assert int(n[q]) == w.size, ("count is not the number of qualifying rows", q, int(n[q]), w.size)
        have = c[q, :min(w.size, cap)]
        assert np.unique(have).size == have.size, ("a candidate twice", q)
        if w.size <= cap:
            assert np.array_equal(np.sort(have), np.sort(w)), ("kept set differs", q, np.setxor1d(have, w)[:6])
        else:
            assert np.isin(have, w).all(), ("a kept key that does not qualify", q)


def check_halfmax(got, want):
    """PHASE 0: every slot equals the reference, untouched slots (idle columns, the guard) included."""
    got, want = np.asarray(got, _U64), np.asarray(want, _U64)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, ("halfmax differs", bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


def check_bounds(v, bound, truth):
    """Rigorous bounds: v - bound <= truth <= v + bound for every finite entry (v, truth [n, nq]; bound broadcastable).
    -> worst |v - truth| / bound."""
    v, truth = np.asarray(v, _F64), np.asarray(truth, _F64)
    bound = np.broadcast_to(np.asarray(bound, _F64), v.shape)
    ok = np.isfinite(v) & np.isfinite(truth) & np.isfinite(bound)
    err = np.abs(v - truth)[ok]
    assert (err <= bound[ok]).all(), ("a selection score further from the true score than its bound", float(err.max()),
                                      float((err / np.maximum(bound[ok], 1e-300)).max()))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(err > 0, err / bound[ok], 0.0).max(initial=0.0))


# --------------------------------------------------------------------------- #
# the library
# --------------------------------------------------------------------------- #
class _GemmCall(C.Structure):
    _fields_ = [("phase", C.c_int32), ("family", C.c_int32), ("ct", C.c_int32), ("metric", C.c_int32), ("groupb", C.c_int32),
                ("n_rows", C.c_uint32), ("pitch4", C.c_uint32), ("num_tiles", C.c_uint32), ("tile_stride", C.c_uint32),
                ("grid", C.c_uint32), ("cus", C.c_uint32), ("cap", C.c_uint32), ("qb_pitch16", C.c_uint32), ("live", C.c_uint32),
                ("eps", C.c_float), ("gam", C.c_float), ("floor_abs", C.c_float), ("under_abs", C.c_float)]


_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp, u64, u32, i = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        lib.gemm_instance.argtypes = [i, i, i, i, i, u32, C.POINTER(u64), C.POINTER(u32), C.POINTER(i), C.POINTER(u32), C.POINTER(u64)]
        lib.gemm_grid_rule.argtypes = [i, i, i, i, i, u32, u32, u32]
        lib.gemm_grid_rule.restype = u32
        lib.gemm_tile_pad_rows.restype = u32
        lib.gemm_rows_per_tile.argtypes = [i]
        lib.gemm_rows_per_tile.restype = u32
        lib.gemm_tiles.argtypes = [C.POINTER(_GemmCall)] + [vp, u64] * 10
        lib.gemm_rows_to_bf16.argtypes = [vp, u64, u64, u64, u32, vp, u64, u32, u32]
        lib.gemm_queries_to_bf16.argtypes = [vp, u64, u32, u32, vp, u64, u32, u32, u32, u32, u32]
        lib.gemm_cn_stats.argtypes = [vp, u64, u64, vp, u64, u32]
        lib.gemm_group_max.argtypes = [vp, u64, u64, vp, u64, u32]
        lib.gemm_query_norm.argtypes = [vp, u64, u32, i, i, vp, u64]
        lib.gemm_tau_margin.argtypes = [vp, u64, vp, u64, u32, i, u32, i, i, C.c_float, C.c_float]
        for f in (lib.gemm_instance, lib.gemm_tiles, lib.gemm_rows_to_bf16, lib.gemm_queries_to_bf16, lib.gemm_cn_stats,
                  lib.gemm_group_max, lib.gemm_query_norm, lib.gemm_tau_margin):
            f.restype = C.c_int
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _len(a):
    return 0 if a is None else a.size


def _check(rc, what):
    if rc == -1:
        raise ValueError(f"{what}: the harness refused the arguments (out of the uploaded arrays' bounds, or out of range)")
    if rc:
        raise RuntimeError(f"{what}: HIP error {rc}")


def instance(phase, family, ct, metric, groupb, pitch4):
    """-> None when the picker has no instance, else dict(lds, threads, ktail, per_cu, fn)."""
    lds, th, kt, pc, fn = C.c_uint64(0), C.c_uint32(0), C.c_int(0), C.c_uint32(0), C.c_uint64(0)
    rc = load().gemm_instance(phase, family, ct, metric, int(groupb), pitch4, C.byref(lds), C.byref(th), C.byref(kt), C.byref(pc), C.byref(fn))
    if rc < 0:
        raise ValueError("gemm_instance: not a question the picker answers")
    return None if rc == 0 else dict(lds=lds.value, threads=th.value, ktail=bool(kt.value), per_cu=pc.value, fn=fn.value)


def grid_rule(phase, family, ct, metric, groupb, pitch4, num_tiles, cus):
    return load().gemm_grid_rule(phase, family, ct, metric, int(groupb), pitch4, num_tiles, cus)


def tiles(phase, family, ct, metric, rows, n_rows, pitch4, num_tiles, tile_stride=1, grid=0, cus=0, queries=None, qb16=None,
          qb_pitch16=0, cn=None, gmax=None, qn=None, eps=0.0, gam=0.0, floor_abs=0.0, under_abs=0.0, live=0, tau=None, cap=0,
          halfmax_extra=GUARD, halfmax_len=None, cand_len=None, count_len=None):
    """One tile launch.  PHASE 0 -> halfmax (flat, [64 ct * RW * num_tiles] + guard, prefilled with SENT_KEY); PHASE 1 ->
    (cand flat [64 ct * cap] + guard of SENT_KEY, count [64 ct] zeros + guard of SENT_U32)."""
    gbn, RW = 64 * ct, wave_groups(family)
    groupb = gmax is not None
    d = _GemmCall(phase, family, ct, metric, int(groupb), n_rows, pitch4, num_tiles, tile_stride, grid, cus, cap, qb_pitch16, live,
                  float(eps), float(gam), float(floor_abs), float(under_abs))
    rows = np.ascontiguousarray(rows)
    f = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    queries, qb16, cn, gmax, qn, tau = f(queries, _F32), f(qb16, _U16), f(cn, _F32), f(gmax, _F32), f(qn, _F32), f(tau, _F32)
    halfmax = cand = count = None
    if phase == 0:
        halfmax = np.full(gbn * RW * num_tiles + halfmax_extra if halfmax_len is None else halfmax_len, SENT_KEY, _U64)
    else:
        cand = np.full(gbn * cap + GUARD if cand_len is None else cand_len, SENT_KEY, _U64)
        count = np.full(gbn + GUARD if count_len is None else count_len, SENT_U32, _U32)
        count[:gbn] = 0
    rc = load().gemm_tiles(C.byref(d), _ptr(rows), rows.nbytes, _ptr(queries), _len(queries), _ptr(qb16), _len(qb16), _ptr(cn), _len(cn),
                           _ptr(gmax), _len(gmax), _ptr(qn), _len(qn), _ptr(tau), _len(tau), _ptr(halfmax), _len(halfmax), _ptr(cand),
                           _len(cand), _ptr(count), _len(count))
    _check(rc, "gemm_tiles")
    return halfmax if phase == 0 else (cand, count)


def rows_to_bf16(rows, r0, n, pitch16, out, grid=0):
    rows = np.ascontiguousarray(rows, _F32)
    out = np.ascontiguousarray(out, _U16).copy()
    _check(load().gemm_rows_to_bf16(_ptr(rows), rows.size, r0, n, rows.shape[1], _ptr(out), out.size, pitch16, grid), "gemm_rows_to_bf16")
    return out


def queries_to_bf16(q, nv, kpad, gbn, live, blocks, grid=0, out_len=None):
    q = np.ascontiguousarray(q, _F32)
    out = np.full(blocks * gbn * kpad + GUARD if out_len is None else out_len, SENT_U16, _U16)
    _check(load().gemm_queries_to_bf16(_ptr(q), q.size, q.shape[1], nv, _ptr(out), out.size, kpad, gbn, live, blocks, grid), "gemm_queries_to_bf16")
    return out


def cn_stats(cn, n, grid=0):
    cn = np.ascontiguousarray(cn, _F32)
    stats = np.zeros(4, _U32)
    stats[3] = SENT_U32
    _check(load().gemm_cn_stats(_ptr(cn), cn.size, n, _ptr(stats), stats.size, grid), "gemm_cn_stats")
    return stats


def group_max_dev(cn, n, grid=0, gmax_len=None):
    cn = np.ascontiguousarray(cn, _F32)
    out = np.full((n + 63) // 64 + 8 if gmax_len is None else gmax_len, SENT_F32_BITS, _U32).view(_F32)
    _check(load().gemm_group_max(_ptr(cn), cn.size, n, _ptr(out), out.size, grid), "gemm_group_max")
    return out


def query_norm(q, nv, gbn):
    q = np.ascontiguousarray(q, _F32)
    out = np.full(gbn + 8, SENT_F32_BITS, _U32).view(_F32)
    _check(load().gemm_query_norm(_ptr(q), q.size, q.shape[1], nv, gbn, _ptr(out), out.size), "gemm_query_norm")
    return out


def tau_margin(tau, q, nv, cmax, metric, bf16, floor_abs, under_abs=0.0):
    q = np.ascontiguousarray(q, _F32)
    tau = np.ascontiguousarray(tau, _F32).copy()
    bits = int(np.array([cmax], _F32).view(_U32)[0])
    _check(load().gemm_tau_margin(_ptr(tau), tau.size, _ptr(q), q.size, q.shape[1], nv, bits, metric, int(bf16), float(floor_abs),
                                  float(under_abs)), "gemm_tau_margin")
    return tau
