"""ctypes loader of tests/kernel_harness/libtile_harness.so (built by ``make -C wdbx-py_amd/csrc all``), a numpy restatement
of the int8 tile kernel's epilogues (kernels_tiles8.h::gemm_i8_kernel) and the checkers of tests/test_gpu_tile_kernels.py.

The harness launches the library's own ``gemm_i8_kernel`` instances (chosen, sized and launched by the helpers behind the
kernel), ``gbad_with_mask_kernel`` and ``group_ref_kernel`` on arrays the caller hands it.

The checkers are plain numpy on int64 / float64 and never look at the code under test: they take what a launch was GIVEN
(bytes, tables, thresholds) and what it EMITTED (pairs, counters, keys).  The test module feeds them the kernels' output on
the GPU and, on the CPU, the restatement below and a list of deliberately wrong restatements that they must reject.

Tolerances (derived from the constants the kernel documents, u = 2^-24; nothing here is tuned against an output):

PHASE 1, inner product.  The kernel keeps row r for query q iff D >= T with
    T = e_inv A1 - 1 - e_ai E' - e_bi M',  A1 = (tau / s_q)(1 -+ 2e-6),  E' = 1.000003 E / s_q,  e_inv = 1 / s_g ...
i.e., times s_g s_q:  s_g s_q D + 1.000003 (a_g E + b_g M) >= tau - 2e-6 |tau| - s_g s_q.  So every kept row has
    ub >= tau - [ s_g s_q  +  2e-6 |tau|  +  3e-6 (a_g E + b_g M)  +  12 u (|tau| + a_g E + b_g M + s_g s_q + |s_g s_q D|) ]
with ub = s_g s_q D + a_g E + b_g M in float64: one unit of D, the 2e-6 folded into A1, the two 1.000003 factors, and the
fp32 roundings of the chain (1 / s_q, tau / s_q, A1: 2, the reciprocal of s_g: 2, the products with it, three fmas, D as
fp32 beyond 2^24: at most 12, each relative to a magnitude in the bracket).
L2 (keep iff 2 (s_g s_q D + bound) - |c|^2 >= tau): the same at tau / 2, doubled, plus 2e-6 |D| on the dot product and the norm
taken 0.9999 x 0.999997 low:
    slack = 2 s_g s_q + 2e-6 |tau| + 6e-6 bound + 4e-6 |s_g s_q D| + 1.03e-4 |c|^2 + 12 u (|tau| + 2 bound + 2 s_g s_q + 2 |s_g s_q D| + |c|^2).
A zero query (s_q = 0) is compared unscaled (its unit of D is s_g), an all-zero group (1 / s_g overflows) with 2^60 in place of
1 / s_g (its unit is 2^-60 s_q): the slack takes these units.  Rows whose slack is not finite (a_g, E or a norm infinite) have
no tightness statement: `keep_rule` reports their share.

PHASE 0.  lb = w - 1.000001 err - 4e-7 |w|, w = s_g s_q Dmax, err = a_g E + b_g M: the emitted score is at most the float64
value of w - err and at most  1e-6 err + 4e-7 |w| + 8 u (|w| + err)  below it.  L2: v = 2 w - 1.0001 |c|^2 - 8e-7 |2 w| - 2.000002 err:
at most  1e-4 |c|^2 + 8e-7 |2 w| + 2e-6 err + 8 u (|2 w| + |c|^2 + 2 err)  below 2 w - |c|^2 - 2 err of the float64 best row."""
import ctypes as C
from dataclasses import dataclass, field, replace  # noqa: F401  (replace: re-exported for the tests)
from pathlib import Path

import numpy as np

from select_harness import GUARD, SENT_KEY, SENT_U32, U, f2ord, g8_offset, make_keys, ord2f  # noqa: F401

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "kernel_harness" / "tile_harness.hip"
LIBRARY = ROOT / "tests" / "kernel_harness" / "libtile_harness.so"

I8, U8, U32, U64, I64, F32, F64 = np.int8, np.uint8, np.uint32, np.uint64, np.int64, np.float32, np.float64
COS, L2 = 0, 1
G8_ROWS = 256
LDS_B_MAX = 96 * 1024
PAIR_D_UNKNOWN = 0x800000
PITCHES = [128, 256, 384, 640, 768, 1152, 1536]


def ring_rule(ct, pitch8):
    """kernels_tiles8.h::gemm8_ring and the compile-time instances' own rings, restated (the GPU suite compares)."""
    if pitch8 == 384:
        return 3 if ct == 4 else 6
    if pitch8 == 768 and ct != 4:
        return 6
    steps = pitch8 // 64
    return 2 if ct == 4 else 6 if steps % 6 == 0 else 4 if steps % 4 == 0 else 2


def fits(ct, pitch8, metric=COS):
    return 64 * ct * pitch8 <= LDS_B_MAX and not (metric == L2 and ct == 4)


@dataclass
class Tile:
    """One launch: the arrays the kernel is given (rows / q8 as plain [n, pitch8] int8, packed on the way in)."""
    ct: int
    pitch8: int
    rows: np.ndarray          # [tiles_alloc * 256, pitch8] int8
    q8: np.ndarray            # [64 ct, pitch8] int8
    groups: np.ndarray        # [n_groups, 4] fp32 {s_g, a_g, b_g, vouch}
    qpar: np.ndarray          # [64 ct, 4] fp32 {s_q, E, M, 1 / s_q}
    n_rows: int
    nv: int                   # real queries (the others: zero bytes, zero qpar, tau = +inf)
    metric: int = COS
    num_tiles: int = 0        # 0: all tiles of `rows`
    tile_stride: int = 1
    gbad: np.ndarray = None   # [n_groups] uint64, or [n_classes, n_groups] (multi)
    cn: np.ndarray = None     # [n_rows] fp32 (L2)
    tau: np.ndarray = None    # [64 ct] fp32
    gref: np.ndarray = field(default_factory=lambda: np.array([np.inf, np.inf], F32))
    masked: bool = False
    multi: bool = False
    variant: int = 0
    class_row: tuple = (0,) * 16
    grid: int = 1
    pair_cap: int = 0         # 0: room for everything a wave can produce

    @property
    def gbn(self):
        return 64 * self.ct

    @property
    def tiles(self):
        return self.num_tiles or len(self.rows) // G8_ROWS

    def waves_tiles(self, b, grid=None):
        return range(b, self.tiles, grid or self.grid)

    def cap(self):
        return self.pair_cap or -(-self.tiles // self.grid) * 32 * self.gbn


def pack_rows(rows):
    """[n, pitch8] int8 (n a multiple of 32) -> the fragment-ordered bytes"""
    n, pitch8 = rows.shape
    r, c = np.meshgrid(np.arange(n), np.arange(pitch8), indexing="ij")
    flat = np.zeros(n * pitch8, I8)
    flat[g8_offset(r, c, pitch8)] = rows
    return flat


def dots(rows, q8):
    """The int64 dot products of the very bytes uploaded, [rows, queries] (float64 products and sums of them are exact:
    127 * 127 * 1536 < 2^53)."""
    return np.rint(rows.astype(F64) @ q8.astype(F64).T).astype(I64)


def bad_bits(gbad_row, n):
    """uint64 [groups] -> bool [n]: bit r % 64 of word r / 64"""
    r = np.arange(n)
    return ((np.asarray(gbad_row, U64)[r >> 6] >> (r & 63).astype(U64)) & U64(1)).astype(bool)


def bad_matrix(t, phase):
    """bool [rows, 64 ct]: row r may not be returned to / vouch for query q (what the launch's gbad says to the instance)."""
    n = len(t.rows)
    out = np.zeros((n, t.gbn), bool)
    if t.multi:
        for j in range(t.gbn // 16):
            out[:, 16 * j:16 * j + 16] = bad_bits(t.gbad[t.class_row[j]], n)[:, None]
    elif phase == 0 or t.masked:
        out[:] = bad_bits(t.gbad, n)[:, None]
    return out


# --------------------------------------------------------------------------- #
# the kernel's epilogues restated (fp32; fma through float64: products of two fp32 are exact there)
# --------------------------------------------------------------------------- #
def _fma(a, b, c):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def _f(x):
    return np.asarray(x, F32)


def bswz(c, r, odd):
    """g8_bswz"""
    return np.where(odd, (c & ~7) | ((c & 7) ^ ((r >> 1) & 7)), (c & ~15) | ((c & 15) ^ (r & 15)))


def _kernel_dots(t, bug):
    """D as the kernel forms it: with bug 'swizzle_parity' the fragment reads use the other parity's XOR key, so a query's
    16-byte pieces arrive permuted."""
    q8 = t.q8
    if bug == "swizzle_parity":
        P = t.pitch8 // 16
        odd = bool((t.pitch8 // 128) & 1)
        r, c = np.meshgrid(np.arange(t.gbn), np.arange(P), indexing="ij")
        src = bswz(bswz(c, r, not odd), r, odd)
        src = np.where(src < P, src, c)
        q8 = q8.reshape(t.gbn, P, 16)[r, src].reshape(t.gbn, t.pitch8)
    return dots(t.rows, q8)


def _row_tables(t, n, stride_in_group=True):
    g = np.arange(n) >> 6
    return t.groups[g, 0], t.groups[g, 1], t.groups[g, 2], t.groups[g, 3]


def restate_phase1(t, bug=None):
    """-> dict(pairs [grid * 8, cap], guard, count) as the harness returns them (order inside a list: by row, query)."""
    n = t.tiles * G8_ROWS
    D = _kernel_dots(t, bug)[:n]
    l2 = t.metric == L2
    pre = not l2 and not (t.variant == 13 and not t.masked and not t.multi)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        tau = _f(0.5) * t.tau if l2 else t.tau
        padded = ~(tau < np.inf)
        w = np.where(t.qpar[:, 3] == 0, F32(1), t.qpar[:, 3]).astype(F32)
        A = _f(tau * w)
        A1 = np.where(padded, F32(np.inf), _f(A - _f(F32(2e-6) * np.abs(A)))).astype(F32)
        Ep, Mp = _f(_f(t.qpar[:, 1] * w) * F32(1.000003)), _f(_f(t.qpar[:, 2] * w) * F32(1.000003))
        s_g, a_g, b_g, _ = _row_tables(t, n)
        rcp = _f(F32(1) / s_g)
        e_inv = np.where(rcp < np.inf, rcp, F32(2.0 ** 60)).astype(F32)
        e_ai, e_bi = _f(a_g * e_inv), _f(b_g * e_inv)
        one = F32(1.0 if bug == "slack_sign" else -1.0)
        T = _fma(-e_bi[:, None], Mp[None, :], _fma(-e_ai[:, None], Ep[None, :], _fma(e_inv[:, None], A1[None, :], one)))
        d = D.astype(F32)
        if l2:
            cn = t.cn[np.minimum(np.arange(n), t.n_rows - 1)]
            u = np.where(np.isnan(cn), F32(np.inf),
                         np.where(cn < np.inf, _f(_f(_f(F32(0.5) * cn) * F32(0.9999)) * e_inv), F32(-np.inf))).astype(F32)
            wq = _f(w * F32(0.999997))
            f = _f(_fma(-u[:, None], wq[None, :], d) + _f(F32(2e-6) * np.abs(d)))
            keep = ~(f < T) & (A1 < np.inf)[None, :]
        else:
            keep = ~(d < T) & ~padded[None, :]
        if pre:
            aref, bref = t.gref[0], t.gref[1]
            Uq = _fma(-bref, Mp, _fma(-aref, Ep, A1))
            Uq = _f(Uq - _f(F32(4e-6) * _f(_f(np.abs(A1) + _f(aref * Ep)) + _f(bref * Mp))))
            if bug == "pre_strict":
                Uq = _f(Uq + F32(1e-3) * np.abs(Uq))
            pre_hit = ~(d < _fma(e_inv[:, None], Uq[None, :], F32(-1.0)))
            anyhit = pre_hit.reshape(n // 32, 32, t.gbn // 16, 16).any(axis=(1, 3))          # [block, column group]
            ordinary = ((a_g <= aref) & (b_g <= bref)).reshape(n // 32, 32)[:, 0]
            go = np.where(ordinary[:, None], anyhit, True)
            keep &= np.repeat(np.repeat(go, 32, axis=0), 16, axis=1)
    keep &= (np.arange(n) < t.n_rows)[:, None]
    if t.masked or t.multi:
        bad = bad_matrix(t, 1)[:n]
        if bug == "bad_shift":  # the wave's 32 bits from the other half of the group's word
            bad = bad.reshape(n // 64, 2, 32, t.gbn)[:, ::-1].reshape(n, t.gbn)
        keep &= ~bad
    cap = t.cap()
    pairs = np.full(t.grid * 8 * cap + GUARD, SENT_KEY, U64)
    count = np.full(t.grid * 8, SENT_U32, U32)
    for b in range(min(t.grid, t.tiles)):
        for wave in range(8):
            out = []
            for tl in t.waves_tiles(b):
                r0 = (tl * t.tile_stride * 8 + wave) * 32
                rr, qq = np.nonzero(keep[r0:r0 + 32])
                dd = D[r0 + rr, qq]
                row = r0 + rr
                if bug == "row_half":
                    row = row ^ 16
                d24 = np.where((dd > -(1 << 23)) & (dd < (1 << 23)), dd & 0xFFFFFF, PAIR_D_UNKNOWN).astype(U64)
                out.append((d24 << U64(40)) | (qq.astype(U64) << U64(32)) | row.astype(U64))
            out = np.concatenate(out)
            wid = b * 8 + wave
            count[wid] = len(out)
            m = min(len(out), cap)
            pairs[wid * cap:wid * cap + m] = out[:m]
    return {"pairs": pairs[:t.grid * 8 * cap].reshape(t.grid * 8, cap), "guard": pairs[t.grid * 8 * cap:], "count": count}


def restate_phase0(t, bug=None):
    """-> dict(halfmax [64 ct, 8 * num_tiles], guard)"""
    nt = t.tiles
    D = _kernel_dots(t, bug)
    bad = bad_matrix(t, 0)
    hm = np.full(t.gbn * 8 * nt + GUARD, SENT_KEY, U64)
    out = hm[:t.gbn * 8 * nt].reshape(t.gbn, 8 * nt)
    l2 = t.metric == L2
    with np.errstate(invalid="ignore", over="ignore"):
        for tl in range(nt):
            for wave in range(8):
                r0 = (tl * t.tile_stride * 8 + wave) * 32
                gt = t.groups[((tl if bug == "stride_ignored" else tl * t.tile_stride) * 8 + wave) * 32 >> 6]
                b = bad[r0:r0 + 32]
                if bug == "bad_shift":
                    b = bad[(r0 ^ 32):(r0 ^ 32) + 32]
                d = D[r0:r0 + 32]
                sq, E, M = t.qpar[:, 0], t.qpar[:, 1], t.qpar[:, 2]
                err = _f(_f(gt[1] * E) + _f(gt[2] * M))
                if l2:
                    ss = _f(_f(F32(2.0) * gt[0]) * sq)
                    rows = np.minimum(np.arange(r0, r0 + 32), t.n_rows - 1)
                    cnh = _f(t.cn[rows] * F32(1.0001))
                    df = d.astype(F32)
                    v = _f(_fma(ss[None, :], df, -cnh[:, None]) - _f(F32(8e-7) * np.abs(_f(ss[None, :] * df))))
                    v = np.where(b | np.isnan(v), F32(-np.inf), v)
                    best = v.max(axis=0)
                    none = best == -np.inf
                    lb = _f(best - _f(_f(F32(2.0) * err) * F32(1.000001)))
                else:
                    m = np.where(b, np.iinfo(np.int32).min, d).max(axis=0)
                    none = m == np.iinfo(np.int32).min
                    w = _f(_f(gt[0] * sq) * m.astype(F32))
                    lb = _f(_f(w - _f(err * F32(1.000001))) - _f(F32(4e-7) * np.abs(w)))
                lb = np.where((gt[3] != 1.0) | none | np.isnan(lb), F32(-np.inf), lb).astype(F32)
                ht = tl * 8 + wave
                out[:, ht] = np.where(lb == -np.inf, U64(0), make_keys(f2ord(lb + F32(0.0)), np.full(t.gbn, ht)))
    return {"halfmax": out, "guard": hm[t.gbn * 8 * nt:]}


# --------------------------------------------------------------------------- #
# checkers
# --------------------------------------------------------------------------- #
def check_pairs(t, out, D, exact_set=None):
    """Structure of a PHASE 1 output, whatever the thresholds: -> kept, bool [rows, 64 ct].
    Every wave's list holds only pairs of ITS rows (tiles b, b + grid, ...; rows of wave w), of rows < n_rows and real queries, none
    twice; the D24 field is the int64 dot product (PAIR_D_UNKNOWN exactly when |D| >= 2^23); bad rows (masked, multi) are
    absent; pair_count is the number produced: with room for them exactly the list's entries, and what lies behind them, behind
    a full list and behind the last list is untouched.  exact_set: bool [rows, 64 ct], the set that must be produced exactly
    (then pair_count is checked against it also where a list overflowed)."""
    cap = t.cap()
    n = t.tiles * G8_ROWS
    pairs, count = out["pairs"], out["count"]
    assert pairs.shape == (t.grid * 8, cap)
    assert (out["guard"] == SENT_KEY).all(), "words behind the last list were written"
    kept = np.zeros((n, t.gbn), bool)
    bad = bad_matrix(t, 1)[:n]
    for wid in range(t.grid * 8):
        b, wave = divmod(wid, 8)
        if b >= t.tiles:
            assert count[wid] == SENT_U32 and (pairs[wid] == SENT_KEY).all(), ("an idle workgroup wrote", wid)
            continue
        c = int(count[wid])
        m = min(c, cap)
        assert (pairs[wid, m:] == SENT_KEY).all(), ("entries behind pair_count were written", wid)
        p = pairs[wid, :m]
        row, q, d24 = (p & U64(0xFFFFFFFF)).astype(I64), ((p >> U64(32)) & U64(0xFF)).astype(I64), (p >> U64(40)).astype(I64)
        assert (row < t.n_rows).all(), ("a row past the end", wid, row[row >= t.n_rows][:4])
        assert (q < t.nv).all(), ("a padded query", wid)
        tl = row // G8_ROWS
        assert ((row // 32) % 8 == wave).all() and (tl % t.grid == b).all(), ("a pair in another wave's list", wid)
        assert not kept[row, q].any() and len(np.unique(row * 256 + q)) == len(row), ("a pair twice", wid)
        kept[row, q] = True
        assert not bad[row, q].any(), ("a bad row was emitted", wid, row[bad[row, q]][:4])
        ref = D[row, q]
        want = np.where((ref > -(1 << 23)) & (ref < (1 << 23)), ref & 0xFFFFFF, PAIR_D_UNKNOWN)
        wrong = np.flatnonzero(d24 != want)
        assert not len(wrong), ("D24 differs from the int64 dot product", wid, row[wrong][:4], q[wrong][:4], d24[wrong][:4], want[wrong][:4])
        if exact_set is not None:
            mine = np.zeros(n, bool)
            for tt in t.waves_tiles(b):
                r0 = (tt * 8 + wave) * 32
                mine[r0:r0 + 32] = True
            expect = int(exact_set[mine].sum())
            assert c == expect, ("pair_count", wid, c, expect)
    if exact_set is not None and (count[:min(t.grid, t.tiles) * 8] <= cap).all():
        assert (kept == exact_set[:n]).all(), ("pairs missing", np.argwhere(kept != exact_set[:n])[:4])
    return kept


def _units(t, n):
    """(s_g, s_q) as the kernel scales D: 2^-60 for a group whose reciprocal overflows fp32, 1 for a zero query"""
    with np.errstate(divide="ignore", over="ignore"):
        s_g = t.groups[np.arange(n) >> 6, 0]
        sg = np.where(np.isfinite(_f(F32(1) / s_g)), s_g.astype(F64), 2.0 ** -60)
    sq = np.where(t.qpar[:, 0] > 0, t.qpar[:, 0].astype(F64), 1.0)
    return sg, sq


def keep_rule(t, D):
    """float64: (must, may_not, skipped share).  must[r, q]: the rule of the issue says keep (the upper bound reaches tau, or is
    NaN: nothing is known); may_not[r, q]: the row lies further below tau than the documented slack (module docstring).  Rows
    >= n_rows, padded queries and -- where the instance reads the bad rows -- bad rows are in neither.  L2: a NaN norm is never
    kept under a finite tau and a finite bound (at tau = -inf, or against an infinite bound, the kernel's test -inf < T is false
    and the row goes to the exact pass, where its NaN score is never a result: no statement), an infinite one always.  skipped = the share of (row, real query) entries without a tightness statement."""
    n = t.tiles * G8_ROWS
    D = D[:n].astype(F64)
    g = np.arange(n) >> 6
    s_g, a_g, b_g = (t.groups[g, i].astype(F64) for i in range(3))
    s_q, E, M = (t.qpar[:, i].astype(F64) for i in range(3))
    tau = t.tau.astype(F64)
    sgu, squ = _units(t, n)
    with np.errstate(invalid="ignore", over="ignore"):
        ssd = (s_g[:, None] * s_q[None, :]) * D
        bound = a_g[:, None] * E[None, :] + b_g[:, None] * M[None, :]
        unit = sgu[:, None] * squ[None, :]
        if t.metric == L2:
            cn = np.full(n, np.nan)
            cn[:t.n_rows] = t.cn[:t.n_rows].astype(F64)
            ub = 2.0 * (ssd + bound) - cn[:, None]
            must = ~(ub < tau[None, :])
            must = np.where(np.isnan(cn)[:, None], False, np.where(np.isinf(cn)[:, None], True, must))
            mag = np.abs(tau)[None, :] + 2 * bound + 2 * unit + 2 * np.abs(ssd) + np.abs(cn)[:, None]
            slack = 2 * unit + 2e-6 * np.abs(tau)[None, :] + 6e-6 * bound + 4e-6 * np.abs(ssd) + 1.03e-4 * np.abs(cn)[:, None] + 12 * U * mag
        else:
            ub = ssd + bound
            must = ~(ub < tau[None, :])
            mag = np.abs(tau)[None, :] + bound + unit + np.abs(ssd)
            slack = unit + 2e-6 * np.abs(tau)[None, :] + 3e-6 * bound + 12 * U * mag
        stated = np.isfinite(ub) & (np.isfinite(slack) | np.isneginf(tau)[None, :])  # (tau = -inf: every row is kept, nothing to state)
        may_not = stated & (ub < tau[None, :] - slack)
        if t.metric == L2:
            may_not |= np.isnan(cn)[:, None] & np.isfinite(bound) & np.isfinite(tau)[None, :]
    live = np.zeros((n, t.gbn), bool)
    live[:t.n_rows, :t.nv] = True
    live &= (t.tau < np.inf)[None, :]
    if t.masked or t.multi:
        live &= ~bad_matrix(t, 1)[:n]
    skipped = float((live & ~stated).sum()) / max(1, int(live.sum()))
    return must & live, may_not & live, skipped


def check_keep(t, kept, D):
    """Safety (hard) and tightness of a PHASE 1 kept set against `keep_rule`; -> the skipped share."""
    must, may_not, skipped = keep_rule(t, D)
    lost = np.argwhere(must & ~kept)
    assert not len(lost), ("rows whose upper bound reaches tau were dropped", len(lost), lost[:4])
    loose = np.argwhere(may_not & kept)
    assert not len(loose), ("rows kept further below tau than the documented slack", len(loose), loose[:4])
    return skipped


def check_halfmax(t, out, D):
    """PHASE 0 against float64 (module docstring): the key of (query, slot 8 t + wave) is 0 exactly when the group does not vouch,
    all 32 rows are bad (L2: or carry a NaN norm), or the float64 bound is NaN or -inf; otherwise its row half is the slot, its
    score at most the float64 lower bound of the block's best non-bad row and at most the derived slack below it.  Everything
    outside [0, 64 ct) x [0, 8 num_tiles) keeps its sentinel."""
    nt = t.tiles
    hm = out["halfmax"]
    assert hm.shape == (t.gbn, 8 * nt)
    assert (out["guard"] == SENT_KEY).all(), "words behind halfmax were written"
    bad = bad_matrix(t, 0)
    s_q, E, M = (t.qpar[:, i].astype(F64) for i in range(3))
    for tl in range(nt):
        for wave in range(8):
            ht = tl * 8 + wave
            r0 = (tl * t.tile_stride * 8 + wave) * 32
            gt = t.groups[r0 >> 6].astype(F64)
            d = D[r0:r0 + 32].astype(F64)
            good = ~bad[r0:r0 + 32]
            with np.errstate(invalid="ignore", over="ignore"):
                err = gt[1] * E + gt[2] * M
                if t.metric == L2:
                    cn = t.cn[np.minimum(np.arange(r0, r0 + 32), t.n_rows - 1)].astype(F64)
                    good = good & ~np.isnan(cn)[:, None]
                    w2 = 2.0 * gt[0] * s_q[None, :] * d
                    v = np.where(good, w2 - cn[:, None], -np.inf)
                    best = v.argmax(axis=0)
                    q = np.arange(t.gbn)
                    value = v[best, q] - 2.0 * err
                    slack = 1e-4 * np.abs(cn[best]) + 8e-7 * np.abs(w2[best, q]) + 2e-6 * err + 8 * U * (np.abs(w2[best, q]) + np.abs(cn[best]) + 2 * err)
                else:
                    dmax = np.where(good, d, -np.inf).max(axis=0)
                    w = gt[0] * s_q * dmax
                    value = w - err
                    slack = 1e-6 * err + 4e-7 * np.abs(w) + 8 * U * (np.abs(w) + err)
            zero = (gt[3] != 1.0) | ~good.any(axis=0) | np.isnan(value) | (value == -np.inf)
            key = hm[:, ht]
            assert ((key == 0) == zero).all(), ("key 0 exactly when nothing vouches", ht, np.flatnonzero((key == 0) != zero)[:4])
            k = key[~zero]
            assert ((~k & U64(0xFFFFFFFF)) == U64(ht)).all(), ("row half", ht)
            score = ord2f((k >> U64(32)).astype(U32)).astype(F64)
            v, s = value[~zero], slack[~zero]
            assert (score <= v).all(), ("not a lower bound", ht, np.flatnonzero(~zero)[score > v][:4], score[score > v][:2], v[score > v][:2])
            assert (score >= v - s).all(), ("further below the bound than the slack", ht, (v - score)[score < v - s][:2], s[score < v - s][:2])


def gbad_with_mask_py(gbad, mask, mask_words, mask_stride, class_mask):
    """gbad_with_mask_kernel restated: [n_classes, n_groups] uint64"""
    gbad = np.asarray(gbad, U64)
    ng = len(gbad)
    cm = [0] if class_mask is None else list(class_mask)
    out = np.zeros((len(cm), ng), U64)
    for y, m in enumerate(cm):
        if m < 0:
            out[y] = gbad
            continue
        words = np.zeros(2 * ng, U64)
        k = min(mask_words, 2 * ng)
        words[:k] = np.asarray(mask, U32)[m * mask_stride:m * mask_stride + k]
        out[y] = gbad | ~(words[0::2] | (words[1::2] << U64(32)))
    return out


def group_ref_py(groups):
    """group_ref_kernel restated in float64: (a_ref, b_ref as fp32, sum a, sum b, count, ordinary mask).  Groups within
    1e-5 relative of the 1.5 x mean cut are returned as `edge` (their side depends on the fp32 sums' order)."""
    g = np.asarray(groups, F32)
    with np.errstate(invalid="ignore"):
        fin = (g[:, 0] > 0) & (g[:, 1] >= 0) & (g[:, 1] < np.inf) & (g[:, 2] >= 0) & (g[:, 2] < np.inf)
    cnt = int(fin.sum())
    sa, sb = float(g[fin, 1].astype(F64).sum()), float(g[fin, 2].astype(F64).sum())
    ma, mb = (sa / cnt, sb / cnt) if cnt else (0.0, 0.0)
    a, b = g[:, 1].astype(F64), g[:, 2].astype(F64)
    with np.errstate(invalid="ignore"):
        ordinary = fin & (a <= 1.5 * ma) & (b <= 1.5 * mb)
        edge = fin & ((np.abs(a - 1.5 * ma) <= 1e-5 * 1.5 * ma) | (np.abs(b - 1.5 * mb) <= 1e-5 * 1.5 * mb))
    aref = g[ordinary, 1].max() if ordinary.any() else F32(0)
    bref = g[ordinary, 2].max() if ordinary.any() else F32(0)
    return F32(aref), F32(bref), sa, sb, cnt, ordinary, edge


# --------------------------------------------------------------------------- #
# the library
# --------------------------------------------------------------------------- #
class _TileCall(C.Structure):
    _fields_ = [("ct", C.c_int32), ("metric", C.c_int32), ("masked", C.c_int32), ("multi", C.c_int32), ("variant", C.c_int32),
                ("n_rows", C.c_uint32), ("pitch8", C.c_uint32), ("num_tiles", C.c_uint32), ("tile_stride", C.c_uint32),
                ("grid", C.c_uint32), ("cus", C.c_uint32), ("pair_cap", C.c_uint32), ("n_classes", C.c_uint32),
                ("n_class_groups", C.c_uint64), ("class_row", C.c_uint8 * 16)]


_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        lib.tile_lds_b_max.restype = u32
        lib.tile_pair_d_unknown.restype = u32
        lib.tile_instance.argtypes = [i32, i32, u32, i32, i32, i32, i32, C.POINTER(C.c_int), C.POINTER(u64)]
        lib.tile_instance.restype = i32
        lib.tile_phase0.argtypes = [C.POINTER(_TileCall)] + [vp, u64] * 7
        lib.tile_phase0.restype = i32
        lib.tile_phase1.argtypes = [C.POINTER(_TileCall)] + [vp, u64] * 10
        lib.tile_phase1.restype = i32
        lib.tile_gbad_with_mask.argtypes = [vp, u64, vp, u64, u64, u64, vp, u32, vp, u64, u32]
        lib.tile_gbad_with_mask.restype = i32
        lib.tile_group_ref.argtypes = [vp, u64, u32, vp]
        lib.tile_group_ref.restype = i32
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _len(a):
    return 0 if a is None else a.size


def _check(rc, what):
    if rc == -1:
        raise ValueError(f"{what}: the harness refused the arguments")
    if rc:
        raise RuntimeError(f"{what}: HIP error {rc}")


def instance(phase, ct, pitch8, l2=False, masked=False, multi=False, variant=0):
    """-> (has, ring, lds bytes); ValueError: not a question the pickers answer"""
    ring, lds = C.c_int(0), C.c_uint64(0)
    rc = load().tile_instance(phase, ct, pitch8, int(l2), int(masked), int(multi), variant, C.byref(ring), C.byref(lds))
    _check(-1 if rc < 0 else 0, "tile_instance")
    return bool(rc), ring.value, lds.value


_PACKED = {}


def _packed(rows):
    key = (rows.__array_interface__["data"][0], rows.shape)
    if key not in _PACKED or _PACKED[key][0] is not rows:
        _PACKED[key] = (rows, pack_rows(rows))
    return _PACKED[key][1]


def _call(t, cus=0, grid=None):
    d = _TileCall(ct=t.ct, metric=t.metric, masked=int(t.masked), multi=int(t.multi), variant=t.variant, n_rows=t.n_rows, pitch8=t.pitch8,
                  num_tiles=t.tiles, tile_stride=t.tile_stride, grid=t.grid if grid is None else grid, cus=cus, pair_cap=t.cap())
    gbad = None if t.gbad is None else np.ascontiguousarray(t.gbad, U64)
    if t.multi:
        d.n_classes, d.n_class_groups = gbad.shape
        d.class_row = (C.c_uint8 * 16)(*t.class_row)
    return d, gbad


def phase0(t, guard=GUARD):
    """One PHASE 0 launch.  -> dict(halfmax [64 ct, 8 num_tiles], guard)"""
    d, gbad = _call(t)
    flat = _packed(t.rows)
    groups, qpar, q8 = np.ascontiguousarray(t.groups, F32), np.ascontiguousarray(t.qpar, F32), np.ascontiguousarray(t.q8, I8)
    cn = None if t.cn is None else np.ascontiguousarray(t.cn, F32)
    n = t.gbn * 8 * t.tiles
    hm = np.full(n + guard, SENT_KEY, U64)
    rc = load().tile_phase0(C.byref(d), _ptr(flat), flat.size, _ptr(groups), len(groups), _ptr(cn), _len(cn), _ptr(gbad), _len(gbad),
                            _ptr(q8), q8.size, _ptr(qpar), len(qpar), _ptr(hm), hm.size)
    _check(rc, "tile_phase0")
    return {"halfmax": hm[:n].reshape(t.gbn, 8 * t.tiles), "guard": hm[n:]}


def phase1(t, cus=0, grid=None, short=0):
    """One PHASE 1 launch.  -> dict(pairs [grid * 8, cap], guard, count [grid * 8]).  short: words withheld from the pairs array
    (the harness must then refuse)."""
    d, gbad = _call(t, cus, grid)
    flat = _packed(t.rows)
    groups, qpar, q8 = np.ascontiguousarray(t.groups, F32), np.ascontiguousarray(t.qpar, F32), np.ascontiguousarray(t.q8, I8)
    cn = None if t.cn is None else np.ascontiguousarray(t.cn, F32)
    tau, gref = np.ascontiguousarray(t.tau, F32), np.ascontiguousarray(t.gref, F32)
    cap, lists = t.cap(), t.grid * 8
    pairs = np.full(lists * cap + GUARD - short, SENT_KEY, U64)
    count = np.full(lists, SENT_U32, U32)
    rc = load().tile_phase1(C.byref(d), _ptr(flat), flat.size, _ptr(groups), len(groups), _ptr(cn), _len(cn), _ptr(gref), gref.size,
                            _ptr(gbad), _len(gbad), _ptr(q8), q8.size, _ptr(qpar), len(qpar), _ptr(tau), tau.size, _ptr(pairs), pairs.size,
                            _ptr(count), count.size)
    _check(rc, "tile_phase1")
    return {"pairs": pairs[:lists * cap].reshape(lists, cap), "guard": pairs[lists * cap:], "count": count}


def gbad_with_mask(gbad, mask, mask_words, mask_stride=0, class_mask=None, grid_x=0):
    """-> [n_classes, n_groups] uint64 and the guard words behind"""
    gbad = np.ascontiguousarray(gbad, U64)
    mask = None if mask is None else np.ascontiguousarray(mask, U32)
    cm = None if class_mask is None else np.ascontiguousarray(class_mask, np.int32)
    ny = 1 if cm is None else len(cm)
    out = np.full(ny * len(gbad) + GUARD, SENT_KEY, U64)
    rc = load().tile_gbad_with_mask(_ptr(gbad), len(gbad), _ptr(mask), _len(mask), mask_words, mask_stride, _ptr(cm), ny, _ptr(out), out.size,
                                    grid_x)
    _check(rc, "tile_gbad_with_mask")
    return out[:ny * len(gbad)].reshape(ny, len(gbad)), out[ny * len(gbad):]


def group_ref(groups, grid_x=0):
    """-> the 8 words {a_ref, b_ref, sum a, sum b, count, 0, 0, 0} as uint32"""
    groups = np.ascontiguousarray(groups, F32)
    ref = np.full(8, SENT_U32, U32)
    _check(load().tile_group_ref(_ptr(groups), len(groups), grid_x, _ptr(ref)), "tile_group_ref")
    return ref
