"""ctypes loader of ``tests/kernel_harness/libstage_harness.so`` -- the int8 batch stages around the tile kernel, each launched
ALONE -- with their numpy restatements and the checkers of ``tests/test_gpu_stage_kernels.py``.

Kernels: ``scatter_pairs_kernel``, ``refine_pairs_kernel<METRIC, REG>``, ``mark_lost_kernel``, ``place_queries_kernel``,
``pad_tau_kernel`` (kernels_tiles8.h), ``range_batch_bound_kernel`` (kernels_range_batch.h), ``gather_rows_kernel`` and
``normalize_rows_kernel`` (kernels_aux.h).  The checkers are plain numpy on int64 and float64; they see only what a launch was
given and what it emitted.  The restatements (``*_py``) are one admissible behaviour each, with named bugs for the CPU half of
the test module: every checker accepts its restatement and rejects each wrong one.

The second stage's slack (``refine_bounds64``).  The checker evaluates the kernel's formulas (the comment above
``refine_pairs_kernel`` and ``refine_bounds``) in float64 from the fp32 inputs and the fp32 constants:
    err = a_g E + b_g M
    cosine   w = s_g s_q D        lb = w - 1.000001 err - 4e-7 |w|       ub = w + 1.00001 err + 4e-6 (|w| + err) + s_g s_q
    L2       w = 2 s_g s_q D      lb = w - 1.0001 cn - 8e-7 |w| - 2 (1.000001) err
                                  ub = w - 0.9999 cn + 2 (1.00001) err + 8e-6 (|w| + err) + 2 s_g s_q
The kernel takes the same chain in fp32.  Counting its roundings (products by 2 are exact; (float)D is exact below 2^24):
err 3 (two products, one sum -- or 2 when the compiler contracts a product into an fma), s_g s_q 1, w 1, and then for the
longest chain, the L2 ub: cn 0.9999 (1), the difference (1), 1.00001 err (1), the sum (1), |w| + err (1), times 8e-6 (1), the
sum (1), + ss (1) -- 13 roundings in all, each of relative size u = 2^-24 on an intermediate no larger in magnitude than
    S = |w| + |cn| (1.0001) + 2.1 err + 8e-6 (|w| + err) + 2 s_g s_q        (the sum of the terms' magnitudes)
so |fl(bound) - bound| <= 13 u S (1 + 13 u): taken as delta = 16 u S per entry, whichever contraction into fmas the compiler
chooses (an fma only removes a rounding).  The threshold is the k-th largest of the vouching lower bounds, and an order
statistic moves by at most the largest move of its arguments: |tau2 - T| <= delta_max over the vouching entries.  So with
slack(e) = delta_e + delta_max the kernel must keep e when ub_e >= T + slack(e), and must drop it when ub_e < T_low - slack(e);
in between the checker, which never reads the kernel's bounds, does not decide (``undecided``; the cases are chosen so that
this is at most 5 % of a list, asserted on the CPU).  T_low: in the branch that takes the threshold by ``block_kth_threshold``
the kernel's tau2 is its k-th largest lower bound with the low KTH_LOW_BIT bits of the ordered pattern cleared, so T_low =
that clearing applied to fl32(T - delta_max) (clearing is monotone); in the wave-list branch T_low = T - delta_max.
Nothing here was tuned against an output.

Normalisation (``normalize_tolerance``).  s = sum x^2 by one fma per element, pitch / 64 deep per lane, then six adds; every
term is non-negative, so fl(s) = s (1 + theta), |theta| <= (m + 6) u / (1 - (m + 6) u), m = ceil(pitch / 64).  The square root
halves that and adds its own rounding, the division adds one: relative error of an element at most ((m + 6) / 2 + 2) u to
first order; the tolerance allows the square root and the division one ulp (2 u) each instead of half: ((m + 6) / 2 + 4) u."""
import ctypes as C
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from rank_harness import f2ord, ord2f

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "kernel_harness" / "stage_harness.hip"
LIBRARY = ROOT / "tests" / "kernel_harness" / "libstage_harness.so"

U = 2.0 ** -24
F32, F64, U32, U64, I32, I64 = np.float32, np.float64, np.uint32, np.uint64, np.int32, np.int64
COS, L2 = 0, 1  # WDBX_METRIC_COSINE, WDBX_METRIC_L2 (include/wdbx_hip.h)
GUARD = 64
SENT_KEY, SENT_U32, SENT_F32_BITS = 0xDEADBEEFCAFEF00D, 0xABABABAB, 0x7FC12345
INT_MIN = -(1 << 31)
D_UNKNOWN = 0x800000  # the 24-bit field's "unknown"
SCATTER_LISTS, REFINE_R, KTH_LOW_BIT = 16, 8, 8
GAMMA = F32(2e-6)  # kernels_range_batch.h::RANGE_BATCH_GAMMA


def sent_f32(n):
    return np.full(n, SENT_F32_BITS, U32).view(F32)


# --------------------------------------------------------------------------- #
# scatter_pairs_kernel
# --------------------------------------------------------------------------- #
def make_pairs(D, q, row):
    """(D's low 24 bits << 40) | (q << 32) | row, as the tile kernel appends them"""
    return ((np.asarray(D, I64).astype(U64) & U64(0xFFFFFF)) << U64(40)) | (np.asarray(q, U64) << U64(32)) | np.asarray(row, U64)


def scatter_entries(pairs, bug=None):
    """the candidate entries of pairs: (uint32(D) << 32) | ~row, D the sign-extended 24-bit field, INT_MIN for the unknown pattern"""
    p = np.asarray(pairs, U64)
    hi = (p >> U64(32)).astype(U32)
    if bug == "logical_shift":
        d = (hi >> U32(8)).astype(I64)
        unknown = d == D_UNKNOWN
    else:
        d = hi.view(I32).astype(I64) >> 8
        unknown = d == -(1 << 23)
    d = np.where(unknown, INT_MIN, d)
    row = p & U64(0xFFFFFFFF)
    low = row if bug == "row_not_inverted" else (~row) & U64(0xFFFFFFFF)
    return ((d.astype(U64) & U64(0xFFFFFFFF)) << U64(32)) | low, ((p >> U64(32)) & U64(255)).astype(I64)


@dataclass
class Scatter:
    pairs: np.ndarray       # [nlists * pair_cap] uint64
    pair_count: np.ndarray  # [nlists] uint32
    nlists: int
    pair_cap: int
    cand: np.ndarray        # [nq * cap + GUARD] uint64, as uploaded
    count: np.ndarray       # [nq (+ guard)] uint32, as uploaded
    cap: int
    lost: np.ndarray        # [2] uint32: the flag and a guard word
    nq: int


def _taking_part(s):
    """the pairs that take part: the first min(pair_count[w], pair_cap) of every list, in list order"""
    take = [s.pairs[w * s.pair_cap: w * s.pair_cap + min(int(s.pair_count[w]), s.pair_cap)] for w in range(s.nlists)]
    return np.concatenate(take) if take else np.zeros(0, U64)


def scatter_py(s, bug=None):
    """one admissible outcome: every query's entries in list order behind its counter"""
    cand, count, lost = s.cand.copy(), s.count.copy(), s.lost.copy()
    if (s.pair_count > s.pair_cap).any() and bug != "lost_unset":
        lost[0] = 1
    ent, q = scatter_entries(_taking_part(s), bug)
    for qq in np.unique(q):
        mine = ent[q == qq]
        at = int(count[qq])
        room = max(0, min(len(mine), s.cap - at))
        cand[qq * s.cap + at: qq * s.cap + at + room] = mine[:room]
        count[qq] = U32(at + len(mine))
    return cand, count, lost


def check_scatter(s, cand, count, lost):
    ent, q = scatter_entries(_taking_part(s))
    want_lost = 1 if (s.pair_count > s.pair_cap).any() else int(s.lost[0])
    assert int(lost[0]) == want_lost, ("*lost", int(lost[0]), want_lost)
    assert np.array_equal(lost[1:], s.lost[1:]), "the word behind *lost"
    assert np.array_equal(count[s.nq:], s.count[s.nq:]), "the words behind the counters"
    assert np.array_equal(cand[s.nq * s.cap:], s.cand[s.nq * s.cap:]), "the guard keys behind the candidate buffers"
    for qq in range(s.nq):
        mine = np.sort(ent[q == qq])
        at, total = int(s.count[qq]), int(s.count[qq]) + len(mine)
        assert int(count[qq]) == total, ("count", qq, int(count[qq]), total)
        buf, was = cand[qq * s.cap:(qq + 1) * s.cap], s.cand[qq * s.cap:(qq + 1) * s.cap]
        lo, hi = min(at, s.cap), min(total, s.cap)
        assert np.array_equal(buf[:lo], was[:lo]) and np.array_equal(buf[hi:], was[hi:]), ("slots outside the appended range", qq)
        got = np.sort(buf[lo:hi])
        if total <= s.cap:
            assert np.array_equal(got, mine), ("multiset", qq)
        else:  # overflow: cap - at of the entries, each no more often than it occurs
            vals, n_got = np.unique(got, return_counts=True)
            v_all, n_all = np.unique(mine, return_counts=True)
            pos = np.searchsorted(v_all, vals)
            ok = (pos < len(v_all)) & (v_all[np.minimum(pos, len(v_all) - 1)] == vals) if len(v_all) else np.zeros(len(vals), bool)
            assert ok.all() and (n_got <= n_all[pos]).all(), ("overflowed buffer holds a stranger", qq)


# --------------------------------------------------------------------------- #
# mark_lost_kernel
# --------------------------------------------------------------------------- #
def mark_lost_py(count, nq, lost, cap, over_list, bug=None):
    count = count.copy()
    over = None if over_list is None else over_list.copy()
    c = count[:nq].astype(I64)
    was_over = (c >= cap) if bug == "ge_cap" else (c > cap)
    if lost is not None and int(lost[0]):
        raise_ = ~was_over
        count[:nq] = np.where(raise_, cap + 1, c).astype(U32)
    now_over = count[:nq].astype(I64) > cap
    if bug == "ge_cap":
        now_over = count[:nq].astype(I64) >= cap
    listed = np.flatnonzero(was_over if bug == "list_before_raise" else now_over)
    if over is not None:
        over[0] = len(listed)
        over[1:1 + len(listed)] = listed
    return count, over


def check_mark_lost(count_in, nq, lost, cap, over_in, count, over):
    c = count_in[:nq].astype(I64)
    want = np.where(c <= cap, cap + 1, c) if (lost is not None and int(lost[0])) else c
    assert np.array_equal(count[:nq].astype(I64), want), "counters"
    assert np.array_equal(count[nq:], count_in[nq:]), "the words behind the counters"
    if over_in is None:
        assert over is None
        return
    listed = np.flatnonzero(want > cap)
    assert int(over[0]) == len(listed), ("over_list[0]", int(over[0]), len(listed))
    assert np.array_equal(np.sort(over[1:1 + len(listed)].astype(I64)), listed), "the listed queries"
    assert np.array_equal(over[1 + len(listed):], over_in[1 + len(listed):]), "the words behind the list"


# --------------------------------------------------------------------------- #
# refine_pairs_kernel
# --------------------------------------------------------------------------- #
@dataclass
class Refine:
    metric: int
    k: int
    cap: int
    nq: int
    cand: np.ndarray    # [nq * cap + GUARD] uint64 as uploaded
    count: np.ndarray   # [nq] uint32 as uploaded
    groups: np.ndarray  # [n_groups, 4] float32 {s_g, a_g, b_g, vouch}
    gbad: np.ndarray    # [n_groups] uint64
    cn: np.ndarray      # [n_groups * 64] float32
    qpar: np.ndarray    # [nq, 4] float32 {s_q, E, M, 1 / s_q}


def entry_fields(e):
    e = np.asarray(e, U64)
    row = (~e & U64(0xFFFFFFFF)).astype(I64)
    D = (e >> U64(32)).astype(U32).view(I32).astype(I64)
    return row, D


def make_entries(D, row):
    return ((np.asarray(D, I64).astype(U64) & U64(0xFFFFFFFF)) << U64(32)) | ((~np.asarray(row, I64).astype(U64)) & U64(0xFFFFFFFF))


def refine_bounds64(c, q, entries, bug=None):
    """(bad, vouch, lb, ub, delta) per entry in float64 (module docstring); lb = -inf where the entry cannot vouch"""
    row, D = entry_fields(entries)
    g = row >> 6
    bad = ((c.gbad[g] >> (row & 63).astype(U64)) & U64(1)).astype(bool)
    gt = c.groups[g].astype(F64)
    s_q, E, M = (F64(v) for v in c.qpar[q, :3])
    Df = D.astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        err = gt[:, 1] * E + gt[:, 2] * M
        if c.metric == L2:
            cn = np.zeros(len(row)) if bug == "no_norm" else c.cn[row].astype(F64)
            ss = 2.0 * gt[:, 0] * s_q
            w = ss * Df
            lb = w - cn * F64(F32(1.0001)) - F64(F32(8e-7)) * np.abs(w) - 2.0 * err * F64(F32(1.000001))
            ub = (w - cn * F64(F32(0.9999))) + 2.0 * err * F64(F32(1.00001)) + F64(F32(8e-6)) * (np.abs(w) + err) + ss
            S = np.abs(w) + np.abs(cn) * 1.0001 + 2.1 * err + 8e-6 * (np.abs(w) + err) + np.abs(ss)
        else:
            ss = gt[:, 0] * s_q
            w = ss * Df
            lb = w - err * F64(F32(1.000001)) - F64(F32(4e-7)) * np.abs(w)
            ub = w + err * F64(F32(1.00001)) + F64(F32(4e-6)) * (np.abs(w) + err) + ss
            S = np.abs(w) + 1.1 * err + 4e-6 * (np.abs(w) + err) + np.abs(ss)
    unknown = D == INT_MIN
    vouches = gt[:, 3] == 1.0
    if bug == "all_groups_vote":
        vouches = np.ones(len(row), bool)
    lb = np.where(unknown | ~vouches | np.isnan(lb), -np.inf, lb)
    ub = np.where(unknown | ~vouches | np.isnan(ub), np.inf, ub)  # (a group that does not vouch: no bound is believed)
    if bug != "bad_rows_vote":
        lb = np.where(bad, -np.inf, lb)
    ub = np.where(bad, -np.inf, ub)
    vouch = lb > -np.inf
    delta = np.where(np.isfinite(S), 16 * U * S, 0.0)
    return bad, vouch, lb, ub, delta


def t_low_of(t, lds_branch):
    if not lds_branch:
        return t
    o = f2ord(F32(t) + F32(0.0))  # (the kernel orders lb + 0.0f)
    f = F64(ord2f(o & ~U32((1 << KTH_LOW_BIT) - 1))[0])
    return min(f, t)  # (fl32 may round up: never above what it was given)


def refine_verdict(c, q, entries, lds_branch):
    """None: the kernel must leave the list alone.  Else (bad, must_keep, must_drop, T) per entry."""
    n = len(entries)
    if n > c.cap or n <= c.k:
        return None
    bad, vouch, lb, ub, delta = refine_bounds64(c, q, entries)
    if int(vouch.sum()) < c.k:
        return None
    T = np.sort(lb[vouch])[-c.k]
    dmax = float(delta[vouch].max())
    slack = delta + dmax
    T_low = t_low_of(T - dmax, lds_branch)
    must_keep = ~bad & ((ub == np.inf) | (ub >= T + slack))
    must_drop = bad | (ub < T_low - delta)
    return bad, must_keep, must_drop, T


def undecided_share(c, lds_branch):
    """the largest share of a list's entries the checker cannot decide, over the case's queries"""
    worst = 0.0
    for q in range(c.nq):
        n = int(c.count[q])
        if n > c.cap:
            continue
        v = refine_verdict(c, q, c.cand[q * c.cap: q * c.cap + n], lds_branch)
        if v is not None:
            worst = max(worst, float((~v[1] & ~v[2]).mean()))
    return worst


def refine_py(c, lds_branch, bug=None):
    """one admissible outcome in float64: threshold = the exact k-th largest vouching lower bound, lowered as
    block_kth_threshold lowers it in the LDS branch; stable compaction"""
    cand, count = c.cand.copy(), c.count.copy()
    for q in range(c.nq):
        n = int(count[q])
        if n > c.cap or n <= c.k:
            continue
        e = cand[q * c.cap: q * c.cap + n].copy()
        bad, vouch, lb, ub, _ = refine_bounds64(c, q, e, bug if bug in ("bad_rows_vote", "all_groups_vote", "no_norm") else None)
        if int(vouch.sum()) < c.k + (1 if bug == "k_plus_1" else 0):
            continue
        T = t_low_of(np.sort(lb[vouch])[-c.k - (1 if bug == "k_plus_1" else 0)], lds_branch)
        keep = ~bad & ~((ub <= T) if bug == "non_strict" else (ub < T))
        out = e[keep]
        if bug == "duplicate" and len(out) and len(out) < n:
            out = np.concatenate([out, out[:1]])
        cand[q * c.cap: q * c.cap + len(out)] = out
        count[q] = len(out)
    return cand, count


def check_refine(c, lds_branch, cand, count):
    """-> the entries dropped over all queries (so that a test can see that the case did drop something)"""
    dropped = 0
    assert np.array_equal(cand[c.nq * c.cap:], c.cand[c.nq * c.cap:]), "the guard keys behind the lists"
    for q in range(c.nq):
        n = int(c.count[q])
        was = c.cand[q * c.cap:(q + 1) * c.cap]
        got = cand[q * c.cap:(q + 1) * c.cap]
        v = None if n > c.cap else refine_verdict(c, q, was[:n], lds_branch)
        if v is None:
            assert int(count[q]) == n and np.array_equal(got, was), ("a list the kernel must leave alone", q, n, int(count[q]))
            continue
        bad, must_keep, must_drop, T = v
        m = int(count[q])
        assert c.k <= m <= n, ("count", q, m, n)
        assert np.array_equal(got[n:], was[n:]), ("slots behind the list", q)
        out = got[:m]
        assert len(np.unique(out)) == m, ("a duplicate in the output", q)
        kept = np.isin(was[:n], out)
        assert int(kept.sum()) == m, ("the output holds a stranger", q)  # (the input's entries are distinct)
        assert not (kept & bad).any(), ("a bad row survived", q)
        assert kept[must_keep].all(), ("SAFETY: an entry whose upper bound reaches the threshold was dropped", q, T,
                                       int((must_keep & ~kept).sum()))
        assert not kept[must_drop].any(), ("TIGHTNESS: an entry whose upper bound is below the threshold was kept", q, T,
                                          int((must_drop & kept).sum()))
        dropped += n - m
    return dropped


# --------------------------------------------------------------------------- #
# place_queries_kernel, pad_tau_kernel
# --------------------------------------------------------------------------- #
def place_queries_py(q, slot_query, pitch4, out):
    out = out.copy()
    w = pitch4 * 4
    for s, src in enumerate(slot_query):
        out[s * w:(s + 1) * w] = 0.0 if src < 0 else q[src * w:(src + 1) * w]
    return out


def pad_tau_py(tau, slot_query):
    tau = tau.copy()
    tau[:len(slot_query)][np.asarray(slot_query) < 0] = np.inf
    return tau


# --------------------------------------------------------------------------- #
# range_batch_bound_kernel
# --------------------------------------------------------------------------- #
def range_batch_bound_py(nv, gbn, qpar, tau_in, tau, rc, bug=None):
    qpar, tau, rc = qpar.copy(), tau.copy(), rc.copy()
    rc[:gbn] = 0
    tau[nv:gbn] = np.inf
    up = F32(1.0) + F32(1.1920929e-7)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(nv):
            s_q, E, M, _ = qpar[r]
            G = F32(F32(GAMMA * (E if bug == "gamma_e" else M)) * F32(1.000001))
            add = F32(G * F32(1.000001))
            qpar[r, 1] = F32(F32(E + add) * up)
            if bug != "m_unwidened":
                qpar[r, 2] = F32(F32(M + add) * up)
            lim = F32(1e38) * (s_q if s_q > 0 else F32(1.0))
            tau[r] = tau_in[r] if bug == "tau_unlimited" else np.fmin(tau_in[r], lim)
    return qpar, tau, rc


def check_range_batch_bound(nv, gbn, qpar_in, tau_in, tau_was, rc_was, qpar, tau, rc):
    bits = lambda a: np.ascontiguousarray(a, F32).view(U32)  # noqa: E731
    assert np.array_equal(bits(qpar[nv:]), bits(qpar_in[nv:])), "qpar of the slots at or above nv"
    assert np.array_equal(bits(qpar[:nv, [0, 3]]), bits(qpar_in[:nv, [0, 3]])), "s_q, 1 / s_q"
    assert (rc[:gbn] == 0).all() and np.array_equal(rc[gbn:], rc_was[gbn:]), "result counters"
    assert np.array_equal(bits(tau[gbn:]), bits(tau_was[gbn:])), "tau behind the block"
    assert (tau[nv:gbn] == np.inf).all(), "tau of the padded slots"
    g = F64(GAMMA)
    for r in range(nv):
        s_q, E, M = (F64(x) for x in qpar_in[r, :3])
        E2, M2 = F64(qpar[r, 1]), F64(qpar[r, 2])
        G = g * M
        for name, a, b in (("E", E, E2), ("M", M, M2)):
            if a == np.inf:
                assert b == np.inf, (name, "+inf must stay")
                continue
            ulp = F64(np.spacing(F32(b)))
            assert b - a >= G, ("SAFETY: widened by less than gamma M", name, r, b - a, G)
            assert b - a <= G * (1 + 4e-6) + 4 * ulp, ("TIGHTNESS", name, r, b - a, G)
        with np.errstate(over="ignore"):
            lim = F32(1e38) * (F32(s_q) if s_q > 0 else F32(1.0))
        want = np.fmin(F32(tau_in[r]), lim)
        assert bits(np.array([tau[r]]))[0] == bits(np.array([want]))[0], ("tau", r, tau[r], want)


# --------------------------------------------------------------------------- #
# normalize_rows_kernel
# --------------------------------------------------------------------------- #
def normalize_tolerance(pitch):
    return ((-(-pitch // 64) + 6) / 2 + 4) * U


# --------------------------------------------------------------------------- #
# the library
# --------------------------------------------------------------------------- #
_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        for f in (lib.stage_scatter_lists, lib.stage_refine_r, lib.stage_kth_low_bit):
            f.argtypes, f.restype = [], u32
        lib.stage_range_batch_gamma.argtypes, lib.stage_range_batch_gamma.restype = [], C.c_float
        lib.stage_scatter.argtypes = [vp, u64, vp, u32, u32, vp, u64, vp, u64, u32, vp, u64]
        lib.stage_refine_shape.argtypes = [i32, u32, i32, vp]
        lib.stage_refine.argtypes = [i32, i32, i32, u32, vp, u64, vp, u32, u32, vp, u64, vp, u64, vp, u64, vp, u64]
        lib.stage_mark_lost.argtypes = [vp, u64, u32, vp, u32, vp, u64, u32]
        lib.stage_place_queries.argtypes = [vp, u64, vp, u32, u32, vp, u64]
        lib.stage_pad_tau.argtypes = [vp, u64, vp, u32]
        lib.stage_range_batch_bound.argtypes = [u32, u32, vp, u64, vp, u64, vp, u64, vp, u64]
        lib.stage_gather_rows.argtypes = [vp, u64, u32, vp, u64, vp, u64, u32]
        lib.stage_normalize_rows.argtypes = [vp, u64, u64, u32, u32]
        for f in (lib.stage_scatter, lib.stage_refine_shape, lib.stage_refine, lib.stage_mark_lost, lib.stage_place_queries, lib.stage_pad_tau,
                  lib.stage_range_batch_bound, lib.stage_gather_rows, lib.stage_normalize_rows):
            f.restype = C.c_int
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc, what):
    if rc == -1:
        raise ValueError(f"{what}: the harness refused the arguments (out of the uploaded arrays' bounds, or out of range)")
    if rc:
        raise RuntimeError(f"{what}: HIP error {rc}")


def _c(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype).copy()


def constants():
    lib = load()
    return lib.stage_scatter_lists(), lib.stage_refine_r(), lib.stage_kth_low_bit(), F32(lib.stage_range_batch_gamma())


def scatter(s):
    cand, count, lost = _c(s.cand, U64), _c(s.count, U32), _c(s.lost, U32)
    pairs, pc = _c(s.pairs, U64), _c(s.pair_count, U32)
    _check(load().stage_scatter(_ptr(pairs), len(pairs), _ptr(pc), s.nlists, s.pair_cap, _ptr(cand), len(cand), _ptr(count), len(count),
                                s.cap, _ptr(lost), len(lost)), "stage_scatter")
    return cand, count, lost


def refine_shape(k, cap, lds_lists=False):
    """(reg, waves, n_lds, lds bytes, raise) of the launch"""
    out = np.zeros(5, U64)
    _check(load().stage_refine_shape(int(k), int(cap), int(lds_lists), _ptr(out)), "stage_refine_shape")
    return tuple(int(x) for x in out)


def refine(c, lds_lists=False, n_lds=0):
    cand, count = _c(c.cand, U64), _c(c.count, U32)
    groups, gbad, cn, qpar = _c(c.groups, F32), _c(c.gbad, U64), _c(c.cn, F32), _c(c.qpar, F32)
    _check(load().stage_refine(c.metric, c.k, int(lds_lists), int(n_lds), _ptr(cand), len(cand), _ptr(count), c.nq, c.cap, _ptr(groups),
                               len(groups), _ptr(gbad), len(gbad), _ptr(cn), len(cn), _ptr(qpar), len(qpar)), "stage_refine")
    return cand, count


def mark_lost(count, nq, lost, cap, over_list, threads=0):
    count, lost, over = _c(count, U32), _c(lost, U32), _c(over_list, U32)
    _check(load().stage_mark_lost(_ptr(count), len(count), int(nq), _ptr(lost), int(cap), _ptr(over), 0 if over is None else len(over),
                                  int(threads)), "stage_mark_lost")
    return count, over


def place_queries(q, slot_query, pitch4, out):
    q, sq, out = _c(q, F32), _c(slot_query, I32), _c(out, F32)
    _check(load().stage_place_queries(_ptr(q), len(q) // (4 * pitch4), _ptr(sq), int(pitch4), len(sq), _ptr(out), len(out) // 4),
           "stage_place_queries")
    return out


def pad_tau(tau, slot_query):
    tau, sq = _c(tau, F32), _c(slot_query, I32)
    _check(load().stage_pad_tau(_ptr(tau), len(tau), _ptr(sq), len(sq)), "stage_pad_tau")
    return tau


def range_batch_bound(nv, gbn, qpar, tau_in, tau, rc):
    qpar, tau_in, tau, rc = _c(qpar, F32), _c(tau_in, F32), _c(tau, F32), _c(rc, U32)
    _check(load().stage_range_batch_bound(int(nv), int(gbn), _ptr(qpar), len(qpar), _ptr(tau_in), len(tau_in), _ptr(tau), len(tau), _ptr(rc),
                                          len(rc)), "stage_range_batch_bound")
    return qpar, tau, rc


def gather_rows(rows, pitch4, src, dst, grid=0):
    rows, src, dst = _c(rows, F32), _c(src, U64), _c(dst, F32)
    w = 4 * pitch4
    _check(load().stage_gather_rows(_ptr(rows), len(rows) // w, int(pitch4), _ptr(src), len(src), _ptr(dst), len(dst) // w, int(grid)),
           "stage_gather_rows")
    return dst


def normalize_rows(rows, n, pitch, grid=0):
    rows = _c(rows, F32)
    _check(load().stage_normalize_rows(_ptr(rows), len(rows) // pitch, int(n), int(pitch), int(grid)), "stage_normalize_rows")
    return rows
