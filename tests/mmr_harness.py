"""ctypes loader of tests/kernel_harness/libmmr_harness.so (built by ``make -C wdbx-py_amd/csrc all``) and the plain numpy
references of the two kernels it launches, ``mmr_pairs_kernel`` and ``mmr_select_kernel``.

The references never look at the code under test.  ``greedy_f32`` is the selection of include/wdbx_hip.h written down as a
loop: every product and difference one numpy float32 operation (numpy rounds each to nearest, as ``__fmul_rn`` / ``__fsub_rn``
do; it has no fused multiply-add to contract into), ``maxsim`` folded with a NaN-ignoring maximum, the winner the unpicked
position with the largest value, ties (``-0 == +0`` among them) to the smaller position, NaN values below every number.
``greedy_exact`` is the same loop over ``fractions.Fraction`` for the integer corpora, where no operation rounds.  Scores of
the pairs kernel are judged by the statements of tests/listed_harness.py (integer corpora ``==``, float corpora inside
``score_bound64`` and bit-equal to ``rescore_kernel``)."""
import ctypes as C
from fractions import Fraction
from pathlib import Path

import numpy as np

from select_harness import GUARD, METRIC_COSINE, METRIC_L2  # noqa: F401  (re-exported)

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "kernel_harness" / "mmr_harness.hip"
LIBRARY = ROOT / "tests" / "kernel_harness" / "libmmr_harness.so"

_U32, _U64, _I64, _F32 = np.uint32, np.uint64, np.int64, np.float32
MAX_POOL = 2048
SENT_G = np.array([0x7FC12345], _U32).view(_F32)[0]  # a NaN with a payload no kernel produces
SENT_IDX = np.int64(-0x2152411021524111)
SENT_OUT = np.array([0x4B1D4B1D], _U32).view(_F32)[0]


def table_of(ms):
    """pool sizes -> the query table [nq, 4] uint32 (row0, m, g0 low, g0 high), rows and squares back to back"""
    ms = np.asarray(ms, _I64)
    row0 = np.concatenate([[0], np.cumsum(ms)[:-1]])
    g0 = np.concatenate([[0], np.cumsum(ms * ms)[:-1]])
    return np.stack([row0, ms, g0 & 0xFFFFFFFF, g0 >> 32], axis=1).astype(_U32)


def squares(buf, ms):
    """the flat G buffer -> one [m, m] view per query"""
    out, at = [], 0
    for m in ms:
        out.append(buf[at:at + m * m].reshape(m, m))
        at += m * m
    return out


# --------------------------------------------------------------------------- #
# references
# --------------------------------------------------------------------------- #
def _better(v, best):
    """v beats best: a number beats NaN, a larger number beats a smaller one; equal values (and two NaNs) do not"""
    if np.isnan(v):
        return False
    return np.isnan(best) or v > best


def greedy_f32(rel, G, lam, k):
    """rel [m] float32 (ranking domain), G [m, m] float32 -> (positions [picks], values float32 [picks])"""
    rel, G, lam = np.asarray(rel, _F32), np.asarray(G, _F32), _F32(lam)
    m = rel.size
    picks = min(int(k), m)
    if picks == 0:
        return np.zeros(0, _I64), np.zeros(0, _F32)
    with np.errstate(invalid="ignore", over="ignore"):
        lrel = (lam * rel).astype(_F32)
        one_minus = _F32(_F32(1.0) - lam)
        maxsim = np.full(m, -np.inf, _F32)
        picked = np.zeros(m, bool)
        pos, val = [0], [lrel[0]]
        picked[0] = True
        while len(pos) < picks:
            g = G[pos[-1]]
            maxsim = np.where(np.isnan(g), maxsim, np.maximum(maxsim, g)).astype(_F32)
            v = (lrel - (one_minus * maxsim).astype(_F32)).astype(_F32)
            best = -1
            for i in np.flatnonzero(~picked):
                if best < 0 or _better(v[i], v[best]):
                    best = int(i)
            picked[best] = True
            pos.append(best)
            val.append(v[best])
    return np.asarray(pos, _I64), np.asarray(val, _F32)


def greedy_fast_f32(rel, G, lam, k):
    """greedy_f32 with the inner scan vectorised (the same operations; for the large shapes)"""
    rel, G, lam = np.asarray(rel, _F32), np.asarray(G, _F32), _F32(lam)
    m = rel.size
    picks = min(int(k), m)
    if picks == 0:
        return np.zeros(0, _I64), np.zeros(0, _F32)
    with np.errstate(invalid="ignore", over="ignore"):
        lrel = (lam * rel).astype(_F32)
        one_minus = _F32(_F32(1.0) - lam)
        maxsim = np.full(m, -np.inf, _F32)
        picked = np.zeros(m, bool)
        pos, val = [0], [lrel[0]]
        picked[0] = True
        while len(pos) < picks:
            g = G[pos[-1]]
            maxsim = np.where(np.isnan(g), maxsim, np.maximum(maxsim, g)).astype(_F32)
            v = (lrel - (one_minus * maxsim).astype(_F32)).astype(_F32)
            free = np.flatnonzero(~picked)
            vf = v[free]
            if np.all(np.isnan(vf)):
                best = int(free[0])
            else:
                best = int(free[np.flatnonzero(vf == np.nanmax(vf))[0]])
            picked[best] = True
            pos.append(best)
            val.append(v[best])
    return np.asarray(pos, _I64), np.asarray(val, _F32)


def greedy_exact(rel, G, lam, k):
    """integers rel [m], G [m, m] and a Fraction lambda -> (positions, Fraction values); no rounding anywhere"""
    m = len(rel)
    picks = min(int(k), m)
    if picks == 0:
        return [], []
    lam = Fraction(lam)
    lrel = [lam * int(r) for r in rel]
    maxsim = [None] * m
    picked = [False] * m
    pos, val = [0], [lrel[0]]
    picked[0] = True
    while len(pos) < picks:
        p = pos[-1]
        best, best_v = -1, None
        for i in range(m):
            g = int(G[p][i])
            maxsim[i] = g if maxsim[i] is None else max(maxsim[i], g)
            if picked[i]:
                continue
            v = lrel[i] - (1 - lam) * maxsim[i]
            if best < 0 or v > best_v:
                best, best_v = i, v
        picked[best] = True
        pos.append(best)
        val.append(best_v)
    return pos, val


def expect_select(ms, G, cand, rel, lam, k, negate, greedy=greedy_f32):
    """the whole output of a launch: (idx int64 [nq * k + GUARD], score, mmr), sentinels behind"""
    nq = len(ms)
    idx = np.full(nq * k + GUARD, SENT_IDX, _I64)
    score = np.full(nq * k + GUARD, SENT_OUT, _F32)
    mmr = np.full(nq * k + GUARD, SENT_OUT, _F32)
    idx[:nq * k], score[:nq * k], mmr[:nq * k] = -1, 0.0, 0.0
    row0 = 0
    for q, (m, g) in enumerate(zip(ms, squares(G, ms))):
        r = np.asarray(rel[row0:row0 + m], _F32)
        pos, val = greedy(r, g, lam, k)
        n = len(pos)
        idx[q * k:q * k + n] = np.asarray(cand[row0:row0 + m], _I64)[pos]
        score[q * k:q * k + n] = -r[pos] if negate else r[pos]
        mmr[q * k:q * k + n] = val
        row0 += m
    return idx, score, mmr


def same_f32(got, want, what=""):
    """bit-equal float32 words, or NaN on both sides (0 x inf has no specified sign or payload); None when equal, else the
    first difference"""
    got, want = np.asarray(got, _F32), np.asarray(want, _F32)
    if got.shape != want.shape:
        return f"{what}: shape {got.shape}, not {want.shape}"
    g, w = got.reshape(-1), want.reshape(-1)
    bad = np.flatnonzero((g.view(_U32) != w.view(_U32)) & ~(np.isnan(g) & np.isnan(w)))
    if bad.size == 0:
        return None
    i = int(bad[0])
    return f"{what}: {bad.size} words differ, first {i}: {got.reshape(-1)[i]!r}, not {want.reshape(-1)[i]!r}"


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
        lib.mmr_pairs.argtypes = [i32, vp, u64, u32, vp, u32, vp, u64]
        lib.mmr_select.argtypes = [vp, u32, vp, u64, vp, vp, u64, vp, vp, vp, u64, C.c_float, i32, i32]
        lib.mmr_pairs.restype = lib.mmr_select.restype = C.c_int
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc, what):
    if rc == -1:
        raise ValueError(f"{what}: the harness refused the arguments (out of the uploaded arrays' bounds, or no such instance)")
    if rc:
        raise RuntimeError(f"{what}: HIP error {rc}")


def pairs(metric, rows, ms, front=0):
    """mmr_pairs_kernel on gathered rows [sum ms, pitch] -> the whole G buffer: `front` sentinel words, the squares back to
    back, GUARD sentinel words (the table's g0 are shifted by front)."""
    rows = np.ascontiguousarray(rows, _F32)
    assert rows.ndim == 2 and rows.shape[1] % 4 == 0 and rows.shape[0] == sum(ms)
    table = table_of(ms)
    g0 = (table[:, 2].astype(_U64) | (table[:, 3].astype(_U64) << _U64(32))) + _U64(front)
    table[:, 2], table[:, 3] = (g0 & _U64(0xFFFFFFFF)).astype(_U32), (g0 >> _U64(32)).astype(_U32)
    table = np.ascontiguousarray(table)
    words = front + sum(m * m for m in ms) + GUARD
    buf = np.full(words, SENT_G, _F32)
    rc = load().mmr_pairs(int(metric), _ptr(rows), rows.shape[0], rows.shape[1] // 4, _ptr(table), len(ms), _ptr(buf), buf.size)
    _check(rc, "mmr_pairs")
    return buf


def select(ms, G, cand, rel, lam, k, negate=False, with_mmr=True):
    """mmr_select_kernel -> (idx, score, mmr), each nq * k words and GUARD sentinels behind (mmr None without the array)"""
    table = np.ascontiguousarray(table_of(ms))
    G = np.ascontiguousarray(G, _F32).reshape(-1)
    if G.size == 0:
        G = np.zeros(1, _F32)
    cand = np.ascontiguousarray(cand, _U64)
    rel = np.ascontiguousarray(rel, _F32)
    if cand.size == 0:
        cand, rel = np.zeros(1, _U64), np.zeros(1, _F32)
    n = len(ms) * k + GUARD
    idx = np.full(n, SENT_IDX, _I64)
    score = np.full(n, SENT_OUT, _F32)
    mmr = np.full(n, SENT_OUT, _F32) if with_mmr else None
    rc = load().mmr_select(_ptr(table), len(ms), _ptr(G), G.size, _ptr(cand), _ptr(rel), cand.size, _ptr(idx), _ptr(score), _ptr(mmr),
                           n, float(lam), int(k), int(bool(negate)))
    _check(rc, "mmr_select")
    return idx, score, mmr
