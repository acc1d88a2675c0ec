"""The reference fold of the discovery search (``wdbx_index_search_discover``, include/wdbx_hip.h), in numpy float32
operations in the contract's order.  It never looks at the code under test: it takes ``r``, the scores in the ranking domain
(float32; NaN = the score is NaN) that the library's own exact path returned -- ``rescore_kernel`` in the kernel tests,
``wdbx_index_search_rows`` in the C ABI tests -- and folds them per pair:

* ``wins = #{i : r(p_i) > r(n_i)}`` (a tie is no win);
* ``loss = sum_i fminf(r(p_i) - r(n_i), 0.0f)``, accumulated in float32 from 0.0f in pair order;
* a row is dead when any ``r(p_i) - r(n_i)`` is NaN (a NaN score, inf - inf) or the target's score is NaN.

Target mode orders by (wins descending, ``t = r(target) + 0.0f`` descending, row ascending); context mode by (``loss + 0.0f``
descending, row ascending)."""
import numpy as np

_F32, _U32, _U64, _I64 = np.float32, np.uint32, np.uint64, np.int64
MAX_PAIRS = 32
ZONES = MAX_PAIRS + 1


def fold(r_ctx):
    """r_ctx [2 * pairs, rows] (pair i: rows 2 i positive, 2 i + 1 negative) -> (wins int64 [rows], loss f32 [rows], dead bool
    [rows])"""
    r_ctx = np.asarray(r_ctx, _F32)
    n_rows = r_ctx.shape[1]
    wins = np.zeros(n_rows, _I64)
    loss = np.zeros(n_rows, _F32)
    dead = np.zeros(n_rows, bool)
    with np.errstate(invalid="ignore"):
        for i in range(r_ctx.shape[0] // 2):
            p, n = r_ctx[2 * i], r_ctx[2 * i + 1]
            d = (p - n).astype(_F32)
            dead |= np.isnan(d)
            wins += p > n
            loss = (loss + np.fmin(d, _F32(0.0))).astype(_F32)
    return wins, loss, dead


def target_fold(r_target, r_ctx, eligible):
    """-> (t f32 [rows], wins int64 [rows], alive bool [rows]): t = r(target) + 0.0f; alive rows may be returned"""
    r_target = np.asarray(r_target, _F32)
    wins, _, dead = fold(np.asarray(r_ctx, _F32).reshape(-1, r_target.size))
    alive = np.asarray(eligible, bool) & ~dead & ~np.isnan(r_target)
    return (r_target + _F32(0.0)).astype(_F32), wins, alive


def context_fold(r_ctx, eligible):
    """-> (loss + 0.0f f32 [rows], alive bool [rows])"""
    _, loss, dead = fold(r_ctx)
    return (loss + _F32(0.0)).astype(_F32), np.asarray(eligible, bool) & ~dead


def _pad(rows, score, wins, k):
    n = min(len(rows), k)
    idx = np.full(k, -1, _I64)
    sc = np.zeros(k, _F32)
    w = np.zeros(k, np.uint8)
    idx[:n], sc[:n], w[:n] = rows[:n], score[:n], wins[:n]
    return idx, sc, w


def target_answer(r_target, r_ctx, eligible, k, l2=False):
    """the contract's answer of one query: (idx int64 [k], score f32 [k], wins uint8 [k]); score in the caller's units (L2:
    the positive squared distance, -t + 0.0f); unused slots -1 / 0 / 0"""
    t, wins, alive = target_fold(r_target, r_ctx, eligible)
    rows = np.flatnonzero(alive)
    order = rows[np.lexsort((rows, -t[rows].astype(np.float64), -wins[rows]))]
    score = ((-t[order]) + _F32(0.0)).astype(_F32) if l2 else t[order]
    return _pad(order, score, wins[order], k)


def context_answer(r_ctx, eligible, k):
    """... of a context-mode query: the score is the loss as computed (<= 0, the ranking domain for either metric), wins 0"""
    loss, alive = context_fold(r_ctx, eligible)
    rows = np.flatnonzero(alive)
    order = rows[np.lexsort((rows, -loss[rows].astype(np.float64)))]
    return _pad(order, loss[order], np.zeros(order.size, np.uint8), k)
