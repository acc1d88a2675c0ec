"""A round's matrix-core groups in ONE launch (scan_u42_mfma_kernel with grid (grid_x, groups), kernels_scan42.h): the groups are
resident together and walk the tiles together.  What a query gets must not depend on that: per query the survivors counter, the
words of surv_p and the set of candidate keys equal those of the same queries launched 16 at a time (grid (3, 1): another split
of the tiles over the waves).  The harness launches pick_scan42_mfma's instance (non-temporal loads) in both shapes; the instance
with plain loads, which the library runs for such a launch, differs in the loads' cache policy alone and is held to the VALU
passes' answers through the library (tests/test_gpu_u42_round_calls.py).

6144 + 37 rows x 384: three tiles per wave at grid_x = 8 and a ragged last tile; at grid_x = 16 some waves take one tile and
some two.  nq = 32, 64 and 54 (a short last group of 6).  Thresholds per column in turn -inf (every row survives both stages),
the median exact score (half of them at least) and +inf (none); query 23, one of the +inf columns, holds a NaN and is MARKED:
every row is its candidate whatever its threshold says."""
import numpy as np
import pytest

import select_harness as S
import u42_mfma_harness as MH
import u42_share_harness as H

pytestmark = pytest.mark.gpu

F32 = np.float32
N, D, NQ = 6144 + 37, 384, 64
MARKED_QUERY = 23
_CACHE = {}


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(F32)


def _case():
    """planes, queries, thresholds and the reference: the four groups launched one at a time with grid_x = 3, computed once"""
    if not _CACHE:
        rng = np.random.default_rng(4242)
        rows, queries = _unit(rng.standard_normal((N, D))), _unit(rng.standard_normal((NQ, D)))
        med = np.median(rows.astype(np.float64) @ queries.astype(np.float64).T, axis=0).astype(F32)
        tau = np.where(np.arange(NQ) % 3 == 0, -np.inf, np.where(np.arange(NQ) % 3 == 1, med, np.inf)).astype(F32)
        queries[MARKED_QUERY, 17] = np.nan
        assert tau[MARKED_QUERY] == np.inf
        planes = H.quantise(rows, D)
        ref = []
        for g in range(NQ // 16):
            r = MH.scan(planes, queries[16 * g:16 * g + 16], N, tau[16 * g:16 * g + 16], N, 3)
            assert (r["guard"] == S.SENT_KEY).all()
            ref.append(r)
        for r in ref:
            for a in r.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _CACHE.update(planes=planes, queries=queries, tau=tau, ref=ref)
    return _CACHE


def _keys(r, j, cap):
    held = min(int(r["count"][j]), cap)
    assert (r["cand"][j, held:] == S.SENT_KEY).all()
    return r["cand"][j, :held]


def _check(c, r, nq, cap):
    assert (r["guard"] == S.SENT_KEY).all()
    for j in range(nq):
        ref, k = c["ref"][j // 16], j % 16
        assert int(r["survivors"][j]) == int(ref["survivors"][k]), j
        assert np.array_equal(r["surv_p"][j], ref["surv_p"][k]), j
        assert int(r["count"][j]) == int(ref["count"][k]), j
        want, got = _keys(ref, k, N), _keys(r, j, cap)
        if int(r["count"][j]) <= cap:
            assert np.array_equal(np.sort(got), np.sort(want)), j
        else:  # overflow: cap distinct keys of the column's own, nothing behind them
            assert got.size == cap and np.unique(got).size == cap and np.isin(got, want).all(), j


@pytest.mark.parametrize("grid_x", [8, 16])
@pytest.mark.parametrize("nq", [32, 64, 54])
def test_groups_in_one_launch_equal_a_launch_per_group(nq, grid_x):
    c = _case()
    r = MH.scan(c["planes"], c["queries"][:nq], N, c["tau"][:nq], N, grid_x)
    _check(c, r, nq, N)
    # the three kinds of columns are what they were meant to be, and the marked query keeps every row
    count = r["count"][:nq].astype(np.int64)
    kind, plain = np.arange(nq) % 3, np.arange(nq) != MARKED_QUERY
    assert (count[kind == 0] == N).all() and (count[(kind == 2) & plain] == 0).all()
    assert (count[kind == 1] >= N // 2).all() and (count[kind == 1] < N).all()
    assert count[MARKED_QUERY] == N and r["qc"]["flags"][MARKED_QUERY] == MH.MARKED
    assert (r["qc"]["flags"][nq:] == MH.ABSENT).all()


def test_a_small_capacity_overflows_per_column():
    c = _case()
    cap = 5
    r = MH.scan(c["planes"], c["queries"], N, c["tau"], cap, 8)
    _check(c, r, NQ, cap)
    assert (r["count"] > cap).sum() >= NQ // 3 * 2 - 2
