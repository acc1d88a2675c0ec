"""The split planes' full pass with 2 and 4 queries per read of the four-bit plane (scan_u42_kernel<UC, QP>, kernels_scan42.h)
against the same harness's QP = 1 launches, the kernel alone: per query the survivor counter, the candidate count and the
sorted candidate keys must be equal bit for bit (the order in which waves append is not defined for the lone pass either).

4 096 + 37 rows (a partial last tile), planes from rows_to_u42_kernel, d = 64 (2 units: a short last chunk at UC = 4), 192
(6 units) and 384 (12 units).  Eight (query, threshold) slots, so that the groups of QP = 2 are slots {0,1} {2,3} {4,5} {6,7}
and those of QP = 4 are {0 .. 3} {4 .. 7}:
  0  query A, -inf      every row survives: a refine on every tile
  1  query B, 1e30      keeps no row
  2  query C, quarter   about a quarter of the rows survive: more than 64 per wave, refines in mid-pass
  3  query C, quarter   the same query twice in one group
  4  query D, quarter   } a pair of two DIFFERENT queries that both refine in mid-pass, at different rates: the two lists
  5  query A, half      } reach 64 on different tiles
  6  query D, few       about 40 survivors in all: refined behind the last tile only
  7  query B, 1e30
The thresholds are order statistics of the four-bit upper bound w4 + m4 of the numpy restatement
(tests/test_selection_bounds_u42.py); the conditions they are chosen for are asserted on the QP = 1 results."""
import numpy as np
import pytest

import select_harness as S
import u42_share_harness as H
from test_selection_bounds_u42 import quantise_u42, u42_bound, u42_first

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 4096 + 37
TILES = (N + 63) // 64
DIMS = [64, 192, 384]
GRIDS = [1, 3]  # 4 and 12 waves: 16 - 17 and 5 - 6 tiles per wave
_CASE = {}
_LONE = {}


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(F32)


def _case(d):
    """rows, planes, the eight slots: computed once per dimension and shared, never modified"""
    if d not in _CASE:
        rng = np.random.default_rng(4242 + d)
        rows = _unit(rng.random((N, d)) * 2 - 1)
        qa, qb, qc, qd = _unit(rng.random((4, d)) * 2 - 1)
        h, _, s, a4, _ = quantise_u42(rows)

        def up4(q):
            return np.sort((u42_first(h, s, q)[1] + u42_bound(s, a4, q, d)).astype(F32))[::-1]

        none = F32(1e30)
        quarter, quarter_d, few, half = F32(up4(qc)[N // 4]), F32(up4(qd)[N // 4]), F32(up4(qd)[40]), F32(up4(qa)[N // 2])
        queries = np.stack([qa, qb, qc, qc, qd, qa, qd, qb])
        tau = np.array([-np.inf, none, quarter, quarter, quarter_d, half, few, none], F32)
        _CASE[d] = dict(planes=H.quantise(rows, d), queries=queries, tau=tau)
    return _CASE[d]


def _lone(d, grid_x):
    """the QP = 1 launch all shared ones are compared with; the premises of the case are asserted here"""
    if (d, grid_x) not in _LONE:
        c = _case(d)
        r = H.scan(c["planes"], c["queries"], N, c["tau"], N, grid_x, 1)
        assert (r["guard"] == S.SENT_KEY).all()
        surv, count = r["survivors"].astype(np.int64), r["count"].astype(np.int64)
        print(f"d={d} grid_x={grid_x}: survivors {surv.tolist()}, candidates {count.tolist()}")
        waves = 4 * grid_x
        assert surv[0] == count[0] == N                                    # every tile fills a wave's list
        assert surv[1] == count[1] == 0 and surv[7] == count[7] == 0       # a query of a group that keeps no row
        assert 64 * waves < surv[2] < N // 2 and surv[3] == surv[2]         # some wave holds more than 64: a refine in mid-pass
        assert 0 < surv[6] < 64                                             # ... and one that refines behind the last tile only
        # slots 4 and 5, one pair: both hold more than 64 per wave somewhere, so both refine in mid-pass.  A wave with x
        # survivors refines floor(x / 64) times at 64 (the rest goes behind its last tile), so slot 4 refines at most
        # surv[4] // 64 times in all and slot 5 at least (surv[5] - 63 waves) // 64 times: more often, hence on tiles on which
        # slot 4 does not -- the two queries of the pair cross 64 on different tiles
        assert 64 * waves < surv[4] < N // 2 and 64 * waves < surv[5] < N - 64 * waves
        assert surv[4] != surv[5] and (surv[5] - 63 * waves) // 64 > surv[4] // 64
        assert (count <= surv).all()
        _LONE[(d, grid_x)] = r
    return _LONE[(d, grid_x)]


def _keys(r, i):
    n = int(r["count"][i])
    assert n <= r["cand"].shape[1]
    return np.sort(r["cand"][i, :n])


@pytest.mark.parametrize("grid_x", GRIDS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("qp", [2, 4])
def test_shared_pass_equals_the_lone_passes(qp, d, grid_x):
    c, one = _case(d), _lone(d, grid_x)
    r = H.scan(c["planes"], c["queries"], N, c["tau"], N, grid_x, qp)
    assert (r["guard"] == S.SENT_KEY).all()
    assert np.array_equal(r["survivors"], one["survivors"])
    assert np.array_equal(r["count"], one["count"])
    for i in range(8):
        n = int(r["count"][i])
        assert np.array_equal(_keys(r, i), _keys(one, i)), (qp, d, grid_x, i)
        assert (r["cand"][i, n:] == S.SENT_KEY).all()
        rows = S.key_row(r["cand"][i, :n])
        assert rows.size == np.unique(rows).size and (n == 0 or rows.max() < N)
    # the query that appears twice in one group
    assert int(r["count"][2]) > 0 and np.array_equal(_keys(r, 2), _keys(r, 3))


@pytest.mark.parametrize("pair", ["all_few", "both_refine"])
@pytest.mark.parametrize("qp", [2, 4])
def test_overflow_of_one_query_leaves_its_neighbours_complete(qp, pair):
    """A capacity between the candidate counts of a pair's two queries: the larger one overflows (its counter counts on to the
    exact total, the first cap keys are valid keys of its lone pass), the other one in the same group is complete and within
    capacity.  all_few: {A -inf, D few} at cap = 128; both_refine: {A half, D quarter}, both refining in mid-pass, at the mean
    of their two candidate counts.  At QP = 4 the group holds the pair twice."""
    d, grid_x = 192, 3
    c, one = _case(d), _lone(d, grid_x)
    big, small = (0, 6) if pair == "all_few" else (5, 4)
    n_big, n_small = int(one["count"][big]), int(one["count"][small])
    cap = 128 if pair == "all_few" else (n_big + n_small) // 2
    assert 0 < n_small <= cap < n_big
    pick = [big, small, big, small]
    r = H.scan(c["planes"], c["queries"][pick], N, c["tau"][pick], cap, grid_x, qp)
    assert (r["guard"] == S.SENT_KEY).all()
    for slot, i in enumerate(pick):
        assert int(r["survivors"][slot]) == int(one["survivors"][i])
        assert int(r["count"][slot]) == int(one["count"][i])
        if i == big:
            rows = S.key_row(r["cand"][slot])
            assert rows.size == np.unique(rows).size == cap and rows.max() < N
            assert np.isin(r["cand"][slot], one["cand"][big, :n_big]).all()
        else:
            assert np.array_equal(_keys(r, slot), _keys(one, i))
            assert (r["cand"][slot, n_small:] == S.SENT_KEY).all()
