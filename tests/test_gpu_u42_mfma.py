"""The split planes' full pass on the matrix cores (u42_query_i16_kernel + scan_u42_mfma_kernel, kernels_scan42.h), the kernels
alone: the query's 16-bit operands and constants, the survivor entries (2^-9 P^ bit for bit from the exact integer sum), the
survivor and candidate sets against float64, the candidate keys against the float64 form of w6, overflow, bad rows and
marked queries.

1000 rows (neither a multiple of 64 nor of 16), planes from rows_to_u42_kernel, d = 384 (12 units) and 352, 320, 288 (11, 10
and 9 units: a short last chunk with three, two and one live lane groups).  Sixteen (query, threshold) slots of one group:
  0  query A, -inf     every row survives: its list is refined behind every 16-row block that fills it to 48
  1  query B, +inf     keeps no row
  2  query C, quarter  about a quarter of the rows survive: the lists come due in mid-pass, on other tiles than slot 0's
  3  query C, quarter  the same query twice in one group
  4  query D, few      about 40 survivors in all: refined behind the last tile only
  5 .. 15              further queries at thresholds between a tenth and nine tenths of the rows
Thresholds are order statistics of the float64 scores.  A marked query (see kernels_scan42.h) has its threshold read as -inf
in both stages: every row is its candidate and the counter ends above a capacity below the row count, behind `cap` real keys
-- the kernel does not leave the buffer empty, since rescore_kernel reads min(count, cap) keys and they must name rows."""
import numpy as np
import pytest

import select_harness as S
import u42_harness as U
import u42_mfma_harness as MH
import u42_mfma_model as M
import u42_share_harness as H

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
N = 1000
DIMS = [384, 352, 320, 288]  # 12, 11, 10 and 9 units: every unit count with an instance
_CASE = {}


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(F32)


def _case(d, bad=False):
    """rows, planes and their numpy reading, sixteen slots: computed once per dimension and shared, never modified"""
    if (d, bad) not in _CASE:
        rng = np.random.default_rng(4616 + d)
        rows = _unit(rng.random((N, d)) * 2 - 1)
        if bad:
            rows[5, 7] = np.nan       # a negative scale: skipped
            rows[9, 3] = np.inf       # a NaN scale: survives every comparison, appended with +inf
            rows[N - 1, :] = -np.inf
        queries = _unit(rng.standard_normal((16, d)))
        queries[3] = queries[2]
        planes = H.quantise(rows, d)
        truth = np.stack([S.scores64(np.nan_to_num(rows, nan=0.0, posinf=0.0, neginf=0.0), q) for q in queries])
        order = np.sort(truth, axis=1)[:, ::-1]
        frac = [0, 0, 0.25, 0.25, 0.04, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.15, 0.02]
        tau = np.array([order[i, int(f * N)] for i, f in enumerate(frac)], F32)
        tau[0], tau[1] = -np.inf, np.inf
        l, a6 = U.unpack_l(planes["lrec"], d // 32)
        _CASE[(d, bad)] = dict(rows=rows, planes=planes, queries=queries, tau=tau, truth=truth, h=U.unpack_h(planes["h"], N),
                               l=l, a6=a6.view(F32), s=planes["sa4"][:, 0], a4=planes["sa4"][:, 1])
    return _CASE[(d, bad)]


def _check_query(c, r, slot, qi, t, cap, good=None):
    """one query of a launch against the restatement and float64; -> (survivors, candidates)"""
    q, d = c["queries"][qi], c["queries"].shape[1]
    good = np.ones(N, bool) if good is None else good
    qq = M.quantise_query(q)
    kc = {name: r["qc"][name][slot] for name in MH.QC_FIELDS}
    assert r["qc"]["flags"][slot] == 0
    # the operands: H and L of every element, in the fragments' order
    assert np.array_equal(r["bytes"][slot, 0], qq["H"]) and np.array_equal(r["bytes"][slot, 1], qq["L"])
    assert not r["pad_bytes"][slot].any()
    assert kc["delta"] == qq["delta"] and kc["dp"] == qq["delta"] * F32(2.0 ** -9)
    real = np.linalg.norm(q.astype(F64) - F64(qq["delta"]) * qq["Q"])
    assert real <= F64(kc["e2"]) <= 1.001 * real + 1e-19
    want = M.query_consts(q, qq)
    for name in ("qsum32", "qsum305", "q2", "round1"):
        assert abs(F64(kc[name]) - F64(want[name])) <= 1e-5 * abs(F64(want[name])) + 1e-6 * F64(want["q2"]), name
    # survivor entries: 2^-9 P^ from the exact integer sum, bit for bit
    p4, p_int = M.p_bits(c["h"], qq["Q"], kc["dp"])
    surv = r["surv_p"][slot] != S.SENT_U32
    assert int(r["survivors"][slot]) == int(surv.sum())
    assert np.array_equal(r["surv_p"][slot][surv], p4.view(np.uint32)[surv])
    # ... complete, and none that the bound excludes by more than its own roundings
    s64, q64 = c["s"].astype(F64), q.astype(F64)
    truth = c["truth"][qi]
    w4_64 = s64 * (4.0 * F64(qq["delta"]) * p_int - 30.5 * q64.sum())
    m4_64 = c["a4"].astype(F64) * F64(kc["q2"]) + s64 * F64(kc["round1"])
    assert np.all(np.abs(w4_64 - truth)[good] <= m4_64[good])
    assert not ((truth >= t) & good & ~surv).any(), "a row that reaches tau did not survive"
    assert not (surv & good & ~(w4_64 + 1.001 * m4_64 + 1e-30 >= t)).any(), "a survivor the four-bit bound excludes"
    # candidates
    count = int(r["count"][slot])
    keys = r["cand"][slot, :min(count, cap)]
    assert (r["cand"][slot, min(count, cap):] == S.SENT_KEY).all()
    rows = S.key_row(keys).astype(np.int64)
    assert rows.size == np.unique(rows).size and (rows.size == 0 or rows.max() < N)
    assert surv[rows].all()
    w6_64 = s64 * (4.0 * F64(qq["delta"]) * p_int + c["l"].astype(F64) @ q64 - 32.0 * q64.sum())
    m6_64 = c["a6"].astype(F64) * F64(kc["q2"]) + s64 * F64(kc["round1"])
    assert np.all(np.abs(w6_64 - truth)[good] <= m6_64[good])
    rnd = 6e-6 * (d + 8) * s64 * np.abs(q64).sum()
    g = good[rows]
    w = S.ord2f(S.key_ord(keys)).astype(F64)
    assert np.all(np.abs(w[g] - w6_64[rows][g]) <= rnd[rows][g] * (1 + S.M_SLACK) + 1e-45)
    if count <= cap:
        kept = np.zeros(N, bool)
        kept[rows] = True
        assert not ((truth >= t) & good & ~kept).any(), "a row that reaches tau is no candidate"
        assert not (kept & good & ~(w6_64 + 1.001 * m6_64 + 1e-30 >= t)).any(), "a candidate the six-bit bound excludes"
    return int(surv.sum()), count


@pytest.mark.parametrize("grid_x", [1, 3])
@pytest.mark.parametrize("d", DIMS)
def test_a_full_group(d, grid_x):
    assert MH.has_instance(d // 32)
    c = _case(d)
    r = MH.scan(c["planes"], c["queries"], N, c["tau"], N, grid_x)
    assert (r["guard"] == S.SENT_KEY).all()
    got = [_check_query(c, r, i, i, c["tau"][i], N) for i in range(16)]
    print(f"d={d} grid_x={grid_x}: (survivors, candidates) {got}")
    assert got[0] == (N, N)                       # low tau: every row survives and is a candidate
    assert got[1] == (0, 0)                       # tau = +inf: nothing is kept
    assert got[2] == got[3] and N // 4 <= got[2][0] < N
    if grid_x == 1:
        assert got[2][0] > 48 * 4      # four waves: some wave's list came due in mid-pass, tiles after slot 0's first refine
    assert 0 < got[4][1] <= got[4][0] < N
    assert np.array_equal(np.sort(r["cand"][2, :got[2][1]]), np.sort(r["cand"][3, :got[3][1]]))


@pytest.mark.parametrize("nq", [1, 15, 33])
def test_short_groups(nq):
    """1 and 15 queries: one short group; 33: two full groups and a group of one.  Absent columns write nothing."""
    d = 384
    c = _case(d)
    pick = np.arange(nq) % 16
    pick = pick[::-1].copy()  # (other columns than in the full group)
    r = MH.scan(c["planes"], c["queries"][pick], N, c["tau"][pick], N, 2)
    assert (r["guard"] == S.SENT_KEY).all()
    for slot, qi in enumerate(pick):
        _check_query(c, r, slot, qi, c["tau"][qi], N)
    groups = (nq + 15) // 16
    assert (r["qc"]["flags"][nq:groups * 16] == MH.ABSENT).all() and not r["bytes"][nq:].any()


def test_a_small_capacity_counts_on():
    """tau = -inf with cap = 100: the counter ends at the exact total, above cap; the first cap keys are real keys"""
    d, cap = 384, 100
    c = _case(d)
    tau = c["tau"].copy()
    tau[:4] = -np.inf
    r = MH.scan(c["planes"], c["queries"], N, tau, cap, 2)
    assert (r["guard"] == S.SENT_KEY).all()
    for i in range(16):
        s, n = _check_query(c, r, i, i, tau[i], cap)
        if i < 4:
            assert s == n == N and (r["cand"][i] != S.SENT_KEY).all()


def test_nan_and_inf_rows():
    d = 384
    c = _case(d, bad=True)
    good = np.isfinite(c["rows"]).all(axis=1)
    assert (~good).sum() == 3
    r = MH.scan(c["planes"], c["queries"], N, c["tau"], N, 2)
    assert (r["guard"] == S.SENT_KEY).all()
    for i in range(16):
        _check_query(c, r, i, i, c["tau"][i], N, good)
        rows = S.key_row(r["cand"][i, :int(r["count"][i])])
        assert 5 not in rows                                # a NaN element: never a candidate
        assert 9 in rows and N - 1 in rows                  # an infinite element: always one, whatever tau (slot 1: +inf)
        inf_keys = r["cand"][i, :int(r["count"][i])][np.isin(rows, (9, N - 1))]
        assert np.all(S.ord2f(S.key_ord(inf_keys)) == np.inf)


@pytest.mark.parametrize("kind", ["nan", "inf", "tiny", "huge"])
def test_a_marked_query(kind):
    d = 384
    c = _case(d)
    queries, tau = c["queries"].copy(), c["tau"].copy()
    slot = 6
    if kind == "nan":
        queries[slot, 11] = np.nan
    elif kind == "inf":
        queries[slot, 11] = np.inf
    else:
        queries[slot] *= F32(1e-30 if kind == "tiny" else 1e30)
    for cap in (100, N):
        r = MH.scan(c["planes"], queries, N, tau, cap, 2)
        assert (r["guard"] == S.SENT_KEY).all()
        assert r["qc"]["flags"][slot] == MH.MARKED and not r["bytes"][slot].any()
        assert int(r["count"][slot]) == int(r["survivors"][slot]) == N      # above cap = 100; every row at cap = N
        rows = S.key_row(r["cand"][slot, :cap])
        assert rows.size == np.unique(rows).size == cap and rows.max() < N
        for i in (0, 2, 5, 7, 15):                                           # its neighbours are what they were
            _check_query(c, r, i, i, tau[i], cap)
