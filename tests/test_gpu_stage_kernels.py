"""The int8 batch stages around the tile kernel, each launched ALONE through tests/kernel_harness/libstage_harness.so
(tests/stage_harness.py): pair scatter, second selection stage, overflow marks, slot placement, the range block's bounds, row
gather and normalisation.  The CPU half feeds every checker its numpy restatement, which it must accept, and a handful of
deliberately wrong restatements, each of which it must reject; the GPU half feeds the checkers what the kernels emit."""
import zlib

import numpy as np
import pytest

import stage_harness as H
from stage_harness import COS, F32, F64, GUARD, I32, I64, L2, U32, U64
from test_selection_bounds import quantise_i8_query

gpu = pytest.mark.gpu


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# --------------------------------------------------------------------------- #
# scatter_pairs_kernel
# --------------------------------------------------------------------------- #
D_EDGES = [0, 1, -1, (1 << 23) - 1, -((1 << 23) - 1), H.D_UNKNOWN]


def _scatter_case(nlists, pair_cap, kind):
    rng = _rng("scatter", nlists, pair_cap, kind)
    nq, cap = 256, 512
    pc = rng.integers(0, min(pair_cap, 48) + 1, nlists).astype(U32)
    pc[0] = min(pair_cap, 48)
    pairs = np.full(nlists * pair_cap, 0x0000FF00FFFFFFFF, U64)  # (unused slots name query 255, beyond any small counter array)
    count = np.zeros(nq + 2, U32)
    count[nq:] = H.SENT_U32
    if kind == "one_query":
        qs = np.array([7])
    else:
        qs = np.setdiff1d(np.arange(256), np.arange(3, 256, 5))  # some queries absent
    if kind == "append":
        count[:nq] = rng.integers(0, 9, nq)
    if kind == "buffer_overflow":
        cap, qs = 16, np.array([4, 5, 6])
    if kind == "list_overflow":
        pc[0] = pair_cap
        pc[nlists // 2] = pair_cap + 7
    for w in range(nlists):
        have = min(int(pc[w]), pair_cap)
        D = rng.integers(-(1 << 23) + 1, 1 << 23, have)
        D[:len(D_EDGES)] = D_EDGES[:have]
        pairs[w * pair_cap: w * pair_cap + have] = H.make_pairs(D, rng.choice(qs, have), rng.integers(0, 1 << 32, have, dtype=np.uint64))
    cand = np.full(nq * cap + GUARD, H.SENT_KEY, U64)
    return H.Scatter(pairs, pc, nlists, pair_cap, cand, count, cap, np.array([0, H.SENT_U32], U32), nq)


SCATTER_CASES = [(n, pc, "plain") for n in (1, 16, 17, 40) for pc in (64, 2048)] + \
                [(17, 64, "one_query"), (40, 64, "append"), (40, 64, "buffer_overflow"), (17, 64, "list_overflow"), (1, 64, "list_overflow")]


@pytest.mark.parametrize("nlists,pair_cap,kind", SCATTER_CASES)
def test_scatter_checker_accepts_the_restatement_and_rejects_wrong_ones(nlists, pair_cap, kind):
    s = _scatter_case(nlists, pair_cap, kind)
    H.check_scatter(s, *H.scatter_py(s))
    bugs = ["logical_shift", "row_not_inverted"] + (["lost_unset"] if kind == "list_overflow" else [])
    for bug in bugs:
        with pytest.raises(AssertionError):
            H.check_scatter(s, *H.scatter_py(s, bug))


def test_scatter_entries_of_the_edge_values():
    ent, q = H.scatter_entries(H.make_pairs(D_EDGES, [9] * 6, [5] * 6))
    hi = (ent >> U64(32)).astype(U32).view(I32)
    assert hi.tolist() == [0, 1, -1, (1 << 23) - 1, -((1 << 23) - 1), H.INT_MIN] and (q == 9).all()
    assert ((ent & U64(0xFFFFFFFF)) == U64(0xFFFFFFFA)).all()


@gpu
@pytest.mark.parametrize("nlists,pair_cap,kind", SCATTER_CASES)
def test_scatter_pairs_kernel(nlists, pair_cap, kind):
    assert H.constants()[0] == H.SCATTER_LISTS
    s = _scatter_case(nlists, pair_cap, kind)
    cand, count, lost = H.scatter(s)
    H.check_scatter(s, cand, count, lost)
    assert int(lost[0]) == (1 if kind == "list_overflow" else 0)
    if kind == "buffer_overflow":
        assert (count[[4, 5, 6]] > s.cap).all()
    # the unknown pattern of list 0 (pair 5) came out as exactly INT_MIN
    if pair_cap >= 6 and kind == "one_query":
        buf = cand[7 * s.cap: 7 * s.cap + int(count[7])]
        assert (((buf >> U64(32)).astype(U32).view(I32)) == H.INT_MIN).sum() >= 1


@gpu
def test_scatter_harness_refuses_a_query_byte_beyond_the_counters():
    s = _scatter_case(1, 64, "one_query")
    s.count = s.count[:7].copy()  # query 7 needs 8 counters
    with pytest.raises(ValueError):
        H.scatter(s)


# --------------------------------------------------------------------------- #
# mark_lost_kernel
# --------------------------------------------------------------------------- #
def _mark_cases():
    for nq in (1, 64, 251, 256, 300):
        for lost in (None, 0, 1):
            for with_list in (False, True):
                yield nq, lost, with_list


def _mark_case(nq, lost, with_list):
    rng = _rng("mark", nq)
    cap = 100
    count = np.concatenate([rng.choice([0, 3, cap - 1, cap, cap + 1, 1 << 30], nq), [H.SENT_U32] * 4]).astype(U32)
    count[0] = cap
    over = np.full(nq + 1 + 4, H.SENT_U32, U32) if with_list else None
    return count, (None if lost is None else np.array([lost], U32)), cap, over


@pytest.mark.parametrize("nq,lost,with_list", list(_mark_cases()))
def test_mark_lost_checker_accepts_the_restatement_and_rejects_wrong_ones(nq, lost, with_list):
    count, lost_a, cap, over = _mark_case(nq, lost, with_list)
    H.check_mark_lost(count, nq, lost_a, cap, over, *H.mark_lost_py(count, nq, lost_a, cap, over))
    if lost or with_list:
        with pytest.raises(AssertionError):
            H.check_mark_lost(count, nq, lost_a, cap, over, *H.mark_lost_py(count, nq, lost_a, cap, over, "ge_cap"))
    if lost and with_list:
        with pytest.raises(AssertionError):
            H.check_mark_lost(count, nq, lost_a, cap, over, *H.mark_lost_py(count, nq, lost_a, cap, over, "list_before_raise"))


@gpu
@pytest.mark.parametrize("nq,lost,with_list", list(_mark_cases()))
def test_mark_lost_kernel(nq, lost, with_list):
    count, lost_a, cap, over = _mark_case(nq, lost, with_list)
    H.check_mark_lost(count, nq, lost_a, cap, over, *H.mark_lost(count, nq, lost_a, cap, over))


# --------------------------------------------------------------------------- #
# refine_pairs_kernel
# --------------------------------------------------------------------------- #
N_GROUPS, CAP, PITCH8 = 64, 4096, 128
REFINE_KS = [1, 10, 128, 129, 500, 1024, 2048]


def _refine_tables(metric):
    """group and query parameters at the magnitudes of test_gpu_tile_kernels._tables; group 3 has a_g = +inf (and vouches),
    group 5 is all zero, group 7 does not vouch (finite bounds); groups 1 and 2 hold bad rows in their low and high halves"""
    rng = _rng("refine_tables", metric)
    s_g = (rng.uniform(0.5, 1.5, N_GROUPS) * 0.01).astype(F32)
    groups = np.stack([s_g, s_g * F32(70 * np.sqrt(PITCH8)) * rng.uniform(0.9, 1.1, N_GROUPS).astype(F32),
                       s_g * F32(np.sqrt(PITCH8 / 12)) * rng.uniform(0.9, 1.1, N_GROUPS).astype(F32), np.ones(N_GROUPS, F32)], axis=1).astype(F32)
    groups[3, 1] = np.inf
    groups[5] = [0.0, 0.0, 0.0, 1.0]
    groups[7, 3] = 0.0
    gbad = np.zeros(N_GROUPS, U64)
    for r in np.flatnonzero(rng.random(N_GROUPS * 64) < 0.04):
        gbad[r >> 6] |= U64(1) << U64(r & 63)
    gbad[1] = U64(0x00000000FFFFFFFF)
    gbad[2] = U64(0xFFFFFFFF00000000)
    gbad[9] = U64(0)  # (the group of the "one group, one D" list)
    cn = rng.uniform(0.5, 2.0, N_GROUPS * 64).astype(F32)
    cn[rng.choice(np.arange(10 * 64, 48 * 64), 6, replace=False)] = [np.nan, np.nan, np.inf, np.inf, np.nan, np.inf]
    cn[48 * 64:] = 0.0  # (the zero query's rows)
    cn[9 * 64: 10 * 64] = 1.25  # (the "one group, one D" list: one norm as well, so that every ub exceeds every lb for L2 too)
    return groups, gbad, cn


def _qpar_row(rng):
    s_q = F32(rng.uniform(0.5, 1.5) * 0.008)
    return [s_q, s_q * F32(np.sqrt(PITCH8 / 12)) * F32(rng.uniform(0.9, 1.1)), s_q * F32(70 * np.sqrt(PITCH8)) * F32(rng.uniform(0.9, 1.1)),
            F32(1) / s_q]


def _refine_case(metric, k):
    """queries: 0 .. 2 generic lists of k + 1, about 1.5 k and about 3000 entries; 3: k entries (left alone); 4: a counter above
    cap (left alone); 5: E = +inf (nobody vouches: left alone, bad rows included); 6: the zero query (every bound is 0: only
    bad rows go); 7: unknown D almost everywhere (fewer than k vouch: left alone); 8: one group, one D (nothing may go; k < 64)"""
    rng = _rng("refine", metric, k)
    groups, gbad, cn = _refine_tables(metric)
    nq = 9
    cand = np.full(nq * CAP + GUARD, H.SENT_KEY, U64)
    count = np.zeros(nq, U32)
    qpar = np.array([_qpar_row(rng) for _ in range(nq)], F32)
    qpar[5] = [0.0, np.inf, 0.0, 0.0]
    qpar[6] = 0.0

    def fill(q, n, D=None, rows=None):
        rows = rng.choice(N_GROUPS * 64, n, replace=False) if rows is None else rows
        if D is None:
            D = rng.integers(-1_000_000, 1_000_000, n)
            D[rng.choice(n, max(1, n // 50), replace=False)] = H.INT_MIN
            # the rows that must not vote carry the largest dot products: a wrong vote moves the threshold
            row_bad = ((gbad[rows >> 6] >> (rows & 63).astype(U64)) & U64(1)).astype(bool)
            D[row_bad | ((rows >> 6) == 7)] = rng.integers(1_500_000, 2_000_000, int((row_bad | ((rows >> 6) == 7)).sum()))
        cand[q * CAP: q * CAP + n] = H.make_entries(D, rows)
        count[q] = n

    sizes = [k + 1, min(max(k + 2, (3 * k) // 2), 4000), 3000 if k < 3000 else 4000, k]
    for q, n in enumerate(sizes):
        fill(q, n)
    count[4] = CAP + 5
    fill(5, min(max(k + 40, 200), 4000))
    # (the zero query's rows have |c|^2 = 0, so that L2 too has lb = ub = 0 exactly: a tie at the threshold that a non-strict
    # drop test gets wrong; 1024 such rows, so from k = 1024 on the list is no longer than k and is left alone)
    n6 = min(max(int(1.3 * k) + 60, 200), 1000)
    fill(6, n6, None, rng.choice(np.arange(48 * 64, 64 * 64), n6, replace=False))
    n7 = min(k + 50, 4000)
    D7 = np.full(n7, H.INT_MIN, I64)
    D7[:max(k - 1, 0)] = rng.integers(-1000, 1000, max(k - 1, 0))
    rows7 = np.setdiff1d(np.arange(N_GROUPS * 64), np.concatenate([np.arange(64, 192), np.arange(7 * 64, 8 * 64)]))
    fill(7, n7, D7, rng.choice(rows7, n7, replace=False))
    if k < 60:
        fill(8, 64, np.full(64, 123_456, I64), np.arange(9 * 64, 10 * 64))
    else:
        fill(8, 0, np.zeros(0, I64), np.zeros(0, I64))
    c = H.Refine(metric, k, CAP, nq, cand, count, groups, gbad, cn, qpar)
    # lists 1 and 2: the k entries that set the threshold stand clear of the rest (+100 000 units of D, several widths of a
    # bound), so that the (k + 1)-th largest lower bound is a visibly different threshold from the k-th
    for q in (1, 2):
        n = int(count[q])
        e = cand[q * CAP: q * CAP + n]
        _, vouch, lb, _, _ = H.refine_bounds64(c, q, e)
        if int(vouch.sum()) > k:
            top = np.argsort(np.where(vouch, lb, -np.inf))[-k:]
            rows, D = H.entry_fields(e)
            D[top] += 100_000
            cand[q * CAP: q * CAP + n] = H.make_entries(D, rows)
    return c


REFINE_BUGS = ["non_strict", "bad_rows_vote", "all_groups_vote", "k_plus_1", "duplicate"]


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("k", REFINE_KS)
def test_refine_checker_accepts_the_restatement_and_few_entries_are_undecided(metric, k):
    c = _refine_case(metric, k)
    for lds_branch in (True, False):
        dropped = H.check_refine(c, lds_branch, *H.refine_py(c, lds_branch))
        assert dropped > 0
        assert H.undecided_share(c, lds_branch) <= 0.05


@pytest.mark.parametrize("metric,bug", [(m, b) for m in (COS, L2) for b in REFINE_BUGS] + [(L2, "no_norm")])
def test_refine_checker_rejects_wrong_restatements(metric, bug):
    rejected = 0
    for k in (10, 128, 500):
        c = _refine_case(metric, k)
        for lds_branch in (True, False):
            try:
                H.check_refine(c, lds_branch, *H.refine_py(c, lds_branch, bug))
            except AssertionError:
                rejected += 1
    assert rejected == 6, (bug, rejected)


def test_refine_lists_that_must_stay():
    c = _refine_case(COS, 10)
    cand, count = H.refine_py(c, True)
    for q in (3, 4, 5, 7):
        assert count[q] == c.count[q] and np.array_equal(cand[q * CAP:(q + 1) * CAP], c.cand[q * CAP:(q + 1) * CAP])
    # the zero query: only its bad rows go; one group, one D: nothing goes
    bad = H.refine_bounds64(c, 6, c.cand[6 * CAP: 6 * CAP + int(c.count[6])])[0]
    assert count[6] == c.count[6] - bad.sum() and bad.sum() > 0 and count[8] == 64
    # the list of query 5 keeps its bad rows
    assert H.refine_bounds64(c, 5, c.cand[5 * CAP: 5 * CAP + int(c.count[5])])[0].any()


def _refine_launches():
    for metric in (COS, L2):
        for k in REFINE_KS:
            for lds_lists in ((False, True) if k <= 128 else (False,)):
                for lds_branch in (True, False):
                    yield metric, k, lds_lists, lds_branch


@gpu
@pytest.mark.parametrize("metric,k,lds_lists,lds_branch", list(_refine_launches()))
def test_refine_pairs_kernel(metric, k, lds_lists, lds_branch):
    assert H.constants()[1:3] == (H.REFINE_R, H.KTH_LOW_BIT)
    c = _refine_case(metric, k)
    reg, waves, n_lds, lds, raise_ = H.refine_shape(k, CAP, lds_lists)
    assert reg == int(k <= 128 and not lds_lists) and lds <= 128 * 1024 and n_lds == min(CAP, H.REFINE_R * 64 * waves)
    assert int(c.count[:4].max()) <= n_lds  # (the generic lists fit the LDS branch of this shape)
    # the wave-list branch: n_lds = k, so every list the kernel works on is longer
    cand, count = H.refine(c, lds_lists, 0 if lds_branch else k)
    dropped = H.check_refine(c, lds_branch, cand, count)
    assert dropped > 0
    if k < 60:
        assert count[8] == 64


@gpu
def test_refine_harness_refuses_rows_beyond_the_tables():
    c = _refine_case(COS, 10)
    c.groups = c.groups[:32].copy()
    with pytest.raises(ValueError):
        H.refine(c)


# --------------------------------------------------------------------------- #
# place_queries_kernel, pad_tau_kernel
# --------------------------------------------------------------------------- #
PLACE_CASES = [(1, 64), (24, 192), (96, 256), (25, 63 + 1), (1, 192 + 1)]  # (1 x 193 and 25 x 64 = 1600: no multiple of 256)


def _place_case(pitch4, slots):
    rng = _rng("place", pitch4, slots)
    nq = slots // 2 + 3
    q = rng.standard_normal(nq * pitch4 * 4).astype(F32)
    sq = rng.permutation(nq)[:slots].astype(I32) if nq >= slots else rng.integers(0, nq, slots).astype(I32)
    sq[rng.choice(slots, max(1, slots // 7), replace=False)] = -1
    sq[1 % slots], sq[slots - 1] = sq[0], -1  # a query in two slots, a pad at the end
    if sq[0] < 0:
        sq[0] = sq[1 % slots] = 2
    out = H.sent_f32((slots * pitch4 + 5) * 4)
    tau = rng.standard_normal(slots + 8).astype(F32)
    real = np.flatnonzero(sq >= 0)
    tau[real[0]], tau[real[1]] = np.nan, -np.inf
    return q, sq, out, tau


@gpu
@pytest.mark.parametrize("pitch4,slots", PLACE_CASES)
def test_place_queries_and_pad_tau_kernels(pitch4, slots):
    q, sq, out, tau = _place_case(pitch4, slots)
    got = H.place_queries(q, sq, pitch4, out)
    assert np.array_equal(got.view(U32), H.place_queries_py(q, sq, pitch4, out).view(U32))
    assert (got[:slots * pitch4 * 4].reshape(slots, -1)[sq < 0].view(U32) == 0).all()
    assert np.array_equal(got[slots * pitch4 * 4:].view(U32), out[slots * pitch4 * 4:].view(U32))
    t = H.pad_tau(tau, sq)
    assert np.array_equal(t.view(U32), H.pad_tau_py(tau, sq).view(U32))
    assert (t[:slots][sq < 0] == np.inf).all() and np.array_equal(t[:slots][sq >= 0].view(U32), tau[:slots][sq >= 0].view(U32))
    assert np.isnan(t[:slots]).sum() == 1 and (t[:slots] == -np.inf).sum() == 1


def test_place_and_pad_restatements():
    q, sq, out, tau = _place_case(24, 192)
    got = H.place_queries_py(q, sq, 24, out)[:192 * 96].reshape(-1, 96)
    assert (got[:192][sq < 0] == 0).all() and np.array_equal(got[0], q.reshape(-1, 96)[sq[0]]) and np.array_equal(got[0], got[1])
    assert (H.pad_tau_py(tau, sq)[:192][sq < 0] == np.inf).all()


# --------------------------------------------------------------------------- #
# range_batch_bound_kernel
# --------------------------------------------------------------------------- #
RANGE_CASES = [(gbn, nv) for gbn in (64, 128, 256) for nv in (1, gbn - 5, gbn)]


def _range_case(gbn, nv):
    rng = _rng("range", gbn, nv)
    d = 96
    qpar = np.zeros((gbn + 3, 4), F32)
    for r in range(gbn + 3):
        q = rng.standard_normal(d).astype(F32) * F32(rng.choice([1e-3, 1.0, 50.0]))
        if r % 11 == 2:
            q[:] = 0                      # the zero query: s_q = 0
        elif r % 11 == 5:
            q *= F32(1e-34)               # a vanishing query
        elif r % 11 == 7:
            q[3] = np.inf                 # E = +inf
        _, s_q, E, M = quantise_i8_query(q)
        qpar[r] = [s_q, E, M, (F32(1.0) / s_q) if s_q > 0 else 0.0]
    tau_in = rng.standard_normal(max(nv, 1)).astype(F32)
    special = [np.inf, -np.inf, 3e38, -3e38, 1e37, 0.0]
    tau_in[:min(nv, len(special))] = special[:nv]
    if nv > 20:
        tau_in[10:16] = F32(2e36)  # above 1e38 s_q for the small queries
    tau = H.sent_f32(gbn + 4)
    rc = np.full(gbn + 4, H.SENT_U32, U32)
    return qpar, tau_in, tau, rc


@pytest.mark.parametrize("gbn,nv", RANGE_CASES)
def test_range_bound_checker_accepts_the_restatement_and_rejects_wrong_ones(gbn, nv):
    qpar, tau_in, tau, rc = _range_case(gbn, nv)
    H.check_range_batch_bound(nv, gbn, qpar, tau_in, tau, rc, *H.range_batch_bound_py(nv, gbn, qpar, tau_in, tau, rc))
    for bug in ("gamma_e", "m_unwidened", "tau_unlimited"):
        with pytest.raises(AssertionError):
            H.check_range_batch_bound(nv, gbn, qpar, tau_in, tau, rc, *H.range_batch_bound_py(nv, gbn, qpar, tau_in, tau, rc, bug))


@gpu
@pytest.mark.parametrize("gbn,nv", RANGE_CASES)
def test_range_batch_bound_kernel(gbn, nv):
    assert H.constants()[3] == H.GAMMA
    qpar, tau_in, tau, rc = _range_case(gbn, nv)
    H.check_range_batch_bound(nv, gbn, qpar, tau_in, tau, rc, *H.range_batch_bound(nv, gbn, qpar, tau_in, tau, rc))


# --------------------------------------------------------------------------- #
# gather_rows_kernel, normalize_rows_kernel
# --------------------------------------------------------------------------- #
AUX_PITCH4 = [1, 25, 96, 200]


@gpu
@pytest.mark.parametrize("pitch4", AUX_PITCH4)
@pytest.mark.parametrize("n,grid", [(1, 0), (5, 0), (1027, 0), (1027, 7)])
def test_gather_rows_kernel(pitch4, n, grid):
    rng = _rng("gather", pitch4, n)
    w, n_rows = 4 * pitch4, 300
    rows = rng.standard_normal(n_rows * w).astype(F32)
    src = rng.integers(0, n_rows, n).astype(U64)
    src[: min(n, 40)] = np.arange(n_rows - 1, n_rows - 41, -1)[: min(n, 40)]  # a reversed run
    if n > 50:
        src[40:50] = 17                                                       # repeats
    dst = H.sent_f32((n + 3) * w)
    got = H.gather_rows(rows, pitch4, src, dst, grid)
    assert np.array_equal(got[: n * w].view(U32), rows.reshape(n_rows, w)[src.astype(I64)].reshape(-1).view(U32))
    assert np.array_equal(got[n * w:].view(U32), dst[n * w:].view(U32))


def _normalize_case(pitch4):
    rng = _rng("normalize", pitch4)
    pitch, n = 4 * pitch4, 37
    rows = (rng.standard_normal((n + 2, pitch)) * rng.choice([1e-3, 1.0, 1e3], (n + 2, 1))).astype(F32)
    rows[3] = 0.0
    rows[4, 0] = np.nan
    rows[5] = F32(1e-24) * rng.choice([-1.0, 1.0], pitch).astype(F32)   # every square underflows to zero in fp32
    rows[6] = F32(1e20) * rng.choice([-1.0, 1.0], pitch).astype(F32)    # every square overflows in fp32
    return rows, n, pitch


@gpu
@pytest.mark.parametrize("pitch4", AUX_PITCH4)
@pytest.mark.parametrize("grid", [0, 3])
def test_normalize_rows_kernel(pitch4, grid):
    import wdbx_oracle as O

    rows, n, pitch = _normalize_case(pitch4)
    got = H.normalize_rows(rows.reshape(-1), n, pitch, grid).reshape(rows.shape)
    assert np.array_equal(got[n:].view(U32), rows[n:].view(U32)), "rows behind n"
    assert np.array_equal(got[3].view(U32), rows[3].view(U32)) and np.array_equal(got[4].view(U32), rows[4].view(U32))
    ordinary = np.setdiff1d(np.arange(n), [3, 4, 5, 6])
    r64 = rows[ordinary].astype(F64)
    want = r64 / np.sqrt((r64 * r64).sum(axis=1, keepdims=True))  # the oracle's rule, n > 0, in float64
    assert (np.abs(got[ordinary].astype(F64) - want) <= H.normalize_tolerance(pitch) * np.abs(want)).all()
    # rows whose squares leave fp32: the reference stores what its own fp32 norm gives -- the row itself when the norm
    # underflows to 0, zeros when it overflows to +inf -- and so does the kernel (a float64 norm would normalise both)
    with np.errstate(over="ignore", under="ignore"):
        for r in (5, 6):
            assert np.array_equal(got[r].view(U32), np.asarray(O.normalize_vector(rows[r]), F32).view(U32)), r
    assert np.array_equal(got[5].view(U32), rows[5].view(U32)) and (got[6] == 0).all()
