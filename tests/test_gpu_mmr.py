"""MMR search on the MI355X through the C ABI (wdbx_index_search_mmr).  1. integer corpora, where no operation rounds: ids,
scores and values ``==`` an int64 reference, pool and greedy from the definition; 2. float corpora with NO tolerance: the pool
from ``search``, the similarities from ``search_rows`` with ``get_rows`` of the candidates as queries, the numpy float32 loop
of tests/mmr_harness.py -- every bit equal -- and a cluster of near-duplicates that fills the plain top-10 and not the MMR
answer; 3. a float64 cross-check on committed seeds, each re-screened by the test; 4. lambda = 1 equals the plain search; 5.
pool edges, determinism and the rounds; 6. refusals.

Rounds.  A query of 2048 candidates at d = 1028 takes 2048 * 4112 B of gathered rows and a 16 MiB square, 24.03 MiB; nine of
them are 216.3 MiB and FIT the 256 MiB budget, so that call is one round.  The test therefore forces the budget with option
``mmr_scratch_mib`` (64 MiB: two queries to a round, five rounds) and also demands the same bytes as the one-round call."""
import numpy as np
import pytest

import listed_harness as LH
import mmr_harness as MH

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
N_INT = 5000
_F32, _F64, _U32 = np.float32, np.float64, np.uint32
LAMBDAS4 = (0, 1, 2, 3, 4)  # lambda * 4: 0, 0.25, 0.5, 0.75, 1 -- every product and difference exact
NQS = (1, 2, 9, 33)
K_FETCH = ((1, 1), (10, 40), (40, 40), (64, 65), (10, 2048))


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


_CASES = {}


def _int_case(native, d, metric):
    """the shapes of test_gpu_search_rows.py's _int_case: 5 000 un-normalised rows with elements in {-2 .. 2}"""
    key = (d, metric)
    if key not in _CASES:
        rng = np.random.default_rng(1000 + 10 * d + metric)
        rows = rng.integers(-2, 3, size=(N_INT, d)).astype(np.int64)
        queries = rng.integers(-2, 3, size=(256, d)).astype(np.int64)
        ix = native.NativeIndex(d, metric, 0, capacity_rows=N_INT)
        ix.add(rows.astype(_F32), normalize=False)
        _CASES[key] = (ix, rows, queries)
    return _CASES[key]


def _float_case(native, metric):
    """20 000 x 384 unit rows, three queries, and behind the corpus 50 near-duplicates of each query's nearest row"""
    key = ("float", metric)
    if key not in _CASES:
        rng = np.random.default_rng(4100 + metric)
        base = rng.standard_normal((20000, 384)).astype(_F32)
        base /= np.linalg.norm(base, axis=1, keepdims=True)
        anchors = [17, 4242, 19999]
        queries, dups = [], []
        for a in anchors:
            u = rng.standard_normal(384)
            u /= np.linalg.norm(u)
            q = base[a].astype(_F64) + 0.5 * u
            queries.append((q / np.linalg.norm(q)).astype(_F32))
            c = base[a][None, :] + 1e-3 * rng.standard_normal((50, 384)).astype(_F32)
            dups.append((c / np.linalg.norm(c, axis=1, keepdims=True)).astype(_F32))
        rows = np.concatenate([base] + dups).astype(_F32)
        ix = native.NativeIndex(384, metric, 0, capacity_rows=len(rows))
        ix.add(rows, normalize=False)
        _CASES[key] = (ix, rows, np.stack(queries), anchors)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for case in _CASES.values():
        case[0].close()
    _CASES.clear()


def _mask_words(native, allowed):
    return native.pack_row_mask(allowed)


# ---- 1. exact arithmetic -----------------------------------------------------------------------------------------------------
def _int_reference(rows, s, metric, allowed, lam4, k, fetch_k):
    """one query (s: its int64 score of every row, the squared distance under L2), from the definition, in int64 with every
    value scaled by 4: (ids, scores, 4 * values)"""
    ids = np.flatnonzero(allowed)
    order = np.lexsort((ids, -s[ids] if metric == COS else s[ids]))[:fetch_k]
    pool = ids[order]
    rel = s[pool] if metric == COS else -s[pool]
    c = rows[pool]
    m = len(pool)
    picks = min(k, m)
    pos, val4 = [0], [lam4 * rel[0]]
    picked = np.zeros(m, bool)
    picked[0] = True
    maxsim = None
    while len(pos) < picks:
        p = c[pos[-1]]
        g = c @ p if metric == COS else -((c - p) ** 2).sum(axis=1)
        maxsim = g if maxsim is None else np.maximum(maxsim, g)
        v4 = lam4 * rel - (4 - lam4) * maxsim
        v4m = np.where(picked, np.iinfo(np.int64).min, v4)
        best = int(np.flatnonzero(v4m == v4m.max())[0])  # ties to the smaller position
        picked[best] = True
        pos.append(best)
        val4.append(v4[best])
    pos = np.asarray(pos, np.int64)
    return pool[pos], s[pool][pos], np.asarray(val4, np.int64)


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [3, 384])
def test_integer_corpora_equal_the_int64_reference(native, d, metric):
    ix, rows, queries = _int_case(native, d, metric)
    rng = np.random.default_rng(50 + d + metric)
    masks = [None, rng.random(N_INT) < 0.6]
    qs = queries[:max(NQS)]
    S = qs @ rows.T if metric == COS else (qs ** 2).sum(axis=1)[:, None] - 2 * (qs @ rows.T) + (rows ** 2).sum(axis=1)[None, :]
    for k, fetch_k in K_FETCH:
        for allowed in masks:
            words = None if allowed is None else _mask_words(native, allowed)
            ok = np.ones(N_INT, bool) if allowed is None else allowed
            for lam4 in LAMBDAS4:
                want = [_int_reference(rows, S[q], metric, ok, lam4, k, fetch_k) for q in range(max(NQS))]
                for nq in NQS:
                    idx, score, mmr = ix.search_mmr(queries[:nq].astype(_F32), k, fetch_k, lam4 / 4, mask=words)
                    assert ix.get_option("last_mmr_path") == 1
                    assert ix.get_option("last_mmr_candidates") == nq * min(fetch_k, int(ok.sum()))
                    for q in range(nq):
                        w_idx, w_score, w_val4 = want[q]
                        what = (d, metric, k, fetch_k, allowed is not None, lam4, nq, q)
                        n = len(w_idx)
                        assert n == min(k, fetch_k, int(ok.sum()))
                        assert np.array_equal(idx[q, :n], w_idx), what
                        assert np.array_equal(score[q, :n].astype(_F64), w_score.astype(_F64)), what
                        assert np.array_equal(mmr[q, :n].astype(_F64) * 4, w_val4.astype(_F64)), what
                        assert (idx[q, n:] == -1).all() and not score[q, n:].any() and not mmr[q, n:].any(), what


# ---- 2. float corpora, no tolerance ------------------------------------------------------------------------------------------
def _from_existing_paths(ix, q, metric, k, fetch_k, lam, words=None):
    """the answer of one query put together from calls that existed before: (ids, scores, values)"""
    p_idx, p_score = ix.search(q[None, :], fetch_k, mask_words=words)
    m = int((p_idx[0] >= 0).sum())
    cand, score = p_idx[0, :m], p_score[0, :m]
    rel = (-score if metric == L2 else score).astype(_F32)
    stored = np.concatenate([ix.get_rows(int(r), 1) for r in cand])
    srt = np.sort(cand)
    r_idx, r_score = ix.search_rows(stored, m, srt.astype(np.uint64))  # query j = stored row j, ranked over the candidates
    assert (r_idx >= 0).all()
    G = np.empty((m, m), _F32)
    where = {int(r): i for i, r in enumerate(cand)}
    for j in range(m):
        at = np.fromiter((where[int(r)] for r in r_idx[j]), np.int64, m)
        G[at, j] = -r_score[j] if metric == L2 else r_score[j]
    pos, val = MH.greedy_fast_f32(rel, G, lam, k)
    return cand[pos], score[pos], val, G


@pytest.mark.parametrize("metric", [COS, L2])
def test_float_corpora_bit_for_bit_and_duplicates_diversified(native, metric):
    ix, rows, queries, anchors = _float_case(native, metric)
    for k, fetch_k in ((10, 40), (10, 200), (40, 40)):
        for lam in (0.25, 0.5):
            idx, score, mmr = ix.search_mmr(queries, k, fetch_k, lam)
            for q in range(len(queries)):
                w_idx, w_score, w_val, G = _from_existing_paths(ix, queries[q], metric, k, fetch_k, lam)
                what = (metric, k, fetch_k, lam, q)
                assert np.array_equal(G.view(_U32), G.T.view(_U32)), what
                assert np.array_equal(idx[q], w_idx), what
                assert MH.same_f32(score[q], w_score) is None, (what, MH.same_f32(score[q], w_score))
                assert MH.same_f32(mmr[q], w_val) is None, (what, MH.same_f32(mmr[q], w_val))
    # the plain top-10 is the anchor and its near-duplicates; the lambda = 0.5 answer from a pool of 200 is not
    plain, _ = ix.search(queries, 10)
    idx, _, _ = ix.search_mmr(queries, 10, 200, 0.5)
    for q, a in enumerate(anchors):
        cluster = set(range(20000 + 50 * q, 20050 + 50 * q)) | {a}
        assert set(plain[q].tolist()) <= cluster, (metric, q)
        assert not np.array_equal(idx[q], plain[q]), (metric, q)
        assert len(set(idx[q].tolist()) - cluster) >= 5, (metric, q, idx[q])
        assert idx[q, 0] == plain[q, 0]


# ---- 3. float64 cross-check on committed seeds -------------------------------------------------------------------------------
SEEDS = (11, 12, 13, 14, 15, 16)  # screened on the CPU with _greedy64 before they were committed
N64, D64, K64, FETCH64, LAM64 = 3000, 384, 10, 40, 0.5


def _corpus64(seed, metric):
    rng = np.random.default_rng(9000 + seed)
    rows = rng.standard_normal((N64, D64)).astype(_F32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    q = rng.standard_normal(D64).astype(_F32)
    q /= np.linalg.norm(q)
    return rows.astype(_F32), q.astype(_F32)


def _greedy64(rows, q, metric):
    """float64 pool and greedy; returns (ids, the smallest of gap / (2 * bound) over the pool's edge and every step)"""
    pitch4 = D64 // 4
    rel_all = LH.score64(rows, q[None, :], metric)[0]
    e_all = LH.score_bound64(rows, q[None, :], metric, pitch4)[0]
    order = np.lexsort((np.arange(N64), -rel_all))
    pool = order[:FETCH64]
    edge = (rel_all[order[FETCH64 - 1]] - rel_all[order[FETCH64]]) / (2 * max(e_all[order[FETCH64 - 1]], e_all[order[FETCH64]]))
    rel, e_rel = rel_all[pool], e_all[pool]
    c = rows[pool]
    G = LH.score64(c, c, metric)          # [j, i], symmetric
    E = LH.score_bound64(c, c, metric, pitch4)
    lam, u3 = LAM64, 3 * 2.0 ** -24
    maxsim, e_sim = np.full(FETCH64, -np.inf), np.zeros(FETCH64)
    picked = np.zeros(FETCH64, bool)
    pos = [0]
    picked[0] = True
    worst = edge
    while len(pos) < K64:
        p = pos[-1]
        e_sim = np.maximum(e_sim, E[p])
        maxsim = np.maximum(maxsim, G[p])
        v = lam * rel - (1 - lam) * maxsim
        bound = lam * e_rel + (1 - lam) * e_sim + u3 * (lam * np.abs(rel) + (1 - lam) * np.abs(maxsim))
        free = np.flatnonzero(~picked)
        by = free[np.argsort(-v[free], kind="stable")]
        best, second = by[0], by[1]
        worst = min(worst, (v[best] - v[second]) / (2 * max(bound[best], bound[second])))
        picked[best] = True
        pos.append(int(best))
    return pool[np.asarray(pos)], worst


@pytest.mark.parametrize("metric", [COS, L2])
def test_float64_greedy_on_committed_seeds(native, metric):
    for seed in SEEDS:
        rows, q = _corpus64(seed, metric)
        want, margin = _greedy64(rows, q, metric)
        print(f"seed {seed} metric {metric}: smallest gap / (2 * bound) = {margin:.1f}")
        assert margin > 1.0, f"seed {seed} does not pass the screen: a gap of {margin:.3f} times twice the rounding bound"
        ix = native.NativeIndex(D64, metric, 0, capacity_rows=N64)
        try:
            ix.add(rows, normalize=False)
            idx, _, _ = ix.search_mmr(q[None, :], K64, FETCH64, LAM64)
        finally:
            ix.close()
        assert np.array_equal(idx[0], want), (seed, metric)


# ---- 4. lambda = 1 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
def test_lambda_one_is_the_plain_search(native, metric):
    ix, rows, queries, _ = _float_case(native, metric)
    rng = np.random.default_rng(77 + metric)
    allowed = rng.random(len(rows)) < 0.3
    for words in (None, _mask_words(native, allowed)):
        for k, fetch_k in ((1, 1), (10, 40), (40, 40), (10, 2048)):
            idx, score, mmr = ix.search_mmr(queries, k, fetch_k, 1.0, mask=words)
            p_idx, p_score = ix.search(queries, fetch_k, mask_words=words)
            assert np.array_equal(idx, p_idx[:, :k]), (metric, k, fetch_k)
            assert MH.same_f32(score, p_score[:, :k]) is None, (metric, k, fetch_k)
            if words is not None:
                assert allowed[idx].all()


# ---- 5. pool edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
def test_pool_edges(native, metric):
    ix, rows, queries = _int_case(native, 384, metric)
    q = queries[:3].astype(_F32)
    # a mask that leaves three rows
    allowed = np.zeros(N_INT, bool)
    allowed[[5, 1234, 4999]] = True
    idx, score, mmr = ix.search_mmr(q, 10, 40, 0.5, mask=_mask_words(native, allowed))
    assert ix.get_option("last_mmr_candidates") == 9
    for r in range(3):
        assert sorted(idx[r, :3].tolist()) == [5, 1234, 4999] and (idx[r, 3:] == -1).all()
        assert not score[r, 3:].any() and not mmr[r, 3:].any()
    # a short mask is refused under the lock, the handle answers afterwards
    with pytest.raises(Exception):
        ix.search_mmr(q, 10, 40, 0.5, mask=np.zeros(3, _U32))
    # two identical calls, identical bytes
    a = ix.search_mmr(q, 40, 200, 0.25)
    b = ix.search_mmr(q, 40, 200, 0.25)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # an empty index: nothing launched
    empty = native.NativeIndex(384, metric, 0, capacity_rows=16)
    try:
        idx, score, mmr = empty.search_mmr(q, 5, 10, 0.5)
        assert (idx == -1).all() and not score.any() and not mmr.any()
        assert empty.get_option("last_mmr_path") == 0 and empty.get_option("last_mmr_rounds") == 0
    finally:
        empty.close()


@pytest.mark.parametrize("metric", [COS, L2])
def test_nan_and_removed_rows_are_never_picked(native, metric):
    rng = np.random.default_rng(300 + metric)
    rows = rng.standard_normal((600, 64)).astype(_F32)
    dead = np.array([0, 7, 64, 599])
    rows[dead[:2], 3] = np.nan
    rows[dead[2:]] = np.nan  # what a removed row looks like
    ix = native.NativeIndex(64, metric, 0, capacity_rows=600)
    try:
        ix.add(rows, normalize=False)
        idx, score, mmr = ix.search_mmr(rows[100:104] + _F32(0.01), 600, 600, 0.5)
        assert ix.get_option("last_mmr_candidates") == 4 * 596
        for r in range(4):
            got = idx[r, :596]
            assert sorted(got.tolist()) == sorted(set(range(600)) - set(dead.tolist()))
            assert (idx[r, 596:] == -1).all() and not np.isnan(mmr[r]).any() and not np.isnan(score[r]).any()
    finally:
        ix.close()


def test_rounds_follow_the_budget_and_do_not_change_the_answer(native):
    d, nq = 1028, 9
    rng = np.random.default_rng(1028)
    rows = rng.integers(-2, 3, size=(N_INT, d)).astype(_F32)
    q = rng.integers(-2, 3, size=(nq, d)).astype(_F32)
    ix = native.NativeIndex(d, COS, 0, capacity_rows=N_INT)
    try:
        ix.add(rows, normalize=False)
        one = ix.search_mmr(q, 10, 2048, 0.5)
        assert ix.get_option("last_mmr_rounds") == 1 and ix.get_option("last_mmr_candidates") == nq * 2048
        ix.set_option("mmr_scratch_mib", 64)
        many = ix.search_mmr(q, 10, 2048, 0.5)
        assert ix.get_option("last_mmr_rounds") == 5 > 1
        assert all(x.tobytes() == y.tobytes() for x, y in zip(one, many))
        for bad in (0, 257, -1):
            with pytest.raises(Exception):
                ix.set_option("mmr_scratch_mib", bad)
        assert ix.get_option("mmr_scratch_mib") == 64
    finally:
        ix.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(native):
    import ctypes as C

    ix, rows, queries = _int_case(native, 3, COS)
    q = np.ascontiguousarray(queries[:2].astype(_F32))
    good = ix.search_mmr(q, 10, 40, 0.5)
    lib, h = ix._lib, ix._h
    f32p, i64p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
    idx, score, mmr = np.empty((2, 10), np.int64), np.empty((2, 10), _F32), np.empty((2, 10), _F32)
    short = np.zeros(3, _U32)
    P = lambda a, t: a.ctypes.data_as(t)  # noqa: E731

    def call(nq=2, k=10, fetch_k=40, lam=0.5, queries=P(q, f32p), mask=None, words=0, oi=P(idx, i64p), os_=P(score, f32p)):
        return lib.wdbx_index_search_mmr(h, queries, nq, k, fetch_k, lam, 0, mask, words, oi, os_, P(mmr, f32p))

    refused = [dict(nq=0), dict(nq=-1), dict(k=0), dict(k=2049, fetch_k=2049), dict(fetch_k=9), dict(fetch_k=2049),
               dict(lam=float("nan")), dict(lam=-0.25), dict(lam=1.5), dict(lam=float("inf")), dict(queries=None), dict(oi=None),
               dict(os_=None), dict(mask=P(short, u32p), words=3)]
    for kw in refused:
        assert call(**kw) == -1, kw  # WDBX_E_INVALID
        again = ix.search_mmr(q, 10, 40, 0.5)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(good, again)), kw
    assert call() == 0
    # out_mmr may be null
    assert lib.wdbx_index_search_mmr(h, P(q, f32p), 2, 10, 40, 0.5, 0, None, 0, P(idx, i64p), P(score, f32p), None) == 0
    assert np.array_equal(idx, good[0]) and np.array_equal(score, good[1])
