"""Discovery search on the MI355X through the C ABI (wdbx_index_search_discover), with NO tolerance.

Reference: for each vector, ``wdbx_index_range_search`` with the threshold that lets every row through (-inf for cosine, +inf
for L2) gives every row's score, bit-identical to the discovery pass's ``r`` by contract (a row it does not return scored
NaN).  The fold, the order and the cut are tests/discover_reference.py (numpy float32 in the contract's order); ids, score
BITS and wins are compared with ``==``."""
import numpy as np
import pytest

import discover_reference as DR

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
_F32 = np.float32
SHAPES = [(3000, 32), (4000, 384)]


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


_CASES = {}


def _case(native, n, d, metric):
    """n rows around a common direction (so a negative at the corpus mean is nearer to almost every row than a positive at
    one row), a few near-duplicates of row 7 behind them, one row with a NaN element; the range-search scores are cached per
    vector.  -> (index, rows, score cache, the three pairs A, B, C of the zone tests)"""
    key = (n, d, metric)
    if key not in _CASES:
        rng = np.random.default_rng(9000 + n + 10 * d + metric)
        centre = rng.standard_normal(d)
        centre /= np.linalg.norm(centre)
        rows = (centre[None, :] + rng.standard_normal((n, d)) / np.sqrt(d)).astype(_F32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        dup = rows[7][None, :] + 2e-2 * rng.standard_normal((5, d)).astype(_F32) / np.sqrt(d) * 4
        rows[n - 6:n - 1] = dup / np.linalg.norm(dup, axis=1, keepdims=True)
        mean = rows.astype(np.float64).mean(axis=0)
        mean = (mean / np.linalg.norm(mean)).astype(_F32)
        rng1 = np.random.default_rng(1)
        near7 = rows[7] + 0.05 * rng1.standard_normal(d).astype(_F32) / np.sqrt(d) * 4
        near7 /= np.linalg.norm(near7)
        pairs = [(rows[7].copy(), mean), (rows[100].copy(), mean), (near7.astype(_F32), mean)]
        rows[n // 2, d // 3] = np.nan
        ix = native.NativeIndex(d, metric, 0, capacity_rows=n)
        ix.add(rows, normalize=False)
        _CASES[key] = (ix, rows, {}, pairs)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for case in _CASES.values():
        case[0].close()
    _CASES.clear()


def _scores(case, metric, v):
    """r(row, v) for every row in the ranking domain, float32; NaN where the range search does not return the row"""
    ix, rows, cache = case[:3]
    key = np.ascontiguousarray(v, _F32).tobytes()
    if key not in cache:
        off, ids, sc = ix.range_search(np.asarray(v, _F32)[None, :], -np.inf if metric == COS else np.inf)
        r = np.full(len(rows), np.nan, _F32)
        r[ids] = sc if metric == COS else -sc
        assert off[1] == len(ids) >= len(rows) - 1  # (every row but the NaN one)
        cache[key] = r
    return cache[key]


def _eligible(case, allowed=None, exclude=()):
    ok = np.ones(len(case[1]), bool) if allowed is None else allowed.copy()
    ok[list(exclude)] = False
    return ok


def _r_ctx(case, metric, pairs):
    n_rows = len(case[1])
    return np.stack([_scores(case, metric, v) for pair in pairs for v in pair]) if pairs else np.zeros((0, n_rows), _F32)


def _reference(case, metric, target, pairs, k, allowed=None, exclude=()):
    ok = _eligible(case, allowed, exclude)
    if target is None:
        return DR.context_answer(_r_ctx(case, metric, pairs), ok, k)
    return DR.target_answer(_scores(case, metric, target), _r_ctx(case, metric, pairs), ok, k, l2=metric == L2)


def _call(ix, queries, k, **kw):
    """queries: [(target or None, [(positive, negative)])] -> the library's answer"""
    targets = [t for t, _ in queries]
    ctx, off = [], [0]
    for _, pairs in queries:
        ctx += [v for pair in pairs for v in pair]
        off.append(len(ctx) // 2)
    return ix.search_discover(None if targets[0] is None else np.stack(targets), np.stack(ctx) if ctx else None, off, k, **kw)


def _assert_equal(got, want, q=0):
    idx, score, wins = got
    assert (idx[q] == want[0]).all(), (idx[q][:12], want[0][:12])
    assert (score[q].view(np.uint32) == want[1].view(np.uint32)).all()
    assert (wins[q] == want[2]).all()


def _vectors(case, rng, count):
    rows = case[1]
    v = rows[rng.integers(0, len(rows) // 2 - 10, size=count)] + 0.05 * rng.standard_normal((count, rows.shape[1])).astype(_F32)
    return [(x / np.linalg.norm(x)).astype(_F32) for x in v]


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("n,d", SHAPES)
def test_zero_pairs_equals_recommend_with_one_positive(native, metric, n, d):
    case = _case(native, n, d, metric)
    ix = case[0]
    t = _vectors(case, np.random.default_rng(5), 1)[0]
    got = _call(ix, [(t, [])], 10)
    rec = ix.search_recommend(t[None, :], [0, 1, 1], 10)
    assert got[0].tobytes() == rec[0].tobytes() and got[1].tobytes() == rec[1].tobytes() and (got[2] == 0).all()
    _assert_equal(got, _reference(case, metric, t, [], 10))
    assert ix.get_option("last_discover_path") == 2 and ix.get_option("last_discover_zone_slots") == 1


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("k,select_min_k", [(1, 200), (10, 200), (128, 200), (129, 200), (200, 200), (200, 0), (64, 50)])
def test_target_mode_spans_zones(native, metric, n, d, k, select_min_k):
    """three pairs whose positives sit at single rows and whose negatives sit at the corpus mean: few rows win any pair, so
    the answer runs through several wins values"""
    case = _case(native, n, d, metric)
    ix, pairs = case[0], case[3]
    t = _vectors(case, np.random.default_rng(6), 1)[0]
    want = _reference(case, metric, t, pairs, k)
    zones = len(set(want[2][want[0] >= 0].tolist()))
    if k >= 200:
        assert zones >= 3  # (the reference itself: the test cannot quietly degrade to one zone)
    ix.set_option("select_min_k", select_min_k)
    try:
        got = _call(ix, [(t, pairs)], k)
    finally:
        ix.set_option("select_min_k", 200)
    _assert_equal(got, want)
    assert ix.get_option("last_discover_path") == 2 and ix.get_option("last_discover_zone_slots") == zones


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("n,d,k", [(3000, 32, 200), (4000, 384, 10), (4000, 384, 129)])
def test_context_mode(native, metric, n, d, k):
    case = _case(native, n, d, metric)
    ix, pairs = case[0], [case[3][0], case[3][2]]
    want = _reference(case, metric, None, pairs, k)
    if k != 129:
        assert (want[1][want[0] >= 0] == 0).sum() >= 2 and (want[1] < 0).sum() >= 2  # (several loss-0 rows, several negative)
    zero = want[0][(want[0] >= 0) & (want[1] == 0)]
    assert (np.diff(zero) > 0).all()  # (loss 0: in row order)
    got = _call(ix, [(None, pairs)], k)
    _assert_equal(got, want)
    assert (got[1] <= 0).all() and (got[2] == 0).all()  # (the loss, never converted -- L2 included)
    assert ix.get_option("last_discover_path") == 1 and ix.get_option("last_discover_zone_slots") == 0
    ix.set_option("select_min_k", 5)
    try:
        _assert_equal(_call(ix, [(None, pairs)], k), want)
    finally:
        ix.set_option("select_min_k", 200)


@pytest.mark.parametrize("metric", [COS, L2])
def test_k_above_the_eligible_count(native, metric):
    case = _case(native, 3000, 32, metric)
    ix, rows, pairs = case[0], case[1], case[3]
    allowed = np.zeros(len(rows), bool)
    allowed[[3, 7, 100, len(rows) // 2, len(rows) - 3, len(rows) - 2]] = True  # (one of them the NaN row)
    words = native.pack_row_mask(allowed)
    t = _vectors(case, np.random.default_rng(7), 1)[0]
    for target in (t, None):
        want = _reference(case, metric, target, pairs, 10, allowed=allowed)
        assert (want[0] >= 0).sum() == 5
        got = _call(ix, [(target, pairs)], 10, mask_words=words)
        _assert_equal(got, want)
        assert (got[0][0][5:] == -1).all() and (got[1][0][5:] == 0).all() and (got[2][0][5:] == 0).all()


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("k", [10, 200])
def test_three_queries_equal_each_alone_and_runs_are_bit_equal(native, metric, k):
    case = _case(native, 4000, 384, metric)
    ix, pairs = case[0], case[3]
    v = _vectors(case, np.random.default_rng(9), 7)
    queries = [(v[0], []), (v[1], pairs[:1]), (v[2], pairs + [(v[3], v[4]), (v[5], v[5])])]  # 0, 1 and 5 pairs, one a tie
    first = _call(ix, queries, k)
    slots = ix.get_option("last_discover_zone_slots")
    again = _call(ix, queries, k)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    alone_slots = 0
    for q, (t, p) in enumerate(queries):
        alone = _call(ix, [(t, p)], k)
        alone_slots += ix.get_option("last_discover_zone_slots")
        for a, b in zip(first, alone):
            assert a[q].tobytes() == b[0].tobytes()
        _assert_equal(first, _reference(case, metric, t, p, k), q)
    assert slots == alone_slots >= 3
    ctx = [(None, pairs[:1]), (None, pairs), (None, queries[2][1])]
    first = _call(ix, ctx, k)
    again = _call(ix, ctx, k)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    for q, (_, p) in enumerate(ctx):
        _assert_equal(first, _reference(case, metric, None, p, k), q)


# (name, select_min_k, lds_lists): lists in registers up to k = 128 and in LDS above, the LDS lists whatever k is, the select chain
ROUTES = [("lists", 200, 0), ("lds_lists", 200, 1), ("select", 1, 0)]


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [20, 100])
def test_every_ranking_route_and_its_launch_counts(native, metric, d):
    """2 500 rows never bind the scratch bound, so all queries and all (query, zone) slots are ONE round each.  Context mode:
    the scoring launch (a scan launch), then one merge launch over the partial lists or one select-and-sort bracket per query.
    Target mode: the scoring launch, the zone launch (a merge launch) and the same tail over the zone slots."""
    case = _case(native, 2500, d, metric)
    ix, pairs = case[0], case[3]
    v = _vectors(case, np.random.default_rng(30 + d), 9)
    more = pairs + [(v[5], v[6]), (v[7], v[7])]
    five = [(v[0], []), (v[1], pairs[:1]), (v[2], more), (v[3], pairs), (v[4], pairs[1:])]
    calls = []  # (queries, k, the reference of each; target mode: the zone slots) -- references first: they run range searches
    for target in (True, False):
        for queries in (five[2:3], five):
            queries = [(t if target else None, p if target or p else pairs) for t, p in queries]
            for k in (1, 10, 129):
                want = [_reference(case, metric, t, p, k) for t, p in queries]
                zones = sum(len(set(w[2][w[0] >= 0].tolist())) for w in want) if target else 0
                calls.append((queries, k, want, zones))
    ix.profile(True)
    try:
        for name, select_min_k, lds_lists in ROUTES:
            ix.set_option("select_min_k", select_min_k)
            ix.set_option("lds_lists", lds_lists)
            for queries, k, want, zones in calls:
                nq, target = len(queries), queries[0][0] is not None
                ix.profile_read()
                got = _call(ix, queries, k)
                prof = ix.profile_read()
                what = (name, target, nq, k, zones, prof)
                for q in range(nq):
                    _assert_equal(got, want[q], q)
                assert ix.get_option("last_discover_path") == (2 if target else 1), what
                assert ix.get_option("last_discover_zone_slots") == zones, what
                assert prof["scan_launches"] == 1, what
                slots = zones if target else nq
                assert prof["merge_launches"] == (1 if target else 0) + (slots if name == "select" else 1), what
            # 257 queries (the five, again and again): a round holds at most 256 queries, so the second round writes its one
            # query's results from slot 256 on; the first round's (query, zone) slots pass 256 too, so its zone stage takes
            # several rounds of at most 256 slots, each ranked from its first slot on
            for five_queries, _, five_want, _ in (calls[4], calls[10]):
                target = five_queries[0][0] is not None
                want = [five_want[q % 5] for q in range(257)]
                ix.profile_read()
                got = _call(ix, [five_queries[q % 5] for q in range(257)], 10)
                prof = ix.profile_read()
                for q in range(257):
                    _assert_equal(got, want[q], q)
                assert prof["scan_launches"] == 2, (name, target, prof)
                if not target:
                    assert prof["merge_launches"] == (257 if name == "select" else 2), (name, prof)
                    continue
                zones = [len(set(w[2][w[0] >= 0].tolist())) for w in want]
                per_round = [sum(zones[:256]), zones[256]]
                zone_rounds = [-(-z // 256) for z in per_round]
                assert zone_rounds[0] >= 2 and ix.get_option("last_discover_zone_slots") == sum(per_round), (name, per_round)
                tails = sum(per_round) if name == "select" else sum(zone_rounds)
                assert prof["merge_launches"] == sum(zone_rounds) + tails, (name, per_round, prof)
    finally:
        ix.profile(False)
        ix.set_option("select_min_k", 200)
        ix.set_option("lds_lists", 0)


@pytest.mark.parametrize("metric", [COS, L2])
def test_normalize_vectors(native, metric):
    """scaled vectors with normalize_vectors: the reference takes each r from the range search with normalize_queries, which
    normalises with the same kernel (cosine; L2 never normalises)"""
    case = _case(native, 3000, 32, metric)
    ix, rows, _, pairs = case
    t = 2.0 * _vectors(case, np.random.default_rng(12), 1)[0]
    scaled = [(3.0 * p, 0.5 * n) for p, n in pairs]

    def r(v):
        off, ids, sc = ix.range_search(np.asarray(v, _F32)[None, :], -np.inf if metric == COS else np.inf, normalize_queries=True)
        out = np.full(len(rows), np.nan, _F32)
        out[ids] = sc if metric == COS else -sc
        return out

    r_ctx = np.stack([r(v) for pair in scaled for v in pair])
    ok = np.ones(len(rows), bool)
    _assert_equal(_call(ix, [(t, scaled)], 50, normalize_vectors=True), DR.target_answer(r(t), r_ctx, ok, 50, l2=metric == L2))
    _assert_equal(_call(ix, [(None, scaled)], 50, normalize_vectors=True), DR.context_answer(r_ctx, ok, 50))


@pytest.mark.parametrize("metric", [COS, L2])
def test_mask_and_exclusion(native, metric):
    case = _case(native, 4000, 384, metric)
    ix, rows, pairs = case[0], case[1], case[3]
    rng = np.random.default_rng(8)
    t = _vectors(case, rng, 1)[0]
    allowed = rng.random(len(rows)) < 0.3
    allowed[:40] = [i % 3 == 0 for i in range(40)]  # (a word with mixed bits)
    allowed[[7, len(rows) - 2, len(rows) - 3]] = True
    words = native.pack_row_mask(allowed)
    for target in (t, None):
        plain = _reference(case, metric, target, pairs, 10)
        exclude = sorted({0, len(rows) - 1, int(plain[0][0]), int(plain[0][3])})
        _assert_equal(_call(ix, [(target, pairs)], 10, mask_words=words), _reference(case, metric, target, pairs, 10, allowed=allowed))
        got = _call(ix, [(target, pairs)], 10, exclude_rows=exclude)
        _assert_equal(got, _reference(case, metric, target, pairs, 10, exclude=exclude))
        assert not set(got[0][0].tolist()) & set(exclude)
        masked_ex = sorted({r for r in exclude if allowed[r]} | {int(np.flatnonzero(allowed)[5]), 7})
        _assert_equal(_call(ix, [(target, pairs)], 10, mask_words=words, exclude_rows=masked_ex),
                      _reference(case, metric, target, pairs, 10, allowed=allowed, exclude=masked_ex))


def test_empty_index(native):
    ix = native.NativeIndex(64, COS, 0, capacity_rows=16)
    try:
        one = np.ones((2, 64), _F32)
        idx, score, wins = ix.search_discover(one, np.ones((4, 64), _F32), [0, 1, 2], 5)
        assert (idx == -1).all() and (score == 0).all() and (wins == 0).all()
        idx, score, wins = ix.search_discover(None, np.ones((4, 64), _F32), [0, 1, 2], 5)
        assert (idx == -1).all() and (score == 0).all() and (wins == 0).all()
        assert ix.get_option("last_discover_path") == 0 and ix.get_option("last_discover_zone_slots") == 0
    finally:
        ix.close()


def test_refusals_leave_the_handle_usable(native):
    case = _case(native, 3000, 32, COS)
    ix, rows, pairs = case[0], case[1], case[3]
    n = len(rows)
    t = _vectors(case, np.random.default_rng(10), 1)[0][None, :]
    ctx = np.stack([v for pair in pairs for v in pair])
    many = np.repeat(ctx[:2], 33, axis=0)
    bad = [
        (dict(targets=t, context=ctx, off=[0, 3], k=0), "k=0"),
        (dict(targets=t, context=ctx, off=[0, 3], k=native.MAX_K + 1), "k="),
        (dict(targets=t, context=many, off=[0, 33], k=5), "query 0 has 33 context pairs"),
        (dict(targets=t, context=np.concatenate([ctx, ctx[:2]]), off=[1, 4], k=5), "pair_offsets[0] = 1"),
        (dict(targets=np.repeat(t, 2, axis=0), context=ctx[:4], off=[0, 3, 2], k=5), "pair_offsets decrease at entry 2 (query 1)"),
        (dict(targets=None, context=ctx, off=[0, 3, 3], k=5), "query 1 has no context pair"),
        (dict(targets=t, context=ctx, off=[0, 3], k=5, mask_words=np.zeros((n + 31) // 32 - 1, np.uint32)), "row mask"),
        (dict(targets=t, context=ctx, off=[0, 3], k=5, exclude_rows=[3, 3]), "entry 1 is 3"),
        (dict(targets=t, context=ctx, off=[0, 3], k=5, exclude_rows=[1, n]), f"entry 1 is {n}"),
        (dict(targets=t, context=ctx, off=[0, 3], k=5, exclude_rows=list(range(1025))), "exclude_rows holds 1025 rows"),
    ]
    want = _reference(case, COS, t[0], pairs, 5)
    for kw, text in bad:
        kw = dict(kw)
        with pytest.raises(native.HipBackendError) as err:
            ix.search_discover(kw.pop("targets"), kw.pop("context"), kw.pop("off"), kw.pop("k"), **kw)
        assert text in str(err.value), (text, str(err.value))
        _assert_equal(ix.search_discover(t, ctx, [0, 3], 5), want)


def test_raw_abi_refusals_and_null_out_wins(native):
    """what the Python wrapper cannot send: nq < 1, every required pointer null in turn, a null exclude_rows with a count --
    each refused with WDBX_E_INVALID and followed by a good call; then out_wins = NULL, which is allowed"""
    import ctypes as C

    case = _case(native, 3000, 32, COS)
    ix, pairs = case[0], case[3]
    t = np.ascontiguousarray(_vectors(case, np.random.default_rng(11), 1)[0][None, :])
    ctx = np.ascontiguousarray(np.stack([v for pair in pairs for v in pair]))
    off = np.array([0, 3], np.uint64)
    good = ix.search_discover(t, ctx, off, 5)
    lib, h = ix._lib, ix._h
    f32p, i64p, u64p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    idx, score, wins = np.empty((1, 5), np.int64), np.empty((1, 5), _F32), np.empty((1, 5), np.uint8)
    P = lambda a, ty: a.ctypes.data_as(ty)  # noqa: E731

    def call(nq=1, k=5, tg=P(t, f32p), cx=P(ctx, f32p), offs=P(off, u64p), excl=None, n_excl=0, oi=P(idx, i64p),
             os_=P(score, f32p), ow=P(wins, u8p)):
        return lib.wdbx_index_search_discover(h, tg, cx, offs, nq, k, 0, None, 0, excl, n_excl, oi, os_, ow)

    refused = [dict(nq=0), dict(nq=-1), dict(k=0), dict(k=native.MAX_K + 1), dict(cx=None), dict(offs=None), dict(oi=None),
               dict(os_=None), dict(excl=None, n_excl=2)]
    for kw in refused:
        assert call(**kw) == -1, kw  # WDBX_E_INVALID
        again = ix.search_discover(t, ctx, off, 5)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(good, again)), kw
    assert call() == 0
    assert np.array_equal(idx, good[0]) and np.array_equal(score, good[1]) and np.array_equal(wins, good[2])
    idx[:], score[:] = -9, -9
    assert call(ow=None) == 0
    assert idx.tobytes() == good[0].tobytes() and score.tobytes() == good[1].tobytes()
