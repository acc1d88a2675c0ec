"""Recommend search on the MI355X through the C ABI (wdbx_index_search_recommend), with NO tolerance.

Reference: existing code only.  For each example, ``wdbx_index_range_search`` with the threshold that lets every row through
(-inf for cosine, +inf for L2) gives every row's score, bit-identical to the recommend pass's ``r`` by contract (a row it does
not return scored NaN).  The fold (max over the positives, max over the negatives, ``p > n``), the order (favoured by (p
descending, row), then disfavoured by (n ascending, row)) and the cut are done here in numpy float32; ids, score BITS and
sides are compared with ``==``."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
_F32 = np.float32
ZERO = _F32(0.0)


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


_CASES = {}


def _case(native, n, d, metric):
    """n rows around a common direction (so a negative at the corpus mean is near every row), a few near-duplicates of row 7
    behind them, one row with a NaN element; the range-search scores are cached per example vector"""
    key = (n, d, metric)
    if key not in _CASES:
        rng = np.random.default_rng(7000 + n + 10 * d + metric)
        centre = rng.standard_normal(d)
        centre /= np.linalg.norm(centre)
        rows = (centre[None, :] + rng.standard_normal((n, d)) / np.sqrt(d)).astype(_F32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        dup = rows[7][None, :] + 2e-3 * rng.standard_normal((5, d)).astype(_F32)
        rows[n - 6:n - 1] = dup / np.linalg.norm(dup, axis=1, keepdims=True)
        rows[n // 2, d // 3] = np.nan
        ix = native.NativeIndex(d, metric, 0, capacity_rows=n)
        ix.add(rows, normalize=False)
        _CASES[key] = (ix, rows, {})
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for case in _CASES.values():
        case[0].close()
    _CASES.clear()


def _scores(case, metric, v):
    """r(row, v) for every row in the ranking domain, float32; NaN where the range search does not return the row"""
    ix, rows, cache = case
    key = v.tobytes()
    if key not in cache:
        off, ids, sc = ix.range_search(v[None, :], -np.inf if metric == COS else np.inf)
        r = np.full(len(rows), np.nan, _F32)
        r[ids] = sc if metric == COS else -sc
        assert off[1] == len(ids) >= len(rows) - 1  # (every row but the NaN one)
        cache[key] = r
    return cache[key]


def _reference(case, metric, pos, neg, k, allowed=None, exclude=()):
    """(ids int64 [k], score float32 [k], side uint8 [k]) of one query from the definition"""
    n_rows = len(case[1])
    rp = np.stack([_scores(case, metric, v) for v in pos])
    rn = np.stack([_scores(case, metric, v) for v in neg]) if len(neg) else np.full((1, n_rows), -np.inf, _F32)
    nan = np.isnan(rp).any(axis=0) | np.isnan(rn).any(axis=0)
    with np.errstate(invalid="ignore"):
        p, n = np.fmax.reduce(rp, axis=0), np.fmax.reduce(rn, axis=0)
    ok = ~nan
    if allowed is not None:
        ok &= allowed
    ok[list(exclude)] = False
    with np.errstate(invalid="ignore"):
        fav = ok & (p > n)
    dis = ok & ~fav
    rows = np.arange(n_rows)
    f_rows, d_rows = rows[fav], rows[dis]
    f_key = (p[fav] + ZERO).astype(_F32)
    d_key = ((-n[dis]) + ZERO).astype(_F32)
    f_order = np.lexsort((f_rows, -f_key))
    d_order = np.lexsort((d_rows, -d_key))
    ids = np.concatenate([f_rows[f_order], d_rows[d_order]])[:k]
    # out_score: the key value back in the caller's units, as the ranking tail converts it (L2 negates the favoured key, cosine
    # the disfavoured one; -0 comes back as +0)
    f_out = f_key[f_order] if metric == COS else (-f_key[f_order]) + ZERO
    d_out = (-d_key[d_order]) + ZERO if metric == COS else d_key[d_order]
    score = np.concatenate([f_out, d_out]).astype(_F32)[:k]
    side = np.concatenate([np.ones(len(f_rows), np.uint8), np.zeros(len(d_rows), np.uint8)])[:k]
    pad = k - len(ids)
    return (np.concatenate([ids, np.full(pad, -1)]).astype(np.int64), np.concatenate([score, np.zeros(pad, _F32)]),
            np.concatenate([side, np.zeros(pad, np.uint8)]), int(fav.sum()))


def _call(ix, queries, k, **kw):
    """queries: [(pos list, neg list)] -> the library's answer"""
    ex, off = [], [0]
    for pos, neg in queries:
        ex += list(pos)
        off.append(len(ex))
        ex += list(neg)
        off.append(len(ex))
    return ix.search_recommend(np.stack(ex), off, k, **kw)


def _assert_equal(got, want, q=0):
    idx, score, side = got
    assert (idx[q] == want[0]).all(), (idx[q][:12], want[0][:12])
    assert (score[q].view(np.uint32) == want[1].view(np.uint32)).all()
    assert (side[q] == want[2]).all()


def _examples(case, rng, count):
    rows = case[1]
    v = rows[rng.integers(0, len(rows) - 10, size=count)] + 0.05 * rng.standard_normal((count, rows.shape[1])).astype(_F32)
    return [(x / np.linalg.norm(x)).astype(_F32) for x in v]


SHAPES = [(2000, 64), (20000, 384), (70000, 516)]


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("npos,nneg,k", [(1, 1, 10), (5, 4, 64), (8, 0, 129), (32, 32, 10), (3, 1, 200)])
def test_matches_reference(native, metric, n, d, npos, nneg, k):
    case = _case(native, n, d, metric)
    rng = np.random.default_rng(npos * 100 + nneg)
    ex = _examples(case, rng, npos + nneg)
    pos, neg = ex[:npos], ex[npos:]
    want = _reference(case, metric, pos, neg, k)
    _assert_equal(_call(case[0], [(pos, neg)], k), want)
    assert case[0].get_option("last_recommend_path") == (1 if want[3] >= k else 2)


@pytest.mark.parametrize("metric", [COS, L2])
def test_one_positive_is_the_exact_top_k(native, metric):
    case = _case(native, 20000, 384, metric)
    ix, rows, _ = case
    q = _examples(case, np.random.default_rng(5), 1)
    got = _call(ix, [(q, [])], 10)
    _assert_equal(got, _reference(case, metric, q, [], 10))
    # (the reference above IS the exact top-k in exact_score's arithmetic.  wdbx_index_search sums a row in its scan's own lane
    # order, an ulp away, so only its ids are compared -- on this seeded corpus no two of the best scores are that close)
    idx, _ = ix.search(q[0][None, :], 10)
    assert (got[0][0] == idx[0]).all()
    assert (got[2] == 1).all() and ix.get_option("last_recommend_path") == 1 and ix.get_option("last_recommend_short") == 0


@pytest.mark.parametrize("metric", [COS, L2])
def test_negative_equal_to_positive_disfavours_every_row(native, metric):
    case = _case(native, 2000, 64, metric)
    q = _examples(case, np.random.default_rng(6), 1)
    got = _call(case[0], [(q, q)], 10)
    assert (got[2] == 0).all() and (got[0] >= 0).all()
    _assert_equal(got, _reference(case, metric, q, q, 10))
    assert case[0].get_option("last_recommend_path") == 2 and case[0].get_option("last_recommend_short") == 1


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("k", [10, 200])
def test_fewer_than_k_favoured_rows(native, metric, k):
    """the negative at the corpus mean is nearer to almost every row than the positive (row 7): only row 7 and its
    near-duplicates are favoured, the second pass fills the rest"""
    case = _case(native, 20000, 384, metric)
    ix, rows, _ = case
    mean = np.nanmean(rows.astype(np.float64), axis=0)
    neg = [(mean / np.linalg.norm(mean)).astype(_F32)]
    pos = [rows[7].copy()]
    want = _reference(case, metric, pos, neg, k)
    assert 0 < want[3] < 10
    got = _call(ix, [(pos, neg)], k)
    _assert_equal(got, want)
    assert got[2][0].sum() == want[3]
    assert ix.get_option("last_recommend_path") == 2 and ix.get_option("last_recommend_short") == 1


@pytest.mark.parametrize("metric", [COS, L2])
def test_mask_and_exclusion(native, metric):
    case = _case(native, 20000, 384, metric)
    ix, rows, _ = case
    rng = np.random.default_rng(8)
    ex = _examples(case, rng, 4)
    allowed = rng.random(len(rows)) < 0.3
    allowed[:40] = [i % 3 == 0 for i in range(40)]  # (a word with mixed bits)
    words = native.pack_row_mask(allowed)
    plain = _reference(case, metric, ex[:3], ex[3:], 10)
    exclude = sorted({0, len(rows) - 1, int(plain[0][0]), int(plain[0][3])})
    _assert_equal(_call(ix, [(ex[:3], ex[3:])], 10, mask_words=words), _reference(case, metric, ex[:3], ex[3:], 10, allowed=allowed))
    got = _call(ix, [(ex[:3], ex[3:])], 10, exclude_rows=exclude)
    _assert_equal(got, _reference(case, metric, ex[:3], ex[3:], 10, exclude=exclude))
    assert not set(got[0][0].tolist()) & set(exclude)
    masked_ex = [r for r in exclude if allowed[r]] + [int(np.flatnonzero(allowed)[5])]
    _assert_equal(_call(ix, [(ex[:3], ex[3:])], 10, mask_words=words, exclude_rows=sorted(set(masked_ex))),
                  _reference(case, metric, ex[:3], ex[3:], 10, allowed=allowed, exclude=masked_ex))


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("k", [10, 200])
def test_three_queries_equal_each_alone_and_runs_are_bit_equal(native, metric, k):
    case = _case(native, 20000, 384, metric)
    ix = case[0]
    ex = _examples(case, np.random.default_rng(9), 14)
    queries = [(ex[:1], []), (ex[1:4], ex[4:5]), (ex[5:6], ex[5:6] + ex[6:14])]
    first = _call(ix, queries, k)
    short = ix.get_option("last_recommend_short")
    again = _call(ix, queries, k)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    alone_short = 0
    for q, (pos, neg) in enumerate(queries):
        alone = _call(ix, [(pos, neg)], k)
        alone_short += ix.get_option("last_recommend_short")
        for a, b in zip(first, alone):
            assert a[q].tobytes() == b[0].tobytes()
        _assert_equal(first, _reference(case, metric, pos, neg, k), q)
    assert short == alone_short >= 1  # (the third query's positive is also a negative: all of its rows are disfavoured)


def test_empty_index(native):
    ix = native.NativeIndex(64, COS, 0, capacity_rows=16)
    try:
        idx, score, side = ix.search_recommend(np.ones((2, 64), _F32), [0, 1, 2], 5)
        assert (idx == -1).all() and (score == 0).all() and (side == 0).all()
        assert ix.get_option("last_recommend_path") == 0
    finally:
        ix.close()


def test_refusals_leave_the_handle_usable(native):
    case = _case(native, 2000, 64, COS)
    ix, rows, _ = case
    n = len(rows)
    v = np.stack(_examples(case, np.random.default_rng(10), 3))
    many = np.repeat(v[:1], 65, axis=0)
    bad = [
        (dict(examples=v, offsets=[0, 2, 3], k=0), "k=0"),
        (dict(examples=v, offsets=[0, 2, 3], k=native.MAX_K + 1), "k="),
        (dict(examples=v, offsets=[0, 0, 3], k=5), "query 0 has no positive example"),
        (dict(examples=v, offsets=[0, 2, 3, 3, 3], k=5), "query 1 has no positive example"),
        (dict(examples=many, offsets=[0, 33, 65], k=5), "query 0 has 65 examples"),
        (dict(examples=np.concatenate([v, v[:2]]), offsets=[1, 2, 5], k=5), "example_offsets[0] = 1"),
        (dict(examples=v, offsets=[0, 2, 1, 3, 3], k=5), "example_offsets decrease at entry 2 (query 0)"),
        (dict(examples=v, offsets=[0, 2, 3], k=5, mask_words=np.zeros((n + 31) // 32 - 1, np.uint32)), "row mask"),
        (dict(examples=v, offsets=[0, 2, 3], k=5, exclude_rows=[3, 3]), "entry 1 is 3"),
        (dict(examples=v, offsets=[0, 2, 3], k=5, exclude_rows=[5, 4]), "entry 1 is 4"),
        (dict(examples=v, offsets=[0, 2, 3], k=5, exclude_rows=[1, n]), f"entry 1 is {n}"),
        (dict(examples=v, offsets=[0, 2, 3], k=5, exclude_rows=list(range(1025))), "exclude_rows holds 1025 rows"),
    ]
    want = _reference(case, COS, list(v[:2]), list(v[2:]), 5)
    for kw, text in bad:
        kw = dict(kw)
        with pytest.raises(native.HipBackendError) as err:
            ix.search_recommend(kw.pop("examples"), kw.pop("offsets"), kw.pop("k"), **kw)
        assert text in str(err.value), (text, str(err.value))
        _assert_equal(ix.search_recommend(v, [0, 2, 3], 5), want)
    full = ix.search_recommend(v, [0, 2, 3], 5, exclude_rows=list(range(1024)))
    _assert_equal(full, _reference(case, COS, list(v[:2]), list(v[2:]), 5, exclude=range(1024)))


def test_raw_abi_refusals_and_null_out_side(native):
    """what the Python wrapper cannot send: nq < 1, every required pointer null in turn, a null exclude_rows with a count --
    each refused with WDBX_E_INVALID and followed by a good call; then out_side = NULL, which is allowed"""
    import ctypes as C

    case = _case(native, 2000, 64, COS)
    ix = case[0]
    v = np.ascontiguousarray(np.stack(_examples(case, np.random.default_rng(11), 3)))
    off = np.array([0, 2, 3], np.uint64)
    good = ix.search_recommend(v, off, 5)
    lib, h = ix._lib, ix._h
    f32p, i64p, u64p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    idx, score, side = np.empty((1, 5), np.int64), np.empty((1, 5), _F32), np.empty((1, 5), np.uint8)
    P = lambda a, t: a.ctypes.data_as(t)  # noqa: E731

    def call(nq=1, k=5, ex=P(v, f32p), offs=P(off, u64p), excl=None, n_excl=0, oi=P(idx, i64p), os_=P(score, f32p),
             sd=P(side, u8p)):
        return lib.wdbx_index_search_recommend(h, ex, offs, nq, k, 0, None, 0, excl, n_excl, oi, os_, sd)

    refused = [dict(nq=0), dict(nq=-1), dict(k=0), dict(k=native.MAX_K + 1), dict(ex=None), dict(offs=None), dict(oi=None),
               dict(os_=None), dict(excl=None, n_excl=2)]
    for kw in refused:
        assert call(**kw) == -1, kw  # WDBX_E_INVALID
        again = ix.search_recommend(v, off, 5)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(good, again)), kw
    assert call() == 0
    assert np.array_equal(idx, good[0]) and np.array_equal(score, good[1]) and np.array_equal(side, good[2])
    # out_side may be null
    idx[:], score[:] = -9, -9
    assert call(sd=None) == 0
    assert idx.tobytes() == good[0].tobytes() and score.tobytes() == good[1].tobytes()


# ---- every ranking route of the host call, and what each launches -------------------------------------------------------------
# (name, select_min_k, lds_lists): lists in registers up to k = 128 and in LDS above, the LDS lists whatever k is, the select chain
ROUTES = [("lists", 200, 0), ("lds_lists", 200, 1), ("select", 1, 0)]


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [20, 100])
def test_every_ranking_route_and_its_launch_counts(native, metric, d):
    """2 500 rows never bind the scratch bound, so a pass is ONE round: one scan launch, then one merge launch over the partial
    lists or, on the select route, one select-and-sort bracket per slot.  The disfavoured pass runs for the short queries only
    (here: a positive that is also the negative, and row 7 against the corpus mean), with the metric flipped in its tail."""
    case = _case(native, 2500, d, metric)
    ix, rows, _ = case
    ex = _examples(case, np.random.default_rng(40 + d), 12)
    mean = np.nanmean(rows.astype(np.float64), axis=0)
    mean = (mean / np.linalg.norm(mean)).astype(_F32)
    five = [(ex[:1], []), (ex[1:4], ex[4:5]), ([rows[7].copy()], [mean]), (ex[5:6], ex[5:6]), (ex[6:9], ex[9:12])]
    calls = [(queries, k, [_reference(case, metric, pos, neg, k) for pos, neg in queries])
             for queries in (five[3:4], five) for k in (1, 10, 129)]  # (references first: they run range searches)
    ix.profile(True)
    try:
        for name, select_min_k, lds_lists in ROUTES:
            ix.set_option("select_min_k", select_min_k)
            ix.set_option("lds_lists", lds_lists)
            for queries, k, want in calls:
                nq, ns = len(queries), sum(w[3] < k for w in want)
                assert ns >= 1
                ix.profile_read()
                got = _call(ix, queries, k)
                prof = ix.profile_read()
                what = (name, nq, k, prof)
                for q in range(nq):
                    _assert_equal(got, want[q], q)
                assert ix.get_option("last_recommend_path") == 2 and ix.get_option("last_recommend_short") == ns, what
                assert prof["scan_launches"] == 2, what  # (one round per side)
                assert prof["merge_launches"] == (nq + ns if name == "select" else 2), what
            # 257 queries (the five, again and again): a round holds at most 256, so the favoured pass's second round writes its
            # one query's results from slot 256 on; the short queries (fewer than 256) are one round of the disfavoured pass
            want = [calls[4][2][q % 5] for q in range(257)]
            ns = sum(w[3] < 10 for w in want)
            assert 1 <= ns <= 256
            ix.profile_read()
            got = _call(ix, [five[q % 5] for q in range(257)], 10)
            prof = ix.profile_read()
            what = (name, "two rounds", ns, prof)
            for q in range(257):
                _assert_equal(got, want[q], q)
            assert ix.get_option("last_recommend_short") == ns, what
            assert prof["scan_launches"] == 3, what
            assert prof["merge_launches"] == (257 + ns if name == "select" else 3), what
    finally:
        ix.profile(False)
        ix.set_option("select_min_k", 200)
        ix.set_option("lds_lists", 0)
