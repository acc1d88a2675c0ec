"""Search among listed rows on the MI355X (wdbx_index_search_rows and its public forms): the exact top-k of an explicit row
list.  1. integer corpora, where every fp32 score is exact: ids and scores equal a numpy int64 reference with ``==`` on every
route; 2. float corpora against a float64 brute force inside the rounding band of tests/test_gpu_range_search.py; 3. bit
identity with the other search paths; 4. NaN / removed rows; 5. refusals; 6. the facade and config FILTER_GATHER_MAX_ROWS."""
import asyncio
import shutil
import tempfile

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
KEYS, LISTS, SELECT = 1, 2, 3
N_INT = 5000
SIZES = (0, 1, 63, 64, 65, 257, 4097, N_INT)
KS = (1, 10, 16, 17, 64, 65, 128, 129, 200, 2048)
NQS = (1, 2, 7, 8, 9, 33, 256)


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


# the routes, forced through their options: (rows_keys_max, select_min_k) -> what last_rows_path must say
def _routes(k, n_ids):
    if n_ids == 0:
        return [((8192, 200), 0)]
    out = [((1 << 30, 200), KEYS), ((0, 0), LISTS)]
    if k >= 200:
        out.append(((0, 200), SELECT))
    return out


def _search(ix, queries, k, ids, route, path):
    ix.set_option("rows_keys_max", route[0])
    ix.set_option("select_min_k", route[1])
    idx, score = ix.search_rows(queries, k, ids)
    assert ix.get_option("last_rows_path") == path, (route, path)
    return idx, score


# ---- 1. exact ids on exact arithmetic -------------------------------------------------------------------------------------
_INT = {}


def _int_case(native, d, metric):
    """5 000 rows and 256 queries with integer elements in {-2 .. 2} (d = 3: 125 distinct rows, so hundreds tie exactly), the
    index that holds them un-normalised and the int64 score of every (query, row), computed once per shape."""
    key = (d, metric)
    if key not in _INT:
        rng = np.random.default_rng(1000 + 10 * d + metric)
        rows = rng.integers(-2, 3, size=(N_INT, d)).astype(np.int64)
        queries = rng.integers(-2, 3, size=(256, d)).astype(np.int64)
        if metric == COS:
            score = queries @ rows.T
        else:
            score = ((queries[:, None, :] - rows[None, :, :]) ** 2).sum(axis=2)
        ix = native.NativeIndex(d, metric, 0, capacity_rows=N_INT)
        ix.add(rows.astype(np.float32), normalize=False)
        _INT[key] = (ix, queries.astype(np.float32), score)
    return _INT[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for ix, _, _ in _INT.values():
        ix.close()
    _INT.clear()


def _int_expected(score, metric, ids, nq, k):
    """(score descending, row ascending); L2: (distance ascending, row ascending); unused slots -1 / 0"""
    e_idx = np.full((nq, k), -1, np.int64)
    e_score = np.zeros((nq, k), np.float32)
    if len(ids):
        for qi in range(nq):
            s = score[qi, ids]
            order = np.lexsort((ids, -s if metric == COS else s))[:k]
            e_idx[qi, : len(order)] = ids[order]
            e_score[qi, : len(order)] = s[order]
    return e_idx, e_score


def _lists(rng, n_ids):
    """random, and clustered in the first / last 300 rows (the last row included)"""
    if n_ids in (0, N_INT):
        return [np.arange(n_ids, dtype=np.int64)]
    out = [np.sort(rng.choice(N_INT, n_ids, replace=False))]
    if n_ids <= 300:
        out.append(np.sort(rng.choice(300, n_ids, replace=False)))
        tail = np.sort(rng.choice(np.arange(N_INT - 300, N_INT - 1), n_ids - 1, replace=False))
        out.append(np.concatenate([tail, [N_INT - 1]]).astype(np.int64))
    return out


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [3, 54, 100])
def test_integer_corpora_equal_the_int64_reference_on_every_route(native, d, metric):
    ix, queries, score = _int_case(native, d, metric)
    rng = np.random.default_rng(d + metric)
    cases = []  # (ids, k, nq)
    for n_ids in SIZES:  # every list size and placement
        for ids in _lists(rng, n_ids):
            cases += [(ids, 10, 1), (ids, 10, 9)]
    for k in KS:  # every k, with k - 1, k and k + 1 listed rows and a long list
        for n_ids in sorted({max(k - 1, 1), k, k + 1, 4097}):
            ids = _lists(rng, n_ids)[0]
            cases += [(ids, k, 1), (ids, k, 8)]
    for nq in NQS:  # every query count, on each query block (8, 4, 1)
        for k in (10, 65, 129):
            for n_ids in (257, 4097):
                cases.append((_lists(rng, n_ids)[0], k, nq))
    seen = set()
    for ids, k, nq in cases:
        want = _int_expected(score, metric, ids, nq, k)
        for route, path in _routes(k, len(ids)):
            idx, sc = _search(ix, queries[:nq], k, ids, route, path)
            what = (d, metric, len(ids), k, nq, path)
            assert np.array_equal(idx, want[0]), what
            assert np.array_equal(sc, want[1]), what
            seen.add(path)
    assert seen == {0, KEYS, LISTS, SELECT}
    # (lists kept in LDS whatever k is: the other instance of the list route)
    ix.set_option("lds_lists", 1)
    try:
        for ids, k, nq in [(_lists(rng, 4097)[0], 10, 9), (_lists(rng, 257)[0], 128, 2)]:
            idx, sc = _search(ix, queries[:nq], k, ids, (0, 0), LISTS)
            want = _int_expected(score, metric, ids, nq, k)
            assert np.array_equal(idx, want[0]) and np.array_equal(sc, want[1]), (d, metric, k, nq, "lds_lists")
    finally:
        ix.set_option("lds_lists", 0)


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [20, 100])
def test_launch_counts_of_every_route(native, d, metric):
    """2 500 rows never bind the scratch bound, so a call is ONE round: the scoring launch (a scan launch), then one merge launch
    over the keys or the partial lists or, on the select route, one select-and-sort bracket per query"""
    n = 2500
    rng = np.random.default_rng(8000 + 10 * d + metric)
    rows = rng.integers(-2, 3, size=(n, d)).astype(np.int64)
    queries = rng.integers(-2, 3, size=(257, d)).astype(np.int64)
    score = queries @ rows.T if metric == COS else np.stack([((q[None, :] - rows) ** 2).sum(axis=1) for q in queries])
    ids = np.sort(rng.choice(n, 1500, replace=False))
    # (rows_keys_max, select_min_k, lds_lists) -> last_rows_path
    routes = [((1 << 30, 200, 0), KEYS), ((0, 200, 0), LISTS), ((0, 200, 1), LISTS), ((0, 1, 0), SELECT)]
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.add(rows.astype(np.float32), normalize=False)
        keep = ix.get_option("rows_keys_max")
        ix.profile(True)
        try:
            for route, path in routes:
                ix.set_option("lds_lists", route[2])
                for k in (1, 10, 129):
                    for nq in (1, 5):
                        want = _int_expected(score, metric, ids, nq, k)
                        ix.profile_read()
                        idx, sc = _search(ix, queries[:nq].astype(np.float32), k, ids, route, path)
                        prof = ix.profile_read()
                        what = (d, metric, route, k, nq, prof)
                        assert np.array_equal(idx, want[0]) and np.array_equal(sc, want[1]), what
                        assert prof["scan_launches"] == 1, what
                        assert prof["merge_launches"] == (nq if path == SELECT else 1), what
                # 257 queries: a round holds at most 256, so the second round writes its one query's results from slot 256 on
                want = _int_expected(score, metric, ids, 257, 10)
                ix.profile_read()
                idx, sc = _search(ix, queries.astype(np.float32), 10, ids, route, path)
                prof = ix.profile_read()
                what = (d, metric, route, "two rounds", prof)
                assert np.array_equal(idx, want[0]) and np.array_equal(sc, want[1]), what
                assert prof["scan_launches"] == 2, what
                assert prof["merge_launches"] == (257 if path == SELECT else 2), what
        finally:
            ix.profile(False)
            ix.set_option("rows_keys_max", keep)
            ix.set_option("select_min_k", 200)
            ix.set_option("lds_lists", 0)


# ---- 2. float data against float64 ----------------------------------------------------------------------------------------
def _float_corpus(n, d, metric, seed):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    if metric == COS:
        rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    return rows


def _check_float(rows, q, metric, ids, k, got_idx, got_score, what):
    r, q64 = rows[ids].astype(np.float64), q.astype(np.float64)
    if metric == COS:
        ref = r @ q64
        band = 2e-5 * np.maximum(1.0, np.linalg.norm(r, axis=1) * np.linalg.norm(q64))
        better = ref  # higher is better
    else:
        ref = ((r - q64) ** 2).sum(axis=1)
        band = 2e-5 * np.maximum(1.0, (r * r).sum(axis=1) + q64 @ q64)
        better = -ref
    kk = min(k, len(ids))
    assert np.all(got_idx[kk:] == -1) and np.all(got_score[kk:] == 0), what
    g_idx, g_score = got_idx[:kk], got_score[:kk]
    assert np.all(g_idx >= 0) and len(np.unique(g_idx)) == kk, what  # no duplicates, every slot used
    pos = np.minimum(np.searchsorted(ids, g_idx), len(ids) - 1)
    assert np.array_equal(ids[pos], g_idx), (what, "a row outside the list came back")
    kth = np.sort(better)[::-1][kk - 1]
    got = np.zeros(len(ids), bool)
    got[pos] = True
    must = better > kth + band
    assert not np.any(must & ~got), (what, ids[must & ~got][:5])
    assert np.all(better[pos] >= kth - band[pos]), what
    assert np.all(np.abs(g_score.astype(np.float64) - ref[pos]) <= band[pos]), what
    key = (-g_score if metric == COS else g_score).astype(np.float64)
    assert np.array_equal(np.lexsort((g_idx, key)), np.arange(kk)), (what, "order")


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("n,d", [(10000, 384), (10000, 768), (1000, 4096)])
def test_float_corpora_against_float64(native, n, d, metric):
    rows = _float_corpus(n, d, metric, seed=n + d + metric)
    queries = _float_corpus(9, d, metric, seed=7 * d + metric)
    rng = np.random.default_rng(d)
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.add(rows, normalize=False)
        for n_ids in (n * 3 // 10, 50):
            ids = np.sort(rng.choice(n, n_ids, replace=False)).astype(np.int64)
            for k in (10, 100):
                for nq in (1, 9):
                    for route, path in _routes(k, n_ids):
                        idx, sc = _search(ix, queries[:nq], k, ids, route, path)
                        for qi in range(nq):
                            _check_float(rows, queries[qi], metric, ids, k, idx[qi], sc[qi], (n, d, metric, n_ids, k, nq, path, qi))


# ---- 3. bit-identity with the existing paths ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
def test_bit_identical_to_search_masked_search_and_batch(native, metric):
    n, d, k = 131072, 64, 10
    rng = np.random.default_rng(5 + metric)
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 16, d))
        ix.profile(True)
        ix.profile_read()
        # lone queries: the u8 selection scan + exact re-scoring, no fp32 repair
        for q in queries[:3]:
            u_idx, u_score = ix.search(q, k)
            assert ix.get_option("last_single_path") == 2 and ix.profile_read()["scan_launches"] == 0
            ids = np.union1d(u_idx[0], rng.choice(n, 3000, replace=False)).astype(np.int64)
            allowed = np.zeros(n, bool)
            allowed[ids] = True
            m_idx, m_score = ix.search(q, k, mask_words=native.pack_row_mask(allowed))
            assert ix.get_option("last_single_path") == 2 and ix.profile_read()["scan_launches"] == 0
            for route, path in _routes(k, len(ids)):
                idx, score = _search(ix, q, k, ids, route, path)
                assert ix.profile_read()["scan_launches"] == 1  # (the scoring launch of the listed rows is a scan launch)
                assert np.array_equal(idx, u_idx) and np.array_equal(score.view(np.uint32), u_score.view(np.uint32)), path
                assert np.array_equal(idx, m_idx) and np.array_equal(score.view(np.uint32), m_score.view(np.uint32)), path
        # a batch: the int8 tiles + exact re-scoring
        b_idx, b_score = ix.search(queries, k)
        assert ix.get_option("last_gemm_family") in (0, 1, 2, 3)
        repaired = ix.get_option("last_batch_repaired") != 0 and ix.batch_status(len(queries))["overflowed"] != 0
        ids = np.union1d(b_idx.ravel(), rng.choice(n, 3000, replace=False)).astype(np.int64)
        ids = ids[ids >= 0]
        for route, path in _routes(k, len(ids)):
            idx, score = _search(ix, queries, k, ids, route, path)
            assert np.array_equal(idx, b_idx), path
            if not repaired:
                assert np.array_equal(score.view(np.uint32), b_score.view(np.uint32)), path


# ---- 4. NaN and removed rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
def test_nan_and_removed_rows_are_never_returned(native, metric):
    n, d = 2000, 54
    rows = _float_corpus(n, d, metric, seed=3)
    dead = np.array([0, 5, 77, 1024, n - 1])
    rows[dead[:3]] = np.nan           # removed rows (HipFlatIndex.remove writes NaN)
    rows[dead[3:], 7] = np.nan        # a NaN element
    q = _float_corpus(2, d, metric, seed=4)
    live = np.setdiff1d(np.arange(n), dead)
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.add(rows, normalize=False)
        ids = np.union1d(dead, live[::7]).astype(np.int64)
        n_live = len(ids) - len(dead)
        for k in (10, 400):
            for route, path in _routes(k, len(ids)):
                idx, score = _search(ix, q, k, ids, route, path)
                assert not np.isin(idx, dead).any() and not np.isnan(score).any(), (k, path)
                assert np.all((idx >= 0).sum(axis=1) == min(k, n_live)), (k, path)
                for qi in range(2):
                    _check_float(rows, q[qi], metric, np.setdiff1d(ids, dead), min(k, n_live), idx[qi][: min(k, n_live)],
                                 score[qi][: min(k, n_live)], (k, path))
                idx, score = _search(ix, q, k, dead, route, path)  # a list made only of such rows
                assert np.all(idx == -1) and np.all(score == 0), (k, path)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(native):
    n, d = 1000, 16
    rows = _float_corpus(n, d, COS, seed=8)
    q = _float_corpus(1, d, COS, seed=9)
    with native.NativeIndex(d, COS, 0, capacity_rows=n) as ix:
        ix.add(rows, normalize=False)
        good = np.array([3, 10, 500, n - 1])
        want = ix.search_rows(q, 4, good)
        assert sorted(want[0][0].tolist()) == good.tolist()
        for ids, k in (([10, 3, 500], 2), ([3, 10, 10, 500], 2), ([3, 10, n], 2), (good, 0), (good, 2049)):
            with pytest.raises(native.HipBackendError) as e:
                ix.search_rows(q, k, np.asarray(ids))
            assert e.value.code == -1, (ids, k)  # WDBX_E_INVALID
            again = ix.search_rows(q, 4, good)   # a correct call follows
            assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
        # a list built before an add stays valid afterwards: row numbers do not move
        ix.add(_float_corpus(500, d, COS, seed=10), normalize=False)
        again = ix.search_rows(q, 4, good)
        assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
        idx, _ = ix.search_rows(q, 2, np.array([n, n + 499]))  # ... and the new rows can be listed
        assert sorted(idx[0].tolist()) == [n, n + 499]
        idx, score = ix.search_rows(q, 3, np.empty(0, np.int64))  # n_ids == 0 is valid
        assert np.all(idx == -1) and np.all(score == 0) and ix.get_option("last_rows_path") == 0


# ---- 6. the facade --------------------------------------------------------------------------------------------------------
@pytest.fixture()
def temp_dir():
    path = tempfile.mkdtemp(prefix="wdbx_rows_")
    yield path
    shutil.rmtree(path, ignore_errors=True)


def _brute(unit, q, names, limit, threshold=0.0):
    """[(id, float64 score)] best first over the named rows (row_<i>), as VectorStore._merge cuts it"""
    qn = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64))
    rows = np.array(sorted({int(v[4:]) for v in names}))
    s = unit[rows].astype(np.float64) @ qn
    order = np.argsort(-s, kind="stable")
    out = [(f"row_{rows[i]}", float(s[i])) for i in order if not (threshold > 0 and s[i] < threshold)]
    return out[:limit]


def _same(got, want):
    assert [g[0] for g in got] == [w[0] for w in want]
    np.testing.assert_allclose([g[1] for g in got], [w[1] for w in want], atol=2e-5, rtol=0)


def test_facade_search_among_and_filter_gather(temp_dir):
    from wdbx_amd import WDBX

    d, n = 16, 4000
    raw = O.synth_rows(O.SEED_CORPUS, 0, n, d)
    unit = raw / np.linalg.norm(raw.astype(np.float64), axis=1, keepdims=True)
    meta = {f"row_{i}": {"tenant": "a" if i % 571 == 3 else "b" if i % 8 == 1 else "c"} for i in range(n)}
    w = WDBX(vector_dimension=d, num_shards=2, data_dir=temp_dir, enable_plugins=False)
    vs = w.vector_store
    vs.bulk_store(raw, metadata=meta)
    assert all(1500 < ix.next_index < 2500 for ix in vs.indices)
    rng = np.random.default_rng(2)
    q = O.synth_rows(O.SEED_QUERY, 0, 1, d)[0]
    names = [f"row_{i}" for i in rng.permutation(n)[:300]]  # any order
    assert w.delete_vector(names[5]) is True
    asked = names + ["nobody", "row_999999", names[7]]  # unknown ids, a repeated id and a deleted one are ignored
    live = [v for v in names if v != names[5]]
    got = w.vector_search_among(q.tolist(), asked, limit=10)
    assert vs.last_search_path == "threads"
    _same(got, _brute(unit, q, live, 10))
    assert all(g[2] == meta[g[0]] for g in got)
    t = got[4][1] - 1e-4  # a threshold between the 5th and the following scores
    cut = w.vector_search_among(q.tolist(), asked, limit=10, threshold=t)
    _same(cut, _brute(unit, q, live, 10, threshold=t))
    assert 5 <= len(cut) < 10
    assert [g[0] for g in w.vector_search_among(q.tolist(), asked, limit=3)] == [g[0] for g in got[:3]]
    assert w.vector_search_among(q.tolist(), [], limit=10) == []
    assert w.vector_search_among(q.tolist(), ["nobody", names[5]], limit=10) == []
    qs = O.synth_rows(O.SEED_QUERY, 1, 5, d)
    batch = w.vector_search_batch_among(qs.tolist(), asked, limit=7)
    for qi in range(5):
        _same(batch[qi], _brute(unit, qs[qi], live, 7))
    _same(asyncio.run(w.vector_search_among_async(q.tolist(), asked, limit=10)), got)

    # config FILTER_GATHER_MAX_ROWS: a selective pushed-down filter answers from its rows alone
    def calls():
        return sum(ix.rows_searches for ix in vs.indices)

    flt_a, flt_b = {"tenant": "a"}, {"tenant": "b"}
    n_a = sum(1 for v in meta.values() if v["tenant"] == "a")
    assert n_a == 7
    before = calls()
    masked_a = w.vector_search(q.tolist(), limit=10, filter_metadata=flt_a, prefilter=True)
    masked_b = w.vector_search(q.tolist(), limit=10, filter_metadata=flt_b, prefilter=True)
    masked_batch = w.vector_search_batch(qs.tolist(), limit=10, filter_metadata=flt_a, prefilter=True)
    assert calls() == before  # the option is 0 by default: the mask path, as before
    w.config.set("FILTER_GATHER_MAX_ROWS", 100)
    got_a = w.vector_search(q.tolist(), limit=10, filter_metadata=flt_a, prefilter=True)
    used = calls() - before
    assert 1 <= used <= 2 and vs.last_search_path == "threads"
    assert any(ix._native.get_option("last_rows_path") in (KEYS, LISTS) for ix in vs.indices)
    assert len(got_a) == n_a
    _same(got_a, masked_a)
    _same(got_a, _brute(unit, q, [v for v, m in meta.items() if m["tenant"] == "a"], 10))
    got_batch = w.vector_search_batch(qs.tolist(), limit=10, filter_metadata=flt_a, prefilter=True)
    for a, b in zip(got_batch, masked_batch):
        _same(a, b)
    _same(asyncio.run(vs.search_async(q.tolist(), limit=10, filter_metadata=flt_a, prefilter=True)), masked_a)
    assert calls() > before + used
    # a filter matching 500 rows stays on the mask path
    before = calls()
    assert w.vector_search(q.tolist(), limit=10, filter_metadata=flt_b, prefilter=True) == masked_b
    assert calls() == before
    # the cached list is rebuilt after store / delete / update_metadata
    w.vector_store(q.tolist(), {"tenant": "a"}, id="fresh")
    now = w.vector_search(q.tolist(), limit=10, filter_metadata=flt_a, prefilter=True)
    assert now[0][0] == "fresh" and len(now) == n_a + 1
    assert w.delete_vector(got_a[0][0]) is True
    now = w.vector_search(q.tolist(), limit=10, filter_metadata=flt_a, prefilter=True)
    assert got_a[0][0] not in [r[0] for r in now] and len(now) == n_a
    assert w.update_metadata("row_1", {"tenant": "a"}) is True
    now = w.vector_search(q.tolist(), limit=10, filter_metadata=flt_a, prefilter=True)
    assert "row_1" in [r[0] for r in now] and len(now) == n_a + 1
    assert calls() >= before + 3
    asyncio.run(w.shutdown())
