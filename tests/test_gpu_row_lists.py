"""Batched search among listed rows with one row list PER QUERY on the MI355X (wdbx_index_search_row_lists and its public
forms).  1. - 4. integer corpora, where every fp32 score is exact (the scheme of tests/test_gpu_search_rows.py: 5 000
un-normalised rows with elements in {-2 .. 2}; at d = 1028 the largest |score| is 4 112 for the inner product and
16 * 1028 = 16 448 for the squared distance, both exact in fp32): ids AND scores equal a numpy int64 reference with
``array_equal`` on every kernel instance, on the block of one, over two rounds and on the list-by-list routes; 5. float data:
bit identity with wdbx_index_search_rows per query, inside the float64 band; 6. NaN / removed rows; 7. refusals; 8. the facade.

The share counts 1, 7, 8, 9 and 17 over twelve lists that each have a query need 17 + 9 + 8 + 7 + 8 * 1 = 49 queries, so
case 1 runs 49 queries per shape, not 40."""
import ctypes as C
import shutil
import tempfile

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
N_INT = 5000
CHUNK = 256  # ROWLISTS_CHUNK (host_rowlists.h; tests/test_row_lists_host.py pins the constant)
E_INVALID = -1
MAX_K = 2048


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


_INT = {}


def _int_case(native, d, metric):
    """5 000 rows and 300 queries with integer elements in {-2 .. 2}, the index that holds them un-normalised and the int64
    score of every (query, row), computed once per shape and left unchanged."""
    key = (d, metric)
    if key not in _INT:
        rng = np.random.default_rng(2000 + 10 * d + metric)
        rows = rng.integers(-2, 3, size=(N_INT, d)).astype(np.int64)
        queries = rng.integers(-2, 3, size=(300, d)).astype(np.int64)
        # (the products in float64 -- every value is a small integer, so the sums are exact -- then int64 for good)
        score = np.rint(queries.astype(np.float64) @ rows.T.astype(np.float64)).astype(np.int64)
        if metric == L2:
            score = (queries * queries).sum(axis=1)[:, None] + (rows * rows).sum(axis=1)[None, :] - 2 * score
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


def _expected(score, metric, lists, which, k):
    """per query (score descending, row ascending); L2: (distance ascending, row ascending); unused slots -1 / 0"""
    nq = len(which)
    e_idx = np.full((nq, k), -1, np.int64)
    e_score = np.zeros((nq, k), np.float32)
    for qi, c in enumerate(which):
        ids = np.asarray(lists[c], np.int64)
        if len(ids):
            s = score[qi, ids]
            order = np.lexsort((ids, -s if metric == COS else s))[:k]
            e_idx[qi, : len(order)] = ids[order]
            e_score[qi, : len(order)] = s[order]
    return e_idx, e_score


def _pick(rng, n):
    return np.sort(rng.choice(N_INT, n, replace=False)).astype(np.uint64)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


# ---- 1. every instance -------------------------------------------------------------------------------------------------------
SHARES = (17, 9, 8, 7, 1, 1, 1, 1, 1, 1, 1, 1)


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [3, 54, 100, 520, 1028])  # pitch4 <= 128: NI = 2; 130: NI = 4; 257: the NI = 0 loop
def test_every_instance_equals_the_int64_reference(native, d, metric):
    ix, queries, score = _int_case(native, d, metric)
    ix.set_option("rows_keys_max", 8192)
    rng = np.random.default_rng(d + metric)
    for turn, k in enumerate((1, 10, 128, 600)):
        lengths = [0, 1, 3, k - 1, k, k + 1, CHUNK - 1, CHUNK, CHUNK + 1, 1000, 4097]
        lists = [_pick(rng, n) for n in lengths]
        lists.append(np.unique(np.concatenate([rng.choice(N_INT - 1, 39, replace=False), [N_INT - 1]])).astype(np.uint64))  # the last row
        # every list has a query; the share counts move over the lists from k to k; interleaved in the caller's order
        shares = SHARES[-3 * turn:] + SHARES[:-3 * turn] if turn else SHARES
        which = np.repeat(np.arange(12), shares)
        which = which[np.random.default_rng(turn).permutation(len(which))]
        assert len(which) == 49 and sorted(np.bincount(which, minlength=12).tolist()) == sorted(SHARES)
        got = ix.search_row_lists(queries[:49], k, lists, which)
        assert ix.get_option("last_lists_path") == 1 and ix.get_option("last_lists_rounds") == 1
        items = sum(-(-len(r) // CHUNK) * -(-n // 8) for r, n in zip(lists, np.bincount(which, minlength=12)))
        assert ix.get_option("last_lists_items") == items
        _same(got, _expected(score, metric, lists, which, k), (d, metric, k))


# ---- 2. the block of one ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [54, 520, 1028])
def test_a_list_per_query_runs_the_block_of_one(native, d, metric):
    ix, queries, score = _int_case(native, d, metric)
    ix.set_option("rows_keys_max", 8192)
    rng = np.random.default_rng(10 + d + metric)
    nq, k = 33, 10
    lengths = [0, 1, 3, 9, 10, 11, CHUNK - 1, CHUNK, CHUNK + 1, 1000, 4097] + [int(n) for n in rng.integers(1, 700, nq - 11)]
    lists = [_pick(rng, n) for n in lengths]
    which = rng.permutation(nq)
    got = ix.search_row_lists(queries[:nq], k, lists, which)
    assert ix.get_option("last_lists_path") == 1
    assert ix.get_option("last_lists_items") == sum(-(-n // CHUNK) for n in lengths)  # one query block per chunk
    _same(got, _expected(score, metric, lists, which, k), (d, metric))


# ---- 3. rounds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
def test_more_than_256_queries_take_two_rounds(native, metric):
    ix, queries, score = _int_case(native, 54, metric)
    ix.set_option("rows_keys_max", 8192)
    rng = np.random.default_rng(20 + metric)
    nq, k = 300, 10
    lists = [_pick(rng, 64) for _ in range(nq)]
    which = np.arange(nq)
    got = ix.search_row_lists(queries, k, lists, which)
    assert ix.get_option("last_lists_rounds") == 2 and ix.get_option("last_lists_path") == 1
    _same(got, _expected(score, metric, lists, which, k), metric)
    # shared lists over two rounds: 300 queries on 3 lists, the middle list's queries straddle the round boundary
    lists = [_pick(rng, n) for n in (700, 64, 300)]
    which = rng.integers(0, 3, nq)
    got = ix.search_row_lists(queries, k, lists, which)
    assert ix.get_option("last_lists_rounds") == 2
    _same(got, _expected(score, metric, lists, which, k), (metric, "shared"))


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [20, 100])
def test_launch_counts_per_round(native, d, metric):
    """every round is one scoring launch (a scan launch) and one merge launch over the slots' keys with their list lengths as
    counts; 300 queries are two rounds, the second writes its results from slot 256 on"""
    n = 2500
    rng = np.random.default_rng(7000 + 10 * d + metric)
    rows = rng.integers(-2, 3, size=(n, d)).astype(np.int64)
    queries = rng.integers(-2, 3, size=(300, d)).astype(np.int64)
    score = queries @ rows.T if metric == COS else np.stack([((q[None, :] - rows) ** 2).sum(axis=1) for q in queries])
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.add(rows.astype(np.float32), normalize=False)
        keep = ix.get_option("rows_keys_max")
        ix.set_option("rows_keys_max", 8192)
        ix.profile(True)
        try:
            for nq, k, rounds in [(1, 1, 1), (1, 10, 1), (1, 129, 1), (5, 1, 1), (5, 10, 1), (5, 129, 1), (300, 10, 2)]:
                lists = [np.sort(rng.choice(n, int(m), replace=False)).astype(np.uint64) for m in rng.integers(1, 400, min(nq, 7))]
                which = rng.integers(0, len(lists), nq)
                which[: len(lists)] = np.arange(len(lists))[:nq]  # (every list has a query)
                ix.profile_read()
                got = ix.search_row_lists(queries[:nq].astype(np.float32), k, lists, which)
                prof = ix.profile_read()
                what = (d, metric, nq, k, prof)
                assert ix.get_option("last_lists_path") == 1 and ix.get_option("last_lists_rounds") == rounds, what
                _same(got, _expected(score, metric, lists, which, k), what)
                assert prof["scan_launches"] == rounds and prof["merge_launches"] == rounds, what
        finally:
            ix.profile(False)
            ix.set_option("rows_keys_max", keep)


# ---- 4. the list-by-list route, alone and mixed ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
def test_fall_back_and_mixed_routes_give_the_same_answers(native, metric):
    ix, queries, score = _int_case(native, 100, metric)
    rng = np.random.default_rng(30 + metric)
    lists = [_pick(rng, 64), _pick(rng, 65), _pick(rng, 0), _pick(rng, 2000)]
    which = np.array([0, 1, 1, 0, 2, 3, 1, 0, 3, 0, 2, 1], np.int32)
    k = 10
    want = _expected(score, metric, lists, which, k)
    try:
        for keys_max, path in ((8192, 1), (64, 2), (0, 3)):
            ix.set_option("rows_keys_max", keys_max)
            got = ix.search_row_lists(queries[: len(which)], k, lists, which)
            assert ix.get_option("last_lists_path") == path, keys_max
            _same(got, want, (metric, keys_max))
    finally:
        ix.set_option("rows_keys_max", 8192)
    # only empty lists: nothing is launched
    got = ix.search_row_lists(queries[:3], k, [lists[2], lists[2]], [0, 1, 0])
    assert ix.get_option("last_lists_path") == 0 and ix.get_option("last_lists_items") == 0
    assert np.all(got[0] == -1) and np.all(got[1] == 0)


# ---- 5. float data: bit identity with search_rows, inside the float64 band ------------------------------------------------------
def _float_corpus(n, d, metric, seed):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    if metric == COS:
        rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    return rows


def _check_float(rows, q, metric, ids, k, got_idx, got_score, what):
    """(the rule of tests/test_gpu_search_rows.py::_check_float)"""
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
def test_float_data_is_bit_identical_to_search_rows_per_query(native, metric):
    n, d, nq, k = 10000, 384, 20, 10
    rows = _float_corpus(n, d, metric, seed=n + d + metric)
    queries = _float_corpus(nq, d, metric, seed=7 * d + metric)
    rng = np.random.default_rng(d + metric)
    lists = [np.sort(rng.choice(n, 500, replace=False)).astype(np.uint64) for _ in range(nq)]
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.add(rows, normalize=False)
        idx, score = ix.search_row_lists(queries, k, lists, np.arange(nq))
        assert ix.get_option("last_lists_path") == 1
        shared = ix.search_row_lists(queries, k, lists[:2], np.arange(nq) % 2)  # the block of eight on float data too
        for qi in range(nq):
            one = ix.search_rows(queries[qi], k, lists[qi])
            assert np.array_equal(idx[qi], one[0][0]), (metric, qi)
            assert np.array_equal(score[qi].view(np.uint32), one[1][0].view(np.uint32)), (metric, qi)
            _check_float(rows, queries[qi], metric, lists[qi].astype(np.int64), k, idx[qi], score[qi], (metric, qi))
            one = ix.search_rows(queries[qi], k, lists[qi % 2])
            assert np.array_equal(shared[0][qi], one[0][0]), (metric, qi, "shared")
            assert np.array_equal(shared[1][qi].view(np.uint32), one[1][0].view(np.uint32)), (metric, qi, "shared")


# ---- 6. NaN and removed rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
def test_nan_and_removed_rows_are_never_returned(native, metric):
    n, d = 2000, 54
    rows = _float_corpus(n, d, metric, seed=3)
    dead = np.array([0, 5, 77, 1024, n - 1])
    rows[dead[:3]] = np.nan           # removed rows (HipFlatIndex.remove writes NaN)
    rows[dead[3:], 7] = np.nan        # a NaN element
    q = _float_corpus(4, d, metric, seed=4)
    live = np.setdiff1d(np.arange(n), dead)
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.add(rows, normalize=False)
        ids = np.union1d(dead, live[::7]).astype(np.uint64)
        n_live = len(ids) - len(dead)
        for k in (10, 400):
            idx, score = ix.search_row_lists(q, k, [ids, dead.astype(np.uint64)], [0, 1, 0, 1])
            assert not np.isin(idx, dead).any() and not np.isnan(score).any(), k
            kk = min(k, n_live)
            for qi in (0, 2):
                assert (idx[qi] >= 0).sum() == kk, (k, qi)
                _check_float(rows, q[qi], metric, np.setdiff1d(ids.astype(np.int64), dead), kk, idx[qi][:kk], score[qi][:kk], (k, qi))
            for qi in (1, 3):  # a list made only of such rows
                assert np.all(idx[qi] == -1) and np.all(score[qi] == 0), (k, qi)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(native):
    n, d = 1000, 16
    rows = _float_corpus(n, d, COS, seed=8)
    q = np.ascontiguousarray(_float_corpus(3, d, COS, seed=9))
    lib = native.load_library()
    f32p, i64p, u64p, i32p = (C.POINTER(t) for t in (C.c_float, C.c_int64, C.c_uint64, C.c_int32))
    with native.NativeIndex(d, COS, 0, capacity_rows=n) as ix:
        ix.add(rows, normalize=False)
        good = [np.array([3, 10, 500, n - 1], np.uint64), np.array([7, 8], np.uint64)]
        which = [0, 1, 0]
        want = ix.search_row_lists(q, 4, good, which)
        assert sorted(want[0][0].tolist()) == [3, 10, 500, n - 1] and sorted(want[0][1].tolist()) == [-1, -1, 7, 8]
        out_idx, out_score = np.empty((3, MAX_K + 1), np.int64), np.empty((3, MAX_K + 1), np.float32)

        def call(lists, which, offsets=None, nq=3, k=4, n_lists=None):
            flat = np.ascontiguousarray(np.concatenate([np.asarray(r, np.uint64) for r in lists] + [np.empty(0, np.uint64)]))
            off = np.concatenate([[0], np.cumsum([len(r) for r in lists])]) if offsets is None else offsets
            off = np.ascontiguousarray(off, np.uint64)
            w = np.ascontiguousarray(which, np.int32)
            return lib.wdbx_index_search_row_lists(ix._h, q.ctypes.data_as(f32p), nq, k, 0, flat.ctypes.data_as(u64p),
                                                   off.ctypes.data_as(u64p), len(lists) if n_lists is None else n_lists,
                                                   w.ctypes.data_as(i32p), out_idx.ctypes.data_as(i64p), out_score.ctypes.data_as(f32p))

        assert call(good, which) == 0
        refused = [
            dict(lists=[good[0], [10, 3, 500]], which=which),            # an unsorted list
            dict(lists=[[3, 10, 10, 500], good[1]], which=which),        # a duplicate
            dict(lists=[good[0], [3, 10, n]], which=which),              # a row equal to the row count
            dict(lists=[good[0], good[1], [5, 4]], which=which),         # ... in a list no query names
            dict(lists=good, which=which, offsets=[1, 4, 6]),            # offsets not starting at 0
            dict(lists=good, which=which, offsets=[0, 4, 3]),            # decreasing offsets
            dict(lists=good, which=[0, -1, 0]),                          # no "-1 = every row"
            dict(lists=good, which=[0, 2, 0]),                           # = n_lists
            dict(lists=good, which=which, k=0),
            dict(lists=good, which=which, k=MAX_K + 1),
            dict(lists=good, which=which, nq=0),
            dict(lists=good, which=which, n_lists=0),
            dict(lists=good, which=which, n_lists=-1),
        ]
        for kw in refused:
            assert call(**kw) == E_INVALID, kw
            again = ix.search_row_lists(q, 4, good, which)  # a correct call follows
            assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1]), kw
        with pytest.raises(native.HipBackendError) as e:
            ix.search_row_lists(q, 4, [good[0], np.array([9, 9], np.uint64)], which)
        assert e.value.code == E_INVALID and "list 1" in e.value.message and "entry 1" in e.value.message
        with pytest.raises(ValueError):
            ix.search_row_lists(q, 4, good, [0, 1])  # the binding: one entry per query


# ---- 8. the facade ----------------------------------------------------------------------------------------------------------
@pytest.fixture()
def temp_dir():
    path = tempfile.mkdtemp(prefix="wdbx_row_lists_")
    yield path
    shutil.rmtree(path, ignore_errors=True)


def test_facade_among_each_and_filter_gather_per_query(temp_dir):
    import asyncio

    from wdbx_amd import WDBX

    d, n, nq = 16, 4000, 12
    raw = O.synth_rows(O.SEED_CORPUS, 0, n, d)
    # five selective tenants (7 - 40 rows each), one that matches an eighth of the store, the rest
    def tenant(i):
        for t, m in enumerate((571, 331, 211, 149, 101)):
            if i % m == 3:
                return f"t{t}"
        return "b" if i % 8 == 1 else "c"
    meta = {f"row_{i}": {"tenant": tenant(i)} for i in range(n)}
    w = WDBX(vector_dimension=d, num_shards=2, data_dir=temp_dir, enable_plugins=False)
    vs = w.vector_store
    vs.bulk_store(raw, metadata=meta)
    rng = np.random.default_rng(2)
    qs = O.synth_rows(O.SEED_QUERY, 1, nq, d)
    id_lists = []
    for qi in range(nq):
        names = [f"row_{i}" for i in rng.permutation(n)[: int(rng.integers(1, 400))]]
        id_lists.append(names + ["nobody", names[0]])  # an unknown and a repeated id
    id_lists[3] = []
    id_lists[5] = list(id_lists[4])  # two queries with one list
    before = sum(ix.rows_searches for ix in vs.indices)
    got = w.vector_search_batch_among_each(qs.tolist(), id_lists, limit=7)
    assert sum(ix.rows_searches for ix in vs.indices) - before == len(vs.indices)  # one call per shard for the batch
    assert all(ix._native.get_option("last_lists_path") == 1 for ix in vs.indices)
    for qi in range(nq):
        assert got[qi] == w.vector_search_among(qs[qi].tolist(), id_lists[qi], limit=7), qi
    assert got[3] == [] and all(len(got[qi]) == 7 for qi in range(nq) if len(id_lists[qi]) > 20)
    with pytest.raises(ValueError):
        w.vector_search_batch_among_each(qs.tolist(), id_lists[:-1], limit=7)

    # a batch with a filter per query: the filters that travel as their rows share one call per shard
    filters = [{"tenant": f"t{qi % 5}"} for qi in range(nq)]
    filters[5], filters[10], filters[11] = None, {"tenant": "b"}, {"tenant": "c"}  # (t0 .. t4 all stay in the batch)

    def run(per_query):
        w.config.set("FILTER_GATHER_MAX_ROWS", 100)
        w.config.set("FILTER_GATHER_PER_QUERY", per_query)
        start = [ix.rows_searches for ix in vs.indices]
        out = w.vector_search_batch(qs.tolist(), limit=10, filter_metadata=filters, prefilter=True)
        return out, [ix.rows_searches - s for ix, s in zip(vs.indices, start)]

    off, calls_off = run(False)
    on, calls_on = run(True)
    assert on == off
    assert all(r[2]["tenant"] == f["tenant"] for res, f in zip(on, filters) if f for r in res)
    assert calls_off == [5, 5] and calls_on == [1, 1]  # per shard: a call per selective filter against one call
    asyncio.run(w.shutdown())
