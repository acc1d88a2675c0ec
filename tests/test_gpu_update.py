"""wdbx_index_set_rows_at / wdbx_index_remove_rows through the C ABI on the MI355X.

Twin indices hold the same rows and have every derived copy built (a search on each route first).  Index A takes a set of
updates row by row through ``set_rows``, index B the same updates in ONE ``set_rows_at``: afterwards both answer every route
with equal ids and equal score bits, the copies' coverages are unchanged, the top-k id set is the float64 oracle's on the
updated rows, and copies of a query planted at rows 0, 63, 64 and the last row win that query."""
import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

# K: the selection routes take a corpus from k * 8 * 128 rows on (u8_single_eligible and its kin): 2 048 <= N
N, K, NQ = 3001, 2, 16
COVERAGES = ("shadow_rows", "shadowg_rows", "shadow8_rows", "shadow6_rows", "shadow42_rows")

# option sets that steer a blocking search onto each route (applied on top of BASE), and how many queries go in one call
BASE = {"single_min_rows": 0, "gemm_min_rows": 0, "gemm_min_work": 1, "gemm_min_queries": 4, "scan_shadow": 2, "scan_u6": 0,
        "scan_u42": 0, "gemm_bf16": 3}
ROUTES = [
    ("u8 scan", {"gemm_min_queries": 1 << 30}, 1),
    ("u6 rounds", {"gemm_min_queries": 1 << 30, "scan_u6": 1}, NQ),
    ("u42 rounds", {"gemm_min_queries": 1 << 30, "scan_u6": 1, "scan_u42": 1}, NQ),
    ("i8 tiles", {"gemm_bf16": 3}, NQ),
    ("bf16 shadow tiles", {"gemm_bf16": 2}, NQ),
    ("bf16 tiles", {"gemm_bf16": 1}, NQ),
    ("fp32 tiles", {"gemm_bf16": 0}, NQ),
    ("fp32 scan", {"gemm_min_queries": 1 << 30, "scan_shadow": 0}, 1),
]


E_INVALID = -1  # WDBX_E_INVALID


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


def _answers(ix, queries):
    """{route: (idx, score bits)} of the queries on every route"""
    out = {}
    for name, opts, per_call in ROUTES:
        for key, value in {**BASE, **opts}.items():
            ix.set_option(key, value)
        idx, score = [], []
        for q0 in range(0, len(queries), per_call):
            i, s = ix.search(queries[q0:q0 + per_call], K)
            idx.append(i)
            score.append(s)
        out[name] = (np.concatenate(idx), np.concatenate(score).view(np.uint32))
    return out


def _coverages(ix):
    return {name: ix.get_option(name) for name in COVERAGES}


def _corpus(d, metric):
    rows = O.synth_rows(O.SEED_CORPUS, 0, N, d).astype(np.float32)
    queries = O.synth_rows(O.SEED_QUERY, 0, NQ, d).astype(np.float32)
    if metric == "cosine":
        rows, queries = O.normalize_rows_fast(rows), O.normalize_rows_fast(queries)
    return rows, queries


def _exact_topk(rows, q, metric):
    r, q = rows.astype(np.float64), q.astype(np.float64)
    s = r @ q if metric == "cosine" else -((r - q) ** 2).sum(axis=1)
    s = np.where(np.isnan(s), -np.inf, s)
    order = np.lexsort((np.arange(len(s)), -s))
    return order[:K], s[order[:K + 1]]


def _updates(d, queries, metric, seed=3):
    """row numbers (sorted) and their new contents: a random sixth of the rows and rows 0, 63, 64 and the last, which become
    copies of queries 0 .. 3; one NaN row, one zero row among them"""
    rng = np.random.default_rng(seed)
    planted = [0, 63, 64, N - 1]
    ids = np.unique(np.concatenate([rng.choice(N, N // 6, replace=False), planted]))
    new = rng.standard_normal((len(ids), d)).astype(np.float32)
    if metric == "cosine":
        new = O.normalize_rows_fast(new)
    free = [i for i, r in enumerate(ids) if r not in planted]
    new[free[0]] = np.nan
    new[free[1]] = 0.0
    for qi, r in enumerate(planted):
        new[int(np.searchsorted(ids, r))] = queries[qi]
    return ids.astype(np.uint64), new, planted


@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("d", [96, 384])
def test_one_listed_update_equals_the_per_row_updates_on_every_route(native, d, metric):
    rows, queries = _corpus(d, metric)
    ids, new, planted = _updates(d, queries, metric)
    m = native.METRIC_COSINE if metric == "cosine" else native.METRIC_L2
    with native.NativeIndex(d, metric=m, capacity_rows=N) as a, native.NativeIndex(d, metric=m, capacity_rows=N) as b:
        for ix in (a, b):
            ix.add(rows)
            _answers(ix, queries)                      # builds every copy the routes read
        cov = _coverages(a)
        assert cov == _coverages(b)
        if metric == "cosine":                         # every copy exists and covers every row
            assert all(cov[name] == N for name in COVERAGES), cov
        for r, row in zip(ids, new):
            a.set_rows(int(r), row)
        b.set_rows_at(ids, new)
        assert _coverages(a) == cov and _coverages(b) == cov
        assert np.array_equal(a.get_rows(0, N).view(np.uint32), b.get_rows(0, N).view(np.uint32))
        got_a, got_b = _answers(a, queries), _answers(b, queries)
        updated = b.get_rows(0, N)
    expect = rows.copy()
    expect[ids.astype(np.int64)] = new
    assert np.array_equal(updated.view(np.uint32), expect.view(np.uint32))
    exact = [_exact_topk(expect, q, metric) for q in queries]
    for name, _, _ in ROUTES:
        ia, sa = got_a[name]
        ib, sb = got_b[name]
        assert np.array_equal(ia, ib), name
        assert np.array_equal(sa, sb), name
        for qi in range(NQ):
            top, s = exact[qi]
            if s[K - 1] - s[K] > 1e-5:                 # (a k-th score tied within fp32 rounding names no unique set)
                assert set(ib[qi].tolist()) == set(top.tolist()), (name, qi)
        for qi, r in enumerate(planted):
            assert ib[qi, 0] == r, (name, qi)


def test_normalize_and_the_launch_count(native):
    d = 96
    rows, queries = _corpus(d, "cosine")
    rng = np.random.default_rng(9)
    with native.NativeIndex(d, capacity_rows=N) as a, native.NativeIndex(d, capacity_rows=N) as b:
        for ix in (a, b):
            ix.add(rows)
            _answers(ix, queries)
        ids = np.unique(rng.choice(N, 400, replace=False)).astype(np.uint64)
        raw = (rng.standard_normal((len(ids), d)) * 3).astype(np.float32)
        raw[5] = 0.0
        for r, row in zip(ids, raw):
            a.set_rows(int(r), row, normalize=True)
        b.set_rows_at(ids, raw, normalize=True)
        many = b.get_option("last_update_launches")
        assert np.array_equal(a.get_rows(0, N).view(np.uint32), b.get_rows(0, N).view(np.uint32))
        got_a, got_b = _answers(a, queries), _answers(b, queries)
        for name, _, _ in ROUTES:
            assert np.array_equal(got_a[name][0], got_b[name][0]) and np.array_equal(got_a[name][1], got_b[name][1]), name
        # launches per call: the same for 3 rows and for every row
        b.set_rows_at(ids[:3], raw[:3], normalize=True)
        three = b.get_option("last_update_launches")
        every = np.arange(N, dtype=np.uint64)
        b.set_rows_at(every, rows)
        assert b.get_option("last_update_launches") == three == many == 3
        b.remove_rows(ids[:3])
        assert b.get_option("last_update_launches") == 3


def test_removed_rows_appear_on_no_route_and_compact_still_works(native):
    d = 96
    rows, queries = _corpus(d, "cosine")
    rng = np.random.default_rng(4)
    with native.NativeIndex(d, capacity_rows=N) as a, native.NativeIndex(d, capacity_rows=N) as b:
        for ix in (a, b):
            ix.add(rows)
        first = _answers(b, queries)
        _answers(a, queries)
        # the rows the queries like best, and some others
        ids = np.unique(np.concatenate([first["fp32 scan"][0][:, :2].ravel(), rng.choice(N, 200, replace=False),
                                        [0, 63, 64, N - 1]])).astype(np.uint64)
        nan_row = np.full(d, np.nan, np.float32)
        for r in ids:
            a.set_rows(int(r), nan_row)
        b.remove_rows(ids)
        assert np.array_equal(a.get_rows(0, N).view(np.uint32), b.get_rows(0, N).view(np.uint32))
        stored = b.get_rows(0, N).view(np.uint32)
        assert np.all(stored[ids.astype(np.int64)] == 0x7FC00000)
        got_a, got_b = _answers(a, queries), _answers(b, queries)
        gone = set(ids.tolist())
        for name, _, _ in ROUTES:
            assert np.array_equal(got_a[name][0], got_b[name][0]) and np.array_equal(got_a[name][1], got_b[name][1]), name
            assert not gone & set(got_b[name][0].ravel().tolist()), name
            assert np.all(got_b[name][0] >= 0), name
        keep = np.setdiff1d(np.arange(N, dtype=np.uint64), ids)
        b.compact(keep)
        assert b.size() == len(keep)
        after = _answers(b, queries)
        for name, _, _ in ROUTES:
            assert np.array_equal(keep[after[name][0]], got_b[name][0]), name


def test_error_cases_and_the_empty_list(native):
    d = 20
    rows = O.synth_rows(O.SEED_CORPUS, 0, 100, d).astype(np.float32)
    with native.NativeIndex(d, capacity_rows=128) as ix:
        ix.add(rows)
        new = np.ones((2, d), np.float32)
        for bad in ([7, 7], [7, 3], [5, 100], [100, 101]):
            with pytest.raises(native.HipBackendError) as e:
                ix.set_rows_at(bad, new)
            assert e.value.code == E_INVALID
            with pytest.raises(native.HipBackendError) as e:
                ix.remove_rows(bad)
            assert e.value.code == E_INVALID
        assert np.array_equal(ix.get_rows(0, 100), rows)      # a refused list writes nothing
        lib = ix._lib
        assert lib.wdbx_index_set_rows_at(ix._h, None, 2, new.ctypes.data_as(native._f32p), 0) == E_INVALID
        ids = np.array([1, 2], np.uint64)
        assert lib.wdbx_index_set_rows_at(ix._h, ids.ctypes.data_as(native._u64p), 2, None, 0) == E_INVALID
        assert lib.wdbx_index_remove_rows(ix._h, None, 2) == E_INVALID
        assert lib.wdbx_index_set_rows_at(None, ids.ctypes.data_as(native._u64p), 2, new.ctypes.data_as(native._f32p), 0) == E_INVALID
        # n == 0: a no-op, null pointers or not
        assert lib.wdbx_index_set_rows_at(ix._h, None, 0, None, 0) == 0
        assert lib.wdbx_index_remove_rows(ix._h, None, 0) == 0
        ix.set_rows_at([], np.empty((0, d), np.float32))
        ix.remove_rows([])
        assert ix.get_option("last_update_launches") == 0
        assert np.array_equal(ix.get_rows(0, 100), rows)
        # first and last row of a narrow index
        ix.set_rows_at([0, 99], new)
        back = ix.get_rows(0, 100)
        assert np.array_equal(back[[0, 99]], new) and np.array_equal(back[1:99], rows[1:99])
        assert ix.get_option("last_update_launches") == 1      # no copy exists yet: the scatter alone
