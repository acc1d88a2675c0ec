"""Distance matrix among listed rows on the MI355X through the C ABI (wdbx_index_search_matrix): every line against what
wdbx_index_search_rows returns for the anchor's stored vector over the list without the anchor -- ids and score bits -- on all
three routes; duplicates, removed rows, run-to-run identity, refusals, launch accounting and the device bytes of the call."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
KEYS, LISTS, SELECT = 1, 2, 3
N_ROWS = 3000
SIZES = (0, 1, 2, 9, 257, 600)
KS = (1, 10, 129)
# (rows_keys_max, select_min_k) -> what last_matrix_path must say
ROUTES = (((8192, 200), KEYS), ((0, 0), LISTS), ((0, 1), SELECT))


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


_IX = {}


def _index(native, d, metric):
    """3 000 random rows (cosine: normalised at add time), row 7 removed (a NaN row), rows 11 and 2 900 one vector"""
    key = (d, metric)
    if key not in _IX:
        rng = np.random.default_rng(500 + 10 * d + metric)
        rows = rng.standard_normal((N_ROWS, d)).astype(np.float32)
        rows[2900] = rows[11]
        ix = native.NativeIndex(d, metric, 0, capacity_rows=N_ROWS)
        ix.add(rows, normalize=metric == COS)
        ix.set_rows(7, np.full((1, d), np.nan, np.float32))
        _IX[key] = ix
    return _IX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for ix in _IX.values():
        ix.close()
    _IX.clear()


def _set_route(ix, route):
    ix.set_option("rows_keys_max", route[0])
    ix.set_option("select_min_k", route[1])


def _ids(seed, n, must=()):
    """n strictly increasing row numbers, not contiguous, holding `must`"""
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(N_ROWS), np.asarray(must, np.int64))
    pick = rng.choice(rest, n - len(must), replace=False)
    return np.sort(np.concatenate([pick, np.asarray(must, np.int64)])).astype(np.uint64)


def _reference(ix, ids, k):
    """line i: wdbx_index_search_rows(get_rows(ids[i]), normalize 0, the list without entry i), all lines in one
    wdbx_index_search_row_lists call (bit-identical to the single calls by its contract)"""
    _set_route(ix, ROUTES[0][0])
    n = len(ids)
    queries = np.concatenate([ix.get_rows(int(r), 1) for r in ids])
    lists = [np.delete(ids, i) for i in range(n)]
    return ix.search_row_lists(queries, k, lists, np.arange(n, dtype=np.int32), normalize_queries=False)


def _same(got, want):
    return (got[0] == want[0]).all() and (got[1].view(np.uint32) == want[1].view(np.uint32)).all()


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [64, 384, 1100])
@pytest.mark.parametrize("n", SIZES)
def test_every_line_is_the_listed_row_search_without_the_anchor(native, d, metric, n):
    ix = _index(native, d, metric)
    ids = _ids(n * 31 + d, n, must=(7, 11, 2900) if n >= 9 else ())
    for k in KS:
        want = _reference(ix, ids, k) if n else (np.empty((0, k), np.int64), np.empty((0, k), np.float32))
        for route, path in ROUTES:
            _set_route(ix, route)
            got = ix.search_matrix(ids, k)
            assert got[0].shape == (n, k) and got[1].shape == (n, k)
            assert ix.get_option("last_matrix_path") == (path if n else 0), (route, n, k)
            assert ix.get_option("last_matrix_rounds") == -(-n // 256)
            assert _same(got, want), (route, n, k, np.argwhere(got[0] != want[0])[:5])
        if n:
            # self never comes back, and a line has at most n - 1 results
            assert not (got[0] == ids.astype(np.int64)[:, None]).any()
            assert ((got[0] >= 0).sum(axis=1) <= n - 1).all()
            assert np.isin(got[0][got[0] >= 0], ids.astype(np.int64)).all()
        if n >= 9:
            at = int(np.searchsorted(ids, 7))
            assert (got[0][at] == -1).all() and (got[1][at] == 0).all()  # the removed row's own line
            assert not (got[0] == 7).any()                                # and it is nobody's neighbour
    _set_route(ix, ROUTES[0][0])


@pytest.mark.parametrize("metric", [COS, L2])
def test_forty_copies_of_one_vector(native, metric):
    d = 64
    rng = np.random.default_rng(77 + metric)
    rows = rng.standard_normal((500, d)).astype(np.float32)
    copies = np.sort(rng.choice(500, 40, replace=False))
    rows[copies] = rows[copies[0]]
    with native.NativeIndex(d, metric, 0, capacity_rows=500) as ix:
        ix.add(rows, normalize=metric == COS)
        ids = np.sort(np.union1d(copies, rng.choice(500, 100, replace=False))).astype(np.uint64)
        for route, path in ROUTES:
            _set_route(ix, route)
            idx, score = ix.search_matrix(ids, 10)
            assert ix.get_option("last_matrix_path") == path
            for c in copies:
                line = idx[int(np.searchsorted(ids, c))]
                assert line.tolist() == [int(x) for x in copies if x != c][:10]  # ten other copies, score-tied, in row order
                assert len(set(score[int(np.searchsorted(ids, c))].view(np.uint32).tolist())) == 1


def test_two_runs_give_identical_bytes(native):
    ix = _index(native, 384, COS)
    ids = _ids(5, 600)
    for route, _ in ROUTES:
        _set_route(ix, route)
        a = ix.search_matrix(ids, 10)
        b = ix.search_matrix(ids, 10)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    _set_route(ix, ROUTES[0][0])


def test_refusals_leave_the_handle_usable(native):
    ix = _index(native, 64, COS)
    good = np.array([3, 5, 9], np.uint64)
    want = ix.search_matrix(good, 2)
    lib = native.load_library()
    for ids, k, entry in (([5, 3, 9], 2, 1), ([3, 3, 9], 2, 1), ([3, 5, N_ROWS], 2, 2), ([1 << 40], 2, 0), ([3, 5, 9], 0, None),
                          ([3, 5, 9], native.MAX_K + 1, None), ([3, 5, 9], -1, None)):
        with pytest.raises(native.HipBackendError) as e:
            _raw(native, ix, np.asarray(ids, np.uint64), k)
        assert e.value.code == -1, (ids, k)  # WDBX_E_INVALID
        if entry is not None:
            assert f"entry {entry}" in str(e.value)
        assert _same(ix.search_matrix(good, 2), want)
    out_i, out_s = np.empty((3, 2), np.int64), np.empty((3, 2), np.float32)
    u64p, i64p, f32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_float)
    for args in ((None, 3, 2, out_i.ctypes.data_as(i64p), out_s.ctypes.data_as(f32p)),
                 (good.ctypes.data_as(u64p), 3, 2, None, out_s.ctypes.data_as(f32p)),
                 (good.ctypes.data_as(u64p), 3, 2, out_i.ctypes.data_as(i64p), None)):
        assert lib.wdbx_index_search_matrix(ix._h, *args) == -1
        assert _same(ix.search_matrix(good, 2), want)
    # nothing listed: WDBX_OK, nothing launched, null buffers are fine
    ix.profile(True)
    ix.profile_read()
    assert lib.wdbx_index_search_matrix(ix._h, None, 0, 2, None, None) == 0
    assert ix.get_option("last_matrix_path") == 0 and ix.get_option("last_matrix_rounds") == 0
    read = ix.profile_read()
    ix.profile(False)
    assert read["scan_launches"] == 0 and read["merge_launches"] == 0


def _raw(native, ix, ids, k):
    out_i, out_s = np.empty((len(ids), 8), np.int64), np.empty((len(ids), 8), np.float32)  # (room for any k the loop passes that could be served)
    rc = native.load_library().wdbx_index_search_matrix(ix._h, ids.ctypes.data_as(C.POINTER(C.c_uint64)), len(ids), k,
                                                        out_i.ctypes.data_as(C.POINTER(C.c_int64)),
                                                        out_s.ctypes.data_as(C.POINTER(C.c_float)))
    native._check(rc)


def test_launch_accounting(native):
    ix = _index(native, 64, L2)
    ids = _ids(9, 600)
    ix.profile(True)
    try:
        for route, path in ROUTES:
            _set_route(ix, route)
            ix.profile_read()
            ix.search_matrix(ids, 10)
            read = ix.profile_read()
            assert read["scan_launches"] == 3, (path, read)                      # one scoring launch per round
            assert read["merge_launches"] == (600 if path == SELECT else 3), (path, read)  # one ranking launch per round / anchor
    finally:
        ix.profile(False)
        _set_route(ix, ROUTES[0][0])


def test_the_call_s_buffers_are_counted(native):
    d, n, k = 64, 257, 10
    rows = np.random.default_rng(3).standard_normal((1000, d)).astype(np.float32)
    with native.NativeIndex(d, COS, 0, capacity_rows=1000) as ix:
        ix.add(rows, normalize=True)
        before = ix.get_option("device_bytes_resident")
        ix.search_matrix(np.arange(0, 2 * n, 2, dtype=np.uint64), k)
        assert ix.get_option("last_matrix_path") == KEYS
        after = ix.get_option("device_bytes_resident")
        # the list, a round's keys (256 anchors x 257 listed rows) and the results
        need = 4 * n + 8 * 256 * n + n * k * (8 + 4)
        print(f"device_bytes_resident {before} -> {after} (+{after - before}); list + keys + results = {need}")
        assert after - before >= need
        again = ix.get_option("device_bytes_resident")
        ix.search_matrix(np.arange(0, 2 * n, 2, dtype=np.uint64), k)
        assert ix.get_option("device_bytes_resident") == again  # kept and reused
