"""Search groups on the MI355X through the C ABI (wdbx_index_search_groups / wdbx_index_search_group_members): the k best labels as
the distinct search ranks them, each with its best group_size rows.

The statement checked everywhere: with D = wdbx_index_search_distinct(same queries, k, mask, options), out_label equals D's, and
every slot's members and score BITS equal wdbx_index_search_rows(query, the rows of D's label that the mask allows -- taken from
the labels in numpy --, group_size); out_count = min(group_size, eligible rows), counted in numpy.  The corpora are integer
({-2 .. 2}, un-normalised): every fp32 score is exact, so the within-an-ulp exception of the header cannot apply and member 0 is
D's row.  3 000 rows at d = 48 (one load per lane) and d = 384 (two); both metrics."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
NONE = 0xFFFFFFFF
N = 3000
NQ = 9
DIMS = (48, 384)


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


_CASES = {}


def _case(native, d, metric):
    key = (d, metric)
    if key not in _CASES:
        rng = np.random.default_rng(900 + 10 * d + metric)
        rows = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
        queries = rng.integers(-2, 3, size=(NQ, d)).astype(np.float32)
        ix = native.NativeIndex(d, metric, 0, capacity_rows=N + 64)
        ix.add(rows, normalize=False)
        _CASES[key] = (ix, rows, queries)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for case in _CASES.values():
        case[0].close()
    _CASES.clear()


def _layouts():
    rng = np.random.default_rng(5)
    per_row = rng.permutation(N).astype(np.uint32) * 7 + 3                      # a label per row, sparse values
    runs = np.repeat(np.arange(N), rng.integers(1, 8, size=N))[:N].astype(np.uint32)[rng.permutation(N)]  # runs of 1 .. 7, scattered
    half = (np.arange(N) + 10).astype(np.uint32)
    half[rng.choice(N, N // 2, replace=False)] = 4_000_000_000                  # one label holds half the corpus
    mixed = runs.copy()
    mixed[rng.choice(N, 400, replace=False)] = NONE                             # NONE rows mixed in
    return {"per_row": per_row, "runs": runs, "half": half, "mixed": mixed}


LAYOUTS = _layouts()


def _words(native, allow):
    return None if allow is None else native.pack_row_mask(allow)


def _check_groups(native, ix, queries, labels, k, g, allow=None, live=None, n=N):
    """the module docstring's statement; returns the groups call's four arrays"""
    words = _words(native, allow)
    d_idx, d_sc, d_lab = ix.search_distinct(queries, k, mask_words=words)
    idx, sc, lab, cnt = ix.search_groups(queries, k, g, mask_words=words)
    assert ix.get_option("last_groups_path") == 1
    assert np.array_equal(lab, d_lab)
    eligible = np.ones(n, bool) if allow is None else np.asarray(allow[:n], bool).copy()
    if live is not None:
        eligible &= live
    full = np.full(n, NONE, np.uint32)
    full[:min(len(labels), n)] = labels[:n]
    for q in range(len(queries)):
        for s in range(k):
            what = (q, s, k, g)
            if d_idx[q, s] < 0:
                assert np.all(idx[q, s] == -1) and not sc[q, s].view(np.uint32).any() and cnt[q, s] == 0 and lab[q, s] == NONE, what
                continue
            rows = np.array([d_idx[q, s]]) if d_lab[q, s] == NONE else np.nonzero((full == d_lab[q, s]) & eligible)[0]
            r_idx, r_sc = ix.search_rows(queries[q:q + 1], g, rows)
            assert np.array_equal(idx[q, s], r_idx[0]), what
            assert np.array_equal(sc[q, s].view(np.uint32), r_sc[0].view(np.uint32)), what
            assert cnt[q, s] == min(g, len(rows)) == int((idx[q, s] >= 0).sum()), what
            assert idx[q, s, 0] == d_idx[q, s] and sc[q, s, 0] == d_sc[q, s], what
            assert not (sc[q, s].view(np.uint32) == 0x80000000).any(), what  # (- 0 comes back as + 0)
    return idx, sc, lab, cnt


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_members_equal_search_rows_over_the_distinct_labels(native, layout, d, metric):
    ix, rows, queries = _case(native, d, metric)
    ix.set_labels(0, LAYOUTS[layout])
    for nq, k, g in ((1, 10, 3), (7, 4, 1), (9, 3, 64)):
        _check_groups(native, ix, queries[:nq], LAYOUTS[layout], k, g)


@pytest.mark.parametrize("metric", [COS, L2])
def test_a_handle_without_labels_gives_every_row_its_own_group(native, metric):
    ix, rows, queries = _case(native, 48, metric)
    ix.set_labels(0, np.full(N, NONE, np.uint32))
    idx, sc, lab, cnt = _check_groups(native, ix, queries[:7], np.full(N, NONE, np.uint32), 10, 3)
    assert np.all(cnt == 1) and np.all(idx[:, :, 1:] == -1) and np.all(lab == NONE)
    fresh = native.NativeIndex(48, metric, 0, capacity_rows=N)  # no label was ever set
    try:
        fresh.add(rows, normalize=False)
        f = fresh.search_groups(queries[:7], 10, 3)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(f, (idx, sc, lab, cnt)))
        assert fresh.get_option("last_groups_tasks") == 70 and fresh.get_option("last_groups_rounds") == 1
    finally:
        fresh.close()


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", DIMS)
def test_answers_do_not_depend_on_segments_or_distinct_routes(native, d, metric):
    ix, rows, queries = _case(native, d, metric)
    ix.set_labels(0, LAYOUTS["half"])
    base, tasks = None, {}
    try:
        for seg in (4, 64, 2048):
            for overfetch in (0, 4):
                ix.set_option("groups_segment_rows", seg)
                ix.set_option("distinct_overfetch", overfetch)
                out = _check_groups(native, ix, queries, LAYOUTS["half"], 5, 7) if base is None else ix.search_groups(queries, 5, 7)
                assert ix.get_option("last_distinct_path") in ((3,) if overfetch == 0 else (1, 2))
                tasks[seg] = ix.get_option("last_groups_tasks")
                again = ix.search_groups(queries, 5, 7)  # two runs give equal bytes
                for a, b, c in zip(out, again, base or out):
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8)), (seg, overfetch)
                base = base or out
    finally:
        ix.set_option("groups_segment_rows", 2048)
        ix.set_option("distinct_overfetch", 4)
    # the half-corpus label is in every query's top 5 here or not; where it is, its run of 1 500 is cut into ceil(1500 / seg) tasks
    in_top = int((base[2] == 4_000_000_000).sum())
    assert in_top >= 1
    for seg in (4, 64, 2048):
        assert tasks[seg] == NQ * 5 - in_top + in_top * -(-(N // 2) // seg), seg


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("mask", ["ones", "zeros", "alternate", "best_removed", "few"])
def test_masks(native, mask, metric):
    ix, rows, queries = _case(native, 384, metric)
    labels = LAYOUTS["mixed"]
    ix.set_labels(0, labels)
    allow = np.ones(N, bool)
    if mask == "zeros":
        allow[:] = False
    elif mask == "alternate":
        allow[::2] = False
    elif mask == "best_removed":
        allow[np.unique(ix.search_groups(queries, 10, 2)[0][:, :, 0])] = False
    elif mask == "few":
        allow[:] = False
        allow[np.random.default_rng(1).choice(N, 25, replace=False)] = True
    idx, sc, lab, cnt = _check_groups(native, ix, queries, labels, 10, 4, allow=allow)
    got = idx[idx >= 0]
    assert np.all(allow[got])
    if mask == "zeros":
        assert got.size == 0 and not cnt.any()


@pytest.mark.parametrize("metric", [COS, L2])
def test_k_above_the_label_count_and_group_size_above_the_runs(native, metric):
    ix, rows, queries = _case(native, 48, metric)
    labels = (np.arange(N) % 6).astype(np.uint32)  # six labels of 500 rows
    ix.set_labels(0, labels)
    ix.set_option("groups_segment_rows", 64)
    try:
        idx, sc, lab, cnt = _check_groups(native, ix, queries[:7], labels, 9, 64)
    finally:
        ix.set_option("groups_segment_rows", 2048)
    assert np.all(cnt[:, :6] == 64) and np.all(cnt[:, 6:] == 0) and np.all(idx[:, 6:] == -1) and np.all(lab[:, 6:] == NONE)


@pytest.mark.parametrize("metric", [COS, L2])
def test_tombstones_compact_growth_and_the_empty_index(native, metric):
    d = 48
    rng = np.random.default_rng(77 + metric)
    rows = rng.integers(-2, 3, size=(N, d)).astype(np.float32)
    queries = rng.integers(-2, 3, size=(NQ, d)).astype(np.float32)
    labels = LAYOUTS["runs"]
    ix = native.NativeIndex(d, metric, 0, capacity_rows=2 * N)
    try:
        # an empty index: every slot -1, nothing launched
        idx, sc, lab, cnt = ix.search_groups(queries, 4, 3)
        assert np.all(idx == -1) and not sc.any() and np.all(lab == NONE) and not cnt.any() and ix.get_option("last_groups_path") == 0
        ix.add(rows[:2000], normalize=False)
        ix.set_labels(0, labels[:2000])
        # rows removed as NaN tombstones
        live = np.ones(2000, bool)
        dead = np.unique(ix.search_groups(queries, 5, 2)[0][:, :, 0])
        dead = dead[dead >= 0]
        live[dead] = False
        for r in dead:
            ix.set_rows(int(r), np.full((1, d), np.nan, np.float32))
        idx = _check_groups(native, ix, queries, labels[:2000], 5, 3, live=live, n=2000)[0]
        assert not np.isin(idx[idx >= 0], dead).any()
        # set_labels on a grown index: the new rows are NONE until labelled
        ix.add(rows[2000:], normalize=False)
        live = np.concatenate([live, np.ones(N - 2000, bool)])
        _check_groups(native, ix, queries, labels[:2000], 5, 3, live=live)
        ix.set_labels(2000, labels[2000:])
        _check_groups(native, ix, queries, labels, 5, 3, live=live)
        # after compact: the labels move with their rows
        keep = np.nonzero(live)[0][::2]
        ix.compact(keep)
        assert np.array_equal(ix.get_labels(0, len(keep)), labels[keep])
        _check_groups(native, ix, queries, labels[keep], 5, 3, n=len(keep))
    finally:
        ix.close()


@pytest.mark.parametrize("metric", [COS, L2])
def test_group_members_alone(native, metric):
    ix, rows, queries = _case(native, 384, metric)
    labels = LAYOUTS["mixed"]
    ix.set_labels(0, labels)
    k, g = 6, 4
    allow = np.ones(N, bool)
    allow[::3] = False
    for words in (None, native.pack_row_mask(allow)):
        idx, sc, lab, cnt = ix.search_groups(queries, k, g, mask_words=words)
        m_idx, m_sc, m_cnt = ix.search_group_members(queries, lab, idx[:, :, 0], g, mask_words=words)
        assert np.array_equal(m_idx, idx) and np.array_equal(m_sc.view(np.uint32), sc.view(np.uint32)) and np.array_equal(m_cnt, cnt)
        assert ix.get_option("last_groups_path") == 1
    # a label not on the handle, an unlabelled slot by its row, an unused slot, a labelled slot whose row says nothing
    some_none = int(np.nonzero(labels == NONE)[0][5])
    label0 = int(labels[labels != NONE][0])
    slot_labels = np.array([[123_456_789, NONE, NONE, label0]], np.uint32)
    slot_rows = np.array([[0, some_none, -1, 0]], np.int64)
    assert not (labels == 123_456_789).any()
    m_idx, m_sc, m_cnt = ix.search_group_members(queries[:1], slot_labels, slot_rows, g)
    assert m_cnt.tolist() == [[0, 1, 0, min(g, int((labels == label0).sum()))]]
    assert np.all(m_idx[0, 0] == -1) and np.all(m_idx[0, 2] == -1) and not m_sc[0, 0].any() and not m_sc[0, 2].any()
    r_idx, r_sc = ix.search_rows(queries[:1], g, [some_none])
    assert np.array_equal(m_idx[0, 1], r_idx[0]) and np.array_equal(m_sc[0, 1].view(np.uint32), r_sc[0].view(np.uint32))
    r_idx, r_sc = ix.search_rows(queries[:1], g, np.nonzero(labels == label0)[0])
    assert np.array_equal(m_idx[0, 3], r_idx[0]) and np.array_equal(m_sc[0, 3].view(np.uint32), r_sc[0].view(np.uint32))
    # an unlabelled slot whose row the mask removes: eligibility still applies
    deny = np.ones(N, bool)
    deny[some_none] = False
    m_idx, m_sc, m_cnt = ix.search_group_members(queries[:1], slot_labels, slot_rows, g, mask_words=native.pack_row_mask(deny))
    assert m_cnt[0, 1] == 0 and np.all(m_idx[0, 1] == -1)


def test_every_refusal_leaves_the_handle_usable(native):
    ix, rows, queries = _case(native, 48, COS)
    labels = LAYOUTS["runs"]
    ix.set_labels(0, labels)
    lib, h, INVALID = ix._lib, ix._h, -1
    from wdbx_amd._native import _f32p, _i64p

    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    k, g = 4, 3
    q = np.ascontiguousarray(queries[:2])
    idx, sc = np.empty((2, k, g), np.int64), np.empty((2, k, g), np.float32)
    lab, cnt = np.empty((2, k), np.uint32), np.empty((2, k), np.int32)
    words = native.pack_row_mask(np.ones(N, bool))
    good_lab, good_row = np.full((2, k), NONE, np.uint32), np.zeros((2, k), np.int64)
    P = lambda a, t: a.ctypes.data_as(t)  # noqa: E731

    def groups(nq=2, k_=k, g_=g, qp=P(q, _f32p), mask=None, n_mask=0, oi=P(idx, _i64p), os_=P(sc, _f32p)):
        return lib.wdbx_index_search_groups(h, qp, nq, k_, g_, 0, mask, n_mask, oi, os_, P(lab, u32p), P(cnt, i32p))

    def members(nq=2, k_=k, g_=g, qp=P(q, _f32p), mask=None, n_mask=0, sl=P(good_lab, u32p), sr=P(good_row, _i64p),
                oi=P(idx, _i64p), os_=P(sc, _f32p)):
        return lib.wdbx_index_search_group_members(h, qp, nq, k_, g_, 0, mask, n_mask, sl, sr, oi, os_, P(cnt, i32p))

    def good():
        want = ix.search_groups(q, k, g)
        assert groups() == 0 and np.array_equal(idx, want[0]) and np.array_equal(cnt, want[3])
        assert members() == 0 and np.all(idx[:, :, 0] == 0) and np.all(cnt == 1)

    good()
    short = (N + 31) // 32 - 1
    bad_row = good_row.copy()
    bad_row[1, 2] = N
    for fn in (groups, members):
        for kwargs in (dict(nq=0), dict(nq=-1), dict(k_=0), dict(k_=native.MAX_K + 1), dict(g_=0), dict(g_=native.MAX_GROUP_SIZE + 1),
                       dict(qp=None), dict(oi=None), dict(os_=None), dict(mask=P(words, u32p), n_mask=short)):
            assert fn(**kwargs) == INVALID, (fn.__name__, kwargs)
            assert native.load_library().wdbx_last_error()
            good()
    for kwargs in (dict(sl=None), dict(sr=None), dict(sr=P(bad_row, _i64p))):
        assert members(**kwargs) == INVALID, kwargs
        good()
    # NULL out_label / out_count are allowed
    assert lib.wdbx_index_search_groups(h, P(q, _f32p), 2, k, g, 0, None, 0, P(idx, _i64p), P(sc, _f32p), None, None) == 0
    assert lib.wdbx_index_search_group_members(h, P(q, _f32p), 2, k, g, 0, None, 0, P(good_lab, u32p), P(good_row, _i64p),
                                               P(idx, _i64p), P(sc, _f32p), None) == 0
    # the option's range
    for value in (3, 65537, 0, -1):
        with pytest.raises(native.HipBackendError):
            ix.set_option("groups_segment_rows", value)
    assert ix.get_option("groups_segment_rows") == 2048
    for value in (4, 65536, 2048):
        ix.set_option("groups_segment_rows", value)
    good()
