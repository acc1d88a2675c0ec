"""Multi-vector search on the MI355X (wdbx_index_search_multivector and its public forms): the labels ranked by the sum over a
query's vectors of each vector's best score among the label's rows.  1. integer corpora, where every fp32 score and sum is
exact: ids, scores and labels equal a numpy reference with ``==`` at every round size and on every ranking route; 2. float
corpora: bit identity with a fold of the handle's own range-search scores; 3. masks, removed rows, NaN and inf; 4. the label
order's life cycle, refusals and the empty index; 5. the one-shard facade and the REST field."""
import asyncio
import ctypes

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
NONE = 0xFFFFFFFF
N_INT = 5000
COUNTS = (1, 7, 8, 9, 33)           # vectors of the queries of one call, mixed
KS = (1, 10, 64, 65, 129, 200, 2048)
ROUND_OPTIONS = (256, 8, 3, 1)


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


# ---- the reference -----------------------------------------------------------------------------------------------------------
def _label_order(labels):
    """labels: uint32 per row (NONE = a label of its own) -> (dense label position of each row, smallest row of each label,
    stored label of each label), the labels in the label order: stored value ascending, then the NONE rows by row number"""
    n = len(labels)
    key = (labels.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    order = np.argsort(key, kind="stable")
    lab = labels[order]
    new = np.ones(n, bool)
    new[1:] = (lab[1:] != lab[:-1]) | (lab[1:] == NONE)
    dense = np.empty(n, np.int64)
    dense[order] = np.cumsum(new) - 1
    return dense, order[new].astype(np.int64), lab[new].astype(np.uint32)


def _maxima(score, dense, n_labels, eligible=None):
    """score [T, n] in the ranking domain (bigger = better; L2: the negated distance) -> (m [T, n_labels] the best score of each
    vector among each label's eligible rows, has [T, n_labels] whether there is one); a NaN score is never eligible"""
    m = np.full((len(score), n_labels), -np.inf, score.dtype)
    has = np.zeros((len(score), n_labels), bool)
    for t in range(len(score)):
        e = ~np.isnan(score[t])
        if eligible is not None:
            e &= eligible if eligible.ndim == 1 else eligible[t]
        np.maximum.at(m[t], dense[e], score[t][e])
        has[t, dense[e]] = True
    return m, has


def _ranked(m, has, lo, hi):
    """one query (vectors lo .. hi - 1): the label positions in (sum descending, position ascending) and every label's sum, the
    left fold in m's dtype from +0.0; a label without an eligible row for some vector, or with a NaN sum, is left out"""
    total = np.zeros(m.shape[1], m.dtype)
    with np.errstate(invalid="ignore"):
        for t in range(lo, hi):
            total = total + m[t]
    alive = np.nonzero(has[lo:hi].all(axis=0) & ~np.isnan(total))[0]
    return alive[np.lexsort((alive, -total[alive]))], total


def _expected(order, total, row0, lab, k, metric):
    top = order[:k]
    e_idx = np.full(k, -1, np.int64)
    e_score = np.zeros(k, np.float32)
    e_label = np.full(k, NONE, np.uint32)
    e_idx[: len(top)] = row0[top]
    e_score[: len(top)] = (total[top] if metric == COS else -total[top]) + 0.0
    e_label[: len(top)] = lab[top]
    return e_idx, e_score, e_label


def _expected_call(m, has, offsets, row0, lab, k, metric):
    want = [_expected(*_ranked(m, has, int(offsets[q]), int(offsets[q + 1])), row0, lab, k, metric) for q in range(len(offsets) - 1)]
    return tuple(np.stack([w[i] for w in want]) for i in range(3))


def _planned_rounds(total, option):
    """host_multivector.h on a small corpus (the scratch never binds): rounds of at most `option` vectors, whole blocks of 8
    while more vectors follow"""
    rounds, left = 0, total
    while left:
        take = min(left, option)
        if take < left and take >= 8:
            take = take // 8 * 8
        left -= take
        rounds += 1
    return rounds


def _domain(queries, rows, metric):
    """float64 scores [T, n] in the ranking domain, exact for small integers"""
    q, r = queries.astype(np.float64), rows.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if metric == COS:
            return q @ r.T
        return -np.stack([((v[None, :] - r) ** 2).sum(axis=1) for v in q])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _search(ix, vectors, offsets, k, option=256, mask_words=None):
    ix.set_option("multivector_round_vectors", option)
    out = ix.search_multivector(vectors, offsets, k, mask_words=mask_words)
    ix.set_option("multivector_round_vectors", 256)
    return out


# ---- 1. exact ids on exact arithmetic ----------------------------------------------------------------------------------------
def _layouts(n):
    rng = np.random.default_rng(11)
    consecutive = (np.arange(n) // 10).astype(np.uint32)          # 10 consecutive rows per label
    scattered = consecutive[rng.permutation(n)]                   # the same labels at random
    big = (np.arange(n) + 100).astype(np.uint32)                  # one label of 4000 rows among singletons ...
    big[rng.choice(n, 4000, replace=False)] = 4_000_000_000
    big[rng.choice(n, 50, replace=False)] = NONE                  # ... and some rows that are labels of their own
    return {"consecutive": consecutive, "scattered": scattered, "big": big}


OFFSETS = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.uint64)
_INT = {}


def _int_case(native, d, metric):
    """5 000 rows and 58 query vectors with integer elements in {-2 .. 2} (d = 3: 125 distinct rows, so hundreds tie exactly),
    the index that holds them un-normalised and the exact score of every (vector, row), computed once."""
    key = (d, metric)
    if key not in _INT:
        rng = np.random.default_rng(3000 + 10 * d + metric)
        rows = rng.integers(-2, 3, size=(N_INT, d))
        vectors = rng.integers(-2, 3, size=(int(OFFSETS[-1]), d))
        ix = native.NativeIndex(d, metric, 0, capacity_rows=N_INT)
        ix.add(rows.astype(np.float32), normalize=False)
        score = _domain(vectors, rows, metric)
        assert np.abs(score).max() * max(COUNTS) < 2 ** 24  # every fp32 score and sum is exact
        _INT[key] = (ix, vectors.astype(np.float32), score, rows)
    return _INT[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for case in _INT.values():
        case[0].close()
    _INT.clear()


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [3, 384, 520, 1100])  # d = 3: exact ties; 384 / 520 / 1100: the three pitch classes
def test_integer_corpora_equal_the_reference_at_every_round_size(native, d, metric):
    ix, vectors, score, _ = _int_case(native, d, metric)
    total = int(OFFSETS[-1])
    for name, labels in _layouts(N_INT).items():
        ix.set_labels(0, labels)
        dense, row0, lab = _label_order(labels)
        n_labels = len(row0)
        m, has = _maxima(score, dense, n_labels)
        for k in KS:
            e_idx, e_score, e_label = _expected_call(m, has, OFFSETS, row0, lab, k, metric)
            if k > n_labels:  # k above the label count: -1 / 0 / NONE slots
                assert (e_idx[:, n_labels:] == -1).all() and (e_idx[:, :n_labels] >= 0).all()
            for option in ROUND_OPTIONS:
                idx, sc, lb = _search(ix, vectors, OFFSETS, k, option)
                what = (name, k, option)
                assert np.array_equal(idx, e_idx), what
                assert np.array_equal(sc, e_score), what
                assert np.array_equal(lb, e_label), what
                assert ix.get_option("last_multivector_rounds") == _planned_rounds(total, option), what
                assert ix.get_option("last_multivector_vectors") == total, what
                assert ix.get_option("last_multivector_labels") == n_labels, what


def test_radix_select_route_at_small_k_and_scan_launch_count(native):
    ix, vectors, score, _ = _int_case(native, 384, COS)
    labels = _layouts(N_INT)["scattered"]
    ix.set_labels(0, labels)
    dense, row0, lab = _label_order(labels)
    m, has = _maxima(score, dense, len(row0))
    e_idx, e_score, e_label = _expected_call(m, has, OFFSETS, row0, lab, 10, COS)
    ix.set_option("select_min_k", 5)  # k = 10 goes down the radix-select route: a key per label
    try:
        for option in ROUND_OPTIONS:
            idx, sc, lb = _search(ix, vectors, OFFSETS, 10, option)
            assert np.array_equal(idx, e_idx) and np.array_equal(sc, e_score) and np.array_equal(lb, e_label), option
    finally:
        ix.set_option("select_min_k", 200)
    # the lists in LDS instead of registers (option lds_lists): the same answer
    ix.set_option("lds_lists", 1)
    try:
        idx, sc, lb = _search(ix, vectors, OFFSETS, 10, 8)
        assert np.array_equal(idx, e_idx) and np.array_equal(sc, e_score) and np.array_equal(lb, e_label)
    finally:
        ix.set_option("lds_lists", 0)
    # the scoring launches count as scan launches: one per round
    ix.profile(True)
    ix.profile_read()
    _search(ix, vectors, OFFSETS, 10, 8)
    prof = ix.profile_read()
    ix.profile(False)
    assert prof["scan_launches"] == _planned_rounds(int(OFFSETS[-1]), 8) == 8 and prof["merge_launches"] >= 8
    # the option's range
    for bad in (0, 257, -1):
        with pytest.raises(native.HipBackendError):
            ix.set_option("multivector_round_vectors", bad)
    assert ix.get_option("multivector_round_vectors") == 256


# (name, select_min_k, lds_lists): lists in registers up to k = 128 and in LDS above, the LDS lists whatever k is, the select chain
ROUTES = [("lists", 200, 0), ("lds_lists", 200, 1), ("select", 1, 0)]


def _planned_ranked(offsets, option):
    """host_multivector.h on a small corpus: per round, how many queries END in it (those are ranked there)"""
    total, ends = int(offsets[-1]), [int(o) for o in offsets[1:]]
    out, first = [], 0
    while first < total:
        take = min(total - first, option)
        if take < total - first and take >= 8:
            take = take // 8 * 8
        out.append(sum(first < e <= first + take for e in ends))
        first += take
    return out


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [20, 100])
def test_ranking_routes_and_their_launch_counts(native, d, metric):
    """per round: the scoring launch (a scan launch) and the reduce-and-rank bracket; a round that ends queries then ranks them
    with one merge launch over their partial lists or, on the select route, one select-and-sort bracket per query.  Rounds of
    3 vectors: queries that span rounds, rounds that rank none, one or two queries, and results written from a later query on."""
    n = 2500
    rng = np.random.default_rng(6000 + 10 * d + metric)
    rows = rng.integers(-2, 3, size=(n, d))
    labels = (np.arange(n) // 10).astype(np.uint32)[rng.permutation(n)]
    dense, row0, lab = _label_order(labels)
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.add(rows.astype(np.float32), normalize=False)
        ix.set_labels(0, labels)
        ix.profile(True)
        try:
            for counts in ((3,), (1, 3, 2, 4, 2)):
                offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
                vectors = rng.integers(-2, 3, size=(int(offsets[-1]), d))
                m, has = _maxima(_domain(vectors, rows, metric), dense, len(row0))
                for k in (1, 10, 129):
                    want = _expected_call(m, has, offsets, row0, lab, k, metric)
                    for name, select_min_k, lds_lists in ROUTES:
                        ix.set_option("select_min_k", select_min_k)
                        ix.set_option("lds_lists", lds_lists)
                        for option in (256, 3):
                            ranked = _planned_ranked(offsets, option)
                            ix.profile_read()
                            got = _search(ix, vectors.astype(np.float32), offsets, k, option)
                            prof = ix.profile_read()
                            what = (name, counts, k, option, ranked, prof)
                            for g, w in zip(got, want):
                                assert np.array_equal(g, w), what
                            assert ix.get_option("last_multivector_rounds") == len(ranked), what
                            assert prof["scan_launches"] == len(ranked), what
                            tails = sum(ranked) if name == "select" else sum(r > 0 for r in ranked)
                            assert prof["merge_launches"] == len(ranked) + tails, what
        finally:
            ix.profile(False)
            ix.set_option("select_min_k", 200)
            ix.set_option("lds_lists", 0)


def test_a_handle_without_labels_ranks_every_row_by_its_sum(native):
    _, vectors, score, rows = _int_case(native, 3, COS)
    with native.NativeIndex(3, COS, 0, capacity_rows=N_INT) as plain:
        plain.add(rows.astype(np.float32), normalize=False)
        labels = np.full(N_INT, NONE, np.uint32)
        dense, row0, lab = _label_order(labels)
        assert np.array_equal(row0, np.arange(N_INT))
        m, has = _maxima(score, dense, N_INT)
        for k in (10, 300):
            e_idx, e_score, e_label = _expected_call(m, has, OFFSETS, row0, lab, k, COS)
            idx, sc, lb = _search(plain, vectors, OFFSETS, k, 8)
            assert np.array_equal(idx, e_idx) and np.array_equal(sc, e_score) and (lb == NONE).all(), k


# ---- 2. float corpora: bit identity with a fold of the handle's own range-search scores --------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
def test_float_corpus_is_the_fold_of_range_search_scores_bit_for_bit(native, metric):
    n, d = 4096, 384
    counts = (1, 8, 9, 33)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    rows = O.normalize_rows_fast(O.synth_rows(O.SEED_CORPUS, 0, n, d))
    vectors = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, int(offsets[-1]), d))
    labels = _layouts(n)["scattered"]
    dense, row0, lab = _label_order(labels)
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.add(rows, normalize=False)
        ix.set_labels(0, labels)
        r_off, r_rows, r_scores = ix.range_search(vectors, np.inf if metric == L2 else -np.inf)
        score = np.empty((len(vectors), n), np.float32)
        for t in range(len(vectors)):
            lo, hi = int(r_off[t]), int(r_off[t + 1])
            assert hi - lo == n
            score[t, r_rows[lo:hi]] = r_scores[lo:hi] if metric == COS else -r_scores[lo:hi]
        m, has = _maxima(score, dense, len(row0))
        assert m.dtype == np.float32
        for q in range(len(counts)):  # the sums are distinct for this seed: the ids are decided
            order, total = _ranked(m, has, int(offsets[q]), int(offsets[q + 1]))
            assert total.dtype == np.float32 and len(np.unique(total[order])) == len(order) == len(row0)
        for k in (10, 200):
            e_idx, e_score, e_label = _expected_call(m, has, offsets, row0, lab, k, metric)
            for option in (256, 8, 3):
                idx, sc, lb = _search(ix, vectors, offsets, k, option)
                assert np.array_equal(_bits(sc), _bits(e_score)), (k, option)
                assert np.array_equal(idx, e_idx) and np.array_equal(lb, e_label), (k, option)


# ---- 3. masks, removed rows, NaN and inf ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
def test_masks_dead_rows_nan_and_inf(native, metric):
    n, d = 700, 24
    rng = np.random.default_rng(17 + metric)
    rows = rng.integers(-2, 3, size=(n, d)).astype(np.float64)
    vectors = rng.integers(-2, 3, size=(12, d)).astype(np.float64)
    offsets = np.array([0, 3, 12], np.uint64)
    labels = (rng.permutation(n) // 7).astype(np.uint32)
    dense, row0, lab = _label_order(labels)
    n_labels = len(row0)
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.add(rows.astype(np.float32), normalize=False)
        ix.set_labels(0, labels)

        def check(vecs, offs, stored, eligible, words, what, k=10):
            m, has = _maxima(_domain(vecs, stored, metric), dense, n_labels, eligible)
            e = _expected_call(m, has, offs, row0, lab, k, metric)
            for option in (256, 3):
                got = _search(ix, vecs.astype(np.float32), offs, k, option, mask_words=words)
                for g, w in zip(got, e):
                    assert np.array_equal(g, w), (what, option)
            return got, (m, has)

        (idx0, _, lab0), (m0, _) = check(vectors, offsets, rows, None, None, "plain")
        top_label = int(lab0[0][0])
        members = np.nonzero(labels == top_label)[0]
        # a mask that removes a label's best row for the first vector changes that maximum
        score = _domain(vectors, rows, metric)
        best = int(members[np.argmax(score[0][members])])
        allowed = np.ones(n, bool)
        allowed[best] = False
        allowed[members[score[0][members] == score[0][best]]] = False  # (and the rows that tie with it)
        _, (m1, _) = check(vectors, offsets, rows, allowed, native.pack_row_mask(allowed), "best rows masked", k=100)
        pos = int(np.nonzero(lab == top_label)[0][0])
        assert m1[0][pos] < m0[0][pos]
        # a mask that removes every row of a label removes the label
        allowed = labels != top_label
        (idx, _, lb), _ = check(vectors, offsets, rows, allowed, native.pack_row_mask(allowed), "label masked", k=100)
        assert not (lb == top_label).any() and (idx[:, 99] == -1).all() and (idx[:, 98] >= 0).all()
        # a short mask is refused and the handle stays usable
        with pytest.raises(native.HipBackendError):
            ix.search_multivector(vectors.astype(np.float32), offsets, 10, mask_words=native.pack_row_mask(allowed)[:-1])
        check(vectors, offsets, rows, None, None, "after the refusal")
        # a removed row (NaN row) and a row with a NaN element are never eligible
        stored = rows.copy()
        second = int(members[members != best][0])
        stored[best] = np.nan
        stored[second, 3] = np.nan
        ix.set_rows(best, stored[best][None, :].astype(np.float32))
        ix.set_rows(second, stored[second][None, :].astype(np.float32))
        (idx, _, _), _ = check(vectors, offsets, stored, None, None, "dead rows", k=100)
        both = labels != int(lab0[0][1])
        check(vectors, offsets, stored, both, native.pack_row_mask(both), "dead rows and a mask")
        # a query vector containing NaN: every slot of THAT query is -1, the other query is untouched
        holed = vectors.copy()
        holed[1, 5] = np.nan
        (idx, sc, lb), _ = check(holed, offsets, stored, None, None, "NaN in a query vector")
        assert (idx[0] == -1).all() and (sc[0] == 0).all() and (lb[0] == NONE).all() and (idx[1] >= 0).all()
        if metric == COS:
            # inf rows: a label of ONE row that is all +inf scores +inf against an all-positive vector and -inf against an
            # all-negative one: the sum is NaN and the label is not returned; a label with other rows keeps a finite maximum
            # for the negative vector and comes first with +inf
            lone = (rng.permutation(n) // 7).astype(np.uint32)
            single = int(np.nonzero(np.isfinite(stored).all(axis=1))[0][0])
            lone[single] = 4_000_000_000
            ix.set_labels(0, lone)
            dense, row0, lab = _label_order(lone)
            n_labels = len(row0)
            shared = int(np.nonzero((lone == lone[(single + 1) % n]) & np.isfinite(stored).all(axis=1))[0][0])
            assert shared != single and (lone == lone[shared]).sum() > 1
            stored[single] = np.inf
            stored[shared] = np.inf
            ix.set_rows(single, stored[single][None, :].astype(np.float32))
            ix.set_rows(shared, stored[shared][None, :].astype(np.float32))
            ones = np.ones((1, d))
            vecs = np.concatenate([ones, -ones, ones, ones, vectors[:2]])
            offs = np.array([0, 2, 4, 6], np.uint64)
            (idx, sc, lb), _ = check(vecs, offs, stored, None, None, "inf rows", k=n_labels)
            assert single not in idx[0] and idx[0][0] == row0[dense[shared]] and np.isposinf(sc[0][0])
            assert single in idx[1][:2] and np.isposinf(sc[1][:2]).all()
            assert single not in idx[2]  # (0 * inf: its scores against the random vectors are NaN)
            assert (idx[0] >= 0).sum() == n_labels - 1


# ---- 4. life cycle, refusals, the empty index ----------------------------------------------------------------------------------
def test_label_order_follows_relabelling_add_compact_and_clear(native):
    n, d = 900, 24
    rng = np.random.default_rng(3)
    rows = rng.integers(-2, 3, size=(n + 50, d)).astype(np.float64)
    vectors = rng.integers(-2, 3, size=(11, d)).astype(np.float64)
    offsets = np.array([0, 2, 11], np.uint64)
    labels = rng.integers(0, 60, size=n).astype(np.uint32)
    with native.NativeIndex(d, COS, 0, capacity_rows=n) as ix:
        def check(stored, cur_labels, what, k=10):
            dense, row0, lab = _label_order(cur_labels)
            m, has = _maxima(_domain(vectors, stored, COS), dense, len(row0))
            e = _expected_call(m, has, offsets, row0, lab, k, COS)
            got = _search(ix, vectors.astype(np.float32), offsets, k, 8)
            for g, w in zip(got, e):
                assert np.array_equal(g, w), what
            assert ix.get_option("last_multivector_labels") == len(row0), what
            return got

        # an empty index: every slot -1, nothing launched
        idx, sc, lb = _search(ix, vectors.astype(np.float32), offsets, 5)
        assert (idx == -1).all() and (sc == 0).all() and (lb == NONE).all()
        assert [ix.get_option("last_multivector_" + x) for x in ("rounds", "vectors", "labels")] == [0, 0, 0]
        ix.add(rows[:n].astype(np.float32), normalize=False)
        check(rows[:n], np.full(n, NONE, np.uint32), "no labels")
        ix.set_labels(100, labels[100:400])  # a prefix-free range: the rest stay NONE
        part = np.full(n, NONE, np.uint32)
        part[100:400] = labels[100:400]
        check(rows[:n], part, "partly labelled")
        ix.set_labels(0, labels)
        first = check(rows[:n], labels, "labelled", k=70)
        assert (first[0][:, 60:] == -1).all() and (first[0][:, :60] >= 0).all()
        relabelled = ((labels + 1) % 7).astype(np.uint32)
        ix.set_labels(0, relabelled)
        check(rows[:n], relabelled, "relabelled")
        ix.set_labels(0, labels)
        ix.add(rows[n:].astype(np.float32), normalize=False)  # new rows are labels of their own
        check(rows, np.concatenate([labels, np.full(50, NONE, np.uint32)]), "grown", k=200)
        keep = np.sort(rng.choice(n, 600, replace=False))
        ix.compact(keep)
        check(rows[keep], labels[keep], "compacted")
        # a distinct search between two calls shares the label order and leaves the answer alone
        ix.set_option("distinct_overfetch", 0)
        ix.search_distinct(vectors[:3].astype(np.float32), 10)
        ix.set_option("distinct_overfetch", 4)
        check(rows[keep], labels[keep], "after a distinct search")
        ix.clear()
        ix.add(rows[:n].astype(np.float32), normalize=False)
        check(rows[:n], np.full(n, NONE, np.uint32), "cleared")
        assert ix.get_option("device_bytes_resident") > 0


def test_refusals_leave_the_handle_usable(native):
    n, d = 300, 8
    rng = np.random.default_rng(5)
    rows = rng.integers(-2, 3, size=(n, d)).astype(np.float64)
    vectors = rng.integers(-2, 3, size=(1030, d)).astype(np.float32)
    labels = (np.arange(n) // 3).astype(np.uint32)
    dense, row0, lab = _label_order(labels)
    with native.NativeIndex(d, COS, 0, capacity_rows=n) as ix:
        ix.add(rows.astype(np.float32), normalize=False)
        ix.set_labels(0, labels)
        good = np.array([0, 4, 5], np.uint64)
        m, has = _maxima(_domain(vectors[:5], rows, COS), dense, len(row0))
        want = _expected_call(m, has, good, row0, lab, 10, COS)

        def usable(what):
            got = ix.search_multivector(vectors[:5], good, 10)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), what

        usable("first")
        refused = [("nq < 1", vectors[:0], [0], 10, None),
                   ("k = 0", vectors[:5], good, 0, None),
                   ("k above the maximum", vectors[:5], good, native.MAX_K + 1, None),
                   ("offsets[0] != 0", vectors[:5], [1, 5], 10, None),
                   ("a query with no vector", vectors[:5], [0, 5, 5], 10, None),
                   ("decreasing offsets", vectors[:5], [0, 6, 5], 10, None),
                   ("more than 1024 vectors", vectors[:1030], [0, 1025, 1030], 10, None),
                   ("a short mask", vectors[:5], good, 10, native.pack_row_mask(np.ones(n, bool))[:-1])]
        for what, vecs, offs, k, words in refused:
            with pytest.raises(native.HipBackendError):
                ix.search_multivector(vecs, offs, k, mask_words=words)
            usable(what)
        # 1024 vectors are allowed
        idx, _, _ = ix.search_multivector(vectors[:1030], [0, 1024, 1030], 3)
        assert (idx >= 0).all()
        # null buffers, straight through the C ABI
        f32p, u64p, i64p, u32p = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32))
        v = np.ascontiguousarray(vectors[:5])
        o = np.ascontiguousarray(good)
        oi, osc = np.empty((2, 10), np.int64), np.empty((2, 10), np.float32)
        args = [v.ctypes.data_as(f32p), o.ctypes.data_as(u64p), 2, 10, 0, None, 0, oi.ctypes.data_as(i64p), osc.ctypes.data_as(f32p), None]
        lib = native.load_library()
        assert lib.wdbx_index_search_multivector(ix._h, *args) == 0      # out_label may be null
        assert np.array_equal(oi, want[0]) and np.array_equal(osc, want[1])
        for slot in (0, 1, 7, 8):
            bad = list(args)
            bad[slot] = None
            assert lib.wdbx_index_search_multivector(ix._h, *bad) != 0, slot
            usable(f"null argument {slot}")


# ---- 5. the facade -------------------------------------------------------------------------------------------------------------
def test_facade_over_one_shard_and_rest_field(tmp_path):
    from wdbx_amd import WDBX, api

    d, n, nv = 16, 2000, 5  # (one shard below MAX_K rows: vector_search(limit=n) returns every row)
    raw = O.synth_rows(O.SEED_CORPUS, 0, n, d)
    rng = np.random.default_rng(9)
    doc = rng.integers(0, 200, size=n)
    meta = {f"row_{i}": ({"doc": f"doc{doc[i]}", "lang": "en" if i % 3 else "de"} if i % 50 else {"lang": "en"}) for i in range(n)}
    w = WDBX(vector_dimension=d, num_shards=1, data_dir=str(tmp_path / "multivector"), enable_plugins=False,
             config={"DISTINCT_KEY": "doc"})
    w.vector_store.bulk_store(raw, metadata=meta)
    qs = O.synth_rows(O.SEED_QUERY, 0, nv, d)

    # every row's score for every vector through an exhaustive vector_search, maxima and sums in Python
    per_vector = [{vid: s for vid, s, _ in w.vector_search(q.tolist(), limit=n)} for q in qs]
    assert all(len(p) == n for p in per_vector)

    def brute(limit, flt=None, threshold=0.0):
        docs = {}
        for i in range(n):
            vid = f"row_{i}"
            docs.setdefault(meta[vid].get("doc", vid), []).append(vid)
        out = []
        for members in docs.values():
            live = [v for v in members if not flt or all(meta[v].get(k) == x for k, x in flt.items())]
            if live:
                out.append((-sum(max(p[v] for v in live) for p in per_vector), int(members[0][4:]), members[0]))
        return [(vid, -neg) for neg, _, vid in sorted(out) if not (threshold > 0 and -neg < threshold)][:limit]

    def same(got, want):
        assert [g[0] for g in got] == [x[0] for x in want]
        np.testing.assert_allclose([g[1] for g in got], [x[1] for x in want], atol=2e-5 * nv, rtol=0)
        assert all(g[2] == meta[g[0]] for g in got)

    got = w.vector_search_multivector(qs.tolist(), limit=10)
    same(got, brute(10))
    same(w.vector_search_multivector(qs.tolist(), limit=300), brute(300))  # every document and every unlabelled row: 200 + 40
    assert len(brute(300)) == 240
    assert got[4][1] - got[5][1] > 1e-3 and got[5][1] > 0
    t = (got[4][1] + got[5][1]) / 2
    cut = w.vector_search_multivector(qs.tolist(), limit=10, threshold=t)
    same(cut, brute(10, threshold=t))
    assert len(cut) == 5
    flt = {"lang": "de"}
    same(w.vector_search_multivector(qs.tolist(), limit=10, filter_metadata=flt), brute(10, flt=flt))
    same(asyncio.run(w.vector_search_multivector_async(qs.tolist(), limit=10)), brute(10))
    rest = asyncio.run(api.search_endpoint(w, {"query_vectors": qs.tolist(), "limit": 10, "filter_metadata": flt}))["results"]
    assert [r["vector_id"] for r in rest] == [x[0] for x in brute(10, flt=flt)]
    with pytest.raises(ValueError):
        asyncio.run(api.search_endpoint(w, {"query_vectors": qs.tolist(), "query_vector": qs[0].tolist()}))
    asyncio.run(w.shutdown())
