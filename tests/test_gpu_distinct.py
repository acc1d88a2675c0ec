"""Distinct search on the MI355X (wdbx_index_search_distinct and its public forms): the exact top-k with at most one row per
label.  1. integer corpora, where every fp32 score is exact: ids, scores and labels equal a numpy int64 reference with ``==``
on every route; 2. float corpora: bit identity with the handle's own range search (full pass) and ordinary search (over-fetch);
3. masks, removed rows and NaN rows; 4. the labels' life cycle; 5. the facade over two shards and the REST field."""
import asyncio

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
NONE = 0xFFFFFFFF
N_INT = 5000
NQ_MAX = 33
KS = (1, 10, 64, 65, 129, 200, 2048)
NQS = (1, 7, 8, 9, 33)


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


# ---- the reference: rank, keep the first row of each label, cut ------------------------------------------------------------
def _ranking(score, metric, eligible=None):
    """rows by (score descending, row ascending); L2: (distance ascending, row ascending); only the eligible ones"""
    rows = np.arange(len(score)) if eligible is None else np.nonzero(eligible)[0]
    s = score[rows]
    return rows[np.lexsort((rows, -s if metric == COS else s))]


def _first_per_label(ranked, labels):
    lab = labels[ranked]
    keep = lab == NONE
    _, first = np.unique(lab, return_index=True)
    keep[first] = True
    return keep  # (the first NONE found by unique is kept anyway)


def _expected(ranked, score, labels, k, dtype=np.float32):
    keep = _first_per_label(ranked, labels)
    rows = ranked[keep][:k]
    e_idx = np.full(k, -1, np.int64)
    e_score = np.zeros(k, dtype)
    e_label = np.full(k, NONE, np.uint32)
    e_idx[: len(rows)] = rows
    e_score[: len(rows)] = score[rows]
    e_label[: len(rows)] = labels[rows]
    return e_idx, e_score, e_label


def _expected_path(ranked, labels, n, k, overfetch):
    """what host_labels.h decides: 3 without an over-fetch; else 1 when every query's walk over its top-k' is final"""
    if overfetch == 0:
        return 3
    kp = min(n, 2048, overfetch * k)
    for r in ranked:
        found = int(_first_per_label(r[:kp], labels).sum())
        if not (found >= k or len(r) < kp or kp >= n):
            return 2
    return 1


# ---- 1. exact ids on exact arithmetic ---------------------------------------------------------------------------------------
def _layouts(n):
    rng = np.random.default_rng(11)
    consecutive = (np.arange(n) // 10).astype(np.uint32)          # 10 consecutive rows per label
    scattered = consecutive[rng.permutation(n)]                   # the same labels at random
    big = (np.arange(n) + 100).astype(np.uint32)                  # one label of 4000 rows among singletons ...
    big[rng.choice(n, 4000, replace=False)] = 4_000_000_000
    big[rng.choice(n, 50, replace=False)] = NONE                  # ... and some rows that are labels of their own
    return {"consecutive": consecutive, "scattered": scattered, "big": big}


_INT = {}


def _int_case(native, d, metric):
    """5 000 rows and 33 queries with integer elements in {-2 .. 2} (d = 3: 125 distinct rows, so hundreds tie exactly), the
    index that holds them un-normalised, the int64 score of every (query, row) and each query's ranking, computed once."""
    key = (d, metric)
    if key not in _INT:
        rng = np.random.default_rng(2000 + 10 * d + metric)
        rows = rng.integers(-2, 3, size=(N_INT, d)).astype(np.int64)
        queries = rng.integers(-2, 3, size=(NQ_MAX, d)).astype(np.int64)
        if metric == COS:
            score = queries @ rows.T
        else:
            score = np.stack([((q[None, :] - rows) ** 2).sum(axis=1) for q in queries])
        ix = native.NativeIndex(d, metric, 0, capacity_rows=N_INT)
        ix.add(rows.astype(np.float32), normalize=False)
        ranked = [_ranking(score[q], metric) for q in range(NQ_MAX)]
        _INT[key] = (ix, queries.astype(np.float32), score, ranked)
    return _INT[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for case in _INT.values():
        case[0].close()
    _INT.clear()


def _distinct(ix, queries, k, overfetch, mask_words=None):
    ix.set_option("distinct_overfetch", overfetch)
    out = ix.search_distinct(queries, k, mask_words=mask_words)
    return out, ix.get_option("last_distinct_path")


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [3, 384, 768, 1100])  # d = 3: exact ties; 384 / 768 / 1100: the three pitch classes
def test_integer_corpora_equal_the_int64_reference_on_every_route(native, d, metric):
    ix, queries, score, ranked = _int_case(native, d, metric)
    shapes = sorted({(nq, k) for nq in (1, 9) for k in KS} | {(nq, k) for nq in NQS for k in (10, 200)})
    seen_paths = set()
    for name, labels in _layouts(N_INT).items():
        ix.set_labels(0, labels)
        n_labels = len(set(labels[labels != NONE].tolist())) + int((labels == NONE).sum())
        for nq, k in shapes:
            want = [_expected(ranked[q], score[q], labels, k) for q in range(nq)]
            e_idx, e_score, e_label = (np.stack([w[i] for w in want]) for i in range(3))
            if k > n_labels:  # k above the label count: -1 / 0 / NONE slots
                assert (e_idx[:, n_labels:] == -1).all() and (e_idx[:, :n_labels] >= 0).all()
            # the full pass alone, the default over-fetch, and an over-fetch of k' = k (short wherever a label repeats)
            for overfetch in (0, 4, 1):
                (idx, sc, lab), path = _distinct(ix, queries[:nq], k, overfetch)
                what = (name, nq, k, overfetch, path)
                assert path == _expected_path(ranked[:nq], labels, N_INT, k, overfetch), what
                assert np.array_equal(idx, e_idx), what
                assert np.array_equal(sc, e_score), what
                assert np.array_equal(lab, e_label), what
                seen_paths.add((name, overfetch, path))
                if path != 1:
                    assert ix.get_option("last_distinct_labels") == n_labels, what
                    assert n_labels <= ix.get_option("last_distinct_items") <= n_labels + -(-N_INT // 64), what
                    assert 1 <= ix.get_option("last_distinct_short") <= nq, what
                else:
                    assert ix.get_option("last_distinct_short") == 0, what
    # per layout: the full pass when asked for; the default answers small k from the over-fetch alone wherever labels are
    # many, and needs the full pass for k above the label count; the 4000-row label with k' = k falls short
    for name in ("consecutive", "scattered", "big"):
        assert (name, 0, 3) in seen_paths
    assert ("consecutive", 4, 1) in seen_paths and ("scattered", 4, 1) in seen_paths
    assert ("consecutive", 4, 2) in seen_paths and ("scattered", 4, 2) in seen_paths  # (k = 2048 > 500 labels)
    assert ("big", 1, 2) in seen_paths
    ix.set_option("distinct_overfetch", 4)


def test_full_pass_counts_its_scoring_launches_as_scan_launches(native):
    ix, queries, score, ranked = _int_case(native, 384, COS)
    ix.set_labels(0, _layouts(N_INT)["scattered"])
    ix.profile(True)
    ix.profile_read()
    _distinct(ix, queries[:9], 10, 0)
    prof = ix.profile_read()
    ix.profile(False)
    ix.set_option("distinct_overfetch", 4)
    assert prof["scan_launches"] == 1 and prof["merge_launches"] >= 2  # one round: scoring, then ranking + merge


# (name, select_min_k, lds_lists): lists in registers up to k = 128 and in LDS above, the LDS lists whatever k is, the select chain
ROUTES = [("lists", 200, 0), ("lds_lists", 200, 1), ("select", 1, 0)]


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [20, 100])
def test_full_pass_ranking_routes_and_their_launch_counts(native, d, metric):
    """2 500 rows never bind the scratch bound, so the full pass is ONE round: the scoring launch (a scan launch), the label
    ranking launch and then one merge launch over its partial lists or, on the select route, one select-and-sort bracket per
    query (all merge launches)."""
    n = 2500
    rng = np.random.default_rng(5000 + 10 * d + metric)
    rows = rng.integers(-2, 3, size=(n, d)).astype(np.int64)
    queries = rng.integers(-2, 3, size=(257, d)).astype(np.int64)
    score = queries @ rows.T if metric == COS else np.stack([((q[None, :] - rows) ** 2).sum(axis=1) for q in queries])
    labels = (np.arange(n) // 10).astype(np.uint32)[rng.permutation(n)]
    ranked = [_ranking(score[q], metric) for q in range(257)]
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.add(rows.astype(np.float32), normalize=False)
        ix.set_labels(0, labels)
        ix.profile(True)
        try:
            for name, select_min_k, lds_lists in ROUTES:
                ix.set_option("select_min_k", select_min_k)
                ix.set_option("lds_lists", lds_lists)
                for k in (1, 10, 129):
                    for nq in (1, 5):
                        want = [_expected(ranked[q], score[q], labels, k) for q in range(nq)]
                        ix.profile_read()
                        (idx, sc, lab), path = _distinct(ix, queries[:nq].astype(np.float32), k, 0)
                        prof = ix.profile_read()
                        what = (name, k, nq, path, prof)
                        assert path == 3, what
                        for i, got in enumerate((idx, sc, lab)):
                            assert np.array_equal(got, np.stack([w[i] for w in want])), what
                        assert prof["scan_launches"] == 1, what
                        assert prof["merge_launches"] == 1 + (nq if name == "select" else 1), what
                # 257 queries: a round holds at most 256, so the second round writes its one query's results from slot 256 on
                want = [_expected(ranked[q], score[q], labels, 10) for q in range(257)]
                ix.profile_read()
                (idx, sc, lab), path = _distinct(ix, queries.astype(np.float32), 10, 0)
                prof = ix.profile_read()
                what = (name, "two rounds", path, prof)
                assert path == 3, what
                for i, got in enumerate((idx, sc, lab)):
                    assert np.array_equal(got, np.stack([w[i] for w in want])), what
                assert prof["scan_launches"] == 2, what
                assert prof["merge_launches"] == 2 + (257 if name == "select" else 2), what
        finally:
            ix.profile(False)
            ix.set_option("select_min_k", 200)
            ix.set_option("lds_lists", 0)
            ix.set_option("distinct_overfetch", 4)


# ---- 2. float corpora: bit identity with the handle's other searches ---------------------------------------------------------
def _dedupe(rows, scores, labels, k):
    keep = _first_per_label(rows, labels)
    r, s = rows[keep][:k], scores[keep][:k]
    idx = np.full(k, -1, np.int64)
    sc = np.zeros(k, np.float32)
    idx[: len(r)] = r
    sc[: len(s)] = s
    return idx, sc


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("metric", [COS, L2])
def test_float_corpus_matches_range_search_and_search_bit_for_bit(native, metric):
    n, d, nq = 5000, 384, 9
    rows = O.normalize_rows_fast(O.synth_rows(O.SEED_CORPUS, 0, n, d))
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, nq, d))
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        ix.add(rows, normalize=False)
        offsets, r_rows, r_scores = ix.range_search(queries, np.inf if metric == L2 else -np.inf)
        for name, labels in _layouts(n).items():
            ix.set_labels(0, labels)
            for k in (10, 200):
                # the full pass: the range search's full ranking, deduplicated
                (idx, sc, lab), path = _distinct(ix, queries, k, 0)
                assert path == 3
                for q in range(nq):
                    lo, hi = int(offsets[q]), int(offsets[q + 1])
                    assert hi - lo == n
                    e_idx, e_sc = _dedupe(r_rows[lo:hi], r_scores[lo:hi], labels, k)
                    assert np.array_equal(idx[q], e_idx), (name, k, q)
                    assert np.array_equal(_bits(sc[q]), _bits(e_sc)), (name, k, q)
                    assert np.array_equal(lab[q][idx[q] >= 0], labels[idx[q][idx[q] >= 0]])
                # the over-fetch where it answers alone: the ordinary search at k', deduplicated
                (idx1, sc1, _), path = _distinct(ix, queries, k, 4)
                if path == 1:
                    kp = min(n, 2048, 4 * k)
                    s_idx, s_sc = ix.search(queries, kp)
                    for q in range(nq):
                        e_idx, e_sc = _dedupe(s_idx[q], s_sc[q], labels, k)
                        assert np.array_equal(idx1[q], e_idx) and np.array_equal(_bits(sc1[q]), _bits(e_sc)), (name, k, q)
            if name != "big":
                assert path == 1, name  # (k = 200 of 500 labels from the top 800 rows)


def test_over_fetch_through_the_selection_and_batched_paths(native):
    n, d, nq = 70_000, 64, 16
    rng = np.random.default_rng(5)
    labels = (rng.permutation(n) // 10).astype(np.uint32)
    with native.NativeIndex(d, COS, 0, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, nq, d))
        ix.set_labels(0, labels)
        for qs, k in ((queries, 10), (queries, 300), (queries[:1], 10), (queries[:1], 300)):
            (idx, sc, lab), path = _distinct(ix, qs, k, 4)
            assert path == 1, (len(qs), k)
            kp = min(2048, 4 * k)
            s_idx, s_sc = ix.search(qs, kp)
            for q in range(len(qs)):
                e_idx, e_sc = _dedupe(s_idx[q], s_sc[q], labels, k)
                assert np.array_equal(idx[q], e_idx) and np.array_equal(_bits(sc[q]), _bits(e_sc)), (len(qs), k, q)
                assert np.array_equal(lab[q], labels[idx[q]])
        # the full pass on this corpus: the range search's full ranking, deduplicated
        offsets, r_rows, r_scores = ix.range_search(queries[:2], -np.inf)
        (idx3, sc3, _), path = _distinct(ix, queries[:2], 300, 0)
        assert path == 3
        for q in range(2):
            e_idx, e_sc = _dedupe(r_rows[int(offsets[q]):int(offsets[q + 1])], r_scores[int(offsets[q]):int(offsets[q + 1])], labels, 300)
            assert np.array_equal(idx3[q], e_idx) and np.array_equal(_bits(sc3[q]), _bits(e_sc)), q


# ---- 3. masks, removed rows, NaN rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
def test_masks_and_dead_rows(native, metric):
    n, d = 700, 24
    rng = np.random.default_rng(17 + metric)
    rows = rng.integers(-2, 3, size=(n, d)).astype(np.int64)
    queries = rng.integers(-2, 3, size=(9, d)).astype(np.int64)
    score = queries @ rows.T if metric == COS else np.stack([((q[None, :] - rows) ** 2).sum(axis=1) for q in queries])
    labels = (rng.permutation(n) // 7).astype(np.uint32)
    q0 = _ranking(score[0], metric)
    best = int(q0[0])
    best_label = labels[best]
    with native.NativeIndex(d, metric, 0, capacity_rows=n) as ix:
        stored = rows.astype(np.float32)
        ix.add(stored, normalize=False)
        ix.set_labels(0, labels)
        qf = queries.astype(np.float32)

        def check(eligible, words, what, k=10):
            for overfetch in (0, 4, 1):
                (idx, sc, lab), _ = _distinct(ix, qf, k, overfetch, mask_words=words)
                for q in range(len(qf)):
                    e = _expected(_ranking(score[q], metric, eligible), score[q], labels, k)
                    assert np.array_equal(idx[q], e[0]) and np.array_equal(sc[q], e[1]) and np.array_equal(lab[q], e[2]), (what, overfetch, q)
            return idx, lab

        # a mask that removes a label's best row: the label appears through its next row
        allowed = np.ones(n, bool)
        allowed[best] = False
        check(allowed, native.pack_row_mask(allowed), "best row masked")
        idx, lab = check(allowed, native.pack_row_mask(allowed), "best row masked, every label", k=100)
        slot = np.nonzero(lab[0] == best_label)[0]
        assert len(slot) == 1 and idx[0][slot[0]] != best and labels[idx[0][slot[0]]] == best_label
        # a mask that removes a whole label: the label vanishes
        allowed = labels != best_label
        check(allowed, native.pack_row_mask(allowed), "label masked")
        idx, lab = check(allowed, native.pack_row_mask(allowed), "label masked, every label", k=100)
        assert not (lab == best_label).any() and (idx[:, 99] == -1).all() and (idx[:, 98] >= 0).all()
        # a short mask is refused and the handle stays usable
        with pytest.raises(native.HipBackendError):
            ix.search_distinct(qf, 10, mask_words=native.pack_row_mask(allowed)[:-1])
        check(np.ones(n, bool), None, "after the refusal")
        # removed rows (NaN rows) and rows with a NaN element never represent a label
        dead = np.ones(n, bool)
        dead[best] = False
        second = int(q0[1])
        dead[second] = False
        ix.set_rows(best, np.full((1, d), np.nan, np.float32))
        holed = stored[second].copy()
        holed[3] = np.nan
        ix.set_rows(second, holed[None, :])
        idx, lab = check(dead, None, "dead rows")
        assert best not in idx[0] and second not in idx[0]
        both = dead & (labels != labels[int(q0[2])])
        check(both, native.pack_row_mask(both), "dead rows and a mask")
        # refusals as wdbx_index_search_masked_n's
        for bad_k in (0, 2049):
            with pytest.raises(native.HipBackendError):
                ix.search_distinct(qf, bad_k)
        check(dead, None, "after the refusals")


# ---- 4. the labels' life cycle -----------------------------------------------------------------------------------------------
def test_label_lifecycle(native):
    n, d = 900, 384
    rows = O.normalize_rows_fast(O.synth_rows(O.SEED_CORPUS, 0, n, d))
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 9, d))
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 60, size=n).astype(np.uint32)
    with native.NativeIndex(d, COS, 0, capacity_rows=n) as ix:
        # an empty index: nothing launched
        (idx, sc, lab), path = _distinct(ix, queries, 5, 4)
        assert path == 0 and (idx == -1).all() and (sc == 0).all() and (lab == NONE).all()
        ix.add(rows, normalize=False)
        assert (ix.get_labels(0, n) == NONE).all()
        # a handle with no labels equals wdbx_index_search bit for bit, whatever the over-fetch says
        s_idx, s_sc = ix.search(queries, 10)
        for overfetch in (4, 0):
            (idx, sc, lab), path = _distinct(ix, queries, 10, overfetch)
            assert path == 1 and np.array_equal(idx, s_idx) and np.array_equal(_bits(sc), _bits(s_sc)) and (lab == NONE).all()
        allowed = rng.random(n) < 0.5
        words = native.pack_row_mask(allowed)
        m_idx, m_sc = ix.search(queries, 10, mask_words=words)
        (idx, sc, _), _ = _distinct(ix, queries, 10, 4, mask_words=words)
        assert np.array_equal(idx, m_idx) and np.array_equal(_bits(sc), _bits(m_sc))
        # labels set after a first distinct search take effect; get_labels round-trips; a range past the end is refused
        ix.set_labels(100, labels[100:400])
        got = ix.get_labels(0, n)
        assert np.array_equal(got[100:400], labels[100:400]) and (got[:100] == NONE).all() and (got[400:] == NONE).all()
        with pytest.raises(native.HipBackendError):
            ix.set_labels(n - 1, labels[:2])
        with pytest.raises(native.HipBackendError):
            ix.get_labels(n, 1)
        ix.set_labels(0, labels)
        assert np.array_equal(ix.get_labels(0, n), labels)

        def check(cur_labels, n_rows, what):
            for overfetch in (0, 4):
                (idx, sc, lab), _ = _distinct(ix, queries, 10, overfetch)
                for q in range(len(queries)):
                    live = idx[q][idx[q] >= 0]
                    assert len(set(lab[q][: len(live)].tolist())) == len(live), (what, q)  # one row per label
                    assert np.array_equal(lab[q][: len(live)], cur_labels[live]), (what, q)
            return idx

        first = check(labels, n, "labelled")
        assert not np.array_equal(first, s_idx)  # (60 labels over 900 rows: the plain top-10 repeats labels)
        # a second labelling replaces the first (the label order is rebuilt)
        relabelled = (labels + 1) % 7
        ix.set_labels(0, relabelled)
        again = check(relabelled, n, "relabelled")
        assert (again[:, 7:] == -1).all() and (again[:, :7] >= 0).all()  # seven labels in all
        ix.set_labels(0, labels)
        # labels survive reserve ...
        ix.reserve(4 * n)
        assert np.array_equal(ix.get_labels(0, n), labels)
        assert np.array_equal(check(labels, n, "reserved"), first)
        # ... new rows start as NONE ...
        ix.add(rows[:50], normalize=False)
        assert np.array_equal(ix.get_labels(0, n), labels) and (ix.get_labels(n, 50) == NONE).all()
        check(np.concatenate([labels, np.full(50, NONE, np.uint32)]), n + 50, "grown")
        # ... move under compact ...
        keep = np.sort(rng.choice(n, 600, replace=False))
        ix.compact(keep)
        assert np.array_equal(ix.get_labels(0, 600), labels[keep])
        idx = check(labels[keep], 600, "compacted")
        (idx0, sc0, _), _ = _distinct(ix, queries, 10, 0)
        offsets, r_rows, r_scores = ix.range_search(queries, -np.inf)
        for q in range(len(queries)):  # the survivors' best per label: the range search's ranking of the compacted rows
            lo, hi = int(offsets[q]), int(offsets[q + 1])
            e_idx, e_sc = _dedupe(r_rows[lo:hi], r_scores[lo:hi], labels[keep], 10)
            assert hi - lo == 600 and np.array_equal(idx0[q], e_idx) and np.array_equal(_bits(sc0[q]), _bits(e_sc)), q
        # ... and reset on clear
        ix.clear()
        ix.add(rows, normalize=False)
        assert (ix.get_labels(0, n) == NONE).all()
        (idx, sc, lab), path = _distinct(ix, queries, 10, 0)
        assert path == 1 and np.array_equal(idx, s_idx) and np.array_equal(_bits(sc), _bits(s_sc))
        assert ix.get_option("device_bytes_resident") > 0


def test_label_order_counts_in_device_bytes(native):
    n, d = 2000, 16
    with native.NativeIndex(d, COS, 0, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        ix.set_labels(0, (np.arange(n) // 4).astype(np.uint32))
        q = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 1, d))
        _distinct(ix, q, 5, 4)  # (answered by the over-fetch: no label order yet)
        before = ix.get_option("device_bytes_resident")
        _distinct(ix, q, 5, 0)
        assert ix.get_option("device_bytes_resident") >= before + 2 * 4 * n


# ---- 5. the facade -----------------------------------------------------------------------------------------------------------
def test_facade_distinct_over_two_shards_and_rest_field(tmp_path):
    from wdbx_amd import WDBX, api

    d, n = 16, 3000
    raw = O.synth_rows(O.SEED_CORPUS, 0, n, d)
    rng = np.random.default_rng(9)
    doc = rng.integers(0, 200, size=n)
    meta = {f"row_{i}": ({"doc": f"doc{doc[i]}", "lang": "en" if i % 3 else "de"} if i % 50 else {"lang": "en"}) for i in range(n)}
    w = WDBX(vector_dimension=d, num_shards=2, data_dir=str(tmp_path / "distinct"), enable_plugins=False,
             config={"DISTINCT_KEY": "doc"})
    vs = w.vector_store
    vs.bulk_store(raw, metadata=meta)
    assert all(1000 < ix.next_index < 2000 for ix in vs.indices)
    q = O.synth_rows(O.SEED_QUERY, 0, 1, d)[0]

    def dedupe(full, limit, threshold=0.0):
        seen, out = set(), []
        for vid, s, m in full:
            if threshold > 0 and s < threshold:
                break
            key = m.get("doc")
            if key is not None:
                if key in seen:
                    continue
                seen.add(key)
            out.append((vid, s))
            if len(out) == limit:
                break
        return out

    def same(got, want):
        assert [g[0] for g in got] == [x[0] for x in want]
        np.testing.assert_allclose([g[1] for g in got], [x[1] for x in want], atol=2e-5, rtol=0)
        assert all(g[2] == meta[g[0]] for g in got)

    # an exhaustive vector_search (every row of both shards), deduplicated in Python
    full = w.vector_search(q.tolist(), limit=n)  # (above MAX_K: shard by shard, every row of both)
    assert len(full) == n and len({m.get("doc") for _, _, m in full if "doc" in m}) == 200
    got = w.vector_search_distinct(q.tolist(), limit=10)
    same(got, dedupe(full, 10))
    assert len({g[2].get("doc", g[0]) for g in got}) == 10
    same(w.vector_search_distinct(q.tolist(), limit=250), dedupe(full, 250))  # every label and every unlabelled row: 200 + 60
    t = got[4][1] - 1e-4
    cut = w.vector_search_distinct(q.tolist(), limit=10, threshold=t)
    same(cut, dedupe(full, 10, threshold=t))
    assert 5 <= len(cut) < 10
    # a filter travels as the mask: a document is shown by its best MATCHING chunk
    flt = {"lang": "de"}
    full_de = [r for r in full if r[2].get("lang") == "de"]
    same(w.vector_search_distinct(q.tolist(), limit=10, filter_metadata=flt), dedupe(full_de, 10))
    same(asyncio.run(w.vector_search_distinct_async(q.tolist(), limit=10)), dedupe(full, 10))
    # update_metadata relabels: the best hit joins the second hit's document and disappears behind it or replaces it
    top, second = got[0][0], got[1][0]
    moved = dict(meta[top], doc=meta[second].get("doc", "fresh"))
    assert vs.update_metadata(top, moved)
    meta[top] = moved
    full = w.vector_search(q.tolist(), limit=n)  # (above MAX_K: shard by shard, every row of both)
    same(w.vector_search_distinct(q.tolist(), limit=10), dedupe(full, 10))
    # the REST field
    body = {"query_vector": q.tolist(), "limit": 10, "distinct": True}
    rest = asyncio.run(api.search_endpoint(w, body))["results"]
    assert [r["vector_id"] for r in rest] == [x[0] for x in dedupe(full, 10)]
    plain = asyncio.run(api.search_endpoint(w, {"query_vector": q.tolist(), "limit": 10, "distinct": False}))["results"]
    assert [r["vector_id"] for r in plain] == [r[0] for r in full[:10]]
    with pytest.raises(ValueError):
        asyncio.run(api.search_endpoint(w, {"query_vector": q.tolist(), "distinct": "yes"}))
    asyncio.run(w.shutdown())
