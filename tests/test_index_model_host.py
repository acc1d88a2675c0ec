"""tests/index_model.py without a device: the generator is deterministic and its committed seeds cover every (mutation kind,
state of the copies) cell and every special form; the model's mutations equal a loop-by-loop restatement; ``compare`` flags
planted differences and accepts equal results; the float64 reference alone decides at least 90 % of the (checkpoint, query)
pairs of the committed sequences."""
import numpy as np
import pytest

import index_model as M

METRICS = ("cosine", "l2")


def _committed(metric):
    return [(M.ops(seed, metric, d), metric, d) for seed, d in M.SEEDS[metric]]


def test_route_options_are_those_of_the_update_tests():
    import test_gpu_update as U

    assert (M.BASE, M.ROUTES, M.K, M.NQ, M.COVERAGES) == (U.BASE, U.ROUTES, U.K, U.NQ, U.COVERAGES)
    assert set(M.ROUTE_REPORTS) == {name for name, _, _ in M.ROUTES} == M.routes_of("cosine")
    assert M.routes_of("cosine") - M.routes_of("l2") == set(M.COSINE_ONLY)
    assert M.route_report("u42 rounds", "l2") == {"last_single_path": 2, "last_single_u6": 0, "last_single_u42": 0}
    assert M.route_report("u42 rounds", "cosine") == M.ROUTE_REPORTS["u42 rounds"]


@pytest.mark.parametrize("metric", METRICS)
def test_the_generator_is_deterministic_and_its_ops_are_plain(metric):
    for seed, d in M.SEEDS[metric]:
        seq = M.ops(seed, metric, d)
        assert seq == M.ops(seed, metric, d)
        assert 10 <= len(seq) <= 14
        assert eval(repr(seq)) == seq                    # printable, and the print replays
        for op in seq:
            assert op[0] in M.KINDS and type(op[-1]) is bool

            def plain(x):
                return all(plain(y) for y in x) if isinstance(x, tuple) else type(x) in (int, float, str, bool)
            assert plain(op), op
    assert len(M.SEEDS[metric]) == 6 and sorted(d for _, d in M.SEEDS[metric]) == [96] * 5 + [384]


@pytest.mark.parametrize("metric", METRICS)
def test_committed_seeds_cover_every_cell_and_every_form(metric):
    seqs = _committed(metric)
    hit, forms = M.cells(seqs)
    want = {(kind, state) for kind in M.KINDS for state in M.STATES}     # every kind can meet every state
    print(f"{metric}: cells hit {len(hit & want)} of {len(want)}: {sorted(hit)}")
    print(f"{metric}: forms {sorted(forms)}")
    assert not want - hit, sorted(want - hit)
    wanted_forms = set(M.FORMS) | (set(M.FORMS_L2) if metric == "l2" else set())
    assert not wanted_forms - forms, sorted(wanted_forms - forms)
    for seq, _, d in seqs:
        log = M.trace(seq, metric, d)
        # per sequence: growth beyond the capacity, and an add straight after an add
        assert any("add beyond the capacity" in f for _, _, f in log)
        assert any("add after add, no search between" in f for _, _, f in log)
        # the row count at every checkpoint (a clear's own is the empty index)
        m = M.Model(d, metric)
        for op in seq:
            m.apply(op)
            assert op[0] == "clear" or M.N_MIN <= m.n <= M.N_MAX
        assert m.cap > M.INITIAL_CAPACITY
    if metric == "l2":
        _one_bound_around_the_outlier_at_d384()


def _one_bound_around_the_outlier_at_d384():
    """The GPU test asserts that the per-group bounds switch on at the outlier row and off at its overwrite only where the
    corpus had the one bound before (largest squared norm <= 1.5 x the mean).  The d = 384 L2 sequence must be such a case,
    with room to spare on both sides, or that assertion would run nowhere."""
    (seed, d), = [sd for sd in M.SEEDS["l2"] if sd[1] == 384]
    seq = M.ops(seed, "l2", d)
    log = M.trace(seq, "l2", d)
    out = [i for i, (_, _, f) in enumerate(log) if "outlier norm" in f]
    back = [i for i, (_, _, f) in enumerate(log) if "outlier overwritten back" in f]
    assert len(out) == 1 and len(back) == 1 and 0 < out[0] < back[0]
    assert seq[out[0] - 1][0] != "clear" and seq[back[0]][0] == "set_rows"
    m = M.Model(d, "l2")
    ratio = {}
    for i, op in enumerate(seq):
        m.apply(op)
        if m.n:
            sq = (m.rows.astype(np.float64) ** 2).sum(axis=1)
            sq = sq[np.isfinite(sq)]
            ratio[i] = sq.max() / sq.mean()
    print(f"l2 d 384: largest / mean squared norm before the outlier {ratio[out[0] - 1]:.3f}, with it {ratio[out[0]]:.1f}, "
          f"after its overwrite {ratio[back[0]]:.3f}")
    assert ratio[out[0] - 1] < 1.4 and ratio[out[0]] > 3.0 and ratio[back[0]] < 1.4


# ---- the model against a second restatement, loop by loop ---------------------------------------------------------------
def _loop_compact(rows, labels, keep):
    out_rows, out_labels = [], []
    for src in keep:
        out_rows.append([x for x in rows[int(src)]])
        if labels is not None:
            out_labels.append(labels[int(src)])
    return out_rows, (out_labels if labels is not None else None)


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32).reshape(-1).view(np.uint32), np.asarray(b, np.float32).reshape(-1).view(np.uint32))


@pytest.mark.parametrize("metric", METRICS)
def test_model_mutations_equal_a_loop_by_loop_restatement(metric):
    rng = np.random.default_rng(11)
    d = 3
    for case in range(300):
        n = int(rng.integers(1, 30))
        m = M.Model(d, metric)
        m.add(rng.standard_normal((n, d)).astype(np.float32))
        if case % 2:
            m.set_labels(0, rng.integers(0, 5, n).astype(np.uint32))
        rows = [[x for x in r] for r in m.rows]
        labels = None if m.labels is None else list(m.labels)
        ids = np.sort(rng.choice(n, int(rng.integers(0, n + 1)), replace=False))
        new = rng.standard_normal((len(ids), d)).astype(np.float32)
        which = case % 4
        if which == 0:
            m.set_rows_at(ids, new)
            for j, r in enumerate(ids):
                for c in range(d):
                    rows[int(r)][c] = new[j, c]
        elif which == 1:
            m.remove_rows(ids)
            for r in ids:
                for c in range(d):
                    rows[int(r)][c] = np.float32(np.nan)
            assert m.removed().tolist() == [i in set(ids.tolist()) for i in range(n)]
        elif which == 2:
            m.compact(ids)
            rows, labels = _loop_compact(rows, labels, ids)
        else:
            m.clear()
            rows, labels = [], None
            assert m.labels is None
        assert m.n == len(rows)
        assert np.isnan(m.rows).tolist() == [[bool(np.isnan(x)) for x in r] for r in rows]
        assert _same(np.nan_to_num(m.rows), np.nan_to_num(np.asarray(rows, np.float32).reshape(-1, d)))
        assert (m.labels is None) == (labels is None)
        if labels is not None:
            assert m.labels.tolist() == [int(x) for x in labels]
        # rows appended afterwards are labels of their own while labels exist
        m.add(np.ones((2, d), np.float32))
        assert m.labels is None or m.labels[-2:].tolist() == [M.LABEL_NONE] * 2


# ---- the checker has teeth ----------------------------------------------------------------------------------------------
def _topk_result():
    ids = np.arange(32, dtype=np.int64).reshape(16, 2)
    scores = np.linspace(0.1, 0.9, 32, dtype=np.float32).reshape(16, 2)
    return ids, scores


def _range_result():
    offsets = np.array([0, 3, 3, 7], np.int64)
    rows = np.array([5, 2, 9, 1, 4, 8, 3], np.int64)
    scores = np.linspace(0.9, 0.2, 7, dtype=np.float32)
    return offsets, rows, scores


def test_compare_accepts_equal_results_and_flags_planted_differences():
    a = _topk_result()
    assert M.compare(a, tuple(x.copy() for x in a), "search, u8 scan") is None
    # one swapped id
    ids = a[0].copy()
    ids[7] = ids[7][::-1]
    said = M.compare(a, (ids, a[1]), "search, u8 scan")
    assert said is not None and "search, u8 scan" in said and "query 7, position 0" in said and "14" in said and "15" in said
    # one score differing in its last bit
    scores = a[1].copy()
    scores.view(np.uint32)[11, 1] ^= 1
    said = M.compare(a, (a[0], scores), "search, fp32 scan")
    assert said is not None and "query 11, position 1" in said and "score bits" in said
    # NaN scores with equal bits are equal; a different shape is a difference
    nan = a[1].copy()
    nan[0, 0] = np.nan
    assert M.compare((a[0], nan), (a[0], nan.copy())) is None
    assert M.compare(a, (a[0][:, :1], a[1][:, :1])) is not None
    # a range result with one row missing
    r = _range_result()
    assert M.compare(r, tuple(x.copy() for x in r), "range_search", "range") is None
    short = (np.array([0, 3, 3, 6], np.int64), np.delete(r[1], 5), np.delete(r[2], 5))
    said = M.compare(r, short, "range_search", "range")
    assert said is not None and "query 2" in said and "position 2" in said
    # the same rows in another order: equal only where the order is not promised
    flipped = (r[0], r[1].copy(), r[2].copy())
    flipped[1][:3], flipped[2][:3] = r[1][:3][::-1], r[2][:3][::-1]
    assert M.compare(r, flipped, "range_search", "range", ordered=True) is not None
    assert M.compare(r, flipped, "range_search", "range", ordered=False) is None
    last_bit = (r[0], r[1], r[2].copy())
    last_bit[2].view(np.uint32)[6] ^= 1
    assert "score bits" in M.compare(r, last_bit, "range_search", "range", ordered=False)


def test_reference_check_flags_a_wrong_row_and_skips_ties():
    m = M.Model(8, "l2")
    rng = np.random.default_rng(2)
    m.add(rng.standard_normal((50, 8)).astype(np.float32))
    m.set_rows_at([7], m.queries[:1])
    m.remove_rows([9])
    exact = [M.separated_topk(*M.scores64(m.rows, q, "l2"), M.K, M.gamma(8))[0] for q in m.queries]
    ids = np.stack(exact).astype(np.int64)
    errors, checked, skipped = M.reference_check(m, 8, "search", (ids, None))
    assert not errors and checked == M.NQ and skipped == 0 and ids[0, 0] == 7 and 9 not in ids
    wrong = ids.copy()
    wrong[3, 1] = [r for r in range(50) if r not in ids[3]][0]
    assert len(M.reference_check(m, 8, "search", (wrong, None))[0]) == 1
    m.set_rows_at([20, 21, 22], np.repeat(m.queries[5:6], 3, axis=0))       # a tie at the k-th score names no unique set
    _, checked, skipped = M.reference_check(m, 8, "search", (wrong, None))    # (three equal rows tie for other queries too)
    assert skipped >= 1 and checked + skipped == M.NQ
    assert not M.separated_topk(*M.scores64(m.rows, m.queries[5], "l2"), M.K, M.gamma(8))[1]
    # range: the threshold between two rows' scores
    s, _ = M.scores64(m.rows, m.queries[0], "l2")
    order = np.argsort(-s)
    t = np.float32(-(s[order[4]] + s[order[5]]) / 2)
    good = (np.array([0, 5]), order[:5].astype(np.int64), None)
    assert not M.reference_check(m, 8, "range_search", good, thresholds=t)[0]
    assert M.reference_check(m, 8, "range_search", (np.array([0, 4]), order[:4].astype(np.int64), None), thresholds=t)[0]
    assert M.reference_check(m, 8, "range_search", (np.array([0, 6]), order[:6].astype(np.int64), None), thresholds=t)[0]


# ---- how much the float64 reference decides -----------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_float64_reference_decides_nine_pairs_in_ten_at_every_checkpoint(metric):
    pairs = undecided = 0
    for seed, d in M.SEEDS[metric]:
        m = M.Model(d, metric)
        g = M.gamma((d + 3) // 4 * 4)
        for i, op in enumerate(M.ops(seed, metric, d)):
            m.apply(op)
            if not m.n:
                continue
            here = sum(not M.separated_topk(*M.scores64(m.rows, q, metric), M.K, g)[1] for q in m.queries)
            assert here <= 0.10 * M.NQ, (seed, d, i, op, here)
            pairs += M.NQ
            undecided += here
    print(f"{metric}: {undecided} of {pairs} (checkpoint, query) pairs have a top-{M.K} gap inside the fp32 error: "
          f"{100.0 * undecided / pairs:.3f} %; at no checkpoint more than 10 % of its {M.NQ} queries")
    assert undecided <= 0.10 * pairs
