"""The index as a state machine on the MI355X: a handle that went through a history of mutations answers every search call
bit for bit like a fresh handle built from the final rows in one ``add`` (tests/index_model.py states the contract, the
model, the sequences and the calls).

Per committed seed and metric the sequence is replayed on handle A (created with a capacity below its first add).  After
every op comes a checkpoint: a fresh handle F is built from the model, every call of the table runs on both with the same
options and must give equal ids and equal score bits, A's rows and labels must equal the model's, both must report the same
path, the coverages must not exceed the row count, and the plain routes, ``search_rows``, ``range_search`` and
``search_distinct`` are held against float64 scores of the model's rows.

Copies that lag: a checkpoint searches every route, which brings every copy up to the row count.  So the handle that carries
the history is searched only at the ops whose flag ``warm`` is set; the checkpoint of any other op runs on a second handle
that replays the sequence up to that op (searching the routes at the same warm ops) and is then closed.  Either way the
handle a mutation meets has been searched exactly at the warm ops before it.  A ``clear`` leaves no row to search: its
checkpoint is the size and the coverages (all zero).

That the copies lag is read from the handle, not only counted by the generator: before a checkpoint searches anything, the
five coverages the library reports (``shadow_rows``, ``shadowg_rows``, ``shadow8_rows``, ``shadow6_rows``,
``shadow42_rows``) must not pass the reach that ``index_model.Trace`` keeps for the sequence (the row count at the last warm
op, cut by ``compact`` and ``clear``), which lies below the row count after an add that no search followed; after a warm
checkpoint they equal the row count (cosine: all five; L2: the u8 copy, the one whose route reports that it ran there).
The sixth coverage, ``cn_rows`` of the squared norms, has no option that reports it and is not observed here."""
import time

import numpy as np
import pytest

import index_model as M

pytestmark = pytest.mark.gpu

CASES = [(metric, seed, d) for metric in ("cosine", "l2") for seed, d in M.SEEDS[metric]]


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


def _handle(native, model, capacity):
    metric = native.METRIC_COSINE if model.metric == "cosine" else native.METRIC_L2
    return native.NativeIndex(model.d, metric=metric, capacity_rows=capacity)


def _fresh(native, model):
    """the twin: the model's rows in one add, its labels in one set_labels"""
    f = _handle(native, model, model.n)
    f.add(model.rows)
    if model.labels is not None:
        f.set_labels(0, model.labels)
    return f


def _search_every_route(ix, model):
    for entry in M.call_table(model, (), full=False):
        M.run_call(ix, entry)


def _lagging(ix, trace, where):
    """before anything is searched: the handle's own coverages do not pass the reach the trace keeps"""
    reach = trace.cov if trace.built else 0
    cov = {name: ix.get_option(name) for name in M.COVERAGES}
    assert all(0 <= c <= reach for c in cov.values()), f"coverages {cov} beyond {reach} of {trace.m.n} rows\n{where}"
    return cov


def _replayed(native, seq, upto, d, metric, where):
    """a handle that went through seq[0 .. upto], every route searched after the warm ops before op upto"""
    trace = M.Trace(d, metric)
    model = trace.m
    ix = _handle(native, model, M.INITIAL_CAPACITY)
    for i, op in enumerate(seq[:upto + 1]):
        kind, args = model.concrete(op)
        trace.step(op)
        M.apply_to_handle(ix, kind, args)
        if op[-1] and i < upto and model.n:
            _search_every_route(ix, model)
    _lagging(ix, trace, where)
    return ix


class Tally:
    def __init__(self):
        self.routes, self.checked, self.skipped, self.calls = set(), 0, 0, 0
        self.at, self.group_bounds = 0, {}     # the op being checked; {op: group_bounds_active after its checkpoint}


def _checkpoint(native, a, model, recent, full, tally, where):
    n = model.n
    assert a.size() == n, where
    cov = {name: a.get_option(name) for name in M.COVERAGES}
    assert all(0 <= c <= n for c in cov.values()), (cov, n, where)
    if n == 0:
        return
    assert np.array_equal(a.get_rows(0, n).view(np.uint32), model.rows.view(np.uint32)), "stored rows differ from the model: " + where
    labels = model.labels if model.labels is not None else np.full(n, M.LABEL_NONE, np.uint32)
    assert np.array_equal(a.get_labels(0, n), labels), "labels differ from the model: " + where
    removed, planted = model.removed(), model.planted()
    with _fresh(native, model) as f:
        for entry in M.call_table(model, recent, full):
            name, _, _, kind, _, ref = entry
            got_a, said_a = M.run_call(a, entry)
            got_f, said_f = M.run_call(f, entry)
            tally.calls += 1
            diff = M.compare(got_a, got_f, name, kind)
            assert diff is None, f"{diff}\n{where}"
            assert said_a == said_f, f"{name}: the mutated handle reports {said_a}, the fresh one {said_f}\n{where}"
            # removed rows (and rows a compaction dropped: they have no number any more) are in no result
            ids = got_a[1] if kind == "range" else got_a[0]
            ids = ids[ids >= 0]
            assert np.all(ids < n), f"{name}: a row past the end came back\n{where}"
            if name != "search_multivector":     # (its row NAMES the label: the label's smallest row number, live or not)
                assert not removed[ids].any(), f"{name}: a removed row came back\n{where}"
            if name.startswith("search, "):
                route = name[len("search, "):]
                want = M.route_report(route, model.metric)
                if route not in M.routes_of(model.metric):   # (no such route for this metric: the library says what ran instead)
                    assert said_f == want, f"{name}: reports {said_f}, expected {want}\n{where}"
                elif said_f == want:                         # (the fresh handle started from zeros: the route did run)
                    tally.routes.add(route)
                for qi, row in planted.items():
                    assert got_a[0][qi, 0] == row, f"{name}: query {qi} does not find its copy at row {row}\n{where}"
            if ref is not None:
                errors, checked, skipped = M.reference_check(model, a.pitch, ref[0], got_a, **ref[1])
                assert not errors, f"{name}: {errors[0]} ({len(errors)} in all)\n{where}"
                tally.checked += checked
                tally.skipped += skipped
        bounds = a.get_option("group_bounds_active")
        assert bounds == f.get_option("group_bounds_active"), "group bounds decided differently\n" + where
        tally.group_bounds[tally.at] = bounds
    cov = {name: a.get_option(name) for name in M.COVERAGES}
    assert all(0 <= c <= n for c in cov.values()), (cov, n, where)


@pytest.mark.parametrize("metric,seed,d", CASES)
def test_mutated_handle_answers_like_a_fresh_build_at_every_checkpoint(native, metric, seed, d):
    t0 = time.perf_counter()
    seq = M.ops(seed, metric, d)
    trace = M.Trace(d, metric)
    model = trace.m
    tally, recent = Tally(), []
    a = _handle(native, model, M.INITIAL_CAPACITY)
    lagged = 0
    try:
        for i, op in enumerate(seq):
            kind, args = model.concrete(op)
            trace.step(op)
            M.apply_to_handle(a, kind, args)
            n = model.n
            recent = [] if kind in ("compact", "clear") else (M.recent_rows(model, kind, args) + recent)[:60]
            where = f"seed {seed}, metric {metric}, d {d}, after op {i} {op!r} of index_model.ops({seed}, {metric!r}, {d}) =\n{seq!r}"
            tally.at = i
            if op[-1] or not n:
                _checkpoint(native, a, model, recent, True, tally, where)       # (leaves A warm)
                warm = ("shadow8_rows",) if metric == "l2" else M.COVERAGES
                assert all(a.get_option(c) == n for c in warm), ({c: a.get_option(c) for c in M.COVERAGES}, n, where)
            else:                                                              # A goes on with lagging copies
                cov = _lagging(a, trace, where)
                lagged += trace.built and max(cov.values()) < n
                # what extends no copy is checked on A itself
                assert a.size() == n, where
                assert np.array_equal(a.get_rows(0, n).view(np.uint32), model.rows.view(np.uint32)), "stored rows differ from the model: " + where
                labels = model.labels if model.labels is not None else np.full(n, M.LABEL_NONE, np.uint32)
                assert np.array_equal(a.get_labels(0, n), labels), "labels differ from the model: " + where
                assert _lagging(a, trace, where) == cov
                with _replayed(native, seq, i, d, metric, where) as twin:
                    _checkpoint(native, twin, model, recent, True, tally, where + "\n(on a replay of the ops so far)")
    finally:
        a.close()
    where = f"seed {seed}, metric {metric}, d {d}, ops {seq!r}"
    assert tally.routes == M.routes_of(metric), f"routes that never ran: {M.routes_of(metric) - tally.routes}; {where}"
    assert tally.skipped <= 0.10 * (tally.checked + tally.skipped), (tally.skipped, tally.checked, where)
    # ops that met copies which exist and end below the row count, as the handle itself reported them
    log = M.trace(seq, metric, d)
    want = sum(1 for op, (_, state, _) in zip(seq, log) if op[0] == "add" and not op[-1] and state != "never built")
    assert lagged >= want, (lagged, want, where)
    if metric == "l2":
        # Which bounds a batch takes is a decision both handles must share (asserted at every checkpoint).  Where the corpus
        # had the one bound before the outlier row (largest squared norm <= 1.5 x the mean: d = 384; at d = 96 standard-normal
        # rows already pass it), the outlier switches the per-group bounds on and its overwrite switches them off again.
        out = [i for i, (_, _, f) in enumerate(log) if "outlier norm" in f]
        back = [i for i, (_, _, f) in enumerate(log) if "outlier overwritten back" in f]
        if d == 384:      # (test_index_model_host.py pins that this sequence is such a case)
            assert out and back and tally.group_bounds.get(out[0] - 1) == 0, (tally.group_bounds, where)
        if out and tally.group_bounds.get(out[0] - 1) == 0:
            assert tally.group_bounds[out[0]] == 1, (tally.group_bounds, where)
            if back:
                assert tally.group_bounds[back[0]] == 0, (tally.group_bounds, where)
    print(f"index state {metric} seed {seed} d {d}: {len(seq)} ops, {tally.calls} calls compared, float64 reference checked "
          f"{tally.checked} results and skipped {tally.skipped}, {lagged} ops left every copy short of the row count, {time.perf_counter() - t0:.2f} s")


def test_a_stale_twin_is_noticed_on_every_route(native):
    """The comparison has teeth: the twin is built from the model BEFORE the last set_rows_at of a sequence (a wrong twin,
    nothing else is touched).  On every route ``compare`` reports a difference at the query of a row that op planted."""
    metric = "cosine"
    seed, d = M.SEEDS[metric][0]
    seq = M.ops(seed, metric, d)
    last = max(i for i, op in enumerate(seq) if op[0] == "set_rows_at")
    before, after = M.Model(d, metric), M.Model(d, metric)
    for op in seq[:last]:
        before.apply(op)
        after.apply(op)
    after.apply(seq[last])
    assert before.n == after.n
    newly = [qi for qi, row in after.planted().items() if before.planted().get(qi) != row
             or not np.array_equal(before.rows[row].view(np.uint32), after.rows[row].view(np.uint32))]
    assert newly, "the op plants no new winner"
    with _replayed(native, seq, last, d, metric, "the stale-twin control") as a, _fresh(native, before) as stale, _fresh(native, after) as fresh:
        for entry in M.call_table(after, (), full=False):
            got_a, got_s, got_f = (M.run_call(ix, entry)[0] for ix in (a, stale, fresh))
            assert M.compare(got_a, got_f, entry[0]) is None, entry[0]
            for qi in newly:
                said = M.compare(tuple(x[qi:qi + 1] for x in got_a), tuple(x[qi:qi + 1] for x in got_s), entry[0])
                assert said is not None and entry[0] in said, (entry[0], qi)
                assert got_a[0][qi, 0] == after.planted()[qi]
