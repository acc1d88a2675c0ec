"""The checkers of the fp32 scan and range tests must be able to fail (CPU): tests/scan_harness.py's numpy models of the
documented behaviour -- partition, key order, mask, NaN / infinity rules, count past cap -- pass the very checker functions
the GPU tests use, and every deliberately wrong model is rejected by them."""
import numpy as np
import pytest

import scan_harness as S

METRICS = (S.METRIC_COSINE, S.METRIC_L2)
# a ragged instance: 22 quads on 32 lanes x 1 quad (10 idle slots); 2101 rows as in the GPU list tests
L, QPL, PITCH4, N = 32, 1, 22, 2101


def _corpus(kind, seed=0):
    rng = np.random.default_rng(seed)
    rows, q = (S.int_corpus if kind == "int" else S.float_corpus)(rng, N, PITCH4 * 4)
    rows[1] = 0.0
    rows[2, 0], q[0, 0] = np.inf, 1.0
    rows[4, 7] = np.nan
    return rows, q[0], S.special_masks(N, rng)


def _dump_check(out, rows, q, metric, kind, mask):
    cls = S.row_class(rows)
    if kind == "int":
        exact = S.exact_keys(np.where(np.isfinite(rows), rows, 0), q, metric)
        v, _ = S.truth64(rows, q, metric)
        inf = np.flatnonzero(cls == 2)
        exact[inf] = S.make_keys(S.f2ord(v[inf].astype(np.float32)), inf)
        S.check_dump(out, N, cls, mask, exact=exact)
    else:
        v, s = S.truth64(rows, q, metric)
        with np.errstate(invalid="ignore"):
            S.check_dump(out, N, cls, mask, value=v, band=S.gamma(S.scan_roundings(L, QPL, PITCH4, False, metric)) * s)


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("metric", METRICS)
def test_the_dump_model_passes(kind, metric):
    rows, q, masks = _corpus(kind)
    for mask in (None, masks["random"], masks["edge"], masks["zeros"], masks["ones"]):
        _dump_check(S.model_dump(rows, q, metric, L, QPL, N + 9, mask), rows, q, metric, kind, mask)


DUMP_MUTANTS = ["last_quad_dropped", "idle_slot_not_zeroed", "last_row_skipped", "mask_shifted", "l2_sign"]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("mutant", DUMP_MUTANTS)
def test_wrong_dump_models_are_rejected(mutant, kind):
    rows, q, masks = _corpus(kind)
    mask = masks["random"] if mutant == "mask_shifted" else None
    metrics = (S.METRIC_L2,) if mutant == "l2_sign" else METRICS
    for metric in metrics:
        with pytest.raises(AssertionError):
            _dump_check(S.model_dump(rows, q, metric, L, QPL, N + 9, mask, mutant=mutant), rows, q, metric, kind, mask)


def test_a_write_behind_the_rows_and_a_negative_zero_are_rejected():
    rows, q, _ = _corpus("int")
    out = S.model_dump(rows, q, S.METRIC_COSINE, L, QPL, N + 9)
    out[N] = 0
    with pytest.raises(AssertionError):
        _dump_check(out, rows, q, S.METRIC_COSINE, "int", None)
    out = S.model_dump(rows, q, S.METRIC_COSINE, L, QPL, N + 9)
    assert S.key_ord(out[1:2])[0] == 0x80000000  # the zero row: +0
    out[1] = S.make_keys(S.f2ord(np.float32(-0.0)), [1])[0]
    for kind in ("int", "float"):
        with pytest.raises(AssertionError):
            _dump_check(out, rows, q, S.METRIC_COSINE, kind, None)


LIST_LAUNCHES = [(65, 1, 0, 0), (65, 3, 0, 1), (64, 3, 90, 0), (129, 1, 0, 1), (1, 3, 0, 0), (128, 2, 140, 1)]


@pytest.mark.parametrize("metric", METRICS)
def test_the_list_model_passes(metric):
    rows, q, masks = _corpus("int", 1)
    keys = S.model_dump(rows, q, metric, L, QPL, N, masks["random"])
    for k, grid_x, chunk, wgm in LIST_LAUNCHES:
        part = S.model_lists(keys, k, L, N, grid_x, chunk, wgm)
        S.check_lists(part, k, grid_x if wgm else grid_x * 4, S.list_rows(L, N, grid_x, chunk, wgm), keys)
    # the partition covers every row exactly once (1051 groups: a chunk of at least 88 on 12 waves); a chunk past the need
    # leaves waves without rows
    for grid_x, chunk in ((1, 0), (3, 0), (3, 88), (3, 100), (2, 140)):
        behind = S.list_rows(L, N, grid_x, chunk, 0)
        assert np.array_equal(np.sort(np.concatenate(behind)), np.arange(N))
    assert any(len(b) == 0 for b in S.list_rows(L, N, 3, 100, 0))


@pytest.mark.parametrize("mutant", ["last_row_twice", "last_row_skipped", "ties_higher_row_first", "lost_on_64_boundary"])
def test_wrong_list_models_are_rejected(mutant):
    rows, q, _ = _corpus("int", 1)
    rows[N - 1] = q * 4 / max(1.0, float(np.abs(q[np.isfinite(q)]).max()))  # (the last row ranks high: it belongs in its list)
    rows[N - 1, 0] = 4.0
    for metric in METRICS:
        keys = S.model_dump(np.where(np.isinf(rows), 0, rows), q, metric, L, QPL, N)
        if metric == S.METRIC_L2:
            rows2 = rows.copy()
            rows2[N - 1] = q  # distance 0: the best row
            keys = S.model_dump(np.where(np.isinf(rows2), 0, rows2), q, metric, L, QPL, N)
        k, grid_x, wgm = (65, 1, 1) if mutant == "lost_on_64_boundary" else (128, 1, 0)
        part = S.model_lists(keys, k, L, N, grid_x, 0, wgm, mutant=mutant)
        with pytest.raises(AssertionError):
            S.check_lists(part, k, grid_x if wgm else grid_x * 4, S.list_rows(L, N, grid_x, 0, wgm), keys)


def _range_setup(metric, seed=2):
    rows, q, masks = _corpus("int", seed)
    keys = S.model_dump(np.where(np.isinf(rows), 0, rows), q, metric, L, QPL, N)
    s = S.ord2f(S.key_ord(keys[keys != 0])).astype(np.float64)
    thr = np.float32(np.median(-s if metric == S.METRIC_L2 else s))  # sits exactly on rows' scores (integers: many ties)
    return keys, thr, masks


@pytest.mark.parametrize("metric", METRICS)
def test_the_range_model_passes(metric):
    keys, thr, masks = _range_setup(metric)
    for t in (thr, np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan), np.float32(0.0), np.float32(-0.0)):
        for mask in (None, masks["random"], masks["edge"]):
            ok = S.range_passes(keys, t, metric)
            if mask is not None:
                ok &= S.mask_bits(mask, N)
            want = keys[ok]
            for cap in (N + 3, max(1, want.size // 2)):
                out, count = S.model_range(keys, t, metric, cap, cap + S.GUARD, mask)
                S.check_range(out[:cap], out[cap:], count, cap, want)
    assert S.range_passes(keys, np.float32(np.nan), metric).sum() == 0
    assert 0 < S.range_passes(keys, thr, metric).sum() < N
    # >= / <= : the rows ON the threshold pass
    on = S.ord2f(S.key_ord(keys)) == (-thr if metric == S.METRIC_L2 else thr)
    assert on.any() and S.range_passes(keys, thr, metric)[on & (keys != 0)].all()


@pytest.mark.parametrize("mutant", ["count_clamped", "flush_remainder_dropped", "gt_for_ge", "mask_shifted", "last_row_twice"])
def test_wrong_range_models_are_rejected(mutant):
    for metric in METRICS:
        keys, thr, masks = _range_setup(metric)
        mask = masks["random"] if mutant == "mask_shifted" else None
        t = np.float32(-np.inf) if metric == S.METRIC_COSINE and mutant == "last_row_twice" else np.float32(np.inf) if mutant == "last_row_twice" else thr
        ok = S.range_passes(keys, t, metric)
        if mask is not None:
            ok &= S.mask_bits(mask, N)
        want = keys[ok]
        cap = max(1, want.size // 2) if mutant == "count_clamped" else N + 3
        out, count = S.model_range(keys, t, metric, cap, cap + S.GUARD, mask, mutant=mutant)
        with pytest.raises(AssertionError):
            S.check_range(out[:cap], out[cap:], count, cap, want)


def test_the_roundings_counted_per_instance():
    # d = 384 on (8, 12): 12 fmas + fold 2 + 3 tree steps; L2: + 2 for the squared difference
    assert S.scan_roundings(8, 12, 96, False, S.METRIC_COSINE) == 17 and S.scan_roundings(8, 12, 96, False, S.METRIC_L2) == 19
    # the generic L = 64 body at 777 quads: 13 quads per lane on two accumulators (7 deep) + fold 3 + 6 tree steps
    assert S.scan_roundings(64, 0, 777, True, S.METRIC_COSINE) == 16
    assert S.range_roundings(64, 259, S.METRIC_COSINE) == 5 + 2 + 6 and S.range_roundings(1, 1, S.METRIC_L2) == 1 + 2 + 0 + 2
