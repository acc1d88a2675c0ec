"""recommend_kernel ALONE on the MI355X (tests/recommend_harness.py launches it from the library's own headers): every output
word of both sides in all three ranking modes, with sentinel guards in front of and behind the output.

Integer corpora (elements in {-2 .. 2}: every fp32 sum is exact): keys ``==`` an int64 reference of the fold.  Float corpora:
each ``r`` comes from the existing ``rescore_kernel`` (tests/select_harness.py), the fold is numpy float32, keys bit-equal.
Shapes: rows 1 / 63 / 257 / 1000 (fewer rows than waves, a ragged last stride), dims 8 / 100 / 384 / 516 / 1028 (every NI
instance, a ragged pitch), examples 1+0 / 1+1 / 8+0 / 5+4 (a block edge) / 32+32, k 1 .. 129 and select_min_k."""
import numpy as np
import pytest

import recommend_harness as RH
import select_harness as SH

pytestmark = pytest.mark.gpu

COS, L2 = RH.METRIC_COSINE, RH.METRIC_L2
_F32, _U32, _U64, _I64 = np.float32, np.uint32, np.uint64, np.int64
ROWS = (1, 63, 257, 1000)
DIMS = (8, 100, 384, 516, 1028)
EXAMPLES = ((1, 0), (1, 1), (8, 0), (5, 4), (32, 32))
KS = (1, 10, 64, 65, 128, 129, 200)  # (200: the default select_min_k)
BLOCKS = 3  # 12 waves


def _check_all(metric, rows, examples, r, k_shift, mask=None, exclude=None, eligible=None, example_sets=EXAMPLES):
    n_rows = rows.shape[0]
    eligible = np.ones(n_rows, bool) if eligible is None else eligible
    at, ks_seen = 0, set()
    for npos, nneg in example_sets:
        table = np.array([[0, npos, npos + nneg]], _U32)
        for side in (1, 0):
            want = RH.row_keys(r[:npos + nneg], npos, side, eligible)
            got, front, back = RH.recommend_pass(metric, 2, side, rows, examples, table, 1, BLOCKS, mask=mask, exclude=exclude)
            assert (front == RH.SENT_KEY).all() and (back == RH.SENT_KEY).all()
            assert (got[0] == want).all(), (npos, nneg, side, np.flatnonzero(got[0] != want)[:5])
            for j in range(3):  # three of the k values per (examples, side), rotating: all of them over a test
                k = KS[(at + k_shift) % len(KS)]
                at += 1
                ks_seen.add(k)
                for mode in ((1, 0) if k <= 128 else (0,)):
                    for blocks in (BLOCKS, 1) if j == 0 else (BLOCKS,):
                        got, front, back = RH.recommend_pass(metric, mode, side, rows, examples, table, k, blocks, mask=mask,
                                                             exclude=exclude)
                        assert (front == RH.SENT_KEY).all() and (back == RH.SENT_KEY).all()
                        assert (got[0] == RH.lists_of(want, k, blocks)).all(), (npos, nneg, side, k, mode, blocks)
    assert ks_seen == set(KS)  # (the rotation covered every k: at least three example sets times two sides)


def _int_scores(metric, rows, examples):
    rows, examples = rows.astype(_I64), examples.astype(_I64)
    if metric == COS:
        return examples @ rows.T
    return -((examples[:, None, :] - rows[None, :, :]) ** 2).sum(axis=2)


def _float_scores(metric, rows, examples):
    """r [examples, rows] from rescore_kernel: the candidates of every example are all the rows"""
    n_rows = rows.shape[0]
    cand = np.tile(RH.make_keys(np.zeros(n_rows, _F32), np.arange(n_rows)), (examples.shape[0], 1))
    keys, guard = SH.rescore(metric, RH.pad4(rows), RH.pad4(examples), cand, np.full(examples.shape[0], n_rows, _U32))
    assert ((keys & _U64(0xFFFFFFFF)) == (cand & _U64(0xFFFFFFFF)))[keys != 0].all()
    r = RH.ord2f(keys >> _U64(32))
    return np.where(keys == 0, _F32(np.nan), r).astype(_F32)


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n_rows", ROWS)
def test_integer_corpora(metric, d, n_rows):
    rng = np.random.default_rng(n_rows * 7 + d + metric)
    rows = rng.integers(-2, 3, size=(n_rows, d))
    examples = rng.integers(-2, 3, size=(64, d))
    examples[32] = examples[0]  # (32+32: the first negative is the first positive)
    _check_all(metric, rows.astype(_F32), examples.astype(_F32), _int_scores(metric, rows, examples), k_shift=n_rows + d)


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n_rows", ROWS)
def test_float_corpora(metric, d, n_rows):
    rng = np.random.default_rng(n_rows * 11 + d + metric)
    rows = rng.standard_normal((n_rows, d)).astype(_F32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    examples = rng.standard_normal((64, d)).astype(_F32)
    examples /= np.linalg.norm(examples, axis=1, keepdims=True)
    _check_all(metric, rows, examples, _float_scores(metric, rows, examples), k_shift=n_rows + d + 3)


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", (100, 516, 1028))
def test_special_inputs(metric, d):
    """a NaN element, a mask word with mixed bits, excluded rows first / middle / last, p == n ties and +-0 scores"""
    n_rows = 257
    rng = np.random.default_rng(d + metric)
    rows = rng.integers(-2, 3, size=(n_rows, d)).astype(_F32)
    examples = rng.integers(-2, 3, size=(9, d)).astype(_F32)
    examples[5] = examples[0]      # 5+4: the first negative is the first positive -- p <= n everywhere, ties where it is the best
    rows[40] = examples[0]         # L2: r = -0.0 against examples 0 and 5
    rows[41] = 0                   # cosine: r = +0 against every example
    rows[100, d - 1] = np.nan      # (the last element: the ragged quad)
    allowed = rng.random(n_rows) < 0.6
    allowed[[40, 41, 100]] = True
    mask = np.packbits(np.concatenate([allowed, np.zeros(-n_rows % 32, bool)]), bitorder="little").view(_U32)
    exclude = np.array([0, 128, n_rows - 1], _U32)
    r = _float_scores(metric, rows, examples)
    assert np.isnan(r[:, 100]).all() and not np.isnan(np.delete(r, 100, axis=1)).any()
    eligible = np.ones(n_rows, bool)
    sets = ((1, 0), (5, 4), (1, 1))
    _check_all(metric, rows, examples, r, k_shift=d, example_sets=sets)
    eligible = allowed.copy()
    _check_all(metric, rows, examples, r, k_shift=d + 1, mask=mask, eligible=eligible, example_sets=sets)
    eligible[exclude] = False
    _check_all(metric, rows, examples, r, k_shift=d + 2, mask=mask, exclude=exclude, eligible=eligible, example_sets=sets)
    # the tie and the zeros, spelled out: a negative equal to the positive leaves no row favoured, and row 40 (L2) / 41
    # (cosine) carries the key of +0.0 on the disfavoured side
    pair, one = examples[[0, 5]], np.array([[0, 1, 2]], _U32)
    assert not RH.row_keys(r[[0, 5]], 1, 1, np.ones(n_rows, bool)).any()
    got, _, _ = RH.recommend_pass(metric, 2, 1, rows, pair, one, 1, BLOCKS)
    assert not got.any()
    zero_row = 40 if metric == L2 else 41
    dis = RH.row_keys(r[[0, 5]], 1, 0, np.ones(n_rows, bool))
    assert dis[zero_row] == RH.make_keys(np.zeros(1, _F32), [zero_row])[0]
    got, _, _ = RH.recommend_pass(metric, 2, 0, rows, pair, one, 1, BLOCKS)
    assert (got[0] == dis).all()


def test_several_queries_share_a_launch():
    """grid.y > 1: every query reads its own table entry and writes its own slice"""
    rng = np.random.default_rng(3)
    rows = rng.integers(-2, 3, size=(257, 100))
    examples = rng.integers(-2, 3, size=(20, 100))
    table = np.array([[0, 1, 1], [1, 4, 5], [5, 13, 20]], _U32)
    r = _int_scores(COS, rows, examples)
    for side in (1, 0):
        want = [RH.row_keys(r[t[0]:t[2]], t[1] - t[0], side, np.ones(257, bool)) for t in table]
        got, front, back = RH.recommend_pass(COS, 2, side, rows.astype(_F32), examples.astype(_F32), table, 1, BLOCKS)
        assert (got == np.stack(want)).all() and (front == RH.SENT_KEY).all() and (back == RH.SENT_KEY).all()
        for mode, k in ((1, 10), (0, 129)):
            got, front, back = RH.recommend_pass(COS, mode, side, rows.astype(_F32), examples.astype(_F32), table, k, BLOCKS)
            assert (got == np.stack([RH.lists_of(w, k, BLOCKS) for w in want])).all()
            assert (front == RH.SENT_KEY).all() and (back == RH.SENT_KEY).all()
