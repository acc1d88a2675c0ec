"""discover_kernel and discover_zone_kernel ALONE on the MI355X (tests/discover_harness.py launches them from the library's own
headers): every output word -- target mode's key and wins byte per row and the counts per wins value, context mode's key per
row or per-workgroup lists, the zone stage's keys or lists -- with sentinel guards in front of and behind the arrays.

Each ``r`` comes from the existing ``rescore_kernel`` (tests/select_harness.py), the fold is tests/discover_reference.py
(numpy float32 in the contract's order), and every comparison is bit for bit.  Shapes: dims 8 / 384 (NI 2), 1024 (NI 4), 1100
(NI 0, a ragged pitch); rows 1 / 3 / 257 / 4099 (fewer rows than waves, a ragged last stride, the past-the-end clamp); pairs
0 / 1 / 3 / 4 / 5 / 32 (block cuts 2, 4 + 2, 8, 8 + 2, 8 x 8), with the target in front (pair 0 at an odd staged offset) and
without it at an odd or an even one."""
import numpy as np
import pytest

import discover_harness as DH
import select_harness as SH

pytestmark = pytest.mark.gpu

COS, L2 = DH.METRIC_COSINE, DH.METRIC_L2
_F32, _U8, _U32, _U64 = np.float32, np.uint8, np.uint32, np.uint64
ROWS = (1, 3, 257, 4099)
DIMS = (8, 384, 1024, 1100)
PAIRS = (0, 1, 3, 4, 5, 32)
BLOCKS = 3  # 12 waves


def _scores(metric, rows, vectors):
    """r [vectors, rows] from rescore_kernel: the candidates of every vector are all the rows; NaN where it scored NaN"""
    n_rows = rows.shape[0]
    cand = np.tile(DH.make_keys(np.zeros(n_rows, _F32), np.arange(n_rows)), (vectors.shape[0], 1))
    keys, _ = SH.rescore(metric, DH.pad4(rows), DH.pad4(vectors), cand, np.full(vectors.shape[0], n_rows, _U32))
    assert ((keys & _U64(0xFFFFFFFF)) == (cand & _U64(0xFFFFFFFF)))[keys != 0].all()
    return np.where(keys == 0, _F32(np.nan), DH.ord2f(keys >> _U64(32))).astype(_F32)


def _guards_ok(*guards):
    for g in guards:
        sent = DH.SENT_BYTE if g.dtype == _U8 else DH.SENT_KEY
        assert (g == sent).all()


def _check_all(metric, rows, vectors, r, mask=None, exclude=None, eligible=None, pairs=PAIRS):
    """vectors: [target, p0, n0, p1, n1, ...]; target mode reads them from 0, context mode from 1 or 2"""
    n_rows = rows.shape[0]
    eligible = np.ones(n_rows, bool) if eligible is None else eligible
    for P in pairs:
        # target mode: the records
        want_key, want_wins, want_counts = DH.records(r[0], r[1:1 + 2 * P], eligible)
        start = np.full((1, DH.ZONES), 7, _U32) if P == 3 else None  # (the kernel adds to the counts)
        key, wins, counts, guards = DH.discover_pass(metric, 3, rows, vectors, [[0, P]], 1, BLOCKS, mask=mask, exclude=exclude,
                                                     counts_in=start)
        _guards_ok(*guards)
        assert (key[0] == want_key).all(), (P, np.flatnonzero(key[0] != want_key)[:5])
        assert (wins[0] == want_wins).all(), (P, np.flatnonzero(wins[0] != want_wins)[:5])
        assert (counts[0] == want_counts + (7 if P == 3 else 0)).all(), (P, counts[0], want_counts)
        if P == 0:
            continue
        # context mode: the same pairs read from an even offset (2: the vectors shifted by one) or the odd one they sit at
        first = 1 + (P % 2 if 2 * P + 2 <= vectors.shape[0] - 1 else 0)
        staged = vectors if first == 1 else np.concatenate([vectors[:1], vectors])
        want = DH.context_keys(r[1:1 + 2 * P], eligible)
        got, front, back = DH.discover_pass(metric, 2, rows, staged, [[first, P]], 1, BLOCKS, mask=mask, exclude=exclude)
        _guards_ok(front, back)
        assert (got[0] == want).all(), (P, np.flatnonzero(got[0] != want)[:5])
        for mode, k, blocks in ((1, 10, BLOCKS), (1, 128, 1), (0, 129, BLOCKS)):
            got, front, back = DH.discover_pass(metric, mode, rows, staged, [[first, P]], k, blocks, mask=mask, exclude=exclude)
            _guards_ok(front, back)
            assert (got[0] == DH.lists_of(want, k, blocks)).all(), (P, mode, k, blocks)


def _corpus(seed, n_rows, d):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n_rows, d)).astype(_F32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    vectors = rng.standard_normal((65, d)).astype(_F32)
    vectors /= np.linalg.norm(vectors, axis=1, keepdims=True)
    vectors[4] = vectors[3]  # pair 1: positive == negative -- no win, loss term 0
    if n_rows > 5:
        rows[5] = rows[2]    # duplicate rows: every value ties, the row number decides
    return rows, vectors


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n_rows", ROWS)
def test_every_output_word(metric, d, n_rows):
    rows, vectors = _corpus(n_rows * 13 + d + metric, n_rows, d)
    r = _scores(metric, rows, vectors)
    wins, loss, dead = DH.DR.fold(r[1:7])
    assert not dead.any() and (wins <= 2).all()  # (pair 1 is never won)
    if n_rows > 5:
        assert (r[:, 5] == r[:, 2]).all()
    _check_all(metric, rows, vectors, r)


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", (8, 1024, 1100))
def test_special_inputs(metric, d):
    """a NaN row, an Inf row, a mask word with mixed bits together with excluded rows first / middle / last"""
    n_rows = 257
    rows, vectors = _corpus(d + metric, n_rows, d)
    rows[100, d - 1] = np.nan   # (the last element: the ragged quad)
    rows[101, 0] = np.inf       # L2: every r is -inf, so every pair's difference is NaN; cosine: +-inf scores
    rng = np.random.default_rng(d)
    allowed = rng.random(n_rows) < 0.6
    allowed[[2, 5, 100, 101]] = True
    mask = np.packbits(np.concatenate([allowed, np.zeros(-n_rows % 32, bool)]), bitorder="little").view(_U32)
    exclude = np.array([0, 128, n_rows - 1], _U32)
    r = _scores(metric, rows, vectors)
    assert np.isnan(r[:, 100]).all() and np.isinf(r[:, 101]).all()
    key, wins, counts, _ = DH.discover_pass(metric, 3, rows, vectors, [[0, 3]], 1, BLOCKS)
    assert key[0, 100] == 0 and wins[0, 100] == 0 and counts.sum() == np.count_nonzero(key[0])
    if metric == L2:
        assert key[0, 101] == 0 and counts.sum() == n_rows - 2
    key, _, _, _ = DH.discover_pass(metric, 3, rows, vectors, [[0, 0]], 1, BLOCKS)
    assert key[0, 100] == 0 and key[0, 101] != 0  # (no pair: the Inf row's target score alone is a score)
    pairs = (0, 1, 3, 5)
    _check_all(metric, rows, vectors, r, pairs=pairs)
    eligible = allowed.copy()
    _check_all(metric, rows, vectors, r, mask=mask, eligible=eligible, pairs=pairs)
    eligible[exclude] = False
    _check_all(metric, rows, vectors, r, mask=mask, exclude=exclude, eligible=eligible, pairs=pairs)


def test_several_queries_share_a_launch():
    """grid.y > 1: every query reads its own table entry and writes its own slices and counts"""
    rows, vectors = _corpus(3, 257, 100)
    r = _scores(COS, rows, vectors)
    ones = np.ones(257, bool)
    table = np.array([[0, 0], [1, 1], [6, 5]], _U32)  # targets 0, 1, 6
    want = [DH.records(r[t], r[t + 1:t + 1 + 2 * p], ones) for t, p in table]
    key, wins, counts, guards = DH.discover_pass(COS, 3, rows, vectors, table, 1, BLOCKS)
    _guards_ok(*guards)
    for q in range(3):
        assert (key[q] == want[q][0]).all() and (wins[q] == want[q][1]).all() and (counts[q] == want[q][2]).all()
    table = np.array([[0, 1], [3, 4], [11, 5]], _U32)
    want = [DH.context_keys(r[t:t + 2 * p], ones) for t, p in table]
    got, front, back = DH.discover_pass(COS, 2, rows, vectors, table, 1, BLOCKS)
    _guards_ok(front, back)
    assert (got == np.stack(want)).all()
    for mode, k in ((1, 10), (0, 129)):
        got, front, back = DH.discover_pass(COS, mode, rows, vectors, table, k, BLOCKS)
        _guards_ok(front, back)
        assert (got == np.stack([DH.lists_of(w, k, BLOCKS) for w in want])).all()


@pytest.mark.parametrize("n_rows", (1, 63, 257, 4099))
def test_zone_kernel_on_hand_made_records(n_rows):
    """records of two query slots: random wins 0 .. 3, some keys 0 (ineligible rows, in no zone), tied scores; entries that
    name both slots, an empty zone and zone 0"""
    rng = np.random.default_rng(n_rows)
    score = rng.integers(-3, 4, size=(2, n_rows)).astype(_F32)  # (few values: the row number decides often)
    rec_key = DH.make_keys(score, np.tile(np.arange(n_rows), (2, 1)))
    rec_wins = rng.integers(0, 4, size=(2, n_rows)).astype(_U8)
    dead = rng.random((2, n_rows)) < 0.2
    rec_key[dead] = 0
    rec_wins[dead] = 0
    table = np.array([[0, 3], [1, 0], [0, 7], [1, 2], [0, 0]], _U32)
    want = [DH.zone_keys(rec_key[s], rec_wins[s], z) for s, z in table]
    got, front, back = DH.zone_pass(2, rec_key, rec_wins, table, 1, BLOCKS)
    _guards_ok(front, back)
    assert (got == np.stack(want)).all()
    assert not want[2].any()
    for mode, k, blocks in ((1, 1, BLOCKS), (1, 10, BLOCKS), (1, 128, 1), (0, 129, BLOCKS), (0, 10, 1)):
        got, front, back = DH.zone_pass(mode, rec_key, rec_wins, table, k, blocks)
        _guards_ok(front, back)
        assert (got == np.stack([DH.zone_lists_of(w, k, blocks) for w in want])).all(), (mode, k, blocks)
