"""matrix_kernel ALONE on the MI355X (tests/matrix_harness.py launches it from the library's own headers): every output word of
both sinks -- a key per (anchor, listed row), or per-workgroup lists in registers and in LDS -- with sentinel guards in front
of and behind the arrays.

The scores come from the existing ``rescore_kernel`` (tests/select_harness.py) with the listed rows as its queries, and every
comparison is bit for bit.  Shapes: dims 8 / 384 (NI 2), 1024 (NI 4), 1100 (NI 0, a ragged pitch); lists of 1 (only self), 2,
3 (fewer rows than waves), 9 (a ragged anchor block for 8 and 4), 257 and 1030 (a ragged last stride, several workgroups);
k 10 with 8 anchors per block, 128 with 4, 129 with the lists in LDS; the listed rows are not contiguous in the corpus, one
vector sits at two list positions, and one listed row holds a NaN (as anchor and as candidate)."""
import numpy as np
import pytest

import matrix_harness as MH
import select_harness as SH

pytestmark = pytest.mark.gpu

COS, L2 = MH.METRIC_COSINE, MH.METRIC_L2
_F32, _U32, _U64 = np.float32, np.uint32, np.uint64
LISTS = (1, 2, 3, 9, 257, 1030)
DIMS = (8, 384, 1024, 1100)
BLOCKS = 3  # 12 waves


def _case(seed, n_ids, d):
    """a corpus about twice the list, the list a sorted random part of it; list positions 1 and n - 2 hold one vector, position
    n // 2 a NaN (lists of 9 and more)"""
    rng = np.random.default_rng(seed)
    n_rows = 2 * n_ids + 5
    rows = rng.standard_normal((n_rows, d)).astype(_F32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    ids = np.sort(rng.choice(n_rows, n_ids, replace=False)).astype(_U32)
    if n_ids >= 3:
        rows[ids[n_ids - 2]] = rows[ids[1]]
    if n_ids >= 9:
        rows[ids[n_ids // 2], d // 2] = np.nan
    return rows, ids


def _scores(metric, rows, ids):
    """r [n_ids, n_ids] from rescore_kernel: query i is the listed row i as stored, its candidates are all the listed rows"""
    cand = np.tile(MH.make_keys(np.zeros(ids.size, _F32), ids), (ids.size, 1))
    padded = MH.pad4(rows)
    keys, _ = SH.rescore(metric, padded, padded[ids], cand, np.full(ids.size, ids.size, _U32))
    assert ((keys & _U64(0xFFFFFFFF)) == (cand & _U64(0xFFFFFFFF)))[keys != 0].all()
    return np.where(keys == 0, _F32(np.nan), MH.ord2f(keys >> _U64(32))).astype(_F32)


def _guards_ok(*guards):
    for g in guards:
        assert (g == MH.SENT_KEY).all()


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n_ids", LISTS)
def test_every_output_word(metric, d, n_ids):
    rows, ids = _case(n_ids * 17 + d + metric, n_ids, d)
    r = _scores(metric, rows, ids)
    want = MH.pair_keys(r, ids)
    if n_ids >= 3:
        a, b = 1, n_ids - 2
        if a != b:  # the duplicated vector: each copy is the other's neighbour, with the score a row has against itself
            assert want[a, b] != 0 and want[b, a] != 0 and (r[a, b] == r[a, a] or np.isnan(r[a, a]))
    if n_ids >= 9:
        nan = n_ids // 2
        assert (want[nan] == 0).all() and (want[:, nan] == 0).all()  # the NaN row: no line of its own, nobody's neighbour
    assert (np.diag(want) == 0).all()

    # a key per (anchor, listed row): 8 anchors per block in two rounds (the second starts inside the list), then the block of one
    cut = min(n_ids, 256) if n_ids < 1030 else 515  # (515: a first anchor that is no multiple of the block)
    got = []
    for first, na in ((0, cut), (cut, n_ids - cut)):
        if na:
            keys, front, back = MH.matrix_pass(metric, 2, 8, rows, ids, first, na, 1, BLOCKS)
            _guards_ok(front, back)
            got.append(keys)
    got = np.concatenate(got)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    tail = min(n_ids, 5)
    keys, front, back = MH.matrix_pass(metric, 2, 1, rows, ids, n_ids - tail, tail, 1, 1)
    _guards_ok(front, back)
    assert (keys == want[n_ids - tail:]).all()

    # lists: registers with 8, 4 and 1 anchors per block, LDS with 1; one launch with every anchor, one from position 1 on
    for mode, qb, k, blocks, first in ((1, 8, 10, BLOCKS, 0), (1, 4, 128, BLOCKS, min(1, n_ids - 1)), (1, 1, 10, 1, 0),
                                       (0, 1, 129, BLOCKS, 0)):
        na = n_ids - first
        if mode == 0 and n_ids > 257:
            first, na = n_ids - 40, 40  # (the LDS lists of 1030 anchors x 129: the last 40 say as much)
        lists, front, back = MH.matrix_pass(metric, mode, qb, rows, ids, first, na, k, blocks)
        _guards_ok(front, back)
        for i in range(na):
            ref = MH.lists_of(want[first + i], k, blocks)
            assert (lists[i] == ref).all(), (mode, qb, k, first + i)


@pytest.mark.parametrize("metric", [COS, L2])
def test_symmetry_and_run_to_run(metric):
    """G[i][j] == G[j][i] bit for bit (the sums are symmetric in their operands), and two launches write the same words"""
    rows, ids = _case(99 + metric, 257, 384)
    a, f, b = MH.matrix_pass(metric, 2, 8, rows, ids, 0, 257, 1, BLOCKS)
    again, _, _ = MH.matrix_pass(metric, 2, 8, rows, ids, 0, 257, 1, 5)
    _guards_ok(f, b)
    assert (a == again).all()
    score = a >> _U64(32)
    assert (score == score.T).all()
