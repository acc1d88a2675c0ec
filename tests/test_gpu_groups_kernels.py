"""The two kernels of the groups search by themselves: group_members_kernel and group_merge_kernel (kernels_groups.h), launched
by tests/kernel_harness/groups_harness.hip on arrays built here.  Every output word and the guards in front of and behind each
buffer are compared with the numpy restatement of tests/groups_harness.py.

Instances launched -- every one the pickers can return:
  group_members_kernel<METRIC, NI>: METRIC cosine / L2; NI 2 (pitch4 1, 64, 65, 128), 4 (129, 256), 0 (257, 300)
  group_merge_kernel<METRIC>:       METRIC cosine / L2

Corpora: the integer and the Gaussian corpus of test_gpu_listed_kernels.py (581 rows) with its special rows: 5 holds a NaN (key
0), 6 holds + inf, 7 denormals, 8 equals query 0 (L2: - 0.0, the key carries + 0.0), 9 is all - 1; query 1 is zero.  The
integer corpus gives exact ties, the smaller row must win (the key holds ~row).  The expected keys are int64 arithmetic
(integer corpus) or rescore_kernel's keys, checked there against float64 within gamma(m) * S, m = ceil(pitch4 / 64) + 8 for
the inner product, + 10 for L2; one launch of a direct task per (query, row) puts this kernel's own keys under the same bound.

Tasks: the label order is a permutation of the rows cut into runs of 1 (the NaN row alone: all zeros), 2, 3, 4, 5, 9 (holds the
other special rows), 64, 65 and 257 positions -- with four waves and U = 4, 2, 1 rows in flight: no trip for three waves, a
clamped tail, full trips --, each for queries 0, 1 and 2, and direct-row tasks (the NaN row, the row equal to the query, row 0,
the last row).  group_size 1, 2, 3, 63, 64: above, at and below the run.  Masks: none, ones, zeros (every task all zeros),
every other row, each run's best row removed.

Merge: synthetic sorted lists, 1, 2, 63, 64, 65 and 130 lists per slot (one trip, a full trip, a second and a third trip of the
64-list walk), short lists with zeros behind, lists of zeros only, a slot without lists, a non-zero task base, scores + 0.0 and
+- inf; rows, scores in the caller's units (L2: - 0 + 0 = + 0, compared as bits), -1 / 0 behind the members, and the count."""
import zlib

import numpy as np
import pytest

import groups_harness as G
import listed_harness as L
from groups_harness import METRIC_COSINE as COS, METRIC_L2 as L2M
from test_gpu_listed_kernels import N_ROWS, NQ, R_DEN, R_EQ, R_INF, R_M1, R_NAN, _corpus, _keys

U32, U64, F32 = np.uint32, np.uint64, np.float32
PITCHES = [1, 64, 65, 128, 129, 256, 257, 300]
RUNS = [1, 2, 3, 4, 5, 9, 64, 65, 257]
SIZES = [1, 2, 3, 63, 64]
MASKS = ["none", "ones", "zeros", "alternate", "best_removed"]


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


def _order():
    """A permutation of the rows: position 0 the NaN row (the run of 1), the run of 9 holds the other special rows"""
    special = [R_INF, R_DEN, R_EQ, R_M1]
    rest = np.setdiff1d(np.arange(N_ROWS), [R_NAN] + special)
    rest = _rng("order").permutation(rest)
    at9 = sum(RUNS[:5])
    order = np.concatenate([[R_NAN], rest[:at9 - 1], special, rest[at9 - 1:]]).astype(U32)
    assert sorted(order.tolist()) == list(range(N_ROWS)) and sum(RUNS) <= N_ROWS
    return order


ORDER = _order()


def _tasks():
    tasks, start = [], 0
    for run in RUNS:
        tasks += [(q, start, run, 0) for q in (0, 1, 2)]
        start += run
    tasks += [(q, r, 1, 1) for q in (0, 2) for r in (R_NAN, R_EQ, 0, N_ROWS - 1)]
    return np.array(tasks, U32)


TASKS = _tasks()


def _mask(name, K):
    words = (N_ROWS + 31) // 32
    if name == "none":
        return None
    if name == "ones":
        return np.full(words, 0xFFFFFFFF, U32)
    if name == "zeros":
        return np.zeros(words, U32)
    allow = np.ones(words * 32, bool)
    if name == "alternate":
        allow[1::2] = False
    else:  # the best row of every run (for the run's first query) may not be returned
        for query, start, count, direct in TASKS.astype(np.int64):
            if not direct:
                rows = ORDER[start:start + count]
                allow[rows[np.argmax(K[query, rows])]] = False
    return np.packbits(allow, bitorder="little").view(U32)


@pytest.mark.gpu
@pytest.mark.parametrize("pitch4", PITCHES)
@pytest.mark.parametrize("metric", [COS, L2M])
@pytest.mark.parametrize("kind", ["int", "float"])
def test_members_every_word(kind, metric, pitch4):
    rows, q = _corpus(kind, pitch4)
    K = _keys(kind, metric, pitch4)
    nonzero = 0
    for mask_name in MASKS:
        mask = _mask(mask_name, K)
        for g in SIZES:
            got, front, back = G.members(metric, rows, q, ORDER, TASKS, g, mask)
            want = G.expect_members(K, ORDER, TASKS, g, mask)
            what = (kind, metric, pitch4, mask_name, g)
            assert np.all(front == G.SENT_KEY) and np.all(back == G.SENT_KEY), what
            bad = np.argwhere(got != want)
            assert bad.size == 0, (what, bad[:4].tolist(), [hex(int(got[tuple(b)])) for b in bad[:4]])
            if mask_name == "zeros":
                assert not got.any(), what
            nonzero += int((got != 0).sum())
    assert nonzero  # (the comparison was not of zeros with zeros)
    # what the words read back say about the special rows, mask none, g = 64
    got = G.members(metric, rows, q, ORDER, TASKS, 64, None)[0]
    assert not got[0].any() and not got[1].any(), "a run of the NaN row alone: all zeros"
    direct0 = len(RUNS) * 3
    assert not got[direct0].any(), "the NaN row as a direct task: all zeros"
    assert int(got[direct0 + 1, 0]) & 0xFFFFFFFF == (~R_EQ & 0xFFFFFFFF) and not got[direct0 + 1, 1:].any()
    if metric == L2M:
        assert int(got[direct0 + 1, 0]) >> 32 == L.ORD_PLUS_ZERO, "- 0.0 becomes the key of + 0.0"


@pytest.mark.gpu
@pytest.mark.parametrize("pitch4", PITCHES)
@pytest.mark.parametrize("metric", [COS, L2M])
def test_member_scores_against_float64(metric, pitch4):
    rows, q = _corpus("float", pitch4)
    tasks = np.array([(qi, r, 1, 1) for qi in range(NQ) for r in range(N_ROWS)], U32)
    got, front, back = G.members(metric, rows, q, ORDER, tasks, 1, None)
    assert np.all(front == G.SENT_KEY) and np.all(back == G.SENT_KEY)
    keys = got.reshape(NQ, N_ROWS)
    rows_of = (~keys & U64(0xFFFFFFFF)).astype(np.int64)
    assert np.all((keys == 0) | (rows_of == np.arange(N_ROWS)[None, :]))
    worst = L.check_scores64(keys, rows, q, metric, pitch4)
    print(f"metric {metric} pitch4 {pitch4}: largest error over its float64 bound {worst:.3f}")
    assert np.array_equal(keys, _keys("float", metric, pitch4)), "bit-identical to rescore_kernel"


def _lists(rng, n_lists, g, used_rows):
    """n_lists sorted lists of g keys: unique rows, scores from a small set (ties between lists, + 0.0, infinities)"""
    out = np.zeros((n_lists, g), U64)
    for i in range(n_lists):
        fill = int(rng.choice([0, 1, g // 2, g, g, g]))
        if fill == 0:
            continue
        rows = []
        while len(rows) < fill:
            r = int(rng.integers(0, 2 ** 32 - 300))
            if r not in used_rows:
                used_rows.add(r)
                rows.append(r)
        score = rng.choice(np.array([0.0, 1.5, -2.25, 3.0e-41, np.inf, -np.inf, 7.0, -7.0], F32), size=fill).astype(F32)
        score = np.where(rng.random(fill) < 0.5, score, rng.standard_normal(fill).astype(F32))
        keys = L.make_keys(L.f2ord(score + F32(0.0)), np.array(rows, U64))
        out[i, :fill] = np.sort(keys)[::-1]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("g", SIZES)
@pytest.mark.parametrize("metric", [COS, L2M])
def test_merge_every_word(metric, g):
    rng = _rng("merge", metric, g)
    per_slot = [1, 0, 2, 63, 64, 0, 65, 130, 1, 3]
    for task_base in (0, 1000):
        used = set()
        partial = _lists(rng, sum(per_slot), g, used)
        partial[0] = 0  # (a slot whose one list is empty: count 0)
        short = sum(per_slot[:8])  # (slot 8's one list holds a single key: a count between 0 and g wherever g > 1)
        partial[short] = 0
        partial[short, 0] = L.make_keys(L.f2ord(np.array([1.25], F32)), np.array([4294960000], U64))[0]
        slot_task0 = (np.concatenate([[0], np.cumsum(per_slot)]) + task_base).astype(U64)
        idx, score, count, guards = G.merge(metric, partial, slot_task0, g, task_base)
        w_idx, w_score, w_count = G.expect_merge(metric, partial, slot_task0, g, task_base)
        what = (metric, g, task_base)
        assert G.guards_intact(guards), what
        assert np.array_equal(idx, w_idx), what
        assert np.array_equal(score.view(U32), w_score.view(U32)), what  # (bits: + 0.0 is not - 0.0)
        assert np.array_equal(count, w_count), what
        for s, n in enumerate(per_slot):
            if n == 0 or s == 0:
                assert count[s] == 0 and np.all(idx[s] == -1) and not score[s].view(U32).any(), what
        assert w_count.max() == g and w_count[8] == 1
