"""The listed-row, label and multi-vector kernels by themselves: subset_kernel (kernels_subset.h), rowlists_kernel
(kernels_rowlists.h), label_keys_kernel and label_rank_kernel (kernels_labels.h) and multivector_rank_kernel
(kernels_multivector.h), launched by tests/kernel_harness/listed_harness.hip on arrays built here, with an explicit grid.

Through the host calls these kernels run with grids of two workgroups per CU, so on test-sized lists a wave owns 0 or 1 rows:
the stride loop, the U rows in flight with the clamped re-read of the last row, the merge of four non-trivial wave lists, a
short last query block on the key routes, register lists with a block of 4 at k <= 64 and any store outside what is read back
stay unseen.  Here every output word, the sentinels around it and a guard behind the buffer are compared with plain numpy
(tests/listed_harness.py, whose docstring derives m of the float64 bound: m = ceil(pitch4 / 64) + 8 for the inner product,
+ 10 for L2).

Instances launched -- every one the pickers can return:
  subset_kernel<METRIC, QB, NI, MODE>: METRIC cosine / L2; (MODE, QB) in (0, 1), (1, 1), (1, 4), (1, 8), (2, 1), (2, 8); NI 2, 4, 0
  rowlists_kernel<METRIC, QB, NI>:     METRIC cosine / L2; QB 1, 8; NI 2, 4, 0
  label_keys_kernel<METRIC, QB, NI>:   METRIC cosine / L2; QB 1, 8; NI 2, 4, 0
  label_rank_kernel<MODE>, multivector_rank_kernel<MODE>: MODE 0, 1, 2

Shapes, and why:
  pitch4 1, 63, 64, 65, 128 (NI 2: partial first load; second load empty, partial, full), 129, 256 (NI 4), 257, 300 (NI 0: the
  loop, ragged last trip).  Every column is filled, the reference scores the full pitch.  pitch4 = 1 of the integer corpus is
  dim = 3 (three columns of -1, 0, 1 and a constant fourth): many exact ties, the smaller row must win.
  subset: the whole cross product of grid_x 1, 2, 3; n_ids 1, UW - 1, UW, UW + 1, 2UW + 3, 101 with W = 4 grid_x and U = 4, 2, 1 by NI (no trip, a trip
  whose tail is clamped, a full trip, a second trip); ids hold row 0, the last row and from 7 entries on every special row; nq 1, qb - 1, qb, qb + 1; k 1, 63, 64, 65,
  128 in registers (both registers, their boundary), 1, 64, 129, 2048 in LDS (2048: the 64 KiB attribute); k > n_ids included;
  key_stride = n_ids + 3 (sentinels between the queries).
  rowlists: items of n = 1, 4U - 1, 4U, 4U + 1, 256 with nq 1, 7, 8, non-zero first and offset, two items of one slot on
  adjacent chunks, lists of different lengths under one stride.
  label_keys: n 1, 63, 64, 65, 64 * 9 + 5; grid_x 1, 2; one label / a label per row / runs of 1, 2, 3, 5 / a label over three
  spans; masks none, ones, zeros, every other row, each label's best row removed; nq 1, 7, 8, 9.  The longest order (the one
  with more than two spans) runs the whole cross product of layout, mask, nq and grid_x; the short ones run every (layout, mask,
  n) with the eight (nq, grid_x) pairs in turn.
  label_rank: synthetic keys with zeros, labels of 1, 2, 70 items, n_labels 1, 63, 64, 65, 256, 257, 600, grid_x 1, 2, 3.
  multivector_rank: segments of 1, 3, 4, 5, 9 vectors with v0 > 0, three ranked segments in one launch, the carry chain of
  three launches against one launch, scores 1e8, 1, -1e8 (a fold out of order shows), zero maxima (NaN for good), - 0.0.

Special rows in every scoring test: 5 holds a NaN (key 0), 6 holds + inf (as float64 says), 7 denormals, 8 equals query 0
(L2: - 0.0, the key's score half must be that of + 0.0), 9 is all - 1 and query 1 is zero.

The CPU half (no marker) gives the checkers a procedural numpy restatement of each kernel's output layout (accepted) and the
deliberately wrong restatements of WRONG (each rejected)."""
import zlib
from functools import lru_cache

import numpy as np
import pytest

import listed_harness as L
from listed_harness import METRIC_COSINE as COS, METRIC_L2 as L2M

U32, U64, F32, F64 = np.uint32, np.uint64, np.float32, np.float64
PITCHES = [1, 63, 64, 65, 128, 129, 256, 257, 300]
N_ROWS = 64 * 9 + 5
N_SUBSET_ROWS = 300
NQ = 17
R_NAN, R_INF, R_DEN, R_EQ, R_M1 = 5, 6, 7, 8, 9
SPECIAL = [R_NAN, R_INF, R_DEN, R_EQ, R_M1]
Q_ZERO = 1


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


# --------------------------------------------------------------------------- #
# inputs (built once, never changed)
# --------------------------------------------------------------------------- #
@lru_cache(maxsize=None)
def _corpus(kind, pitch4):
    rng = _rng("corpus", kind, pitch4)
    P = pitch4 * 4
    if kind == "int":
        lim = 1 if pitch4 == 1 else 4
        rows = rng.integers(-lim, lim + 1, size=(N_ROWS, P)).astype(F32)
        q = rng.integers(-lim, lim + 1, size=(NQ, P)).astype(F32)
        if pitch4 == 1:
            rows[:, 3] = 1.0
        rows[R_DEN] = (rng.integers(-4, 5, size=P).astype(F64) * 2.0 ** -149).astype(F32)
    else:
        rows = (rng.standard_normal((N_ROWS, P)) / np.sqrt(P)).astype(F32)
        q = (rng.standard_normal((NQ, P)) / np.sqrt(P)).astype(F32)
        # (two denormal elements among ordinary ones: gamma(m) * S has no underflow term, so S must stay a normal number)
        rows[R_DEN, :2] = (rng.integers(1, 1000, size=2).astype(F64) * 2.0 ** -149).astype(F32)
    q[Q_ZERO] = 0.0
    rows[R_NAN, P // 2] = np.nan
    rows[R_INF, 0] = np.inf
    rows[R_EQ] = q[0]
    rows[R_M1] = -1.0
    rows.setflags(write=False)
    q.setflags(write=False)
    return rows, q


@lru_cache(maxsize=None)
def _int_keys(metric, pitch4):
    rows, q = _corpus("int", pitch4)
    ordinary = np.setdiff1d(np.arange(N_ROWS), [R_NAN, R_INF, R_DEN])
    K = L.exact_keys(rows, q, metric, ordinary)
    assert np.all(K[:, R_NAN] == 0)
    if metric == L2M:
        assert int(K[0, R_EQ] >> U64(32)) == L.ORD_PLUS_ZERO
    K.setflags(write=False)
    return K


@lru_cache(maxsize=None)
def _float_keys(metric, pitch4):
    """rescore_kernel's keys of every (query, row) of the float corpus, checked against float64 once"""
    import select_harness as S
    rows, q = _corpus("float", pitch4)
    cand = np.broadcast_to(L.make_keys(np.zeros(N_ROWS, U32), np.arange(N_ROWS)), (NQ, N_ROWS))
    K, guard = S.rescore(metric, rows, q, cand, np.full(NQ, N_ROWS, U32), grid_x=8)
    assert np.all(guard == L.SENT_KEY)
    L.check_scores64(K, rows, q, metric, pitch4)
    K = K.copy()
    K.setflags(write=False)
    return K


def _keys(kind, metric, pitch4):
    return _int_keys(metric, pitch4) if kind == "int" else _float_keys(metric, pitch4)


def _ids(n_ids, n_rows, seed):
    """A strictly increasing list with row 0 and the last row (the clamped re-read hits the end of the rows array) and, from
    seven entries on, every special row; the others at random."""
    if n_ids == 1:
        return np.array([n_rows - 1], U32)
    fixed = [0, n_rows - 1] + (SPECIAL if n_ids >= 7 else [])
    pool = np.setdiff1d(np.arange(1, n_rows - 1), SPECIAL)
    inner = _rng("ids", seed, n_ids).choice(pool, size=n_ids - len(fixed), replace=False)
    return np.sort(np.concatenate([fixed, inner])).astype(U32)


def _special_words_of_subset(got, ids, nq, mode, k, grid_x, stride, metric):
    """What the words READ BACK say about the special rows (not only the reference): the NaN row's key is 0 (keys) or in no
    list; under L2 the key of the row equal to query 0 carries the score half of + 0.0 (keys), and it or a tie of it heads its
    workgroup's list of query 0 (no score is above - 0.0 + 0.0f)."""
    if R_NAN not in ids:
        return
    at = {r: int(np.flatnonzero(ids == r)[0]) for r in (R_NAN, R_EQ)}
    if mode == 2:
        assert all(int(got[q * stride + at[R_NAN]]) == 0 for q in range(nq)), "the NaN row's key is 0"
        if metric == L2M:
            assert int(got[at[R_EQ]]) == (L.ORD_PLUS_ZERO << 32) | (~R_EQ & 0xFFFFFFFF), "- 0.0 becomes the key of + 0.0"
        return
    words = got[:nq * k * grid_x]
    assert not np.any((words != 0) & (words & U64(0xFFFFFFFF) == U64(~R_NAN & 0xFFFFFFFF))), "the NaN row is in no list"
    if metric == L2M:
        head = int(got[at[R_EQ] % (4 * grid_x) // 4])  # (query 0, entry 0, the workgroup that owns the row)
        assert head >> 32 == L.ORD_PLUS_ZERO, "- 0.0 heads the list as + 0.0"


def _subset_n_ids(pitch4, grid_x):
    UW = L.rows_in_flight(pitch4) * 4 * grid_x
    return [1, UW - 1, UW, UW + 1, 2 * UW + 3, 101]


def _nqs(qb):
    return sorted({n for n in (1, qb - 1, qb, qb + 1) if n >= 1})


def _ks(mode):
    return {0: [1, 64, 129, 2048], 1: [1, 63, 64, 65, 128], 2: [1]}[mode]


def _rowlists_case(qb, pitch4, n_rows):
    """(ids, items, n_slots, stride): list 0 = 256 + 4U + 1 rows in two adjacent chunks, list 1 = 4U - 1 rows, list 2 = 4U,
    list 3 = one row; five unused entries in front of the id array."""
    Uf = L.rows_in_flight(pitch4)
    lens = [256 + 4 * Uf + 1, 4 * Uf - 1, 4 * Uf, 1]
    nqs = [8, 7, 1, 1] if qb == 8 else [2, 1, 1, 1]
    ids, items, first, slot = [np.full(5, n_rows - 1, U32)], [], 5, 0
    for i, (n, nq) in enumerate(zip(lens, nqs)):
        ids.append(_ids(n, n_rows, ("rowlists", i)))
        for b0 in range(0, nq, qb):
            for off in range(0, n, 256):
                items.append([first + off, min(256, n - off), slot + b0, min(qb, nq - b0), off])
        first += n
        slot += nq
    items.sort(key=lambda it: (it[0], it[2]))  # (the items of one chunk are neighbours, as the host makes them)
    return np.concatenate(ids), np.array(items, U32), slot, lens[0] + 2


LAYOUTS = ["one", "own", "runs", "three_spans"]
MASKS = ["none", "ones", "zeros", "alternate", "best_removed"]


def _labels(layout, n):
    rng = _rng("labels", layout, n)
    if layout == "one":
        return np.zeros(n, np.int64)
    if layout == "own":
        return np.arange(n)
    if layout == "runs":
        lab = np.repeat(np.arange(n), np.resize([1, 2, 3, 5], n))[:n]
    else:
        lab = np.concatenate([np.arange(10), np.full(200, 10), np.arange(11, 11 + n)])[:n]
    return lab[rng.permutation(n)]


def _mask(kind, n_rows, lo, K0):
    words = (n_rows + 31) // 32
    if kind == "none":
        return None
    if kind == "ones":
        return np.full(words, 0xFFFFFFFF, U32)
    if kind == "zeros":
        return np.zeros(words, U32)
    if kind == "alternate":
        return np.full(words, 0x55555555, U32)
    bits = np.ones(words * 32, bool)
    order = lo["order"].astype(np.int64)
    starts = np.flatnonzero(np.r_[True, lo["dense"][1:] != lo["dense"][:-1]])
    for a, b in zip(starts, np.r_[starts[1:], order.size]):
        bits[order[a:b][np.argmax(K0[order[a:b]])]] = False
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(U32).reshape(-1)


@lru_cache(maxsize=None)
def _item_keys(n_labels, V):
    """Synthetic item keys [V, key_stride] (three unused words behind the items) and label_item0: labels of 1, 2 and 70 items;
    scores from a palette on which fp32 addition does not associate, - 0.0 included; one key in nine is 0."""
    rng = _rng("items", n_labels, V)
    sizes = np.resize([1, 2, 1, 1, 70, 1, 2], n_labels)
    t = np.r_[0, np.cumsum(sizes)].astype(U32)
    n_items = int(t[-1])
    palette = np.array([1e8, 1.0, -1e8, 0.5, 3e-8, -0.0, 7.0, -1.0, 16777216.0], F32)
    scores = palette[rng.integers(0, palette.size, size=(V, n_items))]
    scores = np.where(rng.random((V, n_items)) < 0.5, scores, rng.standard_normal((V, n_items)).astype(F32))
    keys = L.make_keys(L.f2ord(scores.reshape(-1)).reshape(scores.shape), rng.integers(0, 2 ** 20, size=(V, n_items)))
    keys[rng.random((V, n_items)) < 1 / 9] = 0
    if n_labels > 2:
        keys[:, t[1]:t[2]] = 0  # (label 1: no eligible row for any vector)
    out = np.full((V, n_items + 3), L.SENT_KEY, U64)
    out[:, :n_items] = keys
    out.setflags(write=False)
    return out, t


# --------------------------------------------------------------------------- #
# procedural restatements of the kernels' output layouts (the CPU half): what each wave does, trip by trip
# --------------------------------------------------------------------------- #
WRONG = ["tail_kept", "idle_slot_writes", "tie_to_larger_row", "ownership_W_grid_x", "mask_word_row_shr_6", "item_not_advanced",
         "fold_reversed", "nan_sum_ranked"]


def _store(buf, at, v):
    if at < buf.size:  # (a wrong restatement may aim behind the guard)
        buf[at] = v


def _merged(wave_lists, k, wrong):
    """four wave lists -> the workgroup's k words (multiset top k, zeros behind)"""
    allk = [int(x) for lst in wave_lists for x in sorted(lst, reverse=True)[:k]]
    if wrong == "tie_to_larger_row":
        allk.sort(key=lambda x: (-(x >> 32), x & 0xFFFFFFFF))  # (~row ascending = row descending)
    else:
        allk.sort(reverse=True)
    return (allk + [0] * k)[:k]


def model_subset(K, ids, nq, qb, mode, k, grid_x, key_stride, Uf, wrong=None):
    buf = L.sentinel_buf(L.subset_words(mode, nq, len(ids), k, grid_x, key_stride))
    n_ids = len(ids)
    W = grid_x if wrong == "ownership_W_grid_x" else 4 * grid_x
    for q in range(-(-nq // qb) * qb):
        writes = q < nq or wrong == "idle_slot_writes"
        qq = min(q, nq - 1)
        for x in range(grid_x):
            lists = []
            for wave in range(4):
                lst, cur = [], x * 4 + wave
                while cur < n_ids:
                    for u in range(Uf):
                        idx = cur + u * W
                        live = idx < n_ids or wrong == "tail_kept"
                        key = K[qq, ids[min(idx, n_ids - 1)]] if live else 0
                        if mode == 2:
                            if live and writes:
                                _store(buf, q * key_stride + idx, key)
                        elif key:
                            lst.append(key)
                    cur += Uf * W
                lists.append(lst)
            if mode != 2 and writes:
                for i, v in enumerate(_merged(lists, k, wrong)):
                    _store(buf, q * k * grid_x + i * grid_x + x, v)
    return buf


def model_rowlists(K, ids, items, n_slots, stride, qb, Uf, wrong=None):
    buf = L.sentinel_buf(n_slots * stride)
    for first, n, slot, nq, offset in np.asarray(items, np.int64):
        for b in range(qb):
            writes = b < nq or wrong == "idle_slot_writes"
            for wave in range(4):
                for cur in range(wave, n, Uf * 4):
                    for u in range(Uf):
                        idx = cur + u * 4
                        if (idx < n or wrong == "tail_kept") and writes:
                            _store(buf, (slot + b) * stride + offset + idx, K[slot + min(b, nq - 1), ids[first + min(idx, n - 1)]])
    return buf


def model_label_keys(K, lo, mask, nq, qb, key_stride, grid_x, Uf, wrong=None):
    buf = L.sentinel_buf(nq * key_stride)
    order, dense, span_item0, n = lo["order"], lo["dense"], lo["span_item0"], lo["n"]
    for q in range(-(-nq // qb) * qb):
        writes = q < nq or wrong == "idle_slot_writes"
        qq = min(q, nq - 1)
        for span in range(lo["n_spans"]):  # (wave span % (4 grid_x) takes it; the spans are disjoint, so the order is free)
            p0, p1 = span * 64, min(span * 64 + 64, n)
            item, cur_label, best = int(span_item0[span]), dense[p0], 0
            for cur in range(p0, p1, Uf):
                for u in range(Uf):
                    if cur + u >= p1:
                        break
                    row, lab = int(order[cur + u]), dense[cur + u]
                    if lab != cur_label:
                        if writes:
                            _store(buf, q * key_stride + item, best)
                        best, cur_label = 0, lab
                        if not (wrong == "item_not_advanced" and u > 0):
                            item += 1
                    if mask is None:
                        allowed = True
                    elif wrong == "mask_word_row_shr_6":
                        allowed = (int(mask[row >> 6]) >> (row & 31)) & 1
                    else:
                        allowed = (int(mask[row >> 5]) >> (row & 31)) & 1
                    if allowed:
                        best = max(best, int(K[qq, row]))
            if writes:
                _store(buf, q * key_stride + item, best)
    return buf


def model_label_rank(item_keys, label_item0, nq, mode, k, grid_x, wrong=None):
    n_labels = len(label_item0) - 1
    buf = L.sentinel_buf(L.rank_words(mode, nq, n_labels, k, grid_x))
    stride = grid_x * (64 if wrong == "ownership_W_grid_x" else 256)
    for q in range(nq):
        for x in range(grid_x):
            lists = []
            for wave in range(4):
                lst = []
                for l0 in range((x * 4 + wave) * 64, n_labels, stride):
                    for l in range(l0, min(l0 + 64, n_labels)):
                        key = max(int(v) for v in item_keys[q, label_item0[l]:label_item0[l + 1]])
                        if mode == 2:
                            _store(buf, q * n_labels + l, key)
                        elif key:
                            lst.append(key)
                lists.append(lst)
            if mode != 2:
                for i, v in enumerate(_merged(lists, k, wrong)):
                    _store(buf, q * k * grid_x + i * grid_x + x, v)
    return buf


def _score_of(key):
    """key_score of kernels_common.h on one Python integer"""
    o = key >> 32
    u = (o ^ 0x80000000) if o & 0x80000000 else (~o & 0xFFFFFFFF)
    return np.array([u], U32).view(F32)[0]


def _key_of(score, row):
    """make_key of kernels_common.h on one float32 and one row"""
    u = int(np.array([score], F32).view(U32)[0])
    o = (~u & 0xFFFFFFFF) if u >> 31 else (u ^ 0x80000000)
    return (o << 32) | (~row & 0xFFFFFFFF)


def model_multivector(item_keys, label_item0, segs, acc, slots, mode, k, grid_x, wrong=None):
    """wave by wave, 64 labels per trip, a lane per label; four vectors' columns in flight with the clamped re-read of the
    segment's last vector (dropped), the fold in vector order"""
    n_labels = len(label_item0) - 1
    buf = L.sentinel_buf(L.rank_words(mode, slots, n_labels, k, grid_x))
    acc_out = None if acc is None else np.array(acc, F32)
    for _, v0, v1, slot, carry in np.asarray(segs, np.int64):
        carry_in, carry_out = carry & L.MV_CARRY_IN, carry & L.MV_CARRY_OUT
        for x in range(grid_x):
            lists = []
            for wave in range(4):
                lst = []
                for l0 in range((x * 4 + wave) * 64, n_labels, grid_x * 256):
                    for l in range(l0, min(l0 + 64, n_labels)):
                        i0, i1 = int(label_item0[l]), int(label_item0[l + 1])
                        terms = []
                        for v in range(v0, v1, 4):
                            best = [0, 0, 0, 0]
                            for i in range(i0, i1):
                                for u in range(4):
                                    best[u] = max(best[u], int(item_keys[min(v + u, v1 - 1), i]))
                            terms += [best[u] for u in range(4) if v + u < v1]
                        if wrong == "fold_reversed":
                            terms.reverse()
                        s = F32(acc[l]) if carry_in else F32(0.0)
                        with np.errstate(invalid="ignore", over="ignore"):
                            for b in terms:
                                s = F32(s + _score_of(b)) if b else F32(np.nan)
                        if carry_out:
                            acc_out[l] = s
                            continue
                        key = _key_of(s, l) if (s == s or wrong == "nan_sum_ranked") else 0
                        if mode == 2:
                            _store(buf, slot * n_labels + l, key)
                        elif key:
                            lst.append(key)
                lists.append(lst)
            if not carry_out and mode != 2:
                for i, v in enumerate(_merged(lists, k, wrong)):
                    _store(buf, slot * k * grid_x + i * grid_x + x, v)
    return buf, acc_out


# --------------------------------------------------------------------------- #
# the CPU half
# --------------------------------------------------------------------------- #
def _cpu_subset(wrong, pitch4=1, mode=1, qb=4, nq=3, k=5, grid_x=2, n_ids=None, metric=COS):
    K = _int_keys(metric, pitch4)
    Uf = L.rows_in_flight(pitch4)
    n_ids = 2 * Uf * 4 * grid_x + 3 if n_ids is None else n_ids
    ids = _ids(n_ids, N_SUBSET_ROWS, "cpu")
    stride = n_ids + 3
    got = model_subset(K, ids, nq, qb, mode, k, grid_x, stride, Uf, wrong)
    return L.same_words(got, L.expect_subset(K, ids, nq, mode, k, grid_x, stride), f"subset {wrong}")


def _cpu_rowlists(wrong, qb=8, pitch4=129):
    K = _int_keys(L2M, pitch4)
    ids, items, n_slots, stride = _rowlists_case(qb, pitch4, N_SUBSET_ROWS)
    got = model_rowlists(K, ids, items, n_slots, stride, qb, L.rows_in_flight(pitch4), wrong)
    return L.same_words(got, L.expect_rowlists(K, ids, items, n_slots, stride), f"rowlists {wrong}")


def _cpu_label_keys(wrong, layout="runs", mask="alternate", n=64 * 3 + 5, nq=7, qb=8, pitch4=1):
    K = _int_keys(COS, pitch4)
    lo = L.label_order(_labels(layout, n))
    m = _mask(mask, n, lo, K[0])
    stride = lo["n_items"] + 3
    got = model_label_keys(K, lo, m, nq, qb, stride, 2, L.rows_in_flight(pitch4), wrong)
    return L.same_words(got, L.expect_label_keys(K, lo, m, nq, stride), f"label_keys {wrong}")


def _cpu_label_rank(wrong, mode=1, n_labels=257, k=5, grid_x=2):
    keys, t = _item_keys(n_labels, 3)
    got = model_label_rank(keys, t, 3, mode, k, grid_x, wrong)
    return L.same_words(got, L.expect_label_rank(keys, t, 3, mode, k, grid_x), f"label_rank {wrong}")


def _mv_segs(V):
    """three ranked segments over vectors 1 .. V: 3, 4 and the rest (v0 > 0: vector 0 belongs to nobody)"""
    return np.array([[0, 1, 4, 0, 0], [1, 4, 8, 1, 0], [2, 8, V, 2, 0]], U32)


def _cpu_multivector(wrong, mode=2, n_labels=70, k=5, grid_x=2):
    keys, t = _item_keys(n_labels, 13)
    segs = _mv_segs(13)
    got, _ = model_multivector(keys, t, segs, None, 3, mode, k, grid_x, wrong)
    want, _ = L.expect_multivector(keys, t, segs, None, 3, mode, k, grid_x)
    return L.same_words(got, want, f"multivector {wrong}")


def test_restatements_are_accepted():
    for pitch4, mode, qb, nq, k in [(1, 1, 4, 5, 5), (65, 0, 1, 2, 129), (129, 2, 8, 9, 1), (257, 1, 8, 7, 64), (1, 2, 1, 1, 1)]:
        for grid_x in (1, 3):
            for metric in (COS, L2M):
                assert _cpu_subset(None, pitch4, mode, qb, nq, k, grid_x, metric=metric) is None
    assert _cpu_subset(None, n_ids=1) is None
    for qb in (1, 8):
        for pitch4 in (1, 129, 257):
            assert _cpu_rowlists(None, qb, pitch4) is None
    for layout in LAYOUTS:
        for mask in MASKS:
            for n, nq, qb in [(1, 1, 1), (65, 9, 8), (64 * 3 + 5, 7, 8)]:
                assert _cpu_label_keys(None, layout, mask, n, nq, qb) is None
    for mode in L.MODES:
        for n_labels in (1, 65, 257):
            assert _cpu_label_rank(None, mode, n_labels) is None
        assert _cpu_multivector(None, mode) is None
    # the carry chain in the restatement: out only, in and out, in and ranked = one launch over all the vectors
    keys, t = _item_keys(70, 13)
    acc = np.full(70 + 8, L.SENT_ACC, F32)
    for segs in ([[0, 1, 4, L.MV_NO_SLOT, 2]], [[0, 4, 9, L.MV_NO_SLOT, 3]], [[0, 9, 13, 0, 1]]):
        got, acc2 = model_multivector(keys, t, segs, acc, 1, 2, 1, 1)
        want, acc = L.expect_multivector(keys, t, segs, acc, 1, 2, 1, 1)
        assert L.same_words(got, want) is None and L.same_acc(acc2, acc) is None
    whole, _ = L.expect_multivector(keys, t, [[0, 1, 13, 0, 0]], None, 1, 2, 1, 1)
    assert L.same_words(got, whole) is None
    assert np.all(acc[70:].view(U32) == L.SENT_ACC.view(U32)) and np.isnan(acc[1])


@pytest.mark.parametrize("wrong", WRONG)
def test_wrong_restatement_is_rejected(wrong):
    tried = {
        "tail_kept": [lambda w: _cpu_subset(w, mode=2, qb=1, nq=1), lambda w: _cpu_subset(w, mode=1, k=64), lambda w: _cpu_rowlists(w)],
        "idle_slot_writes": [lambda w: _cpu_subset(w, mode=2, qb=8, nq=7), lambda w: _cpu_subset(w, mode=1, qb=4, nq=3),
                             lambda w: _cpu_rowlists(w), lambda w: _cpu_label_keys(w)],
        "tie_to_larger_row": [lambda w: _cpu_subset(w, pitch4=1, mode=1, k=5), lambda w: _cpu_subset(w, pitch4=1, mode=0, qb=1, nq=1, k=64)],
        "ownership_W_grid_x": [lambda w: _cpu_subset(w, mode=1, k=64), lambda w: _cpu_label_rank(w, n_labels=600, k=64)],
        "mask_word_row_shr_6": [lambda w: _cpu_label_keys(w, mask="best_removed")],  # (words that differ)
        "item_not_advanced": [_cpu_label_keys, lambda w: _cpu_label_keys(w, mask="none", pitch4=129, qb=1, nq=1)],
        "fold_reversed": [_cpu_multivector],
        "nan_sum_ranked": [_cpu_multivector, lambda w: _cpu_multivector(w, mode=1, k=64)],
    }[wrong]
    for case in tried:
        assert case(None) is None, "the right restatement of this case is accepted"
        assert case(wrong) is not None, f"{wrong}: the checkers accepted a wrong restatement"


# --------------------------------------------------------------------------- #
# the GPU half
# --------------------------------------------------------------------------- #
KINDS = ["int", "float"]
METRICS = [COS, L2M]


@pytest.mark.gpu
@pytest.mark.parametrize("pitch4", PITCHES)
@pytest.mark.parametrize("metric", METRICS)
def test_rescore_keys_meet_both_statements(metric, pitch4):
    """The anchor of the float corpora (float64 bound, checked in _float_keys) and rescore_kernel on the integer corpus: exact."""
    import select_harness as S
    K = _float_keys(metric, pitch4)
    assert np.all(K[:, R_NAN] == 0)
    if metric == L2M:
        assert int(K[0, R_EQ] >> U64(32)) == L.ORD_PLUS_ZERO
    rows, q = _corpus("int", pitch4)
    cand = np.broadcast_to(L.make_keys(np.zeros(N_ROWS, U32), np.arange(N_ROWS)), (NQ, N_ROWS))
    got, _ = S.rescore(metric, rows, q, cand, np.full(NQ, N_ROWS, U32), grid_x=8)
    assert L.same_words(got.reshape(-1), _int_keys(metric, pitch4).reshape(-1), "rescore, integer corpus") is None


@pytest.mark.gpu
@pytest.mark.parametrize("pitch4", PITCHES)
@pytest.mark.parametrize("mode,qb", L.SUBSET_PAIRS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", KINDS)
def test_subset_kernel(kind, metric, mode, qb, pitch4):
    rows, q = _corpus(kind, pitch4)
    rows = rows[:N_SUBSET_ROWS]
    K = _keys(kind, metric, pitch4)
    nqs, ks = _nqs(qb), _ks(mode)
    for grid_x in (1, 2, 3):
        for n_ids in _subset_n_ids(pitch4, grid_x):
            ids = _ids(n_ids, N_SUBSET_ROWS, (pitch4, grid_x))
            stride = n_ids + 3
            for nq in nqs:
                for k in ks:  # (the whole cross product: grid_x, n_ids, nq, k)
                    got = L.subset(metric, mode, qb, rows, q[:nq], ids, k, grid_x, stride)
                    bad = L.same_words(got, L.expect_subset(K, ids, nq, mode, k, grid_x, stride), f"grid {grid_x} n_ids {n_ids} nq {nq} k {k}")
                    assert bad is None, bad
                    _special_words_of_subset(got, ids, nq, mode, k, grid_x, stride, metric)


@pytest.mark.gpu
@pytest.mark.parametrize("pitch4", PITCHES)
@pytest.mark.parametrize("qb", L.BLOCKS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", KINDS)
def test_rowlists_kernel(kind, metric, qb, pitch4):
    rows, q = _corpus(kind, pitch4)
    K = _keys(kind, metric, pitch4)
    ids, items, n_slots, stride = _rowlists_case(qb, pitch4, N_SUBSET_ROWS)
    got = L.rowlists(metric, qb, rows[:N_SUBSET_ROWS], q[:n_slots], ids, items, stride)
    bad = L.same_words(got, L.expect_rowlists(K, ids, items, n_slots, stride), "rowlists")
    assert bad is None, bad
    # the special rows in the words read back: list 0 (slots 0 .., the first of them query 0) holds them all
    first, slots0 = int(items[0, 0]), 8 if qb == 8 else 2
    list0 = ids[first:first + 256 + 4 * L.rows_in_flight(pitch4) + 1]
    at = {r: int(np.flatnonzero(list0 == r)[0]) for r in (R_NAN, R_EQ)}
    assert all(int(got[s * stride + at[R_NAN]]) == 0 for s in range(slots0)), "the NaN row's key is 0"
    if metric == L2M:
        assert int(got[at[R_EQ]]) == (L.ORD_PLUS_ZERO << 32) | (~R_EQ & 0xFFFFFFFF), "- 0.0 becomes the key of + 0.0"


@pytest.mark.gpu
@pytest.mark.parametrize("pitch4", PITCHES)
@pytest.mark.parametrize("qb", L.BLOCKS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", KINDS)
def test_label_keys_kernel(kind, metric, qb, pitch4):
    rows, q = _corpus(kind, pitch4)
    K = _keys(kind, metric, pitch4)
    pi = PITCHES.index(pitch4)
    pairs = [(nq, grid_x) for nq in (1, 7, 8, 9) for grid_x in (1, 2)]

    def run(layout, mask, n, nq, grid_x):
        lo = L.label_order(_labels(layout, n))
        m = _mask(mask, n, lo, K[0])
        stride = lo["n_items"] + 3
        got = L.label_keys(metric, qb, rows[:n], q[:nq], lo, m, stride, grid_x)
        bad = L.same_words(got, L.expect_label_keys(K, lo, m, nq, stride), f"{layout} {mask} n {n} nq {nq} grid {grid_x}")
        assert bad is None, bad
        return got, lo, stride

    for li, layout in enumerate(LAYOUTS):
        for mi, mask in enumerate(MASKS):
            # n = 64 * 9 + 5 is the one order with more than two spans (a wave walks several, a label covers three): the whole
            # cross product of nq and grid_x there
            for nq, grid_x in pairs:
                got, lo, stride = run(layout, mask, N_ROWS, nq, grid_x)
                if mask in ("none", "ones"):  # the special rows in the words read back
                    item = {r: int(np.searchsorted(lo["item_start"], np.flatnonzero(lo["order"] == r)[0], "right")) - 1 for r in (R_NAN, R_EQ)}
                    alone = {r: lo["item_start"][item[r]] + 1 == np.append(lo["item_start"], lo["n"])[item[r] + 1] for r in item}
                    if alone[R_NAN]:
                        assert all(int(got[qq * stride + item[R_NAN]]) == 0 for qq in range(nq)), "the NaN row's key is 0"
                    if metric == L2M:
                        assert int(got[item[R_EQ]]) >> 32 == L.ORD_PLUS_ZERO, "- 0.0 + 0.0f is the best score of its item"
            # the short orders: every (layout, mask, n), the eight (nq, grid_x) pairs in turn -- for a fixed n the twenty (layout,
            # mask) pairs meet all eight, and the turn starts elsewhere for every pitch
            for ni, n in enumerate((1, 63, 64, 65)):
                run(layout, mask, n, *pairs[(li * 5 + mi + 3 * ni + pi) % 8])


@pytest.mark.gpu
@pytest.mark.parametrize("n_labels", [1, 63, 64, 65, 256, 257, 600])
@pytest.mark.parametrize("mode", L.MODES)
def test_label_rank_kernel(mode, n_labels):
    keys, t = _item_keys(n_labels, 3)
    for grid_x in (1, 2, 3):
        for k in _ks(mode):
            got = L.label_rank(mode, keys, t, k, grid_x)
            bad = L.same_words(got, L.expect_label_rank(keys, t, 3, mode, k, grid_x), f"grid {grid_x} k {k}")
            assert bad is None, bad


@pytest.mark.gpu
@pytest.mark.parametrize("n_labels", [1, 70, 300])
@pytest.mark.parametrize("mode", L.MODES)
def test_multivector_rank_kernel(mode, n_labels):
    V = 23
    keys, t = _item_keys(n_labels, V)
    acc0 = np.full(n_labels + 8, L.SENT_ACC, F32)
    for grid_x in (1, 2, 3):
        for k in _ks(mode):  # (2048 in LDS: the 64 KiB attribute; 65 and 128: the second register)
            what = f"grid {grid_x} k {k}"
            # three ranked segments, slots 0 to 2, of 3, 4 and 15 vectors; then segments of 1, 5 and 9
            for segs in (_mv_segs(V), np.array([[0, 2, 3, 2, 0], [1, 3, 8, 0, 0], [2, 8, 17, 1, 0]], U32)):
                got, _ = L.multivector_rank(mode, keys, t, segs, None, 3, k, grid_x)
                want, _ = L.expect_multivector(keys, t, segs, None, 3, mode, k, grid_x)
                bad = L.same_words(got, want, what)
                assert bad is None, bad
            # the carry chain: out only (3 vectors), in and out (5), in and ranked (9) = one launch over the 17
            acc = acc0
            for segs in ([[0, 1, 4, L.MV_NO_SLOT, 2]], [[0, 4, 9, L.MV_NO_SLOT, 3]], [[0, 9, 18, 0, 1]]):
                got, acc_got = L.multivector_rank(mode, keys, t, segs, acc, 1, k, grid_x)
                want, acc = L.expect_multivector(keys, t, segs, acc, 1, mode, k, grid_x)
                bad = L.same_words(got, want, what) or L.same_acc(acc_got, acc, what)
                assert bad is None, bad
            whole, _ = L.multivector_rank(mode, keys, t, [[0, 1, 18, 0, 0]], None, 1, k, grid_x)
            bad = L.same_words(got, whole, what + ", chain against one launch")
            assert bad is None, bad
    # a carried - 0.0 plus a score of - 0.0 stays - 0.0: this kernel has no + 0.0f.  Label 0 alone is alive in vector 5.
    planted = keys.copy()
    planted[5, :int(t[-1])] = 0
    planted[5, int(t[0]):int(t[1])] = L.make_keys(L.f2ord(F32(-0.0)), [1234])[0]
    acc = acc0.copy()
    acc[:n_labels] = -0.0
    got, _ = L.multivector_rank(mode, planted, t, [[0, 5, 6, 0, 1]], acc, 1, 1, 1)
    want, _ = L.expect_multivector(planted, t, [[0, 5, 6, 0, 1]], acc, 1, mode, 1, 1)
    bad = L.same_words(got, want, "carried -0.0, planted")
    assert bad is None, bad
    assert int(got[0]) == (int(L.f2ord(F32(-0.0))[0]) << 32) | 0xFFFFFFFF, "label 0's key carries the score half of - 0.0"
    # the same on the random keys, with a carried NaN that stays NaN
    acc[0] = np.nan
    got, _ = L.multivector_rank(mode, keys, t, [[0, 5, 6, 0, 1]], acc, 1, 1, 1)
    want, _ = L.expect_multivector(keys, t, [[0, 5, 6, 0, 1]], acc, 1, mode, 1, 1)
    bad = L.same_words(got, want, "carried -0.0")
    assert bad is None, bad


@pytest.mark.gpu
def test_harness_refuses_what_would_leave_the_arrays():
    rows, q = _corpus("int", 1)
    K = _int_keys(COS, 1)
    ids = _ids(9, N_SUBSET_ROWS, "refuse")
    with pytest.raises(ValueError):  # an id at n_rows
        L.subset(COS, 2, 1, rows[:N_SUBSET_ROWS - 1], q[:1], ids, 1, 1, 9)
    with pytest.raises(ValueError):  # key_stride < n_ids
        L.subset(COS, 2, 1, rows, q[:2], ids, 1, 1, 8)
    with pytest.raises(ValueError):  # no such instance
        L.subset(COS, 0, 8, rows, q[:2], ids, 4, 1, 0)
    with pytest.raises(ValueError):  # register lists beyond 128
        L.subset(COS, 1, 1, rows, q[:2], ids, 129, 1, 0)
    with pytest.raises(ValueError):  # first + n leaves the ids
        L.rowlists(COS, 1, rows, q[:1], ids, [[5, 5, 0, 1, 0]], 9)
    with pytest.raises(ValueError):  # offset + n leaves the stride
        L.rowlists(COS, 1, rows, q[:1], ids, [[0, 5, 0, 1, 5]], 9)
    lo = L.label_order(_labels("runs", 65))
    with pytest.raises(ValueError):  # span_item0 inconsistent with dense
        L.label_keys(COS, 1, rows[:65], q[:1], lo, None, lo["n_items"], 1, span_item0=lo["span_item0"] + U32(1))
    with pytest.raises(ValueError):  # a short mask
        L.label_keys(COS, 1, rows[:65], q[:1], lo, np.zeros(2, U32), lo["n_items"], 1)
    keys, t = _item_keys(65, 3)
    with pytest.raises(ValueError):  # label_item0 beyond the key stride
        L.label_rank(2, keys[:, :10], t, 1, 1)
    with pytest.raises(ValueError):  # v1 above the uploaded key rows
        L.multivector_rank(2, keys, t, [[0, 0, 4, 0, 0]], None, 1, 1, 1)
    acc = np.zeros(65, F32)
    with pytest.raises(ValueError):  # one segment reads acc, another writes it
        L.multivector_rank(2, keys, t, [[0, 0, 1, 0, 1], [1, 1, 3, L.MV_NO_SLOT, 2]], acc, 1, 1, 1)
    assert K.shape == (NQ, N_ROWS)
