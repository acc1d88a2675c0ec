"""ctypes loader of tests/kernel_harness/liblisted_harness.so (built by ``make -C wdbx-py_amd/csrc all``) and the plain numpy
references of the five kernels it launches: ``subset_kernel``, ``rowlists_kernel``, ``label_keys_kernel``,
``label_rank_kernel`` and ``multivector_rank_kernel``.

The references never look at the code under test.  They are declarative: a key is a pure function of an fp32 score and a row
(``keys_of``), a list is the descending top k of the non-zero keys a workgroup owns (``top_lists``), an item key is a maximum
over a run of positions, a multi-vector sum is a float32 fold in vector order.  Every ``expect_*`` returns the WHOLE output
buffer, guard included, with the sentinel wherever the kernel must not write, so a comparison is ``np.array_equal`` on every
word (``same_words`` says where two buffers differ).

Scores.  Three statements, each strong where the others are weak:

* integer corpora: every product, difference, square and partial sum is an integer below 2^24 (or an integer multiple of
  2^-149 below 2^24 of them, for the denormal row), so every fp32 operation is exact in whatever order and the score is
  ``float32(score64)`` bit for bit (``exact_keys`` asserts the premise on the ordinary rows);
* float corpora against float64: ``|score - score64| <= gamma(m) * S`` (``score_bound64``).  m counts the roundings one term
  goes through, from the operation order kernels_aux.h states for exact_score / exact_finish: lane j accumulates quads j,
  j + 64, ... with one fma per component and quad, T = ceil(pitch4 / 64) of them (the product is not rounded on its own);
  the fold (x + y) + (z + w) is two additions deep; the xor tree 32 .. 1 is six additions; under L2 every difference c - q
  is rounded before it is squared, and a factor (1 + d)^2 counts as two.  So m = T + 8 for the inner product and T + 10 for
  L2.  S = sum |c_i q_i| for the inner product and the float64 sum itself for L2, where every term is non-negative.  Nothing
  here is tuned against an output;
* bit for bit against ``rescore_kernel`` (``select_harness.rescore``) on the same rows and queries, the equality the headers
  of the three scoring kernels claim."""
import ctypes as C
from pathlib import Path

import numpy as np

from select_harness import (GUARD, METRIC_COSINE, METRIC_L2, SENT_KEY, U, f2ord, gamma, make_keys, ord2f)  # noqa: F401  (re-exported)

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "kernel_harness" / "listed_harness.hip"
LIBRARY = ROOT / "tests" / "kernel_harness" / "liblisted_harness.so"

_U32, _U64, _F32, _F64 = np.uint32, np.uint64, np.float32, np.float64

LABEL_SPAN = 64
MV_CARRY_IN, MV_CARRY_OUT = 1, 2
MV_NO_SLOT = 0xFFFFFFFF
MAX_K = 2048
# what an accumulator entry holds before a launch (a finite float, so that "both NaN" never hides it)
SENT_ACC = np.array([0x4B1D4B1D], _U32).view(_F32)[0]
ORD_PLUS_ZERO = 0x80000000  # f2ord(+0.0)

# every (mode, qb) pair pick_subset accepts, the qb of the other pickers, the modes of the rank kernels
SUBSET_PAIRS = [(0, 1), (1, 1), (1, 4), (1, 8), (2, 1), (2, 8)]
BLOCKS = [1, 8]
MODES = [0, 1, 2]


def ni_of(pitch4):
    """The NI of the instance the pickers choose: loads per lane of a row (0 = the loop)."""
    return 2 if pitch4 <= 128 else 4 if pitch4 <= 256 else 0


def rows_in_flight(pitch4):
    """U of the three scoring kernels: rows whose loads a wave issues together."""
    return {2: 4, 4: 2, 0: 1}[ni_of(pitch4)]


# --------------------------------------------------------------------------- #
# scores and keys
# --------------------------------------------------------------------------- #
def score64(rows, queries, metric):
    """[nq, n_rows] float64 from the fp32 operands: c.q, or -(sum (c - q)^2), the direct form the exact kernels use."""
    r, q = np.asarray(rows, _F32).astype(_F64), np.asarray(queries, _F32).astype(_F64)
    with np.errstate(invalid="ignore", over="ignore"):
        if metric == METRIC_L2:
            return -np.stack([((r - qq) ** 2).sum(axis=1) for qq in q])
        return q @ r.T


def fmas_per_lane(pitch4):
    return (pitch4 + 63) // 64


def roundings(pitch4, metric):
    """m of the module docstring."""
    return fmas_per_lane(pitch4) + 2 + 6 + (2 if metric == METRIC_L2 else 0)


def score_bound64(rows, queries, metric, pitch4):
    """gamma(m) * S per (query, row)."""
    r, q = np.asarray(rows, _F32).astype(_F64), np.asarray(queries, _F32).astype(_F64)
    with np.errstate(invalid="ignore", over="ignore"):
        S = np.abs(score64(rows, queries, metric)) if metric == METRIC_L2 else np.abs(q) @ np.abs(r).T
    return gamma(roundings(pitch4, metric)) * S


def keys_of(scores, rows):
    """[.., n] float32 scores of rows [n] -> keys: 0 for a NaN score, else make_key(score + 0.0f, row)."""
    s = np.asarray(scores, _F32)
    with np.errstate(invalid="ignore"):
        k = make_keys(f2ord((s + _F32(0.0)).reshape(-1)).reshape(s.shape), np.broadcast_to(np.asarray(rows, _U64), s.shape))
    return np.where(np.isnan(s), _U64(0), k).astype(_U64)


def key_scores(keys):
    keys = np.asarray(keys, _U64)
    return ord2f((keys >> _U64(32)).astype(_U32).reshape(-1)).reshape(keys.shape)


def exact_keys(rows, queries, metric, ordinary):
    """Integer corpora: the key of every (query, row), [nq, n_rows].  ordinary: the rows whose scores must be integers below
    2^24 (the premise that makes every fp32 operation exact); the special rows are taken as float32(score64)."""
    s = score64(rows, queries, metric)
    o = s[:, ordinary]
    assert np.all(o == np.rint(o)) and np.all(np.abs(o) < 2 ** 24), "not an integer corpus"
    a = np.abs(np.asarray(rows, _F64)[ordinary])
    assert np.all(a == np.rint(a)) and (a.max() + np.abs(queries).max()) ** 2 * rows.shape[1] < 2 ** 24
    with np.errstate(over="ignore"):
        return keys_of(s.astype(_F32), np.arange(rows.shape[0]))


def check_scores64(keys, rows, queries, metric, pitch4):
    """The float64 statement on keys [nq, n_rows]: a NaN score64 <-> key 0, an infinite one <-> that infinity, a finite one
    within gamma(m) * S.  Returns the largest error over its bound (for the record)."""
    s64 = score64(rows, queries, metric)
    got = key_scores(keys).astype(_F64)
    nan, inf = np.isnan(s64), np.isinf(s64)
    assert np.array_equal(np.asarray(keys) == 0, nan), "key 0 exactly where the float64 score is NaN"
    assert np.array_equal(got[inf], s64[inf]), "an infinite score keeps its sign"
    fin = ~nan & ~inf
    err, bound = np.abs(got[fin] - s64[fin]), score_bound64(rows, queries, metric, pitch4)[fin]
    worst = np.flatnonzero(err > bound)
    assert worst.size == 0, f"{worst.size} scores off their float64 bound, first: err {err[worst[0]]:g} > {bound[worst[0]]:g}"
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def mask_allows(mask, rows):
    """bit r of the word array: 1 = row r may be returned (null mask: every row)"""
    rows = np.asarray(rows, _U32)
    if mask is None:
        return np.ones(rows.shape, bool)
    return ((np.asarray(mask, _U32)[rows >> _U32(5)] >> (rows & _U32(31))) & _U32(1)).astype(bool)


# --------------------------------------------------------------------------- #
# label orders (inputs, built by sorting (label, row))
# --------------------------------------------------------------------------- #
def label_order(labels):
    """labels [n] -> dict(order, dense, span_item0, label_item0, item_label, n_items, n_labels, n_spans): positions sorted by
    (label, row); an item is a maximal run of one label inside one span of 64 positions, numbered in position order."""
    labels = np.asarray(labels, np.int64)
    n = labels.size
    order = np.lexsort((np.arange(n), labels)).astype(_U32)
    lab = labels[order]
    new_label = np.ones(n, bool)
    new_label[1:] = lab[1:] != lab[:-1]
    dense = (np.cumsum(new_label) - 1).astype(_U32)
    new_span = np.arange(n) % LABEL_SPAN == 0
    new_item = new_label | new_span
    item = np.cumsum(new_item) - 1
    n_items, n_labels, n_spans = int(item[-1]) + 1, int(dense[-1]) + 1, (n + LABEL_SPAN - 1) // LABEL_SPAN
    span_item0 = np.append(item[new_span], n_items).astype(_U32)
    label_item0 = np.append(item[new_label], n_items).astype(_U32)
    return {"order": order, "dense": dense, "span_item0": span_item0, "label_item0": label_item0, "item_start": np.flatnonzero(new_item),
            "n": n, "n_items": n_items, "n_labels": n_labels, "n_spans": n_spans}


# --------------------------------------------------------------------------- #
# references: the whole output buffer of each kernel
# --------------------------------------------------------------------------- #
def top_lists(keys, owner, grid_x, k):
    """keys [n] of the entries, owner [n] = the workgroup of each -> [k, grid_x]: column x = the descending top k of workgroup
    x's non-zero keys, zeros behind."""
    out = np.zeros((k, grid_x), _U64)
    for x in range(grid_x):
        mine = keys[(owner == x) & (keys != 0)]
        mine = np.sort(mine)[::-1][:k]
        out[:mine.size, x] = mine
    return out


def entry_owner(n, grid_x):
    """subset_kernel: wave w of the grid takes list entries w, w + 4 grid_x, ...; four waves to a workgroup"""
    return (np.arange(n) % (4 * grid_x)) // 4


def label_owner(n_labels, grid_x):
    """the rank kernels: a wave takes 64 consecutive labels per trip"""
    return ((np.arange(n_labels) // 64) % (4 * grid_x)) // 4


def sentinel_buf(words):
    return np.full(words + GUARD, SENT_KEY, _U64)


def subset_words(mode, nq, n_ids, k, grid_x, key_stride):
    return nq * key_stride if mode == 2 else nq * k * grid_x


def expect_subset(K, ids, nq, mode, k, grid_x, key_stride):
    """K [>= nq, n_rows] the key of every (query, row)."""
    ids = np.asarray(ids, np.int64)
    buf = sentinel_buf(subset_words(mode, nq, ids.size, k, grid_x, key_stride))
    owner = entry_owner(ids.size, grid_x)
    for q in range(nq):
        if mode == 2:
            buf[q * key_stride:q * key_stride + ids.size] = K[q, ids]
        else:
            buf[q * k * grid_x:(q + 1) * k * grid_x] = top_lists(K[q, ids], owner, grid_x, k).reshape(-1)
    return buf


def expect_rowlists(K, ids, items, n_slots, stride):
    """K [n_slots, n_rows] the key of every (slot's query, row); items [n, 5] = first, n, slot, nq, offset."""
    buf = sentinel_buf(n_slots * stride)
    ids = np.asarray(ids, np.int64)
    for first, n, slot, nq, offset in np.asarray(items, np.int64):
        for b in range(nq):
            at = (slot + b) * stride + offset
            buf[at:at + n] = K[slot + b, ids[first:first + n]]
    return buf


def expect_label_keys(K, lo, mask, nq, key_stride):
    """K [>= nq, n_rows]; lo: a label_order.  Item i of query q = the largest key among the item's allowed rows."""
    buf = sentinel_buf(nq * key_stride)
    order = lo["order"].astype(np.int64)
    allowed = mask_allows(mask, order)
    for q in range(nq):
        kp = np.where(allowed, K[q, order], _U64(0))
        buf[q * key_stride:q * key_stride + lo["n_items"]] = np.maximum.reduceat(kp, lo["item_start"])
    return buf


def label_best(item_keys, label_item0):
    """item_keys [.., >= n_items] -> [.., n_labels]: the largest key over each label's consecutive items (every label has one)"""
    t = np.asarray(label_item0, np.int64)
    assert np.all(t[1:] > t[:-1])
    return np.maximum.reduceat(np.asarray(item_keys, _U64)[..., :t[-1]], t[:-1], axis=-1)


def rank_words(mode, slots, n_labels, k, grid_x):
    return slots * n_labels if mode == 2 else slots * k * grid_x


def expect_label_rank(item_keys, label_item0, nq, mode, k, grid_x):
    n_labels = len(label_item0) - 1
    buf = sentinel_buf(rank_words(mode, nq, n_labels, k, grid_x))
    best = label_best(item_keys[:nq], label_item0)
    owner = label_owner(n_labels, grid_x)
    for q in range(nq):
        if mode == 2:
            buf[q * n_labels:(q + 1) * n_labels] = best[q]
        else:
            buf[q * k * grid_x:(q + 1) * k * grid_x] = top_lists(best[q], owner, grid_x, k).reshape(-1)
    return buf


def fold_f32(best, start):
    """best [V, n_labels] keys in vector order, start [n_labels] float32 -> the float32 sum, one vector at a time; a zero key
    makes it NaN for good."""
    s = np.array(start, _F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in range(best.shape[0]):
            s = np.where(best[v] != 0, (s + key_scores(best[v])).astype(_F32), _F32(np.nan)).astype(_F32)
    return s


def expect_multivector(item_keys, label_item0, segs, acc, slots, mode, k, grid_x):
    """item_keys [V, >= n_items]; segs [n, 5] = query, v0, v1, slot, carry; acc: the accumulator before the launch (sentinels
    behind n_labels) or None.  Returns (out buffer, acc afterwards).  The key of a ranked label is make_key(sum, label) with NO
    + 0.0f (the sum starts from + 0.0f, so only a carried - 0.0 could show), 0 for a NaN sum."""
    n_labels = len(label_item0) - 1
    buf = sentinel_buf(rank_words(mode, slots, n_labels, k, grid_x))
    acc_out = None if acc is None else np.array(acc, _F32)
    best = label_best(item_keys, label_item0)
    owner = label_owner(n_labels, grid_x)
    for _, v0, v1, slot, carry in np.asarray(segs, np.int64):
        start = acc[:n_labels] if carry & MV_CARRY_IN else np.zeros(n_labels, _F32)
        s = fold_f32(best[v0:v1], start)
        if carry & MV_CARRY_OUT:
            acc_out[:n_labels] = s
            continue
        keys = np.where(np.isnan(s), _U64(0), make_keys(f2ord(s), np.arange(n_labels))).astype(_U64)
        if mode == 2:
            buf[slot * n_labels:(slot + 1) * n_labels] = keys
        else:
            buf[slot * k * grid_x:(slot + 1) * k * grid_x] = top_lists(keys, owner, grid_x, k).reshape(-1)
    return buf, acc_out


# --------------------------------------------------------------------------- #
# checkers
# --------------------------------------------------------------------------- #
def same_words(got, want, what=""):
    """Every word of the buffer, guard included.  Returns None when equal, else a description of the first difference."""
    got, want = np.asarray(got, _U64), np.asarray(want, _U64)
    if got.shape != want.shape:
        return f"{what}: {got.shape} words, not {want.shape}"
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    i = int(bad[0])
    where = "guard" if i >= got.size - GUARD else "word"
    return f"{what}: {bad.size} words differ, first {where} {i}: {int(got[i]):#018x}, not {int(want[i]):#018x}"


def same_acc(got, want, what=""):
    """float32 accumulators: bit-equal, or NaN on both sides."""
    got, want = np.asarray(got, _F32), np.asarray(want, _F32)
    ok = (got.view(_U32) == want.view(_U32)) | (np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(~ok)
    if bad.size == 0:
        return None
    i = int(bad[0])
    return f"{what}: {bad.size} accumulator entries differ, first {i}: {got[i]!r}, not {want[i]!r}"


# --------------------------------------------------------------------------- #
# the library
# --------------------------------------------------------------------------- #
_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        lib.listed_subset.argtypes = [i32, i32, i32, vp, u64, u32, vp, u32, vp, u32, vp, u64, u64, i32, u32]
        lib.listed_rowlists.argtypes = [i32, i32, vp, u64, u32, vp, u32, vp, u64, vp, u32, vp, u64, u64, u32]
        lib.listed_label_keys.argtypes = [i32, i32, vp, u64, u32, vp, u32, vp, vp, u32, vp, u64, vp, u64, vp, u64, u64, u32]
        lib.listed_label_rank.argtypes = [i32, vp, u64, u64, u32, vp, u32, vp, u64, i32, u32]
        lib.listed_multivector_rank.argtypes = [i32, vp, u64, u64, u32, vp, u32, vp, u32, vp, u64, vp, u64, i32, u32]
        for f in (lib.listed_subset, lib.listed_rowlists, lib.listed_label_keys, lib.listed_label_rank, lib.listed_multivector_rank):
            f.restype = C.c_int
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc, what):
    if rc == -1:
        raise ValueError(f"{what}: the harness refused the arguments (out of the uploaded arrays' bounds, or no such instance)")
    if rc:
        raise RuntimeError(f"{what}: HIP error {rc}")


def _c(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _quads(a):
    a = _c(a, _F32)
    assert a.ndim == 2 and a.shape[1] % 4 == 0
    return a, a.shape[1] // 4


def subset(metric, mode, qb, rows, queries, ids, k, grid_x, key_stride=0, words=None):
    """subset_kernel on queries [nq, pitch] -> the whole buffer, sentinels where the kernel did not write, guard behind."""
    (rows, p4), (queries, qp4), ids = _quads(rows), _quads(queries), _c(ids, _U32)
    assert p4 == qp4
    nq = queries.shape[0]
    buf = sentinel_buf(subset_words(mode, nq, ids.size, k, grid_x, key_stride) if words is None else words)
    rc = load().listed_subset(int(metric), int(mode), int(qb), _ptr(rows), rows.shape[0], p4, _ptr(queries), nq, _ptr(ids), ids.size,
                              _ptr(buf), buf.size, int(key_stride), int(k), int(grid_x))
    _check(rc, "listed_subset")
    return buf


def rowlists(metric, qb, rows, queries, ids, items, stride, words=None, grid_x=None):
    """rowlists_kernel on queries [n_slots, pitch], items [n, 5] = first, n, slot, nq, offset -> the whole key buffer."""
    (rows, p4), (queries, qp4), ids, items = _quads(rows), _quads(queries), _c(ids, _U32), _c(items, _U32)
    assert p4 == qp4 and items.ndim == 2 and items.shape[1] == 5
    n_slots = queries.shape[0]
    buf = sentinel_buf(n_slots * stride if words is None else words)
    rc = load().listed_rowlists(int(metric), int(qb), _ptr(rows), rows.shape[0], p4, _ptr(queries), n_slots, _ptr(ids), ids.size,
                                _ptr(items), items.shape[0], _ptr(buf), buf.size, int(stride),
                                items.shape[0] if grid_x is None else int(grid_x))
    _check(rc, "listed_rowlists")
    return buf


def label_keys(metric, qb, rows, queries, lo, mask, key_stride, grid_x, words=None, span_item0=None):
    """label_keys_kernel on queries [nq, pitch] over the label order lo -> the whole item key buffer."""
    (rows, p4), (queries, qp4), mask = _quads(rows), _quads(queries), _c(mask, _U32)
    assert p4 == qp4
    nq = queries.shape[0]
    order, dense = _c(lo["order"], _U32), _c(lo["dense"], _U32)
    span = _c(lo["span_item0"] if span_item0 is None else span_item0, _U32)
    buf = sentinel_buf(nq * key_stride if words is None else words)
    rc = load().listed_label_keys(int(metric), int(qb), _ptr(rows), rows.shape[0], p4, _ptr(queries), nq, _ptr(order), _ptr(dense),
                                  order.size, _ptr(span), span.size, _ptr(mask), 0 if mask is None else mask.size, _ptr(buf),
                                  buf.size, int(key_stride), int(grid_x))
    _check(rc, "listed_label_keys")
    return buf


def label_rank(mode, item_keys, label_item0, k, grid_x, words=None):
    """label_rank_kernel on item_keys [nq, key_stride] -> the whole output buffer."""
    item_keys, t = _c(item_keys, _U64), _c(label_item0, _U32)
    nq, key_stride = item_keys.shape
    buf = sentinel_buf(rank_words(mode, nq, t.size - 1, k, grid_x) if words is None else words)
    rc = load().listed_label_rank(int(mode), _ptr(item_keys), item_keys.size, key_stride, nq, _ptr(t), t.size - 1, _ptr(buf), buf.size,
                                  int(k), int(grid_x))
    _check(rc, "listed_label_rank")
    return buf


def multivector_rank(mode, item_keys, label_item0, segs, acc, slots, k, grid_x, words=None):
    """multivector_rank_kernel on item_keys [V, key_stride], segs [n, 5] = query, v0, v1, slot, carry -> (the whole output buffer,
    acc afterwards).  acc (or None) is copied: the caller's stays as it was."""
    item_keys, t, segs = _c(item_keys, _U64), _c(label_item0, _U32), _c(segs, _U32)
    assert segs.ndim == 2 and segs.shape[1] == 5
    V, key_stride = item_keys.shape
    acc = None if acc is None else np.array(acc, _F32)
    buf = sentinel_buf(rank_words(mode, slots, t.size - 1, k, grid_x) if words is None else words)
    rc = load().listed_multivector_rank(int(mode), _ptr(item_keys), item_keys.size, key_stride, V, _ptr(t), t.size - 1, _ptr(segs),
                                        segs.shape[0], _ptr(acc), 0 if acc is None else acc.size, _ptr(buf), buf.size, int(k), int(grid_x))
    _check(rc, "listed_multivector_rank")
    return buf, acc
