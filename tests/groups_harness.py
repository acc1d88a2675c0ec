"""ctypes loader of tests/kernel_harness/libgroups_harness.so (built by ``make -C wdbx-py_amd/csrc all``) and the plain numpy
restatement of the two kernels it launches, ``group_members_kernel`` and ``group_merge_kernel`` (kernels_groups.h).

The reference never looks at the code under test.  It takes K [nq, n_rows], the key of every (query, row) -- int64 arithmetic
for the integer corpora, ``rescore_kernel``'s keys (checked against float64 once, tests/listed_harness.py) for the float ones
-- and states what each kernel's whole output buffer holds:
  members: per task the ``g`` largest non-zero keys of the rows at its positions that the mask allows, descending, zeros behind;
  merge:   per slot the ``g`` largest non-zero keys over its lists, converted as merge_kernel converts a key -- row, score
           (L2: negated, - 0 + 0 = + 0), -1 / 0 in the unused member slots -- and the count of members."""
import ctypes as C
from pathlib import Path

import numpy as np

from listed_harness import key_scores, mask_allows
from select_harness import METRIC_COSINE, METRIC_L2  # noqa: F401  (re-exported)

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "kernel_harness" / "groups_harness.hip"
LIBRARY = ROOT / "tests" / "kernel_harness" / "libgroups_harness.so"

_U32, _U64, _I64, _I32, _F32 = np.uint32, np.uint64, np.int64, np.int32, np.float32
GUARD = 64
SENT_KEY = np.uint64(0xDEADBEEFCAFEF00D)
SENT_IDX = np.int64(-0x0123456789ABCDEF)
SENT_SCORE = np.array([0x4B1D4B1D], _U32).view(_F32)[0]
SENT_COUNT = np.int32(-77)
MAX_GROUP_SIZE = 64

_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        lib.groups_members.argtypes = [i32, vp, u32, u32, vp, u32, vp, u32, vp, u64, vp, u32, i32, vp, u64]
        lib.groups_members.restype = i32
        lib.groups_merge.argtypes = [i32, vp, u64, vp, u64, u32, i32, vp, vp, vp, u64]
        lib.groups_merge.restype = i32
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc, what):
    if rc == -1:
        raise ValueError(f"{what}: the harness refused the arguments")
    if rc:
        raise RuntimeError(f"{what}: HIP error {rc}")


def members(metric, rows, queries, order, tasks, g, mask=None):
    """group_members_kernel on rows / queries whose width is a multiple of 4 -> (partial [n_tasks, g], front guard, back guard)"""
    rows, queries = np.ascontiguousarray(rows, _F32), np.ascontiguousarray(queries, _F32)
    assert rows.shape[1] % 4 == 0 and rows.shape[1] == queries.shape[1]
    order = np.ascontiguousarray(order, _U32)
    tasks = np.ascontiguousarray(tasks, _U32).reshape(-1, 4)
    mask = None if mask is None else np.ascontiguousarray(mask, _U32)
    n_out = tasks.shape[0] * g
    buf = np.full(n_out + 2 * GUARD, SENT_KEY, _U64)
    rc = load().groups_members(int(metric), _ptr(rows), rows.shape[0], rows.shape[1] // 4, _ptr(queries), queries.shape[0],
                               _ptr(order), order.size, _ptr(mask), 0 if mask is None else mask.size, _ptr(tasks), tasks.shape[0],
                               int(g), _ptr(buf), GUARD)
    _check(rc, "groups_members")
    return buf[GUARD:GUARD + n_out].reshape(tasks.shape[0], g), buf[:GUARD], buf[GUARD + n_out:]


def merge(metric, partial, slot_task0, g, task_base=0):
    """group_merge_kernel -> (idx [n_slots, g], score, count [n_slots], their six guards as one tuple)"""
    partial = np.ascontiguousarray(partial, _U64).reshape(-1, g)
    slot_task0 = np.ascontiguousarray(slot_task0, _U64)
    n_slots = slot_task0.size - 1
    idx = np.full(n_slots * g + 2 * GUARD, SENT_IDX, _I64)
    score = np.full(n_slots * g + 2 * GUARD, SENT_SCORE, _F32)
    count = np.full(n_slots + 2 * GUARD, SENT_COUNT, _I32)
    rc = load().groups_merge(int(metric), _ptr(partial), partial.shape[0], _ptr(slot_task0), int(task_base), n_slots, int(g),
                             _ptr(idx), _ptr(score), _ptr(count), GUARD)
    _check(rc, "groups_merge")
    guards = (idx[:GUARD], idx[-GUARD:], score[:GUARD], score[-GUARD:], count[:GUARD], count[-GUARD:])
    return (idx[GUARD:-GUARD].reshape(n_slots, g), score[GUARD:-GUARD].reshape(n_slots, g), count[GUARD:-GUARD], guards)


def guards_intact(guards):
    return (np.all(guards[0] == SENT_IDX) and np.all(guards[1] == SENT_IDX) and np.all(guards[2].view(_U32) == SENT_SCORE.view(_U32))
            and np.all(guards[3].view(_U32) == SENT_SCORE.view(_U32)) and np.all(guards[4] == SENT_COUNT) and np.all(guards[5] == SENT_COUNT))


# --------------------------------------------------------------------------- #
# reference
# --------------------------------------------------------------------------- #
def top_keys(keys, g):
    """the g largest non-zero keys, descending, zeros behind"""
    keys = np.asarray(keys, _U64)
    best = np.sort(keys[keys != 0])[::-1][:g]
    out = np.zeros(g, _U64)
    out[:best.size] = best
    return out


def expect_members(K, order, tasks, g, mask=None):
    """K [nq, n_rows] -> [n_tasks, g]"""
    out = np.zeros((len(tasks), g), _U64)
    for t, (query, start, count, direct) in enumerate(np.asarray(tasks, np.int64).reshape(-1, 4)):
        rows = np.array([start], _U32) if direct else np.asarray(order, _U32)[start:start + count]
        keys = np.where(mask_allows(mask, rows), K[query, rows], _U64(0))
        out[t] = top_keys(keys, g)
    return out


def expect_merge(metric, partial, slot_task0, g, task_base=0):
    partial = np.asarray(partial, _U64).reshape(-1, g)
    n_slots = len(slot_task0) - 1
    idx = np.full((n_slots, g), -1, _I64)
    score = np.zeros((n_slots, g), _F32)
    count = np.zeros(n_slots, _I32)
    for s in range(n_slots):
        best = top_keys(partial[int(slot_task0[s]) - task_base:int(slot_task0[s + 1]) - task_base].reshape(-1), g)
        m = int((best != 0).sum())
        count[s] = m
        idx[s, :m] = (~best[:m] & _U64(0xFFFFFFFF)).astype(_I64)
        sc = key_scores(best[:m])
        score[s, :m] = (-sc + _F32(0.0)) if metric == METRIC_L2 else sc
    return idx, score, count
