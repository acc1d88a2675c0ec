"""ctypes loader of tests/kernel_harness/librecommend_harness.so (built by ``make -C wdbx-py_amd/csrc all``) and the plain
numpy reference of the kernel it launches, ``recommend_kernel``.

The reference never looks at the code under test: it takes a matrix ``r`` [examples, rows] of scores in the ranking domain
(int64 for the integer corpora, float32 from ``rescore_kernel`` for the float ones; NaN = the row scored NaN), folds it as
include/wdbx_hip.h states (``p`` = max over the positives, ``n`` = max over the negatives or -inf, favoured when ``p > n``),
builds every row's 64-bit key for the asked side and lays the keys out as the kernel's three modes do: a key per row, or per
workgroup the sorted k best keys of the rows its four waves walk (wave ``w`` of the grid takes rows ``w, w + W, ...``)."""
import ctypes as C
from pathlib import Path

import numpy as np

from select_harness import METRIC_COSINE, METRIC_L2  # noqa: F401  (re-exported)

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "kernel_harness" / "recommend_harness.hip"
LIBRARY = ROOT / "tests" / "kernel_harness" / "librecommend_harness.so"

_U32, _U64, _I64, _F32 = np.uint32, np.uint64, np.int64, np.float32
GUARD = 64
SENT_KEY = np.uint64(0xDEADBEEFCAFEF00D)

_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        lib.recommend_pass.argtypes = [i32, i32, i32, vp, u32, u32, vp, u32, vp, u32, vp, u64, vp, u32, i32, u32, vp, u64, u64]
        lib.recommend_pass.restype = i32
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pad4(x):
    x = np.asarray(x, _F32)
    pitch = (x.shape[1] + 3) // 4 * 4
    out = np.zeros((x.shape[0], pitch), _F32)
    out[:, :x.shape[1]] = x
    return out


def recommend_pass(metric, mode, side, rows, examples, table, k, blocks, mask=None, exclude=None):
    """recommend_kernel on padded rows / examples -> (keys, front guard, back guard); keys is [nq, n_rows] (mode 2) or
    [nq, k, blocks] (modes 0, 1)."""
    rows, examples = np.ascontiguousarray(pad4(rows)), np.ascontiguousarray(pad4(examples))
    table = np.ascontiguousarray(table, _U32).reshape(-1, 3)
    nq, n_rows = table.shape[0], rows.shape[0]
    n_out = nq * n_rows if mode == 2 else nq * k * blocks
    buf = np.full(n_out + 2 * GUARD, SENT_KEY, _U64)
    mask = None if mask is None else np.ascontiguousarray(mask, _U32)
    exclude = None if exclude is None or not len(exclude) else np.ascontiguousarray(exclude, _U32)
    rc = load().recommend_pass(int(metric), int(mode), int(side), _ptr(rows), n_rows, rows.shape[1] // 4, _ptr(examples),
                               examples.shape[0], _ptr(table), nq, _ptr(mask), 0 if mask is None else mask.size, _ptr(exclude),
                               0 if exclude is None else exclude.size, int(k), int(blocks), _ptr(buf), n_out, GUARD)
    if rc == -1:
        raise ValueError("recommend_pass: the harness refused the arguments")
    if rc:
        raise RuntimeError(f"recommend_pass: HIP error {rc}")
    keys = buf[GUARD:GUARD + n_out]
    return (keys.reshape(nq, n_rows) if mode == 2 else keys.reshape(nq, k, blocks)), buf[:GUARD], buf[GUARD + n_out:]


# --------------------------------------------------------------------------- #
# reference
# --------------------------------------------------------------------------- #
def f2ord(f):
    u = np.asarray(f, _F32).view(_U32).astype(_U64)
    return np.where(u >> np.uint64(31), u ^ np.uint64(0xFFFFFFFF), u ^ np.uint64(0x80000000))


def ord2f(o):
    o = np.asarray(o, _U64)
    u = np.where(o & np.uint64(0x80000000), o ^ np.uint64(0x80000000), o ^ np.uint64(0xFFFFFFFF))
    return u.astype(_U32).view(_F32)


def make_keys(score, rows):
    """(orderable(score) << 32) | ~row, as kernels_common.h"""
    return (f2ord(score) << np.uint64(32)) | (np.asarray(rows, _U64) ^ np.uint64(0xFFFFFFFF))


def row_keys(r, npos, side, eligible):
    """r [examples, rows] ranking-domain scores (int64, or float32 with NaN), the first npos rows of it the positives -> the
    key of every row for `side` (0 where the row emits nothing)"""
    r = np.asarray(r)
    n_rows = r.shape[1]
    if r.dtype.kind == "i":
        nan = np.zeros(n_rows, bool)
        p = r[:npos].astype(_I64).max(axis=0)
        n = r[npos:].astype(_I64).max(axis=0) if r.shape[0] > npos else np.full(n_rows, -2 ** 40, _I64)  # (stands for -inf)
        fav = p > n
        value = (p if side else -n).astype(_F32)  # (small integers: exact)
    else:
        r = r.astype(_F32)
        nan = np.isnan(r).any(axis=0)
        with np.errstate(invalid="ignore"):
            p = np.fmax.reduce(r[:npos], axis=0)
            n = np.fmax.reduce(r[npos:], axis=0) if r.shape[0] > npos else np.full(n_rows, -np.inf, _F32)
            fav = p > n
        value = ((p if side else -n) + _F32(0.0)).astype(_F32)
    emit = np.asarray(eligible, bool) & ~nan & (fav == bool(side))
    value = (value + _F32(0.0)).astype(_F32)
    return np.where(emit, make_keys(value, np.arange(n_rows)), np.uint64(0))


def lists_of(keys, k, blocks):
    """a query's keys per row -> [k, blocks]: per workgroup the k best keys of its rows, descending, 0-padded"""
    n_rows = keys.size
    W = 4 * blocks
    out = np.zeros((k, blocks), _U64)
    owner = (np.arange(n_rows) % W) // 4
    for b in range(blocks):
        mine = keys[owner == b]
        mine = np.sort(mine[mine != 0])[::-1][:k]
        out[:mine.size, b] = mine
    return out
