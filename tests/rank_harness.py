"""ctypes loader of tests/kernel_harness/librank_harness.so (built by ``make -C wdbx-py_amd/csrc all``) and the numpy side
of the 64-bit ordering keys: ``key = (f2ord(score) << 32) | ~row``, 0 = absent, bigger = better.

The harness launches the library's own ranking kernels (``merge_kernel``, ``kth_score_kernel``, the radix select chain) on
arrays the caller hands it; tests/test_gpu_rank_kernels.py compares what comes back with plain integer arithmetic."""
import ctypes as C
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "kernel_harness" / "rank_harness.hip"
LIBRARY = ROOT / "tests" / "kernel_harness" / "librank_harness.so"

METRIC_COSINE, METRIC_L2 = 0, 1
MAX_K = 2048
KTH_MAX_N = 16 * 1024  # KTH_R * 1024

_U32 = np.uint32
_U64 = np.uint64


# --------------------------------------------------------------------------- #
# keys
# --------------------------------------------------------------------------- #
def f2ord(x):
    """float32 -> uint32 whose unsigned order is the floats' order (-0.0 just below +0.0)."""
    u = np.atleast_1d(np.asarray(x, dtype=np.float32)).view(_U32)
    return np.where(u >> _U32(31) != 0, ~u, u ^ _U32(0x80000000)).astype(_U32)


def ord2f(o):
    """The inverse of :func:`f2ord`, on every bit pattern."""
    o = np.atleast_1d(np.asarray(o, dtype=_U32))
    u = np.where(o & _U32(0x80000000) != 0, o ^ _U32(0x80000000), ~o).astype(_U32)
    return u.view(np.float32)


def make_keys(ords, rows):
    """ords: uint32 ordered scores, rows: row numbers below 2^32 -> uint64 keys."""
    ords = np.asarray(ords, dtype=_U64)
    low = (~np.asarray(rows, dtype=_U64)) & _U64(0xFFFFFFFF)
    return (ords << _U64(32)) | low


def key_ord(keys):
    return (np.asarray(keys, dtype=_U64) >> _U64(32)).astype(_U32)


def key_row(keys):
    return ((~np.asarray(keys, dtype=_U64)) & _U64(0xFFFFFFFF)).astype(_U64)


# --------------------------------------------------------------------------- #
# the library
# --------------------------------------------------------------------------- #
class _RankMerge(C.Structure):
    _fields_ = [("q_stride", C.c_uint64), ("i_stride", C.c_uint64), ("p_stride", C.c_uint64), ("P", C.c_uint32),
                ("list_len", C.c_int32), ("k", C.c_int32), ("metric", C.c_int32), ("row_base", C.c_uint32),
                ("idx_base", C.c_int64), ("over_cap", C.c_uint32), ("no_fast", C.c_int32)]


_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp = C.c_void_p
        lib.rank_merge_geometry.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        lib.rank_merge.argtypes = [C.POINTER(_RankMerge), C.c_int, C.c_int, vp, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
        lib.rank_kth.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int, vp]
        lib.rank_select.argtypes = [vp, C.c_uint64, vp, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint32,
                                    C.c_int64, C.c_uint32, vp, vp, vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        for f in (lib.rank_merge_geometry, lib.rank_merge, lib.rank_kth, lib.rank_select):
            f.restype = C.c_int
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc, what):
    if rc == -1:
        raise ValueError(f"{what}: the harness refused the arguments (out of the uploaded arrays' bounds, or out of range)")
    if rc:
        raise RuntimeError(f"{what}: HIP error {rc}")


def merge_geometry(k, lds_lists=0):
    """(waves per workgroup, bytes of dynamic LDS, register-list instance?) as the library chooses them for k."""
    w, lds, reg = C.c_int(0), C.c_uint64(0), C.c_int(0)
    _check(load().rank_merge_geometry(int(k), int(lds_lists), C.byref(w), C.byref(lds), C.byref(reg)), "rank_merge_geometry")
    return w.value, lds.value, bool(reg.value)


# what the output arrays hold before the launch: a query the kernel must skip comes back with these
SENT_KEY, SENT_IDX, SENT_F32, SENT_U32 = 0xDEADBEEFDEADBEEF, -777, 0x7FC12345, 0xABABABAB


def merge(inp, nq, k, P, list_len, q_stride, i_stride, p_stride, metric=METRIC_COSINE, row_base=0, idx_base=0, P_dev=None,
          only_if_over=None, over_cap=0, no_fast=0, lds_lists=0):
    """One merge_kernel launch of nq workgroups.  Returns dict(keys [nq,k] uint64, idx [nq,k] int64, score [nq,k] uint32 bit
    patterns, kth [nq] uint32 bit patterns, over [nq] uint32)."""
    inp = np.ascontiguousarray(inp, dtype=_U64)
    d = _RankMerge(int(q_stride), int(i_stride), int(p_stride), int(P), int(list_len), int(k), int(metric), int(row_base),
                   int(idx_base), int(over_cap), int(no_fast))
    out = {"keys": np.full((nq, k), SENT_KEY, _U64), "idx": np.full((nq, k), SENT_IDX, np.int64),
           "score": np.full((nq, k), SENT_F32, _U32), "kth": np.full(nq, SENT_F32, _U32), "over": np.full(nq, SENT_U32, _U32)}
    pd = None if P_dev is None else np.ascontiguousarray(P_dev, dtype=_U32)
    oo = None if only_if_over is None else np.ascontiguousarray(only_if_over, dtype=_U32)
    assert pd is None or pd.shape == (nq,)
    assert oo is None or oo.shape == (nq,)
    rc = load().rank_merge(C.byref(d), int(lds_lists), int(nq), _ptr(inp), inp.size, _ptr(pd), _ptr(oo), _ptr(out["keys"]),
                           _ptr(out["idx"]), _ptr(out["score"]), _ptr(out["kth"]), _ptr(out["over"]))
    _check(rc, "rank_merge")
    return out


def kth(keys, n, q_stride, nq, k):
    """kth_score_kernel over keys[q * q_stride .. + n) for q < nq -> [nq] uint32 bit patterns of out_kth."""
    keys = np.ascontiguousarray(keys, dtype=_U64)
    out = np.full(nq, SENT_F32, _U32)
    _check(load().rank_kth(_ptr(keys), keys.size, int(n), int(q_stride), int(nq), int(k), _ptr(out)), "rank_kth")
    return out


def select(keys, k, metric=METRIC_COSINE, row_base=0, idx_base=0, grid=0, alt=None, count=0, cap=0):
    """The radix select chain of one query over ``keys``.  With ``alt`` (the key-per-row dump) the source is chosen on the
    device: ``keys[:count]`` when ``count <= cap``, else ``alt``."""
    keys = np.ascontiguousarray(keys, dtype=_U64)
    a = None if alt is None else np.ascontiguousarray(alt, dtype=_U64)
    out = {"keys": np.full(k, SENT_KEY, _U64), "idx": np.full(k, SENT_IDX, np.int64), "score": np.full(k, SENT_F32, _U32),
           "kth": np.full(1, SENT_F32, _U32)}
    total, cnt = C.c_uint32(0), C.c_uint32(0)
    rc = load().rank_select(_ptr(keys) if keys.size else None, keys.size, _ptr(a), 0 if a is None else a.size,
                            0 if a is None else 1, int(count), int(cap), int(k), int(metric), int(row_base), int(idx_base), int(grid),
                            _ptr(out["keys"]), _ptr(out["idx"]), _ptr(out["score"]), _ptr(out["kth"]), C.byref(total), C.byref(cnt))
    _check(rc, "rank_select")
    out["total"], out["out_count"] = total.value, cnt.value
    return out
