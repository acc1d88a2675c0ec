"""ctypes loader of tests/kernel_harness/libmatrix_harness.so (built by ``make -C wdbx-py_amd/csrc all``) and the layout half
of the reference of the kernel it launches, ``matrix_kernel``: from a matrix ``r`` [anchors, listed rows] of scores (float32,
NaN = scored NaN; the tests take it from ``rescore_kernel``) the key of every (anchor, listed row) -- 0 at the anchor's own
list position and where the score is NaN -- laid out as the kernel's sinks do: a key per listed row, or per workgroup the
sorted k best keys of the listed rows its four waves walk (wave ``w`` of the grid takes list positions ``w, w + W, ...``)."""
import ctypes as C
from pathlib import Path

import numpy as np

from recommend_harness import METRIC_COSINE, METRIC_L2, lists_of, make_keys, ord2f, pad4  # noqa: F401  (re-exported)

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "kernel_harness" / "matrix_harness.hip"
LIBRARY = ROOT / "tests" / "kernel_harness" / "libmatrix_harness.so"

_U32, _U64, _F32 = np.uint32, np.uint64, np.float32
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
        lib.matrix_pass.argtypes = [i32, i32, i32, vp, u32, u32, vp, u32, u32, u32, i32, u32, vp, u64, u64]
        lib.matrix_pass.restype = i32
        _lib = lib
    return _lib


def matrix_pass(metric, mode, qb, rows, ids, first, na, k, blocks):
    """matrix_kernel on padded rows for the anchors at list positions [first, first + na) -> (keys, front guard, back guard);
    keys is [na, n_ids] (mode 2) or [na, k, blocks] (modes 0, 1)."""
    rows = np.ascontiguousarray(pad4(rows))
    ids = np.ascontiguousarray(ids, _U32)
    n_out = na * ids.size if mode == 2 else na * k * blocks
    buf = np.full(n_out + 2 * GUARD, SENT_KEY, _U64)
    rc = load().matrix_pass(int(metric), int(mode), int(qb), rows.ctypes.data_as(C.c_void_p), rows.shape[0], rows.shape[1] // 4,
                            ids.ctypes.data_as(C.c_void_p), ids.size, int(first), int(na), int(k), int(blocks),
                            buf.ctypes.data_as(C.c_void_p), n_out, GUARD)
    if rc == -1:
        raise ValueError("matrix_pass: the harness refused the arguments")
    if rc:
        raise RuntimeError(f"matrix_pass: HIP error {rc}")
    keys = buf[GUARD:GUARD + n_out]
    return (keys.reshape(na, ids.size) if mode == 2 else keys.reshape(na, k, blocks)), buf[:GUARD], buf[GUARD + n_out:]


def pair_keys(r, ids):
    """r [n_ids, n_ids] scores of listed row j against anchor i -> the keys [n_ids, n_ids]: 0 on the diagonal (self, by list
    position) and where the score is NaN"""
    r = np.asarray(r, _F32)
    ids = np.asarray(ids, _U64)
    keys = make_keys((r + _F32(0.0)).astype(_F32), np.broadcast_to(ids, r.shape))
    keys = np.where(np.isnan(r), np.uint64(0), keys)
    keys[np.arange(ids.size), np.arange(ids.size)] = 0
    return keys.astype(_U64)
