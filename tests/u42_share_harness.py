"""ctypes loader of tests/kernel_harness/libu42_share_harness.so (built by ``make -C wdbx-py_amd/csrc all``): the library's own
``rows_to_u42_kernel`` and one launch of ``scan_u42_kernel<UC, QP>`` -- QP = 1, 2 or 4 queries per read of the four-bit plane --
on planes, thresholds and a capacity the caller hands it (kernels_scan42.h)."""
import ctypes as C
from pathlib import Path

import numpy as np

from select_harness import GUARD, SENT_F32, SENT_KEY, SENT_U32
from u42_harness import lpitch_py

ROOT = Path(__file__).resolve().parent.parent
LIBRARY = ROOT / "tests" / "kernel_harness" / "libu42_share_harness.so"

_U32, _U64, _F32 = np.uint32, np.uint64, np.float32

_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        lib.u42sh_quantise.argtypes = [vp, u64, u32, u32, vp, vp, vp]
        lib.u42sh_quantise.restype = C.c_int
        lib.u42sh_scan.argtypes = [u32, u32, u32, u32, u32, u32, u32, vp, u64, vp, vp, u64, vp, vp, vp, u64, vp, vp]
        lib.u42sh_scan.restype = C.c_int
        _lib = lib
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _check(rc, what):
    if rc == -1:
        raise ValueError(f"{what}: the harness refused the arguments")
    if rc:
        raise RuntimeError(f"{what}: HIP error {rc}")


def quantise(rows, dim):
    """rows: [n, pitch] fp32, pitch a multiple of 32 -> dict(h [tiles, units, 64, 4] dwords, sa4 [n, 2] fp32, lrec [n, lpitch]
    dwords) as rows_to_u42_kernel leaves them"""
    rows = np.ascontiguousarray(rows, _F32)
    n, pitch = rows.shape
    units, tiles = pitch // 32, (n + 63) // 64
    h = np.full((tiles, units, 64, 4), SENT_U32, _U32)
    sa4 = np.full((n, 2), SENT_F32, _U32)
    lrec = np.full((n, lpitch_py(units)), SENT_U32, _U32)
    _check(load().u42sh_quantise(_ptr(rows), n, int(dim), pitch, _ptr(h), _ptr(sa4), _ptr(lrec)), "u42sh_quantise")
    return {"h": h, "sa4": sa4.view(_F32), "lrec": lrec}


def scan(planes, queries, n_rows, tau, cap, grid_x, qp):
    """One launch of scan_u42_kernel<UC, qp>, grid (grid_x, nq / qp).  -> dict(cand [nq, cap] uint64, guard [GUARD] -- the keys
    behind the last buffer --, count [nq], survivors [nq])."""
    h, lrec = np.ascontiguousarray(planes["h"], _U32), np.ascontiguousarray(planes["lrec"], _U32)
    sa4 = np.ascontiguousarray(planes["sa4"], _F32)
    queries, tau = np.ascontiguousarray(queries, _F32), np.ascontiguousarray(tau, _F32)
    nq, units = queries.shape[0], h.shape[1]
    assert h.shape == ((n_rows + 63) // 64, units, 64, 4) and sa4.shape == (n_rows, 2) and lrec.shape == (n_rows, lpitch_py(units))
    assert tau.shape == (nq,) and nq % qp == 0
    cand = np.full(nq * cap + GUARD, SENT_KEY, _U64)
    count, surv = np.zeros(nq, _U32), np.zeros(nq, _U32)
    rc = load().u42sh_scan(int(n_rows), units, queries.shape[1], nq, int(qp), int(cap), int(grid_x), _ptr(h), h.size, _ptr(sa4), _ptr(lrec),
                           lrec.size, _ptr(queries), _ptr(tau), _ptr(cand), cand.size, _ptr(count), _ptr(surv))
    _check(rc, "u42sh_scan")
    return {"cand": cand[:nq * cap].reshape(nq, cap), "guard": cand[nq * cap:], "count": count, "survivors": surv}
