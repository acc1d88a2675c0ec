"""ctypes loader of tests/kernel_harness/libu42_mfma_harness.so (built by ``make -C wdbx-py_amd/csrc all``): the library's own
``u42_query_i16_kernel`` and one launch of ``scan_u42_mfma_kernel`` -- 16 queries per read of the four-bit plane on the matrix
cores -- on planes, thresholds and a capacity the caller hands it (kernels_scan42.h).  The planes come from
tests/u42_share_harness.py."""
import ctypes as C
from pathlib import Path

import numpy as np

from select_harness import GUARD, SENT_KEY, SENT_U32
from u42_harness import lpitch_py

ROOT = Path(__file__).resolve().parent.parent
LIBRARY = ROOT / "tests" / "kernel_harness" / "libu42_mfma_harness.so"

_U32, _U64, _F32 = np.uint32, np.uint64, np.float32
QC_FIELDS = ("dp", "qsum305", "qsum32", "q2", "round1", "e2", "delta")  # then the flags word
MARKED, ABSENT = 1, 2

_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        lib.u42m_has_instance.argtypes = [u32]
        lib.u42m_has_instance.restype = C.c_int
        lib.u42m_scan.argtypes = [u32, u32, u32, u32, u32, u32, vp, u64, vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp]
        lib.u42m_scan.restype = C.c_int
        _lib = lib
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def has_instance(units):
    return bool(load().u42m_has_instance(int(units)))


def scan(planes, queries, n_rows, tau, cap, grid_x):
    """u42_query_i16_kernel, then one launch with grid (grid_x, ceil(nq / 16)).  -> dict(cand [nq, cap] uint64, guard [GUARD],
    count [nq], survivors [nq], surv_p [nq, n_rows] dwords (SENT_U32 where no survivor entry was made), bytes [nq, 2, dimp]
    int8 (H, L of every query, read back from the fragments), qc: dict of [groups * 16] arrays)"""
    h, lrec = np.ascontiguousarray(planes["h"], _U32), np.ascontiguousarray(planes["lrec"], _U32)
    sa4 = np.ascontiguousarray(planes["sa4"], _F32)
    queries, tau = np.ascontiguousarray(queries, _F32), np.ascontiguousarray(tau, _F32)
    nq, units = queries.shape[0], h.shape[1]
    assert h.shape == ((n_rows + 63) // 64, units, 64, 4) and sa4.shape == (n_rows, 2) and lrec.shape == (n_rows, lpitch_py(units))
    assert tau.shape == (nq,)
    groups, chunks = (nq + 15) // 16, (units + 3) // 4
    cand = np.full(nq * cap + GUARD, SENT_KEY, _U64)
    count, surv = np.zeros(nq, _U32), np.zeros(nq, _U32)
    surv_p = np.full((nq, n_rows), SENT_U32, _U32)
    qb = np.full((groups, chunks, 2, 2, 4, 16, 4), SENT_U32, _U32)  # [group][chunk][parity][H, L][kg][col][t]
    qc = np.full((groups * 16, 8), SENT_U32, _U32)
    rc = load().u42m_scan(int(n_rows), units, queries.shape[1], nq, int(cap), int(grid_x), _ptr(h), h.size, _ptr(sa4), _ptr(lrec),
                          lrec.size, _ptr(queries), _ptr(tau), _ptr(cand), cand.size, _ptr(count), _ptr(surv), _ptr(surv_p), _ptr(qb),
                          qb.size, _ptr(qc))
    if rc == -1:
        raise ValueError("u42m_scan: the harness refused the arguments")
    if rc:
        raise RuntimeError(f"u42m_scan: HIP error {rc}")
    # element 32 (4 chunk + kg) + 8 t + 4 parity + b = byte b of dword t
    by = qb.view(np.int8).reshape(groups, chunks, 2, 2, 4, 16, 4, 4)             # [g][c][par][hl][kg][col][t][b]
    by = by.transpose(0, 5, 3, 1, 4, 6, 2, 7).reshape(groups * 16, 2, chunks * 128)  # [g][col][hl][c][kg][t][par][b]
    consts = {name: qc[:, i].view(_F32).copy() for i, name in enumerate(QC_FIELDS)}
    consts["flags"] = qc[:, 7].copy()
    return {"cand": cand[:nq * cap].reshape(nq, cap), "guard": cand[nq * cap:], "count": count, "survivors": surv, "surv_p": surv_p,
            "bytes": by[:, :, :units * 32], "pad_bytes": by[:, :, units * 32:], "qc": consts}
