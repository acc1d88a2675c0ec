"""ctypes loader of tests/kernel_harness/libu42_harness.so (built by ``make -C wdbx-py_amd/csrc all``) and the numpy side of the
split six-bit planes' layouts (kernels_scan42.h).

The harness launches the library's own ``rows_to_u42_kernel`` (next to ``rows_to_u6_kernel`` on the same rows) and
``scan_u42_kernel`` on arrays the caller hands it.  The planes a scan reads are arguments: what the quantiser produced, or
planes packed by hand from the numpy restatement of tests/test_selection_bounds_u42.py."""
import ctypes as C
from pathlib import Path

import numpy as np

from select_harness import GUARD, SENT_F32, SENT_KEY, SENT_U32

ROOT = Path(__file__).resolve().parent.parent
LIBRARY = ROOT / "tests" / "kernel_harness" / "libu42_harness.so"

_U8, _U32, _U64, _F32 = np.uint8, np.uint32, np.uint64, np.float32


def unit_chunk_py(units):
    """kernels_scan42.h::u42_unit_chunk restated"""
    if not units:
        return 0
    for uc in (8, 6, 4):
        if units % uc == 0:
            return uc
    return 4 if units <= 4 else 6 if units <= 6 else 8


def lpitch_py(units):
    """dwords of one l record: the remainders and a6, in whole 128-byte lines"""
    return (units * 2 + 1 + 31) // 32 * 32


# --------------------------------------------------------------------------- #
# layouts
# --------------------------------------------------------------------------- #
def pack_h(h):
    """h [n, units * 32] (0 .. 15) -> dwords [tiles][units][64][4]: dword t byte b = element 8t+b in the low nibble, element
    8t+4+b in the high one.  Rows past n in the last tile: 8 (the zero point's h)."""
    h = np.asarray(h, _U32)
    n, dimp = h.shape
    units, tiles = dimp // 32, (n + 63) // 64
    full = np.full((tiles * 64, units, 4, 2, 4), 8, _U32)
    full[:n] = h.reshape(n, units, 4, 2, 4)
    dw = np.zeros((tiles * 64, units, 4), _U32)
    for b in range(4):
        dw |= (full[:, :, :, 0, b] | (full[:, :, :, 1, b] << _U32(4))) << _U32(8 * b)
    return np.ascontiguousarray(dw.reshape(tiles, 64, units, 4).transpose(0, 2, 1, 3))


def unpack_h(dw, n):
    """the inverse of :func:`pack_h` by the scan kernel's own extraction -> [n, units * 32] uint8"""
    dw = np.asarray(dw, _U32)
    tiles, units = dw.shape[0], dw.shape[1]
    per_row = dw.transpose(0, 2, 1, 3).reshape(tiles * 64, units, 4)
    out = np.zeros((tiles * 64, units, 4, 2, 4), _U32)
    lo, hi = per_row & _U32(0x0F0F0F0F), (per_row >> _U32(4)) & _U32(0x0F0F0F0F)
    for b in range(4):
        out[:, :, :, 0, b] = (lo >> _U32(8 * b)) & _U32(0xFF)
        out[:, :, :, 1, b] = (hi >> _U32(8 * b)) & _U32(0xFF)
    return out.reshape(tiles * 64, units * 32)[:n].astype(_U8)


def pack_l(l, a6, fill=SENT_U32):
    """l [n, units * 32] (0 .. 3), a6 [n] fp32 -> records [n, lpitch] dwords: dword g of the row holds elements 16 g .. 16 g + 15,
    element 4 j + b in bits [8 b + 2 j, 8 b + 2 j + 1]; then a6's bits; the rest of the record is `fill`."""
    l = np.asarray(l, _U32)
    n, dimp = l.shape
    units = dimp // 32
    rec = np.full((n, lpitch_py(units)), fill, _U32)
    g = l.reshape(n, units * 2, 4, 4)  # [row][dword][j][b]
    dw = np.zeros((n, units * 2), _U32)
    for j in range(4):
        for b in range(4):
            dw |= g[:, :, j, b] << _U32(8 * b + 2 * j)
    rec[:, :units * 2] = dw
    rec[:, units * 2] = np.asarray(a6, _F32).view(_U32)
    return rec


def unpack_l(rec, units):
    """-> (l [n, units * 32] uint8 by the refine's own extraction, a6 bit patterns [n])"""
    rec = np.asarray(rec, _U32)
    n = rec.shape[0]
    out = np.zeros((n, units * 2, 4, 4), _U32)
    for j in range(4):
        m = (rec[:, :units * 2] >> _U32(2 * j)) & _U32(0x03030303)
        for b in range(4):
            out[:, :, j, b] = (m >> _U32(8 * b)) & _U32(0xFF)
    return out.reshape(n, units * 32).astype(_U8), rec[:, units * 2].copy()


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
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        lib.u42h_unit_chunk.argtypes = [u32]
        lib.u42h_unit_chunk.restype = C.c_int
        lib.u42h_lpitch.argtypes = [u32]
        lib.u42h_lpitch.restype = u32
        lib.u42h_quantise.argtypes = [vp, u64, u64, u64, u32, u32, u32, vp, vp, vp, vp, vp]
        lib.u42h_quantise.restype = C.c_int
        lib.u42h_scan.argtypes = [u32, u32, u32, u32, u32, u32, vp, u64, vp, vp, u64, vp, vp, vp, u64, vp, vp]
        lib.u42h_scan.restype = C.c_int
        _lib = lib
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _check(rc, what):
    if rc == -1:
        raise ValueError(f"{what}: the harness refused the arguments")
    if rc:
        raise RuntimeError(f"{what}: HIP error {rc}")


def quantise(rows, dim, r0=0, n=None, grid=0):
    """rows: [n_alloc, pitch] fp32, pitch a multiple of 32.  -> dict(h [tiles, units, 64, 4], sa4 bits [n_alloc, 2],
    lrec [n_alloc, lpitch], codes6 [tiles, units * 2, 64, 3], sa6 bits [n_alloc, 2]); what a kernel leaves alone keeps the sentinels."""
    rows = np.ascontiguousarray(rows, _F32)
    n_alloc, pitch = rows.shape
    n = n_alloc if n is None else n
    units, tiles = pitch // 32, (n_alloc + 63) // 64
    out = {"h": np.full((tiles, units, 64, 4), SENT_U32, _U32), "sa4": np.full((n_alloc, 2), SENT_F32, _U32),
           "lrec": np.full((n_alloc, lpitch_py(units)), SENT_U32, _U32), "codes6": np.full((tiles, units * 2, 64, 3), SENT_U32, _U32),
           "sa6": np.full((n_alloc, 2), SENT_F32, _U32)}
    rc = load().u42h_quantise(_ptr(rows), n_alloc, int(r0), int(n), int(dim), pitch, int(grid), _ptr(out["h"]), _ptr(out["sa4"]),
                              _ptr(out["lrec"]), _ptr(out["codes6"]), _ptr(out["sa6"]))
    _check(rc, "u42h_quantise")
    return out


def scan(h, sa4, lrec, queries, n_rows, tau, cap, grid_x):
    """One launch of scan_u42_kernel, grid (grid_x, nq).  -> dict(cand [nq, cap] uint64, guard [GUARD] -- the keys behind the
    last buffer --, count [nq], survivors [nq])."""
    h, lrec = np.ascontiguousarray(h, _U32), np.ascontiguousarray(lrec, _U32)
    sa4, queries, tau = np.ascontiguousarray(sa4, _F32), np.ascontiguousarray(queries, _F32), np.ascontiguousarray(tau, _F32)
    nq, units = queries.shape[0], h.shape[1]
    assert h.shape == ((n_rows + 63) // 64, units, 64, 4) and sa4.shape == (n_rows, 2) and lrec.shape == (n_rows, lpitch_py(units))
    assert tau.shape == (nq,)
    cand = np.full(nq * cap + GUARD, SENT_KEY, _U64)
    count, surv = np.zeros(nq, _U32), np.zeros(nq, _U32)
    rc = load().u42h_scan(int(n_rows), units, queries.shape[1], nq, int(cap), int(grid_x), _ptr(h), h.size, _ptr(sa4), _ptr(lrec), lrec.size,
                          _ptr(queries), _ptr(tau), _ptr(cand), cand.size, _ptr(count), _ptr(surv))
    _check(rc, "u42h_scan")
    return {"cand": cand[:nq * cap].reshape(nq, cap), "guard": cand[nq * cap:], "count": count, "survivors": surv}
