"""ctypes loader of tests/kernel_harness/libupdate_harness.so (built by ``make -C wdbx-py_amd/csrc all``) and the array
bookkeeping of tests/test_gpu_update_kernels.py.

The harness runs the kernels behind ``wdbx_index_set_rows_at`` / ``wdbx_index_remove_rows`` -- ``update_scatter_kernel``,
``update_refresh_kernel``, ``rows_to_i8g_list_kernel`` -- (mode ``LIST``), what ``wdbx_index_set_rows`` does once per listed
row with the range quantisers (mode ``PER_ROW``), or the range quantisers over each copy's whole coverage (mode ``RANGE``),
on arrays the caller hands it.  Every copy is one numpy array with ``GUARD`` cells behind what the library would allocate;
all of them go in and come back, so a cell no kernel touched keeps what the caller put there."""
import ctypes as C
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "kernel_harness" / "update_harness.hip"
LIBRARY = ROOT / "tests" / "kernel_harness" / "libupdate_harness.so"

LIST, PER_ROW, RANGE = 0, 1, 2
GUARD = 64  # cells behind every array that no kernel may touch
COPIES = ("cn", "r16", "r8", "s8", "c6", "sa6", "h42", "sa42", "l42", "r8g", "grp", "gbad")


class UpdCase(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("dim", "pitch", "pitch16", "pitch8", "pitch8g", "normalize")] + \
               [(n, C.c_uint64) for n in ("n_rows", "round_rows", "cov_cn", "cov_16", "cov_8", "cov_6", "cov_42", "cov_g")] + \
               [(n + "_bytes", C.c_uint64) for n in ("rows",) + COPIES]


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(str(LIBRARY))
        _lib.upd_run.restype = C.c_int
        _lib.upd_run.argtypes = [C.c_int, C.POINTER(UpdCase), C.c_void_p, C.c_uint64] + [C.c_void_p] * 14 + [C.POINTER(C.c_int)]
    return _lib


def u42_lpitch(units):
    return (units * 2 + 1 + 31) // 32 * 32


class Shape:
    """The pitches and array shapes the library gives rows of ``dim`` elements, and which copies such rows can have."""

    def __init__(self, dim, n_rows):
        self.dim, self.n = dim, n_rows
        self.pitch = (dim + 3) // 4 * 4
        self.pitch16 = (self.pitch + 127) // 128 * 128
        self.pitch8 = (dim + 15) // 16 * 16
        self.pitch8g = (dim + 127) // 128 * 128
        self.tiles = (n_rows + 63) // 64
        self.has_u6 = self.pitch % 16 == 0
        self.has_u42 = self.pitch % 32 == 0
        self.units6, self.units42 = self.pitch // 16, self.pitch // 32
        self.lpitch = u42_lpitch(self.units42)

    def sizes(self):
        """name -> (dtype, cells the library's layout holds for n rows)"""
        n, t = self.n, self.tiles
        return {
            "rows": (np.float32, n * self.pitch), "cn": (np.float32, n), "r16": (np.uint16, n * self.pitch16),
            "r8": (np.uint8, n * self.pitch8), "s8": (np.float32, n), "c6": (np.uint32, t * self.units6 * 192),
            "sa6": (np.float32, n * 2), "h42": (np.uint32, t * self.units42 * 256), "sa42": (np.float32, n * 2),
            "l42": (np.uint32, n * self.lpitch), "r8g": (np.int8, t * 64 * self.pitch8g), "grp": (np.float32, t * 4),
            "gbad": (np.uint64, t),
        }

    def blank(self, byte):
        """Every copy filled with one sentinel byte, guard cells included."""
        return {name: np.frombuffer(bytes([byte]) * ((cells + GUARD) * np.dtype(dt).itemsize), dt).copy()
                for name, (dt, cells) in self.sizes().items() if name != "rows"}

    def rows_array(self, rows, byte=0xAB):
        """[n, dim] -> the flat pitch-strided array with zero pads and a guard of sentinel bytes behind it."""
        out = np.frombuffer(bytes([byte]) * ((self.n * self.pitch + GUARD) * 4), np.float32).copy()
        body = np.zeros((self.n, self.pitch), np.float32)
        body[:, :self.dim] = rows
        out[:self.n * self.pitch] = body.reshape(-1)
        return out


def run(mode, shape, coverage, rows_flat, copies, row_list=(), src=None, normalize=False, round_rows=0):
    """One harness run on COPIES of the arrays given; returns (rows_flat, copies, launches).  coverage: dict copy family
    (cn, 16, 8, 6, 42, g) -> rows covered (missing or 0: absent)."""
    c = UpdCase()
    c.dim, c.pitch, c.pitch16, c.pitch8, c.pitch8g = shape.dim, shape.pitch, shape.pitch16, shape.pitch8, shape.pitch8g
    c.normalize, c.n_rows, c.round_rows = int(normalize), shape.n, round_rows
    for fam in ("cn", "16", "8", "6", "42", "g"):
        setattr(c, "cov_" + fam, int(coverage.get(fam, 0)))
    rows_flat = rows_flat.copy()
    copies = {k: v.copy() for k, v in copies.items()}
    c.rows_bytes = rows_flat.nbytes
    for name in COPIES:
        setattr(c, name + "_bytes", copies[name].nbytes)
    ids = np.ascontiguousarray(row_list, np.uint32)
    src_arr = None if src is None else np.ascontiguousarray(src, np.float32)
    launches = C.c_int(-1)
    rc = lib().upd_run(mode, C.byref(c), ids.ctypes.data if ids.size else None, ids.size,
                       None if src_arr is None else src_arr.ctypes.data, rows_flat.ctypes.data,
                       *[copies[name].ctypes.data for name in COPIES], C.byref(launches))
    assert rc == 0, f"upd_run(mode={mode}) returned {rc}"
    return rows_flat, copies, launches.value
