"""ctypes loader of tests/kernel_harness/libu42_convert_harness.so (built by ``make -C wdbx-py_amd/csrc all``): the split
six-bit planes' converts alone, kernels_scan42.h::u42_unpack8 and ::u42_rem4, one thread per dword."""
import ctypes as C
from pathlib import Path

import numpy as np

from select_harness import SENT_F32

ROOT = Path(__file__).resolve().parent.parent
LIBRARY = ROOT / "tests" / "kernel_harness" / "libu42_convert_harness.so"

_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        for f in (lib.u42c_nibbles, lib.u42c_remainders):
            f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
            f.restype = C.c_int
        _lib = lib
    return _lib


def _run(fn, dwords, per):
    dwords = np.ascontiguousarray(dwords, np.uint32)
    out = np.full((dwords.size, per), SENT_F32, np.uint32)
    rc = fn(dwords.ctypes.data_as(C.c_void_p), dwords.size, out.ctypes.data_as(C.c_void_p))
    if rc == -1:
        raise ValueError("the harness refused the arguments")
    if rc:
        raise RuntimeError(f"HIP error {rc}")
    return out


def nibbles(dwords):
    """-> bit patterns [n, 8]: element e of each h-plane dword as u42_unpack8 returns it"""
    return _run(load().u42c_nibbles, dwords, 8)


def remainders(dwords):
    """-> bit patterns [n, 16]: element 4 j + b of each l-record dword as u42_rem4 returns it"""
    return _run(load().u42c_remainders, dwords, 16)
