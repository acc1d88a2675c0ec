"""ctypes loader of tests/kernel_harness/libdiscover_harness.so (built by ``make -C wdbx-py_amd/csrc all``) and the layout
half of the reference of the two kernels it launches, ``discover_kernel`` and ``discover_zone_kernel``.  The fold itself is
tests/discover_reference.py (numpy float32 in the contract's order); here its results become what the kernels write: a key
per row, target mode's records (key, wins byte, counts per wins value), or per workgroup the sorted k best keys of the rows
its four waves walk -- ``discover_kernel``: wave ``w`` of the grid takes rows ``w, w + W, ...``; ``discover_zone_kernel``:
the 64-row chunks ``w, w + W, ...``."""
import ctypes as C
from pathlib import Path

import numpy as np

import discover_reference as DR
from recommend_harness import METRIC_COSINE, METRIC_L2, lists_of, make_keys, ord2f, pad4  # noqa: F401  (re-exported)

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "kernel_harness" / "discover_harness.hip"
LIBRARY = ROOT / "tests" / "kernel_harness" / "libdiscover_harness.so"

_U8, _U32, _U64, _I64, _F32 = np.uint8, np.uint32, np.uint64, np.int64, np.float32
GUARD = 64
SENT_KEY = np.uint64(0xDEADBEEFCAFEF00D)
SENT_BYTE = np.uint8(0xA5)
ZONES = DR.ZONES

_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        lib.discover_pass.argtypes = [i32, i32, vp, u32, u32, vp, u32, vp, u32, vp, u64, vp, u32, i32, u32, vp, u64, vp, vp, u64]
        lib.discover_pass.restype = i32
        lib.discover_zone_pass.argtypes = [i32, vp, vp, u32, u32, vp, u32, i32, u32, vp, u64, u64]
        lib.discover_zone_pass.restype = i32
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raise(rc, what):
    if rc == -1:
        raise ValueError(f"{what}: the harness refused the arguments")
    if rc:
        raise RuntimeError(f"{what}: HIP error {rc}")


def discover_pass(metric, mode, rows, vectors, table, k, blocks, mask=None, exclude=None, counts_in=None):
    """discover_kernel on padded rows / vectors; table [nq][2] {first staged vector, pairs}.  Modes 0, 1 -> (keys [nq, k,
    blocks], front, back); mode 2 -> (keys [nq, n_rows], front, back); mode 3 -> (keys [nq, n_rows], wins [nq, n_rows], counts
    [nq, 33], guards) with guards = (key front, key back, wins front, wins back); the counts start from counts_in (zeros)."""
    rows, vectors = np.ascontiguousarray(pad4(rows)), np.ascontiguousarray(pad4(vectors))
    table = np.ascontiguousarray(table, _U32).reshape(-1, 2)
    nq, n_rows = table.shape[0], rows.shape[0]
    n_out = nq * n_rows if mode >= 2 else nq * k * blocks
    buf = np.full(n_out + 2 * GUARD, SENT_KEY, _U64)
    wins = np.full(n_out + 2 * GUARD, SENT_BYTE, _U8) if mode == 3 else None
    counts = None
    if mode == 3:
        counts = np.zeros((nq, ZONES), _U32) if counts_in is None else np.ascontiguousarray(counts_in, _U32).copy()
    mask = None if mask is None else np.ascontiguousarray(mask, _U32)
    exclude = None if exclude is None or not len(exclude) else np.ascontiguousarray(exclude, _U32)
    rc = load().discover_pass(int(metric), int(mode), _ptr(rows), n_rows, rows.shape[1] // 4, _ptr(vectors), vectors.shape[0],
                              _ptr(table), nq, _ptr(mask), 0 if mask is None else mask.size, _ptr(exclude),
                              0 if exclude is None else exclude.size, int(k), int(blocks), _ptr(buf), n_out, _ptr(wins), _ptr(counts),
                              GUARD)
    _raise(rc, "discover_pass")
    keys = buf[GUARD:GUARD + n_out]
    if mode == 3:
        guards = (buf[:GUARD], buf[GUARD + n_out:], wins[:GUARD], wins[GUARD + n_out:])
        return keys.reshape(nq, n_rows), wins[GUARD:GUARD + n_out].reshape(nq, n_rows), counts, guards
    return (keys.reshape(nq, n_rows) if mode == 2 else keys.reshape(nq, k, blocks)), buf[:GUARD], buf[GUARD + n_out:]


def zone_pass(mode, rec_key, rec_wins, table, k, blocks):
    """discover_zone_kernel on records rec_key / rec_wins [slots, n_rows]; table [entries][2] {query slot, zone} -> (keys
    [entries, n_rows] (mode 2) or [entries, k, blocks], front, back)"""
    rec_key = np.ascontiguousarray(rec_key, _U64)
    rec_wins = np.ascontiguousarray(rec_wins, _U8)
    table = np.ascontiguousarray(table, _U32).reshape(-1, 2)
    n_slots, n_rows = rec_key.shape
    assert rec_wins.shape == rec_key.shape
    ne = table.shape[0]
    n_out = ne * n_rows if mode == 2 else ne * k * blocks
    buf = np.full(n_out + 2 * GUARD, SENT_KEY, _U64)
    rc = load().discover_zone_pass(int(mode), _ptr(rec_key), _ptr(rec_wins), n_slots, n_rows, _ptr(table), ne, int(k), int(blocks),
                                   _ptr(buf), n_out, GUARD)
    _raise(rc, "discover_zone_pass")
    keys = buf[GUARD:GUARD + n_out]
    return (keys.reshape(ne, n_rows) if mode == 2 else keys.reshape(ne, k, blocks)), buf[:GUARD], buf[GUARD + n_out:]


# --------------------------------------------------------------------------- #
# reference layouts
# --------------------------------------------------------------------------- #
def context_keys(r_ctx, eligible):
    """context mode: the key of every row (0 where the row emits nothing)"""
    loss, alive = DR.context_fold(r_ctx, eligible)
    return np.where(alive, make_keys(loss, np.arange(loss.size)), np.uint64(0))


def records(r_target, r_ctx, eligible):
    """target mode: (keys u64 [rows], wins u8 [rows], counts u32 [33])"""
    t, wins, alive = DR.target_fold(r_target, r_ctx, eligible)
    keys = np.where(alive, make_keys(t, np.arange(t.size)), np.uint64(0))
    w = np.where(alive, wins, 0).astype(_U8)
    return keys, w, np.bincount(wins[alive], minlength=ZONES).astype(_U32)


def zone_keys(rec_key, rec_wins, zone):
    return np.where(np.asarray(rec_wins) == zone, rec_key, np.uint64(0)).astype(_U64)


def zone_lists_of(keys, k, blocks):
    """a (query, zone) entry's keys per row -> [k, blocks]: per workgroup the k best keys of its 64-row chunks"""
    W = 4 * blocks
    out = np.zeros((k, blocks), _U64)
    owner = ((np.arange(keys.size) // 64) % W) // 4
    for b in range(blocks):
        mine = keys[owner == b]
        mine = np.sort(mine[mine != 0])[::-1][:k]
        out[:mine.size, b] = mine
    return out
