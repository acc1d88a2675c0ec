"""ctypes binding of ``libwdbx_hip.so`` (C ABI declared in ``include/wdbx_hip.h``).

No PyTorch and no CPU fallback: if the library is missing, or no AMD GPU is
visible, the backend raises ``HipBackendError`` -- it never computes a result
any other way.
"""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Optional, Tuple

import numpy as np

METRIC_COSINE = 0
METRIC_L2 = 1
MAX_K = 2048
MAX_EXAMPLES = 64        # WDBX_MAX_EXAMPLES: positives + negatives of one recommend query
MAX_EXCLUDE_ROWS = 1024  # WDBX_MAX_EXCLUDE_ROWS
MAX_CONTEXT_PAIRS = 32   # WDBX_MAX_CONTEXT_PAIRS: (positive, negative) pairs of one discovery query
MAX_GROUP_SIZE = 64      # WDBX_MAX_GROUP_SIZE: members one group of wdbx_index_search_groups holds
UNIQUE_ID_BYTES = 128

_LIB_NAME = "libwdbx_hip.so"


class HipBackendError(RuntimeError):
    """Raised for every failure of the HIP backend (code + library message)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"wdbx_hip error {code}: {message}")
        self.code = code
        self.message = message


_lib: Optional[C.CDLL] = None

_u64p = C.POINTER(C.c_uint64)
_i64p = C.POINTER(C.c_int64)
_f32p = C.POINTER(C.c_float)
_dblp = C.POINTER(C.c_double)

LABEL_NONE = 0xFFFFFFFF  # WDBX_LABEL_NONE: the row is a label of its own

# name -> (restype, argtypes); the one place the ABI is spelled out for Python.
SIGNATURES = {
    "wdbx_hip_version": (C.c_int, []),
    "wdbx_last_error": (C.c_char_p, []),
    "wdbx_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "wdbx_index_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]),
    "wdbx_index_destroy": (None, [C.c_void_p]),
    "wdbx_index_dim": (C.c_int, [C.c_void_p]),
    "wdbx_index_row_pitch": (C.c_int, [C.c_void_p]),
    "wdbx_index_size": (C.c_int, [C.c_void_p, _u64p]),
    "wdbx_index_capacity": (C.c_int, [C.c_void_p, _u64p]),
    "wdbx_index_reserve": (C.c_int, [C.c_void_p, C.c_uint64]),
    "wdbx_index_clear": (C.c_int, [C.c_void_p]),
    "wdbx_index_add": (C.c_int, [C.c_void_p, _f32p, C.c_uint64, C.c_int, _u64p]),
    "wdbx_index_set_rows": (C.c_int, [C.c_void_p, C.c_uint64, _f32p, C.c_uint64, C.c_int]),
    "wdbx_index_set_rows_at": (C.c_int, [C.c_void_p, _u64p, C.c_uint64, _f32p, C.c_int]),
    "wdbx_index_remove_rows": (C.c_int, [C.c_void_p, _u64p, C.c_uint64]),
    "wdbx_index_get_rows": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _f32p]),
    "wdbx_index_fill_synthetic": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _u64p]),
    "wdbx_index_compact": (C.c_int, [C.c_void_p, _u64p, C.c_uint64]),
    "wdbx_index_search": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _i64p, _f32p]),
    "wdbx_index_search_masked": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), _i64p,
                                           _f32p]),
    "wdbx_index_search_masked_n": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_uint64,
                                             _i64p, _f32p]),
    "wdbx_index_search_multimask": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.POINTER(C.c_uint32)),
                                              _u64p, C.c_int, C.POINTER(C.c_int32), _i64p, _f32p]),
    "wdbx_index_search_rows": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _u64p, C.c_uint64, _i64p, _f32p]),
    "wdbx_index_search_matrix": (C.c_int, [C.c_void_p, _u64p, C.c_uint64, C.c_int, _i64p, _f32p]),
    "wdbx_index_search_row_lists": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _u64p, _u64p, C.c_int,
                                              C.POINTER(C.c_int32), _i64p, _f32p]),
    "wdbx_index_set_labels": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]),
    "wdbx_index_get_labels": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]),
    "wdbx_index_search_distinct": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_uint64,
                                             _i64p, _f32p, C.POINTER(C.c_uint32)]),
    "wdbx_index_search_groups": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32),
                                           C.c_uint64, _i64p, _f32p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
    "wdbx_index_search_group_members": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32),
                                                  C.c_uint64, C.POINTER(C.c_uint32), _i64p, _i64p, _f32p,
                                                  C.POINTER(C.c_int32)]),
    "wdbx_index_search_multivector": (C.c_int, [C.c_void_p, _f32p, _u64p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32),
                                                C.c_uint64, _i64p, _f32p, C.POINTER(C.c_uint32)]),
    "wdbx_index_search_mmr": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                        C.POINTER(C.c_uint32), C.c_uint64, _i64p, _f32p, _f32p]),
    "wdbx_index_search_recommend": (C.c_int, [C.c_void_p, _f32p, _u64p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32),
                                              C.c_uint64, _u64p, C.c_uint64, _i64p, _f32p, C.POINTER(C.c_uint8)]),
    "wdbx_index_search_discover": (C.c_int, [C.c_void_p, _f32p, _f32p, _u64p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32),
                                             C.c_uint64, _u64p, C.c_uint64, _i64p, _f32p, C.POINTER(C.c_uint8)]),
    "wdbx_index_range_search": (C.c_int, [C.c_void_p, _f32p, C.c_int, _f32p, C.c_int, C.POINTER(C.c_uint32), C.c_uint64,
                                          C.c_uint64, _u64p, _i64p, _f32p]),
    "wdbx_index_range_search_batch": (C.c_int, [C.c_void_p, _f32p, C.c_int, _f32p, C.c_int, C.POINTER(C.c_uint32), C.c_uint64,
                                                C.c_uint64, _u64p, _i64p, _f32p]),
    "wdbx_device_alloc": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "wdbx_device_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "wdbx_device_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "wdbx_device_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "wdbx_device_fill_synthetic": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]),
    "wdbx_index_search_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "wdbx_index_synchronize": (C.c_int, [C.c_void_p]),
    "wdbx_index_search_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "wdbx_index_search_batch_masked_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint32),
                                                        C.c_uint64, C.c_void_p, C.c_void_p]),
    "wdbx_index_batch_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_int)]),
    "wdbx_index_profile_read_gemm": (C.c_int, [C.c_void_p, _u64p, _dblp]),
    "wdbx_index_profile_read_sample": (C.c_int, [C.c_void_p, _u64p, _dblp]),
    "wdbx_comm_unique_id": (C.c_int, [C.c_void_p]),
    "wdbx_index_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64]),
    "wdbx_index_comm_destroy": (C.c_int, [C.c_void_p]),
    "wdbx_index_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _u64p]),
    "wdbx_index_comm_set_row_base": (C.c_int, [C.c_void_p, C.c_uint64]),
    "wdbx_index_search_sharded_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "wdbx_group_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]),
    "wdbx_group_destroy": (None, [C.c_void_p]),
    "wdbx_group_add": (C.c_int, [C.c_void_p, _f32p, C.c_uint64, C.c_int, _u64p]),
    "wdbx_group_size": (C.c_int, [C.c_void_p, _u64p]),
    "wdbx_group_search": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, _i64p, _f32p]),
    "wdbx_group_attach": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]),
    "wdbx_group_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _u64p]),
    "wdbx_group_stat": (C.c_int, [C.c_void_p, C.c_char_p, _i64p]),
    "wdbx_group_search_merged": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int, _i64p, _f32p]),
    "wdbx_group_search_merged_masked": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(C.POINTER(C.c_uint32)), _i64p, _f32p]),
    "wdbx_group_search_merged_masked_n": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.POINTER(C.POINTER(C.c_uint32)), _u64p, _i64p, _f32p]),
    "wdbx_group_attach_ex": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "wdbx_group_set_row_bases": (C.c_int, [C.c_void_p, _u64p, C.c_int]),
    "wdbx_group_queries_upload": (C.c_int, [C.c_void_p, _f32p, C.c_int, C.c_int]),
    "wdbx_group_queries_synthetic": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int]),
    "wdbx_group_search_resident": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "wdbx_group_synchronize": (C.c_int, [C.c_void_p]),
    "wdbx_group_results": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _i64p, _f32p]),
    "wdbx_index_comm_allgather_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "wdbx_index_search_sharded_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                                         C.c_void_p]),
    "wdbx_index_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "wdbx_index_profile_read": (C.c_int, [C.c_void_p, _u64p, _dblp, _u64p, _dblp]),
    "wdbx_index_probe_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, _dblp]),
    "wdbx_index_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "wdbx_index_get_option": (C.c_int, [C.c_void_p, C.c_char_p, _i64p]),
}


def library_path() -> Path:
    env = os.environ.get("WDBX_HIP_LIBRARY")
    if env:
        return Path(env)
    return Path(__file__).resolve().parent / _LIB_NAME


def load_library() -> C.CDLL:
    """Load the shared library and declare every entry point.  Raises
    ``HipBackendError`` when it is absent (build it with
    ``python __graft_entry__.py`` or ``make -C wdbx-py_amd/csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not path.exists():
        raise HipBackendError(-100, f"{path} not built: run `make -C wdbx-py_amd/csrc` (needs hipcc)")
    try:
        lib = C.CDLL(str(path))
    except OSError as e:  # missing ROCm runtime etc.
        raise HipBackendError(-101, f"cannot load {path}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError = ABI mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != 0:
        msg = load_library().wdbx_last_error()
        raise HipBackendError(rc, msg.decode("utf-8", "replace") if msg else "")


def device_count() -> int:
    n = C.c_int(0)
    rc = load_library().wdbx_device_count(C.byref(n))
    if rc != 0:
        return 0
    return n.value


def _as_f32(a, shape_last: int) -> np.ndarray:
    arr = np.ascontiguousarray(a, dtype=np.float32)
    if arr.ndim == 1:
        arr = arr.reshape(1, -1)
    if arr.ndim != 2 or arr.shape[1] != shape_last:
        raise ValueError(f"expected rows of length {shape_last}, got array of shape {arr.shape}")
    return arr


MAX_CALL_MASKS = 64  # WDBX_MAX_CALL_MASKS: row masks one wdbx_index_search_multimask call takes


def pack_row_mask(allowed: np.ndarray) -> np.ndarray:
    """bool[n] -> uint32 words for ``wdbx_index_search_masked`` (bit r%32 of word r//32)."""
    allowed = np.asarray(allowed, dtype=bool)
    padded = np.zeros(((allowed.size + 31) // 32) * 32, dtype=bool)
    padded[: allowed.size] = allowed
    return np.packbits(padded, bitorder="little").view(np.uint32)


class DeviceBuffer:
    """A raw HBM allocation owned through the library (no torch)."""

    def __init__(self, index: "NativeIndex", nbytes: int):
        self._index = index
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _check(index._lib.wdbx_device_alloc(index._h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, host: np.ndarray) -> None:
        host = np.ascontiguousarray(host)
        if host.nbytes > self.nbytes:
            raise ValueError("upload larger than the device buffer")
        _check(self._index._lib.wdbx_device_upload(self._index._h, self.ptr, host.ctypes.data, host.nbytes))

    def download(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        if out.nbytes > self.nbytes:
            raise ValueError("download larger than the device buffer")
        _check(self._index._lib.wdbx_device_download(self._index._h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self) -> None:
        if self.ptr and self._index._h:
            _check(self._index._lib.wdbx_device_free(self._index._h, self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class NativeIndex:
    """Thin object wrapper over one ``wdbx_index*`` (one shard in one GPU's HBM)."""

    def __init__(self, dim: int, metric: int = METRIC_COSINE, device_id: int = 0, capacity_rows: int = 1024):
        self._lib = load_library()
        self._h = None
        h = C.c_void_p()
        _check(self._lib.wdbx_index_create(int(device_id), int(dim), int(metric), int(capacity_rows), C.byref(h)))
        self._h = h.value
        self.dim = int(dim)
        self.metric = int(metric)
        self.device_id = int(device_id)
        self.pitch = int(self._lib.wdbx_index_row_pitch(self._h))

    # -- lifecycle --
    def close(self) -> None:
        if self._h:
            self._lib.wdbx_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state --
    def size(self) -> int:
        n = C.c_uint64(0)
        _check(self._lib.wdbx_index_size(self._h, C.byref(n)))
        return n.value

    def capacity(self) -> int:
        n = C.c_uint64(0)
        _check(self._lib.wdbx_index_capacity(self._h, C.byref(n)))
        return n.value

    def reserve(self, rows: int) -> None:
        _check(self._lib.wdbx_index_reserve(self._h, int(rows)))

    def clear(self) -> None:
        _check(self._lib.wdbx_index_clear(self._h))

    # -- ingest --
    def add(self, rows, normalize: bool = False) -> int:
        arr = _as_f32(rows, self.dim) if np.size(rows) else np.empty((0, self.dim), np.float32)
        first = C.c_uint64(0)
        _check(self._lib.wdbx_index_add(self._h, arr.ctypes.data_as(_f32p), arr.shape[0], int(normalize),
                                        C.byref(first)))
        return first.value

    def set_rows(self, first_row: int, rows, normalize: bool = False) -> None:
        arr = _as_f32(rows, self.dim)
        _check(self._lib.wdbx_index_set_rows(self._h, int(first_row), arr.ctypes.data_as(_f32p), arr.shape[0],
                                             int(normalize)))

    def set_rows_at(self, rows_idx, rows, normalize: bool = False) -> None:
        """Overwrite the stored rows ``rows_idx`` (strictly increasing row numbers) with ``rows[len(rows_idx), dim]`` in one
        call: every derived copy is refreshed for exactly those rows, as ``set_rows`` once per row would leave it."""
        ids = np.ascontiguousarray(rows_idx, dtype=np.uint64).reshape(-1)
        arr = _as_f32(rows, self.dim) if ids.size else np.empty((0, self.dim), np.float32)
        if arr.shape[0] != ids.size:
            raise ValueError(f"{ids.size} row numbers for {arr.shape[0]} rows")
        _check(self._lib.wdbx_index_set_rows_at(self._h, ids.ctypes.data_as(_u64p), ids.size, arr.ctypes.data_as(_f32p),
                                                int(normalize)))

    def remove_rows(self, rows_idx) -> None:
        """Turn the stored rows ``rows_idx`` (strictly increasing) into removed rows (NaN: never a result) in one call."""
        ids = np.ascontiguousarray(rows_idx, dtype=np.uint64).reshape(-1)
        _check(self._lib.wdbx_index_remove_rows(self._h, ids.ctypes.data_as(_u64p), ids.size))

    def get_rows(self, first_row: int, n: int) -> np.ndarray:
        out = np.empty((int(n), self.dim), np.float32)
        _check(self._lib.wdbx_index_get_rows(self._h, int(first_row), int(n), out.ctypes.data_as(_f32p)))
        return out

    def compact(self, src_rows) -> None:
        """Keep exactly the rows ``src_rows`` (strictly increasing), moved down to rows 0 .. len - 1 in that order."""
        src = np.ascontiguousarray(src_rows, dtype=np.uint64)
        _check(self._lib.wdbx_index_compact(self._h, src.ctypes.data_as(_u64p), src.size))

    def fill_synthetic(self, seed: int, counter_row0: int, n: int, normalize: bool) -> int:
        first = C.c_uint64(0)
        _check(self._lib.wdbx_index_fill_synthetic(self._h, int(seed), int(counter_row0), int(n), int(normalize),
                                                   C.byref(first)))
        return first.value

    # -- search (host buffers, blocking) --
    def search(self, queries, k: int, normalize_queries: bool = False,
               mask_words: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """``mask_words``: optional uint32 bit mask over the stored rows (bit r%32 of word r//32 set =
        row r may be returned), see :func:`pack_row_mask`."""
        q = _as_f32(queries, self.dim)
        nq = q.shape[0]
        idx = np.empty((nq, int(k)), np.int64)
        score = np.empty((nq, int(k)), np.float32)
        if mask_words is None:
            _check(self._lib.wdbx_index_search(self._h, q.ctypes.data_as(_f32p), nq, int(k), int(normalize_queries),
                                               idx.ctypes.data_as(_i64p), score.ctypes.data_as(_f32p)))
        else:
            m = np.ascontiguousarray(mask_words, dtype=np.uint32)
            if m.size < (self.size() + 31) // 32:
                raise ValueError("mask has fewer bits than the index has rows")
            # (the library checks the length again under the handle's lock: rows may have been added since the line above)
            _check(self._lib.wdbx_index_search_masked_n(self._h, q.ctypes.data_as(_f32p), nq, int(k),
                                                        int(normalize_queries), m.ctypes.data_as(C.POINTER(C.c_uint32)), m.size,
                                                        idx.ctypes.data_as(_i64p), score.ctypes.data_as(_f32p)))
        return idx, score

    def search_multimask(self, queries, k: int, masks, query_mask,
                         normalize_queries: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """One row mask PER QUERY in one batched call: ``masks`` is a list of uint32 word arrays (:func:`pack_row_mask`),
        ``query_mask[i]`` the index of query i's mask in it, or -1 for every row.  Results in the order of ``queries``,
        each the exact top-``k`` of the rows its mask allows -- one pass over the int8 tiles for all masks together when
        they are what a masked batch would run (``get_option("last_batch_masked") == 2``), the per-mask calls otherwise."""
        q = _as_f32(queries, self.dim)
        nq = q.shape[0]
        words = [np.ascontiguousarray(m, dtype=np.uint32).reshape(-1) for m in masks]
        which = np.ascontiguousarray(query_mask, dtype=np.int32).reshape(-1)
        if which.size != nq:
            raise ValueError(f"query_mask has {which.size} entries for {nq} queries")
        u32p = C.POINTER(C.c_uint32)
        ptrs = (u32p * max(len(words), 1))(*[m.ctypes.data_as(u32p) for m in words])
        counts = np.array([m.size for m in words], dtype=np.uint64)
        idx = np.empty((nq, int(k)), np.int64)
        score = np.empty((nq, int(k)), np.float32)
        # (lengths, mask numbers and k are checked by the library, the lengths under the handle's lock)
        _check(self._lib.wdbx_index_search_multimask(self._h, q.ctypes.data_as(_f32p), nq, int(k), int(normalize_queries), ptrs,
                                                     counts.ctypes.data_as(_u64p), len(words), which.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     idx.ctypes.data_as(_i64p), score.ctypes.data_as(_f32p)))
        return idx, score

    def search_rows(self, queries, k: int, row_ids, normalize_queries: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """The exact top-``k`` of the listed rows only (``row_ids``: strictly increasing row numbers of this index), in the
        format and order of :meth:`search`; the cost follows the list, not the index.  An empty list gives rows of -1."""
        q = _as_f32(queries, self.dim)
        nq = q.shape[0]
        ids = np.ascontiguousarray(row_ids, dtype=np.uint64).reshape(-1)
        idx = np.empty((nq, int(k)), np.int64)
        score = np.empty((nq, int(k)), np.float32)
        _check(self._lib.wdbx_index_search_rows(self._h, q.ctypes.data_as(_f32p), nq, int(k), int(normalize_queries),
                                                ids.ctypes.data_as(_u64p), ids.size, idx.ctypes.data_as(_i64p),
                                                score.ctypes.data_as(_f32p)))
        return idx, score

    def search_matrix(self, rows, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """The distance matrix among the listed rows (``rows``: strictly increasing row numbers of this index): line ``i`` is
        the exact top-``k`` of the listed rows other than ``rows[i]`` itself, with the stored row ``rows[i]`` as the query,
        in the format and order of :meth:`search_rows` and with its score bits.  Returns ``(idx[n, k], score[n, k])``."""
        ids = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        idx = np.empty((ids.size, int(k)), np.int64)
        score = np.empty((ids.size, int(k)), np.float32)
        # (the list and k are checked by the library, the list under the handle's lock)
        _check(self._lib.wdbx_index_search_matrix(self._h, ids.ctypes.data_as(_u64p), ids.size, int(k), idx.ctypes.data_as(_i64p),
                                                  score.ctypes.data_as(_f32p)))
        return idx, score

    def search_row_lists(self, queries, k: int, lists, query_list,
                         normalize_queries: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """:meth:`search_rows` with one row list PER QUERY in one batched call: ``lists`` is a sequence of uint64 arrays
        (each strictly increasing row numbers of this index, possibly empty), ``query_list[i]`` the index of query i's list
        in it.  Results in the order of ``queries``, each bit-identical to ``search_rows(queries[i], k, lists[query_list[i]])``."""
        q = _as_f32(queries, self.dim)
        nq = q.shape[0]
        arrays = [np.ascontiguousarray(r, dtype=np.uint64).reshape(-1) for r in lists]
        which = np.ascontiguousarray(query_list, dtype=np.int32).reshape(-1)
        if which.size != nq:
            raise ValueError(f"query_list has {which.size} entries for {nq} queries")
        offsets = np.zeros(len(arrays) + 1, dtype=np.uint64)
        if arrays:
            np.cumsum([a.size for a in arrays], out=offsets[1:])
        rows = np.concatenate(arrays) if arrays else np.empty(0, np.uint64)
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        idx = np.empty((nq, int(k)), np.int64)
        score = np.empty((nq, int(k)), np.float32)
        # (the lists, the list numbers and k are checked by the library, the lists under the handle's lock)
        _check(self._lib.wdbx_index_search_row_lists(self._h, q.ctypes.data_as(_f32p), nq, int(k), int(normalize_queries),
                                                     rows.ctypes.data_as(_u64p), offsets.ctypes.data_as(_u64p), len(arrays),
                                                     which.ctypes.data_as(C.POINTER(C.c_int32)), idx.ctypes.data_as(_i64p),
                                                     score.ctypes.data_as(_f32p)))
        return idx, score

    # -- distinct search: at most one row per label --
    def set_labels(self, first_row: int, labels) -> None:
        """Labels (any uint32; :data:`LABEL_NONE` = the row is a label of its own) of rows ``first_row ..``."""
        lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        _check(self._lib.wdbx_index_set_labels(self._h, int(first_row), lab.size, lab.ctypes.data_as(C.POINTER(C.c_uint32))))

    def get_labels(self, first_row: int, n: int) -> np.ndarray:
        out = np.empty(int(n), np.uint32)
        _check(self._lib.wdbx_index_get_labels(self._h, int(first_row), int(n), out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def search_distinct(self, queries, k: int, normalize_queries: bool = False,
                        mask_words: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The exact top-``k`` with at most one row per label: per query the rows ranked as :meth:`search` ranks them, the
        first row of each label kept, cut at ``k``.  Returns ``(rows int64, scores f32, labels uint32)``, each ``[nq, k]``;
        unused slots hold -1 / 0 / :data:`LABEL_NONE`.  ``mask_words`` as in :meth:`search`."""
        q = _as_f32(queries, self.dim)
        nq = q.shape[0]
        idx = np.empty((nq, int(k)), np.int64)
        score = np.empty((nq, int(k)), np.float32)
        label = np.empty((nq, int(k)), np.uint32)
        u32p = C.POINTER(C.c_uint32)
        m = None if mask_words is None else np.ascontiguousarray(mask_words, dtype=np.uint32)
        # (k, nq and the mask's length are checked by the library, the length under the handle's lock)
        _check(self._lib.wdbx_index_search_distinct(self._h, q.ctypes.data_as(_f32p), nq, int(k), int(normalize_queries),
                                                    None if m is None else m.ctypes.data_as(u32p), 0 if m is None else m.size,
                                                    idx.ctypes.data_as(_i64p), score.ctypes.data_as(_f32p),
                                                    label.ctypes.data_as(u32p)))
        return idx, score, label

    # -- search groups: the k best labels, each with its best group_size rows --
    def search_groups(self, queries, k: int, group_size: int, normalize_queries: bool = False,
                      mask_words: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """:meth:`search_distinct` with a group size: the groups are its labels, in its order, and each slot holds the
        label's best ``group_size`` eligible rows, ranked as :meth:`search_rows` ranks them (the same score bits).  Returns
        ``(rows int64 [nq, k, g], scores f32 [nq, k, g], labels uint32 [nq, k], counts int32 [nq, k])``; unused member
        slots hold -1 / 0, unused groups -1 / 0 / :data:`LABEL_NONE` / 0.  ``mask_words`` as in :meth:`search`."""
        q = _as_f32(queries, self.dim)
        nq = q.shape[0]
        shape = (nq, max(int(k), 0), max(int(group_size), 0))
        idx = np.empty(shape, np.int64)
        score = np.empty(shape, np.float32)
        label = np.empty(shape[:2], np.uint32)
        count = np.empty(shape[:2], np.int32)
        u32p = C.POINTER(C.c_uint32)
        m = None if mask_words is None else np.ascontiguousarray(mask_words, dtype=np.uint32)
        # (k, group_size, nq and the mask's length are checked by the library, the length under the handle's lock)
        _check(self._lib.wdbx_index_search_groups(self._h, q.ctypes.data_as(_f32p), nq, int(k), int(group_size),
                                                  int(normalize_queries), None if m is None else m.ctypes.data_as(u32p),
                                                  0 if m is None else m.size, idx.ctypes.data_as(_i64p),
                                                  score.ctypes.data_as(_f32p), label.ctypes.data_as(u32p),
                                                  count.ctypes.data_as(C.POINTER(C.c_int32))))
        return idx, score, label, count

    def search_group_members(self, queries, slot_labels, slot_rows, group_size: int, normalize_queries: bool = False,
                             mask_words: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Stage 2 of :meth:`search_groups` on given slots ``[nq, k]``: a slot with ``slot_rows < 0`` is unused, one with
        label :data:`LABEL_NONE` is the single row ``slot_rows``, any other label means that label's rows on this handle
        (none: count 0).  Returns ``(rows [nq, k, g], scores [nq, k, g], counts [nq, k])``."""
        q = _as_f32(queries, self.dim)
        nq = q.shape[0]
        lab = np.ascontiguousarray(slot_labels, dtype=np.uint32).reshape(nq, -1)
        row = np.ascontiguousarray(slot_rows, dtype=np.int64).reshape(nq, -1)
        if lab.shape != row.shape:
            raise ValueError(f"slot_labels {lab.shape} and slot_rows {row.shape} differ")
        k = lab.shape[1]
        shape = (nq, k, max(int(group_size), 0))
        idx = np.empty(shape, np.int64)
        score = np.empty(shape, np.float32)
        count = np.empty((nq, k), np.int32)
        u32p = C.POINTER(C.c_uint32)
        m = None if mask_words is None else np.ascontiguousarray(mask_words, dtype=np.uint32)
        _check(self._lib.wdbx_index_search_group_members(self._h, q.ctypes.data_as(_f32p), nq, k, int(group_size),
                                                         int(normalize_queries), None if m is None else m.ctypes.data_as(u32p),
                                                         0 if m is None else m.size, lab.ctypes.data_as(u32p),
                                                         row.ctypes.data_as(_i64p), idx.ctypes.data_as(_i64p),
                                                         score.ctypes.data_as(_f32p), count.ctypes.data_as(C.POINTER(C.c_int32))))
        return idx, score, count

    def search_multivector(self, vectors, offsets, k: int, normalize_queries: bool = False,
                           mask_words: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Late interaction (MaxSim): query ``i`` is the vectors ``offsets[i] .. offsets[i + 1] - 1`` of ``vectors``; the
        labels are ranked by the sum over the query's vectors of each vector's best score among the label's rows (fp32,
        folded in vector order).  Returns ``(rows int64, scores f32, labels uint32)``, each ``[nq, k]``: a label's smallest
        row, its sum and its stored label; unused slots hold -1 / 0 / :data:`LABEL_NONE`.  ``mask_words`` as in
        :meth:`search`."""
        v = _as_f32(vectors, self.dim)
        off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        nq = off.size - 1
        if nq >= 1 and int(off[-1]) != v.shape[0]:
            raise ValueError(f"offsets end at {int(off[-1])}, {v.shape[0]} vectors given")
        idx = np.empty((max(nq, 0), int(k)), np.int64)
        score = np.empty((max(nq, 0), int(k)), np.float32)
        label = np.empty((max(nq, 0), int(k)), np.uint32)
        u32p = C.POINTER(C.c_uint32)
        m = None if mask_words is None else np.ascontiguousarray(mask_words, dtype=np.uint32)
        # (nq, k, the offsets and the mask's length are checked by the library, the length under the handle's lock)
        _check(self._lib.wdbx_index_search_multivector(self._h, v.ctypes.data_as(_f32p), off.ctypes.data_as(_u64p), nq, int(k),
                                                       int(normalize_queries),
                                                       None if m is None else m.ctypes.data_as(u32p), 0 if m is None else m.size,
                                                       idx.ctypes.data_as(_i64p), score.ctypes.data_as(_f32p),
                                                       label.ctypes.data_as(u32p)))
        return idx, score, label

    def search_mmr(self, queries, k: int, fetch_k: int, lambda_mult: float, normalize_queries: bool = False,
                   mask: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Maximal marginal relevance: per query ``k`` rows picked greedily from its exact top-``fetch_k``, each pick the
        candidate with the largest ``lambda_mult * relevance - (1 - lambda_mult) * (largest similarity to a row already
        picked)`` (fp32, include/wdbx_hip.h states every rounding).  Returns ``(rows int64, scores f32, mmr f32)``, each
        ``[nq, k]`` in pick order: the row, its relevance as :meth:`search` returns it, the value it won with; unused slots
        hold -1 / 0 / 0.  ``mask``: uint32 words as in :meth:`search` (``mask_words``)."""
        q = _as_f32(queries, self.dim)
        nq = q.shape[0]
        idx = np.empty((nq, int(k)), np.int64)
        score = np.empty((nq, int(k)), np.float32)
        mmr = np.empty((nq, int(k)), np.float32)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint32)
        # (nq, k, fetch_k, lambda and the mask's length are checked by the library, the length under the handle's lock)
        _check(self._lib.wdbx_index_search_mmr(self._h, q.ctypes.data_as(_f32p), nq, int(k), int(fetch_k), float(lambda_mult),
                                               int(normalize_queries),
                                               None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               0 if m is None else m.size, idx.ctypes.data_as(_i64p), score.ctypes.data_as(_f32p),
                                               mmr.ctypes.data_as(_f32p)))
        return idx, score, mmr

    def search_recommend(self, examples, offsets, k: int, normalize_examples: bool = False,
                         mask_words: Optional[np.ndarray] = None,
                         exclude_rows=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Rows ranked by positive and negative examples: query ``i``'s positives are the vectors ``offsets[2 i] ..
        offsets[2 i + 1] - 1`` of ``examples``, its negatives ``offsets[2 i + 1] .. offsets[2 i + 2] - 1``.  Per row ``p`` is
        the best score over the positives and ``n`` over the negatives; rows with ``p > n`` (favoured) come first by ``p``, the
        others follow by ``n`` ascending.  Returns ``(rows int64, scores f32, sides uint8)``, each ``[nq, k]``: the row, the
        value it was ranked by (``p`` or ``n``, as :meth:`search` returns scores) and 1 for favoured / 0 for disfavoured;
        unused slots hold -1 / 0 / 0.  ``mask_words`` as in :meth:`search`; ``exclude_rows``: strictly increasing row numbers
        that never come back."""
        v = _as_f32(examples, self.dim)
        off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        if off.size < 3 or off.size % 2 == 0:
            raise ValueError(f"offsets holds {off.size} entries: 2 * queries + 1 needed")
        nq = (off.size - 1) // 2
        if int(off[-1]) != v.shape[0]:
            raise ValueError(f"offsets end at {int(off[-1])}, {v.shape[0]} examples given")
        idx = np.empty((nq, int(k)), np.int64)
        score = np.empty((nq, int(k)), np.float32)
        side = np.empty((nq, int(k)), np.uint8)
        m = None if mask_words is None else np.ascontiguousarray(mask_words, dtype=np.uint32)
        ex = None if exclude_rows is None else np.ascontiguousarray(exclude_rows, dtype=np.uint64).reshape(-1)
        # (nq, k, the offsets, the mask's length and the exclusion list are checked by the library, the last two under the lock)
        _check(self._lib.wdbx_index_search_recommend(self._h, v.ctypes.data_as(_f32p), off.ctypes.data_as(_u64p), nq, int(k),
                                                     int(normalize_examples),
                                                     None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                     0 if m is None else m.size,
                                                     None if ex is None or not ex.size else ex.ctypes.data_as(_u64p),
                                                     0 if ex is None else ex.size, idx.ctypes.data_as(_i64p),
                                                     score.ctypes.data_as(_f32p), side.ctypes.data_as(C.POINTER(C.c_uint8))))
        return idx, score, side

    def search_discover(self, targets, context, pair_offsets, k: int, normalize_vectors: bool = False,
                        mask_words: Optional[np.ndarray] = None,
                        exclude_rows=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Rows ranked by context pairs and a target: query ``q``'s pairs are ``pair_offsets[q] .. pair_offsets[q + 1] - 1``,
        pair ``i`` the vectors ``2 i`` (positive) and ``2 i + 1`` (negative) of ``context``.  With ``targets`` ([nq, dim]) rows
        rank by (pairs won descending, target score descending, row); with ``targets=None`` (context search) by the loss, the
        sum over the pairs of ``min(r(positive) - r(negative), 0)``, descending.  Returns ``(rows int64, scores f32, wins
        uint8)``, each ``[nq, k]``: the score is the target's (as :meth:`search` returns scores) or the loss (<= 0, the
        ranking domain for either metric); unused slots hold -1 / 0 / 0.  ``mask_words`` and ``exclude_rows`` as in
        :meth:`search_recommend`."""
        off = np.ascontiguousarray(pair_offsets, dtype=np.uint64).reshape(-1)
        if off.size < 2:
            raise ValueError(f"pair_offsets holds {off.size} entries: queries + 1 needed")
        nq = off.size - 1
        t = None if targets is None else _as_f32(targets, self.dim)
        if t is not None and t.shape[0] != nq:
            raise ValueError(f"{t.shape[0]} targets for {nq} queries")
        c = None
        if context is not None and np.size(context):
            c = _as_f32(context, self.dim)
        if 2 * int(off[-1]) != (0 if c is None else c.shape[0]):
            raise ValueError(f"pair_offsets end at {int(off[-1])} pairs, {0 if c is None else c.shape[0]} context vectors given")
        idx = np.empty((nq, int(k)), np.int64)
        score = np.empty((nq, int(k)), np.float32)
        wins = np.empty((nq, int(k)), np.uint8)
        m = None if mask_words is None else np.ascontiguousarray(mask_words, dtype=np.uint32)
        ex = None if exclude_rows is None else np.ascontiguousarray(exclude_rows, dtype=np.uint64).reshape(-1)
        # (nq, k, the offsets, the mask's length and the exclusion list are checked by the library, the last two under the lock)
        _check(self._lib.wdbx_index_search_discover(self._h, None if t is None else t.ctypes.data_as(_f32p),
                                                    None if c is None else c.ctypes.data_as(_f32p), off.ctypes.data_as(_u64p),
                                                    nq, int(k), int(normalize_vectors),
                                                    None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    0 if m is None else m.size,
                                                    None if ex is None or not ex.size else ex.ctypes.data_as(_u64p),
                                                    0 if ex is None else ex.size, idx.ctypes.data_as(_i64p),
                                                    score.ctypes.data_as(_f32p), wins.ctypes.data_as(C.POINTER(C.c_uint8))))
        return idx, score, wins

    def range_search(self, queries, thresholds, normalize_queries: bool = False,
                     mask_words: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Every row whose score reaches its query's threshold (cosine / inner product: score >= t; L2: squared distance
        <= t), exact fp32, per query sorted like :meth:`search`.  ``thresholds``: one per query (a scalar serves all).
        Returns CSR ``(offsets int64[nq + 1], rows int64[total], scores f32[total])``: query i's results are
        ``[offsets[i], offsets[i + 1])``.  A first call guesses the capacity (the previous answer's size, at least 4096 per
        query); if the answer is larger, one more call with the exact total (a third only if rows were added in between;
        after three the call raises)."""
        return self._range_call(self._lib.wdbx_index_range_search, queries, thresholds, normalize_queries, mask_words)

    def range_search_batch(self, queries, thresholds, normalize_queries: bool = False,
                           mask_words: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """:meth:`range_search` for a batch: the same arguments and the same answer, bit for bit, through
        ``wdbx_index_range_search_batch`` -- one int8 tile pass per block of up to 256 queries where the library's route
        allows it (``get_option("last_range_batch_path")``), the per-query path otherwise."""
        return self._range_call(self._lib.wdbx_index_range_search_batch, queries, thresholds, normalize_queries, mask_words)

    def _range_call(self, entry, queries, thresholds, normalize_queries, mask_words):
        q = _as_f32(queries, self.dim)
        nq = q.shape[0]
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, dtype=np.float32), (nq,)))
        m = None
        if mask_words is not None:
            m = np.ascontiguousarray(mask_words, dtype=np.uint32)
            if m.size < (self.size() + 31) // 32:
                raise ValueError("mask has fewer bits than the index has rows")
        offsets = np.zeros(nq + 1, np.uint64)
        # the guess: the previous answer's size (repeated queries of one kind then take one call), at least 4096 per query
        capacity = max(4096 * nq, getattr(self, "_range_hint", 0))
        for _ in range(3):
            rows = np.empty(capacity, np.int64)
            scores = np.empty(capacity, np.float32)
            _check(entry(
                self._h, q.ctypes.data_as(_f32p), nq, t.ctypes.data_as(_f32p), int(normalize_queries),
                m.ctypes.data_as(C.POINTER(C.c_uint32)) if m is not None else None, m.size if m is not None else 0,
                capacity, offsets.ctypes.data_as(_u64p), rows.ctypes.data_as(_i64p), scores.ctypes.data_as(_f32p)))
            total = int(offsets[nq])
            self._range_hint = total
            if total <= capacity:
                return offsets.astype(np.int64), rows[:total], scores[:total]
            capacity = total
        raise HipBackendError(-6, "range search: the result kept growing between calls (concurrent adds)")

    # -- device-resident path --
    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def device_queries_synthetic(self, seed: int, counter_row0: int, n: int, normalize: bool) -> DeviceBuffer:
        buf = self.alloc(int(n) * self.pitch * 4)
        _check(self._lib.wdbx_device_fill_synthetic(self._h, buf.ptr, int(seed), int(counter_row0), int(n),
                                                    int(normalize)))
        return buf

    def device_queries(self, queries) -> DeviceBuffer:
        q = _as_f32(queries, self.dim)
        padded = np.zeros((q.shape[0], self.pitch), np.float32)
        padded[:, : self.dim] = q
        buf = self.alloc(padded.nbytes)
        buf.upload(padded)
        return buf

    def search_device(self, d_queries: DeviceBuffer, nq: int, k: int, d_idx: DeviceBuffer, d_score: DeviceBuffer,
                      query_offset: int = 0, sharded: bool = False) -> None:
        """Enqueue ``nq`` scans (asynchronous); ``query_offset`` = first query row in ``d_queries``."""
        fn = self._lib.wdbx_index_search_sharded_device if sharded else self._lib.wdbx_index_search_device
        qptr = d_queries.ptr + int(query_offset) * self.pitch * 4
        _check(fn(self._h, qptr, int(nq), int(k), d_idx.ptr, d_score.ptr))

    def synchronize(self) -> None:
        _check(self._lib.wdbx_index_synchronize(self._h))

    # -- batched queries on the MFMA path (extension) --
    def search_batch_device(self, d_queries: DeviceBuffer, nq: int, k: int, d_idx: DeviceBuffer,
                            d_score: DeviceBuffer, query_offset: int = 0, sharded: bool = False) -> None:
        qptr = d_queries.ptr + int(query_offset) * self.pitch * 4
        fn = self._lib.wdbx_index_search_sharded_batch_device if sharded else self._lib.wdbx_index_search_batch_device
        _check(fn(self._h, qptr, int(nq), int(k), d_idx.ptr, d_score.ptr))

    def search_batch_masked_device(self, d_queries: DeviceBuffer, nq: int, k: int, mask_words, d_idx: DeviceBuffer,
                                   d_score: DeviceBuffer, query_offset: int = 0) -> None:
        """:meth:`search_batch_device` with a row mask from the host (see :func:`pack_row_mask`): one masked pass over the
        int8 tiles where they run (``get_option("last_batch_masked") == 1``).  The library checks the mask's length."""
        m = np.ascontiguousarray(mask_words, dtype=np.uint32)
        qptr = d_queries.ptr + int(query_offset) * self.pitch * 4
        _check(self._lib.wdbx_index_search_batch_masked_device(self._h, qptr, int(nq), int(k), m.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                               m.size, d_idx.ptr, d_score.ptr))

    def batch_status(self, nq: int):
        counts = np.zeros(max(int(nq), 1), np.uint32)
        cap, over = C.c_uint32(0), C.c_int(0)
        _check(self._lib.wdbx_index_batch_status(self._h, counts.ctypes.data_as(C.POINTER(C.c_uint32)), int(nq),
                                                 C.byref(cap), C.byref(over)))
        return {"counts": counts[: int(nq)], "capacity": cap.value, "overflowed": over.value}

    def profile_read_gemm(self):
        n, ms = C.c_uint64(0), C.c_double(0)
        _check(self._lib.wdbx_index_profile_read_gemm(self._h, C.byref(n), C.byref(ms)))
        return {"gemm_launches": n.value, "gemm_ms": ms.value}

    def profile_read_sample(self):
        n, ms = C.c_uint64(0), C.c_double(0)
        _check(self._lib.wdbx_index_profile_read_sample(self._h, C.byref(n), C.byref(ms)))
        return {"sample_launches": n.value, "sample_ms": ms.value}

    # -- shard group (RCCL) --
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        _check(load_library().wdbx_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, nranks: int, rank: int, unique_id: bytes, global_row_base: int) -> None:
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        buf = C.create_string_buffer(unique_id, UNIQUE_ID_BYTES)
        _check(self._lib.wdbx_index_comm_init(self._h, int(nranks), int(rank), buf, int(global_row_base)))

    def comm_destroy(self) -> None:
        _check(self._lib.wdbx_index_comm_destroy(self._h))

    def comm_info(self):
        """What RCCL reports for this handle's communicator: ranks, this rank, and the handle's global row base."""
        n, r, base = C.c_int(0), C.c_int(-1), C.c_uint64(0)
        _check(self._lib.wdbx_index_comm_info(self._h, C.byref(n), C.byref(r), C.byref(base)))
        return {"rccl_nranks": n.value, "rccl_rank": r.value, "row_base": base.value}

    def comm_set_row_base(self, global_row_base: int) -> None:
        _check(self._lib.wdbx_index_comm_set_row_base(self._h, int(global_row_base)))

    def comm_allgather_host(self, payload: bytes, nranks: int) -> list:
        """All-gather ``payload`` (same length on every rank) through the handle's RCCL communicator; returns the
        ranks' payloads in rank order.  Launcher-side plumbing only (barrier, max of a time, cross-checks)."""
        send = C.create_string_buffer(payload, len(payload))
        recv = C.create_string_buffer(len(payload) * int(nranks))
        _check(self._lib.wdbx_index_comm_allgather_host(self._h, send, recv, len(payload)))
        raw = recv.raw
        return [raw[i * len(payload):(i + 1) * len(payload)] for i in range(int(nranks))]

    # -- measurement / knobs --
    def profile(self, enable: bool) -> None:
        _check(self._lib.wdbx_index_profile(self._h, int(enable)))

    def profile_read(self):
        sl, ml = C.c_uint64(0), C.c_uint64(0)
        sm, mm = C.c_double(0), C.c_double(0)
        _check(self._lib.wdbx_index_profile_read(self._h, C.byref(sl), C.byref(sm), C.byref(ml), C.byref(mm)))
        return {"scan_launches": sl.value, "scan_ms": sm.value, "merge_launches": ml.value, "merge_ms": mm.value}

    def probe_read_ms(self, nontemporal: bool = True, blocks: int = 0, reps: int = 20) -> float:
        ms = C.c_double(0)
        _check(self._lib.wdbx_index_probe_read(self._h, int(nontemporal), int(blocks), int(reps), C.byref(ms)))
        return ms.value

    def set_option(self, name: str, value: int) -> None:
        _check(self._lib.wdbx_index_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int64(0)
        _check(self._lib.wdbx_index_get_option(self._h, name.encode(), C.byref(v)))
        return v.value


class NativeGroup:
    """S shards on S distinct devices in one process (``wdbx_group_*``): contiguous row ranges, RCCL
    all-gather of the per-shard key lists, merge on the first device."""

    def __init__(self, device_ids, dim: int, metric: int = METRIC_COSINE, cap_per_shard: int = 1 << 20):
        self._lib = load_library()
        self._h = None
        self._attached = ()
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        h = C.c_void_p()
        _check(self._lib.wdbx_group_create(ids, len(device_ids), int(dim), int(metric), int(cap_per_shard), C.byref(h)))
        self._h = h.value
        self.dim = int(dim)

    EXCHANGE_AUTO, EXCHANGE_RCCL, EXCHANGE_COPY = 0, 1, 2

    @classmethod
    def attach(cls, shards, exchange: int = 0) -> "NativeGroup":
        """A group over existing :class:`NativeIndex` shards (``wdbx_group_attach_ex``): the shards stay owned by their
        creators; merged results number the rows ``stride * shard + local_row`` (see :meth:`info`) unless
        :meth:`set_row_bases` says otherwise.  ``exchange``: 0 = RCCL when every shard has its own device (device copies
        otherwise), 1 = RCCL or fail, 2 = device copies."""
        self = cls.__new__(cls)
        self._lib = load_library()
        self._h = None
        self._attached = tuple(shards)  # keep the handles alive as long as the group
        arr = (C.c_void_p * len(shards))(*[s._h for s in shards])
        h = C.c_void_p()
        _check(self._lib.wdbx_group_attach_ex(arr, len(shards), int(exchange), C.byref(h)))
        self._h = h.value
        self.dim = shards[0].dim
        return self

    def set_row_bases(self, bases) -> None:
        arr = (C.c_uint64 * len(bases))(*[int(b) for b in bases])
        _check(self._lib.wdbx_group_set_row_bases(self._h, arr, len(bases)))

    # -- device-resident form: queries live on every shard's device, results on the first shard's --
    def queries_upload(self, queries, normalize_queries: bool = False) -> int:
        q = _as_f32(queries, self.dim)
        _check(self._lib.wdbx_group_queries_upload(self._h, q.ctypes.data_as(_f32p), q.shape[0], int(normalize_queries)))
        return q.shape[0]

    def queries_synthetic(self, seed: int, counter_row0: int, nq: int, normalize: bool) -> None:
        _check(self._lib.wdbx_group_queries_synthetic(self._h, int(seed), int(counter_row0), int(nq), int(normalize)))

    def search_resident(self, first_query: int, nq: int, k: int, k_out: Optional[int] = None) -> None:
        """Asynchronous: enqueue the search of resident queries ``[first_query, first_query + nq)`` on every shard."""
        _check(self._lib.wdbx_group_search_resident(self._h, int(first_query), int(nq), int(k), int(k_out or k)))

    def synchronize(self) -> None:
        _check(self._lib.wdbx_group_synchronize(self._h))

    def results(self, nq: int, k_out: int) -> Tuple[np.ndarray, np.ndarray]:
        idx = np.empty((int(nq), int(k_out)), np.int64)
        score = np.empty((int(nq), int(k_out)), np.float32)
        _check(self._lib.wdbx_group_results(self._h, int(nq), int(k_out), idx.ctypes.data_as(_i64p),
                                            score.ctypes.data_as(_f32p)))
        return idx, score

    def info(self):
        n, r, stride = C.c_int(0), C.c_int(0), C.c_uint64(0)
        _check(self._lib.wdbx_group_info(self._h, C.byref(n), C.byref(r), C.byref(stride)))
        return {"shards": n.value, "rccl_nranks": r.value, "row_stride": stride.value}

    def stat(self, name: str) -> int:
        """A counter of the group: ``exchanges`` (exchange + merge steps enqueued so far), ``dispatches``, ``unusable``."""
        v = C.c_int64(0)
        _check(self._lib.wdbx_group_stat(self._h, name.encode(), C.byref(v)))
        return v.value

    def search_merged(self, queries, k: int, k_out: int, normalize_queries: bool = False,
                      mask_words=None) -> Tuple[np.ndarray, np.ndarray]:
        """Per-shard top-``k``, merged into the ``k_out`` best of their union (``k <= k_out <= shards * k``).
        ``mask_words``: optional list with one uint32 mask (see :func:`pack_row_mask`) or ``None`` per shard -- only rows whose
        bit is set compete (metadata filter pushed down into every shard's scan)."""
        q = _as_f32(queries, self.dim)
        idx = np.empty((q.shape[0], int(k_out)), np.int64)
        score = np.empty((q.shape[0], int(k_out)), np.float32)
        if mask_words is None:
            _check(self._lib.wdbx_group_search_merged(self._h, q.ctypes.data_as(_f32p), q.shape[0], int(k), int(k_out),
                                                      int(normalize_queries), idx.ctypes.data_as(_i64p),
                                                      score.ctypes.data_as(_f32p)))
        else:
            keep = [None if m is None else np.ascontiguousarray(m, dtype=np.uint32) for m in mask_words]
            if self._attached and len(keep) != len(self._attached):
                raise ValueError(f"{len(keep)} masks for {len(self._attached)} shards")
            for s, m in enumerate(keep):  # as NativeIndex.search does; the library checks again under the group's locks
                if m is not None and self._attached and m.size < (self._attached[s].size() + 31) // 32:
                    raise ValueError(f"shard {s}: mask has fewer bits than the shard has rows")
            u32p = C.POINTER(C.c_uint32)
            arr = (u32p * len(keep))(*[C.cast(None, u32p) if m is None else m.ctypes.data_as(u32p) for m in keep])
            counts = (C.c_uint64 * len(keep))(*[0 if m is None else m.size for m in keep])
            _check(self._lib.wdbx_group_search_merged_masked_n(self._h, q.ctypes.data_as(_f32p), q.shape[0], int(k), int(k_out),
                                                               int(normalize_queries), arr, counts, idx.ctypes.data_as(_i64p),
                                                               score.ctypes.data_as(_f32p)))
        return idx, score

    def close(self) -> None:
        if self._h:
            self._lib.wdbx_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, rows, normalize: bool = False) -> int:
        arr = _as_f32(rows, self.dim)
        first = C.c_uint64(0)
        _check(self._lib.wdbx_group_add(self._h, arr.ctypes.data_as(_f32p), arr.shape[0], int(normalize), C.byref(first)))
        return first.value

    def size(self) -> int:
        n = C.c_uint64(0)
        _check(self._lib.wdbx_group_size(self._h, C.byref(n)))
        return n.value

    def search(self, queries, k: int, normalize_queries: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        q = _as_f32(queries, self.dim)
        idx = np.empty((q.shape[0], int(k)), np.int64)
        score = np.empty((q.shape[0], int(k)), np.float32)
        _check(self._lib.wdbx_group_search(self._h, q.ctypes.data_as(_f32p), q.shape[0], int(k), int(normalize_queries),
                                           idx.ctypes.data_as(_i64p), score.ctypes.data_as(_f32p)))
        return idx, score
