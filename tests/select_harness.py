"""ctypes loader of tests/kernel_harness/libselect_harness.so (built by ``make -C wdbx-py_amd/csrc all``), the numpy side of
the shadows' layouts, and the property checkers of tests/test_gpu_select_kernels.py.

The harness launches the library's own selection kernels -- ``rows_to_u8_kernel``, ``rows_to_u6_kernel``,
``row_sqnorm_kernel``, ``rows_to_i8g_kernel``, ``queries_to_i8_kernel``, ``scan8_kernel`` (phases 0, 1, 2), ``scan8_sample4_kernel``, ``scan8_u6_sample_kernel``,
``scan8_u6_kernel``, ``rescore_kernel``, ``u6_cut_kernel`` -- on arrays the caller hands it.  The shadows a scan reads are
arguments: what a quantiser kernel produced, or bytes / codes / scales built by hand.

The checkers are plain numpy on float64 and never look at the code under test: they take what a scan was GIVEN (scales,
query) and what it EMITTED (keys), and the float64 scores of the fp32 rows.  tests/test_gpu_select_kernels.py feeds them
the kernels' output on the GPU and, on the CPU, the numpy restatements of tests/test_selection_bounds*.py and a list of
deliberately wrong restatements that they must reject."""
import ctypes as C
from pathlib import Path

import numpy as np

from rank_harness import METRIC_COSINE, METRIC_L2, f2ord, key_ord, key_row, make_keys, ord2f  # noqa: F401  (re-exported)

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "kernel_harness" / "select_harness.hip"
LIBRARY = ROOT / "tests" / "kernel_harness" / "libselect_harness.so"

_U8, _U32, _U64, _F32, _F64 = np.uint8, np.uint32, np.uint64, np.float32, np.float64
U = 2.0 ** -24  # unit roundoff of fp32

# kScan8Shapes of kernels_scan8.h: 16-byte pieces per row, lanes per row, loads per lane (restated; the GPU suite compares
# it with what the library's scan8_shape answers)
SCAN8_SHAPES = [(8, 8, 1), (16, 8, 2), (24, 8, 3), (32, 16, 2), (48, 16, 3), (64, 32, 2), (96, 32, 3), (128, 64, 2), (192, 64, 3),
                (256, 64, 4)]
U6_CUT_SEG = 16 * 1024

# what the output arrays hold before a launch: a slot the kernel must leave alone comes back with these
SENT_BYTE, SENT_U32, SENT_F32, SENT_KEY = 0xAB, 0xABABABAB, 0x7FC12345, 0xDEADBEEFDEADBEEF
GUARD = 64  # keys behind every candidate buffer that no kernel may touch


def gamma(n):
    """The classic bound of n fp32 roundings: n u / (1 - n u)."""
    return n * U / (1.0 - n * U)


def scan8_shape_py(dim):
    for pieces, L, qpl in SCAN8_SHAPES:
        if pieces * 16 >= dim:
            return pieces, L, qpl
    return None


def u6_unit_chunk_py(units):
    for uc in range(8, 3, -1):
        if units % uc == 0:
            return uc
    return 0


# --------------------------------------------------------------------------- #
# layouts
# --------------------------------------------------------------------------- #
def pack_u6(codes):
    """codes [n, units * 16] (values 0 .. 63) -> dwords [tiles][units][64][3] of kernels_scan6.h: dword t byte b = code 4t+b in
    the low six bits, bits [2t, 2t+1] of code 12+b in the top two.  Rows past n in the last tile: code 32."""
    codes = np.asarray(codes, _U32)
    n, dimp = codes.shape
    units, tiles = dimp // 16, (n + 63) // 64
    full = np.full((tiles * 64, units, 16), 32, _U32)
    full[:n] = codes.reshape(n, units, 16)
    dw = np.zeros((tiles * 64, units, 3), _U32)
    for t in range(3):
        for b in range(4):
            dw[:, :, t] |= (full[:, :, 4 * t + b] | (((full[:, :, 12 + b] >> _U32(2 * t)) & _U32(3)) << _U32(6))) << _U32(8 * b)
    return np.ascontiguousarray(dw.reshape(tiles, 64, units, 3).transpose(0, 2, 1, 3))


def unpack_u6(dw, n):
    """The inverse of :func:`pack_u6` by the scan kernels' own extraction (u6_unpack) -> codes [n, units * 16] uint8."""
    dw = np.asarray(dw, _U32)
    tiles, units = dw.shape[0], dw.shape[1]
    per_row = dw.transpose(0, 2, 1, 3).reshape(tiles * 64, units, 3)
    out = np.zeros((tiles * 64, units, 16), _U32)
    for t in range(3):
        lo = per_row[:, :, t] & _U32(0x3F3F3F3F)
        for b in range(4):
            out[:, :, 4 * t + b] = (lo >> _U32(8 * b)) & _U32(0xFF)
    hi = ((per_row[:, :, 0] >> _U32(6)) & _U32(0x03030303)) | ((per_row[:, :, 1] >> _U32(4)) & _U32(0x0C0C0C0C)) | \
         ((per_row[:, :, 2] >> _U32(2)) & _U32(0x30303030))
    for b in range(4):
        out[:, :, 12 + b] = (hi >> _U32(8 * b)) & _U32(0xFF)
    return out.reshape(tiles * 64, units * 16)[:n].astype(_U8)


def g8_offset(r, col, pitch8):
    """kernels_tiles8.h::g8_offset restated: blocks of 32 rows, inside a block k-steps of 64 columns = 2 KiB, inside a k-step
    two 1 KiB fragments (rows 0-15, 16-31) in which lane 16 kb + (r & 15) owns the 16 bytes [64 s + 16 kb, +16) of its row."""
    r, col = np.asarray(r, np.int64), np.asarray(col, np.int64)
    return (r >> 5) * 32 * pitch8 + (col >> 6) * 2048 + ((r >> 4) & 1) * 1024 + ((((col >> 4) & 3) << 4) + (r & 15)) * 16 + (col & 15)


def i8g_pitch(dim):
    """The tile path's byte pitch (host_index.h::i8g_pitch): the dimension rounded up to 128."""
    return (dim + 127) // 128 * 128


def ungather_i8g(flat, n, pitch8):
    """The fragment-ordered bytes of rows [0, n) as [n, pitch8] int8."""
    r, c = np.meshgrid(np.arange(n), np.arange(pitch8), indexing="ij")
    return np.asarray(flat, np.int8)[g8_offset(r, c, pitch8)]


def pad_u8(u, pitch8, fill=128):
    """bytes [n, dim] -> [n, pitch8], the padding at the zero point."""
    u = np.asarray(u, _U8)
    out = np.full((u.shape[0], pitch8), fill, _U8)
    out[:, :u.shape[1]] = u
    return out


def pad_f32(x, pitch):
    x = np.asarray(x, _F32)
    out = np.zeros((x.shape[0], pitch), _F32)
    out[:, :x.shape[1]] = x
    return out


# --------------------------------------------------------------------------- #
# float64 truth and the documented bounds
# --------------------------------------------------------------------------- #
def scores64(rows, q, metric=METRIC_COSINE):
    """The value a scan selects by, in float64 from the fp32 operands: c.q, or 2 c.q - |c|^2 for L2.  Rows with a NaN
    element score NaN; rows with an infinite element whatever IEEE gives (the checkers treat them by their class)."""
    r, qq = np.asarray(rows, _F32).astype(_F64), np.asarray(q, _F32).astype(_F64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = r @ qq
        if metric == METRIC_L2:
            s = 2.0 * s - (r * r).sum(axis=1)
    return s


def row_class(rows):
    """0 finite, 1 holds a NaN (never a result), 2 holds an infinity and no NaN (always a candidate)."""
    rows = np.asarray(rows)
    nan = np.isnan(rows).any(axis=1)
    inf = np.isinf(rows).any(axis=1) & ~nan
    return np.where(nan, 1, np.where(inf, 2, 0))


def u8_bound64(scale, q, metric=METRIC_COSINE, cn=None, phase2=False):
    """m of kernels_scan8.h in float64 from the scales (and cached norms) the scan was given: 0.51 s |q|_1; L2: 2 m + 3e-5 |c|^2;
    range search on cosine: + 1e-3 s |q|_1."""
    q1 = np.abs(np.asarray(q, _F32).astype(_F64)).sum()
    s = np.asarray(scale, _F32).astype(_F64)
    m = 0.51 * s * q1
    if metric == METRIC_L2:
        m = 2.0 * m + 3e-5 * np.asarray(cn, _F32).astype(_F64)
    elif phase2:
        m = m + 1e-3 * s * q1
    return m


def u6_bound64(s, a, q, dimp):
    """m of kernels_scan6.h in float64: a |q|_2 + 6e-6 (dimp + 8) s |q|_1 (+ a * 1e-37, the floor u6_query_sums adds to |q|_2)."""
    qq = np.asarray(q, _F32).astype(_F64)
    s, a = np.asarray(s, _F32).astype(_F64), np.asarray(a, _F32).astype(_F64)
    return a * (np.sqrt((qq * qq).sum()) + 1e-37) + 6e-6 * (dimp + 8) * s * np.abs(qq).sum()


# What the kernels add on top of the documented m, relative: their own (1 + 1e-5) round-up of |q|_1 and |q|_2, the fp32
# summation of those norms (lane-strided, then a tree: at most 64 + 6 roundings deep up to 4096 elements, gamma(70) = 4.2e-6),
# the constants 0.51f / 6e-6f / (1 + 1e-5)f as fp32 (1 u each) and the three or four products and fmas that form m (1 u each):
# 1e-5 + 4.2e-6 + 8 u < 1.5e-5, taken as 2e-5.
M_SLACK = 2e-5


def check_w(keys, n_rows, truth, m64, cls):
    """From a tau = -inf pass: every row that is not NaN appears exactly once, NaN rows and rows >= n_rows never; an infinite
    row carries +inf when its w is NaN; |w - truth| <= m64 (1 + 2e-5) on every finite row.  Returns w per row (NaN where absent)."""
    keys = np.asarray(keys, _U64)
    rows = key_row(keys).astype(np.int64)
    assert rows.size == np.unique(rows).size, "a row was appended twice"
    assert rows.size == 0 or rows.max() < n_rows, "a row past the end was appended"
    want = np.flatnonzero(cls != 1)
    assert np.array_equal(np.sort(rows), want), ("kept set at tau = -inf", np.setxor1d(rows, want)[:8])
    w = np.full(n_rows, np.nan)
    w[rows] = ord2f(key_ord(keys)).astype(_F64)
    assert not np.isnan(w[want]).any(), "a key carries a NaN score"
    fin = np.flatnonzero(cls == 0)
    err = np.abs(w[fin] - truth[fin])
    bad = fin[~(err <= m64[fin] * (1 + M_SLACK))]
    assert bad.size == 0, ("|w - c.q| above the bound", bad[:8], err[np.isin(fin, bad)][:8], m64[bad][:8])
    return w


def check_kept(keys, count, cap, n_rows, truth, m64, cls, t, mask=None):
    """The selection property of one full pass at threshold t.  SAFETY: every row whose float64 score is >= t is kept, every
    infinite row is kept, no NaN row, no row >= n_rows, no masked-out row and no duplicate is.  TIGHTNESS: every kept finite
    row has score >= t - 2 m64 (1 + 2e-5).  count is the exact number kept, also past cap; keys[:min(count, cap)] are the kept."""
    keys = np.asarray(keys, _U64)
    have = min(int(count), cap)
    rows = key_row(keys[:have]).astype(np.int64)
    assert rows.size == np.unique(rows).size, "a row was appended twice"
    assert rows.size == 0 or rows.max() < n_rows, "a row past the end was appended"
    allowed = np.ones(n_rows, bool) if mask is None else mask_bits(mask, n_rows)
    assert allowed[rows].all(), "a masked-out row was appended"
    assert not (cls[rows] == 1).any(), "a row with a NaN element was appended"
    with np.errstate(invalid="ignore"):
        must = allowed & ((cls == 2) | ((cls == 0) & (truth >= t)))
        may = allowed & ((cls == 2) | ((cls == 0) & (truth >= t - 2.0 * m64 * (1 + M_SLACK))))
    kept = np.zeros(n_rows, bool)
    kept[rows] = True
    if int(count) <= cap:
        missing = np.flatnonzero(must & ~kept)
        assert missing.size == 0, ("SAFETY: rows at or above the threshold were dropped", t, missing[:8], truth[missing][:8])
    else:
        assert int(count) >= int(must.sum()), ("count below the rows that must be kept", int(count), int(must.sum()))
    loose = np.flatnonzero(kept & ~may)
    assert loose.size == 0, ("TIGHTNESS: kept rows further than 2 m below the threshold", t, loose[:8], truth[loose][:8], m64[loose][:8])
    assert int(must.sum()) <= int(count) <= int(may.sum()), (int(must.sum()), int(count), int(may.sum()))
    return kept


def sample_rows(grp, tile_stride, n_rows):
    """The rows the documented mapping assigns to sampled group grp: row0 = (grp >> 2) * tile_stride * 256 + (grp & 3) * 64."""
    row0 = (grp >> 2) * tile_stride * 256 + (grp & 3) * 64
    return np.arange(row0, min(row0 + 64, n_rows)) if row0 < n_rows else np.arange(0)


def check_halfmax(halfmax, num_tiles, tile_stride, n_rows, truth, m64, cls, mask=None):
    """One query's sampled lower bounds: 0 exactly when no row of the group may vouch; otherwise the low half names the group
    and the score is a VALID lower bound (<= the best float64 score among the group's vouching rows) that is not needlessly
    low (>= the best of score - 2 m64 (1 + 2e-5) among them)."""
    halfmax = np.asarray(halfmax, _U64)
    assert halfmax.shape == (num_tiles * 4,)
    allowed = np.ones(n_rows, bool) if mask is None else mask_bits(mask, n_rows)
    for grp in range(num_tiles * 4):
        rows = sample_rows(grp, tile_stride, n_rows)
        rows = rows[(cls[rows] == 0) & allowed[rows]]
        key = int(halfmax[grp])
        if rows.size == 0:
            assert key == 0, ("a group without a vouching row has a lower bound", grp, hex(key))
            continue
        assert key != 0, ("a group with vouching rows has none", grp)
        assert int(key_row(np.array([key], _U64))[0]) == grp, ("the key does not name its group", grp, hex(key))
        lo = float(ord2f(key_ord(np.array([key], _U64)))[0])
        best = float(truth[rows].max())
        floor = float((truth[rows] - 2.0 * m64[rows] * (1 + M_SLACK)).max())
        assert lo <= best, ("NOT a lower bound of the group's best score", grp, lo, best)
        assert lo >= floor, ("lower bound further than 2 m below the group's best", grp, lo, floor)


def mask_bits(mask, n_rows):
    mask = np.asarray(mask, _U32)
    r = np.arange(n_rows)
    return ((mask[r >> 5] >> (r & 31).astype(_U32)) & _U32(1)).astype(bool)


def thresholds_from(truth, cls, rng, extra=()):
    """Thresholds that sit ON the rows' own scores: the fp32 neighbours of exact scores, values inside the densest cluster of
    near-equal scores, both zeros, both infinities."""
    fin = np.sort(truth[cls == 0])
    out = [np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf)]
    if fin.size:
        picks = fin[rng.integers(0, fin.size, 4)].tolist() + [fin[0], fin[-1], fin[fin.size // 2]]
        if fin.size > 8:  # the densest cluster: the 8 consecutive sorted scores that span the least
            i = int(np.argmin(fin[7:] - fin[:-7]))
            picks += [fin[i], fin[i + 3], 0.5 * (fin[i + 3] + fin[i + 4]), fin[i + 7]]
        for v in picks:
            with np.errstate(over="ignore"):
                f = np.float32(v)
            if np.isfinite(f):
                out += [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    out += [np.float32(e) for e in extra]
    return out


# --------------------------------------------------------------------------- #
# the library
# --------------------------------------------------------------------------- #
class _SelScan8(C.Structure):
    _fields_ = [("phase", C.c_int32), ("metric", C.c_int32), ("n_rows", C.c_uint32), ("dim", C.c_uint32), ("qquads", C.c_uint32),
                ("nq", C.c_uint32), ("num_tiles", C.c_uint32), ("tile_stride", C.c_uint32), ("sample_nt", C.c_uint32),
                ("tau_n", C.c_uint32), ("tau_k", C.c_int32), ("cap", C.c_uint32), ("grid_x", C.c_uint32)]


class _SelScan6(C.Structure):
    _fields_ = [("sample", C.c_int32), ("n_rows", C.c_uint32), ("units", C.c_uint32), ("qpitch", C.c_uint32), ("nq", C.c_uint32),
                ("num_tiles", C.c_uint32), ("tile_stride", C.c_uint32), ("cap", C.c_uint32), ("grid_x", C.c_uint32)]


_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        lib.sel_scan8_shape.argtypes = [u32, C.POINTER(u32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
        lib.sel_u6_unit_chunk.argtypes = [u32]
        lib.sel_u6_cut_seg.argtypes = []
        lib.sel_u6_cut_seg.restype = u32
        lib.sel_rows_to_u8.argtypes = [vp, u64, u64, u64, u32, u32, u32, u32, vp, vp]
        lib.sel_rows_to_u6.argtypes = [vp, u64, u64, u64, u32, u32, u32, vp, vp]
        lib.sel_row_sqnorm.argtypes = [vp, u64, u64, u64, u32, u32, vp, vp]
        lib.sel_g8_offset.argtypes = [u64, u32, u32]
        lib.sel_g8_offset.restype = u64
        lib.sel_rows_to_i8g.argtypes = [vp, u64, u64, u64, u64, u32, u32, u32, u32, vp, vp, vp]
        lib.sel_queries_to_i8.argtypes = [vp, u32, u32, u32, u32, u32, u32, vp, vp, vp, vp, vp]
        lib.sel_scan8.argtypes = [C.POINTER(_SelScan8), vp, u64, vp, vp, vp, vp, vp, vp, vp, u64, vp, u64, vp]
        lib.sel_scan6.argtypes = [C.POINTER(_SelScan6), vp, u64, vp, vp, vp, vp, u64, vp, u64, vp, vp]
        lib.sel_rescore.argtypes = [i32, vp, u64, u32, vp, u32, vp, u64, vp, u32, u32]
        lib.sel_u6_cut.argtypes = [vp, vp, u32, i32, u32, vp, u64, vp, u32]
        for f in (lib.sel_scan8_shape, lib.sel_u6_unit_chunk, lib.sel_rows_to_u8, lib.sel_rows_to_u6, lib.sel_row_sqnorm, lib.sel_rows_to_i8g, lib.sel_queries_to_i8, lib.sel_scan8,
                  lib.sel_scan6, lib.sel_rescore, lib.sel_u6_cut):
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


def _c(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def scan8_shape(dim):
    """(pieces, L, QPL, has a scan8_sample4 instance) as the library's scan8_shape answers, None when no instance serves dim."""
    p, L, q, s4 = C.c_uint32(0), C.c_int(0), C.c_int(0), C.c_int(0)
    if load().sel_scan8_shape(int(dim), C.byref(p), C.byref(L), C.byref(q), C.byref(s4)):
        return None
    return p.value, L.value, q.value, bool(s4.value)


def u6_unit_chunk(units):
    return load().sel_u6_unit_chunk(int(units))


def rows_to_u8(rows, dim, r0=0, n=None, grid=0, pitch8=None):
    """rows: [n_alloc, pitch] fp32.  -> (bytes [n_alloc, pitch8] uint8, scale bit patterns [n_alloc] uint32); rows outside
    [r0, n) keep the sentinels."""
    rows = _c(rows, _F32)
    n_alloc, pitch = rows.shape
    n = n_alloc if n is None else n
    pitch8 = scan8_shape_py(dim)[0] * 16 if pitch8 is None else pitch8
    out, scale = np.full((n_alloc, pitch8), SENT_BYTE, _U8), np.full(n_alloc, SENT_F32, _U32)
    _check(load().sel_rows_to_u8(_ptr(rows), n_alloc, int(r0), int(n), int(dim), pitch, pitch8, int(grid), _ptr(out), _ptr(scale)),
           "sel_rows_to_u8")
    return out, scale


def rows_to_u6(rows, dim, r0=0, n=None, grid=0):
    """rows: [n_alloc, pitch] fp32, pitch a multiple of 16.  -> (dwords [tiles, units, 64, 3] uint32, {s, a} bit patterns
    [n_alloc, 2] uint32); what the kernel leaves alone keeps the sentinels."""
    rows = _c(rows, _F32)
    n_alloc, pitch = rows.shape
    n = n_alloc if n is None else n
    codes = np.full(((n_alloc + 63) // 64, pitch // 16, 64, 3), SENT_U32, _U32)
    sa = np.full((n_alloc, 2), SENT_F32, _U32)
    _check(load().sel_rows_to_u6(_ptr(rows), n_alloc, int(r0), int(n), int(dim), pitch, int(grid), _ptr(codes), _ptr(sa)), "sel_rows_to_u6")
    return codes, sa


def row_sqnorm(rows, r0=0, n=None, grid=0, stats=None):
    """-> (cn bit patterns [n_alloc] uint32, the statistics words [3] uint32 or None)."""
    rows = _c(rows, _F32)
    n_alloc, pitch = rows.shape
    n = n_alloc if n is None else n
    cn = np.full(n_alloc, SENT_F32, _U32)
    st = None if stats is None else np.array(stats, _U32)
    _check(load().sel_row_sqnorm(_ptr(rows), n_alloc, int(r0), int(n), pitch, int(grid), _ptr(cn), _ptr(st)), "sel_row_sqnorm")
    return cn, st


def rows_to_i8g(rows, dim, n_rows=None, g0=0, g1=None, grid=0):
    """rows: [n_alloc, pitch] fp32 of which the first n_rows exist.  -> (bytes in the kernel's order [g1 * 64 * pitch8] int8,
    groups bit patterns [g1, 4] uint32 = {s_g, a_g, b_g, vouch}, gbad [g1] uint64); groups outside [g0, g1) keep the sentinels."""
    rows = _c(rows, _F32)
    n_alloc, pitch = rows.shape
    n_rows = n_alloc if n_rows is None else n_rows
    g1 = (n_rows + 63) // 64 if g1 is None else g1
    pitch8 = i8g_pitch(dim)
    out = np.full(g1 * 64 * pitch8, SENT_BYTE, _U8).view(np.int8)
    groups, gbad = np.full((g1, 4), SENT_F32, _U32), np.full(g1, SENT_KEY, _U64)
    rc = load().sel_rows_to_i8g(_ptr(rows), n_alloc, int(g0), int(g1), int(n_rows), int(dim), pitch, pitch8, int(grid), _ptr(out),
                                _ptr(groups), _ptr(gbad))
    _check(rc, "sel_rows_to_i8g")
    return out, groups, gbad


def queries_to_i8(q, dim, gbn, grid=0):
    """q: [nv, pitch] fp32, a block of gbn >= nv queries.  -> dict(bytes [gbn, pitch8] int8, qpar bit patterns [gbn, 4] uint32 =
    {s_q, E, M, 1 / s_q}, tau [gbn] uint32 bit patterns, count [gbn], lost [1]); everything starts at the sentinels."""
    q = _c(q, _F32)
    nv, pitch = q.shape
    pitch8 = i8g_pitch(dim)
    out = np.full((gbn, pitch8), SENT_BYTE, _U8).view(np.int8)
    qpar, tau = np.full((gbn, 4), SENT_F32, _U32), np.full(gbn, SENT_F32, _U32)
    count, lost = np.full(gbn, SENT_U32, _U32), np.full(1, SENT_U32, _U32)
    rc = load().sel_queries_to_i8(_ptr(q), nv, int(gbn), int(dim), pitch, pitch8, int(grid), _ptr(out), _ptr(qpar), _ptr(tau), _ptr(count),
                                  _ptr(lost))
    _check(rc, "sel_queries_to_i8")
    return {"bytes": out, "qpar": qpar, "tau": tau, "count": count, "lost": lost}


def scan8(phase, metric, shadow, scale, queries, dim, cn=None, mask=None, tau=None, tau_keys=None, tau_k=0, num_tiles=0, tile_stride=1,
          sample_nt=0, cap=0, grid_x=0):
    """One launch of scan8_kernel<phase> (phase 3: scan8_sample4_kernel).  shadow: [n_rows, pieces * 16] uint8; queries:
    [nq, qquads * 4] fp32.  Sample passes -> dict(halfmax [nq, num_tiles * 4] uint64, count [nq]); full passes ->
    dict(cand [nq, cap] uint64, guard [GUARD] uint64 -- the keys behind the last buffer --, count [nq])."""
    shadow, scale, queries = _c(shadow, _U8), _c(scale, _F32), _c(queries, _F32)
    n_rows, nq = shadow.shape[0], queries.shape[0]
    assert scale.shape == (n_rows,) and queries.shape[1] % 4 == 0
    cn, mask, tau, tau_keys = _c(cn, _F32), _c(mask, _U32), _c(tau, _F32), _c(tau_keys, _U64)
    assert cn is None or cn.shape == (n_rows,)
    assert mask is None or mask.shape == ((n_rows + 31) // 32,)
    assert tau is None or tau.shape == (nq,)
    sample = phase in (0, 3)
    halfmax = np.full(nq * num_tiles * 4 + GUARD, SENT_KEY, _U64) if sample else None
    cand = None if sample else np.full(nq * cap + GUARD, SENT_KEY, _U64)
    count = np.full(nq, SENT_U32 if sample else 0, _U32)  # (the sample pass zeroes the counters the full pass adds to)
    d = _SelScan8(int(phase), int(metric), n_rows, int(dim), queries.shape[1] // 4, nq, int(num_tiles), int(tile_stride), int(sample_nt),
                  0 if tau_keys is None else tau_keys.size, int(tau_k), int(cap), int(grid_x))
    rc = load().sel_scan8(C.byref(d), _ptr(shadow), shadow.size, _ptr(scale), _ptr(cn), _ptr(queries), _ptr(mask), _ptr(tau),
                          _ptr(tau_keys), _ptr(halfmax), 0 if halfmax is None else halfmax.size, _ptr(cand),
                          0 if cand is None else cand.size, _ptr(count))
    _check(rc, "sel_scan8")
    if sample:
        return {"halfmax": halfmax[:nq * num_tiles * 4].reshape(nq, num_tiles * 4), "guard": halfmax[nq * num_tiles * 4:], "count": count}
    return {"cand": cand[:nq * cap].reshape(nq, cap), "guard": cand[nq * cap:], "count": count}


def scan6(sample, codes, sa, queries, n_rows, tau=None, num_tiles=0, tile_stride=1, cap=0, grid_x=0):
    """One launch of scan8_u6_sample_kernel / scan8_u6_kernel.  codes: [tiles, units, 64, 3] uint32; sa: [n_rows, 2] fp32;
    queries: [nq, qpitch] fp32.  Returns as :func:`scan8`, plus count2 [nq]."""
    codes, sa, queries, tau = _c(codes, _U32), _c(sa, _F32), _c(queries, _F32), _c(tau, _F32)
    nq, units = queries.shape[0], codes.shape[1]
    assert codes.shape == ((n_rows + 63) // 64, units, 64, 3) and sa.shape == (n_rows, 2)
    assert tau is None or tau.shape == (nq,)
    halfmax = np.full(nq * num_tiles * 4 + GUARD, SENT_KEY, _U64) if sample else None
    cand = None if sample else np.full(nq * cap + GUARD, SENT_KEY, _U64)
    count, count2 = np.full(nq, SENT_U32 if sample else 0, _U32), np.full(nq, SENT_U32, _U32)
    d = _SelScan6(int(bool(sample)), int(n_rows), units, queries.shape[1], nq, int(num_tiles), int(tile_stride), int(cap), int(grid_x))
    rc = load().sel_scan6(C.byref(d), _ptr(codes), codes.size, _ptr(sa), _ptr(queries), _ptr(tau), _ptr(halfmax),
                          0 if halfmax is None else halfmax.size, _ptr(cand), 0 if cand is None else cand.size, _ptr(count), _ptr(count2))
    _check(rc, "sel_scan6")
    if sample:
        return {"halfmax": halfmax[:nq * num_tiles * 4].reshape(nq, num_tiles * 4), "guard": halfmax[nq * num_tiles * 4:], "count": count,
                "count2": count2}
    return {"cand": cand[:nq * cap].reshape(nq, cap), "guard": cand[nq * cap:], "count": count, "count2": count2}


def rescore(metric, rows, queries, cand, count, grid_x=0):
    """rescore_kernel<metric> in place on a copy of cand [nq, cap] -> (keys [nq, cap], guard [GUARD])."""
    rows, queries, cand, count = _c(rows, _F32), _c(queries, _F32), _c(cand, _U64), _c(count, _U32)
    nq, cap = cand.shape
    assert rows.shape[1] % 4 == 0 and queries.shape == (nq, rows.shape[1]) and count.shape == (nq,)
    buf = np.concatenate([cand.reshape(-1), np.full(GUARD, SENT_KEY, _U64)])
    rc = load().sel_rescore(int(metric), _ptr(rows), rows.shape[0], rows.shape[1] // 4, _ptr(queries), nq, _ptr(buf), buf.size, _ptr(count),
                            cap, int(grid_x))
    _check(rc, "sel_rescore")
    return buf[:nq * cap].reshape(nq, cap), buf[nq * cap:]


def u6_cut(cand, count, k, cap2, count2_init=0):
    """u6_cut_kernel on cand [nq, cap] -> (short lists [nq, cap2], guard [GUARD], count2 [nq])."""
    cand, count = _c(cand, _U64), _c(count, _U32)
    nq, cap = cand.shape
    out = np.full(nq * cap2 + GUARD, SENT_KEY, _U64)
    count2 = np.full(nq, count2_init, _U32)
    _check(load().sel_u6_cut(_ptr(cand), _ptr(count), cap, int(k), nq, _ptr(out), out.size, _ptr(count2), int(cap2)), "sel_u6_cut")
    return out[:nq * cap2].reshape(nq, cap2), out[nq * cap2:], count2
