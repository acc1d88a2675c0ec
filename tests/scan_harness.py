"""ctypes loader of tests/kernel_harness/libscan_harness.so (built by ``make -C wdbx-py_amd/csrc all``), an independent Python
restatement of the fp32 scan's shape rules, numpy models of the documented behaviour, and the property checkers of
tests/test_gpu_scan_kernels.py and tests/test_gpu_range_kernels.py.

The harness launches the library's own ``scan_kernel`` / ``scan_kernel_generic`` instance for a pitch and the scan options,
``scan_kernel_listed``, the picked ``range_scan_kernel`` instance and ``range_filter_kernel`` on arrays the caller hands it.

The checkers are plain numpy and never look at the code under test.  tests/test_scan_checkers.py feeds them the models of
this file on the CPU, and a list of deliberately wrong models that they must reject."""
import ctypes as C
from pathlib import Path

import numpy as np

from rank_harness import METRIC_COSINE, METRIC_L2, f2ord, key_ord, key_row, make_keys, ord2f  # noqa: F401  (re-exported)
from select_harness import GUARD, SENT_KEY, SENT_U32, gamma, mask_bits  # noqa: F401  (re-exported)

ROOT = Path(__file__).resolve().parent.parent
LIBRARY = ROOT / "tests" / "kernel_harness" / "libscan_harness.so"

_U32, _U64, _F32, _F64, _I64 = np.uint32, np.uint64, np.float32, np.float64, np.int64
LANES = (0, 8, 16, 32, 64)  # the settings of option scan_lanes


# --------------------------------------------------------------------------- #
# the shape rules, restated from choose_scan / plan_scan / pick_range_scan as they stood before host_scan_plan.h existed
# --------------------------------------------------------------------------- #
def scan_form_py(pitch4, lanes=0, generic=0, force_ragged=0):
    """-> (L, QPL, ragged, generic); QPL = 0 for the generic kernel."""
    if not generic and pitch4 < 16 and not lanes:
        for L, Q in ((1, 1), (2, 1), (4, 1), (8, 1), (4, 2), (4, 3), (8, 2)):
            slots = L * Q
            waste = slots - pitch4
            if waste < 0 or waste * 8 > slots * 3:
                continue
            return L, Q, bool(waste != 0 or force_ragged), False
    if not generic and pitch4 >= 16:
        aligned = pitch4 % 8 == 0
        best_l, best_q, best_waste = 0, 0, 1 << 30
        for tier in (0, 1):
            if tier == 1 and (aligned or best_l >= 16):
                break
            for L in (8, 16, 32, 64):
                if lanes and L != lanes:
                    continue
                if tier == 1 and (L < 16 or L > 32):
                    continue
                for Q in ((3, 4, 6, 8, 12) if tier == 0 else (1, 2)):
                    waste = L * Q - pitch4
                    if waste < 0 or waste * 3 > L * Q:
                        continue
                    if (waste < best_waste) if aligned else (L > best_l or (L == best_l and waste < best_waste)):
                        best_l, best_q, best_waste = L, Q, waste
        if best_l and best_waste * 3 <= best_l * best_q:
            return best_l, best_q, bool(best_waste != 0 or force_ragged), False
    return generic_lanes_py(pitch4), 0, False, True


def generic_lanes_py(pitch4):
    L = 1
    while L < 8 and L < pitch4:
        L *= 2
    return 64 if pitch4 > 768 else L


def passes_in_flight_py(qpl):
    """U of scan_body; the generic body has one pass in flight."""
    return 1 if qpl == 0 or qpl >= 12 else 2 if qpl >= 6 else 3 if qpl >= 4 else 4 if qpl == 3 else 6 if qpl == 2 else 8


def range_form_py(pitch4):
    """-> (P, NI) of range_scan_kernel."""
    for bound, form in ((1, (1, 1)), (2, (2, 1)), (4, (4, 1)), (8, (8, 1)), (16, (16, 1)), (32, (32, 1)), (64, (64, 1)),
                        (128, (64, 2)), (192, (64, 3)), (256, (64, 4))):
        if pitch4 <= bound:
            return form
    return 64, 0


def range_passes_py(ni):
    return 1 if ni == 0 else 2 if ni >= 3 else 4


def plan_py(n_rows, L, k, select, lds_lists, lds_extra, cu_count, per_cu, opt_blocks, wg_merge, blocked):
    """plan_scan's numbers -> (mode, groups, max_blocks, blocks, partial lists, chunk, LDS bytes, needs the attribute)."""
    R = 64 // L
    groups = (n_rows + R - 1) // R
    lds = (0 if select else 4 * k * 8) + lds_extra
    blocks = (cu_count * min(per_cu, 2)) & 0xFFFFFFFF
    if opt_blocks > 0:
        blocks = opt_blocks & 0xFFFFFFFF
    max_blocks = max(1, ((groups + 3) & 0xFFFFFFFF) // 4)  # (32-bit arithmetic, as the parent's)
    blocks = max(1, min(blocks, max_blocks))
    mode = 2 if select else 1 if (k <= 128 and not lds_lists) else 0
    return (mode, groups, max_blocks, blocks, blocks if wg_merge else blocks * 4,
            ((groups + blocks * 4 - 1) & 0xFFFFFFFF) // (blocks * 4) if blocked else 0, lds, int(lds > 64 * 1024))


def enumerate_forms(max_pitch4=768):
    """Every specialised form the picker returns over pitches 1 .. max_pitch4 and the lane settings -> {form: (pitch4, lanes)}
    with the FIRST pitch that yields it; forms are (L, QPL, ragged)."""
    first = {}
    for p in range(1, max_pitch4 + 1):
        for lanes in LANES:
            L, Q, ragged, gen = scan_form_py(p, lanes)
            if not gen:
                first.setdefault((L, Q, ragged), (p, lanes))
    return first


def enumerate_generic(max_pitch4=1000):
    """{L: (pitch4, lanes)} of the generic kernel, first pitch each; lanes = 8 is how a short row reaches it without
    scan_generic."""
    first = {}
    for p in range(1, max_pitch4 + 1):
        for lanes in LANES:
            L, _, _, gen = scan_form_py(p, lanes)
            if gen:
                first.setdefault(L, (p, lanes))
    return first


def enumerate_range(max_pitch4=1000):
    first = {}
    for p in range(1, max_pitch4 + 1):
        first.setdefault(range_form_py(p), p)
    return first


GENERIC_WIDE_PITCH4 = 777  # just above 768, not a multiple of 8 * 64: the eight-load loop, the pair loop (twice) and the single tail all run


def scan_cases():
    """The launches the GPU tests parametrise over: (id, pitch4, lanes, generic, force_ragged, (L, QPL, ragged, generic))."""
    out = []
    for (L, Q, ragged), (p, lanes) in sorted(enumerate_forms().items()):
        out.append((f"L{L}q{Q}{'r' if ragged else 'e'}-p{p}", p, lanes, 0, 0, (L, Q, ragged, False)))
        if not ragged:  # the exact fits, forced onto their ragged instance
            out.append((f"L{L}q{Q}forced-p{p}", p, lanes, 0, 1, (L, Q, True, False)))
    for L, (p, lanes) in sorted(enumerate_generic().items()):
        if L == 64:
            p = GENERIC_WIDE_PITCH4
        out.append((f"genericL{L}-p{p}", p, lanes, 1 if L != 64 else 0, 0, (L, 0, False, True)))
    return out


# --------------------------------------------------------------------------- #
# corpora and truth
# --------------------------------------------------------------------------- #
def int_corpus(rng, n, d, nq=1):
    """Small integers in [-4, 4] as fp32: up to 3200 elements every partial sum of either metric stays below 2^24."""
    assert d <= 3200
    return rng.integers(-4, 5, (n, d)).astype(_F32), rng.integers(-4, 5, (nq, d)).astype(_F32)


def float_corpus(rng, n, d, nq=1):
    return rng.standard_normal((n, d)).astype(_F32), rng.standard_normal((nq, d)).astype(_F32)


def truth64(rows, q, metric):
    """(value, S) in float64 from the fp32 operands: value = c.q or -sum (c - q)^2 (what IEEE gives on infinities and NaNs),
    S = sum |c_i q_i| or sum (c_i - q_i)^2, the scale of the rounding-error band."""
    r, qq = np.asarray(rows, _F32).astype(_F64), np.asarray(q, _F32).astype(_F64)
    with np.errstate(invalid="ignore", over="ignore"):
        if metric == METRIC_L2:
            S = ((r - qq) ** 2).sum(axis=1)
            return -S, S
        return (r * qq).sum(axis=1), np.abs(r * qq).sum(axis=1)


def exact_keys(rows, q, metric, mask=None):
    """Integer corpus: the keys of every row from int64 arithmetic (0 for a masked-out row)."""
    r, qq = np.asarray(rows).astype(_I64), np.asarray(q).astype(_I64)
    s = -(((r - qq) ** 2).sum(axis=1)) if metric == METRIC_L2 else r @ qq
    assert np.abs(s).max(initial=0) < 2 ** 24
    keys = make_keys(f2ord(s.astype(_F32) + _F32(0.0)), np.arange(len(r)))
    if mask is not None:
        keys = np.where(mask_bits(mask, len(r)), keys, _U64(0))
    return keys


def scan_roundings(L, qpl, pitch4, generic, metric):
    """m: the longest chain of fp32 roundings between the operands and a row's score.
    Specialised: a lane's QPL fmas into one accumulator component, the fold (x + y) + (z + w) (2), log2 L tree steps.
    Generic: two accumulators, each ceil(ceil(pitch4 / L) / 2) fmas deep, the fold ((x0 + x1) + (y0 + y1)) + (...) (3), the
    tree.  L2 adds the rounding of the difference c - q, which enters squared -- two factors (1 + e) -- so it counts twice (the
    square itself enters the fma unrounded)."""
    tree = int(np.log2(L))
    if generic:
        per_lane = (pitch4 + L - 1) // L
        m = (per_lane + 1) // 2 + 3 + tree
    else:
        m = qpl + 2 + tree
    return m + (2 if metric == METRIC_L2 else 0)


def range_roundings(P, pitch4, metric):
    """exact_score: ceil(pitch4 / P) fmas per lane, the fold (2), log2 P tree steps; L2: + the squared difference (2)."""
    return (pitch4 + P - 1) // P + 2 + int(np.log2(P)) + (2 if metric == METRIC_L2 else 0)


def row_class(rows):
    """0 finite, 1 holds a NaN, 2 holds an infinity and no NaN."""
    rows = np.asarray(rows)
    nan = np.isnan(rows).any(axis=1)
    return np.where(nan, 1, np.where(np.isinf(rows).any(axis=1), 2, 0))


def special_masks(n, rng):
    """name -> mask words: all ones, all zeros, random, and one whose only allowed rows sit at bits 0 and 31 of a word and in
    the last (partial) word."""
    words = (n + 31) // 32
    edge = np.zeros(words, _U32)
    edge[0] = 0x80000001 if n >= 32 else 1
    edge[-1] |= _U32(1) << _U32((n - 1) & 31)  # the last row
    if words > 2:
        edge[words // 2] = 0x80000001
    return {"ones": np.full(words, 0xFFFFFFFF, _U32), "zeros": np.zeros(words, _U32),
            "random": rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(_U32), "edge": edge}


# --------------------------------------------------------------------------- #
# the documented partition
# --------------------------------------------------------------------------- #
def wave_rows(L, n_rows, grid_x, chunk, wave):
    """The rows wave `wave` of the grid visits: row groups of 64 / L rows; strided (chunk = 0): groups wave, wave + W, ...;
    blocked: groups [wave * chunk, (wave + 1) * chunk)."""
    R = 64 // L
    groups = (n_rows + R - 1) // R
    W = grid_x * 4
    g = np.arange(wave * chunk, min((wave + 1) * chunk, groups)) if chunk else np.arange(wave, groups, W)
    rows = (g[:, None] * R + np.arange(R)[None, :]).reshape(-1)
    return rows[rows < n_rows]


def list_rows(L, n_rows, grid_x, chunk, wg_merge):
    """The rows behind every partial list of a launch, in list order."""
    per_wave = [wave_rows(L, n_rows, grid_x, chunk, w) for w in range(grid_x * 4)]
    if not wg_merge:
        return per_wave
    return [np.concatenate(per_wave[4 * b:4 * b + 4]) for b in range(grid_x)]


def top_keys(keys, k):
    """The k largest non-zero keys in descending order, zeros behind."""
    keys = np.asarray(keys, _U64)
    keys = np.sort(keys[keys != 0])[::-1][:k]
    return np.concatenate([keys, np.zeros(k - keys.size, _U64)])


# --------------------------------------------------------------------------- #
# checkers
# --------------------------------------------------------------------------- #
def check_dump(part, n_rows, cls, mask=None, exact=None, value=None, band=None):
    """A mode-2 launch: part = the whole partials array of one query (n_rows keys, then what must stay untouched).
    Masked-out rows and rows with a NaN element are exactly 0; every other key names its row; its score equals the integer
    reference (exact: [n_rows] keys) or lies within band of value (an infinite value: equal); a zero value inside a zero band is
    +0; nothing at or beyond n_rows is written."""
    part = np.asarray(part, _U64)
    assert (part[n_rows:] == _U64(SENT_KEY)).all(), "a key at or beyond n_rows (or the guard) was written"
    keys = part[:n_rows]
    allowed = np.ones(n_rows, bool) if mask is None else mask_bits(mask, n_rows)
    dead = ~allowed | (cls == 1)
    assert (keys[dead] == 0).all(), ("a masked-out or NaN row has a key", np.flatnonzero(dead & (keys != 0))[:8])
    live = np.flatnonzero(~dead)
    assert (keys[live] != _U64(SENT_KEY)).all(), ("a row was never written", live[keys[live] == _U64(SENT_KEY)][:8])
    assert np.array_equal(key_row(keys[live]).astype(_I64), live), "a key names another row"
    if exact is not None:
        want = np.where(dead, _U64(0), np.asarray(exact, _U64))
        bad = np.flatnonzero(keys != want)
        assert bad.size == 0, ("key != integer reference", bad[:8], [hex(int(x)) for x in keys[bad][:4]], [hex(int(x)) for x in want[bad][:4]])
        return
    got = ord2f(key_ord(keys[live])).astype(_F64)
    v, b = np.asarray(value, _F64)[live], np.asarray(band, _F64)[live]
    assert not np.isnan(got).any(), "a key carries a NaN score"
    fin = np.isfinite(v)
    assert np.array_equal(got[~fin], v[~fin]), ("an infinite row's score", live[~fin][:8], got[~fin][:8], v[~fin][:8])
    err = np.abs(got[fin] - v[fin])
    bad = ~(err <= b[fin])
    assert not bad.any(), ("score outside gamma(m) S", live[fin][bad][:8], err[bad][:8], b[fin][bad][:8])
    zero = live[(v == 0) & (b == 0)]
    assert (key_ord(keys[zero]) == _U32(0x80000000)).all(), "a zero score is not +0"


def check_lists(partials, k, n_lists, rows_of_list, row_keys):
    """A list-mode launch: partials = one query's k * n_lists keys in the transposed layout partials[i * n_lists + list].
    Every list equals the k largest non-zero keys of the rows behind it (row_keys: [n_rows] dump keys), descending, zeros
    only behind the real keys."""
    lists = np.asarray(partials, _U64)[:k * n_lists].reshape(k, n_lists)
    assert len(rows_of_list) == n_lists
    for p, rows in enumerate(rows_of_list):
        want = top_keys(np.asarray(row_keys, _U64)[rows], k)
        got = lists[:, p]
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            raise AssertionError(("partial list", p, "entry", i, hex(int(got[i])), hex(int(want[i])), "rows behind it", len(rows)))


def range_passes(keys, thr, metric):
    """The documented rule on the keys' own scores: cosine score >= thr, L2 distance <= thr, NaN (a zero key) never."""
    keys = np.asarray(keys, _U64)
    s = ord2f(key_ord(keys))
    with np.errstate(invalid="ignore"):
        ok = (-s <= _F32(thr)) if metric == METRIC_L2 else (s >= _F32(thr))
    return ok & (keys != 0)


def check_range(out, guard, count, cap, want_keys):
    """One query of a range launch: count is the exact total, also past cap; out[:min(count, cap)] are distinct expected keys --
    all of them when they fit; every slot behind them and the guard are untouched."""
    out, want = np.asarray(out, _U64), np.asarray(want_keys, _U64)
    assert int(count) == want.size, ("count is not the exact total", int(count), want.size)
    have = min(int(count), cap)
    got = out[:have]
    assert np.unique(got).size == have, "a key was emitted twice"
    assert np.isin(got, want).all(), ("a key that does not pass (or a wrong score)", [hex(int(x)) for x in got[~np.isin(got, want)][:4]])
    if want.size <= cap:
        assert np.array_equal(np.sort(got), np.sort(want)), "a passing row is missing"
    assert (out[have:] == _U64(SENT_KEY)).all(), "a slot behind the emitted keys was written"
    assert (np.asarray(guard, _U64) == _U64(SENT_KEY)).all(), "the guard was written"


# --------------------------------------------------------------------------- #
# numpy models of the documented behaviour (tests/test_scan_checkers.py); `mutant` names a deliberate fault
# --------------------------------------------------------------------------- #
def model_dump(rows, q, metric, L, qpl, n_alloc, mask=None, mutant=None):
    """Mode 2 of an instance with L * qpl slots per row -> [n_alloc] keys (SENT_KEY behind the rows)."""
    rows, q = np.asarray(rows, _F32), np.asarray(q, _F32)
    n, d = rows.shape
    r, qq = rows.astype(_F64), q.astype(_F64)
    if mutant == "last_quad_dropped":
        r, qq = r[:, :d - 4], qq[:d - 4]
    with np.errstate(invalid="ignore", over="ignore"):
        s = -((r - qq) ** 2).sum(axis=1) if metric == METRIC_L2 else (r * qq).sum(axis=1)
        if mutant == "idle_slot_not_zeroed" and L * qpl * 4 > d:  # the clamped slot adds the last quad once more
            lr, lq = rows[:, d - 4:].astype(_F64), q[d - 4:].astype(_F64)
            s = s + (-((lr - lq) ** 2).sum(axis=1) if metric == METRIC_L2 else (lr * lq).sum(axis=1))
        if mutant == "l2_sign" and metric == METRIC_L2:
            s = -s
        s32 = s.astype(_F32) + _F32(0.0)
    keys = make_keys(f2ord(s32), np.arange(n))
    allowed = np.ones(n, bool) if mask is None else mask_bits(mask, n)
    if mutant == "mask_shifted" and mask is not None:
        allowed = np.concatenate([[True], allowed[:-1]])
    keys = np.where(allowed & ~np.isnan(s32), keys, _U64(0))
    out = np.full(n_alloc, SENT_KEY, _U64)
    out[:n] = keys
    if mutant == "last_row_skipped":
        out[n - 1] = SENT_KEY
    return out


def model_lists(row_keys, k, L, n_rows, grid_x, chunk, wg_merge, mutant=None):
    """List modes -> the transposed partials [k * n_lists]."""
    behind = list_rows(L, n_rows, grid_x, chunk, wg_merge)
    out = np.zeros((k, len(behind)), _U64)
    for p, rows in enumerate(behind):
        if mutant == "last_row_skipped":
            rows = rows[rows != n_rows - 1]
        keys = np.asarray(row_keys, _U64)[rows]
        if mutant == "last_row_twice" and (rows == n_rows - 1).any():
            keys = np.concatenate([keys, keys[rows == n_rows - 1]])
        keys = keys[keys != 0]
        if mutant == "ties_higher_row_first":  # order by (score, row) instead of (score, ~row)
            order = np.lexsort((key_row(keys), key_ord(keys)))[::-1]
            col = keys[order]
        else:
            col = np.sort(keys)[::-1]
        if mutant == "lost_on_64_boundary" and col.size > 64:  # the entry that moves from register 0 to register 1 is dropped
            col = np.delete(col, 64)
        col = col[:k]
        out[:col.size, p] = col
    return out.reshape(-1)


def model_range(row_keys, thr, metric, cap, n_out, mask=None, mutant=None, stage_order=None):
    """Range scan / filter over candidate keys -> (out [n_out], count): passing keys appended through a 64-key stage."""
    keys = np.asarray(row_keys, _U64)
    ok = range_passes(keys, thr, metric)
    if mutant == "gt_for_ge":
        s = ord2f(key_ord(keys))
        with np.errstate(invalid="ignore"):
            ok = ((-s < _F32(thr)) if metric == METRIC_L2 else (s > _F32(thr))) & (keys != 0)
    if mask is not None:
        allowed = mask_bits(mask, keys.size)
        if mutant == "mask_shifted":
            allowed = np.concatenate([[True], allowed[:-1]])
        ok &= allowed
    passing = keys[ok]
    if mutant == "last_row_twice" and ok[-1]:
        passing = np.concatenate([passing, keys[-1:]])
    if mutant == "flush_remainder_dropped":  # pushes of 48 keys: every flush of 64 leaves a remainder that is lost
        kept, fill = [], 0
        for i in range(0, passing.size, 48):
            chunk = passing[i:i + 48]
            if fill + chunk.size >= 64:
                kept.append(chunk[:64 - fill])
                fill = 0
            else:
                kept.append(chunk)
                fill += chunk.size
        passing = np.concatenate(kept) if kept else passing
    out = np.full(n_out, SENT_KEY, _U64)
    m = min(passing.size, cap)
    out[:m] = passing[:m]
    count = passing.size
    if mutant == "count_clamped":
        count = min(count, cap)
    return out, count


# --------------------------------------------------------------------------- #
# the library
# --------------------------------------------------------------------------- #
class _ScnScan(C.Structure):
    _fields_ = [("listed", C.c_int32), ("lanes", C.c_int32), ("generic", C.c_int32), ("force_ragged", C.c_int32), ("nt", C.c_int32),
                ("metric", C.c_int32), ("mode", C.c_int32), ("k", C.c_int32), ("n_rows", C.c_uint32), ("pitch4", C.c_uint32),
                ("grid_x", C.c_uint32), ("grid_y", C.c_uint32), ("chunk", C.c_uint32), ("wg_merge", C.c_int32),
                ("over_cap", C.c_uint32), ("y_partials", C.c_uint32)]


_lib = None


def load():
    global _lib
    if _lib is None:
        if not LIBRARY.exists():
            raise FileNotFoundError(f"{LIBRARY} is missing: build it with `make -C wdbx-py_amd/csrc all`")
        lib = C.CDLL(str(LIBRARY))
        vp, u32, u64, i32, ip = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_int)
        lib.scn_scan_form.argtypes = [i32, i32, i32, i32, ip, ip, ip, ip, ip]
        lib.scn_listed_lanes.argtypes = [i32]
        lib.scn_range_form.argtypes = [u32, ip, ip, ip]
        lib.scn_plan.argtypes = [u64, i32, i32, i32, i32, u64, u32, i32, C.c_int64, i32, i32, vp]
        lib.scn_scan.argtypes = [C.POINTER(_ScnScan), vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64]
        lib.scn_range_scan.argtypes = [i32, vp, u64, u32, vp, u32, vp, vp, u64, vp, u64, vp, u32, u32]
        lib.scn_range_filter.argtypes = [i32, vp, u64, u32, vp, u32, vp, vp, u64, vp, u32, vp, u64, vp, u32, u32]
        for f in (lib.scn_scan_form, lib.scn_listed_lanes, lib.scn_range_form, lib.scn_plan, lib.scn_scan, lib.scn_range_scan,
                  lib.scn_range_filter):
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


def scan_form(pitch4, lanes=0, generic=0, force_ragged=0):
    """(L, QPL, ragged, generic, the pickers have every instance of it) as the library answers."""
    v = [C.c_int(0) for _ in range(5)]
    _check(load().scn_scan_form(int(pitch4), int(lanes), int(generic), int(force_ragged), *[C.byref(x) for x in v]), "scn_scan_form")
    return v[0].value, v[1].value, bool(v[2].value), bool(v[3].value), bool(v[4].value)


def listed_lanes(pitch4):
    return load().scn_listed_lanes(int(pitch4))


def range_form(pitch4):
    v = [C.c_int(0) for _ in range(3)]
    _check(load().scn_range_form(int(pitch4), *[C.byref(x) for x in v]), "scn_range_form")
    return v[0].value, v[1].value, bool(v[2].value)


def plan(n_rows, L, k, select, lds_lists, lds_extra, cu_count, per_cu, opt_blocks, wg_merge, blocked):
    out = np.zeros(8, _U64)
    _check(load().scn_plan(int(n_rows), int(L), int(k), int(select), int(lds_lists), int(lds_extra), int(cu_count), int(per_cu),
                           int(opt_blocks), int(wg_merge), int(blocked), _ptr(out)), "scn_plan")
    return tuple(int(x) for x in out)


def scan(rows, queries, metric, mode, k=1, lanes=0, generic=0, force_ragged=0, nt=1, grid_x=1, chunk=0, wg_merge=0, mask=None,
         only_if_over=None, over_cap=0, y_partials=None, over_list=None, grid_y=None, partials_len=None):
    """One launch.  rows: [n_rows, pitch]; queries: [nq, pitch].  A plain launch scans grid_y = nq queries; with over_list the
    listed repair kernel scans the queries it names on grid_y grid rows.  Returns the partials array [nq, y_partials] uint64
    -- per query k * lists keys (transposed lists) or n_rows keys (mode 2), SENT_KEY wherever nothing was written -- and the
    guard behind it."""
    rows, queries = _c(rows, _F32), _c(queries, _F32)
    n_rows, pitch = rows.shape
    nq = queries.shape[0]
    assert pitch % 4 == 0 and queries.shape[1] == pitch
    lists = grid_x if wg_merge else grid_x * 4
    need = n_rows if mode == 2 else k * lists
    y_partials = need if y_partials is None else y_partials
    mask, only_if_over, over_list = _c(mask, _U32), _c(only_if_over, _U32), _c(over_list, _U32)
    part = np.full((nq * y_partials if partials_len is None else partials_len) + GUARD, SENT_KEY, _U64)
    listed = over_list is not None
    d = _ScnScan(int(listed), int(lanes), int(generic), int(force_ragged), int(nt), int(metric), int(mode), int(k), n_rows, pitch // 4,
                 int(grid_x), int(nq if grid_y is None else grid_y), int(chunk), int(wg_merge), int(over_cap), int(y_partials))
    rc = load().scn_scan(C.byref(d), _ptr(rows), rows.size, _ptr(queries), queries.size, _ptr(mask), 0 if mask is None else mask.size,
                         _ptr(part), part.size, _ptr(only_if_over), 0 if only_if_over is None else only_if_over.size,
                         _ptr(over_list), 0 if over_list is None else over_list.size)
    _check(rc, "scn_scan")
    body = part[:part.size - GUARD]
    return (body.reshape(nq, y_partials) if partials_len is None else body), part[part.size - GUARD:]


def range_scan(metric, rows, queries, thr, cap, mask=None, grid_x=1, count_init=0):
    """-> (out [nq, cap], guard [GUARD], count [nq])."""
    rows, queries, thr, mask = _c(rows, _F32), _c(queries, _F32), _c(thr, _F32), _c(mask, _U32)
    n_rows, pitch = rows.shape
    nq = queries.shape[0]
    assert pitch % 4 == 0 and queries.shape[1] == pitch and thr.shape == (nq,)
    out, count = np.full(nq * cap + GUARD, SENT_KEY, _U64), np.full(nq, count_init, _U32)
    rc = load().scn_range_scan(int(metric), _ptr(rows), n_rows, pitch // 4, _ptr(queries), nq, _ptr(thr), _ptr(mask),
                               0 if mask is None else mask.size, _ptr(out), out.size, _ptr(count), int(cap), int(grid_x))
    _check(rc, "scn_range_scan")
    return out[:nq * cap].reshape(nq, cap), out[nq * cap:], count


def range_filter(metric, rows, queries, thr, cand, cand_count, cap, grid_x=1):
    """cand: [nq, cand_cap] keys.  -> (out [nq, cap], guard [GUARD], count [nq])."""
    rows, queries, thr = _c(rows, _F32), _c(queries, _F32), _c(thr, _F32)
    cand, cand_count = _c(cand, _U64), _c(cand_count, _U32)
    n_rows, pitch = rows.shape
    nq, cand_cap = cand.shape
    assert pitch % 4 == 0 and queries.shape == (nq, pitch) and thr.shape == (nq,) and cand_count.shape == (nq,)
    out, count = np.full(nq * cap + GUARD, SENT_KEY, _U64), np.zeros(nq, _U32)
    rc = load().scn_range_filter(int(metric), _ptr(rows), n_rows, pitch // 4, _ptr(queries), nq, _ptr(thr), _ptr(cand), cand.size,
                                 _ptr(cand_count), cand_cap, _ptr(out), out.size, _ptr(count), int(cap), int(grid_x))
    _check(rc, "scn_range_filter")
    return out[:nq * cap].reshape(nq, cap), out[nq * cap:], count
