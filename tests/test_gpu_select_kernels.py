"""The selection kernels by themselves: the u8 / u6 / i8 quantisers, the row norms, the u8 and u6 selection scans, the exact
re-scoring and the cut, launched by tests/kernel_harness/select_harness.hip on arrays built here.

The promise under test: reduced precision only SELECTS, under a rigorous bound, and the exact fp32 pass decides.  A margin a
little too small, a quantiser that rounds differently from what the proof assumes, a sampled group mapped to the wrong rows,
a padding byte off the zero point lose a true top-k row only on the rare query whose k-th best row sits inside the error
band, so the end-to-end suites on random vectors stay green.  Here the band is where the thresholds are put.

References are numpy: float64 for every "true" score; the float32 restatements of tests/test_selection_bounds*.py for what is
defined element by element (bytes, codes, scales: compared BIT FOR BIT with the kernels' output); properties, with
tolerances derived from fp32 rounding analysis (select_harness.gamma, select_harness.M_SLACK), for what is summed.

The CPU half (no marker) keeps the GPU half honest: the checkers of tests/select_harness.py must accept the restatements on
every family with nothing excluded, and must reject each of a list of deliberately wrong restatements."""
import zlib

import numpy as np
import pytest

import select_harness as S
from test_selection_bounds import (_block_kth_threshold, _datasets, quantise_i8_groups, quantise_i8_query, quantise_u8, u8_bound,
                                   u8_score)
from test_selection_bounds_u6 import _queries, quantise_u6, u6_bound, u6_score

U8, U32, U64, F32, F64 = np.uint8, np.uint32, np.uint64, np.float32, np.float64
COS, L2 = S.METRIC_COSINE, S.METRIC_L2
INF_ORD = 0xFF800000  # f2ord(+inf)

# every entry of kScan8Shapes at its upper edge or one element beyond the previous one (so that padding bytes exist)
U8_DIMS = [100, 128, 129, 384, 400, 768, 1000, 1536, 1537, 3000, 4096]
# units per row of the u6 shadow: every unit chunk 8 .. 4 (24 -> 8, 25 -> 5, 6 -> 6, 7 -> 7, 48 -> 8, 256 -> 8, 20 -> 5, 4 -> 4)
U6_UNITS = [24, 25, 6, 7, 48, 256, 4]


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


# --------------------------------------------------------------------------- #
# inputs
# --------------------------------------------------------------------------- #
def _families(rng, per, d, grid=127):
    """The row families of test_selection_bounds.py, `per` rows each, plus: elements just below the integers of the row's
    quantisation grid (where truncation and rounding differ by a whole step), midpoints of THIS grid, and the special rows
    (one NaN, all NaN, +inf, -inf, all zero)."""
    out = [(name, rows.astype(F32)) for name, rows in _datasets(rng, per, d)]
    below = (rng.integers(1, grid, size=(per, d)) - 0.01) / grid
    below[:, 0] = 1.0
    out.append(("just_below_integers", below.astype(F32)))
    mid = (rng.integers(-(grid - 1), grid, size=(per, d)) + 0.5) / grid
    mid[:, 0] = 1.0
    out.append(("grid_midpoints", mid.astype(F32)))
    sp = rng.standard_normal((8, d)).astype(F32)
    sp[0, d // 2] = np.nan
    sp[1, :] = np.nan
    sp[2, 1] = np.inf
    sp[3, d - 1] = -np.inf
    sp[4, :] = 0.0
    sp[5, 0], sp[5, 2] = np.inf, np.nan  # both: the NaN decides
    out.append(("special", sp))
    return out


def _corpus(rng, per, d, grid=127):
    fams = _families(rng, per, d, grid)
    rows = np.concatenate([r for _, r in fams])
    names = np.concatenate([[name] * len(r) for name, r in fams])
    return rows, names


def _ref_row(names):
    """The row the aligned queries are built for, and whose exact score is always among the thresholds."""
    return int(np.flatnonzero(names == "grid_midpoints")[0])


def _query_list(rng, d, rows, names, grid=127):
    """_queries() of test_selection_bounds_u6.py plus two queries aligned with the quantisation residual of a row on the
    grid's midpoints (every element half a step off): its signs (the L-infinity x L1 bound of the u8 scan is attained) and the
    residual itself (Cauchy-Schwarz of the u6 scan is attained)."""
    qs = [(n, np.asarray(q, F32)) for n, q in _queries(rng, d)]
    c = rows[_ref_row(names)][None, :]
    if grid == 127:
        u, sc = quantise_u8(c)
        r = c[0].astype(F64) - F64(sc[0]) * (u[0].astype(F64) - 128.0)
    else:
        u, sc, _ = quantise_u6(c)
        r = c[0].astype(F64) - F64(sc[0]) * (u[0].astype(F64) - 32.0)
    qs.append(("residual_signs", np.where(r >= 0, 1.0, -1.0).astype(F32)))
    qs.append(("residual", (r / np.abs(r).max()).astype(F32)))
    return qs


def _finite_scores_only(rows, qs, big=1e37):
    """Drops the rows whose scores would leave the fp32 range against one of the queries (the scans' w would be infinite and
    the bound says nothing): a property of the INPUTS, decided in float64 before anything is run."""
    keep = np.ones(len(rows), bool)
    r = np.where(np.isfinite(rows), rows, 0).astype(F64)
    for _, q in qs:
        qq = q.astype(F64)
        keep &= (np.abs(r) @ np.abs(qq) < big) & ((r * r).sum(axis=1) < big)
    return keep


def _cut(rows, names, qs):
    """rows, names without the rows _finite_scores_only drops.  The cut may thin a family (mixed_scales loses its largest
    scales to |c|^2 >= 1e37) but never empty it: at least half of every family stays, on the safe and on the tight side."""
    ok = _finite_scores_only(rows, qs)
    for fam in np.unique(names):
        assert 2 * int(ok[names == fam].sum()) >= int((names == fam).sum()), (fam, int(ok[names == fam].sum()))
    return rows[ok], names[ok]


# --------------------------------------------------------------------------- #
# the kernels' arithmetic restated for the CPU half (what the GPU half gets from the harness)
# --------------------------------------------------------------------------- #
def _restated_u8(rows, q, metric=COS, phase2=False, margin=0.51, cn=None):
    """(w, m) of scan8_kernel from the restated quantiser: float32, the restatements' summation order."""
    u, sc = quantise_u8(rows)
    with np.errstate(invalid="ignore", over="ignore"):
        w = u8_score(u, sc, q)
        m = (u8_bound(sc, q) * F32(margin / 0.51)).astype(F32)
        if metric == L2:
            w = (F32(2.0) * w - cn).astype(F32)
            m = (F32(2.0) * m + F32(3e-5) * cn).astype(F32)
        elif phase2:
            q1 = F32(np.abs(q).sum(dtype=F32)) * F32(1.0 + 1e-5)
            m = (m + F32(1e-3) * sc * q1).astype(F32)
    return u, sc, w, m


def _keys_of_pass(w, m, sc, t, mask=None):
    """The full pass restated: keep = !(s < 0) && !(w + m < t) [&& mask bit]; key = (w or +inf when w is NaN, row)."""
    with np.errstate(invalid="ignore", over="ignore"):
        keep = ~(sc < 0) & ~((w + m).astype(F32) < F32(t))
    if mask is not None:
        keep &= S.mask_bits(mask, len(w))
    rows = np.flatnonzero(keep)
    score = np.where(np.isnan(w[rows]), F32(np.inf), w[rows] + F32(0.0)).astype(F32)
    return S.make_keys(S.f2ord(score), rows)


def _halfmax_of_pass(w, m, sc, num_tiles, tile_stride, shift=0, mask=None):
    """The sample pass restated: per group the maximum of w - m over its vouching rows (shift: a WRONG mapping, for the
    rejection test)."""
    n = len(w)
    out = np.zeros(num_tiles * 4, U64)
    allowed = np.ones(n, bool) if mask is None else S.mask_bits(mask, n)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = (w - m).astype(F32)
    for grp in range(num_tiles * 4):
        rows = S.sample_rows(grp, tile_stride, n) + shift
        rows = rows[rows < n]
        rows = rows[(sc[rows] >= 0) & ~np.isnan(lo[rows]) & allowed[rows]]
        if rows.size:
            out[grp] = S.make_keys(S.f2ord(F32(lo[rows].max() + F32(0.0))), [grp])[0]
    return out


# --------------------------------------------------------------------------- #
# CPU: the harness is the product's code
# --------------------------------------------------------------------------- #
def test_select_harness_is_built_from_the_product_headers_and_defines_no_kernel():
    src = S.SOURCE.read_text()
    for header in ("kernels_common.h", "kernels_merge_select.h", "kernels_scan8.h", "kernels_scan6.h", "kernels_tiles8.h", "kernels_aux.h"):
        assert f'#include "{header}"' in src, header
    assert "__global__" not in src
    csrc = S.ROOT / "wdbx-py_amd" / "csrc"
    mk = (csrc / "Makefile").read_text()
    assert "select_harness.hip" in mk and "libselect_harness.so" in mk and "$(SELECT_HARNESS)" in mk.split("clean:")[1]
    assert "$(SELECT_HARNESS)" in [ln for ln in mk.splitlines() if ln.startswith("all:")][0]
    # the pickers and the launch grids live next to the kernels now, and the library goes through the same ones
    host = (csrc / "host_index.h").read_text()
    scan8, scan6 = (csrc / "kernels_scan8.h").read_text(), (csrc / "kernels_scan6.h").read_text()
    for moved in ("struct Scan8Shape", "kScan8Shapes[]", "Scan8Shape* scan8_shape(uint32_t", "scan8_fn pick_scan8(", "scan8_fn pick_scan8_sample4("):
        assert moved in scan8 and moved not in host, moved
    for moved in ("int u6_unit_chunk(uint32_t", "scan6_fn pick_scan6("):
        assert moved in scan6 and moved not in host, moved
    for helper in ("scan8_shape", "pick_scan8<", "pick_scan8_sample4<", "u6_unit_chunk", "pick_scan6", "rows_to_u8_grid", "rows_to_u6_grid",
                   "row_sqnorm_grid", "rows_to_i8g_grid", "queries_to_i8_grid", "scan_sample_grid", "scan_full_grid"):
        call = helper if helper.endswith("<") else helper + "("
        assert call in src and call in host, helper
    assert host.count("rows_to_u8_grid(") == 2 and host.count("rows_to_u6_grid(") == 2 and host.count("row_sqnorm_grid(") == 2
    assert host.count("rows_to_i8g_grid(") == 2 and host.count("queries_to_i8_grid(") == 1
    assert "+ 3) / 4, 65536)), dim3(256)" not in host  # (no quantiser grid is spelt out in line any more)


def test_restated_tables_match_the_headers():
    scan8 = (S.ROOT / "wdbx-py_amd" / "csrc" / "kernels_scan8.h").read_text()
    table = scan8[scan8.index("kScan8Shapes[] = {"):]
    table = table[:table.index("};")]
    for pieces, L, qpl in S.SCAN8_SHAPES:
        assert "{%d, %d, %d}" % (pieces, L, qpl) in table
        assert pieces == L * qpl  # (a row is read as L lanes x QPL loads: nothing of it is skipped, nothing beyond it read)
    assert table.count("{") == len(S.SCAN8_SHAPES) + 1
    assert sorted({S.scan8_shape_py(d)[0] for d in U8_DIMS}) == [p for p, _, _ in S.SCAN8_SHAPES]  # U8_DIMS reaches every shape
    assert any(S.scan8_shape_py(d)[0] * 16 > d for d in U8_DIMS)  # ... and rows with padding bytes
    assert [S.u6_unit_chunk_py(u) for u in U6_UNITS] == [8, 5, 6, 7, 8, 8, 4]
    assert "constexpr uint32_t U6_CUT_SEG = KTH_R * 1024;" in (S.ROOT / "wdbx-py_amd" / "csrc" / "kernels_scan6.h").read_text()


def test_u6_layout_round_trips_and_places_rows():
    rng = _rng("u6 layout")
    for n, units in ((1, 4), (64, 6), (65, 7), (200, 25)):
        codes = rng.integers(1, 64, size=(n, units * 16)).astype(U8)
        dw = S.pack_u6(codes)
        assert dw.shape == ((n + 63) // 64, units, 64, 3)
        assert np.array_equal(S.unpack_u6(dw, n), codes)
        # row r, unit u sits at dword ((r >> 6) * units * 64 + u * 64 + (r & 63)) * 3: rows_to_u6_kernel's address
        flat = dw.reshape(-1)
        r, u = n - 1, units - 1
        at = ((r >> 6) * units * 64 + u * 64 + (r & 63)) * 3
        assert (int(flat[at]) & 0x3F) == codes[r, u * 16] and ((int(flat[at + 2]) >> 24) & 0x3F) == codes[r, u * 16 + 11]


# --------------------------------------------------------------------------- #
# CPU: the checkers accept the restatements on every family, and the inputs are vetted
# --------------------------------------------------------------------------- #
def _u8_case(d, metric, seed="cpu"):
    rng = _rng("u8 case", d, metric, seed)
    rows, names = _corpus(rng, 24, d)
    qs = _query_list(rng, d, rows, names)
    rows, names = _cut(rows, names, qs)
    return rng, rows, names, qs


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [100, 129, 384, 1000])
def test_checkers_accept_the_u8_restatement(d, metric):
    rng, rows, names, qs = _u8_case(d, metric)
    n, cls = len(rows), S.row_class(rows)
    with np.errstate(invalid="ignore", over="ignore"):
        cn = (rows * rows).sum(axis=1, dtype=F32) if metric == L2 else None
    for phase2 in (False, True):
        for qname, q in qs:
            truth = S.scores64(rows, q, metric)
            u, sc, w, m = _restated_u8(rows, q, metric, phase2, cn=cn)
            assert np.isfinite(w[cls == 0]).all(), (d, qname)  # the inputs keep every finite row's w finite
            m64 = S.u8_bound64(sc, q, metric, cn, phase2)
            S.check_w(_keys_of_pass(w, m, sc, -np.inf), n, truth, m64, cls)
            for t in S.thresholds_from(truth, cls, rng, extra=[truth[_ref_row(names)]]):
                keys = _keys_of_pass(w, m, sc, t)
                S.check_kept(keys, keys.size, n, n, truth, m64, cls, t)
            for stride in (1, 2):
                tiles = max(1, (n + 255) // 256 // stride)
                S.check_halfmax(_halfmax_of_pass(w, m, sc, tiles, stride), tiles, stride, n, truth, m64, cls)


def _restated_u6(rows, q, dimp):
    u, s, a = quantise_u6(rows)
    with np.errstate(invalid="ignore", over="ignore"):
        return u, s, a, u6_score(u, s, q), u6_bound(s, a, q, dimp)


@pytest.mark.parametrize("d", [96, 112, 400, 768])
def test_checkers_accept_the_u6_restatement(d):
    rng = _rng("u6 case", d)
    rows, names = _corpus(rng, 24, d, grid=31)
    qs = _query_list(rng, d, rows, names, grid=31)
    rows, names = _cut(rows, names, qs)
    n, cls = len(rows), S.row_class(rows)
    u, s, a = quantise_u6(rows)
    check_u6_quantiser(u, s.view(U32), a, rows, d, d, names)
    for qname, q in qs:
        truth = S.scores64(rows, q)
        u, s, a, w, m = _restated_u6(rows, q, d)
        assert np.isfinite(w[cls == 0]).all(), (d, qname)
        m64 = S.u6_bound64(s, a, q, d)
        S.check_w(_keys_of_pass(w, m, s, -np.inf), n, truth, m64, cls)
        for t in S.thresholds_from(truth, cls, rng, extra=[truth[_ref_row(names)]]):
            keys = _keys_of_pass(w, m, s, t)
            S.check_kept(keys, keys.size, n, n, truth, m64, cls, t)
        tiles = max(1, (n + 255) // 256)
        S.check_halfmax(_halfmax_of_pass(w, m, s, tiles, 1), tiles, 1, n, truth, m64, cls)


# --------------------------------------------------------------------------- #
# the quantisers' checkers (used on the restatements here and on the kernels' output below)
# --------------------------------------------------------------------------- #
def check_u8_quantiser(bytes_, scale_bits, rows, dim):
    """bytes [n, pitch8] and scale bit patterns against quantise_u8, bit for bit; the padding at the zero point."""
    u, sc = quantise_u8(rows[:, :dim])
    assert np.array_equal(bytes_[:, :dim], u), ("bytes", np.argwhere(bytes_[:, :dim] != u)[:4])
    assert (bytes_[:, dim:] == 128).all(), "a padding byte is not the zero point 128"
    cls = S.row_class(rows[:, :dim])
    fin = cls == 0
    assert np.array_equal(scale_bits[fin], sc.view(U32)[fin]), ("scale bits", np.flatnonzero(scale_bits[fin] != sc.view(U32)[fin])[:4])
    assert (scale_bits[cls == 1] == F32(-1.0).view(U32)).all(), "a NaN row's scale is not -1"
    assert np.isnan(scale_bits[cls == 2].view(F32)).all(), "an infinite row's scale is not NaN"
    assert (bytes_[~fin] == 128).all(), "a non-finite row's bytes are not 128"


def check_u6_quantiser(codes, s_bits, a, rows, dim, dimp, names=None):
    """codes [n, dimp] and s bit patterns against quantise_u6, bit for bit; codes in 1 .. 63, padding 32; the stored residual
    a: SAFE (a >= |c - s k|_2 in float64, every row) and TIGHT.

    Tight side: the kernel forms rho_i = fl(fl(x_i - s k_i) * inv) (two roundings; s * inv = 1 within 3 u), sums dimp squares
    with fmas in some order (relative gamma(dimp), halved by the root but taken whole), then one root, one fma with 1.0005f
    and 1e-4f (each within u of the decimal constant) and one product with s:  a <= (1.0005 |r|_2 + 1e-4 s)(1 + gamma(dimp + 16)).
    Underflowing residuals or squares only make a smaller.  Vanishing rows (max|c| < 1.2e-30) are named and excluded from the
    tight side only: there a = max|c| (sqrt(dim) + 1) is deliberately the whole row's norm, not its residual's."""
    n = len(rows)
    u_ref, s_ref, _ = quantise_u6(rows[:, :dim])
    assert codes.min() >= 1 and codes.max() <= 63
    assert np.array_equal(codes[:, :dim], u_ref), ("codes", np.argwhere(codes[:, :dim] != u_ref)[:4])
    assert (codes[:, dim:] == 32).all(), "a padding element's code is not the zero point 32"
    cls = S.row_class(rows[:, :dim])
    fin = cls == 0
    assert np.array_equal(s_bits[fin], s_ref.view(U32)[fin]), "s bits"
    assert (s_bits[cls == 1] == F32(-1.0).view(U32)).all() and (a[cls == 1] == 0).all(), "a NaN row is not {-1, 0}"
    assert np.isnan(s_bits[cls == 2].view(F32)).all() and (a[cls == 2] == 0).all(), "an infinite row is not {NaN, 0}"
    assert (codes[~fin] == 32).all()
    s64 = s_bits.view(F32).astype(F64)
    c = rows[fin][:, :dim].astype(F64)
    real = np.linalg.norm(c - s64[fin, None] * (codes[fin][:, :dim].astype(F64) - 32.0), axis=1)
    a64 = a.astype(F64)[fin]
    bad = np.flatnonzero(~(a64 >= real))
    assert bad.size == 0, ("SAFETY: a below the real residual norm", None if names is None else names[fin][bad][:4], a64[bad][:4], real[bad][:4])
    mx = np.abs(rows[fin][:, :dim]).max(axis=1)
    vanishing = mx < F32(1.2e-30)
    g = S.gamma(dimp + 16)
    loose = np.flatnonzero(~vanishing & ~(a64 <= (1.0005 * real + 1e-4 * s64[fin]) * (1 + g)))
    assert loose.size == 0, ("TIGHTNESS: a above its documented form", a64[loose][:4], real[loose][:4])
    # ... and not below it either, so the stored number IS the documented one: (1.0005 |r|_2 + 1e-4 s)(1 - gamma) - 1e-11 s (a
    # residual's fp32 value is off by at most 2^-150 absolute beyond its relative rounding: with s >= 1.2e-30 / 31 that is 2e-14 s
    # per element, 1.3e-12 s on the norm of 4096 of them)
    low = np.flatnonzero(~vanishing & ~(a64 >= (1.0005 * real + 1e-4 * s64[fin]) * (1 - g) - 1e-11 * s64[fin]))
    assert low.size == 0, ("a below its documented form", a64[low][:4], real[low][:4])
    van = np.flatnonzero(vanishing)
    assert (s64[fin][van] == 0).all(), "a vanishing row's scale is not 0"
    want = (mx[van].astype(F32) * (np.sqrt(F32(dim)) + F32(1.0))).astype(F32)
    assert np.all(np.abs(a[fin][van].astype(F64) - want.astype(F64)) <= 4 * S.U * want.astype(F64) + 2.0 ** -149), "a of a vanishing row"


def _i8_corpus(rng, d):
    """64 rows per family, so that every 64-row group of the tile path's shadow is one family (a group shares one scale), then a
    group of normal rows with the special rows inside it, cut off in the middle of its last 16-row quarter."""
    fams = _families(rng, 64, d)
    rows = np.concatenate([r for name, r in fams if name != "special"] + [rng.standard_normal((40, d)).astype(F32)])
    names = [name for name, _ in fams if name != "special"] + ["special"]
    sp = dict(fams)["special"]
    n = len(rows)
    rows[n - 40 + 3 * np.arange(len(sp))] = sp
    return rows, names


def check_i8_groups(bytes_rows, groups, gbad, rows, n_rows, dim, names):
    """The group table and bytes of rows_to_i8g_kernel.  bytes_rows: [g * 64, pitch8] int8 (ungathered); groups: [g, 4] float32
    {s_g, a_g, b_g, vouch}; gbad: [g] uint64; rows: [>= n_rows, >= dim] float32.

    Bit for bit against quantise_i8_groups: the bytes and s_g.  By property, against float64 norms of the kernel's OWN bytes and
    of the residuals delta = c / s_g - n they leave (what the bound's identity c = s_g (n + delta) uses):
      safe   a_g >= s_g max|n_r|_2,  b_g >= s_g max|delta_r|_2                                             (every group)
      tight  a_g <= s_g max|n_r|_2 * 1.0002 (1 + gamma),
             b_g <= s_g ((max|delta_r|_2 + 2e-5 sqrt(d)) * 1.0002 + 2e-5 sqrt(d)) (1 + gamma),  gamma = gamma(pitch8 + 8):
    a sum of pitch8 fma terms in any order (halved by the root, taken whole), the root, the constant and two products.  The
    kernel's residual c * inv - n differs from delta by the rounding of c * inv (half an ulp below 128: 3.8e-6) and by
    s_g * inv = 1 +- 2 u on a value of at most 127 (1.5e-5): under 2e-5 per element, 2e-5 sqrt(d) on the norm -- the allowance
    the kernel adds and the one the tight side grants once more.  Vanishing groups (max|c| < 1.2e-30: all bytes 0, the scale
    widened to 2 max, a flat residual of 1/2 per element) are named and left out of the tight side of b_g only."""
    g = len(groups)
    pitch8 = bytes_rows.shape[1]
    full = np.zeros((g * 64, dim), F32)
    full[:n_rows] = rows[:n_rows, :dim]
    n_ref, s_ref, _, _ = quantise_i8_groups(full)
    assert np.array_equal(bytes_rows[:, :dim], n_ref), ("bytes", np.argwhere(bytes_rows[:, :dim] != n_ref)[:4])
    assert (bytes_rows[:, dim:] == 0).all(), "a padding byte is not 0"
    cls = S.row_class(full)
    assert (bytes_rows[cls != 0] == 0).all() and (bytes_rows[n_rows:] == 0).all(), "a non-finite row or a row past the end is not a zero row"
    assert np.array_equal(groups[:, 0].view(U32), s_ref[::64].view(U32)), "s_g bits"
    gam = S.gamma(pitch8 + 8)
    for i in range(g):
        sl = slice(i * 64, i * 64 + 64)
        s_g, a_g, b_g = (float(v) for v in groups[i, :3])
        ok = cls[sl] == 0
        nb = bytes_rows[sl][ok].astype(F64)
        c = full[sl][ok].astype(F64)
        delta = (c / s_g - nb[:, :dim]) if s_g > 0 else np.zeros_like(c)
        nn = np.sqrt((nb * nb).sum(axis=1)).max(initial=0.0)
        dn = np.sqrt((delta * delta).sum(axis=1)).max(initial=0.0)
        has_inf = bool((cls[sl] == 2).any())
        want_bad = sum(1 << j for j in range(64) if cls[i * 64 + j] == 1 or i * 64 + j >= n_rows)
        assert int(gbad[i]) == want_bad, ("gbad", names[i], hex(int(gbad[i])), hex(want_bad))
        assert groups[i, 3] == (0.0 if has_inf else 1.0), ("vouch word", names[i])
        if has_inf:
            assert a_g == np.inf, ("a group with an infinite row must go to the exact pass", names[i])
        else:
            assert a_g >= s_g * nn * (1 - 1e-14), ("SAFETY a_g", names[i], a_g, s_g * nn)
            assert a_g <= s_g * nn * 1.0002 * (1 + gam), ("TIGHTNESS a_g", names[i], a_g, s_g * nn)
        assert b_g >= s_g * dn * (1 - 1e-14), ("SAFETY b_g", names[i], b_g, s_g * dn)
        vanishing = np.abs(c).max(initial=0.0) < F32(1.2e-30)
        if not vanishing:
            assert b_g <= s_g * ((dn + 2e-5 * np.sqrt(dim)) * 1.0002 + 2e-5 * np.sqrt(dim)) * (1 + gam), ("TIGHTNESS b_g", names[i], b_g, s_g * dn)


def check_i8_query(bytes_, qpar, q, dim, real):
    """One query of queries_to_i8_kernel: bytes [pitch8] int8, qpar [4] float32 {s_q, E, M, 1 / s_q}, q [>= dim] float32.
    Bytes, s_q and 1 / s_q bit for bit against quantise_i8_query; E and M by property against float64, with eps = q / s_q - m:
      safe   E >= s_q |eps|_2,  M >= s_q (|m|_2 + |eps|_2)
      tight  E <= s_q ((|eps|_2 + 2e-5 sqrt(d)) 1.0002 + 2e-5 sqrt(d) + 1e-6 |m|_2 1.0002) (1 + gamma),  M likewise
    (the allowances of check_i8_groups).  A vanishing query is left out of the tight side only.  A padded query (not real):
    all zero.  A query with a non-finite element: zeros, s_q = 0, E = +inf."""
    pitch8 = len(bytes_)
    s_q, E, M, inv = (float(v) for v in qpar)
    if not real:
        assert s_q == 0 and inv == 0 and E == 0 and M == 0 and (bytes_ == 0).all(), "a padded query is not all zero"
        return
    m_ref, s_ref, _, _ = quantise_i8_query(q[:dim])
    assert np.array_equal(bytes_[:dim], m_ref) and (bytes_[dim:] == 0).all(), "query bytes"
    assert qpar[:1].view(U32)[0] == np.array([s_ref], F32).view(U32)[0], "s_q bits"
    want_inv = F32(1.0) / F32(s_ref) if s_ref > 0 else F32(0)
    assert qpar[3:4].view(U32)[0] == np.array([want_inv], F32).view(U32)[0], "1 / s_q bits"
    if not np.isfinite(q[:dim]).all():
        assert s_q == 0 and E == np.inf, "a non-finite query must make every row a candidate"
        return
    mb, q64 = bytes_.astype(F64), q[:dim].astype(F64)
    eps = (q64 / s_q - mb[:dim]) if s_q > 0 else np.zeros(dim)
    en, mn = np.sqrt((eps * eps).sum()), np.sqrt((mb * mb).sum())
    assert E >= s_q * en * (1 - 1e-14) and M >= s_q * (mn + en) * (1 - 1e-14), ("SAFETY E / M", E, M, s_q * en, s_q * (mn + en))
    if np.abs(q64).max() >= F32(1.2e-30):
        gam, e_up = S.gamma(pitch8 + 8), (en + 2e-5 * np.sqrt(dim)) * 1.0002 + 2e-5 * np.sqrt(dim)
        assert E <= s_q * (e_up + 1e-6 * mn * 1.0002) * (1 + gam) and M <= s_q * (mn * 1.0002 + e_up) * (1 + gam), ("TIGHTNESS E / M", E, M)


def _i8_queries(rng, d):
    """The query families of test_i8_tile_bound_holds."""
    return [(n, np.asarray(q, F32)) for n, q in (
        ("normal", rng.standard_normal(d)), ("ones", np.ones(d)), ("one_hot", np.eye(d)[3]), ("heavy", rng.standard_t(1.5, size=d)),
        ("tiny", 1e-33 * rng.standard_normal(d)), ("midpoints", (rng.integers(-126, 127, size=d) + 0.5) / 127.0))]


def check_i8_tile_bound(bytes_rows, groups, rows, n_rows, dim, qbytes, qpar, q):
    """test_i8_tile_bound_holds on the quantisers' outputs: |c.q - s_g s_q D| <= a_g E + b_g M with the exact integer D, on
    every finite row (a group holding an infinite row has a_g = +inf: the bound is trivially true there).  Zero violations."""
    D = bytes_rows[:n_rows].astype(np.int64) @ qbytes.astype(np.int64)
    gi = np.arange(n_rows) // 64
    s_g, a_g, b_g = (groups[gi, j].astype(F64) for j in range(3))
    s_q, E, M = (float(v) for v in qpar[:3])
    exact = S.scores64(rows[:n_rows, :dim], q[:dim])
    fin = S.row_class(rows[:n_rows, :dim]) == 0
    with np.errstate(invalid="ignore"):
        slack = (a_g * E + b_g * M) - np.abs(s_g * s_q * D - exact)
    assert np.all(slack[fin] >= 0), ("i8 tile bound", np.flatnonzero(fin & ~(slack >= 0))[:6], float(np.nanmin(slack[fin])))


def _restated_i8_tables(rows, n_rows, d):
    """(bytes [g * 64, pitch8], groups [g, 4], gbad [g]) as the restatement gives them, in the kernel's output format."""
    g, pitch8 = (n_rows + 63) // 64, S.i8g_pitch(d)
    full = np.zeros((g * 64, d), F32)
    full[:n_rows] = rows[:n_rows]
    n, s_r, a_r, b_r = quantise_i8_groups(full)
    cls = S.row_class(full)
    groups = np.stack([s_r[::64], a_r[::64], b_r[::64], np.where(np.isinf(a_r[::64]), 0, 1).astype(F32)], axis=1).astype(F32)
    gbad = np.array([sum(1 << j for j in range(64) if cls[i * 64 + j] == 1 or i * 64 + j >= n_rows) for i in range(g)], U64)
    bytes_rows = np.zeros((g * 64, pitch8), np.int8)
    bytes_rows[:, :d] = n
    return bytes_rows, groups, gbad


@pytest.mark.parametrize("d", [40, 128, 384, 1000])
def test_checkers_accept_the_i8_restatements_and_reject_wrong_ones(d):
    rng = _rng("i8 cpu", d)
    rows, names = _i8_corpus(rng, d)
    n_rows, pitch8 = len(rows) - 5, S.i8g_pitch(d)
    bytes_rows, groups, gbad = _restated_i8_tables(rows, n_rows, d)
    check_i8_groups(bytes_rows, groups, gbad, rows, n_rows, d, names)
    # the layout restatement is a bijection of every 32-row block onto its 32 * pitch8 bytes
    r, c = np.meshgrid(np.arange(64), np.arange(pitch8), indexing="ij")
    off = S.g8_offset(r, c, pitch8)
    assert np.array_equal(np.sort(off.reshape(-1)), np.arange(64 * pitch8))
    assert np.array_equal(np.sort(off[:32].reshape(-1)), np.arange(32 * pitch8))
    flat = np.zeros(bytes_rows.size, np.int8)
    rr, cc = np.meshgrid(np.arange(len(bytes_rows)), np.arange(pitch8), indexing="ij")
    flat[S.g8_offset(rr, cc, pitch8)] = bytes_rows
    assert np.array_equal(S.ungather_i8g(flat, len(bytes_rows), pitch8), bytes_rows)
    for qname, q in _i8_queries(rng, d) + [("with_inf", np.where(np.arange(d) == 1, np.inf, 1.0).astype(F32))]:
        m, s_q, E, M = quantise_i8_query(q)
        qb = np.zeros(pitch8, np.int8)
        qb[:d] = m
        qpar = np.array([s_q, E, M, F32(1.0) / s_q if s_q > 0 else 0], F32)
        check_i8_query(qb, qpar, q, d, True)
        if np.isfinite(q).all():  # (a non-finite query has E = +inf: every row goes to the exact pass)
            check_i8_tile_bound(bytes_rows, groups, rows, n_rows, d, qb, qpar, q)
    check_i8_query(np.zeros(pitch8, np.int8), np.zeros(4, F32), q, d, False)
    # wrong: the table of the neighbouring group; the maximum taken over the non-finite rows too; a fragment half swapped
    with pytest.raises(AssertionError):
        check_i8_groups(bytes_rows, np.roll(groups, 1, axis=0), gbad, rows, n_rows, d, names)
    shifted = groups.copy()
    shifted[:, 2] = groups[:, 2] * F32(0.5)  # b_g halved: below the residuals it has to cover
    with pytest.raises(AssertionError, match="SAFETY b_g"):
        check_i8_groups(bytes_rows, shifted, gbad, rows, n_rows, d, names)
    swapped = flat.copy().reshape(-1, 2, 1024)[:, ::-1].reshape(-1)
    with pytest.raises(AssertionError, match="bytes"):
        check_i8_groups(S.ungather_i8g(swapped, len(bytes_rows), pitch8), groups, gbad, rows, n_rows, d, names)


# --------------------------------------------------------------------------- #
# CPU: the checkers reject wrong restatements
# --------------------------------------------------------------------------- #
def _staircase(rng, n, d):
    """Rows whose score against the returned query rises from one 64-row group to the next by far more than the error band:
    a lower bound taken from the wrong group is visibly not one."""
    q = rng.standard_normal(d).astype(F32)
    q /= np.linalg.norm(q)
    rows = (0.05 * rng.standard_normal((n, d)) + np.outer(1.0 + (np.arange(n) // 64), q)).astype(F32)
    return rows, q


def _wrong_u8(kind):
    """A deliberately wrong restatement of the u8 path -> the checker call that must raise."""
    d = 129
    rng, rows, names, qs = _u8_case(d, COS, "wrong")
    q = dict(qs)["residual_signs" if kind == "margin_0.49" else "ones"]
    n, cls = len(rows), S.row_class(rows)
    truth = S.scores64(rows, q)
    u, sc, w, m = _restated_u8(rows, q, margin=0.49 if kind == "margin_0.49" else 0.51)
    m64 = S.u8_bound64(sc, q)
    if kind == "margin_0.49":
        t = np.nextafter(F32(truth[_ref_row(names)]), F32(-np.inf))
        keys = _keys_of_pass(w, m, sc, t)
        return lambda: S.check_kept(keys, keys.size, n, n, truth, m64, cls, t)
    if kind == "truncation":
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            fin = cls == 0
            inv = np.where(fin, F32(1.0) / np.where(sc > 0, sc, 1).astype(F32), 0).astype(F32)
            ut = (np.clip(np.trunc(np.where(fin[:, None], rows, 0) * inv[:, None]), -127, 127) + 128).astype(U8)
        w = u8_score(ut, sc, q)
    elif kind == "missing_128_sum_q":
        w = (sc * (u.astype(F32) * q[None, :]).sum(axis=1, dtype=F32)).astype(F32)
    elif kind == "neighbour_scale":
        w = u8_score(u, np.roll(sc, -1), q)
    else:
        raise AssertionError(kind)
    return lambda: S.check_w(_keys_of_pass(w, m, sc, -np.inf), n, truth, m64, cls)


@pytest.mark.parametrize("kind", ["margin_0.49", "truncation", "missing_128_sum_q", "neighbour_scale"])
def test_checkers_reject_a_wrong_u8_restatement(kind):
    call = _wrong_u8(kind)
    with pytest.raises(AssertionError):
        call()


def test_checkers_reject_the_other_wrong_restatements():
    rng = _rng("wrong others")
    # zero point 127 in the padding
    d = 100
    rows = rng.standard_normal((40, d)).astype(F32)
    u, sc = quantise_u8(rows)
    check_u8_quantiser(S.pad_u8(u, 128), sc.view(U32), rows, d)
    with pytest.raises(AssertionError, match="padding"):
        check_u8_quantiser(S.pad_u8(u, 128, fill=127), sc.view(U32), rows, d)
    # a without its round-up, on the midpoints of the six-bit grid
    d = 96
    rows = dict(_families(rng, 200, d, grid=31))["grid_midpoints"]
    u, s, a = quantise_u6(rows)
    check_u6_quantiser(u, s.view(U32), a, rows, d, d)
    k = u.astype(F32) - F32(32)
    with np.errstate(invalid="ignore"):
        inv = (F32(31.0) / np.abs(rows).max(axis=1)).astype(F32)
        rho = ((rows.astype(F64) - s.astype(F64)[:, None] * k).astype(F32) * inv[:, None]).astype(F32)
        bare = (s * np.sqrt((rho * rho).sum(axis=1, dtype=F32), dtype=F32)).astype(F32)
    with pytest.raises(AssertionError, match="SAFETY"):
        check_u6_quantiser(u, s.view(U32), bare, rows, d, d)
    # a sampled group shifted by 64 rows
    n, d = 1024, 128
    rows, q = _staircase(rng, n, d)
    cls, truth = S.row_class(rows), S.scores64(rows, q)
    u, sc, w, m = _restated_u8(rows, q)
    m64 = S.u8_bound64(sc, q)
    S.check_halfmax(_halfmax_of_pass(w, m, sc, 4, 1), 4, 1, n, truth, m64, cls)
    with pytest.raises(AssertionError, match="NOT a lower bound"):
        S.check_halfmax(_halfmax_of_pass(w, m, sc, 4, 1, shift=64), 4, 1, n, truth, m64, cls)
    with pytest.raises(AssertionError, match="further than 2 m below"):  # ... and one group too low
        S.check_halfmax(_shift_down(_halfmax_of_pass(w, m, sc, 4, 1)), 4, 1, n, truth, m64, cls)


def _shift_down(halfmax):
    """Every group's key carries the score of the group before it (a mapping one group too low) under its own name."""
    out = halfmax.copy()
    out[1:] = (halfmax[:-1] & U64(0xFFFFFFFF00000000)) | (halfmax[1:] & U64(0xFFFFFFFF))
    return out


# --------------------------------------------------------------------------- #
# GPU: the tables, the quantisers
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
def test_library_pickers_match_the_restated_tables():
    for d in list(range(1, 70)) + U8_DIMS + [4095, 4097, 5000]:
        want = S.scan8_shape_py(d)
        got = S.scan8_shape(d)
        assert (got is None) == (want is None) and (got is None or got[:3] == want), d
        if got:
            assert got[3] == (got[2] <= 3)
    for units in range(1, 300):
        assert S.u6_unit_chunk(units) == S.u6_unit_chunk_py(units), units
    assert S.load().sel_u6_cut_seg() == S.U6_CUT_SEG


@pytest.mark.gpu
@pytest.mark.parametrize("d", U8_DIMS)
def test_rows_to_u8_kernel_matches_its_restatement_bit_for_bit(d):
    rng = _rng("u8 quant", d)
    rows, names = _corpus(rng, 16, d)
    pitch = (d + 3) // 4 * 4
    padded = S.pad_f32(rows, pitch)
    n = len(rows)
    assert n % 64 != 0
    pitch8 = S.scan8_shape_py(d)[0] * 16
    bytes_, scale = S.rows_to_u8(padded, d)
    assert bytes_.shape == (n, pitch8)
    check_u8_quantiser(bytes_, scale, padded, d)
    # the float64 bound check of test_u8_row_bound_holds on the KERNEL's bytes and scales
    fin = S.row_class(rows) == 0
    for qname, q in _query_list(rng, d, rows, names):
        ok = fin & _finite_scores_only(rows, [(qname, q)])
        w = u8_score(bytes_[ok][:, :d], scale.view(F32)[ok], q).astype(F64)
        slack = u8_bound(scale.view(F32)[ok], q).astype(F64) - np.abs(w - S.scores64(rows[ok], q))
        assert np.all(slack >= 0), (d, qname, names[ok][slack < 0][:4])
    # a refresh of rows [r0, n1) touches nothing else; one workgroup and more workgroups than rows give the same bytes
    for r0, n1, grid in ((5, n - 3, 0), (0, n, 1), (63, 65, 7), (0, n, n)):
        b2, s2 = S.rows_to_u8(padded, d, r0=r0, n=n1, grid=grid)
        assert np.array_equal(b2[r0:n1], bytes_[r0:n1]) and np.array_equal(s2[r0:n1], scale[r0:n1])
        assert (b2[:r0] == S.SENT_BYTE).all() and (b2[n1:] == S.SENT_BYTE).all()
        assert (s2[:r0] == S.SENT_F32).all() and (s2[n1:] == S.SENT_F32).all()


@pytest.mark.gpu
@pytest.mark.parametrize("units", U6_UNITS)
@pytest.mark.parametrize("pad", [0, 3])
def test_rows_to_u6_kernel_matches_its_restatement(units, pad):
    dimp = units * 16
    d = dimp - pad
    rng = _rng("u6 quant", units, pad)
    rows, names = _corpus(rng, 16, d, grid=31)
    padded = S.pad_f32(rows, dimp)
    n = len(rows)
    assert n % 64 != 0
    dw, sa = S.rows_to_u6(padded, d)
    assert dw.shape == ((n + 63) // 64, units, 64, 3)
    codes = S.unpack_u6(dw, n)
    check_u6_quantiser(codes, sa[:, 0].copy(), sa[:, 1].copy().view(F32), padded, d, dimp, names)
    # the float64 bound check of test_u6_row_bound_holds with the KERNEL's codes, s and a
    fin = S.row_class(rows) == 0
    s, a = sa[:, 0].copy().view(F32), sa[:, 1].copy().view(F32)
    for qname, q in _query_list(rng, d, rows, names, grid=31):
        ok = fin & _finite_scores_only(rows, [(qname, q)])
        w = u6_score(codes[ok][:, :d], s[ok], q).astype(F64)
        slack = u6_bound(s[ok], a[ok], q, dimp).astype(F64) - np.abs(w - S.scores64(rows[ok], q))
        assert np.all(slack >= 0), (units, qname, names[ok][slack < 0][:4])
    # rows outside [r0, n1) keep the sentinel, in the code dwords and in {s, a}; any grid gives the same
    for r0, n1, grid in ((5, n - 3, 0), (0, n, 1), (63, 66, 7)):
        dw2, sa2 = S.rows_to_u6(padded, d, r0=r0, n=n1, grid=grid)
        per_row = dw.transpose(0, 2, 1, 3).reshape(-1, units, 3)
        per_row2 = dw2.transpose(0, 2, 1, 3).reshape(-1, units, 3)
        assert np.array_equal(per_row2[r0:n1], per_row[r0:n1]) and np.array_equal(sa2[r0:n1], sa[r0:n1])
        assert (per_row2[:r0] == S.SENT_U32).all() and (per_row2[n1:] == S.SENT_U32).all()
        assert (sa2[:r0] == S.SENT_F32).all() and (sa2[n1:] == S.SENT_F32).all()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [100, 384, 1000, 4096])
def test_row_sqnorm_kernel(d):
    """|cn - |c|^2| <= gamma(pitch + 2) |c|^2 + pitch 2^-149: a sum of `pitch` non-negative fma terms in any order (each
    product is fused, so only the additions round); squares below the fp32 range lose at most half a denormal step each."""
    rng = _rng("sqnorm", d)
    rows, names = _corpus(rng, 16, d)
    pitch = (d + 3) // 4 * 4
    padded = S.pad_f32(rows, pitch)
    n = len(rows)
    cn_bits, st = S.row_sqnorm(padded, stats=[0, 0, 0])
    cn = cn_bits.view(F32)
    cls = S.row_class(rows)
    with np.errstate(over="ignore", invalid="ignore"):
        true = (padded.astype(F64) ** 2).sum(axis=1)
    fin = (cls == 0) & (true < 3.0e38)
    assert np.all(np.abs(cn[fin].astype(F64) - true[fin]) <= S.gamma(pitch + 2) * true[fin] + pitch * 2.0 ** -149)
    assert np.isnan(cn[cls == 1]).all() and np.isinf(cn[cls == 2]).all()
    assert np.isinf(cn[(cls == 0) & (true > 3.5e38)]).all()
    nonnan = cn_bits[~np.isnan(cn)]
    assert st[0] == nonnan.max()  # float bits of non-negative values order like unsigned integers
    assert st[2] == int((cn < np.inf).sum())
    ssum = cn[cn < np.inf].astype(F64).sum()
    assert abs(float(st[1:2].view(F32)[0]) - ssum) <= S.gamma(n + 8) * ssum
    # a refresh in place (cn_max_bits == nullptr): rows outside keep the sentinel.  With a null pointer there are no words to
    # look at: all that can be observed of "leaves the words alone" is that the norms are right and nothing faulted
    cn2, st2 = S.row_sqnorm(padded, r0=3, n=n - 2, grid=3, stats=None)
    assert np.array_equal(cn2[3:n - 2], cn_bits[3:n - 2]) and (cn2[:3] == S.SENT_F32).all() and (cn2[n - 2:] == S.SENT_F32).all()
    base = [0x3F800000, 0x40000000, 7]
    _, st3 = S.row_sqnorm(padded[:0].reshape(0, pitch) if False else padded, r0=n, n=n, stats=base)
    assert st3.tolist() == base  # words handed over and no rows: nothing is added to them


@pytest.mark.gpu
@pytest.mark.parametrize("d", [40, 100, 128, 129, 384, 1000, 1536])
def test_rows_to_i8g_kernel_matches_its_restatement(d):
    rng = _rng("i8g", d)
    rows, names = _i8_corpus(rng, d)
    n_alloc = len(rows)
    n_rows = n_alloc - 5  # the last rows of the allocation do not exist yet: zero rows, bad-row bits
    pitch, pitch8 = (d + 3) // 4 * 4, S.i8g_pitch(d)
    padded = S.pad_f32(rows, pitch)
    g = (n_rows + 63) // 64
    # the layout: the library's g8_offset against its numpy restatement, on every (row, column) of two blocks and a far one
    lib = S.load()
    for r in list(range(64)) + [1000, 12345]:
        assert all(lib.sel_g8_offset(r, c, pitch8) == int(S.g8_offset(r, c, pitch8)) for c in range(0, pitch8, 7))
    flat, groups, gbad = S.rows_to_i8g(padded, d, n_rows=n_rows)
    bytes_rows = S.ungather_i8g(flat, g * 64, pitch8)
    check_i8_groups(bytes_rows, groups.view(F32), gbad, padded, n_rows, d, names)
    # a refresh of groups [g0, g1) leaves the other groups' bytes and table entries alone; any grid gives the same
    for g0, g1, grid in ((1, g - 1, 0), (0, g, 1), (2, 3, 5)):
        f2, gr2, gb2 = S.rows_to_i8g(padded, d, n_rows=n_rows, g0=g0, g1=g1, grid=grid)
        lo, hi = g0 * 64 * pitch8, g1 * 64 * pitch8
        assert np.array_equal(f2[lo:hi], flat[lo:hi]) and np.array_equal(gr2[g0:g1], groups[g0:g1]) and np.array_equal(gb2[g0:g1], gbad[g0:g1])
        assert (f2[:lo].view(U8) == S.SENT_BYTE).all() and (gr2[:g0] == S.SENT_F32).all() and (gb2[:g0] == S.SENT_KEY).all()
    # the float64 bound check of test_i8_tile_bound_holds on BOTH kernels' outputs
    qs = _i8_queries(rng, d) + [("with_inf", np.where(np.arange(d) == 1, np.inf, 1.0).astype(F32)),
                                ("with_nan", np.where(np.arange(d) == d - 1, np.nan, 1.0).astype(F32))]
    nv, gbn = len(qs), len(qs) + 3
    qblock = np.stack([S.pad_f32(q[None, :], pitch)[0] for _, q in qs])
    out = S.queries_to_i8(qblock, d, gbn)
    assert (out["tau"] == 0x7F800000).all() and (out["count"] == 0).all() and out["lost"][0] == 0
    for i in range(gbn):
        check_i8_query(out["bytes"][i], out["qpar"][i].view(F32), qblock[min(i, nv - 1)], d, i < nv)
    for i, (qname, q) in enumerate(qs[:-2]):
        check_i8_tile_bound(bytes_rows, groups.view(F32), padded, n_rows, d, out["bytes"][i], out["qpar"][i].view(F32), qblock[i])
    for i in (nv - 2, nv - 1):
        assert out["qpar"][i].view(F32)[1] == np.inf and out["qpar"][i].view(F32)[0] == 0, qs[i][0]
    # a block without padding, more workgroups than queries: the same bits
    out2 = S.queries_to_i8(qblock, d, nv, grid=nv)
    assert np.array_equal(out2["bytes"], out["bytes"][:nv]) and np.array_equal(out2["qpar"], out["qpar"][:nv])


# --------------------------------------------------------------------------- #
# GPU: the u8 scans
# --------------------------------------------------------------------------- #
def _u8_chain(d, metric, seed, per=16):
    """A corpus, its queries, and the shadow the QUANTISER KERNEL makes of it (the product's chain)."""
    rng = _rng("u8 scan", d, metric, seed)
    rows, names = _corpus(rng, per, d)
    qs = _query_list(rng, d, rows, names)
    rows, names = _cut(rows, names, qs)
    pitch = (d + 3) // 4 * 4
    padded = S.pad_f32(rows, pitch)
    bytes_, scale_bits = S.rows_to_u8(padded, d)
    cn = S.row_sqnorm(padded)[0].view(F32) if metric == L2 else None
    return rng, rows, names, padded, qs, bytes_, scale_bits.view(F32), cn


def _queries_block(q, nq, pitch):
    out = np.zeros((nq, pitch), F32)
    out[:, :len(q)] = q
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("phase", [1, 2])
@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", U8_DIMS)
def test_scan8_full_pass_is_safe_and_tight(d, metric, phase):
    rng, rows, names, padded, qs, shadow, scale, cn = _u8_chain(d, metric, "full")
    n, pitch, cls = len(rows), padded.shape[1], S.row_class(rows)
    assert pitch // 4 <= S.scan8_shape_py(d)[0] * 4
    mask = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(U32)
    for qi, (qname, q) in enumerate(qs):
        truth = S.scores64(rows, q, metric)
        m64 = S.u8_bound64(scale, q, metric, cn, phase == 2)
        # tau = -inf: every row that is not NaN, each with the kernel's own w
        r = S.scan8(phase, metric, shadow, scale, _queries_block(q, 1, pitch), d, cn=cn, tau=[-np.inf], cap=n + 1)
        assert r["count"][0] == int((cls != 1).sum()) and (r["guard"] == S.SENT_KEY).all(), (d, qname)
        keys = r["cand"][0, :r["count"][0]]
        w = S.check_w(keys, n, truth, m64, cls)
        assert (S.key_ord(keys)[cls[S.key_row(keys).astype(np.int64)] == 2] == INF_ORD).all()  # infinite rows: +inf
        assert (r["cand"][0, r["count"][0]:] == S.SENT_KEY).all()
        # the thresholds sit on the rows' own scores; one launch, a query (the same) and a buffer per threshold
        ts = S.thresholds_from(truth, cls, rng, extra=[truth[_ref_row(names)]])
        use_mask = mask if qi % 3 == 1 else None
        r = S.scan8(phase, metric, shadow, scale, _queries_block(q, len(ts), pitch), d, cn=cn, mask=use_mask, tau=ts, cap=n + 1)
        assert (r["guard"] == S.SENT_KEY).all()
        for i, t in enumerate(ts):
            kept = S.check_kept(r["cand"][i], r["count"][i], n + 1, n, truth, m64, cls, t, use_mask)
            got = r["cand"][i, :r["count"][i]]
            assert (r["cand"][i, r["count"][i]:] == S.SENT_KEY).all()
            # the keys carry the same w as the tau = -inf pass, bit for bit
            assert np.array_equal(np.sort(got), np.sort(keys[kept[S.key_row(keys).astype(np.int64)]])), (d, qname, float(t))


@pytest.mark.gpu
@pytest.mark.parametrize("phase", [1, 2])
@pytest.mark.parametrize("d", [100, 384, 3000])
def test_scan8_buffers_counts_and_grids(d, phase):
    rng, rows, names, padded, qs, shadow, scale, cn = _u8_chain(d, L2, "buffers", per=24)
    n, pitch, cls = len(rows), padded.shape[1], S.row_class(rows)
    qname, q = qs[0]
    truth = S.scores64(rows, q, L2)
    t = F32(np.sort(truth[cls == 0])[n // 3])  # about two thirds of the rows qualify
    ref = S.scan8(phase, L2, shadow, scale, _queries_block(q, 1, pitch), d, cn=cn, tau=[t], cap=n)
    S.check_kept(ref["cand"][0], ref["count"][0], n, n, truth, S.u8_bound64(scale, q, L2, cn), cls, t)  # the reference run against float64
    total = int(ref["count"][0])
    want = np.sort(ref["cand"][0, :total])
    assert total > 129
    for cap in (1, 63, 64, 65, 128, 129):
        # three queries with three thresholds: everything, the reference's, nothing but the infinite rows
        r = S.scan8(phase, L2, shadow, scale, _queries_block(q, 3, pitch), d, cn=cn, tau=[-np.inf, t, np.inf], cap=cap)
        assert r["count"].tolist() == [int((cls != 1).sum()), total, int((cls == 2).sum())], cap
        assert (r["guard"] == S.SENT_KEY).all(), cap
        got = r["cand"][1]
        assert np.isin(got[:min(cap, total)], want).all() and np.unique(got).size == cap  # distinct kept keys, nothing else
        inf_keys = r["cand"][2, :min(cap, r["count"][2])]
        assert (S.key_ord(inf_keys) == INF_ORD).all() and (r["cand"][2, r["count"][2]:] == S.SENT_KEY).all()
    L = S.scan8_shape_py(d)[1]
    wave_passes = (n + 64 // L - 1) // (64 // L)
    for grid_x in (1, 3, (wave_passes + 3) // 4 + 5):
        r = S.scan8(phase, L2, shadow, scale, _queries_block(q, 1, pitch), d, cn=cn, tau=[t], cap=n, grid_x=grid_x)
        assert r["count"][0] == total and np.array_equal(np.sort(r["cand"][0, :total]), want), grid_x


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", U8_DIMS)
def test_scan8_sample_passes(d, metric):
    rng = _rng("u8 sample", d, metric)
    n = 1024 + 64 + 17  # the last sampled tile ends early, its last group does not exist
    stair, q0 = _staircase(rng, n, d)
    fam, _ = _corpus(rng, 8, d)
    rows = stair.copy()
    at = rng.choice(n, len(fam), replace=False)
    rows[at] = fam  # every family and the special rows, scattered over the groups
    rows[256:320] = np.nan  # a group that cannot vouch at all
    qs = [("staircase", q0)] + [(nm, np.asarray(v, F32)) for nm, v in _queries(rng, d)]
    ok = _finite_scores_only(rows, qs)
    rows[~ok] = 0.0
    pitch = (d + 3) // 4 * 4
    padded = S.pad_f32(rows, pitch)
    shadow, scale_bits = S.rows_to_u8(padded, d)
    scale = scale_bits.view(F32)
    cn = S.row_sqnorm(padded)[0].view(F32) if metric == L2 else None
    cls = S.row_class(rows)
    qblock = np.stack([_queries_block(q, 1, pitch)[0] for _, q in qs])
    mask = rng.integers(0, 1 << 32, (n + 31) // 32, dtype=np.uint64).astype(U32)
    mask[10] = 0  # rows 320 .. 351 masked out
    has4 = S.scan8_shape_py(d)[2] <= 3
    for num_tiles, stride, use_mask in ((5, 1, None), (2, 2, None), (1, 4, None), (5, 1, mask), (3, 1, None)):
        r = S.scan8(0, metric, shadow, scale, qblock, d, cn=cn, mask=use_mask, num_tiles=num_tiles, tile_stride=stride)
        assert (r["count"] == 0).all() and (r["guard"] == S.SENT_KEY).all()
        for i, (qname, q) in enumerate(qs):
            S.check_halfmax(r["halfmax"][i], num_tiles, stride, n, S.scores64(rows, q, metric), S.u8_bound64(scale, q, metric, cn), cls,
                            use_mask)
        for grid_x in (1, 3, num_tiles + 7):
            r2 = S.scan8(0, metric, shadow, scale, qblock, d, cn=cn, mask=use_mask, num_tiles=num_tiles, tile_stride=stride, grid_x=grid_x)
            assert np.array_equal(r2["halfmax"], r["halfmax"]), grid_x
        if not has4:
            continue
        # scan8_sample4_kernel: the same lower bounds bit for bit, for every number of queries around its 4 (3) per workgroup
        for nq in (1, 3, 4, 5, 7):
            for nt in (0, 1):
                a = S.scan8(0, metric, shadow, scale, qblock[:nq], d, cn=cn, mask=use_mask, num_tiles=num_tiles, tile_stride=stride,
                            sample_nt=nt)
                b = S.scan8(3, metric, shadow, scale, qblock[:nq], d, cn=cn, mask=use_mask, num_tiles=num_tiles, tile_stride=stride,
                            sample_nt=nt)
                assert np.array_equal(a["halfmax"], r["halfmax"][:nq]) and np.array_equal(b["halfmax"], a["halfmax"]), (nq, nt)
                assert (b["count"] == 0).all() and (b["guard"] == S.SENT_KEY).all(), (nq, nt)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [100, 384])
def test_sample4_lower_bounds_equal_phase0_bit_for_bit_on_cosine(d):
    """Regression: left to the compiler's contraction, `w - m` became fma(s, x, -m) in scan8_kernel<PHASE 0> and
    fma(-0.51 s, |q|_1, w) in scan8_sample4_kernel on the cosine metric; a quarter of the groups differed in the last place
    (26 of 100 at d = 100, 23 of 100 at d = 384 on this corpus).  Both kernels now share scan8_lower_bound."""
    rng = _rng("sample4 regression", d)
    n = 1105
    rows, _ = _staircase(rng, n, d)
    pitch = (d + 3) // 4 * 4
    padded = S.pad_f32(rows, pitch)
    shadow, sb = S.rows_to_u8(padded, d)
    qb = np.stack([_queries_block(rng.standard_normal(d).astype(F32), 1, pitch)[0] for _ in range(5)])
    a = S.scan8(0, COS, shadow, sb.view(F32), qb, d, num_tiles=5, tile_stride=1)["halfmax"]
    b = S.scan8(3, COS, shadow, sb.view(F32), qb, d, num_tiles=5, tile_stride=1)["halfmax"]
    assert np.array_equal(a, b), np.argwhere(a != b)[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [100, 768])
def test_scan8_in_kernel_threshold(d):
    """tau_keys / tau_n / tau_k: the kept set is that of tau = ord2f(block k-th of the keys' score halves); fewer than k keys:
    every row."""
    rng, rows, names, padded, qs, shadow, scale, cn = _u8_chain(d, COS, "tau keys", per=24)
    n, pitch, cls = len(rows), padded.shape[1], S.row_class(rows)
    q = qs[0][1]
    truth = S.scores64(rows, q)
    fin = np.sort(truth[cls == 0])
    for tau_n, k, absent in ((1024, 10, 0.0), (1000, 128, 0.3), (65, 64, 0.0), (64, 1, 0.5), (5, 10, 0.0), (300, 40, 0.9)):
        lows = rng.choice(fin, tau_n).astype(F32)
        keys = S.make_keys(S.f2ord(lows), np.arange(tau_n))
        keys[rng.random(tau_n) < absent] = 0
        ordv = _block_kth_threshold(S.key_ord(keys).astype(U64), k)
        t = F32(-np.inf) if ordv == 0 else S.ord2f(np.array([ordv], U32))[0]
        a = S.scan8(1, COS, shadow, scale, _queries_block(q, 1, pitch), d, tau_keys=keys, tau_k=k, cap=n)
        b = S.scan8(1, COS, shadow, scale, _queries_block(q, 1, pitch), d, tau=[t], cap=n)
        assert a["count"][0] == b["count"][0], (tau_n, k)
        assert np.array_equal(np.sort(a["cand"][0, :a["count"][0]]), np.sort(b["cand"][0, :b["count"][0]])), (tau_n, k)
        if ordv == 0:
            assert a["count"][0] == int((cls != 1).sum())


@pytest.mark.gpu
def test_scan8_on_a_hand_built_shadow():
    """Bytes, scales and norms chosen here, not by the quantiser: s (sum (u - 128) q) is exact in float64, so every byte
    position, the scale of the right row and the zero point are observable through w.  What is left of |w - truth| is the
    kernel's own fp32 arithmetic: the sum of P = pieces * 16 products u_i q_i in any order (gamma(P) sum |u_i q_i|), the sum
    behind 128 sum q (gamma(P) 128 |q|_1), their difference and the product with s (three roundings of at most
    sum |u_i q_i| + 128 |q|_1):  gamma(P + 8) s (sum |u_i q_i| + 128 |q|_1).

    The query buffer is shorter than the padded row here (qquads < pieces * 4: bytes beyond the buffer must not count), for the
    full pass, both sample kernels and both metrics.  Elsewhere in this file the same holds wherever dim is not a shape's upper
    edge (pitch = dim rounded to 4 < pieces * 16), which is what exercises the clamp of scan8_sample4_kernel in
    test_scan8_sample_passes."""
    rng = _rng("u8 hand")
    for d in (129, 1000):
        pieces = S.scan8_shape_py(d)[0]
        n, pitch = 333, (d + 3) // 4 * 4
        assert pitch // 4 < pieces * 4
        u = rng.integers(0, 256, size=(n, pieces * 16)).astype(U8)
        scale = (10.0 ** rng.uniform(-3, 3, n)).astype(F32)
        scale[7], scale[100], scale[101] = -1.0, np.nan, -0.5
        cn = (scale * scale * F32(100.0)).astype(F32)
        q = rng.standard_normal(d).astype(F32)
        qb = _queries_block(q, 1, pitch)
        cls = np.where(scale < 0, 1, np.where(np.isnan(scale), 2, 0))
        s64, q64 = np.where(cls == 0, scale, 0).astype(F64), q.astype(F64)
        dot = s64 * ((u[:, :d].astype(F64) - 128.0) @ q64)
        rounding = S.gamma(pieces * 16 + 8) * s64 * (u[:, :d].astype(F64) @ np.abs(q64) + 128.0 * np.abs(q64).sum())
        for metric in (COS, L2):
            truth = dot if metric == COS else 2.0 * dot - cn.astype(F64)
            tol = rounding if metric == COS else 2.0 * rounding + S.U * (np.abs(2.0 * dot) + cn.astype(F64))  # (+ the fma with -|c|^2)
            r = S.scan8(1, metric, u, scale, qb, d, cn=cn, tau=[-np.inf], cap=n)
            S.check_w(r["cand"][0, :r["count"][0]], n, truth, tol / (1 + S.M_SLACK), cls)
            # the sample passes see the same bytes: each group's lower bound against the hand-made truth and the documented m
            m64 = S.u8_bound64(np.where(cls == 0, scale, 0), q, metric, cn) + tol
            for ph in (0, 3):
                hm = S.scan8(ph, metric, u, scale, qb, d, cn=cn, num_tiles=2, tile_stride=1)["halfmax"][0]
                S.check_halfmax(hm, 2, 1, n, truth, m64, cls)


@pytest.mark.gpu
def test_rescore_gives_identical_bits_from_the_u8_and_the_u6_list():
    """kernels_scan6.h: "the same kernel as behind the u8 scan: bit-identical scores".  One corpus, one query, the candidate
    lists of the u8 and of the u6 full pass re-scored: every row that is in both carries the same key."""
    rng = _rng("rescore both")
    n, d = 3000, 384
    rows = rng.standard_normal((n, d)).astype(F32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    q = rng.standard_normal(d).astype(F32)
    qb = q[None, :].copy()
    tau = [F32(np.sort(S.scores64(rows, q))[-400])]
    shadow, sb = S.rows_to_u8(rows, d)
    dw, sa = S.rows_to_u6(rows, d)
    r8 = S.scan8(1, COS, shadow, sb.view(F32), qb, d, tau=tau, cap=n)
    r6 = S.scan6(False, dw, sa.view(F32), qb, n, tau=tau, cap=n)
    k8, _ = S.rescore(COS, rows, qb, r8["cand"], r8["count"])
    k6, _ = S.rescore(COS, rows, qb, r6["cand"], r6["count"])
    k8, k6 = k8[0, :r8["count"][0]], k6[0, :r6["count"][0]]
    both = np.intersect1d(S.key_row(k8), S.key_row(k6))
    assert both.size >= 400
    by8 = dict(zip(S.key_row(k8).tolist(), k8.tolist()))
    by6 = dict(zip(S.key_row(k6).tolist(), k6.tolist()))
    assert all(by8[r] == by6[r] for r in both.tolist())


# --------------------------------------------------------------------------- #
# GPU: the u6 scans
# --------------------------------------------------------------------------- #
def _u6_chain(units, pad, seed, per=16):
    dimp = units * 16
    d = dimp - pad
    rng = _rng("u6 scan", units, pad, seed)
    rows, names = _corpus(rng, per, d, grid=31)
    qs = _query_list(rng, d, rows, names, grid=31)
    rows, names = _cut(rows, names, qs)
    padded = S.pad_f32(rows, dimp)
    dw, sa = S.rows_to_u6(padded, d)
    return rng, rows, names, padded, qs, dw, sa.view(F32), d, dimp


@pytest.mark.gpu
@pytest.mark.parametrize("units,pad", [(24, 0), (25, 3), (6, 0), (7, 5), (48, 1), (256, 0), (4, 2)])
def test_scan6_full_pass_is_safe_and_tight(units, pad):
    rng, rows, names, padded, qs, dw, sa, d, dimp = _u6_chain(units, pad, "full")
    n, cls = len(rows), S.row_class(rows)
    for qname, q in qs:
        truth = S.scores64(rows, q)
        m64 = S.u6_bound64(sa[:, 0], sa[:, 1], q, dimp)
        r = S.scan6(False, dw, sa, _queries_block(q, 1, dimp), n, tau=[-np.inf], cap=n + 1)
        assert r["count"][0] == int((cls != 1).sum()) and (r["guard"] == S.SENT_KEY).all(), (units, qname)
        assert r["count2"][0] == S.SENT_U32  # the full pass leaves the cut's counter alone
        keys = r["cand"][0, :r["count"][0]]
        S.check_w(keys, n, truth, m64, cls)
        assert (S.key_ord(keys)[cls[S.key_row(keys).astype(np.int64)] == 2] == INF_ORD).all()
        ts = S.thresholds_from(truth, cls, rng, extra=[truth[_ref_row(names)]])
        r = S.scan6(False, dw, sa, _queries_block(q, len(ts), dimp), n, tau=ts, cap=n + 1)
        assert (r["guard"] == S.SENT_KEY).all()
        for i, t in enumerate(ts):
            kept = S.check_kept(r["cand"][i], r["count"][i], n + 1, n, truth, m64, cls, t)
            got = r["cand"][i, :r["count"][i]]
            assert np.array_equal(np.sort(got), np.sort(keys[kept[S.key_row(keys).astype(np.int64)]])), (units, qname, float(t))


@pytest.mark.gpu
@pytest.mark.parametrize("units", [24, 25, 7])
def test_scan6_buffers_counts_and_grids(units):
    rng, rows, names, padded, qs, dw, sa, d, dimp = _u6_chain(units, 0, "buffers", per=24)
    n, cls = len(rows), S.row_class(rows)
    q = qs[0][1]
    truth = S.scores64(rows, q)
    t = F32(np.sort(truth[cls == 0])[n // 3])
    ref = S.scan6(False, dw, sa, _queries_block(q, 1, dimp), n, tau=[t], cap=n)
    S.check_kept(ref["cand"][0], ref["count"][0], n, n, truth, S.u6_bound64(sa[:, 0], sa[:, 1], q, dimp), cls, t)  # against float64
    total = int(ref["count"][0])
    want = np.sort(ref["cand"][0, :total])
    assert total > 129
    for cap in (1, 63, 64, 65, 128, 129):
        r = S.scan6(False, dw, sa, _queries_block(q, 3, dimp), n, tau=[-np.inf, t, np.inf], cap=cap)
        assert r["count"].tolist() == [int((cls != 1).sum()), total, int((cls == 2).sum())], cap
        assert (r["guard"] == S.SENT_KEY).all(), cap
        got = r["cand"][1]
        assert np.isin(got[:min(cap, total)], want).all() and np.unique(got).size == cap
        assert (r["cand"][2, r["count"][2]:] == S.SENT_KEY).all()
    for grid_x in (1, 3, (n + 63) // 64 + 5):
        r = S.scan6(False, dw, sa, _queries_block(q, 1, dimp), n, tau=[t], cap=n, grid_x=grid_x)
        assert r["count"][0] == total and np.array_equal(np.sort(r["cand"][0, :total]), want), grid_x


@pytest.mark.gpu
@pytest.mark.parametrize("units", [24, 25, 6, 7, 4])
def test_scan6_sample_pass(units):
    dimp = units * 16
    d = dimp
    rng = _rng("u6 sample", units)
    n = 1024 + 64 + 17
    stair, q0 = _staircase(rng, n, d)
    fam, _ = _corpus(rng, 8, d, grid=31)
    rows = stair.copy()
    at = rng.choice(n, len(fam), replace=False)
    rows[at] = fam
    rows[256:320] = np.nan
    qs = [("staircase", q0)] + [(nm, np.asarray(v, F32)) for nm, v in _queries(rng, d)]
    ok = _finite_scores_only(rows, qs)
    rows[~ok] = 0.0
    dw, sa = S.rows_to_u6(rows, d)
    sa = sa.view(F32)
    cls = S.row_class(rows)
    qblock = np.stack([q for _, q in qs]).astype(F32)
    for num_tiles, stride in ((5, 1), (2, 2), (1, 4), (3, 1)):
        for nq in (7, 1, 4, 5):
            r = S.scan6(True, dw, sa, qblock[:nq], n, num_tiles=num_tiles, tile_stride=stride)
            assert (r["count"] == 0).all() and (r["count2"] == 0).all() and (r["guard"] == S.SENT_KEY).all()
            for i, (qname, q) in enumerate(qs[:nq]):
                S.check_halfmax(r["halfmax"][i], num_tiles, stride, n, S.scores64(rows, q), S.u6_bound64(sa[:, 0], sa[:, 1], q, dimp), cls)
            if nq == 7:
                full = r["halfmax"]
            else:
                assert np.array_equal(r["halfmax"], full[:nq])
        r2 = S.scan6(True, dw, sa, qblock, n, num_tiles=num_tiles, tile_stride=stride, grid_x=1)
        assert np.array_equal(r2["halfmax"], full)


@pytest.mark.gpu
@pytest.mark.parametrize("units", [24, 256])
def test_u6_scan_on_exactly_representable_rows(units):
    """Rows that ARE s * k: the residual is zero, a = 1e-4 s, and what is left of |w - c.q| are the scan's own fp32 roundings
    -- the term 6e-6 (dimp + 8) s |q|_1 is what has to cover them (the bound without it is a |q|_2 = 1e-4 s |q|_2)."""
    dimp = units * 16
    rng = _rng("u6 exact", units)
    n = 300
    k = rng.integers(-31, 32, size=(n, dimp))
    k[:, 0] = 31
    s = (2.0 ** rng.integers(-8, 8, n)).astype(F32)
    rows = (s[:, None].astype(F64) * k / 31.0 * 31.0).astype(F32)  # max|c| = 31 s, s = max / 31 exactly (powers of two)
    dw, sa = S.rows_to_u6(rows, dimp)
    sa = sa.view(F32)
    assert np.array_equal(S.unpack_u6(dw, n).astype(np.int64) - 32, k) and np.array_equal(sa[:, 0], s)
    assert np.all(sa[:, 1] <= s * F32(1.0001e-4))
    # (the biased query makes the partial sums large, sum u q ~ 32 dimp, so their roundings are far above a |q|_2)
    for q in (rng.standard_normal(dimp).astype(F32), np.ones(dimp, F32), (1e3 * rng.standard_t(1.5, dimp)).astype(F32),
              (1.0 + 0.01 * rng.standard_normal(dimp)).astype(F32)):
        truth = S.scores64(rows, q)
        m64 = S.u6_bound64(sa[:, 0], sa[:, 1], q, dimp)
        cls = np.zeros(n, np.int64)
        r = S.scan6(False, dw, sa, _queries_block(q, 1, dimp), n, tau=[-np.inf], cap=n)
        S.check_w(r["cand"][0, :n], n, truth, m64, cls)
        # every row's own score as a threshold (the largest fp32 not above it): the row itself must be kept
        ts = truth.astype(F32)
        ts = np.where(ts.astype(F64) > truth, np.nextafter(ts, F32(-np.inf)), ts)
        r = S.scan6(False, dw, sa, _queries_block(q, n, dimp), n, tau=ts, cap=n)
        for i, t in enumerate(ts):
            S.check_kept(r["cand"][i], r["count"][i], n, n, truth, m64, cls, t)


# --------------------------------------------------------------------------- #
# GPU: re-scoring and the cut
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [100, 384, 1000, 4096])
def test_rescore_kernel(d, metric):
    """score within gamma(pitch / 64 + 10) sum |c_i q_i| (cosine) or sum (c_i - q_i)^2 (L2) of float64: lane j adds every
    64th quad in four fma chains of pitch / 256 terms, then 2 + 6 additions fold the lanes (L2: one more rounding in each
    difference, taken twice by the square)."""
    rng = _rng("rescore", d, metric)
    rows, names = _corpus(rng, 16, d)
    qs = _query_list(rng, d, rows, names)[:3]
    ok = _finite_scores_only(rows, qs, big=1e18)
    rows = rows[ok | (S.row_class(rows) != 0)]
    assert len(rows) >= 150
    pitch = (d + 3) // 4 * 4
    padded = S.pad_f32(rows, pitch)
    n, cls = len(rows), S.row_class(rows)
    nq, cap = len(qs), n + 5
    qblock = np.stack([_queries_block(q, 1, pitch)[0] for _, q in qs])
    order = np.stack([np.concatenate([p, p[:5]]) for p in (rng.permutation(n) for _ in range(nq))])  # [nq, cap] valid rows
    junk = S.f2ord(rng.standard_normal(cap).astype(F32))  # the selection's scores: the kernel must not care
    cand = np.stack([S.make_keys(junk, order[i]) for i in range(nq)])
    count = np.array([n, n - 7, n + 1000], U32)[:nq]  # the last one overflowed: the kernel takes the cap slots there are
    out, guard = S.rescore(metric, padded, qblock, cand, count)
    assert (guard == S.SENT_KEY).all()
    g = S.gamma(pitch // 256 + 1 + 10)
    for i, (qname, q) in enumerate(qs):
        have = min(int(count[i]), cap)
        assert np.array_equal(out[i, have:], cand[i, have:]), "a slot at or beyond min(count, cap) was touched"
        c64, q64 = rows[order[i][:have]].astype(F64), q.astype(F64)
        with np.errstate(invalid="ignore", over="ignore"):
            if metric == COS:
                exact, scale = c64 @ q64, np.abs(c64) @ np.abs(q64)
            else:
                exact = -((c64 - q64) ** 2).sum(axis=1)
                scale = -exact * (1 + 4 * S.U)
        key = out[i, :have]
        nan = np.isnan(exact)
        assert (key[nan] == 0).all(), "a NaN score did not become key 0"
        assert np.array_equal(S.key_row(key[~nan]).astype(np.int64), order[i][:have][~nan]), "a key changed its row"
        got = S.ord2f(S.key_ord(key[~nan])).astype(F64)
        f = np.isfinite(exact[~nan]) & (np.abs(scale[~nan]) < 1e37)
        assert np.all(np.abs(got[f] - exact[~nan][f]) <= g * scale[~nan][f] + pitch * 2.0 ** -149), (d, qname)
        assert np.array_equal(got[~f & np.isinf(exact[~nan])], exact[~nan][~f & np.isinf(exact[~nan])])
    # the same candidates in another order and from another grid: identical bits per row
    out2, _ = S.rescore(metric, padded, qblock[:1], cand[:1, ::-1][:, cap - n:].copy(), [n], grid_x=3)
    a = out[0, :n][np.argsort(order[0][:n], kind="stable")]
    b = out2[0, :n][np.argsort(order[0][:n][::-1], kind="stable")]
    assert np.array_equal(a, b)


@pytest.mark.gpu
def test_u6_cut_kernel():
    rng = _rng("cut")
    seg, cap2 = S.U6_CUT_SEG, 4096
    cap = 3 * seg + 100
    cases = [100, seg - 1, seg, seg + 1, 2 * seg + 5, 3 * seg, cap, cap + 1]
    for k in (1, 10, 32):
        nq = len(cases)
        cand = np.zeros((nq, cap), U64)
        for i, c in enumerate(cases):
            m = min(c, cap)
            x = rng.standard_normal(m).astype(F32)
            x[rng.random(m) < 0.01] = np.nan  # re-scored NaN rows are key 0
            keys = S.make_keys(S.f2ord(np.nan_to_num(x)), rng.permutation(1 << 20)[:m])
            keys[np.isnan(x)] = 0
            cand[i, :m] = keys
        count = np.array(cases, U32)
        out, guard, count2 = S.u6_cut(cand, count, k, cap2)
        assert (guard == S.SENT_KEY).all()
        for i, c in enumerate(cases):
            if c > cap:
                assert count2[i] > cap2  # the buffer in front overflowed: "repair this query"
                continue
            assert count2[i] <= cap2, (k, c, int(count2[i]))
            short = out[i, :count2[i]]
            assert (out[i, count2[i]:] == S.SENT_KEY).all()
            best = np.sort(cand[i, :c])[::-1][:k]
            best = best[best != 0]
            assert np.isin(best, short).all(), (k, c)
            assert np.isin(short, cand[i, :c]).all() and np.unique(short).size == short.size
            assert count2[i] <= ((c + seg - 1) // seg) * max(4 * k, k + 64), (k, c, int(count2[i]))  # it cuts
    # thousands of ties at the k-th score: the short list overflows, says so, and writes nothing beyond cap2
    ties = S.make_keys(np.full(2 * seg, S.f2ord(F32(0.25))[0], U32), np.arange(2 * seg))
    out, guard, count2 = S.u6_cut(ties[None, :], [2 * seg], 10, cap2)
    assert count2[0] > cap2 and (guard == S.SENT_KEY).all() and np.isin(out[0], ties).all()


# --------------------------------------------------------------------------- #
# GPU: the chain
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["u8", "u6"])
def test_the_selection_chain_on_a_corpus_inside_the_error_band(path):
    """quantiser -> sample -> kth_score_kernel -> full pass -> rescore -> (u6: cut) -> merge_kernel, on a corpus whose best
    rows are a cluster far tighter than one quantisation step: dozens of rows sit inside the band around the k-th score.
    The float64 top-k is among the candidates ALWAYS; the final ids are the float64 ranking wherever the float64 gap to the
    neighbours exceeds the fp32 re-scoring error."""
    import rank_harness as R
    rng = _rng("chain", path)
    n, d, k = 64 * 64 + 33, 384, 10
    q = rng.standard_normal(d).astype(F32)
    q /= np.linalg.norm(q)
    rows = rng.standard_normal((n, d)).astype(F32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    cluster = rng.choice(n, 80, replace=False)
    rows[cluster] = (q + 2e-4 * rng.standard_normal((80, d))).astype(F32)  # scores 1 +- 1e-5: one u8 step is 1e-3 |q|_1
    rows[rng.choice(np.setdiff1d(np.arange(n), cluster), 3, replace=False), 5] = np.nan
    truth = S.scores64(rows, q)
    cls = S.row_class(rows)
    order = np.argsort(-np.where(cls == 0, truth, -np.inf), kind="stable")
    top = order[:k]
    qb = q[None, :].copy()
    tiles = (n + 255) // 256
    num_tiles, stride = tiles // 2, 2
    if path == "u8":
        shadow, sbits = S.rows_to_u8(rows, d)
        scale = sbits.view(F32)
        m64 = S.u8_bound64(scale, q)
        hm = S.scan8(0, COS, shadow, scale, qb, d, num_tiles=num_tiles, tile_stride=stride)["halfmax"]
    else:
        dw, sa = S.rows_to_u6(rows, d)
        sa = sa.view(F32)
        m64 = S.u6_bound64(sa[:, 0], sa[:, 1], q, d)
        hm = S.scan6(True, dw, sa, qb, n, num_tiles=num_tiles, tile_stride=stride)["halfmax"]
    S.check_halfmax(hm[0], num_tiles, stride, n, truth, m64, cls)
    tau = R.kth(hm[0], hm.shape[1], hm.shape[1], 1, k).view(F32)
    assert tau[0] <= np.sort(truth[cls == 0])[-k]  # a lower bound of the true k-th best score
    cap = 4096
    if path == "u8":
        r = S.scan8(1, COS, shadow, scale, qb, d, tau=tau, cap=cap)
    else:
        r = S.scan6(False, dw, sa, qb, n, tau=tau, cap=cap)
    S.check_kept(r["cand"][0], r["count"][0], cap, n, truth, m64, cls, tau[0])
    cnt = int(r["count"][0])
    assert k <= cnt < n // 4 and set(top.tolist()) <= set(S.key_row(r["cand"][0, :cnt]).tolist())
    assert int((np.abs(truth[cluster] - np.sort(truth[cls == 0])[-k]) < m64[cluster]).sum()) >= 24  # dozens inside the band
    keys, _ = S.rescore(COS, rows, qb, r["cand"], r["count"])
    if path == "u6":
        short, _, count2 = S.u6_cut(keys, r["count"], k, 4096)
        assert count2[0] <= 4096
        keys, cnt = short, int(count2[0])
    out = R.merge(keys[0], 1, k, P=keys.shape[1], list_len=1, q_stride=keys.shape[1], i_stride=0, p_stride=1,
                  P_dev=np.array([cnt], U32))
    ids = out["idx"][0]
    # fp32 re-scoring error of unit vectors: gamma(d / 64 + 10) * sum |c_i q_i| <= gamma(16) * 1
    eps = S.gamma(d // 256 + 11) * 1.0
    assert set(ids.tolist()) <= set(order[:k + 40].tolist())
    t_sorted = truth[order]
    for pos in range(k):
        gap_up = t_sorted[pos - 1] - t_sorted[pos] if pos else np.inf
        gap_dn = t_sorted[pos] - t_sorted[pos + 1]
        if gap_up > 2 * eps and gap_dn > 2 * eps:
            assert ids[pos] == order[pos], (path, pos)
    assert np.all(np.abs(out["score"][0].view(F32).astype(F64) - truth[ids]) <= eps)
