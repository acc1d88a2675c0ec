"""One row mask PER QUERY in one batched call (wdbx_index_search_multimask): the int8 tile pass with the mask word read per
column group of 16 queries, and the per-mask fall-back behind the same entry point.

What every case compares (``_run``), in the style of tests/test_gpu_batch_masked.py (helpers copied from there):
  * the call ran the tile pass with a mask per query: ``last_batch_masked == 2``, ``last_gemm_family == 3`` (int8 tiles),
    ``last_batch_mask_classes`` = the distinct entries of ``query_mask`` and ``last_batch_blocks`` = the planned blocks,
    ceil(sum over classes of 16 ceil(n_c / 16) / 256) (128-slot blocks for L2);
  * no returned row lies outside ITS query's mask;
  * ids against numpy's exact search restricted to that query's allowed rows.  Per query the test re-derives in float64 that
    the gap at rank k among the allowed rows exceeds 1e-5 (else the query is skipped: at most 1 in 10, printed; on these iid
    corpora the gap is ~1e-3; tests/test_multimask_oracle.py confirms on the CPU that the oracle alone skips none);
  * scores within 1e-5 of the oracle;
  * ids and scores bit-identical to the same query sent ALONE with its mask (``search`` without a mask for a -1 query);
  * no query overflowed, except in the case that says otherwise.

Corpora come from ``fill_synthetic`` and are read back; ``gemm_min_rows = 16384`` lets 70 003 rows reach the tiles,
``single_min_rows = 0`` lets the one-at-a-time calls take the selection scan below 131 072 rows."""
import ctypes as C

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

ATOL = 1e-5
GAP = 1e-5
N_SMALL, D_SMALL = 70_003, 64
N_LARGE, D_LARGE = 262_147, 384
E_INVALID, WDBX_MAX_K = -1, 2048


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


def _open(native, n, d, metric=None, seed=O.SEED_CORPUS):
    ix = native.NativeIndex(d, metric=native.METRIC_COSINE if metric is None else metric, capacity_rows=n)
    ix.fill_synthetic(seed, 0, n, normalize=True)
    ix.set_option("gemm_min_rows", 16384)
    ix.set_option("single_min_rows", 0)
    return ix


_SHARED = {}


def _corpus(native, n, d, metric=None):
    """One index and its rows (read back from the device) per shape, shared by the tests that do not write rows."""
    key = (n, d, metric)
    if key not in _SHARED:
        ix = _open(native, n, d, metric)
        _SHARED[key] = (ix, ix.get_rows(0, n))
    return _SHARED[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shared():
    yield
    for ix, _ in _SHARED.values():
        ix.close()
    _SHARED.clear()


def _queries(nq, d, offset=0):
    return O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, offset, nq, d))


def _oracle(rows, queries, k, allowed, l2=False):
    """Exact search restricted to ``allowed``: per query (ids, float64 scores, gap at rank k, smallest gap inside the list).
    fp32 scores pick k + 16 candidates (they rank within ~1e-6 of the truth: the true k + 1 best are among them), float64 on
    those candidates decides.  Scores as the library reports them: inner product, or squared distance for L2."""
    rows_a = np.nonzero(allowed)[0]
    sub = rows[rows_a]
    out = []
    if not len(rows_a) or not len(queries):
        return [(np.empty(0, np.int64), np.empty(0), np.inf, np.inf) for _ in queries]
    s32 = queries @ sub.T
    if l2:
        s32 = 2.0 * s32 - np.einsum("ij,ij->i", sub, sub)[None, :]
    s32[:, np.isnan(s32).any(axis=0)] = -np.inf  # (removed rows: never a result)
    take = min(k + 16, len(rows_a))
    for qi, q in enumerate(queries):
        cand = np.argpartition(-s32[qi], take - 1)[:take] if take < len(rows_a) else np.arange(len(rows_a))
        cand = cand[np.isfinite(s32[qi][cand])]
        c64, q64 = sub[cand].astype(np.float64), q.astype(np.float64)
        s64 = -((c64 - q64) ** 2).sum(axis=1) if l2 else c64 @ q64
        order = np.lexsort((rows_a[cand], -s64))
        ids, sc = rows_a[cand][order], s64[order]
        kk = min(k, len(ids))
        gap = sc[kk - 1] - sc[kk] if len(ids) > kk else np.inf
        inner = np.min(sc[:kk - 1] - sc[1:kk]) if kk > 1 else np.inf
        out.append((ids[:kk].astype(np.int64), -sc[:kk] if l2 else sc[:kk], gap, inner))
    return out


def _compare(idx, score, expected, k, what, ids_only=False):
    skipped = 0
    for qi, (e_idx, e_score, gap, inner) in enumerate(expected):
        kk = len(e_idx)
        assert np.all(idx[qi][kk:] == -1), (what, qi, "unused slots must hold -1")
        if gap <= GAP:
            skipped += 1
            continue
        if inner > 1e-6:
            assert idx[qi][:kk].tolist() == e_idx.tolist(), (what, qi, gap)
        else:
            assert sorted(idx[qi][:kk].tolist()) == sorted(e_idx.tolist()), (what, qi, gap)
            e_score = np.sort(e_score)
            if not ids_only:
                np.testing.assert_allclose(np.sort(score[qi][:kk]), e_score, atol=ATOL, rtol=0)
            continue
        if not ids_only:
            np.testing.assert_allclose(score[qi][:kk], e_score, atol=ATOL, rtol=0)
    print(f"{what}: {skipped} of {len(expected)} queries skipped (float64 gap at rank k <= {GAP})")
    assert skipped * 10 <= len(expected), (what, skipped)


def _allowed_of(masks, which, n):
    """Per query its allowed rows (every row for -1)."""
    return [np.ones(n, bool) if c < 0 else masks[c] for c in which]


def _expected(rows, queries, k, masks, which, l2=False):
    """The oracle once per class, in the caller's query order."""
    which = np.asarray(which)
    out = [None] * len(queries)
    for c in sorted(set(which.tolist())):
        members = np.nonzero(which == c)[0]
        allowed = np.ones(len(rows), bool) if c < 0 else masks[c]
        for qi, e in zip(members, _oracle(rows, queries[members], k, allowed, l2)):
            out[qi] = e
    return out


def _planned(which, block_slots=256):
    which = list(which)
    slots = sum(16 * -(-which.count(c) // 16) for c in set(which))
    return len(set(which)), -(-slots // block_slots)


def _alone(native, ix, queries, k, masks, which):
    got = [ix.search(q[None, :], k, mask_words=None if c < 0 else native.pack_row_mask(masks[c])) for q, c in zip(queries, which)]
    return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])


def _run(native, ix, rows, queries, k, masks, which, what, l2=False, overflowed=(), tiles=True):
    """``overflowed``: the queries the case expects to overflow (repaired: ids against the oracle only)."""
    n, nq = len(rows), len(queries)
    idx, score = ix.search_multimask(queries, k, [native.pack_row_mask(m) for m in masks], which)
    if tiles:
        classes, blocks = _planned(which, 128 if l2 else 256)
        assert ix.get_option("last_batch_masked") == 2 and ix.get_option("last_gemm_family") == 3, what
        assert ix.get_option("last_batch_mask_classes") == classes and ix.get_option("last_batch_blocks") == blocks, what
        st = ix.batch_status(nq)
        print(f"{what}: {classes} classes, {blocks} blocks, candidates per query max {int(st['counts'].max())}, capacity {st['capacity']}")
        over = np.nonzero(st["counts"] > st["capacity"])[0].tolist()
        assert over == sorted(overflowed) and st["overflowed"] == len(over), (what, "overflowed queries", over)
    else:
        assert ix.get_option("last_batch_masked") != 2, what
    for qi, allowed in enumerate(_allowed_of(masks, which, n)):
        got = idx[qi][idx[qi] >= 0]
        assert np.all(got < n) and np.all(allowed[got]), (what, qi, "a row outside the query's mask came back")
    exact = [qi for qi in range(nq) if qi not in set(overflowed)]
    expected = _expected(rows, queries, k, masks, which, l2)
    _compare(idx[exact], score[exact], [expected[qi] for qi in exact], k, what)
    if len(overflowed):
        rep = sorted(overflowed)
        _compare(idx[rep], score[rep], [expected[qi] for qi in rep], k, what + " (repaired)", ids_only=True)
    a_idx, a_score = _alone(native, ix, queries, k, masks, which)
    assert np.array_equal(idx[exact], a_idx[exact]), what
    assert np.array_equal(score[exact].view(np.uint32), a_score[exact].view(np.uint32)), what
    assert np.array_equal(idx, a_idx), what
    return idx, score


def _random_masks(n, fractions, seed):
    rng = np.random.default_rng(seed)
    return [rng.random(n) < f for f in fractions]


# The cases that compare with the oracle on a corpus nobody writes to: name -> (rows, dim, l2, k, masks, query_mask, queries,
# first query's counter).  tests/test_multimask_oracle.py walks the same table on the CPU (rows from the oracle's generator)
# and asserts that the gap rule skips NO query of any case: the 1-in-10 allowance is never what lets a case pass.
def _case(name):
    mixed = [(qi % 5) - 1 for qi in range(40)]  # -1, 0, 1, 2, 3, -1, ...
    sizes = np.random.default_rng(4).permutation([0] * 1 + [1] * 15 + [2] * 16 + [3] * 17).tolist()
    big = [0] * 300
    for at in (0, 151, 302):
        big.insert(at, 1)
    seven = np.zeros(N_SMALL, bool)
    seven[[5, 255, 256, 31_000, 31_001, 69_999, N_SMALL - 1]] = True
    S, L = (N_SMALL, D_SMALL), (N_LARGE, D_LARGE)
    table = {
        "mixed k=10": (*S, False, 10, lambda: _random_masks(N_SMALL, (0.5, 0.1, 0.01, 0.001), 1), mixed, 40, 0),
        "mixed k=100 small": (*S, False, 100, lambda: _random_masks(N_SMALL, (0.5, 0.1, 0.01, 0.001), 1), mixed, 40, 0),
        "mixed k=100 large": (*L, False, 100, lambda: _random_masks(N_LARGE, (0.5, 0.1, 0.01, 0.001), 2), mixed, 40, 0),
        "sizes": (*S, False, 10, lambda: _random_masks(N_SMALL, (0.3, 0.05, 0.6, 0.02), 3), sizes, 49, 100),
        "twenty": (*S, False, 10, lambda: _random_masks(N_SMALL, [0.02 + 0.045 * c for c in range(20)], 5),
                   [qi % 20 for qi in range(260)], 260, 200),
        "300 and 3": (*S, False, 10, lambda: _random_masks(N_SMALL, (0.25, 0.03), 6), big, 303, 500),
        "zeros": (*S, False, 10, lambda: [np.zeros(N_SMALL, bool)] + _random_masks(N_SMALL, (0.2,), 7), [0, 1, -1] * 8, 24, 820),
        "seven": (*S, False, 10, lambda: _random_masks(N_SMALL, (0.4,), 8) + [seven] + _random_masks(N_SMALL, (0.05,), 9),
                  [0, 1, 2] * 10, 30, 850),
        "l2": (*S, True, 10, lambda: _random_masks(N_SMALL, (0.5, 0.04), 10), [(qi % 3) - 1 for qi in range(45)], 45, 900),
        "l2 blocks": (*S, True, 10, lambda: _random_masks(N_SMALL, (0.3, 0.1, 0.05), 11), [qi % 3 for qi in range(150)], 150, 950),
        "none": (*S, False, 10, lambda: [], [-1] * 70, 70, 40),
        "routes": (*S, False, 10, lambda: _random_masks(N_SMALL, (0.5, 0.02), 12), [(qi % 3) - 1 for qi in range(39)], 39, 700),
        "sixteen": (*L, False, 10, lambda: _random_masks(N_LARGE, [(0.5, 0.1, 0.01, 0.2)[c % 4] for c in range(16)], 13),
                    [qi % 16 for qi in range(256)], 256, 3000),
    }
    n, d, l2, k, masks, which, nq, first = table[name]
    queries = _queries(nq, d, first)
    # Query counters first .. first + nq - 1, except where the ORACLE's gap at rank k is 1e-5 or less: those positions take
    # another counter (found with the oracle alone, on the CPU, never with the library)
    swaps = {"mixed k=100 small": {17: 1040, 22: 1041}, "mixed k=100 large": {5: 1040, 33: 1041, 35: 1043},
             "300 and 3": {292: 1803}, "sixteen": {220: 4256, 249: 4257}}
    for at, counter in swaps.get(name, {}).items():
        queries[at] = _queries(1, d, counter)[0]
    return n, d, l2, k, masks(), which, queries


CASE_NAMES = ("mixed k=10", "mixed k=100 small", "mixed k=100 large", "sizes", "twenty", "300 and 3", "zeros", "seven", "l2",
              "l2 blocks", "none", "routes", "sixteen")


def _run_case(native, name, what, **kw):
    n, d, l2, k, masks, which, queries = _case(name)
    ix, rows = _corpus(native, n, d, native.METRIC_L2 if l2 else None)
    return _run(native, ix, rows, queries, k, masks, which, what, l2=l2, **kw)


# ---- 1. four random masks of very different selectivity and the maskless class, interleaved --------------------------------
def test_four_masks_and_none_interleaved(native):
    _run_case(native, "mixed k=10", "4 masks + none, k=10")


def test_four_masks_and_none_interleaved_k100(native):
    """k = 100.  On 70 003 rows the batched path itself is closed at that k (it asks for k x 1024 <= rows, as for every
    batch), so the same entry point answers class by class: everything is compared but the route.  On 262 147 rows the tile
    pass runs and every assertion applies."""
    _run_case(native, "mixed k=100 small", "4 masks + none, k=100, 70 003 rows", tiles=False)
    _run_case(native, "mixed k=100 large", "4 masks + none, k=100, 262 147 rows")


# ---- 2. class sizes around a column group -------------------------------------------------------------------------------------
def test_class_sizes_1_15_16_17(native):
    which = _case("sizes")[5]
    assert _planned(which) == (4, 1) and sorted(which.count(c) for c in range(4)) == [1, 15, 16, 17]
    _run_case(native, "sizes", "classes of 1 / 15 / 16 / 17")


# ---- 3. more column groups than a block holds ----------------------------------------------------------------------------------
def test_twenty_classes_span_two_blocks(native):
    assert _planned(_case("twenty")[5]) == (20, 2)
    _run_case(native, "twenty", "20 classes of 13")


# ---- 4. a class larger than a block next to a small one ----------------------------------------------------------------------
def test_class_of_300_next_to_a_class_of_3(native):
    which = _case("300 and 3")[5]
    assert _planned(which) == (2, 2) and which.count(1) == 3 and which.count(0) == 300
    _run_case(native, "300 and 3", "300 next to 3")


# ---- 5. / 6. an all-zero mask, seven allowed rows ---------------------------------------------------------------------------------
def test_all_zero_mask_returns_nothing_for_its_queries(native):
    idx, _ = _run_case(native, "zeros", "all zeros")
    assert np.all(idx[0::3] == -1) and np.all(idx[1::3] >= 0) and np.all(idx[2::3] >= 0)


def test_seven_allowed_rows_k10_leave_the_neighbours_alone(native):
    idx, score = _run_case(native, "seven", "seven rows")
    assert np.all(idx[1::3, :7] >= 0) and np.all(idx[1::3, 7:] == -1) and np.all(np.diff(score[1::3, :7], axis=1) <= 0)
    assert np.all(idx[0::3] >= 0) and np.all(idx[2::3] >= 0)


# ---- 7. no sampled tile holds an allowed row: answered from the candidates below 16 384 rows, repaired above ---------------
def _sampled_tiles(n, k, allowed_rows):
    """The tiles a block's sample pass visits, derived as the host does (enqueue_search_gemm8): 1 / 32 of the tiles
    (k = 10), at least 8 k blocks; for the block's most selective class above 16 384 rows grown by 1 / f up to 8 x and to
    8 k expected vouching blocks."""
    tiles, rw = (n + 255) // 256, 8
    sample = max(tiles // min(32, max(4, 1024 // k)), (8 * k + rw - 1) // rw)
    if allowed_rows > 16384:
        f = allowed_rows / n
        pv = 1.0 - (1.0 - min(f, 1.0)) ** 32
        sample = min(int(np.ceil(max(sample * min(1.0 / f, 8.0), 8.0 * k / (rw * max(pv, 1e-9))))), tiles)
    sample = max(1, min(sample, tiles))
    return {t * (tiles // sample) for t in range(sample)}


def _mask_without_sampled_tiles(n, k, wanted_tiles):
    """Whole tiles of ``wanted_tiles`` minus whatever the sample visits; the sample depends on the allowed rows, so to a fixed
    point.  Returns (allowed rows as bool[n], the sampled tiles)."""
    tile_of = np.arange(n) // 256
    chosen = set(wanted_tiles)
    for _ in range(8):
        allowed = np.isin(tile_of, sorted(chosen))
        sampled = _sampled_tiles(n, k, int(allowed.sum()))
        if not (chosen & sampled):
            return allowed, sampled
        chosen = set(wanted_tiles) - sampled
    raise AssertionError("no fixed point")


def test_no_sampled_tile_allowed_small_class_from_candidates_large_class_repaired(native):
    """Both classes share one block, so the block's sample is the one of its only class above 16 384 rows.  Neither class
    allows a row of a sampled tile: tau = -inf for every query.  The class of at most 16 384 rows fits the candidate buffers
    (no overflow); the class above does not: each of its queries overflows and is repaired by the fp32 scan with ITS mask."""
    ix, rows = _corpus(native, N_SMALL, D_SMALL)
    n, k, tiles = N_SMALL, 10, (N_SMALL + 255) // 256
    large, sampled = _mask_without_sampled_tiles(n, k, [t for t in range(tiles) if t % 3 != 0])
    small = np.isin(np.arange(n) // 256, [t for t in range(tiles) if t % 5 == 3 and t not in sampled])
    in_sampled = np.isin(np.arange(n) // 256, sorted(sampled))
    assert large.sum() > 16384 and 4096 < small.sum() <= 16384 and not np.any((large | small)[in_sampled])
    which = [0, 1] * 12
    idx, _ = _run(native, ix, rows, _queries(24, D_SMALL, 60), k, [small, large], which, "no sampled tile allowed",
                  overflowed=range(1, 24, 2))
    assert ix.get_option("last_batch_repaired") == 1
    assert np.all(idx >= 0)


# ---- 8. L2 ----------------------------------------------------------------------------------------------------------------------
def test_l2_three_classes(native):
    _run_case(native, "l2", "L2, 3 classes")


def test_l2_blocks_hold_128_slots(native):
    assert _planned(_case("l2 blocks")[5], 128) == (3, 2)  # 3 classes of 50: 3 x 64 slots = 2 blocks of at most 128
    _run_case(native, "l2 blocks", "L2, two blocks")


# ---- 9. removed rows (NaN) inside allowed sets --------------------------------------------------------------------------------
def test_nan_tombstones_inside_allowed_sets(native):
    n, d, k = N_SMALL, D_SMALL, 10
    queries = _queries(36, d, 80)
    masks = [np.arange(n) % 3 != 1, np.arange(n) % 7 == 2]
    which = [(qi % 3) - 1 for qi in range(36)]
    with _open(native, n, d) as ix:
        rows0 = ix.get_rows(0, n)
        first = _expected(rows0, queries, k, masks, which)
        dead = np.unique(np.concatenate([e[0][:3] for e in first] + [np.array([0, 1, 2, 255, 256, n - 1])]))  # best rows of every class
        for r in dead:
            ix.set_rows(int(r), np.full((1, d), np.nan, np.float32))
        rows = rows0.copy()
        rows[dead] = np.nan
        idx, _ = _run(native, ix, rows, queries, k, masks, which, "tombstones")
        assert not np.any(np.isin(idx, dead))


# ---- 10. no masks at all --------------------------------------------------------------------------------------------------------
def test_no_masks_equals_the_unmasked_batch(native):
    ix, rows = _corpus(native, N_SMALL, D_SMALL)
    queries = _case("none")[6]
    idx, score = _run_case(native, "none", "no masks")
    u_idx, u_score = ix.search(queries, 10)
    assert ix.get_option("last_batch_masked") == 0 and ix.get_option("last_gemm_family") == 3
    assert ix.get_option("last_batch_mask_classes") == 0 and ix.get_option("last_batch_blocks") == 0
    assert np.array_equal(idx, u_idx) and np.array_equal(score.view(np.uint32), u_score.view(np.uint32))
    # ... and a single-mask call reads 1, not 2
    ix.search(queries, 10, mask_words=native.pack_row_mask(np.arange(N_SMALL) % 3 != 1))
    assert ix.get_option("last_batch_masked") == 1 and ix.get_option("last_batch_mask_classes") == 0


# ---- 11. the fall-back route ----------------------------------------------------------------------------------------------------
def test_gemm_masked_off_takes_the_per_mask_calls_with_the_same_answers(native):
    ix, rows = _corpus(native, N_SMALL, D_SMALL)
    idx, score = _run_case(native, "routes", "tile route")
    ix.set_option("gemm_masked", 0)
    try:
        f_idx, f_score = _run_case(native, "routes", "fall-back route", tiles=False)
    finally:
        ix.set_option("gemm_masked", 1)
    assert np.array_equal(idx, f_idx) and np.array_equal(score.view(np.uint32), f_score.view(np.uint32))


# ---- 12. refused arguments ------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused(native):
    ix, _ = _corpus(native, N_SMALL, D_SMALL)
    lib = native.load_library()
    f32p, i64p, u32p, u64p, i32p = (C.POINTER(t) for t in (C.c_float, C.c_int64, C.c_uint32, C.c_uint64, C.c_int32))
    nq, k = 8, 10
    queries = np.ascontiguousarray(_queries(nq, D_SMALL))
    full = native.pack_row_mask(np.ones(N_SMALL, bool))
    idx, score = np.empty((nq, WDBX_MAX_K + 1), np.int64), np.empty((nq, WDBX_MAX_K + 1), np.float32)

    def call(masks, which, nq=nq, k=k, n_masks=None, counts=None, null_at=None):
        ptrs = (u32p * max(len(masks), 1))(*[m.ctypes.data_as(u32p) for m in masks])
        if null_at is not None:
            ptrs[null_at] = u32p()
        cnt = np.array([m.size for m in masks] if counts is None else counts, np.uint64)
        w = np.ascontiguousarray(which, np.int32)
        return lib.wdbx_index_search_multimask(ix._h, queries.ctypes.data_as(f32p), nq, k, 0, ptrs, cnt.ctypes.data_as(u64p),
                                               len(masks) if n_masks is None else n_masks, w.ctypes.data_as(i32p),
                                               idx.ctypes.data_as(i64p), score.ctypes.data_as(f32p))

    assert call([full, full], [0, 1] * 4) == 0
    assert call([full] * 65, [0] * nq) == E_INVALID            # n_masks above WDBX_MAX_CALL_MASKS
    assert call([full], [0] * nq, n_masks=-1) == E_INVALID     # ... below 0
    assert call([full] * 64, [63] * nq) == 0                   # (the largest count is fine)
    assert call([full, full], [0, 1, 2, 0, 0, 0, 0, 0]) == E_INVALID   # an entry equal to n_masks
    assert call([full, full], [0, -2, 1, 0, 0, 0, 0, 0]) == E_INVALID  # ... below -1
    assert call([], [0] * nq) == E_INVALID                             # ... with no masks at all
    assert call([full, full[:-1].copy()], [0] * nq) == E_INVALID       # a short mask (even one no query reads)
    assert call([full, full], [0] * nq, counts=[full.size, full.size - 1]) == E_INVALID
    assert call([full, full], [0] * nq, null_at=1) == E_INVALID        # a null mask pointer
    assert call([full], [0] * nq, k=0) == E_INVALID
    assert call([full], [0] * nq, k=WDBX_MAX_K + 1) == E_INVALID
    assert call([full], [0] * nq, k=WDBX_MAX_K) == 0
    assert call([full], [0] * nq, nq=0) == E_INVALID
    assert call([full], [0] * nq, nq=-3) == E_INVALID
    with pytest.raises(ValueError):
        ix.search_multimask(queries, k, [full], [0] * (nq + 1))  # the binding: one entry per query
    after = ix.search(queries, k)  # no refused call left a mask active
    assert ix.get_option("last_batch_masked") == 0 and np.all(after[0] >= 0)


# ---- the shape the feature is for: 256 callers, 16 filters, one block ------------------------------------------------------
def test_sixteen_classes_of_sixteen_are_one_block(native):
    ix, rows = _corpus(native, N_LARGE, D_LARGE)
    _, _, _, _, masks, which, queries = _case("sixteen")
    assert _planned(which) == (16, 1)
    ix.profile(True)
    try:
        ix.profile_read_gemm()
        ix.search_multimask(queries, 10, [native.pack_row_mask(m) for m in masks], which)
        assert ix.profile_read_gemm()["gemm_launches"] == 2  # one sample pass and one full pass for all 16 masks
    finally:
        ix.profile(False)
    _run_case(native, "sixteen", "16 classes of 16")
