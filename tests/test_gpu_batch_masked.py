"""Filtered batch search: a row mask on the int8 tile path (wdbx_index_search_masked(_n) with enough queries,
wdbx_index_search_batch_masked_device, the shard group's masked calls).

What every case compares (``_run``):
  * the call ran the masked tile pass: ``last_batch_masked == 1`` and ``last_gemm_family == 3`` (int8 tiles);
  * ids against numpy's exact search restricted to the allowed rows.  Per query the test re-derives in float64 that the gap
    at rank k among the allowed rows exceeds 1e-5 (else the query is skipped: at most 1 in 10, printed; for these iid corpora
    the gap is ~1e-3).  That gap guards the SET of the k best; their ORDER is compared too wherever the float64 scores of
    neighbours inside the list differ by more than 1e-6 (fp32 sums of d <= 384 products of unit vectors round within ~1e-7);
  * scores within 1e-5 of the oracle;
  * ids and scores bit-identical to the same queries sent one at a time with the same mask (the per-query masked selection
    scan + exact re-scoring that existed before), for every query;
  * NO query overflowed: every candidate count is within the capacity and nothing was repaired.  The masked pass filters
    at append, so a mask -- however selective -- must not fill the candidate or pair lists with masked-out rows; were it
    to, the repair scans would still answer exactly and only this assertion (and the bit comparison: a repaired query
    carries the repair scan's scores, whose summation order is not ``rescore_kernel``'s) would tell.  Overflow is expected
    in ONE case of this file, the near-duplicate corpus of case 9, which checks it on its own.

Corpora come from ``fill_synthetic`` and are read back; ``gemm_min_rows = 16384`` lets these small corpora reach the tiles,
``single_min_rows = 0`` lets the one-at-a-time calls take the selection scan below 131 072 rows (as ``smoke()`` does)."""
import ctypes as C

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

ATOL = 1e-5
GAP = 1e-5
N_SMALL, N_LARGE = 70_003, 262_147


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
    if not len(rows_a):
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


def _compare(idx, score, expected, k, what):
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
            np.testing.assert_allclose(np.sort(score[qi][:kk]), e_score, atol=ATOL, rtol=0)
            continue
        np.testing.assert_allclose(score[qi][:kk], e_score, atol=ATOL, rtol=0)
    print(f"{what}: {skipped} of {len(expected)} queries skipped (float64 gap at rank k <= {GAP})")
    assert skipped * 10 <= len(expected), (what, skipped)


def _singles(ix, queries, k, words):
    got = [ix.search(q[None, :], k, mask_words=words) for q in queries]
    return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])


def _run(native, ix, rows, queries, k, allowed, what, l2=False, singles=True):
    words = native.pack_row_mask(allowed)
    idx, score = ix.search(queries, k, mask_words=words)
    assert ix.get_option("last_batch_masked") == 1 and ix.get_option("last_gemm_family") == 3, what
    assert ix.get_option("last_batch_allowed_rows") == int(np.count_nonzero(allowed)), what
    assert not np.any(idx >= len(allowed)) and np.all(allowed[idx[idx >= 0]]), (what, "a masked-out row came back")
    st = ix.batch_status(len(queries))
    print(f"{what}: candidates per query max {int(st['counts'].max())}, capacity {st['capacity']}, allowed rows {int(allowed.sum())}")
    assert st["overflowed"] == 0 and np.all(st["counts"] <= st["capacity"]), (what, "a query overflowed and went to the repair scan")
    assert np.all(st["counts"] <= np.count_nonzero(allowed)), what
    _compare(idx, score, _oracle(rows, queries, k, allowed, l2), k, what)
    if singles:
        s_idx, s_score = _singles(ix, queries, k, words)
        assert ix.get_option("last_batch_masked") == 0
        assert np.array_equal(idx, s_idx) and np.array_equal(score.view(np.uint32), s_score.view(np.uint32)), what
    return idx, score


# ---- 1. dense mask, every query-block width and the blocks around them --------------------------------------------------
@pytest.mark.parametrize("nq", [4, 64, 65, 256, 257])
@pytest.mark.parametrize("d,k", [(384, 10), (96, 1)])
def test_dense_mask(native, nq, d, k):
    ix, rows = _corpus(native, N_SMALL, d)
    allowed = np.arange(N_SMALL) % 3 != 1
    _run(native, ix, rows, _queries(nq, d), k, allowed, f"dense d={d} k={k} nq={nq}")


@pytest.mark.parametrize("d,k", [(384, 1), (96, 10)])
def test_dense_mask_other_k(native, d, k):
    ix, rows = _corpus(native, N_SMALL, d)
    _run(native, ix, rows, _queries(65, d, 300), k, np.arange(N_SMALL) % 3 != 1, f"dense d={d} k={k}")


def test_dense_mask_large_corpus_k100(native):
    ix, rows = _corpus(native, N_LARGE, 384)
    _run(native, ix, rows, _queries(64, 384), 100, np.arange(N_LARGE) % 3 != 1, "dense n=262147 k=100")


def test_dense_mask_l2(native):
    ix, rows = _corpus(native, N_SMALL, 384, native.METRIC_L2)
    _run(native, ix, rows, _queries(65, 384), 10, np.arange(N_SMALL) % 3 != 1, "dense L2", l2=True)


# ---- 2. a selective random mask ---------------------------------------------------------------------------------------------
def test_random_one_in_fifty(native):
    ix, rows = _corpus(native, N_SMALL, 384)
    allowed = np.random.default_rng(7).random(N_SMALL) < 0.02
    queries = _queries(64, 384, 20)
    idx, score = _run(native, ix, rows, queries, 10, allowed, "random 1 in 50")
    for qi in (0, 63):  # the helper above against the oracle module's own masked search
        o_idx, o_score = O.flat_search(rows, queries[qi], 10, normalize_query=False, allowed=allowed)
        assert idx[qi].tolist() == o_idx.tolist()
        np.testing.assert_allclose(score[qi], o_score, atol=ATOL, rtol=0)


# ---- 3. / 4. / 5. all ones, all zeros, fewer allowed rows than k -------------------------------------------------------------
def test_all_ones_equals_the_unmasked_batch(native):
    ix, rows = _corpus(native, N_SMALL, 384)
    queries = _queries(70, 384, 40)
    idx, score = _run(native, ix, rows, queries, 10, np.ones(N_SMALL, bool), "all ones")
    u_idx, u_score = ix.search(queries, 10)
    assert ix.get_option("last_batch_masked") == 0 and ix.get_option("last_gemm_family") == 3
    assert np.array_equal(idx, u_idx) and np.array_equal(score.view(np.uint32), u_score.view(np.uint32))


def test_all_zeros_returns_nothing(native):
    ix, rows = _corpus(native, N_SMALL, 384)
    idx, score = ix.search(_queries(64, 384), 10, mask_words=native.pack_row_mask(np.zeros(N_SMALL, bool)))
    assert ix.get_option("last_batch_masked") == 1 and ix.get_option("last_batch_allowed_rows") == 0
    assert np.all(idx == -1)


def test_seven_allowed_rows_k10(native):
    ix, rows = _corpus(native, N_SMALL, 384)
    allowed = np.zeros(N_SMALL, bool)
    allowed[[5, 255, 256, 31_000, 31_001, 69_999, N_SMALL - 1]] = True
    idx, score = _run(native, ix, rows, _queries(64, 384), 10, allowed, "seven rows")
    assert np.all(idx[:, :7] >= 0) and np.all(idx[:, 7:] == -1)
    assert np.all(np.diff(score[:, :7], axis=1) <= 0)


# ---- 6. bits past the last row, odd word count -----------------------------------------------------------------------------
def test_bits_past_the_end_are_ignored(native):
    n = N_SMALL + 32  # (an ODD number of mask words, the last one partly used)
    queries = _queries(64, 384)
    with _open(native, n, 384) as ix:
        rows = ix.get_rows(0, n)
        allowed = np.arange(n) % 3 != 1
        words = native.pack_row_mask(allowed).copy()
        assert words.size == (n + 31) // 32 and words.size % 2 == 1 and n % 32 != 0
        words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)  # every bit past n
        idx, score = ix.search(queries, 10, mask_words=words)
        assert ix.get_option("last_batch_masked") == 1 and ix.get_option("last_gemm_family") == 3
        assert ix.get_option("last_batch_allowed_rows") == int(np.count_nonzero(allowed))
        assert np.all(idx >= 0) and np.all(idx < n)
        _compare(idx, score, _oracle(rows, queries, 10, allowed), 10, "bits past the end")
        c_idx, c_score = ix.search(queries, 10, mask_words=native.pack_row_mask(allowed))
        assert np.array_equal(idx, c_idx) and np.array_equal(score, c_score)
        # ... and a mask that allows ONLY the last rows: nothing past the end comes back in their place
        tail = np.zeros(n, bool)
        tail[-3:] = True
        w2 = native.pack_row_mask(tail).copy()
        w2[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
        idx, _ = ix.search(queries, 10, mask_words=w2)
        assert ix.get_option("last_batch_masked") == 1 and ix.get_option("last_batch_allowed_rows") == 3
        assert np.all(np.sort(idx[:, :3], axis=1) == np.arange(n - 3, n)) and np.all(idx[:, 3:] == -1)


# ---- 7. planted rows: a masked-out row must not vouch for the threshold ----------------------------------------------------
def test_masked_out_copies_of_the_queries_do_not_vouch(native):
    """Copies of four queries in EVERY 256-row tile (so in every tile any sample visits) and 20 000 more spread over the
    corpus, all masked out.  Were one of them to vouch in the sample pass, tau would be ~1 for its query and the full pass
    would keep nothing."""
    n, d, k, nq, planted_q = N_SMALL, 384, 10, 64, 4
    queries = _queries(nq, d, 500)
    tiles = (n + 255) // 256
    with _open(native, n, d) as ix:
        planted = np.zeros(n, bool)
        rows = ix.get_rows(0, n)
        for p in range(planted_q):
            at = np.minimum(np.arange(tiles) * 256 + 17 + 40 * p, n - 1 - p)
            spread = (np.arange(5000) * 14 + 3 + p) % n
            where = np.unique(np.concatenate([at, spread]))
            planted[where] = True
            rows[where] = queries[p]
        ix.set_rows(0, rows)
        rows = ix.get_rows(0, n)
        allowed = ~planted
        assert np.count_nonzero(planted) >= planted_q * 5000
        idx, score = _run(native, ix, rows, queries, k, allowed, "planted", singles=False)
        assert not np.any(planted[idx])
        assert np.all(score[:planted_q, 0] < 0.9)  # (the copies would score 1)
        st = ix.batch_status(nq)
        assert np.all(st["counts"] <= ix.get_option("last_batch_allowed_rows"))
        s_idx, s_score = _singles(ix, queries[:8], k, native.pack_row_mask(allowed))
        assert np.array_equal(idx[:8], s_idx) and np.array_equal(score[:8], s_score)  # (a few one at a time, too)


# ---- 8. whole tiles masked out, every sampled tile among them ---------------------------------------------------------------
def _sampled_tiles(n, k, allowed_rows):
    """The tiles the sample pass visits, derived as the host does (enqueue_search_gemm8): 1 / 32 of the tiles (k = 10), at
    least 8 k blocks; for a mask of more than 16 384 rows grown by 1 / f up to 8 x and to 8 k expected vouching blocks."""
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


def test_whole_tiles_masked_out_small_mask_is_answered_from_the_candidates(native):
    """Every fifth tile allowed, none of them a sampled tile, at most 16 384 rows: no block vouches, tau stays -inf, EVERY
    allowed row is a candidate of every query -- and fits, since the capacity covers such a mask: no overflow, no repair."""
    ix, rows = _corpus(native, N_SMALL, 384)
    tiles, nq, k = (N_SMALL + 255) // 256, 64, 10
    allowed, sampled = _mask_without_sampled_tiles(N_SMALL, k, [t for t in range(tiles) if t % 5 == 3])
    assert 4096 < allowed.sum() <= 16384 and not np.any(allowed[np.isin(np.arange(N_SMALL) // 256, sorted(sampled))])
    _run(native, ix, rows, _queries(nq, 384, 60), k, allowed, "tiles, small mask")
    # the candidates as the full pass left them (second selection stage off: it would drop most of them again): ALL allowed rows
    ix.set_option("gemm8_refine", 0)
    try:
        idx, score = ix.search(_queries(nq, 384, 60), k, mask_words=native.pack_row_mask(allowed))
        st = ix.batch_status(nq)
    finally:
        ix.set_option("gemm8_refine", 1)
    assert np.all(st["counts"] == allowed.sum()) and st["capacity"] >= allowed.sum() and st["overflowed"] == 0
    _compare(idx, score, _oracle(rows, _queries(nq, 384, 60), k, allowed), k, "tiles, small mask, no refine")


def test_whole_tiles_masked_out_large_mask_is_repaired_with_the_mask(native):
    """Two tiles in three allowed, none of them a sampled tile, more than 16 384 rows: tau = -inf again, but the rows do not
    fit: every query overflows and is repaired on the device by the MASKED fp32 scan.  Exact, no masked-out row, ids those
    of the one-at-a-time calls.  (Scores: within 1e-5 of the oracle.  The repair scan sums in another order than
    ``rescore_kernel``: measured on an MI355X, 64 repaired queries had scores 1 ulp apart from the single-query paths --
    1043946391 vs 1043946392 as bit patterns -- exactly as repaired queries of an unmasked batch do.)"""
    ix, rows = _corpus(native, N_SMALL, 384)
    tiles, nq, k = (N_SMALL + 255) // 256, 64, 10
    allowed, sampled = _mask_without_sampled_tiles(N_SMALL, k, [t for t in range(tiles) if t % 3 != 0])
    assert allowed.sum() > 16384 and not np.any(allowed[np.isin(np.arange(N_SMALL) // 256, sorted(sampled))])
    queries, words = _queries(nq, 384, 60), native.pack_row_mask(allowed)
    idx, score = ix.search(queries, k, mask_words=words)
    assert ix.get_option("last_batch_masked") == 1 and ix.get_option("last_gemm_family") == 3
    assert ix.get_option("last_batch_repaired") == 1
    st = ix.batch_status(nq)
    assert st["overflowed"] == nq and np.all(st["counts"] > st["capacity"])
    assert np.all(idx >= 0) and np.all(allowed[idx])
    _compare(idx, score, _oracle(rows, queries, k, allowed), k, "tiles, large mask")
    s_idx, _ = _singles(ix, queries, k, words)
    assert np.array_equal(idx, s_idx)


# ---- 9. overflow: repaired on the device by the MASKED scan ----------------------------------------------------------------
def test_overflow_is_repaired_with_the_mask_honoured(native):
    n, d, nq, k = 120_001, 64, 32, 10
    queries = _queries(nq, d)
    with _open(native, n, d) as ix:
        rows = ix.get_rows(0, n)
        rows[1::2] = queries[3]  # half the corpus equals query 3
        ix.set_rows(0, rows)
        rows = ix.get_rows(0, n)
        allowed = np.arange(n) % 4 != 1  # every second copy (rows 1, 5, 9, ...) is masked out
        words = native.pack_row_mask(allowed)
        idx, score = ix.search(queries, k, mask_words=words)
        assert ix.get_option("last_batch_masked") == 1 and ix.get_option("last_gemm_family") == 3
        assert ix.get_option("last_batch_repaired") == 1
        st = ix.batch_status(nq)
        assert st["overflowed"] >= 1 and st["counts"][3] > st["capacity"]
        assert np.all(allowed[idx])
        assert idx[3].tolist() == list(range(3, 4 * k, 4))  # exact ties: ascending rows, the allowed copies only
        assert np.all(score[3] == score[3][0]) and abs(score[3][0] - 1.0) < 1e-6
        keep = [qi for qi in range(nq) if qi != 3]
        _compare(idx[keep], score[keep], _oracle(rows, queries[keep], k, allowed), k, "overflow")


# ---- 10. removed rows (NaN) and a mask ------------------------------------------------------------------------------------
def test_nan_tombstones_and_a_mask(native):
    n, d, k = N_SMALL, 384, 10
    queries = _queries(64, d, 80)
    with _open(native, n, d) as ix:
        rows0 = ix.get_rows(0, n)
        allowed = np.arange(n) % 3 != 1
        first = _oracle(rows0, queries, k, allowed)
        dead = np.unique(np.concatenate([e[0][:3] for e in first] + [np.array([0, 1, 2, 255, 256, n - 1])]))  # best rows, allowed or not
        for r in dead:
            ix.set_rows(int(r), np.full((1, d), np.nan, np.float32))
        rows = rows0.copy()
        rows[dead] = np.nan
        live = allowed.copy()
        live[dead] = False
        words = native.pack_row_mask(allowed)
        idx, score = ix.search(queries, k, mask_words=words)
        assert ix.get_option("last_batch_masked") == 1 and ix.get_option("last_gemm_family") == 3
        assert not np.any(np.isin(idx, dead)) and np.all(allowed[idx])
        _compare(idx, score, _oracle(rows, queries, k, live), k, "tombstones")
        s_idx, s_score = _singles(ix, queries, k, words)
        assert np.array_equal(idx, s_idx) and np.array_equal(score, s_score)


# ---- 11. shapes that stay on the per-query paths --------------------------------------------------------------------------
def test_select_range_k_and_other_families_keep_the_old_path(native):
    ix, rows = _corpus(native, N_LARGE, 384)
    allowed = np.arange(N_LARGE) % 3 != 1
    words = native.pack_row_mask(allowed)
    queries = _queries(32, 384, 90)
    idx, score = ix.search(queries, 250, mask_words=words)
    assert ix.get_option("last_batch_masked") == 0
    _compare(idx, score, _oracle(rows, queries, 250, allowed), 250, "k=250")
    for name, value, back in (("gemm_bf16", 2, 3), ("gemm_masked", 0, 1), ("gemm8_variant", 13, 0)):
        ix.set_option(name, value)
        try:
            idx, score = ix.search(queries, 10, mask_words=words)
            assert ix.get_option("last_batch_masked") == 0, name
        finally:
            ix.set_option(name, back)
        _compare(idx, score, _oracle(rows, queries, 10, allowed), 10, name)
    idx, score = ix.search(queries, 10, mask_words=words)
    assert ix.get_option("last_batch_masked") == 1


# ---- 12. the mask does not leak ----------------------------------------------------------------------------------------------
def test_the_mask_does_not_outlive_its_call(native):
    ix, rows = _corpus(native, N_SMALL, 384)
    queries = _queries(64, 384, 120)
    before = ix.search(queries, 10)
    shadow = ix.get_option("shadowg_rows")
    ix.search(queries, 10, mask_words=native.pack_row_mask(np.arange(N_SMALL) % 7 == 0))
    assert ix.get_option("last_batch_masked") == 1
    after = ix.search(queries, 10)
    assert ix.get_option("last_batch_masked") == 0
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert ix.get_option("shadowg_rows") == shadow == N_SMALL
    assert np.array_equal(ix.get_rows(0, N_SMALL).view(np.uint32), rows.view(np.uint32))
    one = ix.search(queries[:1], 10)  # (and a lone query sees every row again)
    assert np.array_equal(one[0][0], before[0][0])


# ---- 13. a short mask is refused -------------------------------------------------------------------------------------------
def test_short_mask_is_refused_for_a_batch(native):
    ix, _ = _corpus(native, N_SMALL, 384)
    lib = native.load_library()
    queries = np.ascontiguousarray(_queries(64, 384))
    words = native.pack_row_mask(np.ones(N_SMALL, bool))[:-1].copy()
    idx, score = np.empty((64, 10), np.int64), np.empty((64, 10), np.float32)
    f32p, i64p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
    rc = lib.wdbx_index_search_masked_n(ix._h, queries.ctypes.data_as(f32p), 64, 10, 0, words.ctypes.data_as(u32p), words.size,
                                        idx.ctypes.data_as(i64p), score.ctypes.data_as(f32p))
    assert rc == -1  # WDBX_E_INVALID
    dq = ix.device_queries(queries)
    d_idx, d_score = ix.alloc(64 * 10 * 8), ix.alloc(64 * 10 * 4)
    with pytest.raises(native.HipBackendError) as err:
        ix.search_batch_masked_device(dq, 64, 10, words, d_idx, d_score)
    assert err.value.code == rc
    after = ix.search(queries, 10)  # the refused mask was not left active
    assert ix.get_option("last_batch_masked") == 0 and np.all(after[0] >= 0)


# ---- 14. the device-resident entry point --------------------------------------------------------------------------------------
def test_device_entry_point_equals_the_host_entry_point(native):
    ix, rows = _corpus(native, N_SMALL, 384)
    nq, k = 130, 10
    queries = _queries(nq, 384, 200)
    allowed = np.arange(N_SMALL) % 3 != 1
    words = native.pack_row_mask(allowed)
    h_idx, h_score = ix.search(queries, k, mask_words=words)
    dq = ix.device_queries(queries)
    d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
    ix.search_batch_masked_device(dq, nq, k, words, d_idx, d_score)
    ix.synchronize()
    assert ix.get_option("last_batch_masked") == 1 and ix.get_option("last_gemm_family") == 3
    st = ix.batch_status(nq)
    assert st["overflowed"] == 0 and np.all(st["counts"] <= np.count_nonzero(allowed))
    assert np.array_equal(d_idx.download(np.int64, (nq, k)), h_idx)
    assert np.array_equal(d_score.download(np.float32, (nq, k)), h_score)


# ---- 15. a group of two shards on one GPU, one of them masked -----------------------------------------------------------
def test_group_with_one_masked_shard(native):
    n, d, nq, k = N_SMALL, 384, 16, 10
    whole, rows = _corpus(native, n, d)
    half = 35_001
    queries = _queries(nq, d, 260)
    m0 = np.arange(half) % 3 != 1
    allowed = np.concatenate([m0, np.ones(n - half, bool)])
    w_idx, w_score = _run(native, whole, rows, queries, k, allowed, "whole index")
    shards = [native.NativeIndex(d, capacity_rows=half) for _ in range(2)]
    try:
        shards[0].add(rows[:half])
        shards[1].add(rows[half:])
        for s in shards:
            s.set_option("gemm_min_rows", 16384)
        with native.NativeGroup.attach(shards) as grp:
            grp.set_row_bases([0, half])
            before = grp.stat("exchanges")
            idx, score = grp.search_merged(queries, k, k, mask_words=[native.pack_row_mask(m0), None])
            assert grp.stat("exchanges") - before == 1  # one chunk of 16 queries: one exchange, not 16
            assert shards[0].get_option("last_batch_masked") == 1 and shards[0].get_option("last_gemm_family") == 3
            assert shards[1].get_option("last_batch_masked") == 0 and shards[1].get_option("last_gemm_family") == 3
    finally:
        for s in shards:
            s.close()
    assert np.array_equal(idx, w_idx) and np.array_equal(score, w_score)
