"""GPU parity: the HIP path (through the C ABI) against the oracle on identical inputs.

Bar: row ids and their order bit-exact (integer/index work), scores within 1e-5
absolute for cosine on unit rows (BASELINE.json north_star), 1e-5 relative for L2
on un-normalised data.  A differing id is accepted only where the
fp64 shadow shows the two candidates closer than fp32 can resolve.
"""
import json
from pathlib import Path

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

ATOL = 1e-5

# Pre-screened query offsets per BASELINE config (tools/prescreen_queries.py): the best k + 1 float64 scores of
# these queries have no adjacent gap below 1e-5, so their ids are asserted EXACTLY -- no tolerance helper is involved.
_STRICT = json.loads((Path(__file__).resolve().parent / "golden" / "strict_queries.json").read_text())
# how often the tolerant comparison (fuzz / adversarial inputs only) accepted a difference: printed at the end of the run
PARITY_STATS = {"tolerant_comparisons": 0, "tolerated_swaps": 0, "strict_queries": 0}


def _strict_queries(name, count, d):
    """The first ``count`` accepted query offsets of config ``name`` and the queries themselves."""
    rec = _STRICT["configs"][name]
    offs = rec["accepted"][:count]
    assert len(offs) == count and rec["dim"] == d, (name, len(rec["accepted"]), count)
    return offs, np.concatenate([O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, o, 1, d)) for o in offs])


def _assert_strict(idx, score, expected, rtol=0.0, config="t"):
    """``expected`` = oracle.slab_search_screened(...): ids identical, scores within the north-star tolerance, and the
    fixture confirmed on the bytes read back (every query's float64 gap is what the pre-screen promised for ``config``)."""
    for qi, (e_idx, e_score, gap) in enumerate(expected):
        assert gap >= 0.5 * _STRICT["configs"][config]["gap_min"], f"query {qi}: float64 gap {gap} -- not a pre-screened query"
        assert idx[qi][: len(e_idx)].tolist() == e_idx.tolist(), f"query {qi}: ids differ from the oracle (float64 gap {gap})"
        np.testing.assert_allclose(score[qi][: len(e_idx)], e_score, atol=ATOL, rtol=rtol)
        PARITY_STATS["strict_queries"] += 1


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


def _ids_match(got_idx, got_score, exp_idx, exp_score, tie=1e-6):
    """For fuzz / adversarial / unscreened inputs ONLY (the BASELINE configs assert exact ids, ``_assert_strict``): ids
    equal, or differing only by swaps between candidates whose oracle scores are closer than fp32 summation-order noise
    (or a flip at the cut-off rank).  Returns the number of positions it tolerated (0 = identical)."""
    got_idx, exp_idx = list(got_idx), list(exp_idx)
    PARITY_STATS["tolerant_comparisons"] += 1
    if got_idx == exp_idx:
        return 0
    swaps = 0
    for p, (g, e) in enumerate(zip(got_idx, exp_idx)):
        if g == e:
            continue
        swaps += 1
        scale = max(1.0, abs(float(exp_score[p])))
        if g in exp_idx:
            other = exp_idx.index(g)
            assert abs(float(exp_score[other]) - float(exp_score[p])) <= tie * scale, (p, g, e)
        else:
            assert p >= len(exp_idx) - 2 and abs(float(got_score[p]) - float(exp_score[p])) <= tie * scale, (p, g, e)
    PARITY_STATS["tolerated_swaps"] += swaps
    return swaps


def _rows(seed, n, d, normalize=True):
    r = O.synth_rows(seed, 0, n, d)
    return O.normalize_rows_fast(r) if normalize else r


def _check(idx, score, rows, q, k, metric=O.METRIC_COSINE, rtol=0.0):
    """Compare one query's GPU result with the oracle."""
    n = rows.shape[0]
    kk = min(k, n)
    o_idx, o_score = O.flat_search(rows, q, kk, metric, normalize_query=False)
    assert idx.shape == (k,) and score.shape == (k,)
    assert np.all(idx[kk:] == -1), "unused slots must hold -1"
    got_idx, got_score = idx[:kk], score[:kk]
    if rtol:
        np.testing.assert_allclose(got_score, o_score, rtol=rtol, atol=ATOL)
    else:
        np.testing.assert_allclose(got_score, o_score, rtol=0, atol=ATOL)
    PARITY_STATS["tolerant_comparisons"] += 1
    if not np.array_equal(got_idx, o_idx):
        s64 = O.flat_scores_f64(rows, q, metric)
        bad = np.nonzero(got_idx != o_idx)[0]
        PARITY_STATS["tolerated_swaps"] += len(bad)
        for p in bad:
            gap = abs(s64[got_idx[p]] - s64[o_idx[p]])
            scale = max(1.0, abs(s64[o_idx[p]])) if rtol else 1.0
            assert gap <= 4e-7 * scale * max(1, rows.shape[1] // 64), (
                f"rank {p}: gpu row {got_idx[p]} vs oracle row {o_idx[p]} differ by {gap} in fp64")
        assert sorted(got_idx.tolist()) == sorted(o_idx.tolist()) or len(bad) <= 2


# --------------------------------------------------------------------------- #
# generator + normalisation on the device
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("d", [4, 7, 384, 1000])
def test_device_generator_bit_exact(native, d):
    with native.NativeIndex(d, capacity_rows=300) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 12345, 257, normalize=False)
        got = ix.get_rows(0, 257)
    np.testing.assert_array_equal(got, O.synth_rows(O.SEED_CORPUS, 12345, 257, d))


@pytest.mark.parametrize("d", [4, 7, 384])
def test_device_normalize_matches_reference_normalize(native, d):
    raw = O.synth_rows(O.SEED_CORPUS, 0, 200, d)
    raw[17] = 0.0  # zero row stays zero (indexing.py:853-856)
    with native.NativeIndex(d) as ix:
        ix.add(raw, normalize=True)
        got = ix.get_rows(0, 200)
    with np.errstate(all="ignore"):
        exp = O.normalize_rows(raw)
    np.testing.assert_allclose(got, exp, rtol=1e-6, atol=1e-30)
    assert np.all(got[17] == 0)


def test_add_get_roundtrip_and_growth(native):
    rows = _rows(1, 5000, 20, normalize=False)
    with native.NativeIndex(20, capacity_rows=16) as ix:
        assert ix.size() == 0
        assert ix.add(rows[:100]) == 0
        assert ix.add(rows[100:100]) == 100  # empty add
        assert ix.add(rows[100:]) == 100     # forces several re-allocations
        assert ix.size() == 5000 and ix.capacity() >= 5000
        np.testing.assert_array_equal(ix.get_rows(0, 5000), rows)
        ix.set_rows(42, np.zeros((1, 20), np.float32))
        assert np.all(ix.get_rows(42, 1) == 0)
        ix.clear()
        assert ix.size() == 0


# --------------------------------------------------------------------------- #
# search parity on seeded inputs
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n,d,k", [
    (1, 4, 1), (1, 4, 5), (7, 4, 10), (63, 8, 10), (64, 8, 64), (65, 16, 65), (1000, 7, 10),
    (1000, 384, 10), (1000, 384, 100), (4096, 768, 10), (10_000, 384, 10), (10_000, 384, 1000),
    (3333, 1000, 17), (5000, 128, 2048), (20_000, 96, 1), (2500, 1536, 10), (999, 3072, 10),
    (777, 4096, 5), (300, 20, 300), (5000, 100, 10), (4000, 200, 33), (3000, 300, 10), (2000, 50, 10),
    (1500, 2000, 10), (6000, 68, 70), (900, 3000, 250),
])
def test_cosine_search_matches_oracle(native, n, d, k):
    rows = _rows(O.SEED_CORPUS, n, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 3, d))
    with native.NativeIndex(d) as ix:
        ix.add(rows)
        for q in queries:
            idx, score = ix.search(q, k)
            _check(idx[0], score[0], rows, q, k)


def test_config_c1_shape_10k_384_top10(native):
    """BASELINE configs[0]: 10k x 384, cosine, top-10, one shard -- 64 pre-screened queries, ids EXACTLY the oracle's, in one
    call and one query per call (the reference's call shape, indexing.py:983-1030)."""
    n, d, k = 10_000, 384, 10
    _, queries = _strict_queries("c1", 64, d)
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        exp = O.slab_search_screened(ix.get_rows, n, queries, k, O.METRIC_COSINE, slab=n)
        idx, score = ix.search(queries, k)  # batch entry point
        _assert_strict(idx, score, exp)
        idx1, score1 = _single_calls(ix, queries, k)
        _assert_strict(idx1, score1, exp)


def test_query_normalised_on_device(native):
    rows = _rows(O.SEED_CORPUS, 2000, 384)
    q = O.synth_rows(O.SEED_QUERY, 5, 1, 384)[0] * 7.5
    with native.NativeIndex(384) as ix:
        ix.add(rows)
        idx, score = ix.search(q, 10, normalize_queries=True)
    _check(idx[0], score[0], rows, O.normalize_vector(q), 10)


def test_exact_ties_are_ordered_by_row(native):
    d, n = 16, 1000
    rows = np.zeros((n, d), np.float32)
    rows[np.arange(n), np.arange(n) % d] = 1.0  # exactly representable one-hot rows
    q = np.zeros(d, np.float32)
    q[3] = 1.0
    with native.NativeIndex(d) as ix:
        ix.add(rows)
        idx, score = ix.search(q, 100)
    hit = np.arange(3, n, d)  # 63 rows score exactly 1.0, the rest exactly 0.0
    assert idx[0, :len(hit)].tolist() == hit.tolist()
    rest = [r for r in range(n) if r % d != 3][: 100 - len(hit)]
    assert idx[0, len(hit):].tolist() == rest
    assert np.all(score[0, :len(hit)] == 1.0) and np.all(score[0, len(hit):] == 0.0)


def test_duplicate_rows_far_apart_keep_row_order(native):
    rows = _rows(O.SEED_CORPUS, 50_000, 384)
    rows[40_000] = rows[123]
    rows[7] = rows[123]
    q = rows[123].copy()
    with native.NativeIndex(384) as ix:
        ix.add(rows)
        idx, score = ix.search(q, 5)
    assert idx[0, :3].tolist() == [7, 123, 40_000]
    assert score[0, 0] == score[0, 1] == score[0, 2]


def test_k_larger_than_n_pads_with_minus_one(native):
    rows = _rows(3, 5, 8)
    with native.NativeIndex(8) as ix:
        ix.add(rows)
        idx, score = ix.search(rows[0], 12)
    assert sorted(idx[0, :5].tolist()) == [0, 1, 2, 3, 4] and np.all(idx[0, 5:] == -1)
    assert idx[0, 0] == 0


def test_empty_index_returns_nothing(native):
    with native.NativeIndex(8) as ix:
        idx, score = ix.search(np.ones(8, np.float32), 4)
    assert np.all(idx == -1)


def test_nan_rows_are_never_returned(native):
    rows = _rows(5, 100, 8)
    rows[10, 3] = np.nan
    rows[50, :] = np.nan
    with native.NativeIndex(8) as ix:
        ix.add(rows)
        idx, _ = ix.search(rows[0], 100)
    got = idx[0][idx[0] >= 0].tolist()
    assert 10 not in got and 50 not in got and len(got) == 98


def test_negative_scores_and_zero_rows(native):
    rows = _rows(9, 300, 32)
    rows[5] = 0.0
    q = -rows[17]
    with native.NativeIndex(32) as ix:
        ix.add(rows)
        idx, score = ix.search(q, 300)
    _check(idx[0], score[0], rows, q, 300)
    assert idx[0, -1] == 17 and score[0, -1] < -0.99


@pytest.mark.parametrize("n,d,k", [(1000, 16, 10), (5000, 768, 100), (2000, 7, 25), (3000, 64, 700)])
def test_l2_extension_matches_oracle(native, n, d, k):
    rows = _rows(O.SEED_CORPUS, n, d, normalize=False)
    q = O.synth_rows(O.SEED_QUERY, 0, 1, d)[0]
    with native.NativeIndex(d, metric=native.METRIC_L2) as ix:
        ix.add(rows)
        idx, dist = ix.search(q, k)
    _check(idx[0], dist[0], rows, q, k, metric=O.METRIC_L2, rtol=1e-5)
    assert np.all(np.diff(dist[0]) >= 0)


@pytest.mark.parametrize("opts", [
    {"scan_lanes": 8}, {"scan_lanes": 16}, {"scan_lanes": 32}, {"scan_lanes": 64}, {"scan_generic": 1},
    {"scan_blocked": 1}, {"scan_nt": 1}, {"scan_blocks": 1}, {"scan_blocks": 3}, {"scan_blocks": 2048},
    {"scan_lanes": 32, "scan_blocked": 1, "scan_nt": 1}, {"lds_lists": 1}, {"lds_lists": 1, "scan_generic": 1},
    {"select_min_k": 1}, {"select_min_k": 1, "scan_generic": 1, "scan_blocked": 1}, {"zero_copy": 0},
])
def test_every_kernel_variant_gives_the_same_answer(native, opts):
    rows = _rows(O.SEED_CORPUS, 30_011, 384)
    q = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 1, 384))[0]
    with native.NativeIndex(384) as ix:
        ix.add(rows)
        base_idx, base_score = ix.search(q, 50)
        for name, v in opts.items():
            ix.set_option(name, v)
        idx, score = ix.search(q, 50)
    _check(idx[0], score[0], rows, q, 50)
    assert np.array_equal(idx, base_idx)
    np.testing.assert_allclose(score, base_score, atol=2e-6)


def test_result_independent_of_grid_size_bitwise(native):
    """The total order on keys makes the answer independent of how waves split the rows."""
    rows = _rows(O.SEED_CORPUS, 70_000, 128)
    q = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 3, 1, 128))[0]
    outs = []
    with native.NativeIndex(128) as ix:
        ix.add(rows)
        for blocks in (1, 7, 256, 1024):
            ix.set_option("scan_blocks", blocks)
            outs.append(ix.search(q, 200))
    for idx, score in outs[1:]:
        assert np.array_equal(idx, outs[0][0]) and np.array_equal(score, outs[0][1])


def test_device_resident_path_matches_host_path(native):
    rows = _rows(O.SEED_CORPUS, 20_000, 384)
    with native.NativeIndex(384) as ix:
        ix.add(rows)
        ix.set_option("gemm_min_work", 0)  # (40 queries x 20 k rows would take the blocking call to the tiles: both on the scan here)
        nq, k = 40, 10
        dq = ix.device_queries_synthetic(O.SEED_QUERY, 0, nq, normalize=True)
        q_host = dq.download(np.float32, (nq, ix.pitch))[:, :384]
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        ix.profile(True)
        ix.search_device(dq, nq, k, d_idx, d_score)
        ix.synchronize()
        prof = ix.profile_read()
        idx = d_idx.download(np.int64, (nq, k))
        score = d_score.download(np.float32, (nq, k))
        h_idx, h_score = ix.search(q_host, k)
    assert prof["scan_launches"] == nq and prof["scan_ms"] > 0 and prof["merge_launches"] >= 1
    assert np.array_equal(idx, h_idx) and np.array_equal(score, h_score)
    for i in range(nq):
        _check(idx[i], score[i], rows, q_host[i], k)


@pytest.mark.parametrize("n,d,k,metric", [
    (10_000, 384, 10, "cosine"),      # 512 partial lists of the fp32 scan: 5120 keys, 5 per thread
    (1_500, 128, 16, "cosine"),       # the largest k of the register path
    (1_500, 128, 17, "cosine"),       # the smallest k of the medium-k form (threshold by bitwise search, LDS sort of the keys above it)
    (300_000, 384, 100, "cosine"),    # the medium-k form on ~1 000 re-scored candidates (config 3's k)
    (300_000, 128, 128, "l2"),
    (2_000, 64, 180, "cosine"),       # 8 lists x 180 keys; the largest k below the radix select
    (20_000, 96, 100, "cosine"),      # more keys than the registers hold (512 lists x 100): the list walk, both options
    (700, 64, 1, "l2"),
    (37, 384, 10, "cosine"),          # fewer rows than lists, k > rows in some of them
    (300_000, 384, 10, "cosine"),     # u8 selection: the re-scored candidates (lists of one key) are what is merged
    (300_000, 128, 10, "l2"),
])
def test_register_merge_gives_the_same_keys_as_the_list_walk(native, n, d, k, metric):
    """merge_kernel's register paths (all keys loaded at once; k <= 16: k rounds of wave-wide maximum; k <= 512: threshold +
    LDS sort; option merge_fast, default on) against its list walk on the same inputs: identical ids AND scores, through the device-resident entry point (whose final
    ranking is always the merge kernel) -- and against the oracle."""
    met = O.METRIC_L2 if metric == "l2" else O.METRIC_COSINE
    rows = _rows(O.SEED_CORPUS + 3, n, d, normalize=(metric == "cosine"))
    nq = 12
    with native.NativeIndex(d, metric=native.METRIC_L2 if metric == "l2" else native.METRIC_COSINE) as ix:
        ix.add(rows)
        dq = ix.device_queries_synthetic(O.SEED_QUERY, 5, nq, normalize=True)
        q_host = dq.download(np.float32, (nq, ix.pitch))[:, :d]
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        out = {}
        for fast in (1, 0):
            ix.set_option("merge_fast", fast)
            for i in range(nq):                       # lone queries: one chain of launches each
                ix.search_device(dq, 1, k, d_idx, d_score, query_offset=i)
            ix.synchronize()
            lone = (d_idx.download(np.int64, (nq, k))[:1].copy(), d_score.download(np.float32, (nq, k))[:1].copy())
            ix.search_device(dq, nq, k, d_idx, d_score)   # and as one call of several queries
            ix.synchronize()
            out[fast] = (d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k)), lone)
    assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1])
    assert np.array_equal(out[1][2][0], out[0][2][0]) and np.array_equal(out[1][2][1], out[0][2][1])
    for i in range(nq):
        _check(out[1][0][i], out[1][1][i], rows, q_host[i], k, metric=met, rtol=1e-5 if metric == "l2" else 0.0)


@pytest.mark.parametrize("n,d,k,metric", [(10_000, 384, 10, "cosine"), (7, 64, 10, "cosine"), (250_000, 384, 10, "cosine"),
                                          (250_000, 128, 100, "l2"), (40_000, 768, 3, "l2")])
def test_lone_blocking_call_learns_of_completion_from_its_slot(native, n, d, k, metric):
    """A lone blocking search through a staging slot: the chain's last kernel writes a sequence number into the slot behind
    its results and the caller polls that word (option poll_done, default on) instead of waiting on its event.  Same answers
    as the event wait, call after call (sequence numbers never repeat within a slot), also from several threads at once and
    next to masked calls (which keep the event wait)."""
    import threading

    met = native.METRIC_L2 if metric == "l2" else native.METRIC_COSINE
    rows = _rows(O.SEED_CORPUS + 21, n, d, normalize=(metric == "cosine"))
    qs = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 40, 48, d))
    mask = native.pack_row_mask(np.arange(n) % 2 == 0)
    with native.NativeIndex(d, metric=met) as ix:
        ix.add(rows)
        out = {}
        for poll in (1, 0):
            ix.set_option("poll_done", poll)
            out[poll] = [ix.search(q, k) for q in qs]
        ix.set_option("poll_done", 1)
        masked = [ix.search(q, k, mask_words=mask) for q in qs[:4]]
        got = [None] * len(qs)

        def worker(t):
            for i in range(t, len(qs), 6):
                got[i] = ix.search(qs[i], k)

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    for i in range(len(qs)):
        assert np.array_equal(out[1][i][0], out[0][i][0]) and np.array_equal(out[1][i][1], out[0][i][1])
        assert np.array_equal(got[i][0], out[0][i][0]) and np.array_equal(got[i][1], out[0][i][1])
        _check(out[1][i][0][0], out[1][i][1][0], rows, qs[i], k, metric=O.METRIC_L2 if metric == "l2" else O.METRIC_COSINE,
               rtol=1e-5 if metric == "l2" else 0.0)
    for m_idx, _ in masked:
        assert all(r % 2 == 0 for r in m_idx[0].tolist() if r >= 0)


def test_single_rank_rccl_group_equals_local_search(native):
    """The sharded entry point with a 1-rank RCCL communicator: all-gather + second merge must be
    the identity, with global row numbers = local + base."""
    rows = _rows(O.SEED_CORPUS, 9000, 384)
    with native.NativeIndex(384) as ix:
        ix.add(rows)
        uid = native.NativeIndex.comm_unique_id()
        ix.comm_init(1, 0, uid, global_row_base=1_000_000)
        nq, k = 5, 10
        dq = ix.device_queries_synthetic(O.SEED_QUERY, 0, nq, normalize=True)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        ix.search_device(dq, nq, k, d_idx, d_score, sharded=True)
        ix.synchronize()
        g_idx, g_score = d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))
        ix.search_device(dq, nq, k, d_idx, d_score, sharded=False)
        ix.synchronize()
        l_idx, l_score = d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))
        ix.comm_destroy()
    assert np.array_equal(g_idx, l_idx + 1_000_000) and np.array_equal(g_score, l_score)


def test_two_half_shards_merge_to_the_single_shard_answer(native):
    """Contiguous row ranges: per-shard top-k + merge == single-shard top-k."""
    rows = _rows(O.SEED_CORPUS, 40_000, 384)
    q = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 1, 1, 384))[0]
    k = 20
    with native.NativeIndex(384) as whole, native.NativeIndex(384) as lo, native.NativeIndex(384) as hi:
        whole.add(rows)
        lo.add(rows[:25_000])
        hi.add(rows[25_000:])
        w_idx, w_score = whole.search(q, k)
        a_idx, a_score = lo.search(q, k)
        b_idx, b_score = hi.search(q, k)
    cand = [(float(s), int(i)) for i, s in zip(a_idx[0], a_score[0])] + \
           [(float(s), int(i) + 25_000) for i, s in zip(b_idx[0], b_score[0])]
    cand.sort(key=lambda t: (-t[0], t[1]))
    assert [c[1] for c in cand[:k]] == w_idx[0].tolist()
    assert [np.float32(c[0]) for c in cand[:k]] == w_score[0].tolist()


def test_invalid_arguments_are_reported_not_crashed(native):
    with native.NativeIndex(8) as ix:
        ix.add(_rows(1, 10, 8))
        with pytest.raises(native.HipBackendError):
            ix.search(np.ones(8, np.float32), 0)
        with pytest.raises(native.HipBackendError):
            ix.search(np.ones(8, np.float32), native.MAX_K + 1)
        with pytest.raises(native.HipBackendError):
            ix.get_rows(5, 10)
        with pytest.raises(native.HipBackendError):
            ix.set_option("no_such_option", 1)
        with pytest.raises(ValueError):
            ix.search(np.ones(9, np.float32), 1)
    with pytest.raises(native.HipBackendError):
        native.NativeIndex(8, device_id=99)
    with pytest.raises(native.HipBackendError):
        native.NativeIndex(0)


# --------------------------------------------------------------------------- #
# BASELINE sizes: full comparison where the oracle finishes in seconds, and
# size-independent properties at the largest sizes
# --------------------------------------------------------------------------- #
def _single_calls(ix, queries, k):
    """One query per call: the default single-query path (never the batched tiles)."""
    out = [ix.search(q, k) for q in queries]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def _assert_u8_selection_ran(ix, n_queries):
    """The calls since the last profile read ran on scan8_kernel (u8 selection scan + exact fp32 re-scoring):
    one full-pass launch per query, no fp32 scan launch (repairs are conditional and untimed)."""
    assert ix.get_option("last_single_path") == 2
    assert ix.profile_read()["scan_launches"] == 0
    assert ix.profile_read_gemm()["gemm_launches"] == n_queries


def test_two_coalesced_queries_share_one_pass_on_a_large_shard(native):
    """From 3 M rows a call with 2 or 3 queries (two coalesced callers) already runs as ONE pass on the i8 tiles (0.71 ms
    against 2 x 0.60 ms at 10 M x 384); smaller shards and raised `gemm_min_queries` keep the per-query scans.  Ids and
    scores against the slab-streamed oracle either way."""
    n, d, k = 3_200_000, 128, 10
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 3, d))
        expect = O.slab_search(lambda r0, c: ix.get_rows(r0, c), n, queries, k, O.METRIC_COSINE, 1 << 20)
        ix.profile(True)
        for nq in (2, 3):
            ix.profile_read(), ix.profile_read_gemm()
            idx, score = ix.search(queries[:nq], k)
            assert ix.get_option("last_gemm_family") == 3 and ix.profile_read_gemm()["gemm_launches"] == 2   # sample + full pass
            assert ix.batch_status(nq)["overflowed"] == 0
            for i in range(nq):
                assert idx[i].tolist() == expect[i][0].tolist()
                np.testing.assert_allclose(score[i], expect[i][1], atol=1e-5, rtol=0)
        ix.set_option("gemm_min_queries", 5)          # raised: batching from 5 queries, per-query selection scans below
        ix.profile_read(), ix.profile_read_gemm()
        idx, score = ix.search(queries, k)
        assert ix.get_option("last_single_path") == 2 and ix.profile_read_gemm()["gemm_launches"] == 3
        for i in range(3):
            assert idx[i].tolist() == expect[i][0].tolist()


def test_config_c2_1m_384_top10_full_oracle(native):
    n, d, k = 1_000_000, 384, 10
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        rows = ix.get_rows(0, n)  # the exact bytes the kernel scans
        # generator spot checks against the numpy restatement
        for r0 in (0, 499_000, n - 1000):
            np.testing.assert_allclose(rows[r0:r0 + 1000], O.normalize_rows_fast(O.synth_rows(O.SEED_CORPUS, r0, 1000, d)),
                                       rtol=1e-6, atol=1e-30)
        _, queries = _strict_queries("c2", 8, d)  # pre-screened: ids asserted exactly
        exp = O.slab_search_screened(lambda r0, c: rows[r0:r0 + c], n, queries, k, O.METRIC_COSINE, slab=n)
        idx, score = ix.search(queries, k)  # one call, 8 queries: the batched tiles
        _assert_strict(idx, score, exp)
        # the same queries one per call: the default single-query path (u8 selection scan), BASELINE configs[1]
        ix.profile(True)
        ix.profile_read(), ix.profile_read_gemm()
        idx1, score1 = _single_calls(ix, queries, k)
        _assert_u8_selection_ran(ix, len(queries))
        ix.profile(False)
        _assert_strict(idx1, score1, exp)
        assert np.array_equal(idx1, idx)
        # self match: a stored row finds itself first with score ~1
        idx, score = ix.search(rows[777_777], k)
        assert idx[0, 0] == 777_777 and abs(score[0, 0] - 1.0) < 1e-5


def test_config_t_10m_384_top10_single_queries_vs_oracle(native):
    """North-star shape 10M x 384 cosine top-10 on the path bench.py times: ONE QUERY PER CALL, so every query
    makes its own u8 selection scan (scan8_kernel) + exact fp32 re-scoring.  Oracle: exact fp32 scores of the
    bytes read back from HBM, slab by slab, ranked with the oracle's total order."""
    n, d, k = 10_000_000, 384, 10
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        _, queries = _strict_queries("t", 12, d)  # pre-screened offsets: ids asserted exactly
        ix.profile(True)
        ix.profile_read(), ix.profile_read_gemm()
        idx, score = _single_calls(ix, queries, k)
        _assert_u8_selection_ran(ix, len(queries))
        assert np.all(np.diff(score, axis=1) <= 0) and np.all(idx >= 0) and np.all(idx < n)
        exp = O.slab_search_screened(ix.get_rows, n, queries, k, O.METRIC_COSINE, slab=1_000_000)
        _assert_strict(idx, score, exp)
        # the device-resident entry point bench.py drives (pipelined, conditional repair launches queued)
        dq = ix.device_queries(queries)
        d_idx, d_score = ix.alloc(len(queries) * k * 8), ix.alloc(len(queries) * k * 4)
        ix.search_device(dq, len(queries), k, d_idx, d_score)
        ix.synchronize()
        _assert_u8_selection_ran(ix, len(queries))
        assert np.array_equal(d_idx.download(np.int64, (len(queries), k)), idx)
        assert np.array_equal(d_score.download(np.float32, (len(queries), k)), score)
        # one call with all queries: the batched tiles must give the same answer
        bidx, bscore = ix.search(queries, k)
        assert np.array_equal(bidx, idx) and np.allclose(bscore, score, atol=1e-6, rtol=0)
        # k = 100, single query (an offset pre-screened at k = 100), against the oracle too
        _, q100 = _strict_queries("t_k100", 1, d)
        ix.profile_read(), ix.profile_read_gemm()
        idx100, score100 = ix.search(q100[0], 100)
        _assert_u8_selection_ran(ix, 1)
        _assert_strict(idx100, score100, O.slab_search_screened(ix.get_rows, n, q100, 100, O.METRIC_COSINE, slab=1_000_000),
                       config="t_k100")


def test_config_c4_10m_384_one_call_of_256_queries_vs_oracle(native):
    """BASELINE configs[3] at its OWN size: 10M x 384 fp32, cosine, top-10, ONE call carrying 256 queries -- the 256-wide
    int8 tile instance bench.py's c4 leg times (gemm_i8_kernel<., 8, 3, 384>: sample pass + full pass = 2 tile launches),
    through the device entry point (no host-side repair: no query may overflow) and through the blocking one.  Oracle: one
    sgemm per 1 M-row slab over the rows read back from HBM, per query the reference's ranking (indexing.py:983-1030)."""
    n, d, nq, k = 10_000_000, 384, 256, 10
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        _, queries = _strict_queries("c4", nq, d)  # 256 pre-screened offsets: ids asserted exactly
        dq = ix.device_queries(queries)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        ix.search_batch_device(dq, nq, k, d_idx, d_score)  # (builds the i8 shadow)
        ix.synchronize()
        ix.profile(True)
        ix.profile_read_gemm()
        ix.search_batch_device(dq, nq, k, d_idx, d_score)
        ix.synchronize()
        assert ix.get_option("last_gemm_family") == 3 and ix.get_option("shadowg_rows") == n
        assert ix.profile_read_gemm()["gemm_launches"] == 2
        st = ix.batch_status(nq)
        assert st["overflowed"] == 0 and int(st["counts"].max()) <= st["capacity"]
        idx, score = d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))
        assert np.all(np.diff(score, axis=1) <= 0) and np.all(idx >= 0) and np.all(idx < n)
        exp = O.slab_search_screened(ix.get_rows, n, queries, k, O.METRIC_COSINE, slab=1_000_000)
        _assert_strict(idx, score, exp)
        # the blocking entry point picks the same pass by itself and returns the same bytes
        bidx, bscore = ix.search(queries, k)
        assert ix.get_option("last_gemm_family") == 3
        assert np.array_equal(bidx, idx) and np.array_equal(bscore, score)


def test_config_c3_full_10m_768_l2_top100_vs_oracle(native):
    """BASELINE configs[2] at its FULL size: 10M x 768 fp32, L2, top-100, single-query calls (u8 selection scan),
    against the oracle's direct-form distances over the 30 GB read back from HBM in slabs.  Unit-norm rows so
    the absolute tolerance is meaningful."""
    n, d, k = 10_000_000, 768, 100
    with native.NativeIndex(d, metric=native.METRIC_L2, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        _, queries = _strict_queries("c3", 2, d)  # pre-screened at k = 100: ids asserted exactly
        ix.profile(True)
        ix.profile_read(), ix.profile_read_gemm()
        idx, dist = _single_calls(ix, queries, k)
        _assert_u8_selection_ran(ix, len(queries))
        assert np.all(np.diff(dist, axis=1) >= 0) and np.all(idx >= 0) and np.all(idx < n)
        exp = O.slab_search_screened(ix.get_rows, n, queries, k, O.METRIC_L2, slab=250_000)
        _assert_strict(idx, dist, exp, rtol=1e-5, config="c3")


def test_config_c3_shape_l2_top100_768(native):
    """BASELINE config 3 shape (L2, top-100, d=768) at 2M rows against the oracle, unit-norm rows so
    the absolute tolerance is meaningful."""
    n, d, k = 2_000_000, 768, 100
    with native.NativeIndex(d, metric=native.METRIC_L2, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        q = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 1, d))[0]
        idx, dist = ix.search(q, k)
        best = []
        slab = 500_000
        for r0 in range(0, n, slab):
            rows = ix.get_rows(r0, slab)
            s = O.flat_scores(rows, q, O.METRIC_L2)
            top = O._topk_desc(-s, k)
            best += [(float(s[t]), int(t) + r0) for t in top]
        exp = sorted(best, key=lambda t: (t[0], t[1]))[:k]
        np.testing.assert_allclose(dist[0], [e[0] for e in exp], atol=ATOL, rtol=1e-5)
        _ids_match(idx[0], dist[0], [e[1] for e in exp], [e[0] for e in exp])


# --------------------------------------------------------------------------- #
# batched queries on the fp32 MFMA path (BASELINE config 4 shape; extension)
# --------------------------------------------------------------------------- #
def _oracle_batch(rows, queries, k):
    s = rows @ queries.T  # fp32 sgemm
    out = []
    for qi in range(queries.shape[0]):
        top = O._topk_desc(s[:, qi], k)
        out.append((top, s[top, qi]))
    return out


# tile families: 3 = i8 tiles over the group-scaled i8 shadow (default), 2 = bf16 tiles over the bf16 shadow, 1 = bf16 tiles on
# the fp32 rows, 0 = exact fp32 tiles
@pytest.mark.parametrize("family", [3, 2, 1, 0])
@pytest.mark.parametrize("n,d,nq,k", [(200_000, 384, 256, 10), (100_003, 384, 100, 10), (70_001, 100, 40, 50),
                                      (300_000, 128, 513, 5), (90_000, 768, 130, 10), (66_000, 1000, 70, 3)])
def test_batched_mfma_path_matches_oracle(native, n, d, nq, k, family):
    with native.NativeIndex(d, capacity_rows=n) as ix:
        assert ix.get_option("gemm_bf16") == 3
        ix.set_option("gemm_bf16", family)
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        rows = ix.get_rows(0, n)
        dq = ix.device_queries_synthetic(O.SEED_QUERY, 0, nq, normalize=True)
        queries = dq.download(np.float32, (nq, ix.pitch))[:, :d]
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        ix.profile(True)
        ix.search_batch_device(dq, nq, k, d_idx, d_score)
        st = ix.batch_status(nq)
        g = ix.profile_read_gemm()
        idx, score = d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))
        assert ix.get_option("last_gemm_family") == family
        assert ix.get_option("shadow_rows") == (n if family == 2 else 0)
        assert ix.get_option("shadowg_rows") == (n if family == 3 else 0)
    block = 256 if (family != 3 or d <= 384) else 128 if d <= 768 else 64   # the i8 tiles keep the query block in LDS
    assert st["overflowed"] == 0 and g["gemm_launches"] == 2 * ((nq + block - 1) // block)
    assert np.all(st["counts"] >= k) and st["counts"].max() <= st["capacity"]
    exp = _oracle_batch(rows, queries, k)
    for qi in range(nq):
        np.testing.assert_allclose(score[qi], exp[qi][1], atol=ATOL, rtol=0)
        _ids_match(idx[qi], score[qi], exp[qi][0], exp[qi][1])


def test_blocking_search_picks_the_batched_path_and_agrees_with_scans(native):
    n, d, nq, k = 150_000, 384, 64, 10
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, nq, d))
        ix.profile(True)
        b_idx, b_score = ix.search(queries, k)
        assert ix.profile_read_gemm()["gemm_launches"] == 2 and ix.profile_read()["scan_launches"] == 0
        ix.set_option("gemm_min_queries", 1 << 30)
        ix.profile_read_gemm()
        p_idx, p_score = ix.search(queries, k)              # one shadow selection scan per query
        assert ix.profile_read_gemm()["gemm_launches"] == nq and ix.profile_read()["scan_launches"] == 0
        ix.set_option("scan_shadow", 0)
        s_idx, s_score = ix.search(queries, k)              # fp32 scans
        assert ix.profile_read()["scan_launches"] == nq
    np.testing.assert_allclose(b_score, s_score, atol=2e-6, rtol=0)
    assert np.array_equal(p_idx, b_idx) and np.array_equal(p_score, b_score)  # same re-scoring arithmetic
    for qi in range(nq):
        _ids_match(b_idx[qi], b_score[qi], s_idx[qi], s_score[qi])


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_small_corpus_batches_choose_their_path_by_work_and_agree_with_the_oracle(native, metric):
    """Below gemm_min_rows a blocking batch goes to the matrix cores from queries x rows >= gemm_min_work (the tiles cost their
    launches whatever they hold) and to the fp32 scan -- a round of queries as ONE grid -- below it.  Same ids as the oracle
    on both, and the two paths agree with each other; rounds of 1 .. 33 queries through the one-grid scan, with a row mask,
    equal a launch per query bit for bit."""
    n, d, k = 30_000, 128, 10
    met = native.METRIC_L2 if metric == "l2" else native.METRIC_COSINE
    omet = O.METRIC_L2 if metric == "l2" else O.METRIC_COSINE
    rows = _rows(O.SEED_CORPUS + 33, n, d, normalize=(metric == "cosine"))
    qs = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 70, 64, d))
    mask = native.pack_row_mask(np.arange(n) % 3 != 1)
    with native.NativeIndex(d, metric=met) as ix:
        ix.add(rows)
        ix.profile(True)
        ix.profile_read_gemm(), ix.profile_read()
        big = ix.search(qs, k)                                  # 64 x 30 000 = 1.92 M >= 800 k: tiles
        g = ix.profile_read_gemm()
        assert g["gemm_launches"] == 2 and ix.profile_read()["scan_launches"] == 0
        small = ix.search(qs[:8], k)                            # 8 x 30 000 = 240 k: the scan, one grid for the round
        assert ix.profile_read_gemm()["gemm_launches"] == 0 and ix.profile_read()["scan_launches"] == 8
        ix.set_option("gemm_min_work", 0)
        scan64 = ix.search(qs, k)                               # all 64 on the scan: two rounds of 32
        per = {}
        for og in (1, 0):
            ix.set_option("scan_one_grid", og)
            per[og] = [ix.search(qs[:b], k) for b in (1, 2, 31, 32, 33)] + [ix.search(qs[:5], k, mask_words=mask)]
    for a, b in zip(per[1], per[0]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(big[0], scan64[0])
    np.testing.assert_allclose(big[1], scan64[1], rtol=2e-6, atol=2e-6)
    assert np.array_equal(small[0], scan64[0][:8]) and np.array_equal(small[1], scan64[1][:8])
    for i in range(64):
        _check(big[0][i], big[1][i], rows, qs[i], k, metric=omet, rtol=1e-5 if metric == "l2" else 0.0)
    assert all(r % 3 != 1 for r in per[1][-1][0].ravel().tolist() if r >= 0)


def test_batched_path_candidate_overflow_is_repaired_exactly(native):
    """Half of the corpus equals query 3: every such row passes its threshold, the candidate buffer
    overflows, and the blocking entry point must fall back to the exact scan for that query."""
    n, d, nq, k = 120_000, 64, 32, 10
    rows = _rows(O.SEED_CORPUS, n, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, nq, d))
    rows[1::2] = queries[3]
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.add(rows)
        idx, score = ix.search(queries, k)
        st = ix.batch_status(nq)
    assert st["overflowed"] >= 1 and st["counts"][3] > st["capacity"]
    assert idx[3].tolist() == list(range(1, 2 * k, 2))  # exact ties -> ascending rows
    assert np.all(score[3] == score[3][0]) and abs(score[3][0] - 1.0) < 1e-6
    for qi in range(nq):
        if qi != 3:  # (the BLAS oracle does not give bit-equal scores to equal rows, so no id check there)
            _check(idx[qi], score[qi], rows, queries[qi], k)


def test_batched_device_entry_point_repairs_overflow_on_the_device(native):
    """The asynchronous batched entry point (no host in the loop): a query whose candidate buffer overflows -- half the
    corpus equals it -- is re-run exactly by the conditional repair launches queued behind its block; every other query
    pays a 4-us empty launch.  Both tile families that select (i8, bf16), cosine and L2."""
    n, d, nq, k = 140_000, 128, 70, 10
    rows = _rows(O.SEED_CORPUS, n, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, nq, d))
    rows[1::2] = queries[3]
    for metric in (native.METRIC_COSINE, native.METRIC_L2):
        for family in (3, 2):
            with native.NativeIndex(d, metric=metric, capacity_rows=n) as ix:
                ix.set_option("gemm_bf16", family)
                ix.add(rows)
                dq = ix.device_queries(queries)
                d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
                ix.search_batch_device(dq, nq, k, d_idx, d_score)
                ix.synchronize()
                st = ix.batch_status(nq)
                assert ix.get_option("last_gemm_family") == family and ix.get_option("last_batch_repaired") == 1
                assert st["overflowed"] >= 1 and st["counts"][3] > st["capacity"]
                idx, score = d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))
                ix.set_option("gemm_min_queries", 1 << 30)
                ix.set_option("scan_shadow", 0)
                r_idx, r_score = ix.search(queries, k)          # fp32 scans
            assert idx[3].tolist() == list(range(1, 2 * k, 2)) and np.array_equal(idx[3], r_idx[3]) and np.array_equal(score[3], r_score[3])
            for qi in range(nq):
                np.testing.assert_allclose(score[qi], r_score[qi], atol=2e-6, rtol=2e-6)
                _ids_match(idx[qi], score[qi], r_idx[qi], r_score[qi])


def test_masked_search_is_exact_topk_of_allowed_rows(native):
    rows = _rows(O.SEED_CORPUS, 50_000, 384)
    q = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 2, 1, 384))[0]
    rng = np.random.default_rng(0)
    with native.NativeIndex(384) as ix:
        ix.add(rows)
        for frac in (0.5, 0.01, 0.0002):
            allowed = rng.random(50_000) < frac
            idx, score = ix.search(q, 10, mask_words=native.pack_row_mask(allowed))
            o_idx, o_score = O.flat_search(rows, q, 10, normalize_query=False, allowed=allowed)
            assert idx[0, : len(o_idx)].tolist() == o_idx.tolist() and np.all(idx[0, len(o_idx):] == -1)
            np.testing.assert_allclose(score[0, : len(o_idx)], o_score, atol=ATOL, rtol=0)
        none = ix.search(q, 5, mask_words=native.pack_row_mask(np.zeros(50_000, bool)))[0]
        assert np.all(none == -1)
        # a mask does not leak into the next, unmasked call
        idx, score = ix.search(q, 10)
        _check(idx[0], score[0], rows, q, 10)


def test_radix_select_path_edge_cases(native):
    """Large-k path (key per row + radix select): k > n, NaN rows, masks, exact ties, and equality with
    the list path for the same k."""
    rows = _rows(O.SEED_CORPUS, 20_000, 96)
    rows[5] = np.nan
    rows[100:200] = rows[7]  # 101 exact ties
    q = rows[7].copy()
    allowed = np.ones(20_000, bool)
    allowed[::3] = False
    with native.NativeIndex(96) as ix:
        ix.add(rows)
        for k in (300, 1000, 2048):
            idx, score = ix.search(q, k)
            ix.set_option("select_min_k", 0)          # same k through the list kernels
            l_idx, l_score = ix.search(q, k)
            ix.set_option("select_min_k", 200)
            assert np.array_equal(idx, l_idx) and np.array_equal(score, l_score)
            assert idx[0, :101].tolist() == [7] + list(range(100, 200)) and 5 not in idx[0].tolist()
        idx, score = ix.search(q, 500, mask_words=native.pack_row_mask(allowed))
        o_idx, o_score = O.flat_search(np.nan_to_num(rows, nan=0.0), q, 20_000, normalize_query=False)
        exp = [i for i in o_idx.tolist() if allowed[i] and i != 5][:500]
        assert sorted(idx[0].tolist()[:101]) == sorted(exp[:101])  # the tie block, any BLAS order
        assert idx[0].tolist()[101:] == exp[101:]
    small = _rows(3, 40, 8)
    with native.NativeIndex(8) as ix:
        ix.add(small)
        idx, score = ix.search(small[0], 400)
        assert np.all(idx[0, 40:] == -1) and sorted(idx[0, :40].tolist()) == list(range(40))
        _check(idx[0], score[0], small, small[0], 400)


@pytest.mark.parametrize("n,d,nq,k", [(150_000, 384, 256, 10), (70_001, 100, 40, 50)])
def test_batched_path_query_block_widths_agree(native, n, d, nq, k):
    """The MFMA kernel's 64-, 128- and 256-query tiles run the same fp32 FMA chain per (row, query):
    bit-identical results whichever block width serves the batch."""
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        dq = ix.device_queries_synthetic(O.SEED_QUERY, 0, nq, normalize=True)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        outs = []
        for ct in (0, 1, 2, 4):
            ix.set_option("gemm_ct", ct)
            ix.search_batch_device(dq, nq, k, d_idx, d_score)
            assert ix.batch_status(nq)["overflowed"] == 0
            outs.append((d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))))
    for o in outs[1:]:
        assert np.array_equal(outs[0][0], o[0]) and np.array_equal(outs[0][1], o[1])


@pytest.mark.parametrize("k,opts", [(25, {}), (25, {"scan_generic": 1}), (300, {}), (25, {"lds_lists": 1}),
                                    (150, {}), (150, {"select_min_k": 0}), (300, {"select_min_k": 0}), (512, {"select_min_k": 0})])
def test_massive_exact_ties_match_the_c_oracle(native, k, opts):
    """Every vector stored 10 times: the answer is decided by the tie rule (row ascending) at every
    rank.  The C oracle sums each row in one fixed order, so its ties are exact like the kernel's."""
    import c_oracle as CO

    base = _rows(O.SEED_CORPUS, 5000, 96)
    rows = np.tile(base, (10, 1))
    q = base[123].copy()
    with native.NativeIndex(96) as ix:
        ix.add(rows)
        for name, v in opts.items():
            ix.set_option(name, v)
        idx, score = ix.search(q, k)
        midx, _ = ix.search(q, k, mask_words=native.pack_row_mask(np.arange(50_000) % 3 != 0))
    o_idx, o_score = CO.flat_search(rows, q, k)
    assert idx[0].tolist() == o_idx.tolist()
    np.testing.assert_allclose(score[0], o_score, atol=ATOL, rtol=0)
    assert idx[0, :10].tolist() == list(range(123, 50_000, 5000)) and len(set(score[0, :10].tolist())) == 1
    m_idx, _ = CO.flat_search(rows, q, k, allowed=(np.arange(50_000) % 3 != 0))
    assert midx[0].tolist() == m_idx.tolist()


# ---- more keys tied at the k-th score than the medium-k merge sorts in LDS (1 024): its way out is the list walk ---------
_TIE_N, _TIE_D, _TIE_COPIES = 540_000, 96, 1500


@pytest.fixture(scope="module")
def tie_corpus():
    """540 k rows (every k below reaches the u8 selection scan, whose re-scored candidates the merge ranks) holding 1 500
    identical copies of one vector and 1 500 near-duplicates of another: base + noise small enough that all 1 500 cosine
    scores against the base lie within 2^-15 relative (in fact within 64 units of the ordered score: checked here with the
    C oracle)."""
    import c_oracle as CO

    rows = _rows(O.SEED_CORPUS, _TIE_N, _TIE_D)
    rng = np.random.default_rng(20240611)
    a, b = O.normalize_rows_fast(rng.standard_normal((2, _TIE_D)).astype(np.float32))
    where = rng.permutation(_TIE_N)[: 2 * _TIE_COPIES]
    rows[where[:_TIE_COPIES]] = a
    near = b[None, :] + rng.standard_normal((_TIE_COPIES, _TIE_D)).astype(np.float32) * np.float32(2e-5)
    rows[where[_TIE_COPIES:]] = O.normalize_rows_fast(near.astype(np.float32))
    for q, copies in ((a, where[:_TIE_COPIES]), (b, where[_TIE_COPIES:])):
        idx, score = CO.flat_search(rows, q, _TIE_COPIES)
        assert sorted(idx.tolist()) == sorted(copies.tolist())
        bits = score.view(np.uint32).astype(np.int64)  # (positive floats: their bit patterns order like the ordered score)
        assert score.min() > 0.99 and bits.max() - bits.min() < 64, (bits.max() - bits.min())
    return rows, a, b


def _assert_tied_answer(idx, score, o_idx, o_score, exact):
    assert len(set(idx.tolist())) == len(idx) and np.all(idx >= 0), "a row returned twice / missing"
    assert np.all(score[1:] <= score[:-1]), "scores not in descending order"
    np.testing.assert_allclose(score, o_score, atol=ATOL, rtol=0)
    if exact:  # identical rows: identical scores, the order is the tie rule (row ascending)
        assert idx.tolist() == o_idx.tolist()


@pytest.mark.parametrize("k,opts", [(150, {}), (300, {"select_min_k": 0}), (512, {"select_min_k": 0}), (25, {"lds_lists": 1}), (25, {})])
def test_more_than_1024_keys_tied_at_the_kth_score(native, tie_corpus, k, opts):
    import c_oracle as CO

    rows, a, b = tie_corpus
    queries = np.stack([a, b, rows[7]])
    oracle = [CO.flat_search(rows, q, k) for q in queries]
    with native.NativeIndex(_TIE_D, capacity_rows=_TIE_N) as ix:
        ix.add(rows)
        for name, v in opts.items():
            ix.set_option(name, v)
        ix.set_option("lone_host_select", 0)  # (a lone blocking query's candidates are ranked by merge_kernel, not by the host)
        got = {}
        for fast in (1, 0):
            ix.set_option("merge_fast", fast)
            lone = [ix.search(q, k) for q in queries]
            assert ix.get_option("last_single_path") == 2  # the u8 selection scan: merge_kernel ranks its re-scored candidates
            batch = ix.search(queries, k)  # one round of single-query passes, one merge launch for the three
            got[fast] = lone, batch
        for fast in (1, 0):
            lone, batch = got[fast]
            for qi, (o_idx, o_score) in enumerate(oracle):
                _assert_tied_answer(lone[qi][0][0], lone[qi][1][0], o_idx, o_score, exact=qi == 0)
                _assert_tied_answer(batch[0][qi], batch[1][qi], o_idx, o_score, exact=qi == 0)
        for qi in range(len(queries)):  # the two merges rank the same exact scores: identical, near-duplicates included
            assert np.array_equal(got[1][0][qi][0], got[0][0][qi][0]) and np.array_equal(got[1][0][qi][1], got[0][0][qi][1]), qi
        assert np.array_equal(got[1][1][0], got[0][1][0]) and np.array_equal(got[1][1][1], got[0][1][1])


def test_zero_query_ties_every_row(native):
    """Dot products with a zero query are all +0.0: the answer is rows 0 .. k - 1 by the tie rule alone."""
    rows = _rows(O.SEED_CORPUS, 200_000, 96)
    q = np.zeros(96, np.float32)
    with native.NativeIndex(96, capacity_rows=len(rows)) as ix:
        ix.add(rows)
        for opts in ({}, {"lone_host_select": 0}, {"merge_fast": 0}, {"scan_shadow": 0, "merge_fast": 1}, {"select_min_k": 0}):
            for name, v in opts.items():
                ix.set_option(name, v)
            for k in (25, 150, 300):
                idx, score = ix.search(q, k)
                assert idx[0].tolist() == list(range(k)), (opts, k)
                assert np.array_equal(score[0].view(np.uint32), np.zeros(k, np.uint32)), (opts, k)


@pytest.mark.parametrize("k_out", [200, 512])
def test_group_merge_of_shards_full_of_duplicates(native, k_out):
    """8 shards sharing the device, 190 copies of one vector in each: the 8 x 140 gathered keys of the final merge are all
    tied, more than its LDS sort holds."""
    import c_oracle as CO

    S, per, d, k = 8, 6000, 96, 140
    rows = _rows(O.SEED_CORPUS, S * per, d)
    rng = np.random.default_rng(77)
    a = O.normalize_rows_fast(rng.standard_normal((1, d)).astype(np.float32))[0]
    for s in range(S):
        rows[s * per + rng.permutation(per)[:190]] = a
    bounds = [s * per for s in range(S + 1)]
    queries = np.stack([a, rows[11]])
    expect = []
    for q in queries:  # the union of the shards' own best 140, best first
        cand = []
        for s in range(S):
            i, sc = CO.flat_search(rows[bounds[s]: bounds[s + 1]], q, k)
            cand += [(-float(x), int(r) + bounds[s]) for r, x in zip(i, sc)]
        cand.sort()
        expect.append(cand[:k_out])
    outs = []
    for fast in (1, 0):
        shards, grp = _attached_group(native, rows, bounds, d, merge_fast=fast)
        try:
            idx, score = grp.search_merged(queries, k, k_out)
            lone = grp.search_merged(queries[0], k, k_out)
        finally:
            grp.close()
            for sh in shards:
                sh.close()
        assert np.array_equal(lone[0][0], idx[0]) and np.array_equal(lone[1][0], score[0])
        assert idx[0].tolist() == [r for _, r in expect[0]], f"merge_fast={fast}: tied rows out of order or repeated"
        for qi in range(2):
            assert len(set(idx[qi].tolist())) == k_out
            np.testing.assert_allclose(score[qi], [-x for x, _ in expect[qi]], atol=ATOL, rtol=0)
        assert _ids_match(idx[1], score[1], [r for _, r in expect[1]], [-x for x, _ in expect[1]]) <= 4
        outs.append((idx, score))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_batched_path_exact_ties_match_the_c_oracle(native):
    import c_oracle as CO

    base = _rows(O.SEED_CORPUS, 20_000, 64)
    rows = np.tile(base, (4, 1))  # 80k rows, every vector 4 times
    queries = base[[5, 77, 19_999] + list(range(100, 129))].copy()
    with native.NativeIndex(64) as ix:
        ix.add(rows)
        idx, score = ix.search(queries, 12)  # 32 queries -> MFMA path
        assert ix.batch_status(32)["overflowed"] == 0
    for qi, q in enumerate(queries):
        o_idx, o_score = CO.flat_search(rows, q, 12)
        assert idx[qi].tolist() == o_idx.tolist(), qi
        np.testing.assert_allclose(score[qi], o_score, atol=ATOL, rtol=0)


def test_concurrent_searches_and_adds_from_threads(native):
    """The reference calls search from 4-worker pools per index while adds may arrive (indexing.py:692,
    :1045-1048; unguarded there).  Here the handle serialises: every answer must be exact for SOME
    prefix of the rows that were present, and nothing may crash."""
    import threading

    d = 128
    rows = _rows(O.SEED_CORPUS, 60_000, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 16, d))
    expect_full = [O.flat_search(rows, q, 10, normalize_query=False)[0].tolist() for q in queries]
    expect_half = [O.flat_search(rows[:30_000], q, 10, normalize_query=False)[0].tolist() for q in queries]
    errors = []
    with native.NativeIndex(d, capacity_rows=1000) as ix:
        ix.add(rows[:30_000])

        def searcher(tid):
            try:
                for it in range(40):
                    qi = (tid + it) % len(queries)
                    idx, _ = ix.search(queries[qi], 10)
                    got = idx[0].tolist()
                    if got != expect_half[qi] and got != expect_full[qi]:
                        # mid-ingest state: must still be a sorted, in-range answer
                        assert all(0 <= g < 60_000 for g in got)
            except Exception as e:  # pragma: no cover
                errors.append(e)

        def adder():
            try:
                for b in range(30_000, 60_000, 3000):
                    ix.add(rows[b:b + 3000])
            except Exception as e:  # pragma: no cover
                errors.append(e)

        threads = [threading.Thread(target=searcher, args=(t,)) for t in range(6)] + [threading.Thread(target=adder)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert ix.size() == 60_000
        for qi, q in enumerate(queries):
            assert ix.search(q, 10)[0][0].tolist() == expect_full[qi]


def test_in_process_group_api_single_device(native):
    """wdbx_group_*: the in-process shard group (ncclCommInitAll).  One GPU here, so one shard: the
    group call must equal the plain index (the multi-device exchange is the same all-gather + merge
    the per-rank path uses)."""
    rows = _rows(O.SEED_CORPUS, 30_000, 384)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 70, 384))
    with native.NativeGroup([0], 384, cap_per_shard=40_000) as grp:
        assert grp.add(rows[:10_000]) == 0 and grp.add(rows[10_000:]) == 10_000 and grp.size() == 30_000
        for k in (10, 100, 300):
            idx, score = grp.search(queries, k)
            for i in (0, 33, 69):
                _check(idx[i], score[i], rows, queries[i], k)
        with pytest.raises(native.HipBackendError):
            grp.add(rows[:20_000])  # over capacity
    with pytest.raises(native.HipBackendError):
        native.NativeGroup([0, 0], 8)


def test_soak_1m_rows_many_queries_both_paths(native):
    """1 M x 384, 512 queries through the batched MFMA path and 96 through single-query scans, every
    result compared with the oracle (fp32 sgemm scores, total order on (score, row))."""
    n, d, k = 1_000_000, 384, 10
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        rows = ix.get_rows(0, n)
        queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 1000, 512, d))
        b_idx, b_score = ix.search(queries, k)                 # batched path
        assert ix.batch_status(512)["overflowed"] == 0
        ix.set_option("gemm_min_queries", 1 << 30)
        s_idx, s_score = ix.search(queries[:96], k)            # scan path
    s = rows @ queries.T
    worst = 0.0
    for qi in range(512):
        top = O._topk_desc(s[:, qi], k)
        exp_score = s[top, qi]
        worst = max(worst, float(np.max(np.abs(b_score[qi] - exp_score))))
        np.testing.assert_allclose(b_score[qi], exp_score, atol=ATOL, rtol=0)
        _ids_match(b_idx[qi], b_score[qi], top, exp_score)
        if qi < 96:
            np.testing.assert_allclose(s_score[qi], exp_score, atol=ATOL, rtol=0)
            _ids_match(s_idx[qi], s_score[qi], top, exp_score)
    assert worst < 1e-6, worst


def test_sharded_batched_path_single_rank_equals_local_batch(native):
    """Batched MFMA path + RCCL exchange (1-rank communicator): identical to the local batched result with
    rows shifted by the rank's base."""
    n, d, nq, k = 120_000, 128, 150, 10
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        ix.comm_init(1, 0, native.NativeIndex.comm_unique_id(), global_row_base=7_000_000)
        dq = ix.device_queries_synthetic(O.SEED_QUERY, 0, nq, normalize=True)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        ix.search_batch_device(dq, nq, k, d_idx, d_score, sharded=True)
        assert ix.batch_status(nq)["overflowed"] == 0
        g_idx, g_score = d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))
        ix.search_batch_device(dq, nq, k, d_idx, d_score, sharded=False)
        ix.synchronize()
        l_idx, l_score = d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))
        ix.comm_destroy()
    assert np.array_equal(g_idx, l_idx + 7_000_000) and np.array_equal(g_score, l_score)


@pytest.mark.parametrize("family", [3, 2, 1, 0])
@pytest.mark.parametrize("n,d,nq,k,unit", [(150_000, 384, 128, 10, True), (100_003, 100, 40, 25, False),
                                            (200_000, 64, 300, 5, False)])
def test_batched_l2_path_matches_oracle(native, n, d, nq, k, unit, family):
    """L2 on the batched path: MFMA pass ranks by 2 c.q - |c|^2 with a rounding-error margin, the kept
    candidates are re-scored with the direct form.  Includes queries that sit almost ON stored rows
    (distance << norm: the case where the norm form cancels) and exact duplicates."""
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((n, d)).astype(np.float32) * (1.0 if unit else 3.0)
    if unit:
        rows = O.normalize_rows_fast(rows)
    queries = rng.standard_normal((nq, d)).astype(np.float32) * (1.0 if unit else 3.0)
    if unit:
        queries = O.normalize_rows_fast(queries)
    queries[0] = rows[12_345] + np.float32(1e-4) * rng.standard_normal(d).astype(np.float32)   # near-duplicate
    queries[1] = rows[99_999]                                                                    # exact hit, distance 0
    rows[[5, 70_000, 70_001]] = rows[99_999]                                                     # tie group
    with native.NativeIndex(d, metric=native.METRIC_L2, capacity_rows=n) as ix:
        ix.set_option("gemm_bf16", family)
        ix.add(rows)
        ix.profile(True)
        idx, dist = ix.search(queries, k)
        g = ix.profile_read_gemm()
        st = ix.batch_status(nq)
        fam = ix.get_option("last_gemm_family")
        ix.set_option("gemm_l2", 0)
        s_idx, s_dist = ix.search(queries[:8], k)  # the scan path on the same handle
    assert g["gemm_launches"] >= 2 and st["overflowed"] == 0
    assert fam == family or (family == 2 and fam == 1)  # (short rows: the padded bf16 copy would be no smaller than the fp32 rows)
    assert idx[1, :4].tolist() == [5, 70_000, 70_001, 99_999] and np.all(dist[1, :4] == 0.0)
    assert idx[0, 0] == 12_345 and dist[0, 0] < 1e-5
    for qi in range(nq):
        s64 = O.flat_scores_f64(rows, queries[qi], O.METRIC_L2)
        order = np.lexsort((np.arange(n), s64))[:k]
        np.testing.assert_allclose(dist[qi], s64[order], rtol=1e-5, atol=1e-5)
        if idx[qi].tolist() != order.tolist():
            for a, b in zip(idx[qi].tolist(), order.tolist()):
                assert a == b or abs(s64[a] - s64[b]) <= 1e-5 * max(1.0, s64[b]), (qi, a, b)
        if qi < 8:
            assert idx[qi].tolist() == s_idx[qi].tolist()
            np.testing.assert_allclose(dist[qi], s_dist[qi], rtol=2e-6, atol=2e-6)


# --------------------------------------------------------------------------- #
# bf16 selection tiles: the error margin, the shadow copy, the fallbacks
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("family", [3, 2, 1])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_bf16_selection_is_exact_when_scores_differ_below_bf16_resolution(native, family, metric):
    """2000 rows sit in a tight cluster around query 0 (scores within 2e-5 of each other, far below what
    bf16 products resolve, ~4e-3): the selection pass cannot rank them, so the margin has to keep all of
    them and the fp32 re-scoring decides.  The answer must equal the single-query scan's, id for id."""
    n, d, nq, k = 150_000, 128, 128, 50
    rng = np.random.default_rng(5)
    rows = O.normalize_rows_fast(rng.standard_normal((n, d)).astype(np.float32))
    queries = O.normalize_rows_fast(rng.standard_normal((nq, d)).astype(np.float32))
    cluster = rng.choice(n, 2000, replace=False)
    noise = rng.standard_normal((2000, d)).astype(np.float32)
    eps = rng.uniform(1e-3, 6e-3, (2000, 1)).astype(np.float32)
    rows[cluster] = O.normalize_rows_fast(queries[0] + eps * noise / np.sqrt(d))
    m = native.METRIC_L2 if metric == "l2" else native.METRIC_COSINE
    with native.NativeIndex(d, metric=m, capacity_rows=n) as ix:
        ix.set_option("gemm_bf16", family)
        ix.add(rows)
        b_idx, b_score = ix.search(queries, k)
        st = ix.batch_status(nq)
        # (the i8 tiles serve both metrics since round 3)
        assert ix.get_option("last_gemm_family") == family and st["overflowed"] == 0
        assert st["counts"][0] >= 2000  # the whole cluster had to be kept for query 0
        ix.set_option("gemm_min_queries", 1 << 30)
        s_idx, s_score = ix.search(queries[:16], k)  # scan path, same handle
    assert set(b_idx[0].tolist()) <= set(cluster.tolist())
    s64 = O.flat_scores_f64(rows, queries[0], O.METRIC_L2 if metric == "l2" else O.METRIC_COSINE)
    order = np.lexsort((np.arange(n), s64 if metric == "l2" else -s64))[:k]
    for a, b in zip(b_idx[0].tolist(), order.tolist()):
        assert a == b or abs(s64[a] - s64[b]) <= 2e-7, (a, b, s64[a], s64[b])
    np.testing.assert_allclose(b_score[0], s_score[0], atol=2e-6, rtol=2e-6)
    for qi in range(1, 16):  # (query 0's cluster is ranked by fp32 summation-order noise: judged against f64 above)
        np.testing.assert_allclose(b_score[qi], s_score[qi], atol=2e-6, rtol=2e-6)
        _ids_match(b_idx[qi], b_score[qi], s_idx[qi], s_score[qi])


@pytest.mark.parametrize("family,shadow_rows", [(3, "shadowg_rows"), (2, "shadow_rows")])
def test_tile_shadow_copies_follow_adds_overwrites_and_clear(native, family, shadow_rows):
    n, d, nq, k = 120_000 + 17, 96, 64, 10                    # (not a multiple of the i8 copy's 64-row groups)
    rows = _rows(O.SEED_CORPUS, n + 40_000, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, nq, d))
    with native.NativeIndex(d, capacity_rows=n) as ix:          # capacity grows on the second add
        ix.set_option("gemm_bf16", family)
        ix.add(rows[:n])
        idx, score = ix.search(queries, k)
        assert ix.get_option("last_gemm_family") == family and ix.get_option(shadow_rows) == n
        for qi in (0, 31, 63):
            _check(idx[qi], score[qi], rows[:n], queries[qi], k)
        # append: new rows must be visible to the batched path (shadow extended, capacity regrown)
        ix.add(rows[n:])
        idx, score = ix.search(queries, k)
        assert ix.get_option(shadow_rows) == n + 40_000
        for qi in (0, 31, 63):
            _check(idx[qi], score[qi], rows, queries[qi], k)
        # overwrite rows in place with copies of query 5: they must win for query 5, through the shadow
        rows[[7, 50_000, n + 1]] = queries[5]
        ix.set_rows(7, rows[7:8])
        ix.set_rows(50_000, rows[50_000:50_001])
        ix.set_rows(n + 1, rows[n + 1:n + 2])
        assert ix.get_option(shadow_rows) == n + 40_000   # overwritten rows are re-converted in place, nothing else
        idx, score = ix.search(queries, k)
        assert idx[5, :3].tolist() == [7, 50_000, n + 1] and np.all(np.abs(score[5, :3] - 1.0) < 1e-6)
        _check(idx[9], score[9], rows, queries[9], k)
        ix.clear()
        assert ix.get_option(shadow_rows) == 0
        ix.add(rows[:70_000])
        idx, score = ix.search(queries, k)
        _check(idx[3], score[3], rows[:70_000], queries[3], k)


@pytest.mark.parametrize("shrink", ["clear", "compact"])
def test_i8_groups_behind_the_last_row_never_vouch_after_the_corpus_shrank(native, shrink):
    """the i8 tiles read whole 256-row tiles and trust the group table's bad-row bits for rows past the
    end.  After clear() + fewer rows, or a compaction that drops LIVE tail rows, the 64-row groups between ceil(n / 64) and
    the end of the last tile used to keep the old corpus's bytes, scales and 'good' bits: when that tile is sampled their
    lower bounds entered the k-th largest, the threshold rose above the true k-th score and true neighbours were dropped.
    Here the stale rows are exact copies of the queries (score 1.0) in 6 distinct 32-row blocks, k = 4, every tile sampled."""
    n1, d, nq, k = 100_000, 96, 64, 4
    n2 = 256 * 273 + 5                                          # last tile: rows 69 888 .. 70 143, 5 of them live
    rows = _rows(O.SEED_CORPUS, n1, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, nq, d))
    stale = [69_952 + 32 * j + 3 for j in range(6)]             # inside the tile's groups 1093 .. 1095: past n2
    rows[stale] = queries[0]
    with native.NativeIndex(d, capacity_rows=n1) as ix:
        ix.set_option("gemm_sample_div", 1)                     # the sample pass visits every tile, so also the last one
        ix.add(rows)
        idx, score = ix.search(queries, k)
        assert ix.get_option("last_gemm_family") == 3 and ix.get_option("shadowg_rows") == n1
        assert sorted(idx[0].tolist()) == stale[:k] and np.all(np.abs(score[0] - 1.0) < 1e-6)
        if shrink == "clear":
            ix.clear()
            ix.add(rows[:n2])
        else:
            ix.compact(np.arange(n2, dtype=np.uint64))          # keeps a prefix: nothing moves, live tail rows are dropped
        assert ix.size() == n2
        idx, score = ix.search(queries, k)
        assert ix.get_option("last_gemm_family") == 3 and ix.get_option("shadowg_rows") == n2
        st = ix.batch_status(nq)
        assert st["overflowed"] == 0 and np.all(st["counts"] >= k)   # (a threshold from stale rows leaves query 0 no candidate)
        for qi in (0, 1, 17, 63):
            _check(idx[qi], score[qi], rows[:n2], queries[qi], k)
        # growing again into the same tile: the rows become live with their NEW contents
        fresh = _rows(77, 300, d)
        ix.add(fresh)
        both = np.concatenate([rows[:n2], fresh])
        idx, score = ix.search(queries, k)
        for qi in (0, 5):
            _check(idx[qi], score[qi], both, queries[qi], k)


def test_bf16_selection_handles_nan_rows_huge_norms_and_zero_queries(native):
    n, d, nq, k = 100_000, 64, 130, 8
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[11] = np.nan                      # never returned
    rows[12] *= 1e3                        # dominates inner products; enters the error margin through max |c|
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    queries[4] = 0.0                       # every score equal: rows 0..k-1 by the tie rule
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.add(rows)
        b_idx, b_score = ix.search(queries, k)
        st = ix.batch_status(nq)
        ix.set_option("gemm_min_queries", 1 << 30)
        s_idx, s_score = ix.search(queries, k)
    assert 11 not in b_idx.ravel().tolist()
    assert st["overflowed"] >= 1           # the zero query selects everything and is repaired on the scan path
    assert b_idx[4].tolist() == [i for i in range(k + 1) if i != 11][:k] and np.all(b_score[4] == 0.0)
    for qi in range(nq):
        # (row 12's terms are ~1e3 and cancel to a few hundred: two fp32 summation orders differ by ~1e-3 there)
        np.testing.assert_allclose(b_score[qi], s_score[qi], rtol=1e-5, atol=2e-5)
        _ids_match(b_idx[qi], b_score[qi], s_idx[qi], s_score[qi], tie=1e-5)


# --------------------------------------------------------------------------- #
# single queries over the bf16 shadow (selection pass + exact re-scoring + on-device repair)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("path", [2, 1])  # u8 selection scan (default) / bf16 tile kernel with one live column
@pytest.mark.parametrize("metric", ["cosine", "l2"])
@pytest.mark.parametrize("n,d,k", [(200_000, 384, 10), (150_003, 100, 100), (70_001, 768, 1), (90_000, 1000, 7)])
def test_single_query_shadow_selection_matches_oracle_and_fp32_scan(native, metric, n, d, k, path):
    m = native.METRIC_L2 if metric == "l2" else native.METRIC_COSINE
    om = O.METRIC_L2 if metric == "l2" else O.METRIC_COSINE
    with native.NativeIndex(d, metric=m, capacity_rows=n) as ix:
        assert ix.get_option("scan_shadow") == 2 and ix.get_option("single_min_rows") == 131072
        ix.set_option("scan_shadow", path)
        ix.set_option("single_min_rows", 0)   # lone queries on corpora this small default to the fp32 scan (launch latency)
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        rows = ix.get_rows(0, n)
        queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 50, 12, d))
        ix.profile(True)
        got = [ix.search(q, k) for q in queries]            # nq = 1 calls
        # (u8 scan: one full-pass launch per query + one sample launch per call; tile path: a launch pair per query)
        assert ix.profile_read()["scan_launches"] == 0
        assert ix.profile_read_gemm()["gemm_launches"] == (1 if path == 2 else 2) * len(queries)
        assert ix.profile_read_sample()["sample_launches"] == (len(queries) if path == 2 else 0)
        assert ix.get_option("last_single_path") == path
        assert ix.get_option("shadow8_rows" if path == 2 else "shadow_rows") == n
        assert ix.get_option("shadow_rows" if path == 2 else "shadow8_rows") == 0   # only the copy in use is built
        ix.set_option("scan_shadow", 0)
        ref = [ix.search(q, k) for q in queries]
        assert ix.profile_read()["scan_launches"] == len(queries)
    for q, (idx, score), (r_idx, r_score) in zip(queries, got, ref):
        s64 = O.flat_scores_f64(rows, q, om)
        order = np.lexsort((np.arange(n), s64 if metric == "l2" else -s64))[:k]
        np.testing.assert_allclose(score[0], s64[order], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(score[0], r_score[0], rtol=2e-6, atol=2e-6)
        _ids_match(idx[0], score[0], r_idx[0], r_score[0])
        for a, b in zip(idx[0].tolist(), order.tolist()):
            assert a == b or abs(s64[a] - s64[b]) <= 1e-5 * max(1.0, abs(s64[b])), (a, b)


@pytest.mark.parametrize("path", [2, 1])
def test_single_query_shadow_overflow_is_repaired_on_the_device(native, path):
    """Half of the corpus equals query 1: its selection keeps far more candidates than the buffer holds.  The
    asynchronous device entry point has no host in the loop, so the fp32 scan that follows as a conditional
    repair launch must produce the exact answer (ties in ascending row order); queries 0 and 2 do not overflow
    and must keep their selection results."""
    n, d, k = 120_000, 128, 10
    rows = _rows(O.SEED_CORPUS, n, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 3, d))
    rows[1::2] = queries[1]
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.set_option("scan_shadow", path)
        ix.add(rows)
        dq = ix.device_queries(queries)
        d_idx, d_score = ix.alloc(3 * k * 8), ix.alloc(3 * k * 4)
        ix.profile(True)
        ix.search_device(dq, 3, k, d_idx, d_score)
        ix.synchronize()
        assert ix.profile_read_gemm()["gemm_launches"] == (3 if path == 2 else 6)
        idx, score = d_idx.download(np.int64, (3, k)), d_score.download(np.float32, (3, k))
        ix.set_option("scan_shadow", 0)
        ix.search_device(dq, 3, k, d_idx, d_score)
        ix.synchronize()
        r_idx, r_score = d_idx.download(np.int64, (3, k)), d_score.download(np.float32, (3, k))
    assert idx[1].tolist() == list(range(1, 2 * k, 2)) and np.all(score[1] == score[1][0])
    assert np.array_equal(idx[1], r_idx[1]) and np.array_equal(score[1], r_score[1])   # the repair IS the fp32 scan
    # the blocking entry point with a lone query: no repair launches are queued, the overflow word written by the final
    # merge makes the host run the fp32 scan after its synchronisation
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.set_option("scan_shadow", path)
        ix.set_option("single_min_rows", 0)
        ix.add(rows)
        ix.profile(True)
        b_idx, b_score = ix.search(queries[1], k)
        assert ix.get_option("last_single_path") == 0 or path == 1   # the last pass was the repairing fp32 scan (u8 path)
        assert ix.profile_read()["scan_launches"] == (1 if path == 2 else 0)
        assert np.array_equal(b_idx[0], r_idx[1]) and np.array_equal(b_score[0], r_score[1])
        c_idx, c_score = ix.search(queries[0], k)              # no overflow: no fp32 scan at all
        assert ix.profile_read()["scan_launches"] == 0 and ix.get_option("last_single_path") == path
        _ids_match(c_idx[0], c_score[0], r_idx[0], r_score[0])
    for qi in (0, 2):
        _check(idx[qi], score[qi], rows, queries[qi], k)
        _ids_match(idx[qi], score[qi], r_idx[qi], r_score[qi])


@pytest.mark.parametrize("path", [2, 1])
def test_single_query_shadow_selection_through_the_sharded_entry_point(native, path):
    n, d, k, nq = 100_000, 128, 10, 40      # 40 queries: one all-gather per 32 (exchange_batch), selection per query
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.set_option("scan_shadow", path)
        ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
        ix.comm_init(1, 0, native.NativeIndex.comm_unique_id(), global_row_base=3_000_000)
        dq = ix.device_queries_synthetic(O.SEED_QUERY, 0, nq, normalize=True)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        ix.profile(True)
        ix.search_device(dq, nq, k, d_idx, d_score, sharded=True)
        ix.synchronize()
        assert ix.profile_read_gemm()["gemm_launches"] == (1 if path == 2 else 2) * nq and ix.profile_read()["scan_launches"] == 0
        assert ix.profile_read_sample()["sample_launches"] == (2 if path == 2 else 0)   # rounds of 32 queries
        g_idx, g_score = d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))
        ix.search_device(dq, nq, k, d_idx, d_score, sharded=False)
        ix.synchronize()
        l_idx, l_score = d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))
        ix.set_option("scan_shadow", 0)
        ix.search_device(dq, nq, k, d_idx, d_score, sharded=True)
        ix.synchronize()
        s_idx, s_score = d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))
        ix.comm_destroy()
    assert np.array_equal(g_idx, l_idx + 3_000_000) and np.array_equal(g_score, l_score)
    np.testing.assert_allclose(g_score, s_score, atol=2e-6, rtol=0)
    for qi in range(nq):
        _ids_match(g_idx[qi], g_score[qi], s_idx[qi], s_score[qi])


def test_masked_and_large_k_single_queries_stay_on_the_fp32_scan(native):
    n, d = 80_000, 96
    rows = _rows(O.SEED_CORPUS, n, d)
    q = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 3, 1, d))[0]
    allowed = np.arange(n) % 5 != 0
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.add(rows)
        ix.profile(True)
        idx, score = ix.search(q, 10)                        # a lone query on 80 k rows: fp32 scan (fewer launches to wait for)
        assert ix.profile_read()["scan_launches"] == 1 and ix.get_option("last_single_path") == 0
        ix.set_option("single_min_rows", 0)
        # row masks: honoured by the u8 selection scan, not by the bf16 tile path (-> fp32 scan there)
        idx, score = ix.search(q, 10, mask_words=native.pack_row_mask(allowed))
        assert ix.profile_read()["scan_launches"] == 0 and ix.profile_read_gemm()["gemm_launches"] == 1
        o_idx, o_score = O.flat_search(rows, q, 10, normalize_query=False, allowed=allowed)
        assert idx[0].tolist() == o_idx.tolist()
        ix.set_option("scan_shadow", 1)
        idx, score = ix.search(q, 10, mask_words=native.pack_row_mask(allowed))
        assert ix.profile_read()["scan_launches"] == 1 and ix.profile_read_gemm()["gemm_launches"] == 0
        assert idx[0].tolist() == o_idx.tolist()
        ix.set_option("scan_shadow", 2)
        idx, score = ix.search(q, 300)                       # radix-select path
        assert ix.profile_read()["scan_launches"] == 1 and ix.profile_read_gemm()["gemm_launches"] == 0
        _check(idx[0], score[0], rows, q, 300)
        idx, score = ix.search(q, 10)                        # and back on the shadow
        assert ix.profile_read()["scan_launches"] == 0 and ix.profile_read_gemm()["gemm_launches"] == 1
        _check(idx[0], score[0], rows, q, 10)
    # short rows: the 128-element padded shadow would be no smaller than the fp32 rows -> fp32 scan / fp32-row tiles
    small = _rows(O.SEED_CORPUS, 70_000, 48)
    with native.NativeIndex(48, capacity_rows=70_000) as ix:
        ix.add(small)
        ix.profile(True)
        idx, score = ix.search(small[5], 10)
        assert ix.profile_read()["scan_launches"] == 1 and ix.get_option("shadow_bytes") == 0
        assert ix.get_option("shadow8_bytes") == 0 and ix.get_option("last_single_path") == 0
        _check(idx[0], score[0], small, small[5], 10)
        qs = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 8, 48))
        idx, score = ix.search(qs, 10)                        # batched: the i8 tiles (128 bytes per row against 192 of fp32)
        assert ix.get_option("last_gemm_family") == 3 and ix.get_option("shadow_bytes") == 0
        _check(idx[3], score[3], small, qs[3], 10)
        ix.set_option("gemm_bf16", 2)
        idx, score = ix.search(qs, 10)                        # bf16 tiles: on the fp32 rows (the padded bf16 copy would be larger)
        assert ix.get_option("last_gemm_family") == 1 and ix.get_option("shadow_bytes") == 0
        _check(idx[3], score[3], small, qs[3], 10)


def test_u8_selection_scan_adversarial_rows(native):
    """Rows that stress the u8 quantisation bound: one huge element per row (coarse scale, large error bound),
    all-equal rows, zero rows, a NaN row, an Inf row, a cluster around the query closer together than one
    quantisation step, and rows overwritten after the shadow was built.  Answers must equal the fp32 scan's."""
    n, d, k = 120_000, 200, 20
    rng = np.random.default_rng(21)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[:20_000, 7] *= 60.0                      # outlier element: scale 60x coarser for these rows
    rows[20_000:20_100] = 0.25                    # all elements equal
    rows[20_100:20_200] = 0.0                     # zero rows (scale 0)
    rows[30_000] = np.nan
    rows[30_001, 3] = np.inf
    q = rng.standard_normal(d).astype(np.float32)
    cluster = rng.choice(np.arange(40_000, n), 500, replace=False)
    rows[cluster] = q * 3.0 + rng.standard_normal((500, d)).astype(np.float32) * 1e-3   # far below one step of 3|q|max/127
    queries = np.stack([q, -q, rows[5], np.zeros(d, np.float32), rows[20_050]])
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.set_option("single_min_rows", 0)
        ix.add(rows)
        got = [ix.search(x, k) for x in queries]
        assert ix.get_option("last_single_path") == 2 and ix.get_option("shadow8_rows") == n
        ix.set_option("scan_shadow", 0)
        ref = [ix.search(x, k) for x in queries]
        ix.set_option("scan_shadow", 2)
        rows[77] = q * 5.0                        # overwrite after the shadow exists: must win for q
        ix.set_rows(77, rows[77:78])
        assert ix.get_option("shadow8_rows") == n   # the overwritten row was re-quantised in place
        got_after = ix.search(q, k)
        ix.set_option("scan_shadow", 0)
        ref_after = ix.search(q, k)
    for (idx, score), (r_idx, r_score) in zip(got + [got_after], ref + [ref_after]):
        np.testing.assert_array_equal(np.isinf(score), np.isinf(r_score))
        fin = np.isfinite(r_score)
        np.testing.assert_allclose(score[fin], r_score[fin], rtol=3e-6, atol=1e-4)
        _ids_match(idx[0], np.nan_to_num(score[0], posinf=3e38), r_idx[0], np.nan_to_num(r_score[0], posinf=3e38), tie=3e-6)
        assert 30_000 not in idx[0].tolist()
    assert got_after[0][0, 0] == 77 and set(got[0][0][0].tolist()) <= set(cluster.tolist())


@pytest.mark.parametrize("family", [3, 2, 1])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_batched_tiles_with_huge_infinite_and_nan_rows(native, family, metric):
    """The batched selection tiles must not lose a row whose bf16 image overflows: a FINITE fp32 element beyond the
    largest bf16 (3.39e38) used to round to +-inf, and inf * 0 or inf - inf made the selection score NaN while the
    fp32 score is finite.  Now finite values are clamped at conversion, and any 64-row group that holds a row with an
    infinite NORM (such elements, or a true infinity) sends all its rows to the exact pass.  NaN rows (removed rows)
    are never results and cost nothing.  Answers must equal the fp32 scan's."""
    n, d, k = 140_000, 200, 12
    rng = np.random.default_rng(33)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    q[7], q[8], q[3] = 0.5, -0.499, 0.0
    rows[500] = 0.0
    rows[500, 7] = rows[500, 8] = 3.4e38        # finite, beyond bf16: bf16 inf - inf = NaN; fp32 score 3.4e35: the winner
    rows[90_000, 3] = 3.4e38                    # finite, beyond bf16, against q[3] = 0: bf16 inf * 0 = NaN; fp32 score ordinary
    rows[90_000, :3] = q[:3] * 40.0             # ... and large enough to be a top row for q
    rows[90_000, 4:] = q[4:] * 40.0
    rows[120_001, 5] = np.inf                   # a true infinity: +inf / -inf / NaN by the sign of q[5], as in the fp32 scan
    rows[60_000:68_000] = np.nan                # 8000 removed rows
    queries = np.stack([q, -q, rows[77], np.where(np.arange(d) == 5, 0.0, q).astype(np.float32)] * 2)
    m = native.METRIC_L2 if metric == "l2" else native.METRIC_COSINE
    with native.NativeIndex(d, metric=m, capacity_rows=n) as ix:
        ix.add(rows)
        ix.set_option("gemm_bf16", family)
        idx, score = ix.search(queries, k)
        if family == 3:
            assert ix.get_option("last_gemm_family") == 3           # (its bounds are per 64-row group by construction)
        else:
            assert ix.get_option("last_gemm_family") == min(family, 2) and ix.get_option("group_bounds_active") == 1
        assert ix.batch_status(len(queries))["overflowed"] == 0
        ix.set_option("scan_shadow", 0)
        ix.set_option("gemm_min_queries", 1 << 30)
        r_idx, r_score = ix.search(queries, k)
    with np.errstate(all="ignore"):
        for i in range(len(queries)):
            np.testing.assert_array_equal(np.isinf(score[i]), np.isinf(r_score[i]))
            fin = np.isfinite(r_score[i])
            np.testing.assert_allclose(score[i][fin], r_score[i][fin], rtol=3e-6, atol=1e-4)
            _ids_match(idx[i], np.nan_to_num(score[i], posinf=3e38, neginf=-3e38), r_idx[i],
                       np.nan_to_num(r_score[i], posinf=3e38, neginf=-3e38), tie=3e-6)
            assert not (set(idx[i].tolist()) & set(range(60_000, 68_000)))
    if metric == "cosine":
        assert idx[0, 0] == 500 and 90_000 in idx[0].tolist()


def test_i8_prefilter_epilogue_keeps_exactly_the_same_candidates(native):
    """The default PHASE-1 instance for 256-query blocks of 384-byte rows since round 3 (`gemm8_variant=13` = the round-2 form): a launch-constant prefilter in front of the exact tile
    epilogue on ORDINARY groups.  It may only skip work, never a candidate: per-query candidate counts and results must
    equal the product form's, also with outlier groups (not ordinary: exact epilogue), removed rows and a padded block."""
    n, d, nq, k = 300_000, 384, 250, 10
    rng = np.random.default_rng(12)
    rows = O.normalize_rows_fast(rng.standard_normal((n, d)).astype(np.float32))
    rows[70_000:70_064] *= 40.0           # an outlier group: bounds far above the ordinary ones
    rows[150_000:150_500] = np.nan        # removed rows
    queries = O.normalize_rows_fast(rng.standard_normal((nq, d)).astype(np.float32))
    queries[7] = rows[70_010] / 40.0      # its best rows live in the outlier group
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.add(rows)
        dq = ix.device_queries(queries)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        out = {}
        ix.set_option("gemm8_refine", 0)   # (the raw candidate sets of the tile kernel, before the second stage thins them)
        for variant in (13, 0, 12, 13):
            ix.set_option("gemm8_variant", variant)
            ix.search_batch_device(dq, nq, k, d_idx, d_score)
            st = ix.batch_status(nq)
            out.setdefault(variant, []).append((st["counts"].copy(), d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))))
        assert ix.get_option("last_gemm_family") == 3
    (c0, i0, s0), (c0b, _, _) = out[13]
    assert np.array_equal(c0, c0b)
    for variant in (0, 12):  # the default (prefilter tests in one block) and its branch-per-column-group form
        c12, i12, s12 = out[variant][0]
        assert np.array_equal(c0, c12) and np.array_equal(i0, i12) and np.array_equal(s0, s12), variant
    assert i0[7, 0] == 70_010


def test_removed_experiment_options_are_refused(native):
    """The library keeps three int8 tile epilogue forms (`gemm8_variant` 0 = 14, 12, 13) and no timing-only instance of the
    u8 scan: a probe script that asks for a removed form fails loudly instead of silently timing the product form."""
    n, d = 256, 128
    rows = O.normalize_rows_fast(np.random.default_rng(5).standard_normal((n, d)).astype(np.float32))
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.add(rows)
        with pytest.raises(native.HipBackendError) as err:
            ix.set_option("scan8_ablate", 1)
        assert err.value.code == -1 and "unknown option" in err.value.message
        for kept in (12, 13, 14, 0):
            ix.set_option("gemm8_variant", kept)
            assert ix.get_option("gemm8_variant") == kept
        for previous in (0, 13):
            ix.set_option("gemm8_variant", previous)
            for removed in (1, 6, 8, 29, 31):
                with pytest.raises(native.HipBackendError) as err:
                    ix.set_option("gemm8_variant", removed)
                assert err.value.code == -1 and "gemm8_variant" in err.value.message, removed
                assert ix.get_option("gemm8_variant") == previous


@pytest.mark.parametrize("metric,k", [("cosine", 10), ("cosine", 150), ("l2", 10), ("l2", 100)])
def test_i8_second_stage_drops_rows_but_never_an_answer(native, metric, k):
    """refine_pairs_kernel (round 3): between the tile pass and the exact pass every candidate's own bounds (from the
    integer dot product its pair carries) are compared with the k-th largest lower bound among the query's candidates.
    Answers with and without it must be bit-identical -- ties, an outlier group, removed rows, an infinite row, a zero query
    and a padded block included -- while the rows the exact pass reads shrink several-fold."""
    n, d, nq = 300_000, 384, 250
    rng = np.random.default_rng(21)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    if metric == "cosine":
        rows = O.normalize_rows_fast(rows)
    rows[70_000:70_064] *= 4.0            # an outlier group (not ORDINARY for the prefilter: the exact tile epilogue)
    rows[150_000:150_500] = np.nan        # removed rows
    rows[200_000, 3] = np.inf             # its group vouches for nothing: bounds (-inf, +inf), always kept
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    if metric == "cosine":
        queries = O.normalize_rows_fast(queries)
    queries[7] = rows[70_010] / (4.0 if metric == "cosine" else 1.0)
    queries[9] = 0.0
    rows[[11, 5_000, 123_456, 250_001, 299_999]] = queries[3]   # five exact ties for the best place of query 3
    with native.NativeIndex(d, metric=native.METRIC_L2 if metric == "l2" else native.METRIC_COSINE, capacity_rows=n) as ix:
        ix.add(rows)
        dq = ix.device_queries(queries)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        out = {}
        for refine in (0, 1):
            ix.set_option("gemm8_refine", refine)
            ix.search_batch_device(dq, nq, k, d_idx, d_score)
            st = ix.batch_status(nq)
            assert ix.get_option("last_gemm_family") == 3
            out[refine] = (st["counts"].astype(np.int64), st["overflowed"], d_idx.download(np.int64, (nq, k)),
                           d_score.download(np.float32, (nq, k)))
        ix.set_option("gemm_min_queries", 1 << 30)   # the exact fp32 scan, query by query
        ix.set_option("scan_shadow", 0)
        s_idx, s_score = ix.search(queries[:12], k)
    (c0, o0, i0, s0), (c1, o1, i1, s1) = out[0], out[1]
    assert np.array_equal(i0, i1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
    assert o0 == o1
    assert np.all(c1 <= c0)
    ordinary = np.ones(nq, bool)
    ordinary[[7, 9]] = False
    assert c1[ordinary].mean() * 3 < c0[ordinary].mean(), (c0[ordinary].mean(), c1[ordinary].mean())
    assert i1[3, :5].tolist() == [11, 5_000, 123_456, 250_001, 299_999]
    for qi in range(12):
        if qi == 9:
            continue   # (all scores equal: every path returns the first k rows, checked below)
        np.testing.assert_allclose(s1[qi], s_score[qi], rtol=1e-5, atol=2e-5)
        _ids_match(i1[qi], s1[qi], s_idx[qi], s_score[qi], tie=1e-6)
    if metric == "cosine":
        assert np.all(s1[9] == 0.0)


@pytest.mark.parametrize("metric,k", [("cosine", 500), ("cosine", 2048), ("l2", 2048)])
def test_i8_second_stage_at_large_k(native, metric, k):
    """The second stage's launch at the k where its dynamic LDS request used to pass what a launch may ask for (64 KiB from
    k = 482 without the function's limit raised, a CU's 160 KiB from k = 1205): refine_launch_for keeps it within 128 KiB by
    running fewer waves (host_refine.h).  On the smallest corpus the batched path accepts at that k -- the sample's bounds
    reach k from ceil(k / 8) tiles on, but the entry point asks for max(65 536, 1024 k) rows first -- the answers with and
    without the stage are bit-identical and agree with the fp32 scan."""
    n, d, nq = max(65_536, 1024 * k), 64, 20   # (d = 64: the shortest rows the int8 tiles take)
    rng = np.random.default_rng(482 + k)
    rows = rng.random((n, d), dtype=np.float32) - np.float32(0.5)
    queries = rng.random((nq, d), dtype=np.float32) - np.float32(0.5)
    if metric == "cosine":
        rows, queries = O.normalize_rows_fast(rows), O.normalize_rows_fast(queries)
    rows[1_000:1_040] = np.nan   # removed rows
    with native.NativeIndex(d, metric=native.METRIC_L2 if metric == "l2" else native.METRIC_COSINE, capacity_rows=n) as ix:
        ix.add(rows)
        dq = ix.device_queries(queries)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        out = {}
        for refine in (0, 1):
            ix.set_option("gemm8_refine", refine)
            ix.search_batch_device(dq, nq, k, d_idx, d_score)
            st = ix.batch_status(nq)
            assert ix.get_option("last_gemm_family") == 3
            out[refine] = (st["counts"].astype(np.int64), d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k)))
        ix.set_option("gemm_min_queries", 1 << 30)   # the exact fp32 scan, query by query
        ix.set_option("scan_shadow", 0)
        s_idx, s_score = ix.search(queries[:3], k)
    (c0, i0, s0), (c1, i1, s1) = out[0], out[1]
    assert np.array_equal(i0, i1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
    assert np.all(c1 <= c0) and np.all(c1 >= k)
    for qi in range(3):
        np.testing.assert_allclose(s1[qi], s_score[qi], rtol=1e-5, atol=2e-5)
        _ids_match(i1[qi], s1[qi], s_idx[qi], s_score[qi], tie=1e-6)


@pytest.mark.parametrize("metric,d,k", [("cosine", 384, 10), ("l2", 768, 100), ("cosine", 256, 10), ("l2", 100, 40)])
def test_u8_sample_pass_for_several_queries_per_workgroup(native, metric, d, k):
    """scan8_sample4_kernel: on a shard whose sample does not stay cached the round's sample pass loads every sampled row
    once per 4 queries (3 at 384 / 768 bytes per row) instead of once per query.  Same arithmetic per query, so not only
    the answers but the thresholds -- hence the candidate counters -- are identical; rounds that do not fill the last
    workgroup (13 queries), removed rows and a row mask included.  (`scan8_sample4=2` forces it on a small, cached sample.)"""
    n = 400_000
    rng = np.random.default_rng(91)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((45, d)).astype(np.float32)
    if metric == "cosine":
        rows, queries = O.normalize_rows_fast(rows), O.normalize_rows_fast(queries)
    rows[10_000:10_200] = np.nan
    allowed = rng.random(n) < 0.3
    mode = native.METRIC_L2 if metric == "l2" else native.METRIC_COSINE
    with native.NativeIndex(d, metric=mode, capacity_rows=n) as ix:
        ix.add(rows)
        dq = ix.device_queries(queries)
        d_idx, d_score = ix.alloc(45 * k * 8), ix.alloc(45 * k * 4)
        out = {}
        for mode4 in (0, 2):
            ix.set_option("scan8_sample4", mode4)
            got = []
            for nq in (32, 13, 45):
                ix.search_device(dq, nq, k, d_idx, d_score)
                ix.synchronize()
                assert ix.get_option("last_single_path") == 2
                last = nq if nq <= 32 else nq - 32
                got.append((ix.batch_status(last)["counts"].copy(), d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))))
            got.append(ix.search(queries[:9], k, mask_words=native.pack_row_mask(allowed)))
            out[mode4] = got
        ix.set_option("scan_shadow", 0)
        s_idx, s_score = ix.search(queries[:6], k)
    for (c0, i0, s0), (c1, i1, s1) in zip(out[0][:3], out[2][:3]):
        assert np.array_equal(c0, c1) and np.array_equal(i0, i1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
    assert np.array_equal(out[0][3][0], out[2][3][0]) and np.array_equal(out[0][3][1], out[2][3][1])
    i1, s1 = out[2][2][1], out[2][2][2]
    for qi in range(6):
        np.testing.assert_allclose(s1[qi], s_score[qi], rtol=1e-5, atol=2e-5)
        _ids_match(i1[qi], s1[qi], s_idx[qi], s_score[qi], tie=1e-6)


def test_i8_second_stage_keeps_pairs_whose_dot_product_does_not_fit_24_bits(native):
    """d = 1024 and rows / queries of +-1 / sqrt(d): every byte is +-127, so a row equal to the query has D = 1024 * 127^2 =
    16.5 M, beyond the 24-bit field a pair carries (|D| < 2^23) -- stored as "unknown", which the second stage must always
    keep (bounds -inf / +inf) and never count towards its threshold.  Opposite rows have D = -16.5 M (never candidates)."""
    n, d, nq, k = 70_000, 1024, 8, 10
    rng = np.random.default_rng(9)
    signs = np.where(rng.random((n, d)) < 0.5, -1.0, 1.0).astype(np.float32) / np.float32(np.sqrt(d))
    queries = np.where(rng.random((nq, d)) < 0.5, -1.0, 1.0).astype(np.float32) / np.float32(np.sqrt(d))
    same = [7, 64, 4_099, 33_333, 69_999]
    signs[same] = queries[0]
    signs[[100, 200]] = -queries[0]
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.add(signs)
        dq = ix.device_queries(queries)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        out = {}
        for refine in (0, 1):
            ix.set_option("gemm8_refine", refine)
            ix.search_batch_device(dq, nq, k, d_idx, d_score)
            st = ix.batch_status(nq)
            assert ix.get_option("last_gemm_family") == 3 and st["overflowed"] == 0
            out[refine] = (st["counts"].astype(np.int64), d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k)))
        ix.set_option("gemm_min_queries", 1 << 30)
        ix.set_option("scan_shadow", 0)
        s_idx, s_score = ix.search(queries, k)
    (c0, i0, s0), (c1, i1, s1) = out[0], out[1]
    assert np.array_equal(i0, i1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
    assert i1[0, :5].tolist() == same and np.allclose(s1[0, :5], 1.0, atol=1e-5)
    assert np.all(c1 <= c0) and c1[0] >= 5
    for qi in range(nq):
        np.testing.assert_allclose(s1[qi], s_score[qi], rtol=1e-5, atol=2e-5)
        _ids_match(i1[qi], s1[qi], s_idx[qi], s_score[qi], tie=1e-6)


def test_i8_second_stage_with_more_candidates_than_its_lds_holds(native):
    """12 000 rows within the bound's width of one query: more candidates than the second stage keeps in LDS (8 192), fewer
    than the candidate buffer holds -- its wave-list form takes the threshold.  Same answers as without the stage."""
    n, d, nq, k = 200_000, 384, 8, 150
    rng = np.random.default_rng(5)
    rows = O.normalize_rows_fast(rng.standard_normal((n, d)).astype(np.float32))
    queries = O.normalize_rows_fast(rng.standard_normal((nq, d)).astype(np.float32))
    near = rng.choice(n, 12_000, replace=False)
    rows[near] = O.normalize_rows_fast(queries[0] + 2e-4 * rng.standard_normal((12_000, d)).astype(np.float32))
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.add(rows)
        dq = ix.device_queries(queries)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        out = {}
        for refine in (0, 1):
            ix.set_option("gemm8_refine", refine)
            ix.search_batch_device(dq, nq, k, d_idx, d_score)
            st = ix.batch_status(nq)
            assert ix.get_option("last_gemm_family") == 3 and st["overflowed"] == 0
            out[refine] = (st["counts"].astype(np.int64), st["capacity"], d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k)))
    (c0, cap, i0, s0), (c1, _, i1, s1) = out[0], out[1]
    assert 8192 < c0[0] <= cap, (c0[0], cap)
    assert np.array_equal(i0, i1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
    assert np.all(c1 <= c0) and c1[1:].mean() * 3 < c0[1:].mean()
    assert set(i1[0].tolist()) <= set(near.tolist())


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_block_threshold_search_selects_like_the_sorted_lists(native, metric):
    """The thresholds of the selection paths come from a bitwise block search (kth_score_kernel; at most 2^-15 relative
    below the k-th largest sampled lower bound) unless `lds_lists=1` forces the sorted-list kernels (exact k-th largest).
    Both are valid thresholds: answers identical, and the search keeps at most a sliver more candidates -- on the batched
    i8 tiles (before the second stage) and on the single-query u8 scan (candidate counters of a round)."""
    n, d, nq, k = 400_000, 384, 64, 10
    rng = np.random.default_rng(33)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    if metric == "cosine":
        rows, queries = O.normalize_rows_fast(rows), O.normalize_rows_fast(queries)
    with native.NativeIndex(d, metric=native.METRIC_L2 if metric == "l2" else native.METRIC_COSINE, capacity_rows=n) as ix:
        ix.add(rows)
        dq = ix.device_queries(queries)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        ix.set_option("gemm8_refine", 0)
        got = {}
        for lists in (1, 0):
            ix.set_option("lds_lists", lists)
            ix.search_batch_device(dq, nq, k, d_idx, d_score)
            st = ix.batch_status(nq)
            assert ix.get_option("last_gemm_family") == 3 and st["overflowed"] == 0
            b = (st["counts"].astype(np.int64), d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k)))
            ix.search_device(dq, 32, k, d_idx, d_score)          # a round of 32 single queries on the u8 scan
            ix.synchronize()
            assert ix.get_option("last_single_path") == 2
            s = (ix.batch_status(32)["counts"].astype(np.int64), d_idx.download(np.int64, (32, k)), d_score.download(np.float32, (32, k)))
            got[lists] = (b, s)
    for which in (0, 1):
        (c_exact, i_exact, s_exact), (c_search, i_search, s_search) = got[1][which], got[0][which]
        assert np.array_equal(i_exact, i_search) and np.array_equal(s_exact.view(np.uint32), s_search.view(np.uint32)), which
        assert np.all(c_search >= c_exact) and np.all(c_search <= c_exact * 1.01 + 2), (which, c_exact[:8], c_search[:8])


def test_i8_tiles_outlier_groups_are_graceful_and_lost_pairs_are_repaired(native):
    """(1) Every 64-row group holds one row 1000x larger than the rest: the group scale is set by it and the other rows
    quantise to zeros, yet the bounds stay selective (no overflow) and the answers exact.  (2) 100 all-zero queries make
    EVERY row a candidate: the waves' candidate pair lists overflow (8192 pairs per tile and wave), the whole call is
    flagged and repaired on the scan path.  Slow, never wrong."""
    n, d, nq, k = 420_000, 64, 130, 8    # (6-7 tiles per wave: 100 zero queries x 32 rows x 7 tiles overflow a 16384-pair list)
    rng = np.random.default_rng(12)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[::64] *= 1e3
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.add(rows)
        dq = ix.device_queries(queries)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        ix.search_batch_device(dq, nq, k, d_idx, d_score)
        st = ix.batch_status(nq)
        assert ix.get_option("last_gemm_family") == 3 and st["overflowed"] == 0 and st["counts"].max() < 3000
        b_idx, b_score = d_idx.download(np.int64, (nq, k)), d_score.download(np.float32, (nq, k))
        zq = queries.copy()
        zq[:100] = 0.0
        dz = ix.device_queries(zq)
        ix.search_batch_device(dz, nq, k, d_idx, d_score)      # the device entry point reports, the caller repairs
        assert ix.batch_status(nq)["overflowed"] == nq
        z_idx, z_score = ix.search(zq, k)                       # the blocking entry point repairs by itself
        ix.set_option("gemm_min_queries", 1 << 30)
        ix.set_option("scan_shadow", 0)
        s_idx, s_score = ix.search(queries, k)
    for qi in range(nq):
        # (the outlier rows' terms are ~1e3 and cancel: two fp32 summation orders differ by ~1e-3 there)
        np.testing.assert_allclose(b_score[qi], s_score[qi], rtol=1e-5, atol=2e-3)
        _ids_match(b_idx[qi], b_score[qi], s_idx[qi], s_score[qi], tie=1e-5)
        if qi >= 100:
            assert z_idx[qi].tolist() == b_idx[qi].tolist()
        else:
            assert z_idx[qi].tolist() == list(range(k)) and np.all(z_score[qi] == 0.0)


@pytest.mark.parametrize("frac", [0.5, 0.01, 0.0002, 0.0])
def test_u8_selection_scan_with_row_masks(native, frac):
    """Metadata filter push-down on the u8 path: the sample only counts allowed rows (a threshold vouched for by a
    filtered-out row would be wrong), very selective masks leave the threshold at -inf and every allowed row is
    re-scored, and a mask that allows more rows than the candidate buffer holds is repaired by the masked fp32 scan."""
    n, d, k = 150_000, 384, 10
    rows = _rows(O.SEED_CORPUS, n, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 9, 3, d))
    rng = np.random.default_rng(4)
    allowed = rng.random(n) < frac
    best = [int(O.flat_search(rows, q, 1, normalize_query=False)[0][0]) for q in queries]
    allowed[best[0]] = False                 # the unfiltered winner of query 0 is filtered out
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.set_option("single_min_rows", 0)
        ix.add(rows)
        ix.profile(True)
        for q in queries:
            idx, score = ix.search(q, k, mask_words=native.pack_row_mask(allowed))
            assert ix.get_option("last_single_path") == 2 and ix.profile_read()["scan_launches"] == 0
            o_idx, o_score = O.flat_search(rows, q, k, normalize_query=False, allowed=allowed)
            assert idx[0, : len(o_idx)].tolist() == o_idx.tolist() and np.all(idx[0, len(o_idx):] == -1)
            np.testing.assert_allclose(score[0, : len(o_idx)], o_score, atol=ATOL, rtol=0)
        idx, score = ix.search(queries[0], k)  # the mask does not leak into the next call
        assert idx[0, 0] == best[0]


@pytest.mark.parametrize("n,d,k", [(300_000, 96, 200), (1_100_000, 96, 1000), (2_200_000, 64, 2048)])
def test_u8_selection_scan_large_k(native, n, d, k):
    """k >= 200 on the selection scan: thresholds and the final top-k by radix select (over the sampled maxima and
    over the re-scored candidates).  Exact ties, NaN rows, a row mask, and an overflowing query whose answer comes
    from the conditional key-per-row repair scan -- all against the fp32 large-k path on the same handle."""
    rng = np.random.default_rng(31)
    rows = O.normalize_rows_fast(rng.standard_normal((n, d)).astype(np.float32))
    q = O.normalize_vector(rng.standard_normal(d).astype(np.float32))
    rows[5] = np.nan
    rows[1000:1100] = rows[7]                       # 101 exact ties
    allowed = np.ones(n, bool)
    allowed[::3] = False
    hot = O.normalize_vector(rng.standard_normal(d).astype(np.float32))
    rows[n // 2:: 2] = hot                          # a quarter of the corpus equals query `hot`: its candidates overflow
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.add(rows)
        ix.profile(True)
        got = [ix.search(x, k) for x in (q, rows[7].copy())]
        assert ix.get_option("last_single_path") == 2 and ix.profile_read()["scan_launches"] == 0
        got_m = ix.search(q, k, mask_words=native.pack_row_mask(allowed))
        got_hot = ix.search(hot, k)
        assert ix.batch_status(1)["overflowed"] == 1
        ix.set_option("scan_shadow", 0)
        ref = [ix.search(x, k) for x in (q, rows[7].copy())]
        ref_m = ix.search(q, k, mask_words=native.pack_row_mask(allowed))
        ref_hot = ix.search(hot, k)
    for (idx, score), (r_idx, r_score) in zip(got + [got_m], ref + [ref_m]):
        np.testing.assert_allclose(score, r_score, atol=2e-6, rtol=0)
        _ids_match(idx[0], score[0], r_idx[0], r_score[0])
        assert 5 not in idx[0].tolist()
    assert got[1][0][0, :101].tolist() == [7] + list(range(1000, 1100))
    assert not (set(got_m[0][0].tolist()) & set(np.flatnonzero(~allowed).tolist()))
    assert np.array_equal(got_hot[0], ref_hot[0]) and np.array_equal(got_hot[1], ref_hot[1])   # the repair IS the fp32 path
    assert got_hot[0][0, :k].tolist() == list(range(n // 2, n, 2))[:k]


def test_overwrites_refresh_norms_and_shadows_in_place_for_l2(native):
    """replace_vector / remove in the middle of a corpus: the cached norms and both shadow copies of exactly those
    rows are refreshed at once (L2 uses the norms in its selection), everything else stays valid."""
    n, d, k = 300_000, 128, 5
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    queries = rng.standard_normal((8, d)).astype(np.float32)
    with native.NativeIndex(d, metric=native.METRIC_L2, capacity_rows=n) as ix:
        ix.add(rows)
        ix.search(queries, k)                      # builds norms + the group-scaled i8 shadow (L2 batches run on the i8 tiles since round 3)
        ix.search(queries[0], k)                   # builds the u8 shadow
        assert ix.get_option("shadowg_rows") == n and ix.get_option("shadow8_rows") == n
        for step, r in enumerate((123_456, 7, n - 1, 200_000)):
            rows[r] = queries[step] * (1.0 if step % 2 == 0 else 50.0)     # exact hit / a row with a huge norm
            ix.set_rows(r, rows[r:r + 1])
            assert ix.get_option("shadowg_rows") == n and ix.get_option("shadow8_rows") == n
            b_idx, b_dist = ix.search(queries, k)                            # batched L2
            s_idx, s_dist = ix.search(queries[step], k)                      # single query on the u8 scan
            assert ix.get_option("last_single_path") == 2
            if step % 2 == 0:
                assert b_idx[step, 0] == r and b_dist[step, 0] == 0.0 and s_idx[0, 0] == r and s_dist[0, 0] == 0.0
            ref_idx, ref_dist = O.flat_search(rows, queries[step], k, metric=O.METRIC_L2, normalize_query=False)
            assert s_idx[0].tolist() == ref_idx.tolist() and b_idx[step].tolist() == ref_idx.tolist()
            np.testing.assert_allclose(s_dist[0], ref_dist, rtol=1e-5, atol=1e-4)
        rows[123_456] = 0.0                         # remove = zero the row (indexing.py convention)
        ix.set_rows(123_456, rows[123_456:123_457])
        s_idx, s_dist = ix.search(queries[0], k)
        ref_idx, ref_dist = O.flat_search(rows, queries[0], k, metric=O.METRIC_L2, normalize_query=False)
        # (under L2 the zero vector is a legitimate near neighbour of a random query: |q|^2 < |c - q|^2)
        assert s_idx[0].tolist() == ref_idx.tolist() and s_idx[0, 0] == 123_456
        np.testing.assert_allclose(s_dist[0], ref_dist, rtol=1e-5, atol=1e-4)


def test_in_process_group_local_stage_uses_the_selection_scan(native):
    """wdbx_group_search on a shard large enough for the u8 selection scan (its local stage ends in keys, not in
    idx/score): same answers as the oracle for k in the list and in the radix-select range."""
    n, d = 150_000, 128
    rows = _rows(O.SEED_CORPUS, n, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 40, d))
    with native.NativeGroup([0], d, cap_per_shard=n) as grp:
        assert grp.add(rows) == 0 and grp.size() == n
        for k in (10, 120):
            idx, score = grp.search(queries, k)
            for i in (0, 17, 39):
                _check(idx[i], score[i], rows, queries[i], k)


@pytest.mark.parametrize("family", [3, 2])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_outlier_norms_do_not_turn_a_batch_into_per_query_repairs(native, metric, family):
    """One row with a norm 1000x the others.  With ONE corpus-wide bound every query's selection degenerates (every
    row is a candidate, every query is repaired by a full scan); with per-group bounds (chosen automatically when the
    norms vary a lot) the outlier only loosens its own 64 rows and no query overflows.  Results equal the fp32 scans."""
    n, d, nq, k = 200_000, 128, 64, 10
    rng = np.random.default_rng(17)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    rows[100_123] *= 1000.0
    queries = rng.standard_normal((nq, d)).astype(np.float32)
    m = native.METRIC_L2 if metric == "l2" else native.METRIC_COSINE
    i8 = family == 3                           # the i8 tiles' bounds are per 64-row group (and, for L2, per row) by construction
    with native.NativeIndex(d, metric=m, capacity_rows=n) as ix:
        ix.set_option("gemm_bf16", family)
        ix.add(rows)
        b_idx, b_score = ix.search(queries, k)
        st = ix.batch_status(nq)
        assert ix.get_option("last_gemm_family") == (3 if i8 else 2) and st["overflowed"] == 0
        assert i8 or ix.get_option("group_bounds_active") == 1
        assert st["counts"].max() < 3000
        ix.set_option("group_bounds", 0)              # force the single global bound: the cliff
        g_idx, g_score = ix.search(queries, k)
        st0 = ix.batch_status(nq) if ix.get_option("group_bounds_active") == 0 else None
        ix.set_option("gemm_min_queries", 1 << 30)
        ix.set_option("scan_shadow", 0)
        s_idx, s_score = ix.search(queries, k)
    assert np.array_equal(g_idx, b_idx)
    for qi in range(nq):
        np.testing.assert_allclose(b_score[qi], s_score[qi], rtol=1e-5, atol=1e-3)
        _ids_match(b_idx[qi], b_score[qi], s_idx[qi], s_score[qi], tie=1e-5)
    # normalised rows: the cheap global bound stays in use
    unit = O.normalize_rows_fast(rows)
    with native.NativeIndex(d, metric=m, capacity_rows=n) as ix:
        ix.set_option("gemm_bf16", family)
        ix.add(unit)
        ix.search(queries, k)
        assert (i8 or ix.get_option("group_bounds_active") == 0) and ix.batch_status(nq)["overflowed"] == 0



# --------------------------------------------------------------------------- #
# the in-process shard group: per-shard host threads, exchange, merge (host_group.h)
# --------------------------------------------------------------------------- #
def _attached_group(native, rows, bounds, d, exchange=0, **opts):
    """Shards = contiguous row ranges of ``rows`` in indices of their own on device 0 + a group attached over them."""
    shards = []
    for b, e in zip(bounds[:-1], bounds[1:]):
        ix = native.NativeIndex(d, capacity_rows=max(e - b, 1))
        for o, v in opts.items():
            ix.set_option(o, v)
        if e > b:
            ix.add(rows[b:e])
        shards.append(ix)
    grp = native.NativeGroup.attach(shards, exchange=exchange)
    grp.set_row_bases(bounds[:-1])
    return shards, grp


@pytest.mark.parametrize("S,n,d", [(2, 90_000, 384), (3, 500_000, 128), (8, 640_000, 96), (5, 30_000, 64)])
def test_group_of_shards_sharing_one_device_equals_the_single_shard_answer(native, S, n, d):
    """S shards driven by S host threads inside ONE library call, exchange by device copies (the shards share the GPU,
    so they cannot be RCCL ranks): with contiguous row ranges the merged result must equal the single-shard result bit
    for bit, on the fp32 scan (small shards), the u8 selection scan (large shards), for k in the list and
    radix-select ranges, for k_out up to S * k, through the blocking and the device-resident entry points."""
    rows = _rows(O.SEED_CORPUS, n, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 70, d))
    per = -(-n // S)
    bounds = [min(i * per, n) for i in range(S + 1)]
    with native.NativeIndex(d, capacity_rows=n) as whole:
        whole.add(rows)
        shards, grp = _attached_group(native, rows, bounds, d)
        try:
            info = grp.info()
            assert info["shards"] == S and info["rccl_nranks"] == 0  # device-copy exchange, and it says so
            for k in (10, 100, 250):
                w_idx, w_score = _single_calls(whole, queries, k)
                g_idx, g_score = grp.search(queries, k)
                # (ids and order identical; scores bit-equal when shard and whole corpus take the same kernel path, within
                # fp32 summation-order noise when one re-scores candidates and the other ranks scan-kernel scores)
                assert np.array_equal(g_idx, w_idx) and np.allclose(g_score, w_score, atol=1e-6, rtol=0), k
            _check(g_idx[7], g_score[7], rows, queries[7], 250)
            # lone queries (the facade's shape), one call each
            w_idx, w_score = _single_calls(whole, queries[:5], 10)
            for i in range(5):
                g_idx, g_score = grp.search(queries[i], 10)
                assert np.array_equal(g_idx[0], w_idx[i]) and np.allclose(g_score[0], w_score[i], atol=1e-6, rtol=0)
            # k_out = S * k: the whole union of the per-shard lists, best first (the reference's pre-filter list)
            k = 4
            u_idx, u_score = grp.search_merged(queries[:3], k, S * k)
            for qi in range(3):
                cand = []
                for s, ix in enumerate(shards):
                    if ix.size():
                        si, ss = ix.search(queries[qi], min(k, ix.size()))
                        cand += [(-float(sc), int(r) + bounds[s]) for r, sc in zip(si[0], ss[0]) if r >= 0]
                cand.sort()
                got = [(-float(sc), int(r)) for r, sc in zip(u_idx[qi], u_score[qi]) if r >= 0]
                assert len(got) == min(len(cand), S * k) and [r for _, r in got] == [r for _, r in cand[: len(got)]]
                assert np.allclose([sc for sc, _ in got], [sc for sc, _ in cand[: len(got)]], atol=1e-6, rtol=0)
            # device-resident form: queries placed once on every shard's device, asynchronous searches of sub-ranges
            grp.queries_upload(queries)
            grp.search_resident(10, 40, 10)
            grp.synchronize()
            r_idx, r_score = grp.results(40, 10)
            w_idx, w_score = _single_calls(whole, queries[10:50], 10)
            assert np.array_equal(r_idx, w_idx) and np.allclose(r_score, w_score, atol=1e-6, rtol=0)
            with pytest.raises(native.HipBackendError):
                grp.search_resident(60, 20, 10)  # beyond the resident queries
            with pytest.raises(native.HipBackendError):
                grp.results(41, 10)
        finally:
            grp.close()
            for ix in shards:
                ix.close()


def test_config_c5_shape_80m_384_in_8_shards_vs_oracle(native):
    """BASELINE configs[4] in SHAPE: 80 M x 384 fp32, cosine, top-10, num_shards = 8 with 10 M contiguous rows each,
    per-shard top-k exchanged and merged on the device -- on the ONE GPU of this box (154 GB of its 288 GB: fp32 rows + u8
    shadows), so the exchange is the group's device-copy form, not the 8-rank RCCL all-gather an 8-GPU node runs (the
    merge kernel, the global row numbering, the per-shard threads and every scan kernel are the same).  Oracle: the rows
    read back from every shard, one sgemm per 1 M-row slab, ranked over all 80 M rows with the reference's order."""
    S, per, d, k = 8, 10_000_000, 384, 10
    shards, grp = [], None
    try:
        for s in range(S):
            ix = native.NativeIndex(d, capacity_rows=per)
            ix.fill_synthetic(O.SEED_CORPUS, s * per, per, normalize=True)
            shards.append(ix)
        grp = native.NativeGroup.attach(shards)
        grp.set_row_bases([s * per for s in range(S)])
        assert grp.info()["shards"] == S
        _, queries = _strict_queries("c5", 6, d)                # pre-screened on all 80 M rows: ids asserted exactly
        idx, score = grp.search(queries, k)                      # one call, six queries
        one = [grp.search(q, k) for q in queries[:2]]            # lone queries (mapped staging)
        assert all(ix.get_option("last_single_path") == 2 for ix in shards)  # every shard ran its u8 selection scan
        exp = O.slab_search_screened(lambda r0, c: shards[r0 // per].get_rows(r0 % per, c), S * per, queries, k, O.METRIC_COSINE,
                                     slab=1_000_000)
        _assert_strict(idx, score, exp)
        for qi in range(2):
            assert np.array_equal(one[qi][0][0], idx[qi]) and np.array_equal(one[qi][1][0], score[qi])
        assert len(np.unique(idx // per)) >= 4                   # the answers really come from several shards
    finally:
        if grp:
            grp.close()
        for ix in shards:
            ix.close()


def test_group_with_synthetic_resident_queries_and_an_empty_shard(native):
    """Queries generated on every shard's device (the bench's form) + a shard without rows in the middle."""
    n, d, k = 200_000, 384, 10
    bounds = [0, 120_000, 120_000, n]
    shards, grp = [], None
    try:
        for b, e in zip(bounds[:-1], bounds[1:]):
            ix = native.NativeIndex(d, capacity_rows=max(e - b, 1))
            if e > b:
                ix.fill_synthetic(O.SEED_CORPUS, b, e - b, normalize=True)
            shards.append(ix)
        grp = native.NativeGroup.attach(shards)
        grp.set_row_bases(bounds[:-1])
        grp.queries_synthetic(O.SEED_QUERY, 0, 24, normalize=True)
        grp.search_resident(0, 24, k)
        idx, score = grp.results(24, k)
        rows = _rows(O.SEED_CORPUS, n, d)
        queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 24, d))
        for i in (0, 11, 23):
            _check(idx[i], score[i], rows, queries[i], k)
    finally:
        if grp:
            grp.close()
        for ix in shards:
            ix.close()


def test_group_searches_and_per_shard_batches_from_two_threads(native):
    """an attached group shares the facade's live per-shard handles.  One thread runs group searches,
    another runs batched searches (the matrix-core pass: it re-uploads the handle's own query buffer and rewrites its
    result buffers) and single searches on the SAME handles; every answer of both must stay the right one."""
    import threading

    S, n, d, k = 2, 300_000, 128, 10
    rows = _rows(O.SEED_CORPUS, n, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 48, d))
    other = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 5000, 64, d))
    bounds = [0, n // 2, n]
    shards, grp = _attached_group(native, rows, bounds, d)
    try:
        with native.NativeIndex(d, capacity_rows=n) as whole:
            whole.add(rows)
            want_g = _single_calls(whole, queries, k)
        want_s = [ix.search(other, k) for ix in shards]
        want_1 = [ix.search(other[3], k) for ix in shards]
        errors, stop = [], threading.Event()

        def per_shard():
            try:
                while not stop.is_set():
                    for s, ix in enumerate(shards):
                        bi, bs = ix.search(other, k)          # >= 4 queries: batched pass, handle's own d_q / outputs
                        if not (np.array_equal(bi, want_s[s][0]) and np.array_equal(bs, want_s[s][1])):
                            errors.append(("batched", s))
                        oi, os_ = ix.search(other[3], k)      # lone query: mapped staging
                        if not (np.array_equal(oi, want_1[s][0]) and np.array_equal(os_, want_1[s][1])):
                            errors.append(("single", s))
            except Exception as e:  # noqa: BLE001
                errors.append(("exception", repr(e)))

        t = threading.Thread(target=per_shard)
        t.start()
        try:
            for rep in range(30):
                gi, gs = grp.search(queries, k)
                assert np.array_equal(gi, want_g[0]) and np.allclose(gs, want_g[1], atol=1e-6, rtol=0), rep
                li, ls = grp.search(queries[rep], k)
                assert np.array_equal(li[0], want_g[0][rep]) and np.allclose(ls[0], want_g[1][rep], atol=1e-6, rtol=0), rep
        finally:
            stop.set()
            t.join()
        assert not errors, errors[:5]
    finally:
        grp.close()
        for ix in shards:
            ix.close()


def test_group_rccl_exchange_is_refused_for_shards_sharing_a_device_when_demanded(native):
    with native.NativeIndex(8) as a, native.NativeIndex(8) as b:
        with pytest.raises(native.HipBackendError):
            native.NativeGroup.attach([a, b], exchange=native.NativeGroup.EXCHANGE_RCCL)
        with pytest.raises(native.HipBackendError):
            native.NativeGroup.attach([a, a])
        grp = native.NativeGroup.attach([a], exchange=native.NativeGroup.EXCHANGE_RCCL)  # one rank: a real communicator
        assert grp.info()["rccl_nranks"] == 1
        grp.close()


def test_exception_barrier_and_error_reporting_never_kill_the_interpreter(native):
    """include/wdbx_hip.h: "never throws".  Arguments that make the host side fail (absurd sizes) come back as error
    codes with a message; the interpreter lives (an exception crossing extern "C" would be std::terminate)."""
    with native.NativeIndex(16) as ix:
        ix.add(np.ones((4, 16), np.float32))
        for bad in (lambda: ix.reserve(1 << 60), lambda: ix.alloc(1 << 62), lambda: ix.search(np.ones(16, np.float32), 0),
                    lambda: ix.batch_status(10**9)):
            with pytest.raises(native.HipBackendError):
                bad()
        idx, _ = ix.search(np.ones(16, np.float32), 2)
        assert idx[0].tolist() == [0, 1]




def test_group_batches_run_the_matrix_core_pass_on_every_shard(native):
    """A group call with enough queries (>= 4 on shards of >= 65 536 rows) lets every shard answer with ONE batched pass
    (i8 selection tiles + exact re-scoring, overflow repaired by conditional launches) and still hands over key lists:
    same merged answer as the single index, also with a query that overflows its candidate buffer on one shard."""
    S, n, d, k = 3, 420_000, 128, 10
    rows = _rows(O.SEED_CORPUS, n, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 96, d))
    rows[150_001:280_000:2] = queries[5]            # shard 1 holds ~65 k copies of query 5
    bounds = [0, 140_000, 280_000, n]
    with native.NativeIndex(d, capacity_rows=n) as whole:
        whole.add(rows)
        whole.set_option("gemm_min_queries", 1 << 30)
        want = _single_calls(whole, queries, k)
    shards, grp = _attached_group(native, rows, bounds, d)
    try:
        for ix in shards:
            ix.profile(True)
            ix.profile_read_gemm()
        g_idx, g_score = grp.search(queries, k)
        for ix in shards:
            assert ix.get_option("last_gemm_family") == 3 and ix.get_option("last_batch_repaired") == 1
            assert ix.profile_read_gemm()["gemm_launches"] == 2      # one sample pass + one full pass per shard
        assert np.array_equal(g_idx, want[0]) and np.allclose(g_score, want[1], atol=1e-6, rtol=0)
        assert g_idx[5].tolist() == list(range(150_001, 150_001 + 2 * k, 2))
        assert shards[1].batch_status(96)["overflowed"] >= 1
        # the same query alone: shard 1's selection scan overflows, its repair was NOT queued (lone queries defer it), the
        # group sees the shard's overflow word after its synchronisation and runs the call again with the repairs in place
        l_idx, l_score = grp.search(queries[5], k)
        assert l_idx[0].tolist() == g_idx[5].tolist() and np.allclose(l_score[0], g_score[5], atol=1e-6, rtol=0)
        l_idx, l_score = grp.search(queries[6], k)   # (and an ordinary lone query)
        assert l_idx[0].tolist() == g_idx[6].tolist() and np.allclose(l_score[0], g_score[6], atol=1e-6, rtol=0)
    finally:
        grp.close()
        for ix in shards:
            ix.close()


def test_group_search_with_a_row_mask_per_shard(native):
    """Metadata filter push-down through the group: every shard applies its own row mask inside its scan (u8 selection
    scan on the large shards, fp32 scan on the small one); the merged answer is the exact top-k of the allowed rows."""
    n, d, k = 500_000, 128, 12
    rows = _rows(O.SEED_CORPUS, n, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 6, d))
    bounds = [0, 220_000, 450_000, n]
    rng = np.random.default_rng(8)
    allowed = rng.random(n) < 0.05
    allowed[220_000:450_000] = True            # shard 1: no restriction, passed as "no mask"
    allowed[460_000:] = False
    shards, grp = _attached_group(native, rows, bounds, d)
    try:
        masks = [native.pack_row_mask(allowed[b:e]) for b, e in zip(bounds[:-1], bounds[1:])]
        masks[1] = None
        idx, score = grp.search_merged(queries, k, k, mask_words=masks)
        lone = [grp.search_merged(q, k, k, mask_words=masks) for q in queries[:2]]
        sub = np.flatnonzero(allowed)
        for qi in range(len(queries)):
            o_idx, o_score = O.flat_search(rows[sub], queries[qi], k, normalize_query=False)
            assert idx[qi].tolist() == sub[o_idx].tolist()
            np.testing.assert_allclose(score[qi], o_score, atol=ATOL, rtol=0)
        for qi in range(2):
            assert np.array_equal(lone[qi][0][0], idx[qi]) and np.allclose(lone[qi][1][0], score[qi], atol=1e-6, rtol=0)
        # and the masks are gone afterwards: an unmasked call sees every row again
        f_idx, _ = grp.search(queries[0], k)
        assert not allowed[f_idx[0]].all()
    finally:
        grp.close()
        for ix in shards:
            ix.close()



@pytest.mark.parametrize("exchange", ["rccl", "copy"])
def test_rccl_group_over_distinct_devices_equals_the_single_index(native, exchange):
    """The N > 1 exchange as a 2+-GPU node runs it (BASELINE configs[4]; skipped on a 1-GPU box): one shard per DEVICE,
    communicators from ncclCommInitAll, S host threads each issuing its ncclAllGather, one merge launch on the root --
    against ONE index holding the same rows: a lone query (mapped staging, deferred repair), a call of 256 queries (one
    matrix-core pass per shard), a call with a row mask per shard, the resident entry point in one call and in calls of one
    query (an exchange per query), and k_out = S * k.  `exchange = copy`: the same shards over peer-access / device-copy
    exchange, the fallback when the communicators do not come up.  The reference shape: vector_store.py:323-345."""
    ndev = native.device_count()
    if ndev < 2:
        pytest.skip("needs >= 2 GPUs (RCCL takes one rank per device); tools/preflight_multigpu.py runs the same stages")
    S, per, d, k = min(ndev, 8), 300_000, 384, 10
    shards, grp, whole = [], None, None
    try:
        for s in range(S):
            ix = native.NativeIndex(d, device_id=s, capacity_rows=per)
            ix.fill_synthetic(O.SEED_CORPUS, s * per, per, normalize=True)
            shards.append(ix)
        whole = native.NativeIndex(d, device_id=0, capacity_rows=S * per)
        whole.fill_synthetic(O.SEED_CORPUS, 0, S * per, normalize=True)
        grp = native.NativeGroup.attach(shards, exchange=native.NativeGroup.EXCHANGE_RCCL if exchange == "rccl"
                                        else native.NativeGroup.EXCHANGE_COPY)
        grp.set_row_bases([s * per for s in range(S)])
        info = grp.info()
        assert info["shards"] == S and info["rccl_nranks"] == (S if exchange == "rccl" else 0)
        queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 256, d))
        for qi in range(6):                                        # lone queries
            g, w = grp.search(queries[qi], k), whole.search(queries[qi], k)
            assert np.array_equal(g[0], w[0]) and np.allclose(g[1], w[1], atol=1e-6, rtol=0), qi
        g, w = grp.search(queries, k), whole.search(queries, k)   # one call of 256: a batched pass per shard
        assert np.array_equal(g[0], w[0]) and np.allclose(g[1], w[1], atol=1e-6, rtol=0)
        assert len(np.unique(g[0] // per)) == S                    # the answers come from every shard
        allowed = (np.arange(S * per) % 5) != 0                    # a row mask per shard
        masks = [native.pack_row_mask(allowed[s * per:(s + 1) * per]) for s in range(S)]
        g = grp.search_merged(queries[:5], k, k, mask_words=masks)
        w = whole.search(queries[:5], k, mask_words=native.pack_row_mask(allowed))
        assert np.array_equal(g[0], w[0]) and np.allclose(g[1], w[1], atol=1e-6, rtol=0)
        u_idx, _ = grp.search_merged(queries[:2], 4, S * 4)        # the whole union of the per-shard lists
        assert u_idx.shape == (2, S * 4) and np.all(u_idx >= 0) and [len(set(r.tolist())) for r in u_idx] == [S * 4] * 2
        grp.queries_upload(queries[:64])
        x0 = grp.stat("exchanges")
        grp.search_resident(0, 48, k)                              # one call: one exchange
        grp.synchronize()
        assert grp.stat("exchanges") - x0 == 1
        r = grp.results(48, k)
        w = _single_calls(whole, queries[:48], k)
        assert np.array_equal(r[0], w[0]) and np.allclose(r[1], w[1], atol=1e-6, rtol=0)
        for i in range(8):                                         # calls of one query: an exchange per query
            grp.search_resident(48 + i, 1, k)
        grp.synchronize()
        assert grp.stat("exchanges") - x0 == 9
        r, w = grp.results(1, k), whole.search(queries[55], k)
        assert np.array_equal(r[0], w[0]) and np.allclose(r[1], w[1], atol=1e-6, rtol=0)
        assert grp.stat("unusable") == 0
    finally:
        if grp:
            grp.close()
        for ix in shards:
            ix.close()
        if whole:
            whole.close()


def test_group_counts_its_exchanges_and_refuses_short_masks(native):
    """On one GPU (device-copy exchange): `wdbx_group_stat("exchanges")` is what bench.py reports as
    `exchanges_in_timed_region`; a row mask shorter than its shard (built before a concurrent add) is refused by the
    library under the group's locks, by the index entry point as well."""
    n, d, k = 150_000, 96, 10
    rows = _rows(O.SEED_CORPUS, n, d)
    bounds = [0, 70_000, n]
    shards, grp = _attached_group(native, rows, bounds, d)
    try:
        grp.queries_upload(O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 40, d)))
        x0 = grp.stat("exchanges")
        grp.search_resident(0, 40, k)
        grp.synchronize()
        assert grp.stat("exchanges") - x0 == 1                     # 40 resident queries, one call: ONE exchange + merge
        for i in range(5):
            grp.search_resident(i, 1, k)
        grp.synchronize()
        assert grp.stat("exchanges") - x0 == 6 and grp.stat("dispatches") > 0 and grp.stat("unusable") == 0
        q = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 1, d))
        full = [native.pack_row_mask(np.ones(b - a, bool)) for a, b in zip(bounds[:-1], bounds[1:])]
        ok_idx, _ = grp.search_merged(q, k, k, mask_words=full)
        assert np.array_equal(ok_idx, grp.search(q, k)[0])
        # the Python wrapper checks lengths; go underneath it to see the library's own check
        import ctypes as C

        short = [full[0], full[1][:-3]]
        with pytest.raises(ValueError):
            grp.search_merged(q, k, k, mask_words=short)
        u32p = C.POINTER(C.c_uint32)
        arr = (u32p * 2)(*[m.ctypes.data_as(u32p) for m in short])
        counts = (C.c_uint64 * 2)(*[m.size for m in short])
        idx, score = np.empty((1, k), np.int64), np.empty((1, k), np.float32)
        rc = grp._lib.wdbx_group_search_merged_masked_n(grp._h, q.ctypes.data_as(C.POINTER(C.c_float)), 1, k, k, 0, arr, counts,
                                                        idx.ctypes.data_as(C.POINTER(C.c_int64)), score.ctypes.data_as(C.POINTER(C.c_float)))
        assert rc == -1 and b"row mask" in grp._lib.wdbx_last_error()
        ix = shards[0]
        rc = ix._lib.wdbx_index_search_masked_n(ix._h, q.ctypes.data_as(C.POINTER(C.c_float)), 1, k, 0, full[0].ctypes.data_as(u32p),
                                                full[0].size - 1, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                score.ctypes.data_as(C.POINTER(C.c_float)))
        assert rc == -1 and b"row mask" in ix._lib.wdbx_last_error()
        assert np.array_equal(grp.search(q, k)[0], ok_idx)          # the group is still usable after a refused call
    finally:
        grp.close()
        for s in shards:
            s.close()


@pytest.mark.parametrize("n,d", [(300_000, 128), (20_000, 384)])
def test_blocking_calls_from_many_threads_pipeline_on_one_handle_and_stay_exact(native, n, d):
    """Round 4: a small blocking call owns a staging slot and waits for ITS event with the handle's mutex released, so the
    next thread enqueues behind it (the reference calls search from 4-worker pools per index, indexing.py:692, :1045-1048).
    8 threads mix lone queries (the u8 selection scan with host-side ranking on the large corpus, the fp32 scan on the small
    one), 3-query calls, masked calls (which keep the mutex) and k = 300 (radix select): every answer must equal the answer
    the same call gives on an idle handle, bit for bit."""
    import threading

    rows = _rows(O.SEED_CORPUS, n, d)
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 0, 24, d))
    allowed = (np.arange(n) % 3) != 1
    mask = native.pack_row_mask(allowed)
    with native.NativeIndex(d, capacity_rows=n) as ix:
        ix.add(rows)

        def call(kind, i):
            if kind == 0:
                return ix.search(queries[i], 10)
            if kind == 1:
                return ix.search(queries[i:i + 3], 7)
            if kind == 2:
                return ix.search(queries[i], 10, mask_words=mask)
            return ix.search(queries[i], 300)

        want = {(kind, i): call(kind, i) for kind in range(4) for i in range(0, 21)}
        for i in (0, 5):
            _check(want[(0, i)][0][0], want[(0, i)][1][0], rows, queries[i], 10)
        errors, done = [], [0] * 8

        def worker(t):
            try:
                for it in range(60):
                    kind, i = (t + it) % 4, (3 * t + it) % 21
                    idx, score = call(kind, i)
                    w_idx, w_score = want[(kind, i)]
                    assert np.array_equal(idx, w_idx) and np.array_equal(score, w_score), (t, it, kind, i)
                    done[t] += 1
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(300)
        assert not errors, errors[:1]
        assert done == [60] * 8
