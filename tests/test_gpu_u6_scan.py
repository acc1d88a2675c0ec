"""The six-bit selection scan (kernels_scan6.h, option scan_u6) against the u8 selection scan on the MI355X: both re-score
their candidates with the same exact kernel and rank the same keys, so ids and scores must agree bit for bit -- on every
shape, with rows that hold NaN / inf, after removals, overwrites and compactions, and through the overflow repair."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 40_000


def _unit(a):
    n = np.linalg.norm(a, axis=1, keepdims=True)
    return (a / np.where(n > 0, n, 1)).astype(np.float32)


def _index(rows, **opts):
    from wdbx_amd import _native

    ix = _native.NativeIndex(rows.shape[1], device_id=0, capacity_rows=len(rows))
    ix.add(rows)
    ix.set_option("single_min_rows", 0)          # (small corpora default to the fp32 scan)
    ix.set_option("gemm_min_rows", 0)
    ix.set_option("gemm_min_queries", 1 << 30)   # rounds of single queries, not the batched tiles
    for name, value in opts.items():
        ix.set_option(name, value)
    return ix


def _both(ix, q, k, expect_u6=True, **kw):
    """the same call on the u6 and on the u8 selection; returns the u6 answer after asserting bit equality"""
    ix.set_option("scan_u6", 1)
    i6, s6 = ix.search(q, k, **kw)
    assert ix.get_option("last_single_path") == 2
    assert ix.get_option("last_single_u6") == (1 if expect_u6 else 0)
    ix.set_option("scan_u6", 0)
    i8, s8 = ix.search(q, k, **kw)
    assert ix.get_option("last_single_path") == 2 and ix.get_option("last_single_u6") == 0
    assert np.array_equal(i6, i8)
    assert np.array_equal(s6.view(np.uint32), s8.view(np.uint32))
    return i6, s6


@pytest.mark.parametrize("d", [96, 384, 400, 768])
@pytest.mark.parametrize("nq", [1, 5, 32, 70])
def test_rounds_equal_the_u8_scan(d, nq):
    rng = np.random.default_rng(1000 * d + nq)
    rows = _unit(rng.standard_normal((N, d)))
    q = _unit(rng.standard_normal((nq, d)))
    with _index(rows) as ix:
        idx, score = _both(ix, q, 10, expect_u6=nq > 1)   # (a lone query keeps the u8 scan's short chain)
        if nq > 1:
            assert ix.get_option("shadow6_rows") == N
        exact = rows.astype(np.float64) @ q[0].astype(np.float64)
        assert set(idx[0].tolist()) == set(np.argsort(-exact)[:10].tolist())
        assert np.all(np.diff(score, axis=1) <= 0)


@pytest.mark.parametrize("k", [1, 10, 32])
def test_k(k):
    rng = np.random.default_rng(k)
    rows = _unit(rng.standard_normal((N, 384)))
    q = _unit(rng.standard_normal((5, 384)))
    with _index(rows) as ix:
        _both(ix, q, k)


def test_scaled_and_clustered_rows():
    """rows of very different norms (inner product), and a tight cluster around one query far below a quantisation step"""
    rng = np.random.default_rng(3)
    rows = (rng.standard_normal((N, 384)) * rng.lognormal(0, 1.5, size=(N, 1))).astype(np.float32)
    q = rng.standard_normal((6, 384)).astype(np.float32)
    where = rng.choice(N, 300, replace=False)
    rows[where] = (q[0] * 2.0 + 1e-3 * rng.standard_normal((300, 384))).astype(np.float32)
    with _index(rows) as ix:
        _both(ix, q, 10)


def test_rows_with_nan_and_inf():
    rng = np.random.default_rng(4)
    rows = _unit(rng.standard_normal((N, 384)))
    q = _unit(rng.standard_normal((5, 384)))
    best = np.argsort(-(rows @ q[0]))[:4]
    rows[best[0], 7] = np.nan            # never returned
    rows[best[1], 9] = np.inf            # always a candidate; its exact score decides
    rows[best[2], :] = np.nan
    rows[123, 5] = -np.inf
    with _index(rows) as ix:
        idx, _ = _both(ix, q, 10)
        assert best[0] not in idx[0] and best[2] not in idx[0]


def test_removed_rows_overwrite_and_compact():
    rng = np.random.default_rng(5)
    d = 384
    rows = _unit(rng.standard_normal((N, d)))
    q = _unit(rng.standard_normal((7, d)))
    with _index(rows) as ix:
        first, _ = _both(ix, q, 10)
        # removed rows: overwritten with NaN, as the Python layer does
        gone = np.unique(first[:, :3].ravel())
        for r in gone:
            ix.set_rows(int(r), np.full((1, d), np.nan, np.float32))
        idx, _ = _both(ix, q, 10)
        assert not set(idx.ravel().tolist()) & set(gone.tolist())
        # overwrite then search: a block in the middle becomes near copies of the queries
        block = _unit(q[np.arange(200) % len(q)] + 0.05 * rng.standard_normal((200, d)))
        ix.set_rows(20_000, block)
        idx, _ = _both(ix, q, 10)
        assert np.all((idx >= 20_000) & (idx < 20_200))
        # compact then search: drop the removed rows and every third row behind row 10 000
        keep = np.setdiff1d(np.arange(N), gone)
        keep = keep[(keep < 10_000) | (keep % 3 != 0)]
        ix.compact(keep)
        assert ix.size() == len(keep)
        idx, _ = _both(ix, q, 10)
        now = ix.get_rows(0, len(keep))
        exact = now.astype(np.float64) @ q[0].astype(np.float64)
        assert set(idx[0].tolist()) == set(np.argsort(-np.nan_to_num(exact, nan=-np.inf))[:10].tolist())
        # rows appended afterwards are picked up lazily
        ix.add(_unit(q[:3] + 0.01 * rng.standard_normal((3, d))))
        idx, _ = _both(ix, q, 10)
        assert idx[0, 0] == len(keep) and ix.get_option("shadow6_rows") == len(keep) + 3


def test_tiny_candidate_buffer_is_repaired():
    """A forced 64-key candidate buffer overflows for every query; the conditional repair launches (the fp32 scan, as behind
    an overflowed u8 buffer) answer instead.  Ids equal the u8 scan's; the scores of a REPAIRED query are the fp32 scan
    kernel's (its own summation order, on either selection path), so they are compared bit for bit with that kernel's."""
    rng = np.random.default_rng(6)
    rows = _unit(rng.standard_normal((N, 384)))
    q = _unit(rng.standard_normal((5, 384)))
    with _index(rows) as ix:
        ix.set_option("scan_u6", 0)
        want = ix.search(q, 10)
        ix.set_option("scan_shadow", 0)
        scan = ix.search(q, 10)
        assert ix.get_option("last_single_path") == 0
        ix.set_option("scan_shadow", 2)
        ix.set_option("scan_u6", 1)
        ix.set_option("scan_u6_cap", 64)
        got = ix.search(q, 10)
        assert ix.get_option("last_single_u6") == 1
        status = ix.batch_status(5)
        assert status["overflowed"] == 5, status
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[0], scan[0])
        assert np.array_equal(got[1].view(np.uint32), scan[1].view(np.uint32))
        ix.set_option("scan_u6_cap", 0)
        got = ix.search(q, 10)
        assert ix.get_option("last_single_u6") == 1 and ix.batch_status(5)["overflowed"] == 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_many_ties_overflow_the_short_list():
    """thousands of exact duplicates of the best row: the cut's short list overflows and the query is repaired exactly"""
    rng = np.random.default_rng(7)
    rows = _unit(rng.standard_normal((N, 384)))
    q = _unit(rng.standard_normal((3, 384)))
    rows[5_000:11_000] = _unit(q[:1] + 0.2 * rng.standard_normal((1, 384)))
    with _index(rows) as ix:
        idx, _ = _both(ix, q, 10)
        assert idx[0].tolist() == list(range(5_000, 5_010))


def test_k_33_and_masks_fall_back():
    from wdbx_amd import _native

    rng = np.random.default_rng(8)
    rows = _unit(rng.standard_normal((N, 384)))
    q = _unit(rng.standard_normal((5, 384)))
    with _index(rows) as ix:
        _both(ix, q, 33, expect_u6=False)
        allowed = rng.random(N) < 0.5
        idx, _ = _both(ix, q, 10, expect_u6=False, mask_words=_native.pack_row_mask(allowed))
        assert np.all(allowed[idx])
        _both(ix, q, 10)                                   # and back on the u6 scan without them


def test_device_resident_round_and_resident_bytes():
    rng = np.random.default_rng(9)
    d, nq, k = 384, 40, 10
    rows = _unit(rng.standard_normal((N, d)))
    q = _unit(rng.standard_normal((nq, d)))
    with _index(rows) as ix:
        dq = ix.device_queries(q)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        out = {}
        for u6 in (1, 0):
            ix.set_option("scan_u6", u6)
            ix.search_device(dq, nq, k, d_idx, d_score)
            ix.synchronize()
            assert ix.get_option("last_single_u6") == u6
            out[u6] = (d_idx.download(np.int64, (nq, k)), d_score.download(np.uint32, (nq, k)))
        assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1])
        tiles = (ix.capacity() + 63) // 64
        assert ix.get_option("shadow6_bytes") == tiles * (d // 16) * 768 + tiles * 64 * 8
