"""The split six-bit scan (kernels_scan42.h, option scan_u42) against the u6 and the u8 selection scans on the MI355X: all three
re-score their candidates with the same exact kernel and rank the same keys, so ids and scores must agree bit for bit -- on
every shape, with rows that hold NaN / inf, after removals, overwrites, compactions and incremental adds, on clustered
near-ties and through the overflow repair.

(A refused allocation of the planes cannot be provoked here without a real out-of-memory, so that fallback has no test.)"""
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


def _three(ix, q, k, expect_u42=True, expect_u6=True, **kw):
    """the same call on the u8 selection, on the u6 pass and on the split planes; returns the last after asserting bit equality"""
    out = []
    for u6, u42 in ((0, 1), (1, 0), (1, 1)):
        ix.set_option("scan_u6", u6)
        ix.set_option("scan_u42", u42)
        out.append(ix.search(q, k, **kw))
        assert ix.get_option("last_single_path") == 2
        assert ix.get_option("last_single_u6") == (1 if u6 and expect_u6 else 0)
        assert ix.get_option("last_single_u42") == (1 if u6 and u42 and expect_u42 else 0)
    for other in out[:-1]:
        assert np.array_equal(out[-1][0], other[0])
        assert np.array_equal(out[-1][1].view(np.uint32), other[1].view(np.uint32))
    return out[-1]


@pytest.mark.parametrize("d", [96, 384, 400, 416, 768])
@pytest.mark.parametrize("nq", [2, 5, 32, 70])
def test_rounds_equal_the_u6_and_u8_scans(d, nq):
    rng = np.random.default_rng(1000 * d + nq)
    n = N + (1 if nq == 5 else 0)
    rows = _unit(rng.standard_normal((n, d)))
    q = _unit(rng.standard_normal((nq, d)))
    with _index(rows) as ix:
        # 400 is not a whole number of 32-element units: the u6 pass; 416 = 26 six-bit units has no u6 instance (its sample
        # pass takes 4 .. 8 units at a time), so the round stays on the u8 scan and the planes are never built
        idx, score = _three(ix, q, 10, expect_u42=d not in (400, 416), expect_u6=d != 416)
        if d not in (400, 416):
            assert ix.get_option("shadow42_rows") == n
            assert 0 < ix.get_option("u42_survivors_sum")
        exact = rows.astype(np.float64) @ q[0].astype(np.float64)
        assert set(idx[0].tolist()) == set(np.argsort(-exact)[:10].tolist())
        assert np.all(np.diff(score, axis=1) <= 0)


def test_default_follows_the_u6_size_rule():
    """scan_u42 = -1 (the default) below the size rule: a forced u6 round keeps the u6 full pass"""
    rng = np.random.default_rng(2)
    rows = _unit(rng.standard_normal((N, 384)))
    q = _unit(rng.standard_normal((5, 384)))
    with _index(rows, scan_u6=1) as ix:
        assert ix.get_option("scan_u42") == -1
        ix.search(q, 10)
        assert ix.get_option("last_single_u6") == 1 and ix.get_option("last_single_u42") == 0
        assert ix.get_option("shadow42_bytes") == 0


@pytest.mark.parametrize("k", [1, 10, 32])
def test_k(k):
    rng = np.random.default_rng(k)
    rows = _unit(rng.standard_normal((N, 384)))
    q = _unit(rng.standard_normal((5, 384)))
    with _index(rows) as ix:
        _three(ix, q, k)


def test_uniform_rows_leave_few_survivors():
    """the bench corpus' family (uniform elements, normalised): the four-bit bound rules out all but a few per cent of the
    rows the u6 bound keeps -- and never a row of the answer"""
    rng = np.random.default_rng(12)
    rows = _unit(rng.random((N, 384)) * 2 - 1)
    q = _unit(rng.random((8, 384)) * 2 - 1)
    with _index(rows) as ix:
        _three(ix, q, 10)
        ix.set_option("scan_u6", 1)
        ix.set_option("scan_u42", 1)
        ix.search(q, 10)
        surv, cand = ix.get_option("u42_survivors_sum"), ix.get_option("u6_candidates_sum")
        print(f"survivors {surv}, candidates {cand} of {8 * N} rows")
        assert cand <= surv < 8 * N // 4


def test_scaled_and_clustered_rows():
    """rows of very different norms (inner product), and a tight cluster around one query far below a quantisation step"""
    rng = np.random.default_rng(3)
    rows = (rng.standard_normal((N, 384)) * rng.lognormal(0, 1.5, size=(N, 1))).astype(np.float32)
    q = rng.standard_normal((6, 384)).astype(np.float32)
    where = rng.choice(N, 300, replace=False)
    rows[where] = (q[0] * 2.0 + 1e-3 * rng.standard_normal((300, 384))).astype(np.float32)
    with _index(rows) as ix:
        _three(ix, q, 10)


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
        idx, _ = _three(ix, q, 10)
        assert best[0] not in idx[0] and best[2] not in idx[0]


def test_removed_rows_overwrite_compact_and_add():
    rng = np.random.default_rng(5)
    d = 384
    rows = _unit(rng.standard_normal((N, d)))
    q = _unit(rng.standard_normal((7, d)))
    with _index(rows[:30_000]) as ix:
        _three(ix, q, 10)
        # rows added incrementally: the planes pick them up at the next round (beyond the first capacity: rebuilt)
        ix.add(rows[30_000:30_001])
        _three(ix, q, 10)
        ix.add(rows[30_001:])
        first, _ = _three(ix, q, 10)
        assert ix.get_option("shadow42_rows") == N
        exact = rows.astype(np.float64) @ q[0].astype(np.float64)
        assert set(first[0].tolist()) == set(np.argsort(-exact)[:10].tolist())
        # removed rows: overwritten with NaN, as the Python layer does
        gone = np.unique(first[:, :3].ravel())
        for r in gone:
            ix.set_rows(int(r), np.full((1, d), np.nan, np.float32))
        idx, _ = _three(ix, q, 10)
        assert not set(idx.ravel().tolist()) & set(gone.tolist())
        # overwrite then search: a block in the middle becomes near copies of the queries
        block = _unit(q[np.arange(200) % len(q)] + 0.05 * rng.standard_normal((200, d)))
        ix.set_rows(20_000, block)
        idx, _ = _three(ix, q, 10)
        assert np.all((idx >= 20_000) & (idx < 20_200))
        # compact then search: drop the removed rows and every third row behind row 10 000
        keep = np.setdiff1d(np.arange(N), gone)
        keep = keep[(keep < 10_000) | (keep % 3 != 0)]
        ix.compact(keep)
        assert ix.size() == len(keep)
        idx, _ = _three(ix, q, 10)
        now = ix.get_rows(0, len(keep))
        exact = now.astype(np.float64) @ q[0].astype(np.float64)
        assert set(idx[0].tolist()) == set(np.argsort(-np.nan_to_num(exact, nan=-np.inf))[:10].tolist())
        ix.add(_unit(q[:3] + 0.01 * rng.standard_normal((3, d))))
        idx, _ = _three(ix, q, 10)
        assert idx[0, 0] == len(keep) and ix.get_option("shadow42_rows") == len(keep) + 3


def test_tiny_candidate_buffer_is_repaired():
    """scan_u6_cap = 64 overflows every query's candidate buffer; the conditional repair launches answer instead (ids equal the
    u8 scan's, scores are the fp32 scan kernel's, as behind an overflowed u6 pass)"""
    rng = np.random.default_rng(6)
    rows = _unit(rng.standard_normal((N, 384)))
    q = _unit(rng.standard_normal((5, 384)))
    with _index(rows) as ix:
        ix.set_option("scan_u6", 0)
        want = ix.search(q, 10)
        ix.set_option("scan_shadow", 0)
        scan = ix.search(q, 10)
        ix.set_option("scan_shadow", 2)
        ix.set_option("scan_u6", 1)
        ix.set_option("scan_u42", 1)
        ix.set_option("scan_u6_cap", 64)
        got = ix.search(q, 10)
        assert ix.get_option("last_single_u42") == 1
        assert ix.batch_status(5)["overflowed"] == 5
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[0], scan[0])
        assert np.array_equal(got[1].view(np.uint32), scan[1].view(np.uint32))
        ix.set_option("scan_u6_cap", 0)
        got = ix.search(q, 10)
        assert ix.get_option("last_single_u42") == 1 and ix.batch_status(5)["overflowed"] == 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_many_ties():
    """thousands of exact duplicates of the best row: every one survives both stages, the cut's short list overflows and the
    query is repaired exactly"""
    rng = np.random.default_rng(7)
    rows = _unit(rng.standard_normal((N, 384)))
    q = _unit(rng.standard_normal((3, 384)))
    rows[5_000:11_000] = _unit(q[:1] + 0.2 * rng.standard_normal((1, 384)))
    with _index(rows) as ix:
        idx, _ = _three(ix, q, 10)
        assert idx[0].tolist() == list(range(5_000, 5_010))


def test_k_33_masks_and_lone_queries_stay_where_they_are():
    from wdbx_amd import _native

    rng = np.random.default_rng(8)
    rows = _unit(rng.standard_normal((N, 384)))
    q = _unit(rng.standard_normal((5, 384)))
    with _index(rows) as ix:
        _three(ix, q, 33, expect_u42=False, expect_u6=False)
        allowed = rng.random(N) < 0.5
        idx, _ = _three(ix, q, 10, expect_u42=False, expect_u6=False, mask_words=_native.pack_row_mask(allowed))
        assert np.all(allowed[idx])
        _three(ix, q[:1], 10, expect_u42=False, expect_u6=False)
        _three(ix, q, 10)


def test_device_resident_round_and_resident_bytes():
    rng = np.random.default_rng(9)
    d, nq, k = 384, 40, 10
    rows = _unit(rng.standard_normal((N, d)))
    q = _unit(rng.standard_normal((nq, d)))
    with _index(rows, scan_u6=1) as ix:
        dq = ix.device_queries(q)
        d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
        out = {}
        for u42 in (0, 1):
            ix.set_option("scan_u42", u42)
            before = ix.get_option("device_bytes_resident")
            ix.search_device(dq, nq, k, d_idx, d_score)
            ix.synchronize()
            assert ix.get_option("last_single_u42") == u42
            out[u42] = (d_idx.download(np.int64, (nq, k)), d_score.download(np.uint32, (nq, k)))
        assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1])
        tiles = (ix.capacity() + 63) // 64
        planes = tiles * (d // 32) * 1024 + tiles * 64 * 8 + tiles * 64 * 128   # h plane, {s, a4}, one 128-byte l record per row
        assert ix.get_option("shadow42_bytes") == planes
        assert ix.get_option("device_bytes_resident") >= before + planes
