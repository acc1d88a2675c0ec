"""Range search on the MI355X (wdbx_index_range_search and its public forms): every row whose score reaches a threshold,
against a float64 brute force.  A row may fall on either side of t only inside a band delta of the float64 score; outside
it membership is exact.  Every returned fp32 score passes the threshold as a float32 comparison and lies within delta of
float64; results are sorted like top-k; both selection paths give bit-identical answers."""
import asyncio
import shutil
import tempfile
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1


def _unit(a):
    n = np.linalg.norm(a, axis=1, keepdims=True)
    return (a / np.where(n > 0, n, 1)).astype(np.float32)


def _corpus(n, d, metric, seed, scaled=False):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    if metric == COS:
        rows = _unit(rows)
    if scaled:
        rows = (rows * rng.uniform(0.25, 4.0, size=(n, 1))).astype(np.float32)
    return rows


def _reference(rows, q, metric):
    r = rows.astype(np.float64)
    q = q.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if metric == COS:
            ref = r @ q
            band = 2e-5 * np.maximum(1.0, np.linalg.norm(r, axis=1) * np.linalg.norm(q))
        else:
            ref = ((r - q) ** 2).sum(axis=1)
            band = 2e-5 * np.maximum(1.0, (r * r).sum(axis=1) + q @ q)
    return ref, np.nan_to_num(band, nan=0.0, posinf=0.0)


def check(rows, q, t, metric, got_rows, got_scores, allowed=None):
    """membership outside the band, fp32 threshold rule, score accuracy, order, no duplicates"""
    ref, band = _reference(rows, q, metric)
    ok = ~np.isnan(ref)
    if allowed is not None:
        ok &= allowed
    if metric == COS:
        must = ok & (ref >= t + band)
        may = ok & (ref >= t - band)
    else:
        must = ok & (ref <= t - band)
        may = ok & (ref <= t + band)
    got_rows = np.asarray(got_rows, np.int64)
    got_scores = np.asarray(got_scores, np.float32)
    assert len(np.unique(got_rows)) == len(got_rows)
    got = np.zeros(len(rows), bool)
    got[got_rows] = True
    assert not np.any(must & ~got), np.flatnonzero(must & ~got)[:10]
    assert not np.any(got & ~may), np.flatnonzero(got & ~may)[:10]
    t32 = np.float32(t)
    assert np.all(got_scores >= t32) if metric == COS else np.all(got_scores <= t32)
    fin = np.isfinite(ref[got_rows])
    assert np.all(np.abs(got_scores[fin] - ref[got_rows][fin]) <= band[got_rows][fin])
    assert np.all(got_scores[~fin] == ref[got_rows][~fin])
    key = (-got_scores if metric == COS else got_scores).astype(np.float64)
    order = np.lexsort((got_rows, key))
    assert np.array_equal(order, np.arange(len(got_rows)))
    return int(got.sum())


def _index(rows, metric, **opts):
    from wdbx_amd import _native

    ix = _native.NativeIndex(rows.shape[1], metric, 0, capacity_rows=max(1, len(rows)))
    ix.add(rows)
    for k, v in opts.items():
        ix.set_option(k, v)
    return ix


def _one(ix, q, t, **kw):
    off, rows, scores = ix.range_search(q, [t], **kw)
    assert off[0] == 0 and off[1] == len(rows)
    return rows, scores


def _thresholds(rows, q, metric):
    """0 hits, a few, more than 2048 (when there are that many rows), every row"""
    ref, _ = _reference(rows, q, metric)
    s = np.sort(ref)[::-1] if metric == COS else np.sort(ref)
    ts = [float(s[0]) + 0.5 if metric == COS else float(s[0]) - 0.5, float(s[min(4, len(s) - 1)])]
    if len(s) > 3000:
        ts.append(float(s[2600]))
    ts.append(-np.inf if metric == COS else np.inf)
    ts.append(float(s[-1]) - 0.5 if metric == COS else float(s[-1]) + 0.5)
    return ts


# ---- 1. the fp32 path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("n,d", [(1, 3), (1000, 54), (10000, 100), (65535, 384), (10000, 768), (1000, 4096), (65535, 3)])
def test_fp32_path(metric, n, d):
    rows = _corpus(n, d, metric, seed=n + d)
    q = _corpus(1, d, metric, seed=7 * d + 1)[0]
    with _index(rows, metric) as ix:
        ts = _thresholds(rows, q, metric)
        for i, t in enumerate(ts):
            r, s = _one(ix, q, t)
            assert ix.get_option("last_range_path") == 0
            hits = check(rows, q, t, metric, r, s)
            if i == 0:
                assert hits == 0
            if i >= len(ts) - 2:  # (+-inf and past the farthest row: every row)
                assert hits == len(rows)


@pytest.mark.parametrize("d", [54, 100])
def test_packed_rows_per_wave_are_bit_identical_to_the_rescore_arithmetic(d):
    """d = 54 / 100: the fp32 range scan packs 4 / 2 rows per wave (16 / 32 lanes each, xor tree cut short); the u8 path's
    exact pass and the top-k re-scoring use 64 lanes per row.  Same bits."""
    rows = _corpus(20000, d, COS, seed=d)
    q = _corpus(1, d, COS, seed=d + 1)[0]
    with _index(rows, COS, single_min_rows=0, gemm_min_rows=0) as ix:
        t = float(np.sort(rows.astype(np.float64) @ q)[-200])
        r0, s0 = _one(ix, q, t)
        assert ix.get_option("last_range_path") == 0
        ix.set_option("range_min_rows", 0)
        r2, s2 = _one(ix, q, t)
        assert ix.get_option("last_range_path") == 2
        assert np.array_equal(r0, r2) and np.array_equal(s0.view(np.uint32), s2.view(np.uint32))
        idx, sc = ix.search(q, 10)
        assert ix.get_option("last_single_path") == 2
        assert np.array_equal(idx[0], r0[:10]) and np.array_equal(sc[0].view(np.uint32), s0[:10].view(np.uint32))


# ---- 2./4. the u8 selection path, overflow -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """200 000 x 128 rows per metric (cosine unit rows; L2 rows of varying scale) on the u8 path by default"""
    out = {}
    for metric in (COS, L2):
        rows = _corpus(200_000, 128, metric, seed=11 + metric, scaled=metric == L2)
        out[metric] = (rows, _index(rows, metric))
    yield out
    for _, ix in out.values():
        ix.close()


@pytest.mark.parametrize("metric", [COS, L2])
def test_u8_path_against_float64_and_bit_identical_to_fp32_path(big, metric):
    rows, ix = big[metric]
    for qi in range(2):
        q = _corpus(1, 128, metric, seed=100 + qi, scaled=metric == L2)[0]
        ref, _ = _reference(rows, q, metric)
        srt = np.sort(ref)[::-1] if metric == COS else np.sort(ref)
        for t in (float(srt[0]) + (0.5 if metric == COS else -0.5), float(srt[9]), float(srt[3000]), float(srt[30000])):
            ix.set_option("scan_shadow", 2)
            r, s = _one(ix, q, t)
            assert ix.get_option("last_range_path") == 2
            check(rows, q, t, metric, r, s)
            ix.set_option("scan_shadow", 0)
            r0, s0 = _one(ix, q, t)
            assert ix.get_option("last_range_path") == 0
            assert np.array_equal(r, r0) and np.array_equal(s.view(np.uint32), s0.view(np.uint32))
    ix.set_option("scan_shadow", 2)


def test_u8_path_agrees_with_top_k(big):
    rows, ix = big[COS]
    q = _corpus(1, 128, COS, seed=321)[0]
    idx, sc = ix.search(q, 150)
    assert ix.get_option("last_single_path") == 2
    t = float(sc[0][149])
    r, s = _one(ix, q, t)
    assert ix.get_option("last_range_path") == 2
    assert np.array_equal(r[:150], idx[0]) and np.array_equal(s[:150].view(np.uint32), sc[0].view(np.uint32))
    assert np.all(s[150:] == np.float32(t))


def test_minus_inf_returns_every_row_once_through_the_grown_buffers(big):
    rows, ix = big[COS]
    q = _corpus(1, 128, COS, seed=99)[0]
    before = ix.get_option("device_bytes_resident")
    r, s = _one(ix, q, -np.inf)
    assert ix.get_option("last_range_path") == 2
    assert len(r) == len(rows) and np.array_equal(np.sort(r), np.arange(len(rows)))
    check(rows, q, -np.inf, COS, r, s)
    assert ix.get_option("device_bytes_resident") > before  # (the candidate / result buffers grew to 200 000 keys)


# ---- 5. masks, tombstones, infinite elements ----------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
def test_mask_equals_unmasked_intersect_mask(big, metric):
    from wdbx_amd import _native

    rows, ix = big[metric]
    q = _corpus(1, 128, metric, seed=55, scaled=metric == L2)[0]
    ref, _ = _reference(rows, q, metric)
    t = float((np.sort(ref)[::-1] if metric == COS else np.sort(ref))[5000])
    allowed = np.random.default_rng(3).random(len(rows)) < 0.3
    for shadow in (2, 0):
        ix.set_option("scan_shadow", shadow)
        r, s = _one(ix, q, t)
        rm, sm = _one(ix, q, t, mask_words=_native.pack_row_mask(allowed))
        keep = allowed[r]
        assert np.array_equal(rm, r[keep]) and np.array_equal(sm.view(np.uint32), s[keep].view(np.uint32))
        check(rows, q, t, metric, rm, sm, allowed=allowed)
    ix.set_option("scan_shadow", 2)


@pytest.mark.parametrize("n", [5000, 140_000])
def test_removed_ids_never_appear_and_infinite_elements_follow_the_rule(n):
    from wdbx_amd.indexing import HipFlatIndex

    d = 64
    rows = _corpus(n, d, COS, seed=n)
    tmp = tempfile.mkdtemp()
    try:
        hx = HipFlatIndex(d, f"{tmp}/ix", config={"HIP_PERSIST_INDEX": False, "HIP_SWALLOW_ERRORS": False,
                                                  "HIP_CAPACITY_ROWS": n + 8})
        hx.add_rows([f"v{i}" for i in range(n)], rows)
        removed = [f"v{i}" for i in range(0, n, 7)]
        for vid in removed:
            assert hx.remove(vid)
        q = rows[1] + 0.1 * rows[2]
        q = q / np.linalg.norm(q)
        res = hx.range_search(q, -1.5)
        assert len(res) == n - len(removed)
        assert not set(removed) & {vid for vid, _ in res}
        assert [s for _, s in res] == sorted((s for _, s in res), reverse=True)
        # rows with +-inf elements: their fp32 score is +-inf (or NaN where an inf meets a zero): kept iff it reaches t
        inf_rows = np.zeros((3, d), np.float32)
        inf_rows[0, 0] = np.inf           # q[0] > 0: +inf
        inf_rows[1, 0] = -np.inf          # -inf: never reaches a finite t
        inf_rows[2, 0], inf_rows[2, 1] = np.inf, -np.inf   # inf - inf = NaN: never returned
        q2 = np.full(d, 1.0 / np.sqrt(d), np.float32)
        raw = hx._native
        base = raw.size()
        raw.add(inf_rows)
        for t in (0.5, -np.inf):
            _, r, s = raw.range_search(q2, [t])
            got = dict(zip(r.tolist(), s.tolist()))
            assert got.get(base) == np.inf
            assert (base + 1 in got) == (t == -np.inf) and base + 2 not in got
            assert all(rr < base or rr == base or rr == base + 1 for rr in got)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---- 6. several queries, the capacity protocol ----------------------------------------------------------------------------
def _raw(ix, qs, ts, capacity):
    from wdbx_amd import _native

    qs = np.ascontiguousarray(qs, np.float32)
    ts = np.ascontiguousarray(ts, np.float32)
    off = np.zeros(len(qs) + 1, np.uint64)
    rows = np.full(max(1, capacity), -5, np.int64)
    scores = np.zeros(max(1, capacity), np.float32)
    rc = ix._lib.wdbx_index_range_search(ix._h, qs.ctypes.data_as(_native._f32p), len(qs), ts.ctypes.data_as(_native._f32p),
                                         0, None, 0, capacity, off.ctypes.data_as(_native._u64p),
                                         rows.ctypes.data_as(_native._i64p), scores.ctypes.data_as(_native._f32p))
    return rc, off.astype(np.int64), rows, scores


@pytest.mark.parametrize("which", ["u8", "fp32"])
def test_several_queries_and_capacity(big, which):
    from wdbx_amd import _native

    rows, ix = big[COS]
    ix.set_option("scan_shadow", 2 if which == "u8" else 0)
    try:
        qs = np.stack([_corpus(1, 128, COS, seed=700 + i)[0] for i in range(70)])  # (two rounds of the library's 64)
        ts = np.linspace(0.45, 0.15, len(qs)).astype(np.float32)
        ts[3] = np.inf
        ts[4] = -np.inf
        off, r, s = ix.range_search(qs, ts)
        for i in (0, 3, 4, 40, 69):
            ri, si = _one(ix, qs[i], float(ts[i]))
            assert np.array_equal(r[off[i]:off[i + 1]], ri) and np.array_equal(s[off[i]:off[i + 1]].view(np.uint32), si.view(np.uint32))
        assert off[4] == off[3] and off[5] - off[4] == len(rows)
        total = int(off[-1])
        rc, off0, rows0, _ = _raw(ix, qs, ts, 0)
        assert rc == 0 and np.array_equal(off0, off) and np.all(rows0 == -5)
        rc, off1, _, _ = _raw(ix, qs, ts, total - 1)
        assert rc == 0 and np.array_equal(off1, off)
        rc, off2, r2, s2 = _raw(ix, qs, ts, total)
        assert rc == 0 and np.array_equal(r2, r) and np.array_equal(s2.view(np.uint32), s.view(np.uint32))
        with pytest.raises(_native.HipBackendError):
            ix.range_search(qs[:2], [0.5, np.nan])
    finally:
        ix.set_option("scan_shadow", 2)


# ---- 7. the facade ----------------------------------------------------------------------------------------------------------
def test_facade_store_and_endpoint():
    from wdbx_amd import WDBX
    from wdbx_amd.api import range_search_endpoint

    d, n = 48, 3000
    rows = _corpus(n, d, COS, seed=77)
    tmp = tempfile.mkdtemp()
    try:
        empty = WDBX(vector_dimension=d, num_shards=3, data_dir=f"{tmp}/e", enable_plugins=False)
        assert empty.vector_search_range(rows[0].tolist(), 0.0) == []
        asyncio.run(empty.shutdown())
        w = WDBX(vector_dimension=d, num_shards=3, data_dir=tmp, enable_plugins=False,
                 config={"WDBX_VECTOR_STORE_SAVE_IMMEDIATELY": False})
        ids = [f"doc{i}" for i in range(n)]
        meta = {vid: {"i": i, "tag": "a" if i % 3 == 0 else "b"} for i, vid in enumerate(ids)}
        assert w.vector_store.batch_store({vid: rows[i].tolist() for i, vid in enumerate(ids)}, meta) == n
        q = rows[10] + 0.5 * rows[20]
        ref = rows.astype(np.float64) @ (q / np.linalg.norm(q)).astype(np.float64)
        t = float(np.sort(ref)[-400])
        for flt in (None, {"tag": "a"}):
            got = w.vector_search_range(q.tolist(), t, filter_metadata=flt)
            allowed = np.array([flt is None or meta[v]["tag"] == "a" for v in ids])
            rws = np.array([int(g[0][3:]) for g in got])
            check(rows, q / np.linalg.norm(q), t, COS, rws, np.array([g[1] for g in got], np.float32), allowed=allowed)
            assert all(g[2] == meta[g[0]] for g in got)
            assert w.vector_search_range(q.tolist(), t, filter_metadata=flt, prefilter=True) == got
            assert w.vector_search_range(q.tolist(), t, filter_metadata=flt, max_results=7) == got[:7]
            assert asyncio.run(w.vector_search_range_async(q.tolist(), t, filter_metadata=flt)) == got
            body = {"query_vector": q.tolist(), "threshold": t, "filter_metadata": flt, "max_results": None}
            resp = asyncio.run(range_search_endpoint(w, body))
            assert resp == {"results": [{"vector_id": v, "similarity": s, "metadata": m} for v, s, m in got]}
        with pytest.raises(ValueError):
            w.vector_search_range([0.0] * (d + 1), 0.5)
        with pytest.raises(ValueError):
            w.vector_search([0.0] * (d + 1), limit=1)
        asyncio.run(w.shutdown())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---- 8. threads ------------------------------------------------------------------------------------------------------------
def test_threads_interleave_range_and_top_k_on_one_handle(big):
    rows, ix = big[COS]
    qs = [_corpus(1, 128, COS, seed=900 + i)[0] for i in range(8)]
    ts = [0.3 + 0.01 * i for i in range(8)]
    serial_range = [_one(ix, q, t) for q, t in zip(qs, ts)]
    serial_topk = [ix.search(q, 20) for q in qs]
    errors = []

    def worker(i):
        try:
            for rep in range(4):
                j = (i + rep) % 8
                r, s = _one(ix, qs[j], ts[j])
                idx, sc = ix.search(qs[j], 20)
                assert np.array_equal(r, serial_range[j][0]) and np.array_equal(s, serial_range[j][1])
                assert np.array_equal(idx, serial_topk[j][0]) and np.array_equal(sc, serial_topk[j][1])
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[:3]
