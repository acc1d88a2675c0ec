"""The k-NN graph of the stored rows on the MI355X through the C ABI (wdbx_index_knn_graph): every line against
wdbx_index_search_matrix over the list of all eligible rows -- ids and score bits, whole arrays -- and against a float64 numpy
ranking; duplicates beyond k, removed and NaN rows, huge and infinite norms, rows below bf16 resolution of one another, rows in
ascending similarity, both routes, run-to-run identity, refusals and the device bytes of the call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
TILES, REPAIR = 1, 2
COPIES = np.arange(5, 5 + 80 * 3, 3)  # 80 rows holding one vector: more than WDBX_MAX_GRAPH_K duplicates
NEAR = np.arange(250, 266)            # rows that differ from one another far below bf16 resolution (2^-8)
GONE, NAN_ROW, BIG = (19, 21), 22, 30

# metric, d, n, k, masked, data: "plain" (copies, near block, removed rows, a NaN row), "sorted" (ascending similarity to row 0),
# "huge" (plain + a row of norm 1e15 sqrt(d)), "inf" (huge + a row with an infinite element)
CASES = [
    (COS, 20, 300, 10, False, "plain"), (L2, 20, 300, 64, True, "plain"), (COS, 384, 300, 1, True, "plain"),
    (L2, 770, 300, 10, False, "plain"), (COS, 384, 1000, 10, False, "plain"), (L2, 384, 1000, 10, True, "plain"),
    (L2, 20, 1000, 1, False, "plain"), (COS, 770, 1000, 64, False, "plain"), (L2, 770, 1000, 1, True, "plain"),
    (COS, 384, 1000, 64, False, "plain"), (COS, 770, 2700, 1, False, "plain"), (L2, 770, 2700, 64, False, "plain"),
    (COS, 20, 2700, 64, True, "plain"), (COS, 384, 2700, 10, True, "plain"), (L2, 384, 2700, 10, False, "plain"),
    (L2, 384, 2700, 64, True, "plain"), (COS, 770, 2700, 10, True, "plain"),
    (COS, 384, 2700, 10, False, "sorted"), (L2, 384, 2700, 10, False, "sorted"), (COS, 20, 1000, 64, False, "sorted"),
    (COS, 20, 1000, 10, True, "sorted"),
    (L2, 384, 1000, 10, False, "huge"), (L2, 20, 2700, 10, True, "huge"), (L2, 384, 1000, 10, False, "inf"),
    # fewer eligible neighbours than k: lines padded with -1 / 0 (the repair route's: from 512 eligible rows on no line is short)
    (L2, 20, 40, 64, False, "sorted"),
]
# the same with the sweep's grid capped (set_option "knn_max_grid"): n = 1000 is 8 anchor tiles in passes of 3, 3 and 2 (the
# last one ragged), n = 2700 is 22 in passes of 5, 5, 5, 5 and 2; "huge" flags every anchor of every pass
CAPPED = [(COS, 384, 1000, 10, False, "plain", 3), (L2, 20, 2700, 64, True, "plain", 5), (L2, 384, 1000, 10, False, "huge", 3)]


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


def _build(native, metric, d, n, masked, data):
    """the index, what it stores (read back), the allowed rows and the eligible ones"""
    rng = np.random.default_rng(9000 + 7 * d + n + metric)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    if data == "sorted":
        sim = rows @ rows[0] if metric == COS else -((rows - rows[0]) ** 2).sum(axis=1)
        rows[1:] = rows[1:][np.argsort(sim[1:], kind="stable")]
    else:
        rows[COPIES] = rows[COPIES[0]]
        rows[NEAR] = rows[NEAR[0]] * (1 + 1e-5 * rng.standard_normal((len(NEAR), d))).astype(np.float32)
    if data in ("huge", "inf"):
        rows[BIG] *= np.float32(1e15)
    if data == "inf":
        rows[BIG + 1, 3] = np.inf
    ix = native.NativeIndex(d, metric, 0, capacity_rows=n)
    ix.add(rows, normalize=metric == COS)
    if data != "sorted":
        ix.remove_rows(GONE)
        ix.set_rows(NAN_ROW, np.full((1, d), np.nan, np.float32))
    allowed = rng.random(n) > 1 / 3 if masked else np.ones(n, bool)
    stored = ix.get_rows(0, n)
    eligible = np.flatnonzero(allowed & ~np.isnan(stored).any(axis=1))
    return ix, stored, allowed, eligible


@pytest.mark.parametrize("metric,d,n,k,masked,data,grid", [c + (0,) for c in CASES] + CAPPED)
def test_every_line_is_the_distance_matrix_over_all_eligible_rows(native, metric, d, n, k, masked, data, grid):
    ix, stored, allowed, eligible = _build(native, metric, d, n, masked, data)
    with ix:
        ix.set_option("knn_max_grid", grid)
        before = ix.get_option("device_bytes_resident")
        mask = native.pack_row_mask(allowed) if masked else None
        got = ix.knn_graph(k, mask=mask)
        path, repaired, passes = (ix.get_option("last_knn_" + o) for o in ("path", "repaired", "passes"))
        print(f"path {path}, passes {passes}, repaired {repaired} of {len(eligible)}, appends {ix.get_option('last_knn_appends')}")
        after = ix.get_option("device_bytes_resident")
        again = ix.knn_graph(k, mask=mask)
        want = np.full((n, k), -1, np.int64), np.zeros((n, k), np.float32)
        want[0][eligible], want[1][eligible] = ix.search_matrix(eligible.astype(np.uint64), k)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
    assert (got[0] == want[0]).all() and (got[1].view(np.uint32) == want[1].view(np.uint32)).all()
    # which route ran, and what it left on the device
    assert path == (TILES if len(eligible) >= 512 and data != "inf" else REPAIR)
    if path == TILES:
        tiles = -(-n // 128)
        assert passes == (-(-tiles // grid) if grid else 1)  # (uncapped, every case here is one launch)
        assert after - before >= (grid or tiles) * 128 * (k + 128) * 8  # the lists are the handle's, counted where every buffer is
        # (an eligible huge norm makes every anchor's bound useless: every list overflows.  Sorted rows: row 0's threshold follows
        # the dense middle of the scores, where more rows than a list holds lie within the margin -- flagged, never silent)
        if data != "sorted":
            assert repaired == (len(eligible) if data == "huge" and allowed[BIG] else 0)
    else:
        assert repaired == len(eligible) > 0
    # nobody lists itself or a row without a line; rows without a line have none
    dead = np.setdiff1d(np.arange(n), eligible)
    assert (got[0] != np.arange(n)[:, None]).all() and not np.isin(got[0], dead).any()
    assert (got[0][dead] == -1).all() and (got[1][dead] == 0).all()
    assert ((got[0][eligible] >= 0).sum(axis=1) == min(k, len(eligible) - 1)).all()
    if data == "plain" and not masked:
        assert np.isin(got[0][COPIES][:, : min(k, 79)], COPIES).all()  # each copy gets k of the 79 others, never itself
    if data in ("plain", "sorted"):  # (not "huge" / "inf": the bound scales with the largest norm, 1e30 d, or is not finite)
        # float64 ranking of what is stored: ids wherever the neighbouring gaps exceed twice exact_score's bound b_E
        # (gamma |a||c|, L2: gamma (|a| + |c|)^2, gamma = 1.05 (pitch + 18) 2^-24), scores within b_E
        x = stored[eligible].astype(np.float64)
        s = x @ x.T if metric == COS else -((x * x).sum(1)[:, None] + (x * x).sum(1)[None, :] - 2 * x @ x.T)
        np.fill_diagonal(s, -np.inf)
        m2 = (x * x).sum(1).max()
        b_e = 1.05 * ((d + 3) // 4 * 4 + 18) * 2.0 ** -24 * (m2 if metric == COS else 4 * m2)
        if metric == L2:
            b_e += 64 * 2.0 ** -53 * 4 * m2 * d  # (the expanded float64 form's own cancellation, far below b_E)
        kk = min(k, len(eligible) - 1)
        order = np.argsort(-s, axis=1, kind="stable")[:, : kk + 1]
        top = np.take_along_axis(s, order, axis=1)
        gap = top[:, :-1] - top[:, 1:] > 2 * b_e  # gap[:, j]: between rank j and rank j + 1
        sure = gap.copy()
        sure[:, 1:] &= gap[:, :-1]
        mine = got[0][eligible]
        assert (mine[:, :kk][sure] == eligible[order[:, :kk]][sure]).all()
        pos = np.searchsorted(eligible, np.where(mine >= 0, mine, eligible[0]))
        ref = np.take_along_axis(s, pos, axis=1)
        mine_s = got[1][eligible].astype(np.float64) * (1 if metric == COS else -1)
        assert (np.abs(mine_s - ref)[mine >= 0] <= b_e).all()


def test_refusals_leave_the_handle_usable(native):
    ix, _, allowed, _ = _build(native, COS, 20, 1000, True, "plain")
    with ix:
        mask = native.pack_row_mask(allowed)
        first = ix.knn_graph(10, mask=mask)
        for bad_k in (0, 65):
            with pytest.raises(native.HipBackendError):
                ix.knn_graph(bad_k, mask=mask)
        with pytest.raises(native.HipBackendError):
            ix.knn_graph(10, mask=mask[:-1])
        assert ix._lib.wdbx_index_knn_graph(ix._h, 10, None, 0, None, None) != 0
        again = ix.knn_graph(10, mask=mask)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
        assert ix.get_option("last_knn_launches") >= 3 and ix.get_option("last_knn_passes") == 1
