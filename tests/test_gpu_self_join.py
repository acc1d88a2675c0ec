"""The similarity self-join of the stored rows on the MI355X through the C ABI (wdbx_index_self_join): offsets, rows and score
bits against the composition the contract names -- wdbx_index_range_search per anchor with the stored row as the query, rows
<= anchor dropped -- and against a float64 numpy reference; planted duplicates across an anchor-block boundary, inside one
fragment, in the diagonal tile and first-with-last; thresholds an ulp either side of a pair's score; ineligible rows, capacity,
the candidate buffer's repair, the exact route, refusals and the empty index."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
SWEEP, EXACT = 1, 2
GAMMA = 2e-6
# exact duplicates: across a tile boundary and a 128-row anchor-block boundary, inside one 16-row fragment, two waves of the diagonal
# tile, the first row with the last
TWINS = [(255, 256), (127, 128), (33, 35), (300, 470), (0, -1)]


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


def _corpus(metric, d, n):
    """clusters of 8 rows around a centre, each row with a noise level of its own: the pairs' scores straddle the threshold"""
    rng = np.random.default_rng(4100 + 7 * d + n + metric)
    centres = rng.standard_normal((-(-n // 8), d))
    sigma = rng.uniform(0.05, 0.2, (n, 1))
    rows = (centres[rng.permutation(n) % len(centres)] + sigma * rng.standard_normal((n, d))).astype(np.float32)
    for a, b in TWINS:
        rows[b] = rows[a]
    return rows, (0.98 if metric == COS else 0.03 * d)


def _build(native, metric, d, n, kind="plain"):
    rows, thr = _corpus(metric, d, n)
    ix = native.NativeIndex(d, metric, 0, capacity_rows=n)
    ix.add(rows, normalize=metric == COS)
    if kind == "inf":  # (written as it is: normalising it would make it a NaN row)
        rows[70, 3] = np.inf
        ix.set_rows(70, rows[70:71])
    if kind == "removed":
        ix.remove_rows((256, 300, 999))
    if kind == "nan":
        ix.set_rows(33, np.full((1, d), np.nan, np.float32))
    allowed = np.random.default_rng(5).random(n) > 1 / 3 if kind == "mask" else np.ones(n, bool)
    ix.set_option("join_min_rows", 0)
    stored = ix.get_rows(0, n)
    return ix, stored, allowed, allowed & ~np.isnan(stored).any(axis=1), np.float32(thr)


def _composition(ix, stored, eligible, thr, mask):
    """the contract: per eligible anchor a range search with the stored row as the query, the rows <= a removed"""
    off, rows, scores = ix.range_search(stored, thr, normalize_queries=False, mask_words=mask)
    anchors = np.repeat(np.arange(len(stored)), np.diff(off))
    keep = (rows > anchors) & eligible[anchors]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(anchors[keep], minlength=len(stored)))])
    return offsets, rows[keep], scores[keep]


def _same(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)))


_REFERENCE = {}  # (metric, d, n) -> what does not depend on join_max_grid: computed once, never changed


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("n", [1000, 2700])
@pytest.mark.parametrize("d", [384, 100, 768, 1000])
@pytest.mark.parametrize("metric", [COS, L2])
def test_the_join_is_the_range_search_of_every_anchor(native, metric, d, n, grid):
    ix, stored, _, eligible, thr = _build(native, metric, d, n)
    with ix:
        ix.set_option("join_max_grid", grid)
        got = ix.self_join(thr)
        assert ix.get_option("last_join_path") == SWEEP and ix.get_option("last_join_blocks") == -(-n // (64 if d == 1000 else 128))
        print(f"candidates {ix.get_option('last_join_candidates')}, pairs {ix.get_option('last_join_pairs')}")
        assert _same(ix.self_join(thr), got)  # the same from run to run
        if (metric, d, n) not in _REFERENCE:
            # thresholds an ulp either side of a pair's own score: the weakest pair of the answer stays at its score and leaves above it
            edge = got[2].min() if metric == COS else got[2].max()
            beyond = np.nextafter(edge, np.float32(np.inf if metric == COS else -np.inf))
            _REFERENCE[(metric, d, n)] = {t.tobytes(): _composition(ix, stored, eligible, t, None) for t in (thr, edge, beyond)}
        ref = _REFERENCE[(metric, d, n)]
        for key, want in ref.items():
            t = np.frombuffer(key, np.float32)[0]
            assert _same(ix.self_join(t), want), t
        sizes = [len(w[1]) for w in ref.values()]
        assert sizes[0] >= sizes[1] > sizes[2] > 0
    offsets, rows, scores = got
    anchors = np.repeat(np.arange(n), np.diff(offsets))
    assert (rows > anchors).all()
    for a, b in TWINS:  # exact duplicates are pairs like any other
        assert b % n in rows[offsets[a]:offsets[a + 1]]
    # float64: every pair beyond exact_score's bound on either side of the threshold is present or absent as it must be
    x = stored.astype(np.float64)
    sq = (x * x).sum(1)
    if metric == COS:
        real = x @ x.T
        bound = GAMMA * np.sqrt(sq[:, None] * sq[None, :])
        inside, outside = real >= thr + bound, real < thr - bound
    else:
        real = np.maximum(sq[:, None] + sq[None, :] - 2 * x @ x.T, 0)
        bound = GAMMA * real + 1e-9 * sq.max()  # (exact_score's relative bound; the expanded float64 form's own cancellation)
        inside, outside = real <= thr - bound, real > thr + bound
    have = np.zeros((n, n), bool)
    have[anchors, rows] = True
    upper = np.triu(np.ones((n, n), bool), 1)
    assert have[inside & upper].all() and not have[outside & upper].any() and not have[~upper].any()


@pytest.mark.parametrize("kind", ["mask", "removed", "nan", "inf"])
@pytest.mark.parametrize("metric", [COS, L2])
def test_ineligible_rows_have_no_segment_and_appear_in_none(native, metric, kind):
    n = 1000
    ix, stored, allowed, eligible, thr = _build(native, metric, 100, n, kind)
    with ix:
        mask = native.pack_row_mask(allowed) if kind == "mask" else None
        got = ix.self_join(thr, mask=mask)
        assert ix.get_option("last_join_path") == SWEEP
        assert _same(got, _composition(ix, stored, eligible, thr, mask))
    dead = np.flatnonzero(~eligible)
    assert len(got[1]) > 0 and (np.diff(got[0])[dead] == 0).all() and not np.isin(got[1], dead).any()
    assert (kind in ("removed", "nan", "mask")) == (len(dead) > 0)


def test_capacity_repair_exact_route_refusals_and_the_empty_index(native):
    n = 2700
    ix, stored, _, eligible, thr = _build(native, COS, 100, n)
    with ix:
        want = ix.self_join(thr)
        total = len(want[1])
        reruns = ix.get_option("last_join_reruns")
        # count only, one short of the answer, exactly the answer
        for cap in (0, total - 1, total):
            got = ix.self_join(thr, capacity=cap)
            assert np.array_equal(got[0], want[0]) and len(got[1]) == (total if cap == total else 0)
        assert _same(ix.self_join(thr, capacity=total), want)
        # the candidate buffer's repair: a first buffer of 64 pairs is grown to the exact count and the sweep runs once more
        ix.set_option("join_pair_cap", 64)
        assert _same(ix.self_join(thr), want)
        assert reruns == 0 and ix.get_option("last_join_reruns") == 1 and ix.get_option("last_join_candidates") > 64
        ix.set_option("join_pair_cap", 0)
        # the exact route gives the sweep's answer
        ix.set_option("join_min_rows", 1 << 30)
        assert _same(ix.self_join(thr), want) and ix.get_option("last_join_path") == EXACT
        # refusals leave the handle usable
        ix.set_option("join_exact_max_rows", n - 1)
        with pytest.raises(native.HipBackendError, match="join_min_rows"):
            ix.self_join(thr)
        ix.set_option("join_min_rows", 0)
        with pytest.raises(native.HipBackendError):
            ix.self_join(np.nan)
        with pytest.raises(native.HipBackendError):
            ix.self_join(thr, mask=native.pack_row_mask(np.ones(n, bool))[:-1])
        assert ix._lib.wdbx_index_self_join(ix._h, float(thr), None, 0, 0, None, None, None) != 0
        offsets = np.zeros(n + 1, np.uint64)
        assert ix._lib.wdbx_index_self_join(ix._h, float(thr), None, 0, 8, offsets.ctypes.data_as(native._u64p), None, None) != 0
        assert _same(ix.self_join(thr), want) and ix.get_option("last_join_path") == SWEEP
    with native.NativeIndex(100, COS, 0, capacity_rows=16) as empty:
        got = empty.self_join(thr)
        assert got[0].tolist() == [0] and len(got[1]) == 0
        assert empty.get_option("last_join_path") == 0 and empty.get_option("last_join_launches") == 0
