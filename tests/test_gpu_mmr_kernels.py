"""The two kernels of wdbx_index_search_mmr ALONE on the MI355X (tests/kernel_harness/mmr_harness.hip through
tests/mmr_harness.py): mmr_pairs_kernel -- every word of the similarity squares with guard words in front and behind, integer
corpora ``==`` an int64 reference, float corpora inside the float64 band and bit-equal to rescore_kernel, every square equal
to its transpose bit for bit -- and mmr_select_kernel on synthetic squares against the numpy float32 loop of the contract,
every output word compared, unused slots and guards included."""
import numpy as np
import pytest

import listed_harness as LH
import mmr_harness as MH
import select_harness as SH

pytestmark = pytest.mark.gpu

COS, L2 = SH.METRIC_COSINE, SH.METRIC_L2
_U32, _F32 = np.uint32, np.float32
POOLS = [1, 2, 7, 8, 9, 63, 64, 65, 257]  # one launch: nine queries with different pools
FRONT = 64


def _pad4(x):
    pad = (-x.shape[1]) % 4
    return np.pad(x, ((0, 0), (0, pad))) if pad else x


def _symmetric(g):
    """G == G.T bit for bit; a NaN similarity is a NaN both ways (its sign and payload are nobody's contract)"""
    nan = np.isnan(g)
    return np.array_equal(nan, nan.T) and np.array_equal(g.view(_U32)[~nan], g.T.view(_U32)[~nan])


def _check_frame(buf, front, words):
    assert np.array_equal(buf[:front].view(_U32), np.full(front, MH.SENT_G, _F32).view(_U32)), "words in front of G were written"
    assert np.array_equal(buf[front + words:].view(_U32), np.full(MH.GUARD, MH.SENT_G, _F32).view(_U32)), "words behind G were written"


# ---- pairs kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [3, 384, 516, 1028])  # pitch4 = 1, 96, 129, 257: NI = 2, 2, 4 and the loop
def test_pairs_on_integer_corpora_equal_int64(d, metric):
    rng = np.random.default_rng(7000 + d + metric)
    rows = rng.integers(-2, 3, size=(sum(POOLS), d)).astype(np.int64)
    buf = MH.pairs(metric, _pad4(rows.astype(_F32)), POOLS, front=FRONT)
    words = sum(m * m for m in POOLS)
    _check_frame(buf, FRONT, words)
    at = 0
    for m, g in zip(POOLS, MH.squares(buf[FRONT:FRONT + words], POOLS)):
        r = rows[at:at + m]
        want = r @ r.T if metric == COS else -((r[:, None, :] - r[None, :, :]) ** 2).sum(axis=2)
        assert np.abs(want).max() < 2 ** 24
        assert np.array_equal(g.astype(np.int64), want) and not np.isnan(g).any(), (d, metric, m)
        assert np.array_equal(g.view(_U32), g.T.view(_U32)), (d, metric, m)
        at += m


@pytest.mark.parametrize("metric", [COS, L2])
@pytest.mark.parametrize("d", [384, 516, 1028])
def test_pairs_on_float_corpora_against_float64_and_rescore(d, metric):
    rng = np.random.default_rng(7100 + d + metric)
    pools = [65, 257]
    rows = rng.standard_normal((sum(pools), d)).astype(_F32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows[3, 5] = np.nan  # a NaN element: its row's similarities are NaN, nobody else's
    rows = _pad4(rows.astype(_F32))
    pitch4 = rows.shape[1] // 4
    buf = MH.pairs(metric, rows, pools, front=FRONT)
    words = sum(m * m for m in pools)
    _check_frame(buf, FRONT, words)
    at = 0
    for m, g in zip(pools, MH.squares(buf[FRONT:FRONT + words], pools)):
        r = rows[at:at + m]
        s64, bound = LH.score64(r, r, metric), LH.score_bound64(r, r, metric, pitch4)
        nan = np.isnan(s64)
        assert np.array_equal(np.isnan(g), nan)
        err = np.abs(g.astype(np.float64) - s64)[~nan]
        print(f"d={d} metric={metric} m={m}: worst error / bound = {(err / np.maximum(bound[~nan], 1e-300)).max():.3f}")
        assert (err <= bound[~nan]).all()
        assert _symmetric(g)
        # rescore_kernel on the same operands: query j against every row i -> key(score + 0.0f, i)
        cand = np.broadcast_to(SH.make_keys(np.zeros(m, _U32), np.arange(m)), (m, m))
        keys, _ = SH.rescore(metric, r, r, cand, np.full(m, m, _U32))
        want = LH.key_scores(keys)  # [j, i]
        ok = ~nan.T
        with np.errstate(invalid="ignore"):
            mine = (g.T + _F32(0.0)).astype(_F32)  # (a key carries score + 0.0f: L2's -0.0 of a row against itself)
        assert np.array_equal(mine[ok].view(_U32), want[ok].view(_U32))
        assert np.array_equal(keys == 0, nan.T)
        at += m


# ---- select kernel -----------------------------------------------------------------------------------------------------------
def _synthetic(rng, ms, special=True):
    """symmetric squares with a unit diagonal, relevances descending; one NaN and one +inf similarity per large square"""
    G, rel = [], []
    for m in ms:
        g = rng.uniform(-1, 1, size=(m, m)).astype(_F32)
        g = np.triu(g) + np.triu(g, 1).T
        np.fill_diagonal(g, 1.0)
        if special and m >= 255:
            g[2, 5] = g[5, 2] = np.nan
            g[1, 9] = g[9, 1] = np.inf
            g[4, 7] = g[7, 4] = -np.inf
        G.append(g.reshape(-1))
        rel.append(np.sort(rng.uniform(0.2, 1, size=m).astype(_F32))[::-1])
    return np.concatenate(G).astype(_F32), np.concatenate(rel).astype(_F32)


SELECT_POOLS = [1, 255, 256, 257, 2048]
_SYN = {}


def _shared():
    if not _SYN:
        rng = np.random.default_rng(7200)
        G, rel = _synthetic(rng, SELECT_POOLS)
        cand = rng.permutation(1 << 20)[:sum(SELECT_POOLS)].astype(np.uint64)
        _SYN["v"] = (G, rel, cand)
    return _SYN["v"]


def _compare(got, want, what):
    (gi, gs, gm), (wi, ws, wm) = got, want
    assert np.array_equal(gi, wi), (what, "rows", np.flatnonzero(gi != wi)[:5])
    assert MH.same_f32(gs, ws, "scores") is None, (what, MH.same_f32(gs, ws, "scores"))
    if gm is not None:
        assert MH.same_f32(gm, wm, "values") is None, (what, MH.same_f32(gm, wm, "values"))


@pytest.mark.parametrize("k", [1, 255, 2048])  # k = 1; k = m for 255, above m for 1, below the rest; k = m for 2048, above the rest
@pytest.mark.parametrize("lam", [0.0, 0.25, 0.5, 1.0])
def test_select_equals_the_float32_loop(lam, k):
    G, rel, cand = _shared()
    for negate in ((False, True) if k == 255 else (False,)):
        got = MH.select(SELECT_POOLS, G, cand, rel, lam, k, negate=negate)
        want = MH.expect_select(SELECT_POOLS, G, cand, rel, lam, k, negate, greedy=MH.greedy_fast_f32)
        _compare(got, want, (lam, k, negate))


def test_the_fast_reference_is_the_plain_loop():
    G, rel, cand = _shared()
    ms = SELECT_POOLS[:4]
    n, g = sum(ms), sum(m * m for m in ms)
    for lam in (0.0, 0.5, 1.0):
        a = MH.expect_select(ms, G[:g], cand[:n], rel[:n], lam, 40, False, greedy=MH.greedy_f32)
        b = MH.expect_select(ms, G[:g], cand[:n], rel[:n], lam, 40, False, greedy=MH.greedy_fast_f32)
        _compare(a, b, lam)


@pytest.mark.parametrize("lam", [0.0, 0.25, 0.5, 1.0])
def test_exact_ties_are_picked_in_position_order(lam):
    ms = [257, 2048, 9]
    G = np.full(sum(m * m for m in ms), 0.5, _F32)
    rel = np.full(sum(ms), 0.75, _F32)
    cand = (np.arange(sum(ms)) * 3 + 1).astype(np.uint64)
    for k in (1, 300, 2048):
        idx, score, mmr = MH.select(ms, G, cand, rel, lam, k)
        row0 = 0
        for q, m in enumerate(ms):
            n = min(k, m)
            assert np.array_equal(idx[q * k:q * k + n], cand[row0:row0 + n].astype(np.int64)), (lam, k, m)
            assert (idx[q * k + n:(q + 1) * k] == -1).all()
            row0 += m
        _compare((idx, score, mmr), MH.expect_select(ms, G, cand, rel, lam, k, False, greedy=MH.greedy_fast_f32), (lam, k))


def test_select_without_a_value_array_and_with_empty_pools():
    rng = np.random.default_rng(7300)
    ms = [0, 40, 0, 1, 0]
    G, rel = _synthetic(rng, ms, special=False)
    cand = rng.permutation(1000)[:sum(ms)].astype(np.uint64)
    for k in (1, 10, 300):
        got = MH.select(ms, G, cand, rel, 0.5, k, with_mmr=False)
        want = MH.expect_select(ms, G, cand, rel, 0.5, k, False)
        assert got[2] is None
        _compare(got, want, k)


def test_nan_values_rank_below_numbers_and_by_position():
    # lambda = 1 leaves (1 - lambda) (x) maxsim = 0 (x) inf = NaN for every candidate whose maxsim is infinite
    m = 12
    g = np.full((m, m), 0.25, _F32)
    g[0, [3, 4, 8]] = np.inf
    g[[3, 4, 8], 0] = np.inf
    rel = np.linspace(1.0, 0.5, m).astype(_F32)
    cand = np.arange(100, 100 + m).astype(np.uint64)
    got = MH.select([m], g.reshape(-1), cand, rel, 1.0, m)
    want = MH.expect_select([m], g.reshape(-1), cand, rel, 1.0, m, False)
    _compare(got, want, "nan")
    assert got[0][:m].tolist() == [100, 101, 102, 105, 106, 107, 109, 110, 111, 103, 104, 108]
    assert np.isnan(got[2][m - 3:m]).all() and not np.isnan(got[2][:m - 3]).any()


def test_harness_refuses_what_would_leave_the_arrays():
    lib = MH.load()
    table = np.ascontiguousarray(MH.table_of([4]))
    G, cand, rel = np.zeros(15, _F32), np.zeros(4, np.uint64), np.zeros(4, _F32)  # a square one word short
    idx, score = np.zeros(8, np.int64), np.zeros(8, _F32)
    rc = lib.mmr_select(MH._ptr(table), 1, MH._ptr(G), G.size, MH._ptr(cand), MH._ptr(rel), 4, MH._ptr(idx), MH._ptr(score), None, 8,
                        0.5, 8, 0)
    assert rc == -1
    rows = np.zeros((3, 4), _F32)  # a row short
    rc = lib.mmr_pairs(0, MH._ptr(rows), 3, 1, MH._ptr(table), 1, MH._ptr(np.zeros(16, _F32)), 16)
    assert rc == -1
