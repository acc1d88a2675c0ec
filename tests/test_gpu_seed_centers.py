"""k-means++ seeding on the MI355X through the C ABI (wdbx_index_seed_centers): chosen rows and potentials, entry for entry,
against a plain loop over Python integers.  Exact-arithmetic corpora (elements from {-2..2}/8 for cosine, {-3..3} for L2, stored
with normalize=0) make every dot product and squared distance exact in fp32 and float64 alike, so the reference's weights ARE the
device's; one real-valued corpus takes each centre's scores from wdbx_index_search_rows, whose bits the contract names.  Mask,
removed rows, the all-duplicates fallback, several candidate chunks, refusals."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
SAT = 2 ** 31 - 1


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


def exact_weights(metric, rows64, eligible):
    """c -> every row's weight against stored row c, in float64 (exact for these corpora)"""
    shift = 0
    if metric == L2:
        big = float((rows64[eligible] ** 2).sum(axis=1).max())
        shift = 100 if big == 0 else max(-100, min(100, 29 - math.frexp(big)[1]))

    def against(c):
        if metric == COS:
            return np.floor(np.clip(1.0 - rows64 @ rows64[c], 0.0, 2.0) * 2.0 ** 30).astype(np.int64)
        return np.minimum(np.floor(((rows64 - rows64[c]) ** 2).sum(axis=1) * 2.0 ** shift), SAT).astype(np.int64)
    return against, shift


def reference(against, eligible, draws, n_centers, n_trials):
    """the contract as a loop: (rows, potentials)"""
    live, w, rows, pots = eligible.copy(), None, [], []
    for c in range(n_centers):
        sampling = np.where(live, w, 0) if c and int(w[live].sum()) else live.astype(np.int64)
        cum, best = np.cumsum(sampling), None
        for j in range(n_trials if c else 1):
            r = int(np.searchsorted(cum, (int(draws[c * n_trials + j]) * int(cum[-1])) >> 64, side="right"))
            wj = np.where(live, against(r), 0)
            wj[r] = 0
            cur = wj if w is None else np.minimum(w, wj)
            if best is None or int(cur.sum()) < best[0]:
                best = (int(cur.sum()), r, cur)
        w = best[2]
        live[best[1]] = False
        rows.append(best[1])
        pots.append(best[0])
    return rows, pots


def exact_corpus(native, metric, n, d, distinct=None):
    rng = np.random.default_rng(100 * n + d + metric)
    if metric == COS and distinct:  # unit vectors with exact products: four entries of +-1/2 (a duplicate of a centre then weighs 0)
        rows = np.zeros((distinct, d), np.float32)
        for v in rows:
            v[rng.choice(d, 4, replace=False)] = rng.choice([-0.5, 0.5], 4)
    elif metric == COS:
        rows = rng.integers(-2, 3, (distinct or n, d)).astype(np.float32) / 8
    else:
        rows = rng.integers(-3, 4, (distinct or n, d)).astype(np.float32)
    rows = rows[np.arange(n) % len(rows)]
    ix = native.NativeIndex(d, metric, 0, capacity_rows=n)
    ix.add(rows, normalize=False)
    return ix, rows.astype(np.float64)


def draws_for(n_centers, n_trials, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 64, n_centers * n_trials, dtype=np.uint64)


def words(allowed):
    return np.packbits(np.pad(allowed, (0, -len(allowed) % 32)), bitorder="little").view(np.uint32)


@pytest.fixture(scope="module")
def corpora(native):
    """one index per (metric, shape), shared by the cases over trials and centres"""
    made = {}

    def get(metric, n, d):
        if (metric, n, d) not in made:
            made[metric, n, d] = exact_corpus(native, metric, n, d)
        return made[metric, n, d]
    yield get
    for ix, _ in made.values():
        ix.close()


@pytest.mark.parametrize("n_centers", [1, 40])
@pytest.mark.parametrize("n_trials", [1, 3, 16])
@pytest.mark.parametrize("n,d", [(70, 32), (1025, 32), (2500, 384)])
@pytest.mark.parametrize("metric", [COS, L2])
def test_rows_and_potentials_equal_the_integer_loop(corpora, metric, n, d, n_trials, n_centers):
    ix, rows64 = corpora(metric, n, d)
    eligible = np.ones(n, bool)
    against, shift = exact_weights(metric, rows64, eligible)
    draws = draws_for(n_centers, n_trials, 7 * n + n_trials)
    got_rows, got_pot = ix.seed_centers(n_centers, draws, n_trials)
    want_rows, want_pot = reference(against, eligible, draws, n_centers, n_trials)
    assert got_rows.tolist() == want_rows and got_pot.tolist() == want_pot
    assert ix.get_option("last_seed_passes") == 1 and ix.get_option("last_seed_launches") == 1 + 3 * n_centers
    if metric == L2:
        assert ix.get_option("last_seed_shift") == shift


@pytest.mark.parametrize("metric,case", [(COS, "mask"), (L2, "removed"), (COS, "duplicates"), (L2, "duplicates"), (L2, "chunks")])
def test_mask_removed_rows_duplicates_and_candidate_chunks(native, metric, case):
    n, d, n_trials, n_centers = (70 if case == "duplicates" else 1025), 32, (5 if case == "chunks" else 3), 40
    ix, rows64 = exact_corpus(native, metric, n, d, distinct=8 if case == "duplicates" else None)
    eligible, mask = np.ones(n, bool), None
    if case == "mask":
        eligible = np.random.default_rng(3).random(n) > 1 / 3
        mask = words(eligible)
    if case == "removed":
        gone = np.arange(3, n, 7)
        ix.remove_rows(gone)
        eligible[gone] = False
    if case == "duplicates":
        n_centers = 12  # more centres than distinct vectors: from the ninth on every weight is 0 and the draws fall back to 1 per row
    if case == "chunks":
        ix.set_option("seed_max_resident", 2)
    against, _ = exact_weights(metric, np.nan_to_num(rows64), eligible)
    draws = draws_for(n_centers, n_trials, 11)
    got_rows, got_pot = ix.seed_centers(n_centers, draws, n_trials, mask=mask)
    want_rows, want_pot = reference(against, eligible, draws, n_centers, n_trials)
    assert got_rows.tolist() == want_rows and got_pot.tolist() == want_pot
    assert len(set(want_rows)) == n_centers and eligible[want_rows].all()
    if case == "duplicates":
        assert want_pot[8:] == [0] * 4
    if case == "chunks":
        assert ix.get_option("last_seed_passes") == 3 and ix.get_option("last_seed_launches") == 1 + 3 + 39 * 5
    ix.close()


@pytest.mark.parametrize("metric", [COS, L2])
def test_real_vectors_weigh_what_search_rows_scores(native, metric):
    n, d, n_centers, n_trials = 1500, 96, 20, 3
    raw = np.random.default_rng(5).standard_normal((n, d)).astype(np.float32)
    ix = native.NativeIndex(d, metric, 0, capacity_rows=n)
    ix.add(raw, normalize=True)
    stored, everything = ix.get_rows(0, n), np.arange(n)
    draws = draws_for(n_centers, n_trials, 13)
    got_rows, got_pot = ix.seed_centers(n_centers, draws, n_trials)
    shift = ix.get_option("last_seed_shift")
    assert metric == COS or shift in (28, 29)  # unit rows: the largest squared norm is within an ulp of 1

    def against(c):  # the contract's own words: the bits search_rows returns with stored row c as the query
        idx, score = ix.search_rows(stored[c], n, everything)
        s = np.empty(n, np.float32)
        s[idx[0]] = score[0]
        if metric == COS:
            return (np.clip(np.float32(1) - s, np.float32(0), np.float32(2)) * np.float32(2 ** 30)).astype(np.int64)
        return np.minimum(np.ldexp(s, shift).astype(np.float64), SAT).astype(np.int64)
    want_rows, want_pot = reference(against, np.ones(n, bool), draws, n_centers, n_trials)
    assert got_rows.tolist() == want_rows and got_pot.tolist() == want_pot
    ix.close()


def test_refusals_leave_the_handle_usable(native, corpora):
    import ctypes as C

    ix, rows64 = corpora(COS, 70, 32)
    draws = draws_for(4, 2, 1)
    three = np.zeros(70, bool)
    three[[4, 9, 60]] = True
    refused = [lambda: ix.seed_centers(0, draws[:0], 2), lambda: ix.seed_centers(native.MAX_CENTERS + 1, np.zeros(2 * 4097, np.uint64), 2),
               lambda: ix.seed_centers(4, draws[:0], 0), lambda: ix.seed_centers(4, np.zeros(4 * 17, np.uint64), 17),
               lambda: ix.seed_centers(4, draws, 2, mask=np.ones(2, np.uint32)), lambda: ix.seed_centers(4, draws, 2, mask=words(three)),
               lambda: ix.seed_centers(71, np.zeros(142, np.uint64), 2)]
    empty = native.NativeIndex(32, COS, 0, capacity_rows=8)
    refused.append(lambda: empty.seed_centers(1, draws[:1], 1))
    for call in refused:
        with pytest.raises(native.HipBackendError) as e:
            call()
        assert e.value.code == -1  # WDBX_E_INVALID
    out = np.zeros(4, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    lib = native.load_library()
    assert lib.wdbx_index_seed_centers(ix._h, 4, 2, None, None, 0, out.ctypes.data_as(u64p), None) == -1
    assert lib.wdbx_index_seed_centers(ix._h, 4, 2, draws.ctypes.data_as(u64p), None, 0, None, None) == -1
    empty.close()
    against, _ = exact_weights(COS, rows64, np.ones(70, bool))
    got_rows, got_pot = ix.seed_centers(4, draws, 2)
    assert (got_rows.tolist(), got_pot.tolist()) == reference(against, np.ones(70, bool), draws, 4, 2)
