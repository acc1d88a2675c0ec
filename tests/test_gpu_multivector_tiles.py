"""The matrix-core scoring route of the multi-vector search on the MI355X (option ``multivector_tiles``, label_keys_tile_kernel):
1. integer corpora, where every fp32 product and sum is exact: ids, scores and labels ``==`` a float64 numpy MaxSim reference;
2. float corpora: ids and score bits equal to the same call on the vector-ALU route (``multivector_tiles = 0``), with masks,
removed rows, NaN, inf and a zero vector; 3. exact ties and one-ulp neighbours are left to the exact arithmetic and counted;
4. the option's range, and an L2 handle keeps the old route."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COS, L2 = 0, 1
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


def _index(native, rows, labels, metric=COS):
    ix = native.NativeIndex(rows.shape[1], metric, 0, capacity_rows=len(rows))
    ix.add(rows.astype(np.float32), normalize=False)
    ix.set_labels(0, labels.astype(np.uint32))
    return ix


def _search(ix, tiles, vectors, offsets, k, mask_words=None):
    """-> ((ids, score bits, labels), tile rounds of the call)"""
    ix.set_option("multivector_tiles", tiles)
    idx, sc, lb = ix.search_multivector(vectors.astype(np.float32), offsets, k, mask_words=mask_words)
    return (idx, np.ascontiguousarray(sc, np.float32).view(np.uint32), lb), ix.get_option("last_multivector_tile_rounds")


def _same(ix, vectors, offsets, k, what, mask_words=None):
    """the tile route against the vector-ALU route of the same handle: ids, score bits, labels"""
    got, rounds = _search(ix, 1, vectors, offsets, k, mask_words)
    want, old_rounds = _search(ix, 0, vectors, offsets, k, mask_words)
    assert rounds >= 1 and old_rounds == 0, what
    for g, w in zip(got, want):
        assert np.array_equal(g, w), what


def _maxsim(vectors, offsets, rows, labels, k):
    """float64 MaxSim: per query the labels by (sum over its vectors of the best score among the label's rows) descending, label
    value ascending; a label is reported as (its smallest row, the sum, its value)"""
    values, row0, dense = np.unique(labels, return_index=True, return_inverse=True)
    score = vectors.astype(np.float64) @ rows.astype(np.float64).T
    best = np.full((len(vectors), len(values)), -np.inf)
    for t in range(len(vectors)):
        np.maximum.at(best[t], dense, score[t])
    nq = len(offsets) - 1
    idx, sc, lb = np.full((nq, k), -1, np.int64), np.zeros((nq, k), np.float32), np.full((nq, k), NONE, np.uint32)
    for q in range(nq):
        total = best[int(offsets[q]):int(offsets[q + 1])].sum(axis=0)
        top = np.lexsort((np.arange(len(values)), -total))[:k]
        idx[q, :len(top)], sc[q, :len(top)], lb[q, :len(top)] = row0[top], total[top] + 0.0, values[top]
    return idx, sc, lb


COUNTS = (1, 32, 33, 128, 129)  # vectors of the queries of one call: the edges of VT = 1 / 2 / 4 and of a 128-vector block


@pytest.mark.parametrize("d", [4, 36, 384])  # below one K-chunk, one chunk and a tail, twelve chunks
def test_integer_corpora_equal_the_float64_reference(native, d):
    n = 197  # four spans, the last one short
    rng = np.random.default_rng(900 + d)
    rows = rng.integers(-2, 3, size=(n, d))
    offsets = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.uint64)
    vectors = rng.integers(-2, 3, size=(int(offsets[-1]), d))
    # (labels, items): every row its own label, runs of 100 rows (items cross span boundaries), one label for everything
    layouts = {"own": (np.arange(n) + 7, n), "runs": (np.arange(n) // 100, 5), "one": (np.zeros(n, np.int64), 4)}
    with _index(native, rows, layouts["own"][0]) as ix:
        for name, (labels, items) in layouts.items():
            ix.set_labels(0, labels.astype(np.uint32))
            for k in (1, 10):
                want = _maxsim(vectors, offsets, rows, labels, k)
                for round_vectors in (256, 64, 32):  # rounds of VT = 4 (two vector blocks), 2 and 1
                    ix.set_option("multivector_round_vectors", round_vectors)
                    (idx, sc, lb), rounds = _search(ix, 1, vectors, offsets, k)
                    what = (name, k, round_vectors)
                    assert rounds == ix.get_option("last_multivector_rounds") >= 2, what
                    assert ix.get_option("last_multivector_pairs") == int(offsets[-1]) * items, what
                    assert np.array_equal(idx, want[0]) and np.array_equal(lb, want[2]), what
                    assert np.array_equal(sc.view(np.float32), want[1]), what


VARIANTS = ("plain", "mask", "removed", "nan", "inf", "zero_vector")


@pytest.mark.parametrize("variant", VARIANTS)
def test_float_corpora_equal_the_vector_alu_route_bit_for_bit(native, variant):
    n, d = 1000, 132
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    vectors = rng.standard_normal((40, d)).astype(np.float32)
    offsets = np.array([0, 8, 40], np.uint64)
    labels = rng.permutation(n) // 7
    words = None
    if variant == "nan":
        rows[[3, 500], [0, 131]] = np.nan
    if variant == "inf":
        rows[[4, 501, 502], [1, 130, 7]] = (np.inf, -np.inf, np.inf)
    if variant == "zero_vector":
        vectors[[2, 20]] = 0.0
    with _index(native, rows, labels) as ix:
        if variant == "mask":
            allowed = rng.random(n) < 0.6
            allowed[labels == labels[0]] = False  # (a label with no allowed row)
            words = native.pack_row_mask(allowed)
        if variant == "removed":
            ix.remove_rows(np.unique(np.concatenate([rng.choice(n, 150, replace=False), np.nonzero(labels == labels[1])[0]])))
        for k in (10, 200):
            _same(ix, vectors, offsets, k, (variant, k), words)
        if variant == "plain":  # Gaussian rows are far apart next to the margin: almost every pair is certain
            _search(ix, 1, vectors, offsets, 10)
            assert ix.get_option("last_multivector_ambiguous") * 100 < ix.get_option("last_multivector_pairs")


def test_ties_and_one_ulp_neighbours_go_to_the_exact_arithmetic(native):
    n, d = 200, 132
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    labels = np.arange(n) // 4 + 2
    rows[10:15] = rows[10]                  # a label whose rows are all one vector
    labels[10:15] = 0
    rows[21] = rows[20]                     # a row and its copy, one element one ulp away
    rows[21, 50] = np.nextafter(rows[21, 50], np.float32(np.inf))
    labels[20:22] = 1
    vectors = rng.standard_normal((33, d)).astype(np.float32)
    offsets = np.array([0, 33], np.uint64)
    with _index(native, rows, labels) as ix:
        _same(ix, vectors, offsets, 10, "ties")
        _search(ix, 1, vectors, offsets, 10)
        assert ix.get_option("last_multivector_ambiguous") >= 2 * 33  # (gap 0 or one product's ulp: the margin cannot hold)
        assert ix.get_option("last_multivector_pairs") > ix.get_option("last_multivector_ambiguous")


def test_option_range_and_l2_keeps_the_old_route(native):
    rng = np.random.default_rng(6)
    rows, vectors = rng.standard_normal((300, 20)), rng.standard_normal((9, 20))
    offsets = np.array([0, 9], np.uint64)
    with _index(native, rows, np.arange(300) // 3, L2) as ix:
        for bad in (2, -2):
            with pytest.raises(native.HipBackendError):
                ix.set_option("multivector_tiles", bad)
        got, rounds = _search(ix, 1, vectors, offsets, 10)
        want, _ = _search(ix, 0, vectors, offsets, 10)
        assert rounds == 0 and all(np.array_equal(g, w) for g, w in zip(got, want))
