"""Option scan_u42_mfma through the library: rounds whose full passes run on the matrix cores in groups of 16 queries
(enqueue_singles_u6, host_index.h) return the ids and fp32 scores of the VALU passes (scan_u42_mfma = 0) byte for byte;
last_u42_mfma_groups reports the groups u42_mfma_groups plans; no query overflows on the plain corpora.

20 490 rows (neither a multiple of 64 nor of 16; the selection scans take a corpus from 8 k x 256 = 20 480 rows at k = 10) x 384,
scan_u42 = 1; one corpus at d = 96, a unit count without an instance, which stays on the VALU kernels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K = 20_490, 10
NQS = [16, 17, 22, 23, 33, 64, 65, 80]
MIN_SHORT = 6  # U42_MFMA_MIN_SHORT of host_index.h
_ROWS = {}


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _corpus(name, d):
    if (name, d) not in _ROWS:
        rng = np.random.default_rng({"uniform": 1, "gaussian": 2, "scaled_clustered": 3}[name] * 1000 + d)
        q = _unit(rng.standard_normal((max(NQS), d)))
        if name == "uniform":
            rows = _unit(rng.random((N, d)) * 2 - 1)
            q = _unit(rng.random((max(NQS), d)) * 2 - 1)
        elif name == "gaussian":
            rows = _unit(rng.standard_normal((N, d)))
        else:
            rows = (rng.standard_normal((N, d)) * rng.lognormal(0, 1.5, size=(N, 1))).astype(np.float32)
            q = rng.standard_normal((max(NQS), d)).astype(np.float32)
            where = rng.choice(N, 300, replace=False)
            rows[where] = (q[0] * 2.0 + 1e-3 * rng.standard_normal((300, d))).astype(np.float32)
        _ROWS[(name, d)] = (rows, q)
    return _ROWS[(name, d)]


@pytest.fixture(scope="module", params=["uniform", "gaussian", "scaled_clustered"])
def corpus(request):
    from wdbx_amd import _native

    rows, q = _corpus(request.param, 384)
    with _native.NativeIndex(384, device_id=0, capacity_rows=N) as index:
        index.add(rows)
        index.set_option("single_min_rows", 0)          # (small corpora default to the fp32 scan)
        index.set_option("gemm_min_rows", 0)
        index.set_option("gemm_min_queries", 1 << 30)   # rounds of single queries, not the batched tiles
        index.set_option("scan_u6", 1)
        index.set_option("scan_u42", 1)
        index.set_option("exchange_batch", 1024)        # a call is one batch, cut into rounds of 64
        yield index, q


def _planned(nq):
    """the groups of 16 of a call: per round of 64, nv // 16 full groups and a short one for a remainder of MIN_SHORT or more"""
    groups = 0
    for q0 in range(0, nq, 64):
        nv = min(64, nq - q0)
        groups += nv // 16 + (1 if nv % 16 >= MIN_SHORT else 0)
    return groups


def _search(ix, q, **opts):
    for name, value in opts.items():
        ix.set_option(name, value)
    idx, score = ix.search(q, K)
    return idx, score.view(np.uint32)


@pytest.mark.parametrize("nq", NQS)
def test_matrix_core_rounds_equal_the_valu_rounds(corpus, nq):
    ix, q = corpus
    q = q[:nq]
    want = _search(ix, q, scan_u42_mfma=0, scan_u42_share=-1)
    assert ix.get_option("last_u42_mfma_groups") == 0 and ix.get_option("last_u42_share") == 4
    surv0 = ix.get_option("u42_survivors_sum")
    for mode in (1, -1):
        got = _search(ix, q, scan_u42_mfma=mode)
        assert ix.get_option("last_single_u42") == 1
        assert ix.get_option("last_u42_mfma_groups") == _planned(nq), (nq, mode)
        assert ix.batch_status(nq)["overflowed"] == 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (nq, mode)
    # the survivors of the last round: the query term lets a few more rows through, never fewer
    if nq <= 64:
        assert ix.get_option("u42_survivors_sum") >= surv0 > 0
    ix.set_option("scan_u42_mfma", -1)


def test_a_launch_per_group_and_one_grid(corpus):
    ix, q = corpus
    q = q[:40]
    want = _search(ix, q, scan_u42_mfma=0)
    for per_query in (1, 0):
        got = _search(ix, q, scan_u42_mfma=1, scan8_per_query=per_query)
        assert ix.get_option("last_u42_mfma_groups") == 3
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), per_query
    ix.set_option("scan8_per_query", -1)
    ix.set_option("scan_u42_mfma", -1)


def test_an_explicit_share_keeps_the_valu_kernels(corpus):
    ix, q = corpus
    for share in (1, 2, 4):
        _search(ix, q[:32], scan_u42_mfma=-1, scan_u42_share=share)
        assert ix.get_option("last_u42_mfma_groups") == 0 and ix.get_option("last_u42_share") == share
    _search(ix, q[:32], scan_u42_mfma=1)       # ... unless the matrix cores are asked for by name
    assert ix.get_option("last_u42_mfma_groups") == 2 and ix.get_option("last_u42_share") == 0
    ix.set_option("scan_u42_share", -1)
    ix.set_option("scan_u42_mfma", -1)


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_a_non_finite_query_in_a_round_of_16(corpus, kind):
    ix, q = corpus
    q = q[:16].copy()
    q[5, 17] = np.nan if kind == "nan" else np.inf
    want = _search(ix, q, scan_u42_mfma=0)
    got = _search(ix, q, scan_u42_mfma=1)
    assert ix.get_option("last_u42_mfma_groups") == 1
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ix.set_option("scan_u42_mfma", -1)


def test_the_option_takes_minus_one_zero_and_one(corpus):
    ix, _ = corpus
    for bad in (-2, 2, 16):
        with pytest.raises(Exception):
            ix.set_option("scan_u42_mfma", bad)
    ix.set_option("scan_u42_mfma", -1)
    assert ix.get_option("scan_u42_mfma") == -1


def test_a_unit_count_without_an_instance_stays_on_the_valu_kernels():
    from wdbx_amd import _native

    rows, q = _corpus("gaussian", 96)
    with _native.NativeIndex(96, device_id=0, capacity_rows=N) as ix:
        ix.add(rows)
        for name, value in (("single_min_rows", 0), ("gemm_min_rows", 0), ("gemm_min_queries", 1 << 30), ("scan_u6", 1), ("scan_u42", 1),
                            ("exchange_batch", 1024)):
            ix.set_option(name, value)
        want = _search(ix, q[:33], scan_u42_mfma=0)
        got = _search(ix, q[:33], scan_u42_mfma=1)
        assert ix.get_option("last_single_u42") == 1
        assert ix.get_option("last_u42_mfma_groups") == 0 and ix.get_option("last_u42_share") == 4
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
