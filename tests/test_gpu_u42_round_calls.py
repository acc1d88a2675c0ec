"""A round's matrix-core groups as one launch, through the library (enqueue_singles_u6, host_index.h): whichever way option
scan8_per_query shapes the launches -- -1 and 0: all groups of a round in one launch whose grid.x u42_mfma_round_grid cuts so
that they are resident together; 1: a launch per group -- a call returns the ids and fp32 scores of the VALU passes
(scan_u42_mfma = 0) byte for byte, last_u42_mfma_groups reports the groups u42_mfma_groups plans and no query overflows.

The corpora and options of tests/test_gpu_u42_mfma_calls.py: 20 490 rows x 384, scan_u42 = 1.  nq = 32 and 64 (one round of two
and of four groups), 70 (a second round with one short group: a lone launch) and 200 (three full rounds and one of 8)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K = 20_490, 384, 10
NQS = [32, 64, 70, 200]
MIN_SHORT = 6  # U42_MFMA_MIN_SHORT of host_index.h


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _rows(name):
    rng = np.random.default_rng({"uniform": 1, "gaussian": 2, "scaled_clustered": 3}[name] * 1000 + D + 7)
    q = _unit(rng.standard_normal((max(NQS), D)))
    if name == "uniform":
        rows = _unit(rng.random((N, D)) * 2 - 1)
        q = _unit(rng.random((max(NQS), D)) * 2 - 1)
    elif name == "gaussian":
        rows = _unit(rng.standard_normal((N, D)))
    else:
        rows = (rng.standard_normal((N, D)) * rng.lognormal(0, 1.5, size=(N, 1))).astype(np.float32)
        q = rng.standard_normal((max(NQS), D)).astype(np.float32)
        where = rng.choice(N, 300, replace=False)
        rows[where] = (q[0] * 2.0 + 1e-3 * rng.standard_normal((300, D))).astype(np.float32)
    return rows, q


@pytest.fixture(scope="module", params=["uniform", "gaussian", "scaled_clustered"])
def corpus(request):
    from wdbx_amd import _native

    rows, q = _rows(request.param)
    with _native.NativeIndex(D, device_id=0, capacity_rows=N) as index:
        index.add(rows)
        index.set_option("single_min_rows", 0)          # (small corpora default to the fp32 scan)
        index.set_option("gemm_min_rows", 0)
        index.set_option("gemm_min_queries", 1 << 30)   # rounds of single queries, not the batched tiles
        index.set_option("scan_u6", 1)
        index.set_option("scan_u42", 1)
        index.set_option("exchange_batch", 1024)        # a call is one batch, cut into rounds of 64
        yield index, q


def _planned(nq):
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
def test_every_launch_shape_equals_the_valu_rounds(corpus, nq):
    ix, q = corpus
    q = q[:nq]
    want = _search(ix, q, scan_u42_mfma=0, scan8_per_query=-1)
    assert ix.get_option("last_u42_mfma_groups") == 0
    for per_query in (-1, 0, 1):
        got = _search(ix, q, scan_u42_mfma=-1, scan8_per_query=per_query)
        assert ix.get_option("last_single_u42") == 1
        assert ix.get_option("last_u42_mfma_groups") == _planned(nq), (nq, per_query)
        assert ix.batch_status(nq)["overflowed"] == 0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (nq, per_query)
    ix.set_option("scan8_per_query", -1)
