"""Option scan_u42_share through the library: rounds whose full passes share one read of the four-bit plane between 2 or 4
queries (enqueue_singles_u6, host_index.h) return the ids and fp32 scores of the lone passes (scan_u42_share = 1) and of the
u6 full pass (scan_u42 = 0) byte for byte; last_u42_share reports the widest group that ran; the survivors are the same.

40 000 uniform-normalised rows x 384 (the size of tests/test_gpu_u42_scan.py), k = 10, scan_u42 = 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K = 40_000, 384, 10
NQS = [1, 2, 3, 5, 65]  # 65: a full round of 64 and a round of one
_DATA = {}


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _data():
    if not _DATA:
        rng = np.random.default_rng(4265)
        _DATA["rows"] = _unit(rng.random((N, D)) * 2 - 1)
        _DATA["q"] = _unit(rng.random((max(NQS), D)) * 2 - 1)
    return _DATA["rows"], _DATA["q"]


@pytest.fixture(scope="module")
def ix():
    from wdbx_amd import _native

    rows, _ = _data()
    with _native.NativeIndex(D, device_id=0, capacity_rows=N) as index:
        index.add(rows)
        index.set_option("single_min_rows", 0)          # (small corpora default to the fp32 scan)
        index.set_option("gemm_min_rows", 0)
        index.set_option("gemm_min_queries", 1 << 30)   # rounds of single queries, not the batched tiles
        index.set_option("scan_u6", 1)
        yield index


def _widest(nq, share):
    """the widest group of the call: rounds of 64, nv // share groups of `share`, then one of 2 and / or one lone query"""
    widest = 0
    for q0 in range(0, nq, 64):
        nv = min(64, nq - q0)
        widest = max(widest, max(w for w in (4, 2, 1) if w <= share and w <= nv))
    return widest


def _search(ix, q, **opts):
    for name, value in opts.items():
        ix.set_option(name, value)
    idx, score = ix.search(q, K)
    return idx, score.view(np.uint32)


@pytest.mark.parametrize("nq", NQS)
def test_shared_rounds_equal_the_lone_passes_and_the_u6_pass(ix, nq):
    _, q = _data()
    q = q[:nq]
    ix.set_option("scan8_per_query", -1)
    u6 = _search(ix, q, scan_u42=0, scan_u42_share=-1)
    assert ix.get_option("last_single_u42") == 0 and ix.get_option("last_u42_share") == 0
    if nq == 1:
        # a lone query through this entry point takes its own path, whatever the option says
        for share in (1, 2, 4):
            got = _search(ix, q, scan_u42=1, scan_u42_share=share)
            assert ix.get_option("last_u42_share") <= 1
            assert np.array_equal(got[0], u6[0]) and np.array_equal(got[1], u6[1])
        return
    out, surv = {}, {}
    for share in (1, 2, 4):
        out[share] = _search(ix, q, scan_u42=1, scan_u42_share=share)
        assert ix.get_option("last_single_u42") == 1
        assert ix.get_option("last_u42_share") == _widest(nq, share), (nq, share)
        surv[share] = ix.get_option("u42_survivors_sum")
    for share in (2, 4):
        assert np.array_equal(out[share][0], out[1][0]) and np.array_equal(out[share][1], out[1][1]), (nq, share)
    assert np.array_equal(out[1][0], u6[0]) and np.array_equal(out[1][1], u6[1])
    assert surv[1] == surv[2] == surv[4] > 0
    # the default shares (or not) as one of the forced settings does
    got = _search(ix, q, scan_u42=1, scan_u42_share=-1)
    assert ix.get_option("last_u42_share") in (1, 2, 4)
    assert np.array_equal(got[0], u6[0]) and np.array_equal(got[1], u6[1])


def test_a_launch_per_group(ix):
    """scan8_per_query = 1: the branch of shards beyond 1 GiB of shadow, one launch per group"""
    _, q = _data()
    q = q[:7]  # at 4 per read: {0 .. 3} {4, 5} {6}
    want = _search(ix, q, scan_u42=1, scan_u42_share=1, scan8_per_query=1)
    for share in (2, 4):
        got = _search(ix, q, scan_u42_share=share)
        assert ix.get_option("last_u42_share") == share
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    one_grid = _search(ix, q, scan8_per_query=0)
    assert np.array_equal(one_grid[0], want[0]) and np.array_equal(one_grid[1], want[1])
    ix.set_option("scan8_per_query", -1)


def test_the_option_takes_minus_one_one_two_and_four(ix):
    for bad in (0, 3, 8):
        with pytest.raises(Exception):
            ix.set_option("scan_u42_share", bad)
    ix.set_option("scan_u42_share", -1)
    assert ix.get_option("scan_u42_share") == -1
