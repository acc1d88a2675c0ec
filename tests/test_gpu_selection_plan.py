"""What the selection plan (wdbx-py_amd/csrc/host_selection.h) decides, seen through the library on the MI355X: every path that
answers by sample -> threshold -> full pass -> re-scoring -> final top-k, at the smallest shape at which it is still taken.

Each case asserts
  * the candidate capacity ``wdbx_index_batch_status`` reports: the formula the path's enqueue function held before the plan
    moved into the header (tests/selection_parent.py);
  * ``last_single_path``, ``last_single_u6``, ``last_single_u42``, ``last_gemm_family``, ``last_sample_qn`` and
    ``last_batch_masked`` of a fresh handle after the call;
  * ids equal to the float64 numpy top-k, position by position.  The seeded rows are such that no two of a query's best k + 1
    float64 scores (among the rows its mask allows) lie closer than 1e-5 -- fp32 sums of at most 384 products of unit vectors
    round within ~1e-6 -- which the case re-derives before it compares, so no tie tolerance is needed.

Shapes and forcing options are those of test_gpu_u6_scan.py / test_gpu_u42_scan.py (40 000 x 384, rounds of single queries)
and of test_gpu_batch_masked.py / test_gpu_multimask.py (70 003 x 64, the tiles from 16 384 rows)."""
import numpy as np
import pytest

import selection_parent as P

pytestmark = pytest.mark.gpu

K = 10
GAP = 1e-5
N_ROUND, D_ROUND, NQ_ROUND = 40_000, 384, 5
N_TILE, D_TILE, NQ_TILE = 70_003, 64, 40

_DATA = {}


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _data(n, d, nq, seed):
    if (n, d) not in _DATA:
        rng = np.random.default_rng(seed)
        rows, queries = _unit(rng.standard_normal((n, d))), _unit(rng.standard_normal((nq, d)))
        _DATA[(n, d)] = (rows, queries, rows.astype(np.float64) @ queries.astype(np.float64).T)
    return _DATA[(n, d)]


def _round_data():
    return _data(N_ROUND, D_ROUND, NQ_ROUND, 20)


def _tile_data():
    return _data(N_TILE, D_TILE, NQ_TILE, 21)


def _tile_masks():
    rng = np.random.default_rng(22)
    return rng.random(N_TILE) < 0.5, rng.random(N_TILE) < 0.17  # (the second: at most 16 384 rows, more than the unmasked capacity)


def _expected(scores, allowed_per_query, k=K):
    """ids of the float64 top-k per query among its allowed rows; asserts the gaps that make the comparison exact"""
    out = []
    for qi, allowed in enumerate(allowed_per_query):
        s = scores[:, qi] if allowed is None else np.where(allowed, scores[:, qi], -np.inf)
        best = np.argsort(-s, kind="stable")[: k + 1]
        assert np.min(-np.diff(s[best])) > GAP, (qi, "the seeded rows must leave no near-tie among the best k + 1")
        out.append(best[:k])
    return np.stack(out)


def _open(rows, **opts):
    from wdbx_amd import _native

    ix = _native.NativeIndex(rows.shape[1], device_id=0, capacity_rows=len(rows))
    ix.add(rows)
    for name, value in opts.items():
        ix.set_option(name, value)
    return ix


def _flags(ix):
    return tuple(ix.get_option(name) for name in ("last_single_path", "last_single_u6", "last_single_u42", "last_gemm_family",
                                                  "last_sample_qn", "last_batch_masked"))


# rounds of single queries: small corpora default to the fp32 scan, several queries to the tiles
ROUNDS = dict(single_min_rows=0, gemm_min_rows=0, gemm_min_queries=1 << 30)


@pytest.mark.parametrize("name, u6, u42, flags", [("u8", 0, 0, (2, 0, 0, 0, 1, 0)), ("u6", 1, 0, (2, 1, 0, 0, 4, 0)),
                                                  ("u42", 1, 1, (2, 1, 1, 0, 4, 0))])
def test_rounds_of_single_queries(name, u6, u42, flags):
    rows, queries, scores = _round_data()
    with _open(rows, scan_u6=u6, scan_u42=u42, **ROUNDS) as ix:
        idx, _ = ix.search(queries, K)
        st = ix.batch_status(NQ_ROUND)
        assert _flags(ix) == flags
    # the u8 round reports its candidate capacity; the u6 / u42 rounds that of the cut's short list (4096 keys), which is what
    # their repair launches test -- their candidate buffers hold 256 x the expected rows
    tile_rows, rw, scaled, factor = P.U8
    plan = P.plan(N_ROUND, tile_rows, rw, K, 0, scaled, factor)
    assert (plan["sample_tiles"], plan["stride"], plan["cap"]) == (20, 7, 4096) and not plan["too_small"]
    assert st["capacity"] == (plan["cap"] if name == "u8" else 4096)
    assert np.array_equal(idx, _expected(scores, [None] * NQ_ROUND))


TILES = dict(single_min_rows=0, gemm_min_rows=16384)


@pytest.mark.parametrize("div", [0, 1])  # 1: the sample visits every tile, stride 1
def test_int8_tiles_without_a_mask(div):
    rows, queries, scores = _tile_data()
    with _open(rows, gemm_sample_div=div, **TILES) as ix:
        idx, _ = ix.search(queries, K)
        st = ix.batch_status(NQ_TILE)
        assert _flags(ix) == (0, 0, 0, 3, 1, 0)
    tile_rows, rw, scaled, factor = P.INT8
    plan = P.plan(N_TILE, tile_rows, rw, K, div, scaled, factor)
    assert (plan["tiles"], plan["sample_tiles"], plan["stride"]) == ((274, 10, 27) if div == 0 else (274, 274, 1))
    assert st["capacity"] == plan["cap"] == (8960 if div == 0 else 4096)
    assert np.array_equal(idx, _expected(scores, [None] * NQ_TILE))


@pytest.mark.parametrize("which", ["half", "small"])
def test_int8_tiles_with_a_mask(which):
    from wdbx_amd import _native

    rows, queries, scores = _tile_data()
    half, small = _tile_masks()
    allowed = half if which == "half" else small
    count = int(np.count_nonzero(allowed))
    assert 16384 < np.count_nonzero(half) and 8960 < np.count_nonzero(small) <= 16384
    with _open(rows, **TILES) as ix:
        idx, _ = ix.search(queries, K, mask_words=_native.pack_row_mask(allowed))
        st = ix.batch_status(NQ_TILE)
        assert _flags(ix) == (0, 0, 0, 3, 1, 1)
    # half: the sample grows by 1 / f to 21 tiles, stride 13: 32 x 10 x 14 expected rows;
    # small: the unmasked sample, and room for ALL the allowed rows
    plan = P.masked_plan(N_TILE, K, 0, count, small_class=count if which == "small" else 0)
    assert plan["sample_tiles"] == (P.masked_sample(N_TILE, *P.INT8[:2], K, 0, count) if which == "half" else 10)
    assert st["capacity"] == plan["cap"] == (4480 if which == "half" else count)
    assert np.array_equal(idx, _expected(scores, [allowed] * NQ_TILE))


def test_int8_tiles_with_a_mask_per_query():
    from wdbx_amd import _native

    rows, queries, scores = _tile_data()
    half, small = _tile_masks()
    query_mask = [qi % 2 for qi in range(NQ_TILE)]  # two classes in one block of 48 slots
    with _open(rows, **TILES) as ix:
        idx, _ = ix.search_multimask(queries, K, [_native.pack_row_mask(half), _native.pack_row_mask(small)], query_mask)
        st = ix.batch_status(NQ_TILE)
        assert _flags(ix) == (0, 0, 0, 3, 1, 2)
        assert ix.get_option("last_batch_mask_classes") == 2 and ix.get_option("last_batch_blocks") == 1
    # the block samples for its most selective class above 16 384 rows, the capacity holds every row of the class below
    plan = P.masked_plan(N_TILE, K, 0, int(np.count_nonzero(half)), small_class=int(np.count_nonzero(small)))
    assert st["capacity"] == plan["cap"] == np.count_nonzero(small)
    assert np.array_equal(idx, _expected(scores, [(half, small)[c] for c in query_mask]))


def test_legacy_bf16_tiles():
    rows, queries, scores = _tile_data()
    with _open(rows, gemm_bf16=1, **TILES) as ix:
        idx, _ = ix.search(queries, K)
        st = ix.batch_status(NQ_TILE)
        assert _flags(ix) == (0, 0, 0, 1, 1, 0)
    tile_rows, rw, scaled, factor = P.LEGACY_BF16
    plan = P.plan(N_TILE, tile_rows, rw, K, 0, scaled, factor)
    assert (plan["tiles"], plan["sample_tiles"], plan["stride"]) == (274, 20, 13)
    assert st["capacity"] == plan["cap"] == 4480
    assert np.array_equal(idx, _expected(scores, [None] * NQ_TILE))
