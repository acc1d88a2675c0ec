"""The handle's device memory: ``get_option("device_bytes_resident")`` counts every allocation the handle holds, buffers a
call releases leave the figure, the shadow copies' own figures are what their layouts say, and destroying a handle that has
used every search entry point frees each buffer once.

Shapes: inner product, d = 128 (the shortest row whose int8 image, padded to 128 bytes, is not larger than the row allows:
``i8_tiles_shape_ok``), 4 099 rows = 17 tiles of 256 with a ragged last one, ``gemm_min_rows = 1024`` and ``gemm_min_work = 0``
so that 8 queries reach the int8 tiles (k = 1 needs 8 * 128 rows).  The batched range search runs on the shape of
``tests/test_gpu_range_batch.py`` (20 011 rows, d = 384): only there can one query have more hits than the 16 384 candidates
per query a handle keeps room for (``RANGE_BATCH_KEEP_CAP``)."""
import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

N, D = 4099, 128
TILE_PAD_ROWS, G8_ROWS = 256, 256
# the group table of the int8 shadow for a capacity: one entry per 64 rows to the end of the padded allocation, and one more
NGROUPS = (N + TILE_PAD_ROWS + 63) // 64 + 1
# the shadow copies' own figures after the sequence of test_the_figure_never_falls_while_buffers_are_kept, by their layouts:
#   i8 groups: whole 256-row tiles of 128-byte rows and one of slack, + 16 bytes per group
SHADOWG_BYTES = ((N + G8_ROWS - 1) // G8_ROWS + 1) * G8_ROWS * 128 + NGROUPS * 16
#   u8: 128 bytes and one fp32 scale per row of the padded allocation
SHADOW8_BYTES = (N + TILE_PAD_ROWS) * (128 + 4)
#   u6 and its split planes: per 64-row tile 8 units of 768 bytes (4 units of 1024 bytes), 8 bytes per row, and for the planes
#   a 128-byte record per row
TILES64 = (N + 63) // 64
SHADOW6_BYTES = TILES64 * (8 * 768 + 64 * 8)
SHADOW42_BYTES = TILES64 * (4 * 1024 + 64 * 8 + 64 * 128)
RANGE_N, RANGE_D, RANGE_BATCH_KEEP_CAP = 20_011, 384, 16384


@pytest.fixture(scope="module")
def native():
    from wdbx_amd import _native

    assert _native.device_count() >= 1, "gpu tests need a visible AMD GPU"
    return _native


def _open(native, n=N, d=D, min_rows=1024):
    ix = native.NativeIndex(d, metric=native.METRIC_COSINE, capacity_rows=n)
    ix.fill_synthetic(O.SEED_CORPUS, 0, n, normalize=True)
    ix.set_option("gemm_min_rows", min_rows)
    ix.set_option("gemm_min_work", 0)
    ix.set_option("single_min_rows", 0)
    return ix


def _queries(nq, d=D, offset=0):
    return O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, offset, nq, d))


@pytest.fixture(scope="module")
def handle(native):
    with _open(native) as ix:
        yield ix


def _resident(ix):
    return ix.get_option("device_bytes_resident")


def test_a_masked_batch_counts_its_bad_row_table(native, handle):
    ix = handle
    q = _queries(8)
    words = native.pack_row_mask(np.arange(N) % 3 != 1)
    assert _resident(ix) == (N + TILE_PAD_ROWS) * D * 4  # a fresh handle holds its rows and nothing else
    ix.search(q, 1)  # the int8 shadow and the tiles' scratch
    assert ix.get_option("last_gemm_family") == 3 and ix.get_option("last_batch_masked") == 0
    ix.search(q[:1], 1, mask_words=words)  # the mask buffer (a lone masked query: the selection scan)
    assert ix.get_option("last_batch_masked") == 0
    before = _resident(ix)
    ix.search(q, 1, mask_words=words)
    assert ix.get_option("last_batch_masked") == 1
    after = _resident(ix)
    print(f"masked batch of 8 at k = 1 over {N} rows: device_bytes_resident {before} -> {after} (+{after - before}), "
          f"bad-row table {8 * NGROUPS} bytes for {NGROUPS} groups")
    # the call's bad-row table (d_gbad8 | ~mask): 8 bytes per 64-row group
    assert after - before >= 8 * NGROUPS


def test_the_figure_never_falls_while_buffers_are_kept(native, handle):
    ix = handle
    q = _queries(8, offset=100)
    ix.set_labels(0, np.arange(N, dtype=np.uint32) % 61)
    figure = _resident(ix)
    rounds = {"gemm_min_queries": 1 << 30, "scan_u6": 1, "scan_u42": 1}  # a round of single queries on the six-bit planes
    steps = (
        ("search, a batch on the int8 tiles", {}, lambda: ix.search(q, 1)),
        ("search, one query on the u8 scan", {}, lambda: ix.search(q[:1], 1)),
        ("search, a round of four on the six-bit planes", rounds, lambda: ix.search(q[:4], 1)),
        ("search_rows", {}, lambda: ix.search_rows(q, 5, np.arange(0, N, 7))),
        ("search_distinct", {}, lambda: ix.search_distinct(q, 5)),
        ("range_search", {}, lambda: ix.range_search(q[:2], 0.2)),
    )
    for name, options, call in steps:
        for option, value in options.items():
            ix.set_option(option, value)
        try:
            call()
        finally:
            for option, value in {"gemm_min_queries": 4, "scan_u6": -1, "scan_u42": -1}.items():
                ix.set_option(option, value)
        now = _resident(ix)
        print(f"{name}: device_bytes_resident {figure} -> {now}; last_single_path {ix.get_option('last_single_path')}, "
              f"last_single_u6 {ix.get_option('last_single_u6')}, last_single_u42 {ix.get_option('last_single_u42')}")
        assert now >= figure, name
        figure = now
    got = {name: ix.get_option(name) for name in ("shadowg_bytes", "shadow8_bytes", "shadow6_bytes", "shadow42_bytes")}
    print(got)
    assert got == {"shadowg_bytes": SHADOWG_BYTES, "shadow8_bytes": SHADOW8_BYTES, "shadow6_bytes": SHADOW6_BYTES,
                   "shadow42_bytes": SHADOW42_BYTES}


def test_a_range_batch_past_the_kept_capacity_releases_its_buffers(native):
    with _open(native, RANGE_N, RANGE_D, min_rows=16384) as ix:
        q = _queries(16, RANGE_D, 500)
        _, s = ix.search(q, 10)
        t = s[:, 4].copy()
        ix.range_search_batch(q, t)  # five hits each: the candidate and key buffers at their first size
        assert ix.get_option("last_range_batch_path") == 2
        kept = _resident(ix)
        ix.range_search_batch(q, t)
        assert _resident(ix) == kept
        t[3] = np.sort(ix.get_rows(0, RANGE_N) @ q[3])[-18000]  # one query with 18 000 hits > RANGE_BATCH_KEEP_CAP
        off, _, _ = ix.range_search_batch(q, t)
        assert off[4] - off[3] > RANGE_BATCH_KEEP_CAP and ix.get_option("last_range_batch_path") == 2
        after = _resident(ix)
        print(f"device_bytes_resident: {kept} with the buffers kept, {after} after the call that grew past {RANGE_BATCH_KEEP_CAP}")
        assert after < kept
        ix.range_search_batch(q, s[:, 4].copy())  # and the next call allocates them again, at the kept capacity
        assert _resident(ix) > after


def _every_family(native):
    """one small call of every search entry point, then the handle is destroyed"""
    with _open(native) as ix:
        q = _queries(8, offset=200)
        ix.set_labels(0, np.arange(N, dtype=np.uint32) % 61)
        words = native.pack_row_mask(np.arange(N) % 2 == 0)
        ids = np.arange(0, N, 5)
        ix.search(q[:1], 10)
        ix.search(q[:1], 200)  # (the radix-select range)
        ix.search(q, 1)
        ix.search(q, 1, mask_words=words)
        ix.search_multimask(q, 1, [words, native.pack_row_mask(np.arange(N) % 2 == 1)], [0, 1, -1, 0, 1, -1, 0, 1])
        ix.search_rows(q, 5, ids)
        ix.search_row_lists(q, 5, [ids, ids[::2]], [0, 1] * 4)
        ix.search_distinct(q, 5)
        ix.search_groups(q[:2], 3, 2)
        ix.search_multivector(q[:6], [0, 3, 6], 3)
        ix.search_mmr(q[:2], 3, 10, 0.5)
        ix.search_recommend(q[:4], [0, 1, 2, 3, 4], 5)
        ix.search_discover(q[:2], q[2:6], [0, 1, 2], 5)
        ix.range_search(q[:2], 0.2)
        ix.range_search_batch(q, 0.2)
        ix.compact(np.arange(1, N))
        ix.search(q, 1)
        figure = _resident(ix)
    return figure


def test_destroy_after_every_family_twice(native):
    first = _every_family(native)
    second = _every_family(native)
    assert first == second > (N + TILE_PAD_ROWS) * D * 4  # the second handle started from empty slots
