"""Batched range search, the parts that need no GPU: the C ABI surface and the device-free host logic of
wdbx-py_amd/csrc/host_range_batch.h (route, blocks, buffer sizes, fallback bookkeeping), driven by
tests/host_harness/range_batch_harness.cpp -- built once plain and once under -fsanitize=address,undefined."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "range_batch_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"


def test_header_binding_and_library_declare_range_search_batch():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bwdbx_index_range_search_batch\s*\(", text)
    from wdbx_amd import _native

    res, args = _native.SIGNATURES["wdbx_index_range_search_batch"]
    assert res is ctypes.c_int and args == _native.SIGNATURES["wdbx_index_range_search"][1] and len(args) == 11
    assert callable(_native.NativeIndex.range_search_batch)
    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    assert hasattr(ctypes.CDLL(str(path)), "wdbx_index_range_search_batch")


def test_python_layers_expose_the_batch_form():
    from wdbx_amd import api
    from wdbx_amd.indexing import HipFlatIndex
    from wdbx_amd.vector_store import VectorStore
    from wdbx_amd.wdbx import WDBX

    assert callable(HipFlatIndex.range_search_batch) and callable(VectorStore.search_range_batch)
    assert callable(WDBX.vector_search_range_batch) and callable(WDBX.vector_search_range_batch_async)
    assert callable(api.range_search_batch_endpoint)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("range_batch_" + request.param) / "range_batch_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return [ln.split() for ln in p.stdout.split("\n") if ln]
    return run


def _blocks(harness, nq, max_block, forced=0):
    return [tuple(map(int, ln)) for ln in harness("blocks", nq, max_block, forced)]


@pytest.mark.parametrize("max_block", [256, 128, 64])
@pytest.mark.parametrize("nq", [1, 3, 4, 17, 63, 64, 65, 128, 129, 255, 256, 257, 300, 513, 1000])
def test_blocks_partition_the_queries_in_order(harness, nq, max_block):
    blocks = _blocks(harness, nq, max_block)
    assert blocks[0][0] == 0 and sum(nv for _, nv, _ in blocks) == nq
    for (q0, nv, ct), nxt in zip(blocks, blocks[1:] + [(nq, 0, 0)]):
        assert q0 + nv == nxt[0] and 1 <= nv <= 64 * ct <= max_block and ct in (1, 2, 4)
        assert ct == min(max_block // 64, 4 if nv > 128 else 2 if nv > 64 else 1)  # the narrowest query block that holds nv
    assert all(nv == max_block for _, nv, _ in blocks[:-1])  # only the last block is partial
    assert len(blocks) == -(-nq // max_block)


def test_named_cuts(harness):
    assert _blocks(harness, 300, 256) == [(0, 256, 4), (256, 44, 1)]
    assert _blocks(harness, 300, 128) == [(0, 128, 2), (128, 128, 2), (256, 44, 1)]
    assert _blocks(harness, 17, 256) == [(0, 17, 1)]
    assert _blocks(harness, 100, 256) == [(0, 100, 2)]
    assert _blocks(harness, 200, 256) == [(0, 200, 4)]
    assert _blocks(harness, 200, 256, forced=1) == [(0, 64, 1), (64, 64, 1), (128, 64, 1), (192, 8, 1)]
    assert _blocks(harness, 10, 128, forced=4) == [(0, 10, 2)]  # (a forced width the shape does not have: the widest it has)
    assert _blocks(harness, 0, 256) == [] and _blocks(harness, 5, 100) == []


def _route(harness, n_rows=200000, nq=16, l2=0, pitch=384, fits=1, bf16=3, variant=0, masked=1, min_rows=65536, min_work=800000,
           min_queries=4, has_mask=0):
    ln = harness("route", n_rows, nq, l2, pitch, fits, bf16, variant, masked, min_rows, min_work, min_queries, has_mask)[0]
    return int(ln[1]), int(ln[3])


def test_block_size_by_metric_and_pitch(harness):
    assert _route(harness, pitch=128) == (1, 256) and _route(harness, pitch=384) == (1, 256)
    assert _route(harness, pitch=512) == (1, 128) and _route(harness, pitch=768) == (1, 128)
    assert _route(harness, l2=1, pitch=384) == (1, 128) and _route(harness, l2=1, pitch=128) == (1, 128)
    assert _route(harness, pitch=896) == (1, 64) and _route(harness, pitch=1536) == (1, 64) and _route(harness, l2=1, pitch=1536) == (1, 64)
    assert _route(harness, pitch=1664) == (0, 0) and _route(harness, pitch=0) == (0, 0)


def test_route_table(harness):
    t = lambda **kw: _route(harness, **kw)[0]
    assert t() == 1
    # the options that say "int8 tiles, product form"
    assert t(bf16=2) == 0 and t(bf16=0) == 0 and t(variant=13) == 0 and t(variant=12) == 0 and t(fits=0) == 0
    # a mask needs the masked instances
    assert t(has_mask=1) == 1 and t(has_mask=1, masked=0) == 0 and t(masked=0) == 1
    # queries: at least range_batch_min_queries
    assert t(nq=3) == 0 and t(nq=4) == 1 and t(nq=4, min_queries=5) == 0 and t(nq=5, min_queries=5) == 1
    assert t(nq=1, min_queries=1) == 1 and t(nq=1, min_queries=0) == 1
    assert t(nq=1, min_queries=1, n_rows=100000) == 0  # (1 x 100 000 rows: the work rule)
    # rows: from 2 x gemm_min_rows always
    assert t(n_rows=131072, nq=3, min_queries=1) == 1 and t(n_rows=131071, nq=3, min_queries=1) == 0  # (3 x 131 071 < 520 000)
    # between gemm_min_rows and twice that: queries x rows >= 0.65 gemm_min_work
    assert t(n_rows=70000, nq=8) == 1 and t(n_rows=70000, nq=7) == 0
    # below gemm_min_rows: queries x rows >= gemm_min_work
    assert t(n_rows=21000, nq=39) == 1 and t(n_rows=21000, nq=38) == 0
    # gemm_min_work off: gemm_min_rows alone
    assert t(n_rows=20011, nq=4, min_rows=16384, min_work=0) == 1 and t(n_rows=16383, nq=300, min_rows=16384, min_work=0) == 0
    assert t(n_rows=1000, nq=256, min_rows=16384, min_work=0) == 0
    # nothing to search, too many rows for 32-bit row keys
    assert t(n_rows=0) == 0 and t(n_rows=0xFFFFFF00) == 0 and t(n_rows=0xFFFFFEFF, nq=4) == 1


def _sizes(harness, nv, ct, cap, pair_opt, n_rows, cus, pitch):
    return {ln[0]: int(ln[1]) for ln in harness("sizes", nv, ct, cap, pair_opt, n_rows, cus, pitch)}


def test_buffer_sizes(harness):
    s = _sizes(harness, 300 - 256, 1, 1024, 0, 10_000_000, 256, 384)
    assert s["pair_cap"] == 16384 and s["waves"] == 2048
    assert s["pairs"] == 2048 * 16384 * 8 and s["pair_count"] == 2048 * 4
    assert s["cand"] == 64 * 1024 * 8 and s["keys"] == 44 * 1024 * 8  # every SLOT has a candidate buffer, every QUERY a result buffer
    assert s["count"] == 257 * 4 and s["rcnt"] == 256 * 4 and s["thr"] == 512 * 4
    assert s["qb8"] == 64 * 384 and s["qpar"] == 64 * 16 and s["tau"] == 64 * 4 and s["fits"] == 1
    s = _sizes(harness, 256, 4, 5000, 64, 20011, 256, 128)
    assert s["pair_cap"] == 64 and s["waves"] == 79 * 8 and s["pairs"] == 79 * 8 * 64 * 8  # (fewer tiles than CUs)
    assert s["cand"] == 256 * 5000 * 8 and s["keys"] == 256 * 5000 * 8 and s["qb8"] == 256 * 128
    # the pair capacity option: 0 = the default, else clamped to [64, 65536]
    assert _sizes(harness, 4, 1, 1, 1, 1000, 8, 128)["pair_cap"] == 64
    assert _sizes(harness, 4, 1, 1, 1 << 20, 1000, 8, 128)["pair_cap"] == 65536
    assert _sizes(harness, 4, 1, 1, 3000, 1000, 8, 128)["pair_cap"] == 3000
    # candidate buffers of a block may grow to 1 GiB
    assert _sizes(harness, 256, 4, (1 << 30) // (256 * 8), 0, 10_000_000, 256, 384)["fits"] == 1
    assert _sizes(harness, 256, 4, (1 << 30) // (256 * 8) + 1, 0, 10_000_000, 256, 384)["fits"] == 0
    assert _sizes(harness, 40, 1, (1 << 30) // (64 * 8) + 1, 0, 10_000_000, 256, 384)["fits"] == 0


def _tally(harness, nq, max_block, lost):
    head, flags = harness("tally", nq, max_block, *lost)
    return {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}, [int(x) for x in flags[1:]]


def test_a_lost_block_maps_to_exactly_its_queries(harness):
    t, flags = _tally(harness, 300, 256, [])
    assert t == {"path": 2, "blocks": 2, "tile_blocks": 2, "fallback": 0, "pairs": 200} and flags == [0] * 300
    t, flags = _tally(harness, 300, 256, [1])
    assert t == {"path": 3, "blocks": 2, "tile_blocks": 1, "fallback": 44, "pairs": 107}
    assert flags == [0] * 256 + [1] * 44
    t, flags = _tally(harness, 300, 128, [0, 2])
    assert t["path"] == 3 and t["fallback"] == 128 + 44 and flags == [1] * 128 + [0] * 128 + [1] * 44
    t, flags = _tally(harness, 8, 256, [0])
    assert t["path"] == 3 and t["fallback"] == 8 and flags == [1] * 8
