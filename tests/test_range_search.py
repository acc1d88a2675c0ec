"""Range search (every row whose score reaches a threshold), the parts that need no GPU: the C ABI surface, the device-free
host assembly of the results (CSR offsets, per-query order, key decoding; wdbx-py_amd/csrc/host_range.h driven by
tests/host_harness/range_harness.cpp) and the store's pure merge step."""
import ctypes
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "range_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"


# ---- the C ABI surface ------------------------------------------------------------------------------------------------
def test_header_binding_and_library_declare_range_search():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bwdbx_index_range_search\s*\(", text)
    from wdbx_amd import _native

    res, args = _native.SIGNATURES["wdbx_index_range_search"]
    assert res is ctypes.c_int and len(args) == 11
    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    assert hasattr(ctypes.CDLL(str(path)), "wdbx_index_range_search")
    assert "`wdbx_index_range_search`" in (ROOT / "INTEGRATION.md").read_text()


def test_public_layers_have_the_range_entry_points():
    from wdbx_amd import api, indexing, vector_store, wdbx

    assert callable(indexing.HipFlatIndex.range_search)
    assert "range_search" not in indexing.VectorIndex.__abstractmethods__
    assert callable(vector_store.VectorStore.search_range) and callable(vector_store.VectorStore.search_range_async)
    assert callable(wdbx.WDBX.vector_search_range) and callable(wdbx.WDBX.vector_search_range_async)
    assert callable(api.range_search_endpoint)


# ---- host assembly: offsets, order, decoding --------------------------------------------------------------------------
def f2ord(f: float) -> int:
    u = struct.unpack("<I", struct.pack("<f", f))[0]
    return u ^ (0xFFFFFFFF if u >> 31 else 0x80000000)


def make_key(score: float, row: int) -> int:
    """make_key of kernels_common.h: (orderable float bits << 32) | ~row"""
    return (f2ord(score) << 32) | (~row & 0xFFFFFFFF)


def f32(x: float) -> float:
    return struct.unpack("<f", struct.pack("<f", x))[0]


def bits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("range") / "range_harness"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", f"-I{INC}", str(HARNESS), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def run_harness(exe, metric_l2, capacity, per_query_keys):
    counts = [len(k) for k in per_query_keys]
    flat = [k for keys in per_query_keys for k in keys]
    stdin = f"{metric_l2} {len(per_query_keys)} {capacity}\n" + " ".join(map(str, counts)) + "\n" + " ".join(map(str, flat)) + "\n"
    r = subprocess.run([str(exe)], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    lines = dict((ln.split()[0], [int(x) for x in ln.split()[1:]]) for ln in r.stdout.splitlines() if ln.strip())
    return lines


def expected(metric_l2, per_query):
    """per_query: list of [(score_in_key, row)] -> (offsets, rows, score bits) as the library must return them"""
    offsets, rows, sbits = [0], [], []
    for pairs in per_query:
        # (score descending, row ascending) on the key's score = what a descending sort of the u64 keys gives
        for s, r in sorted(pairs, key=lambda p: (-p[0], p[1])):
            rows.append(r)
            sbits.append(bits(f32(-s) + 0.0 if metric_l2 else s))
        offsets.append(offsets[-1] + len(pairs))
    return offsets, rows, sbits


@pytest.mark.parametrize("metric_l2", [0, 1])
def test_host_assembly_orders_each_query_and_fills_csr(harness, metric_l2):
    rng = np.random.default_rng(7 + metric_l2)
    per_query = []
    for q in range(7):
        n = [0, 1, 5, 300, 0, 64, 1000][q]
        scores = [f32(x) for x in rng.standard_normal(n)]
        if n > 10:  # exact ties: the row decides (ascending)
            scores[3] = scores[4] = scores[9]
        rows = rng.choice(1 << 31, size=n, replace=False).tolist()
        per_query.append(list(zip(scores, rows)))
    keys = [[make_key(s, r) for s, r in pairs] for pairs in per_query]
    for k in keys:
        np.random.default_rng(1).shuffle(k)
    out = run_harness(harness, metric_l2, 10_000, keys)
    eo, er, es = expected(metric_l2, per_query)
    assert out["offsets"] == eo
    assert out["rows"] == er
    assert out["scores"] == es
    if metric_l2:  # positive distances, ascending within a query
        sc = np.array(out["scores"], np.uint32).view(np.float32)
        for q in range(7):
            seg = sc[eo[q]:eo[q + 1]]
            assert np.all(np.diff(seg) >= 0)


def test_host_assembly_empty_queries_and_zero_hits(harness):
    out = run_harness(harness, 0, 0, [[], [], []])
    assert out["offsets"] == [0, 0, 0, 0]
    assert out["rows"] == [] and out["scores"] == []


def test_host_assembly_capacity_below_total_gives_offsets_only(harness):
    per_query = [[(0.5, 3), (0.75, 1)], [], [(0.25, 9), (0.25, 2), (1.0, 4)]]
    keys = [[make_key(s, r) for s, r in pq] for pq in per_query]
    for cap in (0, 1, 4):
        out = run_harness(harness, 0, cap, keys)
        assert out["offsets"] == [0, 2, 2, 5]
        assert "rows" not in out and "scores" not in out
    out = run_harness(harness, 0, 5, keys)  # exactly enough
    assert out["rows"] == [1, 3, 4, 2, 9]
    assert out["scores"] == [bits(0.75), bits(0.5), bits(1.0), bits(0.25), bits(0.25)]


def test_l2_selection_threshold_is_rounded_down_and_covers_the_exact_pass(harness):
    def tau(qq, t):
        r = subprocess.run([str(harness), "tau"], input=f"{qq!r} {t!r}\n", stdout=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 0
        return struct.unpack("<f", struct.pack("<I", int(r.stdout)))[0]

    for qq, t in [(1.0, 0.5), (1234.5, 17.25), (3.0, 0.0), (0.1, 2.0)]:
        v = tau(qq, t)
        assert v <= qq - t - 1e-5 * abs(t)          # never above: no row the exact pass keeps is lost
        assert v >= qq - t - 2e-5 * abs(t) - 1e-6 * abs(qq - t)  # and not needlessly loose
    assert tau(1.0, float("inf")) == float("-inf")
    assert tau(1.0, float("-inf")) == float("inf")


# ---- the store's merge -------------------------------------------------------------------------------------------------
def test_merge_range_shard_order_ties_cut_and_filters():
    from wdbx_amd.vector_store import matches_filter, merge_range

    meta = {f"v{i}": {"tag": "a" if i % 2 else "b", "i": i} for i in range(12)}
    shard0 = [("v0", 0.9), ("v2", 0.5), ("v4", 0.5), ("v6", 0.1)]
    shard1 = [("v1", 0.7), ("v3", 0.5), ("v5", 0.2)]
    shard2 = [("v7", 0.9), ("v9", 0.5)]
    got = merge_range([shard0, shard1, shard2], meta)
    # stable: equal scores keep shard order, then each shard's own order
    assert [r[0] for r in got] == ["v0", "v7", "v1", "v2", "v4", "v3", "v9", "v5", "v6"]
    assert all(r[2] is meta[r[0]] for r in got)
    assert merge_range([shard0, shard1, shard2], meta, max_results=3) == got[:3]
    assert merge_range([shard0, shard1, shard2], meta, max_results=0) == []
    assert merge_range([[], []], meta) == []
    # post-filter (filter the full answer) == pre-filter (each shard answers only for matching rows), with no limit
    flt = {"tag": "a"}
    post = merge_range([shard0, shard1, shard2], meta, filter_metadata=flt)
    pre_shards = [[r for r in s if matches_filter(meta[r[0]], flt)] for s in (shard0, shard1, shard2)]
    pre = merge_range(pre_shards, meta)
    assert post == pre and [r[0] for r in post] == ["v7", "v1", "v3", "v9", "v5"]
    # the cut comes after the filter
    assert merge_range([shard0, shard1, shard2], meta, filter_metadata=flt, max_results=2) == post[:2]
