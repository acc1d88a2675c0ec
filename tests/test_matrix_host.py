"""Distance matrix among listed rows, the parts that need no GPU: the C ABI surface, the public layers, and the device-free
host side (wdbx-py_amd/csrc/host_matrix.h: route, anchor block, instance, rounds and a round's scratch; the list check is
host_subset.h's) driven by tests/host_harness/matrix_harness.cpp -- built once plain and once under
-fsanitize=address,undefined."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "matrix_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"
BUDGET = 256 << 20
KEYS, LISTS, SELECT = 1, 2, 3
CU = 256


def test_header_binding_and_library_agree_on_the_new_symbol():
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    from wdbx_amd import _native

    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    lib = ctypes.CDLL(str(path))
    doc = (ROOT / "INTEGRATION.md").read_text()
    name, arity = "wdbx_index_search_matrix", 6
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    assert len(m.group(1).split(",")) == arity
    res, args = _native.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == arity
    assert hasattr(lib, name)
    assert f"`{name}`" in doc[doc.index("## F. Every symbol"):]
    # the contract is in the header, next to the declaration
    comment = raw[:raw.index("int " + name)].rsplit("/*", 1)[1]
    for words in ("OTHER", "bit-identical", "last_matrix_path", "last_matrix_rounds", "holds the handle's mutex"):
        assert words in comment, words


def test_public_layers_have_the_entry_points():
    from wdbx_amd import _native, api, indexing, vector_store, wdbx
    from wdbx_amd.config import WDBXConfig

    assert callable(_native.NativeIndex.search_matrix)
    assert callable(indexing.HipFlatIndex.search_matrix)
    vs = vector_store.VectorStore
    assert callable(vs.search_matrix) and callable(vs.search_matrix_async)
    for name in ("vector_search_matrix_pairs", "vector_search_matrix_offsets"):
        assert callable(getattr(wdbx.WDBX, name)) and callable(getattr(wdbx.WDBX, name + "_async"))
    assert callable(api.search_matrix_pairs_endpoint) and callable(api.search_matrix_offsets_endpoint)
    assert WDBXConfig({}).get("MATRIX_MAX_SAMPLE") == 10000


def test_the_kernel_header_is_part_of_the_library_and_uses_no_atomics():
    unit = (INC / "wdbx_hip.hip").read_text()
    assert unit.index('#include "kernels_subset.h"') < unit.index('#include "kernels_matrix.h"')
    kernel = (INC / "kernels_matrix.h").read_text()
    assert "atomic" not in re.sub(r"//[^\n]*", "", kernel)
    make = (INC / "Makefile").read_text()
    assert "kernels_matrix.h" in make and "host_matrix.h" in make


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("matrix_" + request.param) / "matrix_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return [line for line in p.stdout.split("\n") if line]
    return run


def _plan(harness, n_ids, k, pitch4=96, cu=CU, keys_max=8192, select_min_k=200, lds_lists=0):
    lines = harness("plan", n_ids, k, pitch4, cu, keys_max, select_min_k, lds_lists)
    names = ("route", "qb", "round", "blocks", "P", "lds", "scratch_u64", "ni", "mode", "rounds", "scratch_bytes")
    plan = dict(zip(names, map(int, lines[0].split())))
    plan["listed"] = [tuple(map(int, line.split())) for line in lines[1:]]
    return plan


def test_routes_at_their_boundaries(harness):
    assert _plan(harness, 8192, 10)["route"] == KEYS
    assert _plan(harness, 8193, 10)["route"] == LISTS
    assert _plan(harness, 8193, 199)["route"] == LISTS
    assert _plan(harness, 8193, 200)["route"] == SELECT
    assert _plan(harness, 8192, 200)["route"] == KEYS       # (a short list takes the keys whatever k is)
    assert _plan(harness, 5, 10, keys_max=4)["route"] == LISTS
    assert _plan(harness, 4, 10, keys_max=4)["route"] == KEYS
    assert _plan(harness, 5, 7, keys_max=4, select_min_k=8)["route"] == LISTS
    assert _plan(harness, 5, 8, keys_max=4, select_min_k=8)["route"] == SELECT
    assert _plan(harness, 5, 2048, keys_max=0, select_min_k=0)["route"] == LISTS  # (0 = never)
    p = _plan(harness, 0, 10)
    assert (p["route"], p["rounds"], p["scratch_bytes"], p["listed"]) == (0, 0, 0, [])


def test_anchor_blocks_and_sinks(harness):
    # lists: 8 anchors per block up to k = 64, 4 up to 128, lists in LDS and the block of one beyond
    for k, qb, mode in ((1, 8, 1), (64, 8, 1), (65, 4, 1), (128, 4, 1), (129, 1, 0), (2048, 1, 0)):
        p = _plan(harness, 10000, k, select_min_k=0)
        assert (p["route"], p["qb"], p["mode"]) == (LISTS, qb, mode), k
        assert p["lds"] == 4 * qb * k * 8 and p["P"] == p["blocks"]
    p = _plan(harness, 10000, 10, lds_lists=1)
    assert (p["qb"], p["mode"]) == (1, 0)
    # the key routes keep no list: always 8, a key per (anchor, listed row)
    for k in (1, 129, 2048):
        p = _plan(harness, 100, k)
        assert (p["route"], p["qb"], p["mode"], p["lds"]) == (KEYS, 8, 2, 0)
    p = _plan(harness, 10000, 300)
    assert (p["route"], p["qb"], p["mode"]) == (SELECT, 8, 2)
    # a lone listed row is the block of one on every route
    assert (_plan(harness, 1, 10)["qb"], _plan(harness, 1, 10, keys_max=0)["qb"]) == (1, 1)
    assert _plan(harness, 1, 10, keys_max=0)["mode"] == 1


@pytest.mark.parametrize("pitch4, ni", [(1, 2), (2, 2), (96, 2), (128, 2), (129, 4), (256, 4), (257, 0), (275, 0), (4096, 0)])
def test_loads_per_lane_follow_the_pitch(harness, pitch4, ni):
    assert _plan(harness, 100, 10, pitch4=pitch4)["ni"] == ni


@pytest.mark.parametrize("n_ids, want", [(1, [(0, 1)]), (256, [(0, 256)]), (257, [(0, 256), (256, 1)]),
                                         (600, [(0, 256), (256, 256), (512, 88)])])
@pytest.mark.parametrize("k, keys_max", [(10, 8192), (10, 0), (129, 0), (300, 0)])
def test_rounds_are_consecutive_anchors_256_at_most(harness, n_ids, want, k, keys_max):
    p = _plan(harness, n_ids, k, keys_max=keys_max)
    assert p["rounds"] == len(want) and p["round"] == min(n_ids, 256)
    assert [(first, b) for first, b, _ in p["listed"]] == want
    assert all(blocks == -(-b // p["qb"]) for _, b, blocks in p["listed"])
    # never more waves than listed rows, never an empty grid
    assert 1 <= p["blocks"] <= max(1, (n_ids + 3) // 4)


def test_a_round_stays_within_the_scratch_budget(harness):
    worst = [
        dict(n_ids=8192, k=10),                                   # keys, full rounds
        dict(n_ids=8192, k=2048),
        dict(n_ids=1_000_000, k=10, keys_max=1 << 40),            # keys on a long list: fewer anchors per round
        dict(n_ids=5_000_000, k=200),                             # select: a handful of anchors, one at a time
        dict(n_ids=33_000_000, k=2048, keys_max=1 << 40),         # one anchor's keys nearly fill it
        dict(n_ids=100_000, k=2048, select_min_k=0),              # lists at the largest k
        dict(n_ids=100_000, k=64, select_min_k=0),
        dict(n_ids=100_000, k=128, select_min_k=0, cu=1024),
        dict(n_ids=4_000_000_000 // 2, k=10),                     # lists on the longest list one call accepts (about)
    ]
    for case in worst:
        p = _plan(harness, **case)
        assert 0 < p["scratch_bytes"] <= BUDGET, (case, p)
        assert p["scratch_bytes"] == 8 * p["scratch_u64"]
        per_anchor = case["k"] * p["P"] if p["route"] == LISTS else case["n_ids"]
        assert p["scratch_u64"] == p["round"] * per_anchor
        assert 1 <= p["round"] <= 256 and (p["round"] % p["qb"] == 0 or p["round"] == case["n_ids"])
        assert p["rounds"] == -(-case["n_ids"] // p["round"])
    p = _plan(harness, 1_000_000, 10, keys_max=1 << 40)
    assert (p["round"], p["qb"]) == (32, 8)      # 33 anchors' keys fit: whole blocks of 8
    p = _plan(harness, 5_000_000, 200)
    assert (p["round"], p["qb"]) == (6, 1)       # fewer than one block fits: one anchor per block


def test_the_list_check_is_the_listed_row_search_s(harness):
    assert harness("validate", 100) == ["ok 0"]
    assert harness("validate", 100, 0, 5, 99) == ["ok 3"]
    assert harness("validate", 100, 0, 5, 100) == ["bad 2"]      # reaches the row count
    assert harness("validate", 100, 7, 7) == ["bad 1"]           # a repeated row
    assert harness("validate", 100, 7, 3) == ["bad 1"]           # decreasing
    assert harness("validate", 1 << 33, 1 << 32) == ["bad 0"]    # does not fit the 32-bit row numbers
