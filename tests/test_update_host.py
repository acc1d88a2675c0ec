"""Batch upsert and delete of listed rows, the parts that need no GPU: the C ABI surface, the public layers, and the device-free
host side (wdbx-py_amd/csrc/host_update.h: coverage counts, distinct int8 groups, upload rounds, launch count; the list
check is host_subset.h's) driven by tests/host_harness/update_harness.cpp -- built once plain and once under
-fsanitize=address,undefined."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "update_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"
ROUND_BYTES = 256 << 20


@pytest.mark.parametrize("name, arity", [("wdbx_index_set_rows_at", 5), ("wdbx_index_remove_rows", 3)])
def test_header_binding_and_library_agree_on_the_new_symbols(name, arity):
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    from wdbx_amd import _native

    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    lib = ctypes.CDLL(str(path))
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    assert len(m.group(1).split(",")) == arity
    res, args = _native.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == arity
    assert hasattr(lib, name)
    doc = (ROOT / "INTEGRATION.md").read_text()
    assert f"`{name}`" in doc[doc.index("## F. Every symbol"):]
    # the contract is in the header, next to the declarations
    comment = raw[:raw.index("int wdbx_index_set_rows_at")].rsplit("/*", 1)[1]
    for words in ("strictly increasing", "WDBX_E_INVALID", "bit for bit", "last_update_launches", "NaN", "handle's mutex"):
        assert words in comment, words


def test_public_layers_have_the_entry_points():
    from wdbx_amd import _native, api, indexing, vector_store, wdbx

    assert callable(_native.NativeIndex.set_rows_at) and callable(_native.NativeIndex.remove_rows)
    assert callable(indexing.HipFlatIndex.remove_many)
    vs = vector_store.VectorStore
    assert callable(vs.delete_many) and callable(vs.delete_by_filter)
    for name in ("delete_vectors", "delete_by_filter"):
        assert callable(getattr(wdbx.WDBX, name)) and callable(getattr(wdbx.WDBX, name + "_async"))
    assert callable(api.delete_vectors_endpoint)


def test_the_kernel_header_is_part_of_the_library_and_shares_the_per_row_functions():
    unit = (INC / "wdbx_hip.hip").read_text()
    assert unit.index('#include "kernels_aux.h"') < unit.index('#include "kernels_update.h"') < unit.index('#include "host_index.h"')
    make = (INC / "Makefile").read_text()
    assert "kernels_update.h" in make and "host_update.h" in make and "libupdate_harness.so" in make
    kernel = re.sub(r"//[^\n]*", "", (INC / "kernels_update.h").read_text())
    assert "atomic" not in kernel
    # every per-row function is called by its range kernel and by the list form: the two cannot drift
    homes = {"row_sqnorm": "kernels_aux.h", "normalize_row": "kernels_aux.h", "row_piece_to_bf16": "kernels_tiles.h",
             "row_to_u8": "kernels_scan8.h", "row_to_u6": "kernels_scan6.h", "row_to_u42": "kernels_scan42.h",
             "group_to_i8g": "kernels_tiles8.h"}
    for fn, home in homes.items():
        body = re.sub(r"//[^\n]*", "", (INC / home).read_text())
        assert len(re.findall(r"\b%s\(" % fn, body)) == 2, (fn, home)   # its definition and its range kernel's call
        assert len(re.findall(r"\b%s\(" % fn, kernel)) == 1, fn


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("update_" + request.param) / "update_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return [line for line in p.stdout.split("\n") if line]
    return run


NAMES = ("n", "n_cn", "n_16", "n_8", "n_6", "n_42", "n_refresh", "round_rows", "rounds", "launches")


def _plan(harness, ids, n_rows=1000, dim=96, upload=1, cn=0, bf16=0, i8g=0, u8=0, u6=0, u42=0):
    lines = harness("plan", n_rows, dim, upload, cn, bf16, i8g, u8, u6, u42, *ids)
    if lines[0].startswith("bad"):
        return {"bad": int(lines[0].split()[1])}
    plan = dict(zip(NAMES, map(int, lines[0].split())))
    plan["groups"] = list(map(int, lines[1].split()[1:]))
    plan["listed"] = [tuple(map(int, line.split())) for line in lines[2:]]
    return plan


def test_an_empty_list_launches_nothing(harness):
    p = _plan(harness, [], cn=1000, bf16=1000, i8g=1000, u8=1000, u6=1000, u42=1000)
    assert (p["n"], p["rounds"], p["launches"], p["n_refresh"], p["groups"], p["listed"]) == (0, 0, 0, 0, [], [])


def test_one_row_and_all_rows_cost_the_same_launches(harness):
    full = dict(cn=1000, bf16=1000, i8g=1000, u8=1000, u6=1000, u42=1000)
    one = _plan(harness, [17], **full)
    every = _plan(harness, range(1000), **full)
    assert one["launches"] == every["launches"] == 3          # scatter, refresh, int8 groups
    assert (one["n_refresh"], one["groups"], one["listed"]) == (1, [0], [(0, 1)])
    assert every["n_refresh"] == 1000 and every["groups"] == list(range(16)) and every["listed"] == [(0, 1000)]
    assert all(every[k] == 1000 for k in NAMES[:6])
    # which copies exist decides the count, the list's length does not
    assert _plan(harness, [17])["launches"] == 1
    assert _plan(harness, range(1000))["launches"] == 1
    assert _plan(harness, [17], u8=1000)["launches"] == 2
    assert _plan(harness, [17], i8g=1000)["launches"] == 2
    assert _plan(harness, [17], upload=0, **full)["launches"] == 3


def test_lists_that_straddle_each_coverage(harness):
    ids = [0, 99, 100, 101, 499, 500, 999]
    p = _plan(harness, ids, cn=100, bf16=101, i8g=500, u8=1000, u6=1, u42=0)
    assert (p["n_cn"], p["n_16"], p["n_8"], p["n_6"], p["n_42"]) == (2, 3, 7, 1, 0)
    assert p["n_refresh"] == 7
    assert p["groups"] == [0, 1, 7]                            # rows 0, 99 .. 101, 499: below 500
    # a list wholly behind every coverage: only the scatter
    p = _plan(harness, [600, 700], cn=100, bf16=100, i8g=512, u8=600, u6=64, u42=1)
    assert (p["n_refresh"], p["groups"], p["launches"]) == (0, [], 1)
    # a coverage at the row count covers the last row
    p = _plan(harness, [999], cn=1000, u42=999)
    assert (p["n_cn"], p["n_42"], p["launches"]) == (1, 0, 2)


def test_group_lists_at_the_group_boundary_and_in_the_last_partial_group(harness):
    assert _plan(harness, [63, 64, 65], i8g=1000)["groups"] == [0, 1]
    assert _plan(harness, [63], i8g=1000)["groups"] == [0]
    assert _plan(harness, [64, 65], i8g=1000)["groups"] == [1]
    assert _plan(harness, [0, 1, 2, 62, 63], i8g=1000)["groups"] == [0]
    # 1000 rows: the last group holds rows 960 .. 999
    assert _plan(harness, [959, 960, 999], i8g=1000)["groups"] == [14, 15]
    # a coverage that cuts a group: its listed rows below the coverage still name the whole group
    assert _plan(harness, [959, 960, 999], i8g=961)["groups"] == [14, 15]
    assert _plan(harness, [959, 960, 999], i8g=960)["groups"] == [14]


def test_rejected_lists(harness):
    assert _plan(harness, [7, 7]) == {"bad": 1}                # equal neighbours
    assert _plan(harness, [7, 3]) == {"bad": 1}                # decreasing
    assert _plan(harness, [0, 5, 1000]) == {"bad": 2}          # reaches the row count
    assert _plan(harness, [1000]) == {"bad": 0}
    assert _plan(harness, [1 << 32], n_rows=1 << 33) == {"bad": 0}   # does not fit the 32-bit row numbers
    assert "bad" not in _plan(harness, [0, 5, 999])


def test_the_round_cut(harness):
    per_round = ROUND_BYTES // (384 * 4)
    assert harness("rounds", per_round, 384) == [f"{per_round} 1 0 {per_round}"]
    assert harness("rounds", per_round + 1, 384) == [f"{per_round} 2 {per_round} 1"]
    assert harness("rounds", 10_000_000, 384) == [f"{per_round} {-(-10_000_000 // per_round)} "
                                                  f"{10_000_000 // per_round * per_round} {10_000_000 % per_round}"]
    assert harness("rounds", 5, 1 << 20) == ["64 1 0 5"]
    assert harness("rounds", 3, 1 << 27) == ["1 3 2 1"]       # a row larger than a round: one row per round
    # rounds add scatter launches only; a removal uploads nothing and never cuts
    ids = list(range(0, 4000, 2))
    p = _plan(harness, ids, n_rows=4000, dim=1 << 20, u8=4000)
    assert (p["round_rows"], p["rounds"], p["launches"]) == (64, 32, 33)
    assert p["listed"][:2] == [(0, 64), (64, 64)] and p["listed"][-1] == (1984, 16)
    p = _plan(harness, ids, n_rows=4000, dim=1 << 20, upload=0, u8=4000)
    assert (p["round_rows"], p["rounds"], p["launches"]) == (2000, 1, 2)
