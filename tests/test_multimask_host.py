"""Per-query row masks in one batched call, the parts that need no GPU: the C ABI surface and the device-free placement of
the call's queries in the int8 tile kernel's query blocks (wdbx-py_amd/csrc/host_multimask.h), driven by
tests/host_harness/multimask_harness.cpp -- built once plain and once under -fsanitize=address,undefined.

The placement rule: all 16 queries of a column group share one mask; classes ascend with -1 (no
mask) first; the queries of a class keep the caller's order; a class gets at most 15 pad slots per block it touches; blocks
hold at most 256 slots (128 for the L2 width)."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "multimask_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"


def test_header_binding_and_library_declare_search_multimask():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bwdbx_index_search_multimask\s*\(", text)
    assert re.search(r"#define\s+WDBX_MAX_CALL_MASKS\s+64\b", text)
    from wdbx_amd import _native

    res, args = _native.SIGNATURES["wdbx_index_search_multimask"]
    assert res is ctypes.c_int and len(args) == 11
    assert callable(_native.NativeIndex.search_multimask)
    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    assert hasattr(ctypes.CDLL(str(path)), "wdbx_index_search_multimask")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("multimask_" + request.param) / "multimask_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(block_slots, n_masks, classes):
        text = "%d\n%s\n" % (len(classes), " ".join(str(int(c)) for c in classes))
        p = subprocess.run([str(exe), str(block_slots), str(n_masks)], input=text, capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
        lines = p.stdout.split("\n")
        ok, bad = map(int, lines[0].split()[1:])
        if not ok:
            return None, bad
        return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in lines[1:] if ln}, bad
    return run


def _by_counts(counts):
    """class -> number of queries, as one caller-ordered assignment (class after class)."""
    return [c for c, n in counts.items() for _ in range(n)]


def _check(plan, classes, n_masks, block_slots):
    slots, groups, blocks = plan["slots"], plan["groups"], plan["blocks"]
    nq = len(classes)
    # every query exactly once, everything else a pad
    placed = [q for q in slots if q >= 0]
    assert sorted(placed) == list(range(nq)) and all(q >= -1 for q in slots)
    assert len(slots) == 16 * len(groups)
    # every column group holds a single class: that of each of its queries
    for g, c in enumerate(groups):
        for q in slots[16 * g:16 * g + 16]:
            assert q < 0 or classes[q] == c, (g, q)
        assert any(q >= 0 for q in slots[16 * g:16 * g + 16]), ("a column group of pads only", g)
    # classes ascend, -1 first; the queries of a class keep the caller's order
    assert groups == sorted(groups) and plan["classes"] == sorted(set(classes)) == sorted(set(groups))
    for c in set(classes):
        assert [q for q in placed if classes[q] == c] == [q for q in range(nq) if classes[q] == c]
    # blocks: whole column groups, at most block_slots slots, all of them covered in order
    assert blocks[0] == 0 and blocks[-1] == len(groups) and all(a < b for a, b in zip(blocks, blocks[1:]))
    assert all(16 * (b - a) <= block_slots for a, b in zip(blocks, blocks[1:]))
    assert len(blocks) - 1 == -(-16 * len(groups) // block_slots)  # (as few blocks as the slots need)
    # pads: at most 15 per class and block it touches
    for a, b in zip(blocks, blocks[1:]):
        for c in set(groups[a:b]):
            pads = sum(1 for g in range(a, b) if groups[g] == c for q in slots[16 * g:16 * g + 16] if q < 0)
            assert pads <= 15, (c, pads)
    # the arithmetic of the issue: slots = sum over classes of 16 ceil(n_c / 16)
    assert len(slots) == sum(16 * -(-classes.count(c) // 16) for c in set(classes))


CASES = {
    "1/15/16/17": (4, _by_counts({0: 1, 1: 15, 2: 16, 3: 17})),
    "20 classes of 13": (20, _by_counts({c: 13 for c in range(20)})),
    "one class of 300": (1, [0] * 300),
    "all -1": (0, [-1] * 40),
    "all -1 with unused masks": (3, [-1] * 257),
    "interleaved random": (7, np.random.default_rng(11).integers(-1, 7, 500).tolist()),
    "300 next to 3": (2, [1, 0, 1] + [0] * 299 + [1]),
    "one query": (1, [0]),
}


@pytest.mark.parametrize("block_slots", [256, 128])
@pytest.mark.parametrize("name", list(CASES))
def test_placement(harness, name, block_slots):
    n_masks, classes = CASES[name]
    plan, _ = harness(block_slots, n_masks, classes)
    assert plan is not None
    _check(plan, classes, n_masks, block_slots)


def test_planned_blocks_of_the_named_cases(harness):
    # 1 + 15 + 16 + 17 queries: 1 + 1 + 1 + 2 column groups, one block
    plan, _ = harness(256, 4, CASES["1/15/16/17"][1])
    assert plan["groups"] == [0, 1, 2, 3, 3] and plan["blocks"] == [0, 5]
    assert plan["slots"][:17] == [0] + [-1] * 15 + [1]
    # 20 classes of 13: 20 column groups, more than the 16 of one block
    plan, _ = harness(256, 20, CASES["20 classes of 13"][1])
    assert plan["groups"] == list(range(20)) and plan["blocks"] == [0, 16, 20]
    plan, _ = harness(128, 20, CASES["20 classes of 13"][1])
    assert plan["blocks"] == [0, 8, 16, 20]
    # one class of 300: 19 column groups spanning two blocks, 4 pads in all
    plan, _ = harness(256, 1, CASES["one class of 300"][1])
    assert plan["groups"] == [0] * 19 and plan["blocks"] == [0, 16, 19] and plan["slots"].count(-1) == 4
    # 16 classes of 16: exactly one full block, no pad (the shape the feature is for)
    plan, _ = harness(256, 16, [q % 16 for q in range(256)])
    assert plan["blocks"] == [0, 16] and -1 not in plan["slots"]
    assert plan["slots"][:16] == list(range(0, 256, 16))


def test_refusals(harness):
    assert harness(256, 2, [0, 1, 2]) == (None, 2)      # an entry equal to n_masks
    assert harness(256, 2, [0, -2, 1]) == (None, 1)     # below -1
    assert harness(256, 0, [0]) == (None, 0)            # no masks at all: only -1 is valid
    assert harness(256, 2, []) == (None, 0)             # nq < 1
    assert harness(100, 2, [0])[0] is None              # a block width that is no multiple of 16
    assert harness(0, 2, [0])[0] is None
