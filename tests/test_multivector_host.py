"""Multi-vector search (late interaction: labels ranked by the sum of per-vector best scores), the parts that need no GPU: the
C ABI surface, the public layers, and the device-free planning (wdbx-py_amd/csrc/host_multivector.h: rounds of consecutive
vectors, the segments of each round with their carry flags, route / grids / scratch) driven by
tests/host_harness/multivector_harness.cpp -- built once plain and once under -fsanitize=address,undefined."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "multivector_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"
NONE = 0xFFFFFFFF
BUDGET = (256 << 20) // 8  # u64s of DISTINCT_SCRATCH_BYTES
CARRY_IN, CARRY_OUT = 1, 2


def test_header_binding_and_library_agree_on_the_new_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    from wdbx_amd import _native

    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    lib = ctypes.CDLL(str(path))
    doc = (ROOT / "INTEGRATION.md").read_text()
    name, arity = "wdbx_index_search_multivector", 11
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    assert len(m.group(1).split(",")) == arity
    res, args = _native.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == arity
    assert hasattr(lib, name)
    assert f"`{name}`" in doc[doc.index("## F. Every symbol"):]
    assert re.search(r"#define\s+WDBX_MAX_QUERY_VECTORS\s+1024\b", text)


def test_public_layers_have_the_entry_points():
    from wdbx_amd import _native, api, indexing, vector_store, wdbx

    assert callable(_native.NativeIndex.search_multivector)
    assert callable(indexing.HipFlatIndex.search_multivector)
    vs = vector_store.VectorStore
    assert callable(vs.search_multivector) and callable(vs.search_multivector_async)
    assert callable(wdbx.WDBX.vector_search_multivector) and callable(wdbx.WDBX.vector_search_multivector_async)
    assert "query_vectors" in api.search_endpoint.__doc__


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("multivector_" + request.param) / "multivector_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args, stdin=""):
        p = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return p.stdout.split("\n")
    return run


def _plans(harness, cu, sel, cases):
    """cases: (n_items, n_labels, n_spans, k, option, counts) -> a dict per case"""
    stdin = "".join("%d %d %d %d %d %d %s\n" % (*c[:5], len(c[5]), " ".join(map(str, c[5]))) for c in cases)
    lines = [ln for ln in harness("plan", cu, sel, stdin=stdin)]
    out = []
    for i in range(len(cases)):
        head = list(map(int, lines[3 * i].split()))
        keys = ("qb", "round_max", "floor", "select", "score_blocks", "rank_blocks", "lds", "keys_u64", "rank_u64", "n_rounds",
                "n_segments")
        p = dict(zip(keys, head))
        p["rounds"] = np.array(lines[3 * i + 1].split(), dtype=np.int64).reshape(-1, 6)    # first vectors seg0 segs ranked rq0
        p["segments"] = np.array(lines[3 * i + 2].split(), dtype=np.int64).reshape(-1, 5)  # query v0 v1 slot carry
        assert len(p["rounds"]) == p["n_rounds"] and len(p["segments"]) == p["n_segments"]
        out.append(p)
    return out


def _check(case, p, cu, sel):
    n_items, n_labels, n_spans, k, option, counts = case
    what = (case[:5], len(counts), cu, sel)
    off = np.concatenate([[0], np.cumsum(counts)])
    total = int(off[-1])
    assert p["select"] == int(0 < sel <= k), what
    assert p["qb"] in (1, 8), what
    assert 1 <= p["rank_blocks"] <= max(1, min(-(-n_labels // 2048), 2 * cu)), what
    assert p["lds"] == (0 if p["select"] else 4 * k * 8) and p["lds"] <= 64 * 1024, what
    per_segment = n_labels if p["select"] else k * p["rank_blocks"]
    fit = BUDGET // (n_items + per_segment)
    assert p["floor"] == int(fit < 1), what
    assert p["round_max"] == max(1, min(option, fit)), what
    rounds, segs = p["rounds"], p["segments"]
    # rounds partition the vectors in order
    assert rounds[0, 0] == 0 and int(rounds[:, 1].sum()) == total, what
    assert np.array_equal(rounds[1:, 0], np.cumsum(rounds[:, 1])[:-1]), what
    assert rounds[:, 1].min() >= 1 and rounds[:, 1].max() <= p["round_max"], what
    # whole blocks of 8 wherever more than 8 vectors remain and the round may hold a block
    for first, vectors in rounds[:-1, :2]:
        if p["round_max"] >= 8:
            assert vectors % 8 == 0, what
        else:
            assert vectors == p["round_max"], what
    # the segments of the rounds are consecutive and cover the segment list
    assert rounds[0, 2] == 0 and int(rounds[:, 3].sum()) == len(segs), what
    assert np.array_equal(rounds[1:, 2], np.cumsum(rounds[:, 3])[:-1]), what
    seen = np.zeros(total, np.int64)
    ranked_queries = []
    prev_out = None  # the query the previous round's last segment carried out
    for first, vectors, seg0, nsegs, ranked, rq0 in rounds:
        mine = segs[seg0:seg0 + nsegs]
        assert nsegs >= 1, what
        # in vector order, back to back, inside the round
        assert mine[0, 1] == 0 and mine[-1, 2] == vectors, what
        assert np.array_equal(mine[1:, 1], mine[:-1, 2]) and (mine[:, 2] > mine[:, 1]).all(), what
        # one query each, consecutive queries
        assert np.array_equal(mine[1:, 0], mine[:-1, 0] + 1), what
        slot = 0
        for j, (q, v0, v1, s, carry) in enumerate(mine):
            lo, hi = first + v0, first + v1
            assert off[q] <= lo and hi <= off[q + 1], what       # every vector of the segment belongs to its query
            seen[lo:hi] += 1
            assert bool(carry & CARRY_IN) == (off[q] < lo), what
            assert bool(carry & CARRY_OUT) == (hi < off[q + 1]), what
            if carry & CARRY_IN:
                assert j == 0 and prev_out == q, what             # only the first segment, and it continues what was carried out
            if carry & CARRY_OUT:
                assert j == nsegs - 1 and s == -1, what           # only the last segment; it ranks nothing
            else:
                assert s == slot, what
                if slot == 0:
                    assert rq0 == q, what
                slot += 1
                ranked_queries.append(int(q))
        assert slot == ranked, what
        if not (mine[0, 4] & CARRY_IN):
            assert prev_out is None, what                         # whatever was carried out is picked up by the next round
        prev_out = int(mine[-1, 0]) if mine[-1, 4] & CARRY_OUT else None
    assert prev_out is None, what
    assert (seen == 1).all(), what                                # every vector lies in exactly one segment
    assert ranked_queries == list(range(len(counts))), what       # every query is ranked once, in order
    # scratch: the largest round's keys and the most ranked segments' lists / keys
    assert p["keys_u64"] == int(rounds[:, 1].max()) * n_items, what
    assert p["rank_u64"] == int(rounds[:, 4].max()) * per_segment, what
    if not p["floor"]:
        assert p["keys_u64"] + p["rank_u64"] <= BUDGET, what
    else:
        assert p["round_max"] == 1, what
    if option == 1:
        assert (rounds[:, 1] == 1).all() and p["qb"] == 1 and len(rounds) == total, what
    vblocks = -(-min(total, p["round_max"]) // p["qb"])
    assert 1 <= p["score_blocks"] <= max(1, -(-n_spans // 4)) and p["score_blocks"] * vblocks <= max(2 * cu, vblocks), what


def test_random_plans(harness):
    rng = np.random.default_rng(23)
    shapes = [(1, 1, 1), (70, 64, 1), (5100, 4800, 79), (5079, 5000, 79), (1_160_000, 1_000_000, 156_250),
              (10_000_000, 10_000_000, 156_250), (40_000_000, 40_000_000, 625_000)]
    for cu, sel in ((256, 200), (256, 0), (8, 17)):
        cases = []
        for shape in shapes:
            for _ in range(40):
                nq = int(rng.integers(1, 12))
                kind = rng.integers(0, 4)
                if kind == 0:
                    counts = rng.integers(1, 4, size=nq)
                elif kind == 1:
                    counts = rng.integers(1, 40, size=nq)
                elif kind == 2:
                    counts = rng.choice([1, 7, 8, 9, 33, 256, 257, 1024], size=nq)
                else:
                    counts = np.full(nq, int(rng.choice([1, 8, 32])))
                option = int(rng.choice([1, 2, 3, 7, 8, 9, 12, 64, 255, 256]))
                k = int(rng.choice([1, 10, 16, 17, 128, 200, 2048]))
                cases.append((*shape, k, option, counts.tolist()))
        for case, p in zip(cases, _plans(harness, cu, sel, cases)):
            _check(case, p, cu, sel)


def test_planned_shapes(harness):
    # the mixed call of the GPU test at every round option: 1 + 7 + 8 + 9 + 33 = 58 vectors
    counts = [1, 7, 8, 9, 33]
    want = {256: [58], 8: [8] * 7 + [2], 3: [3] * 19 + [1], 1: [1] * 58}
    cases = [(5079, 5000, 79, 10, opt, counts) for opt in want]
    for (case, p), opt in zip(zip(cases, _plans(harness, 256, 200, cases)), want):
        assert p["rounds"][:, 1].tolist() == want[opt]
        _check(case, p, 256, 200)
    # option 8: query 4 (33 vectors from vector 25) is cut by rounds 3 .. 7
    p = _plans(harness, 256, 200, [cases[1]])[0]
    assert [tuple(s) for s in p["segments"][:3]] == [(0, 0, 1, 0, 0), (1, 1, 8, 1, 0), (2, 0, 8, 0, 0)]
    assert [tuple(s) for s in p["segments"][3:6]] == [(3, 0, 8, -1, CARRY_OUT), (3, 0, 1, 0, CARRY_IN), (4, 1, 8, -1, CARRY_OUT)]
    assert tuple(p["segments"][-1]) == (4, 0, 2, 0, CARRY_IN) and tuple(p["segments"][-2]) == (4, 0, 8, -1, CARRY_IN | CARRY_OUT)
    # a label order whose items of ONE vector pass the budget: the floor, one vector per round whatever the option says
    p = _plans(harness, 256, 200, [(40_000_000, 40_000_000, 625_000, 10, 256, [3, 2])])[0]
    assert p["floor"] == 1 and p["round_max"] == 1 and p["rounds"][:, 1].tolist() == [1] * 5 and p["keys_u64"] > BUDGET
    # 10 M rows, 10 per label: 1.16 M items, a 32-vector query in one round of 28 vectors and one of 4
    p = _plans(harness, 256, 200, [(1_160_000, 1_000_000, 156_250, 10, 256, [32])])[0]
    assert p["round_max"] == 28 and p["rounds"][:, 1].tolist() == [24, 8]


def test_label_order_keeps_the_smallest_row_of_each_label(harness):
    labels = [5, NONE, 3, 5, 3, NONE, 9, 4_000_000_000]
    got = [int(x) for x in harness("row0", stdin="%d %d\n%s\n" % (len(labels) + 2, len(labels), " ".join(map(str, labels))))[0].split()]
    # label order: 3 (rows 2, 4), 5 (0, 3), 9 (6), 4e9 (7), then the NONE rows 1, 5 and the unset rows 8, 9
    assert got == [2, 0, 6, 7, 1, 5, 8, 9]
