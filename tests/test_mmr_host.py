"""MMR search (a diversified top-k picked greedily from the pool of the best rows), the parts that need no GPU: the C ABI
surface, the public layers, and the device-free host side (wdbx-py_amd/csrc/host_mmr.h: argument checks, pools, rounds of
consecutive queries within a byte budget, the query table, the pairs kernel's grid and instance choice) driven by
tests/host_harness/mmr_harness.cpp -- built once plain and once under -fsanitize=address,undefined."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "mmr_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"
BUDGET = 256 << 20
MAX_ROUND = 32768
OK, NQ, K, FETCH_K, LAMBDA, BUFFER = range(6)


def test_header_binding_and_library_agree_on_the_new_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    from wdbx_amd import _native

    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    lib = ctypes.CDLL(str(path))
    doc = (ROOT / "INTEGRATION.md").read_text()
    name, arity = "wdbx_index_search_mmr", 12
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    assert len(m.group(1).split(",")) == arity
    res, args = _native.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == arity
    assert args[5] is ctypes.c_float  # lambda travels as a float, not a double
    assert hasattr(lib, name)
    assert f"`{name}`" in doc[doc.index("## F. Every symbol"):]


def test_public_layers_have_the_entry_points():
    from wdbx_amd import _native, api, indexing, vector_store, wdbx

    assert callable(_native.NativeIndex.search_mmr)
    assert callable(indexing.HipFlatIndex.search_mmr)
    vs = vector_store.VectorStore
    assert callable(vs.search_mmr) and callable(vs.search_mmr_async)
    assert callable(wdbx.WDBX.vector_search_mmr) and callable(wdbx.WDBX.vector_search_mmr_async)
    assert '"mmr"' in api.search_endpoint.__doc__


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("mmr_" + request.param) / "mmr_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args, stdin=""):
        p = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return p.stdout.split("\n")
    return run


def _plans(harness, cases):
    """cases: (pitch4, budget, [m]) -> per case (ni, grid, rounds [n, 9])"""
    stdin = "".join("%d %d %d %s\n" % (p4, budget, len(m), " ".join(map(str, m))) for p4, budget, m in cases)
    lines = harness("plan", stdin=stdin)
    out = []
    for i in range(len(cases)):
        n_rounds, ni, gx, gy, gz = map(int, lines[2 * i].split())
        rounds = np.array(lines[2 * i + 1].split(), dtype=np.int64).reshape(-1, 9)
        assert len(rounds) == n_rounds
        out.append((ni, (gx, gy, gz), rounds))
    return out


def _check(case, plan):
    pitch4, budget, m = case
    ni, grid, rounds = plan
    m = np.asarray(m, np.int64)
    what = (pitch4, budget, len(m))
    assert ni == (2 if pitch4 <= 128 else 4 if pitch4 <= 256 else 0), what
    per_query = m * pitch4 * 16 + m * m * 4
    # the rounds cover the queries exactly once, in order
    assert rounds[0, 0] == 0 and int(rounds[:, 1].sum()) == len(m), what
    assert np.array_equal(rounds[1:, 0], np.cumsum(rounds[:, 1])[:-1]), what
    assert rounds[:, 1].min() >= 1 and rounds[:, 1].max() <= MAX_ROUND, what
    for i, (q0, nq, m_max, rows, g_floats, nbytes, first_row0, last_row0, last_g0) in enumerate(rounds):
        mine = m[q0:q0 + nq]
        assert m_max == mine.max() and rows == mine.sum() and g_floats == (mine * mine).sum(), what
        assert nbytes == per_query[q0:q0 + nq].sum(), what
        # within budget, unless a single query passes it alone
        assert nbytes <= budget or nq == 1, what
        # greedy: the next round's first query did not fit any more (or the round was full)
        if i + 1 < len(rounds):
            assert nbytes + per_query[q0 + nq] > budget or nq == MAX_ROUND, what
        # the table: rows and squares back to back
        assert first_row0 == 0 and last_row0 == mine[:-1].sum() and last_g0 == (mine[:-1] ** 2).sum(), what
    big = rounds[np.flatnonzero(rounds[:, 2] == rounds[:, 2].max())[-1]]
    assert grid == (-(-big[2] // 64), -(-big[2] // 8), big[1]), what


def test_random_plans(harness):
    rng = np.random.default_rng(41)
    cases = []
    for pitch4 in (1, 128, 129, 256, 257, 1024):
        for nq in (1, 2, 257):
            for _ in range(6):
                kind = rng.integers(0, 4)
                if kind == 0:
                    m = rng.integers(0, 2049, size=nq)
                elif kind == 1:
                    m = rng.choice([0, 1, 40, 2048], size=nq)
                elif kind == 2:
                    m = np.full(nq, int(rng.choice([1, 200, 2048])))
                else:
                    m = np.where(rng.random(nq) < 0.5, 0, rng.integers(1, 2049, size=nq))
                # the real budget, one that forces a query per round, and two in between
                budget = int(rng.choice([BUDGET, 1, 1 << 20, 48 << 20]))
                cases.append((pitch4, budget, m.tolist()))
    for case, plan in zip(cases, _plans(harness, cases)):
        _check(case, plan)


def test_planned_shapes(harness):
    full = 2048 * 1024 * 16 + 2048 * 2048 * 4  # the worst single query: 2048 rows of 16 KiB and its 16 MiB square
    assert full <= BUDGET
    cases = [
        (1024, BUDGET, [2048] * 12),           # 48 MiB each: five to a round
        (257, BUDGET, [2048] * 9),             # d = 1028, fetch_k = 2048, nq = 9: 24 MiB each, one round of the default budget
        (257, 64 << 20, [2048] * 9),           # ... and the same call with the budget option at 64 MiB: two to a round
        (96, 1, [40, 0, 0, 7, 2048]),          # a budget nothing fits: one query per round, except that empty pools cost nothing
        (96, BUDGET, [0] * 257),               # nothing but empty pools: one round, no gather, no pairs
        (1, BUDGET, [1] * 70000),              # more queries than a grid's z holds
    ]
    plans = _plans(harness, cases)
    for case, plan in zip(cases, plans):
        _check(case, plan)
    assert plans[0][2][:, 1].tolist() == [5, 5, 2]
    assert plans[1][2][:, 1].tolist() == [9]
    assert plans[2][2][:, 1].tolist() == [2, 2, 2, 2, 1]
    assert plans[3][2][:, 1].tolist() == [1, 2, 1, 1]
    assert plans[4][2][:, 1].tolist() == [257] and plans[4][1][0] == 0
    assert plans[5][2][:, 1].tolist() == [32768, 32768, 4464]


def test_argument_checks(harness):
    cases = [
        ((1, 10, 40, "0.5", 1), OK), ((1, 1, 1, "0", 1), OK), ((1, 2048, 2048, "1", 1), OK),
        ((0, 10, 40, "0.5", 1), NQ), ((-3, 10, 40, "0.5", 1), NQ),
        ((1, 0, 40, "0.5", 1), K), ((1, 2049, 2049, "0.5", 1), K),
        ((1, 10, 9, "0.5", 1), FETCH_K), ((1, 10, 2049, "0.5", 1), FETCH_K),
        ((1, 10, 40, "nan", 1), LAMBDA), ((1, 10, 40, "-0.001", 1), LAMBDA), ((1, 10, 40, "1.0000001", 1), LAMBDA),
        ((1, 10, 40, "inf", 1), LAMBDA), ((1, 10, 40, "-0.0", 1), OK),
        ((1, 10, 40, "0.5", 0), BUFFER),
    ]
    got = harness("check", stdin="".join("%d %d %d %s %d\n" % c for c, _ in cases))
    assert [int(x) for x in got[:len(cases)]] == [w for _, w in cases]


def test_pool_sizes(harness):
    cases = [([5, 3, 9, -1, -1], 3), ([-1], 0), ([7], 1), ([0, 1, 2], 3), ([4, -1, 6], 1)]
    got = harness("pool", stdin="".join("%d %s\n" % (len(i), " ".join(map(str, i))) for i, _ in cases))
    assert [int(x) for x in got[:len(cases)]] == [w for _, w in cases]
