"""Discovery search (rows ranked by context pairs and a target), the parts that need no GPU: the C ABI surface, the public
layers, and the device-free host side (wdbx-py_amd/csrc/host_discover.h: the pair offsets' checks, the plans of the scoring
pass and of the zone stage, rounds within the scratch bound, the staged vectors and their table, the zones an answer needs and
the splice) driven by tests/host_harness/discover_harness.cpp -- built once plain and once under
-fsanitize=address,undefined."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "discover_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"
BUDGET = 256 << 20
ZONES = 33


def test_header_binding_and_library_agree_on_the_new_symbol():
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    from wdbx_amd import _native

    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    lib = ctypes.CDLL(str(path))
    doc = (ROOT / "INTEGRATION.md").read_text()
    name, arity = "wdbx_index_search_discover", 14
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    assert len(m.group(1).split(",")) == arity
    res, args = _native.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == arity
    assert hasattr(lib, name)
    assert f"`{name}`" in doc[doc.index("## F. Every symbol"):]
    assert re.search(r"#define\s+WDBX_MAX_CONTEXT_PAIRS\s+%d\b" % _native.MAX_CONTEXT_PAIRS, raw)


def test_public_layers_have_the_entry_points():
    from wdbx_amd import _native, api, indexing, vector_store, wdbx

    assert callable(_native.NativeIndex.search_discover)
    assert callable(indexing.HipFlatIndex.discover)
    vs = vector_store.VectorStore
    assert callable(vs.discover) and callable(vs.discover_async)
    assert callable(wdbx.WDBX.vector_discover) and callable(wdbx.WDBX.vector_discover_async)
    assert callable(api.discover_endpoint)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("discover_" + request.param) / "discover_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args, stdin=""):
        p = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return p.stdout.split("\n")
    return run


def test_offsets_every_refusal_names_the_query_and_the_entry(harness):
    cases = [
        (1, [0, 0], "ok"),                                      # (target mode: no pair is fine)
        (1, [0, 32, 32, 37], "ok"),                             # (32 pairs: the limit itself)
        (0, [0, 1, 33], "ok"),
        (1, [1, 2], "pair_offsets[0] = 1, must be 0"),
        (1, [0, 3, 2], "pair_offsets decrease at entry 2 (query 1): 2 after 3"),
        (1, [0, 1, 34], "query 1 has 33 context pairs, more than 32 (pair_offsets entries 1 and 2)"),
        (0, [0, 2, 2, 3], "query 1 has no context pair and the call has no targets (pair_offsets entries 1 and 2)"),
        (0, [0, 0], "query 0 has no context pair and the call has no targets (pair_offsets entries 0 and 1)"),
    ]
    stdin = "".join(f"{t} {len(off) - 1} " + " ".join(map(str, off)) + "\n" for t, off, _ in cases)
    out = harness("offsets", stdin=stdin)
    assert out[:len(cases)] == [want for _, _, want in cases]


def _plan(harness, *a):
    head, tail = harness("plan", stdin=" ".join(map(str, a)) + "\n")[0].split("|")
    h = list(map(int, head.split()))
    t = list(map(int, tail.split()))
    return h, list(zip(t[::2], t[1::2]))


def test_plan_context_mode_is_the_list_or_key_plan_of_the_pass(harness):
    # 10 M rows, one query, k = 10, 256 CUs: register lists, 2048 workgroups, one round
    (mode, rnd, blocks, P, lds, scratch, rec, _), rounds = _plan(harness, 10_000_000, 1, 10, 0, 256, 200, 0, BUDGET)
    assert (mode, rnd, blocks, P, lds, scratch, rec) == (1, 1, 2048, 2048, 4 * 10 * 8, 10 * 2048, 0) and rounds == [(0, 1)]
    # k from select_min_k on: a key per row; five queries of 10 M keys each do not fit 256 MiB together
    (mode, rnd, blocks, P, lds, scratch, rec, _), rounds = _plan(harness, 10_000_000, 5, 200, 0, 256, 200, 0, BUDGET)
    assert (mode, rnd, P, lds, scratch, rec) == (2, 3, 0, 0, 30_000_000, 0) and rounds == [(0, 3), (3, 2)]


def test_plan_target_mode_rounds_keep_the_records_within_the_budget(harness):
    (mode, rnd, blocks, P, lds, scratch, rec, _), rounds = _plan(harness, 10_000_000, 1, 10, 1, 256, 200, 0, BUDGET)
    assert (mode, rnd, blocks, P, lds, scratch, rec) == (1, 1, 2048, 0, 0, 0, 10_000_000) and rounds == [(0, 1)]
    # 9 bytes per row and query: 256 MiB hold two queries of 10 M rows, not three
    (mode, rnd, blocks, _, _, _, rec, _), rounds = _plan(harness, 10_000_000, 7, 10, 1, 256, 200, 0, BUDGET)
    assert (rnd, rec) == (2, 20_000_000) and rounds == [(0, 2), (2, 2), (4, 2), (6, 1)]
    # a tiny budget: one query per round, every query exactly once; fewer rows than waves: one workgroup per four rows
    (mode, rnd, blocks, _, _, _, rec, _), rounds = _plan(harness, 1000, 5, 300, 1, 256, 200, 1, 100)
    assert (mode, rnd, blocks, rec) == (2, 1, 250, 1000) and rounds == [(q, 1) for q in range(5)]
    (mode, rnd, blocks, _, _, _, rec, _), rounds = _plan(harness, 1000, 5, 129, 1, 256, 0, 0, 9 * 1000 * 3)
    assert (mode, rnd, rec) == (0, 3, 3000) and rounds == [(0, 3), (3, 2)]
    # the pair blocks of 0 / 1 / 3 / 4 / 5 / 32 pairs (read from the k column): 2, 4 + 2, 8, 8 + 2, 8 x 8
    blocks_of = [_plan(harness, 1000, 1, p, 1, 256, 0, 0, BUDGET)[0][7] for p in (1, 3, 4, 5, 32)]
    assert blocks_of == [1, 2, 1, 2, 8]


def test_zone_plan(harness):
    def zplan(*a):
        head, tail = harness("zplan", stdin=" ".join(map(str, a)) + "\n")[0].split("|")
        t = list(map(int, tail.split()))
        return list(map(int, head.split())), list(zip(t[::2], t[1::2]))

    # one slot over 10 M rows: 2048 workgroups of 256 rows at a time, lists of k
    (rnd, blocks, P, lds, scratch), rounds = zplan(10_000_000, 1, 10, 1, 256, BUDGET)
    assert (rnd, blocks, P, lds, scratch) == (1, 2048, 2048, 320, 20480) and rounds == [(0, 1)]
    # few rows: never more workgroups than 256-row pieces
    (rnd, blocks, P, lds, scratch), rounds = zplan(1000, 3, 10, 0, 256, BUDGET)
    assert (rnd, blocks, P, scratch) == (3, 4, 4, 3 * 10 * 4) and rounds == [(0, 3)]
    # the select route under a tiny budget: a key per row, two slots per launch
    (rnd, blocks, P, lds, scratch), rounds = zplan(1000, 5, 300, 2, 256, 2 * 1000 * 8 + 7)
    assert (rnd, P, lds, scratch) == (2, 0, 0, 2000) and rounds == [(0, 2), (2, 2), (4, 1)]


def test_zones_from_the_top_down(harness):
    def counts(**at):
        c = [0] * ZONES
        for zone, n in at.items():
            c[int(zone[1:])] = n
        return " ".join(map(str, c))

    stdin = "".join([
        f"10 {counts(z3=25, z2=100, z0=7)}\n",          # the top zone alone covers k
        f"10 {counts(z32=2, z5=3, z1=50)}\n",           # three zones, the empty ones between them skipped
        f"10 {counts(z3=1, z2=0, z1=4, z0=2)}\n",       # all zones together fall short of k
        f"10 {counts()}\n",                             # no eligible row at all
        f"1 {counts(z0=5)}\n",
        f"10 {counts(z4=10, z3=9)}\n",                  # exactly k: the next zone is not asked for
    ])
    out = harness("zones", stdin=stdin)
    assert out[:6] == ["3:10", "32:2 5:3 1:5", "3:1 1:4 0:2", "", "0:1", "4:10"]


def test_stage_and_table(harness):
    out = harness("stage", stdin="1 3 5 0 0 1 3\n")
    assert out[0] == "100 101 1000 1001 102 1002 1003 1004 1005"
    assert out[1] == "0:0 1:1 4:2"
    out = harness("stage", stdin="0 2 4 0 1 3\n")
    assert out[0] == "1000 1001 1002 1003 1004 1005"
    assert out[1] == "0:1 2:2"


def test_call_rounds_zones_and_splice(harness):
    def counts(**at):
        c = [0] * ZONES
        for zone, n in at.items():
            c[int(zone[1:])] = n
        return " ".join(map(str, c))

    k = 4
    queries = [counts(z2=9), counts(z3=1, z1=2, z0=9), counts(), counts(z32=1, z0=1), counts(z1=3)]
    want = [
        "20:10:2 21:10.5:2 22:11:2 23:11.5:2",
        "1030:515:3 1010:505:1 1011:505.5:1 1000:500:0",
        "-1:0:0 -1:0:0 -1:0:0 -1:0:0",
        "3320:1660:32 3000:1500:0 -1:0:0 -1:0:0",
        "4010:2005:1 4011:2005.5:1 4012:2006:1 -1:0:0",
    ]
    for rnd in (1, 2, 5, 8):
        out = harness("call", stdin=f"5 {k} {rnd}\n" + "\n".join(queries) + "\n")
        assert out[0] == "slots 7"
        assert out[1:6] == want, rnd
