"""Recommend search (rows ranked by positive and negative examples), the parts that need no GPU: the C ABI surface, the public
layers, and the device-free host side (wdbx-py_amd/csrc/host_recommend.h: offset and exclusion checks, the plan of a pass,
rounds within the scratch bound, the short queries and the splice of the two sides) driven by
tests/host_harness/recommend_harness.cpp -- built once plain and once under -fsanitize=address,undefined."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "recommend_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"
BUDGET = 256 << 20


def test_header_binding_and_library_agree_on_the_new_symbol():
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    from wdbx_amd import _native

    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    lib = ctypes.CDLL(str(path))
    doc = (ROOT / "INTEGRATION.md").read_text()
    name, arity = "wdbx_index_search_recommend", 13
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    assert len(m.group(1).split(",")) == arity
    res, args = _native.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == arity
    assert hasattr(lib, name)
    assert f"`{name}`" in doc[doc.index("## F. Every symbol"):]
    assert re.search(r"#define\s+WDBX_MAX_EXAMPLES\s+%d\b" % _native.MAX_EXAMPLES, raw)
    assert re.search(r"#define\s+WDBX_MAX_EXCLUDE_ROWS\s+%d\b" % _native.MAX_EXCLUDE_ROWS, raw)


def test_public_layers_have_the_entry_points():
    from wdbx_amd import _native, api, indexing, vector_store, wdbx

    assert callable(_native.NativeIndex.search_recommend)
    assert callable(indexing.HipFlatIndex.recommend)
    vs = vector_store.VectorStore
    assert callable(vs.recommend) and callable(vs.recommend_async)
    assert callable(wdbx.WDBX.vector_recommend) and callable(wdbx.WDBX.vector_recommend_async)
    assert callable(api.recommend_endpoint)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("recommend_" + request.param) / "recommend_harness"
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
        ([0, 1, 1], "ok"),
        ([0, 3, 5, 6, 6, 70, 70], "ok"),                       # (64 examples: the limit itself)
        ([0, 32, 64], "ok"),
        ([1, 2, 2], "example_offsets[0] = 1, must be 0"),
        ([0, 2, 1], "example_offsets decrease at entry 2 (query 0): 1 after 2"),
        ([0, 1, 1, 0, 2], "example_offsets decrease at entry 3 (query 1): 0 after 1"),
        ([0, 0, 1], "query 0 has no positive example (example_offsets entries 0 and 1)"),
        ([0, 2, 3, 3, 3], "query 1 has no positive example (example_offsets entries 2 and 3)"),
        ([0, 33, 65], "query 0 has 65 examples, more than 64 (example_offsets entries 0 to 2)"),
        ([0, 1, 1, 2, 66], "query 1 has 65 examples, more than 64 (example_offsets entries 2 to 4)"),
    ]
    out = harness("offsets", stdin="".join(f"{(len(o) - 1) // 2} {' '.join(map(str, o))}\n" for o, _ in cases))
    assert out[:len(cases)] == [want for _, want in cases]


def test_exclusion_list_refusals_and_narrowing(harness):
    big = 2 ** 32 + 5
    cases = [
        (100, [], "ok"),
        (100, [0, 50, 99], "ok 0 50 99"),
        (2 ** 32 - 300, [7, 2 ** 32 - 301], f"ok 7 {2 ** 32 - 301}"),
        (100, list(range(0, 1024)), None),                       # (reaches the row count at entry 100)
        (5000, list(range(1024)), "ok " + " ".join(map(str, range(1024)))),
        (5000, list(range(1025)), "exclude_rows holds 1025 rows, more than 1024"),
        (100, [5, 5], "exclude_rows must be strictly increasing row numbers below 100 (entry 1 is 5)"),
        (100, [5, 4], "exclude_rows must be strictly increasing row numbers below 100 (entry 1 is 4)"),
        (100, [100], "exclude_rows must be strictly increasing row numbers below 100 (entry 0 is 100)"),
        (2 ** 40, [big], f"exclude_rows must be strictly increasing row numbers below {2 ** 40} (entry 0 is {big})"),
    ]
    cases[3] = (100, cases[3][1], "exclude_rows must be strictly increasing row numbers below 100 (entry 100 is 100)")
    out = harness("exclude", stdin="".join(f"{n} {len(r)} {' '.join(map(str, r))}\n" for n, r, _ in cases))
    assert out[:len(cases)] == [want for _, _, want in cases]


PLANS = [(n, nq, k, cu, smk, lds, budget)
         for n in (1, 63, 2000, 70000, 10_000_000, 2 ** 32 - 257)
         for nq in (1, 3, 32, 300)
         for k in (1, 64, 128, 129, 199, 200, 2048)
         for cu, smk, lds, budget in ((256, 200, 0, BUDGET), (256, 0, 0, BUDGET), (304, 200, 1, BUDGET), (8, 200, 0, 1 << 20))]


def test_plans_respect_the_scratch_bound_and_cover_every_query_once(harness):
    out = harness("plan", stdin="".join(" ".join(map(str, p)) + "\n" for p in PLANS))
    for (n, nq, k, cu, smk, lds, budget), line in zip(PLANS, out):
        head, tail = line.split("|")
        mode, rnd, blocks, P, lds_bytes, scratch, eblocks = map(int, head.split())
        assert mode == (2 if smk and k >= smk else 1 if k <= 128 and not lds else 0)
        assert 1 <= rnd <= min(nq, 256) and 1 <= blocks <= max(1, (n + 3) // 4) and blocks <= cu * 8
        per_query = n if mode == 2 else k * blocks
        assert scratch == rnd * per_query
        assert scratch * 8 <= budget or rnd == 1  # (a lone query may pass the bound: it cannot be cut further)
        if rnd < min(nq, 256):
            assert (rnd + 1) * per_query * 8 > budget  # (the bound, not caution, made the round smaller)
        assert (P, lds_bytes) == ((blocks, 4 * k * 8) if mode != 2 else (0, 0))
        assert eblocks == k // 8 + (k % 8) // 4 + k % 4
        rounds = np.array(tail.split(), int).reshape(-1, 2)
        assert rounds[0, 0] == 0 and (rounds[1:, 0] == rounds[:-1].sum(axis=1)).all() and rounds[-1].sum() == nq
        assert (rounds[:, 1] <= rnd).all() and (rounds[:, 1] >= 1).all()


def _passes_reference(fav, dis, k):
    """the Python loop: favoured rows cut at k, the gap filled from the disfavoured list, then empty slots"""
    short, rows = [], []
    for q, (f, d) in enumerate(zip(fav, dis)):
        slots = [f"{i}:{0.5 * i:g}:1" for i in f[:k]]
        if len(slots) < k:
            short.append(f"{q}:{k - len(slots)}")
            slots += [f"{i}:{0.25 * i:g}:0" for i in d[:k - len(slots)]]
        slots += ["-1:0:0"] * (k - len(slots))
        rows.append(" ".join(slots))
    return [" ".join(["short"] + short)] + rows


@pytest.mark.parametrize("k", [1, 4, 10])
def test_short_queries_and_splice_against_a_python_loop_for_every_round_size(harness, k):
    rng = np.random.default_rng(k)
    fav_counts = [0, k - 1, k, k + 5, 0, k - 1, 1, k, 2 * k]
    dis_counts = [k + 3, 0, 0, 7, k - 1 if k > 1 else 0, 1, k, 3, 0]  # (among them: a disfavoured list shorter than the gap)
    fav = [rng.permutation(1000)[:c].tolist() for c in fav_counts]
    dis = [(1000 + rng.permutation(1000)[:c]).tolist() for c in dis_counts]
    body = "".join(f"{len(f)} {' '.join(map(str, f))}\n{len(d)} {' '.join(map(str, d))}\n" for f, d in zip(fav, dis))
    want = _passes_reference(fav, dis, k)
    answers = [harness("passes", stdin=f"{len(fav)} {k} {rnd}\n{body}")[:len(want)] for rnd in (1, 2, 4, 9, 256)]
    assert answers[0] == want
    assert all(a == answers[0] for a in answers)  # (the answer does not depend on the round size)
