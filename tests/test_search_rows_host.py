"""Search among listed rows, the parts that need no GPU: the C ABI surface, the public layers, and the device-free host side
(wdbx-py_amd/csrc/host_subset.h: list validation and narrowing, route / query block / grid / scratch sizing) driven by
tests/host_harness/subset_harness.cpp -- built once plain and once under -fsanitize=address,undefined."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "subset_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"

NONE, KEYS, LISTS, SELECT = 0, 1, 2, 3
N_IDS = (0, 1, 63, 64, 65, 257, 4097, 5000)
KS = (1, 10, 16, 17, 64, 65, 128, 129, 200, 2048)
NQS = (1, 2, 7, 8, 9, 33, 256)


def test_header_binding_and_library_declare_search_rows():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bwdbx_index_search_rows\s*\(", text)
    from wdbx_amd import _native

    res, args = _native.SIGNATURES["wdbx_index_search_rows"]
    assert res is ctypes.c_int and len(args) == 9
    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    assert hasattr(ctypes.CDLL(str(path)), "wdbx_index_search_rows")
    assert "`wdbx_index_search_rows`" in (ROOT / "INTEGRATION.md").read_text()


def test_public_layers_have_the_entry_points():
    from wdbx_amd import _native, indexing, vector_store, wdbx
    from wdbx_amd.config import WDBXConfig

    assert callable(_native.NativeIndex.search_rows)
    assert callable(indexing.HipFlatIndex.search_among) and callable(indexing.HipFlatIndex.search_batch_among)
    assert "search_among" not in indexing.VectorIndex.__abstractmethods__
    vs = vector_store.VectorStore
    assert callable(vs.search_among) and callable(vs.search_batch_among) and callable(vs.search_among_async)
    assert callable(wdbx.WDBX.vector_search_among) and callable(wdbx.WDBX.vector_search_batch_among)
    assert WDBXConfig.DEFAULT_CONFIG["FILTER_GATHER_MAX_ROWS"] == 0  # off: no existing call changes path


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("subset_" + request.param) / "subset_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)]
    subprocess.run(cmd, check=True)

    def run(*args, stdin=""):
        p = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return p.stdout.split("\n")
    return run


def _validate(harness, n_rows, ids):
    out = harness("validate", n_rows, len(ids), *ids)
    bad = int(out[0].split()[1])
    rows = [int(x) for x in out[1].split()[1:]] if bad == len(ids) else None
    return bad, rows


def test_validation(harness):
    assert _validate(harness, 10, []) == (0, [])                    # empty: valid
    assert _validate(harness, 0, []) == (0, [])                     # ... on an empty index too
    assert _validate(harness, 10, [0]) == (1, [0])
    assert _validate(harness, 10, [9]) == (1, [9])                  # the last row
    assert _validate(harness, 10, [10]) == (0, None)                # an entry equal to the row count
    assert _validate(harness, 10, [3, 5, 9]) == (3, [3, 5, 9])
    assert _validate(harness, 10, [3, 5, 5]) == (2, None)           # duplicate
    assert _validate(harness, 10, [3, 5, 4]) == (2, None)           # unsorted
    assert _validate(harness, 10, [5, 3]) == (1, None)
    assert _validate(harness, 10, [0, 1, 2, 11]) == (3, None)
    assert _validate(harness, 0, [0]) == (0, None)                  # nothing stored
    # the 2^32 boundary: the last row number 32 bits hold narrows to itself; 2^32 never fits, whatever the row count claims
    top = 2 ** 32
    assert _validate(harness, top, [0, top - 2, top - 1]) == (3, [0, top - 2, top - 1])
    assert _validate(harness, top + 10, [top - 1, top]) == (1, None)
    assert _validate(harness, 2 ** 63, [top + 5]) == (0, None)
    assert _validate(harness, 2 ** 64 - 1, [2 ** 64 - 2]) == (0, None)
    # a long run, every row of an index
    assert int(harness("validate_big", 100000, 0, 100000)[0].split()[1]) == 100000
    assert int(harness("validate_big", 100000, 1, 100000)[0].split()[1]) == 99999  # its last entry = the row count


def _route(n_ids, k, keys_max, select_min_k):
    if n_ids == 0:
        return NONE
    if 0 < keys_max and n_ids <= keys_max:
        return KEYS
    if 0 < select_min_k <= k:
        return SELECT
    return LISTS


@pytest.mark.parametrize("keys_max,select_min_k,lds_lists", [(8192, 200, 0), (0, 200, 0), (0, 0, 0), (64, 17, 1), (1 << 40, 0, 0)])
def test_plan_at_the_edges(harness, keys_max, select_min_k, lds_lists):
    cu = 256
    budget = (256 << 20) // 8
    cases = [(n_ids, nq, k) for n_ids in N_IDS + (10 ** 6, 10 ** 7, 2 ** 32 - 257) for k in KS for nq in NQS]
    lines = harness("plan", cu, keys_max, select_min_k, lds_lists, stdin="".join("%d %d %d\n" % c for c in cases))
    assert len([ln for ln in lines if ln]) == len(cases)
    for (n_ids, nq, k), line in zip(cases, lines):
        route, qb, rnd, blocks, P, lds, scratch = map(int, line.split())
        what = (n_ids, k, nq)
        assert route == _route(n_ids, k, keys_max, select_min_k), what
        if route == NONE:
            continue
        # a query block the kernel is instantiated for (kernels_subset.h: pick_subset_metric)
        if route == LISTS:
            reg = k <= 128 and not lds_lists
            assert qb in ((1, 4, 8) if reg else (1,)), what
            if nq > 1 and reg:
                assert qb == (8 if k <= 64 else 4), what
        else:
            assert qb in (1, 8), what
        if nq == 1:
            assert qb == 1, what  # a lone query is the block of one
        # rounds: whole query blocks, at most 256 queries, all of them when they fit
        assert 1 <= rnd <= min(nq, 256), what
        assert rnd == nq or rnd % qb == 0, what
        qblocks = -(-rnd // qb)
        # the grid: at least one workgroup, never more waves than listed rows (rounded up to a workgroup), about two
        # workgroups per CU over all query blocks
        assert 1 <= blocks <= max(1, -(-n_ids // 4)), what
        assert blocks * qblocks <= 2 * cu + qblocks, what
        if route == LISTS:
            assert P == blocks and lds == 4 * qb * k * 8 and lds <= 64 * 1024, what
            assert scratch == rnd * k * P and scratch <= budget, what
        else:
            assert P == 0 and lds == 0 and scratch == rnd * n_ids, what
            assert scratch <= budget or rnd == 1, what  # (one query's keys are the least a round can hold)
            if rnd == nq == 256 and n_ids * 256 <= budget:
                assert qb == 8, what
