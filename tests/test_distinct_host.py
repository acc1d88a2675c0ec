"""Distinct search (exact top-k with at most one row per label), the parts that need no GPU: the C ABI surface, the public
layers, and the device-free host side (wdbx-py_amd/csrc/host_labels.h: the label order with its spans, items and tables, the
over-fetch and its host walk, rounds / grids / scratch of the full pass) driven by tests/host_harness/labels_harness.cpp --
built once plain and once under -fsanitize=address,undefined."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "labels_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"
NONE = 0xFFFFFFFF
SPAN = 64
ARITY = {"wdbx_index_set_labels": 4, "wdbx_index_get_labels": 4, "wdbx_index_search_distinct": 10}


def test_header_binding_and_library_agree_on_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    from wdbx_amd import _native

    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    lib = ctypes.CDLL(str(path))
    doc = (ROOT / "INTEGRATION.md").read_text()
    for name, arity in ARITY.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert len(m.group(1).split(",")) == arity, name
        res, args = _native.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == arity, name
        assert hasattr(lib, name), name
        assert f"`{name}`" in doc[doc.index("## F. Every symbol"):], name
    assert re.search(r"#define\s+WDBX_LABEL_NONE\s+0xFFFFFFFFu", text) and _native.LABEL_NONE == NONE


def test_public_layers_have_the_entry_points():
    from wdbx_amd import _native, api, indexing, vector_store, wdbx
    from wdbx_amd.config import WDBXConfig

    for name in ("set_labels", "get_labels", "search_distinct"):
        assert callable(getattr(_native.NativeIndex, name))
    assert callable(indexing.HipFlatIndex.set_labels) and callable(indexing.HipFlatIndex.search_distinct)
    vs = vector_store.VectorStore
    assert callable(vs.search_distinct) and callable(vs.search_distinct_async)
    assert callable(wdbx.WDBX.vector_search_distinct) and callable(wdbx.WDBX.vector_search_distinct_async)
    assert "distinct" in api.search_endpoint.__doc__
    assert WDBXConfig.DEFAULT_CONFIG["DISTINCT_KEY"] is None  # off: no existing call changes


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("labels_" + request.param) / "labels_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args, stdin=""):
        p = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return p.stdout.split("\n")
    return run


def _layouts():
    rng = np.random.default_rng(7)
    out = {}
    for n in (0, 1, 63, 64, 65, 257, 5000):
        out[f"none_{n}"] = np.full(n, NONE, np.uint64)
        out[f"one_label_{n}"] = np.full(n, 7, np.uint64)
        runs = np.repeat(np.arange(n), rng.integers(1, 10, size=max(n, 1)))[:n]  # runs of 1 .. 9
        out[f"runs_{n}"] = runs.astype(np.uint64)
        out[f"scattered_{n}"] = rng.integers(0, 300, size=n).astype(np.uint64)   # 300 labels at random
    big = np.arange(5000, dtype=np.uint64) + 10
    big[rng.choice(5000, 4000, replace=False)] = 3                               # one label of 4000 rows among singletons
    out["big_label"] = big
    out["values"] = np.array([0, 7, 4_000_000_000] * 50 + [NONE] * 5 + [0, 4_000_000_000], np.uint64)
    for run in (SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1):                         # run lengths around the span
        out[f"run_{run}"] = np.concatenate([np.full(run, 5), np.arange(100, 103), np.full(run, 9), [NONE, NONE]]).astype(np.uint64)
        out[f"run_{run}_shifted"] = np.concatenate([[1], np.full(run, 5), [2, 2], np.full(run, 9)]).astype(np.uint64)
    # labels set for a prefix of the rows only: the rest are NONE
    out["prefix"] = np.array([4, 4, 9, 4], np.uint64)
    return out


LAYOUTS = _layouts()


def _order(harness, labels, n=None):
    n = len(labels) if n is None else n
    lines = harness("order", stdin="%d %d\n%s\n" % (n, len(labels), " ".join(map(str, labels.tolist()))))
    n_labels, n_items, n_spans = map(int, lines[0].split())
    arr = [np.array(ln.split(), dtype=np.int64) for ln in lines[1:5]]
    return n_labels, n_items, n_spans, arr[0], arr[1], arr[2], arr[3]


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_label_order(harness, name):
    labels = LAYOUTS[name]
    n = len(labels) + (3 if name == "prefix" else 0)
    full = np.concatenate([labels, np.full(n - len(labels), NONE, np.uint64)])
    n_labels, n_items, n_spans, rows, dense, span_item0, label_item0 = _order(harness, labels, n)
    assert n_spans == -(-n // SPAN) and len(rows) == len(dense) == n
    assert len(span_item0) == n_spans + 1 and len(label_item0) == n_labels + 1
    # a permutation sorted by (label, row)
    assert sorted(rows.tolist()) == list(range(n))
    keys = [(int(full[r]), int(r)) for r in rows]
    assert keys == sorted(keys)
    # dense numbering: a new number exactly where the label changes, every NONE row its own
    lab = full[rows] if n else full
    new = np.ones(n, bool)
    if n:
        new[1:] = (lab[1:] != lab[:-1]) | (lab[1:] == NONE)
        assert np.array_equal(dense, np.cumsum(new) - 1)
    assert n_labels == int(new.sum())
    distinct = len(set(full[full != NONE].tolist())) + int((full == NONE).sum())
    assert n_labels == distinct
    # items: maximal runs of one dense label inside one span, numbered in position order
    item_of = np.zeros(n, np.int64)
    start = new | (np.arange(n) % SPAN == 0)
    if n:
        item_of = np.cumsum(start) - 1
    assert n_items == int(start.sum())
    for it in range(n_items):                     # never across a span or a label boundary
        pos = np.nonzero(item_of == it)[0]
        assert len(pos) and len(set((pos // SPAN).tolist())) == 1 and len(set(dense[pos].tolist())) == 1
        assert np.array_equal(pos, np.arange(pos[0], pos[-1] + 1))
    assert span_item0[-1] == n_items and label_item0[-1] == n_items
    for s in range(n_spans):
        assert span_item0[s] == item_of[s * SPAN]
    for l in range(n_labels):                     # every label's items are consecutive: [label_item0[l], label_item0[l + 1])
        its = sorted(set(item_of[dense == l].tolist()))
        assert its == list(range(int(label_item0[l]), int(label_item0[l + 1]))), (l, its)
    assert n_labels <= n_items <= n_labels + n_spans


def test_plan_keeps_scratch_within_budget(harness):
    budget = (256 << 20) // 8
    shapes = []
    for name, labels in LAYOUTS.items():
        if len(labels):
            n_labels, n_items, n_spans = _order(harness, labels)[:3]
            shapes.append((n_items, n_labels, n_spans))
    shapes += [(1_160_000, 1_000_000, 156_250), (10_000_000, 10_000_000, 156_250), (40_000_000, 40_000_000, 625_000)]
    for cu, sel in ((256, 200), (256, 0), (8, 17)):
        cases = [(i, l, s, nq, k) for (i, l, s) in shapes for nq in (1, 8, 9, 256, 1000) for k in (1, 10, 200, 2048)]
        lines = harness("plan", cu, sel, stdin="".join("%d %d %d %d %d\n" % c for c in cases))
        assert len([ln for ln in lines if ln]) == len(cases)
        for (n_items, n_labels, n_spans, nq, k), line in zip(cases, lines):
            qb, rnd, select, sblocks, rblocks, lds, keys, rank = map(int, line.split())
            what = (n_items, n_labels, nq, k, cu, sel)
            assert select == int(0 < sel <= k), what
            assert qb in (1, 8) and (qb == 1 if nq == 1 else True), what
            assert 1 <= rnd <= min(nq, 256) and (rnd == nq or rnd % qb == 0), what
            assert 1 <= rblocks <= max(1, min(-(-n_labels // 2048), 2 * cu)), what
            qblocks = -(-rnd // qb)
            assert 1 <= sblocks <= max(1, -(-n_spans // 4)) and sblocks * qblocks <= 2 * cu + qblocks, what
            assert keys == rnd * n_items, what
            assert rank == rnd * (n_labels if select else k * rblocks), what
            assert lds == (0 if select else 4 * k * 8) and lds <= 64 * 1024, what
            assert keys + rank <= budget or rnd == 1, what  # (one query's keys are the least a round can hold)
            if n_items <= 5100:
                assert keys + rank <= budget, what
                if nq in (8, 9, 256):
                    assert qb == 8 and rnd == nq, what


def test_overfetch_k(harness):
    cases = [(0, 10, 4, 0), (5000, 10, 4, 40), (5000, 10, 0, 0), (5000, 10, -1, 0), (30, 10, 4, 30), (5, 10, 4, 5),
             (10 ** 7, 600, 4, 2048), (10 ** 7, 2048, 1, 2048), (10 ** 7, 1, 1, 1), (10 ** 7, 3, 10 ** 12, 2048)]
    lines = harness("overfetch", stdin="".join("%d %d %d\n" % c[:3] for c in cases))
    assert [int(x) for x in lines if x] == [c[3] for c in cases]


def _walk(harness, labels, ranked, n_rows, k):
    stdin = "%d\n%s\n%s\n" % (len(labels), " ".join(map(str, labels)), " ".join("%d %g" % p for p in ranked))
    lines = harness("walk", len(ranked), n_rows, k, stdin=stdin)
    return (int(lines[0]), [int(x) for x in lines[1].split()], [float(x) for x in lines[2].split()], [int(x) for x in lines[3].split()])


def test_overfetch_walk(harness):
    labels = [5, 5, 7, NONE, 7, 5]  # rows 6, 7 carry no label at all (behind the set prefix)
    ranked = [(1, 9.0), (0, 8.0), (3, 7.0), (4, 6.0), (7, 5.0), (2, 4.0)]
    # two labels wanted, found among the first three: final
    assert _walk(harness, labels, ranked, 100, 2) == (1, [1, 3], [9.0, 7.0], [5, NONE])
    # four found of five wanted, rows remain unseen: not final
    fin, rows, scores, labs = _walk(harness, labels, ranked, 100, 5)
    assert (fin, rows, labs) == (0, [1, 3, 4, 7, -1], [5, NONE, 7, NONE, NONE]) and scores[4] == 0.0
    # ... but final when the ranking reached every row, or ended in an unused slot
    assert _walk(harness, labels, ranked, 6, 5)[0] == 1
    assert _walk(harness, labels, ranked[:3] + [(-1, 0.0)], 100, 5) == (1, [1, 3, -1, -1, -1], [9.0, 7.0, 0.0, 0.0, 0.0], [5, NONE] + [NONE] * 3)
