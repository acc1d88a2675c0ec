"""Search groups (the k best labels, each with its best group_size rows), the parts that need no GPU: the C ABI surface, the
public layers, and the device-free host side (wdbx-py_amd/csrc/host_groups.h: the runs of the label order, the dense label of a
label value, the tasks and the slot table of a call, the rounds) driven by tests/host_harness/groups_harness.cpp -- built once
plain and once under -fsanitize=address,undefined."""
import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "groups_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"
NONE = 0xFFFFFFFF
ARITY = {"wdbx_index_search_groups": 12, "wdbx_index_search_group_members": 13}
BUDGET = 256 << 20


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
    assert re.search(r"#define\s+WDBX_MAX_GROUP_SIZE\s+64\b", text) and _native.MAX_GROUP_SIZE == 64


def test_public_layers_have_the_entry_points():
    from wdbx_amd import _native, api, indexing, vector_store, wdbx

    for name in ("search_groups", "search_group_members"):
        assert callable(getattr(_native.NativeIndex, name))
    assert callable(indexing.HipFlatIndex.search_groups) and callable(indexing.HipFlatIndex.group_members)
    vs = vector_store.VectorStore
    assert callable(vs.search_groups) and callable(vs.search_groups_async)
    assert callable(wdbx.WDBX.vector_search_groups) and callable(wdbx.WDBX.vector_search_groups_async)
    assert "group_size" in api.search_endpoint.__doc__


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("groups_" + request.param) / "groups_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args, stdin=""):
        p = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return p.stdout.split("\n")
    return run


def _layouts():
    rng = np.random.default_rng(11)
    out = {}
    sparse = np.array([0, 7, 4_000_000_000, 123_456_789, 4_294_967_294], np.uint64)  # (the last: the largest value a label has)
    lab = sparse[rng.integers(0, len(sparse), size=400)]
    lab[rng.choice(400, 60, replace=False)] = NONE  # NONE rows interleaved
    out["sparse"] = (lab, 400)
    out["single_label"] = (np.full(37, 9, np.uint64), 37)
    out["single_row"] = (np.array([5], np.uint64), 1)
    out["all_none"] = (np.full(20, NONE, np.uint64), 20)
    out["prefix"] = (np.array([4, 4, 9, 4, NONE, 2], np.uint64), 11)  # rows behind the set prefix are NONE
    out["runs"] = (np.repeat(np.arange(100) * 3 + 1, rng.integers(1, 8, size=100)).astype(np.uint64), None)
    out["empty"] = (np.zeros(0, np.uint64), 0)
    return {k: (v, len(v) if n is None else n) for k, (v, n) in out.items()}


LAYOUTS = _layouts()


def _stdin(labels, n, tail):
    return "%d %d\n%s\n%s\n" % (n, len(labels), " ".join(map(str, labels.tolist())), tail)


def _brute(labels, n):
    """label value -> sorted rows; the label order (rows by (label, row))"""
    full = np.concatenate([labels, np.full(n - len(labels), NONE, np.uint64)])
    order = sorted(range(n), key=lambda r: (int(full[r]), r))
    by_label = {}
    for r in range(n):
        if full[r] != NONE:
            by_label.setdefault(int(full[r]), []).append(r)
    return full, order, by_label


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_dense_label_lookup_against_a_brute_force_map(harness, name):
    labels, n = LAYOUTS[name]
    full, order, by_label = _brute(labels, n)
    probes = sorted(by_label) + [1, 8, 4_294_967_293, 4_294_967_294, NONE, 0]
    lines = harness("runs", stdin=_stdin(labels, n, "%d\n%s" % (len(probes), " ".join(map(str, probes)))))
    n_labels, n_labelled = map(int, lines[0].split())
    pos0 = [int(x) for x in lines[1].split()]
    assert n_labelled == len(by_label) and n_labels == len(by_label) + int((full == NONE).sum())
    assert len(pos0) == n_labels + 1 and pos0[-1] == n and pos0 == sorted(pos0)
    for d, value in enumerate(sorted(by_label)):  # labelled labels ascend by value, their runs hold exactly their rows
        assert [order[p] for p in range(pos0[d], pos0[d + 1])] == by_label[value]
    for d in range(n_labelled, n_labels):         # every NONE row a run of one
        assert pos0[d + 1] - pos0[d] == 1 and full[order[pos0[d]]] == NONE
    for value, line in zip(probes, lines[2:]):
        dense, start, count = map(int, line.split())
        if value in by_label:
            assert dense == sorted(by_label).index(value)
            assert [order[p] for p in range(start, start + count)] == by_label[value]
        else:
            assert (dense, start, count) == (-1, 0, 0), value


def test_slots_from_labels_and_rows(harness):
    labels, n = LAYOUTS["sparse"]
    full, order, by_label = _brute(labels, n)
    none_row = int(np.nonzero(full == NONE)[0][3])
    pairs = [(7, 0), (7, 399), (4_294_967_294, 5), (NONE, none_row), (NONE, 12), (7, -1), (NONE, -1), (55, 3)]
    lines = harness("slots", stdin=_stdin(labels, n, "%d\n%s" % (len(pairs), " ".join("%d %d" % p for p in pairs))))
    got = [tuple(map(int, ln.split())) for ln in lines if ln]
    for (label, row), (start, count, direct) in zip(pairs, got):
        if row < 0 or (label != NONE and label not in by_label):
            assert (count, direct) == (0, 0)       # unused, or a label the handle does not hold: nothing to rank
        elif label == NONE:
            assert (start, count, direct) == (row, 1, 1)  # the row itself, whatever label it carries
        else:
            assert direct == 0 and [order[p] for p in range(start, start + count)] == by_label[label]
    # a handle without labels: every labelled slot ranks nothing, every unlabelled one its row
    lines = harness("slots", stdin=_stdin(np.zeros(0, np.uint64), 50, "3\n7 3\n%d 49\n%d -1" % (NONE, NONE)))
    assert [ln for ln in lines if ln] == ["0 0 0", "49 1 1", "0 0 0"]


@pytest.mark.parametrize("seg", [4, 2048])
def test_task_cutting(harness, seg):
    k = 3
    runs = [1, seg - 1, seg, seg + 1, 2 * seg + 3]
    slots, start = [], 100
    for r in runs:
        slots.append((start, r, 0))
        start += r
    slots += [(17, 1, 1), (0, 0, 0), (4242, 1, 1), (0, 0, 0)]  # direct rows and unused slots, two queries and a half of k = 3
    lines = harness("tasks", k, seg, stdin="%d\n%s\n" % (len(slots), "\n".join("%d %d %d" % s for s in slots)))
    n_tasks = int(lines[0])
    tasks = [tuple(map(int, ln.split())) for ln in lines[1:1 + n_tasks]]
    slot_task0 = [int(x) for x in lines[1 + n_tasks].split()]
    assert len(slot_task0) == len(slots) + 1 and slot_task0[0] == 0 and slot_task0[-1] == n_tasks
    assert slot_task0 == sorted(slot_task0)  # monotone: every task belongs to exactly one slot
    for s, (st, count, direct) in enumerate(slots):
        mine = tasks[slot_task0[s]:slot_task0[s + 1]]
        assert all(t[0] == s // k for t in mine)
        if direct:
            assert mine == [(s // k, st, 1, 1)]
        elif count == 0:
            assert mine == []
        else:
            assert len(mine) == -(-count // seg)
            assert all(t[3] == 0 and 1 <= t[2] <= seg for t in mine)
            assert all(t[2] == seg for t in mine[:-1])          # only the last segment may be short
            covered = [p for t in mine for p in range(t[1], t[1] + t[2])]
            assert covered == list(range(st, st + count))       # every position once, in order


def _plan(harness, slot_task0, g, budget=BUDGET):
    lines = harness("plan", g, budget, stdin="%d\n%s\n" % (len(slot_task0) - 1, " ".join(map(str, slot_task0))))
    return [tuple(map(int, ln.split())) for ln in lines if ln]


def test_plan_rounds_respect_the_budget(harness):
    rng = np.random.default_rng(3)
    for g in (1, 3, 64):
        for counts in ([1] * 10, [0] * 7, rng.integers(0, 5, size=2000).tolist(), [489] * 80, [10 ** 6, 1, 10 ** 6, 0, 5],
                       rng.integers(0, 300_000, size=300).tolist()):
            slot_task0 = np.concatenate([[0], np.cumsum(counts)]).tolist()
            rounds = _plan(harness, slot_task0, g)
            # the rounds tile the slots and the tasks, in order
            assert rounds[0][0] == 0 and rounds[-1][1] == len(counts)
            for a, b in zip(rounds, rounds[1:]):
                assert a[1] == b[0]
            for slot0, slot1, task0, tasks, merge_blocks, nbytes in rounds:
                assert slot1 > slot0 and task0 == slot_task0[slot0] and tasks == slot_task0[slot1] - task0
                assert merge_blocks == -(-(slot1 - slot0) // 4)
                assert nbytes == tasks * (8 * g + 16) + (slot1 - slot0 + 1) * 8
                assert nbytes <= BUDGET or slot1 - slot0 == 1, (g, slot0, slot1)
                if slot1 < len(counts):  # greedy: the next slot would not have fitted
                    more = slot_task0[slot1 + 1] - task0
                    assert more * (8 * g + 16) + (slot1 - slot0 + 2) * 8 > BUDGET
    # ten queries' worth of small slots: one round
    assert len(_plan(harness, list(range(0, 101)), 3)) == 1


def test_one_oversized_slot_still_runs(harness):
    budget = 4096
    slot_task0 = [0, 2, 2, 1000, 1001, 1003]  # slot 2 alone needs 998 * (8 * 3 + 16) bytes
    rounds = _plan(harness, slot_task0, 3, budget)
    assert [(r[0], r[1]) for r in rounds] == [(0, 2), (2, 3), (3, 5)]
    assert rounds[1][3] == 998 and rounds[1][5] > budget
    assert all(r[5] <= budget for r in (rounds[0], rounds[2]))
