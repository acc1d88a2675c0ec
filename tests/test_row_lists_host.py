"""Batched search among listed rows with one row list per query, the parts that need no GPU: the C ABI surface, the public
layers, and the device-free planner (wdbx-py_amd/csrc/host_rowlists.h: CSR check, list validation, routes, slots, rounds,
query blocks, work items) driven by tests/host_harness/rowlists_harness.cpp -- built once plain and once under
-fsanitize=address,undefined.  The planner's output is checked against the properties the kernel and the ranking launch rely
on, not against a second implementation of it."""
import ctypes
import random
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wdbx_hip.h"
HARNESS = ROOT / "tests" / "host_harness" / "rowlists_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"

CHUNK = 256
ROUND_SLOTS = 256
ROUND_KEYS = (256 << 20) // 8
UNUSED, PASS, FALLBACK = 0, 1, 2
OK, BAD_ARG, BAD_OFFSET, BAD_QUERY = 0, 1, 2, 3


def test_header_binding_and_library_declare_search_row_lists():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bwdbx_index_search_row_lists\s*\(", text)
    from wdbx_amd import _native

    res, args = _native.SIGNATURES["wdbx_index_search_row_lists"]
    assert res is ctypes.c_int and len(args) == 11
    path = _native.library_path()
    if not path.exists():
        subprocess.run(["make", "-C", str(INC), "all"], check=True)
    assert hasattr(ctypes.CDLL(str(path)), "wdbx_index_search_row_lists")
    assert f"constexpr uint32_t ROWLISTS_CHUNK = {CHUNK};" in (INC / "host_rowlists.h").read_text()


def test_public_layers_have_the_entry_points():
    from wdbx_amd import _native, api, indexing, vector_store, wdbx
    from wdbx_amd.config import WDBXConfig

    assert callable(_native.NativeIndex.search_row_lists)
    ix = indexing.HipFlatIndex
    assert callable(ix.search_row_lists_raw) and callable(ix.search_batch_among_each) and ix.supports_row_lists is True
    assert callable(vector_store.VectorStore.search_batch_among_each)
    assert callable(wdbx.WDBX.vector_search_batch_among_each)
    assert "vector_id_lists" in api.search_batch_endpoint.__doc__
    assert WDBXConfig.DEFAULT_CONFIG["FILTER_GATHER_PER_QUERY"] is False  # off: no existing call changes path


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("rowlists_" + request.param) / "rowlists_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)]
    subprocess.run(cmd, check=True)

    def run(*args, stdin=""):
        p = subprocess.run([str(exe), *map(str, args)], input=stdin, capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return p.stdout.split("\n")
    return run


def _pair(lengths, which):
    offsets = [0]
    for n in lengths:
        offsets.append(offsets[-1] + n)
    return offsets, "%d %d\n%s\n%s\n" % (len(lengths), len(which), " ".join(map(str, offsets)), " ".join(map(str, which)))


def test_check_of_the_csr_pair(harness):
    def check(offsets, which):
        text = "%d %d\n%s\n%s\n" % (len(offsets) - 1, len(which), " ".join(map(str, offsets)), " ".join(map(str, which)))
        code, where = map(int, harness("check", stdin=text)[0].split()[1:])
        return code, where

    assert check([0, 3, 3, 10], [0, 2, 1, 2]) == (OK, -1)
    assert check([0, 0], [0]) == (OK, -1)                       # one empty list
    assert check([1, 3], [0]) == (BAD_OFFSET, 0)                # does not start at 0
    assert check([0, 5, 4, 9], [0]) == (BAD_OFFSET, 2)          # decreasing: names the offset that falls
    assert check([0, 5, 9, 8], [0]) == (BAD_OFFSET, 3)
    assert check([0, 5], [0, -1, 0]) == (BAD_QUERY, 1)          # no "-1 = every row" here
    assert check([0, 5], [0, 0, 1]) == (BAD_QUERY, 2)           # = n_lists
    assert check([0, 5, 4], [7]) == (BAD_OFFSET, 2)             # offsets are looked at first
    assert check([0], [0])[0] == BAD_ARG                        # n_lists == 0: every query needs a list
    assert check([0, 5], [])[0] == BAD_ARG                      # nq == 0


def test_validation_names_the_first_offending_list_and_entry(harness):
    def validate(n_rows, lists):
        offsets, _ = _pair([len(r) for r in lists], [0])
        text = "%d\n%s\n%s\n" % (len(lists), " ".join(map(str, offsets)), " ".join(str(r) for rows in lists for r in rows))
        out = harness("validate", n_rows, stdin=text)[0].split()
        return out[0] == "valid" or (int(out[1]), int(out[2]))

    assert validate(10, [[0, 1, 9], [], [3]]) is True
    assert validate(10, [[]]) is True
    assert validate(0, [[], []]) is True
    assert validate(10, [[0, 1, 9], [], [3, 3]]) == (2, 1)            # a duplicate
    assert validate(10, [[0, 1, 9], [5, 4], [3, 3]]) == (1, 1)        # unsorted; the FIRST offending list
    assert validate(10, [[0, 10]]) == (0, 1)                          # a row equal to the row count
    assert validate(10, [[2], [10]]) == (1, 0)
    assert validate(10, [[9], [0]]) is True                           # order holds inside a list only: lists may overlap
    assert validate(2 ** 33, [[1], [2 ** 32]]) == (1, 0)              # never fits 32-bit row keys
    assert validate(3, [[0, 1, 2, 3, 4]]) == (0, 3)                   # more entries than rows


def _plan(harness, lengths, which, keys_max):
    offsets, text = _pair(lengths, which)
    lines = harness("plan", keys_max, stdin=text)
    if lines[0] == "refused":
        return None
    head = lines[0].split()
    assert head[0] == "plan"
    plan = {"qb": int(head[1]), "path": int(head[2]), "pass_ids": int(head[3]), "slots": int(head[4]), "offsets": offsets}
    for name, line in zip(("routes", "bases", "slot_query", "slot_len"), lines[1:5]):
        parts = line.split()
        assert parts[0] == name, line
        plan[name] = list(map(int, parts[1:]))
    plan["rounds"] = [tuple(map(int, ln.split()[1:])) for ln in lines[5:] if ln.startswith("round ")]
    plan["items"] = [tuple(map(int, ln.split()[1:])) for ln in lines[5:] if ln.startswith("item ")]
    return plan


def _check_plan(plan, lengths, which, keys_max):
    n_lists, nq = len(lengths), len(which)
    named = set(which)
    # the route of each list follows rows_keys_max; a list no query names has none
    for l in range(n_lists):
        want = UNUSED if l not in named else (PASS if 0 < keys_max and lengths[l] <= keys_max else FALLBACK)
        assert plan["routes"][l] == want, (l, lengths[l], keys_max)
    on_pass = [q for q in range(nq) if plan["routes"][which[q]] == PASS]
    # the uploaded id array: the pass lists back to back, in list order
    base = 0
    for l in range(n_lists):
        if plan["routes"][l] == PASS:
            assert plan["bases"][l] == base
            base += lengths[l]
    assert plan["pass_ids"] == base
    # slots: a bijection onto the queries of the pass, ordered by list, the caller's order kept inside a list
    sq = plan["slot_query"]
    assert plan["slots"] == len(sq) == len(on_pass) and sorted(sq) == on_pass
    assert [(which[q], q) for q in sq] == sorted((which[q], q) for q in on_pass)
    assert plan["slot_len"] == [lengths[which[q]] for q in sq]
    most = max([sum(1 for q in on_pass if which[q] == l) for l in named] + [0])
    assert plan["qb"] == (8 if most > 1 else 1)
    # rounds: consecutive, cover every slot, 256 slots and the byte budget (a lone slot may exceed it), stride = longest list
    slot_round = {}
    nxt_slot, nxt_item = 0, 0
    for r, (slot0, slots, item0, items, stride) in enumerate(plan["rounds"]):
        assert slot0 == nxt_slot and item0 == nxt_item and 1 <= slots <= ROUND_SLOTS
        assert stride == max([1] + plan["slot_len"][slot0:slot0 + slots])
        assert slots * stride <= ROUND_KEYS or slots == 1
        for s in range(slot0, slot0 + slots):
            slot_round[s] = r
        nxt_slot, nxt_item = slot0 + slots, item0 + items
    assert nxt_slot == len(sq) and nxt_item == len(plan["items"])
    # items: every (query, listed entry) pair of the pass exactly once; no block mixes lists; keys inside slots x stride
    seen = set()
    for r, (slot0, slots, item0, items, stride) in enumerate(plan["rounds"]):
        for first, n, slot, bq, offset in plan["items"][item0:item0 + items]:
            assert 1 <= n <= CHUNK and 1 <= bq <= plan["qb"] and slot + bq <= slots
            lists = {which[sq[slot0 + slot + b]] for b in range(bq)}
            assert len(lists) == 1
            l = lists.pop()
            assert offset % CHUNK == 0 and offset + n <= lengths[l] and (n == CHUNK or offset + n == lengths[l])
            assert first == plan["bases"][l] + offset and first + n <= plan["pass_ids"]
            assert (slot + bq - 1) * stride + offset + n - 1 < slots * stride
            for b in range(bq):
                pair = (sq[slot0 + slot + b], offset)
                assert pair not in seen
                seen.add(pair)
    want = {(q, off) for q in on_pass for off in range(0, lengths[which[q]], CHUNK)}
    assert seen == want
    has_fallback = any(rt == FALLBACK for rt in plan["routes"])
    assert plan["path"] == ((2 if has_fallback else 1) if plan["items"] else (3 if has_fallback else 0))


EDGE_LENGTHS = (0, 1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 8192)


@pytest.mark.parametrize("keys_max", [8192, 0, 64, 256, 1 << 40])
def test_plan_over_edge_and_random_tables(harness, keys_max):
    rng = random.Random(1234 + keys_max % 977)
    tables = []
    # every edge length with 1 / 8 / 9 / 17 queries per list, interleaved in caller order
    for per in (1, 8, 9, 17):
        which = [l for _ in range(per) for l in range(len(EDGE_LENGTHS))]
        tables.append((list(EDGE_LENGTHS), which))
    tables.append(([5], [0]))                        # one query, one list
    tables.append(([0, 0], [1, 0, 1]))               # empty lists only
    tables.append(([7, 9, 0], [1] * 300))            # one list, more queries than a round holds
    tables.append(([64] * 40, [l % 40 for l in range(300)]))
    tables.append(([64] * 300, list(range(300))))    # a list per query: the block of one, two rounds
    for _ in range(12):
        n_lists = rng.randint(1, 40)
        lengths = [rng.choice(EDGE_LENGTHS) for _ in range(n_lists)]
        nq = rng.randint(1, 300)
        which = [rng.randrange(n_lists) for _ in range(nq)]
        tables.append((lengths, which))
    for lengths, which in tables:
        plan = _plan(harness, lengths, which, keys_max)
        assert plan is not None
        _check_plan(plan, lengths, which, keys_max)


def test_rounds_respect_the_byte_budget(harness):
    # 200 000 keys per slot: 167 slots fill 256 MiB, so 100 queries on each of three lists take two rounds by bytes alone
    lengths, which = [200000] * 3, [l for l in range(3) for _ in range(100)]
    plan = _plan(harness, lengths, which, 1 << 40)
    _check_plan(plan, lengths, which, 1 << 40)
    assert [r[1] for r in plan["rounds"]] == [167, 133]
    # a list of its own beyond the budget still gets a round (one slot), and the short lists behind it pack again
    lengths, which = [ROUND_KEYS + 5, 10, 10], [0, 1, 2]
    plan = _plan(harness, lengths, which, 1 << 40)
    _check_plan(plan, lengths, which, 1 << 40)
    assert [r[1] for r in plan["rounds"]] == [1, 2]
