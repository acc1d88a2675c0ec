#!/usr/bin/env python3
"""Search groups (the k best labels, each with its best group_size rows) on 10 M x 384 cosine, synthetic, k = 10,
group_size = 3, labels of about 20 scattered rows: one query and a block of 8 --
  * wall ms per call of wdbx_index_search_groups;
  * in the same run and on the same handle, what a caller composed before: one wdbx_index_search_distinct plus, per query and
    slot, one wdbx_index_search_rows over the rows of the slot's label (row lists prepared outside the timed region);
  * wdbx_index_search_distinct alone (stage 1);
and once the degenerate case, 10 labels of rows / 10 rows each, where stage 2 reads the corpus once per query.

    python tools/bench_groups.py [rows] [dim] [reps] [--out FILE]

One JSON line per case on stdout; --out appends them to FILE (default profiles/groups/results.jsonl).  Nothing is a threshold."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "wdbx-py_amd"))
from wdbx_amd import _native  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
flags = {sys.argv[i]: sys.argv[i + 1] for i in range(1, len(sys.argv) - 1) if sys.argv[i].startswith("--")}
args = [a for a in args if a not in flags.values()]
rows = int(args[0]) if len(args) > 0 else 10_000_000
dim = int(args[1]) if len(args) > 1 else 384
reps = int(args[2]) if len(args) > 2 else 7
out_path = Path(flags.get("--out", ROOT / "profiles" / "groups" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)
K, G = 10, 3

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
rng = np.random.default_rng(1)
queries = rng.standard_normal((8, dim)).astype(np.float32)
queries /= np.linalg.norm(queries, axis=1, keepdims=True)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def timed(call):
    call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall)), float(np.min(wall))


def run(case, labels):
    t0 = time.perf_counter()
    ix.set_labels(0, labels)
    ix.search_groups(queries[:1], K, G)  # (builds the label order)
    build_s = time.perf_counter() - t0
    order = np.argsort(labels, kind="stable")
    sorted_labels = labels[order]
    for nq in (1, 8):
        q = queries[:nq]
        idx, score, lab, cnt = ix.search_groups(q, K, G)
        lists = [[np.sort(order[np.searchsorted(sorted_labels, l, "left"):np.searchsorted(sorted_labels, l, "right")])
                  for l in lab[i]] for i in range(nq)]

        def composed():
            ix.search_distinct(q, K)
            return [[ix.search_rows(q[i:i + 1], G, ids) for ids in lists[i]] for i in range(nq)]

        parts = composed()
        same = all(np.array_equal(parts[i][s][0][0], idx[i, s]) and np.array_equal(parts[i][s][1][0].view(np.uint32), score[i, s].view(np.uint32))
                   for i in range(nq) for s in range(K))
        g_med, g_min = timed(lambda: ix.search_groups(q, K, G))
        tasks, rounds = ix.get_option("last_groups_tasks"), ix.get_option("last_groups_rounds")
        c_med, c_min = timed(composed)
        d_med, d_min = timed(lambda: ix.search_distinct(q, K))
        emit({"case": case, "rows": rows, "dim": dim, "k": K, "group_size": G, "nq": nq, "reps": reps,
              "label_order_build_s": build_s, "rows_per_group": float(np.mean([len(x) for r in lists for x in r])),
              "groups_wall_ms": g_med, "groups_wall_ms_min": g_min, "composed_wall_ms": c_med, "composed_wall_ms_min": c_min,
              "distinct_wall_ms": d_med, "distinct_wall_ms_min": d_min, "groups_over_distinct": g_med / d_med,
              "composed_over_groups": c_med / g_med, "tasks": tasks, "rounds": rounds,
              "distinct_path": ix.get_option("last_distinct_path"), "equal_to_composition": bool(same)})


run("labels_of_20", rng.integers(0, max(rows // 20, 1), size=rows).astype(np.uint32))
run("ten_labels", (np.arange(rows) % 10).astype(np.uint32))
ix.close()
