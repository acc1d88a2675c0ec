#!/usr/bin/env python3
"""One row list per query in one batched call (wdbx_index_search_row_lists) against the way such a batch was answered
before: a loop of wdbx_index_search_rows, one call per query with its list.  10 M x 384 cosine, top-10, 256 queries with
their own random sorted lists of 10^2, 10^3 and 10^4 rows; both ways alternate in one process (the per-query loop is the
baseline: nothing of it changed).  Per list length: wall time per batch, device time from the handle's profile events
(scoring launches = scan launches, ranking = merge launches), the listed rows' bytes over the scoring launches' device time
as a share of 8 TB/s, and what the batch costs outside the kernels.

    python tools/bench_row_lists.py [rows] [dim] [k] [reps] [nq] [--out FILE]

One JSON line per case on stdout; --out appends them to FILE (default profiles/row_lists/results.jsonl)."""
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
k = int(args[2]) if len(args) > 2 else 10
reps = int(args[3]) if len(args) > 3 else 7
nq = int(args[4]) if len(args) > 4 else 256
out_path = Path(flags.get("--out", ROOT / "profiles" / "row_lists" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)
HBM = 8e12

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
rng = np.random.default_rng(1)
queries = rng.standard_normal((nq, dim)).astype(np.float32)
queries /= np.linalg.norm(queries, axis=1, keepdims=True)
which = np.arange(nq, dtype=np.int32)


def median(v):
    return float(np.median(v))


def loop(lists):
    out = [ix.search_rows(queries[i], k, lists[i]) for i in range(nq)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


ix.profile(True)
for n_ids in (100, 1000, 10_000):
    if n_ids > rows:
        continue
    # (sorted draws with repeats removed: a few entries short of n_ids on a small index, exactly n_ids in practice at 10 M)
    lists = [np.unique(rng.integers(0, rows, n_ids)).astype(np.uint64) for _ in range(nq)]
    listed = int(sum(len(r) for r in lists))
    a = ix.search_row_lists(queries, k, lists, which)  # warm both, and check that they agree bit for bit
    b = loop(lists)
    same = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))
    ix.profile_read()
    wall = {"lists": [], "loop": []}
    dev = {"lists_scan": [], "lists_merge": [], "loop_scan": [], "loop_merge": []}
    for _ in range(reps):  # alternating
        t0 = time.perf_counter()
        ix.search_row_lists(queries, k, lists, which)
        wall["lists"].append((time.perf_counter() - t0) * 1e3)
        p = ix.profile_read()
        dev["lists_scan"].append(p["scan_ms"])
        dev["lists_merge"].append(p["merge_ms"])
        t0 = time.perf_counter()
        loop(lists)
        wall["loop"].append((time.perf_counter() - t0) * 1e3)
        p = ix.profile_read()
        dev["loop_scan"].append(p["scan_ms"])
        dev["loop_merge"].append(p["merge_ms"])
    scan_ms, merge_ms = median(dev["lists_scan"]), median(dev["lists_merge"])
    rec = {
        "rows": rows, "dim": dim, "k": k, "n_ids": n_ids, "nq": nq, "reps": reps, "equal_per_query_loop": same,
        "lists_path": ix.get_option("last_lists_path"), "lists_items": ix.get_option("last_lists_items"),
        "lists_rounds": ix.get_option("last_lists_rounds"),
        "lists_wall_ms": median(wall["lists"]), "loop_wall_ms": median(wall["loop"]),
        "wall_ratio_loop_over_lists": median(wall["loop"]) / median(wall["lists"]),
        "lists_dev_scan_ms": scan_ms, "lists_dev_merge_ms": merge_ms,
        "loop_dev_scan_ms": median(dev["loop_scan"]), "loop_dev_merge_ms": median(dev["loop_merge"]),
        "lists_outside_kernels_ms": median(wall["lists"]) - scan_ms - merge_ms,
        "loop_outside_kernels_ms": median(wall["loop"]) - median(dev["loop_scan"]) - median(dev["loop_merge"]),
        "listed_bytes": listed * dim * 4,
        "lists_share_of_8TBs": (listed * dim * 4 / (scan_ms * 1e-3) / HBM) if scan_ms > 0 else None,
    }
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")
ix.close()
