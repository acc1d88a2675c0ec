#!/usr/bin/env python3
"""Distinct search (at most one row per label) on 10 M x 384 cosine, synthetic, for two label layouts -- 10 consecutive rows
per label, and the same labels scattered at random:
  * the over-fetch route (distinct_overfetch = 4) against wdbx_index_search at the same k, in ms per query (lone queries,
    wall time, alternating in one process);
  * the full pass (distinct_overfetch = 0), device time of its scoring launches per block of 8 queries (the handle's profile
    events: scoring = scan launches, ranking + merge = merge launches), against the fp32 scan_kernel's single-query time on the
    same corpus (scan_shadow = 0): both read rows * dim * 4 bytes once.

    python tools/bench_distinct.py [rows] [dim] [k] [reps] [--out FILE]

One JSON line per case on stdout; --out appends them to FILE (default profiles/distinct/results.jsonl)."""
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
out_path = Path(flags.get("--out", ROOT / "profiles" / "distinct" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)
HBM = 8e12

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


def median(v):
    return float(np.median(v))


# the fp32 scan of one query on this corpus: the yardstick of the full pass
ix.profile(True)
ix.set_option("scan_shadow", 0)
ix.search(queries[:1], k)
ix.profile_read()
scan = []
for _ in range(reps):
    ix.search(queries[:1], k)
    scan.append(ix.profile_read()["scan_ms"])
ix.set_option("scan_shadow", 2)
scan_ms = median(scan)
emit({"case": "fp32_scan_single_query", "rows": rows, "dim": dim, "k": k, "reps": reps, "scan_dev_ms": scan_ms,
      "share_of_8TBs": rows * dim * 4 / (scan_ms * 1e-3) / HBM if scan_ms > 0 else None})

consecutive = (np.arange(rows, dtype=np.uint64) // 10).astype(np.uint32)
for layout, labels in (("consecutive_10", consecutive), ("scattered_10", consecutive[rng.permutation(rows)])):
    t0 = time.perf_counter()
    ix.set_labels(0, labels)
    set_ms = (time.perf_counter() - t0) * 1e3
    # the over-fetch route against the ordinary search, lone queries
    ix.set_option("distinct_overfetch", 4)
    ix.search_distinct(queries[:1], k)
    ix.search(queries[:1], k)
    wall = {"distinct": [], "search": []}
    paths = set()
    for r in range(reps):
        q = queries[r % 8][None, :]
        t0 = time.perf_counter()
        ix.search_distinct(q, k)
        wall["distinct"].append((time.perf_counter() - t0) * 1e3)
        paths.add(ix.get_option("last_distinct_path"))
        t0 = time.perf_counter()
        ix.search(q, k)
        wall["search"].append((time.perf_counter() - t0) * 1e3)
    emit({"case": "overfetch_vs_search", "layout": layout, "rows": rows, "dim": dim, "k": k, "reps": reps,
          "distinct_ms_per_query": median(wall["distinct"]), "search_ms_per_query": median(wall["search"]),
          "paths": sorted(paths), "set_labels_ms": set_ms})
    # the full pass, a block of 8 queries (the first call builds the label order: timed apart)
    ix.set_option("distinct_overfetch", 0)
    t0 = time.perf_counter()
    full = ix.search_distinct(queries, k)
    first_ms = (time.perf_counter() - t0) * 1e3
    ix.set_option("distinct_overfetch", 4)
    same = bool(np.array_equal(full[0], ix.search_distinct(queries, k)[0]))
    ix.set_option("distinct_overfetch", 0)
    ix.profile_read()
    dev_scan, dev_rank, wall8 = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ix.search_distinct(queries, k)
        wall8.append((time.perf_counter() - t0) * 1e3)
        p = ix.profile_read()
        dev_scan.append(p["scan_ms"])
        dev_rank.append(p["merge_ms"])
    s_ms = median(dev_scan)
    emit({"case": "full_pass_block_of_8", "layout": layout, "rows": rows, "dim": dim, "k": k, "reps": reps,
          "path": ix.get_option("last_distinct_path"), "items": ix.get_option("last_distinct_items"),
          "labels": ix.get_option("last_distinct_labels"), "ids_equal_overfetch": same,
          "first_call_with_label_order_build_ms": first_ms, "wall_ms_per_block": median(wall8),
          "scoring_dev_ms_per_block": s_ms, "ranking_dev_ms_per_block": median(dev_rank),
          "fp32_scan_single_query_dev_ms": scan_ms, "scoring_over_scan": s_ms / scan_ms if scan_ms > 0 else None,
          "scoring_share_of_8TBs": rows * dim * 4 / (s_ms * 1e-3) / HBM if s_ms > 0 else None,
          "device_bytes_resident": ix.get_option("device_bytes_resident")})
    ix.set_option("distinct_overfetch", 4)
ix.close()
