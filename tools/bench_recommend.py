#!/usr/bin/env python3
"""Recommend search (rows ranked by positive and negative examples) on 10 M x 384 cosine, synthetic, k = 10: one query with
1+0, 3+1, 8+8 and 32+32 examples (positives + negatives) --
  * wall ms per call of wdbx_index_search_recommend and the device time of its scoring launches (bracketed as scan launches);
  * in the same run and on the same handle, wdbx_index_search with scan_shadow = 0: the fp32 scan of ONE vector, which reads
    the same N * pitch * 4 bytes once and is the floor;
  * the ratio of the two per example count.

    python tools/bench_recommend.py [rows] [dim] [reps] [--out FILE]

One JSON line per case on stdout; --out appends them to FILE (default profiles/recommend/results.jsonl).  Nothing is a
threshold."""
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
reps = int(args[2]) if len(args) > 2 else 5
out_path = Path(flags.get("--out", ROOT / "profiles" / "recommend" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)
K = 10

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
rng = np.random.default_rng(1)
examples = rng.standard_normal((64, dim)).astype(np.float32)
examples /= np.linalg.norm(examples, axis=1, keepdims=True)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def timed(call):
    call()
    ix.profile_read()
    wall, scan, merge = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        p = ix.profile_read()
        scan.append(p["scan_ms"])
        merge.append(p["merge_ms"])
    return float(np.median(wall)), float(np.median(scan)), float(np.median(merge))


ix.profile(True)
ix.set_option("scan_shadow", 0)
floor_wall, floor_scan, floor_merge = timed(lambda: ix.search(examples[:1], K))
bytes_read = rows * ix.pitch * 4
emit({"case": "fp32_scan_floor", "rows": rows, "dim": dim, "k": K, "reps": reps, "wall_ms": floor_wall, "scan_dev_ms": floor_scan,
      "merge_dev_ms": floor_merge, "bytes_read": bytes_read, "scan_gb_per_s": bytes_read / floor_scan / 1e6 if floor_scan else None})
for npos, nneg in ((1, 0), (3, 1), (8, 8), (32, 32)):
    v = examples[: npos + nneg]
    off = [0, npos, npos + nneg]
    wall, scan, merge = timed(lambda: ix.search_recommend(v, off, K))
    emit({"case": "recommend", "rows": rows, "dim": dim, "k": K, "positives": npos, "negatives": nneg, "reps": reps,
          "path": ix.get_option("last_recommend_path"), "short": ix.get_option("last_recommend_short"),
          "wall_ms": wall, "scan_dev_ms": scan, "merge_dev_ms": merge, "wall_over_floor": wall / floor_wall,
          "scan_dev_over_floor": scan / floor_scan if floor_scan else None,
          "scan_gb_per_s": bytes_read * ix.get_option("last_recommend_path") / scan / 1e6 if scan else None})
ix.close()
