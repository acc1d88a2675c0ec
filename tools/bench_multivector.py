#!/usr/bin/env python3
"""Multi-vector search (late interaction: labels ranked by the sum of per-vector best scores) on 10 M x 384 cosine, synthetic,
10 consecutive rows per label: one query of 8 vectors and one of 32, each timed as a call of its own --
  * wall ms per query;
  * device time of its scoring launches (the handle's profile events: scoring = scan launches) and of its reduce-and-rank +
    merge launches (= merge launches), and the latter's share of the two;
  * the rounds the call took, and the scoring time per block of 8 vectors (the yardstick: the distinct search's full pass on
    the same corpus, profiles/distinct/).

    python tools/bench_multivector.py [rows] [dim] [k] [reps] [--out FILE]

One JSON line per case on stdout; --out appends them to FILE (default profiles/multivector/results.jsonl)."""
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
reps = int(args[3]) if len(args) > 3 else 5
out_path = Path(flags.get("--out", ROOT / "profiles" / "multivector" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
rng = np.random.default_rng(1)
vectors = rng.standard_normal((32, dim)).astype(np.float32)
vectors /= np.linalg.norm(vectors, axis=1, keepdims=True)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def median(v):
    return float(np.median(v))


ix.set_labels(0, (np.arange(rows, dtype=np.uint64) // 10).astype(np.uint32))
ix.profile(True)
t0 = time.perf_counter()
ix.search_multivector(vectors[:1], [0, 1], k)  # (builds and uploads the label order)
first_ms = (time.perf_counter() - t0) * 1e3
for nv in (8, 32):
    ix.search_multivector(vectors[:nv], [0, nv], k)
    ix.profile_read()
    wall, dev_scan, dev_rank = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ix.search_multivector(vectors[:nv], [0, nv], k)
        wall.append((time.perf_counter() - t0) * 1e3)
        p = ix.profile_read()
        dev_scan.append(p["scan_ms"])
        dev_rank.append(p["merge_ms"])
    s_ms, r_ms = median(dev_scan), median(dev_rank)
    emit({"case": "one_query", "vectors": nv, "rows": rows, "dim": dim, "k": k, "reps": reps,
          "rounds": ix.get_option("last_multivector_rounds"), "labels": ix.get_option("last_multivector_labels"),
          "wall_ms_per_query": median(wall), "scoring_dev_ms": s_ms, "reduce_rank_merge_dev_ms": r_ms,
          "reduce_rank_merge_share": r_ms / (s_ms + r_ms) if s_ms + r_ms > 0 else None,
          "scoring_dev_ms_per_block_of_8": s_ms / (nv / 8),
          "first_call_with_label_order_build_ms": first_ms,
          "device_bytes_resident": ix.get_option("device_bytes_resident")})
ix.close()
