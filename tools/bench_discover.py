#!/usr/bin/env python3
"""Discovery search (rows ranked by context pairs and a target) on 10 M x 384 cosine, synthetic, k = 10: one query with a
target and P pairs, P in 1, 4, 16, 32 --
  * device ms of the scoring launch of wdbx_index_search_discover (bracketed as a scan launch), of its zone stage (zone
    launches and their ranking tails, bracketed as merge launches) and wall ms per call, in target mode and in context mode;
  * in the same run and on the same handle, ALTERNATING with it, wdbx_index_search_recommend with P + 1 positives and P
    negatives (32 + 32 for P = 32, the most a recommend query holds): the same number of exact_score_block evaluations per row by the existing kernel -- the comparator;
  * per P the ratio of the two scoring medians and the spread (max - min over the rounds) of each.

    python tools/bench_discover.py [rows] [dim] [rounds] [--out FILE]

Each round runs recommend, discover (target), discover (context) once after one warm-up call each; at least two rounds.  One
JSON line per P on stdout; --out appends them to FILE (default profiles/discover/results.jsonl).  Nothing is a threshold."""
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
rounds = max(2, int(args[2])) if len(args) > 2 else 3
out_path = Path(flags.get("--out", ROOT / "profiles" / "discover" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)
K = 10

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
rng = np.random.default_rng(1)
vectors = rng.standard_normal((65, dim)).astype(np.float32)
vectors /= np.linalg.norm(vectors, axis=1, keepdims=True)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def once(call):
    ix.profile_read()
    t0 = time.perf_counter()
    call()
    wall = (time.perf_counter() - t0) * 1e3
    p = ix.profile_read()
    return wall, p["scan_ms"], p["merge_ms"]


def stats(samples):
    a = np.asarray(samples, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()), "runs": [float(x) for x in a]}


ix.profile(True)
for P in (1, 4, 16, 32):
    target, ctx = vectors[:1], vectors[1:1 + 2 * P]
    # recommend with P + 1 positives and P negatives: 2 P + 1 evaluations per row, as target + P pairs (P = 32: 32 + 32, one
    # evaluation fewer -- a recommend query holds at most 64 examples)
    npos = min(P + 1, _native.MAX_EXAMPLES - P)
    calls = {
        "recommend": lambda: ix.search_recommend(vectors[:npos + P], [0, npos, npos + P], K),
        "target": lambda: ix.search_discover(target, ctx, [0, P], K),
        "context": lambda: ix.search_discover(None, ctx, [0, P], K),
    }
    seen = {name: [] for name in calls}
    info = {}
    for name, call in calls.items():
        call()  # (warm-up: scratch buffers grown, code loaded)
    for _ in range(rounds):
        for name, call in calls.items():
            seen[name].append(once(call))
            if name == "recommend":
                info["recommend_path"] = ix.get_option("last_recommend_path")
            elif name == "target":
                info["zone_slots"] = ix.get_option("last_discover_zone_slots")
    rec = {"case": "discover", "rows": rows, "dim": dim, "k": K, "pairs": P, "rounds": rounds, "recommend_positives": npos,
           "recommend_negatives": P, **info}
    for name, runs in seen.items():
        rec[name] = {"wall_ms": stats([r[0] for r in runs]), "scan_dev_ms": stats([r[1] for r in runs]),
                     "merge_dev_ms": stats([r[2] for r in runs])}
    base = rec["recommend"]["scan_dev_ms"]
    # (recommend's scan time covers both of its passes when the second one ran: per pass below)
    per_pass = base["median"] / max(1, info.get("recommend_path", 1))
    rec["target_scan_over_recommend_pass"] = rec["target"]["scan_dev_ms"]["median"] / per_pass if per_pass else None
    rec["context_scan_over_recommend_pass"] = rec["context"]["scan_dev_ms"]["median"] / per_pass if per_pass else None
    rec["recommend_scan_spread_ms"] = base["max"] - base["min"]
    emit(rec)
ix.close()
