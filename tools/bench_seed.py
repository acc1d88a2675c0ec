#!/usr/bin/env python3
"""k-means++ seeding (wdbx_index_seed_centers) on 1 M x 384 cosine, synthetic, k in {256, 1024}, default trials (2 + int(ln k)) --
  * wall ms of the call, and the device ms between HIP events of its eval launches (scan launches in the profile) and of its
    pick / apply / init launches (merge launches);
  * seed_eval_kernel's bytes per second over rows * pitch * 4 per launch, next to the fp32 scan_kernel's rate on the same handle
    in the same run (single queries with the shadow selection off: the same bytes streamed once per query);
  * with --quality: a synthetic corpus of unequal clusters (sizes spread over two orders of magnitude) through the facade,
    final inertia and empty clusters of init="random" against init="k-means++" at equal seed and max_iter.

    python tools/bench_seed.py [rows] [dim] [rounds] [--k 256,1024] [--quality ROWS] [--out FILE]

One JSON line per k on stdout, appended to FILE (default profiles/seed/results.jsonl).  Nothing is a threshold."""
import json
import math
import random
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "wdbx-py_amd"))
from wdbx_amd import _native  # noqa: E402

flags = {sys.argv[i]: sys.argv[i + 1] for i in range(1, len(sys.argv) - 1) if sys.argv[i].startswith("--")}
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in flags.values()]
rows = int(args[0]) if len(args) > 0 else 1_000_000
dim = int(args[1]) if len(args) > 1 else 384
rounds = max(1, int(args[2])) if len(args) > 2 else 3
ks = [int(v) for v in flags.get("--k", "256,1024").split(",")]
out_path = Path(flags.get("--out", ROOT / "profiles" / "seed" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def median(values):
    return float(np.median(np.asarray(values, np.float64)))


ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
ix.profile(True)
row_bytes = rows * ix.pitch * 4


def drain():
    return {**ix.profile_read(), **ix.profile_read_gemm(), **ix.profile_read_sample()}


# the yardstick: the fp32 scan kernel, one query per launch
ix.set_option("scan_shadow", 0)
ix.set_option("gemm_min_queries", 1 << 30)
queries = np.random.default_rng(1).standard_normal((8, dim)).astype(np.float32)
ix.search(queries, 10, normalize_queries=True)
drain()
yard = []
for _ in range(max(rounds, 3)):
    ix.search(queries, 10, normalize_queries=True)
    p = drain()
    yard.append(p["scan_ms"] / max(1, p["scan_launches"]))
scan_ms = median(yard)

for k in ks:
    trials = min(_native.MAX_SEED_TRIALS, 2 + int(math.log(k)))
    rng = random.Random(7)
    draws = np.array([rng.getrandbits(64) for _ in range(k * trials)], dtype=np.uint64)
    ix.seed_centers(min(k, 8), draws[: min(k, 8) * trials], trials)  # warm-up: the scratch, the code objects
    drain()
    runs = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        picked, potential = ix.seed_centers(k, draws, trials)
        wall = (time.perf_counter() - t0) * 1e3
        runs.append({**drain(), "wall_ms": wall})
    eval_ms = median([r["scan_ms"] / max(1, r["scan_launches"]) for r in runs])
    emit({"rows": rows, "dim": dim, "k": k, "n_trials": trials, "rounds": rounds, "wall_ms": median([r["wall_ms"] for r in runs]),
          "launches": ix.get_option("last_seed_launches"), "passes": ix.get_option("last_seed_passes"),
          "eval_launches": runs[-1]["scan_launches"], "eval_ms_total": median([r["scan_ms"] for r in runs]), "eval_ms_per_launch": eval_ms,
          "pick_apply_ms_total": median([r["merge_ms"] for r in runs]),
          "eval_gbps": row_bytes / (eval_ms * 1e-3) / 1e9 if eval_ms > 0 else 0.0,
          "scan_kernel_ms": scan_ms, "scan_kernel_gbps": row_bytes / (scan_ms * 1e-3) / 1e9 if scan_ms > 0 else 0.0,
          "distinct_rows": int(len(set(picked.tolist()))), "last_potential": int(potential[-1])})
ix.close()

if "--quality" in flags:
    from wdbx_amd import WDBX

    n, clusters, qdim = int(flags["--quality"]), 64, 64
    gen = np.random.default_rng(3)
    sizes = np.geomspace(1, 100, clusters)
    sizes = np.maximum(1, (sizes / sizes.sum() * n).astype(np.int64))
    centres = gen.standard_normal((clusters, qdim))
    data = np.concatenate([c + 0.15 * gen.standard_normal((s, qdim)) for c, s in zip(centres, sizes)]).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        db = WDBX(vector_dimension=qdim, num_shards=1, data_dir=tmp, enable_plugins=False)
        db.vector_store.bulk_store(data, ids=[f"v{i:07d}" for i in range(len(data))])
        for seed in (1, 2, 3):
            rec = {"quality_rows": len(data), "clusters": clusters, "k": clusters, "seed": seed, "max_iter": 25}
            for init in ("random", "k-means++"):
                t0 = time.perf_counter()
                res = db.vector_cluster(clusters, seed=seed, max_iter=25, init=init)
                rec[init] = {"inertia": res["inertia"], "empty": int(sum(1 for c in res["counts"] if c == 0)),
                             "iterations": res["iterations"], "wall_ms": (time.perf_counter() - t0) * 1e3}
            emit(rec)
