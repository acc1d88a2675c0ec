#!/usr/bin/env python3
"""MMR search (a diversified top-k picked greedily from the pool of the fetch_k best rows) on 10 M x 384 cosine, synthetic:
lone queries and batches of 32 at (k, fetch_k) = (10, 40), (10, 200), (100, 2048) --
  * wall ms of wdbx_index_search_mmr against wdbx_index_search with k = fetch_k on the same handle (the pool alone: the
    difference is what the diversification costs);
  * device time from the handle's profile events: the gather and the pairs kernel are bracketed as scan launches, the selection
    kernel as a merge launch, so (the call's scan ms - the pool call's scan ms) is gather + pairs and (merge ms - merge ms) is
    the selection;
  * once per shape, for scale, what a caller does today: the pool through search(), its rows fetched to the host one
    get_rows call per candidate, the similarity square and the same greedy loop in numpy float32.

    python tools/bench_mmr.py [rows] [dim] [reps] [--out FILE]

One JSON line per case on stdout; --out appends them to FILE (default profiles/mmr/results.jsonl).  Nothing is a threshold."""
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
out_path = Path(flags.get("--out", ROOT / "profiles" / "mmr" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)
LAMBDA = 0.5

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
rng = np.random.default_rng(1)
queries = rng.standard_normal((32, dim)).astype(np.float32)
queries /= np.linalg.norm(queries, axis=1, keepdims=True)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def median(v):
    return float(np.median(v))


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
    return median(wall), median(scan), median(merge)


def host_loop(q, k, fetch_k):
    """what a caller does without the call: pool, rows to the host, square and greedy in numpy float32"""
    t0 = time.perf_counter()
    idx, score = ix.search(q[None, :], fetch_k)
    cand = idx[0][idx[0] >= 0]
    rel = score[0][: len(cand)]
    t1 = time.perf_counter()
    c = np.concatenate([ix.get_rows(int(r), 1) for r in cand]).astype(np.float32)
    t2 = time.perf_counter()
    G = (c @ c.T).astype(np.float32)
    lam, one_minus = np.float32(LAMBDA), np.float32(1.0) - np.float32(LAMBDA)
    lrel = lam * rel
    maxsim = np.full(len(cand), -np.inf, np.float32)
    picked = np.zeros(len(cand), bool)
    picked[0] = True
    pos = [0]
    while len(pos) < min(k, len(cand)):
        maxsim = np.maximum(maxsim, G[pos[-1]])
        v = np.where(picked, -np.inf, lrel - one_minus * maxsim)
        best = int(np.argmax(v))
        picked[best] = True
        pos.append(best)
    t3 = time.perf_counter()
    return {"pool_ms": (t1 - t0) * 1e3, "fetch_rows_ms": (t2 - t1) * 1e3, "square_and_greedy_ms": (t3 - t2) * 1e3,
            "total_ms": (t3 - t0) * 1e3, "bytes_fetched": int(c.nbytes)}


ix.profile(True)
for k, fetch_k in ((10, 40), (10, 200), (100, 2048)):
    for nq in (1, 32):
        q = queries[:nq]
        try:
            pool_wall, pool_scan, pool_merge = timed(lambda: ix.search(q, fetch_k))
            mmr_wall, mmr_scan, mmr_merge = timed(lambda: ix.search_mmr(q, k, fetch_k, LAMBDA))
        except _native.HipBackendError as e:  # (recorded, not hidden: the pool is the plain search and fails where it fails)
            emit({"case": "mmr", "rows": rows, "dim": dim, "k": k, "fetch_k": fetch_k, "nq": nq, "error": str(e)})
            continue
        emit({"case": "mmr", "rows": rows, "dim": dim, "k": k, "fetch_k": fetch_k, "nq": nq, "lambda": LAMBDA, "reps": reps,
              "rounds": ix.get_option("last_mmr_rounds"), "candidates": ix.get_option("last_mmr_candidates"),
              "pool_wall_ms": pool_wall, "mmr_wall_ms": mmr_wall, "diversification_wall_ms": mmr_wall - pool_wall,
              "pool_scan_dev_ms": pool_scan, "mmr_scan_dev_ms": mmr_scan, "gather_and_pairs_dev_ms": mmr_scan - pool_scan,
              "pool_merge_dev_ms": pool_merge, "mmr_merge_dev_ms": mmr_merge, "select_dev_ms": mmr_merge - pool_merge,
              "device_bytes_resident": ix.get_option("device_bytes_resident")})
    emit({"case": "host_loop_one_query", "rows": rows, "dim": dim, "k": k, "fetch_k": fetch_k, **host_loop(queries[0], k, fetch_k)})
ix.close()
