#!/usr/bin/env python3
"""Batched range search (wdbx_index_range_search_batch) against wdbx_index_range_search with the same queries, on the
10 M x 384 cosine corpus, one GPU: batches of 4 / 16 / 64 / 256 queries, thresholds giving about 10 and about 1000 hits per
query.  Per (batch size, target) the two entry points run ALTERNATELY on the same handle, `reps` times each; reported are the
medians of the blocking wall time of the call and of the device time by HIP events (per-query path: selection scans + exact
filters; batched: tile passes + exact filters -- the quantiser, the bound kernel and the scatter are not bracketed, the wall
time holds them), the path the batched call took and the pairs its tile passes kept.  The crossover is the smallest batch
size from which the batched call's wall time is below the per-query call's for every target.  One JSON line per case, then a
summary line.

    python tools/bench_range_batch.py [--rows 10000000] [--dim 384] [--reps 5] [--batches 4,16,64,256] [--targets 10,1000]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "wdbx-py_amd"))
from wdbx_amd import _native  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="4,16,64,256")
    ap.add_argument("--targets", default="10,1000")
    a = ap.parse_args()
    n, d = a.rows, a.dim
    batches = [int(x) for x in a.batches.split(",")]
    targets = [int(x) for x in a.targets.split(",")]
    ix = _native.NativeIndex(d, capacity_rows=n)
    ix.fill_synthetic(0xC0FFEE, 0, n, True)
    nq_max = max(batches)
    queries = ix.device_queries_synthetic(0xBEEF, 0, nq_max, True).download(np.float32, (nq_max, ix.pitch))[:, :d].copy()
    top = ix.search(queries, max(targets))[1]  # thresholds: the h-th best score of each query
    ix.set_option("range_batch_min_queries", 1)  # (the route under test, whatever the default says)
    cases = []

    def timed(call, gemm):
        ix.profile(True)
        ix.profile_read()
        ix.profile_read_gemm()
        t0 = time.perf_counter()
        off = call()[0]
        wall = time.perf_counter() - t0
        p = ix.profile_read()
        dev = p["scan_ms"] + p["merge_ms"] + (ix.profile_read_gemm()["gemm_ms"] if gemm else 0.0)
        ix.profile(False)
        return 1e3 * wall, dev, off

    for h in targets:
        for nq in batches:
            q, t = queries[:nq], np.ascontiguousarray(top[:nq, h - 1])
            ref = ix.range_search(q, t)  # warm-up of both (buffers grow once), and the answers agree
            got = ix.range_search_batch(q, t)
            same = all(np.array_equal(x, y) for x, y in zip(ref[:2], got[:2])) and np.array_equal(ref[2].view(np.uint32), got[2].view(np.uint32))
            one, bat = [], []
            for _ in range(a.reps):
                one.append(timed(lambda: ix.range_search(q, t), False)[:2])
                bat.append(timed(lambda: ix.range_search_batch(q, t), True)[:2])
            med = lambda xs, i: float(np.median([x[i] for x in xs]))
            case = {"what": "range_batch", "rows": n, "dim": d, "nq": nq, "target": h, "hits_mean": float(np.mean(np.diff(ref[0]))),
                    "identical": bool(same), "reps": a.reps,
                    "per_query_wall_ms": round(med(one, 0), 3), "per_query_device_ms": round(med(one, 1), 3),
                    "batch_wall_ms": round(med(bat, 0), 3), "batch_device_ms": round(med(bat, 1), 3),
                    "batch_path": ix.get_option("last_range_batch_path"), "batch_blocks": ix.get_option("last_range_batch_blocks"),
                    "batch_pairs": ix.get_option("last_range_batch_pairs"),
                    "fallback_queries": ix.get_option("last_range_batch_fallback_queries")}
            cases.append(case)
            print(json.dumps(case), flush=True)
    wins = [nq for nq in batches if all(c["batch_wall_ms"] < c["per_query_wall_ms"] for c in cases if c["nq"] >= nq)]
    print(json.dumps({"what": "range_batch_summary", "crossover_nq": min(wins) if wins else None,
                      "all_identical": all(c["identical"] for c in cases)}))
    ix.close()


if __name__ == "__main__":
    main()
