#!/usr/bin/env python3
"""Range search (wdbx_index_range_search) on the 10 M x 384 cosine corpus, one GPU: for thresholds chosen to give about
10, 1 000, 100 000 and 1 000 000 hits per query, the hit count, the device time of a lone query by HIP events (selection
scan / fp32 range scan and, on the u8 path, the exact filter), the blocking wall time of the call (download, host sort and
decoding included), and the fraction of 8 TB/s on the bytes the pass reads -- on the default u8 path and on the forced fp32
path.  Prints one JSON line.

    python tools/bench_range.py [--rows 10000000] [--dim 384] [--queries 4] [--reps 3]
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

HBM = 8e12


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--queries", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--targets", default="10,1000,100000,1000000")
    a = ap.parse_args()
    n, d = a.rows, a.dim
    ix = _native.NativeIndex(d, capacity_rows=n)
    ix.fill_synthetic(0xC0FFEE, 0, n, True)
    pitch = ix.pitch
    queries = ix.device_queries_synthetic(0xBEEF, 0, a.queries, True).download(np.float32, (a.queries, pitch))[:, :d].copy()
    # thresholds: the h-th best score from top-k where h <= 2048, else a quantile of the scores over a 200 k-row sample
    sample = ix.get_rows(0, min(n, 200_000)).astype(np.float64)
    targets = [int(x) for x in a.targets.split(",")]
    thr = np.zeros((a.queries, len(targets)), np.float32)
    for qi, q in enumerate(queries):
        s = np.sort(sample @ q.astype(np.float64))[::-1]
        for ti, h in enumerate(targets):
            if h <= _native.MAX_K:
                thr[qi, ti] = ix.search(q, h)[1][0][h - 1]
            else:
                thr[qi, ti] = s[min(len(s) - 1, int(h * len(s) / n))]
    pitch8 = next(p for p in (128, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096) if p >= d)  # (the u8 copy's row bytes)
    out = {"what": "range_search", "rows": n, "dim": d, "metric": "cosine", "queries": a.queries, "reps": a.reps,
           "targets": targets, "paths": {}}
    for path, shadow in (("u8", 2), ("fp32", 0)):
        ix.set_option("scan_shadow", shadow)
        res = []
        for ti, h in enumerate(targets):
            hits, wall, calls = [], [], 0
            ix.range_search(queries[0], [thr[0, ti]])  # warm-up (buffers grow to this size once)
            ix.profile(True)
            ix.profile_read()
            for qi, q in enumerate(queries):
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    off, rows, _ = ix.range_search(q, [thr[qi, ti]])
                    wall.append(time.perf_counter() - t0)
                    calls += 1
                hits.append(int(off[1]))
            p = ix.profile_read()
            ix.profile(False)
            scan_ms, filt_ms = p["scan_ms"] / calls, p["merge_ms"] / calls
            assert ix.get_option("last_range_path") == shadow
            bytes_read = n * (pitch8 + 4) if path == "u8" else n * pitch * 4  # (u8 rows + scales / fp32 rows)
            dev = scan_ms + filt_ms
            res.append({"target": h, "hits_mean": float(np.mean(hits)), "hits": hits,
                        "device_ms": round(dev, 4), "scan_ms": round(scan_ms, 4), "filter_ms": round(filt_ms, 4),
                        "wall_ms": round(1e3 * float(np.median(wall)), 3),
                        "scan_frac_8TBs": round(bytes_read / (scan_ms * 1e-3) / HBM, 3) if scan_ms > 0 else None})
            print(path, res[-1], file=sys.stderr, flush=True)
        out["paths"][path] = res
    ix.set_option("scan_shadow", 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
