#!/usr/bin/env python3
"""Search among listed rows against the masked search for the same allowed set: 10 M x 384 cosine, top-10, random sorted
lists of 10^3 .. 10^6 rows, a lone query and a batch of 256, both calls alternating in one process (the masked path is the
baseline: nothing of it changed).  Per list size and query count: wall time per call, device time from the handle's profile
events (search_rows: its scoring launches = scan launches, plus merge launches; masked: tile kernels / selection scan + merge),
the listed rows' bytes over the scoring launches' device time as a share of 8 TB/s, and the host's share of a search_rows
call (what a call costs with the device time taken out: validation, narrowing, list upload, launches, synchronisation).

    python tools/bench_subset.py [rows] [dim] [k] [reps] [--out FILE]

One JSON line per case on stdout; --out appends them to FILE (default profiles/subset/results.jsonl)."""
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
out_path = Path(flags.get("--out", ROOT / "profiles" / "subset" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)
HBM = 8e12

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
rng = np.random.default_rng(1)
queries = rng.standard_normal((256, dim)).astype(np.float32)
queries /= np.linalg.norm(queries, axis=1, keepdims=True)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def drain():
    p = ix.profile_read()
    g = ix.profile_read_gemm()
    s = ix.profile_read_sample()
    return p, g, s


def median(v):
    return float(np.median(v))


ix.profile(True)
for n_ids in (1000, 10_000, 100_000, 1_000_000):
    if n_ids > rows:
        continue
    ids = np.sort(rng.choice(rows, n_ids, replace=False)).astype(np.uint64)
    allowed = np.zeros(rows, bool)
    allowed[ids] = True
    t0 = time.perf_counter()
    words = _native.pack_row_mask(allowed)
    pack_ms = (time.perf_counter() - t0) * 1e3
    for nq in (1, 256):
        q = queries[:nq]
        # warm both (shadow copies, buffers), and check they agree
        a = ix.search_rows(q, k, ids)
        b = ix.search(q, k, mask_words=words)
        same = bool(np.array_equal(a[0], b[0]))
        drain()
        wall = {"rows": [], "masked": []}
        dev = {"rows_scan": [], "rows_merge": [], "masked": []}
        for _ in range(reps):  # alternating
            t0 = time.perf_counter()
            ix.search_rows(q, k, ids)
            wall["rows"].append((time.perf_counter() - t0) * 1e3)
            p, g, s = drain()
            dev["rows_scan"].append(p["scan_ms"])
            dev["rows_merge"].append(p["merge_ms"])
            t0 = time.perf_counter()
            ix.search(q, k, mask_words=words)
            wall["masked"].append((time.perf_counter() - t0) * 1e3)
            p, g, s = drain()
            dev["masked"].append(p["scan_ms"] + p["merge_ms"] + g["gemm_ms"] + s["sample_ms"])
        scan_ms = median(dev["rows_scan"])
        rec = {
            "rows": rows, "dim": dim, "k": k, "n_ids": n_ids, "nq": nq, "reps": reps, "ids_equal_masked": same,
            "rows_path": ix.get_option("last_rows_path"),
            "rows_wall_ms": median(wall["rows"]), "masked_wall_ms": median(wall["masked"]),
            "rows_dev_scan_ms": scan_ms, "rows_dev_merge_ms": median(dev["rows_merge"]),
            "masked_dev_ms": median(dev["masked"]),
            "rows_host_ms": median(wall["rows"]) - scan_ms - median(dev["rows_merge"]),
            "rows_bytes_per_pass": n_ids * dim * 4,
            "rows_share_of_8TBs": (n_ids * dim * 4 / (scan_ms * 1e-3) / HBM) if scan_ms > 0 else None,
            "mask_pack_ms": pack_ms,
        }
        emit(rec)
ix.close()
