#!/usr/bin/env python3
"""Nearest-centre assignment (wdbx_index_assign) on 10 M x 384 cosine, synthetic, K in {16, 256, 1024, 4096} --
  * per pass the device ms between HIP events: preparation (a sample launch in the profile), the tile pass (a gemm launch),
    the exact launches (scan launches: the winners' scores and the ambiguous rows), the sums pass and its combination (merge
    launches); wall ms of the whole call with every output asked for;
  * the ambiguous share (rows the tile pass could not vouch for);
  * the tile pass's fp32 matrix rate: 2 * rows * pitch * centre slots / tile ms, in TFLOP/s, next to the 157.3 TFLOP/s datasheet
    peak and to the rate the EXISTING fp32 tile kernel reaches in the same run on the same handle (option gemm_bf16 = 0, a batch
    of 256 queries: config 4) -- 2 * rows * pitch * 256 over the device ms of its two launches, sample pass included, so the
    yardstick is understated by the sample pass's share.  The existing kernel is the yardstick, not the new one.

    python tools/bench_assign.py [rows] [dim] [rounds] [--out FILE] [--route 0|1|both] [--metric 0|1]

--route sets option assign_i8 for every call (0 = the fp32 tiles, 1 = the int8 candidate sweep; both = the two alternating per K
in this one process; without it the library's choice).  A line's "route" is what ran (last_assign_path: 1 fp32 tiles, 2 int8
sweep); on the int8 route tile_ms is the sweep (every sweep of the call), sums_ms also holds the exact pass over the candidates
(merge launches), "pairs_per_row" the candidates scored per row and tile_tflops counts integer operations.

One JSON line per K on stdout, appended to FILE (default profiles/assign/results.jsonl).  Nothing is a threshold."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "wdbx-py_amd"))
from wdbx_amd import _native  # noqa: E402

flags = {sys.argv[i]: sys.argv[i + 1] for i in range(1, len(sys.argv) - 1) if sys.argv[i].startswith("--")}
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in flags.values()]
rows = int(args[0]) if len(args) > 0 else 10_000_000
dim = int(args[1]) if len(args) > 1 else 384
rounds = max(2, int(args[2])) if len(args) > 2 else 3
out_path = Path(flags.get("--out", ROOT / "profiles" / "assign" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)
PEAK = 157.3

routes = {"0": (0,), "1": (1,), "both": (0, 1)}.get(flags.get("--route"), (None,))

ix = _native.NativeIndex(dim, metric=int(flags.get("--metric", 0)), capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
ix.profile(True)
rng = np.random.default_rng(1)


def drain():
    return {**ix.profile_read(), **ix.profile_read_gemm(), **ix.profile_read_sample()}


def median(values):
    return float(np.median(np.asarray(values, np.float64)))


# the yardstick: the existing fp32 tile kernel, a batch of 256 queries
ix.set_option("gemm_bf16", 0)
queries = rng.standard_normal((256, dim)).astype(np.float32)
ix.search(queries, 10, normalize_queries=True)
drain()
yard = []
for _ in range(rounds):
    ix.search(queries, 10, normalize_queries=True)
    yard.append(drain()["gemm_ms"])
ix.set_option("gemm_bf16", 3)  # (the default again: the int8 route exists only where the batched path's i8 image does)
yard_tflops = 2.0 * rows * ix.pitch * 256 / (median(yard) * 1e-3) / 1e12 if median(yard) > 0 else 0.0

for k, route in ((k, r) for k in (16, 256, 1024, 4096) for r in routes):
    centers = np.random.default_rng(k).standard_normal((k, dim)).astype(np.float32)
    want = ("center", "score", "sums", "counts")
    if route is not None:
        ix.set_option("assign_i8", route)
    try:
        ix.assign(centers, normalize=True, want=want)
    except _native.HipBackendError as e:  # (an int8 sweep whose candidates would pass the buffer limit: recorded, not timed)
        line = json.dumps({"rows": rows, "dim": dim, "centers": k, "assign_i8": route, "error": str(e)})
        print(line, flush=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")
        continue
    drain()
    runs = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        ix.assign(centers, normalize=True, want=want)
        wall = (time.perf_counter() - t0) * 1e3
        runs.append({**drain(), "wall_ms": wall})
    blocks = ix.get_option("last_assign_center_blocks")
    path = ix.get_option("last_assign_path")
    slots = blocks * ((128 if ix.dim <= 512 else 64) if path == 2 else 32 if k <= 32 else 64 if k <= 64 else 128)
    tile_ms = median([r["gemm_ms"] for r in runs])
    tflops = 2.0 * rows * (-(-dim // 128) * 128 if path == 2 else ix.pitch) * slots / (tile_ms * 1e-3) / 1e12 if tile_ms > 0 else 0.0
    rec = {"rows": rows, "dim": dim, "centers": k, "rounds": rounds, "center_blocks": blocks, "route": path, "why": ix.get_option("last_assign_why"),
           "pairs_per_row": ix.get_option("last_assign_pairs") / rows, "sweeps": ix.get_option("last_assign_sweeps"),
           "prep_ms": median([r["sample_ms"] for r in runs]), "tile_ms": tile_ms,
           "exact_ms": median([r["scan_ms"] for r in runs]), "sums_ms": median([r["merge_ms"] for r in runs]),
           "wall_ms": median([r["wall_ms"] for r in runs]), "launches": ix.get_option("last_assign_launches"),
           "ambiguous_share": ix.get_option("last_assign_ambiguous") / rows, "partials": ix.get_option("last_assign_partials"),
           "tile_tflops": tflops, "tile_share_of_peak": tflops / PEAK,
           "existing_fp32_tile_tflops": yard_tflops, "existing_fp32_tile_ms": median(yard)}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")
ix.close()
