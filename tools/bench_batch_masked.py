#!/usr/bin/env python3
"""Filtered batch search: 10 M x 384 cosine, top-10, 256 queries per call with ONE row mask, through the device-resident
entry point (wdbx_index_search_batch_masked_device).  Masks: allowed fraction 1.0 / 0.5 / 0.1 / 0.01, random rows and runs
of whole 256-row tiles.  Per case: ms per batch, candidates per query, last_batch_repaired, the tile kernels' time
(wdbx_index_profile_read_gemm: sample pass + full pass), and -- in the same process -- the unmasked batch for comparison.

    python tools/bench_batch_masked.py [rows] [dim] [nq] [k] [reps] [--per-query Q] [--out FILE]

--per-query Q: also time Q of the queries one call each with the same mask (the masked per-query selection scan: what a
masked batch cost before this path existed, and what option gemm_masked=0 still runs); the 256-query figure is that time
x nq / Q, an EXTRAPOLATION, and is labelled so.  A library without the masked entry point (an older commit) runs only this
leg.  One JSON line per case on stdout; --out appends them to FILE (default profiles/batch_masked/results.jsonl)."""
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
nq = int(args[2]) if len(args) > 2 else 256
k = int(args[3]) if len(args) > 3 else 10
reps = int(args[4]) if len(args) > 4 else 5
per_query = int(flags.get("--per-query", 0))
out_path = Path(flags.get("--out", ROOT / "profiles" / "batch_masked" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
has_masked = hasattr(ix, "search_batch_masked_device")
dq = ix.device_queries_synthetic(0xBEEF, 0, nq, True)
d_idx, d_score = ix.alloc(nq * k * 8), ix.alloc(nq * k * 4)
rng = np.random.default_rng(1)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def timed(call):
    call()  # warm: shadow copies, buffers
    ix.synchronize()
    ix.profile(True)
    ix.profile_read_gemm()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    ix.synchronize()
    el = (time.perf_counter() - t0) / reps
    g = ix.profile_read_gemm()
    ix.profile(False)
    return el * 1e3, g["gemm_ms"] / reps, g["gemm_launches"] / reps


base = {"rows": rows, "dim": dim, "nq": nq, "k": k, "reps": reps}
ms, gemm_ms, launches = timed(lambda: ix.search_batch_device(dq, nq, k, d_idx, d_score))
st = ix.batch_status(nq)
emit(dict(base, case="unmasked", ms_per_batch=ms, tile_kernels_ms=gemm_ms, tile_launches=launches,
          candidates_per_query=float(st["counts"].mean()), repaired=ix.get_option("last_batch_repaired")))
unmasked_ms = ms

queries = None
if per_query:
    queries = np.ascontiguousarray(dq.download(np.float32, (nq, ix.pitch))[:per_query, :dim])

tiles = (rows + 255) // 256
for frac in (1.0, 0.5, 0.1, 0.01):
    for kind in ("random", "tile_runs"):
        if kind == "random":
            allowed = rng.random(rows) < frac if frac < 1.0 else np.ones(rows, bool)
        else:
            run = 8  # tiles per run
            on = rng.random((tiles + run - 1) // run) < frac if frac < 1.0 else np.ones((tiles + run - 1) // run, bool)
            allowed = np.repeat(on, run * 256)[:rows]
        words = _native.pack_row_mask(allowed)
        rec = dict(base, case=f"{kind} f={frac}", allowed_rows=int(np.count_nonzero(allowed)))
        if has_masked:
            ms, gemm_ms, launches = timed(lambda: ix.search_batch_masked_device(dq, nq, k, words, d_idx, d_score))
            st = ix.batch_status(nq)
            rec.update(ms_per_batch=ms, tile_kernels_ms=gemm_ms, tile_launches=launches,
                       candidates_per_query=float(st["counts"].mean()), overflowed=st["overflowed"],
                       repaired=ix.get_option("last_batch_repaired"), masked_pass=ix.get_option("last_batch_masked"),
                       vs_unmasked_same_process=ms / unmasked_ms)
        if per_query:
            ix.search(queries[:1], k, mask_words=words)
            t0 = time.perf_counter()
            for q in queries:
                ix.search(q[None, :], k, mask_words=words)
            el = (time.perf_counter() - t0) * 1e3
            rec.update(per_query_calls=per_query, per_query_ms_each=el / per_query,
                       per_query_ms_extrapolated_to_nq=el / per_query * nq)
        emit(rec)
ix.close()
