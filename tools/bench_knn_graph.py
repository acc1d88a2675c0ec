#!/usr/bin/env python3
"""The k-NN graph (wdbx_index_knn_graph) on 1 M x 384 cosine, synthetic, k = 15, alternated on ONE handle with the client's
composition (blocks of 256 stored rows through get_rows + a batched search with k + 1, "itself" dropped by the caller) --
  * wall ms of each, and per kind of launch the device ms between HIP events: the sweep (gemm launches in the profile), the
    exact pass and the repair route's scoring (scan launches), the ranking tail (merge launches);
  * the share of repaired anchors and the appended list entries per anchor;
  * the sweep's bf16 matrix rate, 2 * rows * rows * pitch16 / sweep ms in TFLOP/s, next to the rate gemm_bf16w8_kernel reaches in
    the same run on the same handle (option gemm_bf16 = 2, a batch of 256 queries: 2 * rows * pitch16 * 256 over the device ms of
    its two launches, sample pass included, so that yardstick is understated by the sample pass's share).
The composition over all rows is rows / 256 calls; with --blocks B only B evenly spaced blocks run and its wall time is scaled
by (rows / 256) / B, which the record says ("composition_blocks_run").

    python tools/bench_knn_graph.py [rows] [dim] [rounds] [--k K] [--blocks B] [--out FILE]

One JSON line on stdout, appended to FILE (default profiles/knn_graph/results.jsonl).  Nothing is a threshold."""
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
rows = int(args[0]) if len(args) > 0 else 1_000_000
dim = int(args[1]) if len(args) > 1 else 384
rounds = max(1, int(args[2])) if len(args) > 2 else 3
k = int(flags.get("--k", 15))
n_blocks = -(-rows // 256)
blocks_run = min(n_blocks, int(flags.get("--blocks", n_blocks)))
out_path = Path(flags.get("--out", ROOT / "profiles" / "knn_graph" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
ix.profile(True)
pitch16 = (ix.pitch + 127) // 128 * 128


def drain():
    return {**ix.profile_read(), **ix.profile_read_gemm(), **ix.profile_read_sample()}


def median(values):
    return float(np.median(np.asarray(values, np.float64)))


def composition():
    """the client's way: 256 stored rows come down, go up again as queries with k + 1, and the row itself is dropped"""
    lines = 0
    for b in np.linspace(0, n_blocks - 1, blocks_run).astype(np.int64):
        first = int(b) * 256
        count = min(256, rows - first)
        idx, _ = ix.search(ix.get_rows(first, count), k + 1, normalize_queries=False)
        own = np.arange(first, first + count)[:, None]
        lines += int((idx != own).sum(axis=1).clip(max=k).sum())
    return lines


# the yardstick: gemm_bf16w8_kernel over the bf16 shadow copy, a batch of 256 queries
ix.set_option("gemm_bf16", 2)
queries = np.random.default_rng(1).standard_normal((256, dim)).astype(np.float32)
ix.search(queries, 10, normalize_queries=True)
drain()
yard = []
for _ in range(max(rounds, 3)):
    ix.search(queries, 10, normalize_queries=True)
    yard.append(drain()["gemm_ms"])
yard_tflops = 2.0 * rows * pitch16 * 256 / (median(yard) * 1e-3) / 1e12 if median(yard) > 0 else 0.0
ix.set_option("gemm_bf16", 3)

ix.knn_graph(k)  # warm-up: the shadow copy, the scratch, the code objects
composition() if blocks_run <= 8 else None
drain()
graph, comp = [], []
for _ in range(rounds):
    t0 = time.perf_counter()
    ix.knn_graph(k)
    wall = (time.perf_counter() - t0) * 1e3
    graph.append({**drain(), "wall_ms": wall})
    t0 = time.perf_counter()
    composition()
    comp.append((time.perf_counter() - t0) * 1e3 * n_blocks / blocks_run)
    drain()
sweep_ms = median([r["gemm_ms"] for r in graph])
tflops = 2.0 * rows * rows * pitch16 / (sweep_ms * 1e-3) / 1e12 if sweep_ms > 0 else 0.0
rec = {"rows": rows, "dim": dim, "k": k, "rounds": rounds, "path": ix.get_option("last_knn_path"),
       "passes": ix.get_option("last_knn_passes"), "launches": ix.get_option("last_knn_launches"),
       "wall_ms": median([r["wall_ms"] for r in graph]), "sweep_ms": sweep_ms,
       "sweep_ms_per_launch": sweep_ms / max(1, ix.get_option("last_knn_passes")),
       "exact_ms": median([r["scan_ms"] for r in graph]), "rank_ms": median([r["merge_ms"] for r in graph]),
       "repaired_share": ix.get_option("last_knn_repaired") / rows, "appends_per_anchor": ix.get_option("last_knn_appends") / rows,
       "sweep_bf16_tflops": tflops, "gemm_bf16w8_tflops": yard_tflops, "gemm_bf16w8_ms": median(yard),
       "composition_wall_ms": median(comp), "composition_blocks_run": blocks_run, "composition_blocks": n_blocks}
line = json.dumps(rec)
print(line, flush=True)
with open(out_path, "a") as f:
    f.write(line + "\n")
ix.close()
