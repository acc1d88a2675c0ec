#!/usr/bin/env python3
"""The similarity self-join (wdbx_index_self_join) on 1 M x 384 cosine, synthetic rows with about 1 % of them planted as noisy
duplicates of other rows, threshold 0.95, alternated on ONE handle with the client's composition (blocks of 256 stored rows
through get_rows + wdbx_index_range_search_batch, rows <= anchor dropped by the caller) --
  * wall ms of each, and the device ms between HIP events of the sweep (gemm launches in the profile) and of the exact pass
    (merge launches);
  * candidate pairs per result pair;
  * the sweep's integer rate, 2 * tile visits * 256 * block rows * pitch8 / sweep ms in POP/s, next to the rate gemm_i8_kernel
    reaches in the same run on the same handle (a batch of 256 queries: 2 * rows * pitch8 * 256 over the device ms of its
    launches, sample pass included, so that yardstick is understated by the sample pass's share).
The composition over all rows is rows / 256 calls; with --blocks B only B evenly spaced blocks run and its wall time is scaled
by (rows / 256) / B, which the record says ("composition_blocks_run").

    python tools/bench_self_join.py [rows] [dim] [rounds] [--threshold T] [--blocks B] [--out FILE]

One JSON line on stdout, appended to FILE (default profiles/self_join/results.jsonl).  Nothing is a threshold."""
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
thr = np.float32(flags.get("--threshold", 0.95))
n_blocks = -(-rows // 256)
blocks_run = min(n_blocks, int(flags.get("--blocks", n_blocks)))
out_path = Path(flags.get("--out", ROOT / "profiles" / "self_join" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
# about 1 % of the rows become noisy duplicates (cosine about 0.97) of rows in the first half
planted = max(1, rows // 100)
rng = np.random.default_rng(3)
for first in range(0, planted, 8192):
    count = min(8192, planted - first)
    twin = ix.get_rows(first, count) + (0.25 / np.sqrt(dim)) * rng.standard_normal((count, dim)).astype(np.float32)
    ix.set_rows(rows // 2 + first, (twin / np.linalg.norm(twin, axis=1, keepdims=True)).astype(np.float32))
ix.profile(True)
pitch8 = (dim + 127) // 128 * 128
block_rows = 128 if pitch8 <= 768 else 64  # (host_join.h: join_ct8)


def drain():
    return {**ix.profile_read(), **ix.profile_read_gemm(), **ix.profile_read_sample()}


def median(values):
    return float(np.median(np.asarray(values, np.float64)))


def composition():
    """the client's way: 256 stored rows come down, go up again as range queries, and the rows <= anchor are dropped"""
    pairs = 0
    for b in np.linspace(0, n_blocks - 1, blocks_run).astype(np.int64):
        first = int(b) * 256
        count = min(256, rows - first)
        off, hit, _ = ix.range_search_batch(ix.get_rows(first, count), thr, normalize_queries=False)
        anchors = np.repeat(np.arange(first, first + count), np.diff(off))
        pairs += int((hit > anchors).sum())
    return pairs


# the yardstick: gemm_i8_kernel over the same shadow copy, a batch of 256 queries
queries = np.random.default_rng(1).standard_normal((256, dim)).astype(np.float32)
ix.search(queries, 10, normalize_queries=True)
drain()
yard = []
for _ in range(max(rounds, 3)):
    ix.search(queries, 10, normalize_queries=True)
    yard.append(drain()["gemm_ms"])
yard_pops = 2.0 * rows * pitch8 * 256 / (median(yard) * 1e-3) / 1e15 if median(yard) > 0 else 0.0

offsets, _, _ = ix.self_join(thr)  # warm-up: the shadow copy, the buffers, the code objects
composition() if blocks_run <= 8 else None
drain()
join, comp = [], []
for _ in range(rounds):
    t0 = time.perf_counter()
    ix.self_join(thr)
    wall = (time.perf_counter() - t0) * 1e3
    join.append({**drain(), "wall_ms": wall})
    t0 = time.perf_counter()
    composition()
    comp.append((time.perf_counter() - t0) * 1e3 * n_blocks / blocks_run)
    drain()
blocks = ix.get_option("last_join_blocks")
tiles = -(-rows // 256)
visits = sum(tiles - i * block_rows // 256 for i in range(blocks))
sweep_ms = median([r["gemm_ms"] for r in join])
pops = 2.0 * visits * 256 * block_rows * pitch8 / (sweep_ms * 1e-3) / 1e15 if sweep_ms > 0 else 0.0
pairs, cands = ix.get_option("last_join_pairs"), ix.get_option("last_join_candidates")
rec = {"rows": rows, "dim": dim, "threshold": float(thr), "rounds": rounds, "planted": planted,
       "path": ix.get_option("last_join_path"), "blocks": blocks, "launches": ix.get_option("last_join_launches"),
       "reruns": ix.get_option("last_join_reruns"), "pairs": pairs, "candidates": cands,
       "candidates_per_pair": cands / max(1, pairs),
       "wall_ms": median([r["wall_ms"] for r in join]), "wall_ms_all": [r["wall_ms"] for r in join], "sweep_ms": sweep_ms,
       "exact_ms": median([r["merge_ms"] for r in join]), "sweep_i8_pops": pops, "gemm_i8_pops": yard_pops,
       "gemm_i8_ms": median(yard), "composition_wall_ms": median(comp), "composition_wall_ms_all": comp,
       "composition_blocks_run": blocks_run, "composition_blocks": n_blocks}
line = json.dumps(rec)
print(line, flush=True)
with open(out_path, "a") as f:
    f.write(line + "\n")
ix.close()
