#!/usr/bin/env python3
"""Device PCA (wdbx_index_moments / wdbx_index_project) on 10 M x 384 cosine, synthetic; the legs alternate inside every
round of one run --
  * moments: device ms between HIP events of the scatter pass (a gemm launch) and of the column sums, the mean and the float64
    combination (merge launches); wall ms of the whole call;
  * the scatter pass's fp32 matrix rate: rows * 32 * 32 * tiles of the upper triangle * 2 / scatter ms, in TFLOP/s, next to the
    157.3 TFLOP/s datasheet peak and, from the same round, to assign_tile_kernel (wdbx_index_assign, 1024 centres: its gemm
    launch) and to the existing fp32 tile kernel gemm_topk_kernel (option gemm_bf16 = 0, a batch of 256 queries: both its
    launches, the sample pass included, so that yardstick is understated by the sample pass's share);
  * project on 2 and on 32 directions: device ms of its gemm launch, bytes of the stored rows per second, next to
    wdbx_index_probe_read's (the plain read of the same rows) from the same round;
  * the client's composition on CLIENT_ROWS rows (default 1 000 000: the whole corpus would be 15 GB of host rows and twice
    that in float64): get_rows + numpy.cov + a numpy projection, wall ms, next to the device calls' wall ms on the same
    number of rows in a handle of its own.

    python tools/bench_pca.py [rows] [dim] [rounds] [--out FILE] [--client-rows N]

One JSON line on stdout, appended to FILE (default profiles/pca/results.jsonl).  Nothing is a threshold."""
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
rounds = max(2, int(args[2])) if len(args) > 2 else 5
client_rows = int(flags.get("--client-rows", min(rows, 1_000_000)))
out_path = Path(flags.get("--out", ROOT / "profiles" / "pca" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)
PEAK = 157.3

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
ix.profile(True)
ix.set_option("gemm_bf16", 0)
rng = np.random.default_rng(1)
queries = rng.standard_normal((256, dim)).astype(np.float32)
centers = rng.standard_normal((1024, dim)).astype(np.float32)
basis = np.linalg.qr(rng.standard_normal((dim, 32)))[0].T.astype(np.float32)


def drain():
    return {**ix.profile_read(), **ix.profile_read_gemm(), **ix.profile_read_sample()}


def median(values):
    return float(np.median(np.asarray(values, np.float64)))


def timed(call):
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    return out, {**drain(), "wall_ms": wall}


legs = {"moments": lambda: ix.moments(center=True), "project2": lambda: ix.project(basis[:2], offset=mean),
        "project32": lambda: ix.project(basis, offset=mean), "assign": lambda: ix.assign(centers, normalize=True, want=("center",)),
        "gemm": lambda: ix.search(queries, 10, normalize_queries=True)}
mean = ix.moments(want=("mean",))["mean"]
for call in legs.values():  # warm-up: allocations, code objects
    call()
drain()
runs = {name: [] for name in legs}
probe = []
for _ in range(rounds):
    for name, call in legs.items():
        runs[name].append(timed(call)[1])
    probe.append(ix.probe_read_ms())
    drain()

nb = -(-dim // 32)
tiles = nb * (nb + 1) // 2
scatter_ms = median([r["gemm_ms"] for r in runs["moments"]])
flop = lambda ms, work: 2.0 * work / (ms * 1e-3) / 1e12 if ms > 0 else 0.0  # noqa: E731
row_bytes = rows * ix.pitch * 4
rate = lambda ms: row_bytes / (ms * 1e-3) / 1e12 if ms > 0 else 0.0  # noqa: E731
assign_ms, gemm_ms = median([r["gemm_ms"] for r in runs["assign"]]), median([r["gemm_ms"] for r in runs["gemm"]])
rec = {"rows": rows, "dim": dim, "rounds": rounds,
       "partials": ix.get_option("last_moments_partials"), "tile_groups": ix.get_option("last_moments_tile_groups"),
       "scatter_ms": scatter_ms, "sums_mean_combine_ms": median([r["merge_ms"] for r in runs["moments"]]),
       "moments_wall_ms": median([r["wall_ms"] for r in runs["moments"]]),
       "scatter_tflops": flop(scatter_ms, rows * 1024.0 * tiles), "scatter_share_of_peak": flop(scatter_ms, rows * 1024.0 * tiles) / PEAK,
       "assign_tile_ms": assign_ms, "assign_tile_tflops": flop(assign_ms, rows * float(ix.pitch) * 1024),
       "existing_fp32_tile_ms": gemm_ms, "existing_fp32_tile_tflops": flop(gemm_ms, rows * float(ix.pitch) * 256),
       "probe_read_ms": median(probe), "probe_read_tb_s": rate(median(probe))}
for name in ("project2", "project32"):
    ms = median([r["gemm_ms"] for r in runs[name]])
    rec.update({f"{name}_ms": ms, f"{name}_tb_s": rate(ms), f"{name}_wall_ms": median([r["wall_ms"] for r in runs[name]])})
ix.close()

# the client's composition against the two device calls, on a handle of client_rows rows
small = _native.NativeIndex(dim, capacity_rows=client_rows)
small.fill_synthetic(0xC0FFEE, 0, client_rows, True)
small.moments(), small.project(basis[:2])
t0 = time.perf_counter()
got = small.moments(center=True)
values, vectors = np.linalg.eigh(got["scatter"] / (got["count"] - 1))
top = vectors[:, np.argsort(values)[::-1][:2]].T.astype(np.float32)
small.project(top, offset=got["mean"])
device_wall = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
x = small.get_rows(0, client_rows)
cov = np.cov(x, rowvar=False)
values, vectors = np.linalg.eigh(cov)
(x - x.mean(axis=0)) @ vectors[:, np.argsort(values)[::-1][:2]]
client_wall = (time.perf_counter() - t0) * 1e3
small.close()
rec.update({"client_rows": client_rows, "device_fit_and_project_wall_ms": device_wall, "client_composition_wall_ms": client_wall})
line = json.dumps(rec)
print(line, flush=True)
with open(out_path, "a") as f:
    f.write(line + "\n")
