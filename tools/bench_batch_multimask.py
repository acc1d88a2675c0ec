#!/usr/bin/env python3
"""A batch whose queries read DIFFERENT row masks: 10 M x 384 cosine, top-10, 256 queries, F equal classes of random masks
(allowed fraction f), F in {1, 2, 4, 8, 16, 32, 64}, f in {0.1, 0.01}.

    python tools/bench_batch_multimask.py [rows] [dim] [nq] [k] [reps] [--out FILE]

Per (F, f), blocking host calls on one index:
  * "f_calls": F single-mask batched calls of nq / F queries each (NativeIndex.search with mask_words) -- what such a batch
    costs without the multimask entry point, and the only leg a library without it (an older commit) runs;
  * "multimask": ONE wdbx_index_search_multimask call for all nq queries (skipped when the library lacks it).
Reported per leg: wall ms per batch of nq queries, the tile kernels' time and launches from wdbx_index_profile_read_gemm
(sample + full passes), and for the multimask leg its classes, blocks, overflowed queries and the predicted blocks
ceil(sum_c 16 ceil(n_c / 16) / 256).  "mask_copy_ms": the host's share that grows with F, measured on its own -- F blocking
uploads of one mask (rows / 8 bytes each, pageable memory) through wdbx_device_upload.  wall - tile kernels is everything
else: the other kernels, launches (the per-class refine / repair launches among them) and copies.
One JSON line per case on stdout; --out appends them to FILE (default profiles/multimask/results.jsonl)."""
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
nq = int(args[2]) if len(args) > 2 else 256
k = int(args[3]) if len(args) > 3 else 10
reps = int(args[4]) if len(args) > 4 else 5
out_path = Path(flags.get("--out", ROOT / "profiles" / "multimask" / "results.jsonl"))
tag = flags.get("--tag", "")
out_path.parent.mkdir(parents=True, exist_ok=True)

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
has_multi = hasattr(ix, "search_multimask")
dq = ix.device_queries_synthetic(0xBEEF, 0, nq, True)
queries = np.ascontiguousarray(dq.download(np.float32, (nq, ix.pitch))[:, :dim])
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


base = {"tag": tag, "rows": rows, "dim": dim, "nq": nq, "k": k, "reps": reps, "has_multimask": has_multi}
ms, gemm_ms, launches = timed(lambda: ix.search(queries, k))
emit(dict(base, case="unmasked batch", ms_per_batch=ms, tile_kernels_ms=gemm_ms, tile_launches=launches))

scratch = ix.alloc((rows + 31) // 32 * 4)
for frac in (0.1, 0.01):
    pool = [_native.pack_row_mask(rng.random(rows) < frac) for _ in range(64)]
    for F in (1, 2, 4, 8, 16, 32, 64):
        if nq % F:
            continue
        masks, per = pool[:F], nq // F
        which = np.repeat(np.arange(F, dtype=np.int32), per)  # class after class: the F calls take contiguous slices
        rec = dict(base, case=f"F={F} f={frac}", F=F, f=frac, queries_per_class=per,
                   predicted_blocks=-(-F * 16 * -(-per // 16) // 256))

        def f_calls():
            for c in range(F):
                ix.search(queries[c * per:(c + 1) * per], k, mask_words=masks[c])
        ms, gemm_ms, launches = timed(f_calls)
        rec.update(f_calls_ms=ms, f_calls_tile_kernels_ms=gemm_ms, f_calls_tile_launches=launches)
        t0 = time.perf_counter()
        for _ in range(reps):
            for m in masks:
                scratch.upload(m)
        rec.update(mask_copy_ms=(time.perf_counter() - t0) / reps * 1e3)
        if has_multi:
            ms, gemm_ms, launches = timed(lambda: ix.search_multimask(queries, k, masks, which))
            st = ix.batch_status(nq)
            rec.update(multimask_ms=ms, multimask_tile_kernels_ms=gemm_ms, multimask_tile_launches=launches,
                       masked_pass=ix.get_option("last_batch_masked"), classes=ix.get_option("last_batch_mask_classes"),
                       blocks=ix.get_option("last_batch_blocks"), overflowed=st["overflowed"],
                       repaired=ix.get_option("last_batch_repaired"), speedup=rec["f_calls_ms"] / ms)
        emit(rec)
ix.close()
