#!/usr/bin/env python3
"""Distance matrix among a sample of stored rows on 10 M x 384 cosine, synthetic, limit 3 and 10, samples of 10^2 .. 10^4 rows
(65 536 with --big) --
  * wdbx_index_search_matrix: wall ms per call, device ms of its scoring launches (bracketed as scan launches) and of its
    ranking launches (merge launches), the scoring launches' share of the device time;
  * in the same run and on the same handle, ALTERNATING with it, the composition a client has without the call: the sample
    read back with wdbx_index_get_rows (one call per row: the sample is not contiguous) and one wdbx_index_search_rows(nq = n, k + 1,
    the same list) -- unchanged code of the parent commit, the yardstick; its drop of "itself" in Python is NOT timed;
  * per shape the bytes that no longer cross PCIe (the sample down and up again) and whether the two answers agree wherever
    the composition is right (an anchor in its own top k + 1).

    python tools/bench_matrix.py [rows] [dim] [rounds] [--out FILE] [--big 1]

Each round runs the composition, then the call, once after one warm-up each; at least two rounds.  One JSON line per (n, limit)
on stdout; --out appends them to FILE (default profiles/matrix/results.jsonl).  Nothing is a threshold."""
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
rounds = max(2, int(args[2])) if len(args) > 2 else 3
out_path = Path(flags.get("--out", ROOT / "profiles" / "matrix" / "results.jsonl"))
out_path.parent.mkdir(parents=True, exist_ok=True)
samples = [100, 1000, 10000] + ([65536] if flags.get("--big") == "1" else [])

ix = _native.NativeIndex(dim, capacity_rows=rows)
ix.fill_synthetic(0xC0FFEE, 0, rows, True)
ix.profile(True)
rng = np.random.default_rng(1)


def once(call):
    ix.profile_read()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    p = ix.profile_read()
    return out, wall, p["scan_ms"], p["merge_ms"]


def stats(values):
    a = np.asarray(values, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()), "runs": [float(x) for x in a]}


def composition(ids, k):
    vectors = np.stack([ix.get_rows(int(r), 1)[0] for r in ids])  # (the sample is not contiguous: a read per row)
    return ix.search_rows(vectors, min(k + 1, _native.MAX_K), ids)


for n in samples:
    if n > rows:
        continue
    ids = np.sort(rng.choice(rows, n, replace=False)).astype(np.uint64)
    for k in (3, 10):
        composition(ids, k)
        ix.search_matrix(ids, k)
        rec = {"rows": rows, "dim": dim, "n": n, "limit": k, "rounds": rounds}
        old, new = [], []
        for _ in range(rounds):
            got_old, *t_old = once(lambda: composition(ids, k))
            got_new, *t_new = once(lambda: ix.search_matrix(ids, k))
            old.append(t_old)
            new.append(t_new)
        for name, t in (("composition", old), ("matrix", new)):
            wall, scan, merge = (stats([x[i] for x in t]) for i in range(3))
            rec[name] = {"wall_ms": wall, "scan_ms": scan, "merge_ms": merge,
                         "scan_share": scan["median"] / max(scan["median"] + merge["median"], 1e-9)}
        rec["matrix_path"] = ix.get_option("last_matrix_path")
        rec["matrix_rounds"] = ix.get_option("last_matrix_rounds")
        rec["pcie_bytes_saved"] = 2 * n * dim * 4  # the sample down (get_rows) and up again (the queries)
        # the composition's answer with "itself" dropped, where that is right, against the call's
        agree = right = 0
        for i in range(n):
            line = got_old[0][i]
            if int(ids[i]) in line:
                right += 1
                agree += int(line[line != int(ids[i])][:k].tolist() == got_new[0][i].tolist())
        rec["composition_right_lines"], rec["lines_agreeing"] = right, agree
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")
ix.close()
