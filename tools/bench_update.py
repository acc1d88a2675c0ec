"""Wall time of updating / removing n stored rows: the per-row ``set_rows`` loop against one ``set_rows_at`` /
``remove_rows`` call.

    python tools/bench_update.py --rows 1000000 --dim 384 --n 1 100 10000 --repeats 5

Cosine corpus filled on the device, every default copy built by a search on each route first.  Per n: ``repeats`` timings of
each form over the same random stored rows (new contents each time), the median and the spread (max - min) of each in
milliseconds, one JSON line per (operation, n).  On a library without ``wdbx_index_set_rows_at`` (the parent commit) only the
per-row loop is timed, so the same tool gives the parent's lines; alternate the two builds as profiles/README.md describes."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "wdbx-py_amd"))

from wdbx_amd import _native  # noqa: E402

ROUTES = [{"gemm_min_queries": 1 << 30}, {"gemm_min_queries": 1 << 30, "scan_u6": 1, "scan_u42": 1}, {"gemm_min_queries": 4}]


def _build_copies(ix, dim):
    rng = np.random.default_rng(1)
    q = rng.standard_normal((16, dim)).astype(np.float32)
    for opts in ROUTES:
        for key, value in {"single_min_rows": 0, "gemm_min_rows": 0, "gemm_min_work": 1, **opts}.items():
            ix.set_option(key, value)
        ix.search(q, 10, normalize_queries=True)


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 100, 10_000])
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    listed = hasattr(_native.NativeIndex, "set_rows_at")
    rng = np.random.default_rng(7)
    with _native.NativeIndex(args.dim, capacity_rows=args.rows) as ix:
        ix.fill_synthetic(1, 0, args.rows, normalize=True)
        _build_copies(ix, args.dim)
        copies = {name: ix.get_option(name) for name in ("shadow_rows", "shadowg_rows", "shadow8_rows", "shadow6_rows", "shadow42_rows")}
        nan_row = np.full(args.dim, np.nan, np.float32)
        for n in args.n:
            for op in ("set", "remove"):
                loop_ms, call_ms = [], []
                for _ in range(args.repeats + 1):  # (the first pass of each form warms it up and is dropped)
                    ids = np.sort(rng.choice(args.rows, n, replace=False)).astype(np.uint64)
                    new = rng.standard_normal((n, args.dim)).astype(np.float32)

                    def per_row():
                        for r, row in zip(ids, new):
                            ix.set_rows(int(r), row if op == "set" else nan_row, normalize=op == "set")
                    loop_ms.append(_timed(per_row))
                    if listed:
                        call_ms.append(_timed((lambda: ix.set_rows_at(ids, new, normalize=True)) if op == "set"
                                              else (lambda: ix.remove_rows(ids))))
                rec = {"op": op, "n": n, "rows": args.rows, "dim": args.dim, "copies": copies,
                       "per_row_ms_median": float(np.median(loop_ms[1:])), "per_row_ms_spread": float(np.ptp(loop_ms[1:]))}
                if listed:
                    rec.update({"listed_ms_median": float(np.median(call_ms[1:])), "listed_ms_spread": float(np.ptp(call_ms[1:])),
                                "launches": ix.get_option("last_update_launches")})
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
