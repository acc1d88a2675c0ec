"""Candidates per query on the bench corpus (10 M x 384, fill_synthetic's rows, top-10, one round of 32 queries):
the u8 selection scan, the bf16 tiles, the six-bit u6 scan with its stored-residual bound, and the split planes
(kernels_scan42.h): rows that survive the four-bit bound and candidates behind the refine."""
import sys, numpy as np
sys.path.insert(0, "wdbx-py_amd")
from wdbx_amd import _native
ix = _native.NativeIndex(384, capacity_rows=10_000_000)
ix.fill_synthetic(0xC0FFEE, 0, 10_000_000, True)
dq = ix.device_queries_synthetic(0xBEEF, 0, 32, True)
d_idx, d_score = ix.alloc(32 * 10 * 8), ix.alloc(32 * 10 * 4)
ix.set_option("scan_u6", 0)
for path in (2, 1):
    ix.set_option("scan_shadow", path)
    ix.search_device(dq, 32, 10, d_idx, d_score); ix.synchronize()
    st = ix.batch_status(32)
    print("path", path, "candidates mean/min/max", st["counts"].mean(), st["counts"].min(), st["counts"].max(), "cap", st["capacity"])
ix.set_option("scan_shadow", 2)
ix.set_option("scan_u6", -1)
ix.set_option("scan_u42", 0)
ix.search_device(dq, 32, 10, d_idx, d_score); ix.synchronize()
assert ix.get_option("last_single_u6") == 1
st = ix.batch_status(32)
print("u6 scan: candidates mean/max", ix.get_option("u6_candidates_sum") / 32, ix.get_option("u6_candidates_max"),
      "; keys behind the cut mean/max", st["counts"].mean(), st["counts"].max(), "of", st["capacity"], "overflowed", st["overflowed"])
ix.set_option("scan_u42", 1)
ix.search_device(dq, 32, 10, d_idx, d_score); ix.synchronize()
assert ix.get_option("last_single_u42") == 1
print("u42 scan: survivors of the four-bit bound mean", ix.get_option("u42_survivors_sum") / 32, "; candidates mean/max",
      ix.get_option("u6_candidates_sum") / 32, ix.get_option("u6_candidates_max"), "; shadow42_bytes", ix.get_option("shadow42_bytes"))
print("shadow8_bytes", ix.get_option("shadow8_bytes"), "shadow6_bytes", ix.get_option("shadow6_bytes"),
      "shadow_bytes", ix.get_option("shadow_bytes"), "device_bytes_resident", ix.get_option("device_bytes_resident"))
