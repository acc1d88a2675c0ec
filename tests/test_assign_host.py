"""Nearest-centre assignment, the parts that need no GPU: the device-free plan of wdbx_index_assign
(wdbx-py_amd/csrc/host_assign.h) driven by tests/host_harness/assign_harness.cpp -- built once plain and once under
-fsanitize=address,undefined -- and ``HipFlatIndex.assign`` over a stub of the binding: the ingest lock held around the
native call, ids mapped only when a per-row output is asked for."""
import shutil
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
INC = ROOT / "wdbx-py_amd" / "csrc"
HARNESS = ROOT / "tests" / "host_harness" / "assign_harness.cpp"
NAMES = ("mt", "block", "n_blocks", "slots", "lds", "tiles", "grid", "prep_grid", "exact_grid", "partials", "sums_grid",
         "rows_per_partial", "centre_bytes", "aux_bytes", "partial_bytes", "covered")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("assign_" + request.param) / "assign_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return list(map(int, p.stdout.split()))
    return run


def test_blocks_cover_every_centre_once_and_lds_stays_within_the_limit(harness):
    max_centers, block_max, lds_limit, budget, tile_rows = harness("limits")
    assert (max_centers, block_max, tile_rows) == (4096, 128, 128) and 2 * lds_limit <= 160 * 1024
    for dim in (4, 5, 100, 384, 770, 4096):
        pitch = (dim + 3) // 4 * 4
        for k in (1, 2, 31, 32, 33, 64, 65, 127, 128, 129, 255, 257, 1024, 4095, 4096):
            for n_rows, l2 in ((1, 0), (127, 1), (129, 0), (1500, 1), (10_000_000, 0), (10_000_000, 1)):
                p = dict(zip(NAMES, harness("plan", n_rows, k, pitch, 256, l2)))
                assert p["covered"] == 1, (dim, k, n_rows, p)
                assert p["block"] == 32 * p["mt"] <= block_max and p["mt"] in (1, 2, 4)
                assert p["n_blocks"] == -(-k // p["block"]) and p["slots"] == p["n_blocks"] * p["block"]
                assert 0 < p["lds"] <= lds_limit
                resident = 1 if l2 and p["mt"] == 4 else 2  # workgroups a CU holds at once: the persistent grid follows it
                assert p["tiles"] == -(-n_rows // tile_rows) and p["grid"] == max(1, min(p["tiles"], resident * 256))
                assert 1 <= p["partials"] <= 2048 and p["sums_grid"] == -(-p["partials"] // 4)
                assert p["partial_bytes"] == p["partials"] * k * (pitch + 1) * 4 <= max(budget, k * (pitch + 1) * 4)
                assert p["centre_bytes"] == p["slots"] * pitch * 4 and p["aux_bytes"] == p["slots"] * 4 + 8
    assert dict(zip(NAMES, harness("plan", 1000, 16, 384, 256, 0)))["mt"] == 1  # (16 centres do not pay for 128 accumulator rows)


def test_the_validator_refuses_what_the_header_lists(harness):
    ok, bad_count, null_centers, no_output = 0, 1, 2, 3
    assert harness("validate", 1, 1, 1) == [ok] and harness("validate", 4096, 1, 1) == [ok]
    assert harness("validate", 0, 1, 1) == [bad_count] and harness("validate", 4097, 1, 1) == [bad_count]
    assert harness("validate", -3, 1, 1) == [bad_count]
    assert harness("validate", 5, 0, 1) == [null_centers]
    assert harness("validate", 5, 1, 0) == [no_output]


class _StubNative:
    """``_native.NativeIndex.assign``: records what was asked for and whether another thread (an ``add``) could take the lock."""

    def __init__(self, lock, rows):
        self.lock, self.rows, self.calls = lock, rows, []

    def assign(self, centers, normalize=False, mask=None, want=()):
        got = []
        t = threading.Thread(target=lambda: got.append(self.lock.acquire(blocking=False)))
        t.start()
        t.join()
        self.calls.append((tuple(sorted(want)), got[0]))
        out = {"center": np.array([0, -1, 1] * (self.rows // 3), np.int32), "score": np.ones(self.rows, np.float32),
               "sums": np.zeros((2, 4), np.float32), "counts": np.zeros(2, np.uint64)}
        return {k: out[k] for k in want}


def test_the_index_holds_its_ingest_lock_and_maps_ids_only_for_per_row_outputs():
    from wdbx_amd import _native, indexing

    ix = indexing.HipFlatIndex.__new__(indexing.HipFlatIndex)
    ix._ingest_lock = threading.RLock()
    ix._native = _StubNative(ix._ingest_lock, 6)
    ix.vector_dim, ix.metric, ix.next_index, ix.swallow_errors = 4, _native.METRIC_L2, 6, False
    ix.index_to_id, ix._implicit = {r: f"v{r}" for r in range(6)}, []
    centers = np.ones((2, 4), np.float32)
    out = ix.assign(centers, want=("score",))
    assert out["ids"] == ["v0", "v2", "v3", "v5"] and out["rows"].tolist() == [0, 2, 3, 5]
    assert out["center"].tolist() == [0, 1, 0, 1] and out["score"].tolist() == [-1.0] * 4  # (L2: as search returns them)
    sums = ix.assign(centers, want=("sums", "counts"))
    assert sorted(sums) == ["counts", "sums"]  # nothing per row was asked of the device, no id was mapped
    # an add on another thread could not have taken the lock during either native call
    assert ix._native.calls == [(("center", "score"), False), (("counts", "sums"), False)]
