"""The k-NN graph, the parts that need no GPU: the device-free plan and margin of wdbx_index_knn_graph
(wdbx-py_amd/csrc/host_knn.h) driven by tests/host_harness/knn_harness.cpp, built once plain and once under
-fsanitize=address,undefined."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
INC = ROOT / "wdbx-py_amd" / "csrc"
HARNESS = ROOT / "tests" / "host_harness" / "knn_harness.cpp"
NAMES = ("path", "cap", "lds", "anchor_tiles", "cand_tiles", "grid", "passes", "exact_grid", "list_bytes", "count_bytes",
         "flag_bytes", "covered")
NONE, TILES, REPAIR = 0, 1, 2


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("knn_" + request.param) / "knn_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return list(map(int, p.stdout.split()))
    return run


def test_the_plan_keeps_lds_scratch_capacity_and_grid_within_their_limits(harness):
    max_k, anchor_tile, cand_tile, lds_limit, budget, tile_min = harness("limits")
    assert (max_k, anchor_tile, cand_tile) == (64, 128, 128) and 2 * lds_limit <= 160 * 1024
    lds = set()
    for k in (1, 2, 10, 15, 31, 32, 33, 63, 64):
        for n_rows in (1, 127, 128, 129, 511, 512, 513, 2700, 65_536, 65_537, 1_000_000, 100_000_000):
            for cus in (1, 64, 256, 304):
                cap = 3 if cus == 64 else 0  # (the option knn_max_grid: more passes, everything else as without it)
                p = dict(zip(NAMES, harness("plan", n_rows, n_rows, k, cus, 1, 1, cap)))
                assert p["covered"] == 1 and p["grid"] <= (cap or p["grid"]), (k, n_rows, cus, p)
                assert p["path"] == (TILES if n_rows >= tile_min else REPAIR)
                assert p["cap"] >= k + cand_tile and p["cap"] % 64 == 0
                assert 0 < p["lds"] <= lds_limit
                lds.add(p["lds"])
                assert 1 <= p["grid"] <= min(p["anchor_tiles"], 2 * cus) and p["passes"] == -(-p["anchor_tiles"] // p["grid"])
                assert p["anchor_tiles"] == -(-n_rows // anchor_tile) and p["cand_tiles"] == -(-n_rows // cand_tile)
                assert p["list_bytes"] == p["grid"] * anchor_tile * p["cap"] * 8
                assert p["list_bytes"] + p["count_bytes"] <= budget and p["flag_bytes"] == 4 * n_rows
                assert 1 <= p["exact_grid"] <= 8 * cus
    assert len(lds) == 1  # the row length is not an argument of the plan: LDS does not depend on it (dim 4 ... 4096)


def test_the_route_cut_is_monotone_the_fallbacks_repair_and_the_validator_refuses(harness):
    tile_min = harness("limits")[5]
    paths = [harness("plan", 10_000, e, 10, 256, 1, 1)[0] for e in range(0, 2 * tile_min, 37)]
    assert paths[0] == NONE and paths == sorted(paths, key=lambda p: (p != NONE, p == TILES))  # none, then repair, then tiles
    assert harness("plan", 10_000, tile_min - 1, 10, 256, 1, 1)[0] == REPAIR
    assert harness("plan", 10_000, tile_min, 10, 256, 1, 1)[0] == TILES
    assert harness("plan", 10_000, 10_000, 10, 256, 0, 1)[0] == REPAIR  # no room for the bf16 copy
    assert harness("plan", 10_000, 10_000, 10, 256, 1, 0)[0] == REPAIR  # an eligible row with an infinite norm
    assert harness("plan", 0, 0, 10, 256, 1, 1)[0] == NONE
    # the validator: 0 ok, 1 k outside [1, 64], 2 a null output
    assert [harness("validate", k, 1, 1) for k in (1, 64, 0, 65, -1)] == [[0], [0], [1], [1], [1]]
    assert harness("validate", 5, 0, 1) == [2] and harness("validate", 5, 1, 0) == [2]


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("worst", [0, 1])
@pytest.mark.parametrize("dim", [4, 20, 384, 770, 4096])
def test_the_tile_margin_bounds_the_bf16_tile_value(harness, dim, worst, l2):
    """|T - S| <= b_T: T from bf16-rounded operands on an fp32 fma chain, S in float64 from the fp32 operands."""
    violations, max_ppm = harness("margin", dim, l2, 300, 1234 + dim, worst)
    print(f"dim {dim} l2 {l2} worst {worst}: largest |T - S| / b_T = {max_ppm / 1e6:.4f}")
    assert violations == 0 and max_ppm <= 1_000_000
