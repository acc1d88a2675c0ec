"""grid.x of the one launch that holds all matrix-core groups of a round, which needs no GPU: u42_mfma_round_grid
(wdbx-py_amd/csrc/host_selection.h), driven by tests/host_harness/u42_round_grid_harness.cpp -- built once plain and once
under -fsanitize=address,undefined; nothing is preloaded."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "host_harness" / "u42_round_grid_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"

CASES = [(t, cus, wgs, g) for cus in (1, 8, 104, 256, 304) for wgs in (1, 2, 3) for g in (1, 2, 3, 4) for t in (1, 7, 32, 10 ** 5)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def grids(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("u42_round_" + request.param) / "u42_round_grid_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)
    text = "".join("%d %d %d %d\n" % c for c in CASES)
    p = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [tuple(map(int, ln.split())) for ln in p.stdout.split("\n") if ln]
    assert len(lines) == len(CASES) and all(len(ln) == 3 and ln[2] == 8 for ln in lines)
    return {case: ln[:2] for case, ln in zip(CASES, lines)}


def test_never_zero_and_never_more_than_the_tiles_give_work_to(grids):
    for (t, cus, wgs, g), (grid, _) in grids.items():
        assert 1 <= grid <= (t + 3) // 4, (t, cus, wgs, g)


def test_one_group_is_the_lone_pass(grids):
    for (t, cus, wgs, g), (grid, full) in grids.items():
        assert full == min((t + 3) // 4, cus * wgs)
        if g == 1:
            assert grid == full, (t, cus, wgs)


def test_a_multiple_of_the_xcd_count_unless_the_tiles_cap_it(grids):
    for (t, cus, wgs, g), (grid, _) in grids.items():
        if g > 1:
            assert grid == (t + 3) // 4 or (grid % 8 == 0 and grid >= 8), (t, cus, wgs, g)
            if (t + 3) // 4 >= 8:
                assert grid >= 8, (t, cus, wgs, g)


def test_every_group_is_resident_and_no_larger_multiple_would_be(grids):
    for (t, cus, wgs, g), (grid, _) in grids.items():
        if g > 1 and cus * wgs >= 8 * g:
            assert g * grid <= cus * wgs, (t, cus, wgs, g)
            if grid < (t + 3) // 4:  # (not capped by the tiles: the next multiple of 8 no longer fits)
                assert g * (grid + 8) > cus * wgs, (t, cus, wgs, g)


def test_named_devices(grids):
    assert grids[(10 ** 5, 256, 2, 4)][0] == 128
    assert grids[(10 ** 5, 256, 2, 3)][0] == 168
    assert grids[(10 ** 5, 256, 2, 2)][0] == 256
    assert grids[(10 ** 5, 304, 2, 4)][0] == 152
    assert grids[(10 ** 5, 104, 1, 4)][0] == 24
    assert grids[(10 ** 5, 1, 1, 4)][0] == 8      # a device too small to hold the groups at once: the floor
    assert grids[(7, 256, 2, 4)][0] == 2
