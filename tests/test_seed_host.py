"""k-means++ seeding, the parts that need no GPU: the weight function, the shift, the draw's target and the plan of
wdbx_index_seed_centers (wdbx-py_amd/csrc/host_seed.h) driven by tests/host_harness/seed_harness.cpp, built once plain and once
under -fsanitize=address,undefined."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
INC = ROOT / "wdbx-py_amd" / "csrc"
HARNESS = ROOT / "tests" / "host_harness" / "seed_harness.cpp"
NAMES = ("fits", "resident", "passes", "lds", "eval_grid", "span", "blocks", "apply_grid", "state_bytes", "scratch_bytes", "ordered")
SAT = 2 ** 31 - 1


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("seed_" + request.param) / "seed_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return list(map(int, p.stdout.split()))
    return run


@pytest.mark.parametrize("l2,score,shift,want", [
    # cosine: (1 - s) clamped to [0, 2] in units of 2^-30; NaN weighs 0
    (0, 1.0, 0, 0), (0, 1.5, 0, 0), (0, 0.0, 0, 2 ** 30), (0, -1.0, 0, 2 ** 31), (0, -7.0, 0, 2 ** 31), (0, 0.25, 0, 3 * 2 ** 28),
    (0, 1.0 - 2.0 ** -24, 0, 64), (0, float("nan"), 0, 0), (0, float("inf"), 0, 0), (0, float("-inf"), 0, 2 ** 31),
    # L2: the score is the negated squared distance, scaled by 2^shift and saturated at 2^31 - 1
    (1, -0.0, 5, 0), (1, -3.0, 4, 48), (1, -3.0, -1, 1), (1, -0.75, 0, 0), (1, -1.0, 30, 2 ** 30), (1, -1.0, 31, SAT),
    (1, -(2.0 ** 31 - 128), 0, 2 ** 31 - 128), (1, -1e30, 0, SAT), (1, float("-inf"), 0, SAT), (1, float("nan"), 0, SAT),
    (1, -1e-27, 100, 1267),  # 1e-27 * 2^100 = 1267.65
])
def test_the_weight_clamps_truncates_and_saturates(harness, l2, score, shift, want):
    assert harness("weight", l2, float(score).hex(), shift) == [want]


def test_the_shift_keeps_four_times_the_largest_norm_below_two_to_the_31(harness):
    for big in (1.0, 0.999, 1.001, 3456.0, 2.0 ** -40, 3e7, 2.0 ** 29, 2.0 ** 29 - 64):
        (shift,) = harness("shift", float(big).hex())
        assert 4 * big * 2.0 ** shift < 2 ** 31 <= 4 * big * 2.0 ** (shift + 1), (big, shift)
        # the largest distance two such rows can have, 4 M, stays below the saturation; just past it saturates
        assert harness("weight", 1, float(-4 * big).hex(), shift)[0] < SAT
        assert harness("weight", 1, float(-4 * big).hex(), shift + 1) == [SAT]
    assert harness("shift", float(0).hex()) == [100] and harness("shift", float(1e-38).hex()) == [100]
    assert harness("shift", float(3e38).hex()) == [-99]


def test_the_target_of_a_draw_is_below_the_total(harness):
    top = 2 ** 64 - 1
    for total in (1, 2, 1025, 2 ** 31, 2 ** 40 + 12345, top):
        assert harness("mulhi", 0, total) == [0]
        assert harness("mulhi", top, total) == [total - 1]
        assert harness("mulhi", 2 ** 63, total) == [total // 2]
        assert harness("mulhi", 0xDEADBEEFCAFEF00D, total) == [(0xDEADBEEFCAFEF00D * total) >> 64]


def test_the_plan_fits_the_candidates_into_lds_and_covers_every_row(harness):
    for pitch in (4, 32, 96, 384, 772, 1024, 1028, 2048, 4096):
        for n_trials in (1, 3, 5, 16):
            for n_rows in (1, 70, 1025, 2500, 1_000_000, 2 ** 31 - 1):
                for cap in (0, 2):
                    p = dict(zip(NAMES, harness("plan", n_rows, 40, n_trials, pitch, 256, cap)))
                    fit = max(1, 65536 // (4 * pitch))
                    assert p["fits"] == 1 and p["ordered"] == 1
                    assert p["resident"] == min(n_trials, fit, cap or 16) and p["passes"] == -(-n_trials // p["resident"])
                    assert p["resident"] * pitch * 4 <= p["lds"] <= 65536 and p["lds"] >= 512
                    assert 1 <= p["eval_grid"] <= 512 and p["span"] % 2 == 0 and p["eval_grid"] * 4 * p["span"] >= n_rows
                    assert p["blocks"] == -(-n_rows // 1024) and 1 <= p["apply_grid"] <= min(p["blocks"], 2048)
                    assert p["scratch_bytes"] == 4 * n_trials * n_rows
                    assert p["state_bytes"] >= 4 * n_rows + 4 * 32 * p["blocks"] + 8 * p["blocks"] + 16 * 12 + 16 * 40 + 8 * 40 * n_trials
    assert harness("plan", 1000, 4, 16, 1024, 256, 0)[1:3] == [16, 1]   # all 16 resident up to 1 024 floats per row
    assert harness("plan", 1000, 4, 16, 1028, 256, 0)[1:3] == [15, 2]
    assert harness("plan", 1000, 4, 16, 40960, 256, 0)[:3] == [1, 1, 16] and harness("plan", 1000, 4, 16, 40964, 256, 0)[0] == 0
    # the validator: 0 ok, 1 centres, 2 trials, 3 null draws, 4 null output
    assert [harness("validate", c, 3, 1, 1) for c in (1, 4096, 0, 4097)] == [[0], [0], [1], [1]]
    assert [harness("validate", 4, t, 1, 1) for t in (1, 16, 0, 17)] == [[0], [0], [2], [2]]
    assert harness("validate", 4, 3, 0, 1) == [3] and harness("validate", 4, 3, 1, 0) == [4]
