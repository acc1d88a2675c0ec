"""The derived copies of the rows, the parts that need no GPU: the device-free header wdbx-py_amd/csrc/host_copies.h (the
coverage of one copy, its transitions under overwrite, compact, clear and extend, and the decision whether its allocations may
stay) driven by tests/host_harness/copies_harness.cpp -- built once plain and once under -fsanitize=address,undefined -- held
against the reach tests/index_model.py keeps for its committed sequences; and the one launch each range quantiser has in
host_index.h."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import index_model as M

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "host_harness" / "copies_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("copies_" + request.param) / "copies_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return [line for line in p.stdout.split("\n") if line]
    return run


def test_the_header_is_part_of_the_library_and_device_free():
    unit = (INC / "wdbx_hip.hip").read_text()
    assert unit.index('#include "host_update.h"') < unit.index('#include "host_index.h"')
    assert '#include "host_copies.h"' in (INC / "host_update.h").read_text()
    assert "host_copies.h" in (INC / "Makefile").read_text()
    header = re.sub(r"//[^\n]*", "", (INC / "host_copies.h").read_text())
    assert "hip" not in header.lower()


@pytest.mark.parametrize("granule", [1, 64])
def test_overlap_is_the_covered_part_of_the_overwritten_range(harness, granule):
    assert harness("overlap", 1000, granule, 100, 200) == ["100 200"]       # end <= rows
    assert harness("overlap", 1000, granule, 100, 1000) == ["100 1000"]
    assert harness("overlap", 1000, granule, 900, 1100) == ["900 1000"]     # first < rows < end
    assert harness("overlap", 1000, granule, 999, 1001) == ["999 1000"]
    assert harness("overlap", 1000, granule, 1000, 1100) == ["empty"]       # first >= rows
    assert harness("overlap", 1000, granule, 2000, 2001) == ["empty"]
    assert harness("overlap", 0, granule, 0, 10) == ["empty"]               # rows == 0
    assert harness("overlap", 0, granule, 5, 6) == ["empty"]


ROWS = 1000


@pytest.mark.parametrize("granule", [1, 64])
def test_cut_keeps_whole_granules_below_the_first_moved_row(harness, granule):
    for first_moved in (0, 63, 64, 65, ROWS, ROWS + 1, ROWS + 64, 1 << 40):
        want = min(ROWS, first_moved // granule * granule)
        assert harness("drive", granule, f"e{ROWS}", f"c{first_moved}") == [str(ROWS), str(want)], first_moved
    if granule == 64:   # spelled out: 63 drops the whole first group, 65 keeps exactly it, a cut inside the last group drops it
        got = [harness("drive", 64, f"e{ROWS}", f"c{m}")[1] for m in (0, 63, 64, 65, ROWS, ROWS + 1, ROWS + 64)]
        assert got == ["0", "0", "64", "64", "960", "960", "1000"]
    # a cut never extends
    assert harness("drive", granule, "e100", "c500", "c64", "c500") == ["100", "100", "64", "64"]


@pytest.mark.parametrize("granule", [1, 64])
def test_reset_extended_to_and_covers(harness, granule):
    got = harness("drive", granule, "=", "?0", "?1", "e777", "?776", "?777", "?778", "e2000", "?778", "r", "?1", "?0", "e5", "=")
    assert got == ["0", "yes", "no", "777", "yes", "yes", "no", "2000", "yes", "0", "no", "yes", "5", "5"]


def test_every_input_of_the_room_decision(harness):
    for shape in (0, 1):
        for small in (0, 1):
            for refused in (0, 1):
                want = "kept" if not (shape or small) else "no room" if refused else "fresh"
                assert harness("room", shape, small, refused) == [want], (shape, small, refused)


def test_a_refusal_is_remembered_per_capacity_and_never_by_the_bf16_flavour(harness):
    # refused at 1000: blocked there, tried again at 1500 (and refused there), 1000 is forgotten; a success remembers nothing
    assert harness("life", 1, "f1000", "f1000", "s1000", "f1500", "f1500", "f1000") == [
        "fresh", "no room", "no room", "fresh", "no room", "fresh"]
    assert harness("life", 1, "s1000", "s1000", "f2000", "s2000", "s3000", "s3000") == [
        "fresh", "fresh", "fresh", "no room", "fresh", "fresh"]
    # nothing remembered: every call tries again
    assert harness("life", 0, "f1000", "f1000", "s1000", "f1500", "f1500") == ["fresh"] * 5


@pytest.mark.parametrize("metric", ("cosine", "l2"))
def test_the_coverages_follow_the_models_reach_through_every_committed_sequence(harness, metric):
    cut, cleared = 0, 0
    for seed, d in M.SEEDS[metric]:
        t = M.Trace(d, metric)
        steps, after, cuts = [], [], []       # harness ops; per model op the index of its last line; (line of the cut, want at 64)
        for op in M.ops(seed, metric, d):
            kind, warm = op[0], bool(op[-1])
            if kind == "compact":
                keep = t.m.keep_of(op)
                moved = np.flatnonzero(keep != np.arange(len(keep)))
                first_moved = int(moved[0]) if len(moved) else len(keep)
                reach = min(t.cov, first_moved)            # the model's reach directly after the compact
                steps.append(f"c{first_moved}")
                cuts.append((len(steps) - 1, reach // 64 * 64))
            elif kind == "clear":
                steps.append("r")
            t.step(op)
            if warm and t.m.n:
                steps.append(f"e{t.m.n}")
            elif kind == "compact":
                assert t.cov == reach
            steps.append("=")
            after.append((len(steps) - 1, t.cov))
        cut, cleared = cut + len(cuts), cleared + steps.count("r")
        one = list(map(int, harness("drive", 1, *steps)))
        group = list(map(int, harness("drive", 64, *steps)))
        for line, cov in after:
            assert one[line] == cov, (seed, d, line)
            assert group[line] <= cov, (seed, d, line)
        for line, want in cuts:
            assert group[line] == want, (seed, d, line, steps[:line + 1])
    assert cut >= len(M.SEEDS[metric]) and cleared      # the sequences do compact and clear


@pytest.mark.parametrize("kernel", ["rows_to_u8_kernel", "rows_to_u6_kernel", "rows_to_u42_kernel", "rows_to_bf16_kernel",
                                    "row_sqnorm_kernel", "rows_to_i8g_kernel"])
def test_every_range_quantiser_has_one_launch_for_extend_and_refresh(kernel):
    host = re.sub(r"//[^\n]*", "", (INC / "host_index.h").read_text())
    launches = [call.split(";")[0] for call in host.split("hipLaunchKernelGGL(")[1:]]
    assert len(launches) > 40
    assert sum(1 for call in launches if re.search(r"\b%s\b" % kernel, call)) == 1, kernel
