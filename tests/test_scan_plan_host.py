"""The shape rules of the fp32 scan and range kernels, which need no GPU: wdbx-py_amd/csrc/host_scan_plan.h (the scan form of a
pitch and the scan options, the generic / listed lane count, the range form, the grid / partial-list / chunk / LDS arithmetic
of plan_scan), driven by tests/host_harness/scan_plan_harness.cpp -- plain g++ -Wall -Werror -- and compared with the Python
restatement in tests/scan_harness.py, which was written from choose_scan / plan_scan / pick_range_scan as they stood before
the header existed."""
import itertools
import shutil
import subprocess
from pathlib import Path

import pytest

import scan_harness as S

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "host_harness" / "scan_plan_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("scan_plan") / "scan_plan_harness"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(mode, cases):
        text = "".join(" ".join(str(int(x)) for x in c) + "\n" for c in cases)
        p = subprocess.run([str(exe), mode], input=text, capture_output=True, text=True)
        assert p.returncode == 0, (mode, p.returncode, p.stderr[-2000:])
        out = [tuple(map(int, ln.split())) for ln in p.stdout.split("\n") if ln]
        assert len(out) == len(cases)
        return out
    return run


FORM_CASES = list(itertools.product(range(1, 1001), S.LANES, (0, 1), (0, 1)))


def test_the_scan_form_of_every_pitch_equals_the_restatement(harness):
    met = set()
    for c, got in zip(FORM_CASES, harness("form", FORM_CASES)):
        pitch4, lanes, generic, force_ragged = c
        L, qpl, ragged, gen = S.scan_form_py(pitch4, lanes, generic, force_ragged)
        assert got == (L, qpl, int(ragged), int(gen), S.passes_in_flight_py(qpl), pitch4 * 16 if gen else 0), c
        if gen:
            assert L == S.generic_lanes_py(pitch4) and not ragged
        else:
            assert L * qpl >= pitch4 and ragged == (L * qpl > pitch4 or bool(force_ragged)), c
            assert (L * qpl - pitch4) * 8 <= L * qpl * 3, c  # (at most 3/8 of the slots idle on the short rows, a third on the others)
        met.add((L, qpl, bool(ragged), bool(gen)))
    # the forms met = the forms the GPU tests parametrise over (tests/test_gpu_scan_kernels.py), no more and no fewer
    assert met == {c[5] for c in S.scan_cases()}


def test_the_enumeration_of_the_instance_table():
    forms = S.enumerate_forms()
    assert len(forms) == 52
    assert sum(1 for f in forms if f[2]) == 27  # ragged; the other 25 are exact fits, which force_ragged turns ragged as well
    assert sorted(S.enumerate_generic()) == [1, 2, 4, 8, 64]
    assert len(S.scan_cases()) == 52 + 25 + 5
    assert max(p for p, _ in forms.values()) == 768 and forms[(64, 12, False)] == (768, 0)
    # the flagship shapes: d = 384 (96 quads, line aligned) fits (8, 12) exactly; d = 100 takes the wide short form
    assert S.scan_form_py(96) == (8, 12, False, False) and S.scan_form_py(25) == (32, 1, True, False)
    assert S.scan_form_py(75) == (32, 3, True, False) and S.scan_form_py(769) == (64, 0, False, True)


def test_every_form_names_an_instance(harness):
    forms = sorted({(L, q) for L, q, _ in S.enumerate_forms()})
    assert harness("has", forms) == [(1,)] * len(forms)
    assert harness("has", [(1, 2), (2, 2), (4, 4), (8, 5), (16, 7), (64, 16), (3, 1), (128, 3)]) == [(0,)] * 8


def test_the_listed_lane_count_and_the_range_form(harness):
    pitches = [(p,) for p in range(1, 1001)]
    assert harness("listed", pitches) == [(S.generic_lanes_py(p), p * 16) for p, in pitches]
    got = harness("range", pitches)
    assert got == [S.range_form_py(p) for p, in pitches]
    assert len(set(got)) == 11 == len(S.enumerate_range())
    for (p,), (P, NI) in zip(pitches, got):
        assert NI == 0 or P * NI >= p  # (an unrolled instance holds the whole row)


def test_the_plan_arithmetic_equals_the_restatement(harness):
    cases = [(n, L, k, sel, ldsl, extra, cus, per_cu, blocks, wgm, blocked)
             for n, L in itertools.product((1, 7, 63, 64, 65, 2100, 100_000, 10_000_000, 0xFFFFFEFF), (1, 2, 4, 8, 16, 32, 64))
             for k, sel, ldsl, extra in ((1, 0, 0, 0), (128, 0, 0, 0), (129, 0, 0, 0), (128, 0, 1, 0), (300, 0, 0, 12432), (2048, 1, 0, 0),
                                         (2048, 0, 0, 80), (2047, 0, 0, 32))
             for cus, per_cu, blocks in ((256, 1, 0), (256, 2, 0), (256, 8, 0), (304, 2, 7), (1, 1, 1 << 20))
             for wgm, blocked in ((0, 0), (1, 0), (0, 1), (1, 1))]
    for c, got in zip(cases, harness("plan", cases)):
        blocked = c[-1]
        assert got == S.plan_py(*c), c
        mode, groups, max_blocks, blocks, lists, chunk, lds, attr = got
        assert 1 <= blocks <= max_blocks, c
        if blocked and groups + blocks * 4 <= 1 << 32:  # (a blocked launch covers every group while the sum stays in 32 bits)
            assert chunk * blocks * 4 >= groups, c
    # the flagship: 10 M rows of 96 quads on 256 CUs, top-10
    assert harness("plan", [(10_000_000, 8, 10, 0, 0, 0, 256, 2, 0, 1, 0)]) == [(1, 1_250_000, 312_500, 512, 512, 0, 320, 0)]
    assert harness("plan", [(2100, 64, 2048, 0, 0, 777 * 16, 256, 2, 0, 0, 1)]) == [(0, 2100, 525, 512, 2048, 2, 65536 + 12432, 1)]
