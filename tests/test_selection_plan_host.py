"""The plan of the selection rounds, which needs no GPU: wdbx-py_amd/csrc/host_selection.h (sampled tiles, stride, bounds,
expected rows, candidate and pair capacities, the masked sample's growth, the 1 GiB shadow rule), driven by
tests/host_harness/selection_harness.cpp -- built once plain and once under -fsanitize=address,undefined -- and compared field
by field with the expressions the four enqueue functions held before the header existed (tests/selection_parent.py)."""
import itertools
import shutil
import subprocess
from pathlib import Path

import pytest

import selection_parent as P

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "host_harness" / "selection_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"

KS = [1, 10, 32, 100, 128, 129, 200, 1024, P.MAX_K]
DIVS = [0, 1, 7, 64, 1000]
N_MAX = 0xFFFFFEFF  # just under the largest row count the tile entry points accept (n < 0xFFFFFF00)


def _rows(tile_rows):
    # 100 000 rows: tiles / div (12 at 256-row tiles and 1 / 32) stays under ceil(8 k / rw) (20 at k = 10, rw = 4)
    return [1, tile_rows - 1, tile_rows, tile_rows + 1, 100_000, 10_000_000, N_MAX]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("selection_" + request.param) / "selection_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(mode, cases):
        text = "".join(" ".join(str(int(x)) for x in c) + "\n" for c in cases)
        p = subprocess.run([str(exe), mode], input=text, capture_output=True, text=True)
        assert p.returncode == 0, (mode, p.returncode, p.stderr[-2000:])
        out = [tuple(map(int, ln.split())) for ln in p.stdout.split("\n") if ln]
        assert len(out) == len(cases)
        return out
    return run


def test_the_four_callers_have_the_shapes_the_kernels_declare():
    assert P.U8 == (256, 4, True, 32) and P.U6 == (256, 4, True, 256)
    assert P.LEGACY_FP32 == (128, 2, False, 8) and P.LEGACY_BF16 == (256, 4, True, 32) and P.INT8 == (256, 8, True, 32)
    assert P.MAX_K == 2048


def test_sample_stride_bounds_expect_and_capacity_equal_the_parent(harness):
    cases = [(n, tile_rows, rw, k, div, scaled, factor)
             for tile_rows, rw, _, factor in P.CALLERS.values()
             for n, k, div, scaled in itertools.product(_rows(tile_rows), KS, DIVS, (0, 1))]
    failed = 0
    for c, got in zip(cases, harness("sample", cases)):
        n, tile_rows, rw, k, div_opt, scaled, factor = c
        want = P.plan(n, tile_rows, rw, k, div_opt, bool(scaled), factor)
        div, tiles, sample_tiles, stride, bounds, expect, cap = got
        assert got == (want["div"], want["tiles"], want["sample_tiles"], want["stride"], want["bounds"], want["expect"], want["cap"]), c
        assert 1 <= sample_tiles <= tiles and stride >= 1 and stride * sample_tiles <= tiles, c  # (the last sampled tile exists)
        assert 4096 <= cap <= 1 << 22, c
        assert (bounds < k) == want["too_small"], c  # the callers' "corpus too small"
        failed += bounds < k
    assert 0 < failed < len(cases)  # (both outcomes are in the grid)


def test_named_plans(harness):
    # the bench corpus, top-10: 39 063 tiles, 1 / 32 of them sampled
    assert harness("sample", [(10_000_000, *P.U8[:2], 10, 0, 1, 32)]) == [(32, 39063, 1220, 32, 4880, 330, 10560)]
    assert harness("sample", [(10_000_000, *P.U6[:2], 10, 0, 1, 256)]) == [(32, 39063, 1220, 32, 4880, 330, 84480)]
    assert harness("sample", [(10_000_000, *P.INT8[:2], 100, 0, 1, 32)]) == [(10, 39063, 3906, 10, 31248, 1100, 35200)]
    # the exact fp32 tiles keep 1 / 32 whatever k is
    assert harness("sample", [(10_000_000, *P.LEGACY_FP32[:2], 100, 0, 0, 8)]) == [(32, 78125, 2441, 32, 4882, 3300, 26400)]
    # gemm_sample_div = 1: every tile, stride 1
    assert harness("sample", [(20011, *P.INT8[:2], 10, 1, 1, 32)]) == [(1, 79, 79, 1, 632, 20, 4096)]
    # the floor of 8 k bounds decides on a small corpus
    assert harness("sample", [(100_000, *P.U8[:2], 10, 0, 1, 32)]) == [(32, 391, 20, 19, 80, 200, 6400)]
    # the capacity's ceiling
    assert harness("sample", [(N_MAX, *P.U6[:2], P.MAX_K, 1000, 1, 256)])[0][6] == 1 << 22


def test_masked_sample_equals_the_parent_and_only_grows(harness):
    tile_rows, rw, _, _ = P.INT8
    cases = []
    for n in [0] + _rows(tile_rows):
        # a mask never allows more rows than there are -- but 16 384 (no growth whatever n is) and, on the empty corpus,
        # 16 385 (the rule's f = 0 branch) are asked everywhere
        sizes = {a for a in (16385, n // 1000, n // 8, n // 2, n) if a <= n} | {16384} | ({16385} if n == 0 else set())
        cases += [(n, tile_rows, rw, k, div, a) for a in sorted(sizes) for k in KS for div in DIVS]
    grew = 0
    for c, got in zip(cases, harness("masked", cases)):
        n, _, _, k, div_opt, allowed = c
        base, sample_tiles, stride, bounds, expect, cap = got
        want = P.masked_plan(n, k, div_opt, allowed)
        tiles = want["tiles"]
        assert base == P.plan(n, tile_rows, rw, k, div_opt, True, 32)["sample_tiles"], c
        assert (sample_tiles, stride, bounds, expect, cap) == (want["sample_tiles"], want["stride"], want["bounds"], want["expect"], want["cap"]), c
        assert base <= sample_tiles <= max(tiles, 1), c  # never below the unmasked sample, never above the tiles (the clamp's floor is 1)
        if allowed <= 16384:
            assert sample_tiles == base, c
        grew += sample_tiles > base
    assert grew > 0


def test_named_masked_samples(harness):
    tile_rows, rw, _, _ = P.INT8
    n = 10_000_000  # 39 063 tiles, 1 220 of them sampled without a mask at k = 10
    got = harness("masked", [(n, tile_rows, rw, 10, 0, a) for a in (16384, n, n // 2, n // 8, n // 100)])
    assert [g[:2] for g in got] == [(1220, 1220), (1220, 1220), (1220, 2440), (1220, 9760), (1220, 9760)]


def test_pair_capacity_and_the_1gib_rule(harness):
    pairs = [(e, w) for e in (1, 20, 330, 1100, 84480, P.MAX_K * (N_MAX // 256 + 1)) for w in (8, 79 * 8, 2048)]
    assert harness("pairs", pairs) == [(P.pair_cap(e, w),) for e, w in pairs]
    assert harness("pairs", [(330, 2048), (1, 8), (10 ** 9, 8)]) == [(16384,), (16384,), (65536,)]
    sizes = [(0, 384), (1, 16), (1 << 23, 128), ((1 << 23) + 1, 128), (2796202, 384), (2796203, 384), (10_000_000, 384), (N_MAX, 4096)]
    assert harness("gib", sizes) == [(int(P.shadow_over_1gib(n, p)),) for n, p in sizes]
    assert harness("gib", sizes) == [(0,), (0,), (0,), (1,), (0,), (1,), (1,), (1,)]
