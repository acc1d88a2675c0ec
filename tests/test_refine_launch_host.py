"""The launch shape of the second selection stage, which needs no GPU: wdbx-py_amd/csrc/host_refine.h (instance, waves,
n_lds, dynamic LDS bytes of refine_pairs_kernel), driven by tests/host_harness/refine_harness.cpp -- built once plain and
once under -fsanitize=address,undefined -- over every k the batched calls accept.

The arithmetic the launch site held before the header existed asked for max(4 n_lds, 17 k 8) bytes for 1024 threads
whatever k was: above 64 KiB from k = 482 without raising the function's limit, above a CU's 160 KiB from k = 1205.  It is
restated here (old_shape); wherever its request was at most 64 KiB -- every k that worked -- the header must give the same
instance, threads, n_lds and bytes."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "host_harness" / "refine_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"

MAX_K = 2048
BUDGET = 128 * 1024    # the merge kernels' (merge_waves_for, kernels_merge_select.h)
LIMIT = 64 * 1024      # what a launch may ask for without raising the function's limit
CU_LDS = 160 * 1024
STATIC_LDS = (16 + 40 + 1) * 4  # s_wcnt[16], s_k[KTH_SCRATCH = 40], s_tau


def caps(k):
    return [k + 1, 2048, 8192, 8193, 16384, 40000]


def old_shape(k, cap, lds_lists):
    """host_index.h before host_refine.h: (reg, threads, n_lds, lds)"""
    n_lds = min(cap, 8 * 1024)
    return (int(k <= 128 and not lds_lists), 1024, n_lds, max(4 * n_lds, 17 * k * 8))


def merge_waves_for(k):
    """kernels_merge_select.h"""
    return max(1, min(16, BUDGET // (k * 8) - 1))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def shapes(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("refine_" + request.param) / "refine_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)
    cases = [(k, cap, ll) for k in range(1, MAX_K + 1) for cap in caps(k) for ll in (0, 1)]
    text = "".join(f"{k} {cap} {ll}\n" for k, cap, ll in cases)
    p = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [tuple(map(int, ln.split())) for ln in p.stdout.split("\n") if ln]
    assert len(lines) == len(cases) + 1
    return lines[0], dict(zip(cases, lines[1:]))


def test_constants(shapes):
    assert shapes[0] == (8, 16, BUDGET, LIMIT)


def test_every_k_fits_the_lds_budget_and_holds_its_lists(shapes):
    refine_r, max_waves, _, _ = shapes[0]
    for (k, cap, ll), (reg, waves, n_lds, lds, raise_) in shapes[1].items():
        c = (k, cap, ll)
        assert 1 <= waves <= max_waves, c
        threads = 64 * waves
        assert threads >= 40, c  # (the threshold search's scratch is zeroed by the first KTH_SCRATCH threads)
        assert lds <= BUDGET and lds + STATIC_LDS <= CU_LDS, c
        assert 1 <= n_lds <= min(cap, refine_r * threads), c
        assert lds >= 4 * n_lds, c  # n <= n_lds: one upper bound per candidate
        assert lds >= (waves + 1) * k * 8, c  # n > n_lds: a list per wave and the final one ...
        assert lds >= 2 * k * 8, c  # ... at least one wave list plus the final list
        assert raise_ == int(lds > LIMIT), c
        assert reg == int(k <= 128 and not ll), c
        assert waves == merge_waves_for(k), c  # (the merge kernels' rule: one budget, one wave count)


def test_every_k_that_worked_keeps_its_launch(shapes):
    same = changed = 0
    for (k, cap, ll), (reg, waves, n_lds, lds, raise_) in shapes[1].items():
        old = old_shape(k, cap, bool(ll))
        if old[3] <= LIMIT:
            assert (reg, 64 * waves, n_lds, lds) == old and not raise_, (k, cap, ll)
            same += 1
        else:
            assert raise_ or lds <= LIMIT, (k, cap, ll)
            changed += 1
    # the old request passes 64 KiB from k = 482, whatever the cap is
    assert same == sum(k <= 481 for k, _, _ in shapes[1]) > 0 and changed == sum(k > 481 for k, _, _ in shapes[1]) > 0


def test_named_shapes(shapes):
    s = shapes[1]
    assert s[(10, 8192, 0)] == (1, 16, 8192, 32768, 0)     # the bench's batched k
    assert s[(100, 40000, 0)] == (1, 16, 8192, 32768, 0)
    assert s[(129, 8192, 0)] == (0, 16, 8192, 32768, 0)
    assert s[(128, 8192, 1)] == (0, 16, 8192, 32768, 0)
    assert s[(481, 40000, 0)] == (0, 16, 8192, 65416, 0)
    assert s[(482, 40000, 0)] == (0, 16, 8192, 65552, 1)   # 16 waves still, the limit raised
    assert s[(963, 40000, 0)] == (0, 16, 8192, 130968, 1)
    assert s[(964, 40000, 0)] == (0, 15, 7680, 123392, 1)  # the first k whose 17 lists pass 128 KiB
    assert s[(2048, 40000, 0)] == (0, 7, 3584, 131072, 1)
    assert s[(2048, 2049, 0)] == (0, 7, 2049, 131072, 1)
