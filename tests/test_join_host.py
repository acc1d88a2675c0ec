"""The similarity self-join, the parts that need no GPU: the device-free plan and tile test of wdbx_index_self_join
(wdbx-py_amd/csrc/host_join.h) driven by tests/host_harness/join_harness.cpp, built once plain and once under
-fsanitize=address,undefined.  The tile test is held against float64 in the manner of tests/test_selection_bounds_range_batch.py:
rows quantised as group_to_i8g quantises them, and every pair the exact pass could keep must pass D >= T_AB."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
INC = ROOT / "wdbx-py_amd" / "csrc"
HARNESS = ROOT / "tests" / "host_harness" / "join_harness.cpp"
NAMES = ("path", "why", "refused", "ct8", "block_rows", "blocks", "tiles", "lds", "grid", "pair_cap", "tile_visits", "covered")
NONE, SWEEP, EXACT = 0, 1, 2
GAMMA = 2e-6
f32 = np.float32


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("join_" + request.param) / "join_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args, stdin=None):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, input=stdin)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return list(map(int, p.stdout.split()))
    return run


def plan(harness, n, eligible=None, pitch8=384, shadow=1, cus=256, max_grid=0, pair_cap=0, min_rows=1024, exact_max=65536):
    return dict(zip(NAMES, harness("plan", n, n if eligible is None else eligible, pitch8, shadow, cus, max_grid, pair_cap,
                                   min_rows, exact_max)))


def test_the_blocks_partition_the_rows_the_triangle_adds_up_and_lds_stays_in_budget(harness):
    tile_rows, max_pitch8, lds_block_max, pair_bytes_max, pair_cap_min, _, _ = harness("limits")
    assert (tile_rows, max_pitch8, lds_block_max) == (256, 1536, 96 * 1024)
    for dim in (4, 100, 128, 129, 384, 385, 768, 769, 1000, 1536):
        pitch8 = -(-dim // 128) * 128
        block_rows = 128 if pitch8 <= 768 else 64  # block size follows the pitch
        for n in (1024, 1025, 2700, 65_537, 1_000_000):
            for cus, max_grid in ((256, 0), (256, 3), (1, 0)):
                p = plan(harness, n, pitch8=pitch8, cus=cus, max_grid=max_grid)
                assert p["path"] == SWEEP and p["covered"] == 1 and p["refused"] == 0, (dim, n, p)
                assert p["block_rows"] == block_rows == 32 * p["ct8"] and p["blocks"] == -(-n // block_rows)
                assert p["tiles"] == -(-n // tile_rows)
                per_tile = tile_rows // block_rows  # blocks that start at the same tile
                assert p["tile_visits"] == sum(p["tiles"] - i // per_tile for i in range(p["blocks"]))
                assert block_rows * pitch8 <= lds_block_max and p["lds"] == block_rows * pitch8 + 4 * block_rows
                assert p["lds"] <= 97 * 1024  # the resident block and its anchors' norms
                assert 1 <= p["grid"] <= min(p["blocks"], cus, max_grid or cus)
                assert pair_cap_min <= p["pair_cap"] and p["pair_cap"] * 8 <= pair_bytes_max
    assert plan(harness, 5000, pair_cap=100)["pair_cap"] == 100 and plan(harness, 5000, pair_cap=1)["pair_cap"] == pair_cap_min


def test_the_route_table_and_the_validator(harness):
    assert plan(harness, 0)["path"] == NONE and plan(harness, 5000, eligible=1)["path"] == NONE
    assert plan(harness, 5000, eligible=1023)["path"] == EXACT and plan(harness, 5000, eligible=1024)["path"] == SWEEP
    assert plan(harness, 5000, eligible=2, min_rows=0)["path"] == SWEEP
    # what sends a call to the exact route: 1 the row length, 2 no room for the shadow copy, 3 too few eligible rows
    assert [plan(harness, 5000, pitch8=p8)["why"] for p8 in (0, 1664, 200)] == [1, 1, 1]
    assert plan(harness, 5000, shadow=0)["why"] == 2 and plan(harness, 5000, eligible=10)["why"] == 3
    for kw in (dict(pitch8=0), dict(shadow=0), dict(eligible=10)):
        assert plan(harness, 65_536, **kw)["refused"] == 0 and plan(harness, 65_537, **kw)["refused"] == 1
        assert plan(harness, 5000, exact_max=4999, **kw)["refused"] == 1
    assert plan(harness, 10_000_000)["refused"] == 0  # the sweep is never refused by the exact route's limit
    # the validator: 0 ok, 1 a NaN threshold, 2 null offsets, 3 capacity without buffers
    assert harness("validate", 0, 1, 0, 0, 0) == [0] and harness("validate", 0, 1, 9, 1, 1) == [0]
    assert harness("validate", 1, 1, 0, 0, 0) == [1] and harness("validate", 0, 0, 0, 0, 0) == [2]
    assert harness("validate", 0, 1, 9, 0, 1) == [3] and harness("validate", 0, 1, 9, 1, 0) == [3]


def quantise(rows):
    """One 64-row group as group_to_i8g quantises it: (signed bytes as int64, {s_g, a_g, b_g})."""
    dim = rows.shape[1]
    mx = f32(np.abs(rows).max())
    vanishing = mx < f32(1.2e-30)
    s = f32(2) * mx if vanishing else mx / f32(127)
    inv = f32(0) if vanishing else f32(127) / mx
    x = np.clip(np.rint(rows * inv), -127, 127).astype(f32)
    res = np.full_like(rows, 0.5 if mx > 0 else 0.0) if vanishing else rows * inv - x
    n2, d2 = (x.astype(np.float64) ** 2).sum(1).max(), (res.astype(np.float64) ** 2).sum(1).max()
    a_g = s * f32(np.sqrt(n2)) * f32(1.0002)
    b_g = s * (f32(np.sqrt(d2)) * f32(1.0002) + f32(2e-5) * f32(np.sqrt(dim)))
    return x.astype(np.int64), (s, a_g, b_g)


def groups(kind, dim, rng):
    a = rng.standard_normal((64, dim)).astype(f32)
    b = (a[rng.permutation(64)] + 0.15 * rng.standard_normal((64, dim))).astype(f32)  # near-duplicates of A's rows
    if kind in ("unit", "outlier", "vanishing"):
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        b /= np.linalg.norm(b, axis=1, keepdims=True)
    if kind == "unnormalised":
        a *= rng.uniform(0.01, 30, (64, 1)).astype(f32)
        b *= rng.uniform(0.01, 30, (64, 1)).astype(f32)
    if kind == "outlier":
        b[7, 3] = 40.0  # one element owns the group's scale: every other row quantises coarsely
    if kind == "vanishing":
        a *= f32(1e-33)
    return a, b


@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("dim", [100, 384])
@pytest.mark.parametrize("kind", ["unit", "unnormalised", "outlier", "vanishing"])
def test_no_pair_the_exact_pass_could_keep_fails_the_tile_test(harness, kind, dim, l2):
    rng = np.random.default_rng(1000 * dim + 10 * len(kind) + l2)
    a, b = groups(kind, dim, rng)
    (na, ga), (nb, gb) = quantise(a), quantise(b)
    D = na @ nb.T
    cna, cnb = (a * a).sum(1, dtype=f32), (b * b).sum(1, dtype=f32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    if l2:
        real = ((a64[:, None, :] - b64[None, :, :]) ** 2).sum(2)
        fp32 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(2, dtype=f32)
    else:
        real = a64 @ b64.T
        fp32 = a @ b.T
    gam = GAMMA * np.linalg.norm(a64, axis=1)[:, None] * np.linalg.norm(b64, axis=1)[None, :]
    # thresholds across the pairs' scores: the duplicates' level, the bulk's, and both ends
    lines, must = [], []
    for t in np.quantile(real, [0.0, 0.02, 0.5, 0.98, 1.0]).astype(f32):
        need = ((fp32 <= t) | (real * (1 - GAMMA) <= t)) if l2 else ((fp32 >= t) | (real + gam >= t))
        for i, j in zip(*np.nonzero(np.ones_like(need))):
            lines.append(" ".join([str(l2), float(t).hex(), *(float(v).hex() for v in (*ga, *gb)), str(int(D[i, j])),
                                   float(cna[i]).hex(), float(cnb[j]).hex()]))
            must.append(bool(need[i, j]))
    keep = np.array(harness("keep", stdin="\n".join(lines) + "\n"), bool)
    must = np.array(must)
    assert keep.shape == must.shape and not (must & ~keep).any(), f"{(must & ~keep).sum()} pairs lost"
    print(f"{kind} dim {dim} l2 {l2}: {must.sum()} required, {keep.sum()} kept of {keep.size}")
    if kind == "unit":  # the test is a test: it keeps few pairs more than it must
        assert keep.sum() <= must.sum() + 0.05 * keep.size
