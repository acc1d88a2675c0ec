"""The int8 route of nearest-centre assignment, the parts that need no GPU: the device-free plan and inequality of
wdbx-py_amd/csrc/host_assign8.h driven by tests/host_harness/assign8_harness.cpp, built once plain and once under
-fsanitize=address,undefined.  The inequality is held against float64: rows quantised as group_to_i8g quantises a 64-row group,
centres as assign_quant_kernel quantises each one, and for every (row, centre) |real - T| must stay within the header's bound."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
INC = ROOT / "wdbx-py_amd" / "csrc"
HARNESS = ROOT / "tests" / "host_harness" / "assign8_harness.cpp"
NAMES = ("path", "why", "ct8", "block", "n_blocks", "slots", "lds", "tiles", "grid", "quant_grid", "pair_cap", "covered")
FP32, I8 = 1, 2
OFF, PITCH, FEW_ROWS, SHADOW = 1, 2, 3, 4
f32 = np.float32


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("assign8_" + request.param) / "assign8_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args, stdin=None):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, input=stdin)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return p.stdout.split()
    return run


def plan(harness, n=100_000, k=300, pitch8=384, opt=1, min_rows=65536, shadow=1, cus=256, max_grid=0, pair_cap=0):
    return dict(zip(NAMES, map(int, harness("plan", opt, n, min_rows, pitch8, shadow, k, cus, max_grid, pair_cap))))


def test_every_centre_is_in_one_block_and_two_blocks_fit_the_lds(harness):
    for dim in (4, 100, 128, 129, 384, 512, 513, 770, 1024):
        pitch8 = -(-dim // 128) * 128
        block = 128 if pitch8 <= 512 else 64
        for k in (1, 33, 64, 65, 128, 129, 600, 4095, 4096):
            for n, cus, max_grid in ((1, 256, 0), (257, 256, 0), (1_000_000, 256, 3), (1_000_000, 1, 0)):
                p = plan(harness, n=n, k=k, pitch8=pitch8, cus=cus, max_grid=max_grid)
                assert p["path"] == I8 and p["why"] == 0 and p["covered"] == 1, (dim, k, p)
                assert p["block"] == block == 32 * p["ct8"] and p["n_blocks"] == -(-k // block) and p["slots"] == p["n_blocks"] * block
                assert p["lds"] == 2 * block * (pitch8 + 8) <= 160 * 1024
                assert p["tiles"] == -(-n // 256) and 1 <= p["grid"] <= min(p["tiles"], cus, max_grid or cus)
                assert p["quant_grid"] * 4 >= p["slots"] and 64 <= p["pair_cap"] <= (2 << 30) // 8
    assert plan(harness, pair_cap=100)["pair_cap"] == 100 and plan(harness, pair_cap=1)["pair_cap"] == 64


def test_the_route_and_its_reasons(harness):
    # forced: the row count is ignored; what still sends the call to the fp32 tiles: the row length, the shadow copy
    assert plan(harness, n=1)["path"] == I8
    assert [plan(harness, pitch8=p8)["why"] for p8 in (0, 200, 1152, 4096)] == [PITCH] * 4
    assert plan(harness, shadow=0)["why"] == SHADOW and plan(harness, shadow=0)["path"] == FP32
    assert plan(harness, opt=0)["why"] == OFF and plan(harness, opt=0, n=10_000_000)["path"] == FP32
    # the library's choice never takes a handle under 32 768 rows off the fp32 tiles, whatever assign_i8_min_rows says
    for n in (1, 300, 20_000, 32_767):
        p = plan(harness, opt=-1, n=n, min_rows=0)
        assert p["path"] == FP32 and p["why"] in (OFF, FEW_ROWS)
    big, small = plan(harness, opt=-1, n=10_000_000), plan(harness, opt=-1, n=65_535)
    assert small["path"] == FP32 and big["path"] in (FP32, I8) and (big["path"] == I8) == (big["why"] == 0)


def quantise(rows, per_row):
    """group_to_i8g's arithmetic for one group (per_row = False) or with every row a group of its own (the centres)."""
    dim = rows.shape[1]
    mx = np.abs(rows).max(axis=1, keepdims=True).astype(f32) if per_row else np.full((len(rows), 1), np.abs(rows).max(), f32)
    vanishing = mx < f32(1.2e-30)
    safe = np.where(vanishing, f32(1), mx)
    s = np.where(vanishing, f32(2) * mx, mx / f32(127)).astype(f32)
    inv = np.where(vanishing, f32(0), f32(127) / safe).astype(f32)
    x = np.clip(np.rint(rows * inv), -127, 127).astype(f32)
    res = np.where(vanishing, np.where(mx > 0, f32(0.5), f32(0)), rows * inv - x)
    n2, d2 = (x.astype(np.float64) ** 2).sum(1), (res.astype(np.float64) ** 2).sum(1)
    a = s[:, 0] * np.sqrt(n2).astype(f32) * f32(1.0002)
    b = s[:, 0] * (np.sqrt(d2).astype(f32) * f32(1.0002) + f32(2e-5) * f32(np.sqrt(dim)))
    return x.astype(np.int64), s[:, 0], a.astype(f32), b.astype(f32)


def operands(kind, dim, rng):
    c = rng.standard_normal((64, dim)).astype(f32)
    r = (c[rng.permutation(64)] + 0.15 * rng.standard_normal((64, dim))).astype(f32)  # rows near the centres
    if kind in ("unit", "outlier", "vanishing"):
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        r /= np.linalg.norm(r, axis=1, keepdims=True)
    if kind == "unnormalised":
        c *= rng.uniform(0.01, 30, (64, 1)).astype(f32)
        r *= rng.uniform(0.01, 30, (64, 1)).astype(f32)
    if kind == "outlier":
        r[7, 3] = 40.0   # one element owns the group's scale: every other row quantises coarsely
        c[5, 9] = -25.0  # ... and one centre's own
    if kind == "vanishing":
        r *= f32(1e-33)
    return r, c


# 4 kinds x 2 dims x 2 metrics x (64 rows x 64 centres) = 65 536 sampled (row, centre) pairs per build of the harness
@pytest.mark.parametrize("l2", [0, 1])
@pytest.mark.parametrize("dim", [100, 384])
@pytest.mark.parametrize("kind", ["unit", "unnormalised", "outlier", "vanishing"])
def test_the_real_score_stays_within_the_bound_of_T(harness, kind, dim, l2):
    rng = np.random.default_rng(2000 * dim + 10 * len(kind) + l2)
    r, c = operands(kind, dim, rng)
    nr, s_a, a_r, b_r = quantise(r, per_row=False)
    nc, s_c, a_c, b_c = quantise(c, per_row=True)
    s_a, a_a, b_a = s_a[0], a_r.max(), b_r.max()
    a_max, b_max = a_c.max(), b_c.max()
    D = nr @ nc.T
    c2 = (c * c).sum(1, dtype=f32)  # the prepared fp32 norm
    r64, c64 = r.astype(np.float64), c.astype(np.float64)
    real = r64 @ c64.T
    if l2:
        real = 2 * real - (c64 * c64).sum(1)[None, :]
    nu = (dim + 3) // 4 * 4 + 18
    gamma, under = f32(1.02 * nu * 2.0 ** -24 / (1 - nu * 2.0 ** -24) * 1.0102), f32(nu * 2.0 ** -149)
    head = " ".join([str(l2), *(float(v).hex() for v in (s_a, a_a, b_a, a_max, b_max, gamma, under))])
    lines = [f"{head} {float(s_c[j]).hex()} {int(D[i, j])} {float(c2[j]).hex()}" for i in range(64) for j in range(64)]
    out = harness("terms", stdin="\n".join(lines) + "\n")
    T = np.array([float.fromhex(v) for v in out[0::4]]).reshape(64, 64)
    bound = np.array([float.fromhex(v) for v in out[1::4]]).reshape(64, 64)
    margin = np.array([float.fromhex(v) for v in out[2::4]]).reshape(64, 64)
    assert np.isfinite(bound).all() and not np.array(list(map(int, out[3::4])), bool).any()
    worst = np.abs(real - T) / bound
    print(f"{kind} dim {dim} l2 {l2}: |real - T| at most {worst.max():.3f} of the bound {bound.max():.3e}")
    assert (np.abs(real - T) <= bound).all()
    assert (margin >= 2 * bound).all()
    if kind == "unit":  # the bound is a bound: a unit row's margin stays far below the spread of its scores
        assert margin.max() < 0.2


def test_a_bound_that_is_not_finite_keeps_nothing(harness):
    ok = ["0x1p-7", "0x1p0", "0x1p-5", "0x1p0", "0x1p-5", "0x1p-16", "0x1p-140"]  # sA aA bA a_max b_max gamma under
    lines = []
    for i in range(1, 5):  # aA, bA, a_max, b_max: infinite, then NaN
        for bad in ("inf", "nan"):
            lines.append(" ".join(["0", *ok[:i], bad, *ok[i + 1:], "0x1p-7", "100", "0x1p0"]))
    lines.append(" ".join(["1", *ok, "0x1p-7", "100", "0x1p0"]))
    out = harness("terms", stdin="\n".join(lines) + "\n")
    assert list(map(int, out[3::4])) == [1] * 8 + [0]
