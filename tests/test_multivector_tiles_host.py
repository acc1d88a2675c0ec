"""The matrix-core scoring route of the multi-vector search, the parts that need no GPU: the device-free plan
(wdbx-py_amd/csrc/host_multivector_tiles.h) driven by tests/host_harness/multivector_tiles_harness.cpp -- built once plain and
once under -fsanitize=address,undefined -- and the premise of its certainty margin in numpy: two fp32 summation orders of one
dot product both lie within gamma |r| |c| + under of the float64 value (DESIGN.md sections 4.20 and 4.12b)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
INC = ROOT / "wdbx-py_amd" / "csrc"
HARNESS = ROOT / "tests" / "host_harness" / "multivector_tiles_harness.cpp"
NAMES = ("eligible", "vt", "block", "vblocks", "ni", "lds", "grid", "covered")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("mvt_" + request.param) / "multivector_tiles_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)
        assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
        return list(map(int, p.stdout.split()))
    return run


def test_blocks_cover_the_round_and_lds_does_not_depend_on_the_row_length(harness):
    block_max, lds_limit, span, waves = harness("limits")
    assert (block_max, span, waves) == (128, 64, 4) and lds_limit <= 160 * 1024
    for vectors in range(1, 257):
        p = dict(zip(NAMES, harness("plan", 0, vectors, 384, 100_000, 256)))
        assert p["vt"] == (1 if vectors <= 32 else 2 if vectors <= 64 else 4) and p["block"] == 32 * p["vt"] <= block_max
        assert p["vblocks"] == -(-vectors // p["block"]) and p["covered"] == 1 and p["eligible"] == 1
        assert p["grid"] == 256 // p["vblocks"]  # one resident workgroup per CU over all vector blocks together
    for dim in (4, 5, 36, 100, 384, 512, 516, 1024, 1028, 4096):
        pitch = (dim + 3) // 4 * 4
        for vectors in (1, 33, 128, 256):
            p = dict(zip(NAMES, harness("plan", 0, vectors, pitch, 7, 256)))
            assert p["eligible"] == 1 and p["lds"] == 2 * (waves * span + p["block"]) * 36 * 4 <= lds_limit
            assert p["ni"] == (2 if pitch <= 512 else 4 if pitch <= 1024 else 0) and p["grid"] == 2  # (7 spans: two workgroups)


def test_l2_is_refused_and_the_option_routes(harness):
    assert dict(zip(NAMES, harness("plan", 1, 32, 384, 1000, 256)))["eligible"] == 0
    #            option, min_vectors, metric, vectors, pitch
    assert harness("route", 1, 16, 1, 200, 384) == [0] and harness("route", -1, 16, 1, 200, 384) == [0]  # L2: never
    assert harness("route", 0, 1, 0, 200, 384) == [0]
    assert harness("route", 1, 256, 0, 1, 384) == [1]
    assert harness("route", -1, 16, 0, 15, 384) == [0] and harness("route", -1, 16, 0, 16, 384) == [1]


def _chain(prod_terms):
    """fp32 fma chain from 0 over the last axis: s = fl32(a b + s), a b exact in float64"""
    s = np.zeros(prod_terms.shape[:-1], np.float32)
    for t in range(prod_terms.shape[-1]):
        s = (prod_terms[..., t] + s.astype(np.float64)).astype(np.float32)
    return s


def test_two_fp32_orders_of_a_dot_product_stay_within_the_bound():
    rng = np.random.default_rng(412)
    dim, pitch = 770, 772
    mag = np.ldexp(1.0, rng.integers(-20, 21, size=(64, dim)))
    r = (rng.standard_normal((64, dim)) * mag).astype(np.float32)
    c = (rng.standard_normal((64, dim)) * np.ldexp(1.0, rng.integers(-20, 21, size=(64, dim)))).astype(np.float32)
    c[:, 1::2] = c[:, 0::2]           # neighbouring terms cancel: r[2i] c[2i] + r[2i + 1] c[2i + 1] is a rounding residue ...
    r[:, 1::2] = -r[:, 0::2] * (1 + np.ldexp(rng.integers(-3, 4, size=(64, dim // 2)), -23)).astype(np.float32)
    r[:8] = np.ldexp(r[:8], -120)     # ... and some pairs down in the denormal range
    c[:8] = np.ldexp(c[:8], -20)
    rp, cp = (np.pad(x, ((0, 0), (0, pitch - dim))) for x in (r, c))
    prod = rp.astype(np.float64) * cp.astype(np.float64)
    exact = prod.sum(axis=1)
    tile = _chain(prod)  # the matrix cores' order: one chain along K
    # exact_score's order: lane j takes quads j, j + 64, ... element by element, (x + y) + (z + w), then the tree 32 .. 1
    quads = np.pad(prod, ((0, 0), (0, 64 * 4 * 4 - pitch))).reshape(64, 4, 64, 4)  # [pair, trip, lane, element]
    acc = _chain(np.moveaxis(quads, 1, -1))                                         # [pair, lane, element]
    s = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, np.arange(64) ^ o]
    nu = (pitch + 18) * 2.0 ** -24
    bound = nu / (1 - nu) * np.linalg.norm(rp.astype(np.float64), axis=1) * np.linalg.norm(cp.astype(np.float64), axis=1) \
        + (pitch + 18) * 2.0 ** -149
    assert (np.abs(tile - exact) <= bound).all() and (np.abs(s[:, 0] - exact) <= bound).all()
    assert (tile != s[:, 0]).any()  # (the two orders do differ: the margin is not idle)
