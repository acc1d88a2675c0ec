"""How a round's queries are grouped for the shared read of the four-bit plane, which needs no GPU: u42_share_groups
(wdbx-py_amd/csrc/host_selection.h), driven by tests/host_harness/u42_share_groups_harness.cpp -- built once plain and once
under -fsanitize=address,undefined; nothing is preloaded."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "host_harness" / "u42_share_groups_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"

CASES = [(nv, qp) for qp in (1, 2, 4) for nv in range(1, 65)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def groups(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("u42_share_" + request.param) / "u42_share_groups_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)
    text = "".join(f"{nv} {qp}\n" for nv, qp in CASES)
    p = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [list(map(int, ln.split())) for ln in p.stdout.split("\n") if ln]
    assert len(lines) == len(CASES)
    out = {}
    for case, ln in zip(CASES, lines):
        assert len(ln) == 1 + 2 * ln[0], case
        out[case] = list(zip(ln[1::2], ln[2::2]))  # (first, width) per group
    return out


def test_groups_partition_the_round_in_order(groups):
    for (nv, qp), g in groups.items():
        at = 0
        for first, width in g:
            assert first == at and width >= 1, (nv, qp, g)
            at += width
        assert at == nv, (nv, qp, g)


def test_no_group_is_wider_than_qp_and_at_most_two_are_narrower(groups):
    for (nv, qp), g in groups.items():
        widths = [w for _, w in g]
        assert all(w in (1, 2, 4) and w <= qp for w in widths), (nv, qp, g)  # (widths the kernel has instances for)
        assert sum(w < qp for w in widths) <= 2, (nv, qp, g)
        assert widths == sorted(widths, reverse=True), (nv, qp, g)  # the full groups come first
        assert len(g) == nv // qp + bin(nv % qp).count("1"), (nv, qp, g)


def test_named_rounds(groups):
    assert groups[(5, 4)] == [(0, 4), (4, 1)]
    assert groups[(7, 4)] == [(0, 4), (4, 2), (6, 1)]
    assert groups[(3, 2)] == [(0, 2), (2, 1)]
    assert groups[(1, 4)] == [(0, 1)] and groups[(1, 2)] == [(0, 1)]
    assert groups[(64, 2)] == [(2 * i, 2) for i in range(32)]
    assert groups[(64, 1)] == [(i, 1) for i in range(64)]
