"""How a round's queries are split between the matrix-core groups of 16 and the VALU groups, which needs no GPU:
u42_mfma_groups next to u42_share_groups (wdbx-py_amd/csrc/host_selection.h), driven by
tests/host_harness/u42_mfma_groups_harness.cpp -- built once plain and once under -fsanitize=address,undefined; nothing is
preloaded."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "host_harness" / "u42_mfma_groups_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"

MIN_SHORTS = (1, 6, 8, 16, 17)  # 17: no remainder ever goes as a short group
CASES = [(nv, r, qp) for r in MIN_SHORTS for qp in (1, 2, 4) for nv in range(1, 65)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plans(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("u42_mfma_" + request.param) / "u42_mfma_groups_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)
    text = "".join(f"{nv} {r} {qp}\n" for nv, r, qp in CASES)
    p = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    lines = [list(map(int, ln.split())) for ln in p.stdout.split("\n") if ln]
    assert len(lines) == len(CASES)
    out = {}
    for case, ln in zip(CASES, lines):
        assert len(ln) == 3 + 2 * ln[2], case
        out[case] = (ln[0], ln[1], list(zip(ln[3::2], ln[4::2])))  # mfma groups, queries they take, (first, width) per VALU group
    return out


def test_every_query_is_in_exactly_one_group(plans):
    for (nv, r, qp), (ngm, covered, valu) in plans.items():
        seen = []
        for g in range(ngm):
            seen += list(range(16 * g, min(16 * g + 16, covered)))
        for first, width in valu:
            seen += list(range(first, first + width))
        assert seen == list(range(nv)), (nv, r, qp)


def test_full_groups_and_the_short_group(plans):
    for (nv, r, qp), (ngm, covered, valu) in plans.items():
        full, rest = divmod(nv, 16)
        short = rest >= r and rest > 0
        assert ngm == full + (1 if short else 0), (nv, r, qp)
        assert covered == (nv if short else 16 * full), (nv, r, qp)


def test_no_valu_group_where_a_matrix_group_was_due(plans):
    for (nv, r, qp), (ngm, covered, valu) in plans.items():
        left = sum(w for _, w in valu)
        assert left < 16 and left < max(r, 1), (nv, r, qp)   # fewer than a full group, fewer than a short group takes
        assert all(first >= 16 * (nv // 16) for first, _ in valu), (nv, r, qp)
        assert all(w in (1, 2, 4) and w <= qp for _, w in valu), (nv, r, qp)


def test_named_rounds(plans):
    assert plans[(64, 6, 4)] == (4, 64, [])
    assert plans[(49, 6, 4)] == (3, 48, [(48, 1)])
    assert plans[(5, 6, 4)] == (0, 0, [(0, 4), (4, 1)])
    assert plans[(8, 6, 4)] == (1, 8, [])
    assert plans[(37, 6, 4)] == (2, 32, [(32, 4), (36, 1)])
    assert plans[(38, 6, 4)] == (3, 38, [])
    assert plans[(16, 17, 4)] == (1, 16, [])
    assert plans[(31, 17, 2)][:2] == (1, 16)
