"""The device-free plumbing the blocking entry points share (wdbx-py_amd/csrc/host_calls.h): the allowed rows of a host
mask, the padded copy of a call's queries, the host ranking of a lone query's keys and the class-by-class fallback loop --
driven by tests/host_harness/calls_harness.cpp, built once plain and once under -fsanitize=address,undefined, and checked
against numpy.  Each binary runs as a child process; nothing is loaded into this interpreter."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HARNESS = ROOT / "tests" / "host_harness" / "calls_harness.cpp"
INC = ROOT / "wdbx-py_amd" / "csrc"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path_factory.mktemp("calls_" + request.param) / "calls_harness"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                      "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{INC}", str(HARNESS), "-o", str(exe)], check=True)

    def run(mode, cases):
        """cases: lists of non-negative integers, one per line -> the output lines, split into words"""
        text = "".join(" ".join(str(int(v)) for v in case) + "\n" for case in cases)
        p = subprocess.run([str(exe), mode], input=text, capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])
        return [ln.split() for ln in p.stdout.split("\n") if ln]
    return run


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).ravel().tolist()


# ---- mask_allowed_rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [0, 1, 31, 32, 33, 64, 1000])
def test_mask_allowed_rows(harness, n_rows):
    rng = np.random.default_rng(n_rows)
    n_words = (n_rows + 31) // 32
    rows = np.arange(n_words * 32)
    random = rng.integers(0, 1 << 32, n_words, dtype=np.uint64).astype(np.uint32)
    ones = np.full(n_words, 0xFFFFFFFF, np.uint32)
    # bits past the last row set, the rows themselves random: only the rows count
    beyond = random.copy()
    for r in rows[n_rows:]:
        beyond[r // 32] |= np.uint32(1 << (r % 32))
    masks = [random, ones, beyond]
    got = harness("mask", [[n_rows, n_words, *m.tolist()] for m in masks])
    for m, line in zip(masks, got):
        bit = (m[rows // 32] >> (rows % 32).astype(np.uint32)) & 1 if n_words else np.zeros(0, np.uint32)
        assert int(line[0]) == int(bit[:n_rows].sum()), (n_rows, m)
    assert int(got[1][0]) == n_rows
    assert len(got) == 3


# ---- pad_queries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("dim,pitch", [(1, 4), (54, 56), (16, 16)])
def test_pad_queries(harness, dim, pitch, nq):
    rng = np.random.default_rng(dim * 10 + nq)
    # arbitrary bit patterns (NaNs and denormals included): the payload is copied, never computed with
    src = rng.integers(0, 1 << 32, (nq + 2, dim), dtype=np.uint64).astype(np.uint32)
    index = rng.integers(0, nq + 2, nq)
    index[-1] = index[0]  # (a repeated entry)
    cases = [[dim, pitch, nq, nq, 0, *src[:nq].ravel().tolist()],
             [dim, pitch, nq, nq + 2, nq, *index.tolist(), *src.ravel().tolist()]]
    got = harness("pad", cases)
    for line, picked in zip(got, [src[:nq], src[index]]):
        out = np.array([int(w) for w in line], np.uint32).reshape(nq, pitch)
        assert np.array_equal(out[:, :dim], picked)   # bit-equal payload
        assert not out[:, dim:].any()                 # the padding is exactly +0.0


# ---- rank_keys_host ---------------------------------------------------------------------------------------------------
def _make_key(score, row):
    """make_key of kernels_common.h: (orderable(score) << 32) | ~row"""
    u = int(np.float32(score).view(np.uint32))
    o = u ^ (0xFFFFFFFF if u >> 31 else 0x80000000)
    return (o << 32) | (~row & 0xFFFFFFFF)


def _rank_reference(scores, rows, nan_at, k, l2):
    """(score descending, row ascending) -- +0.0 above -0.0, as the keys order them -- without the NaN entries; L2 keys hold
    negated distances and come out as -s + 0.0"""
    live = [(float(s), bool(np.signbit(s)), int(r)) for i, (s, r) in enumerate(zip(scores, rows)) if i not in nan_at]
    live.sort(key=lambda t: (-t[0], t[1], t[2]))
    idx = [t[2] for t in live[:k]]
    sc = [np.float32(scores[list(rows).index(r)]) for r in idx]
    if l2:
        sc = [np.float32(-s) + np.float32(0.0) for s in sc]
    pad = k - len(idx)
    return idx + [-1] * pad, _bits(np.array(sc + [0.0] * pad, np.float32))


@pytest.mark.parametrize("l2", [0, 1])
def test_rank_keys_host(harness, l2):
    rng = np.random.default_rng(5 + l2)
    k = 6
    cases, want = [], []
    for cnt in (0, 3, 6, 40):  # below k, equal to k, above k, and none
        # ties (few distinct values), negative values, both zeros
        scores = rng.choice(np.array([-3.5, -1.0, -0.0, 0.0, 0.25, 0.25, 2.0, 7.0], np.float32), cnt)
        rows = rng.permutation(5000)[:cnt]
        nan_at = set(range(1, cnt, 7))  # (a NaN score reaches the host as a zero key)
        keys = [0 if i in nan_at else _make_key(scores[i], int(rows[i])) for i in range(cnt)]
        cases.append([cnt, k, l2, *keys])
        want.append(_rank_reference(scores, rows, nan_at, k, l2))
    got = harness("rank", cases)
    assert len(got) == len(cases)
    for line, (idx, bits), case in zip(got, want, cases):
        assert [int(w) - 1 for w in line[0::2]] == idx, case[:3]
        assert [int(w) for w in line[1::2]] == bits, case[:3]
        if l2:
            assert 0x80000000 not in [int(w) for w in line[1::2]]  # no -0.0 comes out


def test_rank_keys_host_orders_a_tie_by_row_and_drops_the_zero_key(harness):
    keys = [_make_key(1.0, 9), _make_key(1.0, 4), 0, _make_key(-2.0, 0), _make_key(1.0, 7)]
    (line,) = harness("rank", [[len(keys), 5, 0, *keys]])
    assert [int(w) - 1 for w in line[0::2]] == [4, 7, 9, 0, -1]
    assert [int(w) for w in line[1::2]] == _bits([1.0, 1.0, 1.0, -2.0, 0.0])


# ---- for_each_class ---------------------------------------------------------------------------------------------------
NQ, DIM, K = 7, 3, 2
CLASS_OF = [-1, 0, 2, 0, -1, 2, 2]
CLASSES = [-1, 0, 1, 2]  # (class 1 has no members)
QUERIES = np.arange(NQ * DIM, dtype=np.float32).reshape(NQ, DIM) + np.float32(0.5) * (np.arange(DIM) == 1)


def _classes_run(harness, fail_class, fail_code):
    case = [NQ, DIM, K, fail_class + 1, fail_code, len(CLASSES), *[c + 1 for c in CLASSES], *[c + 1 for c in CLASS_OF], *_bits(QUERIES)]
    lines = harness("classes", [case])
    calls = [ln for ln in lines if ln[0] == "call"]
    (rc,) = [int(ln[1]) for ln in lines if ln[0] == "rc"]
    outs = [ln[1:] for ln in lines if ln[0] == "out"]
    idx = np.array([[int(w) - 7 for w in o[0::2]] for o in outs])
    score = np.array([[int(w) for w in o[1::2]] for o in outs], np.uint32).view(np.float32)
    return calls, rc, idx, score


def _expected_rows(c, members):
    idx = np.array([[int(1000 * QUERIES[q, 0]) + 10 * (c + 1) + j for j in range(K)] for q in members])
    score = np.array([[QUERIES[q, 1] + np.float32(j) + np.float32(0.5 * c) for j in range(K)] for q in members], np.float32)
    return idx, score


def test_for_each_class_gathers_calls_and_scatters(harness):
    calls, rc, idx, score = _classes_run(harness, fail_class=-5, fail_code=0)
    assert rc == 0
    assert [int(c[1]) - 1 for c in calls] == [-1, 0, 2]  # each class with members once, in the order of the list; class 1 skipped
    for c in calls:
        cls = int(c[1]) - 1
        members = [q for q in range(NQ) if CLASS_OF[q] == cls]  # the caller's order
        assert int(c[2]) == len(members)
        assert [int(w) for w in c[3:]] == _bits(QUERIES[members])
        want_idx, want_score = _expected_rows(cls, members)
        assert np.array_equal(idx[members], want_idx) and np.array_equal(score[members], want_score)


def test_for_each_class_stops_at_the_first_failure(harness):
    calls, rc, idx, score = _classes_run(harness, fail_class=0, fail_code=5)
    assert rc == 5
    assert [int(c[1]) - 1 for c in calls] == [-1, 0]  # class 2 was never called
    done = [q for q in range(NQ) if CLASS_OF[q] == -1]
    want_idx, want_score = _expected_rows(-1, done)
    assert np.array_equal(idx[done], want_idx) and np.array_equal(score[done], want_score)
    rest = [q for q in range(NQ) if CLASS_OF[q] != -1]
    assert (idx[rest] == -7).all() and (score[rest] == -7.0).all()  # nothing written for the failed and the later classes
