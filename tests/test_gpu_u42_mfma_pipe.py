"""The matrix-core pass's lists, refine and stage at their edges (scan_u42_mfma_kernel, kernels_scan42.h): a list of
U42_MFMA_LIST_CAP entries takes up to 64 per tile and its last 64 are refined once it holds U42_MFMA_TRIGGER, one stage holds
the kept keys of all sixteen columns and a flush serves every column with one atomic instruction.

Two kinds of inputs, planes from rows_to_u42_kernel:
  random     unit rows and queries with a finite threshold far below every w4 + m4: every row survives every column and is a
             candidate, whatever the roundings
  ladder     rows alpha_r * g for one unit direction g, alpha_r from the levels 1, 1/4, 1/16, 1/64 and -1; column j asks
             (1 + j / 16) g (the columns' keys of one row differ) at a threshold half way down to the next level: the
             restatement's w + m is far from tau on both sides in both stages (asserted), so the survivor and candidate sets are
             the restatement's exactly.
Expected sets come from tests/u42_mfma_model.py; the wave of a tile is tile % (4 grid_x) % 4 (tile = blockIdx.x * 4 + wave, stride
4 grid_x)."""
import re
from pathlib import Path

import numpy as np
import pytest

import select_harness as S
import u42_harness as U
import u42_mfma_harness as MH
import u42_mfma_model as M
import u42_share_harness as H

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
LOW = F32(-1e3)  # a finite threshold far below every w4 + m4 of unit rows and queries
LEVELS = (1.0, 0.25, 0.0625, 0.015625, -1.0)
_SRC = (Path(__file__).resolve().parent.parent / "wdbx-py_amd" / "csrc" / "kernels_scan42.h").read_text()
TRIGGER = int(re.search(r"U42_MFMA_TRIGGER = (\d+);", _SRC).group(1))
LIST_CAP = int(re.search(r"U42_MFMA_LIST_CAP = (\d+);", _SRC).group(1))
_CACHE = {}


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(F32)


def _read(planes, n, d):
    l, a6 = U.unpack_l(planes["lrec"], d // 32)
    return dict(planes=planes, h=U.unpack_h(planes["h"], n), l=l, a6=a6.view(F32), s=planes["sa4"][:, 0], a4=planes["sa4"][:, 1])


def _random(n, d):
    if ("random", n, d) not in _CACHE:
        rng = np.random.default_rng(9100 + n + d)
        rows = _unit(rng.random((n, d)) * 2 - 1)
        c = _read(H.quantise(rows, d), n, d)
        c.update(rows=rows, queries=_unit(rng.standard_normal((16, d))))
        _CACHE[("random", n, d)] = c
    return _CACHE[("random", n, d)]


def _ladder(level, d=384):
    """level [n] ints into LEVELS -> the case; shared per level pattern"""
    key = ("ladder", level.tobytes(), d)
    if key not in _CACHE:
        g = _unit(np.random.default_rng(77).standard_normal((1, d)))[0]
        rows = (np.array(LEVELS, F32)[level][:, None] * g[None, :]).astype(F32)
        c = _read(H.quantise(rows, d), level.size, d)
        c.update(rows=rows, g=g)
        _CACHE[key] = c
    return _CACHE[key]


def _ladder_queries(c, kinds):
    """kinds[j] = number of levels column j keeps (0: none, 1 .. 4: down to that level, 5: every row) -> queries, tau"""
    f = np.array([1 + j / 16 for j in range(len(kinds))], F32)
    queries = (f[:, None] * c["g"][None, :]).astype(F32)
    cut = {0: 2.0, 1: 0.5, 2: 0.125, 3: 0.03125, 4: 0.0, 5: -10.0}
    tau = np.array([cut[k] * float(f[j]) for j, k in enumerate(kinds)], F32)
    return queries, tau


def _model(c, r, slot, q, tau, decisive):
    """-> (p4 bits [n], survivors [n] bool, kept [n] bool, w6 float64 [n]) of one column from the restatement, with the
    constants the device computed"""
    kc = {name: r["qc"][name][slot] for name in MH.QC_FIELDS}
    qq = M.quantise_query(q)
    assert not qq["marked"] and kc["dp"] == qq["delta"] * F32(2.0 ** -9)
    p4, p_int = M.p_bits(c["h"], qq["Q"], kc["dp"])
    w4, m4 = M.first_stage(p4, c["s"], c["a4"], kc)
    w6, m6 = M.refine(p4, c["l"], c["s"], c["a6"], q, kc)
    b4, b6 = (w4 + m4).astype(F64), (w6 + m6).astype(F64)
    if decisive:  # far from tau on both sides, in both stages: no rounding of the restatement decides a row
        slack = 0.05 * max(abs(float(tau)), 0.01)
        assert np.all(np.abs(b4 - float(tau)) > slack) and np.all(np.abs(b6 - float(tau)) > slack)
    surv = ~(b4 < float(tau))
    kept = surv & ~(b6 < float(tau))
    s64, q64 = c["s"].astype(F64), q.astype(F64)
    w6_64 = s64 * (4.0 * F64(qq["delta"]) * p_int + c["l"].astype(F64) @ q64 - 32.0 * q64.sum())
    return p4.view(np.uint32), surv, kept, w6_64


def _check_column(c, r, slot, q, tau, cap, n, decisive=True):
    """counters, entries and keys of one column against the restatement; -> (survivors, candidates)"""
    bits, surv, kept, w6_64 = _model(c, r, slot, q, tau, decisive)
    got = r["surv_p"][slot] != S.SENT_U32
    assert np.array_equal(got, surv), "the survivor set"
    assert np.array_equal(r["surv_p"][slot][got], bits[got]), "2^-9 P^ of the entries, bit for bit"
    assert int(r["survivors"][slot]) == int(surv.sum())
    count = int(r["count"][slot])
    assert count == int(kept.sum())
    held = min(count, cap)
    keys = r["cand"][slot, :held]
    assert (keys != S.SENT_KEY).all() and (r["cand"][slot, held:] == S.SENT_KEY).all()
    rows = S.key_row(keys).astype(np.int64)
    assert rows.size == np.unique(rows).size and (rows.size == 0 or rows.max() < n) and kept[rows].all()
    if count <= cap:
        assert np.array_equal(np.sort(rows), np.flatnonzero(kept)), "the candidate set"
    # the keys are this column's: w6 of this query (the columns' queries differ by 1 / 31 and more)
    w = S.ord2f(S.key_ord(keys)).astype(F64)
    d = q.shape[0]
    rnd = 6e-6 * (d + 8) * c["s"].astype(F64) * np.abs(q.astype(F64)).sum()
    assert np.all(np.abs(w - w6_64[rows]) <= rnd[rows] * (1 + S.M_SLACK) + 1e-45)
    return int(surv.sum()), count


def _wave_of(tile, grid_x):
    return tile % (4 * grid_x) % 4, tile % (4 * grid_x) // 4


def _list_walk(surv, n, grid_x):
    """the fill of a (wave, column) list in front of and behind every tile's append, refines of the last TRIGGER entries behind a
    tile as the kernel does them: -> [(fill before, appended, fill after the append)] over all waves"""
    out, fill = [], {}
    for tile in range((n + 63) // 64):
        w = _wave_of(tile, grid_x)
        add = int(surv[tile * 64:(tile + 1) * 64].sum())
        f = fill.get(w, 0)
        assert f < TRIGGER and f + add <= LIST_CAP - 1
        out.append((f, add, f + add))
        fill[w] = f + add - TRIGGER if f + add >= TRIGGER else f + add
    return out


N_ALL = 4 * 64 * 5 + 37


@pytest.mark.parametrize("grid_x", [1, 3])
def test_every_row_survives_every_column(grid_x):
    """every (wave, column) list takes 64 entries per tile: it crosses the trigger and sits at capacity behind every tile"""
    n, d = N_ALL, 384
    c = _random(n, d)
    tau = np.full(16, LOW, F32)
    r = MH.scan(c["planes"], c["queries"], n, tau, n, grid_x)
    assert (r["guard"] == S.SENT_KEY).all()
    for j in range(16):
        assert _check_column(c, r, j, c["queries"][j], tau[j], n, n, decisive=False) == (n, n)
    walk = _list_walk(np.ones(n, bool), n, grid_x)
    assert sum(after >= TRIGGER for _, _, after in walk) >= n // 64  # (every whole tile, if a tile's 64 reach the trigger)


def _boundary_levels():
    n = 64 * 12
    level = np.full(n, 4)                      # alpha = -1
    tile = lambda t: slice(64 * t, 64 * t + 64)
    level[tile(0)] = 0                         # wave 0: 63 rows at level 1 and one at 1/4, then 64 at level 1, then one
    level[64 * 0 + 63] = 1
    level[tile(4)] = 0
    level[64 * 8] = 0
    level[64 * 1:64 * 1 + TRIGGER // 2] = 0    # wave 1: half a trigger twice: the list reaches T from below in one append of T / 2
    level[64 * 5:64 * 5 + TRIGGER // 2] = 0
    return level


def test_the_boundary_of_the_trigger():
    n, grid_x = 64 * 12, 1
    c = _ladder(_boundary_levels())
    kinds = [1, 2, 0, 5] + [1, 2] * 6
    queries, tau = _ladder_queries(c, kinds)
    r = MH.scan(c["planes"], queries, n, tau, n, grid_x)
    assert (r["guard"] == S.SENT_KEY).all()
    walks = []
    for j in range(16):
        _check_column(c, r, j, queries[j], tau[j], n, n)
        walks.append(_list_walk(r["surv_p"][j] != S.SENT_U32, n, grid_x))
    # column 0 (level 1 only): a list of T - 1 entries takes a tile's 64; column 1 (levels 1 and 1/4): an append ends at exactly T;
    # and a list left at exactly T - 1 behind an append is not refined in the loop
    assert any(f == TRIGGER - 1 and add == 64 for f, add, _ in walks[0])
    assert any(after == TRIGGER for _, _, after in walks[1]) and any(after == TRIGGER and f > 0 for f, _, after in walks[0])
    assert any(after == TRIGGER - 1 for _, _, after in walks[0])


def _mixed_levels():
    n = 4 * 64 * 2 + 5
    level = np.full(n, 3)                      # alpha = 1 / 64: kept by the columns that keep every level
    for t in (0, 2):                           # tiles of waves 0 and 2 (grid_x = 1)
        level[64 * t] = 0                      # one row at level 1
        level[64 * t + 1:64 * t + 63] = 1      # 63 down to level 1 / 4
        level[64 * t + 63] = 2                 # 64 down to level 1 / 16
    return level


MIXED_KINDS = [0, 1, 2, 3, 5, 4, 3, 2, 1, 0, 5, 2, 3]  # per tile of waves 0 and 2: 0, 1, 63, 64 rows, or all rows of every wave


@pytest.mark.parametrize("grid_x", [1, 2])
def test_columns_of_very_different_counts_in_one_flush(grid_x):
    """nq = 13: three absent columns; the stage holds keys of columns with 0, 1, 63, 64 and all rows of the same waves"""
    c = _ladder(_mixed_levels())
    n = c["rows"].shape[0]
    queries, tau = _ladder_queries(c, MIXED_KINDS)
    r = MH.scan(c["planes"], queries, n, tau, n, grid_x)
    assert (r["guard"] == S.SENT_KEY).all()
    got = [_check_column(c, r, j, queries[j], tau[j], n, n) for j in range(len(MIXED_KINDS))]
    want = {0: 0, 1: 2, 2: 126, 3: 128, 4: n, 5: n}
    assert [g[1] for g in got] == [want[k] for k in MIXED_KINDS]
    assert (r["qc"]["flags"][len(MIXED_KINDS):16] == MH.ABSENT).all()


@pytest.mark.parametrize("mixed", [False, True])
def test_a_small_capacity(mixed):
    """cap = 5: the counters end at the restatement's counts, above cap; the first cap keys of each buffer are distinct surviving
    rows of that column; nothing behind them, the neighbours' buffers and the guard included, is written"""
    cap = 5
    if mixed:
        c = _ladder(_mixed_levels())
        queries, tau = _ladder_queries(c, MIXED_KINDS)
    else:
        c = _random(N_ALL, 384)
        queries, tau = c["queries"], np.full(16, LOW, F32)
    n = c["rows"].shape[0]
    r = MH.scan(c["planes"], queries, n, tau, cap, 2)
    assert (r["guard"] == S.SENT_KEY).all()
    for j in range(queries.shape[0]):
        s, k = _check_column(c, r, j, queries[j], tau[j], cap, n, decisive=mixed)
        if not mixed:
            assert s == k == n
    assert (r["count"] > cap).sum() >= (8 if mixed else 16)


@pytest.mark.parametrize("units", [9, 10, 11])
def test_a_short_last_chunk_and_a_ragged_end(units):
    n, d = 4 * 64 + 1, units * 32
    c = _random(n, d)
    tau = np.full(16, LOW, F32)
    tau[5] = np.inf
    r = MH.scan(c["planes"], c["queries"], n, tau, n, 1)
    assert (r["guard"] == S.SENT_KEY).all()
    for j in range(16):
        assert _check_column(c, r, j, c["queries"][j], tau[j], n, n, decisive=False) == ((0, 0) if j == 5 else (n, n))
