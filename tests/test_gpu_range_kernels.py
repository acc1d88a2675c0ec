"""The exact range kernels alone (kernels_range.h), launched by tests/kernel_harness/scan_harness.hip: all 11 (lanes per row,
unrolled loads) forms of range_scan_kernel for both metrics, and range_filter_kernel.

The reference scores are those rescore_kernel returns for every row (select_harness.rescore): kernels_range.h promises
bit-equality with them, so the expected output is exact -- the rows whose reference key passes the threshold, as a set, and
their number as count, also when the buffer is smaller.  rescore_kernel itself is held to float64 by
tests/test_gpu_select_kernels.py; here the integer corpus additionally pins the scores to int64 arithmetic, and the float
corpus to float64 within gamma(m) S (scan_harness.range_roundings: ceil(pitch4 / P) fmas + fold 2 + log2 P tree steps, L2 + 2)."""
import numpy as np
import pytest

import scan_harness as S
import select_harness as H

pytestmark = pytest.mark.gpu

FORMS = sorted(S.enumerate_range().items())  # ((P, NI), first pitch4)
METRICS = (S.METRIC_COSINE, S.METRIC_L2)
COVERED = set()


def _reference_keys(metric, rows, q):
    """rescore_kernel's key of every row for one query (0 for a NaN score)."""
    n = rows.shape[0]
    cand = S.make_keys(np.zeros(n, np.uint32), np.arange(n)).reshape(1, n)
    keys, _ = H.rescore(metric, rows, q.reshape(1, -1), cand, np.array([n], np.uint32))
    return keys[0]


def _thresholds(metric, keys, rng):
    """On the rows' own scores, their fp32 neighbours, both zeros, both infinities, NaN; for L2 the largest distance exactly."""
    s = S.ord2f(S.key_ord(keys[keys != 0])).astype(np.float64)
    s = s[np.isfinite(s)]
    thr = H.thresholds_from(-s if metric == S.METRIC_L2 else s, np.zeros(s.size, int), rng, extra=(np.nan,))
    if metric == S.METRIC_L2 and s.size:
        thr.append(np.float32(-s.min()))
    return thr


def _expected(metric, keys, thr, mask, n):
    ok = S.range_passes(keys, thr, metric)
    if mask is not None:
        ok &= S.mask_bits(mask, n)
    return keys[ok]


def _plant(rows):
    n, d = rows.shape
    if n >= 8:
        rows[1] = 0.0
        rows[2, d // 2] = np.nan
        rows[n - 1, d - 1] = np.nan


@pytest.mark.parametrize("form,pitch4", FORMS, ids=[f"P{f[0]}n{f[1]}-p{p}" for f, p in FORMS])
def test_range_scan_of_every_form(form, pitch4):
    P, NI = form
    if NI == 0:
        pitch4 = 259  # past 256, no multiple of 64: the loop's last trip is partial
    assert S.range_form(pitch4) == (P, NI, True) and S.range_form_py(pitch4) == form
    R, U = 64 // P, S.range_passes_py(NI)
    rng = np.random.default_rng(7000 + pitch4)
    # grid_x = 3: groups no multiple of U * 12, at least three trips per wave; all rows kept -> a wave's stage fills to exactly 64
    # (R = 64: one push) or crosses 64 with a remainder (masks, thresholds) and ends with a partial flush
    groups = 3 * U * 12 + U + 1
    n_big = max(groups * R - (R // 2 if R > 1 else 0), 700)
    for corpus in (S.int_corpus, S.float_corpus):
        rows, qs = corpus(rng, n_big, pitch4 * 4, nq=2)
        _plant(rows)
        for metric in METRICS:
            for n in (n_big, 1, max(1, R - 1)):
                sub = np.ascontiguousarray(rows[:n])
                ref = [_reference_keys(metric, sub, q) for q in qs]
                cls = S.row_class(sub)
                for qi, q in enumerate(qs):  # the reference itself: int64 arithmetic, or float64 within the derived band
                    if corpus is S.int_corpus:
                        S.check_dump(np.concatenate([ref[qi], [np.uint64(S.SENT_KEY)]]), n, cls, exact=S.exact_keys(np.nan_to_num(sub), q, metric))
                    else:
                        v, s = S.truth64(sub, q, metric)
                        with np.errstate(invalid="ignore"):
                            S.check_dump(np.concatenate([ref[qi], [np.uint64(S.SENT_KEY)]]), n, cls, value=v,
                                         band=S.gamma(S.range_roundings(P, pitch4, metric)) * s)
                masks = S.special_masks(n, rng)
                thrs = [_thresholds(metric, r, rng) for r in ref]
                for t in range(0, max(len(x) for x in thrs), 1 if n == n_big else 4):  # (the short corpora: every fourth)
                    thr = np.array([x[t % len(x)] for x in thrs], np.float32)
                    mname = (None, "ones", "random", "edge", "zeros")[t % 5]
                    mask = None if mname is None else masks[mname]
                    want = [_expected(metric, ref[qi], thr[qi], mask, n) for qi in range(2)]
                    total = max(w.size for w in want)
                    for cap, grid_x in ((n + 3, 3), (max(total // 2, 1), 1)) if t % 3 == 0 else ((n + 3, 1 + t % 3),):
                        out, guard, count = S.range_scan(metric, sub, qs, thr, cap, mask=mask, grid_x=grid_x)
                        for qi in range(2):
                            S.check_range(out[qi], guard, count[qi], cap, want[qi])
    COVERED.add((P, NI))


@pytest.mark.parametrize("pitch4", [1, 22, 96, 259])
def test_range_filter(pitch4):
    """Candidate counts 0, 1, 63, 64, 65 and more than 64 x the waves of the grid; cand_count > cand_cap is clamped."""
    rng = np.random.default_rng(8000 + pitch4)
    n, cand_cap = 1500, 600
    counts = np.array([0, 1, 63, 64, 65, 300, 600, 100_000], np.uint32)  # grid_x = 1: 4 waves x 64 = 256 < 300
    nq = counts.size
    for corpus in (S.int_corpus, S.float_corpus):
        rows, qs = corpus(rng, n, pitch4 * 4, nq=nq)
        _plant(rows)
        cand_rows = np.stack([rng.permutation(n)[:cand_cap] for _ in range(nq)])  # (distinct rows per query)
        special = np.array([1, 2, n - 1])  # the zero row and the NaN rows among the candidates of the query that reads all 600
        perm = rng.permutation(n)
        cand_rows[6] = np.concatenate([special, perm[~np.isin(perm, special)]])[:cand_cap]
        cand = S.make_keys(rng.integers(0, 1 << 32, cand_rows.shape, dtype=np.uint64).astype(np.uint32), cand_rows)
        for metric in METRICS:
            ref = [_reference_keys(metric, rows, q) for q in qs]
            have = np.minimum(counts, cand_cap)
            mine = [ref[qi][cand_rows[qi, :have[qi]]] for qi in range(nq)]
            thrs = [_thresholds(metric, m if m.size else ref[qi], rng) for qi, m in enumerate(mine)]
            for t in range(0, max(len(x) for x in thrs), 2):
                thr = np.array([x[t % len(x)] for x in thrs], np.float32)
                want = [_expected(metric, mine[qi], thr[qi], None, n) for qi in range(nq)]
                for cap, grid_x in ((cand_cap + 5, 1), (40, 2)) if t % 4 == 0 else ((cand_cap + 5, 3),):
                    out, guard, count = S.range_filter(metric, rows, qs, thr, cand, counts, cap, grid_x=grid_x)
                    for qi in range(nq):
                        S.check_range(out[qi], guard, count[qi], cap, want[qi])


def test_the_harness_refuses_what_would_leave_the_arrays():
    rng = np.random.default_rng(9)
    rows, q = S.int_corpus(rng, 100, 16)
    thr = np.zeros(1, np.float32)
    with pytest.raises(ValueError):
        S.range_scan(0, rows, q, thr, 10, mask=np.zeros(3, np.uint32))
    with pytest.raises(ValueError):
        S.range_scan(0, rows[:0].reshape(0, 16), q, thr, 10)
    cand = S.make_keys(np.zeros(4, np.uint32), np.array([0, 1, 100, 2])).reshape(1, 4)
    with pytest.raises(ValueError):
        S.range_filter(0, rows, q, thr, cand, np.array([3], np.uint32), 10)  # the third candidate names row 100 of 100
    S.range_filter(0, rows, q, thr, cand, np.array([2], np.uint32), 10)      # (not read: fine)


def test_zz_every_range_form_was_covered():
    """Runs last and needs the range scan cases to have run before it: a form that was not launched fails this test."""
    want = {S.range_form(p)[:2] for p in range(1, 1001)}
    assert len(want) == 11 and want == set(S.enumerate_range())
    assert COVERED == want, ("range forms not launched in this session", sorted(COVERED ^ want))
    print("\nrange forms covered (lanes per row x unrolled loads), both metrics each: " + " ".join(f"{P}x{NI}" for P, NI in sorted(COVERED))
          + " == the picker's set of 11")
