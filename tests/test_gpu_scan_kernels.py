"""The fp32 scan kernels alone (kernels_scan.h), launched by tests/kernel_harness/scan_harness.hip with the instances the
library's own pickers return: every specialised form scan_form can answer (52, plus the 25 exact fits forced onto their
ragged instance), the five generic widths and the listed repair kernel.

Two corpora per shape.  INTEGER: small integers in [-4, 4] as fp32 -- every partial sum of either metric stays below 2^24 up
to 3200 elements, so any summation order gives the same fp32 value and every key must EQUAL the int64 reference; such corpora
are full of ties, so the key order on equal scores is tested everywhere.  FLOAT: normal values against float64 inside
gamma(m) S, m = the longest chain of roundings of the instance (scan_harness.scan_roundings: QPL fmas + fold 2 + log2 L tree
steps; generic: ceil(ceil(pitch4 / L) / 2) fmas + fold 3 + tree; L2 + 2 for the squared difference), S = sum |c_i q_i| or
sum (c_i - q_i)^2.  No measured slack is added."""
import numpy as np
import pytest

import scan_harness as S

pytestmark = pytest.mark.gpu

CASES = S.scan_cases()
METRICS = (S.METRIC_COSINE, S.METRIC_L2)


def _rows_for(L, qpl, grid_x=3):
    """A row count that is no multiple of the rows per pass, whose group count is no multiple of U * 4 * grid_x, with at least
    three trips per wave."""
    R, U = 64 // L, S.passes_in_flight_py(qpl)
    groups = 3 * U * 4 * grid_x + U + 1
    return groups * R - (R // 2 if R > 1 else 0)


def _specials(rows, q, ragged_tail):
    """Plants the edge rows: row 1 zero, row 5 the query itself, row 2 holds +inf in its first element, row 3 holds +inf in its LAST quad (the quad a
    ragged instance's idle slots re-read), row 4 a NaN, and the last row a NaN (the tail lanes of the last group re-read it)."""
    n, d = rows.shape
    if n < 8:
        return
    q[0], q[d - 1] = 1.0, 1.0
    rows[1] = 0.0
    rows[2, 0] = np.inf
    rows[3, d - 1] = np.inf
    rows[4, d // 2] = np.nan
    rows[n - 1, d - 2] = np.nan
    rows[5] = q  # (L2: distance 0, whose negation must come out as +0)


def _band(rows, q, metric, form, pitch4):
    L, qpl, _, gen = form
    v, s = S.truth64(rows, q, metric)
    with np.errstate(invalid="ignore"):
        return v, S.gamma(S.scan_roundings(L, qpl, pitch4, gen, metric)) * s


COVERED = set()  # (L, QPL, ragged, generic, forced) of every dump case that ran in this session
LISTED_COVERED = set()  # lanes per row of every scan_kernel_listed instance that was launched in this session


def test_the_library_picks_the_forms_the_tests_parametrise_over():
    met = set()
    for p in range(1, 1001):
        for lanes in S.LANES:
            for fr in (0, 1):
                L, Q, ragged, gen, has = S.scan_form(p, lanes, 0, fr)
                assert (L, Q, ragged, gen) == S.scan_form_py(p, lanes, 0, fr) and has, (p, lanes, fr)
                met.add((L, Q, ragged, gen))
            assert S.scan_form(p, lanes, 1, 0)[:4] == S.scan_form_py(p, lanes, 1, 0)
        assert S.listed_lanes(p) == S.generic_lanes_py(p)
    assert met == {c[5] for c in CASES}
    assert len(CASES) == 82
    assert S.plan(2100, 64, 300, 0, 0, 777 * 16, 256, 2, 0, 0, 1) == S.plan_py(2100, 64, 300, 0, 0, 777 * 16, 256, 2, 0, 0, 1)
    print(f"\nscan forms the picker can return: {len(met)} = 52 specialised (27 ragged) + 5 generic; all have instances; "
          f"25 exact fits also run force-ragged; listed lanes {sorted({S.listed_lanes(p) for p in range(1, 1001)})}")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_dump_mode_of_every_form(case):
    _, pitch4, lanes, generic, fr, form = case
    L, qpl, ragged, gen = form
    assert S.scan_form(pitch4, lanes, generic, fr)[:4] == form
    d = pitch4 * 4
    rng = np.random.default_rng(1000 + pitch4 * 7 + fr)
    n_big = _rows_for(L, qpl)
    R = 64 // L
    kw = dict(lanes=lanes, generic=generic, force_ragged=fr)
    for corpus in ("int", "float"):
        rows, q = (S.int_corpus if corpus == "int" else S.float_corpus)(rng, n_big, d)
        _specials(rows, q[0], ragged)
        masks = S.special_masks(n_big, rng)
        for metric in METRICS:
            for nt in ((1,) if ragged or gen else (0, 1)):
                for n, grid_x, mname in ((n_big, 3, None), (n_big, 1, "random"), (n_big, 3, "edge"), (1, 1, None), (max(1, R - 1), 1, None),
                                         (min(n_big, 2 * R + 1), 3, "zeros")):
                    sub = np.ascontiguousarray(rows[:n])
                    mask = None if mname is None else S.special_masks(n, rng)[mname] if n != n_big else masks[mname]
                    part, guard = S.scan(sub, q, metric, 2, nt=nt, grid_x=grid_x, mask=mask, partials_len=n + 37, **kw)
                    full = np.concatenate([part, guard])
                    cls = S.row_class(sub)
                    if corpus == "int":
                        fin = np.where(np.isfinite(sub), sub, 0)
                        exact = S.exact_keys(fin, q[0], metric)
                        v, _ = S.truth64(sub, q[0], metric)  # (the planted infinities: IEEE's answer)
                        inf = np.flatnonzero(cls == 2)
                        exact[inf] = S.make_keys(S.f2ord(v[inf].astype(np.float32)), inf)
                        S.check_dump(full, n, cls, mask, exact=exact)
                    else:
                        v, band = _band(sub, q[0], metric, form, pitch4)
                        S.check_dump(full, n, cls, mask, value=v, band=band)
    COVERED.add((L, qpl, ragged, gen, fr))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_list_modes_of_every_form(case):
    """Register lists at k = 65 (an insert crosses from the first register to the second) and LDS lists at k = 129, strided,
    per wave and merged per workgroup, on the integer corpus: every list equals the top-k of the reference keys of its rows.
    At least 2101 rows, and each launch's grid is chosen so that every wave visits at least 4 k rows: k = 65 on 8 waves
    (2080), k = 129 on 4 waves (2064), k = 40 on 12 waves (1920)."""
    _, pitch4, lanes, generic, fr, form = case
    L, qpl, ragged, gen = form
    rng = np.random.default_rng(2000 + pitch4 * 7 + fr)
    n = max(_rows_for(L, qpl), 2101)
    rows, q = S.int_corpus(rng, n, pitch4 * 4)
    mask = S.special_masks(n, rng)["random"]
    for metric in METRICS:
        keys = S.exact_keys(rows, q[0], metric)
        for mode, k, grid_x, wgm, m in ((1, 65, 2, 0, None), (1, 65, 1, 1, mask), (1, 40, 3, 0, None), (0, 129, 1, 1, None), (0, 129, 1, 0, mask),
                                        (0, 40, 3, 1, mask)):
            assert n // (grid_x * 4) >= 4 * k
            part, guard = S.scan(rows, q, metric, mode, k=k, grid_x=grid_x, wg_merge=wgm, mask=m, lanes=lanes, generic=generic, force_ragged=fr)
            want = keys if m is None else np.where(S.mask_bits(m, n), keys, np.uint64(0))
            S.check_lists(part[0], k, grid_x if wgm else grid_x * 4, S.list_rows(L, n, grid_x, 0, wgm), want)
            assert (guard == np.uint64(S.SENT_KEY)).all()


# representative instances for the list matrix: one lane per row, short ragged, the wide short form, a wide ragged one, the two
# generic bodies
LIST_CASES = [c for c in CASES if c[0] in ("L1q1e-p1", "L8q3r-p16", "L32q1r-p22", "L8q12e-p96", "L64q12r-p513", "genericL8-p5", "genericL64-p777")]
assert len(LIST_CASES) == 7


@pytest.mark.parametrize("case", LIST_CASES, ids=[c[0] for c in LIST_CASES])
@pytest.mark.parametrize("corpus", ["int", "float"])
def test_list_matrix(case, corpus):
    """k in {1, 63, 64, 65, 128} on register lists, {1, 128, 129, 300} on LDS lists; strided and chunked partitions (a chunk that
    leaves the last waves without work); a grid with more waves than row groups (empty lists); the four masks.  2101 rows on
    every form: a wave of the one-workgroup launches sees 525 rows, at least 4 k up to k = 128 (k = 129 and 300 run on the same
    rows: the LDS list then fills from fewer than 4 k offers).  The float corpus compares with the instance's own dump keys: the arithmetic is the
    dump's, so the check stays exact."""
    _, pitch4, lanes, generic, fr, form = case
    L, qpl, ragged, gen = form
    R = 64 // L
    rng = np.random.default_rng(3000 + pitch4)
    n = 2101
    rows, q = (S.int_corpus if corpus == "int" else S.float_corpus)(rng, n, pitch4 * 4)
    kw = dict(lanes=lanes, generic=generic, force_ragged=fr)
    masks = S.special_masks(n, rng)
    groups = (n + R - 1) // R
    for metric in METRICS:
        dump = {}
        for mname in (None, "ones", "zeros", "random", "edge"):
            mask = None if mname is None else masks[mname]
            if corpus == "int":
                dump[mname] = S.exact_keys(rows, q[0], metric, mask)
            else:
                dump[mname] = S.scan(rows, q, metric, 2, grid_x=2, mask=mask, **kw)[0][0]
        ks = ((1, 1), (1, 63), (1, 64), (1, 65), (1, 128), (0, 1), (0, 128), (0, 129), (0, 300))
        for i, (mode, k) in enumerate(ks):
            wgm = i & 1
            # strided, one workgroup: every wave makes many trips
            part, guard = S.scan(rows, q, metric, mode, k=k, grid_x=1, wg_merge=wgm, **kw)
            S.check_lists(part[0], k, 1 if wgm else 4, S.list_rows(L, n, 1, 0, wgm), dump[None])
            # chunked on three workgroups: the chunk rounded up + 1, so the last waves find no group
            chunk = (groups + 11) // 12 + 1
            part, guard = S.scan(rows, q, metric, mode, k=k, grid_x=3, chunk=chunk, wg_merge=1 - wgm, mask=masks["random"], **kw)
            S.check_lists(part[0], k, 3 if not wgm else 12, S.list_rows(L, n, 3, chunk, 1 - wgm), dump["random"])
            assert (guard == np.uint64(S.SENT_KEY)).all()
        for mname in ("ones", "zeros", "edge"):
            for mode, k in ((1, 64), (0, 129)):
                part, _ = S.scan(rows, q, metric, mode, k=k, grid_x=3, mask=masks[mname], **kw)
                S.check_lists(part[0], k, 12, S.list_rows(L, n, 3, 0, 0), dump[mname])
        # more waves than row groups: the waves past the last group store empty lists
        few = np.ascontiguousarray(rows[:3 * R + 1])
        fkeys = S.exact_keys(few, q[0], metric) if corpus == "int" else S.scan(few, q, metric, 2, **kw)[0][0]
        for mode, k, wgm in ((1, 5, 0), (0, 129, 0), (1, 65, 1)):
            part, _ = S.scan(few, q, metric, mode, k=k, grid_x=4, wg_merge=wgm, **kw)
            behind = S.list_rows(L, len(few), 4, 0, wgm)
            assert any(len(b) == 0 for b in behind)
            S.check_lists(part[0], k, 4 if wgm else 16, behind, fkeys)


@pytest.mark.parametrize("case", [c for c in LIST_CASES if c[1] <= 96], ids=[c[0] for c in LIST_CASES if c[1] <= 96])
def test_repair_launches_run_only_for_overflowed_queries(case):
    """grid_y = 3 queries with y_partials; the counters over_cap - 1, over_cap, over_cap + 1: only the last query's partials
    change, the others keep the sentinel bit for bit."""
    _, pitch4, lanes, generic, fr, form = case
    L = form[0]
    rng = np.random.default_rng(4000 + pitch4)
    n, k, over_cap = 900, 65, 4096
    rows, q = S.int_corpus(rng, n, pitch4 * 4, nq=3)
    counters = np.array([over_cap - 1, over_cap, over_cap + 1], np.uint32)
    for metric in METRICS:
        for mode, wgm in ((1, 1), (0, 0), (2, 0)):
            need = n if mode == 2 else k * (2 if wgm else 8)
            part, guard = S.scan(rows, q, metric, mode, k=k, grid_x=2, wg_merge=wgm, only_if_over=counters, over_cap=over_cap,
                                 y_partials=need + 11, lanes=lanes, generic=generic, force_ragged=fr)
            assert (part[:2] == np.uint64(S.SENT_KEY)).all() and (guard == np.uint64(S.SENT_KEY)).all()
            assert (part[2, need:] == np.uint64(S.SENT_KEY)).all()
            keys = S.exact_keys(rows, q[2], metric)
            if mode == 2:
                assert np.array_equal(part[2, :n], keys)
            else:
                S.check_lists(part[2], k, 2 if wgm else 8, S.list_rows(L, n, 2, 0, wgm), keys)
            # null counters: every query runs
            part, _ = S.scan(rows, q, metric, mode, k=k, grid_x=2, wg_merge=wgm, y_partials=need + 11, lanes=lanes, generic=generic,
                             force_ragged=fr)
            assert not (part[:, :need] == np.uint64(S.SENT_KEY)).any()


@pytest.mark.parametrize("pitch4", [1, 2, 3, 5, 96, S.GENERIC_WIDE_PITCH4])
def test_the_listed_repair_kernel_gives_what_the_generic_kernel_gives(pitch4):
    """An empty list, one entry, and more entries than grid rows (the loop and its LDS reuse): a listed query's partials are
    scan_kernel_generic's of the same L bit for bit (float corpus: the same body), an unlisted query keeps the sentinel."""
    L = S.listed_lanes(pitch4)
    rng = np.random.default_rng(5000 + pitch4)
    n, nq = (600, 6) if pitch4 <= 96 else (150, 6)
    # k = 2048 on LDS lists: 64 KiB of lists + the staged query, so the launch raises the kernel's dynamic LDS limit first, as
    # plan_scan does
    for corpus in (S.int_corpus, S.float_corpus):
        rows, q = corpus(rng, n, pitch4 * 4, nq=nq)
        for metric in METRICS:
            for mode, k, wgm in ((1, 65, 1), (0, 129, 0), (0, 2048, 1)):
                lists = 2 if wgm else 8
                need = k * lists
                assert k < 2048 or S.plan(n, L, k, 0, 0, pitch4 * 16, 256, 2, 0, wgm, 0)[7] == 1  # (needs the attribute)
                ref = S.scan(rows, q, metric, mode, k=k, grid_x=2, wg_merge=wgm, generic=1, y_partials=need)[0]
                if corpus is S.int_corpus:  # the generic launch itself (k = 2048: its LDS attribute as well) against the reference
                    for qi in range(nq):
                        S.check_lists(ref[qi], k, lists, S.list_rows(L, n, 2, 0, wgm), S.exact_keys(rows, q[qi], metric))
                assert S.scan_form(pitch4, 0, 1, 0)[0] == L
                for listed in ([], [4], [5, 0, 3, 1, 4]):
                    over_list = np.array([len(listed)] + listed + [0xFFFFFFFF], np.uint32)  # (the word behind the list is never read)
                    part, guard = S.scan(rows, q, metric, mode, k=k, grid_x=2, grid_y=2, wg_merge=wgm, over_list=over_list, y_partials=need)
                    for qi in range(nq):
                        if qi in listed:
                            assert np.array_equal(part[qi], ref[qi]), (qi, listed)
                        else:
                            assert (part[qi] == np.uint64(S.SENT_KEY)).all(), (qi, listed)
                    assert (guard == np.uint64(S.SENT_KEY)).all()
    LISTED_COVERED.add(L)


def test_the_harness_refuses_what_would_leave_the_arrays():
    rng = np.random.default_rng(6)
    rows, q = S.int_corpus(rng, 100, 16)
    with pytest.raises(ValueError):
        S.scan(rows, q, 0, 2, partials_len=100 - S.GUARD - 1)  # fewer than n_rows keys in dump mode
    with pytest.raises(ValueError):
        S.scan(rows, q, 0, 1, k=8, grid_x=2, partials_len=8 * 8 - S.GUARD - 1)  # fewer than k x P
    with pytest.raises(ValueError):
        S.scan(rows, q, 0, 1, k=8, mask=np.zeros(3, np.uint32))  # ceil(100 / 32) = 4 words
    with pytest.raises(ValueError):
        S.scan(rows, q, 0, 1, k=129)  # register lists hold 128
    with pytest.raises(ValueError):
        S.scan(rows, np.repeat(q, 2, axis=0), 0, 1, k=8, over_list=np.array([3, 0, 1], np.uint32), y_partials=32)  # n + 1 words
    with pytest.raises(ValueError):
        S.scan(rows, q, 0, 1, k=8, over_list=np.array([1, 1], np.uint32))  # names a query that is not there
    with pytest.raises(ValueError):
        S.scan(rows[:0].reshape(0, 16), q, 0, 2, partials_len=4)  # n_rows == 0


def test_zz_every_form_the_picker_can_return_was_covered():
    """Runs last and needs the whole file to have run before it: the dump cases and the listed launches of this session cover
    exactly what the library's pickers can return.  A form that was not launched fails this test."""
    want = {(L, Q, r, g, 0) for L, Q, r, g in {S.scan_form(p, lanes, 0, 0)[:4] for p in range(1, 1001) for lanes in S.LANES}}
    want |= {(L, Q, True, False, 1) for L, Q, r, g, _ in want if not g and not r}
    assert len(want) == 52 + 5 + 25
    assert COVERED == want, ("scan forms not launched by the dump cases of this session", sorted(COVERED ^ want))
    listed = {S.listed_lanes(p) for p in range(1, 1001)}
    assert listed == {1, 2, 4, 8, 64}
    assert LISTED_COVERED == listed, ("listed lane counts not launched in this session", sorted(LISTED_COVERED ^ listed))
    names = " ".join(f"{L}x{Q}{'r' if r else 'e'}{'F' if f else ''}" if not g else f"g{L}" for L, Q, r, g, f in sorted(COVERED))
    print(f"\nscan forms covered (lanes x quads, r ragged / e exact, F forced ragged, g generic): 52 picked + 25 force-ragged fits + "
          f"5 generic + listed lanes {sorted(LISTED_COVERED)} == the picker's set: {names}")
