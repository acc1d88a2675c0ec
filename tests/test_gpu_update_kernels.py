"""The kernels behind wdbx_index_set_rows_at / wdbx_index_remove_rows alone (kernels_update.h), through
tests/kernel_harness/update_harness.hip: the list forms against the range quantisers they share their per-row functions with.

Reference: the existing range kernels (checked against numpy in tests/test_gpu_select_kernels.py).  Two comparisons per case,
every word of every copy, compared as raw bytes (NaN rows included):
  * copies built by the range kernels over the ORIGINAL rows, then the list form -> must equal the range kernels over the
    whole UPDATED array (unlisted rows keep their cells, guard cells keep their sentinels);
  * copies full of a sentinel byte, then the list form -> must equal what wdbx_index_set_rows' steps leave when run once per
    listed row on the same sentinel arrays (cells of unlisted rows and guard cells keep the sentinel in both)."""
import numpy as np
import pytest

import update_harness as H

pytestmark = pytest.mark.gpu

N = 64 * 5 + 7
DIMS = (20, 96, 384, 400)


def _corpus(dim, seed=5):
    rng = np.random.default_rng(seed + dim)
    return rng.standard_normal((N, dim)).astype(np.float32)


def _new_rows(dim, n, seed=11):
    rng = np.random.default_rng(seed + dim)
    rows = rng.standard_normal((n, dim)).astype(np.float32) * np.float32(0.7)
    if n >= 3:  # the special rows ride among the listed ones: NaN, all zero, one outlier element
        rows[0, dim // 2] = np.nan
        rows[1] = 0.0
        rows[2, 3] = 1.0e6
    return rows


def _full_coverage(shape):
    cov = {"cn": N, "16": N, "8": N, "g": N}
    if shape.has_u6:
        cov["6"] = N
    if shape.has_u42:
        cov["42"] = N
    return cov


def _lists():
    rng = np.random.default_rng(2)
    third = np.sort(rng.choice(N, N // 3, replace=False))
    return {"row0": [0], "last": [N - 1], "63_64": [63, 64], "every": list(range(N)), "third": third.tolist(),
            "few": [5, 63, 64, 130, N - 1]}


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    av, bv = a.view(np.uint8), b.view(np.uint8)
    if not np.array_equal(av, bv):
        bad = np.flatnonzero(av != bv)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at byte {bad[0]} of {av.size}")


def _check(dim, row_list, coverage, src, normalize, round_rows=0):
    shape = H.Shape(dim, N)
    rows0 = shape.rows_array(_corpus(dim))
    blank = shape.blank(0xAB)
    # what set_rows' own steps leave, row by row, from sentinel copies
    rows_ref, per_row, _ = H.run(H.PER_ROW, shape, coverage, rows0, blank, row_list, src, normalize)
    # the list form on the same sentinel copies
    rows_new, listed, launches = H.run(H.LIST, shape, coverage, rows0, blank, row_list, src, normalize, round_rows)
    _same(rows_new, rows_ref, "fp32 rows")
    for name in H.COPIES:
        _same(listed[name], per_row[name], f"{name} (sentinel start)")
    # the range kernels over the original and over the updated array; the list form on top of the former
    _, before, _ = H.run(H.RANGE, shape, coverage, rows0, blank)
    _, after, _ = H.run(H.RANGE, shape, coverage, rows_ref, blank)
    _, patched, _ = H.run(H.LIST, shape, coverage, rows0, before, row_list, src, normalize, round_rows)
    for name in H.COPIES:
        _same(patched[name], after[name], f"{name} (range start)")
    return launches, rows_new


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("which", ["row0", "last", "63_64", "every", "third", "few"])
def test_list_forms_write_the_range_kernels_bytes(dim, which):
    row_list = _lists()[which]
    shape = H.Shape(dim, N)
    _check(dim, row_list, _full_coverage(shape), _new_rows(dim, len(row_list)), normalize=False)


@pytest.mark.parametrize("dim", DIMS)
def test_normalised_rows_are_normalize_rows_kernel_s(dim):
    row_list = _lists()["third"]
    shape = H.Shape(dim, N)
    _, rows_new = _check(dim, row_list, _full_coverage(shape), _new_rows(dim, len(row_list)), normalize=True)
    body = rows_new[:N * shape.pitch].reshape(N, shape.pitch)
    norms = np.linalg.norm(body[row_list[3:], :dim].astype(np.float64), axis=1)
    assert np.allclose(norms, 1.0, atol=1e-5)
    assert not np.any(body[row_list[1]])                    # the zero row stays zero
    assert np.all(body[:, dim:] == 0)                       # pads as copy_padded leaves them


@pytest.mark.parametrize("dim", DIMS)
def test_a_list_whose_tail_lies_past_a_coverage(dim):
    """Each copy covers a different prefix; listed rows behind a copy's coverage leave that copy alone."""
    shape = H.Shape(dim, N)
    coverage = {"cn": 200, "16": 65, "8": N - 1, "g": 128}   # (the int8 copy's coverage ends on a group boundary)
    if shape.has_u6:
        coverage["6"] = 64
    if shape.has_u42:
        coverage["42"] = 1
    for which in ("few", "third", "every", "last"):
        row_list = _lists()[which]
        _check(dim, row_list, coverage, _new_rows(dim, len(row_list)), normalize=False)
    # no copy at all: only the rows are written, one launch
    launches, _ = _check(dim, [0, 64, N - 1], {}, _new_rows(dim, 3), normalize=False)
    assert launches == 1


@pytest.mark.parametrize("dim", DIMS)
def test_removal_writes_the_nan_tombstone(dim):
    shape = H.Shape(dim, N)
    row_list = _lists()["few"]
    launches, rows_new = _check(dim, row_list, _full_coverage(shape), None, normalize=False)
    body = rows_new[:N * shape.pitch].reshape(N, shape.pitch).view(np.uint32)
    assert np.all(body[row_list, :dim] == 0x7FC00000) and np.all(body[row_list, dim:] == 0)
    assert launches == 3


def test_rounds_cut_the_scatter_not_the_answer():
    dim = 96
    shape = H.Shape(dim, N)
    row_list = _lists()["third"]
    src = _new_rows(dim, len(row_list))
    one, _ = _check(dim, row_list, _full_coverage(shape), src, normalize=True)
    cut, _ = _check(dim, row_list, _full_coverage(shape), src, normalize=True, round_rows=10)
    assert one == 3 and cut == -(-len(row_list) // 10) + 2
    # the launch count does not depend on the list's length
    short, _ = _check(dim, [7], _full_coverage(shape), src[:1], normalize=True)
    assert short == one
