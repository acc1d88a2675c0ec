"""The oracle of tests/test_gpu_multimask.py alone, on the CPU: for every case of its table the float64 gap at rank k among
each query's allowed rows exceeds 1e-5, so the gap rule skips NO query and the GPU test's allowance of 1 skipped query in 10
is never what lets a case pass.  Rows come from the oracle's own generator (what ``fill_synthetic`` writes on the device)."""
import numpy as np
import pytest

import test_gpu_multimask as G
import wdbx_oracle as O

_ROWS = {}


def _rows(n, d):
    if (n, d) not in _ROWS:
        _ROWS[(n, d)] = O.normalize_rows_fast(O.synth_rows(O.SEED_CORPUS, 0, n, d))
    return _ROWS[(n, d)]


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_the_oracle_alone_skips_no_query(name):
    n, d, l2, k, masks, which, queries = G._case(name)
    expected = G._expected(_rows(n, d), queries, k, masks, which, l2)
    gaps = np.array([e[2] for e in expected])
    print(f"{name}: smallest gap at rank k {gaps.min():.3e}")
    assert np.all(gaps > G.GAP), (name, np.nonzero(gaps <= G.GAP)[0].tolist(), gaps.min())
