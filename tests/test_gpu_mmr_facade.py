"""MMR search through the facade on the MI355X: ``WDBX.vector_search_mmr`` over one shard returns the store's ids in pick
order with relevance scores, a metadata filter goes in as the row mask, ``threshold`` cuts by relevance, the ``_async`` form and
the REST field agree with the blocking call, two shards raise ``ValueError``.  The reference is the greedy loop in float64 on
the unit rows; every step's gap between the best and the second-best value is asserted to be above 1e-4, three orders of
magnitude above the fp32 rounding of values of size 1 at d = 16, so the float64 picks are the library's picks."""
import asyncio

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu


def _greedy64(unit, q, allowed, limit, fetch_k, lam):
    s = unit @ q
    ids = np.flatnonzero(allowed)
    pool = ids[np.lexsort((ids, -s[ids]))][:fetch_k]
    rel, c = s[pool], unit[pool]
    G = c @ c.T
    pos, picked, maxsim = [0], np.zeros(len(pool), bool), np.full(len(pool), -np.inf)
    picked[0] = True
    gap = np.inf
    while len(pos) < min(limit, len(pool)):
        maxsim = np.maximum(maxsim, G[pos[-1]])
        v = np.where(picked, -np.inf, lam * rel - (1 - lam) * maxsim)
        order = np.argsort(-v, kind="stable")
        if len(pool) - len(pos) > 1:
            gap = min(gap, v[order[0]] - v[order[1]])
        picked[order[0]] = True
        pos.append(int(order[0]))
    return [(int(pool[p]), float(rel[p])) for p in pos], gap


def test_facade_over_one_shard_and_rest_field(tmp_path):
    from wdbx_amd import WDBX, api

    d, n = 16, 2000
    raw = O.synth_rows(O.SEED_CORPUS, 0, n, d).astype(np.float32)
    raw[1000:1012] = raw[7] + 0.01 * O.synth_rows(O.SEED_QUERY, 50, 12, d)  # a dozen near-duplicates of row 7
    meta = {f"row_{i}": {"lang": "en" if i % 3 else "de"} for i in range(n)}
    w = WDBX(vector_dimension=d, num_shards=1, data_dir=str(tmp_path / "mmr"), enable_plugins=False)
    w.vector_store.bulk_store(raw, metadata=meta)
    unit = raw.astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    q = raw[7].astype(np.float64) + 0.4 * O.synth_rows(O.SEED_QUERY, 3, 1, d)[0]  # (row 3: screened, every gap above 1e-4)
    q /= np.linalg.norm(q)
    everyone = np.ones(n, bool)

    def same(got, want):
        picks, gap = want
        assert gap > 1e-4, f"the reference's picks are not safe against fp32 rounding: a gap of {gap:g}"
        assert [g[0] for g in got] == [f"row_{r}" for r, _ in picks]
        np.testing.assert_allclose([g[1] for g in got], [s for _, s in picks], atol=2e-5, rtol=0)
        assert all(g[2] == meta[g[0]] for g in got)

    got = w.vector_search_mmr(q.tolist(), limit=10, fetch_k=40, lambda_mult=0.5)
    same(got, _greedy64(unit, q, everyone, 10, 40, 0.5))
    plain = w.vector_search(q.tolist(), limit=10)
    assert got[0][:2] == plain[0][:2] and [g[0] for g in got] != [p[0] for p in plain]
    dups = {f"row_{r}" for r in [7, *range(1000, 1012)]}
    assert {p[0] for p in plain} <= dups and len({g[0] for g in got} - dups) >= 5
    # fetch_k defaults to 4 * limit; lambda = 1 is the plain search
    same(w.vector_search_mmr(q.tolist(), limit=5), _greedy64(unit, q, everyone, 5, 20, 0.5))
    assert [g[:2] for g in w.vector_search_mmr(q.tolist(), limit=10, lambda_mult=1.0)] == [p[:2] for p in plain]
    # the filter is the row mask: the pool holds matching rows only
    flt = {"lang": "de"}
    allowed = np.array([i % 3 == 0 for i in range(n)])
    filtered = w.vector_search_mmr(q.tolist(), limit=10, fetch_k=40, lambda_mult=0.5, filter_metadata=flt)
    same(filtered, _greedy64(unit, q, allowed, 10, 40, 0.5))
    assert len(filtered) == 10
    # the threshold cuts by relevance, wherever in the pick order
    scores = sorted(g[1] for g in got)
    assert scores[5] - scores[4] > 1e-4 and scores[4] > 0
    t = (scores[4] + scores[5]) / 2
    cut = w.vector_search_mmr(q.tolist(), limit=10, fetch_k=40, lambda_mult=0.5, threshold=t)
    assert cut == [g for g in got if g[1] >= t] and len(cut) == 5
    # async and REST
    assert asyncio.run(w.vector_search_mmr_async(q.tolist(), limit=10, fetch_k=40, lambda_mult=0.5)) == got
    rest = asyncio.run(api.search_endpoint(w, {"query_vector": q.tolist(), "limit": 10, "filter_metadata": flt,
                                               "mmr": {"lambda": 0.5, "fetch_k": 40}}))["results"]
    assert [(r["vector_id"], r["similarity"]) for r in rest] == [g[:2] for g in filtered]
    with pytest.raises(ValueError):
        asyncio.run(api.search_endpoint(w, {"query_vector": q.tolist(), "mmr": {"lambda": 1.5}}))
    asyncio.run(w.shutdown())


def test_two_shards_raise(tmp_path):
    from wdbx_amd import WDBX

    d = 16
    w = WDBX(vector_dimension=d, num_shards=2, data_dir=str(tmp_path / "mmr2"), enable_plugins=False)
    w.vector_store.bulk_store(O.synth_rows(O.SEED_CORPUS, 0, 200, d))
    q = O.synth_rows(O.SEED_QUERY, 0, 1, d)[0].tolist()
    with pytest.raises(ValueError, match="one shard"):
        w.vector_search_mmr(q, limit=5)
    with pytest.raises(ValueError, match="one shard"):
        asyncio.run(w.vector_search_mmr_async(q, limit=5))
    assert len(w.vector_search(q, limit=5)) == 5
    asyncio.run(w.shutdown())
