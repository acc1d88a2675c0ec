"""Distance matrix through the facade on the MI355X: ``WDBX.vector_search_matrix_pairs`` / ``_offsets`` on a small store, with
and without a filter and a seed; a store of two shards answers exactly what a store of one shard answers over the same vectors
(scores compared as bits); the ``_async`` forms and the REST endpoints agree with the blocking calls.  A float64 product on the
unit rows cross-checks the scores."""
import asyncio

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

D, N = 16, 3000


def _bits(pairs):
    return [(p["a"], p["b"], np.float32(p["score"]).view(np.uint32).item()) for p in pairs]


def test_facade_one_and_two_shards_filter_seed_async_and_rest(tmp_path):
    from wdbx_amd import WDBX, api

    raw = O.synth_rows(O.SEED_CORPUS, 0, N, D).astype(np.float32)
    meta = {f"row_{i}": {"lang": "en" if i % 3 else "de"} for i in range(N)}
    stores = []
    for shards in (1, 2):
        w = WDBX(vector_dimension=D, num_shards=shards, data_dir=str(tmp_path / f"matrix{shards}"), enable_plugins=False)
        w.vector_store.bulk_store(raw, metadata=meta)
        stores.append(w)
    one, two = stores
    unit = raw.astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)

    for args in (dict(sample=40, limit=3, seed=11), dict(sample=300, limit=5, filter_metadata={"lang": "de"}, seed=2),
                 dict(limit=4, vector_ids=[f"row_{i}" for i in (5, 1, 2999, 1500, 7, 5)] + ["nope"]),
                 dict(sample=30, limit=100, seed=3)):
        pairs = one.vector_search_matrix_pairs(**args)
        off = one.vector_search_matrix_offsets(**args)
        ids = off["ids"]
        n = len(ids)
        assert n == (5 if "vector_ids" in args else args["sample"]) and ids == sorted(ids)
        per_anchor = min(args["limit"], n - 1)
        assert len(pairs) == n * per_anchor
        assert [p["a"] for p in pairs] == [a for a in ids for _ in range(per_anchor)]  # anchor-major
        for a in ids:
            mine = [p for p in pairs if p["a"] == a]
            assert all(p["b"] != a and p["b"] in ids for p in mine) and len({p["b"] for p in mine}) == per_anchor
            assert [p["score"] for p in mine] == sorted((p["score"] for p in mine), reverse=True)
            # the true nearest among the sample, by the float64 product (margins far above the fp32 rounding are asserted only)
            others = [v for v in ids if v != a]
            exact = sorted(((float(unit[int(a[4:])] @ unit[int(v[4:])]), v) for v in others), reverse=True)
            for p, (s, _) in zip(mine, exact):
                assert abs(p["score"] - s) < 2e-5
        if "filter_metadata" in args:
            assert all(meta[v]["lang"] == "de" for v in ids)
        back = [{"a": ids[r], "b": ids[c], "score": s} for r, c, s in zip(off["offsets_row"], off["offsets_col"], off["scores"])]
        assert back == pairs
        # two shards on the same GPU: the same sample, the same lines, the same score bits
        assert _bits(two.vector_search_matrix_pairs(**args)) == _bits(pairs)
        assert two.vector_search_matrix_offsets(**args) == off
        # the same seed gives the same sample; async and REST agree
        assert one.vector_search_matrix_pairs(**args) == pairs
        assert asyncio.run(one.vector_search_matrix_pairs_async(**args)) == pairs
        assert asyncio.run(two.vector_search_matrix_offsets_async(**args)) == off
        body = {"sample": args.get("sample"), "limit": args["limit"], "filter": args.get("filter_metadata"),
                "vector_ids": args.get("vector_ids"), "seed": args.get("seed")}
        assert asyncio.run(api.search_matrix_pairs_endpoint(one, body)) == {"pairs": pairs}
        assert asyncio.run(api.search_matrix_offsets_endpoint(two, body)) == off
    assert one.vector_search_matrix_pairs(sample=40, limit=3, seed=12) != one.vector_search_matrix_pairs(sample=40, limit=3, seed=11)
    one.vector_store.config.set("MATRIX_MAX_SAMPLE", 20)
    with pytest.raises(ValueError, match="MATRIX_MAX_SAMPLE"):
        one.vector_search_matrix_pairs(sample=21, seed=1)
    assert one.vector_store.last_search_path == "threads"
