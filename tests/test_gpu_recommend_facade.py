"""Recommend search through the facade on the MI355X: ``WDBX.vector_recommend`` returns the store's ids with the folded score
and the side, id examples never come back, a store of two shards answers exactly what a store of one shard answers over the
same vectors (the fold is per row, and a row's score does not depend on its shard), ``average_vector`` equals
``vector_search`` of the combined vector minus the examples, and the ``_async`` form and the REST endpoint agree with the
blocking call.  A float64 fold on the unit rows cross-checks the ids and sides wherever its own margins are above 1e-4."""
import asyncio

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

D, N = 16, 3000


def _stores(tmp_path):
    from wdbx_amd import WDBX

    raw = O.synth_rows(O.SEED_CORPUS, 0, N, D).astype(np.float32)
    meta = {f"row_{i}": {"lang": "en" if i % 3 else "de"} for i in range(N)}
    out = []
    for shards in (1, 2):
        w = WDBX(vector_dimension=D, num_shards=shards, data_dir=str(tmp_path / f"rec{shards}"), enable_plugins=False)
        w.vector_store.bulk_store(raw, metadata=meta)
        out.append(w)
    return raw, meta, out


def test_facade_one_and_two_shards_average_vector_and_rest(tmp_path):
    from wdbx_amd import api

    raw, meta, (one, two) = _stores(tmp_path)
    unit = raw.astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    extra = O.synth_rows(O.SEED_QUERY, 0, 2, D).astype(np.float32)
    positive = ["row_7", extra[0].tolist(), "row_1500"]
    negative = ["row_2999", extra[1].tolist()]
    ids = {"row_7", "row_1500", "row_2999"}
    for limit in (10, 300):
        got = one.vector_recommend(positive, negative, limit=limit, with_side=True)
        assert len(got) == limit and not {g[0] for g in got} & ids          # ids as examples never come back
        assert all(g[2] == meta[g[0]] for g in got)
        sides = [g[3] for g in got]
        assert sides == sorted(sides, reverse=True)
        fav = [g[1] for g in got if g[3]]
        dis = [g[1] for g in got if not g[3]]
        assert fav == sorted(fav, reverse=True) and dis == sorted(dis)
        assert two.vector_recommend(positive, negative, limit=limit, with_side=True) == got   # ids, score bits, sides, in order
        assert one.vector_recommend(positive, negative, limit=limit) == [g[:3] for g in got]
    # float64 cross-check of the fold: p and n of every returned row, the side wherever |p - n| is safely above fp32 rounding
    ex = np.stack([unit[7], extra[0] / np.linalg.norm(extra[0].astype(np.float64)), unit[1500], unit[2999],
                   extra[1] / np.linalg.norm(extra[1].astype(np.float64))]).astype(np.float64)
    s = unit @ ex.T
    p, n = s[:, :3].max(axis=1), s[:, 3:].max(axis=1)
    got = one.vector_recommend(positive, negative, limit=300, with_side=True)
    for vid, score, _, side in got:
        r = int(vid[4:])
        assert abs(score - (p[r] if side else n[r])) < 2e-5
        if abs(p[r] - n[r]) > 1e-4:
            assert side == int(p[r] > n[r])
    # a negative equal to a positive: everything disfavoured
    assert all(g[3] == 0 for g in two.vector_recommend(["row_7"], ["row_7"], limit=20, with_side=True))
    # the filter travels as the row masks
    flt = {"lang": "de"}
    filtered = one.vector_recommend(positive, negative, limit=50, filter_metadata=flt, with_side=True)
    assert len(filtered) == 50 and all(g[2]["lang"] == "de" for g in filtered)
    assert two.vector_recommend(positive, negative, limit=50, filter_metadata=flt, with_side=True) == filtered
    # average_vector: the plain search of avg(pos) + (avg(pos) - avg(neg)), minus the examples
    for w in (one, two):
        pos = [np.asarray(w.vector_store.get("row_7")[0], np.float32), extra[0], np.asarray(w.vector_store.get("row_1500")[0], np.float32)]
        neg = [np.asarray(w.vector_store.get("row_2999")[0], np.float32), extra[1]]
        ap, an = np.mean(np.stack(pos), axis=0, dtype=np.float32), np.mean(np.stack(neg), axis=0, dtype=np.float32)
        plain = [r for r in w.vector_search((ap + (ap - an)).tolist(), limit=10 + 3) if r[0] not in ids][:10]
        assert w.vector_recommend(positive, negative, limit=10, strategy="average_vector") == plain
    # async and REST
    got = one.vector_recommend(positive, negative, limit=10, with_side=True)
    assert asyncio.run(two.vector_recommend_async(positive, negative, limit=10, with_side=True)) == got
    rest = asyncio.run(api.recommend_endpoint(two, {"positive": positive, "negative": negative, "limit": 10}))["results"]
    assert [(r["vector_id"], r["similarity"], r["metadata"], r["side"]) for r in rest] == got
    with pytest.raises(ValueError):
        asyncio.run(api.recommend_endpoint(two, {"positive": []}))
    with pytest.raises(ValueError, match="no stored vector"):
        one.vector_recommend(["row_99999"])
    for w in (one, two):
        asyncio.run(w.shutdown())
