"""Search groups through the facade on the MI355X: ``WDBX.vector_search_groups`` over one and over three shards of one GPU gives
the groups and members of a numpy ranking of the stored (normalised) vectors -- float64, asserted only where its own gaps are
above 1e-5 --, with a filter, through the ``_async`` form and through the REST field."""
import asyncio

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

D, N = 16, 3000


def _expected(unit, meta, q, limit, g, flt=None):
    s = unit @ (q.astype(np.float64) / np.linalg.norm(q.astype(np.float64)))
    order = np.argsort(-s, kind="stable")
    groups, at = [], {}
    for r in order:
        m = meta[f"row_{r}"]
        if flt and any(m.get(k) != v for k, v in flt.items()):
            continue
        key = m.get("doc", f"row_{r}")
        if key not in at:
            if len(groups) == limit:
                continue
            at[key] = len(groups)
            groups.append((key, []))
        if len(groups[at[key]][1]) < g:
            groups[at[key]][1].append((f"row_{r}", float(s[r])))
    return groups


def _gap(unit, meta, q, limit, g, flt):
    """the smallest float64 gap a decision rests on: between the best scores of the first limit + 1 groups, and between the
    first g + 1 members of each of them"""
    wide = _expected(unit, meta, q, limit + 1, g + 1, flt)
    lists = [[hits[0][1] for _, hits in wide]] + [[sc for _, sc in hits] for _, hits in wide]
    return min((a - b for xs in lists for a, b in zip(xs, xs[1:])), default=1.0)


def test_groups_on_one_and_three_shards_filter_async_and_rest(tmp_path):
    from wdbx_amd import WDBX, api

    raw = O.synth_rows(O.SEED_CORPUS, 0, N, D).astype(np.float32)
    rng = np.random.default_rng(9)
    doc = rng.integers(0, 150, size=N)  # about 20 chunks per document; every 50th vector has none
    meta = {f"row_{i}": ({"doc": f"doc{doc[i]}", "lang": "en" if i % 3 else "de"} if i % 50 else {"lang": "en"}) for i in range(N)}
    unit = raw.astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    stores = []
    for shards in (1, 3):
        w = WDBX(vector_dimension=D, num_shards=shards, data_dir=str(tmp_path / f"groups{shards}"), enable_plugins=False,
                 config={"DISTINCT_KEY": "doc"})
        w.vector_store.bulk_store(raw, metadata=meta)
        stores.append(w)
    one, three = stores
    checked = 0
    for seed in range(6):
        q = O.synth_rows(O.SEED_QUERY, seed, 1, D)[0].astype(np.float32)
        for limit, g, flt in ((10, 3, None), (5, 1, None), (4, 8, {"lang": "de"})):
            want = _expected(unit, meta, q, limit, g, flt)
            if _gap(unit, meta, q, limit, g, flt) <= 1e-5:  # (a float64 near-tie where a decision falls: fp32 may go either way)
                continue
            checked += 1
            for w in (one, three):
                got = w.vector_search_groups(q.tolist(), limit=limit, group_size=g, filter_metadata=flt)
                assert [x["key"] for x in got] == [key for key, _ in want], (seed, limit, g)
                for x, (_, hits) in zip(got, want):
                    assert [h[0] for h in x["hits"]] == [vid for vid, _ in hits]
                    assert np.allclose([h[1] for h in x["hits"]], [sc for _, sc in hits], atol=2e-6, rtol=0)
                    assert all(h[2] == meta[h[0]] for h in x["hits"])
            assert three.vector_search_groups(q.tolist(), limit=limit, group_size=g, filter_metadata=flt) == \
                one.vector_search_groups(q.tolist(), limit=limit, group_size=g, filter_metadata=flt)  # score bits too
    assert checked >= 6
    q = O.synth_rows(O.SEED_QUERY, 0, 1, D)[0].astype(np.float32)
    got = one.vector_search_groups(q.tolist(), limit=10, group_size=3)
    assert asyncio.run(three.vector_search_groups_async(q.tolist(), limit=10, group_size=3)) == got
    rest = asyncio.run(api.search_endpoint(three, {"query_vector": q.tolist(), "limit": 10, "group_size": 3}))
    assert [(g["key"], [(h["vector_id"], h["similarity"], h["metadata"]) for h in g["hits"]]) for g in rest["groups"]] == \
        [(g["key"], g["hits"]) for g in got]
    # the threshold drops members below it and the groups it empties
    t = got[4]["hits"][0][1]
    cut = three.vector_search_groups(q.tolist(), limit=10, group_size=3, threshold=t)
    assert cut == [{"key": g["key"], "hits": [h for h in g["hits"] if h[1] >= t]} for g in got if g["hits"][0][1] >= t]
    assert len(cut) == 5
    with pytest.raises(ValueError):
        asyncio.run(api.search_endpoint(three, {"query_vector": q.tolist(), "group_size": 0}))
    for w in stores:
        asyncio.run(w.shutdown())
