"""Discovery search through the facade on the MI355X: ``WDBX.vector_discover`` returns the store's ids with the target's score
(or the loss) and the wins, ids and raw vectors mix in the target and the pairs, id examples never come back, a store of two
shards answers exactly what a store of one shard answers over the same vectors (the fold is per row, and a row's score does
not depend on its shard), a metadata filter travels as the row masks, and the ``_async`` form and the REST endpoint agree
with the blocking call.  A float64 fold on the unit rows cross-checks wins and scores wherever its own margins are above
1e-4."""
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
        w = WDBX(vector_dimension=D, num_shards=shards, data_dir=str(tmp_path / f"disc{shards}"), enable_plugins=False)
        w.vector_store.bulk_store(raw, metadata=meta)
        out.append(w)
    return raw, meta, out


def test_facade_one_and_two_shards_filter_async_and_rest(tmp_path):
    from wdbx_amd import api

    raw, meta, (one, two) = _stores(tmp_path)
    unit = raw.astype(np.float64)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    extra = O.synth_rows(O.SEED_QUERY, 0, 3, D).astype(np.float32)
    context = [("row_7", extra[0].tolist()), (extra[1].tolist(), "row_2999"), ("row_1500", "row_11")]
    ids = {"row_7", "row_2999", "row_1500", "row_11"}
    ex = [x / np.linalg.norm(x.astype(np.float64)) for x in extra]
    pairs = [(unit[7], ex[0]), (ex[1], unit[2999]), (unit[1500], unit[11])]
    diffs = np.stack([unit @ p - unit @ n for p, n in pairs], axis=1)
    for target, tvec, tid in (("row_42", unit[42], {"row_42"}), (extra[2].tolist(), ex[2], set())):
        for limit in (10, 300):
            got = one.vector_discover(target, context, limit=limit, with_wins=True)
            assert len(got) == limit and not {g[0] for g in got} & (ids | tid)  # ids as examples never come back
            assert all(g[2] == meta[g[0]] for g in got)
            wins = [g[3] for g in got]
            assert wins == sorted(wins, reverse=True)
            for w in set(wins):
                s = [g[1] for g in got if g[3] == w]
                assert s == sorted(s, reverse=True)
            assert two.vector_discover(target, context, limit=limit, with_wins=True) == got  # ids, score bits, wins, in order
            assert one.vector_discover(target, context, limit=limit) == [g[:3] for g in got]
        for vid, score, _, w in one.vector_discover(target, context, limit=300, with_wins=True):
            r = int(vid[4:])
            assert abs(score - unit[r] @ tvec) < 2e-5
            if (np.abs(diffs[r]) > 1e-4).all():
                assert w == int((diffs[r] > 0).sum())
    assert len(set(g[3] for g in one.vector_discover("row_42", context, limit=2000, with_wins=True))) >= 3
    # context search: the loss, 0 first in the store's order, never positive, wins 0
    for limit in (10, 1500):
        got = one.vector_discover(None, context, limit=limit, with_wins=True)
        assert len(got) == limit and not {g[0] for g in got} & ids
        assert all(g[1] <= 0 and g[3] == 0 for g in got)
        assert [g[1] for g in got] == sorted((g[1] for g in got), reverse=True)
        assert two.vector_discover(None, context, limit=limit, with_wins=True) == got
        for vid, loss, _, _ in got:
            assert abs(loss - np.minimum(diffs[int(vid[4:])], 0).sum()) < 1e-4
    assert got[0][1] == 0 and got[-1][1] < 0
    # the filter travels as the row masks
    flt = {"lang": "de"}
    filtered = one.vector_discover("row_42", context, limit=50, filter_metadata=flt, with_wins=True)
    assert len(filtered) == 50 and all(g[2]["lang"] == "de" for g in filtered)
    assert two.vector_discover("row_42", context, limit=50, filter_metadata=flt, with_wins=True) == filtered
    # async and REST
    got = one.vector_discover("row_42", context, limit=10, with_wins=True)
    assert asyncio.run(two.vector_discover_async("row_42", context, limit=10, with_wins=True)) == got
    body = {"target": "row_42", "context": [{"positive": p, "negative": n} for p, n in context], "limit": 10}
    rest = asyncio.run(api.discover_endpoint(two, body))["results"]
    assert [(r["vector_id"], r["similarity"], r["metadata"], r["wins"]) for r in rest] == got
    with pytest.raises(ValueError):
        asyncio.run(api.discover_endpoint(two, {"context": []}))
    with pytest.raises(ValueError, match="no stored vector"):
        one.vector_discover("row_99999")
    for w in (one, two):
        asyncio.run(w.shutdown())
