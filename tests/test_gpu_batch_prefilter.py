"""Filter push-down for batches through the real ``WDBX`` on the GPU (the CPU twin with a stub shard:
tests/test_batch_prefilter.py): ~70 k rows on one shard, ``vector_search_batch(prefilter=True)`` against numpy's exact
search restricted to the rows the metadata filter allows."""
import asyncio
import shutil
import tempfile

import numpy as np
import pytest

import wdbx_oracle as O

pytestmark = pytest.mark.gpu

N, D, NQ, LIMIT = 70_003, 384, 24, 10


@pytest.fixture(scope="module")
def store():
    from wdbx_amd import WDBX

    tmp = tempfile.mkdtemp()
    w = WDBX(vector_dimension=D, num_shards=1, data_dir=tmp, enable_plugins=False)
    rows = O.normalize_rows_fast(O.synth_rows(O.SEED_CORPUS, 0, N, D))
    # one row in 40 is "en": a post-filtered top-10 holds ~0.25 of them
    meta = {f"row_{r}": {"lang": "en" if r % 40 == 7 else "xx"} for r in range(N)}
    w.vector_store.bulk_store(rows, metadata=meta)
    ix = w.vector_store.indices[0]._native
    ix.set_option("gemm_min_rows", 16384)  # (70 k rows reach the tiles)
    ix.set_option("single_min_rows", 0)    # (and lone queries the selection scan: the same exact re-scoring, bit for bit)
    yield w, ix, ix.get_rows(0, N)
    asyncio.run(w.shutdown())
    shutil.rmtree(tmp, ignore_errors=True)


def _expected(rows, q, allowed, limit):
    rows_a = np.nonzero(allowed)[0]
    s = rows[rows_a].astype(np.float64) @ q.astype(np.float64)
    order = np.lexsort((rows_a, -s))[: limit + 1]
    gap = s[order[limit - 1]] - s[order[limit]] if len(order) > limit else np.inf
    return rows_a[order[:limit]], s[order[:limit]], gap


def test_batch_prefilter_is_the_exact_search_over_the_allowed_rows(store):
    w, ix, rows = store
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 700, NQ, D))
    flt = {"lang": "en"}
    allowed = np.arange(N) % 40 == 7
    post = w.vector_search_batch(queries.tolist(), limit=LIMIT, filter_metadata=flt)
    assert ix.get_option("last_batch_masked") == 0
    assert all(len(r) < LIMIT for r in post), "the post-filter is meant to under-return here"
    pre = w.vector_search_batch(queries.tolist(), limit=LIMIT, filter_metadata=flt, prefilter=True)
    assert ix.get_option("last_batch_masked") == 1 and ix.get_option("last_gemm_family") == 3
    assert ix.get_option("last_batch_allowed_rows") == int(allowed.sum())
    skipped = 0
    for q, res, few in zip(queries, pre, post):
        e_rows, e_score, gap = _expected(rows, q, allowed, LIMIT)
        assert len(res) == LIMIT and all(m == {"lang": "en"} for _, _, m in res)
        assert [r[0] for r in few] == [r[0] for r in res[: len(few)]]  # the post-filter's hits head the full answer
        if gap <= 1e-5:
            skipped += 1
            continue
        assert sorted(r[0] for r in res) == sorted(f"row_{r}" for r in e_rows)
        np.testing.assert_allclose([r[1] for r in res], e_score, atol=1e-5, rtol=0)
        assert res == w.vector_search(q.tolist(), limit=LIMIT, filter_metadata=flt, prefilter=True)
    print(f"{skipped} of {NQ} queries skipped (float64 gap at rank {LIMIT} <= 1e-5)")
    assert skipped * 10 <= NQ
    # the REST batch route with the field, and the default (config FILTER_PUSHDOWN off): today's post-filter
    from wdbx_amd import api

    body = {"query_vectors": queries[:6].tolist(), "limit": LIMIT, "filter_metadata": flt}
    out = asyncio.run(api.search_batch_endpoint(w, dict(body, prefilter=True)))
    assert [[h["vector_id"] for h in r] for r in out["results"]] == [[h[0] for h in r] for r in pre[:6]]
    out = asyncio.run(api.search_batch_endpoint(w, body))
    assert [[h["vector_id"] for h in r] for r in out["results"]] == [[h[0] for h in r] for r in post[:6]]


def test_async_callers_sharing_a_filter_share_one_masked_pass(store):
    w, ix, rows = store
    queries = O.normalize_rows_fast(O.synth_rows(O.SEED_QUERY, 800, 8, D))
    flt = {"lang": "en"}

    async def many():
        return await asyncio.gather(*[w.vector_store.search_async(q.tolist(), limit=LIMIT, filter_metadata=flt, prefilter=True)
                                      for q in queries])

    ix.profile(True)
    ix.profile_read_gemm()
    got = asyncio.run(many())
    g = ix.profile_read_gemm()
    ix.profile(False)
    assert ix.get_option("last_batch_masked") == 1 and g["gemm_launches"] == 2  # ONE sample pass + ONE full pass for all 8
    for q, res in zip(queries, got):
        assert res == w.vector_search(q.tolist(), limit=LIMIT, filter_metadata=flt, prefilter=True)
