"""One filter PER QUERY in a batch through the public layers on a GPU: ``WDBX.vector_search_batch`` /
``VectorStore.search_batch`` with ``filter_metadata`` as a list -> ``HipFlatIndex.search_batch(row_masks=, mask_of_query=)``
-> ``wdbx_index_search_multimask``.  A small store with three metadata values (on a store this small the library answers
class by class behind the same entry point; the tile pass itself is covered by tests/test_gpu_multimask.py)."""
import asyncio
import shutil
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, N = 16, 600
LANGS = ("en", "de", "fr")


@pytest.fixture(scope="module")
def db():
    from wdbx_amd import WDBX

    temp_dir = tempfile.mkdtemp()
    w = WDBX(vector_dimension=D, num_shards=2, data_dir=temp_dir, enable_plugins=False,
             config={"WDBX_VECTOR_STORE_SAVE_IMMEDIATELY": False})
    asyncio.run(w.initialize())
    rng = np.random.default_rng(5)
    vectors = {f"v{i}": rng.standard_normal(D).astype(np.float32).tolist() for i in range(N)}
    # "fr" is rare: a post-filtered top-5 under-returns for it
    meta = {f"v{i}": {"lang": "fr" if i % 40 == 7 else LANGS[i % 2]} for i in range(N)}
    assert w.vector_store.batch_store(vectors, meta) == N
    yield w
    asyncio.run(w.shutdown())
    shutil.rmtree(temp_dir, ignore_errors=True)


def _queries(n):
    return np.random.default_rng(9).standard_normal((n, D)).astype(np.float32)


FILTERS = [{"lang": "en"}, {"lang": "fr"}, None, {"lang": "de"}, {"lang": "fr"}, {"lang": "en"}, None, {"lang": "de"}, {"lang": "fr"}]


def _same(a, b):
    assert [r[0] for r in a] == [r[0] for r in b]
    np.testing.assert_allclose([r[1] for r in a], [r[1] for r in b], atol=1e-6, rtol=0)


def test_pushed_down_list_equals_per_query_prefiltered_search(db):
    queries = _queries(len(FILTERS))
    got = db.vector_search_batch(queries.tolist(), limit=5, filter_metadata=FILTERS, prefilter=True)
    assert len(got) == len(FILTERS)
    for q, flt, res in zip(queries, FILTERS, got):
        _same(res, db.vector_search(q.tolist(), limit=5, filter_metadata=flt, prefilter=True))
        assert len(res) == 5 and all(r[2]["lang"] == flt["lang"] for r in res if flt)


def test_list_without_prefilter_equals_per_query_post_filtered_search(db):
    queries = _queries(len(FILTERS))
    got = db.vector_search_batch(queries.tolist(), limit=5, filter_metadata=FILTERS)
    for q, flt, res in zip(queries, FILTERS, got):
        _same(res, db.vector_search(q.tolist(), limit=5, filter_metadata=flt))
    assert any(len(res) < 5 for res in got), "the rare value is meant to make the post-filter under-return"


def test_wrong_list_length_raises(db):
    with pytest.raises(ValueError):
        db.vector_search_batch(_queries(3).tolist(), limit=5, filter_metadata=[None, None], prefilter=True)


def test_async_coalesce_filters_one_multimask_call_per_index(db):
    """Six ``search_async`` callers with mixed filters under ``ASYNC_COALESCE_FILTERS``: the answers of one-at-a-time calls,
    and every index saw exactly one call with a mask per query (and no single-mask batch)."""
    store = db.vector_store
    queries = _queries(6)
    filters = [{"lang": "en"}, {"lang": "fr"}, {"lang": "de"}, {"lang": "fr"}, {"lang": "en"}, {"lang": "de"}]
    calls = []
    originals = [(ix._native, ix._native.search_multimask, ix._native.search) for ix in store.indices]

    def spy(s, kind, fn):
        def wrapped(*a, **kw):
            calls.append((s, kind, len(a[0])))
            return fn(*a, **kw)
        return wrapped

    async def run():
        return await asyncio.gather(*[store.search_async(q.tolist(), limit=5, filter_metadata=f, prefilter=True)
                                      for q, f in zip(queries, filters)])

    keep = store.config.get("ASYNC_COALESCE_FILTERS")
    store.config.set("ASYNC_COALESCE_FILTERS", True)
    try:
        for s, (nat, mm, one) in enumerate(originals):
            nat.search_multimask = spy(s, "multimask", mm)
            nat.search = spy(s, "search", one)
        got = asyncio.run(run())
    finally:
        for nat, mm, one in originals:
            del nat.search_multimask, nat.search  # (the instance attributes: the class's methods are back)
        store.config.set("ASYNC_COALESCE_FILTERS", keep)
    assert sorted(calls) == [(s, "multimask", 6) for s in range(len(store.indices))]
    for q, f, res in zip(queries, filters, got):
        _same(res, db.vector_search(q.tolist(), limit=5, filter_metadata=f, prefilter=True))
        assert len(res) == 5 and all(r[2]["lang"] == f["lang"] for r in res)
