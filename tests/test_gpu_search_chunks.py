"""GPU: the query-chunk loops of retrieval.search / search_compact, the row-chunk loops of GalleryIndex, CompactGalleryIndex and
mutual_ranks, run for MORE THAN ONE iteration.  The chunk sizes (retrieval._INDEX_CHUNK_ROWS = 16384, keyword_neighbors'
default_chunk_rows = thousands of rows at test sizes) are shrunk to 128 rows, so 300 queries go in chunks of 128, 128 and 44: the
output slices ``vals[r0:r1]``, the id slices ``query_ids[r0:r1]``, the ragged last chunk and the reuse of the score scratch and of the
split buffer are all exercised at a small shape.

Data: search_cases.int_case(300, 300, 64, seed) - integers in -3 .. 3, so every score is an exact integer, ties abound and every
route must return the int64 oracle bit for bit - with filter_cases.mod_ids and filter_cases.seeded_live as the filter.  Every
chunked result is also compared bit for bit with the same call made at the stock chunk sizes (one chunk)."""
import functools

import pytest
import torch

import filter_cases as fc
import search_cases as sc_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NQ, N, E, SEED, CHUNK = 300, 300, 64, 20, 128


@functools.lru_cache(maxsize=None)
def _case():
    """-> (q, gal, score int64 [NQ, N], q_ids, g_ids, live) on the CPU"""
    q, gal = sc_cases.int_case(NQ, N, E, SEED)
    q_ids, g_ids = fc.mod_ids(NQ, N)
    return q, gal, q.long() @ gal.long().t(), q_ids, g_ids, fc.seeded_live(N, SEED)


@functools.lru_cache(maxsize=None)
def _want(k: int, filtered: bool):
    _, _, score, q_ids, g_ids, live = _case()
    return fc.filtered_topk(score, k, q_ids, g_ids, live) if filtered else sc_cases.stable_topk(score, k)


def _filter(filtered: bool, q_ids=None):
    """the keyword arguments of a filtered (or an unfiltered) call, on the device"""
    if not filtered:
        return {}
    _, _, _, own_ids, g_ids, live = _case()
    return {"query_ids": (own_ids if q_ids is None else q_ids).to(DEV), "gallery_ids": g_ids.to(DEV), "live": live.to(DEV)}


@pytest.fixture
def chunked(monkeypatch):
    """query and gallery rows go in chunks of 128 on every route -> a function that undoes it"""
    from speechclip_plus_amd import keyword_neighbors, retrieval
    assert retrieval._INDEX_CHUNK_ROWS > NQ and keyword_neighbors.default_chunk_rows(N) > NQ, "the stock sizes give one chunk here"
    monkeypatch.setattr(retrieval, "_INDEX_CHUNK_ROWS", CHUNK)
    monkeypatch.setattr(keyword_neighbors, "default_chunk_rows", lambda V, *args, **kwargs: CHUNK)
    return monkeypatch.undo


def _cpu(out):
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in out)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _search(gallery_kind: str, k: int, route, filtered: bool, q_ids=None):
    from speechclip_plus_amd import GalleryIndex, search
    q, gal = _case()[:2]
    g = gal.float().to(DEV)
    if gallery_kind == "index":
        g = GalleryIndex(g)
    out = _cpu(search(q.float().to(DEV), g, k, route=route, **_filter(filtered, q_ids)))
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int64 and out[0].shape == out[1].shape == (NQ, k)
    return out


# ---------------------------------------------------------------------------------------------------- 1. search, k <= 32
@pytest.mark.parametrize("gallery_kind", ("tensor", "index"))
@pytest.mark.parametrize("filtered", (False, True), ids=("unfiltered", "ids+live"))
@pytest.mark.parametrize("route", ("fused", "composition"))
def test_search_in_three_query_chunks_returns_the_oracle(chunked, route, filtered, gallery_kind):
    for k in (1, 32):
        got = _search(gallery_kind, k, route, filtered)
        assert _same_bits(got, _want(k, filtered)), (route, filtered, gallery_kind, k)
    chunked()
    for k in (1, 32):
        assert _same_bits(_search(gallery_kind, k, route, filtered), _want(k, filtered)), "one chunk"


# ---------------------------------------------------------------------------------------------------- 2. search, k > 32
@pytest.mark.parametrize("filtered", (False, True), ids=("unfiltered", "ids+live"))
@pytest.mark.parametrize("k", (40, 301))
def test_wide_search_in_three_query_chunks_returns_the_oracle(chunked, k, filtered):
    want = _want(k, filtered)
    if k > N:
        assert bool((want[1][:, N:] == -1).all()) and bool((want[0][:, N:] == float("-inf")).all()), "the tail past N is fillers"
    assert _same_bits(_search("tensor", k, None, filtered), want)
    assert _same_bits(_search("index", k, "composition", filtered), want)
    chunked()
    assert _same_bits(_search("tensor", k, None, filtered), want), "one chunk"


# ---------------------------------------------------------------------------------------------------- 3. search_compact
def _compact(fallback: str, filtered: bool):
    from speechclip_plus_amd import search_compact
    q, gal = _case()[:2]
    out = _cpu(search_compact(q.float().to(DEV), gal.float().to(DEV), 5, depth=8, fallback=fallback, **_filter(filtered)))
    assert out[0].shape == out[1].shape == (NQ, 5) and out[2].shape == (NQ,) and out[2].dtype == torch.bool
    return out


@pytest.mark.parametrize("filtered", (False, True), ids=("unfiltered", "ids+live"))
@pytest.mark.parametrize("fallback", ("exact", "none"))
def test_search_compact_in_three_query_chunks(chunked, fallback, filtered):
    """the re-rank of exact integers is exact: with the exact fallback the lists are the oracle's, whichever of the certificate or the
    fallback served a query; with or without it the three outputs are those of the one-chunk call"""
    got = _compact(fallback, filtered)
    if fallback == "exact":
        assert _same_bits(got[:2], _want(5, filtered))
    chunked()
    one = _compact(fallback, filtered)
    assert _same_bits(got, one)
    print(f"fallback {fallback}, filtered {filtered}: certified {int(got[2].sum())} of {NQ}")


@pytest.mark.parametrize("filtered", (False, True), ids=("unfiltered", "ids+live"))
def test_search_compact_with_query_chunks_and_fallback_gallery_chunks(chunked, monkeypatch, filtered):
    from speechclip_plus_amd import retrieval
    monkeypatch.setattr(retrieval, "_FALLBACK_CHUNK_ROWS", CHUNK)
    got = _compact("exact", filtered)
    assert not bool(got[2].all()), "some query must go through the fallback, or its gallery chunks are not run"
    assert _same_bits(got[:2], _want(5, filtered))


# ---------------------------------------------------------------------------------------------------- 4. index construction
def test_indexes_built_in_three_row_chunks_equal_the_one_chunk_build(chunked):
    from speechclip_plus_amd import CompactGalleryIndex, GalleryIndex
    gal = _case()[1].float().to(DEV) * 0.37                      # not bf16 numbers: the split's lower terms and dmax are not zero
    dead = torch.arange(0, N, 3)

    def build():
        index = GalleryIndex(gal, cosine=True)
        compact = CompactGalleryIndex(gal, cosine=True)
        whole = (compact.gmax, compact.gtmax, compact.dmax)
        compact.remove(dead)
        tensors = _cpu((index.split.view(torch.int16), compact.coarse.view(torch.int16), compact.rnorm, compact._row_norms()))
        return tensors, whole, (compact.gmax, compact.gtmax, compact.dmax)
    three = build()
    chunked()
    one = build()
    assert _same_bits(three[0], one[0])
    assert three[1] == one[1] and three[2] == one[2] and three[1][2] > 0.0, (three[1:], one[1:])


def test_mutual_ranks_with_a_split_in_three_row_chunks_equals_the_one_chunk_call(chunked):
    from speechclip_plus_amd import mutual_ranks
    q, gal, _, a_ids, b_ids, _ = _case()

    def ranks():
        out = mutual_ranks(q.float().to(DEV), gal.float().to(DEV), a_ids.to(DEV), b_ids.to(DEV))
        return _cpu(out[key] for key in ("ahead_AB", "ahead_BA", "best_AB", "best_BA"))
    three = ranks()
    chunked()
    assert _same_bits(three, ranks())


# ---------------------------------------------------------------------------------------------------- 5. the negative control
@pytest.mark.parametrize("route", ("fused", "composition", None))
def test_query_ids_shifted_by_one_row_do_not_return_the_oracle(chunked, route):
    """what a wrong ``query_ids[r0:r1]`` slice would give: the comparison above must notice it"""
    k = 40 if route is None else 32
    shifted = torch.roll(_case()[3], 1)
    assert not _same_bits(_search("tensor", k, route, True, q_ids=shifted), _want(k, True))
