"""GPU: gallery search (csrc/search.hip through retrieval.search / GalleryIndex / KWClip_GeneralTransformer.retrieve) against int64 and
fp64 on the CPU.  The cases and the yardstick live in tests/search_cases.py; every expectation is computed there, never from the
kernel's own output.  Shapes are the smallest at which the kernel can go wrong: one row / column tile and several, sizes that are no
multiple of the 128-wide tile, one slab and several, E below and above one 64-wide K-tile."""
import pytest
import torch

import search_cases as sc_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _search(q, gal, k, S=None, cosine=False, route="fused"):
    """``route``: "fused" = the new kernel whatever the size; None = what ``search`` picks by itself (at these sizes the composition)"""
    from speechclip_plus_amd import search
    vals, idx = search(q.to(DEV), gal.to(DEV), k, cosine=cosine, slabs=S, route=route)
    torch.cuda.synchronize()
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.shape == idx.shape == (q.shape[0], k)
    return vals.cpu(), idx.cpu()


def _assert_exact(got, want):
    (vals, idx), (wv, wi) = got, want
    assert torch.equal(idx, wi), (idx[(idx != wi).any(dim=1)][:2], wi[(idx != wi).any(dim=1)][:2])
    assert torch.equal(vals, wv)


# ---------------------------------------------------------------------------------------------------- 1. exact, integer data
@pytest.mark.parametrize("nQ,N,E,k,S", ((1, 63, 64, 1, 1), (65, 129, 64, 10, 2), (130, 1000, 192, 32, 3), (64, 128, 64, 32, None),
                                         (3, 5, 64, 10, 1), (4, 0, 64, 3, 1), (0, 200, 64, 5, 1), (70, 300, 20, 7, 2)))
def test_integer_data_is_exact(nQ, N, E, k, S):
    q, gal = sc_cases.int_case(nQ, N, E, seed=nQ + N + E)
    want = sc_cases.int_expected(q, gal, k)
    _assert_exact(_search(q.float(), gal.float(), k, S), want)
    _assert_exact(_search(q.float(), gal.float(), k, None, route=None), want)        # and by the route search picks itself


def test_integer_data_non_contiguous_query_rows():
    from speechclip_plus_amd import GalleryIndex, search
    q, gal = sc_cases.int_case(2 * 67, 400, 64, seed=5)
    wide = torch.zeros(2 * 67, 96)
    wide[:, :64] = q.float()
    view = wide.to(DEV)[::2, :64]                                   # every other row of a wider buffer: pitch 192, unit column stride
    assert not view.is_contiguous()
    index = GalleryIndex(gal.float().to(DEV))
    want = sc_cases.int_expected(q[::2], gal, 10)
    for S in (1, 2):
        vals, idx = search(view, index, 10, slabs=S)
        _assert_exact((vals.cpu(), idx.cpu()), want)
    vals, idx = search(wide.to(DEV).t()[:64].t(), index, 10)        # the same through a copy-free view of the full rows
    _assert_exact((vals.cpu(), idx.cpu()), sc_cases.int_expected(q, gal, 10))


# ---------------------------------------------------------------------------------------------------- 2. ties across boundaries
def test_identical_rows_across_tiles_and_slabs_come_back_in_index_order():
    q, gal = sc_cases.int_case(66, 600, 64, seed=9)
    S = 2
    nT, T = sc_cases.slab_tiles(600, S)
    twins = [5, 5 + sc_cases.TILE, 5 + T * sc_cases.TILE, 7 + T * sc_cases.TILE]   # one column tile apart, one slab apart, same tile
    assert twins[2] < 600 and twins[2] // sc_cases.TILE // T == 1
    gal[twins] = 3 * torch.sign(q[0]) + (q[0] == 0)                 # bit-identical rows that score highest for query 0
    want = sc_cases.int_expected(q, gal, 8)
    assert want[1][0, :4].tolist() == twins
    for slabs in (1, S, None):
        got = _search(q.float(), gal.float(), 8, slabs)
        assert got[1][0, :4].tolist() == twins
        _assert_exact(got, want)


# ---------------------------------------------------------------------------------------------------- 3. arrival order
@pytest.mark.parametrize("increasing", (True, False))
def test_scores_that_rise_or_fall_with_the_index(increasing):
    q, gal = sc_cases.ramp_case(5, 700, 64, increasing)
    want = sc_cases.int_expected(q, gal, 10)
    assert want[1][0, 0].item() == (699 if increasing else 0)
    for S in (1, 2):
        _assert_exact(_search(q.float(), gal.float(), 10, S), want)


# ---------------------------------------------------------------------------------------------------- 4. NaN
def test_nan_gallery_row_ranks_first_for_every_query():
    q, gal = sc_cases.int_case(66, 300, 64, seed=21)                # integer data: everything but the NaN row is exact
    galf = gal.float()
    galf[77, 3] = float("nan")
    s = (q.long() @ gal.long().t()).double()
    s[:, 77] = float("inf")                                         # NaN ranks above every number
    wv, wi = sc_cases.stable_topk(s, 6)
    for S in (1, 3):
        vals, idx = _search(q.float(), galf, 6, S)
        assert bool((idx[:, 0] == 77).all()) and bool(torch.isnan(vals[:, 0]).all())
        assert torch.equal(idx, wi) and torch.equal(vals[:, 1:], wv[:, 1:])


def test_all_nan_query_returns_the_first_k_rows():
    q, gal = sc_cases.int_case(66, 200, 64, seed=22)                # 200: the second column tile is part padding
    qf = q.float()
    qf[3] = float("nan")
    wv, wi = sc_cases.int_expected(q, gal, 12)
    for S in (1, 2):
        vals, idx = _search(qf, gal.float(), 12, S)
        assert idx[3].tolist() == list(range(12)) and bool(torch.isnan(vals[3]).all())
        assert bool((idx < 200).all()) and bool((idx >= 0).all())
        keep = torch.arange(66) != 3
        assert torch.equal(idx[keep], wi[keep]) and torch.equal(vals[keep], wv[keep])


# ---------------------------------------------------------------------------------------------------- 5. slab invariance, determinism
def test_result_does_not_depend_on_the_slab_count_or_the_run():
    q, gal, _, _ = sc_cases.gauss_case(130, 890, 512, 31)            # 7 column tiles, the last one partial
    base = _search(q, gal, 10, 1)
    for S in (1, 2, 7, None):
        vals, idx = _search(q, gal, 10, S)
        assert torch.equal(idx, base[1]) and torch.equal(vals.view(torch.int32), base[0].view(torch.int32)), S


# ---------------------------------------------------------------------------------------------------- 6. accuracy, float data
@pytest.mark.parametrize("route", ("fused", None))
@pytest.mark.parametrize("E", (512, 768))
def test_float_scores_and_lists_within_the_derived_bound(E, route):
    """bound[q, g] = (6 Ep + 8) 2^-24 sum_i |q_i| |g_i| (search_cases.yardstick), derived, not measured.  With f = the kernel's score
    and s = the fp64 score, |f - s| <= bound per pair.  A returned row j and the fp64 k-th best t: f(j) >= f(t) is not guaranteed,
    but j displaced some row of the fp64 top k, so s(j) >= s(t) - (bound(j) + bound(t)).  A row j that is NOT returned has
    f(j) <= f(m) for the returned row m with the smallest fp64 score, so s(j) <= s(m) + bound(j) + bound(m): every row above that is
    returned.  The test asks for a little more than that derivation gives: "2 * bound" is taken as twice the SMALLER of the two rows'
    bounds, which is at most their sum, so either reading of "2 * bound" holds."""
    k, nQ, N = 10, 130, 1000
    q, gal, s64, bound = sc_cases.gauss_case(nQ, N, E, 40 + E)
    vals, idx = _search(q, gal, k, route=route)
    assert bool((idx >= 0).all()) and bool((idx < N).all())
    assert all(len(set(r)) == k for r in idx.tolist())               # no row is listed twice, none is left out
    s_ret, b_ret = torch.gather(s64, 1, idx), torch.gather(bound, 1, idx)
    err = (vals.double() - s_ret).abs()
    print(f"E={E} route={route}: max |f - s| = {float(err.max()):.3e}, max |f - s| / bound = {float((err / b_ret).max()):.4f}, "
          f"bound max = {float(bound.max()):.3e}")
    assert bool((err <= b_ret).all())
    sv, si = torch.sort(s64, dim=1, descending=True, stable=True)
    kth, b_kth = sv[:, k - 1: k], torch.gather(bound, 1, si[:, k - 1: k])
    assert bool((s_ret >= kth - 2 * torch.minimum(b_ret, b_kth)).all())
    m_s, m_pos = s_ret.min(dim=1, keepdim=True)
    m_b = torch.gather(b_ret, 1, m_pos)
    must = s64 > m_s + 2 * torch.minimum(bound, m_b)                             # [nQ, N]: rows that have to be in the list
    listed = torch.zeros(nQ, N, dtype=torch.bool).scatter_(1, idx, True)
    assert not bool((must & ~listed).any())
    print(f"E={E}: lists equal to the fp64 top-{k} in {int((idx == si[:, :k]).all(dim=1).sum())} of {nQ} rows")
    assert bool((vals[:, :-1] >= vals[:, 1:]).all())                 # best first


# ---------------------------------------------------------------------------------------------------- 7. planted margins
@pytest.mark.parametrize("route", ("fused", None))
@pytest.mark.parametrize("E", (512, 768))
def test_planted_margins_give_the_fp64_order(E, route):
    k = 10
    q, gal, planted, s64, bound = sc_cases.planted_case(70, 1500, E, k, 11)
    _, want = sc_cases.stable_topk(s64, k)
    vals, idx = _search(q, gal, k, route=route)
    assert torch.equal(idx, want) and torch.equal(idx, planted)
    assert bool(((vals.double() - torch.gather(s64, 1, idx)).abs() <= torch.gather(bound, 1, idx)).all())
    vals_c, idx_c = _search(sc_cases.unnormalised(q, 1), sc_cases.unnormalised(gal, 2), k, cosine=True, route=route)
    assert torch.equal(idx_c, want)
    err_c = (vals_c.double() - torch.gather(s64, 1, idx)).abs()
    print(f"E={E}: cosine=True on un-normalised copies: max |cos - fp64| = {float(err_c.max()):.3e}")
    # on top of the score bound: each side's 1 / |x| comes from an fp32 sum of E squares (relative error <= (E / 2 + 2) 2^-24 after
    # the square root) and one rounding of the product x / |x|: (E + 8) 2^-24 for both sides together, times |cos| <= 1
    assert bool((err_c <= torch.gather(bound, 1, idx) + (E + 8) * 2.0 ** -24).all())


# ---------------------------------------------------------------------------------------------------- 8. model level
@pytest.fixture(scope="module")
def model():
    from speechclip_plus_amd import HubertArch, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    torch.manual_seed(7122)
    return KWClip_GeneralTransformer(cfg, device=DEV, hubert_state_dict=random_hubert_state_dict(HubertArch(), seed=7122)).eval()


def test_retrieve_from_waveforms_equals_search_on_the_unit_embeddings(model):
    from speechclip_plus_amd import GalleryIndex, search
    from speechclip_plus_amd.head_tail import unit_rows
    g = torch.Generator().manual_seed(3)
    wavs = [(torch.randn(n, generator=g) * 0.3).to(DEV) for n in (8000, 6500, 8000, 5000, 7200)]
    image_feat = torch.randn(300, 512, generator=g).to(DEV)
    vals, idx = model.retrieve(wavs, image_feat, k=7)
    with torch.no_grad():
        emb = model.encode_speech(wavs)["parallel_audio_feat"]
    wv, wi = search(unit_rows(emb.float()), unit_rows(image_feat), 7)
    assert torch.equal(idx, wi) and torch.equal(vals, wv)
    assert idx.shape == (5, 7) and bool((idx >= 0).all()) and bool((idx < 300).all())
    v2, i2 = model.retrieve(emb, GalleryIndex(image_feat, cosine=True), k=7, src="parallel")     # embeddings in, a prepared index
    assert torch.equal(i2, wi)
    assert model.retrieve(emb, image_feat)[1].shape == (5, max(model.recall_at))                 # k defaults to max(recall_at)


def test_recall_from_retrieved_lists_equals_mutual_retrieval_on_fp64_scores(model):
    from speechclip_plus_amd import mutualRetrieval
    k, nQ, N = 10, 70, 1500
    q, gal, planted, s64, _ = sc_cases.planted_case(nQ, N, 512, k, 11)
    # the correct item of query i is the one planted at rank i % 12: ranks 10 and 11 do not exist, those queries have no correct item
    query_ids = torch.arange(nQ)
    cand_ids = -1 - torch.arange(N)
    for i in range(nQ):
        if i % 12 < k:
            cand_ids[planted[i, i % 12]] = i
    want, _, _ = mutualRetrieval(s64, s64.t().contiguous(), query_ids, cand_ids, list(model.recall_at))
    vals, idx = model.retrieve(q.to(DEV), gal.to(DEV))
    got = sc_cases.recall_from_idx(idx.cpu(), query_ids, cand_ids, model.recall_at)
    print("recall from idx", got, "mutualRetrieval on fp64", want)
    assert set(got) == set(want) and all(abs(got[key] - want[key]) < 1e-9 for key in want)
    assert 0.0 < got["recall@1"] < got["recall@5"] < got["recall@10"] < 100.0
