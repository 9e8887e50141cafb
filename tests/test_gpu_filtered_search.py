"""GPU: filtered gallery search (csrc/search_filter.hip through ops.search_topk_filtered / topk_rows_filtered / search_merge,
retrieval.search / GalleryIndex / hard_negatives and KWClip_GeneralTransformer.retrieve) against int64 and fp64 on the CPU.  The
cases, the rule and the reference live in tests/filter_cases.py; every expectation is computed there, never from a kernel's output.
Shapes are the smallest at which the kernels can go wrong: one tile and several, sizes that are no multiple of 128, one slab and
several, slabs without an admissible column, both routes."""
import pytest
import torch

import filter_cases as fc
import search_cases as sc_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = ("fused", None)                    # None: what ``search`` picks by itself (at these sizes the composition)


def _dev(t):
    return None if t is None else t.to(DEV)


def _search(q, gal, k, S=None, route="fused", q_ids=None, g_ids=None, live=None, cosine=False):
    from speechclip_plus_amd import search
    vals, idx = search(q.to(DEV), gal.to(DEV), k, cosine=cosine, slabs=S, route=route, query_ids=_dev(q_ids), gallery_ids=_dev(g_ids),
                       live=_dev(live))
    torch.cuda.synchronize()
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.shape == idx.shape == (q.shape[0], k)
    return vals.cpu(), idx.cpu()


def _same(got, want) -> bool:
    """the exact criterion: the same rows in the same places and the same values (NaN equal to NaN)"""
    (vals, idx), (wv, wi) = got, want
    return torch.equal(idx, wi) and torch.equal(torch.nan_to_num(vals, nan=12345.0), torch.nan_to_num(wv, nan=12345.0))


def _assert_exact(got, want):
    (vals, idx), (wv, wi) = got, want
    bad = (idx != wi).any(dim=1)
    assert torch.equal(idx, wi), (int(bad.sum()), idx[bad][:2], wi[bad][:2])
    assert _same(got, want)


def _assert_sensitive(got, want, adm):
    """the exact criterion must reject the kernel's own result with one excluded row swapped into position 0 of one list, and with
    one list shifted by one place"""
    vals, idx = got
    rows = torch.nonzero((~adm).any(dim=1) & (idx[:, 0] >= 0)).squeeze(1)
    assert rows.numel() > 0, "no query with an excluded row: the case shows nothing"
    i = int(rows[0])
    j = int(torch.nonzero(~adm[i])[0])
    swapped = idx.clone()
    swapped[i, 0] = j
    assert not _same((vals, swapped), want)
    if idx.shape[1] > 1:
        shifted_i, shifted_v = idx.clone(), vals.clone()
        shifted_i[i] = torch.roll(idx[i], 1)
        shifted_v[i] = torch.roll(vals[i], 1)
        assert not _same((shifted_v, shifted_i), want)


def _filters(nQ, N, seed):
    """the three ways a case is run: ids only, live only, both"""
    q_ids, g_ids = fc.mod_ids(nQ, N)
    live = fc.seeded_live(N, seed)
    return (("ids", q_ids, g_ids, None), ("live", None, None, live), ("both", q_ids, g_ids, live))


# ---------------------------------------------------------------------------------------------------- 1. exact, integer data
@pytest.mark.parametrize("nQ,N,E,k,S", ((1, 63, 64, 1, 1), (65, 129, 64, 10, 2), (130, 1000, 192, 32, 3), (70, 300, 20, 7, 2),
                                         (3, 5, 64, 10, 1), (4, 0, 64, 3, 1), (0, 200, 64, 5, 1)))
def test_integer_data_is_exact(nQ, N, E, k, S):
    q, gal = sc_cases.int_case(nQ, N, E, seed=nQ + N + E)
    score = q.long() @ gal.long().t()
    for name, q_ids, g_ids, live in _filters(nQ, N, seed=N + 1):
        want = fc.filtered_topk(score, k, q_ids, g_ids, live)
        got = _search(q.float(), gal.float(), k, S, q_ids=q_ids, g_ids=g_ids, live=live)
        _assert_exact(got, want)
        _assert_exact(_search(q.float(), gal.float(), k, None, route=None, q_ids=q_ids, g_ids=g_ids, live=live), want)
        if nQ >= 65 and N >= 129:
            _assert_sensitive(got, want, fc.admissible(nQ, N, q_ids, g_ids, live))
    if (nQ, N) == (130, 1000):
        q_ids, g_ids = fc.mod_ids(nQ, N)
        assert fc.excluded_in_unfiltered_topk(score, k, q_ids, g_ids) == nQ       # the filter changes every list of this case


# ---------------------------------------------------------------------------------------------------- 2. fillers in the middle
def test_slabs_without_admissible_columns_merge_exactly():
    nQ, N, E, k, _ = fc.SLAB_CASE
    q, gal, q_ids, g_ids = fc.slab_case()
    want = fc.filtered_topk(q.long() @ gal.long().t(), k, q_ids, g_ids)
    base = None
    for S in (1, 2, 5, None):
        got = _search(q.float(), gal.float(), k, S, q_ids=q_ids, g_ids=g_ids)
        _assert_exact(got, want)
        if base is None:
            base = got
        assert torch.equal(got[1], base[1]) and torch.equal(got[0].view(torch.int32), base[0].view(torch.int32)), S
    _assert_exact(_search(q.float(), gal.float(), k, route=None, q_ids=q_ids, g_ids=g_ids), want)
    _assert_sensitive(base, want, fc.admissible(nQ, N, q_ids, g_ids))


# ---------------------------------------------------------------------------------------------------- 3. nothing admissible
@pytest.mark.parametrize("route", ROUTES)
def test_nothing_admissible_gives_fillers_only(route):
    nQ, N, k = 66, 300, 6
    q, gal = sc_cases.int_case(nQ, N, 64, seed=33)
    score = q.long() @ gal.long().t()
    g_ids = torch.full((N,), 5, dtype=torch.int64)
    q_ids = 100 + torch.arange(nQ, dtype=torch.int64)
    q_ids[0] = 5
    for S in ((1, 3) if route == "fused" else (None,)):
        vals, idx = _search(q.float(), gal.float(), k, S, route=route, q_ids=q_ids, g_ids=g_ids)
        assert bool((idx[0] == -1).all()) and bool((vals[0] == float("-inf")).all())
        wv, wi = sc_cases.int_expected(q, gal, k)                    # the others are unaffected
        assert torch.equal(idx[1:], wi[1:]) and torch.equal(vals[1:], wv[1:])
        _assert_exact((vals, idx), fc.filtered_topk(score, k, q_ids, g_ids))
        vals, idx = _search(q.float(), gal.float(), k, S, route=route, live=torch.zeros(N, dtype=torch.bool))
        assert bool((idx == -1).all()) and bool((vals == float("-inf")).all())


# ---------------------------------------------------------------------------------------------------- 4. a filter that removes nothing
def _nan_row_case():
    q, gal = sc_cases.int_case(66, 300, 64, seed=21)
    galf = gal.float()
    galf[77, 3] = float("nan")
    return q.float(), galf


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", ("gauss", "nan_row"))
def test_a_filter_that_removes_nothing_changes_no_bit(case, route):
    from speechclip_plus_amd import search
    if case == "gauss":
        q, gal, _, _ = sc_cases.gauss_case(130, 890, 512, 31)
        k = 10
    else:
        q, gal = _nan_row_case()
        k = 6
    nQ, N = q.shape[0], gal.shape[0]
    q_ids = -1 - torch.arange(nQ, dtype=torch.int64)                # no gallery id is negative
    g_ids = torch.arange(N, dtype=torch.int64)
    live = torch.ones(N, dtype=torch.bool)
    wv, wi = search(q.to(DEV), gal.to(DEV), k, route=route)         # the unfiltered call
    wv, wi = wv.cpu(), wi.cpu()
    for kwargs in ({"q_ids": q_ids, "g_ids": g_ids}, {"live": live}, {"q_ids": q_ids, "g_ids": g_ids, "live": live}):
        vals, idx = _search(q, gal, k, route=route, **kwargs)
        assert torch.equal(idx, wi), sorted(kwargs)
        assert torch.equal(vals.view(torch.int32), wv.view(torch.int32)), sorted(kwargs)
    if case == "nan_row":
        assert bool((wi[:, 0] == 77).all())


# ---------------------------------------------------------------------------------------------------- 5. 64-bit ids
@pytest.mark.parametrize("route", ROUTES)
def test_ids_are_compared_on_all_64_bits(route):
    nQ, N, k = 70, 300, 12
    q, gal = sc_cases.int_case(nQ, N, 64, seed=55)
    q_ids, g_ids = fc.high_word_ids(nQ), fc.high_word_ids(N)
    want = fc.filtered_topk(q.long() @ gal.long().t(), k, q_ids, g_ids)
    assert bool((want[1] >= 0).all())                                # two thirds of the rows stay: on the low words alone, none would
    got = _search(q.float(), gal.float(), k, 2 if route == "fused" else None, route=route, q_ids=q_ids, g_ids=g_ids)
    _assert_exact(got, want)
    assert bool((g_ids[got[1]] != q_ids.unsqueeze(1)).all())


# ---------------------------------------------------------------------------------------------------- 6. NaN
@pytest.mark.parametrize("route", ROUTES)
def test_nan_gallery_row_is_absent_exactly_where_it_is_inadmissible(route):
    qf, galf = _nan_row_case()
    nQ, N, k = 66, 300, 6
    s = (qf.long() @ torch.nan_to_num(galf).long().t()).double()
    s[:, 77] = float("inf")                                         # NaN ranks above every number
    q_ids, g_ids = fc.mod_ids(nQ, N)                                # row 77 carries id 0: excluded for queries 0, 7, 14, ...
    excl = q_ids == g_ids[77]
    assert 0 < int(excl.sum()) < nQ
    live = torch.ones(N, dtype=torch.bool)
    live[77] = False
    for S in ((1, 3) if route == "fused" else (None,)):
        vals, idx = _search(qf, galf, k, S, route=route, q_ids=q_ids, g_ids=g_ids)
        wv, wi = fc.filtered_topk(s, k, q_ids, g_ids)
        assert torch.equal(idx, wi)
        assert not bool((idx[excl] == 77).any()) and bool((idx[~excl, 0] == 77).all()) and bool(torch.isnan(vals[~excl, 0]).all())
        assert torch.equal(vals[excl], wv[excl]) and torch.equal(vals[~excl, 1:], wv[~excl, 1:])
        vals, idx = _search(qf, galf, k, S, route=route, live=live)  # removed: absent for every query, everything exact
        assert not bool((idx == 77).any())
        _assert_exact((vals, idx), fc.filtered_topk(s, k, live=live))


@pytest.mark.parametrize("route", ROUTES)
def test_all_nan_query_returns_the_first_k_admissible_rows(route):
    nQ, N, k = 66, 200, 12
    q, gal = sc_cases.int_case(nQ, N, 64, seed=22)
    qf = q.float()
    qf[3] = float("nan")
    q_ids, g_ids = fc.mod_ids(nQ, N)
    live = fc.seeded_live(N, 8)
    adm = fc.admissible(nQ, N, q_ids, g_ids, live)
    first = torch.nonzero(adm[3]).squeeze(1)[:k]
    assert first.tolist() != list(range(k))
    wv, wi = fc.filtered_topk(q.long() @ gal.long().t(), k, q_ids, g_ids, live)
    for S in ((1, 2) if route == "fused" else (None,)):
        vals, idx = _search(qf, gal.float(), k, S, route=route, q_ids=q_ids, g_ids=g_ids, live=live)
        assert torch.equal(idx[3], first) and bool(torch.isnan(vals[3]).all())
        keep = torch.arange(nQ) != 3
        assert torch.equal(idx[keep], wi[keep]) and torch.equal(vals[keep], wv[keep])


# ---------------------------------------------------------------------------------------------------- 7. real -inf against fillers
def test_row_kernel_keeps_a_real_minus_inf_ahead_of_the_fillers():
    from speechclip_plus_amd import ops
    V, k = 300, 8
    ninf = float("-inf")
    scores = torch.full((2, V), 100.0)                               # every inadmissible column would win
    live = torch.zeros(V, dtype=torch.bool)
    for col, v in ((3, 1.0), (70, ninf), (130, 2.0), (200, ninf), (290, ninf)):
        scores[:, col] = v
        live[col] = True
    scores[1, 130] = ninf                                            # row 1: one finite entry only
    want = fc.filtered_topk(scores.double(), k, live=live)
    assert want[1].tolist() == [[130, 3, 70, 200, 290, -1, -1, -1], [3, 70, 130, 200, 290, -1, -1, -1]]
    before = scores.clone()
    dscores = scores.to(DEV)
    vals, idx = ops.topk_rows_filtered(dscores, V, k, live=live.to(DEV))
    _assert_exact((vals.cpu(), idx.cpu().long()), want)
    assert torch.equal(dscores.cpu(), before)                        # the matrix is not modified


def test_merge_keeps_a_real_minus_inf_of_a_later_slab_ahead_of_an_earlier_filler():
    from speechclip_plus_amd import ops
    ninf = float("-inf")
    k = 6
    lists = [[(1.0, 5)], [(ninf, 200), (ninf, 210)], [(3.0, 300), (ninf, 310)], []]      # per slab, best first; the rest: no entry
    part = torch.zeros(2, len(lists), k, dtype=torch.int64)
    for s, entries in enumerate(lists):
        for r, (v, c) in enumerate(entries):
            part[0, s, r] = fc.word(v, c)
    part[1, 3, 0] = fc.word(float("nan"), 0)                         # row 1: the all-ones word alone
    vals, idx = ops.search_merge(part.to(DEV), k)
    vals, idx = vals.cpu(), idx.cpu()
    assert idx[0].tolist() == [300, 5, 200, 210, 310, -1]
    assert vals[0].tolist() == [3.0, 1.0, ninf, ninf, ninf, ninf]
    assert idx[1].tolist() == [0, -1, -1, -1, -1, -1] and bool(torch.isnan(vals[1, 0])) and vals[1, 1:].tolist() == [ninf] * 5


@pytest.mark.parametrize("route", ROUTES)
def test_search_keeps_a_real_minus_inf_ahead_of_the_fillers(route):
    """rows whose only non-zero coordinate is +-2^100: exact in bf16 (the lower split terms are zero), the product overflows to -inf in
    fp32 and no NaN arises.  The -inf rows sit in later slabs than a slab's fillers."""
    N, E, k = 300, 64, 6
    big = 2.0 ** 100
    q = torch.zeros(3, E)
    q[0, 0] = big
    gal = torch.zeros(N, E)
    gal[:, 0] = (torch.arange(N) % 5).float()
    for col, v in ((10, 2.0), (140, -big), (150, 1.0), (270, -big)):
        gal[col, 0] = v
    live = torch.zeros(N, dtype=torch.bool)
    live[[10, 140, 150, 270]] = True
    score = (q.double() @ gal.double().t()).float().double()         # what fp32 holds: -2^200 is -inf
    assert bool(torch.isinf(score[0, [140, 270]]).all()) and not bool(torch.isnan(score).any())
    want = fc.filtered_topk(score, k, live=live)
    assert want[1][0].tolist() == [10, 150, 140, 270, -1, -1]
    for S in ((1, 3) if route == "fused" else (None,)):
        _assert_exact(_search(q, gal, k, S, route=route, live=live), want)


# ---------------------------------------------------------------------------------------------------- 8. the row kernel directly
@pytest.mark.parametrize("aligned", (True, False))
@pytest.mark.parametrize("rows,V", ((1, 5), (3, 64), (5, 257), (4, 1000)))
def test_row_kernel_on_tie_heavy_integer_scores(rows, V, aligned):
    from speechclip_plus_amd import ops
    g = torch.Generator().manual_seed(rows * 1000 + V)
    scores = torch.randint(-2, 3, (rows, V), generator=g).float()
    q_ids = torch.arange(rows, dtype=torch.int64) % 3 - 1
    g_ids = torch.randint(-1, 2, (V,), generator=g)
    live = fc.seeded_live(V, V, dead=0.3)
    ld = -(-V // 4) * 4 if aligned else (V + 1 if (V + 1) % 4 else V + 2)    # aligned: ld % 4 == 0; else ld % 4 != 0 and an odd base offset
    assert (ld % 4 == 0) == aligned
    buf = torch.full((rows * ld + 4,), 7.0)
    off = 0 if aligned else 1
    view = buf[off: off + rows * ld].view(rows, ld)[:, :V]
    view.copy_(scores)
    dview = buf.to(DEV)[off: off + rows * ld].view(rows, ld)[:, :V]
    assert (dview.data_ptr() % 16 == 0) == aligned
    for k in (1, 10, 32):
        for kwargs in ({"q_ids": q_ids, "g_ids": g_ids}, {"live": live}, {"q_ids": q_ids, "g_ids": g_ids, "live": live}, {}):
            want = fc.filtered_topk(scores.double(), k, **kwargs)
            vals, idx = ops.topk_rows_filtered(dview, V, k, **{n: t.to(DEV) for n, t in kwargs.items()})
            _assert_exact((vals.cpu(), idx.cpu().long()), want)


# ---------------------------------------------------------------------------------------------------- 9. planted order
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("E", (512, 768))
def test_planted_order_survives_exclusion(E, route):
    q, gal, planted, s64, bound, q_ids, g_ids = fc.planted_filter_case(E)
    vals, idx = _search(q, gal, fc.PLANT_K, route=route, q_ids=q_ids, g_ids=g_ids)
    assert torch.equal(idx, planted[:, 3:10])
    assert bool(((vals.double() - torch.gather(s64, 1, idx)).abs() <= torch.gather(bound, 1, idx)).all())


# ---------------------------------------------------------------------------------------------------- 10. float data, derived bound
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("E", (512, 768))
def test_float_scores_and_lists_within_the_derived_bound(E, route):
    """tests/test_gpu_search.py's criterion with the same bound (6 Ep + 8) 2^-24 sum |q_i| |g_i|, restricted to the admissible rows:
    every returned row is admissible, its score within the bound; a returned row is within 2 * bound of the fp64 k-th best
    admissible score; every admissible row above the weakest returned row by more than 2 * bound is returned."""
    k, nQ, N = 10, 130, 1000
    q, gal, s64, bound = sc_cases.gauss_case(nQ, N, E, 40 + E)
    q_ids, g_ids = fc.mod_ids(nQ, N)
    live = fc.seeded_live(N, 40 + E, dead=0.1)
    adm = fc.admissible(nQ, N, q_ids, g_ids, live)
    vals, idx = _search(q, gal, k, route=route, q_ids=q_ids, g_ids=g_ids, live=live)
    assert bool((idx >= 0).all()) and bool((idx < N).all())
    assert bool(torch.gather(adm, 1, idx).all())
    assert all(len(set(r)) == k for r in idx.tolist())
    s_ret, b_ret = torch.gather(s64, 1, idx), torch.gather(bound, 1, idx)
    err = (vals.double() - s_ret).abs()
    print(f"E={E} route={route}: max |f - s| / bound = {float((err / b_ret).max()):.4f}")
    assert bool((err <= b_ret).all())
    sm = s64.masked_fill(~adm, float("-inf"))
    sv, si = torch.sort(sm, dim=1, descending=True, stable=True)
    kth, b_kth = sv[:, k - 1: k], torch.gather(bound, 1, si[:, k - 1: k])
    assert bool((s_ret >= kth - 2 * torch.minimum(b_ret, b_kth)).all())
    m_s, m_pos = s_ret.min(dim=1, keepdim=True)
    m_b = torch.gather(b_ret, 1, m_pos)
    must = adm & (s64 > m_s + 2 * torch.minimum(bound, m_b))
    listed = torch.zeros(nQ, N, dtype=torch.bool).scatter_(1, idx, True)
    assert not bool((must & ~listed).any())
    assert bool((vals[:, :-1] >= vals[:, 1:]).all())


# ---------------------------------------------------------------------------------------------------- 11. determinism
def test_result_does_not_depend_on_the_slab_count_or_the_run():
    q, gal, _, _ = sc_cases.gauss_case(130, 890, 512, 31)
    q_ids, g_ids = fc.mod_ids(130, 890)
    live = fc.seeded_live(890, 4, dead=0.2)
    base = _search(q, gal, 10, 1, q_ids=q_ids, g_ids=g_ids, live=live)
    for S in (1, 2, 7, None):
        vals, idx = _search(q, gal, 10, S, q_ids=q_ids, g_ids=g_ids, live=live)
        assert torch.equal(idx, base[1]) and torch.equal(vals.view(torch.int32), base[0].view(torch.int32)), S


# ---------------------------------------------------------------------------------------------------- 12. index bookkeeping
def test_remove_and_restore_on_a_built_index():
    from speechclip_plus_amd import GalleryIndex, search
    nQ, N, k = 66, 300, 9
    q, gal = sc_cases.int_case(nQ, N, 64, seed=12)
    score = q.long() @ gal.long().t()
    index = GalleryIndex(gal.float().to(DEV))
    split = index.split.clone()
    dq = q.float().to(DEV)
    v0, i0 = search(dq, index, k)
    _assert_exact((v0.cpu(), i0.cpu()), sc_cases.int_expected(q, gal, k))
    dead = torch.unique(sc_cases.int_expected(q, gal, k)[1][:, 0])[:20]      # rows that lead some list: removing them changes it
    assert index.remove(dead.to(DEV)) is index and index.n_live == N - dead.numel()
    live = torch.ones(N, dtype=torch.bool)
    live[dead] = False
    for route in ROUTES:
        v1, i1 = search(dq, index, k, route=route)
        _assert_exact((v1.cpu(), i1.cpu()), fc.filtered_topk(score, k, live=live))
    assert not torch.equal(i1, i0)
    assert torch.equal(index.split, split)                           # the split is not touched
    index.restore(dead[:5].tolist())
    live[dead[:5]] = True
    v2, i2 = search(dq, index, k)
    _assert_exact((v2.cpu(), i2.cpu()), fc.filtered_topk(score, k, live=live))
    assert index.restore() is index and index.live is None and index.n_live == N
    v3, i3 = search(dq, index, k)
    assert torch.equal(i3, i0) and torch.equal(v3.view(torch.int32), v0.view(torch.int32))
    assert torch.equal(index.split, split)
    ids_index = GalleryIndex(gal.float().to(DEV), ids=(torch.arange(N) % 7).to(DEV))      # an index that brings its ids
    q_ids = torch.arange(nQ) % 7
    v4, i4 = search(dq, ids_index, k, query_ids=q_ids.to(DEV))
    _assert_exact((v4.cpu(), i4.cpu()), fc.filtered_topk(score, k, q_ids, torch.arange(N) % 7))
    v5, i5 = search(dq, ids_index, k)                                # no query ids: no filter
    assert torch.equal(i5, i0)


# ---------------------------------------------------------------------------------------------------- 13. model level
@pytest.fixture(scope="module")
def model():
    from speechclip_plus_amd import HubertArch, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    torch.manual_seed(7122)
    return KWClip_GeneralTransformer(cfg, device=DEV, hubert_state_dict=random_hubert_state_dict(HubertArch(), seed=7122)).eval()


def test_retrieve_passes_the_ids_through(model):
    from speechclip_plus_amd import GalleryIndex, search
    from speechclip_plus_amd.head_tail import unit_rows
    g = torch.Generator().manual_seed(3)
    emb = torch.randn(9, 512, generator=g).to(DEV)
    gallery = torch.randn(300, 512, generator=g).to(DEV)
    q_ids = (torch.arange(9) % 4).to(DEV)
    g_ids = (torch.arange(300) % 4).to(DEV)
    vals, idx = model.retrieve(emb, gallery, 7, query_ids=q_ids, gallery_ids=g_ids)
    wv, wi = search(unit_rows(emb.float()), unit_rows(gallery), 7, query_ids=q_ids, gallery_ids=g_ids)
    assert torch.equal(idx, wi) and torch.equal(vals, wv)
    assert bool((g_ids[idx] != q_ids.unsqueeze(1)).all())
    v0, i0 = model.retrieve(emb, gallery, 7)                         # without ids: today's call
    uv, ui = search(unit_rows(emb.float()), unit_rows(gallery), 7)
    assert torch.equal(i0, ui) and torch.equal(v0, uv) and not torch.equal(i0, idx)
    index = GalleryIndex(gallery, cosine=True, ids=g_ids)            # an index brings its own ids
    v2, i2 = model.retrieve(emb, index, 7, query_ids=q_ids)
    assert torch.equal(i2, wi)


# ---------------------------------------------------------------------------------------------------- 14. hard negatives
def test_hard_negatives_never_return_the_anchors_id():
    from speechclip_plus_amd import hard_negatives
    nA, nB, k = 70, 350, 10
    a, b = sc_cases.int_case(nA, nB, 64, seed=14)
    a_ids = torch.arange(nA, dtype=torch.int64)
    b_ids = torch.arange(nB, dtype=torch.int64) // 5                 # five rows per id, the corpora's shape
    vals, idx = hard_negatives(a.float().to(DEV), b.float().to(DEV), a_ids.to(DEV), b_ids.to(DEV), k)
    vals, idx = vals.cpu(), idx.cpu()
    assert bool((idx >= 0).all()) and bool((b_ids[idx] != a_ids.unsqueeze(1)).all())
    score = a.long() @ b.long().t()
    want = fc.filtered_topk(score, k, a_ids, b_ids)
    _assert_exact((vals, idx), want)
    assert fc.excluded_in_unfiltered_topk(score, k, a_ids, b_ids) > 0
    _assert_sensitive((vals, idx), want, fc.admissible(nA, nB, a_ids, b_ids))
