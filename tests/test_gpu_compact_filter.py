"""GPU: filtered compact gallery search (csrc/search_compact_filter.hip through ops.search_coarse_filtered / search_rerank_filtered,
retrieval.search_compact's filter arguments, CompactGalleryIndex.remove / restore, search, hard_negatives and
KWClip_GeneralTransformer.retrieve) against int64 and fp64 on the CPU.  The cases, the filtered certificate rule and every
precondition live in tests/compact_filter_cases.py; nothing is expected from a kernel's own output.  Shapes are the smallest that
reach more than one column tile, an M tail, fillers inside a slab, a slab past the last tile and both sides of the rule."""
import pytest
import torch

import compact_cases as cc
import compact_filter_cases as cf
import filter_cases as fc
import search_cases as sc_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(t):
    return None if t is None else t.to(DEV)


def _compact(q, gallery, k, D=32, S=None, cosine=False, fallback="exact", q_ids=None, g_ids=None, live=None):
    """search_compact with filter arguments; ``gallery``: a CPU tensor or a CompactGalleryIndex on the device"""
    from speechclip_plus_amd import search_compact
    g = gallery.to(DEV) if isinstance(gallery, torch.Tensor) else gallery
    vals, idx, cert = search_compact(q.to(DEV), g, k, cosine=cosine, depth=D, fallback=fallback, slabs=S, query_ids=_dev(q_ids),
                                     gallery_ids=_dev(g_ids), live=_dev(live))
    torch.cuda.synchronize()
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and cert.dtype == torch.bool
    assert vals.shape == idx.shape == (q.shape[0], k) and cert.shape == (q.shape[0],)
    return vals.cpu(), idx.cpu(), cert.cpu()


def _assert_lists(vals, idx, want_vals64, want_idx, ulps=1):
    """idx equal; vals within ``ulps`` fp32 ulps of the fp64 value rounded once where there is an entry, -inf at a filler"""
    assert torch.equal(idx, want_idx), (idx[(idx != want_idx).any(dim=1)][:2], want_idx[(idx != want_idx).any(dim=1)][:2])
    entry = want_idx >= 0
    assert bool((vals[~entry] == float("-inf")).all())
    assert cc.within_ulps(vals[entry], want_vals64[entry], ulps)


def _assert_admissible(idx, nQ, N, q_ids=None, g_ids=None, live=None):
    adm = fc.admissible(nQ, N, q_ids, g_ids, live)
    assert bool((idx < N).all()) and bool((torch.gather(adm, 1, idx.clamp(min=0)) | (idx < 0)).all())


def _same_bits(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------------- 1. Gaussian rows, both filters
@pytest.mark.parametrize("case", range(len(cc.GAUSS_CASES)))
def test_gaussian_rows_with_ids_and_a_live_mask_are_certified_and_exact(case):
    q, gal, em, q_ids, g_ids, live, want_vals, want_idx, k, D = cf.gauss_filtered(case)
    vals, idx, cert = _compact(q, gal, k, D=D, q_ids=q_ids, g_ids=g_ids, live=live)
    print(f"case {cc.GAUSS_CASES[case]}: certified {int(cert.sum())} of {cert.numel()}")
    assert bool(cert.all())
    _assert_lists(vals, idx, want_vals, want_idx, ulps=1)
    _assert_admissible(idx, q.shape[0], gal.shape[0], q_ids, g_ids, live)
    none = _compact(q, gal, k, D=D, fallback="none", q_ids=q_ids, g_ids=g_ids, live=live)
    assert _same_bits(none, (vals, idx, cert))


# ---------------------------------------------------------------------------------------------------- 2. the coarse entry alone
def _coarse(q, gal, D, S, q_ids=None, g_ids=None, live=None):
    """-> (part [nQ, S, D] int64 on the CPU, merged vals, merged idx)"""
    from speechclip_plus_amd import ops
    q16, _ = ops.rows_bf16(q.float().to(DEV))
    g16, _ = ops.rows_bf16(gal.float().to(DEV)) if gal.shape[0] else (torch.zeros(0, q16.shape[1], device=DEV, dtype=torch.bfloat16), None)
    part = ops.search_coarse_filtered(q16, g16, q.shape[0], gal.shape[0], D, q_ids=_dev(q_ids), g_ids=_dev(g_ids), live=_dev(live), slabs=S)
    vals, idx = ops.search_merge(part, D)
    torch.cuda.synchronize()
    assert part.dtype == torch.int64 and part.dim() == 3 and part.shape[0] == q.shape[0] and part.shape[2] == D
    return part.cpu(), vals.cpu(), idx.cpu().long()


def test_coarse_lists_are_words_with_fillers_in_the_middle_slabs_and_do_not_depend_on_the_slab_count():
    """filter_cases.slab_case: integer data (exact in bf16), ids that empty whole slabs and leave three columns in one"""
    nQ, N, E, D, _ = fc.SLAB_CASE
    q, gal, q_ids, g_ids = fc.slab_case()
    score = q.long() @ gal.long().t()
    wv, wi = fc.filtered_topk(score, D, q_ids, g_ids)
    nT = sc_cases.roundup(N, sc_cases.TILE) // sc_cases.TILE
    base = None
    for S in (1, 2, 5, nT + 3):
        part, vals, idx = _coarse(q, gal, D, S, q_ids, g_ids)
        assert part.shape[1] == S
        assert torch.equal(idx, wi) and torch.equal(vals, wv), S
        base = base if base is not None else (vals, idx)
        assert torch.equal(vals.view(torch.int32), base[0].view(torch.int32)) and torch.equal(idx, base[1])
        _, T = sc_cases.slab_tiles(N, S)
        adm = fc.admissible(nQ, N, q_ids, g_ids)
        for s in range(S):                                           # every slab's own list, word for word
            c0, c1 = min(N, s * T * sc_cases.TILE), min(N, (s + 1) * T * sc_cases.TILE)
            sv, si = fc.filtered_topk(score[:, c0:c1], D, q_ids, g_ids[c0:c1])
            for i in (0, 1, 2, 3, nQ - 1):
                want = [fc.word(float(sv[i, r]), int(si[i, r]) + c0) if int(si[i, r]) >= 0 else 0 for r in range(D)]
                assert part[i, s].tolist() == want, (S, s, i)
            if c0 == c1:
                assert not bool(part[:, s].any())                    # a slab past the last tile is empty
        if S == 5:
            counts = torch.stack([adm[:, s * 128: (s + 1) * 128].sum(dim=1) for s in range(5)], dim=1)
            assert bool((counts[:, 1:4] == 0).any()) and bool((counts[:, 1] == 3).any())      # fillers sit in the middle slabs
            assert bool(((part[:, 1:4] == 0).all(dim=2)).any())


def test_admissible_rows_carry_the_bits_of_the_unfiltered_coarse_kernel():
    """a 32-row gallery at D = 32: the unfiltered list holds every row, so every admissible row's value can be compared bit for bit"""
    from speechclip_plus_amd import ops
    nQ, N, E, D = 70, 32, 64, 32
    q, gal = sc_cases.unit_gauss(nQ, E, 61), sc_cases.unit_gauss(N, E, 62)
    q16, _ = ops.rows_bf16(q.to(DEV))
    g16, _ = ops.rows_bf16(gal.to(DEV))
    uv, ui = ops.search_coarse(q16, g16, nQ, N, D)
    torch.cuda.synchronize()
    uv, ui = uv.cpu(), ui.cpu().long()
    assert bool((torch.sort(ui, dim=1).values == torch.arange(N)).all())
    bits = torch.empty(nQ, N, dtype=torch.int32).scatter_(1, ui, uv.view(torch.int32))          # [query, row] -> the unfiltered bits
    q_ids, g_ids = fc.mod_ids(nQ, N, 3)
    live = fc.seeded_live(N, 63, 0.3)
    adm = fc.admissible(nQ, N, q_ids, g_ids, live)
    _, vals, idx = _coarse(q, gal, D, None, q_ids, g_ids, live)
    n_adm = adm.sum(dim=1)
    assert 0 < int(n_adm.min()) and int(n_adm.max()) < N
    for i in range(nQ):
        n = int(n_adm[i])
        assert sorted(idx[i, :n].tolist()) == torch.nonzero(adm[i]).squeeze(1).tolist() and bool((idx[i, n:] == -1).all())
        assert torch.equal(vals[i, :n].view(torch.int32), bits[i, idx[i, :n]])
        assert bool((vals[i, n:] == float("-inf")).all())
    keep = torch.gather(adm, 1, ui)                                                           # and the unfiltered list's order
    for i in range(nQ):
        assert idx[i, : int(n_adm[i])].tolist() == ui[i][keep[i]].tolist()


def test_ids_that_differ_only_above_bit_31_and_negative_ids_are_told_apart():
    nQ, N, E, D = 66, 300, 64, 32
    q, gal = sc_cases.int_case(nQ, N, E, seed=88)
    score = q.long() @ gal.long().t()
    for q_ids, g_ids in ((fc.high_word_ids(nQ), fc.high_word_ids(N)), (-(torch.arange(nQ) % 4) - 1, -(torch.arange(N) % 4) - 1)):
        adm = fc.admissible(nQ, N, q_ids, g_ids)
        assert 0 < int((~adm).sum(dim=1).min()) and int(adm.sum(dim=1).min()) > D
        wv, wi = fc.filtered_topk(score, D, q_ids, g_ids)
        for S in (1, 3):
            _, vals, idx = _coarse(q, gal, D, S, q_ids, g_ids)
            assert torch.equal(idx, wi) and torch.equal(vals, wv)


def test_empty_operands_and_a_gallery_with_every_row_dead():
    from speechclip_plus_amd import ops
    q, gal = sc_cases.int_case(5, 200, 64, seed=4)
    part, vals, idx = _coarse(q, gal, 8, 2, live=torch.zeros(200, dtype=torch.bool))
    assert not bool(part.any()) and bool((idx == -1).all()) and bool((vals == float("-inf")).all())
    part, vals, idx = _coarse(q, gal[:0], 8, None)
    assert not bool(part.any()) and bool((idx == -1).all()) and bool((vals == float("-inf")).all())
    part, vals, idx = _coarse(q[:0], gal, 8, None, q_ids=torch.zeros(0, dtype=torch.int64), g_ids=torch.arange(200))
    assert part.shape == (0, part.shape[1], 8) and vals.shape == (0, 8)
    for N in (200, 0):                                               # and through the public call: certified empty lists
        vals, idx, cert = _compact(q.float(), gal[:N].float(), 4, live=torch.zeros(N, dtype=torch.bool))
        assert bool(cert.all()) and bool((idx == -1).all()) and bool((vals == float("-inf")).all())
    vals, idx, cert = _compact(q[:0].float(), gal.float(), 4, live=torch.ones(200, dtype=torch.bool))
    assert vals.shape == (0, 4) and cert.shape == (0,)


# ---------------------------------------------------------------------------------------------------- 3. the rule's three branches
@pytest.mark.parametrize("n_live", cf.LIVE_COUNTS)
def test_few_live_rows_are_certified_with_fillers_behind_them(n_live):
    """fallback="none": the lists and the mask are the kernels' own"""
    q, gal, live, want_vals, want_idx, k, D = cf.few_live_case(n_live)
    vals, idx, cert = _compact(q, gal, k, D=D, fallback="none", live=live)
    assert bool(cert.all())
    _assert_lists(vals, idx, want_vals, want_idx, ulps=1)
    assert bool((idx[:, min(k, n_live):] == -1).all()) and bool((idx[:, : min(k, n_live)] >= 0).all())


def test_a_crowd_excluded_by_id_is_certified():
    q, gal, q_ids, g_ids, want_idx, k, D = cf.crowd_filtered(cc.CROWD_N)
    vals, idx, cert = _compact(q, gal, k, D=D, fallback="none", q_ids=q_ids, g_ids=g_ids)
    assert bool(cert.all())                                          # query 0 included: unfiltered it is not (compact_cases.crowd_case)
    assert torch.equal(idx, want_idx)
    _assert_admissible(idx, q.shape[0], gal.shape[0], q_ids, g_ids)


def test_a_crowd_partly_excluded_goes_through_the_filtered_fallback():
    q, gal, q_ids, g_ids, want_idx, k, D = cf.crowd_filtered(cc.CROWD_N - cf.CROWD_LEFT_IN)
    first = cc.CROWD_FIRST + cc.CROWD_N - cf.CROWD_LEFT_IN
    vals, idx, cert = _compact(q, gal, k, D=D, q_ids=q_ids, g_ids=g_ids)
    assert not bool(cert[0]) and bool(cert[1:].all())
    assert idx[0].tolist() == list(range(first, first + k)) and first == 108
    assert torch.equal(idx, want_idx)
    v2, i2, c2 = _compact(q, gal, k, D=D, fallback="none", q_ids=q_ids, g_ids=g_ids)
    assert torch.equal(c2, cert) and torch.equal(i2[1:], idx[1:])
    row = i2[0].tolist()                                             # the best k of its candidates: admissible crowd rows, best first
    assert all(first <= j < cc.CROWD_FIRST + cc.CROWD_N for j in row) and row == sorted(row) and len(set(row)) == k
    assert bool((v2[0, :-1] > v2[0, 1:]).all())


# ---------------------------------------------------------------------------------------------------- 4. a bad row healed
def test_removing_a_nan_row_and_a_huge_row_heals_the_index():
    from speechclip_plus_amd import CompactGalleryIndex
    q, gal, live, want_vals, want_idx, k, D = cf.bad_rows_case()
    gd = gal.to(DEV)
    index = CompactGalleryIndex(gd)
    nbytes = 2 * index.Ep * sc_cases.roundup(300, 128)               # rows held by reference, no rnorm: the coarse copy alone
    assert index.nbytes == nbytes and index.norms is None
    before = (index.gmax, index.gtmax, index.dmax)
    assert not any(torch.isfinite(torch.tensor(before)).tolist())
    first = _compact(q, index, k, D=D, fallback="none")
    assert not bool(first[2].any())                                  # eps is not finite: nothing is certified
    assert index.nbytes == nbytes and index.norms is None            # an index that never had a dead row holds nothing more

    assert index.remove([cf.BAD_HUGE_ROW, cf.BAD_NAN_ROW]) is index and index.n_live == 298
    assert index.norms.shape == (3, 300) and index.nbytes == nbytes + 12 * 300
    assert all(0.9 < v < 1.1 for v in (index.gmax, index.gtmax)) and 0.0 < index.dmax < 0.01
    healed = _compact(q, index, k, D=D, fallback="none")
    assert bool(healed[2].all())
    _assert_lists(healed[0], healed[1], want_vals, want_idx, ulps=1)
    assert not bool(((healed[1] == cf.BAD_NAN_ROW) | (healed[1] == cf.BAD_HUGE_ROW)).any())
    assert _same_bits(_compact(q, index, k, D=D), healed)            # everything certified: the fallback has nothing to do
    from speechclip_plus_amd import search
    v_s, i_s = search(q.to(DEV), index, k)                           # search without filter arguments honours the removed rows
    assert torch.equal(i_s.cpu(), healed[1]) and torch.equal(v_s.cpu().view(torch.int32), healed[0].view(torch.int32))

    fresh = CompactGalleryIndex(gd)                                  # the same mask at call time: the same bits
    assert _same_bits(_compact(q, fresh, k, D=D, fallback="none", live=live), healed)
    assert fresh.live is None and (fresh.gmax, fresh.gtmax, fresh.dmax) != (index.gmax, index.gtmax, index.dmax)
    both = _compact(q, index, k, D=D, fallback="none", live=torch.ones(300, dtype=torch.bool))      # AND with the index's own mask
    assert _same_bits(both, healed)

    assert index.restore() is index and index.live is None
    after = (index.gmax, index.gtmax, index.dmax)
    assert torch.equal(torch.tensor(after).view(torch.int32), torch.tensor(before).view(torch.int32))
    assert _same_bits_nan(_compact(q, index, k, D=D, fallback="none"), first)


def _same_bits_nan(a, b):
    """_same_bits where a list may hold NaN values (any NaN equals any NaN: the default NaN is what the kernels write)"""
    va, vb = a[0], b[0]
    return torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(torch.isnan(va), torch.isnan(vb)) and \
        torch.equal(va[~torch.isnan(va)], vb[~torch.isnan(vb)])


# ---------------------------------------------------------------------------------------------------- 5. the fallback's chunk merge
def test_fallback_merge_keeps_the_contract_across_gallery_chunks(monkeypatch):
    from speechclip_plus_amd import retrieval
    monkeypatch.setattr(retrieval, "_FALLBACK_CHUNK_ROWS", cf.MERGE_CHUNK)
    q, gal, q_ids, g_ids, live, want_vals, want_idx, k = cf.merge_case()
    vals, idx, cert = _compact(q, gal, k, q_ids=q_ids, g_ids=g_ids, live=live)
    assert not bool(cert.any())                                      # the live -inf row makes the gallery bound infinite
    assert torch.equal(idx, want_idx)
    assert torch.equal(vals, want_vals.float())                      # integers and -inf: exact on every path
    odd = idx[1::2]
    assert bool((odd[:, -2] == cf.MERGE_INF_ROW).all()) and bool((odd[:, -1] == -1).all())   # the real -inf ahead of the filler
    assert bool((idx[0::2, -1] == 200).all()) and not bool((idx[0::2] == 600).any())         # equal scores: the lower row
    _assert_admissible(idx, q.shape[0], gal.shape[0], q_ids, g_ids, live)


# ---------------------------------------------------------------------------------------------------- 6. index and host layer
@pytest.fixture(scope="module")
def model():
    from speechclip_plus_amd import HubertArch, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    torch.manual_seed(7122)
    return KWClip_GeneralTransformer(cfg, device=DEV, hubert_state_dict=random_hubert_state_dict(HubertArch(), seed=7122)).eval()


def test_hard_negatives_and_retrieve_on_a_compact_index(model):
    """filter_cases.planted_filter_case(512): gaps of 0.05 decide every list, so the compact route (re-rank values) and the
    GalleryIndex route (fp32 scores) must both return the planted ranks 3 .. 9"""
    from speechclip_plus_amd import CompactGalleryIndex, GalleryIndex, hard_negatives, search_compact
    q, gal, planted, s64, bound, q_ids, g_ids = fc.planted_filter_case(512)
    k = fc.PLANT_K
    qd, gd, qi, gi = q.to(DEV), gal.to(DEV), q_ids.to(DEV), g_ids.to(DEV)
    own = CompactGalleryIndex(gd, cosine=True, ids=gi)
    bare = CompactGalleryIndex(gd, cosine=True)
    assert own.ids is gi and bare.ids is None and own.live is None and own.n_live == 1500
    _, want = hard_negatives(qd, GalleryIndex(gd, cosine=True, ids=gi), qi, None, k, cosine=True)
    assert torch.equal(want.cpu(), planted[:, 3:10])
    for B, b_ids in ((own, None), (bare, gi), (own, gi)):
        vals, idx = hard_negatives(qd, B, qi, b_ids, k, cosine=True)
        assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and torch.equal(idx, want)
    v_r, i_r = model.retrieve(qd, own, k=k, query_ids=qi)
    assert torch.equal(i_r, want)
    v_c, i_c, cert = search_compact(qd, own, k, cosine=True, query_ids=qi)
    assert torch.equal(i_c, want) and float((v_c - v_r).abs().max()) < 1e-6      # retrieve brings the queries to unit length first
    print(f"planted, filtered: certified {int(cert.sum())} of {cert.numel()}")
    own.remove(planted[:, 3])                                        # every query's first remaining row leaves the index
    _, i2, _ = search_compact(qd, own, k - 1, cosine=True, query_ids=qi)
    assert torch.equal(i2.cpu(), planted[:, 4:10]) and own.n_live == 1500 - 70
    own.restore(planted[:5, 3])
    _, i3, _ = search_compact(qd, own, k - 1, cosine=True, query_ids=qi)
    assert torch.equal(i3.cpu()[:5], planted[:5, 3:9]) and torch.equal(i3.cpu()[5:], planted[5:, 4:10])


def test_two_runs_give_equal_bits():
    q, gal, em, q_ids, g_ids, live, _, _, k, D = cf.gauss_filtered(0)
    base = _compact(q, gal, k, D=D, S=1, q_ids=q_ids, g_ids=g_ids, live=live)
    for S in (3, 20, None, None):
        assert _same_bits(_compact(q, gal, k, D=D, S=S, q_ids=q_ids, g_ids=g_ids, live=live), base), S


def test_unfiltered_calls_never_reach_the_new_entries(monkeypatch):
    from speechclip_plus_amd import CompactGalleryIndex, ops, search
    q, gal, em, want_vals, want_idx, k, D = cc.gauss_compact(2)
    assert bool(cc.certificate(em.coarse, em.exact, em.eps, 32, k)[0].all())         # certified at ``search``'s depth too
    index = CompactGalleryIndex(gal.to(DEV), ids=torch.arange(300, device=DEV))      # ids alone are no filter: the call has none
    index.remove([3]).restore()                                                      # nothing is removed any more

    def refuse(*args, **kwargs):
        raise AssertionError("an unfiltered call reached a filtered entry")
    monkeypatch.setattr(ops, "search_coarse_filtered", refuse)
    monkeypatch.setattr(ops, "search_rerank_filtered", refuse)
    vals, idx, cert = _compact(q, index, k, D=D)
    assert bool(cert.all()) and torch.equal(idx, want_idx) and cc.within_ulps(vals, want_vals, 1)
    _, i_s = search(q.to(DEV), index, k)
    assert torch.equal(i_s.cpu(), want_idx[:, :k])
    with pytest.raises(AssertionError, match="reached a filtered entry"):
        _compact(q, index, k, D=D, live=torch.ones(300, dtype=torch.bool))           # and a filtered call does reach them
