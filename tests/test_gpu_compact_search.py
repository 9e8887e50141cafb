"""GPU: compact gallery search (csrc/search_compact.hip through ops.rows_bf16 / search_coarse / search_rerank, retrieval.search_compact,
CompactGalleryIndex, search and KWClip_GeneralTransformer.retrieve) against int64 and fp64 on the CPU.  The cases, the bf16 emulation
and the certificate rule live in tests/compact_cases.py; every expectation and every precondition is computed there, never from a
kernel's own output.  Shapes are the smallest at which the kernels can go wrong: one row / column tile and several, sizes that are no
multiple of the 128-wide tile, one slab and several, E below, at and above one 64-wide K-tile, fewer gallery rows than candidates."""
import pytest
import torch

import compact_cases as cc
import search_cases as sc_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _compact(q, gal, k, D=32, S=None, cosine=False, fallback="exact"):
    from speechclip_plus_amd import search_compact
    vals, idx, cert = search_compact(q.to(DEV), gal.to(DEV), k, cosine=cosine, depth=D, fallback=fallback, slabs=S)
    torch.cuda.synchronize()
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and cert.dtype == torch.bool
    assert vals.shape == idx.shape == (q.shape[0], k) and cert.shape == (q.shape[0],)
    return vals.cpu(), idx.cpu(), cert.cpu()


def _assert_exact(got, want):
    (vals, idx), (wv, wi) = got[:2], want
    assert torch.equal(idx, wi), (idx[(idx != wi).any(dim=1)][:2], wi[(idx != wi).any(dim=1)][:2])
    assert torch.equal(vals, wv)


# ---------------------------------------------------------------------------------------------------- 1. exact, integer data
@pytest.mark.parametrize("S", (1, 2, None))
@pytest.mark.parametrize("nQ,N,E,k", ((1, 63, 64, 1), (65, 129, 64, 10), (130, 1000, 192, 32), (3, 5, 64, 10), (4, 0, 64, 3), (0, 200, 64, 5),
                                      (70, 300, 20, 7)))
def test_integer_data_is_exact_on_both_paths(nQ, N, E, k, S):
    """integers -3 .. 3 are exact in bf16, so the coarse scores equal the int64 product and ties abound: a tie at the edge of the
    candidates cannot be certified, so the certified rows and the exact fallback both have to return the int64 list"""
    q, gal = sc_cases.int_case(nQ, N, E, seed=nQ + N + E)
    want = sc_cases.int_expected(q, gal, k)
    vals, idx, cert = _compact(q.float(), gal.float(), k, S=S)
    print(f"({nQ}, {N}, {E}, k={k}, S={S}): certified {int(cert.sum())} of {nQ}")
    _assert_exact((vals, idx), want)
    if N <= 32:
        assert bool(cert.all())                                        # every gallery row is a candidate
    v2, i2, c2 = _compact(q.float(), gal.float(), k, S=S, fallback="none")
    assert torch.equal(c2, cert)
    _assert_exact((v2[cert], i2[cert]), (want[0][cert], want[1][cert]))


# ---------------------------------------------------------------------------------------------------- 2. unit Gaussian rows
@pytest.mark.parametrize("case", range(len(cc.GAUSS_CASES)))
def test_gaussian_rows_are_certified_and_equal_the_fp64_lists(case):
    q, gal, em, want_vals, want_idx, k, D = cc.gauss_compact(case)
    vals, idx, cert = _compact(q, gal, k, D=D)
    err = (vals.double() - want_vals.float().double()).abs() / cc.ulp32(want_vals.float().double())
    print(f"case {cc.GAUSS_CASES[case]}: certified {int(cert.sum())} of {cert.numel()}, max |vals - fp64| = {float(err.max()):.2f} ulp")
    assert bool(cert.all())
    assert torch.equal(idx, want_idx)
    assert cc.within_ulps(vals, want_vals, 1)
    v2, i2, c2 = _compact(q, gal, k, D=D, fallback="none")
    assert torch.equal(c2, cert) and torch.equal(i2, idx) and torch.equal(v2.view(torch.int32), vals.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 3. the kernels alone
@pytest.mark.parametrize("case", (0, 1))
def test_rows_bf16_and_the_coarse_kernel_alone(case):
    """rows_bf16: the bf16 bits torch rounds to, zero padding, norms within 1 ulp of the fp64 norms.  search_coarse at D = 32: with
    b = (Ep + 8) 2^-24 sum |q~| |g~| (the fp32 accumulation bound, compact_cases.Emulation.acc) every returned value lies within b of
    the fp64 product of the bf16 images at its index, the values do not increase, and no column left out exceeds the last kept value
    by more than twice the bound (its own b plus the last kept column's)"""
    from speechclip_plus_amd import ops
    q, gal, em, _, _, _, _ = cc.gauss_compact(case)
    nQ, N, E, D = q.shape[0], gal.shape[0], q.shape[1], 32
    q16, qn = ops.rows_bf16(q.to(DEV))
    g16, gn = ops.rows_bf16(gal.to(DEV))
    assert q16.shape == (sc_cases.roundup(nQ, 128), em.Ep) and g16.shape == (sc_cases.roundup(N, 128), em.Ep)
    for got, want, n, norms, wn in ((q16, em.qt, nQ, qn, em.qn), (g16, em.gt, N, gn, em.gn)):
        got = got.float().cpu()
        assert torch.equal(got[:n, :E], want) and not bool(got[n:].any()) and not bool(got[:, E:].any())
        assert bool(((norms.cpu().double() - wn.double()).abs() <= cc.ulp32(wn.double())).all())
    vals, idx = ops.search_coarse(q16, g16, nQ, N, D)
    torch.cuda.synchronize()
    vals, idx = vals.cpu(), idx.cpu().long()
    assert bool((idx >= 0).all()) and bool((idx < N).all()) and all(len(set(r)) == D for r in idx.tolist())
    ref, b = torch.gather(em.coarse, 1, idx), torch.gather(em.acc, 1, idx)
    err = (vals.double() - ref).abs()
    print(f"case {cc.GAUSS_CASES[case]}: max |coarse - fp64 of the bf16 images| / bound = {float((err / b).max()):.4f}")
    assert bool((err <= b).all())
    assert bool((vals[:, :-1] >= vals[:, 1:]).all())
    listed = torch.zeros(nQ, N, dtype=torch.bool).scatter_(1, idx, True)
    over = em.coarse - vals[:, -1:].double() - (em.acc + b[:, -1:])
    assert not bool(((over > 0) & ~listed).any())


# ---------------------------------------------------------------------------------------------------- 4. slab invariance, determinism
def test_result_does_not_depend_on_the_slab_count_or_the_run():
    q, gal, _, _, _, k, D = cc.gauss_compact(0)                        # 890 rows: 7 column tiles, the last one partial
    base = _compact(q, gal, k, D=D, S=1)
    for S in (2, 7, None, None):
        vals, idx, cert = _compact(q, gal, k, D=D, S=S)
        assert torch.equal(idx, base[1]) and torch.equal(vals.view(torch.int32), base[0].view(torch.int32)) and torch.equal(cert, base[2]), S


# ---------------------------------------------------------------------------------------------------- 5. a crowd
def test_a_crowd_that_cannot_be_certified_goes_through_the_fallback():
    q, gal, want_idx, k, D = cc.crowd_case()
    vals, idx, cert = _compact(q, gal, k, D=D)
    assert not bool(cert[0]) and bool(cert[1:].all())
    assert torch.equal(idx, want_idx)
    _, _, c2 = _compact(q, gal, k, D=D, fallback="none")
    assert torch.equal(c2, cert)


# ---------------------------------------------------------------------------------------------------- 6. ties across boundaries
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
        for fallback in ("exact", "none"):
            vals, idx, cert = _compact(q.float(), gal.float(), 8, S=slabs, fallback=fallback)
            assert idx[0, :4].tolist() == twins                       # inside the candidates the order never needs the fallback
            if fallback == "exact":
                _assert_exact((vals, idx), want)


# ---------------------------------------------------------------------------------------------------- 7. cosine mode
def test_cosine_mode_on_unnormalised_rows():
    """cosine=True on rows times factors 0.5 .. 4 returns the unit rows' lists.  vals: the contract is the fp64 product of the rows
    SCALED IN FP32 by the reciprocal norms the index holds (inputs of the re-rank, written by ops.vq_prep), rounded once - the
    kernel's fp64 sum runs in another order, so 1 ulp; 2 allowed"""
    from speechclip_plus_amd import CompactGalleryIndex, ops, search_compact
    q, gal, _, want_idx = cc.planted_compact()                         # gaps of 0.05: the fp32 reciprocal norms cannot reorder the lists
    k = want_idx.shape[1]
    qu, gu = sc_cases.unnormalised(q, 1).to(DEV), sc_cases.unnormalised(gal, 2).to(DEV)
    index = CompactGalleryIndex(gu, cosine=True)
    vals, idx, cert = search_compact(qu, index, k, cosine=True)
    assert torch.equal(idx.cpu(), want_idx) and bool(cert.all())
    qs = (qu * ops.vq_prep(qu)[1].unsqueeze(1)).cpu()                  # fl32(q_i * q_scale), as the kernels form it
    gs = (gu * index.rnorm.unsqueeze(1)).cpu()
    ref = torch.gather(qs.double() @ gs.double().t(), 1, want_idx)
    assert cc.within_ulps(vals.cpu(), ref, 2)
    cos = torch.gather(q.double() @ gal.double().t(), 1, want_idx)
    assert float((vals.cpu().double() - cos).abs().max()) < (512 + 8) * 2.0 ** -24      # and they are the unit rows' cosines


# ---------------------------------------------------------------------------------------------------- 8. non-finite inputs
def test_nan_gallery_row_is_uncertified_and_ranks_first():
    q, gal = sc_cases.int_case(66, 300, 64, seed=21)
    galf = gal.float()
    galf[77, 3] = float("nan")
    s = (q.long() @ gal.long().t()).double()
    s[:, 77] = float("inf")                                         # NaN ranks above every number
    wv, wi = sc_cases.stable_topk(s, 6)
    for S in (1, 3):
        vals, idx, cert = _compact(q.float(), galf, 6, S=S)
        assert not bool(cert.any())
        assert bool((idx[:, 0] == 77).all()) and bool(torch.isnan(vals[:, 0]).all())
        assert torch.equal(idx, wi) and torch.equal(vals[:, 1:], wv[:, 1:])


def test_all_nan_query_is_uncertified_and_returns_the_first_k_rows():
    q, gal = sc_cases.int_case(66, 200, 64, seed=22)
    qf = q.float()
    qf[3] = float("nan")
    wv, wi = sc_cases.int_expected(q, gal, 12)
    for S in (1, 2):
        vals, idx, cert = _compact(qf, gal.float(), 12, S=S)
        assert not bool(cert[3])
        assert idx[3].tolist() == list(range(12)) and bool(torch.isnan(vals[3]).all())
        assert bool((idx < 200).all()) and bool((idx >= 0).all())
        keep = torch.arange(66) != 3
        assert torch.equal(idx[keep], wi[keep]) and torch.equal(vals[keep], wv[keep])


# ---------------------------------------------------------------------------------------------------- 9. planted margins, public entries
@pytest.fixture(scope="module")
def model():
    from speechclip_plus_amd import HubertArch, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    torch.manual_seed(7122)
    return KWClip_GeneralTransformer(cfg, device=DEV, hubert_state_dict=random_hubert_state_dict(HubertArch(), seed=7122)).eval()


def test_planted_margins_through_every_public_entry(model):
    from speechclip_plus_amd import CompactGalleryIndex, GalleryIndex, search, search_compact
    q, gal, planted, want = cc.planted_compact()
    k = want.shape[1]
    qd, gd = q.to(DEV), gal.to(DEV)
    index = CompactGalleryIndex(gd, cosine=True)
    assert index.rows.data_ptr() == gd.data_ptr()                      # the fp32 rows are held by reference
    assert index.nbytes == 2 * index.Ep * sc_cases.roundup(2000, 128) + 4 * 2000
    assert (index.N, index.E, index.Ep, index.cosine, len(index)) == (2000, 512, 512, True, 2000) and index.device == gd.device
    assert index.coarse.shape == (sc_cases.roundup(2000, 128), 512) and index.coarse.dtype == torch.bfloat16
    assert 0.99 < index.gtmax < 1.01 and 0.99 < index.gmax < 1.01 and 0.001 < index.dmax < 0.004
    vals, idx, cert = search_compact(qd, index, k, cosine=True)
    print(f"planted: certified {int(cert.sum())} of {cert.numel()}")
    assert torch.equal(idx.cpu()[:, :8], planted) and torch.equal(idx.cpu(), want)
    _, i_old = search(qd, GalleryIndex(gd, cosine=True), k, cosine=True)
    assert torch.equal(idx, i_old)
    v_s, i_s = search(qd, index, k, cosine=True)
    assert torch.equal(i_s, idx) and torch.equal(v_s, vals)
    v_r, i_r = model.retrieve(qd, index, k=k)
    assert torch.equal(i_r, idx)
    plain = CompactGalleryIndex(gal.double().to(DEV))                  # not fp32: the index holds one fp32 copy and counts it
    assert plain.rnorm is None and plain.nbytes == 2 * 512 * sc_cases.roundup(2000, 128) + 4 * 2000 * 512
    assert torch.equal(search_compact(qd, plain, k)[1], idx)
