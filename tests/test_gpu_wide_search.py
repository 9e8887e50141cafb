"""GPU: wide search (csrc/topk_wide.hip through ops.topk_rows_wide, retrieval.search / GalleryIndex / hard_negatives and
KWClip_GeneralTransformer.retrieve at k > 32) against the contract restated in plain torch (tests/wide_cases.py), bit for bit in both
``vals`` and ``idx``.  No expectation comes from a kernel's output, except where two kernels are held against each other.  Shapes are the
smallest at which the kernel can go wrong: below, at and above one wave, one 16-byte group, one 1024-column chunk and several, rows that
are and are not 16-byte aligned, every k that pads the sort differently."""
import pytest
import torch

import wide_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = wc.NAN, wc.INF
KS = (33, 64, 100, 1000, 1024)


def _dev(t):
    return None if t is None else t.to(DEV)


def _wide(data, V, k, ld=None, offset=0, q_ids=None, g_ids=None, live=None):
    """ops.topk_rows_wide on ``data`` [rows, V] laid out with pitch ``ld`` at ``offset`` floats off a 16-byte boundary, slack = NaN / +inf"""
    from speechclip_plus_amd import ops
    rows = data.shape[0]
    ld = V if ld is None else ld
    buf, _ = wc.padded(data, ld, offset)
    dbuf = buf.to(DEV)
    assert dbuf.data_ptr() % 16 == 0
    view = torch.as_strided(dbuf, (rows, ld), (ld, 1), offset)
    vals, idx = ops.topk_rows_wide(view, V, k, q_ids=_dev(q_ids), g_ids=_dev(g_ids), live=_dev(live))
    torch.cuda.synchronize()
    assert vals.dtype == torch.float32 and idx.dtype == torch.int32 and vals.shape == idx.shape == (rows, k)
    assert torch.equal(dbuf.cpu().view(torch.int32), buf.view(torch.int32))          # the matrix is not modified
    return vals.cpu(), idx.cpu()


def _first(want, k):
    """the first k places of a restated list of 1024"""
    return want[0][:, :k], want[1][:, :k]


def _assert_bits(got, want, what=""):
    gi, wi = got[1], want[1]
    bad = (gi != wi).any(dim=1)
    assert torch.equal(gi.long(), wi.long()), (what, int(bad.sum()), gi[bad][:1], wi[bad][:1])
    assert wc.same_bits(got, want), what


# ---------------------------------------------------------------------------------------------------- 1. kernel against the restatement
@pytest.mark.parametrize("V", (1, 5, 63, 64, 65, 257, 1000, 4099, 20011))
def test_kernel_equals_the_restatement_for_every_layout(V):
    data = wc.mixed_rows(V, seed=V)
    want = wc.restated_topk(data, V, 1024)                            # V < k: the tail is -inf / -1
    for k in KS:
        for ld in (V, -(-V // 4) * 4, V + 7):
            for offset in (0, 1, 2, 3):
                got = _wide(data, V, k, ld, offset)
                assert bool((got[1] < V).all())                       # slack columns hold NaN and +inf: they would rank first
                _assert_bits(got, _first(want, k), (V, k, ld, offset))


# ---------------------------------------------------------------------------------------------------- 2. ties
def test_a_row_of_one_repeated_value():
    V, k = 20011, 1000
    data = torch.full((3, V), 0.375)
    got = _wide(data, V, k)
    assert got[1].tolist() == [list(range(k))] * 3
    _assert_bits(got, wc.restated_topk(data, V, k))


@pytest.mark.parametrize("k", (100, 1000))
def test_the_boundary_falls_inside_a_long_tie_run(k):
    V = 20011
    data = torch.stack([wc.seven_values(V, seed) for seed in (1, 2, 3)])
    assert int((data == 3.0).sum(dim=1).min()) > 2048                 # the best value alone fills the list more than twice
    for ld, offset in ((V + 1, 0), (V, 1)):
        _assert_bits(_wide(data, V, k, ld, offset), wc.restated_topk(data, V, k), (ld, offset))
    # most of the 3.0 thinned out: their whole run is in (no order needed among them), the boundary lies in the run of 1.0
    data2 = torch.where(data == 3.0, torch.where(torch.arange(V) % 40 == 7, 3.0, -2.0), data)
    n3 = (data2 == 3.0).sum(dim=1)
    assert int(n3.max()) < 1000 and int((data2 == 1.0).sum(dim=1).min()) > 2048
    _assert_bits(_wide(data2, V, 1000), wc.restated_topk(data2, V, 1000))


def test_the_tie_run_starts_before_the_first_admitted_column_and_ends_after_the_last():
    V, k = 20011, 100
    data = torch.full((3, V), 1.25)
    data[:, :3] = -4.0                                                # the run does not start at column 0
    data[:, 5000:5050] = torch.arange(50).float() + 2.0               # 50 larger values in the middle of it
    data[1, 7::2] = 1.0                                               # row 1: every other column of the run is lower
    data[2, V - 1] = 77.0
    got = _wide(data, V, k)
    assert got[1][0].tolist() == list(range(5049, 4999, -1)) + list(range(3, 53))
    _assert_bits(got, wc.restated_topk(data, V, k))
    _assert_bits(_wide(data, V, 1000, V + 5, 3), wc.restated_topk(data, V, 1000))


def test_zeros_nans_and_infinities_rank_by_the_contract():
    V = 300
    g = torch.Generator().manual_seed(5)
    data = torch.where(torch.randint(0, 2, (5, V), generator=g) == 0, 0.0, -0.0)
    data[0, 17] = 1e-30
    data[1, [3, 150, 299]] = NAN                                      # three NaNs at scattered columns
    data[1, 40] = INF
    data[2, ::3] = INF
    data[2, 1::3] = -INF
    data[3] = NAN                                                     # a row that is all NaN
    data[3, 5] = torch.tensor(0x7fc12345, dtype=torch.int32).view(torch.float32)      # with a payload
    data[4] = -INF
    for k in (33, 100, 512):
        got = _wide(data, V, k)
        _assert_bits(got, wc.restated_topk(data, V, k), k)
        assert got[1][1, :4].tolist() == [3, 150, 299, 40]
        assert got[1][3, :33].tolist() == list(range(33)) and got[0].view(torch.int32)[3, 5].item() == 0x7fc12345
        assert got[1][4, :33].tolist() == list(range(33))            # real -inf: its columns, not fillers


def test_a_real_minus_inf_comes_before_the_fillers_under_a_filter():
    V, k = 257, 100
    data = torch.full((3, V), -INF)
    live = torch.ones(V, dtype=torch.bool)
    live[::3] = False                                                 # 171 eligible columns
    live2 = torch.zeros(V, dtype=torch.bool)
    live2[[4, 100, 256]] = True
    got = _wide(data, V, k, live=live)
    assert got[1][0].tolist() == [c for c in range(V) if c % 3][:k]
    _assert_bits(got, wc.restated_topk(data, V, k, live=live))
    got = _wide(data, V, k, live=live2)
    assert got[1][1].tolist() == [4, 100, 256] + [-1] * 97 and bool(torch.isneginf(got[0]).all())
    _assert_bits(got, wc.restated_topk(data, V, k, live=live2))


# ---------------------------------------------------------------------------------------------------- 3. filter
def _filter_case(V, seed):
    g = torch.Generator().manual_seed(seed)
    g_ids = torch.arange(V, dtype=torch.int64) // 5 - 3               # five rows per id, negative ids too
    live = torch.rand(V, generator=g) >= 0.01                         # 1 % dead
    return g_ids, live


@pytest.mark.parametrize("V", (1000, 4099, 20011))
def test_filtered_kernel_equals_the_restatement(V):
    data = wc.mixed_rows(V, seed=V + 1)
    g_ids, live = _filter_case(V, V)
    assert 0 < int((~live).sum()) < V // 20
    q_ids = torch.tensor([0, (V - 1) // 5 - 3, 7, 10 ** 12], dtype=torch.int64)      # the last id is nobody's
    data[0, 15] = 50.0                                                # row 0's best column carries its own id
    data[2, live.logical_not()] = NAN                                 # ineligible NaN columns: they would rank first
    data[3, g_ids == 7] = NAN
    plain = wc.restated_topk(data, V, 1024)
    for mode in ("ids", "live", "both"):
        qi, gi = (q_ids, g_ids) if mode != "live" else (None, None)
        lv = live if mode != "ids" else None
        want = wc.restated_topk(data, V, 1024, qi, gi, lv)
        assert not wc.same_bits(want, plain)
        for k, ld, offset in ((33, V, 0), (100, V + 7, 1), (1000, -(-V // 4) * 4, 0), (1024, V, 2)):
            got = _wide(data, V, k, ld, offset, qi, gi, lv)
            _assert_bits(got, _first(want, k), (mode, k))
            ok = got[1] >= 0
            cols = got[1].long().clamp(min=0)
            if lv is not None:
                assert bool(live[cols][ok].all())
            if qi is not None:
                assert bool((g_ids[cols] != q_ids.unsqueeze(1))[ok].all())
            # an eligible column carries the bits it has in the matrix, which are the bits of the unfiltered call
            assert torch.equal(got[0].view(torch.int32)[ok], torch.gather(data, 1, cols).view(torch.int32)[ok])


def test_fewer_than_k_exactly_k_and_no_eligible_columns():
    V, k = 4099, 100
    data = wc.mixed_rows(V, seed=9)[:3]
    g_ids = torch.zeros(V, dtype=torch.int64)
    g_ids[torch.randperm(V, generator=torch.Generator().manual_seed(1))[:140]] = 1
    g_ids[g_ids.nonzero().squeeze(1)[100:]] = 2                       # 100 columns of id 1, 40 of id 2, the rest id 0
    live = g_ids != 0
    q_ids = torch.tensor([1, 2, 0], dtype=torch.int64)                # row 0: 40 eligible, row 1: exactly 100, row 2: 140
    want = wc.restated_topk(data, V, k, q_ids, g_ids, live)
    assert (want[1] >= 0).sum(dim=1).tolist() == [40, 100, 100]
    _assert_bits(_wide(data, V, k, q_ids=q_ids, g_ids=g_ids, live=live), want)
    none = _wide(data, V, k, live=torch.zeros(V, dtype=torch.bool))
    assert bool((none[1] == -1).all()) and bool(torch.isneginf(none[0]).all())
    everyone = _wide(data, V, k, q_ids=torch.full((3,), 5, dtype=torch.int64), g_ids=torch.full((V,), 5, dtype=torch.int64))
    assert wc.same_bits(everyone, none)


# ---------------------------------------------------------------------------------------------------- 4. against the narrow kernel
def test_consistent_with_the_narrow_kernel_and_with_itself():
    from speechclip_plus_amd import ops
    V = 4099
    data = wc.mixed_rows(V, seed=4)
    d = data.to(DEV)
    for k in (1, 5, 32):
        narrow = ops.topk_rows(d, V, k)
        wide = ops.topk_rows_wide(d, V, k)
        assert wc.same_bits((wide[0].cpu(), wide[1].cpu()), (narrow[0].cpu(), narrow[1].cpu())), k
        _assert_bits((wide[0].cpu(), wide[1].cpu()), wc.restated_topk(data, V, k), k)
    v100, i100 = ops.topk_rows_wide(d, V, 100)
    v32, i32 = ops.topk_rows(d, V, 32)
    assert wc.same_bits((v100[:, :32].cpu(), i100[:, :32].cpu()), (v32.cpu(), i32.cpu()))
    again = ops.topk_rows_wide(d, V, 100)
    assert wc.same_bits((again[0].cpu(), again[1].cpu()), (v100.cpu(), i100.cpu()))
    for k in (33, 1025, 0):                                           # the narrow entries keep their range, the wide one states its own
        if k:
            with pytest.raises(RuntimeError, match="1 <= k <= 32"):
                ops.topk_rows(d, V, k)
        if k != 33:
            with pytest.raises(RuntimeError, match="1 <= k <= 1024"):
                ops.topk_rows_wide(d, V, k)


def test_zero_rows_is_a_no_op():
    from speechclip_plus_amd import ops
    vals = torch.full((0, 100), 7.0, device=DEV)
    v, i = ops.topk_rows_wide(torch.empty(0, 50, device=DEV), 50, 100, vals=vals)
    torch.cuda.synchronize()
    assert v is vals and tuple(i.shape) == (0, 100) and i.dtype == torch.int32


def test_caller_owned_outputs_are_written_in_place():
    from speechclip_plus_amd import ops
    data = wc.mixed_rows(257, seed=2)
    vals = torch.full((6, 64), 7.0, device=DEV)
    idx = torch.full((6, 64), 7, device=DEV, dtype=torch.int32)
    ops.topk_rows_wide(data.to(DEV), 257, 64, vals=vals[1:5], idx=idx[1:5])
    torch.cuda.synchronize()
    _assert_bits((vals[1:5].cpu(), idx[1:5].cpu()), wc.restated_topk(data, 257, 64))
    assert bool((vals[[0, 5]] == 7.0).all()) and bool((idx[[0, 5]] == 7).all())


# ---------------------------------------------------------------------------------------------------- 5. public calls
NQ, N = 130, 3000


@pytest.fixture(scope="module", params=(512, 100), ids=("E512", "E100"))
def case(request):
    """queries, gallery, and - per ``cosine`` - the score matrix ops.cosine_scores_split writes for them, computed once"""
    from speechclip_plus_amd import GalleryIndex, ops
    E = request.param
    g = torch.Generator().manual_seed(E)
    q = (torch.randn(NQ, E, generator=g) * 3).to(DEV)
    gal = (torch.randn(N, E, generator=g) * 0.5).to(DEV)
    gal[11] = gal[10]                                                 # two rows with equal scores against every query
    out = {"q": q, "gal": gal, "E": E}
    for cosine in (False, True):
        index = GalleryIndex(gal, cosine=cosine)
        Np = index.split.shape[0]
        scores = torch.empty(256, Np, device=DEV, dtype=torch.float32)
        rnorm = ops.vq_prep(q)[1] if cosine else None
        ops.cosine_scores_split(q, rnorm, index.split, Np, out=scores)
        torch.cuda.synchronize()
        out[cosine] = (index, scores[:NQ].cpu())
    return out


@pytest.mark.parametrize("cosine", (False, True))
def test_search_equals_the_restatement_over_its_own_scores(case, cosine):
    from speechclip_plus_amd import search
    index, scores = case[cosine]
    want = wc.restated_topk(scores, N, 100)
    for gallery in (case["gal"], index):
        vals, idx = search(case["q"], gallery, 100, cosine=cosine)
        assert vals.dtype == torch.float32 and idx.dtype == torch.int64 and vals.shape == idx.shape == (NQ, 100)
        _assert_bits((vals.cpu(), idx.cpu()), want)
    v2, i2 = search(case["q"], index, 100, cosine=cosine, route="composition")
    assert wc.same_bits((v2.cpu(), i2.cpu()), want)
    v32, i32 = search(case["q"], index, 32, cosine=cosine, route="composition")
    assert wc.same_bits((vals[:, :32].cpu(), idx[:, :32].cpu()), (v32.cpu(), i32.cpu()))


def test_narrow_search_is_what_it_was(case):
    """k <= 32 runs the code and the kernels of before: both routes agree bit for bit, and the lists are the restatement's"""
    from speechclip_plus_amd import search
    index, scores = case[True]
    for k in (5, 32):
        want = wc.restated_topk(scores, N, k)
        for route in ("composition", "fused", None):
            vals, idx = search(case["q"], index, k, cosine=True, route=route)
            _assert_bits((vals.cpu(), idx.cpu()), want, (k, route))


def test_filtered_search_equals_the_restatement_over_the_admissible_rows(case):
    from speechclip_plus_amd import GalleryIndex, hard_negatives, search
    _, scores = case[True]
    g_ids, live = _filter_case(N, 3)
    q_ids = torch.arange(NQ, dtype=torch.int64) * 4 - 3
    want = wc.restated_topk(scores, N, 100, q_ids, g_ids, live)
    vals, idx = search(case["q"], case["gal"], 100, cosine=True, query_ids=_dev(q_ids), gallery_ids=_dev(g_ids), live=_dev(live))
    _assert_bits((vals.cpu(), idx.cpu()), want)
    assert not torch.equal(idx.cpu().int(), wc.restated_topk(scores, N, 100)[1])
    # hard negatives: k = 200, never a row with the anchor's id
    hv, hi = hard_negatives(case["q"], case["gal"], _dev(q_ids), _dev(g_ids), 200, cosine=True)
    hi = hi.cpu()
    assert bool((hi >= 0).all()) and bool((g_ids[hi] != q_ids.unsqueeze(1)).all())
    _assert_bits((hv.cpu(), hi), wc.restated_topk(scores, N, 200, q_ids, g_ids))
    index = GalleryIndex(case["gal"], cosine=True, ids=_dev(g_ids))   # an index brings its own ids
    hv2, hi2 = hard_negatives(case["q"], index, _dev(q_ids), None, 200, cosine=True)
    assert wc.same_bits((hv2.cpu(), hi2.cpu()), (hv.cpu(), hi))


def test_remove_and_restore_at_wide_k(case):
    from speechclip_plus_amd import GalleryIndex, search
    _, scores = case[True]
    index = GalleryIndex(case["gal"], cosine=True)
    plain = wc.restated_topk(scores, N, 100)
    gone = torch.unique(plain[1][:, :3].long().flatten())[:50]        # rows that lead some list
    live = torch.ones(N, dtype=torch.bool)
    live[gone] = False
    index.remove(gone)
    vals, idx = search(case["q"], index, 100, cosine=True)
    assert not bool(torch.isin(idx.cpu(), gone).any())
    _assert_bits((vals.cpu(), idx.cpu()), wc.restated_topk(scores, N, 100, live=live))
    index.restore()
    vals, idx = search(case["q"], index, 100, cosine=True)
    _assert_bits((vals.cpu(), idx.cpu()), plain)


def test_short_gallery_and_refusals_on_the_device(case):
    from speechclip_plus_amd import CompactGalleryIndex, search
    q, gal = case["q"][:5], case["gal"][:40]
    vals, idx = search(q, gal, 64)
    assert bool((idx[:, 40:] == -1).all()) and bool(torch.isneginf(vals[:, 40:]).all())
    assert torch.equal(torch.sort(idx[:, :40], dim=1).values.cpu(), torch.arange(40).expand(5, 40))
    vals, idx = search(q, gal[:0], 64)
    assert bool((idx == -1).all()) and bool(torch.isneginf(vals).all()) and tuple(idx.shape) == (5, 64)
    assert tuple(search(q[:0], gal, 64)[1].shape) == (0, 64)
    with pytest.raises(ValueError, match="at most 32 gallery rows"):
        search(q, gal, 33, route="fused")
    with pytest.raises(ValueError, match="at most 32 gallery rows"):
        search(q, gal, 33, slabs=2)
    with pytest.raises(ValueError, match="GalleryIndex"):
        search(q, CompactGalleryIndex(gal), 33)
    with pytest.raises(ValueError, match="1 <= k <= 1024"):
        search(q, gal, 1025)


# ---------------------------------------------------------------------------------------------------- 6. model level
@pytest.fixture(scope="module")
def model():
    from speechclip_plus_amd import HubertArch, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    torch.manual_seed(7122)
    return KWClip_GeneralTransformer(cfg, device=DEV, hubert_state_dict=random_hubert_state_dict(HubertArch(), seed=7122)).eval()


def test_retrieve_passes_a_wide_k_through(model):
    from speechclip_plus_amd import search
    from speechclip_plus_amd.head_tail import unit_rows
    g = torch.Generator().manual_seed(3)
    emb = torch.randn(9, 512, generator=g).to(DEV)
    gallery = torch.randn(300, 512, generator=g).to(DEV)
    q_ids = (torch.arange(9) % 4).to(DEV)
    g_ids = (torch.arange(300) % 4).to(DEV)
    vals, idx = model.retrieve(emb, gallery, k=64)
    wv, wi = search(unit_rows(emb.float()), unit_rows(gallery), 64)
    assert torch.equal(idx, wi) and torch.equal(vals, wv) and tuple(idx.shape) == (9, 64)
    vals, idx = model.retrieve(emb, gallery, k=64, query_ids=q_ids, gallery_ids=g_ids)
    wv, wi = search(unit_rows(emb.float()), unit_rows(gallery), 64, query_ids=q_ids, gallery_ids=g_ids)
    assert torch.equal(idx, wi) and torch.equal(vals, wv)
    assert bool((g_ids[idx] != q_ids.unsqueeze(1)).all())


# ---------------------------------------------------------------------------------------------------- 7. sensitivity
def test_the_comparison_rejects_a_wrong_order_of_the_kernels_result():
    """host only, on the kernel's result: the bitwise comparison must reject two tied columns swapped, a NaN moved behind a number, and
    a filler put before a real -inf"""
    V, k = 65, 100
    data = torch.round(torch.randn(1, V, generator=torch.Generator().manual_seed(8)) * 2) / 2
    data[0, 20] = NAN
    data[0, 30] = -INF
    want = wc.restated_topk(data, V, k)
    got = _wide(data, V, k)
    _assert_bits(got, want)
    assert got[1][0, 0].item() == 20 and got[1][0, V - 1].item() == 30 and got[1][0, V].item() == -1

    def swapped(a, b):
        v, i = got[0].clone(), got[1].clone()
        v[0, [a, b]] = v[0, [b, a]]
        i[0, [a, b]] = i[0, [b, a]]
        return v, i
    tie = next(p for p in range(1, V - 2) if got[0][0, p] == got[0][0, p + 1])
    assert not wc.same_bits(swapped(tie, tie + 1), want)             # two tied columns swapped: only idx differs
    assert wc.same_bits((swapped(tie, tie + 1)[0], got[1]), want)
    assert not wc.same_bits(swapped(0, 1), want)                     # the NaN behind a number
    assert not wc.same_bits(swapped(V - 1, V), want)                 # a filler before the real -inf: vals are equal, idx is not
    assert torch.equal(swapped(V - 1, V)[0].view(torch.int32), got[0].view(torch.int32))
