"""GPU: the identities between the gallery-search entry points that share a kernel body (csrc/search_kernels.h, csrc/topk_rows.h).
The split and the compact scan are one kernel at two row widths, the filtered entries with no filter are the unfiltered ones, and the
two re-ranks differ in one clause of the certificate.  Each test holds two entries against each other bit for bit on one input; what
the lists must BE is the business of test_gpu_search / _filtered_search / _compact_search / _compact_filter / _keyword_neighbors.

Input: 130 queries (two row tiles, the second with two rows: three of its waves have nothing to scan) x 300 gallery rows (three
column tiles, the last partial) x 384, small integers - exact in bf16 and in every fp32 sum, so equal scores occur - with repeated
rows inside and across column tiles, one NaN gallery row and one all-zero row."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NQ, N, E = 130, 300, 384
NAN_ROW, ZERO_ROW = 140, 3


@functools.lru_cache(maxsize=None)
def _rows():
    """-> (queries [NQ, E], gallery [N, E]) fp32 on the CPU; read only"""
    g = torch.Generator().manual_seed(19)
    q = torch.randint(-2, 3, (NQ, E), generator=g).float()
    gal = torch.randint(-2, 3, (N, E), generator=g).float()
    gal[6] = gal[5]                  # equal scores inside a column tile ...
    gal[200] = gal[5]                # ... and across two
    gal[299] = gal[130]
    gal[NAN_ROW] = float("nan")
    gal[ZERO_ROW] = 0.0
    return q, gal


@functools.lru_cache(maxsize=None)
def _operands():
    """the rows as bf16 [rows padded to 128, 384] on the device: a K6 = 384 split for search_topk, Ep = 384 rows for search_coarse"""
    out = []
    for x in _rows():
        t = torch.zeros(-(-x.shape[0] // 128) * 128, E, dtype=torch.bfloat16)
        t[: x.shape[0]] = x.to(torch.bfloat16)
        assert torch.equal(t[: x.shape[0]].float().nan_to_num(7.0), x.nan_to_num(7.0))      # exact
        out.append(t.to(DEV))
    return tuple(out)


def _ids_and_mask():
    g = torch.Generator().manual_seed(20)
    q_ids = (torch.arange(NQ) % 7).to(DEV)
    g_ids = (torch.arange(N) % 7).to(DEV)
    live = (torch.rand(N, generator=g) < 0.5).to(torch.uint8).to(DEV)
    return q_ids, g_ids, live


def _inert_filter():
    """ids that never match and a mask of ones"""
    return torch.arange(NQ, device=DEV), -1 - torch.arange(N, device=DEV), torch.ones(N, dtype=torch.uint8, device=DEV)


def _bits(t):
    t = t.cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _slab_lists(entry, k, S):
    """the per-slab lists as the C entry writes them (ops merges them away): (part_vals, part_idx) [NQ, S, k]"""
    from speechclip_plus_amd import ops
    from speechclip_plus_amd._lib import check, lib
    q16, g16 = _operands()
    pv = torch.full((NQ, S, k), 7.0, device=DEV)
    pi = torch.full((NQ, S, k), 7, device=DEV, dtype=torch.int32)
    fn = getattr(lib(), entry)
    check(fn(ops._p(q16), ops._p(g16), NQ, N, E, k, S, ops._p(pv), ops._p(pi), ops._stream()), entry)
    torch.cuda.synchronize()
    return pv, pi


def _slab_words(entry, k, S, q_ids, g_ids, live):
    """the per-slab list words as the C entry writes them: part [NQ, S, k] int64"""
    from speechclip_plus_amd import ops
    from speechclip_plus_amd._lib import check, lib
    q16, g16 = _operands()
    part = torch.full((NQ, S, k), 7, device=DEV, dtype=torch.int64)
    fn = getattr(lib(), entry)
    check(fn(ops._p(q16), ops._p(g16), NQ, N, E, k, S, ops._p(q_ids), ops._p(g_ids), ops._p(live), ops._p(part), ops._stream()), entry)
    torch.cuda.synchronize()
    return part.cpu()


# ---------------------------------------------------------------------------------------------------- 1. same scan, two entries
@pytest.mark.parametrize("k", [1, 32])
def test_split_and_compact_scan_write_the_same_slab_lists(k):
    for S in (1, 2):
        a = _slab_lists("sc_search_topk_bf16", k, S)
        b = _slab_lists("sc_search_coarse_bf16", k, S)
        assert _same(a, b), (k, S)
        assert bool((a[1][:, 0, 0] == NAN_ROW).all())                # the lists are lists: NaN on top of the first slab's


@pytest.mark.parametrize("k", [1, 32])
def test_filtered_split_and_compact_scan_write_the_same_words(k):
    q_ids, g_ids, live = _ids_and_mask()
    for S in (1, 2, 4):                                              # S = 4: three column tiles, the last slab is empty
        a = _slab_words("sc_search_topk_filtered_bf16", k, S, q_ids, g_ids, live)
        b = _slab_words("sc_search_coarse_filtered_bf16", k, S, q_ids, g_ids, live)
        assert torch.equal(a, b), (k, S)
        assert bool((a[:, 0, 0] != 0).all())
        if S == 4:
            assert not bool(a[:, 3].any())


# ---------------------------------------------------------------------------------------------------- 2. no filter = unfiltered
@pytest.mark.parametrize("k", [1, 32])
def test_filtered_entries_with_no_filter_or_an_inert_one_give_the_unfiltered_lists(k):
    from speechclip_plus_amd import ops
    q16, g16 = _operands()
    for S in (1, 2):
        for name, unfiltered, filtered in (
                ("split", lambda: ops.search_topk(q16, g16, NQ, N, k, slabs=S),
                 lambda **f: ops.search_topk_filtered(q16, g16, NQ, N, k, slabs=S, **f)),
                ("compact", lambda: ops.search_coarse(q16, g16, NQ, N, k, slabs=S),
                 lambda **f: ops.search_merge(ops.search_coarse_filtered(q16, g16, NQ, N, k, slabs=S, **f), k))):
            want = unfiltered()
            none = filtered()
            q_ids, g_ids, live = _inert_filter()
            inert = filtered(q_ids=q_ids, g_ids=g_ids, live=live)
            torch.cuda.synchronize()
            assert want[1].dtype == none[1].dtype == inert[1].dtype == torch.int32
            assert _same(want, none), (name, k, S)
            assert _same(want, inert), (name, k, S)


# ---------------------------------------------------------------------------------------------------- 3. row selection
def _score_rows(rows, V, ld, offset, seed):
    """[rows, V] integer scores from {0, 1, 2} with pitch ld, the base ``offset`` floats behind a 16-byte boundary.  From six rows on,
    row 4 is constant (with 16-byte loads a lane owns four consecutive columns: the first eight lanes run empty at k = 32) and row 5
    has its 2s in the columns 0, 64, 128, ... (with element loads they all belong to lane 0): both make lanes refill"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((rows * ld + 4,), 9.0)
    m = buf[offset: offset + rows * ld].view(rows, ld)
    m[:, :V] = torch.randint(0, 3, (rows, V), generator=g).float()
    if rows >= 6:
        m[4, :V] = 1.0
        m[5, :V] = torch.randint(0, 2, (V,), generator=g).float()
        m[5, 0:V:64] = 2.0
    d = buf.to(DEV)
    out = d[offset: offset + rows * ld].view(rows, ld)
    assert out.data_ptr() % 16 == 4 * offset
    return out


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("k", [1, 32])
def test_row_selection_with_no_filter_is_topk_rows(k, offset):
    from speechclip_plus_amd import ops
    for rows, V, ld in ((6, 1000, 1000), (2, 5, 8), (2, 257, 260)):
        scores = _score_rows(rows, V, ld, offset, seed=V)
        want = ops.topk_rows(scores, V, k)
        got = ops.topk_rows_filtered(scores, V, k)
        torch.cuda.synchronize()
        assert _same(want, got), (V, k, offset)
        n = min(k, V)
        sv, si = torch.sort(scores.cpu()[:, :V], dim=1, descending=True, stable=True)           # no NaN, no -0: the contract
        assert torch.equal(want[1].cpu()[:, :n].long(), si[:, :n]) and torch.equal(want[0].cpu()[:, :n], sv[:, :n]), (V, k, offset)
        assert bool((want[1][:, n:] == -1).all()) and bool((want[0][:, n:] == float("-inf")).all())


# ---------------------------------------------------------------------------------------------------- 4. re-rank
def _rerank(rows, cand_idx, cand_vals, eps, k):
    """both entries on the same candidates -> ((vals, idx, certified) unfiltered, the same filtered), on the CPU"""
    from speechclip_plus_amd import ops
    q = _rows()[0].to(DEV)
    args = (q, None, rows.to(DEV), None, cand_idx.to(DEV), cand_vals.to(DEV), eps.to(DEV), k)
    a = ops.search_rerank(*args)
    b = ops.search_rerank_filtered(*args)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in a), tuple(t.cpu() for t in b)


def _candidates(D, n_fill):
    """per query the D - n_fill best finite gallery rows by the exact integer score, -1 / -inf behind them"""
    q, gal = _rows()
    score = q.double() @ gal.nan_to_num(0.0).double().t()
    score[:, NAN_ROW] = float("-inf")
    v, i = torch.sort(score, dim=1, descending=True, stable=True)
    cand_idx = torch.full((NQ, D), -1, dtype=torch.int32)
    cand_vals = torch.full((NQ, D), float("-inf"))
    cand_idx[:, : D - n_fill] = i[:, : D - n_fill].int()
    cand_vals[:, : D - n_fill] = v[:, : D - n_fill].float()
    return cand_idx, cand_vals


def test_rerank_entries_agree_on_full_lists():
    """N = 300 > D = 8, every candidate valid: the two certificates are the same test"""
    cand_idx, cand_vals = _candidates(8, 0)
    eps = torch.where(torch.arange(NQ) % 2 == 0, 0.0, 1e9).float()   # odd queries cannot certify
    a, b = _rerank(_rows()[1], cand_idx, cand_vals, eps, 1)
    assert _same(a, b)
    assert torch.equal(a[1][:, 0], cand_idx[:, 0]) and torch.equal(a[0][:, 0], cand_vals[:, 0])     # integer scores: exact
    cert = a[2].bool()
    assert not bool(cert[1::2].any())
    e_k, t = cand_vals[:, 0].double(), cand_vals[:, 7].double()
    strict = e_k - e_k.abs() * 2.0 ** -23 > t
    assert torch.equal(cert[0::2], strict[0::2]) and bool(cert.any())


def test_rerank_entries_both_certify_a_gallery_smaller_than_the_list():
    """N = 5 <= D = 8, three fillers: every gallery row is a candidate under either clause"""
    cand_idx = torch.tensor([[4, 2, 0, 1, 3, -1, -1, -1]], dtype=torch.int32).repeat(NQ, 1)
    rows = _rows()[1][:5]
    cand_vals = torch.cat([torch.gather(_rows()[0] @ rows.t(), 1, cand_idx[:, :5].long()), torch.full((NQ, 3), float("-inf"))], dim=1)
    a, b = _rerank(rows, cand_idx, cand_vals, torch.zeros(NQ), 8)
    assert _same(a, b)
    assert bool(a[2].bool().all())
    assert bool((a[0][:, 5:] == float("-inf")).all()) and bool((a[1][:, 5:] == -1).all())
    assert torch.equal(a[1][:, :5].sort(dim=1).values, torch.arange(5, dtype=torch.int32).repeat(NQ, 1))


def test_rerank_entries_differ_only_on_a_short_list_of_a_large_gallery():
    """N = 300, D = 8, two fillers: unfiltered N > D and n_valid != D - no certificate; filtered n_valid < D - every admissible row is
    a candidate.  The one place the two clauses differ."""
    cand_idx, cand_vals = _candidates(8, 2)
    a, b = _rerank(_rows()[1], cand_idx, cand_vals, torch.zeros(NQ), 3)
    assert _same(a[:2], b[:2])
    assert torch.equal(a[1], cand_idx[:, :3])
    assert not bool(a[2].any()) and bool(b[2].bool().all())
