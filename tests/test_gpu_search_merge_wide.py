"""GPU: ops.search_merge_lists (csrc/search_merge_wide.hip) alone.  Every expectation comes from CPU torch: a score matrix
[rows, V] is cut into S column ranges, ``wide_cases.restated_topk`` gives the list of every range (local columns: what ``search`` returns
for a shard) and the list over all V columns (what the merge must return, bit for bit - ``wide_cases.same_bits``).

Rows: ``wide_cases.mixed_rows`` (a continuous row, a row of ties, a row with NaN / +-inf / +-0, a 7-value row), a row of V equal values
(the order is purely by global row, across ranges) and a row of V real -inf (entries: every one of them ranks ahead of a filler,
whichever range holds it).  Ranges are of unequal length; at S = 7 one is shorter than most k (fillers inside a list) and at least
one is empty (a list of fillers only)."""
import ctypes
import functools

import pytest
import torch

import wide_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = wc.NAN, wc.INF
FRACTIONS = {1: (0.0, 1.0), 2: (0.0, 0.3, 1.0), 7: (0.0, 0.02, 0.02, 0.3, 0.31, 0.55, 0.9, 1.0)}


def _cuts(V: int, S: int):
    """the S + 1 column cuts of V columns: unequal ranges, at S = 7 a very short one and an empty one"""
    return [int(f * V) for f in FRACTIONS[S]]


@functools.lru_cache(maxsize=None)
def _scores(V: int) -> torch.Tensor:
    """[6, V] on the CPU, never modified"""
    x = torch.empty(6, V)
    x[:4] = wc.mixed_rows(V, 100 + V)
    x[4] = 2.5
    x[5] = -INF
    return x


@functools.lru_cache(maxsize=None)
def _filter(V: int):
    g = torch.Generator().manual_seed(V)
    return torch.arange(6, dtype=torch.int64) % 5, torch.arange(V, dtype=torch.int64) % 5, torch.rand(V, generator=g) > 0.2


def _lists(scores, cuts, k, q_ids=None, g_ids=None, live=None):
    """-> (part_vals [S, rows, k], part_idx [S, rows, k], row0 [S]) on the CPU: the restated list of every column range"""
    pv, pi = [], []
    for c0, c1 in zip(cuts[:-1], cuts[1:]):
        v, i = wc.restated_topk(scores[:, c0:c1].contiguous(), c1 - c0, k, q_ids, None if g_ids is None else g_ids[c0:c1],
                                None if live is None else live[c0:c1])
        pv.append(v)
        pi.append(i)
    return torch.stack(pv), torch.stack(pi), torch.tensor(cuts[:-1], dtype=torch.int64)


def _merge(pv, pi, row0, k, **out):
    from speechclip_plus_amd import ops
    vals, idx = ops.search_merge_lists(pv.to(DEV), pi.to(DEV), row0.to(DEV), k, **out)
    torch.cuda.synchronize()
    assert vals.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(vals.shape) == tuple(idx.shape) == (pv.shape[1], k)
    return vals.cpu(), idx.cpu()


def _assert_bits(got, want):
    if not wc.same_bits(got, want):
        bad = torch.nonzero((got[1].long() != want[1].long()) | (got[0].view(torch.int32) != want[0].view(torch.int32)))
        r, p = bad[0].tolist()
        raise AssertionError(f"{bad.shape[0]} places differ; the first: row {r}, place {p}: got {got[0][r, p].item()} / {got[1][r, p].item()}, "
                             f"want {want[0][r, p].item()} / {want[1][r, p].item()}")


# ---------------------------------------------------------------------------------------------------- 1. the grid
@pytest.mark.parametrize("V", (40, 300, 2500))
@pytest.mark.parametrize("S", (1, 2, 7))
@pytest.mark.parametrize("k", (1, 5, 32, 33, 100, 1024))
def test_merge_equals_the_restated_list_over_all_columns(k, S, V):
    scores, cuts = _scores(V), _cuts(V, S)
    pv, pi, row0 = _lists(scores, cuts, k)
    if S == 7:
        assert bool((pi[1] == -1).all()), "an empty range: a list of fillers only"
        assert k <= cuts[1] or bool((pi[0][:, -1] == -1).all()), "a short range: fillers inside a list"
    _assert_bits(_merge(pv, pi, row0, k), wc.restated_topk(scores, V, k))


def test_equal_values_come_back_in_global_row_order_across_ranges():
    V, k = 300, 100
    pv, pi, row0 = _lists(_scores(V)[4:5], _cuts(V, 7), k)
    vals, idx = _merge(pv, pi, row0, k)
    assert idx[0].tolist() == list(range(k)) and bool((vals == 2.5).all())


def test_a_real_minus_inf_in_the_last_range_ranks_ahead_of_the_fillers_of_the_first():
    k = 8
    scores = torch.tensor([[1.0, 3.0, -INF, 2.0, -INF, -INF]])
    pv, pi, row0 = _lists(scores, [0, 2, 4, 6], k)
    assert pi[0, 0].tolist() == [1, 0] + [-1] * 6 and pi[2, 0].tolist() == [0, 1] + [-1] * 6
    vals, idx = _merge(pv, pi, row0, k)
    assert idx[0].tolist() == [1, 3, 0, 2, 4, 5, -1, -1]
    assert bool(torch.isneginf(vals[0, 3:]).all())
    # a filler is known by its index alone: a filler carrying +inf or NaN as its value stays a filler
    pv[0, 0, 2:] = INF
    pv[1, 0, 2:] = NAN
    _assert_bits(_merge(pv, pi, row0, k), (vals, idx))


# ---------------------------------------------------------------------------------------------------- 2. filtered
@pytest.mark.parametrize("k,S,V", ((5, 7, 40), (33, 7, 300), (100, 2, 2500), (1024, 7, 2500)))
def test_merge_of_filtered_lists(k, S, V):
    scores, (q_ids, g_ids, live) = _scores(V), _filter(V)
    pv, pi, row0 = _lists(scores, _cuts(V, S), k, q_ids, g_ids, live)
    want = wc.restated_topk(scores, V, k, q_ids, g_ids, live)
    assert not wc.same_bits(want, wc.restated_topk(scores, V, k)), "the filter changes the lists"
    _assert_bits(_merge(pv, pi, row0, k), want)


# ---------------------------------------------------------------------------------------------------- 3. the 32-bit row word
@pytest.mark.parametrize("k", (5, 100))
def test_global_rows_up_to_the_largest_legal_one(k):
    V, S = 300, 7
    scores, cuts = _scores(V).clone(), _cuts(V, S)
    scores[0, V - 1] = 1e9                                            # the last column leads a list
    pv, pi, row0 = _lists(scores, cuts, k)
    big = 2 ** 31 - 1 - (cuts[-1] - cuts[-2])                         # the last range's rows end at 2^31 - 2
    row0[-1] = big
    wv, wi = wc.restated_topk(scores, V, k)
    wi = wi.long()
    wi = torch.where(wi >= cuts[-2], wi - cuts[-2] + big, wi)
    assert int(wi.max()) == 2 ** 31 - 2, "the largest legal global row is in some list"
    _assert_bits(_merge(pv, pi, row0, k), (wv, wi.int()))


# ---------------------------------------------------------------------------------------------------- 4. strides, outputs, no-op
def test_a_slice_of_query_rows_of_a_larger_buffer_merges_in_place():
    """shard_stride > nQ k: the other rows of the buffer hold +inf at index 0, the best possible entry - one of them in a result is
    visible at once"""
    from speechclip_plus_amd import ops
    V, S, k = 300, 7, 33
    scores = _scores(V)
    pv, pi, row0 = _lists(scores, _cuts(V, S), k)
    bv = torch.full((S, 11, k), INF)
    bi = torch.zeros(S, 11, k, dtype=torch.int32)
    bv[:, 3:9], bi[:, 3:9] = pv, pi
    bv, bi = bv.to(DEV), bi.to(DEV)
    vals = torch.full((6, k), 7.0, device=DEV)
    idx = torch.full((6, k), 7, device=DEV, dtype=torch.int32)
    out = ops.search_merge_lists(bv[:, 3:9], bi[:, 3:9], row0.to(DEV), k, vals=vals, idx=idx)
    assert out[0] is vals and out[1] is idx
    want = wc.restated_topk(scores, V, k)
    _assert_bits((vals.cpu(), idx.cpu()), want)
    # one row of the slice: the row pitch no longer shows in the tensor, the shard stride does
    one = ops.search_merge_lists(bv[:, 4:5], bi[:, 4:5], row0.to(DEV), k)
    _assert_bits((one[0].cpu(), one[1].cpu()), (want[0][1:2], want[1][1:2]))


def test_no_queries_is_a_no_op_and_the_same_input_gives_the_same_bits():
    from speechclip_plus_amd import _lib, ops
    k, S = 100, 2
    vals = torch.full((4, k), 7.0, device=DEV)
    idx = torch.full((4, k), 7, device=DEV, dtype=torch.int32)
    pv = torch.zeros(S, 4, k, device=DEV)
    pi = torch.zeros(S, 4, k, device=DEV, dtype=torch.int32)
    row0 = torch.zeros(S, device=DEV, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert _lib.lib().sc_search_merge_lists_f32(p(pv), p(pi), 4 * k, p(row0), 0, S, k, p(vals), p(idx), None) == 0
    torch.cuda.synchronize()
    assert bool((vals == 7.0).all()) and bool((idx == 7).all()), "nQ = 0 leaves the outputs untouched"
    v0, i0 = ops.search_merge_lists(pv[:, :0], pi[:, :0], row0, k)
    assert tuple(v0.shape) == tuple(i0.shape) == (0, k)
    lists = _lists(_scores(2500), _cuts(2500, 7), 1024)
    a, b = _merge(*lists, 1024), _merge(*lists, 1024)
    assert wc.same_bits(a, b)


# ---------------------------------------------------------------------------------------------------- 5. sensitivity
def test_the_comparison_notices_a_merge_by_local_rows():
    """what forgetting ``row0`` would give: equal values ordered by the row inside the shard - the comparison above must notice"""
    V, k = 300, 100
    scores, cuts = _scores(V), _cuts(V, 7)
    pv, pi, row0 = _lists(scores, cuts, k)
    got = _merge(pv, pi, torch.zeros_like(row0), k)
    assert not wc.same_bits(got, wc.restated_topk(scores, V, k))
