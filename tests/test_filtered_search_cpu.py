"""Filtered gallery search, the checks that need no GPU: the reference against a brute-force loop, the builders' preconditions, the
new entries declared / bound / exported, the C argument checks, the host layers' refusals and the index bookkeeping."""
import os
import re

import pytest
import torch

import filter_cases as fc
import search_cases as sc_cases

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("sc_search_topk_filtered_bf16", "sc_search_merge_u64", "sc_topk_rows_filtered_f32")


# ---------------------------------------------------------------------------------------------------- the reference and the builders
@pytest.mark.parametrize("mode", ("ids", "live", "both", "neither"))
def test_filtered_topk_equals_the_brute_force_loop(mode):
    q, gal = sc_cases.int_case(7, 40, 64, seed=3)
    score = q.long() @ gal.long().t()
    q_ids, g_ids = fc.mod_ids(7, 40, 3) if mode in ("ids", "both") else (None, None)
    live = fc.seeded_live(40, 5) if mode in ("live", "both") else None
    for k in (1, 5, 32):
        got = fc.filtered_topk(score, k, q_ids, g_ids, live)
        want = fc.brute_force_topk(score, k, q_ids, g_ids, live)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0]), (mode, k)
    if mode == "neither":
        assert all(torch.equal(a, b) for a, b in zip(fc.filtered_topk(score, 5), sc_cases.stable_topk(score, 5)))


def test_filtered_topk_keeps_a_real_minus_inf_ahead_of_the_fillers():
    score = torch.tensor([[1.0, 9.0, float("-inf"), 2.0, float("-inf"), 9.0]], dtype=torch.float64)
    live = torch.tensor([1, 0, 1, 1, 1, 0], dtype=torch.bool)
    vals, idx = fc.filtered_topk(score, 6, live=live)
    assert idx.tolist() == [[3, 0, 2, 4, -1, -1]] and vals[0, :2].tolist() == [2.0, 1.0] and bool(torch.isinf(vals[0, 2:]).all())
    assert all(torch.equal(a, b) for a, b in zip((vals, idx), fc.brute_force_topk(score, 6, live=live)))


def test_slab_case_has_an_empty_and_a_short_slab():
    q, gal, q_ids, g_ids = fc.slab_case()                           # asserts its preconditions
    nQ, N, E, k, S = fc.SLAB_CASE
    assert q.shape == (nQ, E) and gal.shape == (N, E) and set(q_ids.tolist()) == set(fc.SLAB_QUERY_IDS)
    adm = fc.admissible(nQ, N, q_ids, g_ids)
    assert int(adm[0, :128].sum()) == 0 and int(adm[1, 128:256].sum()) == 3 and int(adm[2, 384:].sum()) == 0 and bool(adm[3].all())


def test_every_unfiltered_list_of_the_big_integer_case_holds_an_excluded_row():
    nQ, N, E, k = 130, 1000, 192, 32
    q, gal = sc_cases.int_case(nQ, N, E, seed=nQ + N + E)
    q_ids, g_ids = fc.mod_ids(nQ, N)
    hit = fc.excluded_in_unfiltered_topk(q.long() @ gal.long().t(), k, q_ids, g_ids)
    print(f"{hit} of {nQ} unfiltered top-{k} lists hold an excluded row")
    assert hit == nQ


def test_high_word_ids_differ_only_above_bit_31():
    ids = fc.high_word_ids(30)
    assert ids.dtype == torch.int64 and int(ids.min()) == -5 and len(set(ids.tolist())) == 3
    assert set((ids & 0xffffffff).tolist()) == {(-5) & 0xffffffff}
    adm = fc.admissible(4, 30, fc.high_word_ids(4), ids)
    assert int(adm[0].sum()) == 20                                   # a third excluded; on the low words alone it would be all 30


@pytest.mark.parametrize("E", (512, 768))
def test_planted_filter_case_is_decided_by_the_yardstick(E):
    q, gal, planted, s64, bound, q_ids, g_ids = fc.planted_filter_case(E)      # asserts gap > 4
    gap = fc.planted_filter_gap(E)
    print(f"E={E}: smallest gap over bound among the first {fc.PLANT_K} admissible ranks = {gap:.1f}")
    assert gap > 4.0


def test_list_words_order_like_the_contract():
    inf = float("inf")
    u = lambda v, c: fc.word(v, c) & (2 ** 64 - 1)
    assert u(-inf, 7) > 0 and u(-inf, 7) >> 32 == 0x007fffff
    assert u(float("nan"), 0) == 2 ** 64 - 1
    assert u(0.0, 3) == u(-0.0, 3)
    assert u(1.0, 3) > u(1.0, 4) > u(0.5, 0) > u(-1.0, 0) > u(-inf, 0) > u(-inf, 9)
    assert u(float("nan"), 5) > u(inf, 0)


# ---------------------------------------------------------------------------------------------------- declared, bound, exported
def test_symbols_declared_bound_and_exported():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import _lib, build, ops, retrieval
    header = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.sc_abi_version() == 7
    assert "search_filter.hip" in build.SOURCES
    assert "ADMISSIBLE" in header and "g_ids[j] != q_ids[i]" in header
    for name in ("search_topk_filtered", "topk_rows_filtered", "search_merge"):
        assert callable(getattr(ops, name))
    assert sc.hard_negatives is retrieval.hard_negatives and "hard_negatives" in sc.__all__ and "hard_negatives" in retrieval.__all__


def test_argument_checks_need_no_device():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()
    one = 8                                                          # a non-null, 8-byte aligned address that is never dereferenced

    def fused(nQ, N, K6, k, S, q_ids=None, g_ids=None):
        return lib.sc_search_topk_filtered_bf16(None, None, nQ, N, K6, k, S, q_ids, g_ids, None, None, None)
    assert fused(4, 1000, 384, 0, 1) == -1 and b"k" in lib.sc_last_error()
    assert fused(4, 1000, 384, 33, 1) == -1
    assert fused(4, 1000, 320, 5, 1) == -1 and b"K6" in lib.sc_last_error()
    assert fused(4, 1000, 384, 5, 0) == -1 and b"S" in lib.sc_last_error()
    assert fused(4, 1000, 384, 5, 1, q_ids=one) == -1 and b"one side" in lib.sc_last_error()
    assert fused(4, 1000, 384, 5, 1, g_ids=one) == -1 and b"one side" in lib.sc_last_error()
    assert fused(4, 1000, 384, 5, 1) == -1 and b"null" in lib.sc_last_error()      # everything else passed: the output is missing
    assert fused(0, 1000, 384, 5, 2) == 0                                           # nQ == 0: a no-op, nothing is touched

    def merge(nQ, S, k):
        return lib.sc_search_merge_u64(None, nQ, S, k, None, None, None)
    assert merge(4, 1, 0) == -1 and merge(4, 1, 33) == -1 and merge(4, 0, 5) == -1 and merge(-1, 1, 5) == -1
    assert merge(4, 2, 5) == -1 and b"null" in lib.sc_last_error()
    assert merge(0, 3, 5) == 0

    def rows(n, V, k, ld=None, q_ids=None, g_ids=None):
        return lib.sc_topk_rows_filtered_f32(None, V if ld is None else ld, n, V, k, q_ids, g_ids, None, None, None, None)
    assert rows(3, 100, 0) == -1 and b"k" in lib.sc_last_error()
    assert rows(3, 100, 33) == -1
    assert rows(3, 0, 5) == -1 and rows(3, 100, 5, ld=99) == -1
    assert rows(3, 100, 5, q_ids=one) == -1 and b"one side" in lib.sc_last_error()
    assert rows(3, 100, 5, g_ids=one) == -1 and b"one side" in lib.sc_last_error()
    assert rows(3, 100, 5) == -1 and b"null" in lib.sc_last_error()
    assert rows(0, 100, 5) == 0


# ---------------------------------------------------------------------------------------------------- host layers
def test_host_layers_refuse_cpu_tensors():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import ops
    q, g = torch.zeros(3, 64), torch.zeros(5, 64)
    qi, gi = torch.arange(3), torch.arange(5)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.search(q, g, 2, query_ids=qi, gallery_ids=gi)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.search(q, g, 2, live=torch.ones(5, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.hard_negatives(q, g, qi, gi, 2)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.GalleryIndex(g, ids=gi)
    b = torch.zeros(128, 384, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.search_topk_filtered(b, b, 3, 5, 2, q_ids=qi, g_ids=gi)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_rows_filtered(torch.zeros(3, 8), 5, 2, q_ids=qi, g_ids=gi)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.search_merge(torch.zeros(3, 2, 4, dtype=torch.int64), 4)
    model = sc.KWClip_GeneralTransformer(sc.base_parallel_config(), device="cpu")
    with pytest.raises(RuntimeError, match="device tensors only"):
        model.retrieve(torch.zeros(2, 512), torch.zeros(7, 512), k=3, query_ids=torch.arange(2), gallery_ids=torch.arange(7))


def test_search_validates_the_filter_before_anything_runs():
    import speechclip_plus_amd as sc
    q, g = torch.zeros(3, 64), torch.zeros(5, 64)                    # CPU tensors: a check that passes would end in "device tensors only"
    qi, gi = torch.arange(3), torch.arange(5)
    with pytest.raises(ValueError, match="one side"):
        sc.search(q, g, 2, query_ids=qi)
    with pytest.raises(ValueError, match="one side"):
        sc.search(q, g, 2, gallery_ids=gi)
    with pytest.raises(ValueError, match="query_ids must be torch.int64"):
        sc.search(q, g, 2, query_ids=qi.int(), gallery_ids=gi)
    with pytest.raises(ValueError, match="gallery_ids must be torch.int64"):
        sc.search(q, g, 2, query_ids=qi, gallery_ids=gi.float())
    with pytest.raises(ValueError, match="query_ids has shape"):
        sc.search(q, g, 2, query_ids=torch.arange(4), gallery_ids=gi)
    with pytest.raises(ValueError, match="gallery_ids has shape"):
        sc.search(q, g, 2, query_ids=qi, gallery_ids=torch.arange(6))
    with pytest.raises(ValueError, match="gallery_ids has shape"):
        sc.search(q, g, 2, query_ids=qi, gallery_ids=gi.view(5, 1))
    with pytest.raises(ValueError, match="contiguous"):
        sc.search(q, g, 2, query_ids=torch.arange(6)[::2], gallery_ids=gi)
    with pytest.raises(ValueError, match="live must be"):
        sc.search(q, g, 2, live=torch.ones(5))
    with pytest.raises(ValueError, match="live has shape"):
        sc.search(q, g, 2, live=torch.ones(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="b_ids is required"):
        sc.hard_negatives(q, g, qi, None, 2)
    with pytest.raises(ValueError, match="a_ids is required"):
        sc.hard_negatives(q, g, None, gi, 2)


def _bare(cls, **fields):
    obj = cls.__new__(cls)
    for name, value in fields.items():
        setattr(obj, name, value)
    return obj


def test_compact_index_with_a_filter_is_refused():
    import speechclip_plus_amd as sc
    compact = _bare(sc.CompactGalleryIndex, N=5, E=64)
    q = torch.zeros(3, 64)
    for kwargs in ({"query_ids": torch.arange(3), "gallery_ids": torch.arange(5)}, {"live": torch.ones(5, dtype=torch.bool)},
                   {"query_ids": torch.arange(3)}):
        with pytest.raises(ValueError, match="certificate"):
            sc.search(q, compact, 2, **kwargs)


def test_ops_refuse_a_bad_filter_before_any_launch(monkeypatch):
    """dtype, length and one-sided ids are refused by the ops wrappers themselves; ``is_cuda`` is faked so that the checks behind the
    device test are reached without a device (nothing is launched: every call raises first)"""
    from speechclip_plus_amd import ops

    class Fake(torch.Tensor):
        is_cuda = True

    def fake(t):
        return t.as_subclass(Fake)
    b = fake(torch.zeros(128, 384, dtype=torch.bfloat16))
    qi, gi = fake(torch.arange(3)), fake(torch.arange(5))
    with pytest.raises(ValueError, match="one side"):
        ops.search_topk_filtered(b, b, 3, 5, 2, q_ids=qi)
    with pytest.raises(ValueError, match="g_ids must be torch.int64"):
        ops.search_topk_filtered(b, b, 3, 5, 2, q_ids=qi, g_ids=fake(torch.arange(5).int()))
    with pytest.raises(ValueError, match="q_ids has shape"):
        ops.search_topk_filtered(b, b, 3, 5, 2, q_ids=fake(torch.arange(4)), g_ids=gi)
    with pytest.raises(ValueError, match="contiguous"):
        ops.topk_rows_filtered(fake(torch.zeros(3, 8)), 5, 2, q_ids=qi, g_ids=fake(torch.arange(10)[::2]))
    with pytest.raises(ValueError, match="live must be"):
        ops.topk_rows_filtered(fake(torch.zeros(3, 8)), 5, 2, live=fake(torch.ones(5)))


# ---------------------------------------------------------------------------------------------------- index bookkeeping
def test_gallery_index_remove_restore_and_n_live():
    import speechclip_plus_amd as sc
    index = _bare(sc.GalleryIndex, N=10, E=64, split=torch.zeros(128, 384, dtype=torch.bfloat16), ids=None, live=None)
    assert index.n_live == 10 and index.live is None
    assert index.remove([2, 5]) is index
    assert index.live.dtype == torch.bool and index.live.shape == (10,) and index.n_live == 8
    assert index.live.tolist() == [True, True, False, True, True, False, True, True, True, True]
    live = index.live
    index.remove(torch.tensor([5, 9]))
    assert index.live is live and index.n_live == 7                  # in place
    assert index.restore([5]) is index and index.live is live and index.n_live == 8
    index.remove([])
    assert index.n_live == 8
    for bad in ([10], [-1], torch.tensor([3, 11])):
        with pytest.raises(IndexError):
            index.remove(bad)
        with pytest.raises(IndexError):
            index.restore(bad)
    assert index.n_live == 8
    assert index.restore() is index and index.live is None and index.n_live == 10
    assert index.restore([1]).live is None                           # nothing removed: nothing to restore
    assert torch.equal(index.split, torch.zeros(128, 384, dtype=torch.bfloat16))
