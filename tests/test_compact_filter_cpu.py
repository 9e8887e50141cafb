"""Filtered compact gallery search, the checks that need no GPU: the new entries declared / bound / exported, the C argument checks,
the host layers' refusals (every one before a launch), the index bookkeeping and its bounds over live rows, the builders'
preconditions, and the certificate rule restated over the admissible rows (mirrored in tests/compact_filter_cases.py): it never
certifies a list that differs from the fp64 filtered list."""
import inspect
import os
import re

import pytest
import torch

import compact_cases as cc
import compact_filter_cases as cf
import filter_cases as fc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("sc_search_coarse_filtered_bf16", "sc_search_rerank_filtered_f32")


def _bare(cls, **fields):
    obj = cls.__new__(cls)
    for name, value in fields.items():
        setattr(obj, name, value)
    return obj


class Fake(torch.Tensor):
    is_cuda = True


def fake(t):
    """``is_cuda`` is faked so that the checks behind the device test are reached without a device (every call raises first)"""
    return t.as_subclass(Fake)


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
    assert "search_compact_filter.hip" in build.SOURCES
    assert "CERTIFICATE OVER ADMISSIBLE ROWS" in header and "fewer than D entries" in header
    assert callable(ops.search_coarse_filtered) and callable(ops.search_rerank_filtered)
    assert list(inspect.signature(ops.search_coarse_filtered).parameters) == ["q_bf16", "g_bf16", "nQ", "N", "D", "q_ids", "g_ids", "live", "slabs"]
    params = inspect.signature(sc.search_compact).parameters
    assert list(params) == ["queries", "gallery", "k", "cosine", "depth", "fallback", "slabs", "query_ids", "gallery_ids", "live"]
    assert all(params[n].kind is inspect.Parameter.KEYWORD_ONLY and params[n].default is None for n in ("query_ids", "gallery_ids", "live"))
    assert list(inspect.signature(sc.CompactGalleryIndex.__init__).parameters) == ["self", "gallery", "cosine", "ids"]
    for name in ("remove", "restore", "n_live"):
        assert hasattr(sc.CompactGalleryIndex, name)
    assert sc.search_compact is retrieval.search_compact


def test_argument_checks_need_no_device():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()
    one = 8                                                          # a non-null, 8-byte aligned address that is never dereferenced

    def coarse(nQ, N, Ep, D, S, q_ids=None, g_ids=None):
        return lib.sc_search_coarse_filtered_bf16(None, None, nQ, N, Ep, D, S, q_ids, g_ids, None, None, None)
    assert coarse(4, 1000, 512, 0, 1) == -1 and b"D" in lib.sc_last_error()
    assert coarse(4, 1000, 512, 33, 1) == -1
    assert coarse(4, 1000, 96, 5, 1) == -1 and b"Ep" in lib.sc_last_error()
    assert coarse(4, 1000, 512, 5, 0) == -1 and b"S" in lib.sc_last_error()
    assert coarse(-1, 1000, 512, 5, 1) == -1
    assert coarse(4, 1000, 512, 5, 1, q_ids=one) == -1 and b"one side" in lib.sc_last_error()
    assert coarse(4, 1000, 512, 5, 1, g_ids=one) == -1 and b"one side" in lib.sc_last_error()
    assert coarse(4, 1000, 512, 5, 9) == -1 and b"null" in lib.sc_last_error()     # S above the 8 tiles is legal: only the output is missing
    assert coarse(0, 1000, 512, 5, 2) == 0                                          # nQ == 0: a no-op, nothing is touched

    def rerank(nQ, D, k, E=64, ldr=64):
        return lib.sc_search_rerank_filtered_f32(None, 64, None, None, ldr, None, None, None, None, nQ, 10, E, D, k, None, None, None, None)
    assert rerank(3, 8, 9) == -1 and b"k" in lib.sc_last_error()
    assert rerank(3, 33, 2) == -1 and rerank(3, 8, 0) == -1
    assert rerank(3, 8, 2, ldr=63) == -1 and b"shape" in lib.sc_last_error()
    assert rerank(3, 8, 2) == -1 and b"null" in lib.sc_last_error()
    assert rerank(0, 8, 3) == 0


# ---------------------------------------------------------------------------------------------------- host layers
def test_ops_refuse_cpu_tensors_and_bad_filters_before_any_launch():
    from speechclip_plus_amd import ops
    b = torch.zeros(128, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.search_coarse_filtered(b, b, 3, 5, 2, q_ids=torch.arange(3), g_ids=torch.arange(5))
    z = torch.zeros(3, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.search_rerank_filtered(z, None, torch.zeros(5, 64), None, torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 4), torch.zeros(3), 2)
    fb = fake(b)
    qi, gi = fake(torch.arange(3)), fake(torch.arange(5))
    with pytest.raises(ValueError, match="one side"):
        ops.search_coarse_filtered(fb, fb, 3, 5, 2, q_ids=qi)
    with pytest.raises(ValueError, match="one side"):
        ops.search_coarse_filtered(fb, fb, 3, 5, 2, g_ids=gi)
    with pytest.raises(ValueError, match="g_ids must be torch.int64"):
        ops.search_coarse_filtered(fb, fb, 3, 5, 2, q_ids=qi, g_ids=fake(torch.arange(5).int()))
    with pytest.raises(ValueError, match="q_ids has shape"):
        ops.search_coarse_filtered(fb, fb, 3, 5, 2, q_ids=fake(torch.arange(4)), g_ids=gi)
    with pytest.raises(ValueError, match="contiguous"):
        ops.search_coarse_filtered(fb, fb, 3, 5, 2, q_ids=qi, g_ids=fake(torch.arange(10)[::2]))
    with pytest.raises(ValueError, match="live must be"):
        ops.search_coarse_filtered(fb, fb, 3, 5, 2, live=fake(torch.ones(5)))
    with pytest.raises(ValueError, match="live has shape"):
        ops.search_coarse_filtered(fb, fb, 3, 5, 2, live=fake(torch.ones(6, dtype=torch.bool)))
    with pytest.raises(RuntimeError, match="device tensors only"):
        ops.search_coarse_filtered(fb, fb, 3, 5, 2, q_ids=torch.arange(3), g_ids=torch.arange(5))      # ids left on the CPU


def test_search_compact_validates_the_filter_before_anything_runs():
    import speechclip_plus_amd as sc
    q, g = torch.zeros(3, 64), torch.zeros(5, 64)                    # CPU tensors: a check that passes would end in "device tensors only"
    qi, gi = torch.arange(3), torch.arange(5)
    index = _bare(sc.CompactGalleryIndex, N=5, E=64, ids=gi, live=None, coarse=torch.zeros(128, 64, dtype=torch.bfloat16))
    for gallery in (g, index):
        with pytest.raises(ValueError, match="one side"):
            sc.search_compact(q, gallery, 2, gallery_ids=gi)
        with pytest.raises(ValueError, match="query_ids must be torch.int64"):
            sc.search_compact(q, gallery, 2, query_ids=qi.int(), gallery_ids=gi)
        with pytest.raises(ValueError, match="gallery_ids must be torch.int64"):
            sc.search_compact(q, gallery, 2, query_ids=qi, gallery_ids=gi.float())
        with pytest.raises(ValueError, match="query_ids has shape"):
            sc.search_compact(q, gallery, 2, query_ids=torch.arange(4), gallery_ids=gi)
        with pytest.raises(ValueError, match="gallery_ids has shape"):
            sc.search_compact(q, gallery, 2, query_ids=qi, gallery_ids=torch.arange(6))
        with pytest.raises(ValueError, match="contiguous"):
            sc.search_compact(q, gallery, 2, query_ids=torch.arange(6)[::2], gallery_ids=gi)
        with pytest.raises(ValueError, match="live must be"):
            sc.search_compact(q, gallery, 2, live=torch.ones(5))
        with pytest.raises(ValueError, match="live has shape"):
            sc.search_compact(q, gallery, 2, live=torch.ones(4, dtype=torch.bool))
        with pytest.raises(RuntimeError, match="device tensors only"):
            sc.search_compact(q, gallery, 2, query_ids=qi, gallery_ids=gi)
        with pytest.raises(RuntimeError, match="device tensors only"):
            sc.search_compact(q, gallery, 2, live=torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError, match="one side"):
        sc.search_compact(q, g, 2, query_ids=qi)                     # a tensor gallery brings no ids of its own
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.search_compact(q, index, 2, query_ids=qi)                 # the index's ids are taken: the call gets as far as the device test
    with pytest.raises(ValueError, match="gallery must be"):
        sc.search_compact(q, [1, 2], 2, live=torch.ones(5, dtype=torch.bool))
    with pytest.raises(ValueError, match="ids must be torch.int64"):
        sc.CompactGalleryIndex(fake(g), ids=fake(gi.int()))
    with pytest.raises(ValueError, match="ids has shape"):
        sc.CompactGalleryIndex(fake(g), ids=fake(torch.arange(6)))
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.CompactGalleryIndex(g, ids=gi)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.hard_negatives(q, index, qi, None, 2)                     # b_ids default to the compact index's ids
    with pytest.raises(ValueError, match="b_ids is required"):
        sc.hard_negatives(q, _bare(sc.CompactGalleryIndex, N=5, E=64, ids=None, live=None), qi, None, 2)


def test_search_with_filter_arguments_on_a_compact_index_still_raises_and_names_search_compact():
    import speechclip_plus_amd as sc
    compact = _bare(sc.CompactGalleryIndex, N=5, E=64)
    q = torch.zeros(3, 64)
    for kwargs in ({"query_ids": torch.arange(3), "gallery_ids": torch.arange(5)}, {"live": torch.ones(5, dtype=torch.bool)},
                   {"query_ids": torch.arange(3)}):
        with pytest.raises(ValueError, match="certificate") as err:
            sc.search(q, compact, 2, **kwargs)
        assert "search_compact" in str(err.value)


# ---------------------------------------------------------------------------------------------------- index bookkeeping
def test_compact_index_remove_restore_n_live_and_the_bounds_over_live_rows():
    """GalleryIndex's bookkeeping test on a CompactGalleryIndex, plus the three bounds: they follow the live rows (a dead NaN row does
    not enter, a live one does), all rows dead gives zeros, and restore() of everything brings the original floats back"""
    import speechclip_plus_amd as sc
    nan = float("nan")
    norms = torch.tensor([[1.0, 2.0, nan, 4.0, 3.0, 1.0, 1.0, 1.0, 1.0, 9.0],
                          [1.5, 2.5, nan, 4.5, 3.5, 1.0, 1.0, 1.0, 1.0, 9.5],
                          [0.1, 0.2, nan, 0.4, 0.3, 0.1, 0.1, 0.1, 0.1, 0.9]])
    original = (nan, nan, nan)
    coarse = torch.zeros(128, 64, dtype=torch.bfloat16)
    index = _bare(sc.CompactGalleryIndex, N=10, E=64, Ep=64, coarse=coarse, ids=None, live=None, norms=norms, nbytes=0, _top_all=original,
                  gmax=nan, gtmax=nan, dmax=nan)
    assert index.n_live == 10 and index.live is None
    assert index.remove([2, 5]) is index
    assert index.live.dtype == torch.bool and index.live.shape == (10,) and index.n_live == 8
    assert index.live.tolist() == [True, True, False, True, True, False, True, True, True, True]
    assert (index.gmax, index.gtmax, index.dmax) == (9.0, 9.5, float(norms[2, 9]))
    live = index.live
    index.remove(torch.tensor([5, 9]))
    assert index.live is live and index.n_live == 7                  # in place; removing a removed row is legal
    assert (index.gmax, index.gtmax, index.dmax) == (4.0, 4.5, float(norms[2, 3]))
    assert index.restore([5]) is index and index.live is live and index.n_live == 8
    index.remove([])
    assert index.n_live == 8
    for bad in ([10], [-1], torch.tensor([3, 11])):
        with pytest.raises(IndexError):
            index.remove(bad)
        with pytest.raises(IndexError):
            index.restore(bad)
    assert index.n_live == 8
    index.restore([2])                                               # the NaN row is live again: the bounds carry it
    assert all(v != v for v in (index.gmax, index.gtmax, index.dmax))
    index.remove(list(range(10)))
    assert index.n_live == 0 and (index.gmax, index.gtmax, index.dmax) == (0.0, 0.0, 0.0)
    assert index.restore() is index and index.live is None and index.n_live == 10
    assert all(v != v for v in (index.gmax, index.gtmax, index.dmax)) and index._top_all is original
    assert index.restore([1]).live is None                           # nothing removed: nothing to restore
    assert index.norms is norms and index.nbytes == 0                # the norms were there: nothing was computed or counted again
    assert torch.equal(index.coarse, torch.zeros(128, 64, dtype=torch.bfloat16))


# ---------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("mode", ("ids", "live", "both", "neither"))
def test_filtered_certificate_equals_the_brute_force_loop(mode):
    D, k = 8, 3
    for seed in range(6):
        q, gal = cc.squeezed_case(seed, nQ=12, N=40)
        em = cc.Emulation(q, gal)
        q_ids, g_ids = fc.mod_ids(12, 40, 3) if mode in ("ids", "both") else (None, None)
        live = fc.seeded_live(40, seed, 0.7 if seed % 2 else 0.3) if mode in ("live", "both") else None
        adm = fc.admissible(12, 40, q_ids, g_ids, live)
        eps = cf.live_eps(em, live)
        cert, idx, _ = cf.filtered_certificate(em.coarse, em.exact, eps, D, k, adm)
        want_cert, want_idx = cf.brute_force_certificate(em.coarse, em.exact, eps, D, k, adm)
        assert torch.equal(cert, want_cert) and torch.equal(idx, want_idx), (mode, seed)
        if mode == "neither":
            c0, i0, _ = cc.certificate(em.coarse, em.exact, em.eps, D, k)
            assert torch.equal(cert, c0) and torch.equal(idx, i0)


def test_filtered_certificate_edges():
    coarse = torch.tensor([[0.9, 0.5, 0.4, 0.1, 0.8]], dtype=torch.float64)
    exact = coarse.clone()
    eps = torch.tensor([0.01], dtype=torch.float64)
    adm = torch.tensor([[True, True, True, True, False]])
    cert, idx, margin = cf.filtered_certificate(coarse, exact, eps, 3, 2, adm)             # 4 admissible, D = 3: e_2 = 0.5, t = 0.4
    assert cert.tolist() == [True] and idx.tolist() == [[0, 1]] and abs(float(margin[0]) - (0.1 - 0.5 * 2.0 ** -23 - 0.01)) < 1e-7
    cert, _, _ = cf.filtered_certificate(coarse, exact, torch.tensor([0.11], dtype=torch.float64), 3, 2, adm)
    assert cert.tolist() == [False]
    cert, idx, margin = cf.filtered_certificate(coarse, exact, torch.tensor([0.11], dtype=torch.float64), 5, 2, adm)   # fewer than D
    assert cert.tolist() == [True] and idx.tolist() == [[0, 1]] and float(margin[0]) == float("inf")
    cert, _, _ = cf.filtered_certificate(coarse, exact, torch.tensor([float("inf")], dtype=torch.float64), 5, 2, adm)
    assert cert.tolist() == [False]                                                         # eps not finite: never
    bad = coarse.clone()
    bad[0, 4] = float("nan")                                                                # an inadmissible NaN spoils nothing
    cert, idx, _ = cf.filtered_certificate(bad, bad, eps, 3, 2, adm)
    assert cert.tolist() == [True] and idx.tolist() == [[0, 1]]
    bad[0, 1] = float("-inf")                                                               # an admissible candidate that is not finite does
    cert, idx, _ = cf.filtered_certificate(bad, bad, eps, 5, 4, adm)
    assert cert.tolist() == [False] and idx.tolist() == [[0, 2, 3, 1]]                      # and a real -inf stays ahead of the fillers
    none = torch.zeros(1, 5, dtype=torch.bool)
    cert, idx, _ = cf.filtered_certificate(coarse, exact, eps, 3, 2, none)                  # no admissible row: the empty list, certified
    assert cert.tolist() == [True] and idx.tolist() == [[-1, -1]]


def test_filtered_certificate_is_sound_on_squeezed_scores():
    """round 15's soundness test restated: 120 squeezed cases of 40 queries x 300 rows with ids and a live mask, coarse scores = the fp32
    product of the bf16 images, eps from the live rows' norms: a good share of the rows fail the rule, and every row that passes it
    holds the fp64 filtered list"""
    D, k, certified, total = 8, 3, 0, 0
    for seed in range(120):
        q, gal = cc.squeezed_case(seed)
        em = cc.Emulation(q, gal)
        coarse32 = em.qt @ em.gt.t()                                   # fp32 accumulation, within em.acc of the fp64 product
        q_ids, g_ids = fc.mod_ids(40, 300, 5)
        live = fc.seeded_live(300, seed, 0.3)
        adm = fc.admissible(40, 300, q_ids, g_ids, live)
        cert, idx, _ = cf.filtered_certificate(coarse32, em.exact, cf.live_eps(em, live), D, k, adm)
        _, want = fc.filtered_topk(em.exact.float().double(), k, q_ids, g_ids, live)
        assert torch.equal(idx[cert], want[cert]), seed
        certified += int(cert.sum())
        total += cert.numel()
    print(f"certified {certified} of {total}")
    assert 0.2 * total < certified < 0.8 * total


def test_gpu_case_builders_hold_their_preconditions():
    for i in range(len(cc.GAUSS_CASES)):
        cf.gauss_filtered(i)
        ratio, ulps = cf.gauss_filtered_figures(i)
        print(f"case {cc.GAUSS_CASES[i]}: margin / noise = {ratio:.0f}, first k + 1 admissible scores {ulps:.0f} ulps apart")
    for n in cf.LIVE_COUNTS:
        cf.few_live_case(n)
    for excluded in (cc.CROWD_N, cc.CROWD_N - cf.CROWD_LEFT_IN):
        cf.crowd_filtered(excluded)
    cf.bad_rows_case()
    cf.merge_case()
