"""Gallery search, the checks that need no GPU: the new entries are declared, bound and exported; the host layers refuse CPU tensors;
the slab chooser keeps its promises; and the case builders of the GPU tests are what they claim to be."""
import os
import re

import pytest
import torch

import search_cases as sc_cases

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_symbols_declared_bound_and_exported():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import _lib, ops, retrieval
    header = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("sc_search_slabs", "sc_search_topk_bf16"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.sc_abi_version() == 7
    assert "retrieval.py:45-46" in header and "kwClip.py:447-482" in header
    assert sc.search is retrieval.search and sc.GalleryIndex is retrieval.GalleryIndex
    assert {"search", "GalleryIndex"} <= set(sc.__all__)
    assert callable(ops.search_topk)


def test_host_layers_refuse_cpu_tensors():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import ops
    q, g = torch.zeros(3, 64), torch.zeros(5, 64)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.search(q, g, 2)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.GalleryIndex(g)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.search_topk(torch.zeros(128, 384, dtype=torch.bfloat16), torch.zeros(128, 384, dtype=torch.bfloat16), 3, 5, 2)


def test_argument_checks_need_no_device():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()

    def rc(nQ, N, K6, k, S):
        return lib.sc_search_topk_bf16(None, None, nQ, N, K6, k, S, None, None, None)
    assert rc(4, 1000, 384, 0, 1) == -1 and b"k" in lib.sc_last_error()
    assert rc(4, 1000, 384, 33, 1) == -1
    assert rc(4, 1000, 320, 5, 1) == -1 and b"K6" in lib.sc_last_error()
    assert rc(4, 1000, 384, 5, 0) == -1
    assert rc(4, 1000, 384, 5, 7) == -1 and b"slab" in lib.sc_last_error()      # 8 tiles: 6 slabs of 2 tiles already pass the end
    assert rc(4, 0, 384, 5, 2) == -1                                                # an empty gallery has one (empty) slab
    assert rc(0, 1000, 384, 5, 2) == 0                                              # nQ == 0: a no-op, nothing is touched


def test_slab_chooser_properties():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()
    for nQ in (1, 64, 128, 129, 1000, 5000, 25000, 40000):
        for N in (1, 63, 128, 129, 1000, 5000, 100000, 1000000):
            for k in (1, 10, 32):
                S = lib.sc_search_slabs(nQ, N, k)
                nT, T = sc_cases.slab_tiles(N, S)
                assert S >= 1
                assert (S - 1) * T < nT, (nQ, N, k, S)          # whole tiles; the last slab is not empty ...
                for s in range(S - 1):                           # ... so every slab before it is made of full tiles: >= k columns
                    assert min(N, (s + 1) * T * sc_cases.TILE) - s * T * sc_cases.TILE >= k
                if N <= sc_cases.TILE:
                    assert S == 1
    assert lib.sc_search_slabs(40000, 5000, 10) == 1                # the row tiles alone cover the chip
    assert lib.sc_search_slabs(64, 1000000, 10) > 1                 # few queries: the gallery axis is cut
    assert lib.sc_search_slabs(0, 1000, 10) == 1 and lib.sc_search_slabs(10, 0, 10) == 1


def test_retrieve_present_and_refuses_cpu_input():
    import speechclip_plus_amd as sc
    model = sc.KWClip_GeneralTransformer(sc.base_parallel_config(), device="cpu")
    assert callable(model.retrieve)
    with pytest.raises(RuntimeError, match="device tensors only"):
        model.retrieve(torch.zeros(2, 512), torch.zeros(7, 512))
    with pytest.raises(RuntimeError, match="device tensors only"):
        model.retrieve([torch.zeros(8000)], torch.zeros(7, 512), k=3)


def test_stable_topk_is_the_contract():
    score = torch.tensor([[1, 3, 3, -2, 3], [0, 0, 0, 0, 0]])
    vals, idx = sc_cases.stable_topk(score, 4)
    assert idx.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3]] and vals[0].tolist() == [3.0, 3.0, 3.0, 1.0]
    vals, idx = sc_cases.stable_topk(score[:, :2], 4)
    assert idx.tolist() == [[1, 0, -1, -1], [0, 1, -1, -1]] and vals[0, 2:].tolist() == [float("-inf")] * 2
    q, g = sc_cases.int_case(5, 40, 64, 1)
    assert int((q.long() @ g.long().t()).abs().max()) < 2 ** 24 and q.abs().max() <= 3
    qi, gi = sc_cases.ramp_case(4, 700, 64, True)
    s = qi @ gi.t()
    assert bool((s[:, 1:] > s[:, :-1]).all())
    qd, gd = sc_cases.ramp_case(4, 700, 64, False)
    s = qd @ gd.t()
    assert bool((s[:, 1:] < s[:, :-1]).all())


@pytest.mark.parametrize("E", (512, 768))
def test_planted_case_is_decided_by_the_yardstick(E):
    """the planted rows sit at their cosines in rank order, everything else is far below, and every fp64 gap among the first k + 1
    ranks exceeds four times the bound: the fp32 scores cannot change the expected lists"""
    k = 10
    q, gal, planted, s64, bound = sc_cases.planted_case(70, 1500, E, k, 11)
    want = sc_cases.PLANT_COS0 - sc_cases.PLANT_STEP * torch.arange(k, dtype=torch.float64)
    assert torch.allclose(torch.gather(s64, 1, planted), want.expand(70, k), atol=1e-6)
    _, idx = sc_cases.stable_topk(s64, k)
    assert torch.equal(idx, planted)
    rest = s64.clone()
    rest.scatter_(1, planted, 0.0)
    assert float(rest.abs().max()) < 0.3
    assert float(bound.max()) < (6 * E + 8) * 2.0 ** -24 * 1.0001                   # Cauchy-Schwarz on unit rows
    assert sc_cases.planted_min_gap_over_bound(s64, bound, k) > 4.0
