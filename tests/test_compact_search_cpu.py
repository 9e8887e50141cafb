"""Compact gallery search, the checks that need no GPU: the new entries are declared, bound and exported; the host layers refuse CPU
tensors and bad arguments; the error bound ``compact_eps`` holds against an fp64 emulation of the bf16 arithmetic and is tight; and
the certificate rule (mirrored in tests/compact_cases.py) never certifies a list that differs from the fp64 list."""
import os
import re

import pytest
import torch

import compact_cases as cc
import search_cases as sc_cases

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("sc_rows_bf16", "sc_search_coarse_bf16", "sc_search_rerank_f32")


def test_symbols_declared_bound_and_exported():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import _lib, build, ops, retrieval
    header = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.sc_abi_version() == 7
    assert "search_compact.hip" in build.SOURCES
    for name in ("CompactGalleryIndex", "search_compact", "compact_eps"):
        assert getattr(sc, name) is getattr(retrieval, name) and name in sc.__all__ and name in retrieval.__all__
    assert callable(ops.rows_bf16) and callable(ops.search_coarse) and callable(ops.search_rerank)


def test_host_layers_refuse_cpu_tensors():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import ops
    q, g = torch.zeros(3, 64), torch.zeros(5, 64)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.CompactGalleryIndex(g)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.search_compact(q, g, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.search_coarse(torch.zeros(128, 64, dtype=torch.bfloat16), torch.zeros(128, 64, dtype=torch.bfloat16), 3, 5, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rows_bf16(q)


def test_argument_checks_need_no_device():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()

    def coarse(nQ, N, Ep, D, S):
        return lib.sc_search_coarse_bf16(None, None, nQ, N, Ep, D, S, None, None, None)
    assert coarse(4, 1000, 512, 0, 1) == -1 and b"D" in lib.sc_last_error()
    assert coarse(4, 1000, 512, 33, 1) == -1
    assert coarse(4, 1000, 96, 5, 1) == -1 and b"Ep" in lib.sc_last_error()
    assert coarse(4, 1000, 512, 5, 0) == -1
    assert coarse(4, 1000, 512, 5, 7) == -1 and b"slab" in lib.sc_last_error()     # 8 tiles: 6 slabs of 2 tiles already pass the end
    assert coarse(4, 0, 512, 5, 2) == -1
    assert coarse(0, 1000, 512, 5, 2) == 0                                          # nQ == 0: a no-op, nothing is touched
    assert lib.sc_rows_bf16(None, 64, None, 3, 64, None, 100, 64, None, None) == -1 and b"Rp" in lib.sc_last_error()
    assert lib.sc_rows_bf16(None, 64, None, 3, 70, None, 128, 64, None, None) == -1
    assert lib.sc_rows_bf16(None, 64, None, 0, 64, None, 0, 64, None, None) == 0

    def rerank(nQ, D, k):
        return lib.sc_search_rerank_f32(None, 64, None, None, 64, None, None, None, None, nQ, 10, 64, D, k, None, None, None, None)
    assert rerank(3, 8, 9) == -1 and b"k" in lib.sc_last_error()
    assert rerank(3, 33, 2) == -1
    assert rerank(0, 8, 3) == 0


# ---------------------------------------------------------------------------------------------------- the error bound
@pytest.mark.parametrize("E", (64, 512, 768))
def test_compact_eps_bounds_the_emulated_error_on_gaussian_rows(E):
    q, gal = sc_cases.unit_gauss(40, E, 100 + E), sc_cases.unit_gauss(300, E, 200 + E)
    em = cc.Emulation(q, gal)
    err = (em.coarse - em.exact).abs() + em.acc
    ratio = float((err / em.eps.unsqueeze(1)).max())
    print(f"E={E}: eps = {float(em.eps.min()):.5f} .. {float(em.eps.max()):.5f}, max (|coarse - exact| + acc) / eps = {ratio:.4f}")
    assert bool((err <= em.eps.unsqueeze(1)).all())
    assert 0.002 < float(em.eps.min()) and float(em.eps.max()) < 0.006      # the residual-norm form, not the 0.0079 of the worst case


@pytest.mark.parametrize("E", (64, 512, 768))
def test_compact_eps_is_attained_at_the_rounding_midpoint(E):
    """every element 1 + 2^-8 (1 - 2^-10): just below the midpoint of two bf16 numbers, so it rounds to 1 and the residual is parallel to
    the row - Cauchy-Schwarz holds with equality and the bound must be (nearly) attained"""
    v = 1.0 + 2.0 ** -8 * (1.0 - 2.0 ** -10)
    q, gal = torch.full((2, E), v, dtype=torch.float32), torch.full((3, E), v, dtype=torch.float32)
    assert float(q[0, 0]) == v and bool((cc.bf16_image(q) == 1.0).all())
    em = cc.Emulation(q, gal)
    err = (em.coarse - em.exact).abs()
    print(f"E={E}: attained / eps = {float((err / em.eps.unsqueeze(1)).min()):.4f}")
    assert bool((err + em.acc <= em.eps.unsqueeze(1)).all())
    assert bool((err >= 0.9 * em.eps.unsqueeze(1)).all())


def test_compact_eps_carries_non_finite_norms():
    from speechclip_plus_amd import compact_eps
    n = torch.tensor([[1.0, float("nan")], [1.0, 1.0], [0.002, 0.002]])
    eps = compact_eps(n, 1.0, 1.0, 0.002, 64)
    assert eps.dtype == torch.float64 and bool(torch.isfinite(eps[0])) and float(eps[0]) > 0.004
    assert not bool(torch.isfinite(compact_eps(n, float("nan"), 1.0, 0.002, 64)).any())
    assert not bool(torch.isfinite(compact_eps(torch.tensor([[1.0], [float("nan")], [0.1]]), 1.0, 1.0, 0.1, 64)).any())


# ---------------------------------------------------------------------------------------------------- the certificate rule
def test_certificate_rule_is_sound_on_squeezed_scores():
    """200 cases of 40 queries x 300 rows, E = 64, D = 8, k = 3, coarse scores = the fp32 product of the bf16 images: about half the rows
    fail the rule, and every row that passes it holds the fp64 list"""
    D, k, certified, total = 8, 3, 0, 0
    for seed in range(200):
        q, gal = cc.squeezed_case(seed)
        em = cc.Emulation(q, gal)
        coarse32 = em.qt @ em.gt.t()                                   # fp32 accumulation, within em.acc of the fp64 product
        assert bool(((coarse32.double() - em.coarse).abs() <= em.acc).all())
        cert, idx, _ = cc.certificate(coarse32, em.exact, em.eps, D, k)
        _, want = sc_cases.stable_topk(em.exact.float().double(), k)
        assert torch.equal(idx[cert], want[cert]), seed
        certified += int(cert.sum())
        total += cert.numel()
    print(f"certified {certified} of {total}")
    assert 0.3 * total < certified < 0.7 * total


def test_certificate_rule_edges():
    coarse = torch.tensor([[0.9, 0.5, 0.4, 0.1], [0.9, 0.5, float("nan"), 0.1]], dtype=torch.float64)
    exact = torch.tensor([[0.9, 0.5, 0.4, 0.1], [0.9, 0.5, 0.4, 0.1]], dtype=torch.float64)
    eps = torch.tensor([0.01, 0.01], dtype=torch.float64)
    cert, idx, _ = cc.certificate(coarse, exact, eps, 4, 2)            # N <= D: every row is a candidate
    assert cert.tolist() == [True, False] and idx[0].tolist() == [0, 1]
    cert, _, margin = cc.certificate(coarse[:1], exact[:1], eps[:1], 3, 2)         # e_2 = 0.5, t = 0.4: margin 0.1 - eps
    assert cert.tolist() == [True] and abs(float(margin[0]) - (0.1 - 0.5 * 2.0 ** -23 - 0.01)) < 1e-7      # exact is rounded to fp32 first
    cert, _, _ = cc.certificate(coarse[:1], exact[:1], torch.tensor([0.11], dtype=torch.float64), 3, 2)
    assert cert.tolist() == [False]
    cert, _, _ = cc.certificate(coarse[:1], exact[:1], torch.tensor([float("inf")], dtype=torch.float64), 3, 2)
    assert cert.tolist() == [False]


def test_gpu_case_builders_hold_their_preconditions():
    for i in range(len(cc.GAUSS_CASES)):
        cc.gauss_compact(i)
    q, gal, want, k, D = cc.crowd_case()
    assert want[0].tolist() == list(range(cc.CROWD_FIRST, cc.CROWD_FIRST + k))
    cc.planted_compact()
