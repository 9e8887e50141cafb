"""Retrieval ranks, the checks that need no GPU: the entry is declared, bound and exported; the host layers refuse CPU tensors; the
argument checks answer before anything touches a device; and the rule of the GPU tests (tests/rank_cases.py) together with
``recall_from_ranks`` reproduces what ``mutualRetrieval`` reports."""
import ctypes
import os
import re

import pytest
import torch

import rank_cases as rk
import search_cases as sc_cases

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_symbol_declared_bound_and_exported():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import _lib, ops, retrieval
    header = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    assert "sc_rank_counts_bf16" in declared and "sc_rank_counts_bf16" in _lib.SIGNATURES and hasattr(lib, "sc_rank_counts_bf16")
    assert lib.sc_abi_version() == 7
    assert "retrieval.py:45-121" in header and "kwClip.py:447-482" in header
    assert callable(ops.rank_counts)
    for name in ("mutual_ranks", "recall_from_ranks", "mutual_recall"):
        assert name in sc.__all__ and name in retrieval.__all__ and getattr(sc, name) is getattr(retrieval, name)


def test_host_layers_refuse_cpu_tensors():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import ops
    A, B = torch.zeros(3, 64), torch.zeros(5, 64)
    a_ids, b_ids = torch.arange(3), torch.arange(5)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.mutual_ranks(A, B, a_ids, b_ids)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.mutual_recall(A, B, a_ids, b_ids, [1, 5])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rank_counts(torch.zeros(128, 384, dtype=torch.bfloat16), torch.zeros(128, 384, dtype=torch.bfloat16), a_ids, b_ids, 3, 5)


def test_argument_checks_need_no_device():
    """every call here ends in a failed check or in the empty-problem return: no kernel is launched, no pointer is followed"""
    from speechclip_plus_amd import _lib
    lib = _lib.lib()
    names = ("a_split", "b_split", "a_ids", "b_ids", "best_a", "best_b", "ahead_a", "ahead_b")

    def rc(nA, nB, K6, S, null=None, all_null=False):
        ptr = [None if (all_null or n == null) else ctypes.c_void_p(4096) for n in names]
        return lib.sc_rank_counts_bf16(ptr[0], ptr[1], ptr[2], ptr[3], nA, nB, K6, S, ptr[4], ptr[5], ptr[6], ptr[7], None)
    for name in names:
        assert rc(4, 1000, 384, 1, null=name) == -1
        assert name.encode() in lib.sc_last_error(), (name, lib.sc_last_error())
    assert rc(4, 1000, 320, 1, all_null=True) == -1 and b"K6" in lib.sc_last_error()
    assert rc(4, 1000, 0, 1, all_null=True) == -1
    assert rc(4, 1000, 384, 0, all_null=True) == -1 and b"S" in lib.sc_last_error()
    assert rc(-1, 1000, 384, 1, all_null=True) == -1
    assert rc(0, 1000, 384, 2, all_null=True) == 0                  # nA == 0: a no-op, nothing is touched
    assert rc(4, 0, 384, 1, all_null=True) == 0                     # nB == 0 too


def _dicts_from_reference(score, a_ids, b_ids, ks):
    from speechclip_plus_amd import recall_from_ranks
    ref = rk.both_directions(score, a_ids, b_ids)
    AB = recall_from_ranks(ref["ahead_AB"], b_ids.numel(), ks)
    BA = recall_from_ranks(ref["ahead_BA"], a_ids.numel(), ks)
    return AB, BA, {key: 0.5 * (AB[key] + BA[key]) for key in AB}, ref


def _assert_same_recalls(got, want):
    for g, w in zip(got, want):
        assert set(w) <= set(g) and set(g) - set(w) == {"median_rank", "mean_rank"}
        for key in w:
            assert abs(g[key] - w[key]) < 1e-9, (key, g[key], w[key])


def test_rule_and_recall_from_ranks_reproduce_mutual_retrieval_on_the_golden_scores(golden):
    from speechclip_plus_amd import mutualRetrieval
    fx = golden("retrieval.npz")
    s, a_ids, b_ids = torch.from_numpy(fx["score"]), torch.from_numpy(fx["a_ids"]), torch.from_numpy(fx["b_ids"])
    ks = [1, 5, 10]
    AB, BA, mean, _ = _dicts_from_reference(s.double(), a_ids, b_ids, ks)
    _assert_same_recalls((AB, BA, mean), mutualRetrieval(s, s.T, a_ids, b_ids, ks))
    for i, k in enumerate(ks):
        assert abs(AB[f"recall@{k}"] - fx["AB"][i]) < 1e-4 and abs(BA[f"recall@{k}"] - fx["BA"][i]) < 1e-4
        assert abs(mean[f"recall@{k}"] - fx["mean"][i]) < 1e-4


def test_rule_on_a_hand_written_case():
    """query 0: correct candidate 0 scores 2; wrong candidate 1 ties with it and candidate 3 is NaN -> 2 ahead (the correct candidate
    4, scoring less, is not).  query 1: its id is in no candidate -> all 5 ahead.  query 2: its only correct candidate scores +inf ->
    all 5 ahead."""
    from speechclip_plus_amd import mutualRetrieval, recall_from_ranks
    nan, inf = float("nan"), float("inf")
    s = torch.tensor([[2.0, 2.0, 1.0, nan, 0.5],
                      [3.0, 1.0, 0.0, 1.0, 2.0],
                      [0.0, 0.0, inf, 0.0, 0.0]], dtype=torch.float64)
    a_ids = torch.tensor([0, 5, 1])
    b_ids = torch.tensor([0, 9, 1, 9, 0])
    ks = [1, 2, 3, 5, 7]
    AB, BA, mean, ref = _dicts_from_reference(s, a_ids, b_ids, ks)
    assert ref["ahead_AB"].tolist() == [2, 5, 5] and ref["best_AB"].tolist() == [2.0, -inf, inf]
    # candidates as queries: 0 -> its query 0 scores 2, query 1 (wrong, 3) is ahead: 1; 1 and 3 have no correct query: 3;
    # 2 -> its best is +inf: 3; 4 -> query 0 scores 0.5, query 1 (wrong, 2) is ahead: 1
    assert ref["ahead_BA"].tolist() == [1, 3, 3, 3, 1]
    _assert_same_recalls((AB, BA, mean), mutualRetrieval(s, s.t(), a_ids, b_ids, ks))
    assert AB["recall@3"] == pytest.approx(100.0 / 3) and AB["recall@2"] == 0.0 and AB["recall@5"] == pytest.approx(100.0 / 3)
    assert AB["recall@7"] == 100.0                                   # _recall's own: k above the candidate count counts every query
    assert AB["median_rank"] == 6.0 and AB["mean_rank"] == pytest.approx((3 + 6 + 6) / 3)
    assert BA["median_rank"] == 4.0 and BA["mean_rank"] == pytest.approx((2 + 4 + 4 + 4 + 2) / 5)
    even = recall_from_ranks(torch.tensor([0, 3, 1, 9]), 10, [1])
    assert even["median_rank"] == 3.0 and even["mean_rank"] == 4.25 and even["recall@1"] == 25.0     # ranks 1, 2, 4, 10


def test_caption_ids_are_what_they_claim():
    a_ids, b_ids = rk.caption_ids(300, 130, 4)
    assert bool((torch.bincount(a_ids)[10:] == 5).all())
    sa, sb = set(a_ids.tolist()), set(b_ids.tolist())
    assert sa - sb and sb - sa and sa & sb                           # ids absent on either side, and ids on both
    assert int(torch.bincount(b_ids[b_ids >= 0]).max()) == 2          # a query with two correct candidates
    assert rk.caption_ids(1, 1, 0)[1].tolist() == [10]                # the 1 x 1 case holds a correct pair


@pytest.mark.parametrize("E", (512, 768))
def test_planted_ranks_of_the_fp64_reference(E):
    k = 10
    q, gal, planted, s64, bound = sc_cases.planted_case(70, 1500, E, k, 11)
    a_ids, b_ids = rk.planted_ids(planted, 1500)
    ref = rk.both_directions(s64, a_ids, b_ids)
    assert ref["ahead_AB"].tolist() == [i % k for i in range(70)]
    matched = planted[torch.arange(70), torch.arange(70) % k]
    assert bool((ref["ahead_BA"][matched] == 0).all())
    rest = torch.ones(1500, dtype=torch.bool)
    rest[matched] = False
    assert int(rest.sum()) == 1500 - 70 and bool((ref["ahead_BA"][rest] == 70).all())


def test_degenerate_case_expectation():
    A, B, a_ids, b_ids, ref = rk.degenerate_case()
    nA, nB = A.shape[0], B.shape[0]
    assert ref["ahead_AB"][rk.NAN_A] == nB and ref["ahead_AB"][rk.LONELY_A] == nB
    assert ref["ahead_BA"][rk.NAN_B] == nA and ref["ahead_BA"][rk.INF_B] == nA
    assert bool(torch.signbit(A[rk.ZERO_A, ::2]).all()) and not bool(torch.signbit(A[rk.ZERO_A, 1::2]).any())
    zero_row = ref["ahead_AB"][rk.ZERO_A]
    n_correct = int((b_ids == a_ids[rk.ZERO_A]).sum())
    assert n_correct >= 1 and zero_row == nB - n_correct              # every wrong candidate ties with the best: all of them are ahead
