"""Sharded retrieval ranks, the checks that need no GPU: the two new entries declared / bound / exported, their C argument checks, the
host layers' refusals in their order (format errors before device errors), and the model hook's refusal of a group without
``retrieval.fused_ranks``."""
import os
import re

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("sc_rank_best_bf16", "sc_rank_ahead_bf16")


class _OnDevice(torch.Tensor):
    """a tensor that says it is on the device; the checks under test raise before anything reads it"""
    is_cuda = True


# ---------------------------------------------------------------------------------------------------- declared, bound, exported
def test_symbols_declared_bound_and_exported():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import _lib, build, ops
    header = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.sc_abi_version() == 7
    assert "rank.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "rank.hip"))
    assert "rank_parts.hip" not in build.SOURCES and not os.path.exists(os.path.join(build.CSRC, "rank_parts.hip"))
    for name in NAMES + ("sc_rank_counts_bf16",):                     # one file, three entries
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert callable(ops.rank_best) and callable(ops.rank_ahead)
    assert callable(sc.mutual_ranks_sharded) and callable(sc.mutual_recall_sharded)
    assert "mutual_ranks_sharded" in sc.__all__ and "mutual_recall_sharded" in sc.__all__


def _entries():
    """both C entries as f(nA, nB, K6, S) with null pointers throughout"""
    from speechclip_plus_amd import _lib
    lib = _lib.lib()

    def best(nA, nB, K6, S):
        return lib.sc_rank_best_bf16(None, None, None, None, None, nA, nB, K6, S, None, None, None)

    def ahead(nA, nB, K6, S):
        return lib.sc_rank_ahead_bf16(None, None, None, None, None, nA, nB, K6, S, None, None, None, None, None)
    return lib, (("sc_rank_best_bf16", best), ("sc_rank_ahead_bf16", ahead))


def test_argument_checks_need_no_device():
    lib, entries = _entries()
    for name, f in entries:
        for K6 in (0, 64, 383, 385, 768 + 64, -384):
            assert f(3, 5, K6, 1) == -1 and name.encode() in lib.sc_last_error() and b"K6=" in lib.sc_last_error(), (name, K6)
        for S in (0, -1):
            assert f(3, 5, 384, S) == -1 and b"S >= 1" in lib.sc_last_error()
        assert f(-1, 5, 384, 1) == -1 and b"nA >= 0" in lib.sc_last_error()
        assert f(3, -1, 384, 1) == -1 and b"nB >= 0" in lib.sc_last_error()
        assert f(3, 5, 384, 1) == -1 and b"null a_split" in lib.sc_last_error()      # everything else passed: the operands are missing
        assert f(3, 5, 768, 4) == -1 and name.encode() in lib.sc_last_error()
        assert f(0, 5, 384, 1) == 0 and f(3, 0, 384, 1) == 0 and f(0, 0, 768, 3) == 0   # no pair: a no-op, nothing is touched
        assert f(0, 5, 100, 1) == -1 and f(0, 5, 384, 0) == -1                       # ... behind the range checks


# ---------------------------------------------------------------------------------------------------- ops
def _operands(nA=3, nB=5, on_device=False):
    a, b = torch.zeros(128, 384, dtype=torch.bfloat16), torch.zeros(128, 384, dtype=torch.bfloat16)
    a_ids, b_ids = torch.zeros(nA, dtype=torch.int64), torch.zeros(nB, dtype=torch.int64)
    keys = torch.zeros(nA, dtype=torch.int32), torch.zeros(nB, dtype=torch.int32)
    out = (a, b, a_ids, b_ids, nA, nB) + keys
    return tuple(t.as_subclass(_OnDevice) if on_device and isinstance(t, torch.Tensor) else t for t in out)


def test_ops_refuse_cpu_tensors_under_their_own_names():
    from speechclip_plus_amd import ops
    args = _operands()
    with pytest.raises(RuntimeError, match="rank_best runs on the HIP kernels: no CPU path"):
        ops.rank_best(*args)
    with pytest.raises(RuntimeError, match="rank_ahead runs on the HIP kernels: no CPU path"):
        ops.rank_ahead(*args, torch.zeros(3, dtype=torch.int32), torch.zeros(5, dtype=torch.int32))
    dev = _operands(on_device=True)
    with pytest.raises(RuntimeError, match="rank_best runs on the HIP kernels: no CPU path"):      # the mask alone on the host is enough
        ops.rank_best(*dev, b_live=torch.ones(5, dtype=torch.bool))


def test_ops_check_shapes_and_dtypes_before_any_launch():
    from speechclip_plus_amd import ops
    a, b, a_ids, b_ids, nA, nB, key_a, key_b = _operands(on_device=True)
    live = torch.ones(nB, dtype=torch.bool).as_subclass(_OnDevice)
    with pytest.raises(AssertionError):
        ops.rank_best(a, b, a_ids, b_ids, nA, nB, key_a.long(), key_b)                # keys live in int32 storage
    with pytest.raises(AssertionError):
        ops.rank_best(a, b, a_ids, b_ids, nA, nB, key_a, key_b[:4])
    with pytest.raises(AssertionError):
        ops.rank_best(a, b, a_ids.int(), b_ids, nA, nB, key_a, key_b)
    with pytest.raises(AssertionError):
        ops.rank_best(a, b, a_ids, b_ids, 129, nB, key_a, key_b)                      # more rows than the split holds
    with pytest.raises(AssertionError):
        ops.rank_best(a, b, a_ids, b_ids, nA, nB, key_a, key_b, b_live=live[:4])
    with pytest.raises(AssertionError):
        ops.rank_best(a, b, a_ids, b_ids, nA, nB, key_a, key_b, b_live=live.long())
    with pytest.raises(AssertionError):
        ops.rank_ahead(a, b, a_ids, b_ids, nA, nB, key_a, key_b, key_a.clone(), key_b.float())


# ---------------------------------------------------------------------------------------------------- retrieval
def _bare_index(**attrs):
    """a ShardedGalleryIndex that was never built (no device here): the refusals under test come before anything of it is used"""
    import speechclip_plus_amd as sc
    index = object.__new__(sc.ShardedGalleryIndex)
    index.__dict__.update({"ids": None, "group": None, "E": 64, "N": 50, "shards": [], **attrs})
    return index


@pytest.mark.parametrize("which", ("ranks", "recall"))
def test_refusals_and_their_order(which):
    import speechclip_plus_amd as sc

    def call(A, index, a_ids):
        if which == "ranks":
            return sc.mutual_ranks_sharded(A, index, a_ids)
        return sc.mutual_recall_sharded(A, index, a_ids, [1, 5])
    A, a_ids = torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"must be a ShardedGalleryIndex .* goes to mutual_ranks\)"):     # a tensor as the index
        call(A, torch.zeros(50, 64), a_ids)
    with pytest.raises(ValueError, match=r"must be a ShardedGalleryIndex .* goes to mutual_ranks\)"):
        call(A, object.__new__(sc.GalleryIndex), a_ids)
    with pytest.raises(ValueError, match="built without ids="):
        call(A, _bare_index(), a_ids)
    with_ids = _bare_index(ids=torch.zeros(50, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"A must be a \[nA, E\] tensor"):
        call(torch.zeros(64), with_ids, a_ids)
    with pytest.raises(ValueError, match=r"a_ids has shape \(3,\), expected \(4,\)"):              # format errors before the device error
        call(A, with_ids, a_ids[:3])
    with pytest.raises(ValueError, match="a_ids must be torch.int64"):
        call(A, with_ids, a_ids.int())
    with pytest.raises(RuntimeError, match="mutual_ranks_sharded runs on the HIP kernels: device tensors only"):
        call(A, with_ids, a_ids)
    with pytest.raises(RuntimeError, match="device tensors only"):                               # A on the device, its ids not
        call(A.as_subclass(_OnDevice), with_ids, a_ids)


# ---------------------------------------------------------------------------------------------------- model
def _bare_model(fused: bool):
    """the hook reads ``config`` and ``recall_at`` only: no encoder is built"""
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config
    cfg = base_parallel_config()
    if fused:
        cfg.retrieval.fused_ranks = True
    model = KWClip_GeneralTransformer.__new__(KWClip_GeneralTransformer)
    torch.nn.Module.__init__(model)
    model.config, model.recall_at, model.cascaded_branch = cfg, cfg.retrieval.recall_at, None
    return model


def test_validation_epoch_end_with_a_group_needs_fused_ranks():
    model = _bare_model(fused=False)
    with pytest.raises(ValueError, match="retrieval.fused_ranks"):
        model.validation_epoch_end([], group=object())               # raised before the group or the outputs are looked at
    import inspect
    sig = inspect.signature(model.validation_epoch_end)
    assert list(sig.parameters) == ["outputs", "group"] and sig.parameters["group"].default is None
