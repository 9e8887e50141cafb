"""Sharded gallery search, the checks that need no GPU: the new entry declared / bound / exported, its C argument checks, the host
layers' refusals in their order (format errors before device errors), and ``search`` itself where it was."""
import os
import re

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAME = "sc_search_merge_lists_f32"


class _OnDevice(torch.Tensor):
    """a tensor that says it is on the device; the checks under test raise before anything reads it"""
    is_cuda = True


# ---------------------------------------------------------------------------------------------------- declared, bound, exported
def test_symbol_declared_bound_and_exported():
    from speechclip_plus_amd import _lib, build, ops
    header = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    assert NAME in declared and NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    assert lib.sc_abi_version() == 7
    assert "search_merge_wide.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "search_merge_wide.hip"))
    assert callable(ops.search_merge_lists)


def test_argument_checks_need_no_device():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()

    def merge(nQ, S, k, stride=None):
        return lib.sc_search_merge_lists_f32(None, None, nQ * k if stride is None else stride, None, nQ, S, k, None, None, None)
    assert merge(3, 2, 0) == -1 and b"1 <= k <= 1024" in lib.sc_last_error()
    assert merge(3, 2, 1025) == -1 and b"1 <= k <= 1024" in lib.sc_last_error()
    assert merge(3, 0, 100) == -1 and b"S >= 1" in lib.sc_last_error()
    assert merge(3, 2, 100, stride=-1) == -1 and b"shard_stride >= 0" in lib.sc_last_error()
    assert merge(3, 2, 100, stride=299) == -1 and b"shard_stride >= nQ k" in lib.sc_last_error()
    assert merge(-1, 2, 100) == -1 and b"nQ >= 0" in lib.sc_last_error()
    for k in (1, 33, 1024):
        assert merge(3, 2, k) == -1 and b"null" in lib.sc_last_error()         # everything else passed: the operands are missing
    assert merge(0, 2, 100) == 0                                                # nQ == 0: a no-op, nothing is touched
    assert merge(0, 2, 0) == -1 and merge(0, 0, 100) == -1                      # ... behind the range checks


# ---------------------------------------------------------------------------------------------------- ops.search_merge_lists
def _lists(S=2, nQ=3, k=40, on_device=False):
    pv, pi, row0 = torch.zeros(S, nQ, k), torch.zeros(S, nQ, k, dtype=torch.int32), torch.zeros(S, dtype=torch.int64)
    return tuple(t.as_subclass(_OnDevice) for t in (pv, pi, row0)) if on_device else (pv, pi, row0)


def test_search_merge_lists_refuses_cpu_tensors():
    from speechclip_plus_amd import ops
    pv, pi, row0 = _lists()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.search_merge_lists(pv, pi, row0, 40)
    with pytest.raises(RuntimeError, match="no CPU path"):            # one operand on the host is enough
        ops.search_merge_lists(pv.as_subclass(_OnDevice), pi.as_subclass(_OnDevice), row0, 40)


def test_search_merge_lists_reports_format_errors_before_the_device_error():
    from speechclip_plus_amd import ops
    pv, pi, row0 = _lists()                                           # CPU tensors throughout: every error below is about the format
    with pytest.raises(ValueError, match="part_vals must be torch.float32"):
        ops.search_merge_lists(pv.double(), pi, row0, 40)
    with pytest.raises(ValueError, match="part_idx must be torch.int32"):
        ops.search_merge_lists(pv, pi.long(), row0, 40)
    with pytest.raises(ValueError, match="row0 must be torch.int64"):
        ops.search_merge_lists(pv, pi, row0.int(), 40)
    with pytest.raises(ValueError, match="row0 must be a tensor"):
        ops.search_merge_lists(pv, pi, [0, 0], 40)
    with pytest.raises(ValueError, match=r"must both be \[S, nQ, 41\]"):
        ops.search_merge_lists(pv, pi, row0, 41)
    with pytest.raises(ValueError, match="must both be"):
        ops.search_merge_lists(pv, pi[:, :2], row0, 40)
    with pytest.raises(ValueError, match="1 <= k <= 1024"):
        ops.search_merge_lists(torch.zeros(2, 3, 1025), torch.zeros(2, 3, 1025, dtype=torch.int32), row0, 1025)
    with pytest.raises(ValueError, match="row0 has shape"):
        ops.search_merge_lists(pv, pi, torch.zeros(3, dtype=torch.int64), 40)
    with pytest.raises(ValueError, match="part_vals has strides"):
        ops.search_merge_lists(torch.zeros(2, 40, 3).transpose(1, 2), pi, row0, 40)
    big = torch.zeros(2, 7, 40, dtype=torch.int32)
    with pytest.raises(ValueError, match="differ in their shard stride"):
        ops.search_merge_lists(pv, big[:, 2:5], row0, 40)


# ---------------------------------------------------------------------------------------------------- retrieval
def _bare_index(**attrs):
    """a ShardedGalleryIndex that was never built (no device here): the refusals under test come before anything of it is used"""
    import speechclip_plus_amd as sc
    index = object.__new__(sc.ShardedGalleryIndex)
    index.__dict__.update({"ids": None, "group": None, "E": 64, "N": 50, "shards": [], **attrs})
    return index


def test_sharded_index_refuses_cpu_tensors_and_bad_arguments():
    import speechclip_plus_amd as sc
    g = torch.zeros(50, 64)
    with pytest.raises(RuntimeError, match="ShardedGalleryIndex runs on the HIP kernels: device tensors only"):
        sc.ShardedGalleryIndex(g)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.ShardedGalleryIndex(g, shard_rows=7, cosine=True)
    with pytest.raises(ValueError, match=r"ShardedGalleryIndex: gallery must be a \[N, E\] tensor"):
        sc.ShardedGalleryIndex(torch.zeros(50))
    with pytest.raises(ValueError, match="ShardedGalleryIndex: ids must be torch.int64"):     # the format of ids comes before the device
        sc.ShardedGalleryIndex(g.as_subclass(_OnDevice), ids=torch.zeros(50, dtype=torch.int32))
    with pytest.raises(ValueError, match="shard_rows must be a positive int"):
        sc.ShardedGalleryIndex(g.as_subclass(_OnDevice), shard_rows=0)
    compact = object.__new__(sc.CompactGalleryIndex)
    with pytest.raises(ValueError, match="CompactGalleryIndex cannot be a shard"):
        sc.ShardedGalleryIndex(compact)
    with pytest.raises(ValueError, match="CompactGalleryIndex cannot be a shard"):
        sc.ShardedGalleryIndex([compact])


def test_search_sharded_refusals_and_their_order():
    import speechclip_plus_amd as sc
    q, index = torch.zeros(4, 64), _bare_index()
    with pytest.raises(RuntimeError, match="search_sharded runs on the HIP kernels: device tensors only"):
        sc.search_sharded(q, index, 100)
    for k in (0, 1025, 4096):
        with pytest.raises(ValueError, match="1 <= k <= 1024"):
            sc.search_sharded(q, index, k)
    with pytest.raises(ValueError, match="must be a ShardedGalleryIndex"):        # a tensor as the index
        sc.search_sharded(q, torch.zeros(50, 64), 5)
    with pytest.raises(ValueError, match="must be a ShardedGalleryIndex"):
        sc.search_sharded(q, object.__new__(sc.GalleryIndex), 5)
    with pytest.raises(ValueError, match=r"queries must be a \[nQ, E\] tensor"):
        sc.search_sharded(torch.zeros(64), index, 5)
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="built without ids="):
        sc.search_sharded(q, index, 5, query_ids=ids)
    with_ids = _bare_index(ids=torch.zeros(50, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"query_ids has shape \(3,\), expected \(4,\)"):     # format errors before the device error
        sc.search_sharded(q, with_ids, 5, query_ids=ids[:3])
    with pytest.raises(ValueError, match="query_ids must be torch.int64"):
        sc.search_sharded(q, with_ids, 5, query_ids=ids.int())
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.search_sharded(q, with_ids, 5, query_ids=ids)
    with pytest.raises(RuntimeError, match="device tensors only"):                # queries on the device, their ids not
        sc.search_sharded(q.as_subclass(_OnDevice), with_ids, 5, query_ids=ids)


def test_hard_negatives_and_a_sharded_index_need_its_own_ids():
    import speechclip_plus_amd as sc
    q, a_ids = torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="ShardedGalleryIndex takes a_ids and its own ids"):
        sc.hard_negatives(q, _bare_index(), a_ids, None, 5)
    with_ids = _bare_index(ids=torch.zeros(50, dtype=torch.int64))
    with pytest.raises(ValueError, match="ShardedGalleryIndex takes a_ids and its own ids"):
        sc.hard_negatives(q, with_ids, a_ids, torch.zeros(50, dtype=torch.int64), 5)
    with pytest.raises(RuntimeError, match="search_sharded runs on the HIP kernels: device tensors only"):
        sc.hard_negatives(q, with_ids, a_ids, None, 5)


def test_global_rows_of_remove_are_checked_as_on_a_gallery_index():
    index = _bare_index()
    for rows in ([50], [-1], [3, 50]):
        with pytest.raises(IndexError, match=r"ShardedGalleryIndex: rows outside \[0, 50\)"):
            index.remove(rows)
        with pytest.raises(IndexError, match=r"ShardedGalleryIndex: rows outside \[0, 50\)"):
            index.restore(rows)
    assert len(index) == 50


# ---------------------------------------------------------------------------------------------------- search did not move
def test_search_still_states_its_own_limit_at_wide_k():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import retrieval
    N = 262144 + 1
    assert retrieval.wide_max_gallery() == 262144
    g = torch.zeros(1, 4).expand(N, 4).as_subclass(_OnDevice)
    q = torch.zeros(2, 4).as_subclass(_OnDevice)
    with pytest.raises(ValueError, match="at most N = 262144"):
        sc.search(q, g, 100)
    with pytest.raises(ValueError, match="gallery must be a"):        # search does not know the new type
        sc.search(q, _bare_index(), 100)
