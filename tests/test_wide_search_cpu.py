"""Wide search (k up to 1024), the checks that need no GPU: the restated contract on hand-written rows, the comparison's sensitivity,
the new entry declared / bound / exported, its C argument checks, and the host layers' refusals."""
import os
import re

import pytest
import torch

import wide_cases as wc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAN, INF = wc.NAN, wc.INF


# ---------------------------------------------------------------------------------------------------- the restatement
def test_restatement_on_hand_written_rows():
    s = torch.tensor([[1.0, 3.0, 1.0, NAN, -INF, 3.0, INF, -0.0, 0.0, NAN, 99.0, 98.0],
                      [0.0, -0.0, 0.0, -1.0, -0.0, -INF, -INF, 2.0, 2.0, 2.0, 99.0, 98.0]])
    vals, idx = wc.restated_topk(s, 10, 12)                           # columns 10 and 11 are slack
    assert idx.tolist() == [[3, 9, 6, 1, 5, 0, 2, 7, 8, 4, -1, -1],
                            [7, 8, 9, 0, 1, 2, 4, 3, 5, 6, -1, -1]]
    assert bool(torch.isnan(vals[0, :2]).all()) and vals[0, 2:7].tolist() == [INF, 3.0, 3.0, 1.0, 1.0]
    assert vals[0, 7:].tolist() == [0.0, 0.0, -INF, -INF, -INF]
    # the matrix's own bits: the -0 of column 7 keeps its sign, a filler is a plain -inf
    assert vals.view(torch.int32)[0, 7].item() == -2 ** 31 and vals.view(torch.int32)[0, 8].item() == 0
    assert [vals.view(torch.int32)[1, p].item() for p in range(3, 7)] == [0, -2 ** 31, 0, -2 ** 31]
    v3, i3 = wc.restated_topk(s, 10, 3)
    assert i3.tolist() == [[3, 9, 6], [7, 8, 9]]


def test_restatement_with_a_filter():
    s = torch.tensor([[5.0, NAN, 5.0, -INF, 4.0, -INF, 7.0],
                      [5.0, NAN, 5.0, -INF, 4.0, -INF, 7.0],
                      [5.0, NAN, 5.0, -INF, 4.0, -INF, 7.0]])
    g_ids = torch.tensor([0, 1, 1, 2, 2, 0, 3], dtype=torch.int64)
    q_ids = torch.tensor([1, 3, -7], dtype=torch.int64)
    live = torch.tensor([1, 1, 1, 1, 0, 1, 1], dtype=torch.bool)
    vals, idx = wc.restated_topk(s, 7, 6, q_ids, g_ids, live)
    assert idx.tolist() == [[6, 0, 3, 5, -1, -1],                    # NaN (id 1) and the dead 4.0 are absent; a real -inf keeps its column
                            [1, 0, 2, 3, 5, -1],
                            [1, 6, 0, 2, 3, 5]]
    assert vals[0].tolist() == [7.0, 5.0, -INF, -INF, -INF, -INF]
    v0, i0 = wc.restated_topk(s, 7, 6, live=torch.zeros(7, dtype=torch.bool))
    assert bool((i0 == -1).all()) and bool(torch.isneginf(v0).all())


def test_restatement_breaks_long_tie_runs_by_column():
    s = torch.full((1, 5000), 2.5)
    s[0, 4000:4003] = 9.0
    vals, idx = wc.restated_topk(s, 5000, 100)
    assert idx[0].tolist() == [4000, 4001, 4002] + list(range(97))


def test_comparison_rejects_the_three_classic_mistakes():
    s = torch.tensor([[1.0, 3.0, 3.0, NAN, -INF, 0.5]])
    want = wc.restated_topk(s, 6, 8)
    assert wc.same_bits(want, want) and want[1].tolist() == [[3, 1, 2, 0, 5, 4, -1, -1]]

    def swapped(a, b):
        v, i = want[0].clone(), want[1].clone()
        v[0, [a, b]] = v[0, [b, a]]
        i[0, [a, b]] = i[0, [b, a]]
        return v, i
    assert not wc.same_bits(swapped(1, 2), want)                     # two tied columns swapped
    assert not wc.same_bits(swapped(0, 1), want)                     # the NaN behind a number
    assert not wc.same_bits(swapped(5, 6), want)                     # a filler before the real -inf
    v, i = want[0].clone(), want[1].clone()
    v[0, 3] = -0.0 * v[0, 3]                                         # only a sign bit
    assert not wc.same_bits((v, i), want)


# ---------------------------------------------------------------------------------------------------- declared, bound, exported
def test_symbol_declared_bound_and_exported():
    from speechclip_plus_amd import _lib, build, ops
    header = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    name = "sc_topk_rows_wide_f32"
    assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.sc_abi_version() == 7
    assert "topk_wide.hip" in build.SOURCES
    assert "avssl/module/retrieval.py:45-46" in header[header.index("Wide gallery search"):header.index(name + "(")]
    assert callable(ops.topk_rows_wide)


def test_argument_checks_need_no_device():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()
    one = 8                                                          # a non-null, 8-byte aligned address that is never dereferenced

    def rows(n, V, k, ld=None, q_ids=None, g_ids=None):
        return lib.sc_topk_rows_wide_f32(None, V if ld is None else ld, n, V, k, q_ids, g_ids, None, None, None, None)
    assert rows(3, 100, 0) == -1 and b"1 <= k <= 1024" in lib.sc_last_error()
    assert rows(3, 100, 1025) == -1 and b"1 <= k <= 1024" in lib.sc_last_error()
    assert rows(3, 0, 100) == -1 and rows(3, 100, 100, ld=99) == -1 and rows(-1, 100, 100) == -1
    assert rows(3, 100, 100, q_ids=one) == -1 and b"one side" in lib.sc_last_error()
    assert rows(3, 100, 100, g_ids=one) == -1 and b"one side" in lib.sc_last_error()
    for k in (1, 33, 1024):
        assert rows(3, 100, k) == -1 and b"null" in lib.sc_last_error()        # everything else passed: the operands are missing
    assert rows(0, 100, 100) == 0                                               # rows == 0: a no-op, nothing is touched


# ---------------------------------------------------------------------------------------------------- host layers
def test_topk_rows_wide_refuses_cpu_tensors_and_bad_operands():
    from speechclip_plus_amd import ops
    s = torch.zeros(3, 50)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.topk_rows_wide(s, 50, 40)
    with pytest.raises(RuntimeError, match="no CPU path"):            # the device test comes before the k range ...
        ops.topk_rows_wide(s, 50, 2000)
    with pytest.raises(ValueError, match="must be a"):                # ... and behind the shape test
        ops.topk_rows_wide(torch.zeros(50), 50, 40)


class _OnDevice(torch.Tensor):
    """a tensor that says it is on the device; the checks under test raise before anything reads it"""
    is_cuda = True


def test_topk_rows_wide_checks_formats_and_the_k_range_before_any_launch():
    from speechclip_plus_amd import ops
    s = torch.zeros(3, 50).as_subclass(_OnDevice)
    for k in (0, 1025, -3):
        with pytest.raises(RuntimeError, match="1 <= k <= 1024"):
            ops.topk_rows_wide(s, 50, k)
    with pytest.raises(ValueError, match="torch.float32"):
        ops.topk_rows_wide(torch.zeros(3, 50, dtype=torch.float64).as_subclass(_OnDevice), 50, 40)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.topk_rows_wide(torch.zeros(50, 3).as_subclass(_OnDevice).t(), 50, 40)
    with pytest.raises(ValueError, match="expected at least"):
        ops.topk_rows_wide(s, 51, 40)
    with pytest.raises(ValueError, match="one side only"):
        ops.topk_rows_wide(s, 50, 40, q_ids=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="g_ids must be torch.int64"):
        ops.topk_rows_wide(s, 50, 40, q_ids=torch.zeros(3, dtype=torch.int64), g_ids=torch.zeros(50, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"live has shape \(49,\), expected \(50,\)"):
        ops.topk_rows_wide(s, 50, 40, live=torch.ones(49, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="device tensors only"):
        ops.topk_rows_wide(s, 50, 40, live=torch.ones(50, dtype=torch.bool))


def test_narrow_entries_still_refuse_k_33():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()
    assert lib.sc_topk_rows_f32(None, 100, 3, 100, 33, None, None, None) == -1 and b"1 <= k <= 32" in lib.sc_last_error()
    assert lib.sc_topk_rows_filtered_f32(None, 100, 3, 100, 33, None, None, None, None, None, None) == -1
    assert b"1 <= k <= 32" in lib.sc_last_error()


def test_search_refusals_at_wide_k():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import retrieval
    q, g = torch.zeros(4, 64), torch.zeros(50, 64)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.search(q, g, 100)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.search(q, g, 1024)
    with pytest.raises(RuntimeError, match="device tensors only"):
        sc.hard_negatives(q, g, torch.zeros(4, dtype=torch.int64), torch.zeros(50, dtype=torch.int64), 200)
    for kw in ({"route": "fused"}, {"slabs": 2}, {"route": "fused", "slabs": 1}):
        with pytest.raises(ValueError, match="at most 32 gallery rows"):
            sc.search(q, g, 33, **kw)
    with pytest.raises(ValueError, match="route = 'both'"):
        sc.search(q, g, 100, route="both")
    for k in (1025, 4096):
        with pytest.raises(ValueError, match="1 <= k <= 1024"):
            sc.search(q, g, k)
    with pytest.raises(RuntimeError, match="device tensors only"):   # k <= 32: the code of before, and its error
        sc.search(q, g, 32)
    # ids on one side only: the filter's own format errors come before the device error, as at k <= 32
    with pytest.raises(ValueError, match="one side only"):
        sc.search(q, g, 100, query_ids=torch.zeros(4, dtype=torch.int64))
    assert retrieval.WIDE_MAX_K == 1024 and retrieval.wide_max_gallery() == 262144


def test_search_refuses_a_compact_index_at_wide_k():
    import speechclip_plus_amd as sc
    index = object.__new__(sc.CompactGalleryIndex)                    # no device here: the refusal must come before anything is touched
    with pytest.raises(ValueError, match="GalleryIndex"):
        sc.search(torch.zeros(4, 64), index, 33)
    with pytest.raises(ValueError, match="32 candidates"):
        sc.search(torch.zeros(4, 64), index, 1024)


def test_search_states_the_largest_gallery_it_serves_at_wide_k():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import retrieval

    N = retrieval.wide_max_gallery() + 1
    g = torch.zeros(1, 4).expand(N, 4).as_subclass(_OnDevice)
    q = torch.zeros(2, 4).as_subclass(_OnDevice)
    with pytest.raises(ValueError, match="at most N = 262144"):
        sc.search(q, g, 100)
