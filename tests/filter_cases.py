"""Case builders and the CPU reference of the filtered gallery-search tests (tests/test_filtered_search_cpu.py,
tests/test_gpu_filtered_search.py).  Not collected.

The rule under test: gallery row j is admissible for query i iff j < N, ``live`` is absent or live[j] != 0, and the ids are absent or
g_ids[j] != q_ids[i] (int64, all 64 bits).  The expected result is a stable descending sort of the admissible columns, computed here
on the CPU in int64 / fp64 and never derived from what a kernel returns.  Every builder asserts its own precondition."""
import functools
import struct

import torch

import search_cases as sc_cases

TILE = sc_cases.TILE


# ---------------------------------------------------------------------------------------------------- the reference
def admissible(nQ: int, N: int, q_ids=None, g_ids=None, live=None) -> torch.Tensor:
    """[nQ, N] bool: the rule"""
    assert (q_ids is None) == (g_ids is None)
    adm = torch.ones(nQ, N, dtype=torch.bool)
    if live is not None:
        assert live.shape == (N,)
        adm &= (live != 0).unsqueeze(0)
    if q_ids is not None:
        assert q_ids.dtype == g_ids.dtype == torch.int64 and q_ids.shape == (nQ,) and g_ids.shape == (N,)
        adm &= g_ids.unsqueeze(0) != q_ids.unsqueeze(1)
    return adm


def filtered_topk(score: torch.Tensor, k: int, q_ids=None, g_ids=None, live=None):
    """score [nQ, N] (int64 or fp64, no NaN; -inf allowed) -> (vals [nQ, k] fp32, idx [nQ, k] int64) of the contract over the
    admissible columns: a stable descending sort of them, -inf / -1 behind the last one.  A real -inf keeps its column."""
    nQ, N = score.shape
    vals = torch.full((nQ, k), float("-inf"), dtype=torch.float32)
    idx = torch.full((nQ, k), -1, dtype=torch.int64)
    if N == 0 or nQ == 0:
        return vals, idx
    adm = admissible(nQ, N, q_ids, g_ids, live)
    sv, si = torch.sort(score, dim=1, descending=True, stable=True)
    # the admissible columns in front, each group in its sorted order (a stable sort on one bit)
    _, p = torch.sort((~torch.gather(adm, 1, si)).to(torch.int8), dim=1, stable=True)
    sv, si = torch.gather(sv, 1, p), torch.gather(si, 1, p)
    m = min(k, N)
    keep = torch.arange(m).unsqueeze(0) < adm.sum(dim=1, keepdim=True)
    vals[:, :m] = torch.where(keep, sv[:, :m].to(torch.float32), vals[:, :m])
    idx[:, :m] = torch.where(keep, si[:, :m], idx[:, :m])
    return vals, idx


def brute_force_topk(score: torch.Tensor, k: int, q_ids=None, g_ids=None, live=None):
    """the same by a Python loop per row: the check of ``filtered_topk``"""
    nQ, N = score.shape
    vals = torch.full((nQ, k), float("-inf"), dtype=torch.float32)
    idx = torch.full((nQ, k), -1, dtype=torch.int64)
    for i in range(nQ):
        cols = [j for j in range(N) if (live is None or bool(live[j])) and (q_ids is None or int(g_ids[j]) != int(q_ids[i]))]
        cols.sort(key=lambda j: (-float(score[i, j]), j))
        for r, j in enumerate(cols[:k]):
            vals[i, r] = float(score[i, j])
            idx[i, r] = j
    return vals, idx


# ---------------------------------------------------------------------------------------------------- filters
def mod_ids(nQ: int, N: int, m: int = 7):
    """(q_ids [nQ], g_ids [N]) = (i % m, j % m): every query excludes about N / m rows spread over every tile"""
    return torch.arange(nQ, dtype=torch.int64) % m, torch.arange(N, dtype=torch.int64) % m


def seeded_live(N: int, seed: int, dead: float = 0.5) -> torch.Tensor:
    """bool [N] with about ``dead`` of the rows False"""
    return torch.rand(N, generator=torch.Generator().manual_seed(seed)) >= dead


def high_word_ids(n: int, c: int = -5) -> torch.Tensor:
    """c + (j % 3) 2^32: ids that differ only above bit 31"""
    ids = c + (torch.arange(n, dtype=torch.int64) % 3) * 2 ** 32
    assert len(set((ids & 0xffffffff).tolist())) == 1 or n == 0, "the low words must all be equal"
    assert n < 3 or len(set(ids.tolist())) == 3
    return ids


def excluded_in_unfiltered_topk(score: torch.Tensor, k: int, q_ids, g_ids, live=None) -> int:
    """number of queries whose UNFILTERED top-k holds at least one inadmissible row: there the filter changes the answer"""
    _, idx = sc_cases.stable_topk(score, k)
    adm = admissible(score.shape[0], score.shape[1], q_ids, g_ids, live)
    ok = idx >= 0
    return int((ok & ~torch.gather(adm, 1, idx.clamp(min=0))).any(dim=1).sum())


# ---------------------------------------------------------------------------------------------------- fillers in the middle
SLAB_CASE = (200, 640, 64, 32, 5)          # nQ, N, E, k, S: five column tiles, one per slab at S = 5; 3 + 2 tiles at S = 2
SLAB_QUERY_IDS = (100, 101, 300, 999)


@functools.lru_cache(maxsize=None)
def slab_case():
    """Integer data with a gallery sorted by id: id 100 owns exactly tile 0 (columns 0 .. 127), id 101 all but the last 3 columns of
    tile 1, ids 102 .. 104 those three, tile 2 has 128 distinct ids, id 300 owns tiles 3 and 4 - a whole slab at S = 2, two at
    S = 5.  Queries carry 100, 101, 300 and 999 (no such gallery id) in turn.  -> (q, gal, q_ids, g_ids)"""
    nQ, N, E, k, S = SLAB_CASE
    q, gal = sc_cases.int_case(nQ, N, E, seed=77)
    g_ids = torch.empty(N, dtype=torch.int64)
    g_ids[:128] = 100
    g_ids[128:253] = 101
    g_ids[253:256] = torch.tensor([102, 103, 104])
    g_ids[256:384] = 105 + torch.arange(128)
    g_ids[384:] = 300
    assert bool((g_ids[1:] >= g_ids[:-1]).all()), "sorted by id"
    q_ids = torch.tensor(SLAB_QUERY_IDS, dtype=torch.int64)[torch.arange(nQ) % len(SLAB_QUERY_IDS)]
    adm = admissible(nQ, N, q_ids, g_ids)
    for slabs, want_short in ((5, True), (2, False)):
        nT, T = sc_cases.slab_tiles(N, slabs)
        counts = torch.stack([adm[:, s * T * TILE: min(N, (s + 1) * T * TILE)].sum(dim=1) for s in range(slabs)], dim=1)
        assert bool((counts == 0).any()), f"S = {slabs}: no slab without an admissible column"
        if want_short:
            assert bool(((counts > 0) & (counts < k)).any()), f"S = {slabs}: no slab with fewer than k admissible columns"
    assert int((adm[:, 128:256].sum(dim=1) == 3).sum()) == nQ // 4
    return q, gal, q_ids, g_ids


# ---------------------------------------------------------------------------------------------------- planted order
PLANT_K = 7


@functools.lru_cache(maxsize=None)
def planted_filter_case(E: int):
    """search_cases.planted_case(70, 1500, E, 10, 11) with query i carrying id i, its planted rows of rank 0, 1, 2 carrying id i too
    and every other row a distinct negative id: the first 7 admissible ranks are the planted ranks 3 .. 9.
    -> (q, gal, planted, s64, bound, q_ids, g_ids)"""
    nQ, N, k = 70, 1500, 10
    q, gal, planted, s64, bound = sc_cases.planted_case(nQ, N, E, k, 11)
    q_ids = torch.arange(nQ, dtype=torch.int64)
    g_ids = -1 - torch.arange(N, dtype=torch.int64)
    for i in range(nQ):
        g_ids[planted[i, :3]] = i
    adm = admissible(nQ, N, q_ids, g_ids)
    assert bool((adm.sum(dim=1) == N - 3).all())
    masked = s64.masked_fill(~adm, float("-inf"))
    _, want = filtered_topk(s64, PLANT_K, q_ids, g_ids)
    assert torch.equal(want, planted[:, 3:10])
    gap = sc_cases.planted_min_gap_over_bound(masked, bound, PLANT_K)
    assert gap > 4.0, gap                 # the fp32 scores cannot reorder the first 7 admissible ranks or admit an outsider
    return q, gal, planted, s64, bound, q_ids, g_ids


def planted_filter_gap(E: int) -> float:
    q, gal, planted, s64, bound, q_ids, g_ids = planted_filter_case(E)
    adm = admissible(s64.shape[0], s64.shape[1], q_ids, g_ids)
    return sc_cases.planted_min_gap_over_bound(s64.masked_fill(~adm, float("-inf")), bound, PLANT_K)


# ---------------------------------------------------------------------------------------------------- list words
def word(value: float, col: int) -> int:
    """the 64-bit list word of (value, column) as a signed int64: key << 32 | ~column with the key of csrc/topk.hip (float order,
    -0 == +0, every NaN 0xffffffff, -inf 0x007fffff)"""
    if value != value:
        key = 0xffffffff
    else:
        u = struct.unpack("<I", struct.pack("<f", value))[0]
        key = (u ^ (0xffffffff if u >> 31 else 0x80000000)) & 0xffffffff
        if key == 0x7fffffff:
            key = 0x80000000
    w = (key << 32) | (~col & 0xffffffff)
    return w - (1 << 64) if w >= (1 << 63) else w
