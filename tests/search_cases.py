"""Case builders and the fp64 yardstick of the gallery-search tests (tests/test_search_cpu.py, tests/test_gpu_search.py).  Not collected.

Every builder returns CPU tensors from a seeded generator; every expected result is computed on the CPU in int64 or fp64, once per
case, and is never derived from what the kernel returns."""
import functools

import torch

TILE = 128                                   # the kernel's column tile (and row tile)


def roundup(x: int, m: int) -> int:
    return -(-x // m) * m


def slab_tiles(N: int, S: int):
    """(column tiles, tiles per slab) of a gallery of N rows cut into S slabs"""
    nT = roundup(N, TILE) // TILE
    return nT, max(-(-nT // S), 1)


# ---------------------------------------------------------------------------------------------------- exact integer data
def int_case(nQ: int, N: int, E: int, seed: int):
    """queries / gallery drawn from the integers -3 .. 3: bf16 holds them exactly, the lower split terms are zero, every product and
    partial sum is an exact integer far below 2^24 - the kernel's fp32 scores must EQUAL the int64 product, and ties abound."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-3, 4, (nQ, E), generator=g)
    gal = torch.randint(-3, 4, (N, E), generator=g)
    return q, gal


def stable_topk(score: torch.Tensor, k: int):
    """score [nQ, N] (int64 or fp64, no NaN) -> (vals [nQ, k] fp32, idx [nQ, k] int64) of the contract: a stable descending sort, the
    tail past the N-th entry -inf / -1"""
    nQ, N = score.shape
    vals = torch.full((nQ, k), float("-inf"), dtype=torch.float32)
    idx = torch.full((nQ, k), -1, dtype=torch.int64)
    if N > 0 and nQ > 0:
        sv, si = torch.sort(score, dim=1, descending=True, stable=True)
        m = min(k, N)
        vals[:, :m] = sv[:, :m].to(torch.float32)
        idx[:, :m] = si[:, :m]
    return vals, idx


def int_expected(q: torch.Tensor, gal: torch.Tensor, k: int):
    return stable_topk(q.long() @ gal.long().t(), k)


def ramp_case(nQ: int, N: int, E: int, increasing: bool):
    """scores that increase (every tile brings k new bests) or decrease (none after the first) with the gallery index: the gallery's
    first coordinate is a ramp of integers < 2^24 / 3 (exact in the three-way split), the queries are positive integers there and
    zero elsewhere"""
    q = torch.zeros(nQ, E, dtype=torch.int64)
    q[:, 0] = 1 + torch.arange(nQ) % 3
    gal = torch.zeros(N, E, dtype=torch.int64)
    gal[:, 0] = torch.arange(N) if increasing else N - torch.arange(N)
    return q, gal


# ---------------------------------------------------------------------------------------------------- float data, fp64 yardstick
def unit_gauss(n: int, E: int, seed: int) -> torch.Tensor:
    x = torch.randn(n, E, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float()            # what the kernel sees: the fp32 rows


def yardstick(q: torch.Tensor, gal: torch.Tensor):
    """fp32 rows -> (fp64 scores [nQ, N], bound [nQ, N]) with bound = (6 Ep + 8) 2^-24 sum_i |q_i| |g_i|: the summation bound of the
    six-block fp32 accumulation (6 Ep products) plus the dropped low products of the three-way split, evaluated in fp64"""
    Ep = roundup(q.shape[1], 64)
    qd, gd = q.double(), gal.double()
    return qd @ gd.t(), (6 * Ep + 8) * 2.0 ** -24 * (qd.abs() @ gd.abs().t())


@functools.lru_cache(maxsize=None)
def gauss_case(nQ: int, N: int, E: int, seed: int):
    q, gal = unit_gauss(nQ, E, seed), unit_gauss(N, E, seed + 1)
    s64, bound = yardstick(q, gal)
    return q, gal, s64, bound


PLANT_COS0, PLANT_STEP = 0.90, 0.05


@functools.lru_cache(maxsize=None)
def planted_case(nQ: int, N: int, E: int, k: int, seed: int):
    """Unit rows; for every query k gallery rows are planted at cosines 0.90, 0.85, 0.80, ... (gaps of 0.05); every other pair is
    random (|cos| below about 0.25 at E >= 512).  -> (q, gal, planted [nQ, k] gallery indices in rank order, s64, bound)."""
    assert nQ * k <= N
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(nQ, E, generator=gen, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    gal = torch.randn(N, E, generator=gen, dtype=torch.float64)
    gal = gal / gal.norm(dim=1, keepdim=True)
    planted = torch.randperm(N, generator=gen)[: nQ * k].view(nQ, k)
    for i in range(nQ):
        u = gal[planted[i]]
        u = u - (u @ q[i]).unsqueeze(1) * q[i]                   # orthogonal to the query
        u = u / u.norm(dim=1, keepdim=True)
        c = (PLANT_COS0 - PLANT_STEP * torch.arange(k, dtype=torch.float64)).unsqueeze(1)
        gal[planted[i]] = c * q[i] + (1 - c * c).sqrt() * u
    q, gal = q.float(), gal.float()
    s64, bound = yardstick(q, gal)
    return q, gal, planted, s64, bound


def planted_min_gap_over_bound(s64: torch.Tensor, bound: torch.Tensor, k: int) -> float:
    """min over rows and over the first k fp64 ranks r of (score[r] - score[r + 1]) / max(bound[r], bound[r + 1]): above 4 the fp32
    scores (each within its bound) cannot reorder the first k ranks or admit an outsider, with a factor of two to spare"""
    sv, si = torch.sort(s64, dim=1, descending=True, stable=True)
    b = torch.gather(bound, 1, si)
    gap = sv[:, :k] - sv[:, 1: k + 1]
    return float((gap / torch.maximum(b[:, :k], b[:, 1: k + 1])).min())


def unnormalised(x: torch.Tensor, seed: int) -> torch.Tensor:
    """the rows times positive factors between 0.5 and 4"""
    f = 0.5 + 3.5 * torch.rand(x.shape[0], 1, generator=torch.Generator().manual_seed(seed))
    return x * f


def recall_from_idx(idx: torch.Tensor, query_ids: torch.Tensor, cand_ids: torch.Tensor, ks):
    """recall@k in per cent from the retrieved lists: a query hits at k iff one of its first k items carries its id"""
    hit = cand_ids[idx.clamp(min=0)] == query_ids.unsqueeze(1)
    hit &= idx >= 0
    return {f"recall@{k}": 100.0 * hit[:, :k].any(dim=1).float().mean().item() for k in ks}
