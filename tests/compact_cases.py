"""Case builders, the bf16 emulation and the certificate rule of the compact-search tests (tests/test_compact_search_cpu.py,
tests/test_gpu_compact_search.py).  Not collected.

Everything here runs on the CPU in int64 / fp64 from seeded generators (tests/search_cases.py supplies the data); no expectation is
derived from what a kernel returns, and every precondition a GPU test leans on is asserted here, once per case."""
import functools

import torch

import search_cases as sc_cases
from search_cases import roundup

def FALLBACK_BOUND(Ep: int) -> float:
    """search's score bound on unit rows (the exact fallback's scores)"""
    return (6 * Ep + 8) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- fp32 ulps
def ulp32(x: torch.Tensor) -> torch.Tensor:
    """the spacing of fp32 numbers at |x| (fp64 in, fp64 out; normal range)"""
    _, e = torch.frexp(x.double().abs().clamp(min=2.0 ** -120))
    return torch.pow(2.0, (e - 24).double())


def within_ulps(got: torch.Tensor, want64: torch.Tensor, n: int) -> bool:
    """got fp32 within n fp32 ulps of the fp64 value rounded to fp32"""
    w = want64.float().double()
    return bool(((got.double() - w).abs() <= n * ulp32(w)).all())


# ---------------------------------------------------------------------------------------------------- the arithmetic, emulated
def bf16_image(x32: torch.Tensor) -> torch.Tensor:
    """fp32 rows -> their bf16 roundings (nearest even) as fp32"""
    assert x32.dtype == torch.float32
    return x32.bfloat16().float()


def norms3(x32: torch.Tensor) -> torch.Tensor:
    """[3, R] fp32: |x'|, |x~|, |x' - x~| per row, each accumulated in fp64 and rounded once (what sc_rows_bf16 reports)"""
    xt = bf16_image(x32)
    d = x32.double() - xt.double()
    return torch.stack((x32.double().norm(dim=1), xt.double().norm(dim=1), d.norm(dim=1))).float()


class Emulation:
    """q, gal: the SCALED fp32 rows the kernels see.  exact = the fp64 inner products; coarse = the fp64 products of the bf16 images;
    acc = (Ep + 8) 2^-24 sum |q~| |g~|, the fp32 accumulation bound of the coarse kernel; eps = retrieval.compact_eps from the norms."""

    def __init__(self, q: torch.Tensor, gal: torch.Tensor):
        from speechclip_plus_amd.retrieval import compact_eps
        assert q.dtype == torch.float32 and gal.dtype == torch.float32
        self.Ep = roundup(q.shape[1], 64)
        self.qt, self.gt = bf16_image(q), bf16_image(gal)
        self.exact = q.double() @ gal.double().t()
        self.coarse = self.qt.double() @ self.gt.double().t()
        self.acc = (self.Ep + 8) * 2.0 ** -24 * (self.qt.double().abs() @ self.gt.double().abs().t())
        self.qn, self.gn = norms3(q), norms3(gal)
        top = [float(v) for v in self.gn.amax(dim=1)] if gal.shape[0] else [0.0, 0.0, 0.0]
        self.gmax, self.gtmax, self.dmax = top
        self.eps = compact_eps(self.qn, self.gmax, self.gtmax, self.dmax, self.Ep)       # [nQ] fp64


def certificate(coarse: torch.Tensor, exact: torch.Tensor, eps: torch.Tensor, D: int, k: int):
    """The rule of sc_search_rerank_f32, mirrored: coarse / exact [nQ, N] (exact is rounded to fp32 first, as the kernel reports it),
    eps [nQ].  Candidates = the D best coarse scores (stable); -> (certified [nQ] bool, idx [nQ, k] = the candidates' k best by exact
    value, lower row first among equals, margin [nQ] = e_k - |e_k| 2^-23 - t - eps in fp64; +inf where N <= D)."""
    nQ, N = coarse.shape
    e32 = exact.float().double()
    cv, ci = torch.sort(coarse.double(), dim=1, descending=True, stable=True)
    cv, ci = cv[:, :D], ci[:, :D]
    ci_sorted, _ = torch.sort(ci, dim=1)                        # by row, then a stable sort by value: ties keep the lower row first
    e = torch.gather(e32, 1, ci_sorted)
    ev, pos = torch.sort(e, dim=1, descending=True, stable=True)
    idx = torch.gather(ci_sorted, 1, pos)[:, :k]
    finite = torch.isfinite(cv).all(dim=1) & torch.isfinite(e).all(dim=1) & torch.isfinite(eps)
    if N <= D:
        return finite, idx, torch.full((nQ,), float("inf"), dtype=torch.float64)
    e_k, t = ev[:, k - 1], cv[:, D - 1]
    margin = e_k - e_k.abs() * 2.0 ** -23 - (t + eps.double())
    return finite & (margin > 0), idx, margin


# ---------------------------------------------------------------------------------------------------- CPU test 4: squeezed scores
SQUEEZE = 0.075


def squeezed_case(seed: int, nQ: int = 40, N: int = 300, E: int = 64):
    """unit queries against unit gallery rows that all lie near one direction: the scores of a query crowd together (spread about
    SQUEEZE x the spread of random rows), so the k-th exact value clears the D-th coarse value by about eps - half the rows pass
    the rule, half do not"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(nQ, E, generator=g, dtype=torch.float64)
    m = torch.randn(1, E, generator=g, dtype=torch.float64)
    m = m / m.norm()
    gal = m + SQUEEZE * torch.randn(N, E, generator=g, dtype=torch.float64) / E ** 0.5
    return (q / q.norm(dim=1, keepdim=True)).float(), (gal / gal.norm(dim=1, keepdim=True)).float()


# ---------------------------------------------------------------------------------------------------- GPU test 2: Gaussian rows
GAUSS_CASES = ((130, 890, 512, 31, 10, 32), (66, 700, 768, 41, 10, 32), (66, 300, 64, 51, 5, 16))      # nQ, N, E, seed, k, D
MIN_ULPS_APART = 41


@functools.lru_cache(maxsize=None)
def gauss_compact(i: int):
    """GAUSS_CASES[i] -> (q, gal, em, want_vals64 [nQ, k] fp64, want_idx [nQ, k], k, D) with the preconditions asserted: every row passes
    the rule on the emulated coarse values with room for the kernel's accumulation noise on both sides of it, and the first k + 1
    fp64 scores of every row are at least 41 fp32 ulps apart (the re-rank's rounded values then sort as the fp64 values do)"""
    nQ, N, E, seed, k, D = GAUSS_CASES[i]
    q, gal, s64, _ = sc_cases.gauss_case(nQ, N, E, seed)
    em = Emulation(q, gal)
    assert torch.equal(em.exact, s64)
    cert, idx, margin = certificate(em.coarse, em.exact, em.eps, D, k)
    assert bool(cert.all()) and float(margin.min()) > 4 * float(em.acc.max()), (float(margin.min()), float(em.acc.max()))
    sv, si = torch.sort(s64, dim=1, descending=True, stable=True)
    gap = sv[:, :k] - sv[:, 1: k + 1]
    assert bool((gap >= MIN_ULPS_APART * ulp32(sv[:, :k])).all())
    assert torch.equal(idx, si[:, :k])
    return q, gal, em, sv[:, :k], si[:, :k], k, D


# ---------------------------------------------------------------------------------------------------- GPU test 5: the crowd
CROWD_FIRST, CROWD_N, CROWD_STEP = 100, 48, 1e-4


@functools.lru_cache(maxsize=None)
def crowd_case(seed: int = 5, nQ: int = 66, N: int = 400, E: int = 64, k: int = 10, D: int = 32):
    """48 gallery rows (100 .. 147: across the first tile border) at cosines 1 - 1e-4 j to query 0, every other gallery row random;
    the other queries are random directions orthogonal to query 0, so the crowd scores about 0 against them.  Asserted: query 0
    fails the rule on the emulated coarse values by more than ten times the accumulation noise, every other query passes with that
    room, the crowd's exact gaps exceed 4 (6 Ep + 8) 2^-24 (the exact fallback's scores keep their order) and the first k + 1 exact
    values of every row are 4 fp32 ulps apart.  -> (q, gal, want_idx [nQ, k], k, D)"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(nQ, E, generator=g, dtype=torch.float64)
    q[0] /= q[0].norm()
    q[1:] -= (q[1:] @ q[0]).unsqueeze(1) * q[0]
    q = q / q.norm(dim=1, keepdim=True)
    gal = torch.randn(N, E, generator=g, dtype=torch.float64)
    gal = gal / gal.norm(dim=1, keepdim=True)
    rows = torch.arange(CROWD_FIRST, CROWD_FIRST + CROWD_N)
    assert CROWD_FIRST < sc_cases.TILE < CROWD_FIRST + CROWD_N
    u = gal[rows] - (gal[rows] @ q[0]).unsqueeze(1) * q[0]
    u = u / u.norm(dim=1, keepdim=True)
    c = (1.0 - CROWD_STEP * torch.arange(CROWD_N, dtype=torch.float64)).unsqueeze(1)
    gal[rows] = c * q[0] + (1 - c * c).clamp(min=0).sqrt() * u
    q, gal = q.float(), gal.float()
    em = Emulation(q, gal)
    cert, _, margin = certificate(em.coarse, em.exact, em.eps, D, k)
    noise = float(em.acc.max())
    assert not bool(cert[0]) and float(margin[0]) < -10 * noise, (float(margin[0]), noise)
    assert bool(cert[1:].all()) and float(margin[1:].min()) > 10 * noise, (float(margin[1:].min()), noise)
    sv, si = torch.sort(em.exact, dim=1, descending=True, stable=True)
    assert si[0, :CROWD_N].tolist() == rows.tolist()
    assert float((sv[0, : CROWD_N - 1] - sv[0, 1: CROWD_N]).min()) > 4 * FALLBACK_BOUND(roundup(E, 64))
    assert bool(((sv[:, :k] - sv[:, 1: k + 1]) >= 4 * ulp32(sv[:, :k])).all())
    return q, gal, si[:, :k], k, D


# ---------------------------------------------------------------------------------------------------- GPU test 9: planted margins
@functools.lru_cache(maxsize=None)
def planted_compact(seed: int = 11, k: int = 8):
    """search_cases.planted_case(64, 2000, 512, 8, seed) -> (q, gal, planted [64, 8], want_idx [64, k]); asserted: the first k + 1 fp64
    scores of every row are more than twice search's bound apart, so the existing ``search`` and the compact route must both return
    the fp64 list"""
    q, gal, planted, s64, bound = sc_cases.planted_case(64, 2000, 512, 8, seed)
    assert sc_cases.planted_min_gap_over_bound(s64, bound, k) > 2.0
    _, want = sc_cases.stable_topk(s64, k)
    assert torch.equal(want[:, :8], planted)
    return q, gal, planted, want
