"""Case builders and the filtered certificate rule of the filtered compact-search tests (tests/test_compact_filter_cpu.py,
tests/test_gpu_compact_filter.py).  Not collected.

The rule under test is tests/filter_cases.py's (row j is admissible for query i iff j < N, live[j] != 0 where a mask is given, and
g_ids[j] != q_ids[i] where ids are given), the arithmetic is tests/compact_cases.py's emulation, and the certificate is restated over
the admissible rows: the candidates are a query's D best ADMISSIBLE rows by coarse score, a query with fewer than D of them is
certified when everything is finite, every other one iff e_k - |e_k| 2^-23 > t + eps, with eps from the gallery norms over the LIVE
rows.  Everything runs on the CPU in int64 / fp64 from seeded generators; no expectation is derived from what a kernel returns, and
every precondition a GPU test leans on is asserted here, once per case."""
import functools

import torch

import compact_cases as cc
import filter_cases as fc
import search_cases as sc_cases


# ---------------------------------------------------------------------------------------------------- the rule, mirrored
def live_eps(em: cc.Emulation, live=None) -> torch.Tensor:
    """[nQ] fp64: retrieval.compact_eps with gmax / gtmax / dmax over the rows with live[j] != 0 (None: em.eps; no live row: zeros)"""
    from speechclip_plus_amd.retrieval import compact_eps
    if live is None:
        return em.eps
    gn = em.gn[:, live != 0]
    top = [float(v) for v in gn.amax(dim=1)] if gn.shape[1] else [0.0, 0.0, 0.0]
    return compact_eps(em.qn, top[0], top[1], top[2], em.Ep)


def filtered_certificate(coarse: torch.Tensor, exact: torch.Tensor, eps: torch.Tensor, D: int, k: int, adm: torch.Tensor):
    """The rule of sc_search_rerank_filtered_f32, mirrored: coarse / exact [nQ, N] (exact is rounded to fp32 first, as the kernel reports
    it), eps [nQ], adm [nQ, N] bool.  Candidates = the D best admissible coarse scores (stable: lower row first among equals).
    -> (certified [nQ] bool, idx [nQ, k] = the candidates' k best by exact value, lower row first among equals, -1 behind the last
    one, margin [nQ] = e_k - |e_k| 2^-23 - t - eps in fp64; +inf where a query has fewer than D candidates)."""
    nQ, N = coarse.shape
    inf = float("inf")
    if N == 0:
        return torch.isfinite(eps), torch.full((nQ, k), -1, dtype=torch.int64), torch.full((nQ,), inf, dtype=torch.float64)
    e32 = exact.float().double()
    n_adm = adm.sum(dim=1)
    cv, ci = torch.sort(coarse.double(), dim=1, descending=True, stable=True)
    _, p = torch.sort((~torch.gather(adm, 1, ci)).to(torch.int8), dim=1, stable=True)          # the admissible columns in front
    cv, ci = torch.gather(cv, 1, p), torch.gather(ci, 1, p)
    Dn = min(D, N)
    cv, ci = cv[:, :Dn], ci[:, :Dn]
    valid = torch.arange(Dn).unsqueeze(0) < n_adm.unsqueeze(1)                                  # [nQ, Dn]
    # by row, then a stable sort by value: ties keep the lower row first; a filler sorts behind every candidate, a real -inf included
    row_key = torch.where(valid, ci, torch.full_like(ci, N))
    row_sorted, q = torch.sort(row_key, dim=1)
    valid_s = torch.gather(valid, 1, q)
    e = torch.gather(e32, 1, row_sorted.clamp(max=N - 1))
    _, pos = torch.sort(torch.where(valid_s, e, torch.full_like(e, -inf)), dim=1, descending=True, stable=True)
    _, front = torch.sort((~torch.gather(valid_s, 1, pos)).to(torch.int8), dim=1, stable=True)
    pos = torch.gather(pos, 1, front)
    ranked = torch.gather(row_sorted, 1, pos)
    ranked_e = torch.gather(e, 1, pos)
    idx = torch.full((nQ, k), -1, dtype=torch.int64)
    m = min(k, Dn)
    keep = torch.arange(m).unsqueeze(0) < n_adm.unsqueeze(1)
    idx[:, :m] = torch.where(keep, ranked[:, :m], idx[:, :m])
    finite = (torch.isfinite(cv) | ~valid).all(dim=1) & (torch.isfinite(torch.gather(e32, 1, ci)) | ~valid).all(dim=1) & torch.isfinite(eps)
    short = n_adm < D
    margin = torch.full((nQ,), inf, dtype=torch.float64)
    if Dn == D:
        e_k, t = ranked_e[:, k - 1], cv[:, D - 1]
        margin = torch.where(short, margin, e_k - e_k.abs() * 2.0 ** -23 - (t + eps.double()))
    return finite & (short | (margin > 0)), idx, margin


def brute_force_certificate(coarse, exact, eps, D, k, adm):
    """the same by a Python loop per query: the check of ``filtered_certificate`` (finite values only)"""
    nQ, N = coarse.shape
    cert, idx = [], torch.full((nQ, k), -1, dtype=torch.int64)
    e32 = exact.float().double()
    for i in range(nQ):
        cols = [j for j in range(N) if bool(adm[i, j])]
        cand = sorted(cols, key=lambda j: (-float(coarse[i, j]), j))[:D]
        best = sorted(cand, key=lambda j: (-float(e32[i, j]), j))
        for r, j in enumerate(best[:k]):
            idx[i, r] = j
        if len(cand) < D:
            cert.append(True)
        else:
            e_k, t = float(e32[i, best[k - 1]]), float(coarse[i, cand[-1]])
            cert.append(e_k - abs(e_k) * 2.0 ** -23 > t + float(eps[i]))
    return torch.tensor(cert, dtype=torch.bool) & torch.isfinite(eps), idx


def exact_lists(exact: torch.Tensor, k: int, q_ids=None, g_ids=None, live=None):
    """(vals64 [nQ, k] fp64, idx [nQ, k]): filter_cases.filtered_topk of the exact scores, the values kept in fp64 (-inf at a filler)"""
    _, idx = fc.filtered_topk(exact, k, q_ids, g_ids, live)
    vals = torch.gather(exact, 1, idx.clamp(min=0)) if exact.shape[1] else torch.zeros(idx.shape, dtype=torch.float64)
    return torch.where(idx >= 0, vals, torch.full_like(vals, float("-inf"))), idx


def min_ulps_apart(exact: torch.Tensor, k: int, adm: torch.Tensor) -> float:
    """the smallest gap among the first k + 1 admissible exact scores of a query (fewer where it has fewer), in fp32 ulps of the
    larger one; +inf when no query has two admissible rows"""
    sv, _ = torch.sort(exact.masked_fill(~adm, float("-inf")), dim=1, descending=True, stable=True)
    sv = torch.cat((sv, torch.full((sv.shape[0], k + 1), float("-inf"), dtype=sv.dtype)), dim=1)[:, : k + 1]
    pair = torch.isfinite(sv[:, 1:])
    gap = (sv[:, :k] - sv[:, 1:]) / cc.ulp32(sv[:, :k])
    return float(gap.masked_fill(~pair, float("inf")).min()) if gap.numel() else float("inf")


# ---------------------------------------------------------------------------------------------------- 1. Gaussian rows, both filters
GAUSS_CHANGED = (130, 66, 64)              # queries whose unfiltered top-k holds an inadmissible row
GAUSS_FEWEST = (369, 270, 130)             # the fewest admissible rows of a query


@functools.lru_cache(maxsize=None)
def gauss_filtered(i: int):
    """compact_cases.GAUSS_CASES[i] with filter_cases.mod_ids(nQ, N, 7) and seeded_live(N, seed + 1, 0.5) at once
    -> (q, gal, em, q_ids, g_ids, live, want_vals64 [nQ, k], want_idx [nQ, k], k, D).  Asserted: every query passes the filtered rule
    on the emulated coarse values with room for the kernel's accumulation noise on both sides (margin > 4 x noise, as
    compact_cases.gauss_compact requires), the first k + 1 admissible exact scores are MIN_ULPS_APART fp32 ulps apart, the rule's
    list is filtered_topk of the exact scores, and the filter changes the answer of GAUSS_CHANGED[i] queries."""
    nQ, N, E, seed, k, D = cc.GAUSS_CASES[i]
    q, gal, em, _, _, k, D = cc.gauss_compact(i)
    q_ids, g_ids = fc.mod_ids(nQ, N, 7)
    live = fc.seeded_live(N, seed + 1, 0.5)
    adm = fc.admissible(nQ, N, q_ids, g_ids, live)
    eps = live_eps(em, live)
    cert, idx, margin = filtered_certificate(em.coarse, em.exact, eps, D, k, adm)
    noise = float(em.acc.max())
    assert bool(cert.all()) and float(margin.min()) > 4 * noise, (float(margin.min()), noise)
    assert min_ulps_apart(em.exact, k, adm) >= cc.MIN_ULPS_APART
    want_vals, want_idx = exact_lists(em.exact, k, q_ids, g_ids, live)
    assert torch.equal(idx, want_idx)
    assert fc.excluded_in_unfiltered_topk(em.exact, k, q_ids, g_ids, live) == GAUSS_CHANGED[i]
    assert int(adm.sum(dim=1).min()) == GAUSS_FEWEST[i] and GAUSS_FEWEST[i] > D
    return q, gal, em, q_ids, g_ids, live, want_vals, want_idx, k, D


def gauss_filtered_figures(i: int):
    """(margin / noise, ulps apart) of gauss_filtered(i): what the round document quotes"""
    q, gal, em, q_ids, g_ids, live, _, _, k, D = gauss_filtered(i)
    adm = fc.admissible(q.shape[0], gal.shape[0], q_ids, g_ids, live)
    _, _, margin = filtered_certificate(em.coarse, em.exact, live_eps(em, live), D, k, adm)
    return float(margin.min()) / float(em.acc.max()), min_ulps_apart(em.exact, k, adm)


# ---------------------------------------------------------------------------------------------------- 3. the rule's three branches
LIVE_COUNTS = (40, 32, 20, 3, 0)           # more than D, exactly D, between k and D, fewer than k, none


@functools.lru_cache(maxsize=None)
def few_live_case(n_live: int):
    """case 0 of compact_cases.GAUSS_CASES (130 x 890 x 512, k 10, D 32) with only ``n_live`` rows of a seeded permutation live
    -> (q, gal, live, want_vals64, want_idx, k, D).  Asserted: every query is certified by the mirrored rule - by the inequality with
    room for 4 x the accumulation noise where D or more rows are live, by the "fewer than D candidates" clause below that - and the
    rule's list is the exact one."""
    q, gal, em, _, _, k, D = cc.gauss_compact(0)
    nQ, N = q.shape[0], gal.shape[0]
    live = torch.zeros(N, dtype=torch.bool)
    live[torch.randperm(N, generator=torch.Generator().manual_seed(1234))[:n_live]] = True
    assert int(live.sum()) == n_live
    adm = fc.admissible(nQ, N, live=live)
    cert, idx, margin = filtered_certificate(em.coarse, em.exact, live_eps(em, live), D, k, adm)
    assert bool(cert.all())
    if n_live >= D:
        assert float(margin.min()) > 4 * float(em.acc.max()), (float(margin.min()), float(em.acc.max()))
    else:
        assert bool(torch.isinf(margin).all())
    assert min_ulps_apart(em.exact, k, adm) >= 4
    want_vals, want_idx = exact_lists(em.exact, k, live=live)
    assert torch.equal(idx, want_idx) and int((want_idx >= 0).sum(dim=1).max()) == min(k, n_live)
    return q, gal, live, want_vals, want_idx, k, D


CROWD_LEFT_IN = 40                         # crowd rows still admissible for query 0 in the second crowd case: more than D


@functools.lru_cache(maxsize=None)
def crowd_filtered(excluded: int):
    """compact_cases.crowd_case() with query i carrying id i, the first ``excluded`` crowd rows carrying query 0's id and every
    other gallery row a distinct negative id -> (q, gal, q_ids, g_ids, want_idx, k, D).  Asserted: with all 48 crowd rows excluded
    every query passes the filtered rule with more than 10 x the accumulation noise to spare (query 0 failed it unfiltered); with 8
    excluded 40 remain, more than D, and query 0 fails it by more than 10 x the noise while the others pass; the remaining crowd's
    exact gaps keep their order under the exact fallback's scores."""
    q, gal, _, k, D = cc.crowd_case()
    nQ, N = q.shape[0], gal.shape[0]
    assert excluded in (cc.CROWD_N, cc.CROWD_N - CROWD_LEFT_IN) and CROWD_LEFT_IN > D
    q_ids = torch.arange(nQ, dtype=torch.int64)
    g_ids = -1 - torch.arange(N, dtype=torch.int64)
    g_ids[cc.CROWD_FIRST: cc.CROWD_FIRST + excluded] = 0
    adm = fc.admissible(nQ, N, q_ids, g_ids)
    assert int((~adm).sum()) == excluded and int((~adm[0]).sum()) == excluded
    em = cc.Emulation(q, gal)
    cert, _, margin = filtered_certificate(em.coarse, em.exact, em.eps, D, k, adm)
    noise = float(em.acc.max())
    if excluded == cc.CROWD_N:
        assert bool(cert.all()) and float(margin.min()) > 10 * noise, (float(margin.min()), noise)
    else:
        assert not bool(cert[0]) and float(margin[0]) < -10 * noise, (float(margin[0]), noise)
        assert bool(cert[1:].all()) and float(margin[1:].min()) > 10 * noise, (float(margin[1:].min()), noise)
    _, want_idx = exact_lists(em.exact, k, q_ids, g_ids)
    if excluded != cc.CROWD_N:
        first = cc.CROWD_FIRST + excluded
        assert want_idx[0].tolist() == list(range(first, first + k))
    assert min_ulps_apart(em.exact, k, adm) >= 4
    return q, gal, q_ids, g_ids, want_idx, k, D


# ---------------------------------------------------------------------------------------------------- 4. a bad row healed
BAD_NAN_ROW, BAD_HUGE_ROW, BAD_SCALE = 130, 7, 1e6


@functools.lru_cache(maxsize=None)
def bad_rows_case():
    """case 2 of compact_cases.GAUSS_CASES (66 x 300 x 64, k 5, D 16) with gallery row 130 all NaN and row 7 times 1e6
    -> (q, gal, live, want_vals64, want_idx, k, D), ``live`` False at exactly those two rows.  Asserted: over all rows eps is not
    finite (nothing can be certified); over the live rows it is finite and below 0.006, every query passes the filtered rule with
    more than 4 x the accumulation noise to spare, and the rule's list is the exact list over the live rows."""
    q, gal0, em0, _, _, k, D = cc.gauss_compact(2)
    gal = gal0.clone()
    gal[BAD_NAN_ROW] = float("nan")
    gal[BAD_HUGE_ROW] *= BAD_SCALE
    nQ, N = q.shape[0], gal.shape[0]
    live = torch.ones(N, dtype=torch.bool)
    live[[BAD_NAN_ROW, BAD_HUGE_ROW]] = False
    em = cc.Emulation(q, gal)
    assert not bool(torch.isfinite(em.eps).any())
    eps = live_eps(em, live)
    assert bool(torch.isfinite(eps).all()) and float(eps.max()) < 0.006, float(eps.max())
    adm = fc.admissible(nQ, N, live=live)
    # the dead columns hold NaN / huge values: they are inadmissible, so the reference reads zeros there
    exact = em.exact.masked_fill(~adm, 0.0)
    coarse = em.coarse.masked_fill(~adm, 0.0)
    cert, idx, margin = filtered_certificate(coarse, exact, eps, D, k, adm)
    noise = float(em0.acc.max())
    assert bool(cert.all()) and float(margin.min()) > 4 * noise, (float(margin.min()), noise)
    cert32, idx32, margin32 = filtered_certificate(coarse, exact, eps, 32, k, adm)         # and at the depth ``search`` uses
    assert bool(cert32.all()) and float(margin32.min()) > 4 * noise and torch.equal(idx32, idx)
    assert min_ulps_apart(exact, k, adm) >= cc.MIN_ULPS_APART
    want_vals, want_idx = exact_lists(exact, k, live=live)
    assert torch.equal(idx, want_idx)
    assert not bool(((want_idx == BAD_NAN_ROW) | (want_idx == BAD_HUGE_ROW)).any())
    return q, gal, live, want_vals, want_idx, k, D


# ---------------------------------------------------------------------------------------------------- 5. the fallback's chunk merge
MERGE_CHUNK = 256
MERGE_K = 8
MERGE_INF_ROW, MERGE_INF_COL = 650, 5
MERGE_LIVE = (10, 200, 300, 301, 400, 410, 420, 520, 600, MERGE_INF_ROW)      # 2 rows in chunk 0, 5 in chunk 1, 3 in chunk 2
MERGE_TWINS = ((10, 520), (200, 600))      # bit-identical rows in different chunks; the second pair scores lowest for every query
MERGE_GROUP_B_ID = 7                       # carried by rows 300, 301, 400: a query with this id has 7 admissible rows, fewer than k


@functools.lru_cache(maxsize=None)
def merge_case():
    """Integer data (exact on every path), 12 x 700 x 64, k = 8, gallery chunks of 256 rows: ten live rows, two of them in the first
    chunk (fewer than k), twins across chunks, and live row 650 in the last chunk zero but for a -inf in column 5, where every query
    is positive - a real -inf score, and an infinite gallery norm, so no query can be certified.  Even queries carry row 650's id
    (nine admissible rows: the twins 200 / 600 tie for the k-th place, and the lower row must win it); odd queries carry id 7 (seven
    admissible rows: six numbers, the -inf row, one filler).  -> (q, gal, q_ids, g_ids, live, want_vals64, want_idx, k)"""
    nQ, N, E, k = 12, 700, 64, MERGE_K
    g = torch.Generator().manual_seed(404)
    q = torch.randint(1, 4, (nQ, E), generator=g).float()
    gal = torch.randint(-3, 4, (N, E), generator=g).float()
    gal[200] = -3.0                                                  # the lowest score a positive query can give
    for a, b in MERGE_TWINS:
        gal[b] = gal[a]
        assert a // MERGE_CHUNK != b // MERGE_CHUNK
    gal[MERGE_INF_ROW] = 0.0
    gal[MERGE_INF_ROW, MERGE_INF_COL] = float("-inf")
    live = torch.zeros(N, dtype=torch.bool)
    live[list(MERGE_LIVE)] = True
    assert 0 < int(live[:MERGE_CHUNK].sum()) < k and int(live[-(N % MERGE_CHUNK):].sum()) == 3 and N // MERGE_CHUNK == 2
    g_ids = -1 - torch.arange(N, dtype=torch.int64)
    g_ids[[300, 301, 400]] = MERGE_GROUP_B_ID
    g_ids[MERGE_INF_ROW] = 9
    q_ids = torch.where(torch.arange(nQ) % 2 == 0, 9, MERGE_GROUP_B_ID).to(torch.int64)
    exact = torch.zeros(nQ, N, dtype=torch.float64)
    finite_rows = torch.arange(N) != MERGE_INF_ROW
    exact[:, finite_rows] = q.double() @ gal[finite_rows].double().t()
    exact[:, MERGE_INF_ROW] = float("-inf")                          # 0 x finite = 0 everywhere else, positive x -inf in column 5
    assert bool((q[:, MERGE_INF_COL] > 0).all())
    adm = fc.admissible(nQ, N, q_ids, g_ids, live)
    assert adm.sum(dim=1).tolist() == [9, 7] * (nQ // 2)
    want_vals, want_idx = exact_lists(exact, k, q_ids, g_ids, live)
    lowest = exact[:, [j for j in MERGE_LIVE if j not in (200, 600, MERGE_INF_ROW)]].min(dim=1).values
    assert bool((exact[:, 200] < lowest).all()) and bool((exact[:, 200] == exact[:, 600]).all())
    for i in range(nQ):
        row = want_idx[i].tolist()
        if i % 2 == 0:                                               # the tie for the k-th place goes to the lower row
            assert row[-1] == 200 and 600 not in row and MERGE_INF_ROW not in row and row.index(10) < row.index(520)
        else:                                                        # the real -inf is listed, ahead of the one filler
            assert row[-2:] == [MERGE_INF_ROW, -1] and row[-3] == 600 and row[-4] == 200
    return q, gal, q_ids, g_ids, live, want_vals, want_idx, k
