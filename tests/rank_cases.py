"""The rule, the id builders and the degenerate case of the retrieval-rank tests (tests/test_ranks_cpu.py, tests/test_gpu_ranks.py).
Not collected.

``ahead_reference`` is the rule of ``retrieval._recall`` / csrc/rank.hip written out on a score matrix the CPU holds in int64 or fp64;
nothing here is derived from what the kernel returns.  The score builders are those of tests/search_cases.py."""
import functools

import torch

import search_cases as sc_cases


# ---------------------------------------------------------------------------------------------------- the rule
def ahead_reference(score: torch.Tensor, q_ids: torch.Tensor, c_ids: torch.Tensor):
    """score [Q, C] int64 or fp64 (NaN and inf allowed), candidate c correct for query q iff c_ids[c] == q_ids[q] ->
    (ahead [Q] int64, best [Q] fp64).  best = the largest score over the correct, non-NaN candidates (-inf: there is none);
    ahead = #{c : score > best} + #{c not correct : score == best or score is NaN}; a query without a correct candidate or whose best
    is not finite gets ahead = C (it never hits)."""
    s = score.double()
    Q, C = s.shape
    if C == 0:
        return torch.zeros(Q, dtype=torch.int64), torch.full((Q,), float("-inf"), dtype=torch.float64)
    correct = q_ids.view(Q, 1) == c_ids.view(1, C)
    nan = torch.isnan(s)
    usable = correct & ~nan
    best = torch.where(usable, s, torch.full_like(s, float("-inf"))).amax(dim=1)
    b = best.view(Q, 1)
    ahead = (s > b).sum(dim=1) + (~correct & ((s == b) | nan)).sum(dim=1)
    ok = usable.any(dim=1) & torch.isfinite(best)
    return torch.where(ok, ahead, torch.full_like(ahead, C)), best


def both_directions(score: torch.Tensor, a_ids: torch.Tensor, b_ids: torch.Tensor):
    """-> {"ahead_AB", "best_AB", "ahead_BA", "best_BA"} of the [nA, nB] score matrix"""
    ahead_ab, best_ab = ahead_reference(score, a_ids, b_ids)
    ahead_ba, best_ba = ahead_reference(score.t(), b_ids, a_ids)
    return {"ahead_AB": ahead_ab, "best_AB": best_ab, "ahead_BA": ahead_ba, "best_BA": best_ba}


# ---------------------------------------------------------------------------------------------------- ids
def caption_ids(nA: int, nB: int, seed: int):
    """5 rows of A per id (5 captions of an image).  B: one row per id, in shuffled order, except that every 11th row repeats its
    neighbour's id (a query with two correct candidates) and every 7th carries an id A does not know - so that id of A is absent
    from B; ids of B beyond A's last are absent from A, and ids of A beyond B's last are absent from B."""
    a_ids = 10 + torch.arange(nA) // 5
    j = torch.arange(nB)
    b_ids = 10 + j - (j % 11 == 5).long()
    b_ids = torch.where(j % 7 == 3, -1 - j, b_ids)
    return a_ids, b_ids[torch.randperm(nB, generator=torch.Generator().manual_seed(seed))]


def planted_ids(planted: torch.Tensor, nB: int):
    """the correct candidate of query i is the one planted at rank i % k; every other id of B is unique"""
    nA, k = planted.shape
    a_ids = torch.arange(nA)
    b_ids = -1 - torch.arange(nB)
    for i in range(nA):
        b_ids[planted[i, i % k]] = i
    return a_ids, b_ids


# ---------------------------------------------------------------------------------------------------- degenerate values
NAN_A, ZERO_A, LONELY_A, NAN_B, INF_B = 7, 64, 100, 33, 129


@functools.lru_cache(maxsize=None)
def degenerate_case(nA: int = 130, nB: int = 140, E: int = 64, seed: int = 17):
    """integer data (exact scores) with one NaN row in A, one all-zero row in A (its zeros of both signs: every score of the row is a
    zero, ties everywhere), one row of A whose id B does not hold, one NaN row and one +inf row in B.  -> (A fp32, B fp32, a_ids, b_ids,
    expected dict); the expectation treats the +inf row as the documented rule says: an infinity becomes NaN in the split, so the row
    scores NaN against every query."""
    q, gal = sc_cases.int_case(nA, nB, E, seed)
    a_ids, b_ids = caption_ids(nA, nB, seed)
    a_ids = a_ids.clone()
    a_ids[LONELY_A] = 10 ** 12                                        # beyond int32, in no row of B
    A, B = q.float(), gal.float()
    A[ZERO_A] = 0.0
    A[ZERO_A, ::2] = -0.0
    A[NAN_A, 5] = float("nan")
    B[NAN_B, 0] = float("nan")
    B[INF_B, 63] = float("inf")
    qz = q.clone()
    qz[ZERO_A] = 0
    s = (qz.long() @ gal.long().t()).double()
    s[NAN_A, :] = float("nan")
    s[:, NAN_B] = float("nan")
    s[:, INF_B] = float("nan")
    return A, B, a_ids, b_ids, both_directions(s, a_ids, b_ids)
