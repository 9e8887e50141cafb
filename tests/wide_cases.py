"""Wide search (csrc/topk_wide.hip): the order contract restated in plain torch, the comparison the GPU tests use, and the row builders.
Nothing here runs a kernel; every expectation of tests/test_gpu_wide_search.py comes from ``restated_topk``."""
import torch

NAN, INF = float("nan"), float("inf")


def eligible(V: int, q_id=None, g_ids=None, live=None) -> torch.Tensor:
    """[V] bool: column j is eligible iff live is None or live[j] != 0, and the ids are None or g_ids[j] != q_id"""
    e = torch.ones(V, dtype=torch.bool)
    if live is not None:
        e &= live[:V] != 0
    if g_ids is not None:
        e &= g_ids[:V] != q_id
    return e


def restated_topk(scores: torch.Tensor, V: int, k: int, q_ids=None, g_ids=None, live=None):
    """The contract, row by row: the first V columns as fp32 bits, ineligible columns dropped, a STABLE descending sort with NaN above
    every number and -0 == +0 (stable: the lower column first among equals), -inf / -1 behind the last eligible column.
    scores [rows, >= V] fp32 on the CPU -> (vals [rows, k] fp32 - the matrix's own bits -, idx [rows, k] int32)."""
    assert scores.dtype == torch.float32 and scores.device.type == "cpu" and (q_ids is None) == (g_ids is None)
    rows = scores.shape[0]
    vals = torch.full((rows, k), -INF, dtype=torch.float32)
    idx = torch.full((rows, k), -1, dtype=torch.int32)
    for r in range(rows):
        cols = torch.nonzero(eligible(V, None if q_ids is None else q_ids[r], g_ids, live)).squeeze(1)
        v = scores[r, :V][cols]
        key = v.double() + 0.0                                       # -0 + 0 = +0: one key for both zeros
        key = torch.where(torch.isposinf(key), torch.full_like(key, 1e308), key)          # +inf stays above every fp32 number ...
        key = torch.where(torch.isnan(key), torch.full_like(key, INF), key)               # ... and below every NaN
        order = torch.sort(key, stable=True, descending=True).indices[:k]
        n = order.numel()
        vals[r, :n] = v[order]
        idx[r, :n] = cols[order].int()
    return vals, idx


def same_bits(got, want) -> bool:
    """bit for bit: the same columns in the same places, and the same 32 bits in every value (-0 is not +0, NaN payloads count)"""
    (gv, gi), (wv, wi) = got, want
    return (gv.dtype == wv.dtype == torch.float32 and gv.shape == wv.shape and gi.shape == wi.shape
            and torch.equal(gi.to(torch.int64), wi.to(torch.int64)) and torch.equal(gv.contiguous().view(torch.int32), wv.contiguous().view(torch.int32)))


def padded(data: torch.Tensor, ld: int, offset: int = 0):
    """data [rows, V] -> (buf, view): ``view`` [rows, ld] with view[:, :V] = data lies ``offset`` floats into ``buf``; the slack columns
    V .. ld - 1 alternate NaN and +inf (the best possible scores: one of them in a result is visible at once), and so does the
    memory in front of and behind the rows"""
    rows, V = data.shape
    assert ld >= V and 0 <= offset < 4
    buf = torch.empty(rows * ld + 8, dtype=torch.float32)
    buf[0::2] = NAN
    buf[1::2] = INF
    view = buf[offset: offset + rows * ld].view(rows, ld)
    view[:, :V] = data
    return buf, view


def mixed_rows(V: int, seed: int) -> torch.Tensor:
    """[4, V]: a continuous row, a row quantised to eighths (ties everywhere), a row with NaN, +-inf and +-0 sprinkled, a row over a
    7-value set"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(4, V, generator=g)
    x[1] = torch.round(x[1] * 8) / 8
    sp = torch.tensor([NAN, INF, -INF, 0.0, -0.0, 1.5, 1.5])
    pick = torch.randint(0, 4, (V,), generator=g) == 0
    x[2] = torch.where(pick, sp[torch.randint(0, 7, (V,), generator=g)], x[2])
    x[3] = seven_values(V, seed + 1)
    return x


SEVEN = (-2.0, -0.5, -0.0, 0.0, 0.25, 1.0, 3.0)                        # -0 and +0 are one value of the order: six distinct keys


def seven_values(V: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(SEVEN)[torch.randint(0, 7, (V,), generator=g)]
