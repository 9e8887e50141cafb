"""Helpers of tests/test_gpu_neg_loss.py and tests/test_neg_loss_cpu.py (not collected on their own): seeded inputs and the fp64
reference of the contrastive loss with a negative bank (csrc/infonce_neg.hip) - oracle.loss_ref's arithmetic with, per anchor, a list
of bank rows added to the a2b denominator, under torch autograd.  Nothing here needs a GPU."""
import math

import torch

import loss_cases as lc

# (Bg, E, N, M): one row; one float4 beside a one-slot list; one tile less one row at three 16-byte pieces per lane; a ragged second
# tile with a list of 33 (a group of four with one slot); a partial chunk at 3 x 3 tiles; four chunks of 64; the longest list on
# sixteen chunks; 8 x 8 tiles, one chunk of 64
SHAPE_SWEEP = [(1, 4, 3, 2), (2, 20, 5, 1), (63, 768, 300, 32), (65, 68, 300, 33), (130, 100, 1000, 40), (200, 64, 5000, 256),
               (64, 512, 6000, 1024), (512, 100, 2000, 64)]
MAIN = (130, 100, 1000, 40)


def make_bank(Bm, ids, N, seed):
    """Unit Gaussian rows [N, E] whose first min(Bg, N / 2) rows are the batch's own B rows under the batch's ids; the other rows carry
    ids no batch row has.  -> (bank, bank_ids)"""
    Bg, E = Bm.shape
    g = torch.Generator().manual_seed(seed)
    bank = torch.nn.functional.normalize(torch.randn(N, E, generator=g), dim=-1)
    n_own = min(Bg, N // 2)
    bank[:n_own] = Bm[:n_own]
    top = int(ids.max()) + 1 if ids is not None and Bg else 0
    bank_ids = top + torch.arange(N, dtype=torch.int64) // 3
    if ids is not None:
        bank_ids[:n_own] = ids[:n_own]
    return bank, bank_ids


def true_lists(A, bank, ids, bank_ids, M):
    """The true top M of every anchor among the bank rows with another id (fp64 scores, ties to the lower row), padded with -1."""
    s = A.double() @ bank.double().t()
    if ids is not None:
        s = s.masked_fill(ids[:, None] == bank_ids[None, :], -math.inf)
    N = bank.shape[0]
    k = min(M, N)
    vals, idx = torch.sort(s, dim=1, descending=True, stable=True)
    idx = torch.where(vals[:, :k] > -math.inf, idx[:, :k], torch.full_like(idx[:, :k], -1))
    out = torch.full((A.shape[0], M), -1, dtype=torch.int64)
    out[:, :k] = idx
    return out


def make_case(Bg, E, N, M, seed=None, with_ids=True):
    """-> dict(A, B, ids, bank, bank_ids, neg_idx) of the sweep: lc.make_pair rows, ids = arange // 5"""
    seed = Bg * 1000 + E + M if seed is None else seed
    A, Bm = lc.make_pair(Bg, E, seed)
    ids = lc.ids_div5(Bg) if with_ids else None
    bank, bank_ids = make_bank(Bm, ids, N, seed + 1)
    neg_idx = true_lists(A, bank, ids, bank_ids, M)
    return {"A": A, "B": Bm, "ids": ids, "bank": bank, "bank_ids": bank_ids if with_ids else None, "neg_idx": neg_idx}


def slot_mask(neg_idx, N, ids, bank_ids):
    """Which slots take part: 0 <= r < N and, with ids, bank_ids[r] is the id of NO row of the batch."""
    ok = (neg_idx >= 0) & (neg_idx < N)
    if ids is not None and N > 0:
        bid = bank_ids[neg_idx.clamp(0, N - 1)]
        ok = ok & ~torch.isin(bid, ids)
    return ok


def neg_loss_reference(A, Bm, ids, bank, bank_ids, neg_idx, temperature=0.07, margin=0.0, dcl=False, a2b=True, b2a=True,
                       trainable=False, log_inv_temp=None, scale=1.0, dtype=torch.float64):
    """oracle.loss_ref.masked_contrastive_loss's expression on ``dtype`` copies, with x[i, n] = it <A_i, bank[neg_idx[i, n]]> of the
    slots that take part added to the row sums:  lse_row[i] = log(sum_j neg_ij e^{l_ij} + sum_n e^{x_in}).
    -> dict(loss, dA, dB, [dT], x (-inf where the slot takes no part), lse_row, lse_col, logits, used)"""
    assert a2b, "the extras enter the a2b denominator"
    Bg, N = A.shape[0], bank.shape[0]
    a = A.detach().to(dtype).requires_grad_(True)
    b = Bm.detach().to(dtype).requires_grad_(True)
    t = None
    if trainable:
        t0 = torch.tensor(math.log(1 / temperature), dtype=torch.float32) if log_inv_temp is None else log_inv_temp.detach().cpu().float()
        t = t0.to(dtype).reshape(()).requires_grad_(True)
        it = t.exp()
    else:
        it = 1.0 / temperature
    eye = torch.eye(Bg, dtype=torch.bool)
    neg_mask_fl = lc.neg_mask(Bg, ids, dcl).type(dtype)
    logits = a @ b.t() * it
    if margin > 0.0:
        logits = logits - margin * eye.type(dtype)
    pos_logits = logits[eye]
    exp_logits = logits.exp() * neg_mask_fl
    ok = slot_mask(neg_idx, N, ids, bank_ids)
    if N > 0:                          # a row behind a slot that takes no part is never read: a select, not a product
        rows = torch.where(ok[..., None], bank.detach().to(dtype)[neg_idx.clamp(0, N - 1)], torch.zeros((), dtype=dtype))
        x = torch.einsum("ie,ime->im", a, rows) * it
    else:
        x = torch.zeros(neg_idx.shape, dtype=dtype) * it
    extra = torch.where(ok, x.exp(), torch.zeros((), dtype=dtype)).sum(1)
    row_sum = exp_logits.sum(1) + extra
    loss = (-pos_logits + torch.log(row_sum)).mean()
    if b2a:
        loss = (loss + (-pos_logits + torch.log(exp_logits.sum(0))).mean()) / 2
    (scale * loss).backward()
    out = {"loss": loss.detach(), "dA": a.grad, "dB": b.grad}
    if trainable:
        out["dT"] = t.grad
    with torch.no_grad():
        out.update(x=torch.where(ok, x, torch.full((), -math.inf, dtype=dtype)).detach(), lse_row=torch.log(row_sum).detach(),
                   lse_col=torch.log(exp_logits.sum(0)).detach(), logits=logits.detach(), used=ok.sum(1).to(torch.int32))
    return out


def x_err(x, ref):
    """max |x - ref| over the slots that take part; inf unless the -inf pattern is the reference's exactly"""
    x, ref = x.detach().double().cpu(), ref.double()
    fin = torch.isfinite(ref)
    if not bool((torch.isneginf(x) == ~fin).all()):
        return float("inf")
    return float((x[fin] - ref[fin]).abs().max()) if bool(fin.any()) else 0.0
