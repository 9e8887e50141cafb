"""Helpers of tests/test_gpu_queue_loss.py and tests/test_queue_loss_cpu.py (not collected on their own): seeded inputs and the fp64
reference of the contrastive loss with a cross-batch queue (csrc/infonce_queue.hip) - oracle.loss_ref's arithmetic with the queue's
admitted rows added to BOTH denominators, under torch autograd:

    x^A_iq = it <A_i, queue_B[q]>,  x^B_jq = it <B_j, queue_A[q]>;  (i, q) admitted iff there are no ids or queue_ids[q] != index[i]
    lse_row_i = log(sum_{j: neg_ij} e^{l_ij} + sum_{q admitted for i} e^{x^A_iq}),  lse_col_j likewise with x^B

Evaluated in fp32 on the CPU the same expression is the yardstick of the device's error.  Nothing here needs a GPU."""
import math

import torch
import torch.nn.functional as F

import loss_cases as lc

# (Bg, E, Nq, n_ids): one row, the plain loss is 0; 40 % of the entries masked; Bg and E no multiples of 64; one column past a 16-byte
# piece and a chunk boundary; the recipe shape; many chunks
SHAPE_SWEEP = [(1, 4, 3, 2), (5, 8, 3, 3), (130, 100, 1000, 40), (65, 768, 4097, 50), (64, 512, 4096, 6000), (256, 512, 16384, 6000)]
MASK_SHAPES = [(5, 8, 3, 3), (130, 100, 1000, 40), (65, 768, 4097, 50)]         # where dropping the id mask must move the loss by 1e-2
TEMPERATURES = (0.07, 0.01)
VARIANTS = {"default": {}, "margin": dict(margin=0.2), "dcl": dict(dcl=True), "a2b": dict(b2a=False), "b2a": dict(a2b=False)}


# The two tiny cases draw a handful of numbers, so their seeds are chosen for what the cases are there to show (properties of the INPUTS,
# re-asserted by tests/test_queue_loss_cpu.py: test_the_cases_make_the_bounds_bite): every anchor keeps an admitted entry, the queue
# moves the fp64 loss by >= 1e-3 at both temperatures, and at (5, 8, 3, 3) exactly 6 of the 15 entries are masked.  The larger shapes
# take the default seed.
SEEDS = {(1, 4, 3, 2): 17, (5, 8, 3, 3): 22}


def make_case(Bg, E, Nq, n_ids, seed=None, with_ids=True):
    """-> dict(A, B, ids, queue_A, queue_B, queue_ids): A unit rows, B = unit(A + 0.5 noise), queue rows unit randn, ids =
    randint(n_ids) on both sides"""
    seed = SEEDS.get((Bg, E, Nq, n_ids), Bg * 1000 + E + Nq) if seed is None else seed
    g = torch.Generator().manual_seed(seed)
    A = F.normalize(torch.randn(Bg, E, generator=g), dim=-1)
    Bm = F.normalize(A + 0.5 * torch.randn(Bg, E, generator=g), dim=-1)
    queue_A = F.normalize(torch.randn(Nq, E, generator=g), dim=-1)
    queue_B = F.normalize(torch.randn(Nq, E, generator=g), dim=-1)
    ids = torch.randint(0, n_ids, (Bg,), generator=g, dtype=torch.int64)
    queue_ids = torch.randint(0, n_ids, (Nq,), generator=g, dtype=torch.int64)
    return {"A": A, "B": Bm, "ids": ids if with_ids else None, "queue_A": queue_A, "queue_B": queue_B,
            "queue_ids": queue_ids if with_ids else None}


def admitted(ids, queue_ids, Bg, Nq):
    """[Bg, Nq] bool: the reference's mask rule (avssl/module/losses.py:207) over the queue's columns"""
    if ids is None:
        return torch.ones(Bg, Nq, dtype=torch.bool)
    return ids[:, None] != queue_ids[None, :]


def queue_loss_reference(A, Bm, ids, queue_A, queue_B, queue_ids, temperature=0.07, margin=0.0, dcl=False, a2b=True, b2a=True,
                         trainable=False, log_inv_temp=None, scale=1.0, dtype=torch.float64, device=None, mask_queue=True):
    """The expression of the module docstring on ``dtype`` copies (on ``device``, the CPU by default), with torch autograd.
    ``mask_queue`` False admits every entry (what a loss that lost the id mask over the queue would compute).
    -> dict(loss, dA, dB, [dT], x_A, x_B (-inf where not admitted; None for a side that is off), lse_row, lse_col, used_A, used_B)"""
    assert a2b or b2a
    dev = torch.device("cpu") if device is None else device
    Bg, Nq = A.shape[0], (queue_B if a2b else queue_A).shape[0]
    a = A.detach().to(dev, dtype).requires_grad_(True)
    b = Bm.detach().to(dev, dtype).requires_grad_(True)
    t = None
    if trainable:
        t0 = torch.tensor(math.log(1 / temperature), dtype=torch.float32) if log_inv_temp is None else log_inv_temp.detach().cpu().float()
        t = t0.to(dev, dtype).reshape(()).requires_grad_(True)
        it = t.exp()
    else:
        it = 1.0 / temperature
    eye = torch.eye(Bg, dtype=torch.bool, device=dev)
    neg = lc.neg_mask(Bg, ids, dcl).to(dev)
    adm = admitted(ids if mask_queue else None, queue_ids, Bg, Nq).to(dev)
    zero, ninf = torch.zeros((), dtype=dtype, device=dev), torch.full((), -math.inf, dtype=dtype, device=dev)
    logits = a @ b.t() * it
    if margin > 0.0:
        logits = logits - margin * eye.type(dtype)
    pos = logits[eye]
    e = torch.where(neg, logits.exp(), zero)
    row_sum, col_sum = e.sum(1), e.sum(0)
    x_A = x_B = None
    if a2b:
        x_A = a @ queue_B.detach().to(dev, dtype).t() * it
        row_sum = row_sum + torch.where(adm, x_A.exp(), zero).sum(1)
    if b2a:
        x_B = b @ queue_A.detach().to(dev, dtype).t() * it
        col_sum = col_sum + torch.where(adm, x_B.exp(), zero).sum(1)
    total = 0
    if a2b:
        total = total + (-pos + torch.log(row_sum)).mean()
    if b2a:
        total = total + (-pos + torch.log(col_sum)).mean()
    loss = total / 2 if (a2b and b2a) else total
    (scale * loss).backward()
    out = {"loss": loss.detach(), "dA": a.grad, "dB": b.grad}
    if trainable:
        out["dT"] = t.grad
    with torch.no_grad():
        used = adm.sum(1).to(torch.int32)
        out.update(x_A=torch.where(adm, x_A, ninf) if a2b else None, x_B=torch.where(adm, x_B, ninf) if b2a else None,
                   lse_row=torch.log(row_sum), lse_col=torch.log(col_sum), used_A=used if a2b else torch.zeros_like(used),
                   used_B=used if b2a else torch.zeros_like(used))
    return {k: v.cpu() if torch.is_tensor(v) else v for k, v in out.items()}       # evaluated on ``device``, compared on the host


def grad_err(x, ref):
    """max |x - ref| / max |ref|, lc.scale_rel_err's measure, with the scale floored at lc.ZERO_GRAD: at (1, 4, 3, 2) and T = 0.01 a
    one-sided loss has a gradient whose largest entry is below 1e-12 (the positive outweighs the three extras by many orders of
    magnitude), which lc.scale_rel_err takes for analytically zero and answers with inf - there the measure is the absolute error in
    units of 1e-12, finite, and held against the fp32 yardstick's own like every other"""
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    return float((x - ref).abs().max() / max(float(ref.abs().max()), lc.ZERO_GRAD))


def x_err(x, ref):
    """max |x - ref| over the admitted entries; inf unless the -inf pattern is the reference's exactly"""
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    fin = torch.isfinite(ref)
    if not bool((torch.isneginf(x) == ~fin).all()):
        return float("inf")
    return float((x[fin] - ref[fin]).abs().max()) if bool(fin.any()) else 0.0
