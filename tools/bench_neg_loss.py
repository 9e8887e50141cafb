#!/usr/bin/env python3
"""The contrastive loss with a negative bank (MaskedContrastiveLoss.forward(..., bank=, bank_ids=, neg_idx=), csrc/infonce_neg.hip) on
tools/bench_search_sharded.py's protocol: ONE process, two sides alternating in blocks after a warm-up at every switch (and
alternating who goes first), device events around every block, ms per call, the median of five blocks of three.  One JSON line per
measurement with the median and every block of each side and the spread of the blocks.

  loss     (n) the module's forward + backward with a bank
           (t) the same loss as a torch autograd expression on the device: bank[neg_idx], einsum, masked logsumexp
  gather   the two new launches alone (ops.infonce_neg_fwd / ops.infonce_neg_grad on resident operands) against the bytes they
           gather, Bg * M * E * 4 each way: GB/s and the fraction of 5.5 TB/s (MI355X_MICROARCH "Indexed rows", whole rows into registers)
  step     (m) hard_negatives + the loss with the bank, forward + backward, against (p) the plain loss, at the recipe shape

Shapes (Bg, E, N, M): (64, 512, 6000, 32), (64, 768, 6000, 256), (512, 768, 120000, 256), (512, 512, 120000, 1024).  ids = arange // 5,
bank ids all different from the batch's except the first Bg rows (the batch's own images, as a bank of the training set holds them).
Lists are random rows (sorted scores do not change the work), a tenth of the slots -1.  (n) / (t) is a cost to write down, not a gate.

    python tools/bench_neg_loss.py --blocks 5
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from bench_search_sharded import alternate, report                     # noqa: E402

SHAPES = ((64, 512, 6000, 32), (64, 768, 6000, 256), (512, 768, 120000, 256), (512, 512, 120000, 1024))
RECIPE = (64, 512, 6000, 256)          # the per-GPU batch of the shipped recipes, Flickr8k's images, INTEGRATION.md's 256 negatives
GUIDE_TBS = 5.5


def unit_randn(n, E, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, E, device=dev, generator=g), dim=-1)


def operands(Bg, E, N, M, dev):
    A, Bm, bank = unit_randn(Bg, E, dev, 1), unit_randn(Bg, E, dev, 2), unit_randn(N, E, dev, 3)
    bank[:Bg] = Bm
    ids = torch.arange(Bg, device=dev) // 5
    bank_ids = Bg + torch.arange(N, device=dev)
    bank_ids[:Bg] = ids
    g = torch.Generator(device=dev).manual_seed(4)
    neg_idx = torch.randint(0, N, (Bg, M), device=dev, generator=g)
    neg_idx[torch.rand(Bg, M, device=dev, generator=g) < 0.1] = -1
    return A, Bm, ids, bank, bank_ids, neg_idx


def torch_loss(a, b, ids, bank, bank_ids, neg_idx, it):
    """the reference expression on the device (tests/neg_loss_cases.py), default options"""
    N = bank.shape[0]
    logits = a @ b.t() * it
    eye = torch.eye(a.shape[0], dtype=torch.bool, device=a.device)
    neg = (ids[:, None] != ids[None, :]) | eye
    ok = (neg_idx >= 0) & (neg_idx < N)
    r = neg_idx.clamp(0, N - 1)
    ok = ok & ~torch.isin(bank_ids[r], ids)
    x = torch.einsum("ie,ime->im", a, bank[r]) * it
    minf = torch.full((), float("-inf"), device=a.device)
    row = torch.logsumexp(torch.cat([torch.where(neg, logits, minf), torch.where(ok, x, minf)], 1), 1)
    col = torch.logsumexp(torch.where(neg, logits, minf), 0)
    pos = logits[eye]
    return ((row - pos).mean() + (col - pos).mean()) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="whole calls per timed block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls after every switch of sides")
    ap.add_argument("--shapes", type=str, default="0,1,2,3")
    ap.add_argument("--what", type=str, default="loss,gather,step")
    args = ap.parse_args()
    from speechclip_plus_amd import GalleryIndex, hard_negatives, ops
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    dev = torch.device("cuda:0")
    base = {"device": torch.cuda.get_device_name(0), "clock": "device events around blocks of calls, ms per call", "blocks": args.blocks,
            "reps_per_block": args.reps, "warmup_after_every_switch": args.warmup}
    what = args.what.split(",")
    crit = MaskedContrastiveLoss().to(dev)
    it = torch.full((1,), 1 / 0.07, device=dev)
    for Bg, E, N, M in (SHAPES[int(s)] for s in args.shapes.split(",")):
        A, Bm, ids, bank, bank_ids, neg_idx = operands(Bg, E, N, M, dev)
        a, b = A.clone().requires_grad_(True), Bm.clone().requires_grad_(True)
        shape = {"Bg": Bg, "E": E, "N": N, "M": M}
        if "loss" in what:
            def module_side():
                a.grad = b.grad = None
                crit(a, b, ids, bank=bank, bank_ids=bank_ids, neg_idx=neg_idx).backward()

            def torch_side():
                a.grad = b.grad = None
                torch_loss(a, b, ids, bank, bank_ids, neg_idx, it).backward()
            module_side()
            ga = a.grad.clone()
            torch_side()
            agree = float((ga - a.grad).abs().max() / a.grad.abs().max())
            times = alternate((("n", module_side), ("t", torch_side)), args.reps, args.blocks, args.warmup)
            print(json.dumps({"bench": "neg_loss", **shape, **base, "dA_n_vs_t": agree, **report(times, "n", "t")}), flush=True)
        if "gather" in what:
            _, logits, lr, lcol = ops.infonce_fwd(A, Bm, ids, it)
            _, lse_ext, x, used = ops.infonce_neg_fwd(A, bank, neg_idx, ids, bank_ids, it, lr, lcol, logits)
            dA, dot, gs = torch.zeros_like(A), torch.zeros(Bg, device=dev), torch.ones(1, device=dev)

            def fwd_side():
                ops.infonce_neg_fwd(A, bank, neg_idx, ids, bank_ids, it, lr, lcol, logits)

            def grad_side():
                ops.infonce_neg_grad(A, bank, neg_idx, x, lse_ext, gs, it, True, True, dA, dot)
            times = alternate((("fwd", fwd_side), ("grad", grad_side)), 20, args.blocks, args.warmup)
            rec = report(times, "fwd", "grad")
            gathered = float(used.sum()) * E * 4
            for side in ("fwd", "grad"):
                rec[side + "_GBps"] = round(gathered / (rec[side + "_ms_median"] * 1e-3) / 1e9, 1)
                rec[side + "_of_guide"] = round(rec[side + "_GBps"] / (GUIDE_TBS * 1e3), 3)
            print(json.dumps({"bench": "neg_loss_gather", **shape, **base, "reps_per_block": 20, "bytes_gathered": gathered,
                              "bytes_nominal": Bg * M * E * 4, "guide_TBps": GUIDE_TBS, **rec}), flush=True)
    if "step" in what:
        Bg, E, N, M = RECIPE
        A, Bm, ids, bank, bank_ids, _ = operands(Bg, E, N, M, dev)
        a, b = A.clone().requires_grad_(True), Bm.clone().requires_grad_(True)
        index = GalleryIndex(bank, ids=bank_ids)

        def mined_side():
            a.grad = b.grad = None
            lists = hard_negatives(a.detach(), index, ids, None, M)[1]
            crit(a, b, ids, bank=bank, bank_ids=bank_ids, neg_idx=lists).backward()

        def plain_side():
            a.grad = b.grad = None
            crit(a, b, ids).backward()
        times = alternate((("m", mined_side), ("p", plain_side)), args.reps, args.blocks, args.warmup)
        print(json.dumps({"bench": "neg_loss_step", "Bg": Bg, "E": E, "N": N, "M": M, **base, **report(times, "m", "p")}), flush=True)


if __name__ == "__main__":
    main()
