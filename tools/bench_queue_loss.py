#!/usr/bin/env python3
"""The contrastive loss with a cross-batch queue (MaskedContrastiveLoss(..., queue_A=, queue_B=, queue_ids=), csrc/infonce_queue.hip)
on tools/bench_neg_loss.py's protocol: ONE process, two sides alternating in blocks after a warm-up at every switch (and alternating
who goes first), device events around every block, ms per call, the median of five blocks of three.  One JSON line per measurement
with the median and every block of each side and the spread of the blocks.

  loss     (q) the module's forward + backward with a queue
           (t) the same loss as a torch autograd expression on the device: two score products, masked logsumexp over [logits | x]
  parts    (g) the two pairs of products on the exact-fp32 GEMM alone (the scores of both sides; w_A . queue_B and w_B . queue_A) against
           (r) the two row launches alone (ops.infonce_queue_fwd / ops.infonce_queue_grad on resident scores), and the row launches'
           GB/s over the bytes they move - the scores of both sides read and written once per launch, the queue's ids once - as a
           fraction of 6.29 TB/s (MI355X_MICROARCH: float4 copy).  ``gemm_share`` = g / q of the "loss" record's module side.
  step     (q) the loss with the queue against (p) the plain loss, forward + backward, at the recipe shape

Shapes (Bg, E, Nq): (64, 512, 4096), (64, 768, 16384), (512, 512, 16384), (512, 768, 65536).  ids = arange // 5, queue ids = randint over
the same range (so a few entries per anchor are masked).  (q) / (t) is a cost to write down, not a gate.

    python tools/bench_queue_loss.py --blocks 5
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from bench_search_sharded import alternate, report                     # noqa: E402

SHAPES = ((64, 512, 4096), (64, 768, 16384), (512, 512, 16384), (512, 768, 65536))
RECIPE = (64, 512, 4096)               # the per-GPU batch of the shipped recipes, 64 steps of it in the ring
GUIDE_TBS = 6.29


def unit_randn(n, E, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, E, device=dev, generator=g), dim=-1)


def operands(Bg, E, Nq, dev):
    A, Bm, qA, qB = unit_randn(Bg, E, dev, 1), unit_randn(Bg, E, dev, 2), unit_randn(Nq, E, dev, 3), unit_randn(Nq, E, dev, 4)
    ids = torch.arange(Bg, device=dev) // 5
    g = torch.Generator(device=dev).manual_seed(5)
    qids = torch.randint(0, max(1, (Bg + 4) // 5), (Nq,), device=dev, generator=g)
    return A, Bm, ids, qA, qB, qids


def torch_loss(a, b, ids, qA, qB, qids, it):
    """the reference expression on the device (tests/queue_loss_cases.py), default options"""
    logits = a @ b.t() * it
    eye = torch.eye(a.shape[0], dtype=torch.bool, device=a.device)
    neg = (ids[:, None] != ids[None, :]) | eye
    adm = ids[:, None] != qids[None, :]
    minf = torch.full((), float("-inf"), device=a.device)
    xA, xB = a @ qB.t() * it, b @ qA.t() * it
    row = torch.logsumexp(torch.cat([torch.where(neg, logits, minf), torch.where(adm, xA, minf)], 1), 1)
    col = torch.logsumexp(torch.cat([torch.where(neg, logits, minf).t(), torch.where(adm, xB, minf)], 1), 1)
    pos = logits[eye]
    return ((row - pos).mean() + (col - pos).mean()) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="whole calls per timed block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls after every switch of sides")
    ap.add_argument("--shapes", type=str, default="0,1,2,3")
    ap.add_argument("--what", type=str, default="loss,parts,step")
    args = ap.parse_args()
    from speechclip_plus_amd import ops
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    dev = torch.device("cuda:0")
    base = {"device": torch.cuda.get_device_name(0), "clock": "device events around blocks of calls, ms per call", "blocks": args.blocks,
            "reps_per_block": args.reps, "warmup_after_every_switch": args.warmup}
    what = args.what.split(",")
    crit = MaskedContrastiveLoss().to(dev)
    it = torch.full((1,), 1 / 0.07, device=dev)
    for Bg, E, Nq in (SHAPES[int(s)] for s in args.shapes.split(",")):
        A, Bm, ids, qA, qB, qids = operands(Bg, E, Nq, dev)
        a, b = A.clone().requires_grad_(True), Bm.clone().requires_grad_(True)
        shape = {"Bg": Bg, "E": E, "Nq": Nq}
        module_ms = None
        if "loss" in what:
            def module_side():
                a.grad = b.grad = None
                crit(a, b, ids, queue_A=qA, queue_B=qB, queue_ids=qids).backward()

            def torch_side():
                a.grad = b.grad = None
                torch_loss(a, b, ids, qA, qB, qids, it).backward()
            module_side()
            ga = a.grad.clone()
            torch_side()
            agree = float((ga - a.grad).abs().max() / a.grad.abs().max())
            times = alternate((("q", module_side), ("t", torch_side)), args.reps, args.blocks, args.warmup)
            rec = report(times, "q", "t")
            module_ms = rec["q_ms_median"]
            print(json.dumps({"bench": "queue_loss", **shape, **base, "dA_q_vs_t": agree, **rec}), flush=True)
        if "parts" in what:
            loss, logits, lr, lcol = ops.infonce_fwd(A, Bm, ids, it)
            x_A, x_B = ops.queue_scores(A, qB), ops.queue_scores(Bm, qA)
            _, lre, lce, _, _ = ops.infonce_queue_fwd(x_A, x_B, ids, qids, it, loss, lr, lcol, logits, E)
            dot, gs = torch.zeros(Bg, device=dev), torch.ones(1, device=dev)

            def gemm_side():
                ops.queue_scores(A, qB)
                ops.queue_scores(Bm, qA)
                ops.sgemm_mfma(x_A, qB, b_kmajor=True)
                ops.sgemm_mfma(x_B, qA, b_kmajor=True)

            def rows_side():                                 # the values do not change the work: the scores are rewritten in place
                ops.infonce_queue_fwd(x_A, x_B, ids, qids, it, loss, lr, lcol, logits, E)
                ops.infonce_queue_grad(x_A, x_B, lre, lce, gs, it, True, True, dot)
            times = alternate((("g", gemm_side), ("r", rows_side)), 20, args.blocks, args.warmup)
            rec = report(times, "g", "r")
            moved = 2 * (2 * 2 * Bg * Nq * 4) + Nq * 8       # two launches x two sides x (read + write), the ids once
            rec["r_GBps"] = round(moved / (rec["r_ms_median"] * 1e-3) / 1e9, 1)
            rec["r_of_guide"] = round(rec["r_GBps"] / (GUIDE_TBS * 1e3), 3)
            if module_ms:
                rec["gemm_share"] = round(rec["g_ms_median"] / module_ms, 3)
            print(json.dumps({"bench": "queue_loss_parts", **shape, **base, "reps_per_block": 20, "bytes_moved": moved,
                              "guide_TBps": GUIDE_TBS, **rec}), flush=True)
    if "step" in what:
        Bg, E, Nq = RECIPE
        A, Bm, ids, qA, qB, qids = operands(Bg, E, Nq, dev)
        a, b = A.clone().requires_grad_(True), Bm.clone().requires_grad_(True)

        def queue_side():
            a.grad = b.grad = None
            crit(a, b, ids, queue_A=qA, queue_B=qB, queue_ids=qids).backward()

        def plain_side():
            a.grad = b.grad = None
            crit(a, b, ids).backward()
        times = alternate((("q", queue_side), ("p", plain_side)), args.reps, args.blocks, args.warmup)
        print(json.dumps({"bench": "queue_loss_step", "Bg": Bg, "E": E, "Nq": Nq, **base, **report(times, "q", "p")}), flush=True)


if __name__ == "__main__":
    main()
