#!/usr/bin/env python3
"""SigmoidContrastiveLoss (losses.SigmoidContrastiveLoss on csrc/sigmoid_loss.hip) against the same loss as a torch autograd expression
on the same GPU, on tools/bench_search_sharded.py's protocol: ONE process, the two routes alternating in blocks after a warm-up at every
switch (and alternating who goes first), device events around every block, ms per call.  One JSON line per shape with the median and
every block of each route, the spread of the blocks, and how far the two routes' results are apart.

  (k) the module: forward + backward (exp of logit_scale, sc_sigmoid_loss_fwd, sc_sigmoid_loss_grad, two exact-fp32 feature products,
      the two sums of the rows' d t / d b terms)
  (t) the same loss as a torch autograd expression in fp32: matmul, exp(logit_scale) x + bias, the masks built from the ids,
      softplus, weighted sum / B - forward + backward

Shapes (B, E), ids = arange // 5, same_id "ignore", both scalars learnable: (64, 512) the per-GPU batch, (512, 768) the 8-GPU gathered
batch.  The kernel route replaces (t) and has no other claim to exist: k_over_t <= 1 at both shapes is the requirement.  A second line
per shape times the two new launches alone (ops.sigmoid_loss_fwd / ops.sigmoid_loss_grad on resident operands, output allocations
included).

    python tools/bench_sigmoid_loss.py --blocks 7
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from bench_search_sharded import alternate, report                     # noqa: E402

SHAPES = ((64, 512), (512, 768))


def torch_sigmoid_loss(A, Bm, ids, logit_scale, logit_bias):
    """the pairwise sigmoid loss with same-id pairs ignored, as the usual torch expression"""
    B = A.shape[0]
    x = logit_scale.exp() * (A @ Bm.t()) + logit_bias
    eye = torch.eye(B, dtype=torch.bool, device=A.device)
    z = torch.where(eye, 1.0, -1.0)
    w = ((ids[:, None] != ids[None, :]) | eye).float()
    return (w * torch.nn.functional.softplus(-z * x)).sum() / B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="whole calls per timed block")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5, help="untimed calls after every switch of routes")
    ap.add_argument("--shapes", type=str, default="0,1")
    args = ap.parse_args()
    from speechclip_plus_amd import ops
    from speechclip_plus_amd.losses import SigmoidContrastiveLoss
    dev = torch.device("cuda:0")
    base = {"device": torch.cuda.get_device_name(0), "clock": "device events around blocks of calls, ms per call", "blocks": args.blocks,
            "reps_per_block": args.reps, "warmup_after_every_switch": args.warmup}
    norm = torch.nn.functional.normalize
    for B, E in (SHAPES[int(s)] for s in args.shapes.split(",")):
        g = torch.Generator(device=dev).manual_seed(B + E)
        A0 = norm(torch.randn(B, E, device=dev, generator=g), dim=-1)
        B0 = norm(torch.randn(B, E, device=dev, generator=g) + 0.5 * A0, dim=-1)
        ids = torch.arange(B, device=dev) // 5
        crit = SigmoidContrastiveLoss().to(dev)
        ls = torch.nn.Parameter(crit.logit_scale.detach().clone())
        lb = torch.nn.Parameter(crit.logit_bias.detach().clone())
        a, b = A0.clone().requires_grad_(True), B0.clone().requires_grad_(True)
        out = {}

        def kernel_route():
            a.grad = b.grad = crit.logit_scale.grad = crit.logit_bias.grad = None
            out["k"] = crit(a, b, ids)
            out["k"].backward()

        def torch_route():
            a.grad = b.grad = ls.grad = lb.grad = None
            out["t"] = torch_sigmoid_loss(a, b, ids, ls, lb)
            out["t"].backward()
        kernel_route()
        ka, kb, ks, kbias = a.grad.clone(), b.grad.clone(), crit.logit_scale.grad.clone(), crit.logit_bias.grad.clone()
        torch_route()
        t = float(ls.detach().exp())
        agree = {"loss_k": float(out["k"].detach()), "loss_k_minus_t": float((out["k"] - out["t"]).detach()),
                 "dA_k_vs_t": float((ka - a.grad).abs().max() / a.grad.abs().max()),
                 "dB_k_vs_t": float((kb - b.grad).abs().max() / b.grad.abs().max()),
                 "largest_gradient_entry": float(max(a.grad.abs().max(), b.grad.abs().max())),
                 "dt_k": float(ks) / t, "dt_k_vs_t": float((ks - ls.grad).abs() / ls.grad.abs()),
                 "db_k": float(kbias), "db_k_vs_t": float((kbias - lb.grad).abs() / lb.grad.abs()),
                 "counts": crit.last_counts.tolist()}
        times = alternate((("k", kernel_route), ("t", torch_route)), args.reps, args.blocks, args.warmup)
        shape = {"B": B, "E": E, "same_id": "ignore", "ids": "arange // 5", "learnable": True}
        print(json.dumps({"bench": "sigmoid_loss", **shape, **base, **agree, **report(times, "k", "t")}), flush=True)
        # the two new launches alone, on resident operands
        tt, bb, gs = torch.full((1,), t, device=dev), torch.full((1,), -10.0, device=dev), torch.ones(1, device=dev)
        _, s, _ = ops.sigmoid_loss_fwd(A0, B0, ids, tt, bb)

        def fwd_side():
            ops.sigmoid_loss_fwd(A0, B0, ids, tt, bb)

        def grad_side():
            ops.sigmoid_loss_grad(s, ids, gs, tt, bb)
        times = alternate((("fwd", fwd_side), ("grad", grad_side)), args.reps, args.blocks, args.warmup)
        print(json.dumps({"bench": "sigmoid_loss_launches", **shape, **base, **report(times, "fwd", "grad")}), flush=True)


if __name__ == "__main__":
    main()
