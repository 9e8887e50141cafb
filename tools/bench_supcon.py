#!/usr/bin/env python3
"""SupConLoss (losses.SupConLoss on csrc/supcon.hip) against the torch expression of the reference's formula on the same GPU, on
tools/bench_search_sharded.py's protocol: ONE process, the two routes alternating in blocks after a warm-up at every switch (and
alternating who goes first), device events around every block, ms per call.  One JSON line per shape with the median and every block
of each route, the spread of the blocks, and how far the two routes' results are apart.

  (k) the module: forward + backward (sc_supcon_fwd, sc_supcon_grad, two exact-fp32 feature products)
  (t) the same loss as a torch autograd expression in fp32: cat(unbind), matmul / T, row max, masks built from the labels, exp, log,
      masked mean - forward + backward

Shapes (bsz, V, E), mode "all", labels = arange // 5: (64, 2, 512) the per-GPU batch, (512, 2, 768) the 8-GPU gathered batch.  The
kernel route replaces (t) and has no other claim to exist: k_over_t <= 1 at both shapes is the requirement.  A second line per shape
times the two new launches alone (ops.supcon_fwd / ops.supcon_grad on resident operands, output allocations included).

    python tools/bench_supcon.py --blocks 7
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from bench_search_sharded import alternate, report                     # noqa: E402

SHAPES = ((64, 2, 512), (512, 2, 768))


def torch_supcon(features, labels, temperature, base_temperature):
    """Khosla et al.'s loss as the usual torch expression, mode "all": features [bsz, V, E], temperature a [1] parameter"""
    bsz, V = features.shape[:2]
    N = bsz * V
    C = features.transpose(0, 1).reshape(N, -1)                                   # row r = features[r % bsz, r // bsz]
    l = C @ C.t() / temperature
    l = l - l.max(1, keepdim=True).values.detach()                                # the reference subtracts the row maximum before exp
    keep = (~torch.eye(N, dtype=torch.bool, device=features.device)).float()
    w = (labels[:, None] == labels[None, :]).float().repeat(V, V) * keep
    lse = torch.log((l.exp() * keep).sum(1, keepdim=True))
    return -(1 / base_temperature) * ((w * (l - lse)).sum(1) / w.sum(1)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50, help="whole calls per timed block")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5, help="untimed calls after every switch of routes")
    ap.add_argument("--shapes", type=str, default="0,1")
    args = ap.parse_args()
    from speechclip_plus_amd import ops
    from speechclip_plus_amd.losses import SupConLoss
    dev = torch.device("cuda:0")
    base = {"device": torch.cuda.get_device_name(0), "clock": "device events around blocks of calls, ms per call", "blocks": args.blocks,
            "reps_per_block": args.reps, "warmup_after_every_switch": args.warmup}
    for bsz, V, E in (SHAPES[int(s)] for s in args.shapes.split(",")):
        g = torch.Generator(device=dev).manual_seed(bsz + E)
        feats = torch.nn.functional.normalize(torch.randn(bsz, V, E, device=dev, generator=g) + 0.5 * torch.randn(bsz, 1, E, device=dev, generator=g), dim=-1)
        labels = torch.arange(bsz, device=dev) // 5
        crit = SupConLoss().to(dev)
        t_param = torch.nn.Parameter(torch.full((1,), 0.07, device=dev))
        f = feats.clone().requires_grad_(True)
        out = {}

        def kernel_route():
            f.grad = crit.temperature.grad = None
            out["k"] = crit(f, labels=labels)
            out["k"].backward()

        def torch_route():
            f.grad = t_param.grad = None
            out["t"] = torch_supcon(f, labels, t_param, 0.07)
            out["t"].backward()
        kernel_route()
        gk, tk = f.grad.clone(), crit.temperature.grad.clone()
        torch_route()
        agree = {"loss_k_minus_t": float((out["k"] - out["t"]).detach()),
                 "dfeatures_k_vs_t": float((gk - f.grad).abs().max() / f.grad.abs().max()),
                 "dT_k_vs_t": float((tk - t_param.grad).abs() / t_param.grad.abs())}
        times = alternate((("k", kernel_route), ("t", torch_route)), args.reps, args.blocks, args.warmup)
        shape = {"bsz": bsz, "V": V, "E": E, "mode": "all", "labels": "arange // 5"}
        print(json.dumps({"bench": "supcon", **shape, **base, **agree, **report(times, "k", "t")}), flush=True)
        # the two new launches alone, on resident operands
        N = bsz * V
        C = feats.transpose(0, 1).reshape(N, E).contiguous()
        it, gs = torch.full((1,), 1 / 0.07, device=dev), torch.ones(1, device=dev)
        _, logits, lse, _, poscnt = ops.supcon_fwd(C, N, bsz, labels, None, it, 0.07)

        def fwd_side():
            ops.supcon_fwd(C, N, bsz, labels, None, it, 0.07)

        def grad_side():
            ops.supcon_grad(logits, lse, poscnt, bsz, labels, None, gs, it, 0.07)
        times = alternate((("fwd", fwd_side), ("grad", grad_side)), args.reps, args.blocks, args.warmup)
        print(json.dumps({"bench": "supcon_launches", **shape, **base, **report(times, "fwd", "grad")}), flush=True)


if __name__ == "__main__":
    main()
