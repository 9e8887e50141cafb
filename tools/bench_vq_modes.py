#!/usr/bin/env python3
"""The quantiser's soft modes (the mode kernels of csrc/vq.hip + the split-bf16 soft product) against the torch expression on the same GPU, on
tools/bench_supcon.py's protocol: ONE process, the two routes alternating in blocks after a warm-up at every switch (and alternating
who goes first), device events around every block, ms per call.  One JSON line per (shape, mode) with the median and every block of
each route, the spread of the blocks, and how far the two routes' results are apart.

  (k) the kernel route from the masked scores x [Nk, V] on: row statistics of x + g (sc_vq_noisy_rowstats), s as bf16 hi + lo
      (sc_vq_soft_split_bf16), keywords = s . table as one bf16 GEMM over [hi | hi | lo] x [hi | lo | hi] cut into fp32 partials +
      sc_colsum_f32; backward: t = g_out . table^T (bf16 GEMM), dx = s (t - <s, t>) / tau in bf16 (sc_vq_soft_bwd2) - what
      vector_quantizers._KeywordVQFn issues in a soft mode between the cosine scores and the product with the normalised table
  (t) fp32 torch on the same scores and the same materialised noise (ops.vq_gumbel): softmax((x + g) / tau) @ table, forward plus
      autograd backward to x

Shapes (Nk, V, Et): (512, 8112, 512), (1600, 8112, 512), (1600, 19787, 768).  Modes: soft (g = 0) and Gumbel-soft.

    python tools/bench_vq_modes.py --blocks 7
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from bench_search_sharded import alternate, report                     # noqa: E402

SHAPES = ((512, 8112, 512), (1600, 8112, 512), (1600, 19787, 768))
TAU, SEED = 0.1, 20261


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="whole calls per timed block")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls after every switch of routes")
    ap.add_argument("--shapes", type=str, default="0,1,2")
    args = ap.parse_args()
    from speechclip_plus_amd import ops
    from speechclip_plus_amd.vector_quantizers import SPECIAL_TOKENS, VocabTables
    dev = torch.device("cuda:0")
    base = {"device": torch.cuda.get_device_name(0), "clock": "device events around blocks of calls, ms per call", "blocks": args.blocks,
            "reps_per_block": args.reps, "warmup_after_every_switch": args.warmup, "tau": TAU}
    for Nk, V, Et in (SHAPES[int(s)] for s in args.shapes.split(",")):
        g_ = torch.Generator(device=dev).manual_seed(Nk + V)
        table = torch.randn(V, Et, device=dev, generator=g_) * 0.02
        tb = VocabTables(table)
        W = tb.soft_table()
        x = torch.randn(Nk, V, device=dev, generator=g_).clamp_(-3, 3) / 3.0          # cosine-like scores in [-1, 1]
        ops.vq_rowstats(x, V, TAU, SPECIAL_TOKENS)                                    # writes the -inf mask, as the module does
        gout = torch.randn(Nk, Et, device=dev, generator=g_)
        Nkp = -(-Nk // 128) * 128
        gb = torch.zeros(Nkp, tb.Etp, device=dev, dtype=torch.bfloat16)
        tbuf = torch.empty(Nkp, tb.Vp, device=dev, dtype=torch.float32)
        for noise in (False, True):
            noise_g = ops.vq_gumbel(Nk, V, SEED, dev) if noise else None
            xt = x.clone().requires_grad_(True)
            out = {}

            def kernel_route():
                _, stats = ops.vq_noisy_rowstats(x, V, TAU, SEED, noise)
                out["k"] = ops.vq_soft_product(ops.vq_soft_split(x, stats, V, TAU, tb.Vp, SEED, noise), W, Et)[:Nk]
                gb[:Nk, :Et] = gout
                ops.gemm_raw(gb, tb.Etp, tb.table_bf16, tb.Etp, tbuf, tb.Vp, Nkp, tb.Vp, tb.Etp, out_f32=True)
                out["dk"], _ = ops.vq_soft_bwd2(x, stats, tbuf[:Nk], V, TAU, out_bf16=True, Vpad=tb.Vp, seed=SEED, noise=noise)

            def torch_route():
                xt.grad = None
                y = xt + noise_g if noise else xt
                out["t"] = torch.softmax(y / TAU, dim=-1) @ table
                out["t"].backward(gout)
            kernel_route()
            torch_route()
            agree = {"keywords_k_vs_t": float((out["k"] - out["t"].detach()).abs().max() / out["t"].detach().abs().max()),
                     "dx_k_vs_t": float((out["dk"][:, :V].float() - xt.grad).abs().max() / xt.grad.abs().max())}
            times = alternate((("k", kernel_route), ("t", torch_route)), args.reps, args.blocks, args.warmup)
            shape = {"Nk": Nk, "V": V, "Et": Et, "mode": "gumbel_soft" if noise else "soft", "s_split_MB": round(Nkp * 3 * tb.Vp * 2 / 1e6, 1)}
            print(json.dumps({"bench": "vq_modes", **shape, **base, **agree, **report(times, "k", "t")}), flush=True)

            # where the kernel route's time goes: forward alone against backward alone
            def fwd_side():
                _, stats = ops.vq_noisy_rowstats(x, V, TAU, SEED, noise)
                out["stats"] = stats
                ops.vq_soft_product(ops.vq_soft_split(x, stats, V, TAU, tb.Vp, SEED, noise), W, Et)

            def bwd_side():
                gb[:Nk, :Et] = gout
                ops.gemm_raw(gb, tb.Etp, tb.table_bf16, tb.Etp, tbuf, tb.Vp, Nkp, tb.Vp, tb.Etp, out_f32=True)
                ops.vq_soft_bwd2(x, out["stats"], tbuf[:Nk], V, TAU, out_bf16=True, Vpad=tb.Vp, seed=SEED, noise=noise)
            fwd_side()
            times = alternate((("fwd", fwd_side), ("bwd", bwd_side)), args.reps, args.blocks, args.warmup)
            print(json.dumps({"bench": "vq_modes_sides", **shape, **base, **report(times, "fwd", "bwd")}), flush=True)


if __name__ == "__main__":
    main()
