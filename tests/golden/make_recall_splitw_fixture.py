#!/usr/bin/env python3
"""Recall fixture of the split-weight evaluation mode (round 9): the 5000 utterances, weights, batching protocol and the two natural-margin
galleries of make_recall_natural_fixture.py (A = recall_eval_natural.npz, B = recall_eval_natural_b.npz), embedded by the oracle's
emulation of `audio_encoder.eval_weights: split` - every bf16 storage site rounded (oracle.SitedStore, the weighted sum's output
included) and the GEMM weights as W_hi + W_lo (tools/recall_eval.split_emulation_weights; pos_conv bf16).

Stored (tests/golden/recall_eval_splitemu.npz), per gallery g in (a, b): rank_ai_splitemu_g / rank_ia_splitemu_g (the emulation's ranks,
both directions; the fp32 ranks are in the gallery's own fixture); and once: mean_unit_fp32 (the mean of the fp32 oracle's unit
embeddings - all that is needed to measure an implementation's common shift, |mean(a) - mean(a_fp32)|), shift_splitemu (the split
emulation's common-shift norm) and shift_bf16emu_weights (for comparison: the same with bf16 weights = config "all").

    python tests/golden/make_recall_splitw_fixture.py [--threads 8] [--cache DIR]        (~10 min per embedding set on 8 cores; cached)
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..", "tools")))
from recall_eval import eval_set, rank_stats, recalls  # noqa: E402
from storage_ablation import SITES, embeddings  # noqa: E402

SPLIT_CONFIG = "+".join(SITES) + "+wsum+w_split"         # every activation site + the split weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--cache", default="/tmp/ablation")
    ap.add_argument("--out", default=os.path.join(HERE, "recall_eval_splitemu.npz"))
    args = ap.parse_args()
    os.makedirs(args.cache, exist_ok=True)
    torch.set_num_threads(args.threads)
    wavs, ids = eval_set(1000)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True)
    a32 = unit(embeddings("fp32", wavs, args.cache))
    asp = unit(embeddings(SPLIT_CONFIG, wavs, args.cache))
    out = {"config": np.asarray(SPLIT_CONFIG), "mean_unit_fp32": a32.mean(0).numpy().astype(np.float32),
           "shift_splitemu": np.float64((asp - a32).mean(0).norm())}
    path_all = os.path.join(args.cache, "all.npy")
    if os.path.exists(path_all):
        out["shift_bf16emu_weights"] = np.float64((unit(torch.from_numpy(np.load(path_all))) - a32).mean(0).norm())
    for g, name in (("a", "recall_eval_natural.npz"), ("b", "recall_eval_natural_b.npz")):
        fx = np.load(os.path.join(HERE, name))
        img = torch.from_numpy(fx["image"])
        st32, st = rank_stats(a32, img, ids), rank_stats(asp, img, ids)
        assert torch.equal(st32["rank_ai"].long(), torch.from_numpy(fx["rank_ai_fp32"]).long()), "the fp32 oracle no longer gives the gallery fixture's ranks"
        out[f"rank_ai_splitemu_{g}"] = st["rank_ai"].numpy().astype(np.int16)
        out[f"rank_ia_splitemu_{g}"] = st["rank_ia"].numpy().astype(np.int16)
        flips = lambda x, y: [int(((x < k) != (y < k)).sum()) for k in (1, 5, 10)]
        print(f"gallery {g.upper()}: fp32 {recalls(st32['rank_ai'])} / {recalls(st32['rank_ia'])}  split emulation {recalls(st['rank_ai'])} / "
              f"{recalls(st['rank_ia'])}  flips vs fp32 {flips(st32['rank_ai'], st['rank_ai'])} / {flips(st32['rank_ia'], st['rank_ia'])}")
    print({k: float(v) for k, v in out.items() if k.startswith("shift")})
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
