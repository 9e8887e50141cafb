#!/usr/bin/env python3
"""Eval-mode forward of the frozen encoder (through the weighted sum: model.forward_audio) with eval_weights = "bf16" and "split", same process, alternating rounds
(docs/rounds/r09_split_weights.md): B = 64 x 10 s and the ragged batch of bench.py's length mix.

    python tools/bench_split_eval.py [--rounds 5] [--iters 10] [--out FILE]

Prints one JSON line: per batch and mode the median / min / max over the rounds of the mean forward time in ms."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from speechclip_plus_amd import HubertArch, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    sd = random_hubert_state_dict(HubertArch(), seed=7122)
    models = {}
    for mode in ("bf16", "split"):
        cfg = base_parallel_config()
        cfg.audio_encoder.max_audio_len = -1
        cfg.audio_encoder.eval_weights = mode
        models[mode] = KWClip_GeneralTransformer(cfg, device="cuda:0", hubert_state_dict=sd).eval()
    g = torch.Generator().manual_seed(0)
    B, L = 64, 160000
    ragged = [int(v) for v in torch.randint(32000, L + 1, (B,), generator=g)]
    ragged[0] = L
    batches = {"64x10s": [L] * B, "ragged": ragged}
    wav = torch.randn(B, L, generator=g).cuda()
    report = {}
    for tag, lens in batches.items():
        times = {m: [] for m in models}

        def fwd(model):
            with torch.no_grad():
                return model.forward_audio(wav, lens)

        for m in models.values():            # warm-up: plans, LDS attributes
            fwd(m)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for mode, m in models.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fwd(m)
                e1.record()
                torch.cuda.synchronize()
                times[mode].append(e0.elapsed_time(e1) / args.iters)
        report[tag] = {mode: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
                       for mode, t in times.items()}
        report[tag]["split_over_bf16"] = round(report[tag]["split"]["median_ms"] / report[tag]["bf16"]["median_ms"], 4)
    line = json.dumps({"bench": "split_eval", "rounds": args.rounds, "iters": args.iters, **report})
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
