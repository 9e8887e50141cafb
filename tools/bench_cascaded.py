#!/usr/bin/env python3
"""A/B of the fixed-keyword cascaded recipe (config/speechCLIP/model_base/spchclp_c.yaml): one train step at B utterances of
``--seconds`` with the K keyword rows by the constant-query pooling (csrc/kwpool.hip) and by the full-sequence attention block
(MultiheadAttentionAndNorm.query_forward_full), in ONE process on the same model and batch, the two routes alternating in blocks of
``--steps`` timed steps (``--rounds`` blocks each) after warming both up; then the per-launch times of the new kernels at the
recipe's shapes (device events around ``--reps`` launches).  Prints one JSON line.

    python tools/bench_cascaded.py --batch 64 --seconds 10 --steps 10 --rounds 5
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def make(B, L, dev):
    from speechclip_plus_amd import KWClip_GeneralTransformer, cascaded_base_config, random_hubert_state_dict
    from speechclip_plus_amd.speech_encoder import ARCHS
    from speechclip_plus_amd.train import ContrastiveTrainer
    torch.manual_seed(7122)
    sd = random_hubert_state_dict(ARCHS["hubert"], seed=7122)
    cfg = cascaded_base_config()
    cfg.audio_encoder.max_audio_len = -1
    model = KWClip_GeneralTransformer(cfg, device=str(dev), hubert_state_dict=sd).train()
    trainer = ContrastiveTrainer(model)
    g = torch.Generator(device="cpu").manual_seed(7122)
    wav = torch.randn(B, L, generator=g).to(dev)
    wav._sc_ready = True
    img = torch.nn.functional.normalize(torch.randn(B, int(cfg.clip.embed_dim), generator=g), dim=-1).to(dev)
    batch = {"wav": wav, "wav_len": torch.full((B,), L, dtype=torch.long), "image": img, "id": (torch.arange(B) // 5).to(dev)}
    return model, trainer, batch


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def kernel_times(B, R, D, K, E, reps, dev):
    """per-launch milliseconds of the new entry points at the recipe's shapes (device events around ``reps`` launches)"""
    from speechclip_plus_amd import ops
    g = torch.Generator(device="cpu").manual_seed(1)
    X = torch.randn(B, R, D, generator=g).to(torch.bfloat16).to(dev)
    a = (torch.randn(K, D, generator=g) / D ** 0.5).to(dev)
    crow = torch.randn(K, D, generator=g).to(dev)
    c = (a @ crow.t()).contiguous()
    flen = torch.full((B,), R - 1, dtype=torch.int32, device=dev)
    dm = torch.randn(B, K, D, generator=g).to(dev)
    p, _ = ops.kw_pool_fwd(X, a, c, crow, flen, 1)
    x = torch.randn(B, K, E, generator=g).to(dev)
    gam, bet = torch.ones(K * E, device=dev), torch.zeros(K * E, device=dev)
    rm, rv = torch.zeros(K * E, device=dev), torch.ones(K * E, device=dev)
    y, sm, sr = ops.bn_eachkw_fwd(x, gam, bet, rm, rv, True, 0.1, 1e-5)
    calls = {"kw_pool_fwd (scores + pool)": lambda: ops.kw_pool_fwd(X, a, c, crow, flen, 1),
             "kw_pool_bwd fp32 dX (scores + grad + batch sum)": lambda: ops.kw_pool_bwd(X, a, crow, flen, 1, p, dm),
             "kw_pool_bwd bf16 dX": lambda: ops.kw_pool_bwd(X, a, crow, flen, 1, p, dm, dx_dtype=torch.bfloat16),
             "bn_eachkw_fwd (train)": lambda: ops.bn_eachkw_fwd(x, gam, bet, rm, rv, True, 0.1, 1e-5),
             "bn_eachkw_bwd": lambda: ops.bn_eachkw_bwd(x, y, gam, sm, sr)}
    out = {}
    for name, fn in calls.items():
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name] = round(e0.elapsed_time(e1) / reps, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, L = args.batch, int(round(args.seconds * 16000))
    model, trainer, batch = make(B, L, dev)
    att = model.cascaded_branch.self_att
    routes = ("pooled", "full")
    for r in routes:                                     # warm both routes: code objects, plans, workspaces
        att.query_path = r
        for _ in range(args.warmup):
            trainer.step(batch)
    times = {r: [] for r in routes}
    for i in range(args.rounds):
        for r in (routes if i % 2 == 0 else routes[::-1]):        # alternate, and alternate who goes first
            att.query_path = r
            trainer.step(batch)                          # (the first step after a switch absorbs the other route's cached state)
            times[r].append(timed(lambda: trainer.step(batch), args.steps))
    att.query_path = None
    pl = next(reversed(model.audio_encoder._plans.values()))
    rec = {"workload": f"cascaded base, train step, B={B} x {args.seconds:g} s", "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around steps ending in a device synchronise; kernels: device events",
           "steps_per_block": args.steps, "blocks": args.rounds,
           "pooled_ms": [round(t, 3) for t in times["pooled"]], "full_ms": [round(t, 3) for t in times["full"]],
           "pooled_ms_median": round(statistics.median(times["pooled"]), 3), "full_ms_median": round(statistics.median(times["full"]), 3),
           "rows_per_utterance": int(pl.Rout),
           "kernels_ms": kernel_times(B, int(pl.Rout), 768, 8, 512, args.reps, dev)}
    rec["pooled_not_slower"] = rec["pooled_ms_median"] <= rec["full_ms_median"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
