#!/usr/bin/env python3
"""Throughput of the frozen CLIP image tower (speechclip_plus_amd/clip_image.py) at B images per call, per tower: warm-up, then HIP
events around back-to-back calls covering >= --min-s seconds of work; algorithmic FLOP (ClipImageEncoder.flops) / time and the fraction
of the 2.5 PFLOP/s dense-bf16 peak.  For reference the same process times the fp32 torch restatement of openai's VisionTransformer
(tests/test_gpu_clip_image.py: openai_vit_fp32) under bf16 autocast.  One JSON line per tower.

    python3 tools/bench_image_tower.py [--batch 64] [--towers ViT-L/14,ViT-B/32] [--no-torch]
    python3 tools/bench_image_tower.py --profile [--out DIR]     re-runs itself (tower only) as a fresh child under
                                                                 rocprofv3 --kernel-trace --stats: per-kernel split in DIR
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK = 2.5e15


def timed(fn, min_s: float):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(3, int(min_s / max(time.perf_counter() - t0, 1e-6)) + 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--towers", default="ViT-L/14,ViT-B/32")
    ap.add_argument("--min-s", type=float, default=0.5)
    ap.add_argument("--no-torch", action="store_true", help="skip the bf16-autocast torch restatement")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="bench_image_tower_prof")
    a = ap.parse_args()
    if a.profile:
        os.makedirs(a.out, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.out, "-o", "tower", "--",
               sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--towers", a.towers, "--min-s", str(a.min_s), "--no-torch"]
        print(" ".join(cmd), flush=True)
        sys.exit(subprocess.call(cmd))
    import torch
    from speechclip_plus_amd.clip_image import ClipImageEncoder
    from test_gpu_clip_image import openai_vit_fp32
    dev = torch.device("cuda:0")
    for name in a.towers.split(","):
        m = ClipImageEncoder(name, seed=1).to(dev)
        pix = torch.randn(a.batch, 3, 224, 224, generator=torch.Generator().manual_seed(0)).to(dev)
        ms, n = timed(lambda: m(pix), a.min_s)
        fl = m.flops(a.batch)
        row = {"tower": name, "batch": a.batch, "ms": round(ms, 3), "calls": n, "tflop": round(fl / 1e12, 3),
               "tflops": round(fl / ms / 1e9, 1), "peak_fraction": round(fl / ms / 1e-3 / PEAK, 3)}
        if not a.no_torch:
            with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
                ms_t, _ = timed(lambda: openai_vit_fp32(m, pix), a.min_s)
            row.update({"torch_bf16_autocast_ms": round(ms_t, 3), "torch_peak_fraction": round(fl / ms_t / 1e-3 / PEAK, 3),
                        "speedup_vs_torch": round(ms_t / ms, 2)})
        print(json.dumps(row), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
