#!/usr/bin/env python3
"""What raw-audio input costs: ``audio_prep.prep_audio`` of B utterances of S seconds of int16 PCM, mono and stereo, at 44 100 and 48 000 Hz
(speechclip_plus_amd/audio_prep.py, csrc/audio_prep.hip).  Per case, on the GPU:

  kernel_us     sc_audio_resample alone on device-resident PCM: device events around back-to-back launches, after warm-up, the median of
                --repeats such windows
  roofline_us   (a) the bytes the kernel has to move - the PCM once, the fp32 output once - over the HBM bandwidth a float4 copy reaches
                on an MI355X (6.29 TB/s; 8.0 TB/s is the specification)
  prep_ms       the whole call from PCM on the host: packing into the pinned buffer, the one H2D copy, the launch; host clock around work
                that ends in a device synchronise, median
  packed_ms     ``audio_prep.run`` on a batch a loader already packed into pinned memory (``collate_general(pin_memory=True)``): the copy,
                the descriptors and the launch, without the packing; host clock, median
  host_ms       (b) what a user does today: scipy.signal.resample_poly per utterance (to float, to mono, resample) on 16 threads, then the
                pinned fp32 H2D copy of the padded batch; host clock, median

One JSON line per case.  Informational: no threshold.

    python3 tools/bench_audio_prep.py [--batch 64] [--seconds 10] [--repeats 9] [--launches 20]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import numpy as np
    import torch
    from scipy.signal import resample_poly
    from speechclip_plus_amd import audio_prep, ops
    assert torch.cuda.is_available(), "bench_audio_prep.py measures on the GPU: no device, no numbers"
    dev = torch.device("cuda:0")
    B = a.batch
    for sr in (44100, 48000):
        for ch in (1, 2):
            n = int(a.seconds * sr)
            g = torch.Generator().manual_seed(sr + ch)
            xs = [torch.randint(-32768, 32768, (n, ch) if ch > 1 else (n,), generator=g).to(torch.int16) for _ in range(B)]
            P, Q, taps = audio_prep.resample_geometry(sr)
            n_out, tile = audio_prep.out_len(n, sr), audio_prep.tile_outputs(sr)

            # the kernel alone
            raw = audio_prep.pack(audio_prep.as_entries(xs, sr))
            src = raw.packed.to(dev)
            desc = torch.tensor([(raw.offsets[b] * 2, n, ch, n_out, b) for b in range(B)], dtype=torch.int64, device=dev)
            table, first = audio_prep.resample_table(sr, dev)
            out = torch.empty(B, n_out, device=dev)
            launch = lambda: ops.audio_resample(src, desc, table, first, P, Q, taps, tile, out)
            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            windows = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                windows.append(e0.elapsed_time(e1) / a.launches * 1e3)
            kernel_us = statistics.median(windows)
            moved = src.numel() * 2 + out.numel() * 4

            # the whole call from host PCM
            for _ in range(2):
                audio_prep.prep_audio(xs, sr, dev)
            torch.cuda.synchronize()
            prep = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                wav, _ = audio_prep.prep_audio(xs, sr, dev)
                torch.cuda.synchronize()
                prep.append((time.perf_counter() - t0) * 1e3)
            assert torch.equal(wav, out)

            # ... and from a batch a loader packed into pinned memory already: the copy and the launch
            pinned = audio_prep.pack(audio_prep.as_entries(xs, sr), pin_memory=True)
            audio_prep.run(pinned, dev)
            torch.cuda.synchronize()
            packed_ms = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                wav2, _ = audio_prep.run(pinned, dev)
                torch.cuda.synchronize()
                packed_ms.append((time.perf_counter() - t0) * 1e3)
            assert torch.equal(wav2, out)

            # the host alternative
            nps = [x.numpy() for x in xs]

            def one(x):
                f = x.astype(np.float32) / 32768.0
                return resample_poly(f if f.ndim == 1 else f.mean(axis=1), Q, P).astype(np.float32)

            stage = torch.empty(B, n_out, dtype=torch.float32).pin_memory()
            host = []
            with ThreadPoolExecutor(a.threads) as pool:
                for _ in range(max(a.repeats // 3, 2)):
                    t0 = time.perf_counter()
                    for b, y in enumerate(pool.map(one, nps)):
                        stage[b].copy_(torch.from_numpy(y[:n_out]))
                    d = stage.to(dev, non_blocking=True)
                    torch.cuda.synchronize()
                    host.append((time.perf_counter() - t0) * 1e3)
            diff = float((d - wav).abs().max())

            roof = moved / (HBM_MEASURED_TBS * 1e12) * 1e6
            print(json.dumps({"sr": sr, "channels": ch, "batch": B, "seconds": a.seconds, "P": P, "Q": Q, "taps": taps, "tile": tile,
                              "kernel_us": {"median": round(kernel_us, 1), "min": round(min(windows), 1), "max": round(max(windows), 1)},
                              "bytes_moved": moved, "roofline_us_at_6.29_TBs": round(roof, 1),
                              "roofline_us_at_8.0_TBs": round(moved / (HBM_SPEC_TBS * 1e12) * 1e6, 1),
                              "kernel_over_roofline": round(kernel_us / roof, 2), "achieved_TBs": round(moved / kernel_us * 1e-6, 3),
                              "prep_ms": {"median": round(statistics.median(prep), 2), "min": round(min(prep), 2)},
                              "packed_ms": {"median": round(statistics.median(packed_ms), 2), "min": round(min(packed_ms), 2)},
                              "host_ms": {"median": round(statistics.median(host), 1), "min": round(min(host), 1), "threads": a.threads},
                              "host_over_prep": round(statistics.median(host) / statistics.median(prep), 1),
                              "max_abs_diff_scipy_vs_device": diff, "h2d_bytes": {"prep": src.numel() * 2, "host": stage.numel() * 4},
                              "clock": time.strftime("%Y-%m-%d %H:%M:%S %Z")}), flush=True)


if __name__ == "__main__":
    main()
