#!/usr/bin/env python3
"""What raw-image input costs against handing the tower ready-made pixels, at B synthetic 500 x 375 images (speechclip_plus_amd/
image_prep.py, csrc/image_prep.hip).  One process, alternating rounds, host clock around work that ends in a device synchronise:

  (a) tensor   ClipImageEncoder.forward on the fp32 [B, 3, 224, 224] batch, including its pinned H2D copy on the copy stream (the path
               before raw input existed; the CPU transform that made the pixels is NOT in it)
  (b) raw      forward on the packed raw batch on the host: its pinned copy, the table upload, both kernels, warm table cache

and, separately: the two kernels' time per launch (device events around back-to-back launches of each), the host microseconds per batch
spent preparing descriptors (warm plan cache: the look-up; cold: building the batch's tables from warm per-size windows), and the
one-thread CPU transform on this host (PIL + torch if PIL imports, else image_prep.reference_transform; the line says which).
If (b) exceeds (a) by more than the kernels' own time plus 50 us of host work, the preparation is stalling the stream.  One JSON line.

    python3 tools/bench_image_prep.py [--batch 64] [--tower ViT-B/32] [--layers 12] [--rounds 30]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tower", default="ViT-B/32")
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--size", default="500x375")
    a = ap.parse_args()
    import numpy as np
    import torch
    from image_prep_cases import make_source
    from speechclip_plus_amd import image_prep, ops
    from speechclip_plus_amd.clip_image import CLIP_IMAGE_MEAN, CLIP_IMAGE_STD, ClipImageEncoder
    assert torch.cuda.is_available(), "bench_image_prep.py measures on the GPU: no device, no numbers"
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    w, h = (int(v) for v in a.size.split("x"))
    B = a.batch
    imgs = [torch.from_numpy(make_source(w, h, "noise", seed=b)) for b in range(B)]
    m = ClipImageEncoder(a.tower, layers=a.layers, seed=1).to(dev)
    raw_host = image_prep.pack_host(imgs)
    raw_host.packed = raw_host.packed.pin_memory()
    pix_host = m.prep_image(raw_host).cpu().pin_memory()
    cs = ops.shared_stream("h2d", dev, priority=-1)
    main_s = torch.cuda.current_stream(dev)

    def tensor_route():
        with torch.cuda.stream(cs):
            pix = pix_host.to(dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        main_s.wait_event(ev)
        pix.record_stream(main_s)
        return m(pix)

    def raw_route():
        return m(raw_host)

    want = tensor_route()
    assert torch.equal(raw_route(), want), "the two routes must give the same embeddings"
    for _ in range(5):
        tensor_route(), raw_route()
    torch.cuda.synchronize()
    t = {"tensor": [], "raw": []}
    for _ in range(a.rounds):
        for name, fn in (("tensor", tensor_route), ("raw", raw_route)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3)

    # the two kernels alone: back-to-back launches between device events
    pl = image_prep.plan(raw_host.hw, raw_host.offsets)
    src, tab, lut = raw_host.packed.to(dev), pl.tab.to(dev), image_prep.norm_lut().to(dev)
    mid = torch.empty(pl.mid_bytes, dtype=torch.uint8, device=dev)
    seg, _ = m.segments(B, dev)
    A = torch.empty(seg.rows, m.Kp, dtype=torch.bfloat16, device=dev)
    out = torch.empty(B, 3, 224, 224, device=dev)

    def per_launch(fn, n=200):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    k_h = per_launch(lambda: ops.image_resample_h(src, tab, mid, pl))
    k_va = per_launch(lambda: ops.image_resample_v_norm(mid, tab, lut, pl, None, A, seg, m.patch, m.Kp))
    k_vp = per_launch(lambda: ops.image_resample_v_norm(mid, tab, lut, pl, out, None))
    k_patchify = per_launch(lambda: ops.vit_patchify(out, seg, m.patch, m.Kp))

    # host: descriptors per batch
    hw, offs = raw_host.hw, raw_host.offsets
    t0 = time.perf_counter()
    for _ in range(200):
        image_prep.plan(hw, offs)
    warm_us = (time.perf_counter() - t0) / 200 * 1e6
    cold = []
    for _ in range(20):
        image_prep._PLAN_CACHE.clear()
        t0 = time.perf_counter()
        image_prep.plan(hw, offs)
        cold.append((time.perf_counter() - t0) * 1e6)

    # the CPU transform the raw route replaces, one thread
    try:
        from PIL import Image
        mean, std = torch.tensor(CLIP_IMAGE_MEAN).view(3, 1, 1), torch.tensor(CLIP_IMAGE_STD).view(3, 1, 1)
        ow, oh, left, top = image_prep.clip_resize_geometry(w, h)

        def cpu_one(im):
            r = im.resize((ow, oh), Image.BICUBIC).crop((left, top, left + 224, top + 224))
            return torch.from_numpy(np.array(r)).permute(2, 0, 1).float().div(255).sub(mean).div(std)
        pil = [Image.fromarray(t_.numpy(), "RGB") for t_ in imgs[:16]]
        how = "PIL " + __import__("PIL").__version__ + " resize + crop + torch normalise"
    except ImportError:
        cpu_one, pil = (lambda im: image_prep.reference_transform(im.numpy())), imgs[:16]
        how = "image_prep.reference_transform (numpy; PIL does not import)"
    cpu_one(pil[0])
    t0 = time.perf_counter()
    for im in pil:
        cpu_one(im)
    cpu_ms = (time.perf_counter() - t0) / len(pil) * 1e3

    med = {k: statistics.median(v) for k, v in t.items()}
    row = {"tower": a.tower, "layers": m.arch["layers"], "batch": B, "size": a.size, "rounds": a.rounds,
           "tensor_route_ms": {"median": round(med["tensor"], 3), "min": round(min(t["tensor"]), 3)},
           "raw_route_ms": {"median": round(med["raw"], 3), "min": round(min(t["raw"]), 3)},
           "raw_minus_tensor_us": round((med["raw"] - med["tensor"]) * 1e3, 1),
           "kernel_us": {"resample_h": round(k_h, 1), "resample_v_norm_A": round(k_va, 1), "resample_v_norm_pixels": round(k_vp, 1),
                         "vit_patchify": round(k_patchify, 1)},
           "kernels_plus_50_us": round(k_h + k_va + 50, 1),
           "host_descriptor_us": {"warm": round(warm_us, 1), "cold_median": round(statistics.median(cold), 1)},
           "h2d_bytes": {"tensor": pix_host.numel() * 4, "raw": raw_host.packed.numel() + pl.tab.numel() * 4},
           "cpu_transform_ms_per_image": round(cpu_ms, 3), "cpu_transform": how,
           "clock": time.strftime("%Y-%m-%d %H:%M:%S %Z")}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
