#!/usr/bin/env python3
"""Compact gallery search against ``search`` at three sizes, on tools/bench_search.py's protocol: ONE process, the routes alternating in
blocks after warm-up (and rotating who goes first), device events around every block, ms per call.  Prints one JSON line per shape:
the median and every block of every route, the certified fraction, both index sizes and whether the routes return the same lists.

    (s) search         search(queries, GalleryIndex, k) as shipped: the three-way split index, retrieval.default_route picks the route
    (e) compact_exact  search_compact(queries, CompactGalleryIndex, k, depth, fallback="exact"): coarse scan + re-rank + the host's look
                       at the mask (+ the exact fallback for the uncertified queries, if any)
    (n) compact_none   the same with fallback="none": no synchronisation, no fallback

Both indexes are built once, outside the clock.  Unit Gaussian rows: what a trained model's embeddings certify is not measured here.

    python tools/bench_compact_search.py --reps 3 --blocks 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

SHAPES = (("large gallery", 1024, 1000000, 512), ("fused threshold", 25000, 131072, 512), ("SpokenCOCO test", 25000, 5000, 768))


def unit_rows_randn(n, E, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(n, E, device=dev)
    for r0 in range(0, n, 65536):                        # in pieces: no second full-size temporary
        x = torch.randn(min(65536, n - r0), E, device=dev, generator=g)
        out[r0: r0 + x.shape[0]] = x / x.norm(dim=1, keepdim=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", type=str, default="0,1,2")
    ap.add_argument("--custom", type=str, default="", help="further shapes as nQ,N,E;nQ,N,E;... (run instead of --shapes)")
    args = ap.parse_args()
    from speechclip_plus_amd import CompactGalleryIndex, GalleryIndex, ops, search, search_compact
    from speechclip_plus_amd.retrieval import default_route
    dev = torch.device("cuda:0")
    k, D = args.k, args.depth
    shapes = [SHAPES[int(s)] for s in args.shapes.split(",")]
    if args.custom:
        shapes = [("custom",) + tuple(int(v) for v in c.split(",")) for c in args.custom.split(";")]
    for name, nQ, N, E in shapes:
        q, gal = unit_rows_randn(nQ, E, dev, 1), unit_rows_randn(N, E, dev, 2)
        index = GalleryIndex(gal)
        compact = CompactGalleryIndex(gal)
        out = {}

        def parent():
            out["s"] = search(q, index, k)

        def compact_exact():
            out["e"] = search_compact(q, compact, k, depth=D, fallback="exact")

        def compact_none():
            out["n"] = search_compact(q, compact, k, depth=D, fallback="none")

        routes = (("search", parent), ("compact_exact", compact_exact), ("compact_none", compact_none))
        for _, fn in routes:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n, _ in routes}
        for b in range(args.blocks):
            order = routes[b % 3:] + routes[: b % 3]                 # alternate, and rotate who goes first
            for rname, fn in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[rname].append(e0.elapsed_time(e1) / args.reps)
        med = {n: statistics.median(t) for n, t in times.items()}
        spread = max(times["search"]) - min(times["search"])
        cert = out["e"][2]
        rec = {"shape": name, "nQ": nQ, "N": N, "E": E, "k": k, "depth": D, "device": torch.cuda.get_device_name(0),
               "clock": "device events around blocks of --reps calls, ms per call", "reps_per_block": args.reps, "blocks": args.blocks,
               "search_route": default_route(nQ, N), "coarse_slabs": ops.search_slabs(min(nQ, 16384), N, D),
               "search_ms": [round(t, 3) for t in times["search"]], "compact_exact_ms": [round(t, 3) for t in times["compact_exact"]],
               "compact_none_ms": [round(t, 3) for t in times["compact_none"]],
               "search_ms_median": round(med["search"], 3), "compact_exact_ms_median": round(med["compact_exact"], 3),
               "compact_none_ms_median": round(med["compact_none"], 3), "search_spread_ms": round(spread, 3),
               "compact_exact_faster_beyond_spread": med["compact_exact"] < med["search"] - spread,
               "compact_exact_slower_beyond_spread": med["compact_exact"] > med["search"] + spread,
               "certified_fraction": float(cert.float().mean()), "eps_scale": {"gmax": compact.gmax, "gtmax": compact.gtmax, "dmax": compact.dmax},
               "gallery_index_bytes": index.split.numel() * 2, "compact_index_bytes": compact.nbytes,
               "rows_with_equal_lists_exact_vs_search": float((out["e"][1] == out["s"][1]).all(dim=1).float().mean()),
               "rows_with_equal_lists_none_vs_exact": float((out["n"][1] == out["e"][1]).all(dim=1).float().mean())}
        print(json.dumps(rec), flush=True)
        del q, gal, index, compact, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
