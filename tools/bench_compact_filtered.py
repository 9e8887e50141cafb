#!/usr/bin/env python3
"""Filtered compact gallery search against the unfiltered compact call and against the filtered ``search`` on a GalleryIndex, at three
sizes, on tools/bench_filtered_search.py's protocol: ONE process, the routes alternating in blocks after warm-up (and rotating who
goes first), device events around every block, ms per call.  Prints one JSON line per shape: the median and every block of every
route, the spread of every route, the certified fraction, and whether the filtered lists agree.

    (c)  compact            search_compact(queries, CompactGalleryIndex, k, depth=32) without a filter, as shipped: what the filter
                            costs on the compact route is (cf) - (c)
    (cf) compact filtered   the same call with query_ids=..., gallery_ids=..., live=...: csrc/search_compact_filter.hip
    (f)  filtered search    search(queries, GalleryIndex, k, query_ids=..., gallery_ids=..., live=...): csrc/search_filter.hip on the
                            route retrieval.default_route picks, six times the index bytes

The filter has the corpora's shape: five gallery rows per id (five spoken captions per image), every query carries the id of some
gallery row, plus 1 % removed rows.  Both indexes are built once, outside the clock, and so are the per-row norms the call-time mask
needs.  Unit Gaussian rows, fallback="exact" (the certified fraction is reported: an uncertified row costs a pass over the gallery).

    python tools/bench_compact_filtered.py --reps 3 --blocks 5
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
        g_ids = torch.arange(N, device=dev, dtype=torch.int64) // 5                  # five rows per id
        q_ids = (torch.arange(nQ, device=dev, dtype=torch.int64) * 7919) % (-(-N // 5))
        live = torch.rand(N, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) >= 0.01
        compact = CompactGalleryIndex(gal)
        index = GalleryIndex(gal)
        out = {}

        def unfiltered():
            out["c"] = search_compact(q, compact, k, depth=D)

        def compact_filtered():
            out["cf"] = search_compact(q, compact, k, depth=D, query_ids=q_ids, gallery_ids=g_ids, live=live)

        def filtered():
            out["f"] = search(q, index, k, query_ids=q_ids, gallery_ids=g_ids, live=live)

        routes = (("compact", unfiltered), ("compact_filtered", compact_filtered), ("filtered", filtered))
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
        spread = {n: max(t) - min(t) for n, t in times.items()}
        ci, fi = out["cf"][1], out["f"][1]
        adm_ok = bool(((g_ids[ci.clamp(min=0)] != q_ids.unsqueeze(1)) & live[ci.clamp(min=0)] & (ci >= 0)).all())
        rec = {"shape": name, "nQ": nQ, "N": N, "E": E, "k": k, "depth": D, "device": torch.cuda.get_device_name(0),
               "clock": "device events around blocks of --reps calls, ms per call", "reps_per_block": args.reps, "blocks": args.blocks,
               "filtered_search_route": default_route(nQ, N), "coarse_slabs": ops.search_slabs(min(nQ, 16384), N, D),
               "rows_per_query_id": 5, "dead_fraction": round(1.0 - float(live.float().mean()), 5),
               "compact_ms": [round(t, 3) for t in times["compact"]],
               "compact_filtered_ms": [round(t, 3) for t in times["compact_filtered"]],
               "filtered_ms": [round(t, 3) for t in times["filtered"]],
               "compact_ms_median": round(med["compact"], 3), "compact_filtered_ms_median": round(med["compact_filtered"], 3),
               "filtered_ms_median": round(med["filtered"], 3),
               "compact_spread_ms": round(spread["compact"], 3), "compact_filtered_spread_ms": round(spread["compact_filtered"], 3),
               "filtered_spread_ms": round(spread["filtered"], 3),
               "filter_cost_ms": round(med["compact_filtered"] - med["compact"], 3),
               "filter_cost_inside_compact_spread": abs(med["compact_filtered"] - med["compact"]) <= spread["compact"],
               "compact_filtered_faster_than_filtered_search": med["compact_filtered"] < med["filtered"],
               "certified_unfiltered": float(out["c"][2].float().mean()), "certified_filtered": float(out["cf"][2].float().mean()),
               "index_bytes_compact": compact.nbytes, "index_bytes_gallery_index": index.split.numel() * 2,
               "every_returned_row_admissible": adm_ok,
               "rows_with_equal_lists_compact_filtered_vs_filtered_search": float((ci == fi).all(dim=1).float().mean())}
        print(json.dumps(rec), flush=True)
        del q, gal, index, compact, out, g_ids, q_ids, live, ci, fi
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
