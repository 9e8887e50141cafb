#!/usr/bin/env python3
"""Gallery search at three sizes: ``retrieval.search`` (top-k fused into the score GEMM, csrc/search.hip) against the composition that
existed before it and against stock torch, in ONE process, the routes alternating in blocks after warm-up (and alternating who goes
first), device events around every block.  Prints one JSON line per shape: the median and every block of every route.

    (a) fused        search(queries, GalleryIndex, k, route="fused"): the query split + sc_search_topk_bf16 (+ the slab merge); gallery pre-indexed
    (b) composition  per row chunk: ops.cosine_scores_split (query split + the bf16 GEMM over the same pre-split gallery) into a
                     128 MiB fp32 scratch, then ops.topk_rows - what keyword_neighbors does with the token table
    (c) torch        fp32 ``matmul`` + ``torch.topk`` with the same chunking
    (s) search       search(queries, GalleryIndex, k) as shipped: retrieval.default_route picks (a) or (b) by the gallery size

Route (b) needs whole score rows: when 128 rows of scores do not fit 128 MiB (a gallery of a million), it gets the smallest buffer
that holds a 128-row chunk, and the record says so (``scratch_bytes``).

    python tools/bench_search.py --reps 3 --blocks 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

SHAPES = (("Flickr8k validation", 5000, 1000, 512), ("SpokenCOCO test", 25000, 5000, 768), ("large gallery", 1024, 1000000, 512))
SCRATCH = 128 << 20


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
    ap.add_argument("--reps", type=int, default=3, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", type=str, default="0,1,2")
    ap.add_argument("--custom", type=str, default="", help="further shapes as nQ,N,E;nQ,N,E;... (run instead of --shapes)")
    args = ap.parse_args()
    from speechclip_plus_amd import GalleryIndex, ops, search
    from speechclip_plus_amd.retrieval import default_route
    dev = torch.device("cuda:0")
    k = args.k
    shapes = [SHAPES[int(s)] for s in args.shapes.split(",")]
    if args.custom:
        shapes = [("custom",) + tuple(int(v) for v in c.split(",")) for c in args.custom.split(";")]
    for name, nQ, N, E in shapes:
        q, gal = unit_rows_randn(nQ, E, dev, 1), unit_rows_randn(N, E, dev, 2)
        index = GalleryIndex(gal)
        Np = index.split.shape[0]
        chunk = max(128, SCRATCH // (4 * Np) // 128 * 128)
        chunk = min(chunk, -(-nQ // 128) * 128)
        scores = torch.empty(chunk, Np, device=dev, dtype=torch.float32)
        split = torch.empty(chunk, index.split.shape[1], device=dev, dtype=torch.bfloat16)
        vals_b = torch.empty(nQ, k, device=dev, dtype=torch.float32)
        idx_b = torch.empty(nQ, k, device=dev, dtype=torch.int32)
        out = {}

        def fused():
            out["a"] = search(q, index, k, route="fused")

        def auto():
            out["s"] = search(q, index, k)

        def composition():
            for r0 in range(0, nQ, chunk):
                r1 = min(nQ, r0 + chunk)
                rp = -(-(r1 - r0) // 128) * 128
                ops.cosine_scores_split(q[r0:r1], None, index.split, Np, out=scores[:rp], split_out=split[:rp])
                ops.topk_rows(scores[: r1 - r0], N, k, vals=vals_b[r0:r1], idx=idx_b[r0:r1])
            out["b"] = (vals_b, idx_b)

        def stock():
            vs, ix = [], []
            for r0 in range(0, nQ, chunk):
                v, i = torch.topk(q[r0: r0 + chunk] @ gal.t(), k, dim=1)
                vs.append(v)
                ix.append(i)
            out["c"] = (torch.cat(vs), torch.cat(ix))

        routes = (("fused", fused), ("composition", composition), ("torch", stock), ("search", auto))
        for _, fn in routes:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n, _ in routes}
        for b in range(args.blocks):
            order = routes[b % 4:] + routes[: b % 4]                 # alternate, and rotate who goes first
            for rname, fn in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[rname].append(e0.elapsed_time(e1) / args.reps)
        same_ab = float((out["a"][1] == out["b"][1].long()).all(dim=1).float().mean())
        same_ac = float((out["a"][1] == out["c"][1]).all(dim=1).float().mean())
        med = {n: statistics.median(t) for n, t in times.items()}
        spread_b = max(times["composition"]) - min(times["composition"])
        rec = {"shape": name, "nQ": nQ, "N": N, "E": E, "k": k, "device": torch.cuda.get_device_name(0),
               "clock": "device events around blocks of --reps calls, ms per call", "reps_per_block": args.reps, "blocks": args.blocks,
               "slabs": ops.search_slabs(min(nQ, 16384), N, k), "chunk_rows": chunk, "scratch_bytes": scores.numel() * 4,
               "index_bytes": index.split.numel() * 2,
               "fused_ms": [round(t, 3) for t in times["fused"]], "composition_ms": [round(t, 3) for t in times["composition"]],
               "torch_ms": [round(t, 3) for t in times["torch"]], "search_ms": [round(t, 3) for t in times["search"]],
               "search_route": default_route(nQ, N), "search_ms_median": round(med["search"], 3),
               "search_not_slower": med["search"] <= med["composition"] + spread_b,
               "fused_ms_median": round(med["fused"], 3), "composition_ms_median": round(med["composition"], 3),
               "torch_ms_median": round(med["torch"], 3), "composition_spread_ms": round(spread_b, 3),
               "fused_not_slower": med["fused"] <= med["composition"] + spread_b,
               "rows_with_equal_lists_fused_vs_composition": same_ab, "rows_with_equal_lists_fused_vs_torch": same_ac}
        print(json.dumps(rec), flush=True)
        del q, gal, index, scores, split, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
