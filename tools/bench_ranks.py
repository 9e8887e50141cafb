#!/usr/bin/env python3
"""Recall@k of a validation epoch at three sizes: ``retrieval.mutual_recall`` (both directions' ranks out of the score GEMM's epilogue,
csrc/rank.hip) against what the validation epoch ran before it, in ONE process, the routes alternating in blocks after warm-up (and
alternating who goes first), device events around every block.  Prints one JSON line per shape: the median and every block of every
route, and the peak device memory each route allocates above the inputs.

    (p) parent   ``score = a @ b.t()`` (stock fp32 matmul) + ``mutualRetrieval(score, score.t(), ...)``: the [nA, nB] matrix and the
                 masked-maximum / comparison temporaries of ``retrieval._recall`` over it, once per direction
    (n) new      ``mutual_recall(a, b, ...)``: both splits, the two launches of sc_rank_counts_bf16, the finishing rule on the vectors
    (i) indexed  ``mutual_recall(a, GalleryIndex(b), ...)`` with the index built beforehand: what a fixed distractor gallery costs per call

Ids: 5 rows of A per row of B (5 captions per image); rows of B beyond nA / 5 are distractors.  When (p) cannot allocate its matrices
the record says so instead of giving a time.

    python tools/bench_ranks.py --reps 3 --blocks 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

SHAPES = (("Flickr8k validation", 5000, 1000, 512), ("SpokenCOCO test", 25000, 5000, 768), ("distractor gallery", 2000, 1000000, 512))
RECALL_AT = [1, 5, 10, 50]


def unit_rows_randn(n, E, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(n, E, device=dev)
    for r0 in range(0, n, 65536):                        # in pieces: no second full-size temporary
        x = torch.randn(min(65536, n - r0), E, device=dev, generator=g)
        out[r0: r0 + x.shape[0]] = x / x.norm(dim=1, keepdim=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", type=str, default="0,1,2")
    ap.add_argument("--custom", type=str, default="", help="further shapes as nA,nB,E;nA,nB,E;... (run instead of --shapes)")
    args = ap.parse_args()
    from speechclip_plus_amd import GalleryIndex, mutual_recall, mutualRetrieval, ops
    dev = torch.device("cuda:0")
    shapes = [SHAPES[int(s)] for s in args.shapes.split(",")]
    if args.custom:
        shapes = [("custom",) + tuple(int(v) for v in c.split(",")) for c in args.custom.split(";")]
    for name, nA, nB, E in shapes:
        a, b = unit_rows_randn(nA, E, dev, 1), unit_rows_randn(nB, E, dev, 2)
        a_ids, b_ids = torch.arange(nA, device=dev) // 5, torch.arange(nB, device=dev)
        out = {}

        def parent():
            score = a @ b.t()
            out["p"] = mutualRetrieval(score, score.t(), a_ids, b_ids, RECALL_AT)

        def new():
            out["n"] = mutual_recall(a, b, a_ids, b_ids, RECALL_AT)

        def indexed():
            out["i"] = mutual_recall(a, index, a_ids, b_ids, RECALL_AT)

        peak, failed = {}, {}
        for rname, fn in (("parent", parent), ("new", new)):          # peak memory above what is allocated going in: one call each
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()                      # the inputs (and, for the second route, the BLAS workspace the first left)
            try:
                fn()
                torch.cuda.synchronize()
                peak[rname] = torch.cuda.max_memory_allocated() - base
            except torch.cuda.OutOfMemoryError as e:
                failed[rname] = str(e).splitlines()[0]
        index = GalleryIndex(b)
        routes = tuple((n, f) for n, f in (("parent", parent), ("new", new), ("indexed", indexed)) if n not in failed)
        for _, fn in routes:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n, _ in routes}
        for blk in range(args.blocks):
            r = blk % len(routes)
            for rname, fn in routes[r:] + routes[:r]:                 # alternate, and rotate who goes first
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[rname].append(e0.elapsed_time(e1) / args.reps)
        med = {n: statistics.median(t) for n, t in times.items()}
        rec = {"shape": name, "nA": nA, "nB": nB, "E": E, "recall_at": RECALL_AT, "device": torch.cuda.get_device_name(0),
               "clock": "device events around blocks of --reps calls, ms per call", "reps_per_block": args.reps, "blocks": args.blocks,
               "slabs": ops.search_slabs(nA, nB, 1), "score_matrix_bytes": nA * nB * 4, "index_bytes": index.split.numel() * 2}
        for rname in ("parent", "new", "indexed"):
            if rname in failed:
                rec[rname + "_failed"] = failed[rname]
                continue
            rec[rname + "_ms"] = [round(t, 3) for t in times[rname]]
            rec[rname + "_ms_median"] = round(med[rname], 3)
            if rname in peak:
                rec[rname + "_peak_bytes_above_inputs"] = peak[rname]
        if "parent" in med:
            rec["parent_spread_ms"] = round(max(times["parent"]) - min(times["parent"]), 3)
            rec["faster"] = "new" if med["new"] < med["parent"] else "parent"
            rec["max_recall_difference_new_vs_parent"] = max(abs(out["n"][d][key] - out["p"][d][key]) for d in range(3) for key in out["p"][d])
        rec["recall_new_AB"] = out["n"][0]
        print(json.dumps(rec), flush=True)
        del a, b, index, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
