#!/usr/bin/env python3
"""Sharded search (retrieval.search_sharded, csrc/search_merge_wide.hip) on tools/bench_search_wide.py's protocol: ONE process, the two
sides alternating in blocks after a warm-up at every switch (and alternating who goes first), device events around every block, ms per
call, the median of five blocks.  One JSON line per run with the median and every block of each side and the spread of the blocks.

    merge       the merge alone on random best-first lists [S, nQ, k] (distinct values, so torch's order is the same):
                    (s) ops.search_merge_lists(part_vals, part_idx, row0, k)
                    (t) torch.topk over the concatenated [nQ, S k] values + the gather of the global rows   (a time yardstick only:
                        no tie order, fillers not told from real -inf)
                at (nQ, S, k) = (4096, 4, 100), (1024, 8, 256), (1024, 16, 1024)
    capability  1 024 x 1 000 000 x 512 at k = 100 and 256, where ``search`` refuses (more than 262 144 rows at k > 32):
                    (s) search_sharded(q, ShardedGalleryIndex(gallery), k)          four shards (--shard-rows: smaller ones)
                    (t) torch.matmul + torch.topk per gallery chunk of 262 144 rows, torch.topk over the chunks' lists + gather
                and the merge alone at that (nQ, S, k), for its share of the call
    cost        N = 262 144, k = 100, where sharding is not needed:
                    (s) search_sharded on two shards of 131 072 rows
                    (t) search on the whole gallery (this tree)

The indexes are built once, outside the clock.  Unit Gaussian rows.

    python tools/bench_search_sharded.py --blocks 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

MERGE_SHAPES = ((4096, 4, 100), (1024, 8, 256), (1024, 16, 1024))


def unit_rows_randn(n, E, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, E, device=dev, generator=g)
    return x / x.norm(dim=1, keepdim=True)


def alternate(sides, reps, blocks, warmup):
    """sides: ((name, fn), (name, fn)) -> {name: [ms per call of every block]}; a warm-up after every switch, the first side alternating"""
    times = {n: [] for n, _ in sides}
    for b in range(blocks):
        for name, fn in (sides if b % 2 == 0 else sides[::-1]):
            for _ in range(warmup):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    return times


def report(times, a, b):
    rec = {}
    for n, t in times.items():
        rec[n + "_ms"] = [round(v, 4) for v in t]
        rec[n + "_ms_median"] = round(statistics.median(t), 4)
        rec[n + "_spread_ms"] = round(max(t) - min(t), 4)
    rec[f"{a}_over_{b}"] = round(statistics.median(times[a]) / statistics.median(times[b]), 3)
    return rec


def random_lists(nQ, S, k, rows_per_shard, dev, seed):
    """-> (part_vals [S, nQ, k] best first, part_idx [S, nQ, k] int32 rows of the shard, row0 [S])"""
    g = torch.Generator(device=dev).manual_seed(seed)
    pv = torch.sort(torch.randn(S, nQ, k, device=dev, generator=g), dim=2, descending=True).values.contiguous()
    pi = torch.randint(0, rows_per_shard, (S, nQ, k), device=dev, generator=g, dtype=torch.int32)
    return pv, pi, torch.arange(S, device=dev, dtype=torch.int64) * rows_per_shard


def time_merge(ops, nQ, S, k, dev, args):
    pv, pi, row0 = random_lists(nQ, S, k, 250000, dev, 7)
    vals = torch.empty(nQ, k, device=dev, dtype=torch.float32)
    idx = torch.empty(nQ, k, device=dev, dtype=torch.int32)
    cat_v = pv.permute(1, 0, 2).reshape(nQ, S * k).contiguous()       # the torch side's operands are laid out for it outside the clock
    cat_i = (pi.long() + row0.view(S, 1, 1)).permute(1, 0, 2).reshape(nQ, S * k).contiguous()
    out = {}

    def merge():
        ops.search_merge_lists(pv, pi, row0, k, vals=vals, idx=idx)

    def torch_side():
        v, pos = torch.topk(cat_v, k, dim=1, sorted=True)
        out["t"] = (v, torch.gather(cat_i, 1, pos))

    times = alternate((("merge", merge), ("torch", torch_side)), args.merge_reps, args.blocks, args.warmup)
    same = bool(torch.equal(vals, out["t"][0]) and torch.equal(idx.long(), out["t"][1]))
    return times, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="whole calls per timed block")
    ap.add_argument("--merge-reps", type=int, default=100, help="merge launches per timed block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls after every switch of sides")
    ap.add_argument("--parts", type=str, default="merge,capability,cost")
    ap.add_argument("--N", type=int, default=1000000, help="gallery rows of the capability run")
    ap.add_argument("--shard-rows", type=int, default=0, help="capability run: rows per shard (0: the default, wide_max_gallery() = 262 144)")
    args = ap.parse_args()
    from speechclip_plus_amd import GalleryIndex, ShardedGalleryIndex, ops, search, search_sharded
    from speechclip_plus_amd.retrieval import wide_max_gallery
    dev = torch.device("cuda:0")
    base = {"device": torch.cuda.get_device_name(0), "clock": "device events around blocks of calls, ms per call", "blocks": args.blocks,
            "warmup_after_every_switch": args.warmup}
    parts = args.parts.split(",")

    if "merge" in parts:
        for nQ, S, k in MERGE_SHAPES:
            times, same = time_merge(ops, nQ, S, k, dev, args)
            print(json.dumps({**base, "what": "merge", "nQ": nQ, "S": S, "k": k, "reps_per_block": args.merge_reps,
                              **report(times, "merge", "torch"), "equal_lists": same}), flush=True)

    if "capability" in parts:
        nQ, N, E = 1024, args.N, 512
        q, gal = unit_rows_randn(nQ, E, dev, 1), unit_rows_randn(N, E, dev, 2)
        index = ShardedGalleryIndex(gal, shard_rows=args.shard_rows or None)
        S, step = len(index.shards), wide_max_gallery()
        out = {}
        for k in (100, 256):
            def sharded():
                out["s"] = search_sharded(q, index, k)

            def torch_side():
                pv, pi = [], []
                for c0 in range(0, N, step):
                    v, i = torch.topk(q @ gal[c0: c0 + step].t(), k, dim=1, sorted=True)
                    pv.append(v)
                    pi.append(i + c0)
                v, pos = torch.topk(torch.cat(pv, dim=1), k, dim=1, sorted=True)
                out["t"] = (v, torch.gather(torch.cat(pi, dim=1), 1, pos))

            times = alternate((("sharded", sharded), ("torch", torch_side)), args.reps, args.blocks, args.warmup)
            same = float((out["s"][1] == out["t"][1]).all(dim=1).float().mean())
            merge_ms = statistics.median(time_merge(ops, nQ, S, k, dev, args)[0]["merge"])
            rec = report(times, "sharded", "torch")
            print(json.dumps({**base, "what": "capability", "nQ": nQ, "N": N, "E": E, "k": k, "shards": S, "shard_rows": args.shard_rows or step, "reps_per_block": args.reps, **rec,
                              "rows_with_equal_lists": same, "merge_alone_ms": round(merge_ms, 4),
                              "merge_share_of_call": round(merge_ms / rec["sharded_ms_median"], 4)}), flush=True)
        del q, gal, index, out
        torch.cuda.empty_cache()

    if "cost" in parts:
        nQ, N, E, k = 1024, 262144, 512, 100
        q, gal = unit_rows_randn(nQ, E, dev, 1), unit_rows_randn(N, E, dev, 2)
        whole, index = GalleryIndex(gal), ShardedGalleryIndex(gal, shard_rows=N // 2)
        out = {}

        def sharded():
            out["s"] = search_sharded(q, index, k)

        def plain():
            out["w"] = search(q, whole, k)

        times = alternate((("sharded", sharded), ("search", plain)), 10, args.blocks, args.warmup)
        same = bool(torch.equal(out["s"][1], out["w"][1]) and torch.equal(out["s"][0], out["w"][0]))
        merge_ms = statistics.median(time_merge(ops, nQ, 2, k, dev, args)[0]["merge"])
        print(json.dumps({**base, "what": "cost", "nQ": nQ, "N": N, "E": E, "k": k, "shards": 2, "reps_per_block": 10,
                          **report(times, "sharded", "search"), "equal_bits": same, "merge_alone_ms": round(merge_ms, 4)}), flush=True)


if __name__ == "__main__":
    main()
