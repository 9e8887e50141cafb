#!/usr/bin/env python3
"""Sharded ranks (retrieval.mutual_ranks_sharded, csrc/rank.hip's two accumulating entries) against ``mutual_ranks`` on the whole gallery, on
tools/bench_search_sharded.py's protocol: ONE process, the two sides alternating in blocks after a warm-up at every switch (and
alternating who goes first), device events around every block, ms per call, the median of five blocks.  One JSON line per run with
the median and every block of each side and the spread of the blocks.

    (w) mutual_ranks(a, GalleryIndex(b), a_ids, b_ids)                        csrc/rank.hip: two launches on the whole gallery
    (s) mutual_ranks_sharded(a, ShardedGalleryIndex(b, shard_rows, ids), a_ids)   local form: two launches PER SHARD

at shard_rows 262 144, 131 072 and 65 536, and once more at one shard size with 1 % of the gallery's rows removed (where (w) runs on
an index of the surviving rows: the same answer).  Shapes are tools/bench_ranks.py's: 25 000 x 5 000 x 768 (one shard at every size:
what the two-entry form costs where sharding is not needed) and 2 000 x 1 000 000 x 512, five rows of A per id.  The indexes are
built once, outside the clock; both sides split A inside it.  (s) / (w) is a cost to write down, not a gate.

    python tools/bench_ranks_sharded.py --blocks 5
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from bench_ranks import unit_rows_randn                                # noqa: E402
from bench_search_sharded import alternate, report                     # noqa: E402

SHAPES = (("SpokenCOCO test", 25000, 5000, 768), ("distractor gallery", 2000, 1000000, 512))
KEYS = ("ahead_AB", "ahead_BA", "best_AB", "best_BA")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="whole calls per timed block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls after every switch of sides")
    ap.add_argument("--shapes", type=str, default="0,1")
    ap.add_argument("--shard-rows", type=str, default="262144,131072,65536")
    ap.add_argument("--removed-at", type=int, default=131072, help="shard_rows of the run with 1 %% of the rows removed (0: none)")
    args = ap.parse_args()
    from speechclip_plus_amd import GalleryIndex, ShardedGalleryIndex, mutual_ranks, mutual_ranks_sharded, ops
    dev = torch.device("cuda:0")
    base = {"device": torch.cuda.get_device_name(0), "clock": "device events around blocks of calls, ms per call", "blocks": args.blocks,
            "reps_per_block": args.reps, "warmup_after_every_switch": args.warmup}
    runs = [(int(r), False) for r in args.shard_rows.split(",")] + ([(args.removed_at, True)] if args.removed_at else [])
    for name, nA, nB, E in (SHAPES[int(s)] for s in args.shapes.split(",")):
        a, b = unit_rows_randn(nA, E, dev, 1), unit_rows_randn(nB, E, dev, 2)
        a_ids, b_ids = torch.arange(nA, device=dev) // 5, torch.arange(nB, device=dev)
        whole_all = GalleryIndex(b)
        gone = torch.randperm(nB, device=dev, generator=torch.Generator(device=dev).manual_seed(3))[: nB // 100]
        for shard_rows, removed in runs:
            index = ShardedGalleryIndex(b, shard_rows=shard_rows, ids=b_ids)
            whole, w_ids, live = whole_all, b_ids, None
            if removed:
                index.remove(gone)
                live = torch.ones(nB, device=dev, dtype=torch.bool)
                live[gone] = False
                whole, w_ids = GalleryIndex(b[live]), b_ids[live]
            out = {}

            def plain():
                out["w"] = mutual_ranks(a, whole, a_ids, w_ids)

            def sharded():
                out["s"] = mutual_ranks_sharded(a, index, a_ids)

            times = alternate((("sharded", sharded), ("whole", plain)), args.reps, args.blocks, args.warmup)
            s, w = out["s"], out["w"]
            sel = slice(None) if live is None else live
            same = bool(torch.equal(s["ahead_AB"], w["ahead_AB"]) and torch.equal(s["ahead_BA"][sel], w["ahead_BA"])
                        and torch.equal(s["best_AB"], w["best_AB"]) and torch.equal(s["best_BA"][sel], w["best_BA"]))
            sizes = [shard.N for shard in index.shards]
            print(json.dumps({**base, "shape": name, "nA": nA, "nB": nB, "E": E, "shard_rows": shard_rows, "shards": len(sizes),
                              "removed_rows": int(gone.numel()) if removed else 0, "launches_sharded": 2 * len(sizes), "launches_whole": 2,
                              "slabs_whole": ops.search_slabs(nA, whole.N, 1), "slabs_per_shard": sorted({ops.search_slabs(nA, n, 1) for n in sizes}),
                              "partial_last_tiles": sum(1 for n in sizes if n % 128), **report(times, "sharded", "whole"), "equal_vectors": same}),
                  flush=True)
            del index, whole, out
        del a, b, whole_all
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
