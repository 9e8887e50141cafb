#!/usr/bin/env python3
"""Wide search (k > 32, csrc/topk_wide.hip) against what torch offers, on tools/bench_cascaded.py's protocol: ONE process, the two sides
alternating in blocks after a warm-up at every switch (and alternating who goes first), device events around every block, ms per call,
the median of five blocks.  One JSON line per run with the median and every block of each side and the spread of the blocks.

    selection   ONE score matrix built by ops.cosine_scores_split (as many query rows as the composition route's 128 MiB scratch
                holds: what ``search`` selects from per chunk), then
                    (w) ops.topk_rows_wide(scores, N, k)                 the order contract, optionally the filter
                    (t) torch.topk(scores[:, :N], k, sorted=True)        no tie order, no filter
                on the same resident matrix
    search      whole calls over all nQ queries:
                    (w) search(queries, GalleryIndex, k)                 (filtered run: with query_ids / gallery_ids / live)
                    (t) torch.matmul on the fp32 rows (+ masked_fill from the same ids and mask) + torch.topk

Runs: 25 000 x 5 000 x 768 at k = 100 and at k = 1024, 1 024 x 131 072 x 512 at k = 256, and the first shape at k = 100 with the
corpora's filter (five gallery rows per id, 1 % removed rows).  The index is built once, outside the clock.  Unit Gaussian rows.

    python tools/bench_search_wide.py --reps 10 --sel-reps 100 --blocks 5
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

RUNS = (("SpokenCOCO test, k=100", 25000, 5000, 768, 100, False), ("large gallery, k=256", 1024, 131072, 512, 256, False),
        ("SpokenCOCO test, k=1024", 25000, 5000, 768, 1024, False), ("SpokenCOCO test, k=100, filtered", 25000, 5000, 768, 100, True))


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


def report(times):
    rec = {}
    for n, t in times.items():
        rec[n + "_ms"] = [round(v, 4) for v in t]
        rec[n + "_ms_median"] = round(statistics.median(t), 4)
        rec[n + "_spread_ms"] = round(max(t) - min(t), 4)
    w, t = statistics.median(times["wide"]), statistics.median(times["torch"])
    spread = max(rec["wide_spread_ms"], rec["torch_spread_ms"])
    rec["wide_over_torch"] = round(w / t, 3)
    rec["wide_no_slower_than_torch_within_spread"] = w <= t + spread
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="whole search calls per timed block")
    ap.add_argument("--sel-reps", type=int, default=100, help="selection launches per timed block (a launch takes a fraction of a ms)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls after every switch of sides")
    ap.add_argument("--runs", type=str, default="0,1,2,3")
    ap.add_argument("--quantise", type=float, default=0.0, help="selection only: round the scores to multiples of 1 / QUANTISE first (tie-heavy "
                    "rows: the column-ordered admission; torch.topk's lists then differ, it has no tie order)")
    ap.add_argument("--custom", type=str, default="", help="further runs as nQ,N,E,k;nQ,N,E,k;... (instead of --runs)")
    args = ap.parse_args()
    from speechclip_plus_amd import GalleryIndex, ops, search
    from speechclip_plus_amd.keyword_neighbors import default_chunk_rows
    dev = torch.device("cuda:0")
    runs = [RUNS[int(s)] for s in args.runs.split(",")]
    if args.custom:
        runs = [("custom",) + tuple(int(v) for v in c.split(",")) + (False,) for c in args.custom.split(";")]
    for name, nQ, N, E, k, filtered in runs:
        q, gal = unit_rows_randn(nQ, E, dev, 1), unit_rows_randn(N, E, dev, 2)
        index = GalleryIndex(gal)
        g_ids = q_ids = live = None
        if filtered:
            g_ids = torch.arange(N, device=dev, dtype=torch.int64) // 5                  # five rows per id
            q_ids = (torch.arange(nQ, device=dev, dtype=torch.int64) * 7919) % (-(-N // 5))
            live = torch.rand(N, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) >= 0.01
        base = {"run": name, "nQ": nQ, "N": N, "E": E, "k": k, "filtered": filtered, "device": torch.cuda.get_device_name(0),
                "clock": "device events around blocks of --reps calls, ms per call", "reps_per_block": args.reps, "blocks": args.blocks,
                "warmup_after_every_switch": args.warmup, "selection_scores_quantised_to": args.quantise or None}
        out = {}

        # ---- the selection alone, on one resident score matrix
        rows = min(default_chunk_rows(N), -(-nQ // 128) * 128)
        Np = index.split.shape[0]
        scores = torch.empty(rows, Np, device=dev, dtype=torch.float32)
        ops.cosine_scores_split(q[:rows], None, index.split, Np, out=scores[: -(-min(rows, nQ) // 128) * 128])
        if args.quantise:                                             # a handful of distinct scores: the k-th boundary lies in a long tie run
            scores.mul_(args.quantise).round_().div_(args.quantise)
        R = min(rows, nQ)
        qi = None if q_ids is None else q_ids[:R]
        wv = torch.empty(R, k, device=dev, dtype=torch.float32)
        wi = torch.empty(R, k, device=dev, dtype=torch.int32)

        def sel_wide():
            ops.topk_rows_wide(scores[:R], N, k, q_ids=qi, g_ids=g_ids, live=live, vals=wv, idx=wi)

        def sel_torch():
            s = scores[:R, :N]
            if filtered:                                              # what the filter costs a torch user: a masked copy
                s = s.masked_fill((g_ids.unsqueeze(0) == qi.unsqueeze(1)) | ~live.unsqueeze(0), float("-inf"))
            out["t"] = torch.topk(s, k, dim=1, sorted=True)

        times = alternate((("wide", sel_wide), ("torch", sel_torch)), args.sel_reps, args.blocks, args.warmup)
        same = float((wi.long() == out["t"][1]).all(dim=1).float().mean())
        print(json.dumps({**base, "what": "selection", "reps_per_block": args.sel_reps, "rows": R, "score_matrix_MiB": round(R * Np * 4 / 2 ** 20, 1), **report(times),
                          "rows_with_equal_lists": same}), flush=True)
        del scores, wv, wi
        out.clear()
        torch.cuda.empty_cache()

        # ---- whole calls
        def all_wide():
            out["w"] = search(q, index, k, query_ids=q_ids, gallery_ids=g_ids, live=live)

        def all_torch():
            score = q @ gal.t()
            if filtered:
                score.masked_fill_((g_ids.unsqueeze(0) == q_ids.unsqueeze(1)) | ~live.unsqueeze(0), float("-inf"))
            out["t"] = torch.topk(score, k, dim=1, sorted=True)

        times = alternate((("wide", all_wide), ("torch", all_torch)), args.reps, args.blocks, args.warmup)
        same = float((out["w"][1] == out["t"][1]).all(dim=1).float().mean())
        print(json.dumps({**base, "what": "search", **report(times), "rows_with_equal_lists": same}), flush=True)
        del q, gal, index, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
