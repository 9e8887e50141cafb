#!/usr/bin/env python3
"""Caption embeddings at retrieval-set size: ClipModel.encode_text with length-following batching (``bucket=True``: every caption at
the segment class of its own prefix, 32 / 64 / 128 rows) against the same call with ``bucket=False`` (the whole set at the class of
its longest caption).

Captions: ``--captions`` (5000) synthetic ones drawn with a fixed seed.  Lengths: the number of sub-words between <|startoftext|> and
<|endoftext|> is round(lognormal(mu = ln 12, sigma = 0.45)) clipped to [1, 75] - a stand-in for image captions (median 12 sub-words,
~1.5 % longer than 30, a handful past 62); the real distribution of Flickr8k's captions has not been measured here.  The JSON line
carries the histogram per segment class, so the numbers can be re-read against another distribution.  Tokens are uniform in the table.

Method: both variants are warmed up, then alternate for ``--rounds`` rounds in ONE process; a round times ``--iters`` calls between two
device events (host work of the call - bucketing, the small read of the end-of-text positions - included: it is part of the call);
reported: median and min over the rounds, and the largest difference between the two variants' embeddings.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speechclip_plus_amd.clip_text import EOT_TOKEN, SOT_TOKEN, ClipModel  # noqa: E402
from speechclip_plus_amd.clip_text_hip import TEXT_CHUNK_ROWS, text_buckets  # noqa: E402

LEN_MU, LEN_SIGMA = 12.0, 0.45


def synthetic_captions(n: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    words = torch.exp(torch.randn(n, generator=g) * LEN_SIGMA + torch.log(torch.tensor(LEN_MU))).round().clamp(1, 75).long()
    ids = torch.zeros(n, 77, dtype=torch.long)
    ids[:, 0] = SOT_TOKEN
    body = torch.randint(1, SOT_TOKEN, (n, 77), generator=g)
    t = torch.arange(77).unsqueeze(0)
    ids = torch.where((t >= 1) & (t <= words.unsqueeze(1)), body, ids)
    ids[torch.arange(n), words + 1] = EOT_TOKEN
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captions", type=int, default=5000)
    ap.add_argument("--name", default="ViT-B/32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: there is no CPU timing"
    clip = ClipModel(args.name, device="cuda:0").eval()
    ids = synthetic_captions(args.captions, args.seed)
    eot = ids.argmax(-1)
    ids_d = ids.cuda()
    variants = {"bucketed": lambda: clip.encode_text(ids_d, bucket=True), "unbucketed": lambda: clip.encode_text(ids_d, bucket=False)}
    times = {n: [] for n in variants}
    outs = {}
    for n, fn in variants.items():                               # warm-up: code objects, weight conversion, allocator
        fn()
        outs[n] = fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / args.iters)
    med = {n: statistics.median(t) for n, t in times.items()}
    diff = (outs["bucketed"] - outs["unbucketed"]).norm() / outs["unbucketed"].norm()
    buckets = text_buckets(eot.tolist())
    print(json.dumps({
        "tower": args.name, "captions": args.captions, "seed": args.seed,
        "length_distribution": f"sub-words = round(lognormal(ln {LEN_MU:g}, {LEN_SIGMA:g})) clipped to [1, 75]; prefix = sub-words + 2",
        "prefix_median": int((eot + 1).median()), "prefix_max": int((eot + 1).max()),
        "classes": [{"SEG": s, "n_pos": p, "captions": len(i)} for s, p, i in buckets],
        "rows_bucketed": sum(s * len(i) for s, _, i in buckets), "rows_unbucketed": max(s for s, _, _ in buckets) * args.captions,
        "chunk_rows": TEXT_CHUNK_ROWS,
        "ms_median": {n: round(m, 3) for n, m in med.items()}, "ms_min": {n: round(min(t), 3) for n, t in times.items()},
        "unbucketed_over_bucketed": round(med["unbucketed"] / med["bucketed"], 3),
        "captions_per_s_bucketed": round(args.captions / (med["bucketed"] * 1e-3)),
        "rel_l2_between_variants": float(diff), "rounds": args.rounds, "iters": args.iters}), flush=True)


if __name__ == "__main__":
    main()
