#!/usr/bin/env python3
"""Keyword detokenisation at epoch size: keyword_neighbors (split bf16 score GEMM + sc_topk_rows_f32 + fp64 rescoring of the K picks),
ops.topk_rows alone, and the reference's formulation on the same GPU - normalise, matmul and torch.topk in fp32, chunked to the same
score scratch (what already runs on the parent commit: the baseline).

Shapes (rows, V, E, K): (40 000, 8 112, 512, 10) a Flickr8k validation epoch, (40 000, 19 787, 768, 10) COCO's reduced vocabulary,
(8 192, 49 408, 512, 10) the full CLIP vocabulary.  One JSON line per shape.

Method: every variant is warmed up, then the variants alternate for ``--rounds`` rounds in ONE process; a round times ``--iters`` calls
between two device events; reported: median and min over the rounds.  topk_rows alone runs on one chunk of scores (what it meets
inside keyword_neighbors: a chunk that fits the Infinity Cache) and, separately, on a matrix larger than the cache (HBM-bound);
its rate is the bytes of the scores it reads over its time, against the 6.29 TB/s measured copy bandwidth.  The device's current
sclk / mclk as torch reports them are printed with every line (not pinned: shared machine)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from speechclip_plus_amd import ops  # noqa: E402
from speechclip_plus_amd.keyword_neighbors import SCORE_SCRATCH_BYTES, default_chunk_rows, keyword_neighbors  # noqa: E402

COPY_BW = 6.29e12          # measured float4-copy bandwidth of the device, bytes / s of total traffic (79 % of the 8 TB/s HBM3E peak)
SHAPES = ((40000, 8112, 512, 10), (40000, 19787, 768, 10), (8192, 49408, 512, 10))


def torch_reference(kw, table_n, K, chunk):
    """The reference's maths on the device: F.normalize + matmul + torch.topk in fp32, chunked to the same scratch."""
    vals, idx = [], []
    for r0 in range(0, kw.shape[0], chunk):
        s = torch.nn.functional.normalize(kw[r0: r0 + chunk], dim=-1, eps=1e-8) @ table_n.t()
        v, i = torch.topk(s, K)
        vals.append(v)
        idx.append(i)
    return torch.cat(vals), torch.cat(idx)


def clocks():
    try:
        return {"sclk_mhz": torch.cuda.clock_rate(), "mclk_mhz": torch.cuda.memory_clock_rate() if hasattr(torch.cuda, "memory_clock_rate") else None}
    except Exception as e:       # noqa: BLE001 - clocks are a note, not a result
        return {"clocks": f"unavailable ({type(e).__name__})"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="*", default=[0, 1, 2])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: there is no CPU timing"
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda:0")
    for si in args.shapes:
        rows, V, E, K = SHAPES[si]
        g = torch.Generator(device=dev).manual_seed(si)
        table = 0.01 * torch.randn(V, E, device=dev, generator=g)
        kw = 0.01 * torch.randn(rows, E, device=dev, generator=g)
        kw[::2] = table[torch.randint(0, V, (rows - rows // 2,), device=dev, generator=g)]        # half quantised keywords
        table_n = torch.nn.functional.normalize(table, dim=-1, eps=1e-8)
        chunk = default_chunk_rows(V)
        Vp = (V + 127) // 128 * 128
        one_chunk = torch.randn(chunk, Vp, device=dev, generator=g)
        big_rows = max(chunk, (1 << 30) // (4 * Vp))                                              # 1 GiB of scores: past the 256 MiB cache
        big = torch.randn(big_rows, Vp, device=dev, generator=g)
        cache = {}
        variants = {
            "hip_keyword_neighbors": lambda: keyword_neighbors(kw, table, K, tables=cache),
            "torch_fp32_reference": lambda: torch_reference(kw, table_n, K, chunk),
            "topk_rows_one_chunk": lambda: ops.topk_rows(one_chunk, V, K),
            "topk_rows_1gib": lambda: ops.topk_rows(big, V, K),
        }
        times = {n: [] for n in variants}
        for fn in variants.values():                                                              # warm-up: code objects, table caches
            fn()
            fn()
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
        # same answers: share of rows whose index lists are identical, largest value difference (two fp32 score matrices: near-ties differ)
        hv, hi = keyword_neighbors(kw, table, K, tables=cache)
        tv, ti = torch_reference(kw, table_n, K, chunk)
        agree = float((hi.view(rows, K) == ti).all(1).float().mean())
        med = {n: statistics.median(t) for n, t in times.items()}
        out = {"shape": {"rows": rows, "V": V, "E": E, "K": K}, "chunk_rows": chunk, "score_scratch_mib": SCORE_SCRATCH_BYTES >> 20,
               "ms_median": {n: round(m, 4) for n, m in med.items()}, "ms_min": {n: round(min(t), 4) for n, t in times.items()},
               "hip_over_torch": round(med["hip_keyword_neighbors"] / med["torch_fp32_reference"], 4),
               "rows_with_identical_index_lists": round(agree, 5),
               "max_abs_value_diff": float((hv.view(rows, K) - tv).abs().max()),
               "topk_rows_one_chunk_tb_s": round(chunk * V * 4 / (med["topk_rows_one_chunk"] * 1e-3) / 1e12, 3),
               "topk_rows_1gib_tb_s": round(big_rows * V * 4 / (med["topk_rows_1gib"] * 1e-3) / 1e12, 3),
               "topk_rows_1gib_fraction_of_copy_bw": round(big_rows * V * 4 / (med["topk_rows_1gib"] * 1e-3) / COPY_BW, 3),
               "rounds": args.rounds, "iters": args.iters, **clocks()}
        print(json.dumps(out), flush=True)
        del big, one_chunk


if __name__ == "__main__":
    main()
