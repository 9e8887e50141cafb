"""Frozen eval forward of wavlm_base against hubert_base in one process, alternating (64 x 10 s and a ragged U{2..10 s} batch), and
the per-launch time of the plain and the biased attention instances and of the gate kernel at the 64 x 10 s geometry.  Prints
TIME| lines and writes --out (json).  Usage: python tools/bench_wavlm.py [--out wavlm_time.json]"""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "wavlm_time.json"
from speechclip_plus_amd import ops
from speechclip_plus_amd.speech_encoder import FairseqSpeechEncoder_Hubert, S3prlSpeechEncoderPlus

def timed(fn, n=8, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts))

res = {}
hub = FairseqSpeechEncoder_Hubert(name="hubert_base", device="cuda", feat_select_idx="weighted_sum").eval()
wav = S3prlSpeechEncoderPlus("wavlm_base", device="cuda", feat_select_idx="weighted_sum").eval()
rng = np.random.RandomState(0)
for tag, lens in (("64x10s", [160000] * 64), ("ragged U{2..10s}", [int(rng.randint(32000, 160001)) for _ in range(64)])):
    x = torch.randn(64, 160000, device="cuda")
    wl = torch.tensor(lens)
    with torch.no_grad():
        out = {}
        for rep in range(2):                       # alternating
            for name, enc in (("hubert_base", hub), ("wavlm_base", wav)):
                out.setdefault(name, []).append(timed(lambda: enc(x, wl)))
    res[tag] = {k: [round(m, 3) for m, _ in v] for k, v in out.items()}
    print("TIME|forward", tag, res[tag], flush=True)
# per-launch: the two attention instances at 64 x 10 s geometry (R = 504, H = 12) + the gate
B, R, H, D = 64, 504, 12, 768
qk = torch.randn(B * R + 64, 2 * D, device="cuda").to(torch.bfloat16)
vt = torch.randn(B * H * 64 * R + 64 * D, device="cuda").to(torch.bfloat16)
out = torch.zeros(B * R, D, device="cuda", dtype=torch.bfloat16)
valid = torch.full((B,), 499, dtype=torch.int32, device="cuda")
gate = 0.5 + 2 * torch.rand(H, B * R, device="cuda")
table = torch.randn(H, 2 * R - 1, device="cuda")
x = torch.randn(B * R, D, device="cuda").to(torch.bfloat16)
wg, bg, cst = torch.randn(8, 64, device="cuda") * 0.1, torch.zeros(8, device="cuda"), torch.ones(H, device="cuda")
per = {}
for rep in range(2):
    per.setdefault("attn plain", []).append(timed(lambda: ops.attn_fwd(qk, vt, valid, out, B, R, H, D, 0.125), n=20)[0])
    per.setdefault("attn relbias", []).append(timed(lambda: ops.attn_fwd(qk, vt, valid, out, B, R, H, D, 0.125, gate=gate, table=table), n=20)[0])
    per.setdefault("attn plain drop", []).append(timed(lambda: ops.attn_fwd(qk, vt, valid, out, B, R, H, D, 0.125, drop_p=0.1, drop_seed=1), n=20)[0])
    per.setdefault("attn relbias drop", []).append(timed(lambda: ops.attn_fwd(qk, vt, valid, out, B, R, H, D, 0.125, drop_p=0.1, drop_seed=1, gate=gate, table=table), n=20)[0])
    per.setdefault("gate", []).append(timed(lambda: ops.wavlm_gate(x, wg, bg, cst, H, out=gate), n=20)[0])
res["per_launch_ms"] = {k: [round(v, 4) for v in vs] for k, vs in per.items()}
print("TIME|per launch ms", res["per_launch_ms"], flush=True)
json.dump(res, open(OUT, "w"), indent=1)
