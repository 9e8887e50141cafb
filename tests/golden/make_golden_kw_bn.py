#!/usr/bin/env python3
"""Generates tests/golden/kw_bn_fixed.npz from the reference's fixed-count keyword BatchNorm
(avssl/module/speechclip_c_modules/kw_bn.py, a leaf file that imports only torch; loaded by path, nothing of it is copied):

    python tests/golden/make_golden_kw_bn.py <reference checkout>

B = 5, K = 8, E = 16, float64.  Per kind (``eachKw`` with ``parallel: true``; ``same``): the parameters after initialisation from
init_bias / init_scale / std_scale plus a seeded perturbation (so that a wrong parameter layout shows), two train steps on x1, x2
(output, input and parameter gradients of step 1 for ``dy``; the running buffers and num_batches_tracked after step 2), then the
eval-mode output on x2.  The inputs are float32 values; the reference runs in float64 and its results are stored rounded to float32
(2^-24 relative), which keeps the file small.  Data only."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
B, K, E = 5, 8, 16


def main(ref: str) -> None:
    spec = importlib.util.spec_from_file_location("ref_kw_bn", os.path.join(ref, "avssl/module/speechclip_c_modules/kw_bn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.set_default_dtype(torch.float64)
    g = torch.Generator().manual_seed(20260)
    r = lambda *s: torch.randn(*s, generator=g).float().double()
    out = {"init_bias": r(E), "init_scale": r(E).abs() + 0.5, "std_scale": np.float64(1.5),
           "x1": (r(B, K, E) * 2 + 1).float().double(), "x2": (r(B, K, E) - 0.5).float().double(), "dy": r(B, K, E)}
    for kind, parallel in (("eachKw", True), ("same", False)):
        m = mod.Kw_BatchNorm(kw_num=K, kw_dim=E, batchnorm_type=kind, init_bias=out["init_bias"], init_scale=out["init_scale"],
                             std_scale=1.5, learnable=True, parallel=parallel).double()
        bn = m.bn_layer
        reps = K if kind == "eachKw" else 1                   # the initialisation is a rule (init_scale * std_scale, init_bias, repeated
        assert torch.equal(bn.weight.detach(), (out["init_scale"] * 1.5).repeat(reps))        # per slot): checked here, not stored
        assert torch.equal(bn.bias.detach(), out["init_bias"].repeat(reps))
        with torch.no_grad():
            bn.weight.copy_((bn.weight + 0.1 * r(bn.weight.numel())).float().double())
            bn.bias.copy_((bn.bias + 0.1 * r(bn.bias.numel())).float().double())
        out[f"{kind}.weight"], out[f"{kind}.bias"] = bn.weight.detach().clone(), bn.bias.detach().clone()
        m.train()
        x1 = out["x1"].clone().requires_grad_(True)
        y1 = m(x1)
        y1.backward(out["dy"])
        out[f"{kind}.y1"], out[f"{kind}.dx1"] = y1.detach(), x1.grad.clone()
        out[f"{kind}.dweight"], out[f"{kind}.dbias"] = bn.weight.grad.clone(), bn.bias.grad.clone()
        m(out["x2"].clone())
        out[f"{kind}.running_mean"], out[f"{kind}.running_var"] = bn.running_mean.clone(), bn.running_var.clone()
        out[f"{kind}.num_batches_tracked"] = bn.num_batches_tracked.clone()
        m.eval()
        out[f"{kind}.y_eval"] = m(out["x2"].clone()).detach()
    arrs = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    arrs = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in arrs.items()}
    dst = os.path.join(HERE, "kw_bn_fixed.npz")
    np.savez_compressed(dst, **arrs)
    print(dst, len(arrs), "arrays", os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
