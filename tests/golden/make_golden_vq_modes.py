#!/usr/bin/env python3
"""Generate tests/golden/vq_modes.npz: the reference quantiser's other modes on the inputs of vq_v50.npz.

Runs ONLY where a checkout of the reference is (the tests need the .npz alone).  The reference's leaf file
avssl/module/speechclip_c_modules/my_vector_quantizer.py is imported by path, as make_golden.py does, and run on the CPU; the
.npz holds data only: x = 0.3 randn(3, 5, 50), emb = randn(50, 8), an upstream gradient gk, and per case the module's
``subword_prob``, the gradient to ``x`` and (learnable temperature) ``curr_temp.grad``.  The Gumbel modes draw from torch's RNG
and have no fixture: tests/test_vq_modes_cases_cpu.py checks the formula against F.gumbel_softmax on a given noise instead.

    python tests/golden/make_golden_vq_modes.py <reference checkout>
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def load_leaf(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref):
    vqm = load_leaf(ref, "avssl/module/speechclip_c_modules/my_vector_quantizer.py", "ref_vq")
    torch.manual_seed(32)
    V = 50
    x = torch.randn(3, 5, V) * 0.3
    emb = torch.randn(V, 8)
    gk = torch.randn(3, 5, 8)
    out = dict(x=x, emb=emb, gk=gk)

    def train_case(tag, temp, hard, finite_mask=False):
        vq = vqm.SimpleVectorQuantizer(temp=temp, time_first=True, use_gumbel=False, hard=hard).train()
        x0 = x.clone()
        if finite_mask:                      # the special columns at -1e4 instead of -inf: softmax gives exactly 0 there all the same
            x0[..., [0, 2, 3]] = -1e4
        xt = x0.requires_grad_(True)
        r = vq(x=xt * 1.0, prob_msk=[] if finite_mask else [0, 2, 3])
        ((r["subword_prob"] @ emb) * gk).sum().backward()
        out[tag + "_prob"], out[tag + "_gx"], out[tag + "_targets"] = r["subword_prob"], xt.grad, r["targets"]
        if isinstance(vq.curr_temp, torch.nn.Parameter):
            out[tag + "_gtemp"] = vq.curr_temp.grad

    train_case("soft_fixed", "fixed=0.1", False)
    # curr_temp.grad of the reference is NaN with the -inf mask: d (x / temp) / d temp = -x / temp^2 = inf meets a zero gradient.  The
    # *_fin cases run the same module on the same scores with the special columns at -1e4 (prob_msk = []): the same probabilities
    # (exactly 0 there), and the finite temperature gradient the masked formula stands for.
    train_case("hard_learn", "learnable=0.1", True)
    train_case("soft_learn", "learnable=0.1", False)
    train_case("hard_learn_fin", "learnable=0.1", True, finite_mask=True)
    train_case("soft_learn_fin", "learnable=0.1", False, finite_mask=True)
    vq = vqm.SimpleVectorQuantizer(temp="fixed=0.1", time_first=True, use_gumbel=False, hard=False).eval()
    r = vq(x=x.clone())
    out["ev_soft_prob"], out["ev_soft_targets"] = r["subword_prob"], r["targets"]
    np.savez_compressed(os.path.join(HERE, "vq_modes.npz"), **{k: np.asarray(v.detach().cpu().numpy()) for k, v in out.items()})
    print("wrote vq_modes.npz", len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
