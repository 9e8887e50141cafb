"""Generate tests/golden/supcon.npz from the reference implementation of SupConLoss.

    python tests/golden/make_golden_supcon.py <root of the reference checkout>

Runs only where the reference is at hand.  It imports the reference's leaf file avssl/module/losses.py by path (its package's __init__
pulls in far more), runs SupConLoss on the inputs tests/supcon_cases.py builds - in fp32 as it stands, and in fp64 (module and inputs
converted; a learnable temperature keeps its fp32 parameter VALUE) - and stores inputs and results.  No reference source is copied: the
.npz holds data only.  Per case ``name`` of supcon_cases.GOLDEN_CASES:
    name/features [bsz, V, E] f32, name/labels int64 or name/mask f32 (where the case has one), name/T (the temperature the module used:
    its fp32 parameter value, or the python float), name/loss32, name/dfeatures32, name/dtemperature32, name/loss64, name/dfeatures64,
    name/dtemperature64 (the temperature gradients only with a learnable temperature)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.abspath(os.path.join(HERE, "..")), os.path.abspath(os.path.join(HERE, "..", ".."))]   # tests/ and the repository root

import supcon_cases as sc  # noqa: E402


def load_reference(root):
    spec = importlib.util.spec_from_file_location("ref_losses", os.path.join(root, "avssl", "module", "losses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, name, dtype):
    bsz, V, E, _, mode, T, base_temperature, learnable = sc.GOLDEN_CASES[name]
    features, labels, mask = sc.golden_inputs(name)
    crit = ref.SupConLoss(temperature=T, contrast_mode=mode, base_temperature=base_temperature, learnable_temperature=learnable)
    if dtype == torch.float64:
        crit = crit.double()
    f = features.to(dtype).clone().requires_grad_(True)
    loss = crit(f, labels=labels, mask=mask)
    loss.backward()
    out = {"loss": loss.detach().numpy(), "dfeatures": f.grad.numpy()}
    if learnable:
        out["dtemperature"] = crit.temperature.grad.numpy()
        out["T"] = crit.temperature.detach().double().numpy()
    else:
        out["T"] = np.float64(T)
    return out, features, labels, mask


def main(root):
    ref = load_reference(root)
    store = {}
    for name in sc.GOLDEN_CASES:
        r32, features, labels, mask = run(ref, name, torch.float32)
        r64 = run(ref, name, torch.float64)[0]
        store[f"{name}/features"] = features.numpy()
        if labels is not None:
            store[f"{name}/labels"] = labels.numpy().astype(np.int64)
        if mask is not None:
            store[f"{name}/mask"] = mask.numpy()
        store[f"{name}/T"] = r64["T"]
        for tag, r in (("32", r32), ("64", r64)):
            for k in ("loss", "dfeatures", "dtemperature"):
                if k in r:
                    store[f"{name}/{k}{tag}"] = r[k]
        print(name, "loss32", float(r32["loss"]), "loss64", float(r64["loss"]))
    path = os.path.join(HERE, "supcon.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
