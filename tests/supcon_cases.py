"""Helpers of tests/test_gpu_supcon.py and the CPU tests of SupConLoss (not collected on their own): seeded inputs and an fp64 reference
of the supervised contrastive loss (csrc/supcon.hip under losses.SupConLoss), written from the formulas of
include/speechclip_hip.h - no autograd, no reference code.  Nothing here needs a GPU; tests/test_supcon_cases_cpu.py checks this
reference against the fixtures the reference implementation produced (tests/golden/supcon.npz)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from loss_cases import TOL_GRAD, TOL_LOGITS, TOL_LOSS, TOL_LSE, scale_rel_err, wide_ids  # noqa: F401  (the bounds and builders the tests share)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "supcon.npz")

# (bsz, V, E) of the sweep against fp64 - the smallest shapes at which a tile, tail or index rule can go wrong
SHAPES = [(1, 2, 4),        # one non-self column: loss and every gradient are 0
          (2, 2, 20),       # two samples
          (32, 2, 64),      # N = 64: exactly one tile
          (33, 2, 68),      # N = 66, E a multiple of 4 but not of 64
          (65, 2, 768),     # N = 130
          (100, 3, 64),     # V = 3; "one" gives a 100 x 300 rectangle
          (64, 1, 64),      # V = 1: only with labels (without them no anchor has a positive)
          (512, 2, 100)]    # N = 1024, the 8-GPU gathered batch
BASE_TEMPERATURES = (0.07, 1.0)
MODES = ("all", "one")

# the fixtures of tests/golden/supcon.npz: name -> (bsz, V, E, labelling, mode, T, base_temperature, learnable)
#   labelling: "div5" labels = arange // 5, "none" neither labels nor mask, "mask" a random asymmetric float mask, "single" labels = arange
#   (V = 1: no anchor has a positive -> NaN), "zero_row" a mask whose row 2 is zero (-> NaN)
GOLDEN_CASES = {
    "div5_all": (33, 2, 68, "div5", "all", 0.07, 0.07, True),
    "div5_one": (33, 2, 68, "div5", "one", 0.07, 0.07, True),
    "nolabels_all": (33, 2, 68, "none", "all", 0.07, 0.07, True),
    "v3_div5_all": (100, 3, 64, "div5", "all", 0.07, 0.07, True),
    "mask_all": (6, 2, 8, "mask", "all", 0.1, 0.2, True),
    "fixedT_div5_all": (33, 2, 68, "div5", "all", 0.07, 0.07, False),
    "nan_singleton_v1": (8, 1, 8, "single", "all", 0.07, 0.07, True),
    "nan_zero_mask_row": (6, 2, 8, "zero_row", "all", 0.07, 0.07, True),
}
NAN_CASES = ("nan_singleton_v1", "nan_zero_mask_row")


def make_features(bsz, V, E, seed):
    """Unit-normalised views [bsz, V, E] with a shared component per sample (loss_cases.make_pair's correlation, for V views)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(bsz, 1, E, generator=g)
    return F.normalize(torch.randn(bsz, V, E, generator=g) + 0.5 * base, dim=-1)


def labels_div5(bsz):
    return torch.arange(bsz) // 5


def random_mask(bsz, seed, zero_row=None):
    """An asymmetric float mask [bsz, bsz] with weights in (0, 2) and some zeros; ``zero_row``: that row is all zero."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(bsz, bsz, generator=g) * 2 * (torch.rand(bsz, bsz, generator=g) < 0.6)
    m = m + 0.5 * torch.eye(bsz)                     # every anchor keeps its own sample's other view
    if zero_row is not None:
        m[zero_row] = 0.0
    return m.float()


def golden_inputs(name):
    """-> (features, labels, mask) of fixture ``name``, as tests/golden/make_golden_supcon.py builds them."""
    bsz, V, E, labelling = GOLDEN_CASES[name][:4]
    seed = 100 + sorted(GOLDEN_CASES).index(name)
    f = make_features(bsz, V, E, seed)
    if labelling == "div5":
        return f, labels_div5(bsz), None
    if labelling == "single":
        return f, torch.arange(bsz), None
    if labelling == "mask":
        return f, None, random_mask(bsz, seed + 1)
    if labelling == "zero_row":
        return f, None, random_mask(bsz, seed + 1, zero_row=2)
    return f, None, None


def pair_weights(bsz, labels=None, mask=None):
    """M [bsz, bsz] fp64: the identity, [labels_a == labels_b], or the mask as given."""
    if labels is not None:
        labels = labels.reshape(-1)
        return (labels[:, None] == labels[None, :]).double()
    if mask is not None:
        return mask.double()
    return torch.eye(bsz, dtype=torch.float64)


def reference(features, labels=None, mask=None, T=0.07, base_temperature=0.07, mode="all", dtype=torch.float64):
    """The loss and its gradients from the formulas, in ``dtype``.  ``T``: the temperature as a python float - hand it the module's own
    fp32 parameter value (float32(0.07) is not 0.07).  -> dict(loss, logits [Na, N], lse [Na], possum, poscnt, dfeatures (the shape of
    ``features``), dT, abs_gl = sum_ij |g_ij l_ij| / T (the sum of the absolute summands of dT))."""
    bsz, V = features.shape[:2]
    f = features.detach().cpu().to(dtype).reshape(bsz, V, -1)
    E = f.shape[2]
    C = torch.cat(torch.unbind(f, 1), 0)                             # row r = f[r % bsz, r // bsz]
    N = V * bsz
    Na = {"all": N, "one": bsz}[mode]
    l = C[:Na] @ C.t() / T
    keep = torch.ones(Na, N, dtype=dtype)
    keep[torch.arange(Na), torch.arange(Na)] = 0.0
    w = pair_weights(bsz, labels, mask).to(dtype).repeat(Na // bsz, V) * keep
    mx = torch.where(keep > 0, l, torch.full_like(l, -float("inf"))).max(1).values
    lse = mx + torch.log((keep * torch.exp(l - mx[:, None])).sum(1))
    s = w.sum(1)
    possum = (w * l).sum(1)
    loss = -(1.0 / base_temperature) * ((w * (l - lse[:, None])).sum(1) / s).mean()
    p = keep * torch.exp(l - lse[:, None])
    g = -(1.0 / (base_temperature * Na)) * (w / s[:, None] - p)
    dC = g.t() @ C[:Na] / T
    dC[:Na] += g @ C / T
    return {"loss": loss, "logits": l, "lse": lse, "possum": possum, "poscnt": s,
            "dfeatures": dC.view(V, bsz, E).transpose(0, 1).reshape(features.shape), "dT": -(g * l).sum() / T,
            "abs_gl": (g * l).abs().sum() / T}


def load_golden():
    return np.load(GOLDEN)
