"""Helpers of tests/test_gpu_sigmoid_loss.py and tests/test_sigmoid_loss_cases_cpu.py (not collected on their own): the cases of the
pairwise sigmoid loss (SigmoidContrastiveLoss on sc_sigmoid_loss_fwd / sc_sigmoid_loss_grad, csrc/sigmoid_loss.hip), their fp64
reference - the formulas, no autograd - and the bounds.  Nothing here needs a GPU.

    s_ij = <A_i, B_j>,  x_ij = t s_ij + b,  z_ij = +1 if i == j else -1,  same_ij = ids and i != j and ids[i] == ids[j]
    "ignore": w_ij = 0 where same_ij;  "positive": z_ij = +1 where same_ij;  "negative": nothing changes
    loss = (1 / B) sum_ij w_ij softplus(-z_ij x_ij),   g_ij = d loss / d x_ij = -(1 / B) w_ij z_ij sigmoid(-z_ij x_ij)
    dA = t g B,  dB = t g^T A,  d t = sum_ij g_ij s_ij,  d b = sum_ij g_ij

Bounds are the project's own (tests/loss_cases.py), carried over: TOL_LOGITS was set at the multiplier 1 / 0.07 and a product's error is
linear in the multiplier, so the scores get TOL_X(t) = TOL_LOGITS max(1, 0.07 t); the loss gets the score error through a 1-Lipschitz
term, TOL_X(t) sum_ij |g64_ij|, plus the project's loss tolerance, relative above 1; gradients TOL_GRAD of their largest entry; d t and
d b TOL_GRAD of the sum of their absolute summands."""
import functools

import torch

import loss_cases as lc

TOL_LOGITS, TOL_LOSS, TOL_GRAD = lc.TOL_LOGITS, lc.TOL_LOSS, lc.TOL_GRAD
MODES = ("ignore", "positive", "negative")

# (B, E): one pair; tiny, one id group of five; exactly one tile and one K-tile; one row and column into the next tile with a K tail of
# 4; 3 x 3 tiles with ragged edges (ids_div5 puts the group 60 .. 64 across the tile boundary); ids_empty_tile's shape; the 8-GPU
# gathered batch, 64 tiles
SHAPES = [(1, 4), (5, 8), (64, 64), (65, 68), (130, 100), (200, 512), (512, 768)]
EMPTY_TILE_SHAPE, WIDE_SHAPE, SATURATED_SHAPE = (200, 512), (130, 100), (65, 68)

# name -> (t, b), t an fp32 value: the constructor's defaults; a trained state (everything that must see the id mask); x up to 137,
# where exp(x) overflows fp32 and only the stable forms stay finite
SETTINGS = {"default": (10.0, -10.0), "trained": (float(torch.tensor(1 / 0.07, dtype=torch.float32)), -5.0), "saturated": (100.0, 100.0)}


def _cases():
    out = []
    for shape in SHAPES:
        for setting in ("default", "trained"):
            out.append((shape, "none", "ignore", setting))
            out += [(shape, "div5", mode, setting) for mode in MODES]
    out += [(EMPTY_TILE_SHAPE, "empty_tile", "ignore", setting) for setting in ("default", "trained")]
    out += [(WIDE_SHAPE, "wide", mode, "trained") for mode in MODES]
    out += [(SATURATED_SHAPE, "none", "ignore", "saturated"), (SATURATED_SHAPE, "div5", "ignore", "saturated")]
    return out


CASES = _cases()


def case_id(case):
    (B, E), idset, mode, setting = case
    return f"{B}x{E}-{idset}-{mode}-{setting}"


@functools.lru_cache(maxsize=None)
def inputs(shape):
    return lc.make_pair(*shape, seed=sum(shape))


def make_ids(idset, B):
    if idset == "none":
        return None
    return {"div5": lc.ids_div5, "empty_tile": lc.ids_empty_tile, "wide": lc.wide_ids}[idset](B)


def tol_x(t):
    return TOL_LOGITS * max(1.0, 0.07 * t)


def pair_tables(B, ids, same_id):
    """-> (z [B, B] of +-1, w [B, B] of 0 / 1, same [B, B] bool) as the formulas above define them"""
    assert same_id in MODES
    eye = torch.eye(B, dtype=torch.bool)
    same = (ids[:, None] == ids[None, :]) & ~eye if ids is not None else torch.zeros(B, B, dtype=torch.bool)
    z = torch.where(eye | (same if same_id == "positive" else torch.zeros_like(same)), 1.0, -1.0).double()
    w = torch.where(same, 0.0, 1.0).double() if same_id == "ignore" else torch.ones(B, B, dtype=torch.float64)
    return z, w, same


def softplus(u):
    return u.clamp(min=0) + torch.log1p(torch.exp(-u.abs()))


def sigmoid(v):
    e = torch.exp(-v.abs())
    return torch.where(v >= 0, torch.ones_like(e), e) / (1 + e)


def reference(A, Bm, ids, t, b, same_id="ignore", dtype=torch.float64):
    """The formulas in ``dtype`` on ``dtype`` copies of the fp32 inputs, no autograd.
    -> dict(loss, s, x, g, dA, dB, dt, db, counts [3] int64 = positives, negatives, ignored).  In fp32 it is the plain stable evaluation
    that shows what the arithmetic of the format gives."""
    B = A.shape[0]
    a, bm = A.detach().to(dtype), Bm.detach().to(dtype)
    z, w, _ = pair_tables(B, ids, same_id)
    zd, wd = z.to(dtype), w.to(dtype)
    s = a @ bm.t()
    x = t * s + b
    u = -zd * x
    loss = (wd * softplus(u)).sum() / B
    g = -(1.0 / B) * wd * zd * sigmoid(u)
    counts = torch.stack([((w > 0) & (z > 0)).sum(), ((w > 0) & (z < 0)).sum(), (w == 0).sum()])
    return {"loss": loss, "s": s, "x": x, "g": g, "dA": t * (g @ bm), "dB": t * (g.t() @ a), "dt": (g * s).sum(), "db": g.sum(),
            "counts": counts}


def bounds(ref, t):
    """The bound of every quantity for the fp64 reference ``ref`` at scale ``t``"""
    g, s = ref["g"].double(), ref["s"].double()
    loss = float(ref["loss"])
    return {"x": tol_x(t), "loss": tol_x(t) * float(g.abs().sum()) + TOL_LOSS * max(1.0, loss), "g": TOL_GRAD * float(g.abs().max()),
            "dA": TOL_GRAD, "dB": TOL_GRAD, "dt": TOL_GRAD * float((g * s).abs().sum()), "db": TOL_GRAD * float(g.abs().sum())}


def errors(got, ref):
    """The error of every quantity of ``got`` (whichever of loss, x, g, dA, dB, dt, db it holds) against the fp64 reference"""
    out = {}
    for k in ("loss", "dt", "db"):
        if k in got:
            out[k] = abs(float(got[k]) - float(ref[k]))
    for k in ("x", "g"):
        if k in got:
            out[k] = lc.max_abs_err(got[k], ref[k])
    for k in ("dA", "dB"):
        if k in got:
            out[k] = lc.scale_rel_err(got[k], ref[k])
    return out
