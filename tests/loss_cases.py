"""Helpers of tests/test_gpu_loss_optim.py (not collected on their own): seeded inputs and fp64 references for the end of the train
step - MaskedContrastiveLoss on sc_infonce_fwd / sc_infonce_grad and the fused clip + Adam launch (csrc/loss_optim.hip).  Nothing
here needs a GPU; tests/test_loss_cases_cpu.py pins the builders' properties on the CPU."""
import math

import torch
import torch.nn.functional as F

from oracle.loss_ref import masked_contrastive_loss

TILE = 64                     # infonce_fwd_kernel: one workgroup per 64 x 64 tile of the logits, K-tiles of 64

# ---------------------------------------------------------------------------------------------------------------- loss
# (Bg, E) of the default-option sweep: every Bg with two E at least, every E at one ragged multi-tile Bg (65, 130, 200, 1000) at least
SHAPE_SWEEP = [(1, 4), (1, 768), (2, 20), (2, 100), (63, 20), (63, 768), (64, 64), (64, 68), (65, 4), (65, 768), (130, 20), (130, 68),
               (200, 64), (200, 100), (512, 20), (512, 100), (1000, 68), (1000, 768)]
RAGGED_MULTI_TILE = (65, 130, 200, 1000)

# the option sets of tests/golden/make_golden.py: make_loss_variants
VARIANTS = {"margin": dict(margin=0.3), "dcl": dict(dcl=True), "a2b": dict(b2a=False), "b2a": dict(a2b=False),
            "margin_dcl_trainT": dict(margin=0.2, dcl=True, trainable=True)}

# forward bounds of the project at temperature 0.07 (absolute, against fp64: test_infonce_fused_forward_vs_fp64, test_loss_golden)
# and the cap on a gradient's max |g - g64| / max |g64|
TOL_LOGITS, TOL_LSE, TOL_LOSS, TOL_GRAD = 2e-5, 5e-5, 2e-5, 2e-4

WIDE_ID_VALUES = [-1, -2, -65, 2 ** 32, 2 ** 32 + 1, 2 ** 40, 1]


def make_pair(Bg, E, seed):
    """Unit-normalised rows and a correlated partner (the inputs of test_infonce_fused_forward_vs_fp64)."""
    g = torch.Generator().manual_seed(seed)
    A = F.normalize(torch.randn(Bg, E, generator=g), dim=-1)
    Bm = F.normalize(torch.randn(Bg, E, generator=g) + 0.5 * A, dim=-1)
    return A, Bm


def ids_div5(Bg):
    return torch.arange(Bg) // 5


def ids_empty_tile(Bg=200):
    """Groups of 70 equal ids: with dcl, logit tile (0, 0) holds no negative for any of its rows or columns."""
    return torch.arange(Bg) // 70


def ids_empty_tile_permuted(Bg=200, seed=11):
    """The same groups scattered over the tiles."""
    return ids_empty_tile(Bg)[torch.randperm(Bg, generator=torch.Generator().manual_seed(seed))]


def wide_ids(Bg=130, seed=5):
    """ids that are negative or differ only above bit 31, with duplicates."""
    pick = torch.randint(0, len(WIDE_ID_VALUES), (Bg,), generator=torch.Generator().manual_seed(seed))
    return torch.tensor(WIDE_ID_VALUES, dtype=torch.int64)[pick]


def relabel(ids):
    """The same grouping with labels 0 .. k - 1."""
    return torch.unique(ids, return_inverse=True)[1].to(torch.int64)


def neg_mask(Bg, ids, dcl):
    """The negatives of avssl/module/losses.py:196-210, as oracle.loss_ref builds them."""
    eye = torch.eye(Bg, dtype=torch.bool)
    neg = (ids[:, None] != ids[None, :]) if ids is not None else ~eye
    return neg if dcl else (neg | eye)


def rows_without_negatives_per_tile(neg):
    """-> [(ti, tj, rows, cols)]: the 64 x 64 tiles in which some row (or column) of the tile has no negative inside the tile."""
    Bg = neg.shape[0]
    out = []
    for ti in range(0, Bg, TILE):
        for tj in range(0, Bg, TILE):
            t = neg[ti: ti + TILE, tj: tj + TILE]
            rows, cols = int((t.sum(1) == 0).sum()), int((t.sum(0) == 0).sum())
            if rows or cols:
                out.append((ti // TILE, tj // TILE, rows, cols))
    return out


def loss_reference(A, Bm, ids, temperature=0.07, margin=0.0, dcl=False, a2b=True, b2a=True, trainable=False, log_inv_temp=None,
                   scale=1.0, dtype=torch.float64):
    """oracle.loss_ref.masked_contrastive_loss on ``dtype`` copies of the fp32 inputs, with torch autograd in ``dtype``.
    -> dict(loss, dA, dB, [dT], logits, lse_row, lse_col).  ``trainable``: the temperature parameter is log(1 / T) (``log_inv_temp``
    = the module's own fp32 parameter value where given) and dT its gradient.  ``scale`` multiplies the loss before backward().
    The log-sum-exps are the oracle's own arithmetic (log of the masked sum of exp) on the oracle's logits."""
    Bg = A.shape[0]
    a = A.detach().to(dtype).requires_grad_(True)
    b = Bm.detach().to(dtype).requires_grad_(True)
    t = None
    if trainable:
        t0 = torch.tensor(math.log(1 / temperature), dtype=torch.float32) if log_inv_temp is None else log_inv_temp.detach().cpu().float()
        t = t0.to(dtype).reshape(()).requires_grad_(True)
        it = t.exp()
    else:
        it = 1.0 / temperature
    loss = masked_contrastive_loss(a, b, ids, it, margin, dcl, a2b, b2a)
    (scale * loss).backward()
    out = {"loss": loss.detach(), "dA": a.grad, "dB": b.grad}
    if trainable:
        out["dT"] = t.grad
    with torch.no_grad():
        logits = a @ b.t() * it
        if margin > 0.0:
            logits = logits - margin * torch.eye(Bg, dtype=dtype)
        e = logits.exp() * neg_mask(Bg, ids, dcl).to(dtype)
        out.update(logits=logits, lse_row=torch.log(e.sum(1)), lse_col=torch.log(e.sum(0)))
    return out


def max_abs_err(x, ref):
    return float((x.detach().double().cpu() - ref.double()).abs().max())


ZERO_GRAD = 1e-12             # an fp64 gradient below this is the rounding residue of one that is zero analytically


def scale_rel_err(x, ref):
    """max |x - ref| / max |ref|: an fp64 gradient has many entries near zero, where an element-wise rtol says nothing.  Where the
    reference is zero analytically (one row, or one group without dcl: the only negative is the positive itself) there is no scale:
    0 if ``x`` is exactly zero, inf otherwise."""
    ref, x = ref.double(), x.detach().double().cpu()
    if float(ref.abs().max()) < ZERO_GRAD:
        return 0.0 if float(x.abs().max()) == 0.0 else float("inf")
    return float((x - ref).abs().max() / ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------- optimiser
ADAM_SIZES = {1: (1,), 3: (1, 1, 1), 1023: (341, 341, 341), 21513: (7171, 7171, 7171), 600001: (200001, 199999, 200001),
              7600002: (3800001, 2400001, 1000001, 399999)}                     # total -> odd numels; 7.6 M = the parallel-base recipe's
ADAM_BETAS, ADAM_EPS, ADAM_LR, ADAM_FINAL_LR, ADAM_WARMUP, ADAM_MAX_STEP = (0.9, 0.98), 1e-6, 1e-3, 1e-5, 5, 30
# name -> (weight_decay, max_grad_norm, global gradient norm at 0-based step s; None: unit-variance gradients as drawn).  The norm is
# set, not left to the draw, so that the clip is on or off at every size alike - one element included
ADAM_HYPER = {
    "plain": (0.0, 0.0, None),
    "wd_clip4_alternating": (1e-2, 4.0, lambda s: 12.0 if s % 2 else 1.0),              # the clip is on at odd s (coefficient 1 / 3)
    # the coefficient is ~ 0.5, and the + 1e-6 in its denominator moves it by ~ 5e-4 relative
    "clip1e-3_tiny": (0.0, 1e-3, lambda s: 2e-3),
}
SUMSQ_BLOCKS, SUMSQ_THREADS, ADAM_MAX_BLOCKS = 1024, 256, 2048


def adam_params(total, seed):
    """fp32 parameter tensors of ADAM_SIZES[total]; tensor 0 starts in [-1e-3, 1e-3] (its update stays above its own ulp), the
    others at magnitude 1."""
    g = torch.Generator().manual_seed(seed)
    ps = []
    for i, n in enumerate(ADAM_SIZES[total]):
        ps.append((torch.rand(n, generator=g) * 2 - 1) * 1e-3 if i == 0 else torch.randn(n, generator=g))
    return ps


def adam_grads(total, hyper, step, seed):
    """The fp32 gradients of 0-based ``step``, scaled to the global norm that ADAM_HYPER[hyper] sets for it."""
    g = torch.Generator().manual_seed(seed * 1000003 + step)
    gs = [torch.randn(n, generator=g) for n in ADAM_SIZES[total]]
    norm = ADAM_HYPER[hyper][2]
    if norm is None:
        return gs
    k = norm(step) / math.sqrt(sum(float((x.double() ** 2).sum()) for x in gs))
    return [(x.double() * k).float() for x in gs]


def grad_norm64(gs):
    return math.sqrt(sum(float((x.double() ** 2).sum()) for x in gs))


def adam_lr(step):
    from speechclip_plus_amd.optim import linear_warmup_decay
    return ADAM_LR * linear_warmup_decay(step, ADAM_WARMUP, ADAM_MAX_STEP, ADAM_LR, ADAM_FINAL_LR)


class AdamRef64:
    """Plain fp64 restatement of clip_grad_norm_ + torch.optim.Adam (L2 decay folded into the gradient) with Python-double betas."""

    def __init__(self, params, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=0.0, max_grad_norm=0.0):
        self.p = [p.detach().double().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.betas, self.eps, self.wd, self.max_norm = betas, eps, weight_decay, max_grad_norm
        self.step_count = 0
        self.grad_norm = None                     # global norm of the last step's gradients, before the clip

    def step(self, grads, lr):
        self.step_count += 1
        t, (b1, b2) = self.step_count, self.betas
        g = [x.detach().double() for x in grads]
        self.grad_norm = math.sqrt(sum(float((x * x).sum()) for x in g))
        if self.max_norm > 0:
            coef = min(1.0, self.max_norm / (self.grad_norm + 1e-6))
            g = [x * coef for x in g]
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        for i, gi in enumerate(g):
            gi = gi + self.wd * self.p[i]
            self.m[i] = b1 * self.m[i] + (1.0 - b1) * gi
            self.v[i] = b2 * self.v[i] + (1.0 - b2) * gi * gi
            denom = self.v[i].sqrt() / math.sqrt(bc2) + self.eps
            self.p[i] = self.p[i] - (lr / bc1) * (self.m[i] / denom)


class TorchAdam:
    """clip_grad_norm_ + torch.optim.Adam on the CPU in the dtype of ``params``: in fp32 the yardstick of the device's error, in fp64
    the check of AdamRef64."""

    def __init__(self, params, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=0.0, max_grad_norm=0.0):
        self.params = [torch.nn.Parameter(p.detach().clone()) for p in params]
        self.opt = torch.optim.Adam(self.params, lr=ADAM_LR, betas=betas, eps=eps, weight_decay=weight_decay)
        self.max_norm = max_grad_norm

    def set_step_count(self, n):
        for p in self.params:
            st = self.opt.state[p]
            st["step"] = torch.full_like(st["step"], float(n)) if torch.is_tensor(st["step"]) else n

    def step(self, grads, lr):
        for p, g in zip(self.params, grads):
            p.grad = g.detach().to(p.dtype).clone()
        if self.max_norm > 0:
            torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
        for grp in self.opt.param_groups:
            grp["lr"] = lr
        self.opt.step()

    @property
    def p(self):
        return [p.detach() for p in self.params]

    @property
    def m(self):
        return [self.opt.state[p]["exp_avg"] for p in self.params]

    @property
    def v(self):
        return [self.opt.state[p]["exp_avg_sq"] for p in self.params]


def cat_err(xs, refs):
    """max |x - ref| / max |ref| over a list of tensors taken as one vector (0 / 0 = 0)."""
    num = max(float((x.detach().double().cpu().reshape(-1) - r.double().reshape(-1)).abs().max()) for x, r in zip(xs, refs))
    den = max(float(r.double().abs().max()) for r in refs)
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def sumsq_values(n, seed):
    """n values with magnitudes spread log-uniformly over 1e-4 .. 1e2 and random signs, at element 1.. of a 16-byte aligned
    buffer of n + 1 (x[1:] = the same data four bytes off the alignment)."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n + 1, generator=g) * 6 - 4)
    sign = torch.randint(0, 2, (n + 1,), generator=g) * 2 - 1
    return (mag * sign).float()


def sumsq_chain(n, aligned, nblk=SUMSQ_BLOCKS):
    """Longest chain of fp32 additions that one square passes through in sumsq_kernel + the merge of adam_kernel: the pair tree of a
    16-byte vector (2), one addition per grid-stride trip of its thread (vector trips, then scalar-tail trips), the wave tree (6),
    the 4-way block sum (2), a lane's interleaved walk over the partials (ceil(nblk / 64)) and the merge's wave tree (6)."""
    threads = nblk * SUMSQ_THREADS
    if aligned:
        n4 = n // 4
        per_thread = (2 if n4 else 0) + -(-n4 // threads) + -(-(n - 4 * n4) // threads)
    else:
        per_thread = -(-n // threads)
    return per_thread + 6 + 2 + -(-nblk // 64) + 6


def merge_partials_fp32(part):
    """adam_kernel's merge of the sumsq partials, in fp32 on the host: lane l adds partials l, l + 64, ... in order, then a pair
    tree over the 64 lanes."""
    part = part.detach().float().cpu()
    pad = (-part.numel()) % 64
    rows = torch.cat([part, torch.zeros(pad)]).view(-1, 64)
    tot = torch.zeros(64)
    for r in rows:
        tot = tot + r
    off = 32
    while off:
        tot = tot[:off] + tot[off: 2 * off]
        off //= 2
    return float(tot[0])
