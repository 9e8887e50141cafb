"""Helpers of tests/test_gpu_parallel_head.py (not collected on their own): seeded inputs, plain references and bounds for the
parallel branch head - the CLS pooling kernels (csrc/clspool.hip), the B-row tail (csrc/rowtail.hip) and the whole head
(head_tail.ParallelHeadFn against oracle.parallel_branch_forward).  Nothing here needs a GPU; tests/test_head_cases_cpu.py pins the
builders' properties on the CPU.

Every reference is ONE function, generic in dtype: on ``.double()`` inputs it is the reference, on the fp32 inputs on the CPU it is
the yardstick.  The inputs are what the kernels read: fp32 tensors, and ``X`` as fp32 values that bf16 holds exactly.  A kernel is
compared on its own inputs (the pooling forward on given fp32 scores, the backward on given fp32 ``p`` and ``dp``), so the error of
one kernel is not charged to the next.

Error measure: per row of a quantity's natural grouping, ``max |got - ref| / max |ref|`` over the row (``row_errors``).  Bounds
(docs/parity.md, "Parallel head"), two kinds:
  * sums and dot products: ``k u sum |a_i b_i|`` per output element (u = 2^-24, k = the longest chain of additions of the launch
    geometry + 1 for the rounding of the product), evaluated in fp64 next to the reference and taken over the row like the error;
  * quantities through exp, rsqrt, division or GELU: ``max(4 x the yardstick's error on the same case, 2^-23)``.
"""
import math

import numpy as np
import torch

from test_gpu_kernels import _keep_mask

U = 2.0 ** -24
FLOOR = 2.0 ** -23
YARD_FACTOR = 4.0

# ------------------------------------------------------------------------------------------------------------- pooling cases
POOL_B = 4
POOL_SWEEP = [(64, 1, 40), (64, 8, 8), (256, 2, 64), (320, 4, 77), (512, 4, 200), (768, 8, 320), (768, 16, 136), (1024, 8, 512),
              (1024, 16, 72)]
TRAIN_CASES = [(768, 8, 320), (1024, 8, 512), (64, 1, 40)]
TRAIN_P = (0.1, 0.5)
VALUE_BIAS_CASES = [(1, 64, 1), (7, 768, 8), (65, 768, 8), (5, 1024, 8), (3, 768, 1)]            # (B, D, H)
SOFTMAX_REDUCE_CASES = [(1, 13), (255, 25), (257, 13), (1000, 64), (3, 1)]                     # (nblk, NL)
LDS_BYTES = 64 * 1024


def pool_lengths(R):
    """[R, 1, a value that is no multiple of 32, R // 2 + 1]"""
    odd = R - 3 if (R - 3) % 32 else R - 5
    return [R, 1, odd, R // 2 + 1]


def bf16_values(t):
    return t.to(torch.bfloat16).float()


def pool_case(D, H, R, seed=None, B=POOL_B):
    """X [B, R, D] (fp32 values that bf16 holds exactly, rows s >= len zero), the shared score vectors a [H, D] scaled so that the
    scores have a standard deviation of 1.5, a per-utterance dm [B, H, D], lengths."""
    g = torch.Generator().manual_seed(D * 100003 + H * 1009 + R if seed is None else seed)
    lens = torch.tensor(pool_lengths(R), dtype=torch.int32)[:B]
    X = bf16_values(torch.randn(B, R, D, generator=g))
    X = X * (torch.arange(R)[None, :, None] < lens[:, None, None])
    a = torch.randn(H, D, generator=g) * (1.5 / math.sqrt(D))
    dm = torch.randn(B, H, D, generator=g)
    return {"X": X, "a": a, "dm": dm, "lens": lens, "B": B, "D": D, "H": H, "R": R}


def live_mask(lens, R):
    """[B, R] bool: s < n with the kernels' clamp n = max(1, min(len, R))"""
    n = lens.to(torch.int64).clamp(1, R)
    return torch.arange(R)[None, :] < n[:, None]


def dropout_pattern(B, H, R, lens, p, seed):
    """-> (mult [B, H, R] fp32 of 0 / 1 / (1 - p), the seed used).  The keep bits are the library's hash bits (_keep_mask) of the
    first seed from ``seed`` on whose pattern keeps 50 % .. 95 % of the live weights; a live row that would lose every weight keeps
    its first one (len = 1 at p = 0.5 loses its only key every other time; the kernels take any pattern)."""
    live = live_mask(lens, R)[:, None, :].expand(B, H, R)
    for i in range(256):
        sd = (seed * 0x9E3779B1 + i * 0x85EBCA6B) & 0xffffffff         # far apart: seeds that differ in low bits only permute the hash inputs
        keep = torch.from_numpy(_keep_mask(np.arange(B * H * R, dtype=np.int64), sd, p)).view(B, H, R).clone()
        none = ~(keep & live).any(-1)
        keep[..., 0] |= none
        frac = float((keep & live).sum()) / float(live.sum())
        if 0.5 <= frac <= 0.95:
            return (keep.float() / (1.0 - p)).float().contiguous(), sd
    raise AssertionError("no seed gives a pattern inside 50 % .. 95 %")


def train_case(D, H, R, p, seed=None):
    """pool_case + the value path of the layer: Wv [D, D], bv [D], an upstream dctx [B, D].  dm[b, h] = Wv_h^T dctx[b, h] and
    cbias[b, h] = dctx[b, h] . bv_h are formed once in fp64 and rounded to fp32: they are inputs of the kernels, and the reference
    contracts m and psum with the rounded values (the same function of X and a as ctx_h = Wv_h m_h + bv_h psum_h under dctx)."""
    c = pool_case(D, H, R, seed)
    g = torch.Generator().manual_seed(7 + D + H + R + int(p * 100))
    B, dh = c["B"], D // H
    Wv = torch.randn(D, D, generator=g) * D ** -0.5
    bv = torch.randn(D, generator=g) * 0.5
    dctx = torch.randn(B, D, generator=g)
    c["dm"] = torch.einsum("bhj,hjk->bhk", dctx.double().view(B, H, dh), Wv.double().view(H, dh, D)).float().contiguous()
    c["cbias"] = (dctx.double().view(B, H, dh) * bv.double().view(1, H, dh)).sum(-1).float().contiguous()
    c["mult"], c["mult_seed"] = dropout_pattern(B, H, R, c["lens"], p, seed=1000 + int(p * 100))
    c.update(Wv=Wv, bv=bv, dctx=dctx, p_drop=p)
    return c


# ------------------------------------------------------------------------------------------------------------- pooling references
def scores_ref(X, vec):
    """scores[b, h, s] = vec[(b,) h] . X[b, s]"""
    return torch.einsum("brd,hd->bhr", X, vec) if vec.dim() == 2 else torch.einsum("brd,bhd->bhr", X, vec)


def pool_fwd_ref(X, scores, lens, mult=None):
    """Masked softmax over s < n -> p (un-masked by the dropout), w = p mult, psum = sum_s w, m[b, h] = sum_s w X[b, s]."""
    R = X.shape[1]
    live = live_mask(lens, R)[:, None, :]
    p = torch.softmax(scores.masked_fill(~live, float("-inf")), dim=-1)
    w = p * mult.to(p.dtype) if mult is not None else p
    return {"p": p, "w": w, "psum": w.sum(-1), "m": torch.einsum("bhr,brd->bhd", w, X)}


def pool_bwd_ref(X, p, dp, dm, a, lens, mult=None, cbias=None):
    """The formula of the kernel comment: ds = p ((dp + cbias) mult - sum_s p (dp + cbias) mult), dX = sum_h p mult dm + ds a,
    da[b, h] = sum_s ds X[b, s].  ``cbias`` None: dp arrives as (dp + cbias) mult.  (The yardstick; the fp64 reference of the
    backward is autograd on the forward, pool_autograd.)"""
    R = X.shape[1]
    live = live_mask(lens, R)[:, None, :].to(p.dtype)
    dpe = dp if cbias is None else (dp + cbias[..., None]) * (mult.to(p.dtype) if mult is not None else 1.0)
    pl = p * live
    dot = (pl * dpe).sum(-1, keepdim=True)
    ds = pl * (dpe - dot)
    w = pl * mult.to(p.dtype) if mult is not None else pl
    av = a if a.dim() == 3 else a[None].expand(X.shape[0], -1, -1)
    dX = torch.einsum("bhr,bhd->brd", w, dm) + torch.einsum("bhr,bhd->brd", ds, av)
    return {"ds": ds, "dX": dX, "da_part": torch.einsum("bhr,brd->bhd", ds, X)}


def pool_autograd(X, a, dm, lens, mult=None, cbias=None, dtype=torch.float64):
    """autograd in ``dtype`` through scores -> masked softmax -> m, psum of  L = sum m . dm + sum psum cbias  ->  the forward
    quantities, dp = dL / d(p mult) = X . dm, dX, da (shared a: summed over b, as sum_b da_part)."""
    Xd = X.to(dtype).requires_grad_(True)
    ad = a.to(dtype).requires_grad_(True)
    f = pool_fwd_ref(Xd, scores_ref(Xd, ad), lens, mult)
    f["w"].retain_grad()
    L = (f["m"] * dm.to(dtype)).sum()
    if cbias is not None:
        L = L + (f["psum"] * cbias.to(dtype)).sum()
    L.backward()
    dp = f["w"].grad.detach()
    if cbias is not None:
        dp = dp - cbias.to(dtype)[..., None]                      # raw X . dm: the value-bias term is added by the consumer
    return {"scores": scores_ref(Xd, ad).detach(), "p": f["p"].detach(), "m": f["m"].detach(), "psum": f["psum"].detach(), "dp": dp,
            "dX": Xd.grad, "da": ad.grad}


# ------------------------------------------------------------------------------------------------------------- error measure
ZERO = 1e-300


def row_errors(got, ref, dims):
    """max over ``dims`` (the dimensions INSIDE a row) of |got - ref|, relative to the reference row's largest magnitude -> one
    figure per row.  A reference row that is exactly zero has no scale: 0 if the row of ``got`` is exactly zero, inf otherwise."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not dims:
        num, den, gmax = (got - ref).abs(), ref.abs(), got.abs()
    else:
        num, den, gmax = (got - ref).abs().amax(dims), ref.abs().amax(dims), got.abs().amax(dims)
    num = torch.where(torch.isnan(num), torch.full_like(num, float("inf")), num)
    zero = den < ZERO
    e = num / den.clamp_min(ZERO)
    return torch.where(zero, torch.where(gmax == 0, torch.zeros_like(e), torch.full_like(e, float("inf"))), e)


def row_bounds(elem_bound, ref, dims):
    """A per-element absolute bound in the units of row_errors: largest bound of the row over the row's largest |ref|."""
    ref, elem_bound = ref.detach().double().cpu(), elem_bound.detach().double().cpu()
    if not dims:
        return elem_bound / ref.abs().clamp_min(ZERO)
    return elem_bound.amax(dims) / ref.abs().amax(dims).clamp_min(ZERO)


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def yard_bound(yard_err):
    """Bound of a quantity through exp / rsqrt / division / GELU from the yardstick's worst row on the same case."""
    return max(YARD_FACTOR * float(yard_err), FLOOR)


class Report:
    """Collects PARITY lines and violations; ``check`` prints before anything is asserted, ``done`` fails once with the list."""

    def __init__(self):
        self.bad, self.lines = [], []

    def _line(self, case, q, err, yard, bound):
        ys = "-" if yard is None else f"{yard:.3e}"
        line = f"PARITY|{case}|{q}|{err:.3e}|{ys}|{bound:.3e}"
        print(line)
        self.lines.append(line)
        if not err <= bound:
            self.bad.append(f"{case}: {q} error {err:.3e} > bound {bound:.3e} (yardstick {ys})")

    def yard(self, case, q, got, ref, yard, dims, elem_bound=None, rows=None):
        """Every row of ``got`` within max(4 x the yardstick's worst row, 2^-23).  The rows marked in ``rows`` may instead meet
        their own derived bound ``elem_bound`` (dX on the rows of a dropped key: such a row holds -p dot a, the relative error of
        the cancelling sum ``dot``, of which the yardstick is one sample - docs/parity.md).  The line shows the row with the
        largest error / bound."""
        e = row_errors(got, ref, dims).reshape(-1)
        y = float(row_errors(yard, ref, dims).max())
        b = torch.full_like(e, yard_bound(y))
        if rows is not None and bool(rows.any()):
            own = row_bounds(elem_bound, ref, dims).reshape(-1)
            b = torch.where(rows.reshape(-1), torch.maximum(b, own), b)
        i = int((e / b).argmax())
        self._line(case, q, float(e[i]), y, float(b[i]))
        return float(e[i])

    def derived(self, case, q, got, ref, elem_bound, dims, yard=None):
        """Every row of ``got`` within its own derived bound; the line shows the row with the largest error / bound."""
        e, b = row_errors(got, ref, dims).reshape(-1), row_bounds(elem_bound, ref, dims).reshape(-1)
        ratio = torch.where(e == 0, torch.zeros_like(e), e / b.clamp_min(ZERO))
        i = int(ratio.argmax())
        y = None if yard is None else float(row_errors(yard, ref, dims).max())
        self._line(case, q, float(e[i]), y, float(b[i]))
        return float(ratio[i])

    def equal(self, case, q, a, b):
        same = a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())
        self._line(case, q + " (bits)", 0.0 if same else float("inf"), None, 0.0)

    def require(self, case, what, ok):
        if not ok:
            self.bad.append(f"{case}: {what}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


# ------------------------------------------------------------------------------------------------------------- derived bounds: pooling
def nch(D):
    """cls_scores_kernel: 4-element chunks per lane"""
    return (D // 4 + 63) // 64


def k_scores(D):
    """A lane adds 4 NCH products in order, then 6 shuffle levels; + 1 for the product."""
    return 4 * nch(D) + 6 + 1


def scores_bound(X, vec):
    return k_scores(X.shape[-1]) * U * scores_ref(X.double().abs(), vec.double().abs())


def weight_eps(scores, lens):
    """Relative error of the pooling weight w = exp(s - max) / sum * mult inside cls_pool_fwd_kernel, per (b, h), in units of 1:
    the argument s - max is rounded once (u |s - max| on the exponent) and __expf is v_exp_f32 on arg * log2(e): one more rounding
    of the scaled argument (u |s - max| log2(e) ln 2 = u |s - max|) and 1 ulp of the instruction (2 u); the row sum adds
    ceil(n / 64) + 6 terms; reciprocal, product with it and product with mult one rounding each."""
    R = scores.shape[-1]
    live = live_mask(lens, R)[:, None, :]
    s = scores.double().masked_fill(~live, float("-inf"))
    span = (s.amax(-1, keepdim=True) - s).masked_fill(~live, 0.0).amax(-1)                  # [B, H]
    n = lens.to(torch.int64).clamp(1, R).double()[:, None]
    e_exp = 2.0 * span + 2.0
    return U * (2.0 * e_exp + torch.ceil(n / 64) + 6 + 3)


def k_pool_m(n):
    """cls_pool_fwd_kernel: a lane adds every 32nd row (fma), 3 shuffle levels, 2 levels over the 4 waves; + 1 product"""
    return -(-int(n) // 32) + 3 + 2 + 1


def m_bound(X, scores, lens, mult=None):
    """|m - m64| <= (k u + eps_w) sum_s |w X|"""
    f = pool_fwd_ref(X.double(), scores.double(), lens, mult)
    mag = torch.einsum("bhr,brd->bhd", f["w"].abs(), X.double().abs())
    R = X.shape[1]
    k = torch.tensor([k_pool_m(n) for n in lens.clamp(1, R).tolist()], dtype=torch.float64)[:, None, None]
    return (k * U + weight_eps(scores, lens)[..., None]) * mag


def ds_error(p, dp, lens, mult=None, cbias=None):
    """ds = p (dpe - dot) as cls_pool_bwd_kernel forms it from the given p and dp -> (ds, |error| bound), fp64:
         dpe = (dp + cbias) mult: two roundings, 2 u (|dp| + |cbias|) |mult|  (none when it arrives pre-formed);
         dot = sum_s p dpe: a lane adds ceil(n / 64) products, 6 shuffle levels: (ceil(n / 64) + 7) u sum |p dpe| + the dpe errors;
         dpe - dot and the product with p: u each;
         p and dp themselves are the fp32 roundings of the fp64 forward's values (the reference differentiates the fp64 forward)."""
    R = p.shape[-1]
    live = live_mask(lens, R)[:, None, :].double()
    pd_, dpd = p.double() * live, dp.double()
    mu = mult.double() if mult is not None else torch.ones_like(pd_)
    if cbias is not None:
        cb = cbias.double()[..., None]
        dpe, e_dpe = (dpd + cb) * mu, 2 * U * (dpd.abs() + cb.abs()) * mu.abs()
    else:
        dpe, e_dpe = dpd, torch.zeros_like(dpd)
    e_dpe = e_dpe + U * dpe.abs()                 # the kernel's p and dp are the fp32 roundings of the fp64 forward's: u each
    n = lens.to(torch.int64).clamp(1, R).double()[:, None, None]
    dot = (pd_ * dpe).sum(-1, keepdim=True)
    e_dot = (torch.ceil(n / 64) + 7 + 1) * U * (pd_ * dpe.abs()).sum(-1, keepdim=True) + (pd_ * e_dpe).sum(-1, keepdim=True)
    ds = pd_ * (dpe - dot)
    return ds, pd_ * (e_dpe + e_dot + U * (dpe.abs() + dot.abs())) + 2 * U * ds.abs()


def da_bound(X, p, dp, lens, mult=None, cbias=None):
    """da_part[b, h, d] = sum_s ds X: the error of ds (ds_error) through |X|, and the sum over s: a lane adds every 16th row, 2
    shuffle levels, 2 levels over the waves, + 1 product."""
    R = X.shape[1]
    ds, e_ds = ds_error(p, dp, lens, mult, cbias)
    n = lens.to(torch.int64).clamp(1, R).double()[:, None, None]
    k = torch.ceil(n / 16) + 2 + 2 + 1
    Xa = X.double().abs()
    return torch.einsum("bhr,brd->bhd", e_ds, Xa) + k * U * torch.einsum("bhr,brd->bhd", ds.abs(), Xa)


def dx_bound(p, dp, dm, a, lens, mult=None, cbias=None):
    """dX[b, s] = sum_h p mult dm + ds a: 2 H products and additions per element on top of the error of ds and the rounding of
    p mult.  Used as the yardstick's sanity bound on the CPU; on the device dX is held to 4 x the yardstick."""
    R, H = p.shape[-1], p.shape[1]
    ds, e_ds = ds_error(p, dp, lens, mult, cbias)
    live = live_mask(lens, R)[:, None, :].double()
    w = p.double() * live * (mult.double() if mult is not None else 1.0)
    av = (a if a.dim() == 3 else a[None].expand(p.shape[0], -1, -1)).double().abs()
    mag = torch.einsum("bhr,bhd->brd", w.abs(), dm.double().abs()) + torch.einsum("bhr,bhd->brd", ds.abs(), av)
    return torch.einsum("bhr,bhd->brd", e_ds, av) + (2 * H + 2) * U * mag


def pool_lds_limits(H):
    """Largest R (a multiple of 8) that the 64 KiB LDS checks of sc_cls_pool_fwd / _bwd accept: the forward keeps p[H][R] and
    red[4][H][64] floats, the backward ps[H][R], dss[H][R] and red[4][H][64]."""
    words = LDS_BYTES // 4
    fwd = (words - 4 * H * 64) // H
    bwd = (words - 4 * H * 64) // (2 * H)
    return fwd // 8 * 8, bwd // 8 * 8


# ------------------------------------------------------------------------------------------------------------- weighted-sum logits
def softmax_reduce_ref(part, w):
    """out[n] = w_n (d_n - sum_m w_m d_m), d = column sums of part [nblk, NL]"""
    d = part.sum(0)
    return w * (d - (w * d).sum())


def softmax_reduce_bound(part, w):
    """d_n: thread t adds blocks t, t + 256, ..., 6 shuffle levels, 2 levels over the waves; the dot over NL: 6 levels + 1 product;
    the difference and the product with w_n: u each."""
    part, w = part.double(), w.double()
    nblk = part.shape[0]
    k = -(-nblk // 256) + 6 + 2
    d = part.sum(0)
    e_d = k * U * part.abs().sum(0)
    dot = (w * d).sum()
    e_dot = (w.abs() * e_d).sum() + 7 * U * (w * d).abs().sum()
    return w.abs() * (e_d + e_dot + U * (d.abs() + dot.abs())) + U * (w * (d - dot)).abs()


# ------------------------------------------------------------------------------------------------------------- pooling: one case
def pool_reference(c, mult=None, cbias=None):
    """-> (ref, inp): the fp64 quantities of a case and the fp32 tensors the kernels are given: scores, p and dp are the fp64
    forward's values rounded once.  The forward quantities p / m / psum of ``ref`` are re-evaluated on the rounded scores (the
    forward kernel's own input); the backward quantities are autograd's on the fp64 forward."""
    ref = pool_autograd(c["X"], c["a"], c["dm"], c["lens"], mult, cbias)
    inp = {k: ref[k].float().contiguous() for k in ("scores", "p", "dp")}
    f = pool_fwd_ref(c["X"].double(), inp["scores"].double(), c["lens"], mult)
    ref.update(p=f["p"], m=f["m"], psum=f["psum"])
    return ref, inp


def pool_yardstick(c, inp, mult=None, cbias=None):
    """The same operations in fp32 on the CPU, on the kernels' inputs."""
    X, a, dm, lens = c["X"], c["a"], c["dm"], c["lens"]
    y = {"scores": scores_ref(X, a), "dp": scores_ref(X, dm)}
    f = pool_fwd_ref(X, inp["scores"], lens, mult)
    b = pool_bwd_ref(X, inp["p"], inp["dp"], dm, a, lens, mult, cbias)
    y.update(p=f["p"], m=f["m"], psum=f["psum"], dX=b["dX"], da=b["da_part"].double().sum(0))
    return y


def pool_bounds(c, inp, mult=None, cbias=None):
    """Per-element bounds of the derived kind."""
    X, lens = c["X"], c["lens"]
    bd = {"scores": scores_bound(X, c["a"]), "dp": scores_bound(X, c["dm"])}
    bd["m"] = m_bound(X, inp["scores"], lens, mult)
    bd["da"] = da_bound(X, inp["p"], inp["dp"], lens, mult, cbias).sum(0)
    bd["dX"] = dx_bound(inp["p"], inp["dp"], c["dm"], c["a"], lens, mult, cbias)
    return bd


def dropped_key_rows(c, mult):
    """[B, R] bool: the live keys that some head's dropout multiplier drops (there dX holds ds a alone for that head)."""
    live = live_mask(c["lens"], c["R"])
    if mult is None:
        return torch.zeros_like(live)
    return ((mult == 0) & live[:, None, :]).any(1)


POOL_DIMS = {"scores": (1,), "dp": (1,), "p": (2,), "m": (2,), "psum": (), "dX": (2,), "da": (1,)}      # dimensions inside a row
POOL_DERIVED = ("scores", "dp", "m", "da")
POOL_YARD = ("p", "psum", "dX")


def pool_checks(rep, name, c, got, ref, yard, bounds, mult=None):
    """Every quantity of ``got`` against ``ref`` by its own kind of bound."""
    for q, v in got.items():
        if q in POOL_DERIVED:
            rep.derived(name, q, v, ref[q], bounds[q], POOL_DIMS[q], yard[q])
        else:
            rep.yard(name, q, v, ref[q], yard[q], POOL_DIMS[q], bounds.get(q), dropped_key_rows(c, mult) if q == "dX" else None)
    if "p" in got:
        dead = ~live_mask(c["lens"], c["R"])[:, None, :].expand_as(ref["p"])
        rep.require(name, "p is not exactly 0 on s >= n", bool((got["p"].detach().cpu()[dead] == 0).all()))
    if "dX" in got:
        dead = ~live_mask(c["lens"], c["R"])
        rep.require(name, "dX is not exactly 0 on s >= n", bool((got["dX"].detach().cpu()[dead] == 0).all()))


def value_bias_case(B, D, H, seed=5):
    g = torch.Generator().manual_seed(seed + B * 31 + D + H)
    return {"dctx": torch.randn(B, D, generator=g), "bv": torch.randn(D, generator=g) * 0.5, "psum": 0.5 + torch.rand(B, H, generator=g),
            "gbv0": torch.randn(D, generator=g), "B": B, "D": D, "H": H}


def value_bias_ref(c, dtype):
    """cbias[b, h] = sum_j dctx[b, h, j] bv[h, j] ; gbv[h, j] = gbv0 + sum_b dctx[b, h, j] psum[b, h]"""
    B, D, H = c["B"], c["D"], c["H"]
    dh = D // H
    dctx, bv, psum = c["dctx"].to(dtype).view(B, H, dh), c["bv"].to(dtype).view(1, H, dh), c["psum"].to(dtype)
    return {"cbias": (dctx * bv).sum(-1), "gbv": c["gbv0"].to(dtype) + (dctx * psum[..., None]).sum(0).reshape(D)}


def value_bias_bounds(c):
    """cbias: a lane adds ceil(dh / 64) products, 6 shuffle levels, + 1 product; gbv: B products in order, the add onto gbv, + 1"""
    B, D, H = c["B"], c["D"], c["H"]
    dh = D // H
    dctx, bv, psum = c["dctx"].double().view(B, H, dh).abs(), c["bv"].double().view(1, H, dh).abs(), c["psum"].double().abs()
    return {"cbias": (-(-dh // 64) + 6 + 1) * U * (dctx * bv).sum(-1),
            "gbv": (B + 1 + 1) * U * (c["gbv0"].double().abs() + (dctx * psum[..., None]).sum(0).reshape(D))}


def softmax_reduce_case(nblk, NL, seed=9):
    g = torch.Generator().manual_seed(seed + nblk + NL)
    return torch.randn(nblk, NL, generator=g), torch.softmax(torch.randn(NL, generator=g), 0)


# ------------------------------------------------------------------------------------------------------------- row tail (csrc/rowtail.hip)
TAIL_CASES = [(1, 768, 3072, 512), (7, 768, 3072, 512), (65, 768, 3072, 512), (130, 768, 3072, 512), (7, 1024, 4096, 768)]   # (B, D, F, E)
TAIL_H = 8
RT_K = 32                                    # rt_gemm_kernel: K-step
SEED_F, P_F, SEED_D, P_D = 99, 0.25, 7, 0.1  # the hash dropout of the [B, F] and [B, D] sites


def rt_kc(K, S):
    """sc_rt_gemm: K per slice, a multiple of the K-step"""
    return -(-(-(-K // S)) // RT_K) * RT_K


def rt_slices(M, N, K, nbatch=1, num_cus=256):
    """sc_rt_gemm_slices restated (enough workgroups to cover the chip, slices of 128 at least, 8 at most)."""
    tiles = -(-N // 64) * -(-M // 64) * max(nbatch, 1)
    S = max(1, min(min(-(-num_cus // tiles), max(K // 128, 1)), 8))
    return -(-K // rt_kc(K, S))


def k_gemm(K, S, extra=0):
    """One slice adds Kc products in order on the matrix pipe; its consumer (or Slices.total()) adds the S slices; ``extra`` further
    additions (alpha, bias, accumulate, an A operand that is itself a sum of slices plus a bias); + 1 for the product."""
    return rt_kc(K, S) + S + extra + 1


def gelu_grad_ref(x):
    return 0.5 * (1 + torch.erf(x * 0.7071067811865476)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


def keep_rows(rows, cols, seed, p):
    """The hash keep bits of a [rows, cols] site (element index row * cols + col)."""
    return torch.from_numpy(_keep_mask(np.arange(rows * cols, dtype=np.int64), seed, p)).view(rows, cols).clone()


def ln_fwd_ref(z, g, b, eps):
    """-> (out, xhat, rstd)"""
    mean = z.mean(-1, keepdim=True)
    rstd = (((z - mean) ** 2).mean(-1, keepdim=True) + eps).rsqrt()
    xhat = (z - mean) * rstd
    return xhat * g + b, xhat, rstd[..., 0]


def ln_bwd_ref(d, xhat, gamma, rstd):
    """dx = rstd (g - mean g - xhat mean(g xhat)), g = d gamma; dgamma = sum_rows d xhat, dbeta = sum_rows d  (the yardstick; the
    fp64 reference is autograd on ln_fwd_ref)."""
    gg = d * gamma
    dx = rstd[:, None] * (gg - gg.mean(-1, keepdim=True) - xhat * (gg * xhat).mean(-1, keepdim=True))
    return dx, (d * xhat).sum(0), d.sum(0)


def tail_case(B, D, F_, E):
    g = torch.Generator().manual_seed(B * 7919 + D)
    r = lambda *s: torch.randn(*s, generator=g)
    H = TAIL_H
    c = {"B": B, "D": D, "F": F_, "E": E, "H": H, "dh": D // H}
    c["x"], c["W1"], c["b1"], c["C0"] = r(B, D), r(F_, D) * D ** -0.5, r(F_) * 0.5, r(B, F_)
    c["ysl"], c["rs"] = r(3, B, F_) * 0.6, 0.5 + torch.rand(B, H, generator=g)
    c["dy"], c["gW0"], c["gb0"] = r(B, F_), r(F_, D), r(F_)
    c["m"], c["Wv"], c["dc"], c["gWv0"], c["gbv0"] = r(B, H, D), r(D, D) * D ** -0.5, r(B, D), r(D, D), r(D)
    c["g1"], c["g2"], c["be1"], c["be2"] = 1 + 0.1 * r(D), 1 + 0.1 * r(D), 0.1 * r(D), 0.1 * r(D)
    c["bias_d"], c["res0"], c["resB"], c["zsl"] = r(D), r(1, D), r(B, D), r(3, B, D) * 0.6
    c["dys"], c["add"], c["dgam0"], c["dbet0"] = r(3, B, D) * 0.6, r(B, D), r(D), r(D)
    c["wsl"], c["bp"], c["ge"] = r(3, B, E) * 0.6, r(E) * 0.5, r(B, E)
    return c


TAIL_DERIVED = ("gemm_split", "gemm_U", "elem0", "gemm_sliced", "gW", "gb", "h_ctx", "h_gWv", "h_gbv", "h_dm", "lnb_dgamma", "lnb_dbeta",
                "elem1_u", "l2_x")
TAIL_YARD = ("gemm_C", "ln1_out", "ln1_xhat", "ln1_rstd", "lnc_out1", "lnc_out2", "lnc_xhat2", "lnc_rstd2", "lnb_dx", "lnb_dxm", "elem1_f",
             "elem2", "l2_e", "l2_rn", "l2_bwd")
TAIL_VECTORS = ("gb", "h_gbv", "lnb_dgamma", "lnb_dbeta", "ln1_rstd", "lnc_rstd2", "l2_rn")       # one figure per element


def tail_dims(q):
    return () if q in TAIL_VECTORS else (1,)


def tail_reference(c, dtype, inp=None):
    """Every row-tail quantity of a case in ``dtype``.  float64: the reference (LayerNorm, GELU and unit-row backward by autograd)
    -> (r, inp) with ``inp`` the saved tensors a backward kernel is given (xhat, rstd, u, e, 1 / |x|: the fp64 forward's values
    rounded once).  float32: the yardstick on the same ``inp`` (hand-written backward formulas) -> r."""
    t = lambda k: c[k].to(dtype)
    B, D, F_, E, H, dh = c["B"], c["D"], c["F"], c["E"], c["H"], c["dh"]
    ref64 = dtype == torch.float64
    zero = torch.zeros((), dtype=dtype)
    keepF, keepD = keep_rows(B, F_, SEED_F, P_F), keep_rows(B, D, SEED_D, P_D)
    x, W1, b1 = t("x"), t("W1"), t("b1")
    r = {"gemm_split": x @ W1.T}
    r["gemm_U"] = 0.5 * r["gemm_split"] + b1
    r["gemm_C"] = torch.where(keepF, torch.nn.functional.gelu(r["gemm_U"]) / (1 - P_F), zero) + 2 * t("C0")
    ysum = t("ysl")[0] + t("ysl")[1] + t("ysl")[2]
    r["elem0"] = ysum + b1[None] * t("rs").repeat_interleave(F_ // H, dim=1)
    r["gemm_sliced"] = r["elem0"] @ W1
    r["gW"], r["gb"] = t("gW0") + t("dy").T @ x, t("gb0") + t("dy").sum(0)
    m, Wv, dc = t("m"), t("Wv").view(H, dh, D), t("dc").view(B, H, dh)
    r["h_ctx"] = torch.einsum("bhk,hjk->bhj", m, Wv).reshape(B, D)
    r["h_gWv"] = t("gWv0") + torch.einsum("bhj,bhk->hjk", dc, m).reshape(D, D)
    r["h_gbv"] = t("gbv0") + t("dc").sum(0)
    r["h_dm"] = torch.einsum("bhj,hjk->bhk", dc, Wv).reshape(B, H * D)
    # LayerNorm over slices: single (broadcast residual) and chained (per-row residual), dropout on the producer term
    z_pre = torch.where(keepD, (t("zsl")[0] + t("zsl")[1] + t("zsl")[2] + t("bias_d")) / (1 - P_D), zero)
    r["ln1_out"], r["ln1_xhat"], r["ln1_rstd"] = ln_fwd_ref(z_pre + t("res0"), t("g1"), t("be1"), 1e-5)
    z2 = (z_pre + t("resB")).detach().requires_grad_(ref64)
    g1p, b1p = t("g1").detach().requires_grad_(ref64), t("be1").detach().requires_grad_(ref64)
    o1, h1, r1 = ln_fwd_ref(z2, g1p, b1p, 1e-5)
    r["lnc_out1"] = o1.detach()
    r["lnc_out2"], r["lnc_xhat2"], r["lnc_rstd2"] = (v.detach() for v in ln_fwd_ref(o1, t("g2"), t("be2"), 1e-6))
    gin = t("dys")[0] + t("dys")[1] + t("dys")[2] + t("add")
    u64 = ysum + b1
    xs = t("wsl")[0] + t("wsl")[1] + t("wsl")[2] + t("bp")
    if ref64:
        o1.backward(gin)
        dx, dg, db = z2.grad, g1p.grad, b1p.grad
        rn = 1.0 / xs.norm(dim=-1)
        inp = {"xhat": h1.detach().float(), "rstd": r1.detach().float(), "u": u64.float(), "e": (xs * rn[:, None]).float(), "rn": rn.float()}
    else:
        dx, dg, db = ln_bwd_ref(gin, inp["xhat"], t("g1"), inp["rstd"])
    r["lnb_dx"], r["lnb_dxm"] = dx, torch.where(keepD, dx / (1 - P_D), zero)
    r["lnb_dgamma"], r["lnb_dbeta"] = t("dgam0") + dg, t("dbet0") + db
    # elementwise: GELU forward on the slices, GELU backward at the saved pre-activation
    r["elem1_u"] = u64
    r["elem1_f"] = torch.where(keepF, torch.nn.functional.gelu(u64) / (1 - P_F), zero)
    maskF = torch.where(keepF, torch.ones((), dtype=dtype) / (1 - P_F), zero)
    if ref64:
        up = inp["u"].double().requires_grad_(True)
        torch.nn.functional.gelu(up).backward(ysum * maskF)
        r["elem2"] = up.grad
    else:
        r["elem2"] = ysum * maskF * gelu_grad_ref(inp["u"])
    # unit rows
    r["l2_x"] = xs
    if ref64:
        xr = xs.detach().requires_grad_(True)
        er = xr / xr.norm(dim=-1, keepdim=True)
        er.backward(t("ge"))
        r["l2_e"], r["l2_rn"], r["l2_bwd"] = er.detach(), 1.0 / xs.norm(dim=-1), xr.grad
        return {k: v.detach() for k, v in r.items()}, inp
    rn = 1.0 / xs.norm(dim=-1)
    r["l2_e"], r["l2_rn"] = xs * rn[:, None], rn
    r["l2_bwd"] = (t("ge") - inp["e"] * (t("ge") * inp["e"]).sum(-1, keepdim=True)) * inp["rn"][:, None]
    return r


def tail_bounds(c, inp, S):
    """Per-element bounds of the derived kind.  ``S``: the number of slices of the three split products {"x_W1", "sliced", "ctx"}.
       gemm_split   k_gemm(D, S)                        (total() adds the slices)
       gemm_U       k_gemm(D, 1) + 2                    (alpha, bias)
       elem0        ns + 2                              (slices in order, the product bias * rowscale, its addition)
       gemm_sliced  k_gemm(F, S) + ns + 2               (the A operand is elem0's sum, formed in the operand load)
       gW, h_gWv    k_gemm(B, 1) + 1                    (the contraction runs over the B rows; + the accumulate)
       gb, h_gbv    Kc(B) + 1                           (a thread adds the Kc rows of its column in order, then onto gb)
       h_ctx        k_gemm(D, S);   h_dm  k_gemm(dh, 1)
       dgamma/dbeta ns + 1 (slices, add) + ceil(B / 8) (a row group's rows) + 8 (groups) + 1 (onto the contents) + 1 (product)
                    + 1 (xhat is a rounded input)
       elem1_u, l2_x   ns + 1"""
    d = lambda k: c[k].double()
    B, D, F_, H, dh = c["B"], c["D"], c["F"], c["H"], c["dh"]
    ns = 3
    xa, Wa = d("x").abs(), d("W1").abs()
    xw = xa @ Wa.T
    bd = {"gemm_split": k_gemm(D, S["x_W1"]) * U * xw, "gemm_U": (k_gemm(D, 1) + 2) * U * (0.5 * xw + d("b1").abs())}
    amag = d("ysl").abs().sum(0) + d("b1").abs()[None] * d("rs").abs().repeat_interleave(F_ // H, dim=1)
    bd["elem0"] = (ns + 2) * U * amag
    bd["gemm_sliced"] = (k_gemm(F_, S["sliced"]) + ns + 2) * U * (amag @ Wa)
    bd["gW"] = (k_gemm(B, 1) + 1) * U * (d("gW0").abs() + d("dy").abs().T @ xa)
    bd["gb"] = (rt_kc(B, 1) + 1) * U * (d("gb0").abs() + d("dy").abs().sum(0))
    ma, Wva, dca = d("m").abs(), d("Wv").abs().view(H, dh, D), d("dc").abs().view(B, H, dh)
    bd["h_ctx"] = k_gemm(D, S["ctx"]) * U * torch.einsum("bhk,hjk->bhj", ma, Wva).reshape(B, D)
    bd["h_gWv"] = (k_gemm(B, 1) + 1) * U * (d("gWv0").abs() + torch.einsum("bhj,bhk->hjk", dca, ma).reshape(D, D))
    bd["h_gbv"] = (rt_kc(B, 1) + 1) * U * (d("gbv0").abs() + d("dc").abs().sum(0))
    bd["h_dm"] = k_gemm(dh, 1) * U * torch.einsum("bhj,hjk->bhk", dca, Wva).reshape(B, H * D)
    gin = d("dys").abs().sum(0) + d("add").abs()
    k = ns + 1 + -(-B // 8) + 8 + 1 + 1 + 1
    bd["lnb_dgamma"] = k * U * (d("dgam0").abs() + (gin * inp["xhat"].double().abs()).sum(0))
    bd["lnb_dbeta"] = k * U * (d("dbet0").abs() + gin.sum(0))
    bd["elem1_u"] = (ns + 1) * U * (d("ysl").abs().sum(0) + d("b1").abs())
    bd["l2_x"] = (ns + 1) * U * (d("wsl").abs().sum(0) + d("bp").abs())
    return bd


def tail_checks(rep, name, got, ref, yard, bounds):
    for q, v in got.items():
        if q in TAIL_DERIVED:
            rep.derived(name, q, v, ref[q], bounds[q], tail_dims(q), yard[q])
        else:
            rep.yard(name, q, v, ref[q], yard[q], tail_dims(q))


# ------------------------------------------------------------------------------------------------------------- whole head
HEAD_CASES = [(768, 8, 3072, 512), (1024, 8, 4096, 768)]                                       # (d_model, nhead, ffn, E)
HEAD_B, HEAD_T, HEAD_LENS, HEAD_P = 3, 100, (100, 37, 1), 0.1
HEAD_R = (HEAD_T + 1 + 127) // 128 * 128
ZERO_BIAS_PART = 1e-4                        # in_proj_bias key part: exactly zero reference => |grad| < 1e-4 of the bias gradient's scale


def head_weights(d_model, ffn, E, seed=7123):
    """oracle.init_parallel_branch_weights with a ``cls`` that bf16 holds exactly: the head stores the CLS slot of the key / value
    rows in bf16 next to the features, so, like X, its rounding is the input and not an error."""
    import oracle
    W = oracle.init_parallel_branch_weights(d_model, ffn, E, 1, seed)
    W["cls"] = bf16_values(W["cls"])
    return W


def head_inputs(d_model, E, seed=11):
    g = torch.Generator().manual_seed(seed + d_model)
    feat = bf16_values(torch.randn(HEAD_B, HEAD_T, d_model, generator=g))
    return feat, torch.tensor(HEAD_LENS, dtype=torch.int64), torch.randn(HEAD_B, E, generator=g)


def head_drop_fn(mult, k1, kf, k2):
    """The ``drop`` hook of oracle.parallel_branch_forward from the head's four multipliers (the CLS query row only: the other rows
    of the layer do not reach the output)."""
    row0 = {"dropout1": k1, "dropout": kf, "dropout2": k2}

    def drop(site, layer, t):
        m = torch.ones_like(t)
        if site == "attn":
            m[:, :, 0, :] = mult[:, :, : t.shape[-1]].to(t.dtype)
        else:
            m[:, 0] = row0[site].to(t.dtype)
        return t * m

    return drop


def head_host_masks(d_model, nhead, ffn, p=HEAD_P, seed=4242):
    """Four multipliers from the hash bits of four seeds (the CPU module's stand-in for the device's draw)."""
    mk = lambda rows, cols, sd: keep_rows(rows, cols, sd, p).float() / (1.0 - p)
    return (mk(HEAD_B * nhead, HEAD_R, seed).view(HEAD_B, nhead, HEAD_R), mk(HEAD_B, d_model, seed + 1), mk(HEAD_B, ffn, seed + 2),
            mk(HEAD_B, d_model, seed + 3))


def head_reference(W, feat, lens, gout, nhead, drop=None, dtype=torch.float64):
    """oracle.parallel_branch_forward in ``dtype`` under autograd -> {"out", "d_feat", "g_<parameter>"}; in_proj_bias is split into
    its query, key and value parts (the key part is zero analytically: a shift of every score of a row)."""
    import oracle
    Wd = {k: v.detach().to(dtype).requires_grad_(True) for k, v in W.items()}
    f = feat.detach().to(dtype).requires_grad_(True)
    out = oracle.parallel_branch_forward(Wd, f, lens, nhead=nhead, drop=drop)
    assert out.dtype == dtype
    (out * gout.to(dtype)).sum().backward()
    return head_quantities(out.detach(), f.grad, {k: v.grad for k, v in Wd.items()})


def head_quantities(out, d_feat, grads):
    r = {"out": out, "d_feat": d_feat}
    for k, g in grads.items():
        if k.endswith("in_proj_bias"):
            D = g.shape[0] // 3
            r["g_" + k + "[q]"], r["g_" + k + "[k]"], r["g_" + k + "[v]"] = g[:D], g[D: 2 * D], g[2 * D:]
        else:
            r["g_" + k] = g
    return r


def head_dims(q, t):
    """out: row b; d feat: row (b, s); d cls and the parameter gradients: the tensor as one row"""
    return (1,) if q == "out" else (2,) if q == "d_feat" else tuple(range(t.dim()))


def head_checks(rep, name, got, ref, yard):
    for q, v in got.items():
        if q.endswith("in_proj_bias[k]"):
            full = max(float(ref[q[:-3] + "[q]"].abs().max()), float(ref[q[:-3] + "[v]"].abs().max()))
            rep._line(name, q + " (zero reference)", float(v.detach().abs().max()) / full, float(yard[q].abs().max()) / full, ZERO_BIAS_PART)
            rep.require(name, "the fp64 key-part gradient is not zero", float(ref[q].abs().max()) < 1e-12 * full)
        else:
            rep.yard(name, q, v, ref[q], yard[q], head_dims(q, ref[q]))
