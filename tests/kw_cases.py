"""Helpers of tests/test_gpu_kw_kernels.py (not collected on their own): seeded inputs, plain references and bounds for the kernels
of the cascaded+ / hybrid+ keyword branch - continuous integrate-and-fire (csrc/cif.hip), the keyword quantiser's row kernels and
the keyword BatchNorm (csrc/vq.hip), the row softmax of the attention block (csrc/softmax.hip).  Nothing here needs a GPU;
tests/test_kw_cases_cpu.py pins the builders' properties on the CPU.

Every reference is ONE function, generic in dtype, written from the formulas in the kernel comments and include/speechclip_hip.h:
on ``.double()`` inputs it is the reference, on the fp32 inputs on the CPU it is the yardstick.  A kernel is compared on its own
inputs; a downstream kernel is given the fp64 upstream result rounded once to fp32 (or exact bf16 values).  Every backward
reference is autograd on the fp64 forward; the hand-written backward formulas here are the yardstick's, and the CPU module checks
that each equals autograd in fp64 to 1e-12.

Error measure and bounds are the project's (docs/parity.md, "Parallel head"; head_cases.py): per row of a quantity's natural
grouping, ``k u sum |a_i b_i|`` for sums of products, ``max(4 x yardstick, 2^-23)`` through exp / log / rsqrt / division.

Discrete quantities (slot indices, fired marks, keyword counts, argmax) are compared exactly, (1) against the device's own fp32
inputs - fp32 ``floor(c / thr)`` on the host gives the same bits, the library is built without fast-math - and (2) against fp64
from the raw inputs wherever the fp64 decision has margin (``decision_margin``, ``argmax_margin``); at most EXCLUDE_CAP of a case's
rows may lack it."""
import numpy as np
import torch

from head_cases import FLOOR, U, ZERO, Report, bf16_values, keep_rows, rel_l2, row_bounds, row_errors, yard_bound  # noqa: F401

UB = 2.0 ** -8                               # unit roundoff of bf16 (8 significant bits, round to nearest)
ULP = 2.0 ** -23                             # one fp32 ulp, relative
MAXS = 2048                                  # csrc/cif.hip: frames per utterance held in LDS
EXCLUDE_CAP = 0.01
COUNT_MARGIN, ARGMAX_MARGIN = 1e-4, 1e-6


def f32(v):
    """the fp32 value of a Python number, as a Python float"""
    return float(np.float32(v))


def div32(a, b):
    """correctly rounded fp32 a / b, elementwise (tensor / tensor: no reciprocal of a scalar)"""
    a = a.float()
    return a / torch.full_like(a, b)


# =============================================================================================================== CIF: fire kernels
FIRE_SWEEP = [(1, 4), (7, 24), (64, 256), (65, 260), (129, 768), (499, 1024), (2047, 8), (2048, 4)]      # (S, C)
FIRE_THR = (1.0, 0.75, 0.7)
FIRE_T = (0, 3, 75)
FIRE_B = 4


def fire_lengths(S):
    return [S, 1, max(1, 2 * S // 3), S // 2 + 1]


def fire_case(S, C, thr):
    """alpha / csum [4, S] fp32 (csum = the fp64 scan rounded once, as sc_cif_prepare forms it), frames x [4, S, C] of values that
    bf16 holds exactly.  Padded frames weigh 0; exact zeros inside the utterances; utterance 0 holds a frame of 2.3 thr (fires
    twice); utterance 1 is one frame of 0.4 thr (never fires); utterance 3 starts thr / 2, thr / 2, thr, 2 thr: its csum lands
    exactly on thr, 2 thr and 4 thr (thr times a power of two: exact in fp32 for every thr)."""
    thr = f32(thr)
    g = torch.Generator().manual_seed(S * 131 + C * 7 + int(thr * 1000))
    lens = torch.tensor(fire_lengths(S))
    a = torch.rand(FIRE_B, S, generator=g) * (0.6 * thr)
    a = a * (torch.rand(FIRE_B, S, generator=g) > 0.15)
    a[1, 0] = 0.4 * thr
    if S >= 3:
        a[0, S // 2] = 2.3 * thr
    if int(lens[3]) >= 4:
        a[3, 0], a[3, 1], a[3, 2], a[3, 3] = thr / 2, thr / 2, thr, 2 * thr
    a = (a * (torch.arange(S)[None] < lens[:, None])).float().contiguous()
    csum = a.double().cumsum(-1).float().contiguous()
    x = bf16_values(torch.randn(FIRE_B, S, C, generator=g)).contiguous()
    return {"alpha": a, "csum": csum, "x": x, "lens": lens, "thr": thr, "S": S, "C": C, "B": FIRE_B}


def fire_grad(c, T):
    g = torch.Generator().manual_seed(c["S"] * 17 + c["C"] + T)
    return torch.randn(c["B"], T + 1, c["C"], generator=g)


def fire_indices(csum, thr, T):
    """right_s = clip(floor(c_s / thr), 0, T) with the fp32 division of the kernels, left_s = right_{s-1} (0 for s = 0)"""
    right = torch.floor(div32(csum, thr)).clamp(0, T).long()
    left = torch.cat([torch.zeros_like(right[:, :1]), right[:, :-1]], 1)
    return right, left


def fire_weights(alpha, csum, thr, T):
    """-> right, left, fire, extra, lw, rw in the dtype of ``alpha`` (the indices always from the fp32 csum)"""
    right, left = fire_indices(csum, thr, T)
    fire = right - left
    extra = (fire - 1).clamp_min(0)
    rw = torch.where(fire > 0, csum - right.to(csum.dtype) * thr, torch.zeros_like(csum))
    lw = alpha - rw - extra.to(alpha.dtype) * thr
    return right, left, fire, extra, lw, rw


def fire_matrix(lw, rw, left, right, mid, T):
    """W [B, S, T + 1]: frame s puts lw into slot left, rw into slot right and ``mid`` into the slots between"""
    B, S = lw.shape
    W = torch.zeros(B, S, T + 1, dtype=lw.dtype)
    W = W.scatter_add(2, left[..., None], lw[..., None]).scatter_add(2, right[..., None], rw[..., None])
    tt = torch.arange(T + 1)
    between = (tt > left[..., None]) & (tt < right[..., None])
    return W + between.to(lw.dtype) * mid


def fire_fwd(x, alpha, csum, thr, T):
    """out[b, t] = sum_s W[b, s, t] x[b, s]   (dtype of the arguments)"""
    right, left, _, _, lw, rw = fire_weights(alpha, csum, thr, T)
    return torch.einsum("bst,bsc->btc", fire_matrix(lw, rw, left, right, thr, T), x)


def _blocks(v):
    """[B, S, C] -> [nblk, B, S]: sums over the 256-channel blocks"""
    return torch.stack([v[..., i: i + 256].sum(-1) for i in range(0, v.shape[-1], 256)])


def fire_formula(x, alpha, csum, g, thr, T):
    """The kernel comment's formulas: out, dx = lw g[left] + rw g[right] + thr sum g[between], pa = x . g[left] and
    pb = x . (g[right] - g[left]) where the frame fires, per 256-channel block."""
    right, left, fire, _, lw, rw = fire_weights(alpha, csum, thr, T)
    W = fire_matrix(lw, rw, left, right, thr, T)
    C = x.shape[-1]
    gl = torch.gather(g, 1, left[..., None].expand(-1, -1, C))
    gr = torch.gather(g, 1, right[..., None].expand(-1, -1, C))
    fired = (fire > 0)[..., None]
    return {"out": torch.einsum("bst,bsc->btc", W, x), "dx": torch.einsum("bst,btc->bsc", W, g), "pa": _blocks(x * gl),
            "pb": _blocks(torch.where(fired, x * (gr - gl), torch.zeros_like(x)))}


def fire_autograd(x, alpha, csum, g, thr, T):
    """fp64 autograd on fire_fwd -> out, dx, d alpha (direct part: sum of pa over the blocks), d csum (sum of pb)"""
    xd, ad, cd = (t.double().requires_grad_(True) for t in (x, alpha, csum))
    out = fire_fwd(xd, ad, cd, thr, T)
    (out * g.double()).sum().backward()
    return {"out": out.detach(), "dx": xd.grad, "pa_sum": ad.grad, "pb_sum": cd.grad}


def fire_bounds(x, alpha, csum, g, thr, T):
    """Derived per-element bounds (fp64).  The weights themselves are rounded: rw = c - right thr cancels, absolute error
    u (|c| + right thr); lw = alpha - rw - extra thr adds two roundings of its operands.  They are carried through |x| and |g|.
       out   frames of the slot's run + 2 (the fma chain, the first product)
       dx    extra + 3 (lw g[left], the sum over the extra slots, the two fmas)
       pa    4 + 64 + nblk (dot4, the 64-lane LDS column sum) ; pb one more (g[right] - g[left])"""
    x, alpha, csum, g = x.double(), alpha.double(), csum.double(), g.double()
    right, left, fire, extra, lw, rw = fire_weights(alpha, csum, thr, T)
    e_rw = torch.where(fire > 0, U * (csum.abs() + right.double() * thr), torch.zeros_like(csum))
    e_lw = e_rw + 2 * U * (alpha.abs() + rw.abs() + extra.double() * thr)
    Wa = fire_matrix(lw.abs(), rw.abs(), left, right, thr, T)
    E = fire_matrix(e_lw, e_rw, left, right, 0.0, T)
    touched = fire_matrix(torch.ones_like(lw), (fire > 0).double(), left, right, 1.0, T) > 0
    run = touched.sum(1).double()                                                   # [B, T + 1]
    xa, ga = x.abs(), g.abs()
    C = x.shape[-1]
    nblk = (C + 255) // 256
    gl = torch.gather(ga, 1, left[..., None].expand(-1, -1, C))
    gr = torch.gather(ga, 1, right[..., None].expand(-1, -1, C))
    k = 4 + 64 + nblk
    bd = {"out": (run[..., None] + 2) * U * torch.einsum("bst,bsc->btc", Wa, xa) + torch.einsum("bst,bsc->btc", E, xa),
          "dx": (extra.double()[..., None] + 3) * U * torch.einsum("bst,btc->bsc", Wa, ga) + torch.einsum("bst,btc->bsc", E, ga),
          "pa": k * U * _blocks(xa * gl),
          "pb": (k + 1) * U * _blocks(torch.where((fire > 0)[..., None], xa * (gr + gl), torch.zeros_like(xa)))}
    bd["pa_sum"], bd["pb_sum"] = bd["pa"].sum(0), bd["pb"].sum(0)
    return bd


FIRE_DIMS = {"out": (2,), "dx": (2,), "pa": (), "pb": (), "pa_sum": (), "pb_sum": ()}


def fire_checks(rep, name, got, ref, yard, bounds):
    for q, v in got.items():
        rep.derived(name, q, v, ref[q], bounds[q], FIRE_DIMS[q], yard.get(q))


# =============================================================================================================== CIF: bookkeeping
def prepare_ref(a_raw, pad, target, thr, eps, scale, max_feat, T):
    """include/speechclip_hip.h, sc_cif_prepare, in the dtype of ``a_raw``"""
    dt = a_raw.dtype
    a = a_raw.clamp(0, 1) * (~pad).to(dt)
    q = a.sum(-1)
    if scale:
        pos = q > 0
        ratio = torch.where(pos, (thr * target.to(dt) + torch.tensor(eps, dtype=dt)) / torch.where(pos, q, torch.ones_like(q)),
                            torch.zeros_like(q))
    else:
        ratio = torch.ones_like(q)
    alpha = a * ratio[:, None]
    csum = alpha.cumsum(-1)
    total = alpha.sum(-1)
    cap = min(max_feat, T)
    slots = torch.floor(csum / thr).clamp(0, T)
    fired = slots > torch.cat([torch.zeros_like(slots[:, :1]), slots[:, :-1]], 1)
    return {"a_clip": a, "quantity": q, "ratio": ratio, "alpha": alpha, "csum": csum, "total": total,
            "feat_len": torch.floor(total / thr).clamp(1, cap).long(), "fired": fired}


def decision_margin(v, thr):
    """|v / thr - nearest integer| (fp64): the distance of floor(v / thr) from changing"""
    r = v.double() / thr
    return (r - torch.round(r)).abs()


def prepare_case(thr, scale, seed=0, B=6, S=200, ld=256):
    """alpha_raw as a [B, S] view of a [B, ld] buffer, pad as a view of a wider one; values outside [0, 1] (clipped), exact 0 and
    1, one all-zero utterance, padded tails, targets 1 .. 9"""
    g = torch.Generator().manual_seed(1000 + seed + int(thr * 100) + int(scale))
    buf = torch.rand(B, ld, generator=g) * 1.3 - 0.15
    buf[0, 5], buf[0, 6] = 0.0, 1.0
    buf[3, :] = -0.25
    padbuf = torch.zeros(B, ld + 8, dtype=torch.bool)
    lens = [S, S // 2, 1, S, S - 7, 33]
    for b, l in enumerate(lens):
        padbuf[b, l:] = True
    target = torch.tensor([4, 3, 1, 2, 9, 5], dtype=torch.int64)
    return {"a_raw": buf[:, :S], "pad": padbuf[:, :S], "target": target, "thr": f32(thr), "eps": f32(1e-5), "scale": scale, "B": B, "S": S,
            "T": 12, "max_feat": 75}


COUNT_S = (76, 499, 2048)
COUNT_KINDS = ("uniform", "onehot", "wide")


def count_case(S, kind, targets):
    """[len(targets), S] weights in [0, 1]: all equal, one frame only, or log-uniform over [1e-4, 1]"""
    B = len(targets)
    g = torch.Generator().manual_seed(S * 3 + COUNT_KINDS.index(kind))
    if kind == "uniform":
        a = (0.05 + 0.9 * torch.rand(B, 1, generator=g)).expand(B, S).clone()
    elif kind == "onehot":
        a = torch.zeros(B, S)
        a[torch.arange(B), torch.randint(0, S, (B,), generator=g)] = 0.05 + 0.9 * torch.rand(B, generator=g)
    else:
        a = torch.exp(torch.rand(B, S, generator=g) * float(np.log(1e4)) - float(np.log(1e4)))
    return a.float().contiguous(), torch.tensor(targets, dtype=torch.int64)


def count_fp32_total(a, target, thr=1.0, eps=1e-5):
    """The fp64 sum of the weights as sc_cif_prepare scales them in fp32: q = fp32(fp64 sum), ratio = (thr * target + eps) / q and
    a * ratio in fp32 (every operation correctly rounded: the same bits on any IEEE machine)."""
    q = a.double().sum(-1).float()
    ratio = (torch.full_like(q, f32(thr)) * target.float() + torch.full_like(q, f32(eps))) / q
    return (a * ratio[:, None]).double().sum(-1)


def count_shortfalls(a, target, thr=1.0, eps=1e-5, max_feat=75):
    """rows whose fp32-scaled weights sum (in fp64) below min(target, max_feat) thr: floor() then gives one keyword less
    whatever the kernel does - the arithmetic of the scaling, named and kept out of the count assertion"""
    want = target.clamp(0, max_feat).double() * f32(thr)      # (a target of 0 scales to eps: floor 0, clipped up to 1)
    return (count_fp32_total(a, target, thr, eps) < want).nonzero().flatten().tolist()


def prepare_bwd_formula(pa, pb, a_clip, pad, ratio, quantity, gq, scale):
    """The kernel comment: g'_i = sum_blk pa_i + sum_{j >= i} sum_blk pb_j ; scaled: da = r g' - r <g', a> / Q ; + gq ; padded 0.
    An utterance with Q <= 0 was not rescaled: no term through the scaling."""
    ga, gc = pa.sum(0), pb.sum(0)
    gp = ga + gc.flip(-1).cumsum(-1).flip(-1)
    r = ratio[:, None]
    corr = torch.zeros_like(gp[:, :1])
    if scale:
        pos = quantity > 0
        corr = torch.where(pos, (gp * a_clip).sum(-1) * ratio / torch.where(pos, quantity, torch.ones_like(quantity)),
                           torch.zeros_like(quantity))[:, None]
    da = r * gp - corr + (gq[:, None] if gq is not None else 0.0)
    return da * (~pad).to(da.dtype)


def prepare_bwd_autograd(a_raw, pad, target, thr, eps, scale, ga, gc, gq):
    """fp64 autograd through clip -> mask -> quantity -> scaling -> cumsum of  sum alpha ga + sum csum gc + sum quantity gq"""
    ar = a_raw.double().clone().requires_grad_(True)
    r = prepare_ref(ar, pad, target, thr, eps, scale, 75, 75)
    L = (r["alpha"] * ga.double()).sum() + (r["csum"] * gc.double()).sum()
    if gq is not None:
        L = L + (r["quantity"] * gq.double()).sum()
    L.backward()
    return ar.grad, {k: v.detach() for k, v in r.items()}


def prepare_bwd_bound(pa, pb, a_clip, pad, ratio, quantity, gq, scale):
    """g' = nblk fp32 adds of pa + the fp64 suffix sum of (nblk adds of pb) rounded once + 1 add; corr = fp64 <g', a> r / Q (three
    roundings, r and Q rounded inputs); r g' - corr + gq: three more."""
    pa, pb, a, ratio, quantity = pa.double(), pb.double(), a_clip.double(), ratio.double(), quantity.double()
    nblk = pa.shape[0]
    ga, gc = pa.sum(0), pb.sum(0)
    suf = gc.flip(-1).cumsum(-1).flip(-1)
    suf_abs = pb.abs().sum(0).flip(-1).cumsum(-1).flip(-1)
    gp = ga + suf
    e_g = nblk * U * (pa.abs().sum(0) + suf_abs) + U * suf.abs() + U * gp.abs()
    r = ratio.abs()[:, None]
    e = r * e_g + 4 * U * (r * gp.abs())
    if scale:
        pos = quantity > 0
        qs = torch.where(pos, quantity, torch.ones_like(quantity))
        corr = torch.where(pos, (gp * a).sum(-1) * ratio / qs, torch.zeros_like(qs))
        e_corr = torch.where(pos, (e_g * a).sum(-1) * ratio.abs() / qs, torch.zeros_like(qs)) + 6 * U * corr.abs()
        e = e + (e_corr + 2 * U * corr.abs())[:, None]
    if gq is not None:
        e = e + 2 * U * gq.double().abs()[:, None]
    return e * (~pad).double()


def prepare_bwd_case(nblk, scale, with_gq, B=5, S=203, seed=0):
    """a_raw inside [0, 1] with exact 0 and 1 (the precondition of sc_cif_prepare_bwd); utterance 2 all zero"""
    g = torch.Generator().manual_seed(77 + nblk * 10 + int(scale) * 3 + int(with_gq) + seed)
    a_raw = torch.rand(B, S, generator=g)
    a_raw[0, 3], a_raw[0, 4], a_raw[1, 0] = 0.0, 1.0, 1.0
    a_raw[2] = 0.0
    pad = torch.zeros(B, S + 5, dtype=torch.bool)
    for b, l in enumerate([S, S - 1, S, 9, S // 2]):
        pad[b, l:] = True
    return {"a_raw": a_raw, "pad": pad[:, :S], "target": torch.tensor([7, 2, 3, 1, 30], dtype=torch.int64),
            "pa": torch.randn(nblk, B, S, generator=g), "pb": torch.randn(nblk, B, S, generator=g) * 0.3,
            "gq": torch.randn(B, generator=g) if with_gq else None, "thr": 1.0, "eps": f32(1e-5), "scale": scale, "zero_row": 2}


def tail_ref(alpha, csum, out, feat_len, thr, tail_thr, max_feat, T):
    """sc_cif_tail in the dtype of ``alpha``: the weight left in slot feat_len; >= tail_thr: that row *= thr / weight and the count
    grows by one (clipped at max_feat); rows >= the final count are zero."""
    right, left, _, _, lw, rw = fire_weights(alpha, csum, thr, T)
    fl = feat_len[:, None]
    tw = (torch.where(right == fl, rw, torch.zeros_like(rw)) + torch.where(left == fl, lw, torch.zeros_like(lw))).sum(-1)
    ext = tw >= tail_thr
    f = torch.where(ext, thr / torch.where(ext, tw, torch.ones_like(tw)), torch.ones_like(tw))
    fl_new = (feat_len + ext.long()).clamp_max(max_feat)
    o = out.clone()
    for b in range(o.shape[0]):
        if bool(ext[b]) and int(feat_len[b]) <= T:
            o[b, int(feat_len[b])] = o[b, int(feat_len[b])] * f[b]
        o[b, int(fl_new[b]):] = 0
    return {"tw": tw, "factor": f, "extend": ext, "feat_len": fl_new, "out": o}


def tail_case(T, tail_thr=0.5, margin=1e-3, S=40, C=12):
    """thr = 1; utterance b: ``n`` frames of 0.5 (n / 2 keywords), then 0.25 and a last frame that leaves tail_thr -/+ margin in
    the open slot.  T = 75 adds an utterance of 200 x 0.5 whose count is already 75; T small adds one whose count is T."""
    thr = 1.0
    rows = []
    for n, sign in ((4, -1), (4, +1), (10, -1), (2, +1)):
        a = torch.zeros(S if T < 75 else 200)
        a[:n] = 0.5
        a[n], a[n + 1] = 0.25, tail_thr - 0.25 + sign * margin
        rows.append((a, n // 2))
    a = torch.full_like(rows[0][0], 0.5)                     # fills every slot: the count equals min(T, 75)
    rows.append((a, min(T, 75)))
    alpha = torch.stack([r[0] for r in rows]).float().contiguous()
    csum = alpha.double().cumsum(-1).float().contiguous()
    feat_len = torch.tensor([r[1] for r in rows], dtype=torch.int64)
    x = torch.randn(alpha.shape[0], alpha.shape[1], C, generator=torch.Generator().manual_seed(T))
    out = fire_fwd(x.double(), alpha.double(), csum.double(), thr, T).float().contiguous()
    return {"alpha": alpha, "csum": csum, "feat_len": feat_len, "out": out, "thr": thr, "tail_thr": tail_thr, "T": T, "max_feat": 75}


# =============================================================================================================== CIF: weight head
HEAD_SHAPES = [(1, 4), (5, 260), (777, 768), (130, 1024)]               # (rows, C)
HEAD_P = [(0.0, 0.0), (0.5, 0.5), (0.1, 0.0)]
HEAD_SEEDS = (1234, 98765)
HEAD_NBLK = 8


def whead_case(rows, C):
    g = torch.Generator().manual_seed(rows * 13 + C)
    return {"y": torch.randn(rows, C, generator=g), "w": torch.randn(C, generator=g) * C ** -0.5, "b": torch.tensor([0.3]),
            "dalpha": torch.randn(rows, generator=g), "rows": rows, "C": C}


def whead_masks(rows, C, p1, p2, dtype):
    m = lambda p, sd: keep_rows(rows, C, sd, p).to(dtype) / (1.0 - p) if p > 0 else torch.ones(rows, C, dtype=dtype)
    return m(p1, HEAD_SEEDS[0]), m(p2, HEAD_SEEDS[1])


def whead_fwd(y, w, b, m1, m2):
    """alpha[row] = sigmoid(b + sum_c w[c] m2 relu(m1 y[row, c]))"""
    return torch.sigmoid((torch.relu(y * m1) * m2) @ w + b)


def whead_bwd_formula(y, w, alpha, dalpha, m1, m2):
    """g = dalpha a (1 - a) ; dy = g w m2 m1 [m1 y > 0] ; dw = sum_rows g m2 relu(m1 y) ; db = sum g"""
    gg = dalpha * alpha * (1 - alpha)
    h = torch.relu(y * m1)
    return {"dy": torch.where(h > 0, gg[:, None] * w[None] * m2 * m1, torch.zeros_like(h)), "dw": (gg[:, None] * m2 * h).sum(0),
            "db": gg.sum().reshape(1)}


def whead_autograd(c, p1, p2):
    y, w, b = (c[k].double().requires_grad_(True) for k in ("y", "w", "b"))
    m1, m2 = whead_masks(c["rows"], c["C"], p1, p2, torch.float64)
    a = whead_fwd(y, w, b, m1, m2)
    a.backward(c["dalpha"].double())
    return {"alpha": a.detach(), "dy": y.grad, "dw": w.grad, "db": b.grad}


def whead_sum_bounds(c, alpha, p1, p2, nblk=HEAD_NBLK, chain=None):
    """dw / db as the fp64 sum of the kernel's nblk partials: a wave adds ceil(rows / (4 nblk)) rows in order, 2 levels over the
    four waves; g = dalpha a (1 - a) (3 roundings) on a rounded alpha (1), h = relu(m1 y) with the rounded 1 / (1 - p1) (2), the
    rounded 1 / (1 - p2) (1), the product g m2 h (2).  ``chain``: the longest chain of additions instead of the kernel's (the CPU
    module's plain fp32 sum over all rows: ``rows`` at the worst)."""
    m1, m2 = whead_masks(c["rows"], c["C"], p1, p2, torch.float64)
    a, da = alpha.double(), c["dalpha"].double()
    gg = (da * a * (1 - a)).abs()
    k = (-(-c["rows"] // (4 * nblk)) + 2 if chain is None else chain) + 9
    h = torch.relu(c["y"].double() * m1)
    return {"dw": k * U * (gg[:, None] * m2 * h).sum(0), "db": (k * U * gg.sum()).reshape(1)}


ZERO_PAD_CASES = [(0, 0, 1, 0, 1, 3, 8), (2, 3, 10, 1, 7, 0, 8), (1, 2, 6, 0, 6, 2, 768), (0, 4, 9, 2, 9, 1, 768), (3, 1, 5, 0, 5, 0, 8),
                  (0, 2, 7, 3, 5, 0, 24)]                    # (lead, B, P, head, stop, trail, D)


def zero_pad_rows(lead, B, P, head, stop, trail):
    """bool [lead + B P + trail]: the rows sc_rows_zero_pad_bf16 clears"""
    z = torch.zeros(lead + B * P + trail, dtype=torch.bool)
    z[:lead] = True
    for b in range(B):
        z[lead + b * P: lead + b * P + head] = True
        z[lead + b * P + stop: lead + (b + 1) * P] = True
    if trail:
        z[lead + B * P:] = True
    return z


# =============================================================================================================== quantiser
PREP_SHAPES = [(1, 4), (37, 48), (64, 64), (65, 130), (300, 512)]                    # (Nk, Et)
VQ_EPS = 1e-8


def vq_prep_case(Nk, Et):
    g = torch.Generator().manual_seed(Nk * 5 + Et)
    buf = torch.randn(Nk, Et + 4, generator=g)
    if Nk >= 3:
        buf[1] = 0.0
        buf[2] = 1e-10 * torch.randn(Et + 4, generator=g)
    return buf[:, :Et]


def vq_prep_ref(kw, eps=VQ_EPS):
    """rnorm = 1 / max(|kw|, eps), rows kw rnorm"""
    rn = 1.0 / kw.norm(dim=-1).clamp_min(torch.tensor(eps, dtype=kw.dtype))
    return {"rnorm": rn, "kwn": kw * rn[:, None]}


ROWSTATS_V = (5, 205, 256, 257, 1000)
ROWSTATS_TEMP = (0.1, 1.0, 0.03)
ROWSTATS_MASKS = ((0, 2, 3), (), (0,))
ROWSTATS_NK = 24


def rowstats_case(V, seed=0):
    """x64 [Nk, V]: cosine-like scores in fp64 (the raw input), x = its fp32 rounding (what the kernel reads), in a buffer with
    ldx > V.  Row 0: the raw maximum sits in column 0 (masked by two of the three mask sets); row 1: two bit-equal maxima in
    columns 1 and 4 (live under every mask set, distinct at every V); row 2: every column equal."""
    g = torch.Generator().manual_seed(V * 9 + seed)
    x64 = (torch.rand(ROWSTATS_NK, V, generator=g, dtype=torch.float64) * 2 - 1) * 0.9
    x64[0, 0] = 0.99
    x64[1, 1] = x64[1, 4] = 0.9375
    x64[2] = 0.25
    return x64


def first_argmax(x):
    """first index of the row maximum"""
    V = x.shape[-1]
    return torch.where(x == x.amax(-1, keepdim=True), torch.arange(V).expand_as(x), torch.full_like(x, V, dtype=torch.int64)).amin(-1)


def mask_cols(x, cols):
    x = x.clone()
    for c in cols:
        if 0 <= c < x.shape[-1]:
            x[:, c] = float("-inf")
    return x


def argmax_margin(x64):
    """rows whose fp64 argmax is decided: a top-2 gap above ARGMAX_MARGIN, or an exact tie (decided by the index in any precision
    that keeps the tie)"""
    if x64.shape[-1] < 2:
        return torch.ones(x64.shape[0], dtype=torch.bool)
    top = x64.topk(2, dim=-1).values
    gap = top[:, 0] - top[:, 1]
    return (gap > ARGMAX_MARGIN) | (gap == 0)


def rowstats_ref(xm, temp):
    """The kernel's three passes in the dtype of ``xm`` (masked columns already -inf), with exp / log of the library:
    lse_t = m / temp + log sum exp((x - m) / temp), lse_1 = m + log sum exp(x - m), ent = - sum p log(p + 1e-9), p = exp(x - lse_1)"""
    dt = xm.dtype
    inv = torch.tensor(1.0, dtype=dt) / torch.tensor(f32(temp), dtype=dt)
    m = xm.amax(-1, keepdim=True)
    d = xm - m
    lse_t = (m * inv + torch.log(torch.exp(d * inv).sum(-1, keepdim=True)))[:, 0]
    lse_1 = (m + torch.log(torch.exp(d).sum(-1, keepdim=True)))[:, 0]
    p = torch.exp(xm - lse_1[:, None])
    ent = -(p * torch.log(p + torch.tensor(1e-9, dtype=dt))).sum(-1)
    return {"idx": first_argmax(xm), "lse_t": lse_t, "lse_1": lse_1, "ent": ent}


ENT_FEW_ROWS = (5, 8112)       # (Nk, V) of tests/test_gpu_poison_kw.py at which the rows of ``ent`` may meet rowstats_ent_bound


def rowstats_ent_bound(xm):
    """Absolute bound [Nk] of sc_vq_rowstats' ent = -sum_v p log(p + 1e-9), p = exp(x - l), l = LSE(x), with the per-term figures of
    ``perplexity_bound`` (the same fast exp / log on a sum of size log V): p carries U (2 |x - l| + |l| + 2) from its own evaluation and,
    l being formed inside the kernel, U (|l| + ceil(V / 256) + 8) more from l's rounding and the 256-lane sum + trees behind it - with
    the same sign on every term of a row, which the yardstick (one sample per row, with its own l) shows only over many rows; the
    logarithm 3 U |log| + U; the accumulation ceil(V / 256) + 8 additions + 1 product on sum p |log|.  For the shape ENT_FEW_ROWS
    only: every other case keeps the yardstick rule alone."""
    x = xm.double()
    V = x.shape[1]
    l = torch.logsumexp(x, -1, keepdim=True)
    arg = x - l
    p = torch.exp(arg)
    k = -(-V // 256) + 8
    eps = torch.where(p > 0, U * (2 * arg.abs() + 2 * l.abs() + k + 2), torch.zeros_like(p))
    la = torch.log(p + 1e-9).abs()
    return (p * eps * (la + 1) + p * (3 * U * la + U) + (k + 1) * U * p * la).sum(-1)


def perplexity_ref(xm, idx, lse_1):
    """code_perplexity = exp(-sum hp log(hp + 1e-7)), hp = histogram(idx) / Nk ; prob_perplexity the same of ap = mean_n exp(x - lse_1)"""
    dt = xm.dtype
    Nk, V = xm.shape
    hp = torch.bincount(idx, minlength=V).to(dt) / Nk
    ap = torch.exp(xm - lse_1[:, None]).sum(0) / Nk
    e7 = torch.tensor(1e-7, dtype=dt)
    return torch.stack([torch.exp(-(hp * torch.log(hp + e7)).sum()), torch.exp(-(ap * torch.log(ap + e7)).sum())])


def perplexity_bound(xm, idx, lse_1, nchunk):
    """Relative bounds [2] of the two perplexities exp(-H), H = sum_v a log(a + 1e-7): the relative error of exp(-H) is the
    ABSOLUTE error of H, a sum of magnitude log V whose terms carry __logf's error with one sign (v_log_f32 on log2 a, one ulp of
    |log2 a|, times ln 2), and __expf rounds H log2(e) once more - neither averages out as the yardstick's correctly rounded log
    over V terms does.  Derived (fp64):
       a (prob)  exp(x - lse_1): eps_e = u (2 |x - l| + |l| + 2) per term (the difference, the rounded l given, the scaled argument,
                 the instruction); a chunk adds ceil(Nk / nchunk) terms in order, nchunk partials in order, 1 / Nk: + 3
       a (code)  an exact count times the rounded 1 / Nk: 2 u
       log       3 u |log a| + u (the instruction and its product with ln 2; a + 1e-7)
       sum       ceil(V / (1024 nw)) + 6 + 16 + nw additions, + 1 product
       exp(-H)   u (|H| + 2)"""
    x, l = xm.double(), lse_1.double()[:, None]
    Nk, V = x.shape
    nw = min(-(-V // 1024), 32)
    k_sum = -(-V // (1024 * nw)) + 6 + 16 + nw + 1
    arg = x - l
    p = torch.exp(arg)
    eps_e = torch.where(p > 0, U * (2 * arg.abs() + l.abs() + 2), torch.zeros_like(p))
    rpc = -(-Nk // nchunk)
    ap = p.sum(0) / Nk
    e_ap = ((p * eps_e).sum(0) + (rpc + nchunk + 3) * U * p.sum(0)) / Nk
    hp = torch.bincount(idx, minlength=V).double() / Nk
    out = []
    for a, e_a in ((hp, 2 * U * hp), (ap, e_ap)):
        la = torch.log(a + 1e-7).abs()
        e_H = (e_a * (la + 1) + a * (3 * U * la + U) + k_sum * U * a * la).sum()
        H = (a * la).sum()
        out.append(e_H + U * (H + 2))
    return torch.stack(out)


def soft_bwd_formula(xm, lse_t, t, temp):
    """dx = s (t - <s, t>) / temp, s = exp(x / temp - lse_t); masked columns (s = 0) contribute nothing whatever t holds"""
    dt = xm.dtype
    inv = torch.tensor(1.0, dtype=dt) / torch.tensor(f32(temp), dtype=dt)
    s = torch.exp(xm * inv - lse_t[:, None])
    live = s > 0
    tz = torch.where(live, t, torch.zeros_like(t))
    m = (s * tz).sum(-1, keepdim=True)
    return torch.where(live, s * (tz - m) * inv, torch.zeros_like(s))


def soft_bwd_bound(xm, lse_t, t, temp):
    """t - <s, t> cancels where one column holds nearly all of the softmax (s = 1 - 1e-8 at a score gap of 1.8 and temp 0.1): the
    difference is then a rounding of t, against a true value of (1 - s) (t - t'), in any fp32 form of the formula - the yardstick's
    too, of which it is one sample.  Derived per element (fp64):
       s        relative error eps_s = u (|x / temp| + |x / temp - lse_t| + |lse_t| + 4): the rounded 1 / temp, the fma, the rounded
                lse_t the kernel is given, __expf on the scaled argument
       <s, t>   a thread adds ceil(V / 256) products in order, six shuffle levels, the four waves in order: k = ceil(V / 256) + 6 + 4 + 1
       dx       s (e_dot + 2 u (|t| + |dot|)) / temp + (eps_s + 3 u) |dx|"""
    inv = 1.0 / f32(temp)
    x, l, t = xm.double(), lse_t.double()[:, None], t.double()
    arg = x * inv - l
    s = torch.exp(arg)
    live = s > 0
    tz = torch.where(live, t, torch.zeros_like(t))
    eps_s = torch.where(live, U * ((x * inv).abs() + arg.abs() + l.abs() + 4), torch.zeros_like(s))
    k = -(-xm.shape[-1] // 256) + 6 + 4 + 1
    m = (s * tz).sum(-1, keepdim=True)
    e_m = k * U * (s * tz).abs().sum(-1, keepdim=True) + (s * eps_s * tz.abs()).sum(-1, keepdim=True)
    dx = s * (tz - m) * inv
    return inv * s * (e_m + 2 * U * (tz.abs() + m.abs())) + (eps_s + 3 * U) * dx.abs()


SOFT_CANCEL = 0.75


def soft_bwd_cancel_rows(xm, lse_t, temp):
    """[Nk] bool: rows whose largest softmax weight exceeds SOFT_CANCEL.  There t - <s, t> is (1 - s_max) of its operands: every
    rounding of the formula is amplified by 1 / (1 - s_max) > 4 in ANY fp32 form of it, so the yardstick's figure on such a row
    is one sample of that amplification, not a yardstick.  These rows are held to soft_bwd_bound alone; all other rows to the
    yardstick rule with the yardstick taken over those other rows only."""
    s = torch.exp(xm.double() / f32(temp) - lse_t.double()[:, None])
    return s.amax(-1) > SOFT_CANCEL


def soft_bwd_check(rep, name, tag, got, auto, yard, own, cancel, extra=0.0):
    """One PARITY line per group of rows.  ``extra``: one more rounding of the output (bf16), relative to the row's largest entry."""
    e, ey, ob = row_errors(got, auto, (1,)), row_errors(yard, auto, (1,)), row_bounds(own, auto, (1,))
    keep = ~cancel
    if bool(keep.any()):
        y = float(ey[keep].max())
        rep._line(name, tag + f" ({int(keep.sum())} rows, yardstick rule)", float(e[keep].max()), y, yard_bound(y) + extra)
    if bool(cancel.any()):
        r = e[cancel] / (ob[cancel] + extra)
        i = int(r.argmax())
        rep._line(name, tag + f" ({int(cancel.sum())} cancelling rows, derived)", float(e[cancel][i]), float(ey[cancel][i]),
                  float(ob[cancel][i]) + extra)


# --- perplexity cases of their own: the chunking of sc_vq_perplexity depends on Nk
PERP_NK = (1, 17, 300)
PERP_V = 333                                 # two 256-column blocks, the second partial; >= 300 so that every row can hold its own token
PERP_HIST = ("argmax", "one token", "all different")


def perplexity_chunks(Nk):
    """(16, a count above Nk)"""
    return (16, Nk + 3)


def perplexity_case(Nk, V=PERP_V, cols=(0, 2, 3)):
    """-> xm [Nk, V] fp32 scores with the masked columns -inf, lse_1 [Nk] (fp64, rounded once), the three index sets"""
    g = torch.Generator().manual_seed(Nk * 11 + V)
    xm = mask_cols(((torch.rand(Nk, V, generator=g, dtype=torch.float64) * 2 - 1) * 0.9).float(), cols)
    r = rowstats_ref(xm.double(), 1.0)
    live = [v for v in range(V) if v not in cols]
    idx = {"argmax": r["idx"], "one token": torch.full((Nk,), V - 1), "all different": torch.tensor(live[:Nk])}
    return xm, r["lse_1"].float(), idx


def soft_bwd_autograd(xm, t, temp):
    """fp64 autograd of softmax(x / temp) over the live columns under the upstream t"""
    live = torch.isfinite(xm[0])
    xl = xm[:, live].double().requires_grad_(True)
    s = torch.softmax(xl / f32(temp), dim=-1)
    s.backward(t[:, live].double())
    dx = torch.zeros(xm.shape, dtype=torch.float64)
    dx[:, live] = xl.grad
    return dx


def norm_bwd_formula(kw, rnorm, dy, eps=VQ_EPS):
    """y = x r, r = 1 / max(|x|, eps): dx = r (dy - y <y, dy>), and dy / eps where the norm is clamped"""
    y = kw * rnorm[:, None]
    dot = (y * dy).sum(-1, keepdim=True)
    clamped = (rnorm >= 1.0 / torch.tensor(eps, dtype=kw.dtype))[:, None]
    return torch.where(clamped, dy * rnorm[:, None], rnorm[:, None] * (dy - y * dot))


def norm_bwd_autograd(kw, dy, eps=VQ_EPS):
    x = kw.double().requires_grad_(True)
    (x / x.norm(dim=-1, keepdim=True).clamp_min(eps)).backward(dy.double())
    return x.grad


# =============================================================================================================== BatchNorm
BN_SHAPES = [(2, 8), (45, 70), (128, 16), (129, 9), (1600, 64)]                      # (N, E)
BN_EPS, BN_MOM, BN_RL = 1e-5, 0.1, 128


def bn_case(N, E):
    """channel 0: mean 100, unit variance; channel 1: constant 3"""
    g = torch.Generator().manual_seed(N * 3 + E)
    x = torch.randn(N, E, generator=g) * (0.5 + torch.rand(E, generator=g)) + torch.randn(E, generator=g)
    x[:, 0] = 100.0 + torch.randn(N, generator=g)
    x[:, 1] = 3.0
    return {"x": x, "x2": torch.randn(N, E, generator=g) + 0.5, "dy": torch.randn(N, E, generator=g), "gamma": 1 + 0.2 * torch.randn(E, generator=g),
            "beta": 0.3 * torch.randn(E, generator=g), "rm0": 0.1 * torch.randn(E, generator=g), "rv0": 0.5 + torch.rand(E, generator=g),
            "N": N, "E": E}


def bn_train_ref(x, gamma, beta, rm, rv, eps=BN_EPS, mom=BN_MOM):
    """nn.BatchNorm1d in training mode over the rows of x [N, E] -> y, save_mean, save_rstd, the updated running estimates"""
    N = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    rstd = (var + eps).rsqrt()
    y = (x - mean) * rstd * gamma + beta
    return {"y": y, "save_mean": mean, "save_rstd": rstd, "run_mean": (1 - mom) * rm + mom * mean,
            "run_var": (1 - mom) * rv + mom * var * (N / max(N - 1, 1))}


def bn_eval_ref(x, gamma, beta, rm, rv, eps=BN_EPS):
    return (x - rm) * (rv + eps).rsqrt() * gamma + beta


def bn_bwd_formula(x, dy, gamma, mean, rstd):
    """dx = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)) ; dgamma = sum dy xhat ; dbeta = sum dy"""
    xh = (x - mean) * rstd
    dg, db = (dy * xh).sum(0), dy.sum(0)
    N = x.shape[0]
    return {"dx": gamma * rstd * (dy - db / N - xh * (dg / N)), "dgamma": dg, "dbeta": db}


def bn_autograd(c):
    x, gamma, beta = (c[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
    r = bn_train_ref(x, gamma, beta, c["rm0"].double(), c["rv0"].double())
    r["y"].backward(c["dy"].double())
    return {"dx": x.grad, "dgamma": gamma.grad, "dbeta": beta.grad}


def bn_sum_bounds(c, mean32, rstd32):
    """A row lane adds ceil(N / 128) rows in order, lane 0 the 128 lanes, + 1 (the division by N, or the product): k u sum |.|.
    dgamma also carries the rounding of xhat = (x - mean) rstd formed from the rounded save_mean / save_rstd the kernel is given:
    u (|x| + |mean|) rstd + 2 u |xhat|."""
    N = c["N"]
    k = -(-N // BN_RL) + BN_RL + 1
    x, dy = c["x"].double(), c["dy"].double()
    mean, rstd = mean32.double(), rstd32.double()
    xh = (x - mean) * rstd
    e_xh = U * (x.abs() + mean.abs()) * rstd + 2 * U * xh.abs()
    return {"save_mean": k * U * x.abs().sum(0) / N, "dbeta": k * U * dy.abs().sum(0),
            "dgamma": (k + 1) * U * (dy * xh).abs().sum(0) + (dy.abs() * e_xh).sum(0)}


def bn_run_mean_bound(c, mom=BN_MOM):
    """run_mean after the two steps on x and x2: new = (1 - mom) old + mom mean, three roundings a step on |(1 - mom) old| + |mom mean|
    (the rounded 1 - mom and mom, the products, the sum), the error of the means (bn_sum_bounds' k) and of the previous step
    carried through.  A channel whose two terms cancel has no relative accuracy: the bound is absolute."""
    N = c["N"]
    k = -(-N // BN_RL) + BN_RL + 1
    mag, err = c["rm0"].double().abs(), torch.zeros(c["E"], dtype=torch.float64)
    for key in ("x", "x2"):
        x = c[key].double()
        e_mean = k * U * x.abs().sum(0) / N
        mag = (1 - mom) * mag + mom * x.mean(0).abs()
        err = 3 * U * mag + (1 - mom) * err + mom * e_mean
    return err


BN_FOLD = 2.0


def bn_fold_rows(mean, rstd):
    """[E] bool: channels whose mean lies more than BN_FOLD standard deviations from zero.  There x g and mean g of the folded
    y = fma(x, g, b) are each more than BN_FOLD times the normalised value they leave: the channels bn_y_bound is meant for."""
    return mean.double().abs() * rstd.double() > BN_FOLD


def bn_y_bound(x, gamma, beta, mean, rstd):
    """The kernel folds the normalisation into y = fma(x, g, b), g = gamma rstd, b = beta - mean g: where |mean| is large against
    the spread (or the channel is constant) x g and mean g cancel, which (x - mean) rstd gamma + beta - the yardstick - does not
    do.  Roundings: g (1), mean g (2), beta - mean g (1), the fma (1), rstd itself to a few ulp (8 u on the part it scales)."""
    x, gamma, beta, mean, rstd = (t.double() for t in (x, gamma, beta, mean, rstd))
    g = (gamma * rstd).abs()
    return 4 * U * (x.abs() + mean.abs()) * g + 2 * U * beta.abs() + 8 * U * ((x - mean) * rstd * gamma).abs()


# =============================================================================================================== softmax
SOFTMAX_N = (4, 72, 256, 260, 512, 516, 768, 1024)
SOFTMAX_SCALE = (0.37, 0.0361)
SOFTMAX_LONG = (66000, 8)
SOFTMAX_RPB, SOFTMAX_NB, SOFTMAX_SEED = 5, 5, 0x51f15e


def softmax_case(n, scale, rows=None):
    """rows_per_batch = 5 (no multiple of the four waves of a workgroup); batch 1 fully masked, batch 2 with one live key, every
    other batch with at least one; the scores span +-30 (the arguments of exp stay above -23 at either scale)"""
    nb = SOFTMAX_NB if rows is None else rows // SOFTMAX_RPB
    rows = nb * SOFTMAX_RPB
    g = torch.Generator().manual_seed(n * 7 + int(scale * 1e4) + rows)
    scores = (torch.rand(rows, n, generator=g) * 2 - 1) * 30.0
    mask = torch.rand(nb, n, generator=g) < 0.3
    mask[0, n // 2] = False
    mask[1] = True
    mask[2] = True
    mask[2, n - 1] = False
    for b in range(3, nb):
        mask[b, (b * 7) % n] = False
    return {"scores": scores.contiguous(), "mask": mask.contiguous(), "scale": f32(scale), "rows": rows, "n": n, "nb": nb,
            "dP": torch.randn(rows, n, generator=g)}


def softmax_ref(scores, mask, rpb, scale):
    """P = softmax(scale * scores | key mask) with exp (dtype of ``scores``); a fully masked row is all zero"""
    mrow = mask.repeat_interleave(rpb, dim=0)
    v = (scores * scale).masked_fill(mrow, float("-inf"))
    mx = v.amax(-1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp(v - mx)
    s = e.sum(-1, keepdim=True)
    return e * torch.where(s > 0, 1.0 / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))


def softmax_keep(rows, n, p, seed=SOFTMAX_SEED):
    return keep_rows(rows, n, seed, p) if p > 0 else torch.ones(rows, n, dtype=torch.bool)


def softmax_bwd_formula(dP, P, scale, keep, p):
    """dS = scale P (dP' - sum_k P dP'), dP' = keep dP / (1 - p)"""
    gp = torch.where(keep, dP * torch.tensor(1.0 / (1.0 - p), dtype=dP.dtype), torch.zeros_like(dP))
    return scale * P * (gp - (P * gp).sum(-1, keepdim=True))


def softmax_bwd_autograd(scores, mask, rpb, scale, dP, keep, p):
    """fp64 autograd through softmax(scale s | mask) and the dropout multiplier -> (P, dS)"""
    s = scores.double().requires_grad_(True)
    P = softmax_ref(s, mask, rpb, scale)
    (P * keep.double() / (1.0 - p) * dP.double()).sum().backward()
    return P.detach(), s.grad


def softmax_bwd_bound(dP, P, scale, keep, p):
    """dot = sum P dP': a lane's fma chain over its <= 16 values, 6 shuffle levels, + 1 product, + 1 (dP' = dP / (1 - p));
    dP' - dot, the two products with P and scale: u each; the store rounds to bf16."""
    dP, P = dP.double(), P.double()
    gp = torch.where(keep, dP / (1.0 - p), torch.zeros_like(dP))
    n = P.shape[-1]
    k = 4 * ((n // 4 + 63) // 64) + 6 + 2
    dot = (P * gp).sum(-1, keepdim=True)
    e_dot = k * U * (P * gp).abs().sum(-1, keepdim=True)
    dS = scale * P * (gp - dot)
    return scale * P * (e_dot + 2 * U * (gp.abs() + dot.abs())) + (3 * U + UB) * dS.abs()
