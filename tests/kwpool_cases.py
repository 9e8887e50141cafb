"""Inputs and fp64 restatements for the fixed-keyword cascaded branch (csrc/kwpool.hip, the eachKw BatchNorm, the branch head).

``pool_ref``: the constant-query pooling in double, the backward by autograd on that forward.  ``branch_ref``: the K keyword rows
of LN(MHA([cls ; frames]) + .) through nn.MultiheadAttention in double - the full-sequence form the pooled one replaces.
``bn_ref``: the fixed-count BatchNorm through F.batch_norm on the reference's permuted view.

Criterion of the kernel tests: relative L2 error against fp64 <= FP32_BOUND per group of a quantity - per (utterance, query) for
p / m / psum, per utterance for dX (it sums the queries), per query for da / dc (they sum the utterances).  FP32_BOUND = 2e-4 is the
project's stated bound for fp32 kernels (docs/parity.md); a bf16 dX additionally carries one rounding of 2^-8."""
import torch

FP32_BOUND = 2e-4
BF16_ROUND = 2.0 ** -8

KERNEL_D = (768, 1024)
KERNEL_QC = ((8, 8), (9, 9), (1, 1), (16, 16))
KERNEL_R = (128, 200)
KERNEL_ROW0 = (0, 1)


def pool_case(D, Q, C, R, row0, seed=0, peaked=False):
    """B = 4 utterances with flen = 0, 1, 65, R - row0.  X is bf16-representable; scores a . X ~ N(0, 1.5^2).  ``peaked``: the scores
    of query 0 (constant keys included) are stretched to span +-60."""
    g = torch.Generator().manual_seed(1000 * seed + D + 17 * Q + 3 * R + row0)
    B = 4
    X = torch.randn(B, R, D, generator=g).to(torch.bfloat16).float()
    a = torch.randn(Q, D, generator=g) * (1.5 / D ** 0.5)
    crow = torch.randn(C, D, generator=g)
    flen = torch.tensor([0, 1, 65, R - row0], dtype=torch.int32)
    if peaked:
        s = torch.cat([a[0] @ crow.t(), (X[3, row0:] @ a[0])])
        a[0] *= 60.0 / s.abs().max()
    c = (a.double() @ crow.double().t()).float()
    dm = torch.randn(B, Q, D, generator=g)
    cbias = torch.randn(B, Q, generator=g)
    keep = (torch.rand(B, Q, C + R, generator=g) >= 0.25).float()
    mult = keep / 0.75
    return {"B": B, "R": R, "D": D, "Q": Q, "C": C, "row0": row0, "X": X, "a": a, "c": c, "crow": crow, "flen": flen, "dm": dm,
            "cbias": cbias, "mult": mult}


def valid_mask(case):
    """[B, C + R] bool: the keys of an utterance (C constant keys, then the frame rows)."""
    B, R, C, row0 = case["B"], case["R"], case["C"], case["row0"]
    r = torch.arange(R)[None]
    fl = case["flen"].long()[:, None]
    return torch.cat([torch.ones(B, C, dtype=torch.bool), (r >= row0) & (r < row0 + fl)], 1)


def pool_ref(case, mult=None, cbias=None, dtype=torch.float64, X=None):
    """-> dict p, m, psum, dX, da, dc in ``dtype`` (gradients of sum(m dm) + sum(psum cbias))."""
    X = (case["X"] if X is None else X).to(dtype).clone()
    valid = valid_mask(case)
    X = torch.where(valid[:, case["C"]:, None], X, torch.zeros((), dtype=dtype)).requires_grad_(True)       # rows outside the frames: not inputs
    a = case["a"].to(dtype).clone().requires_grad_(True)
    c = case["c"].to(dtype).clone().requires_grad_(True)
    crow = case["crow"].to(dtype)
    B = case["B"]
    s = torch.cat([c[None].expand(B, -1, -1), torch.einsum("qd,brd->bqr", a, X)], 2)
    s = s.masked_fill(~valid[:, None], float("-inf"))
    p = torch.softmax(s, -1)
    w = p if mult is None else p * mult.to(dtype)
    C = case["C"]
    m = w[..., :C] @ crow + torch.einsum("bqr,brd->bqd", w[..., C:], X)
    psum = w.sum(-1)
    loss = (m * case["dm"].to(dtype)).sum()
    if cbias is not None:
        loss = loss + (psum * cbias.to(dtype)).sum()
    dX, da, dc = torch.autograd.grad(loss, (X, a, c))
    return {"p": p.detach(), "m": m.detach(), "psum": psum.detach(), "dX": dX, "da": da, "dc": dc}


GROUP_DIMS = {"p": (2,), "m": (2,), "psum": (), "dX": (1, 2), "da": (1,), "dc": (1,)}


def rel_l2(got, ref, dims):
    """relative L2 error over ``dims`` (an all-zero reference group must be met exactly: error 0 or inf)"""
    got, ref = got.double().cpu(), ref.double()
    if dims:
        num = (got - ref).pow(2).sum(dims).sqrt()
        den = ref.pow(2).sum(dims).sqrt()
    else:
        num, den = (got - ref).abs(), ref.abs()
    err = num / den
    err = torch.where(den == 0, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf"))), err)
    return err


def check(name, got, ref, bounds, failures):
    """prints one PARITY line per quantity, appends the violations to ``failures``; a NaN anywhere is a violation"""
    for k, dims in GROUP_DIMS.items():
        if k not in got:
            continue
        err = rel_l2(got[k], ref[k], dims)
        bound = bounds.get(k, FP32_BOUND)
        worst = float(err.max()) if not torch.isnan(err).any() else float("nan")
        print(f"PARITY|{name}|{k}|{worst:.3e}|{bound:.3e}", flush=True)
        if not worst <= bound:
            failures.append((name, k, worst, bound))
    return failures


# ------------------------------------------------------------------------------------------------ the branch head
def branch_weights(D, H, K, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dtype)
    return {"cls": r(1, K, D), "in_proj_weight": r(3 * D, D, scale=D ** -0.5), "in_proj_bias": r(3 * D, scale=0.1),
            "out_proj.weight": r(D, D, scale=D ** -0.5), "out_proj.bias": r(D, scale=0.1), "ln.weight": 1 + r(D, scale=0.1),
            "ln.bias": r(D, scale=0.1)}


def branch_rows(w, x, lens, H, eps=1e-5):
    """LN(MHA([cls ; x]) + [cls ; x])[:, :K] through nn.MultiheadAttention (eval mode) on the tensors of ``w`` as they are (keys of
    branch_weights), in their dtype."""
    D = x.shape[-1]
    K = w["cls"].shape[1]
    mha = torch.nn.MultiheadAttention(D, H, dropout=0.0, batch_first=True).to(x.dtype).eval()
    B, T = x.shape[:2]
    src = torch.cat([w["cls"].expand(B, -1, -1), x], 1)
    pad = torch.arange(T + K)[None] >= (lens.long()[:, None] + K)
    params = {k: w[k] for k in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")}
    att = torch.func.functional_call(mha, params, (src, src, src), {"key_padding_mask": pad, "need_weights": False})[0]
    return torch.nn.functional.layer_norm(att + src, (D,), w["ln.weight"], w["ln.bias"], eps)[:, :K]


def branch_rows_mult(w, x, lens, H, mult, eps=1e-5):
    """branch_rows written out (nn.MultiheadAttention has no way to take a given dropout mask): the K query rows attend over
    [cls ; x], their attention weights are multiplied by ``mult`` [B, K H, K + T] (row k H + h = query k, head h; entries in the
    order of the keys) before the values are summed.  mult = None is branch_rows itself (tests hold the two against each other)."""
    F = torch.nn.functional
    D = x.shape[-1]
    K = w["cls"].shape[1]
    dh = D // H
    B, T = x.shape[:2]
    src = torch.cat([w["cls"].expand(B, -1, -1), x], 1)
    Wq, Wk, Wv = w["in_proj_weight"].split(D, 0)
    bq, bk, bv = w["in_proj_bias"].split(D, 0)
    q = F.linear(src[:, :K], Wq, bq).view(B, K, H, dh)
    k = F.linear(src, Wk, bk).view(B, T + K, H, dh)
    v = F.linear(src, Wv, bv).view(B, T + K, H, dh)
    s = torch.einsum("bkhd,bjhd->bkhj", q, k) * dh ** -0.5
    pad = torch.arange(T + K)[None] >= (lens.long()[:, None] + K)
    p = torch.softmax(s.masked_fill(pad[:, None, None, :], float("-inf")), -1)
    if mult is not None:
        p = p * mult.to(p.dtype).view(B, K, H, T + K)
    ctx = torch.einsum("bkhj,bjhd->bkhd", p, v).reshape(B, K, D)
    att = F.linear(ctx, w["out_proj.weight"], w["out_proj.bias"])
    return F.layer_norm(att + src[:, :K], (D,), w["ln.weight"], w["ln.bias"], eps)


def branch_ref(w, feat, lens, H, dtype=torch.float64, eps=1e-5, mult=None):
    """branch_rows in ``dtype`` on fresh leaves -> (out [B, K, D], the leaf tensors by name, ``feat`` among them) - call .backward on
    a function of ``out`` and read the leaves' .grad."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in w.items()}
    x = feat.detach().to(dtype).clone().requires_grad_(True)
    out = branch_rows(leaves, x, lens, H, eps) if mult is None else branch_rows_mult(leaves, x, lens, H, mult, eps)
    leaves["feat"] = x
    return out, leaves


def cascaded_ref(W, feat, lens, nhead, training, nhead_clip, sot, eot, vq_temp=0.1, forced_tokens=None, aux=None):
    """The whole KW_CascadedBranch (avssl/model/kw_branches.py:349-382) restated in the dtype of ``W`` (a branch state dict: cls,
    self_att.*, linear_proj.*, bn_layer.bn_layer.*, clip.model.*): the keyword rows through nn.MultiheadAttention, the projection,
    F.batch_norm in the reference's permuted view, oracle.vq_forward, oracle.clip_encode_keywords
    -> (cascaded_audio_feat [B, E], keywords [B, K, Et]).  ``aux``: masked cosine scores, tokens, the running buffers after the step."""
    import oracle
    F = torch.nn.functional
    w = {"cls": W["cls"], "ln.weight": W["self_att.attentionBlock_Norm.weight"], "ln.bias": W["self_att.attentionBlock_Norm.bias"]}
    for k in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"):
        w[k] = W["self_att.multihead_attn_layer." + k]
    rows = branch_rows(w, feat, lens, nhead)
    kw = F.linear(rows, W["linear_proj.weight"], W["linear_proj.bias"])
    rm, rv = W["bn_layer.bn_layer.running_mean"].clone(), W["bn_layer.bn_layer.running_var"].clone()
    kw = bn_ref(kw, W["bn_layer.bn_layer.weight"], W["bn_layer.bn_layer.bias"], rm, rv, training, kind="eachKw")
    emb = W["clip.model.token_embedding.weight"]
    cos = F.normalize(kw, dim=-1, eps=1e-8) @ F.normalize(emb, dim=-1, eps=1e-8).t()
    prob = oracle.vq_forward(cos, vq_temp, training, forced=forced_tokens)
    if aux is not None:
        masked = cos.detach().clone()
        masked[..., [0, 2, 3]] = float("-inf")
        aux.update(cos=masked, tokens=masked.argmax(-1), running_mean=rm, running_var=rv)
    keywords = prob @ emb
    B, K = keywords.shape[:2]
    out = oracle.clip_encode_keywords(W, "clip.model.", keywords, torch.full((B,), K, dtype=torch.long), nhead_clip, sot, eot)
    return out, keywords


# ------------------------------------------------------------------------------------------------ fixed-count BatchNorm
def bn_ref(x, weight, bias, run_mean, run_var, training, momentum=0.1, eps=1e-5, kind="eachKw"):
    """x [B, K, E]; ``eachKw``: F.batch_norm on x.permute(0, 2, 1).reshape(B, E K) (parameters at d K + k); ``same``: on
    x.permute(0, 2, 1) with E channels.  The running buffers are updated in place when training."""
    B, K, E = x.shape
    if kind == "eachKw":
        y = torch.nn.functional.batch_norm(x.permute(0, 2, 1).reshape(B, -1), run_mean, run_var, weight, bias, training, momentum, eps)
        return y.reshape(B, E, K).permute(0, 2, 1)
    y = torch.nn.functional.batch_norm(x.permute(0, 2, 1), run_mean, run_var, weight, bias, training, momentum, eps)
    return y.permute(0, 2, 1)
