"""Helpers of tests/test_gpu_text_tower.py (not collected on their own): the cases, seeded weights and inputs, the fp64 stage
references with their derived bounds, a torch emulation of the product's arithmetic, the whole-tower fp64 reference with its
bf16-storage control, and the planted errors for the frozen CLIP text tower (speechclip_plus_amd/clip_text_hip.py: tower_forward,
tower_backward, KeywordTowerFn, TextTowerFn).  Nothing here needs a GPU or imports GPU code; tests/test_text_tower_cases_cpu.py shows
on the CPU that the emulation keeps every bound, that every planted error breaks one and that the softmax of the cases is not flat.

A STAGE is a dict: ``kind`` (ln / gemm / fc1 / attn_fwd / aux2 / ln_bwd / attn_bwd), ``name``, the stage's own inputs and what the code
under test produced from them.  ``check_stage`` compares one stage element by element with the fp64 definition of the operation on
those inputs (openai/CLIP: layer_norm, linear, u sigmoid(1.702 u) and its exact derivative, causal softmax attention inside a segment,
LayerNorm' plus the residual gradient).  The GPU module turns the recorded kernel calls into stages, the CPU module the emulation.

Bounds (docs/parity.md, "Frozen CLIP text tower"; all fixed before the first GPU run).  U, STORE, KSEC, FTZ and _passes are the trainable
module's: U = 2^-24, one bf16 store 2^-8, second-order factor 2, 2^-106 of absolute slack; where a bound is zero the value must be
exactly the reference.  The attention stages use attn_cases' references and bounds unchanged."""
import numpy as np
import torch

import attn_cases as ac
from attn_cases import Report, rel_l2  # noqa: F401
from test_gpu_trainable_bwd import FTZ, KSEC, STORE, U, _passes

EPS = 1e-5              # nn.LayerNorm's default, what ln_1 / ln_2 carry
K_EPI = 3               # fp32 operations on a GEMM accumulator besides its K products: it starts from the bias (one add), then the (absent)
#                         dropout scale and the residual add - the frozen-forward module's K_eff = K + 3 (csrc/gemm_bf16.hip, serial in k)
LAYERS = 2
BLOCK = 128             # rows of an attention block (clip_text_hip.BLOCK)
ALPHA = 1.702           # QuickGELU: u sigmoid(1.702 u)
QGELU_ULP = 1           # f against bf16(quickgelu_fp64(u)), u the stored pre-activation: at most 1 bf16 ulp ...
QGELU_SHARE = 0.01      # ... in at most 1 % of the elements ("CLIP image tower": v_exp / v_rcp move a result across a rounding boundary rarely)
# Factor on the q and k blocks of every in_proj_weight (and in_proj_bias), so that the softmax is not flat.  nn.MultiheadAttention
# initialises in_proj_weight xavier-uniform: std sqrt(2 / (W + 3 W)) = 0.031 at W = 512, so q and k of a unit-variance LayerNorm row
# have std 0.71 and the scaled score q . k / 8 a std of 0.5: softmax over 8 .. 10 keys within a factor 2 of uniform.  The score grows with
# the factor squared.  Chosen on the CPU from case A's fp64 reference, median of the largest probability over the queries with >= 8 keys
# (both layers; the condition is >= 0.3): factor 1.5 -> 0.28, 2 -> 0.44 (0.47 / 0.40 per layer), 2.5 -> 0.58, 3 -> 0.72.  2 is the
# smallest that meets the condition with margin; beyond it the softmax saturates (3: p > 0.99 in a third of the 3-key rows), dS = P (dP -
# delta) cancels to nothing and the backward stages would be checked on gradients that are mostly rounding.
# test_text_tower_cases_cpu.test_softmax_is_not_flat_and_the_control prints the medians.
QK_FACTOR = 2.0
NOT_FLAT = 0.3

# name -> width, heads, path, B, N (keywords per prompt: the keyword tensor's second dim) or T, counts, and the geometry the product must
# derive: SEG, Bp, M.  n_pos = min(77, N + 2); a count is keywords per prompt, so the EOT sits at position count + 1.
CASES = {
    # three pad sequences, an empty prompt, the 64 x 64 tiles, attn32_*
    "A": dict(W=512, heads=8, path="keyword", B=5, N=8, counts=[8, 1, 4, 0, 6], SEG=32, Bp=8, M=256),
    # the recipe's row count: 128 x 64 tiles for QKV / fc1 / the aux_mode 2 product, 64 x 64 x 4 for out_proj / fc2 / the input gradients
    "B": dict(W=512, heads=8, path="keyword", B=64, N=8, counts=None, SEG=32, Bp=64, M=2048),
    # causal = 64, two sequences per attention block, one pad sequence, an EOT at row 32 of its segment, q_rows = 128
    "C": dict(W=512, heads=8, path="keyword", B=3, N=40, counts=[40, 31, 1], SEG=64, Bp=4, M=256),
    # n_pos = 77, causal = 1, q_rows = 77, EOT rows either side of the 64-key tile edge
    "D": dict(W=768, heads=12, path="keyword", B=3, N=75, counts=[75, 63, 64], SEG=128, Bp=3, M=384),
    # TextTowerFn: a dense dy on every row
    "E": dict(W=512, heads=8, path="text", B=5, T=77, counts=None, SEG=128, Bp=5, M=640),
}


def counts_of(name):
    c = CASES[name]
    if name == "B":             # seeded counts in 0 .. 8 with at least one 0 and one 8
        n = torch.randint(0, 9, (64,), generator=torch.Generator().manual_seed(64)).tolist()
        n[5], n[17] = 0, 8
        return n
    return c["counts"]


def n_pos_of(name):
    c = CASES[name]
    return c["T"] if c["path"] == "text" else min(77, c["N"] + 2)


def geometry(B, T):
    """(SEG, Bp, M, causal argument of the attention kernels): the prompt length rounded up to 32 / 64 / 128, 128 / SEG sequences to an
    attention block, whole blocks - what clip_text_hip._geometry must give"""
    SEG = 32 if T <= 32 else 64 if T <= 64 else 128
    per = BLOCK // SEG
    Bp = -(-B // per) * per
    return SEG, Bp, Bp * SEG, 1 if SEG == BLOCK else SEG


def make_clip(width):
    """ClipModel(layers = 2) on the CPU with seeded random weights: the token / position tables from the model's own seed, the blocks'
    nn defaults under a forked, seeded generator; + 0.1 sigma noise on every LayerNorm gamma / beta (as the oracle test does), the q and k
    blocks of in_proj scaled by QK_FACTOR, and 0.02 sigma on the attention biases, which nn.MultiheadAttention initialises to zero (a zero
    bias would leave the bias path of the QKV and out_proj epilogues unchecked)."""
    from speechclip_plus_amd.clip_text import ClipModel
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1000 + width)
        clip = ClipModel("ViT-B/32" if width == 512 else "ViT-L/14", device="cpu", layers=LAYERS, seed=77 + width).eval()
        with torch.no_grad():
            for blk in clip.model.transformer.resblocks:
                for ln in (blk.ln_1, blk.ln_2):
                    ln.weight.add_(torch.randn_like(ln.weight) * 0.1)
                    ln.bias.add_(torch.randn_like(ln.bias) * 0.1)
                blk.attn.in_proj_bias.add_(torch.randn_like(blk.attn.in_proj_bias) * 0.02)
                blk.attn.out_proj.bias.add_(torch.randn_like(blk.attn.out_proj.bias) * 0.02)
                blk.attn.in_proj_weight[: 2 * width] *= QK_FACTOR
                blk.attn.in_proj_bias[: 2 * width] *= QK_FACTOR
    return clip


def layer_weights(clip, dev="cpu"):
    """per block: the GEMM weights as the bf16 copies the product multiplies (fp64 values), biases and LayerNorm vectors from fp32"""
    bf = lambda t: t.detach().to(torch.bfloat16).to(device=dev, dtype=torch.float64)
    f = lambda t: t.detach().float().to(device=dev, dtype=torch.float64)
    out = []
    for blk in clip.model.transformer.resblocks:
        out.append(dict(wqkv=bf(blk.attn.in_proj_weight), bqkv=f(blk.attn.in_proj_bias), wo=bf(blk.attn.out_proj.weight),
                        bo=f(blk.attn.out_proj.bias), w1=bf(blk.mlp.c_fc.weight), b1=f(blk.mlp.c_fc.bias), w2=bf(blk.mlp.c_proj.weight),
                        b2=f(blk.mlp.c_proj.bias), g1=f(blk.ln_1.weight), be1=f(blk.ln_1.bias), g2=f(blk.ln_2.weight), be2=f(blk.ln_2.bias)))
    return out


def case_inputs(name):
    """keyword path: keywords [B, N, W] = 0.02 randn, counts, d_rows [B, W] (the gradient of the EOT rows); text path: x [B, T, W] = 0.5
    randn and a dense dy"""
    c = CASES[name]
    g = torch.Generator().manual_seed(300 + ord(name))
    if c["path"] == "text":
        return dict(x=torch.randn(c["B"], c["T"], c["W"], generator=g) * 0.5, dy=torch.randn(c["B"], c["T"], c["W"], generator=g))
    return dict(keywords=torch.randn(c["B"], c["N"], c["W"], generator=g) * 0.02, counts=torch.tensor(counts_of(name), dtype=torch.int64),
                d_rows=torch.randn(c["B"], c["W"], generator=g))


# ================================================================================================================== packed rows
def prompt_fp32(kw, counts, tok, pos, n_pos):
    """the element-wise formulation of the prompt (clip_official.py:233-262) in fp32: [B, n_pos, W] = [SOT, kw_1 .. kw_n, EOT, token 0 ..] +
    pos; tok = the embeddings of SOT, EOT and token 0"""
    B, N, W = kw.shape
    x = tok[2].expand(B, n_pos, W).clone()
    x[:, 0] = tok[0]
    for b in range(B):
        n = int(counts[b])
        x[b, 1: n + 1] = kw[b, :n]
        x[b, n + 1] = tok[1]
    return x + pos[:n_pos]


def assemble_ref(kw, counts, tok, pos, Bp, SEG, n_pos):
    """-> (X [Bp SEG, W] bf16: the fp32 prompt rounded once, zero behind n_pos and in pad sequences; eot_row [B] int32)"""
    B, N, W = kw.shape
    X = torch.zeros(Bp, SEG, W, dtype=torch.float32, device=kw.device)
    X[:B, :n_pos] = prompt_fp32(kw, counts, tok, pos, n_pos)
    eot = torch.tensor([b * SEG + int(counts[b]) + 1 for b in range(B)], dtype=torch.int32, device=kw.device)
    return X.to(torch.bfloat16).view(Bp * SEG, W), eot


def live_rows(counts, Bp, SEG, dev="cpu"):
    """[Bp SEG] bool: the rows up to and including each sequence's EOT; every row behind it (incl. n_pos .. SEG - 1) and every row of a pad
    sequence is dead: it must carry exactly zero gradient and must not influence a live row"""
    m = torch.zeros(Bp, SEG, dtype=torch.bool)
    for b, n in enumerate(counts):
        m[b, : int(n) + 2] = True
    return m.view(-1).to(dev)


# ================================================================================================================== fp64 stage references
def qgelu64(u):
    return u * torch.sigmoid(ALPHA * u)


def qgelu_grad64(u):
    s = torch.sigmoid(ALPHA * u)
    return s * (1.0 + ALPHA * u * (1.0 - s))


def qgelu_grad_err(u):
    """Absolute error c(u) of the library's QuickGELU derivative (csrc/sc_common.h act_grad, act = 2), fp64 ``u``:
        sg = 1.f / (1.f + __expf(-1.702f * u));  return sg * (1.f + 1.702f * u * (1.f - sg));
    With x = 1.702 |u| and s = sigmoid(1.702 u).  Roundings, each U relative, and the hardware ulps:
      * the exponent: 1.702f itself, the product with u, and __expf = v_exp_f32(t log2 e) with log2 e rounded and one more product: 4 U x
        absolute on the exponent = 4 U x relative on e; v_exp_f32 1 ulp = 2 U; e enters s through ds / de e = -s (1 - s);
      * 1 + e: U; the division (correctly rounded, or v_rcp_f32 at 1 ulp): 2 U; both relative to s.
        => |d s| <= U (s (1 - s) (4 x + 2) + 3 s).
      * d g / d s = 1 + 1.702 u (1 - 2 s), at most 1 + x in magnitude: the cancellation in 1 - sg at large positive u is in this term.
      * 1 - sg: U (1 - s), times 1.702 |u| s;  1.702f * u: 2 U x (constant and product), times s (1 - s);  the product with (1 - sg): U x s (1 - s);
        1 + ...: U |1 + p| s = U |g|;  the final product: U |g|.
    Sum: U ((1 + x) (s (1 - s) (4 x + 2) + 3 s) + 4 x s (1 - s) + 2 |g|), doubled for the second-order terms (KSEC).  6 U = 3.6e-7 at u = 0."""
    x = ALPHA * u.abs()
    s = torch.sigmoid(ALPHA * u)
    g = qgelu_grad64(u)
    return KSEC * U * ((1.0 + x) * (s * (1.0 - s) * (4.0 * x + 2.0) + 3.0 * s) + 4.0 * x * s * (1.0 - s) + 2.0 * g.abs())


def gemm_ref(A, W, bias=None, res=None):
    """fp64 linear stage + STORE |ref| + 2 U (K + 3) (|A| @ |W|^T + |bias|).  The accumulator starts from the bias and takes K products
    serially; the residual is added in fp32 in front of the ONLY rounding (csrc/gemm_bf16.hip epilogue), so no stage gets 2 STORE.  A row of
    zeros without a bias has bound 0: it must be exactly the residual (or zero)."""
    A, W = A.double(), W.double()
    dot, mag = A @ W.t(), A.abs() @ W.abs().t()
    if bias is not None:
        dot, mag = dot + bias.double(), mag + bias.double().abs()
    ref = dot if res is None else dot + res.double()
    return ref, STORE * ref.abs() + KSEC * U * (A.shape[1] + K_EPI) * mag


def ln_ref(x, g, b):
    """layer_norm in fp64 + the frozen-forward bound: the kernel (csrc/rowops.hip) takes the two-pass mean / variance in fp32 over D
    channels: the mean is off by <= D U mean|x|, rstd by <= D U relative; y = xhat g + beta inherits (|g| (|xhat| + rstd mean|x|) + |beta|) D U"""
    x, g, b = x.double(), g.double(), b.double()
    D = x.shape[1]
    xc = x - x.mean(1, keepdim=True)
    rstd = ((xc * xc).mean(1, keepdim=True) + EPS).rsqrt()
    xh = xc * rstd
    ref = xh * g + b
    return ref, STORE * ref.abs() + KSEC * D * U * (g.abs() * (xh.abs() + rstd * x.abs().mean(1, keepdim=True)) + b.abs())


def ln_bwd_ref(x, dy, g, dres):
    """dx = LN'(x)(dy) + dres in fp64 + the trainable-backward bound.  layernorm_bwd_kernel (csrc/backward.hip) forms
    o = rstd (dy gamma - s1 - xhat s2) in fp32, ADDS the bf16 dres to it in fp32 and rounds once (pack2bf): ONE STORE on the sum.  The
    statistics and the two channel means are fp32 over D channels: D U relative per term, doubled.  A row with dy = 0 has the bound
    STORE |dres|, which bf16(0 + dres) = dres meets exactly; with dres = 0 as well the bound is 0: exactly zero."""
    x, dy, g = x.double(), dy.double(), g.double()
    D = x.shape[1]
    xc = x - x.mean(1, keepdim=True)
    rstd = ((xc * xc).mean(1, keepdim=True) + EPS).rsqrt()
    xh = xc * rstd
    gd = g * dy
    dx = rstd * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True))
    mag = rstd * (gd.abs() + gd.abs().mean(1, keepdim=True) + (xh.abs() + 1.0) * (gd * xh).abs().mean(1, keepdim=True))
    if dres is not None:
        dx = dx + dres.double()
    return dx, STORE * dx.abs() + KSEC * D * U * mag


def aux2_ref(A, Wt, u):
    """The aux_mode 2 product C = bf16(bf16(A . Wt^T) * QuickGELU'(u)) (csrc/gemm_bf16.hip: rr = the values the plain GEMM would have stored,
    v = rr * act_grad(u) in fp32, pack2bf) against (A @ Wt^T) QuickGELU'(u) in fp64: the doubly rounded form
        2 STORE |ref| + 2 K U (|A| @ |Wt|^T) |act'| + c(u) |dot|.
    Two round-to-nearest bf16 roundings: (1 + d1)(1 + d2) - 1 with |d| <= 2^-8 / (1 + 2^-8) is below 2 x 2^-8 by 1.5e-5 relative, which
    also holds the fp32 product's U.  No bias, no residual: K products (the + 3 of the plain stages is not needed; the form the issue
    states).  -> ref, bound, dot, act'"""
    A, Wt, u = A.double(), Wt.double(), u.double()
    dot, mag = A @ Wt.t(), A.abs() @ Wt.abs().t()
    ga = qgelu_grad64(u)
    ref = dot * ga
    return ref, 2 * STORE * ref.abs() + KSEC * A.shape[1] * U * mag * ga.abs() + qgelu_grad_err(u) * dot.abs(), dot, ga


def bf16_ulps(a, b):
    """|ordinal distance| of two bf16 tensors (sign-magnitude bit patterns mapped to a monotone integer)"""
    def o(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (o(a) - o(b)).abs()


# ------------------------------------------------------------------------------------------------------------------ attention
def attn_geometry(SEG):
    """rows of one attention problem and the causal argument of attn_cases.key_mask: a 32-row sequence on its own (attn32_*: one wave per
    (sequence, head)); a 128-row block of two 64-row segments (causal = 64); a 128-row sequence (causal = 1)"""
    return (32, 1) if SEG == 32 else (BLOCK, 64) if SEG == 64 else (BLOCK, 1)


def split_heads(x, R):
    """[M, heads 64] -> [M / R * heads, R, 64] fp64: attention problem n = (block, head)"""
    M, W = x.shape
    return x.double().view(M // R, R, W // 64, 64).permute(0, 2, 1, 3).reshape(-1, R, 64)


def merge_heads(x, heads):
    """inverse of split_heads"""
    n, R, _ = x.shape
    return x.view(n // heads, heads, R, 64).permute(0, 2, 1, 3).reshape(n // heads * R, heads * 64)


def attn_fwd_stage_ref(qkv, SEG, drop_key=None):
    W = qkv.shape[1] // 3
    R, causal = attn_geometry(SEG)
    q, k, v = (split_heads(qkv[:, i * W: (i + 1) * W], R) for i in range(3))
    mask = ac.key_mask(R, R, causal)[None].to(qkv.device)
    return ac.fwd_ref(q, k, v, mask, scale=0.125, drop_key=drop_key), (q, k, v)


def attn_bwd_stage_ref(qkv, dout, SEG):
    """attn32_bwd recomputes maximum and sum (short_bwd_errors, 32 keys); the flash backward is fed the kernel's own out and lse2
    (flash_bwd_errors, 128 keys) - the references and bounds of tests/attn_cases.py, unchanged"""
    f, (q, k, v) = attn_fwd_stage_ref(qkv, SEG)
    R, _ = attn_geometry(SEG)
    d = split_heads(dout, R)
    if SEG == 32:
        ep, dd = ac.short_bwd_errors(f, d, v)
        return ac.bwd_ref(q, k, v, d, f["mask"], scale=0.125, ep=ep, ddelta=dd, R_acc=32), f, (q, k, v, d)
    ep, dd = ac.flash_bwd_errors(f, d)
    return ac.bwd_ref(q, k, v, d, f["mask"], scale=0.125, ep=ep, ddelta=dd), f, (q, k, v, d)


# ================================================================================================================== the criterion
def check(rep, case, what, got, ref, bound):
    """element-wise criterion of the trainable module (_passes without a rel-L2 limit: a zero bound means exactly the reference, FTZ of
    slack elsewhere, everything finite).  Prints PARITY|case|stage @(row, col)|error there|rel-L2|bound there|ratio before it records."""
    ok, ratio, e = _passes(got, ref, bound)
    d = (got.double() - ref).abs() / (bound + FTZ)
    i = int(torch.nan_to_num(d, nan=float("inf")).argmax()) if d.numel() else 0
    err, bd = float((got.double() - ref).abs().flatten()[i]), float(bound.flatten()[i])
    where = tuple(int(j) for j in np.unravel_index(i, tuple(d.shape))) if d.numel() else ()
    line = f"PARITY|{case}|{what} @{where}|{err:.3e}|{e:.3e}|{bd:.3e}|ratio {ratio:.3f}"
    print(line)
    rep.lines.append(line)
    rep.require(case, f"{what}: error {err:.3e} > bound {bd:.3e} at {where} (error / bound {ratio:.3g})", ok)
    return ratio


def check_qgelu(rep, case, what, f, u):
    """f against bf16(quickgelu_fp64(u)), u the kernel's own stored pre-activation: <= 1 bf16 ulp, in <= 1 % of the elements"""
    want = qgelu64(u.double()).to(torch.bfloat16)
    ulps = bf16_ulps(f, want)
    worst, share = int(ulps.max()), float((ulps > 0).double().mean())
    fin = bool(torch.isfinite(f.float()).all())
    line = f"PARITY|{case}|{what}|max {worst} ulp|{rel_l2(f, want.double()):.3e}|off in {share:.3e} of {ulps.numel()}|limit {QGELU_ULP} ulp, {QGELU_SHARE}"
    print(line)
    rep.lines.append(line)
    rep.require(case, f"{what}: {worst} bf16 ulps off bf16(quickgelu(u)), {share:.3g} of the elements differ", fin and worst <= QGELU_ULP and share <= QGELU_SHARE)
    return worst, share


def check_stage(rep, case, st):
    """one stage against its fp64 definition on its own inputs"""
    k, name = st["kind"], st["name"]
    if k == "ln":
        check(rep, case, name, st["got"], *ln_ref(st["x"], st["g"], st["b"]))
    elif k == "gemm":
        check(rep, case, name, st["got"], *gemm_ref(st["A"], st["W"], st.get("bias"), st.get("res")))
    elif k == "fc1":
        check(rep, case, name + " u", st["u"], *gemm_ref(st["A"], st["W"], st["bias"]))
        check_qgelu(rep, case, name + " f = QuickGELU(u)", st["f"], st["u"])
    elif k == "aux2":
        ref, bound, _, _ = aux2_ref(st["A"], st["W"], st["u"])
        check(rep, case, name, st["got"], ref, bound)
    elif k == "ln_bwd":
        check(rep, case, name, st["got"], *ln_bwd_ref(st["x"], st["dy"], st["g"], st["dres"]))
    elif k == "attn_fwd":
        f, _ = attn_fwd_stage_ref(st["qkv"], st["SEG"])
        R, _ = attn_geometry(st["SEG"])
        ac.check(rep, case, name, split_heads(st["out"], R), f["out"], f["bound"])
        if st.get("lse2") is not None:
            ac.check(rep, case, name + " lse2", st["lse2"].double().reshape(-1, R), f["lse2"], f["bound_lse"])
    elif k == "attn_bwd":
        r, _, _ = attn_bwd_stage_ref(st["qkv"], st["dout"], st["SEG"])
        R, _ = attn_geometry(st["SEG"])
        W = st["dqkv"].shape[1] // 3
        for i, n in enumerate(("dq", "dk", "dv")):
            ac.check(rep, case, f"{name} {n}", split_heads(st["dqkv"][:, i * W: (i + 1) * W], R), r[n], r["bound_" + n])
    else:
        raise KeyError(k)


def check_dead_rows(rep, case, what, t, live):
    """every dead row of a gradient tensor exactly zero, every element finite"""
    fin = bool(torch.isfinite(t.float()).all())
    nz = int((t[~live] != 0).sum())
    rep.require(case, f"{what}: {nz} non-zero elements in rows that must carry zero gradient" + ("" if fin else ", not finite"), fin and nz == 0)
    return nz == 0 and fin


# ================================================================================================================== emulation
def _bf(x):
    return x.to(torch.bfloat16)


def emulate_chain(X, dX, layers32, heads, SEG):
    """The product's arithmetic in fp32 torch on bf16 operands, rounded to bf16 where the product stores: X [M, W] bf16 packed rows,
    dX [M, W] bf16 the gradient of the output rows, layers32 = per block the bf16 GEMM weights and fp32 vectors.  The attention goes
    through attn_cases.emulate_*.  -> (stages in the product's order, output rows, input gradient)"""
    M, W = X.shape
    R, causal = attn_geometry(SEG)
    mask = ac.key_mask(R, R, causal)[None]
    F = torch.nn.functional
    lin = lambda a, w, b=None, r=None: _bf(a.float() @ w.float().t() + (0 if b is None else b) + (0 if r is None else r.float()))
    sp = lambda t: split_heads(t, R).float()
    stages, saved = [], []
    for li, w in enumerate(layers32):
        t = f"layer {li} "
        h = _bf(F.layer_norm(X.float(), (W,), w["g1"], w["be1"], EPS))
        stages.append(dict(kind="ln", name=t + "ln_1", x=X, g=w["g1"], b=w["be1"], got=h))
        qkv = lin(h, w["wqkv"], w["bqkv"])
        stages.append(dict(kind="gemm", name=t + "QKV", A=h, W=w["wqkv"], bias=w["bqkv"], got=qkv))
        q, k, v = (sp(qkv[:, i * W: (i + 1) * W]) for i in range(3))
        if SEG == 32:
            o, lse2 = ac.emulate_short_fwd(q, k, v, mask), None
        else:
            o, lse2 = ac.emulate_fwd(q, k, v, mask)
        att = merge_heads(o, heads)
        stages.append(dict(kind="attn_fwd", name=t + "attention", qkv=qkv, SEG=SEG, out=att, lse2=lse2))
        X2 = lin(att, w["wo"], w["bo"], X)
        stages.append(dict(kind="gemm", name=t + "out_proj + residual", A=att, W=w["wo"], bias=w["bo"], res=X, got=X2))
        h2 = _bf(F.layer_norm(X2.float(), (W,), w["g2"], w["be2"], EPS))
        stages.append(dict(kind="ln", name=t + "ln_2", x=X2, g=w["g2"], b=w["be2"], got=h2))
        u = lin(h2, w["w1"], w["b1"])
        f = _bf(u.float() * (1.0 / (1.0 + torch.exp(-1.702 * u.float()))))
        stages.append(dict(kind="fc1", name=t + "fc1", A=h2, W=w["w1"], bias=w["b1"], u=u, f=f))
        Xn = lin(f, w["w2"], w["b2"], X2)
        stages.append(dict(kind="gemm", name=t + "fc2 + residual", A=f, W=w["w2"], bias=w["b2"], res=X2, got=Xn))
        saved.append((X, qkv, o, lse2, X2, u))
        X = Xn
    out = X

    def ln_bwd(x, dy, g, dres):
        x, dy = x.float(), dy.float()
        xc = x - x.mean(1, keepdim=True)
        rstd = ((xc * xc).mean(1, keepdim=True) + EPS).rsqrt()
        xh, gd = xc * rstd, dy * g
        return _bf(rstd * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True)) + dres.float())

    for li in range(len(layers32) - 1, -1, -1):
        w, (Xl, qkv, o, lse2, X2, u) = layers32[li], saved[li]
        t = f"layer {li} bwd "
        w2T, w1T, woT, wqkvT = (w[n].t().contiguous() for n in ("w2", "w1", "wo", "wqkv"))
        uf = u.float()
        sg = 1.0 / (1.0 + torch.exp(-1.702 * uf))
        du = _bf(lin(dX, w2T).float() * (sg * (1.0 + 1.702 * uf * (1.0 - sg))))
        stages.append(dict(kind="aux2", name=t + "fc2 dgrad x QuickGELU'", A=dX, W=w2T, u=u, got=du))
        dh2 = lin(du, w1T)
        stages.append(dict(kind="gemm", name=t + "fc1 dgrad", A=du, W=w1T, got=dh2))
        dX2 = ln_bwd(X2, dh2, w["g2"], dX)
        stages.append(dict(kind="ln_bwd", name=t + "ln_2' + dres", x=X2, dy=dh2, g=w["g2"], dres=dX, got=dX2))
        datt = lin(dX2, woT)
        stages.append(dict(kind="gemm", name=t + "out_proj dgrad", A=dX2, W=woT, got=datt))
        q, k, v = (sp(qkv[:, i * W: (i + 1) * W]) for i in range(3))
        d = sp(datt)
        if SEG == 32:
            g3 = ac.emulate_short_bwd(q, k, v, d, mask)
        else:
            g3 = ac.emulate_bwd(q, k, v, o, d, lse2, mask, scale=0.125)
        dqkv = torch.cat([merge_heads(x, heads) for x in g3], dim=1)
        stages.append(dict(kind="attn_bwd", name=t + "attention", qkv=qkv, dout=datt, SEG=SEG, dqkv=dqkv))
        dh1 = lin(dqkv, wqkvT)
        stages.append(dict(kind="gemm", name=t + "QKV dgrad", A=dqkv, W=wqkvT, got=dh1))
        dX = ln_bwd(Xl, dh1, w["g1"], dX2)
        stages.append(dict(kind="ln_bwd", name=t + "ln_1' + dres", x=Xl, dy=dh1, g=w["g1"], dres=dX2, got=dX))
    return stages, out, dX


def layers32_of(clip):
    """what emulate_chain multiplies: bf16 GEMM weights, fp32 biases and LayerNorm vectors (CPU)"""
    out = []
    for blk in clip.model.transformer.resblocks:
        f = lambda t: t.detach().float()
        out.append(dict(wqkv=_bf(blk.attn.in_proj_weight.detach()), bqkv=f(blk.attn.in_proj_bias), wo=_bf(blk.attn.out_proj.weight.detach()),
                        bo=f(blk.attn.out_proj.bias), w1=_bf(blk.mlp.c_fc.weight.detach()), b1=f(blk.mlp.c_fc.bias),
                        w2=_bf(blk.mlp.c_proj.weight.detach()), b2=f(blk.mlp.c_proj.bias), g1=f(blk.ln_1.weight), be1=f(blk.ln_1.bias),
                        g2=f(blk.ln_2.weight), be2=f(blk.ln_2.bias)))
    return out


# ================================================================================================================== whole tower: fp64 and its control
class _RoundBF16(torch.autograd.Function):
    """a bf16 store: the value is rounded on the way forward, its gradient on the way back"""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def tower64(X0, dOut, layers, heads, SEG, rounded):
    """openai/CLIP's text transformer on packed rows in fp64 (autograd for the input gradient), GEMM weights = the bf16 copies.
    ``rounded``: the CONTROL - the same chain with a bf16 rounding at every site where the product stores bf16: h, qkv, att, X2, h2, u, f and
    the layer output on the way forward, and (the same nodes on the way back) dX, du - rounded twice, as the aux_mode 2 epilogue does -,
    dh2, dX2 (LayerNorm' + dres: one rounding of the sum), datt, dqkv, dh1.  What the kernels round INSIDE (bf16 P and dS of the attention)
    is not in the control.  -> (output rows [M, W], input gradient [M, W], the largest probability of every query [layers][n, R])"""
    r = _RoundBF16.apply if rounded else (lambda t: t)
    M, W = X0.shape
    R, causal = attn_geometry(SEG)
    mask = ac.key_mask(R, R, causal)[None].to(X0.device)
    F = torch.nn.functional
    leaf = X0.double().detach().clone().requires_grad_()
    X, pmax = r(leaf), []
    sp = lambda t: t.view(M // R, R, heads, 64).permute(0, 2, 1, 3).reshape(-1, R, 64)
    for w in layers:
        h = r(F.layer_norm(X, (W,), w["g1"], w["be1"], EPS))
        qkv = r(h @ w["wqkv"].t() + w["bqkv"])
        q, k, v = (sp(qkv[:, i * W: (i + 1) * W]) for i in range(3))
        P = torch.softmax(((q @ k.transpose(-1, -2)) * 0.125).masked_fill(~mask, float("-inf")), dim=-1)
        pmax.append(P.detach().amax(-1))
        att = r(merge_heads(P @ v, heads))
        X2 = r(att @ w["wo"].t() + w["bo"] + X)
        h2 = r(F.layer_norm(X2, (W,), w["g2"], w["be2"], EPS))
        u = r(h2 @ w["w1"].t() + w["b1"])
        f = r(u * torch.sigmoid(ALPHA * u))
        X = r(f @ w["w2"].t() + w["b2"] + X2)
    (X * dOut.double()).sum().backward()
    return X.detach(), leaf.grad, pmax


# ================================================================================================================== planted errors
def plant_row_copy(got, row):
    """a row replaced by the row above it"""
    bad = got.clone()
    bad[row] = got[row - 1]
    return bad


def plant_ulps(got, row, col, n=2):
    """one bf16 element moved by n ulps (away from zero)"""
    bad = got.clone()
    bad.view(torch.int16)[row, col] += n
    return bad


def plant_min_normal(got, row, col):
    """one element set to the smallest positive bf16 normal, 2^-126"""
    bad = got.clone()
    bad[row, col] = 2.0 ** -126
    return bad


def kblock_ratios(got, A, Wt, u, row, k0):
    """aux_mode 2 product: the 64-wide k-block k0 .. k0 + 63 missing from ONE element of ``row``, taken for each element of the row on its
    own -> error / bound [N] (the frozen-forward module's form: the median must exceed 1)"""
    ref, bound, _, ga = aux2_ref(A[row: row + 1], Wt, u[row: row + 1])
    part = (A[row, k0: k0 + 64].double() @ Wt[:, k0: k0 + 64].double().t()) * ga[0]
    return ((got[row].double() - part - ref[0]).abs() / (bound[0] + FTZ))


def plant_attn_fwd(st, ns, query, key):
    """key removed from the softmax of ``query`` in the attention problems ``ns`` (every head of one sequence): the kernel's own output
    with those rows moved by the fp64 difference -> (bad [n, R, 64], ref, bound)"""
    f, _ = attn_fwd_stage_ref(st["qkv"], st["SEG"])
    g, _ = attn_fwd_stage_ref(st["qkv"], st["SEG"], drop_key=(ns, query, key))
    R, _ = attn_geometry(st["SEG"])
    bad = split_heads(st["out"], R).clone()
    bad[ns, query] += g["out"][ns, query] - f["out"][ns, query]
    return bad, f["out"], f["bound"]


def plant_attn_bwd(st, ns, query, key):
    """the contribution of ``query`` to dk / dv of ``key`` removed in the problems ``ns`` (every head of one sequence): dk_j -= scale dS_ij q_i,
    dv_j -= P_ij dO_i in fp64 -> {"dk": (bad, ref, bound), "dv": ...}"""
    r, f, (q, k, v, d) = attn_bwd_stage_ref(st["qkv"], st["dout"], st["SEG"])
    R, _ = attn_geometry(st["SEG"])
    W = st["dqkv"].shape[1] // 3
    P = f["P"][ns]
    dP = d[ns] @ v[ns].transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    out = {}
    for i, name, miss in ((1, "dk", 0.125 * dS[:, query, key, None] * q[ns, query]), (2, "dv", P[:, query, key, None] * d[ns, query])):
        bad = split_heads(st["dqkv"][:, i * W: (i + 1) * W], R).clone()
        bad[ns, key] -= miss
        out[name] = (bad, r[name], r["bound_" + name])
    return out


def per_problem_ratios(got, ref, bound, ns):
    """error / bound of each of the problems ``ns`` on its own (printed next to the verdict: which heads resolve a planted error)"""
    return [round(ac.within(got[n], ref[n], bound[n])[1], 3) for n in ns]


def rejected(tag, got, ref, bound):
    """the element-wise criterion alone must fail -> error / bound (printed)"""
    ok, ratio, _ = _passes(got, ref, bound)
    print(f"SENSITIVITY|{tag}|error / bound {ratio:.3g}")
    assert not ok and ratio > 1.0, f"{tag}: not rejected (error / bound {ratio:.3g})"
    return ratio


def rejected_attn(tag, got, ref, bound):
    """the same through attn_cases.within (the attention stages' criterion)"""
    ok, ratio, _ = ac.within(got, ref, bound)
    print(f"SENSITIVITY|{tag}|error / bound {ratio:.3g}")
    assert not ok and ratio > 1.0, f"{tag}: not rejected (error / bound {ratio:.3g})"
    return ratio


def seq_rel_l2(got, ref):
    """rel-L2 of one sequence's quantity; an exactly zero reference asks for an exactly zero result (-> 0.0, else inf)"""
    ref = ref.double()
    if not ref.numel() or float(ref.abs().max()) == 0.0:
        return 0.0 if (not got.numel() or float(got.double().abs().max()) == 0.0) else float("inf")
    return float((got.double() - ref).norm() / ref.norm())


def planted_suite(stages, tag, SEG, counts, row_copy_seq=1):
    """Every planted error that the stages of one run support, applied on the host to the code's own results; each must be rejected by the
    element-wise criterion alone, and the unperturbed result must pass first.  ``stages``: one whole forward + backward whose gradient
    enters at the EOT rows only.  -> {perturbation: error / bound}"""
    by = {st["name"]: st for st in stages}
    heads = by["layer 0 QKV"]["got"].shape[1] // 192
    live = live_rows(counts, by["layer 0 QKV"]["got"].shape[0] // SEG, SEG, by["layer 0 QKV"]["got"].device)
    eot = lambda b: b * SEG + int(counts[b]) + 1
    out = {}
    # fc2: the EOT row of a sequence replaced by the row above it
    st = by["layer 1 fc2 + residual"]
    ref, bound = gemm_ref(st["A"], st["W"], st["bias"], st["res"])
    assert _passes(st["got"], ref, bound)[0]
    out["fc2 EOT row <- row above"] = rejected(f"{tag}: fc2, EOT row {eot(row_copy_seq)} of sequence {row_copy_seq} <- the row above it",
                                               plant_row_copy(st["got"], eot(row_copy_seq)), ref, bound)
    # the aux_mode 2 product: one 64-wide k-block missing from one element, each element of the row on its own
    st = by["layer 1 bwd fc2 dgrad x QuickGELU'"]
    ref, bound, _, _ = aux2_ref(st["A"], st["W"], st["u"])
    assert _passes(st["got"], ref, bound)[0]
    r = kblock_ratios(st["got"], st["A"], st["W"], st["u"], eot(0), 128)
    med = float(r.median())
    print(f"SENSITIVITY|{tag}: aux_mode 2 product, k-block 128..191 missing from ONE element of row {eot(0)}|error / bound median {med:.3g}, "
          f"min {float(r.min()):.3g}, max {float(r.max()):.3g}; rejected on its own: {float((r > 1).double().mean()):.3f} of {r.numel()}")
    assert med > 1.0, f"{tag}: a k-block missing from a typical element of the aux_mode 2 product is not rejected (median {med:.3g})"
    out["aux_mode 2 k-block (median)"] = med
    # attention: key 0 (SOT) of the second sequence of a block, for its EOT query, in every head.  A head whose softmax is saturated on
    # another key (p(SOT) ~ 0) or on the SOT itself (dS ~ 0) cannot resolve it - what is missing there is below one rounding of the
    # result -, so the per-head ratios are printed and the verdict is the row's: the largest ratio over its elements
    if SEG == 32:
        ns, q, k0 = list(range(heads, 2 * heads)), int(counts[1]) + 1, 0       # problems (sequence 1, head h); keys are the sequence's own rows
    else:
        ns, q, k0 = list(range(heads)), SEG + int(counts[1]) + 1, SEG          # problems (block 0, head h); sequence 1 = rows SEG .. 2 SEG - 1
    st = by["layer 0 attention"]
    bad, ref, bound = plant_attn_fwd(st, ns, q, k0)
    assert ac.within(split_heads(st["out"], attn_geometry(SEG)[0]), ref, bound)[0]
    out["attention fwd: SOT key missing"] = rejected_attn(f"{tag}: attention forward, key {k0} missing from EOT query {q} of sequence 1 "
                                                          f"(per head {per_problem_ratios(bad, ref, bound, ns)})", bad, ref, bound)
    st = by["layer 1 bwd attention"]
    for name, (bad, ref, bound) in plant_attn_bwd(st, ns, q, k0).items():
        out[f"attention bwd: EOT query missing from {name}"] = rejected_attn(
            f"{tag}: attention backward, EOT query {q}'s contribution to {name} of key {k0} missing, sequence 1 "
            f"(per head {per_problem_ratios(bad, ref, bound, ns)})", bad, ref, bound)
    # LayerNorm': one element moved by 2 bf16 ulps
    st = by["layer 1 bwd ln_2' + dres"]
    ref, bound = ln_bwd_ref(st["x"], st["dy"], st["g"], st["dres"])
    assert _passes(st["got"], ref, bound)[0]
    col = int(ref[eot(0)].abs().argmax())
    out["LayerNorm' + 2 ulps"] = rejected(f"{tag}: LayerNorm' + dres, element ({eot(0)}, {col}) + 2 bf16 ulps", plant_ulps(st["got"], eot(0), col), ref, bound)
    # a must-be-zero gradient row: one element set to the smallest positive bf16 normal
    st = by["layer 1 bwd fc1 dgrad"]
    dead = int((~live).nonzero()[0])
    ref, bound = gemm_ref(st["A"], st["W"])
    assert _passes(st["got"], ref, bound)[0] and float(bound[dead].abs().max()) == 0.0
    bad = plant_min_normal(st["got"], dead, 3)
    out["zero row <- 2^-126"] = rejected(f"{tag}: fc1 dgrad, element ({dead}, 3) of a zero-gradient row <- 2^-126", bad, ref, bound)
    rep = Report()
    assert check_dead_rows(rep, tag, "fc1 dgrad", st["got"], live) and not check_dead_rows(rep, tag, "fc1 dgrad (planted)", bad, live)
    return out
