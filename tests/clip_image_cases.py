"""Helpers of tests/test_gpu_clip_image_stages.py (not collected on their own): the cases, seeded weights and pixels, the fp64 stage
references with their derived bounds, a torch emulation of the product's arithmetic, the whole-tower fp64 reference, and the planted
errors for the frozen CLIP image tower (speechclip_plus_amd/clip_image.py, csrc/vit.hip, the ACT = 2 GEMM instances,
sc_hubert_layer_fwd(pre_ln = 1, ffn_act = 2, seg)).  Nothing here needs a GPU or imports GPU code: every function works on the device
of its arguments, so the GPU module runs the same references in fp64 on the device and tests/test_clip_image_cases_cpu.py shows on the
CPU that the emulation keeps every bound, that every planted error breaks one and that the softmax of the cases is not flat.

A RECORD is what one forward leaves, whoever made it (``emulate`` here, the op-by-op sequence of the GPU module there):
    A [rows, Kp] bf16, G [rows, W] fp32, X0 [rows, W] bf16,
    layers[i] = dict(x, h1, qk [rows, 2 W], vt [rows W] flat (per image [H, 64, pitch] at W * row0), ctx, pre, h2, u32 (the fc1 product
                with act = 0 in fp32), ffn, out),
    cls [B, W] fp32, y [B, W] fp32, emb [B, E] fp32.
``w`` is ClipImageEncoder._weights(device): the bf16 GEMM weights and fp32 vectors the product multiplies.

Bounds (docs/parity.md, "CLIP image tower / Stage by stage"; all fixed before the first GPU run).  U, STORE, KSEC, FTZ, K_EPI, EXP_ULP and
the criterion (_passes / text_tower_cases.check) are the existing ones: U = 2^-24, one bf16 store 2^-8, second-order factor 2, 2^-106 of
absolute slack; where a bound is zero the value must be exactly the reference."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import attn_cases as ac
import text_tower_cases as tc
from attn_cases import EXP_ULP
from test_gpu_trainable_bwd import FTZ, KSEC, STORE, U, _passes
from text_tower_cases import ALPHA, EPS, K_EPI, Report, check, check_qgelu, gemm_ref, ln_ref, qgelu64, qgelu_grad64, rejected, rel_l2  # noqa: F401

# name -> tower, blocks, images; rows = B x pitch (56 for ViT-B/32, 264 for ViT-L/14)
CASES = {
    # 50 keys in one 64-key tile (it ends 8 keys behind the image); 280 rows: an M tail in every tile family
    "b32": dict(tower="ViT-B/32", layers=2, B=5, rows=280, seed=32),
    # 257 keys: the fifth key tile holds ONE valid key, the third 128-query block one real query and seven pad rows; V^T at pitch 264
    "l14": dict(tower="ViT-L/14", layers=2, B=3, rows=792, seed=14),
    # the only image is the last one: every tile overrun lands in the zeroed slack
    "l14_one": dict(tower="ViT-L/14", layers=1, B=1, rows=264, seed=15),
    # fc1 has 17 x 16 = 272 > 256 output tiles of 256 x 256: the persistent kernel walks tiles and hands over under the QuickGELU epilogue
    "l14_wide": dict(tower="ViT-L/14", layers=1, B=16, rows=4224, seed=15),
}
FACTORS = (1.0, 1.5, 2.0, 2.5, 3.0)
PMAX_LO, PMAX_HI = 0.3, 0.9
# Factor on the q and k blocks of every in_proj_weight / in_proj_bias: the smallest of FACTORS for which, in every layer of b32 and l14,
# the median over the queries of the largest probability (fp64 reference) lies in [0.3, 0.9].  CLIP's init gives q and k unit variance,
# so q . k / 8 has a standard deviation of 1 and a softmax over 50 / 257 keys is flat: a missing key would hide inside one bf16 rounding.
# test_clip_image_cases_cpu.test_qk_factor prints the medians per factor and asserts that this is the smallest that qualifies.
QK_FACTOR = 2.0
PLANT_MOVES = 4.0         # a removed key must move the fp64 reference by at least this many bounds at one or more elements

_grid = torch.arange(-12.0, 12.0, 1e-4, dtype=torch.float64)
QGELU_LIP = float(qgelu_grad64(_grid).abs().max())      # max |d/du u sigmoid(1.702 u)| = 1.0998 (at u = 1.4): what an error of u is multiplied by
del _grid


def qgelu_err(u):
    """Relative error c(u) of the library's QuickGELU (csrc/sc_common.h qgelu2, contraction off), fp64 ``u``:
        w = u * -2.4554669595930156f;  e = v_exp_f32(w);  d = e + 1.0f;  r = v_rcp_f32(d);  return u * r;
    With x = 1.702 |u| and s = sigmoid(1.702 u) = 1 / (1 + e).  Roundings, each U relative, and the hardware ulps:
      * the constant -1.702 log2(e) is rounded to fp32 (U) and the packed product rounds once more (U): |dw| <= 2 U |w|, and
        e = 2^w turns that into ln 2 . 2 U |w| = 2 U x relative on e;
      * v_exp_f32 at 1 ulp = EXP_ULP U = 2 U relative on e;
      * d = 1 + e: the error of e enters d with the weight e / (1 + e) = 1 - s; the add itself rounds: U relative on d;
      * v_rcp_f32 at 1 ulp = 2 U relative on r; the final product: U.
    Sum, relative to the result u r: U ((1 - s) (2 x + EXP_ULP) + 4), doubled for the second-order terms (KSEC).  10 U = 6.0e-7 at u = 0,
    8 U for u -> +inf; for u -> -inf it grows like 4 U x while the result itself vanishes like e^-x."""
    x = ALPHA * u.abs()
    s = torch.sigmoid(ALPHA * u)
    return KSEC * U * ((1.0 - s) * (2.0 * x + EXP_ULP) + 4.0)


def erf_gelu64(u):
    return 0.5 * u * (1.0 + torch.erf(u * 0.7071067811865476))


# ================================================================================================================== towers and inputs
_towers = {}


def make_tower(name, factor=None):
    """ClipImageEncoder(tower, layers, seed) on the CPU: CLIP's init scales, + 0.1 sigma noise on every LayerNorm gamma / beta, the q and k
    blocks of in_proj_weight / in_proj_bias scaled by ``factor`` (QK_FACTOR).  l14_one and l14_wide share one tower."""
    from speechclip_plus_amd.clip_image import ClipImageEncoder
    c = CASES[name]
    f = QK_FACTOR if factor is None else float(factor)
    key = (c["tower"], c["layers"], c["seed"], f)
    if key not in _towers:
        m = ClipImageEncoder(c["tower"], layers=c["layers"], seed=c["seed"]).eval()
        g = torch.Generator().manual_seed(9000 + c["seed"])
        W = m.width
        with torch.no_grad():
            for ln in [m.ln_pre, m.ln_post] + [x for blk in m.transformer.resblocks for x in (blk.ln_1, blk.ln_2)]:
                ln.weight.add_(0.1 * torch.randn(W, generator=g))
                ln.bias.add_(0.1 * torch.randn(W, generator=g))
            for blk in m.transformer.resblocks:
                blk.attn.in_proj_weight[: 2 * W] *= f
                blk.attn.in_proj_bias[: 2 * W] *= f
        _towers[key] = m
    return _towers[key]


def pixels_of(name):
    c = CASES[name]
    return torch.randn(c["B"], 3, 224, 224, generator=torch.Generator().manual_seed(500 + c["seed"] + c["B"]))


def geometry(m, B):
    return SimpleNamespace(B=B, P=m.patch, Kp=m.Kp, W=m.width, H=m.heads, tokens=m.tokens, pitch=m.pitch, rows=B * m.pitch,
                           layers=m.arch["layers"], E=m.embed_dim)


def real_rows(geo, dev="cpu"):
    """[B tokens] int64: the rows that hold a token (class row first)"""
    return torch.cat([torch.arange(b * geo.pitch, b * geo.pitch + geo.tokens) for b in range(geo.B)]).to(dev)


def row0_of(geo, dev="cpu"):
    return (torch.arange(geo.B) * geo.pitch).to(dev)


def expected_patches(img, geo):
    """the patch GEMM's operand: unfold -> permute -> bf16 in rows 1 .. g^2 of every image, zero class / pad rows and K-pad columns"""
    B, P = img.shape[0], geo.P
    gg = geo.tokens - 1
    pt = img.unfold(2, P, P).unfold(3, P, P).permute(0, 2, 3, 1, 4, 5).reshape(B, gg, 3 * P * P)
    A = torch.zeros(B, geo.pitch, geo.Kp, device=img.device, dtype=torch.bfloat16)
    A[:, 1: 1 + gg, : 3 * P * P] = pt.to(torch.bfloat16)
    return A.reshape(B * geo.pitch, geo.Kp)


# ================================================================================================================== V^T layout, heads
def encode_vt(vrows, geo):
    """rows [rows, W] -> the QKV epilogue's V^T buffer, flat: per image [H, 64, pitch] back to back at W * row0"""
    return torch.cat([vrows[b * geo.pitch: (b + 1) * geo.pitch].t().contiguous().reshape(-1) for b in range(geo.B)])


def vt_rows(vt, geo, wrong=None):
    """the V^T buffer as rows [rows, W] (test_gpu_frozen_fwd._vt_rows' segment branch).  ``wrong`` = (image, pitch'): that image's block is
    decoded at pitch' < pitch (planted error 4); its rows behind pitch' keep their right values"""
    flat, W, p = vt.reshape(-1), geo.W, geo.pitch
    out = []
    for b in range(geo.B):
        r = flat[W * b * p: W * (b + 1) * p].view(W, p).t()
        if wrong is not None and wrong[0] == b:
            r = torch.cat([flat[W * b * p: W * b * p + W * wrong[1]].view(W, wrong[1]).t(), r[wrong[1]:]])
        out.append(r)
    return torch.cat(out)


def heads_of(x, geo):
    """[rows, W] -> [B H, pitch, 64]: attention problem n = (image, head)"""
    return x.view(geo.B, geo.pitch, geo.H, 64).permute(0, 2, 1, 3).reshape(geo.B * geo.H, geo.pitch, 64)


def rows_of(x, geo):
    """inverse of heads_of"""
    return x.view(geo.B, geo.H, geo.pitch, 64).permute(0, 2, 1, 3).reshape(geo.rows, geo.W)


def key_mask(geo, dev="cpu"):
    return ac.key_mask(geo.pitch, geo.tokens)[None].to(dev)


# ================================================================================================================== fp64 stage references
def patch_ref(A, Wc):
    """conv1 as a GEMM, fp32 out, no bias: 2 U (Kp + 3) (|A| @ |W|^T) and no STORE term.  Class rows, pad rows and every row of zeros
    have bound 0: they must be exactly 0."""
    A, Wc = A.double(), Wc.double()
    return A @ Wc.t(), KSEC * U * (A.shape[1] + K_EPI) * (A.abs() @ Wc.abs().t())


def ln_acc(x, g, b):
    """layer_norm in fp64 and ln_ref's accumulation term alone (an fp32 store: no STORE) -> ref, bound, rstd, xhat"""
    x, g, b = x.double(), g.double(), b.double()
    D = x.shape[1]
    xc = x - x.mean(1, keepdim=True)
    rstd = ((xc * xc).mean(1, keepdim=True) + EPS).rsqrt()
    xh = xc * rstd
    return xh * g + b, KSEC * D * U * (g.abs() * (xh.abs() + rstd * x.abs().mean(1, keepdim=True)) + b.abs()), rstd, xh


def embed_ref(G, w, geo, cls_pos=None):
    """ln_pre(e), e = G + pos on the patch rows and cls + pos[0] on the class row, in fp64 on the real rows -> ref, bound [B tokens, W].
    ln_ref's bound (one bf16 store + the fp32 statistics over W channels) plus the ONE fp32 rounding of the sum that the kernel forms
    first (csrc/vit.hip: v = a + p), propagated through the norm: U (|G or cls| + |pos|) rstd |gamma|.
    ``cls_pos`` = (image, t): that image's class row takes pos[t] (planted error 1)."""
    B, T, W = geo.B, geo.tokens, geo.W
    a = G.double().view(B, geo.pitch, W)[:, :T].clone()
    a[:, 0] = w["cls"].double()
    p = w["pos"].double()[None].expand(B, T, W).clone()
    if cls_pos is not None:
        p[cls_pos[0], 0] = w["pos"][cls_pos[1]].double()
    a, p = a.reshape(B * T, W), p.reshape(B * T, W)
    ref, bound = ln_ref(a + p, w["ln_pre_g"], w["ln_pre_b"])
    _, _, rstd, _ = ln_acc(a + p, w["ln_pre_g"], w["ln_pre_b"])
    return ref, bound + U * (a.abs() + p.abs()) * rstd * w["ln_pre_g"].double().abs()


def fc1_ref(A, Wt, bias):
    """fp64 quickgelu(A W^T + b) + STORE |ref| + L . 2 U (K + 3) (|A| @ |W|^T + |b|) + c(u) |u|: the bf16 store, the error of the fp32
    pre-activation through the activation's largest slope L = QGELU_LIP, and qgelu2's own error.  -> ref, bound, u"""
    A, Wt, b = A.double(), Wt.double(), bias.double()
    u = A @ Wt.t() + b
    mag = A.abs() @ Wt.abs().t() + b.abs()
    ref = qgelu64(u)
    return ref, STORE * ref.abs() + QGELU_LIP * KSEC * U * (A.shape[1] + K_EPI) * mag + qgelu_err(u) * u.abs(), u


def proj_ref(y, proj):
    """the class rows @ proj in exact fp32 on the matrix pipe: 2 U (W + 1) (|y| @ |proj|)"""
    y, proj = y.double(), proj.double()
    return y @ proj, KSEC * U * (y.shape[1] + 1) * (y.abs() @ proj.abs())


def attn_ref(L, geo, only=None, drop_key=None):
    """attn_cases.fwd_ref over the recorded q / k / V^T: problem n = (image, head), key_mask(pitch, tokens), scale 0.125, nk = pitch.
    ``only`` = n: that problem alone.  -> (fwd_ref's dict, the kernel's context [n, pitch, 64])"""
    W = geo.W
    q, k = heads_of(L["qk"][:, :W], geo).double(), heads_of(L["qk"][:, W:], geo).double()
    v = heads_of(vt_rows(L["vt"], geo), geo).double()
    got = heads_of(L["ctx"], geo)
    if only is not None:
        q, k, v, got = (t[only: only + 1] for t in (q, k, v, got))
    return ac.fwd_ref(q, k, v, key_mask(geo, q.device), scale=0.125, drop_key=drop_key), got


# ================================================================================================================== the stage checks
def check_record(rep, case, rec, w, geo):
    """every stage of one record against its fp64 definition on the stage's own operands -> {stage: error / bound}"""
    dev = rec["G"].device
    real, W, T = real_rows(geo, dev), geo.W, geo.tokens
    out = {}

    def chk(what, got, ref, bound):
        out[what] = check(rep, case, what, got, ref, bound)

    chk("patch GEMM", rec["G"], *patch_ref(rec["A"], w["conv1"]))
    chk("embed + ln_pre", rec["X0"][real], *embed_ref(rec["G"], w, geo))
    pad = torch.ones(geo.rows, dtype=torch.bool, device=dev)
    pad[real] = False
    rep.require(case, "embed + ln_pre: pad rows not exactly zero", bool((rec["X0"][pad] == 0).all()))
    X = rec["X0"]
    for i, L in enumerate(rec["layers"]):
        t = f"layer {i} "
        rep.require(case, t + "does not read what the stage before it wrote", torch.equal(L["x"], X))
        chk(t + "ln_1", L["h1"][real], *ln_ref(L["x"][real], w[f"l{i}_ln1_g"], w[f"l{i}_ln1_b"]))
        ref, bound = gemm_ref(L["h1"], w[f"l{i}_qkv_w"], w[f"l{i}_qkv_b"])
        chk(t + "QKV q / k", L["qk"], ref[:, : 2 * W], bound[:, : 2 * W])
        chk(t + "QKV V^T", vt_rows(L["vt"], geo), ref[:, 2 * W:], bound[:, 2 * W:])
        f, got = attn_ref(L, geo)
        chk(t + "attention", got[:, :T], f["out"][:, :T], f["bound"][:, :T])
        del f
        chk(t + "out_proj + residual", L["pre"], *gemm_ref(L["ctx"], w[f"l{i}_o_w"], w[f"l{i}_o_b"], res=L["x"]))
        chk(t + "ln_2", L["h2"][real], *ln_ref(L["pre"][real], w[f"l{i}_ln2_g"], w[f"l{i}_ln2_b"]))
        ref, bound, _ = fc1_ref(L["h2"], w[f"l{i}_fc1_w"], w[f"l{i}_fc1_b"])
        chk(t + "fc1 + QuickGELU", L["ffn"], ref, bound)
        worst, share = check_qgelu(rep, case, t + "fc1 = bf16(QuickGELU(fp32 product))", L["ffn"], L["u32"])
        out[t + "fc1 ulps"], out[t + "fc1 share"] = worst, share
        chk(t + "fc1 fp32 product", L["u32"], *_u32_ref(L["h2"], w[f"l{i}_fc1_w"], w[f"l{i}_fc1_b"]))
        chk(t + "fc2 + residual", L["out"], *gemm_ref(L["ffn"], w[f"l{i}_fc2_w"], w[f"l{i}_fc2_b"], res=L["pre"]))
        X = L["out"]
    cls = X[row0_of(geo, dev)].double()
    chk("rows_gather", rec["cls"], cls, torch.zeros_like(cls))
    ref, bound, _, _ = ln_acc(rec["cls"], w["ln_post_g"], w["ln_post_b"])
    chk("ln_post", rec["y"], ref, bound)
    chk("proj", rec["emb"], *proj_ref(rec["y"], w["proj"]))
    return out


def _u32_ref(A, Wt, bias):
    """the act = 0, out_f32 launch that check_qgelu takes its pre-activation from: gemm_ref's accumulation term without STORE"""
    A, Wt, b = A.double(), Wt.double(), bias.double()
    return A @ Wt.t() + b, KSEC * U * (A.shape[1] + K_EPI) * (A.abs() @ Wt.abs().t() + b.abs())


# ================================================================================================================== emulation
def _bf(x):
    return x.to(torch.bfloat16)


def emulate_attn(q, k, v, mask):
    """attn_cases.emulate_fwd (the forward kernel's arithmetic order: fp32 scores, 32-key blocks, the stale-maximum rule, bf16 P into an
    fp32 P.V, one multiply by 1 / l, bf16 store) on the device of its arguments.  q, k, v [n, R, 64]; mask [1, R, R] -> [n, R, 64] bf16"""
    dev = q.device
    q, k, v = q.float(), k.float(), v.float()
    cs = torch.tensor(ac.C32, dtype=torch.float32, device=dev)
    xs = (q @ k.transpose(-1, -2)).masked_fill(~mask.expand(q.shape[0], -1, -1), float("-inf"))
    n, R = xs.shape[0], xs.shape[1]
    m_run = torch.full((n, R), ac.FLOOR_M, dtype=torch.float32, device=dev)
    l = torch.zeros(n, R, dtype=torch.float32, device=dev)
    o = torch.zeros(n, R, 64, dtype=torch.float32, device=dev)
    for k0 in range(0, xs.shape[2], 32):
        xb = xs[..., k0: k0 + 32]
        m_cand = torch.maximum(m_run, xb.amax(-1))
        grow = (m_cand - m_run) * cs > 6.0
        m_new = torch.where(grow, m_cand, m_run)
        alpha = torch.exp2((m_run - m_new) * cs)
        l, o, m_run = l * alpha, o * alpha[..., None], m_new
        mc = m_run * cs
        p = torch.exp2((xb.double() * ac.C32 - mc.double()[..., None]).float())
        l = l + p.sum(-1)
        o = o + p.to(torch.bfloat16).float() @ v[:, k0: k0 + 32]
    return _bf(o * (1.0 / l)[..., None])


def emulate(w, geo, pixels):
    """The product's arithmetic in fp32 torch with a bf16 rounding at every site where the product stores bf16 (the patch operand, the
    LayerNorm outputs, q / k / V^T, the context, the residual streams, the fc1 output) and fp32 everywhere else -> a record"""
    dev = pixels.device
    B, W, T, p = geo.B, geo.W, geo.tokens, geo.pitch
    lin = lambda a, wt, b, r=None: a.float() @ wt.float().t() + b + (0 if r is None else r.float())
    ln = lambda x, g, b: F.layer_norm(x.float(), (W,), g, b, EPS)
    A = expected_patches(pixels.float(), geo)
    G = A.float() @ w["conv1"].float().t()
    e = G.view(B, p, W)[:, :T].clone()
    e[:, 0] = w["cls"]
    X0 = torch.zeros(B, p, W, device=dev, dtype=torch.bfloat16)
    X0[:, :T] = _bf(ln(e + w["pos"], w["ln_pre_g"], w["ln_pre_b"]))
    X = X0.view(geo.rows, W)
    rec = dict(A=A, G=G, X0=X, layers=[])
    mask = key_mask(geo, dev)
    for i in range(geo.layers):
        h1 = _bf(ln(X, w[f"l{i}_ln1_g"], w[f"l{i}_ln1_b"]))
        qkv = _bf(lin(h1, w[f"l{i}_qkv_w"], w[f"l{i}_qkv_b"]))
        qk, vt = qkv[:, : 2 * W].contiguous(), encode_vt(qkv[:, 2 * W:], geo)
        ctx = rows_of(emulate_attn(heads_of(qkv[:, :W], geo), heads_of(qkv[:, W: 2 * W], geo), heads_of(qkv[:, 2 * W:], geo), mask), geo)
        pre = _bf(lin(ctx, w[f"l{i}_o_w"], w[f"l{i}_o_b"], X))
        h2 = _bf(ln(pre, w[f"l{i}_ln2_g"], w[f"l{i}_ln2_b"]))
        u32 = lin(h2, w[f"l{i}_fc1_w"], w[f"l{i}_fc1_b"])
        ffn = _bf(u32 * (1.0 / (1.0 + torch.exp(-ALPHA * u32))))
        out = _bf(lin(ffn, w[f"l{i}_fc2_w"], w[f"l{i}_fc2_b"], pre))
        rec["layers"].append(dict(x=X, h1=h1, qk=qk, vt=vt, ctx=ctx, pre=pre, h2=h2, u32=u32, ffn=ffn, out=out))
        X = out
    rec["cls"] = X[row0_of(geo, dev)].float()
    rec["y"] = ln(rec["cls"], w["ln_post_g"], w["ln_post_b"])
    rec["emb"] = rec["y"] @ w["proj"]
    return rec


# ================================================================================================================== whole tower in fp64
GEMM_WEIGHTS = ("conv1.weight", "attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


def openai_vit64(sd, heads, patch, pixels, bf16_gemm=True):
    """openai/CLIP's VisionTransformer.forward restated in fp64 on the device of ``pixels`` from a state dict with openai's names: conv1
    (no bias) -> class token + positional embedding -> ln_pre -> pre-LN residual blocks [ln_1 -> MultiheadAttention ; ln_2 -> Linear ->
    QuickGELU -> Linear] -> ln_post on the class row -> @ proj.  ``bf16_gemm``: the GEMM weights as the bf16 copies the product
    multiplies.  -> (embeddings [B, E], last block's output [B, tokens, W], per block the largest probability of every query [B, H, T])"""
    dev = pixels.device
    p = {}
    for k, v in sd.items():
        v = v.detach()
        if bf16_gemm and k.endswith(GEMM_WEIGHTS):
            v = v.to(torch.bfloat16)
        p[k] = v.to(device=dev, dtype=torch.float64)
    x = pixels.double()
    B, W = x.shape[0], p["class_embedding"].numel()
    x = F.conv2d(x, p["conv1.weight"], stride=patch).reshape(B, W, -1).permute(0, 2, 1)
    x = torch.cat([p["class_embedding"].expand(B, 1, W), x], dim=1) + p["positional_embedding"]
    x = F.layer_norm(x, (W,), p["ln_pre.weight"], p["ln_pre.bias"], EPS)
    T, pmax = x.shape[1], []
    n_layers = 1 + max(int(k.split(".")[2]) for k in p if k.startswith("transformer.resblocks."))
    for i in range(n_layers):
        q = lambda n: p[f"transformer.resblocks.{i}.{n}"]
        h = F.layer_norm(x, (W,), q("ln_1.weight"), q("ln_1.bias"), EPS)
        qkv = (h @ q("attn.in_proj_weight").t() + q("attn.in_proj_bias")).view(B, T, 3, heads, W // heads).permute(2, 0, 3, 1, 4)
        P = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * (W // heads) ** -0.5, dim=-1)
        pmax.append(P.amax(-1))
        x = x + (P @ qkv[2]).permute(0, 2, 1, 3).reshape(B, T, W) @ q("attn.out_proj.weight").t() + q("attn.out_proj.bias")
        h = F.layer_norm(x, (W,), q("ln_2.weight"), q("ln_2.bias"), EPS)
        u = h @ q("mlp.c_fc.weight").t() + q("mlp.c_fc.bias")
        x = x + qgelu64(u) @ q("mlp.c_proj.weight").t() + q("mlp.c_proj.bias")
    y = F.layer_norm(x[:, 0], (W,), p["ln_post.weight"], p["ln_post.bias"], EPS)
    return y @ p["proj"], x, pmax


def distances(hip, emu, ref):
    """per image: |hip - ref|, |emu - ref|, |hip - emu|, each over |ref|; and the same three over the whole batch"""
    hip, emu, ref = hip.double(), emu.double(), ref.double()
    n = ref.norm(dim=1)
    per = torch.stack([(hip - ref).norm(dim=1) / n, (emu - ref).norm(dim=1) / n, (hip - emu).norm(dim=1) / n], dim=1).cpu()
    return per, tuple(float((a - b).norm() / ref.norm()) for a, b in ((hip, ref), (emu, ref), (hip, emu)))


# ================================================================================================================== planted errors
def plant_embed(rec, w, geo):
    """1: the class row of image 1 given pos[1] instead of pos[0] (the kernel's own rows, that one recomputed in fp64 and stored as bf16)"""
    real = real_rows(geo, rec["G"].device)
    ref, bound = embed_ref(rec["G"], w, geo)
    wrong, _ = embed_ref(rec["G"], w, geo, cls_pos=(1, 1))
    good = rec["X0"][real]
    assert _passes(good, ref, bound)[0]
    bad = good.clone()
    bad[geo.tokens] = wrong[geo.tokens].to(torch.bfloat16)
    return rejected("embed: the class row of image 1 takes pos[1]", bad, ref, bound)


def plant_attn(L, geo, tag):
    """2 / 3: the last valid key (256 / 49) removed from the softmax of the real query that gives it the largest reference probability
    -> (error / bound of the planted result, how many bounds the plant moves the reference by at its best element, (image, head, query))"""
    T, key = geo.tokens, geo.tokens - 1
    f, got = attn_ref(L, geo)
    assert _passes(got[:, :T], f["out"][:, :T], f["bound"][:, :T])[0]
    pk = f["P"][:, :T, key]
    n, qi = divmod(int(pk.argmax()), T)
    p = float(pk[n, qi])
    g, _ = attn_ref(L, geo, only=n, drop_key=(0, qi, key))
    move = g["out"][0, qi] - f["out"][n, qi]
    moves = float((move.abs() / f["bound"][n, qi]).max())
    bad = got.double().clone()
    bad[n, qi] += move
    where = (n // geo.H, n % geo.H, qi)
    print(f"SENSITIVITY|{tag}: key {key} has p = {p:.3f} for (image, head, query) {where}; without it the reference moves by {moves:.3g} bounds")
    ratio = rejected(f"{tag}: attention, key {key} removed from query {qi} of image {where[0]}, head {where[1]}",
                     bad[:, :T], f["out"][:, :T], f["bound"][:, :T])
    return ratio, moves, where


def plant_vt_pitch(L, w, i, geo, image=2, pitch=256):
    """4: the V^T block of ``image`` decoded at pitch 256 instead of 264"""
    W = geo.W
    ref, bound = gemm_ref(L["h1"], w[f"l{i}_qkv_w"], w[f"l{i}_qkv_b"])
    ref, bound = ref[:, 2 * W:], bound[:, 2 * W:]
    assert _passes(vt_rows(L["vt"], geo), ref, bound)[0]
    return rejected(f"QKV V^T: image {image} decoded at pitch {pitch}", vt_rows(L["vt"], geo, wrong=(image, pitch)), ref, bound)


def plant_fc1_row(L, w, i, row=256):
    """5: fc1 row 256 replaced by row 255 (its neighbour across the 256-row tile edge)"""
    ref, bound, _ = fc1_ref(L["h2"][row - 1: row + 1], w[f"l{i}_fc1_w"], w[f"l{i}_fc1_b"])
    good = L["ffn"][row - 1: row + 1]
    assert _passes(good, ref, bound)[0]
    bad = good.clone()
    bad[1] = good[0]
    return rejected(f"fc1: row {row} <- row {row - 1}", bad, ref, bound)


def plant_kblock(L, w, i, row, k0=128):
    """6: the k-block k0 .. k0 + 63 missing from ONE element of an out_proj row, each element of the row in turn -> median error / bound"""
    x, Wo = L["ctx"][row: row + 1], w[f"l{i}_o_w"]
    ref, bound = gemm_ref(x, Wo, w[f"l{i}_o_b"], res=L["x"][row: row + 1])
    assert _passes(L["pre"][row: row + 1], ref, bound)[0]
    part = x[0, k0: k0 + 64].double() @ Wo[:, k0: k0 + 64].double().t()
    r = (L["pre"][row].double() - part - ref[0]).abs() / (bound[0] + FTZ)
    med = float(r.median())
    print(f"SENSITIVITY|out_proj: k-block {k0}..{k0 + 63} missing from ONE element of row {row}|error / bound median {med:.3g}, "
          f"min {float(r.min()):.3g}, max {float(r.max()):.3g}; rejected on its own: {float((r > 1).double().mean()):.3f} of {r.numel()}")
    assert med > 1.0, f"a k-block missing from a typical element of out_proj is not rejected (median {med:.3g})"
    return med


def plant_gather(rec, geo):
    """7: the row row0 + 1 gathered instead of row0"""
    X = rec["layers"][-1]["out"]
    r0 = row0_of(geo, X.device)
    ref = X[r0].double()
    assert _passes(rec["cls"], ref, torch.zeros_like(ref))[0]
    return rejected("rows_gather: row0 + 1 instead of row0", X[r0 + 1].float(), ref, torch.zeros_like(ref))


def plant_erf_gelu(L, w, i, row=3):
    """8: u sigmoid(1.702 u) replaced by the erf-GELU on one row"""
    ref, bound, u = fc1_ref(L["h2"][row: row + 1], w[f"l{i}_fc1_w"], w[f"l{i}_fc1_b"])
    assert _passes(L["ffn"][row: row + 1], ref, bound)[0]
    return rejected(f"fc1: row {row} through the erf-GELU", erf_gelu64(u).to(torch.bfloat16), ref, bound)


def planted_suite(name, rec, w, geo, fc1_row=True):
    """every planted error that the case's record supports -> {plant: error / bound}; each must be rejected by the element-wise criterion
    alone (the unperturbed result is asserted to pass first)"""
    L = rec["layers"][0]
    out = {"1 embed": plant_embed(rec, w, geo)}
    r, moves, _ = plant_attn(L, geo, name)
    out["2 attention key 256" if geo.tokens == 257 else "3 attention key 49"] = r
    out["attention plant, bounds moved"] = moves
    if geo.pitch == 264 and geo.B >= 3:
        out["4 V^T pitch"] = plant_vt_pitch(L, w, 0, geo)
        out["6 out_proj k-block (median)"] = plant_kblock(L, w, 0, row=geo.pitch + 36)
    if fc1_row:
        out["5 fc1 row"] = plant_fc1_row(L, w, 0)
    out["7 rows_gather"] = plant_gather(rec, geo)
    out["8 erf-GELU"] = plant_erf_gelu(L, w, 0)
    return out
