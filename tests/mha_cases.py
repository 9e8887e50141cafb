"""Helpers of tests/test_gpu_mha_block.py and tests/test_mha_cases_cpu.py (not collected on their own): the keyword attention block
``LayerNorm(MultiheadAttention(x) + x)`` of speechclip_plus_amd/mha_block.py (MhaNormFn, FfnNormFn, LayerNormFn) stage by stage
against float64.

Nothing of the block is restated for the device.  A recording proxy (test_gpu_trainable_bwd._Rec) stands in for ``mha_block.ops``;
``check_mha`` / ``check_ffn`` / ``check_ln`` walk the recorded calls in the order the block issues them and compare every one,
element by element, with the fp64 definition of that stage on the stage's own recorded inputs.  The references are BY MEANING:
``scores[b, h] = q_h k_h^T`` of the recorded ``qkv`` split per utterance and head on the host, ``ctx[b, h] = Pd[b, h] V_h``,
``dV = Pd^T dctx``, ``dQ = dS K``, ``dK = dS^T Q`` - never a replay of the call's leading dimensions and batch strides, so the
addressing written in mha_block.py is what is under test.  A walker fails on a recorded call it has no reference for.

``EmuOps`` is a CPU stand-in for ``ops`` with the kernels' arithmetic order (fp32 accumulation over 64-wide K-tiles, bf16 at the
storage sites, the stateless hash masks); its ``gemm_raw`` reads and writes through ``torch.as_strided`` with the call's own
strides, so the real mha_block code runs on the CPU under the same proxy and the same walkers: that is where the bounds are shown to
hold before anything runs on the device (tests/test_mha_cases_cpu.py).

Bounds: docs/parity.md, "Keyword attention block".  The constants are the project's (test_gpu_trainable_bwd, test_gpu_frozen_fwd,
kw_cases); what is new is derived there and fixed before the first GPU run."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import kw_cases as kc
from test_gpu_frozen_fwd import EXP_ULP, GELU_FIT, K_EPI, _gelu, _gemm_ref, _keep, _ln_ref
from test_gpu_kernels import _keep_mask
from test_gpu_trainable_bwd import (BF16_RELL2, F32_RELL2, FTZ, KSEC, STORE, U, _check_call, _keff_colsum, _keff_wgrad,
                                    _passes, _Rec, _RoundBF16, _Seq, rel_l2)
from test_gpu_trainable_bwd import _gelu_grad, _ln_ref as _lnb_ref

EPS = 1e-5
BF = torch.bfloat16
ROWS_JUNK = 1e4                  # rows outside a sequence in rows mode: finite, +-1e4 (test_pad_rows_are_never_mixed_in's convention)

# case -> d_model, heads, utterances, sequence length, live keys per utterance            (docs/parity.md: the path each one reaches)
CASES = {
    "base_tn": dict(Dm=768, H=1, B=2, S=500, lens=[500, 193]),
    "tn_min": dict(Dm=256, H=1, B=3, S=200, lens=[200, 129, 1]),
    "base_short": dict(Dm=768, H=1, B=3, S=130, lens=[130, 64, 5]),
    "large8": dict(Dm=1024, H=8, B=2, S=100, lens=[100, 31]),
    "pad96": dict(Dm=192, H=2, B=3, S=70, lens=[70, 59, 2]),
    "pad8": dict(Dm=64, H=8, B=3, S=20, lens=[20, 9, 1]),
}
FFN_CASE = dict(Dm=256, H=2, B=2, S=70, lens=[70, 33], F=1024)
MODE0 = dict(rows=None, rows_out=None, acc=False, p_att=0.0, p_res=0.0, mask="bool", dcls=False, junk=ROWS_JUNK)
# the stage-by-stage runs: (case, mode overrides)
STAGE_RUNS = [
    ("base_tn", dict()), ("base_tn", dict(rows=1, mask="len")), ("base_tn", dict(rows=0, rows_out=1, dcls=True, mask="len")),
    ("base_tn", dict(acc=True, p_att=0.1)),
    ("tn_min", dict()), ("tn_min", dict(rows=1, rows_out=0, acc=True)), ("tn_min", dict(p_res=0.1, mask="len")),
    ("base_short", dict(mask="len")),
    ("large8", dict()), ("large8", dict(rows=1, rows_out=1, mask="len")), ("large8", dict(acc=True, p_att=0.1)),
    ("pad96", dict()), ("pad8", dict(mask="len")),
]


def roundup(x, m):
    return (x + m - 1) // m * m


def mode_of(over):
    m = dict(MODE0)
    m.update(over)
    return SimpleNamespace(**m)


def mode_id(over):
    return "plain" if not over else "-".join(f"{k}{'' if v is True else v}" for k, v in over.items())


def geom(c):
    Dm, H, B, S = c["Dm"], c["H"], c["B"], c["S"]
    Sp, dh_true = roundup(S, 64), Dm // H
    dh = roundup(dh_true, 64)
    return SimpleNamespace(Dm=Dm, H=H, B=B, S=S, Sp=Sp, dh_true=dh_true, dh=dh, D=H * dh, M=B * Sp, lens=list(c["lens"]),
                           tn=Sp % 256 == 0 and dh % 256 == 0, padded=dh != dh_true, scale=dh_true ** -0.5)


# ---------------------------------------------------------------------------------------------------------------- inputs
def bfr(t):
    return t.to(BF).float()


def make_inputs(name, c, seed=0):
    """seeded CPU tensors: fp32 parameters, the bf16-rounded input [B, S, Dm] (frames behind an utterance's live keys hold ordinary
    values: they are masked keys, not zeros), the output gradient (bf16 values, zero on pad frames) and a CLS-row gradient"""
    g = torch.Generator().manual_seed(1000 + 17 * sorted(list(CASES) + ["ffn"]).index(name) + seed)
    Dm, B, S = c["Dm"], c["B"], c["S"]
    r = lambda *s: torch.randn(*s, generator=g)
    prm = {"Wi": r(3 * Dm, Dm) * Dm ** -0.5, "bi": r(3 * Dm) * 0.1, "Wo": r(Dm, Dm) * Dm ** -0.5, "bo": r(Dm) * 0.1,
           "g": 1 + 0.1 * r(Dm), "beta": 0.1 * r(Dm)}
    if "F" in c:
        Fd = c["F"]
        prm.update({"W1": r(Fd, Dm) * Dm ** -0.5, "b1": r(Fd) * 0.1, "W2": r(Dm, Fd) * Fd ** -0.5, "b2": r(Dm) * 0.1, "g2": 1 + 0.1 * r(Dm),
                    "beta2": 0.1 * r(Dm), "g3": 1 + 0.1 * r(Dm), "beta3": 0.1 * r(Dm)})
    x = bfr(r(B, S, Dm))
    live = torch.arange(S)[None, :] < torch.tensor(c["lens"])[:, None]
    dout = bfr(r(B, S, Dm)) * live[:, :, None]
    return SimpleNamespace(prm=prm, x=x, dout=dout, dcls=bfr(r(B, Dm)), live=live)


def padded_weights(Wi, bi, Wo, H, dh):
    """The padded-head working copies by meaning: every head's dh_true rows of the q / k / v projections (columns of the output
    projection) followed by dh - dh_true zero rows (columns) -> Wi_b [3 H dh, Dm] bf16, bi_f [3 H dh] fp32, Wo_b [Dm, H dh] bf16"""
    Dm = Wo.shape[0]
    dt = Dm // H
    Wi_b = torch.zeros(3, H, dh, Dm, device=Wi.device, dtype=Wi.dtype)
    bi_f = torch.zeros(3, H, dh, device=Wi.device, dtype=bi.dtype)
    Wo_b = torch.zeros(Dm, H, dh, device=Wi.device, dtype=Wo.dtype)
    for j in range(3):
        for h in range(H):
            Wi_b[j, h, :dt] = Wi[j * Dm + h * dt: j * Dm + (h + 1) * dt]
            bi_f[j, h, :dt] = bi[j * Dm + h * dt: j * Dm + (h + 1) * dt]
    for h in range(H):
        Wo_b[:, h, :dt] = Wo[:, h * dt: (h + 1) * dt]
    return Wi_b.view(3 * H * dh, Dm), bi_f.view(3 * H * dh), Wo_b.view(Dm, H * dh)


# ---------------------------------------------------------------------------------------------------------------- CPU emulation of ops
def _mm32(A, W):
    """A [.., M, K] . W [.., N, K]^T with fp32 accumulation, K-tile by K-tile (64) in order"""
    K = A.shape[-1]
    acc = None
    for k0 in range(0, K, 64):
        t = A[..., k0: k0 + 64].float() @ W[..., k0: k0 + 64].float().transpose(-1, -2)
        acc = t if acc is None else acc + t
    return acc


def _keep2(rows, cols, p, seed):
    return torch.from_numpy(_keep_mask(np.arange(rows * cols, dtype=np.int64), seed, p)).view(rows, cols).clone()


def emu_ops():
    """a namespace of plain functions with the signatures mha_block uses of ``ops``"""
    def derived_pair(w):
        wb = w.detach().to(BF).contiguous()
        return wb, wb.t().contiguous()

    def aligned16(t):
        return t

    def _num_cus():
        return 256

    def len_mask(lens, n, add=0):
        m = torch.arange(n)[None, :] >= (lens + add)[:, None]
        m._sc_lens = (lens, int(add))
        return m

    def gemm_raw(A, lda, W, ldw, C, ldc, M, N, K, out_f32=False, nb1=1, nb2=1, sA=(0, 0), sW=(0, 0), sC=(0, 0), tn=False):
        if tn:      # both operands row-indexed by the reduction
            Av = torch.as_strided(A, (nb1, nb2, K, M), (sA[0], sA[1], lda, 1), A.storage_offset()).transpose(-1, -2)
            Wv = torch.as_strided(W, (nb1, nb2, K, N), (sW[0], sW[1], ldw, 1), W.storage_offset()).transpose(-1, -2)
        else:
            Av = torch.as_strided(A, (nb1, nb2, M, K), (sA[0], sA[1], lda, 1), A.storage_offset())
            Wv = torch.as_strided(W, (nb1, nb2, N, K), (sW[0], sW[1], ldw, 1), W.storage_offset())
        Cv = torch.as_strided(C, (nb1, nb2, M, N), (sC[0], sC[1], ldc, 1), C.storage_offset())
        assert C.dtype == (torch.float32 if out_f32 else BF)
        Cv.copy_(_mm32(Av, Wv).to(C.dtype))
        return 0

    def linear_bf16(x, w, bias=None, out=None, residual=None, drop_p=0.0, drop_seed=0):
        acc = _mm32(x, w)
        if bias is not None:
            acc = acc + bias
        if drop_p > 0.0:
            keep = _keep2(x.shape[0], w.shape[0], drop_p, drop_seed)
            acc = torch.where(keep, acc * torch.tensor(1.0 / (1.0 - drop_p), dtype=torch.float32), torch.zeros(()))
        if residual is not None:
            acc = acc + residual.float()
        if out is None:
            return acc.to(BF)
        out.copy_(acc.to(BF))
        return out

    def softmax_fwd(scores, key_mask, rows_per_batch, scale, drop_p=0.0, drop_seed=0):
        n = scores.shape[-1]
        P32 = kc.softmax_ref(scores.reshape(-1, n), key_mask.reshape(-1, n).bool(), rows_per_batch, kc.f32(scale))
        P = P32.to(BF).view(scores.shape)
        if drop_p == 0.0:
            return P, P
        keep = kc.softmax_keep(P32.shape[0], n, drop_p, drop_seed)
        Pd = torch.where(keep, P32 * torch.tensor(1.0 / (1.0 - drop_p), dtype=torch.float32), torch.zeros(())).to(BF)
        return P, Pd.view(scores.shape)

    def softmax_bwd(dP, P, scale, drop_p=0.0, drop_seed=0):
        n = dP.shape[-1]
        keep = kc.softmax_keep(dP.numel() // n, n, drop_p, drop_seed)
        return kc.softmax_bwd_formula(dP.reshape(-1, n), P.float().reshape(-1, n), kc.f32(scale), keep, drop_p).to(BF).view(P.shape)

    def transpose_bf16(x, out=None):
        return x.t().contiguous()

    def layernorm_bf16(x, gamma, beta, out=None, eps=1e-5):
        y = F.layer_norm(x.float(), (x.shape[1],), gamma, beta, eps).to(BF)
        if out is None:
            return y
        out.copy_(y)
        return out

    def layernorm_bwd(x, dy, gamma, eps, want_param_grads=False, acc=None):
        xf, dyf = x.float(), dy.float()
        xc = xf - xf.mean(1, keepdim=True)
        rstd = ((xc * xc).mean(1, keepdim=True) + eps).rsqrt()
        xh = xc * rstd
        gd = gamma * dyf
        dx = (rstd * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True))).to(BF)
        dg, db = (dyf * xh).sum(0), dyf.sum(0)
        if acc is not None:
            acc[0].add_(dg)
            acc[1].add_(db)
            return dx
        return (dx, dg, db) if want_param_grads else dx

    def dropout_bf16(x, p, seed, out=None):
        keep = _keep2(x.shape[0], x.shape[1], p, seed)
        y = torch.where(keep, x.float() / (1 - p), torch.zeros(())).to(BF)
        if out is None:
            return y
        out.copy_(y)
        return out

    def wgrad_bf16(dy, x, gW, gb=None, beta=1.0):
        acc = None
        for r0 in range(0, dy.shape[0], 64):
            t = dy[r0: r0 + 64].float().t() @ x[r0: r0 + 64].float()
            acc = t if acc is None else acc + t
        cs = dy.float().sum(0)
        if beta == 0.0:
            gW.copy_(acc)
            if gb is not None:
                gb.copy_(cs)
        else:
            gW.mul_(beta).add_(acc)
            if gb is not None:
                gb.mul_(beta).add_(cs)

    def act_bf16(u, act, df=None, out=None):
        assert act == 1
        uf = u.float()
        y = (F.gelu(uf) if df is None else df.float() * _gelu_grad(uf.double()).float()).to(BF)
        if out is None:
            return y
        out.copy_(y)
        return out

    def rows_zero_pad(flat, lead, B, P, head, stop, trail):
        flat[kc.zero_pad_rows(lead, B, P, head, stop, trail)] = 0

    return SimpleNamespace(**{k: v for k, v in locals().items() if callable(v)})


# ---------------------------------------------------------------------------------------------------------------- running the block
def build_module(c, prm, dev, p_att=0.0):
    from speechclip_plus_amd.transformer_models import MultiheadAttentionAndNorm
    mod = MultiheadAttentionAndNorm(c["Dm"], c["H"], dropout=p_att).to(dev)
    att, norm = mod.multihead_attn_layer, mod.attentionBlock_Norm
    with torch.no_grad():
        for p, k in ((att.in_proj_weight, "Wi"), (att.in_proj_bias, "bi"), (att.out_proj.weight, "Wo"), (att.out_proj.bias, "bo"),
                     (norm.weight, "g"), (norm.bias, "beta")):
            p.copy_(prm[k])
    return mod


def mha_params(mod):
    att, norm = mod.multihead_attn_layer, mod.attentionBlock_Norm
    return {"Wi": att.in_proj_weight, "bi": att.in_proj_bias, "Wo": att.out_proj.weight, "bo": att.out_proj.bias, "g": norm.weight,
            "beta": norm.bias}


def key_mask(mb, c, dev, kind):
    lens = torch.tensor(c["lens"], dtype=torch.int64, device=dev)
    if kind == "len":
        return mb.ops.len_mask(lens, c["S"], 0)
    return torch.arange(c["S"], device=dev)[None, :] >= lens[:, None]


def run_mha(mb, rec, c, inp, dev, mode, x=None, junk_seed=5):
    """One forward + backward of the block in ``mode`` under the recording proxy ``rec`` (= mb.ops).  On the device the module-level
    API is used (MultiheadAttentionAndNorm.forward / forward_rows); ``p_res`` exists only behind mha_block.mha_norm (the call
    TransformerEncoder._layer makes), and the CPU emulation calls mha_norm too: the modules refuse host tensors.
    -> out, dx, {parameter: gradient (acc mode: post minus pre)}, the recorded forward and backward calls"""
    G = geom(c)
    B, S, Sp, Dm, M = G.B, G.S, G.Sp, G.Dm, G.M
    train = mode.p_att > 0 or mode.p_res > 0 or mode.rows_out is not None
    mod = build_module(c, inp.prm, dev, mode.p_att).train(train)
    prm = mha_params(mod)
    kpm = key_mask(mb, c, dev, mode.mask)
    x = (inp.x if x is None else x).to(dev)
    buf = None
    if mode.rows is None:
        xin = x.clone().requires_grad_()
        leaf = xin
    else:
        off = mode.rows
        g = torch.Generator().manual_seed(junk_seed)
        sign = (torch.randint(0, 2, (M + off, Dm), generator=g) * 2 - 1).to(BF)
        buf = (sign * mode.junk).to(dev)                       # includes the ``off`` rows the last utterance reads behind the buffer
        src0 = buf[:M].view(B, Sp, Dm)
        src0[:, off: off + S] = x.to(BF)
        leaf = buf.requires_grad_()
        src = leaf[:M].view(B, Sp, Dm)
        xin = src[:, off: off + S]
        xin._sc_handle = SimpleNamespace(src=src, inplace_ok=True)
    pre = None
    if mode.acc:        # the optimiser's layout: every gradient a view of one flat fp32 buffer, tagged as FlatAdam tags its views
        g = torch.Generator().manual_seed(77)
        n = sum(p.numel() for p in prm.values())
        flat = (0.01 * torch.randn(n, generator=g)).to(dev)
        pre, o = {}, 0
        for k, p in prm.items():
            p.grad = flat[o: o + p.numel()].view(p.shape)
            p.grad._sc_flat = True
            pre[k] = p.grad.clone()
            o += p.numel()
    torch.manual_seed(1234)
    mb._calls = 0
    rec.calls, rec.on = [], True
    att, norm = mod.multihead_attn_layer, mod.attentionBlock_Norm
    api = dev.type == "cuda" and mode.p_res == 0.0
    if mode.rows_out is None:
        res = mod(xin, kpm) if api else mb.mha_norm(xin, att, norm, kpm, train, p_res=mode.p_res, out_dtype=torch.float32)
    else:
        res = mod.forward_rows(xin, kpm, mode.rows_out) if api else mb.mha_norm(xin, att, norm, kpm, train, rows_out=mode.rows_out)
    fwd, rec.calls = rec.calls, []
    r = SimpleNamespace(G=G, mode=mode, prm={k: p.detach().clone() for k, p in prm.items()}, x=x, kpm=kpm, dy_rows=None, buf=None)
    if mode.rows_out is None:
        r.out = res.detach().clone()
        res.backward(inp.dout.to(dev))
    else:
        br, cls_rows = res
        n_cls = mode.rows_out
        assert (br.head, br.S, br.lead, br.trail) == (n_cls, S - n_cls, mb.ROWS_LEAD, mb.ROWS_TRAIL)
        r.out, r.cls = br.full.detach().clone(), None if cls_rows is None else cls_rows.detach().clone()
        dy = torch.zeros(B, Sp, Dm, dtype=BF, device=dev)
        dy[:, n_cls: S] = inp.dout[:, n_cls:].to(BF)
        r.dy_rows = dy.clone()
        if n_cls:
            r.dy_rows[:, 0] += inp.dcls.to(dev).to(BF) if mode.dcls else 0
            torch.autograd.backward([br.full, cls_rows], [dy, inp.dcls.to(dev) if mode.dcls else torch.zeros_like(cls_rows)])
        else:
            br.full.backward(dy)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    r.fwd, r.bwd = fwd, rec.calls
    rec.calls, rec.on = [], False
    if mode.rows is None:
        r.dx = leaf.grad.detach().clone()
    else:
        r.dx = leaf.grad[:M].view(B, Sp, Dm).detach().clone()           # the gradient in the buffer's own layout
        r.buf = leaf.detach()
    r.grads = {k: (p.grad.double() - pre[k].double() if mode.acc else p.grad).detach().clone() for k, p in prm.items()}       # acc: post minus pre, exact
    r.pre = pre
    for p in prm.values():
        p.grad = None
    return r


def build_encoder(c, prm, dev, p):
    from speechclip_plus_amd.transformer_models import TransformerEncoder
    enc = TransformerEncoder(1, c["Dm"], c["H"], c["F"], dropout=p).to(dev)
    L, n = enc.model.layers[0], enc.model.norm
    with torch.no_grad():
        for q, k in ((L.self_attn.in_proj_weight, "Wi"), (L.self_attn.in_proj_bias, "bi"), (L.self_attn.out_proj.weight, "Wo"),
                     (L.self_attn.out_proj.bias, "bo"), (L.norm1.weight, "g"), (L.norm1.bias, "beta"), (L.linear1.weight, "W1"),
                     (L.linear1.bias, "b1"), (L.linear2.weight, "W2"), (L.linear2.bias, "b2"), (L.norm2.weight, "g2"),
                     (L.norm2.bias, "beta2"), (n.weight, "g3"), (n.bias, "beta3")):
            q.copy_(prm[k])
    return enc


def encoder_params(enc):
    L, n = enc.model.layers[0], enc.model.norm
    return {"Wi": L.self_attn.in_proj_weight, "bi": L.self_attn.in_proj_bias, "Wo": L.self_attn.out_proj.weight, "bo": L.self_attn.out_proj.bias,
            "g": L.norm1.weight, "beta": L.norm1.bias, "W1": L.linear1.weight, "b1": L.linear1.bias, "W2": L.linear2.weight,
            "b2": L.linear2.bias, "g2": L.norm2.weight, "beta2": L.norm2.bias, "g3": n.weight, "beta3": n.bias}


def run_encoder(mb, rec, c, inp, dev, p):
    """TransformerEncoder.forward (one post-LN layer: MhaNormFn with residual dropout, FfnNormFn, then LayerNormFn); on the host the
    same three calls are made directly (the module refuses host tensors)"""
    G = geom(c)
    enc = build_encoder(c, inp.prm, dev, p).train(p > 0)
    prm = encoder_params(enc)
    kpm = key_mask(mb, c, dev, "bool")
    xin = inp.x.to(dev).clone().requires_grad_()
    torch.manual_seed(4321)
    mb._calls = 0
    rec.calls, rec.on = [], True
    if dev.type == "cuda":
        out = enc(xin, kpm)
    else:
        out = enc._layer(enc.model.layers[0], xin.float(), kpm)
        out = mb.LayerNormFn.apply(out, enc.model.norm.weight, enc.model.norm.bias, enc.model.norm.eps)
    fwd, rec.calls = rec.calls, []
    out.backward(inp.dout.to(dev))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    r = SimpleNamespace(G=G, mode=mode_of(dict(p_att=p, p_res=p)), prm={k: q.detach().clone() for k, q in prm.items()}, x=inp.x.to(dev), kpm=kpm,
                        out=out.detach().clone(), dx=xin.grad.clone(), grads={k: q.grad.clone() for k, q in prm.items()}, fwd=fwd,
                        bwd=rec.calls, dy_rows=None, buf=None, pre=None, p=p)
    rec.calls, rec.on = [], False
    return r


# ---------------------------------------------------------------------------------------------------------------- criteria
class Report:
    """largest error / bound per stage and where it occurred, printed in the style of [frozen-fwd]"""

    def __init__(self, tag):
        self.tag, self.rows = tag, {}

    def check(self, stage, got, ref, bound, rell2=None):
        ok, ratio, e = _passes(got, ref, bound, rell2)
        old = self.rows.get(stage, (-1.0, 0.0, ""))
        if ratio > old[0]:
            d = (got.double() - ref).abs() / (bound + FTZ)
            where = np.unravel_index(int(torch.nan_to_num(d, nan=float("inf")).argmax()), tuple(d.shape)) if d.numel() else ()
            self.rows[stage] = (ratio, max(old[1], e), str(tuple(int(i) for i in where)))
        else:
            self.rows[stage] = (old[0], max(old[1], e), old[2])
        assert ok, f"{self.tag} / {stage}: largest error / bound {ratio:.3g} at {self.rows[stage][2]}, rel-L2 {e:.3g} (criterion {rell2})"

    def exact(self, stage, ok):
        assert bool(ok), f"{self.tag} / {stage}: not exact"
        self.rows.setdefault(stage + " (exact)", (0.0, 0.0, ""))

    def show(self):
        for k, v in self.rows.items():
            r, e, w = v if len(v) == 3 else (v[0], v[1], "")
            print(f"[mha-block] {self.tag:>28s} {k:40s} max err/bound {r:8.3g} at {w:18s} rel-L2 {e:9.3g}")


def prod_bound(A, Wm, K, bf16_out, ref):
    """a batched bf16 product ``A @ Wm`` with fp32 accumulation over K (+ K_EPI epilogue operations), stored fp32 or bf16"""
    b = KSEC * U * (K + K_EPI) * (A.abs() @ Wm.abs())
    return b + STORE * ref.abs() if bf16_out else b


def softmax_fwd_bound(scores, mask, rpb, scale, P64):
    """fp32 row softmax of v = scale s behind the key mask, P = e / sum e, e = exp(v - m): the argument carries the roundings of v, of
    m (itself one of the v), of the difference, of the conversion to the exp2 instruction's argument and of the fp32 scale (common
    to v and m: it acts on the difference):
    eps_i = u (|v_i| + |m| + 3 |v_i - m| + EXP_ULP + 4) relative on e_i (+ 4: the reciprocal of the sum, its product, two spare);
    the sum inherits sum_j P_j eps_j and its own k additions (a lane's chain, six shuffle levels - the k of
    kw_cases.softmax_bwd_bound).  Masked keys: exactly zero."""
    live = ~mask.repeat_interleave(rpb, dim=0)
    v = scores.double() * scale
    m = torch.where(live, v, torch.full_like(v, float("-inf"))).amax(-1, keepdim=True)
    z = torch.zeros_like(v)
    eps = torch.where(live, U * (v.abs() + m.abs() + 3 * (v - m).abs() + EXP_ULP + 4), z)
    n = scores.shape[-1]
    k = 4 * ((n // 4 + 63) // 64) + 6 + 2
    # (a live key is no structural zero even where its probability underflows in fp64: the floor keeps its bound above 0)
    return torch.where(live, (KSEC * P64 * (eps + (P64 * eps).sum(-1, keepdim=True) + k * U)).clamp_min(2.0 ** -200), z)


def keff_wgrad(ops, rows, N, K):
    """serial fp32 length of ops.wgrad_bf16: the TN form (test_gpu_trainable_bwd._keff_wgrad), else the transposing form's equal slices"""
    if N % 256 == 0 and K % 256 == 0:
        return _keff_wgrad(ops, rows, N, K)
    tiles = -(-N // 256) * -(-K // 256)
    S = max(1, min(256 // tiles, rows // 512))
    return -(-rows // (64 * S)) * 64 + S


def check_wgrad(rep, ops, c, where):
    """ops.wgrad_bf16 as test_gpu_trainable_bwd._check_call checks it (post - beta pre against dy^T x), for either form of the kernel;
    beta = 1 into a non-zero target: the slice reduction starts from the target's value, one more addend of that magnitude, and
    post - pre is formed behind a rounding at |post|: + KSEC u (|pre| + |post|)"""
    dy, x = c.a[0].double(), c.a[1].double()
    beta = c.kw["beta"]
    rows, N = dy.shape
    keff = keff_wgrad(ops, rows, N, x.shape[1])
    for name, pre, post, ref, mag, k in (("weight", c.a[2], c.pa[2], dy.t() @ x, dy.abs().t() @ x.abs(), keff),
                                         ("bias", c.a[3], c.pa[3], dy.sum(0), dy.abs().sum(0), _keff_colsum(rows))):
        bound = KSEC * U * k * mag
        got = post.double()
        if beta != 0.0:
            got = got - beta * pre.double()
            bound = bound + KSEC * U * (pre.double().abs() + post.double().abs())
        rep.check(f"{where} {name} gradient", got, ref, bound, F32_RELL2)


def check_ln_bwd(rep, c, where):
    """ops.layernorm_bwd by test_gpu_trainable_bwd._ln_ref; ``acc`` targets as in check_wgrad -> dx as the kernel returned it"""
    dx_r, bdx, dg_r, bdg, db_r, bdb, _ = _lnb_ref(c.a[0], c.a[1], c.a[2])
    assert abs(c.a[3] - EPS) < 1e-12
    if "acc" in c.kw:
        dx = c.ret
        for name, i, ref, b in (("dgamma", 0, dg_r, bdg), ("dbeta", 1, db_r, bdb)):
            pre, post = c.kw["acc"][i].double(), c.pkw["acc"][i].double()
            rep.check(f"{where} LayerNorm' {name}", post - pre, ref, b + KSEC * U * (pre.abs() + post.abs()), F32_RELL2)
    else:
        dx, dg, db = c.ret
        rep.check(f"{where} LayerNorm' dgamma", dg, dg_r, bdg, F32_RELL2)
        rep.check(f"{where} LayerNorm' dbeta", db, db_r, bdb, F32_RELL2)
    rep.check(f"{where} LayerNorm' dx", dx, dx_r, bdx)
    return dx


def _heads(t, G):
    """[M, H dh] -> [B, H, Sp, dh] fp64: utterance b = rows b Sp .., head h = columns h dh .."""
    return t.double().reshape(G.B, G.Sp, G.H, G.dh).permute(0, 2, 1, 3)


def _unheads(t, G):
    return t.permute(0, 2, 1, 3).reshape(G.M, G.D)


# ---------------------------------------------------------------------------------------------------------------- the walkers
def check_mha(rep, ops, sf, sb, r, x_in=None, dy_in=None):
    """MhaNormFn's recorded forward (``sf``) and backward (``sb``, both _Seq) against fp64, stage by stage.  ``x_in`` [B, S, Dm]: what
    the block was fed; ``dy_in``: the gradient it was handed.  -> the stage results the sensitivity checks plant errors into"""
    G, mode, prm = r.G, r.mode, r.prm
    B, S, Sp, H, dh, D, Dm, M = G.B, G.S, G.Sp, G.H, G.dh, G.D, G.Dm, G.M
    dev = prm["Wi"].device
    rig = SimpleNamespace(ops=ops)
    st = SimpleNamespace(G=G)
    lens = torch.tensor(G.lens, device=dev)
    key_pad = torch.arange(Sp, device=dev)[None, :] >= lens[:, None]                    # [B, Sp] True = padded key
    # ---- working copies
    if not G.padded:
        Wb = []
        for k in ("Wi", "Wo"):
            c = sf.take("derived_pair")
            rep.exact(f"{k} working copies", torch.equal(c.ret[0], prm[k].to(BF)) and torch.equal(c.ret[1], c.ret[0].t().contiguous()))
            Wb.append(c.ret)
        (Wi_b, WiT), (Wo_b, WoT) = Wb
        bi_f = prm["bi"]
    else:
        Wi_b, bi_f, Wo_b = padded_weights(prm["Wi"].to(BF), prm["bi"], prm["Wo"].to(BF), H, dh)
        WiT, WoT = Wi_b.t().contiguous(), Wo_b.t().contiguous()
    # ---- in_proj
    c = sf.take("linear_bf16")
    xb = c.a[0]
    rep.exact("in_proj operands", torch.equal(c.a[1], Wi_b) and torch.equal(c.a[2], bi_f) and tuple(xb.shape) == (M, Dm))
    if x_in is not None:
        rep.exact("x_b = bf16(x) at the block's pitch", torch.equal(xb.view(B, Sp, Dm)[:, :S], x_in.to(BF)))
    if mode.rows is None:
        rep.exact("x_b pad rows zero", bool((xb.view(B, Sp, Dm)[:, S:] == 0).all()))
    ref, bound = _gemm_ref(xb, Wi_b, bi_f)
    qkv = c.ret
    rep.check("qkv = x_b Wi^T + bi", qkv, ref, bound, BF16_RELL2)
    Q, K, V = (_heads(qkv[:, j * D: (j + 1) * D], G) for j in range(3))
    # ---- scores
    c = sf.take("gemm_raw")
    assert c.kw.get("out_f32") and not c.kw.get("tn")
    scores = c.pa[4]
    ref = Q @ K.transpose(-1, -2)
    rep.check("scores[b, h] = q_h k_h^T", scores, ref, prod_bound(Q, K.transpose(-1, -2), dh, False, ref))
    st.saw_len_mask = sf.c[sf.i].name == "len_mask"
    if st.saw_len_mask:
        c = sf.take("len_mask")
        rep.exact("len_mask", torch.equal(c.ret.bool(), torch.arange(c.a[1], device=dev)[None, :] >= (c.a[0] + c.a[2])[:, None])
                  and torch.equal(c.ret.bool(), key_pad))
    # ---- softmax (+ dropout)
    c = sf.take("softmax_fwd")
    p, seed = c.a[4], c.a[5]
    rep.exact("softmax operands", torch.equal(c.a[0], scores) and torch.equal(c.a[1].bool(), key_pad) and c.a[2] == H * Sp
              and abs(c.a[3] - G.scale) < 1e-15 and p == mode.p_att)
    P, Pd = c.ret
    s2, m2 = scores.view(B * H * Sp, Sp), key_pad
    P64 = kc.softmax_ref(s2.double(), m2, H * Sp, c.a[3])
    bP = softmax_fwd_bound(s2, m2, H * Sp, c.a[3], P64)
    one = (~key_pad).sum(1) == 1                                                          # utterances with one live key: P exactly 1
    one_rows = one.repeat_interleave(H * Sp)
    bP_store = torch.where(one_rows[:, None], torch.zeros_like(bP), bP + STORE * P64)
    rep.check("P = softmax(scale scores | mask)", P.view(B * H * Sp, Sp), P64, bP_store)
    keep = kc.softmax_keep(B * H * Sp, Sp, p, seed).to(dev)
    if p > 0:
        Pd_ref = torch.where(keep, P64 / (1.0 - p), torch.zeros_like(P64))
        bd = torch.where(keep, (bP + 2 * U * P64) / (1.0 - p) + STORE * Pd_ref, torch.zeros_like(P64))
        rep.check("Pd = keep P / (1 - p)", Pd.view(B * H * Sp, Sp), Pd_ref, bd)
        assert 0.85 < float(keep.double().mean()) < 0.95
    else:
        rep.exact("Pd is P", torch.equal(P, Pd))
    rep.exact("P, Pd zero at pad keys", bool((P.view(B, H * Sp, Sp)[key_pad[:, None, :].expand(B, H * Sp, Sp)] == 0).all())
              and bool((Pd.view(B, H * Sp, Sp)[key_pad[:, None, :].expand(B, H * Sp, Sp)] == 0).all()))
    st.P, st.scores, st.key_pad, st.softmax_scale = (P.view(B * H * Sp, Sp), P64, bP_store), s2, key_pad, c.a[3]
    # ---- context
    c = sf.take("transpose_bf16")
    rep.exact("V^T", torch.equal(c.ret, qkv[:, 2 * D:].t()))
    c = sf.take("gemm_raw")
    cx = c.pa[4]
    Pd64 = Pd.double()
    ref = Pd64 @ V
    st.ctx, st.Pd, st.V = (_heads(cx, G), ref, prod_bound(Pd64, V, Sp, True, ref)), Pd64, V
    rep.check("ctx[b, h] = Pd V_h", *st.ctx)
    # ---- out_proj + residual (+ dropout), LayerNorm
    c = sf.take("linear_bf16")
    p_res, seed_res = c.kw.get("drop_p", 0.0), c.kw.get("drop_seed", 0)
    rep.exact("out_proj operands", torch.equal(c.a[0], cx) and torch.equal(c.a[1], Wo_b) and torch.equal(c.a[2], prm["bo"])
              and torch.equal(c.kw["residual"], xb) and p_res == mode.p_res)
    keep_res = _keep(M, Dm, p_res, seed_res, dev) if p_res > 0 else None
    ref, bound = _gemm_ref(cx, Wo_b, prm["bo"], res=xb, keep=keep_res, p=p_res)
    pre = c.ret
    rep.check("pre = drop(ctx Wo^T + bo) + x_b", pre, ref, bound, BF16_RELL2)
    for k in ("g", "beta"):
        c = sf.take("aligned16")
        rep.exact(f"aligned16 {k}", torch.equal(c.ret, prm[k]))
    c = sf.take("layernorm_bf16")
    rep.exact("LayerNorm operands", torch.equal(c.a[0], pre) and abs(c.kw["eps"] - EPS) < 1e-12)
    ref, bound = _ln_ref(pre, prm["g"], prm["beta"])
    out = c.ret
    rep.check("out = LayerNorm(pre)", out, ref, bound, BF16_RELL2)
    st.out_rows = out
    if mode.rows_out is not None:
        c = sf.take("rows_zero_pad")
        lead, trail = c.a[1], c.a[6]
        z = kc.zero_pad_rows(lead, B, Sp, mode.rows_out, S, trail).to(dev)
        rep.exact("rows_zero_pad", c.a[2:6] == (B, Sp, mode.rows_out, S) and bool((c.pa[0][z] == 0).all())
                  and torch.equal(c.pa[0][~z], c.a[0][~z]) and torch.equal(c.a[0][lead: lead + M], out))
        st.flat = c.pa[0]
    # =============================================================================================================== backward
    c = sb.take("layernorm_bwd")
    rep.exact("LayerNorm' operands", torch.equal(c.a[0], pre) and torch.equal(c.a[2], prm["g"]))
    dy = c.a[1]
    if dy_in is not None:
        want = torch.zeros(B, Sp, Dm, device=dev, dtype=BF)
        want[:, :dy_in.shape[1]] = dy_in.to(BF)
        rep.exact("dy = the consumer's gradient, zero pad rows", torch.equal(dy.view(B, Sp, Dm), want))
    st.acc = "acc" in c.kw
    dpre = check_ln_bwd(rep, c, "norm")
    dbr = dpre
    if mode.p_res > 0:
        c = sb.take("dropout_bf16")
        rep.exact("residual dropout' operands", torch.equal(c.a[0], dpre) and c.a[1] == p_res and c.a[2] == seed_res)
        _check_call(rep, rig, c, "residual")
        dbr = c.ret
    c = sb.take("wgrad_bf16")
    rep.exact("out_proj wgrad operands", torch.equal(c.a[0], dbr) and torch.equal(c.a[1], cx))
    st.acc = st.acc and c.kw["beta"] == 1.0
    check_wgrad(rep, ops, c, "out_proj")
    st.gWo = c.pa[2].double() - c.kw["beta"] * c.a[2].double()
    c = sb.take("linear_bf16")
    rep.exact("out_proj dgrad operands", torch.equal(c.a[0], dbr) and torch.equal(c.a[1], WoT))
    _check_call(rep, rig, c, "out_proj")
    dcx = c.ret
    dC = _heads(dcx, G)
    # ---- dP, dS
    c = sb.take("gemm_raw")
    assert c.kw.get("out_f32") and not c.kw.get("tn")
    dP = c.pa[4]
    ref = dC @ V.transpose(-1, -2)
    rep.check("dP = dctx_h V_h^T", dP, ref, prod_bound(dC, V.transpose(-1, -2), dh, False, ref))
    c = sb.take("softmax_bwd")
    rep.exact("softmax' operands", torch.equal(c.a[0], dP) and torch.equal(c.a[1], P) and c.a[2] == st.softmax_scale and c.a[3] == p
              and c.a[4] == seed)
    dP2, Pf = dP.view(B * H * Sp, Sp).double(), P.view(B * H * Sp, Sp).double()
    ref = kc.softmax_bwd_formula(dP2, Pf, c.a[2], keep, p)
    bound = kc.softmax_bwd_bound(dP2, Pf, c.a[2], keep, p)
    bound = torch.where(one_rows[:, None], torch.zeros_like(bound), bound)
    dS = c.ret
    rep.check("dS = scale P (dP' - sum P dP')", dS.view(B * H * Sp, Sp), ref, bound)
    dS64 = dS.double()
    # ---- dV, dQ, dK
    st.saw_tn = []

    def tn_or_transposed(A, Wcols, what):
        if G.tn:
            c = sb.take("gemm_raw")
            st.saw_tn.append(bool(c.kw.get("tn")))
            return c
        c = sb.take("transpose_bf16")
        rep.exact(f"{what}: A^T", torch.equal(c.ret, A.view(B * H * Sp, Sp).t()))
        c = sb.take("transpose_bf16")
        rep.exact(f"{what}: W^T", torch.equal(c.ret, Wcols.t()))
        c = sb.take("gemm_raw")
        st.saw_tn.append(bool(c.kw.get("tn")))
        return c

    c = tn_or_transposed(Pd, dcx, "dV")
    ref = Pd64.transpose(-1, -2) @ dC
    st.dV, st.dctx = (_heads(c.pa[4], G), ref, prod_bound(Pd64.transpose(-1, -2), dC, Sp, True, ref)), dC
    rep.check("dV = Pd^T dctx" + (" (TN)" if G.tn else ""), *st.dV)
    dv_cols = c.pa[4]
    c = sb.take("transpose_bf16")
    rep.exact("K^T", torch.equal(c.ret, qkv[:, D: 2 * D].t()))
    c = sb.take("gemm_raw")
    assert not c.kw.get("tn")
    dq_cols = c.pa[4][:, :D]
    ref = dS64 @ K
    st.dQ = (_heads(dq_cols, G), ref, prod_bound(dS64, K, Sp, True, ref))
    rep.check("dQ = dS K", *st.dQ)
    c = tn_or_transposed(dS, qkv[:, :D], "dK")
    dk_cols = c.pa[4]
    ref = dS64.transpose(-1, -2) @ Q
    rep.check("dK = dS^T Q" + (" (TN)" if G.tn else ""), _heads(dk_cols, G), ref, prod_bound(dS64.transpose(-1, -2), Q, Sp, True, ref))
    assert st.saw_tn == [G.tn, G.tn]
    # ---- in_proj
    c = sb.take("wgrad_bf16")
    dqkv = c.a[0]
    rep.exact("dqkv = [dQ | dK | dV] as the three products left them", torch.equal(dqkv, torch.cat([dq_cols, dk_cols, dv_cols], 1))
              and torch.equal(c.a[1], xb))
    pad_row = (torch.arange(Sp, device=dev)[None, :] >= lens[:, None]).reshape(M)
    if dy_in is not None:
        rep.exact("dqkv zero on pad rows", bool((dqkv[pad_row] == 0).all()))
    check_wgrad(rep, ops, c, "in_proj")
    c = sb.take("linear_bf16")
    rep.exact("in_proj dgrad operands", torch.equal(c.a[0], dqkv) and torch.equal(c.a[1], WiT) and torch.equal(c.kw["residual"], dpre))
    _check_call(rep, rig, c, "in_proj + residual")
    x_, w_ = c.a[0].double(), c.a[1].double()
    ref = x_ @ w_.t() + dpre.double()
    st.dx = (c.ret, ref, KSEC * x_.shape[1] * U * (x_.abs() @ w_.abs().t()) + STORE * ref.abs())       # _check_call's own bound
    if dy_in is not None:
        rep.exact("dx zero on pad rows", bool((c.ret[pad_row] == 0).all()))
    return st


def check_ffn(rep, ops, sf, sb, r, p):
    """FfnNormFn's recorded calls; the ``sb`` portion ends where the attention block's backward begins"""
    prm, G = r.prm, r.G
    dev = prm["W1"].device
    rig = SimpleNamespace(ops=ops)
    M, Dm = G.M, G.Dm
    c = sf.take("linear_bf16")
    xb, W1b, W2b = c.a[0], prm["W1"].to(BF), prm["W2"].to(BF)
    rep.exact("fc1 operands", torch.equal(c.a[1], W1b) and torch.equal(c.a[2], prm["b1"]) and bool((xb.view(G.B, G.Sp, Dm)[:, G.S:] == 0).all()))
    ref, bound = _gemm_ref(xb, W1b, prm["b1"])
    u = c.ret
    rep.check("ffn u = x_b W1^T + b1", u, ref, bound, BF16_RELL2)
    c = sf.take("act_bf16")
    rep.exact("GELU operands", torch.equal(c.a[0], u) and c.a[1] == 1)
    ref = _gelu(u.double())
    f = c.ret
    rep.check("ffn f = gelu(u)", f, ref, STORE * ref.abs() + GELU_FIT)
    if p > 0:
        c = sf.take("dropout_bf16")
        rep.exact("ffn dropout 1 operands", torch.equal(c.a[0], f) and c.a[1] == p)
        _check_call(rep, rig, c, "ffn dropout 1")
        f, seed1 = c.ret, c.a[2]
    c = sf.take("linear_bf16")
    p2, seed2 = c.kw.get("drop_p", 0.0), c.kw.get("drop_seed", 0)
    rep.exact("fc2 operands", torch.equal(c.a[0], f) and torch.equal(c.a[1], W2b) and torch.equal(c.a[2], prm["b2"])
              and torch.equal(c.kw["residual"], xb) and p2 == p)
    ref, bound = _gemm_ref(f, W2b, prm["b2"], res=xb, keep=_keep(M, Dm, p, seed2, dev) if p > 0 else None, p=p)
    pre = c.ret
    rep.check("ffn pre = drop(f W2^T + b2) + x_b", pre, ref, bound, BF16_RELL2)
    c = sf.take("layernorm_bf16")
    rep.exact("ffn LayerNorm operands", torch.equal(c.a[0], pre) and torch.equal(c.a[1], prm["g2"]) and torch.equal(c.a[2], prm["beta2"]))
    ref, bound = _ln_ref(pre, prm["g2"], prm["beta2"])
    rep.check("ffn out = LayerNorm(pre)", c.ret, ref, bound, BF16_RELL2)
    # ---- backward
    c = sb.take("layernorm_bwd")
    rep.exact("ffn LayerNorm' operands", torch.equal(c.a[0], pre) and torch.equal(c.a[2], prm["g2"]))
    dpre = check_ln_bwd(rep, c, "ffn norm")
    dbr = dpre
    if p > 0:
        c = sb.take("dropout_bf16")
        rep.exact("ffn dropout 2' operands", torch.equal(c.a[0], dpre) and c.a[1] == p and c.a[2] == seed2)
        _check_call(rep, rig, c, "ffn dropout 2'")
        dbr = c.ret
    c = sb.take("wgrad_bf16")
    rep.exact("fc2 wgrad operands", torch.equal(c.a[0], dbr) and torch.equal(c.a[1], f))
    check_wgrad(rep, ops, c, "fc2")
    c = sb.take("linear_bf16")
    rep.exact("fc2 dgrad operands", torch.equal(c.a[0], dbr) and torch.equal(c.a[1], W2b.t()))
    _check_call(rep, rig, c, "fc2")
    df = c.ret
    if p > 0:
        c = sb.take("dropout_bf16")
        rep.exact("ffn dropout 1' operands", torch.equal(c.a[0], df) and c.a[1] == p and c.a[2] == seed1)
        _check_call(rep, rig, c, "ffn dropout 1'")
        df = c.ret
    c = sb.take("act_bf16")
    rep.exact("GELU' operands", torch.equal(c.a[0], u) and torch.equal(c.kw["df"], df))
    _check_call(rep, rig, c, "ffn")
    du = c.ret
    c = sb.take("wgrad_bf16")
    rep.exact("fc1 wgrad operands", torch.equal(c.a[0], du) and torch.equal(c.a[1], xb))
    check_wgrad(rep, ops, c, "fc1")
    c = sb.take("linear_bf16")
    rep.exact("fc1 dgrad operands", torch.equal(c.a[0], du) and torch.equal(c.a[1], W1b.t()) and torch.equal(c.kw["residual"], dpre))
    _check_call(rep, rig, c, "fc1 + residual")


def check_ln(rep, sf, sb, r):
    """LayerNormFn: one forward and one backward row-kernel call"""
    prm = r.prm
    c = sf.take("layernorm_bf16")
    rep.exact("final LayerNorm operands", torch.equal(c.a[1], prm["g3"]) and torch.equal(c.a[2], prm["beta3"]))
    ref, bound = _ln_ref(c.a[0], prm["g3"], prm["beta3"])
    rep.check("final out = LayerNorm(x)", c.ret, ref, bound, BF16_RELL2)
    x = c.a[0]
    c = sb.take("layernorm_bwd")
    rep.exact("final LayerNorm' operands", torch.equal(c.a[0], x) and torch.equal(c.a[2], prm["g3"]))
    check_ln_bwd(rep, c, "final norm")


def check_run(rep, ops, r, inp):
    """every recorded call of one run_mha result; asserts from the recorded arguments that the intended branches were taken"""
    G, mode = r.G, r.mode
    sf, sb = _Seq(r.fwd), _Seq(r.bwd)
    if mode.rows_out is None:
        dy_in = inp.dout.to(r.x.device)
    else:
        dy_in = r.dy_rows
    st = check_mha(rep, ops, sf, sb, r, x_in=r.x, dy_in=dy_in)
    assert sf.done() and sb.done(), "recorded calls without a reference: " + str([c.name for c in sf.c[sf.i:] + sb.c[sb.i:]])
    assert st.saw_tn == [G.tn, G.tn] and st.saw_len_mask == (mode.mask == "len") and st.acc == mode.acc
    assert (mode.rows_out is not None) == hasattr(st, "flat")
    return st


def check_encoder_run(rep, ops, r):
    sf, sb = _Seq(r.fwd), _Seq(r.bwd)
    nb = len([c for c in r.bwd])
    # forward: attention block, feed-forward block, final LayerNorm; backward: the reverse
    n_ffn_b = 6 + (2 if r.p > 0 else 0)
    sb_ln, sb_ffn, sb_mha = _Seq(r.bwd[:1]), _Seq(r.bwd[1: 1 + n_ffn_b]), _Seq(r.bwd[1 + n_ffn_b:])
    st = check_mha(rep, ops, sf, sb_mha, r, x_in=r.x)
    check_ffn(rep, ops, sf, sb_ffn, r, r.p)
    check_ln(rep, sf, sb_ln, r)
    assert sf.done() and sb_ln.done() and sb_ffn.done() and sb_mha.done() and nb == 1 + n_ffn_b + len(sb_mha.c)
    return st


# ---------------------------------------------------------------------------------------------------------------- planted errors
def bf16_ulp(v):
    """spacing of bf16 at |v|"""
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -120))) - 7)


def planted_errors(st):
    """-> [(name, got', ref, bound)]: errors planted on the host into the kernels' own results; each must fail the element-wise
    criterion (no rel-L2).  An entry is None where the case cannot show it (one head, no TN form)."""
    G = st.G
    B, H, Sp = G.B, G.H, G.Sp
    out = []
    got, ref, bound = st.ctx
    # one key missing from one (b, h) row of P V: the row's heaviest key
    b, h, q = B - 1, H - 1, 0
    k = int(st.Pd[b, h, q].argmax())
    bad = got.double().clone()
    bad[b, h, q] -= st.Pd[b, h, q, k] * st.V[b, h, k]
    out.append(("ctx: one key missing from one row of P V", bad, ref, bound))
    # V^T of utterance b taken from utterance b + 1
    bad = got.double().clone()
    bad[0] += st.Pd[0] @ st.V[1] - st.Pd[0] @ st.V[0]
    out.append(("ctx: V^T of utterance 0 taken from utterance 1", bad, ref, bound))
    # head h's dQ columns swapped with head h + 1
    if H > 1:
        got, ref, bound = st.dQ
        bad = got.double().clone()
        bad[:, [0, 1]] = bad[:, [1, 0]]
        out.append(("dQ: head 0's columns swapped with head 1's", bad, ref, bound))
    # one pad key let through the softmax (utterance B - 1 has pad keys in every case)
    got, ref, bound = st.P
    row = (B - 1) * H * Sp
    padk = int(st.key_pad[B - 1].nonzero()[0])
    m = st.key_pad[B - 1].clone()
    m[padk] = False
    bad = got.double().clone()
    bad[row] = kc.softmax_ref(st.scores[row: row + 1].double(), m[None], 1, st.softmax_scale)[0].to(BF).double()
    out.append(("P: one pad key let through the softmax", bad, ref, bound))
    # one 64-row K-tile missing from the TN dV
    got, ref, bound = st.dV
    bad = got.double().clone()
    bad[0, 0] -= st.Pd[0, 0, :64].t() @ st.dctx[0, 0, :64]
    out.append(("dV: one 64-row K-tile missing" + (" from the TN form" if G.tn else ""), bad, ref, bound))
    # a two-ulp error in one dx element: where the bound is tightest relative to the value
    got, ref, bound = st.dx
    i = int((ref.abs() / (bound + FTZ)).argmax())
    bad = got.double().clone().view(-1)
    d = float(bad[i] - ref.view(-1)[i])
    bad[i] += (1.0 if d >= 0 else -1.0) * 2 * bf16_ulp(bad[i])
    out.append(("dx: two ulp in one element", bad.view(got.shape), ref, bound))
    return out


def assert_planted_rejected(st):
    names = []
    for name, bad, ref, bound in planted_errors(st):
        assert not _passes(bad, ref, bound)[0], f"{name}: not rejected"
        names.append(name)
    return names


# ---------------------------------------------------------------------------------------------------------------- whole block in fp64
class _RoundFwd(torch.autograd.Function):
    """bf16 on the way forward only (P: its gradient dP stays fp32 in the product)"""

    @staticmethod
    def forward(ctx, t):
        return t.to(BF).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    """bf16 on the way back only (the scores are fp32, their gradient dS is stored as bf16)"""

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return g.to(BF).to(g.dtype)


def _sites(emulate):
    ident = lambda t: t
    if not emulate:
        return ident, ident, ident, ident
    w_ = lambda t: t + (t.to(BF).double() - t).detach()       # the bf16 working copy, gradient straight through to the master
    return _RoundBF16.apply, _RoundFwd.apply, _RoundBwd.apply, w_


def mha_graph(x, P, H, lens, emulate):
    """LN(MHA(x) + x) in fp64 by its definition on the S real rows and the unpadded heads.  ``emulate``: one bf16 rounding at each of
    the product's storage sites - x_b, qkv, P, ctx, pre, out forward; dx, dqkv, dS, dctx, dpre, dy backward; the weights' bf16 copies"""
    st, rf, rb, w_ = _sites(emulate)
    B, S, Dm = x.shape
    dt = Dm // H
    xb = st(x)
    qkv = st(xb @ w_(P["Wi"]).t() + P["bi"])
    q, k, v = (t.reshape(B, S, H, dt).transpose(1, 2) for t in qkv.split(Dm, dim=-1))
    sc = rb(q @ k.transpose(-1, -2)) * dt ** -0.5
    pad = torch.arange(S, device=x.device)[None, :] >= torch.as_tensor(lens, device=x.device)[:, None]
    Pm = rf(torch.softmax(sc.masked_fill(pad[:, None, None, :], float("-inf")), dim=-1))
    ctx = st((Pm @ v).transpose(1, 2).reshape(B, S, Dm))
    pre = st(ctx @ w_(P["Wo"]).t() + P["bo"] + xb)
    return st(F.layer_norm(pre, (Dm,), P["g"], P["beta"], EPS))


def encoder_graph(x, P, H, lens, emulate):
    """the post-LN layer + final LayerNorm of TransformerEncoder (no dropout): sites u, f, pre, out of the feed-forward block and
    the bf16 input / output of the final LayerNorm"""
    st, rf, rb, w_ = _sites(emulate)
    Dm = x.shape[-1]
    y = st(mha_graph(x, P, H, lens, emulate))
    f = st(F.gelu(st(y @ w_(P["W1"]).t() + P["b1"])))
    pre = st(f @ w_(P["W2"]).t() + P["b2"] + y)
    z = st(st(F.layer_norm(pre, (Dm,), P["g2"], P["beta2"], EPS)))
    return st(F.layer_norm(z, (Dm,), P["g3"], P["beta3"], EPS))


def graph_grads(graph, x, prm, H, lens, dout, emulate):
    P = {k: v.detach().double().clone().requires_grad_() for k, v in prm.items()}
    xd = x.detach().double().clone().requires_grad_()
    with torch.enable_grad():
        out = graph(xd, P, H, lens, emulate)
        (out * dout.double()).sum().backward()
    res = {"out": out.detach(), "x": xd.grad}
    res.update({k: v.grad for k, v in P.items()})
    return res


def nn_autograd(x, prm, H, lens, dout):
    """fp64 autograd of nn.MultiheadAttention + residual + nn.LayerNorm"""
    Dm = x.shape[-1]
    dev = x.device
    att = torch.nn.MultiheadAttention(Dm, H, batch_first=True).to(dev).double()
    norm = torch.nn.LayerNorm(Dm, eps=EPS).to(dev).double()
    ps = {"Wi": att.in_proj_weight, "bi": att.in_proj_bias, "Wo": att.out_proj.weight, "bo": att.out_proj.bias, "g": norm.weight,
          "beta": norm.bias}
    with torch.no_grad():
        for k, p in ps.items():
            p.copy_(prm[k].double())
    xd = x.detach().double().clone().requires_grad_()
    pad = torch.arange(x.shape[1], device=dev)[None, :] >= torch.as_tensor(lens, device=dev)[:, None]
    with torch.enable_grad():
        out = norm(att(xd, xd, xd, key_padding_mask=pad, need_weights=False)[0] + xd)
        (out * dout.double()).sum().backward()
    res = {"out": out.detach(), "x": xd.grad}
    res.update({k: p.grad for k, p in ps.items()})
    return res


def whole_block_rows(hip, ctrl, ref, Dm):
    """(name, rel-L2(HIP, control), rel-L2(control, fp64)) per output; the key bias gradient (exactly zero in exact arithmetic: the
    softmax ignores a per-query shift) is left out of ``bi``"""
    rows = []
    for n in ctrl:
        a, b, c = hip[n].double(), ctrl[n], ref[n]
        if n == "bi":
            keep = torch.ones(3 * Dm, dtype=torch.bool, device=a.device)
            keep[Dm: 2 * Dm] = False
            a, b, c = a[keep], b[keep], c[keep]
        rows.append((n, rel_l2(a, b), rel_l2(b, c)))
    return rows
