"""GPU: the trainable HuBERT backward chains as the product calls them - TrainableFrontend.backward_frontend (pos_conv, encoder /
feature LayerNorms, post_extract_proj, conv layers 6 .. 1) and TrainableLayers._layer_backward (post-LN base, pre-LN large) - stage by
stage against float64.

Nothing of the chain is restated here: a recording proxy replaces the ``ops`` module attribute of hubert_frontend_train /
hubert_train and clones every argument before and after each call, so each stage is checked on the bf16 tensors the kernels actually
received.  The float64 reference of a stage is fairseq's definition of that derivative (conv1d with the layer's stride, the grouped
pos_conv with padding 64 and SamePad, weight_norm(dim = 2), layer_norm, exact erf-GELU, softmax attention with the regenerated
dropout masks) evaluated on the stage's inputs, with weights taken from the fp32 parameters rounded to bf16 (the storage format of
the kernels' working copies).  Conv layer 0 is covered by tests/test_gpu_frontend.py and is not checked here.

Bounds: docs/parity.md ("Trainable HuBERT backward"); the constants below carry their derivations.  The bf16 rounding constant and
the subnormal slack were corrected after the first GPU runs, and the attention outputs have no rel-L2 criterion (their element-wise
bound carries the magnitude of the cancelling terms): docs/parity.md records both.
On top of the stage checks, exact invariants that catch addressing errors: neighbour independence, single-frame support, pad-row
junk, repeatability, and the two q / k / v bias gradient layouts.  Whole chains (front end + one layer) are compared with an fp64
chain that rounds to bf16 where the product stores (``_chain64``)."""
import dataclasses
import inspect
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                 # fp32 unit roundoff
STORE = 2.0 ** -8              # one bf16 rounding: unit roundoff of an 8-bit significand, |bf16(v) - v| <= 2^-8 |v|
STORE2 = 2 * STORE             # the GELU' epilogues round twice: C <- bf16(bf16(acc) * gelu'(aux)) (csrc/gemm_epilogue.inc)
KSEC = 2                       # second-order terms: every first-order accumulation bound is doubled
GELU_ABS = 4e-6                # |gelu_grad_as - gelu'| (docs/parity.md, conv layer 0 backward)
ATT_ROUND = 3                  # attention backward: bf16 roundings of in-kernel operands (P, dP / dS, the stored O read by delta)
F32_RELL2 = 1e-4               # fp32 parameter gradients: random-sign fp32 accumulation gives ~u K / sqrt(N) <= 1.6e-5 for
#                                K <= N <= 65536 rows; one of N rows moves the sum by ~N^-1/2 >= 3.9e-3, 39x above the criterion
BF16_RELL2 = 1e-2              # bf16 stage outputs (GEMM-shaped): one rounding = rel-L2 2^-8 / sqrt(3) = 2.3e-3, two 4.6e-3
FTZ = 2.0 ** -106              # absolute slack for flushed subnormals: the MFMA / fp32 paths flush operands and products below
#                                2^-126; <= 2^17 terms of |operand| <= 2^3 lose < 2^-106 (the fp64 reference keeps them)
EPS = 1e-5
SEEDS = (0x1234567, 0x2345678, 0x3456789, 0x456789a, 0x56789ab)      # dropout_input, encoder, attention, out_proj, fc2


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _bf(t):
    return t.detach().to(torch.bfloat16).double()


def _gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ---------------------------------------------------------------------------------------------------------------- recording proxy
def _cl(x):
    if isinstance(x, torch.Tensor):
        return x.detach().clone()
    if isinstance(x, (list, tuple)):
        return type(x)(_cl(v) for v in x)
    if isinstance(x, dict):
        return {k: _cl(v) for k, v in x.items()}
    return x


class _Call:
    def __init__(self, name, pre, post, ret):
        self.name = name
        (self.a, self.kw), (self.pa, self.pkw), self.ret = pre, post, ret


class _Rec:
    """Stands in for ``ops`` inside one module: every function call is forwarded; while ``on``, its arguments are cloned before and
    after the call (buffers are reused: the second posconv_prep overwrites the du slab, ``out=`` views are recycled)."""

    def __init__(self, mod):
        self._m, self.calls, self.on = mod, [], False

    def __getattr__(self, name):
        f = getattr(self._m, name)
        if not inspect.isfunction(f):
            return f

        def wrap(*a, **kw):
            if not self.on:
                return f(*a, **kw)
            pre = _cl((a, kw))
            r = f(*a, **kw)
            self.calls.append(_Call(name, pre, _cl((a, kw)), _cl(r)))
            return r
        return wrap


class _Seq:
    def __init__(self, calls):
        self.c, self.i = list(calls), 0

    def take(self, name):
        assert self.i < len(self.c), f"chain ended before {name}"
        c = self.c[self.i]
        assert c.name == name, f"call {self.i}: {c.name}, expected {name}"
        self.i += 1
        return c

    def done(self):
        return self.i == len(self.c)


# ---------------------------------------------------------------------------------------------------------------- the rig
class _Rig:
    """One HuBERT layer + the trainable front end on a uniform-layout _Plan, driven exactly like the encoder drives them."""

    def __init__(self, large, lens, seed, recs, dropout=True):
        from speechclip_plus_amd import hubert_frontend_train as hft, hubert_train as ht, ops, random_hubert_state_dict
        from speechclip_plus_amd import speech_encoder as se
        self.dev = torch.device("cuda:0")
        self.large, self.ops = large, ops
        self.arch = a = dataclasses.replace(se.ARCHS["hubert_large_ll60k" if large else "hubert"], layers=1, feature_grad_mult=0.1)
        sd = random_hubert_state_dict(a, seed=seed)
        self.front = hft.TrainableFrontend(a, sd, self.dev)
        self.tl = ht.TrainableLayers(a, sd, [0], self.dev)
        self.tl.frontend = self.front
        self.lens = list(lens)
        self.B, self.L = len(lens), max(lens)
        self.pl = pl = se._Plan(a, self.B, self.L, self.dev)
        T = pl.T
        chunk = self.L // T
        self.valid = [min(T, -(-int(l) // chunk)) for l in lens]            # fairseq forward_padding_mask
        pl.valid.copy_(torch.tensor(self.valid, dtype=torch.int32))
        pl.len_dev.copy_(torch.tensor(self.lens, dtype=torch.int64))
        drop = dropout and not large                       # the large arch's dropouts are 0
        self.p_in, self.p_res, self.p_att = (a.dropout_input, a.dropout, a.attention_dropout) if drop else (0.0, 0.0, 0.0)
        assert not drop or (self.p_in, self.p_res, self.p_att) == (0.1, 0.1, 0.1)
        self.rec_f, self.rec_l = recs

    def params(self):
        out = {self.front.fairseq_names[k]: p for k, p in self.front.p.items()}
        out.update({self.tl.fairseq_names[k]: p for k, p in self.tl.p.items()})
        return out

    def wav(self, seed, scale=None):
        g = torch.Generator().manual_seed(seed)
        w = torch.zeros(self.B, self.L)
        for b, l in enumerate(self.lens):
            w[b, :l] = torch.randn(l, generator=g) * (0.5 if scale is None else scale[b])
        return w

    @torch.no_grad()
    def forward(self, wav):
        pl, a = self.pl, self.arch
        self.ops.wav_prep(wav.to(self.dev), pl.len_dev, pl.wav_pad, a.normalize_wav, L=self.L)
        self.front.refresh()
        self.tl.refresh()
        self.front.forward_frontend(pl, self.L, self.p_in, self.p_res, SEEDS[0], SEEDS[1])
        drops = (self.p_res, self.p_att, SEEDS[2], SEEDS[3], SEEDS[4]) if self.p_res > 0 else None
        self.tl.layer_forward(0, pl.hidden[0], pl.hidden[1], pl, True, drops=drops)
        self.st = pl.front                                  # the front end's kept activations (backward_frontend drops the dict)

    def backward(self, dh1=None, dh0=None, train=True, record=False, flat_grads=False):
        """dh1: gradient of hidden[1] -> layer backward -> front end; dh0 alone: front end only.  Returns every gradient."""
        for p in self.params().values():
            p.grad = None
        if flat_grads:        # the optimiser's layout: every layer gradient a view of ONE flat fp32 buffer, q / k / v biases at one stride
            ps = self.tl.layer_parameters(0)
            flat = torch.zeros(sum(p.numel() for p in ps), device=self.dev)
            o = 0
            for p in ps:
                p.grad = flat[o: o + p.numel()].view(p.shape)
                o += p.numel()
        for r in (self.rec_f, self.rec_l):
            r.calls, r.on = [], record
        out = {}
        with torch.no_grad():
            if dh1 is not None:
                dh0 = self.tl._layer_backward(0, self.pl, dh1, need_dx=True, train=train)
                out["dx_layer"] = dh0.clone()
            self.front.backward_frontend(self.pl, dh0)
        torch.cuda.synchronize()
        for r in (self.rec_f, self.rec_l):
            r.on = False
        for n, p in self.params().items():
            out[n] = None if p.grad is None else p.grad.clone()
        return out

    def row_grad(self, seed, rows_of=None, scale=1.0):
        """bf16 [M, D] gradient: noise on frames t < valid_b of the utterances in ``rows_of`` (default all), zero elsewhere"""
        pl = self.pl
        g = torch.Generator().manual_seed(seed)
        d = torch.zeros(self.B, pl.R, self.arch.embed_dim)
        for b in (range(self.B) if rows_of is None else rows_of):
            d[b, : self.valid[b]] = torch.randn(self.valid[b], self.arch.embed_dim, generator=g) * scale
        return d.view(-1, self.arch.embed_dim).to(torch.bfloat16).to(self.dev)


# ---------------------------------------------------------------------------------------------------------------- criteria
class _Report:
    def __init__(self, tag):
        self.tag, self.rows = tag, {}

    def check(self, stage, got, ref, bound, rell2=None):
        ok, ratio, e = _passes(got, ref, bound, rell2)
        old = self.rows.get(stage, (0.0, 0.0))
        self.rows[stage] = (max(old[0], ratio), max(old[1], e))
        assert ok, f"{self.tag} / {stage}: largest error / bound {ratio:.3g}, rel-L2 {e:.3g} (criterion {rell2})"

    def show(self):
        for k, (r, e) in self.rows.items():
            print(f"[trainable-bwd] {self.tag:>14s} {k:38s} max err/bound {r:8.3g}   rel-L2 {e:9.3g}")


def _passes(got, ref, bound, rell2=None):
    got = got.double()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if not bool(torch.isfinite(got).all()):
        return False, float("inf"), float("inf")
    diff = (got - ref).abs()
    zero = bound == 0                            # structural zeros stay exact
    bound = bound + FTZ
    ratio = float((diff / torch.where(zero, torch.ones_like(bound), bound)).max()) if diff.numel() else 0.0
    if bool((diff[zero] != 0).any()):            # structural zeros: exactly zero
        ratio = float("inf")
    e = rel_l2(got, ref) if float(ref.norm()) > 0 else float(got.double().norm())
    return ratio <= 1.0 and (rell2 is None or e <= rell2), ratio, e


def _att_bound(ref, mag, R):
    return STORE * ref.abs() + ATT_ROUND * STORE * mag + KSEC * R * U * mag


def _keff_wgrad(ops, rows, N, K):
    """serial fp32 accumulation length of ops.wgrad_bf16 (TN form): rows per slice (whole 64-row K-tiles), then the slices in order"""
    tiles = -(-N // 256) * -(-K // 256)
    kt = rows // 64
    S = max(1, min(ops._num_cus() // tiles, kt // 4))
    Kc = -(-kt // S) * 64
    return Kc + -(-rows // Kc)


def _keff_colsum(rows):
    nblk = max(1, min(512, rows // 64))                     # ops.colsum_bf16: 64-row-block partials, then the blocks in order
    return -(-rows // nblk) + nblk


def _keff_ln(rows):
    n_part = min(1024, (rows + 3) // 4)                     # ops.layernorm_bwd: one partial per workgroup (4 waves in LDS), then colsum
    return -(-rows // n_part) + 4 + n_part


# ---------------------------------------------------------------------------------------------------------------- fp64 references
def _ln_ref(x, dy, g, dres=None):
    x, dy, g = x.double(), dy.double(), g.double()
    D = x.shape[1]
    mu = x.mean(1, keepdim=True)
    xc = x - mu
    rstd = ((xc * xc).mean(1, keepdim=True) + EPS).rsqrt()
    xh = xc * rstd
    gd = g * dy
    dx = rstd * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True))
    # two-pass fp32 statistics over D channels (wave trees) and the two fp32 channel means: D u relative per term
    mag = rstd * (gd.abs() + gd.abs().mean(1, keepdim=True) + (xh.abs() + 1.0) * (gd * xh).abs().mean(1, keepdim=True))
    bound_dx = KSEC * D * U * mag
    if dres is not None:
        dx = dx + dres.double()
    bound_dx = bound_dx + STORE * dx.abs()
    rows = x.shape[0]
    dg, db = (dy * xh).sum(0), dy.sum(0)
    bdg = KSEC * U * (_keff_ln(rows) * (dy * xh).abs().sum(0) + D * (dy.abs() * (xh.abs() + 1.0)).sum(0))
    bdb = KSEC * U * _keff_ln(rows) * dy.abs().sum(0)
    return dx, bound_dx, dg, bdg, db, bdb, xh


def _row_keep(rows, D, p, seed, dev):
    from test_gpu_kernels import _keep_mask
    keep = _keep_mask(np.arange(rows * D, dtype=np.int64), seed, p)
    return torch.from_numpy(keep).view(rows, D).to(dev)


def _check_dropout(rep, stage, got, x, p, seed):
    keep = _row_keep(x.shape[0], x.shape[1], p, seed, x.device)
    ref = torch.where(keep, x.float() / (1 - p), torch.zeros((), device=x.device)).to(torch.bfloat16)
    assert torch.equal(got, ref), f"{rep.tag} / {stage}: dropout mask"
    rep.rows.setdefault(stage + " (bitwise)", (0.0, 0.0))


def _attn_ref(rig, q, k, v, dout, p_att, seed):
    """fp64 attention over each utterance's R-row pitch: keys t >= valid masked, the forward's probability dropout (applied rate
    round(256 p) / 256) rebuilt on the host; returns dq, dk, dv, magnitudes, and P' / dO for the sensitivity check"""
    from test_gpu_kernels import _keep_mask8
    pl, H = rig.pl, rig.arch.heads
    B, R = pl.B, pl.R
    D = q.shape[1]
    sc = (D // H) ** -0.5
    sh = lambda t: t.double().view(B, R, H, D // H).transpose(1, 2)
    Q, K, V, dO = sh(q), sh(k), sh(v), sh(dout)
    key_ok = torch.arange(R, device=q.device)[None, :] < torch.tensor(rig.valid, device=q.device)[:, None]
    s = (Q @ K.transpose(-1, -2)) * sc
    P = torch.softmax(s.masked_fill(~key_ok[:, None, None, :], float("-inf")), dim=-1)
    if p_att > 0:
        keep, pa = _keep_mask8(np.arange(B * H * R * R, dtype=np.int64), seed, p_att)
        mult = torch.from_numpy(keep).view(B, H, R, R).to(q.device).double() / (1.0 - pa)
    else:
        mult = torch.ones_like(P)
    Pd = P * mult
    O = Pd @ V
    dV = Pd.transpose(-1, -2) @ dO
    dPd = dO @ V.transpose(-1, -2)
    dP = dPd * mult
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dQ, dK = (dS @ K) * sc, (dS.transpose(-1, -2) @ Q) * sc
    dPm = (dO.abs() @ V.abs().transpose(-1, -2)) * mult
    dSm = P * (dPm + (dO.abs() * O.abs()).sum(-1, keepdim=True) + delta.abs())
    mq, mk, mv = (dSm @ K.abs()) * sc, (dSm.transpose(-1, -2) @ Q.abs()) * sc, Pd.transpose(-1, -2) @ dO.abs()
    un = lambda t: t.transpose(1, 2).reshape(B * R, D)
    return [un(t) for t in (dQ, dK, dV, mq, mk, mv)] + [Pd, dO, dS * sc, Q, K]


# ---------------------------------------------------------------------------------------------------------------- generic stage checks
def _check_call(rep, rig, c, where):
    """one recorded call against the fp64 definition of the operation on its own recorded inputs"""
    ops = rig.ops
    n = c.name
    if n == "layernorm_bwd":
        x, dy, g = c.a[0], c.a[1], c.a[2]
        kw = c.kw
        dx_r, bdx, dg_r, bdg, db_r, bdb, _ = _ln_ref(x, dy, g, kw.get("dres"))
        ret = c.ret
        if isinstance(ret, tuple) and len(ret) == 3:           # want_param_grads: (dx, dgamma, dbeta)
            dx, dg, db = ret
            dxd = None
        elif isinstance(ret, tuple):
            dx, dxd = ret
            dg = db = None
        else:
            dx, dxd, dg, db = ret, None, None, None
        rep.check(f"{where} LayerNorm' dx", dx, dx_r, bdx)
        if "acc" in kw:
            dg = c.pkw["acc"][0] - c.kw["acc"][0]
            db = c.pkw["acc"][1] - c.kw["acc"][1]
        if dg is not None:
            rep.check(f"{where} LayerNorm' dgamma", dg, dg_r, bdg, F32_RELL2)
            rep.check(f"{where} LayerNorm' dbeta", db, db_r, bdb, F32_RELL2)
        drop = kw.get("drop")
        if drop is not None and drop[0] > 0:
            keep = _row_keep(dx.shape[0], dx.shape[1], drop[0], drop[1], dx.device)
            ref = torch.where(keep, dx.double() / (1 - drop[0]), torch.zeros((), device=dx.device, dtype=torch.float64))
            rep.check(f"{where} LayerNorm' dropped copy", dxd, ref, STORE * ref.abs())
        if kw.get("sum_acc") is not None:
            src = dxd if dxd is not None else dx
            got = c.pkw["sum_acc"] - c.kw["sum_acc"]
            rep.check(f"{where} branch bias colsum", got, src.double().sum(0),
                      KSEC * U * _keff_ln(src.shape[0]) * src.double().abs().sum(0), F32_RELL2)
    elif n == "wgrad_bf16":
        dy, x = c.a[0].double(), c.a[1].double()
        gW = c.a[2]
        beta = c.kw.get("beta", c.a[4] if len(c.a) > 4 else 1.0)
        gb_pre = c.kw.get("gb", c.a[3] if len(c.a) > 3 else None)
        gb_post = c.pkw.get("gb", c.pa[3] if len(c.pa) > 3 else None)
        if isinstance(gW, (list, tuple)):
            got = torch.cat([post.double() - beta * pre.double() for pre, post in zip(gW, c.pa[2])])
        else:
            got = c.pa[2].double() - beta * gW.double()
        rows, N = dy.shape
        keff = _keff_wgrad(ops, rows, N, x.shape[1])
        rep.check(f"{where} weight gradient", got, dy.t() @ x, KSEC * U * keff * (dy.abs().t() @ x.abs()), F32_RELL2)
        if gb_post is not None:
            rep.check(f"{where} bias gradient", gb_post.double() - beta * gb_pre.double(), dy.sum(0),
                      KSEC * U * _keff_colsum(rows) * dy.abs().sum(0), F32_RELL2)
    elif n == "colsum_bf16":
        x = c.a[0].double()
        rep.check(f"{where} colsum", c.pa[1], x.sum(0), KSEC * U * _keff_colsum(x.shape[0]) * x.abs().sum(0), F32_RELL2)
    elif n == "linear_bf16":
        x, w = c.a[0].double(), c.a[1].double()
        dot, mag = x @ w.t(), x.abs() @ w.abs().t()
        K = x.shape[1]
        res = c.kw.get("residual")
        if c.kw.get("aux_mode", 0) == 2:
            gp = _gelu_grad(c.kw["aux"].double())
            ref = dot * gp
            bound = KSEC * K * U * mag * gp.abs() + GELU_ABS * dot.abs() + (STORE2 - STORE) * ref.abs()   # + STORE below
        else:
            ref, bound = dot, KSEC * K * U * mag
        if res is not None:
            ref = ref + res.double()
        rep.check(f"{where} dgrad", c.ret, ref, bound + STORE * ref.abs(), BF16_RELL2)
    elif n == "act_bf16":
        u, df = c.a[0].double(), c.kw["df"].double()
        ref = df * _gelu_grad(u)
        rep.check(f"{where} GELU'", c.ret, ref, STORE * ref.abs() + GELU_ABS * df.abs())
    elif n == "dropout_bf16":
        _check_dropout(rep, f"{where} dropout", c.ret, c.a[0], c.a[1], c.a[2])
    elif n == "attn_bwd":
        q, k, v, ctx, dout = c.a[0], c.a[1], c.a[2], c.a[3], c.a[4]
        D = q.shape[1]
        assert c.kw["q_rows"] == rig.pl.T
        dq_r, dk_r, dv_r, mq, mk, mv = _attn_ref(rig, q, k, v, dout, c.kw.get("drop_p", 0.0), c.kw.get("drop_seed", 0))[:6]
        R = rig.pl.R
        for name, got, ref, mag in (("dq", c.pa[7], dq_r, mq), ("dk", c.pa[8], dk_r, mk), ("dv", c.pa[9], dv_r, mv)):
            # element-wise only: these are sums whose terms cancel (dS sums to zero over the keys), so a rel-L2 limit would have to
            # scale with ||mag|| / ||ref|| and then no longer resolves one row; the element-wise bound does (sensitivity checks)
            rep.check(f"{where} attention {name}", got, ref, _att_bound(ref, mag, R))
    else:
        return False
    return True


# ---------------------------------------------------------------------------------------------------------------- layer
def _check_layer(rep, rig, dh1, train=True):
    calls = rig.rec_l.calls
    tl, pl, a = rig.tl, rig.pl, rig.arch
    names = [c.name for c in calls]
    if rig.arch.layer_norm_first:
        want = ["wgrad_bf16", "linear_bf16", "wgrad_bf16", "linear_bf16", "layernorm_bwd", "wgrad_bf16", "linear_bf16", "attn_bwd",
                "wgrad_bf16", "colsum_bf16", "linear_bf16", "layernorm_bwd"]
    else:
        want = ["layernorm_bwd", "wgrad_bf16", "linear_bf16", "wgrad_bf16", "linear_bf16", "layernorm_bwd", "wgrad_bf16", "linear_bf16",
                "attn_bwd", "wgrad_bf16", "colsum_bf16", "linear_bf16"]
    if not train:
        want = [n for n in want if n not in ("wgrad_bf16", "colsum_bf16")]
    assert names == want, names
    # the weight operands of the dgrad products are the parameters' bf16 transposes
    cp = tl._copies[0]
    W = lambda n: tl.get(0, n).detach().to(torch.bfloat16)
    assert torch.equal(cp["fc2_wT"], W("fc2.weight").t().contiguous()) and torch.equal(cp["fc1_wT"], W("fc1.weight").t().contiguous())
    assert torch.equal(cp["o_wT"], W("self_attn.out_proj.weight").t().contiguous())
    assert torch.equal(cp["qkv_wT"], torch.cat([W(f"self_attn.{n}.weight") for n in ("q_proj", "k_proj", "v_proj")]).t().contiguous())
    # the chain hands each stage what the stage before produced
    first = calls[0]
    assert torch.equal(first.a[1] if first.name == "layernorm_bwd" else first.a[0], dh1)
    for i, c in enumerate(calls):
        assert _check_call(rep, rig, c, f"layer {i:2d} {c.name}")
    if train:
        qkv_b = calls[names.index("colsum_bf16")].pa[1]
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
            assert torch.equal(tl.get(0, f"self_attn.{n}.bias").grad, qkv_b[j * a.embed_dim: (j + 1) * a.embed_dim]), n


# ---------------------------------------------------------------------------------------------------------------- front end
def _check_front(rep, rig, dh0, sens=False):
    calls = rig.rec_f.calls
    pl, a, st, fr = rig.pl, rig.arch, rig.st, rig.front
    B, R, M, T = pl.B, pl.R, pl.M, pl.T
    C, D, G, Kp = a.conv_dim, a.embed_dim, a.pos_conv_groups, a.pos_conv_kernel
    Dg, halo = D // G, pl.halo
    dev = dh0.device
    sq = _Seq(calls)
    if rig.p_res > 0:
        c = sq.take("dropout_bf16")
        assert torch.equal(c.a[0], dh0)
        _check_call(rep, rig, c, "encoder dropout'")
        dh0 = c.ret
    if not a.layer_norm_first:
        c = sq.take("layernorm_bwd")
        assert torch.equal(c.a[1], dh0) and torch.equal(c.a[0], st["pre"])
        _check_call(rep, rig, c, "encoder")
        dpre = c.ret
    else:
        dpre = dh0
    # ---- pos_conv
    c = sq.take("act_bf16")
    assert torch.equal(c.kw["df"], dpre) and torch.equal(c.a[0], st["u_pos"])
    _check_call(rep, rig, c, "pos_conv")
    du = c.ret
    sq.take("posconv_prep")
    c_w = sq.take("posconv_wgrad")
    c_b = sq.take("colsum_bf16")
    assert torch.equal(c_b.a[0], du)
    _check_call(rep, rig, c_b, "pos_conv bias")
    c_x = sq.take("gemm_raw")
    dxz = c_x.pa[4]
    # fp64 grouped conv on every utterance's T frames (x = the masked input xz, padding 64, SamePad drops frame T)
    wq = fr.pos_weight().detach()
    Wb = _bf(wq).view(G, Dg, Dg, Kp)                                 # [g][co][ci][tap]
    dW = torch.zeros(G, Dg, Dg, Kp, device=dev, dtype=torch.float64)
    dWm = torch.zeros_like(dW)
    xz = pl.xz.double().view(B, R, D)
    duv = du.double().view(B, R, D)
    assert bool((duv[:, T:] == 0).all())
    for b in range(B):
        xp = torch.nn.functional.pad(xz[b, :T], (0, 0, halo, halo))                  # [T + 128, D]
        win = xp.unfold(0, Kp, 1)[:T].reshape(T, G, Dg, Kp)                            # [t][g][ci][tap]
        d = duv[b, :T].reshape(T, G, Dg)
        dW += torch.einsum("tgo,tgic->goic", d, win)
        dWm += torch.einsum("tgo,tgic->goic", d.abs(), win.abs())
        dwin = torch.einsum("tgo,goic->tgic", d, Wb)
        dwinm = torch.einsum("tgo,goic->tgic", d.abs(), Wb.abs())
        dxp, dxpm = torch.zeros_like(xp).view(-1, G, Dg), torch.zeros_like(xp).view(-1, G, Dg)
        for tap in range(Kp):
            dxp[tap: tap + T] += dwin[..., tap]
            dxpm[tap: tap + T] += dwinm[..., tap]
        ref = dxp[halo: halo + T].reshape(T, D) + dpre.double().view(B, R, D)[b, :T]
        bound = STORE * ref.abs() + KSEC * Kp * Dg * U * dxpm[halo: halo + T].reshape(T, D)
        rep.check("pos_conv dgrad + residual", dxz.view(B, R, D)[b, :T], ref, bound, BF16_RELL2)
    Z = 4
    while (B * (R + 2 * halo) // 128) % Z:
        Z -= 1
    bW = KSEC * U * (B * (R + 2 * halo) // Z + Z) * dWm
    gw = c_w.ret.view(G, Dg, Kp, Dg).permute(0, 1, 3, 2)                                 # -> [g][co][ci][tap]
    rep.check("pos_conv weight gradient (G = 16)", gw, dW, bW, F32_RELL2)
    if sens:          # the contribution of utterance 1's first frame
        xp1 = torch.nn.functional.pad(xz[1, :T], (0, 0, halo, halo))
        one = torch.einsum("go,gic->goic", duv[1, 0].view(G, Dg), xp1[:Kp].t().reshape(G, Dg, Kp))
        assert not _passes(gw.double() - one, dW, bW, F32_RELL2)[0], "pos_conv weight gradient: one-frame error not rejected"
    # weight_g / weight_v through weight_norm(dim = 2) in fp64
    g64 = fr.P("encoder.pos_conv.0.weight_g").detach().double().requires_grad_(True)
    v64 = fr.P("encoder.pos_conv.0.weight_v").detach().double().requires_grad_(True)
    with torch.enable_grad():
        nv = v64.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
        w64 = g64 * v64 / nv
        gg_r, gv_r = torch.autograd.grad(w64, [g64, v64], dW.reshape(D, Dg, Kp))
    vh = (v64 / nv).detach()
    bWf = bW.reshape(D, Dg, Kp)
    fp32 = 64 * U * (g64.detach().abs() / nv.detach()) * (dW.abs().reshape(D, Dg, Kp) + vh.abs() * (vh * dW.reshape(D, Dg, Kp)).abs().sum((0, 1), keepdim=True))
    bgg = (vh.abs() * bWf).sum((0, 1), keepdim=True) + 64 * U * (vh * dW.reshape(D, Dg, Kp)).abs().sum((0, 1), keepdim=True)
    bgv = g64.detach().abs() / nv.detach() * (bWf + vh.abs() * (vh.abs() * bWf).sum((0, 1), keepdim=True)) + fp32
    rep.check("pos_conv weight_g gradient", fr.P("encoder.pos_conv.0.weight_g").grad, gg_r, bgg, F32_RELL2)
    rep.check("pos_conv weight_v gradient", fr.P("encoder.pos_conv.0.weight_v").grad, gv_r, bgv, F32_RELL2)
    # padded-frame mask, dropout_input
    c = sq.take("posconv_prep")
    assert torch.equal(c.a[0], dxz)
    fvalid = (torch.arange(R, device=dev)[None, :] < torch.tensor(rig.valid, device=dev)[:, None]).reshape(M, 1)
    assert torch.equal(c.pa[2], torch.where(fvalid, dxz, torch.zeros_like(dxz))), "padded-frame mask"
    dxp_ = c.pa[2]
    if rig.p_in > 0:
        c = sq.take("dropout_bf16")
        assert torch.equal(c.a[0], dxp_)
        _check_call(rep, rig, c, "dropout_input'")
        dxp_ = c.ret
    # ---- post_extract_proj, feature LayerNorm, feature_grad_mult
    c = sq.take("wgrad_bf16")
    assert torch.equal(c.a[0], dxp_) and torch.equal(c.a[1], pl.feat_ln)
    _check_call(rep, rig, c, "post_extract_proj")
    c = sq.take("linear_bf16")
    assert torch.equal(c.a[1], fr.P("post_extract_proj.weight").detach().to(torch.bfloat16).t().contiguous())
    _check_call(rep, rig, c, "post_extract_proj")
    c = sq.take("layernorm_bwd")
    assert torch.equal(c.a[0], pl.conv[-1][:M])
    _check_call(rep, rig, c, "feature")
    df = (c.ret.float() * 0.1).to(torch.bfloat16)            # GradMultiply: checked against what the first conv stage reads
    if sens:
        x, dy = c.a[0], c.a[1]
        dx_r, bdx, dg_r, bdg, db_r, bdb, xh = _ln_ref(x, dy, c.a[2])
        got = (c.pkw["acc"][0] - c.kw["acc"][0]).double() - dy[R].double() * xh[R]       # utterance 1, frame 0
        assert not _passes(got, dg_r, bdg, F32_RELL2)[0], "LayerNorm dgamma: one-row error not rejected"
    # ---- conv layers 6 .. 1
    nl = len(a.conv_kernels)
    ln_mode = a.extractor_mode == "layer_norm"
    du_next = None
    for i in range(nl - 1, 0, -1):
        k, s = a.conv_kernels[i], a.conv_strides[i]
        Ri, Rp, Ti, Tp = pl.R_l[i], pl.R_l[i - 1], pl.T_l[i], pl.T_l[i - 1]
        if ln_mode:
            c = sq.take("act_bf16")
            assert torch.equal(c.kw["df"], df if i == nl - 1 else dx_prev) and torch.equal(c.a[0], st["n"][i])
            _check_call(rep, rig, c, f"conv {i}")
            c = sq.take("layernorm_bwd")
            assert torch.equal(c.a[0], st["u"][i])
            _check_call(rep, rig, c, f"conv {i}")
            du_i = c.ret[0]
        elif i == nl - 1:
            c = sq.take("act_bf16")
            assert torch.equal(c.kw["df"], df) and torch.equal(c.a[0], st["u"][i])
            _check_call(rep, rig, c, f"conv {i}")
            du_i = c.ret
        else:
            du_i = dx_prev
        c = sq.take("wgrad_bf16")
        assert torch.equal(c.a[0], du_i)
        gw_got = c.pa[2].double()
        gb_got = c.pa[3] if a.conv_bias else None
        while sq.i < len(sq.c) and sq.c[sq.i].name == "gemm_raw":
            sq.i += 1
        # the next consumer's input is this layer's input gradient
        nxt = sq.c[sq.i]
        dx_prev = nxt.a[0] if nxt.name == "wgrad_bf16" else nxt.kw["df"] if nxt.name == "act_bf16" else nxt.a[5]
        X = pl.conv[i - 1][: B * Rp].view(B, Rp, C)
        Du = du_i.double().view(B, Ri, C)
        assert bool((Du[:, Ti:] == 0).all()), f"conv {i}: du rows past T_{i}"
        Wt = _bf(fr.P(f"feature_extractor.conv_layers.{i}.0.weight"))                   # [co][ci][tap]
        dWr = torch.zeros(C, k, C, device=dev, dtype=torch.float64)
        dWm = torch.zeros_like(dWr)
        dxr = torch.zeros(B, Rp, C, device=dev, dtype=torch.float64)
        dxm = torch.zeros_like(dxr)
        for b in range(B):
            cols = X[b, :Tp].double().unfold(0, k, s).permute(0, 2, 1)                  # [t][tap][ci]
            d = Du[b, :Ti]
            dWr += torch.einsum("to,tjc->ojc", d, cols)
            dWm += torch.einsum("to,tjc->ojc", d.abs(), cols.abs())
            idx = s * torch.arange(Ti, device=dev)
            for j in range(k):
                dxr[b].index_add_(0, idx + j, d @ Wt[:, :, j])
                dxm[b].index_add_(0, idx + j, d.abs() @ Wt[:, :, j].abs())
        rows = B * Ri
        bW = KSEC * U * _keff_wgrad(rig.ops, rows, C, k * C) * dWm.view(C, k * C)
        rep.check(f"conv {i} weight gradient", gw_got, dWr.view(C, k * C), bW, F32_RELL2)
        if sens and i == 4:        # the first window of utterance 1
            cols1 = X[1, :k].double().reshape(-1)
            assert not _passes(gw_got - torch.outer(Du[1, 0], cols1), dWr.view(C, k * C), bW, F32_RELL2)[0], \
                f"conv {i} weight gradient: one-window error not rejected"
        if gb_got is not None:
            rep.check(f"conv {i} bias gradient", gb_got, Du.sum((0, 1)), KSEC * U * _keff_colsum(rows) * Du.abs().sum((0, 1)), F32_RELL2)
        if not ln_mode and i >= 2:                       # GELU' of the layer below in the epilogue
            gp = _gelu_grad(st["u"][i - 1][: B * Rp].double().view(B, Rp, C))
            ref = dxr * gp
            bound = STORE2 * ref.abs() + KSEC * k * C * U * dxm * gp.abs() + GELU_ABS * dxr.abs()
        else:
            ref, bound = dxr, STORE * dxr.abs() + KSEC * k * C * U * dxm
        got = dx_prev[: B * Rp].view(B, Rp, C)
        rep.check(f"conv {i} dgrad (k = {k}, s = {s})", got, ref, bound)
        if sens and i == 4:        # row 0 of utterance 1 = tap 0 of its first window only
            bad = got.double().clone()
            bad[1, 0] -= Du[1, 0] @ Wt[:, :, 0] * (gp[1, 0] if not ln_mode else 1.0)
            assert not _passes(bad, ref, bound)[0], f"conv {i} dgrad: one-window error not rejected"
    c = sq.take("conv0_layernorm_gelu_bwd" if ln_mode else "conv0_groupnorm_gelu_bwd")     # conv layer 0: tests/test_gpu_frontend.py
    assert sq.done()


# ---------------------------------------------------------------------------------------------------------------- whole chains
class _RoundBF16(torch.autograd.Function):
    """a bf16 storage site: the value is rounded on the way forward and its gradient on the way back (the product stores both)"""

    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _conv64(x, w, b, s):
    """channels-last conv1d (fairseq's Conv1d, no padding) as unfold + matmul: x [B, T, Ci], w [Co, Ci, k] -> [B, To, Co]"""
    y = torch.einsum("btck,ock->bto", x.unfold(1, w.shape[2], s), w)
    return y if b is None else y + b


def _chain64(rig, wav, G, emulate):
    """fairseq's front end + one encoder layer in fp64 on the GPU (no dropout), differentiated with the output gradient G [B, T, D].
    ``emulate``: bf16 at the product's storage sites (every conv output and kept pre-activation, LayerNorm outputs, post_extract_proj,
    pos_conv pre-activation / GELU / residual sum, q / k / v, the un-normalised attention probabilities in front of P.V, context,
    both residual sums, the FFN pre-activation and activation), in both directions, and the GEMM weights as their bf16 copies (the
    parameter gradients themselves stay fp64).  Returns {fairseq name: gradient}."""
    import torch.nn.functional as F
    a, dev = rig.arch, rig.dev
    st = _RoundBF16.apply if emulate else (lambda t: t)
    P = {n: p.detach().double().clone().requires_grad_(True) for n, p in rig.params().items()}

    def w_(n, t=None):                       # GEMM operand: the bf16 working copy, gradient straight through to the fp64 master
        t = P[n] if t is None else t
        return t + (t.to(torch.bfloat16).double() - t).detach() if emulate else t

    B, L, T, D, C, H = rig.B, rig.L, rig.pl.T, a.embed_dim, a.conv_dim, a.heads
    x = torch.zeros(B, L, dtype=torch.float64, device=dev)
    for b, l in enumerate(rig.lens):
        wb = wav[b, :l].double().to(dev)
        x[b, :l] = F.layer_norm(wb, wb.shape) if a.normalize_wav else wb
    ln_mode = a.extractor_mode == "layer_norm"
    h = x[:, :, None]
    for i, (k, s_) in enumerate(zip(a.conv_kernels, a.conv_strides)):
        pre = f"feature_extractor.conv_layers.{i}."
        wi = P[pre + "0.weight"] if i == 0 else w_(pre + "0.weight")
        u = _conv64(h, wi, P.get(pre + "0.bias"), s_)
        if i > 0:
            u = st(u)
        if ln_mode:
            u = F.layer_norm(u, (C,), P[pre + "2.1.weight"], P[pre + "2.1.bias"], 1e-5)
            if i > 0:
                u = st(u)
        elif i == 0:
            u = F.group_norm(u.transpose(1, 2), C, P[pre + "2.weight"], P[pre + "2.bias"], 1e-5).transpose(1, 2)
        h = st(F.gelu(u))
    fgm = a.feature_grad_mult
    h = h * fgm + h.detach() * (1.0 - fgm)                       # GradMultiply
    h = st(F.layer_norm(h, (C,), P["layer_norm.weight"], P["layer_norm.bias"], 1e-5))
    xp = st(h @ w_("post_extract_proj.weight").t() + P["post_extract_proj.bias"])
    valid = torch.arange(T, device=dev)[None, :] < torch.tensor(rig.valid, device=dev)[:, None]
    xz = xp * valid[:, :, None]
    Gp, Kp = a.pos_conv_groups, a.pos_conv_kernel
    g, v = P["encoder.pos_conv.0.weight_g"], P["encoder.pos_conv.0.weight_v"]
    wpos = w_(None, g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())                  # [D, Dg, Kp]
    Dg = D // Gp
    win = F.pad(xz, (0, 0, Kp // 2, Kp // 2)).unfold(1, Kp, 1)[:, :T].reshape(B, T, Gp, Dg, Kp)
    up = st(torch.einsum("btgck,gock->btgo", win, wpos.view(Gp, Dg, Dg, Kp)).reshape(B, T, D) + P["encoder.pos_conv.0.bias"])
    hid = st(xz + st(F.gelu(up)))
    if not a.layer_norm_first:
        hid = st(F.layer_norm(hid, (D,), P["encoder.layer_norm.weight"], P["encoder.layer_norm.bias"], 1e-5))
    # ---- encoder layer 0
    pre = "encoder.layers.0."
    ln = lambda t, n: st(F.layer_norm(t, (D,), P[pre + n + ".weight"], P[pre + n + ".bias"], 1e-5))

    def attn(t):
        q, k_, v_ = (st(t @ w_(pre + f"self_attn.{n}_proj.weight").t() + P[pre + f"self_attn.{n}_proj.bias"]).view(B, T, H, -1)
                     .transpose(1, 2) for n in ("q", "k", "v"))
        sc = (q @ k_.transpose(-1, -2)) * (D // H) ** -0.5
        sc = sc.masked_fill(~valid[:, None, None, :], float("-inf"))
        e = torch.exp(sc - sc.amax(dim=-1, keepdim=True))
        ctx = st(((st(e) @ v_) / e.sum(dim=-1, keepdim=True)).transpose(1, 2).reshape(B, T, D))
        return ctx @ w_(pre + "self_attn.out_proj.weight").t() + P[pre + "self_attn.out_proj.bias"]

    def ffn(t):
        f = st(F.gelu(st(t @ w_(pre + "fc1.weight").t() + P[pre + "fc1.bias"])))
        return f @ w_(pre + "fc2.weight").t() + P[pre + "fc2.bias"]

    if not a.layer_norm_first:
        x1 = ln(st(hid + attn(hid)), "self_attn_layer_norm")
        out = ln(st(x1 + ffn(x1)), "final_layer_norm")
    else:
        p1 = st(hid + attn(ln(hid, "self_attn_layer_norm")))
        out = st(p1 + ffn(ln(p1, "final_layer_norm")))
    names = [n for n in P]
    grads = torch.autograd.grad((out * G).sum(), [P[n] for n in names], allow_unused=True)
    return {n: gr for n, gr in zip(names, grads)}


# ---------------------------------------------------------------------------------------------------------------- fixtures / cases
# Lengths.  The uniform layout's geometry is set by the longest utterance (speech_encoder.conv_out_lengths of it): 40719 / 40400
# samples -> T = 126, R = roundup(T + 2, 128) = T + 2 (two spare frames); 40719 is odd at conv 4 / 5 (507, 253), 40400 at conv 1 - 3
# (4039, 2019, 1009), 20007 / 20000 at conv 1 - 4.  An utterance's valid frames are fairseq's ceil(len / (L // T)): 300 samples next to
# 40719 (chunk 323) and 320 next to 40400 (chunk 320) give exactly one valid frame; 719 alone gives T = 1 for the whole batch.
CASES = {                        # (large, lengths, dropout)
    "base": (False, [40719, 719, 300, 33333], True),
    "large": (True, [40400, 9001, 320], False),
    "base_B1": (False, [20007], True),
    "base_T1": (False, [719], True),
    "large_equal": (True, [20000, 20000], False),
    "base_nodrop": (False, [40719, 719, 300, 33333], False),
}


@pytest.fixture(scope="module")
def rigs():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from speechclip_plus_amd import hubert_frontend_train as hft, hubert_train as ht
    mp = pytest.MonkeyPatch()
    recs = (_Rec(hft.ops), _Rec(ht.ops))           # one proxy per module, shared by every rig
    mp.setattr(hft, "ops", recs[0])
    mp.setattr(ht, "ops", recs[1])
    made = {}

    def get(name):
        if name not in made:
            large, lens, drop = CASES[name]
            made[name] = _Rig(large, lens, seed=41 + len(made), recs=recs, dropout=drop)
            if name in ("base", "large"):
                assert 1 in made[name].valid, made[name].valid
            if name == "base_T1":
                assert made[name].pl.T == 1
        return made[name]

    yield get
    mp.undo()


@pytest.mark.parametrize("case", [c for c in CASES if c != "base_nodrop"])
def test_stage_by_stage_vs_fp64(rigs, case):
    """every stage of the layer backward and of the front-end backward against its fp64 definition; for base / large also the
    sensitivity self-checks: one boundary row removed on the host from the kernel's result is rejected by each criterion family"""
    rig = rigs(case)
    rep = _Report(case)
    rig.forward(rig.wav(7))
    dh1 = rig.row_grad(8)
    sens = case in ("base", "large")
    out = rig.backward(dh1=dh1, record=True)
    _check_layer(rep, rig, dh1)
    _check_front(rep, rig, out["dx_layer"], sens=sens)
    if sens:
        # attention dv: remove query row 0 of utterance 1 from every key's dv
        c = [c for c in rig.rec_l.calls if c.name == "attn_bwd"][0]
        dq_r, dk_r, dv_r, mq, mk, mv, Pd, dO, dSs, Q, K = _attn_ref(rig, c.a[0], c.a[1], c.a[2], c.a[4], c.kw.get("drop_p", 0.0),
                                                                    c.kw.get("drop_seed", 0))
        pl = rig.pl
        u1 = slice(pl.R, 2 * pl.R)
        one = (Pd[1, :, 0, :, None] * dO[1, :, 0, None, :]).transpose(0, 1).reshape(pl.R, -1)      # [key][h d]
        bad = c.pa[9].double().clone()
        bad[u1] -= one
        assert not _passes(bad, dv_r, _att_bound(dv_r, mv, pl.R))[0], "attention dv: one-query error not rejected"
        # dk: query 0 of utterance 1 removed from every key; dq: key 0 of utterance 1 removed from every query
        one = (dSs[1, :, 0, :, None] * Q[1, :, 0, None, :]).transpose(0, 1).reshape(pl.R, -1)
        bad = c.pa[8].double().clone()
        bad[u1] -= one
        assert not _passes(bad, dk_r, _att_bound(dk_r, mk, pl.R))[0], "attention dk: one-query error not rejected"
        one = (dSs[1, :, :, 0, None] * K[1, :, 0, None, :]).transpose(0, 1).reshape(pl.R, -1)
        bad = c.pa[7].double().clone()
        bad[u1] -= one
        assert not _passes(bad, dq_r, _att_bound(dq_r, mq, pl.R))[0], "attention dq: one-key error not rejected"
        # q / k / v bias column sums: one row of dqkv (utterance 1, frame 0)
        c = [c for c in rig.rec_l.calls if c.name == "colsum_bf16"][0]
        x = c.a[0].double()
        b_ = KSEC * U * _keff_colsum(x.shape[0]) * x.abs().sum(0)
        assert not _passes(c.pa[1].double() - x[pl.R], x.sum(0), b_, F32_RELL2)[0], "bias colsum: one-row error not rejected"
    rep.show()


def test_frozen_pass_through_layer(rigs):
    """train = False: no weight gradient is written, dx still meets every stage criterion and equals the trainable pass's dx"""
    for case in ("base", "large"):
        rig = rigs(case)
        rep = _Report(case + " frozen")
        rig.forward(rig.wav(9))
        dh1 = rig.row_grad(10)
        ref = rig.backward(dh1=dh1)
        rig.forward(rig.wav(9))
        out = rig.backward(dh1=dh1, train=False, record=True)
        for n in rig.tl.fairseq_names.values():
            assert out[n] is None, n
        _check_layer(rep, rig, dh1, train=False)
        assert torch.equal(out["dx_layer"], ref["dx_layer"])
        rep.show()


def _stage_rows(rig, b):
    """utterance b's rows of every row-layout gradient the chains produced: the stage outputs, the conv / pos_conv input gradients
    (gemm_raw's C), attention dq / dk / dv and what conv layer 0's backward received"""
    pl, B = rig.pl, rig.B
    pitches = set(pl.R_l) | {pl.R}
    out = []

    def add(tag, t):
        if isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[0] % B == 0 and t.shape[0] // B in pitches:
            p = t.shape[0] // B
            out.append((tag, t[b * p: (b + 1) * p]))

    for who, calls in (("front", rig.rec_f.calls), ("layer", rig.rec_l.calls)):
        for i, c in enumerate(calls):
            for j, t in enumerate(c.ret if isinstance(c.ret, tuple) else (c.ret,)):
                add(f"{who} {i} {c.name} ret {j}", t)
            if c.name == "gemm_raw":
                add(f"{who} {i} gemm_raw C", c.pa[4])
            if c.name == "attn_bwd":
                for j in (7, 8, 9):
                    add(f"{who} {i} attn_bwd {j}", c.pa[j])
            if c.name.startswith("conv0_"):
                add(f"{who} {i} {c.name} dy", c.a[5])
    return out


def _grads_equal(a, b, tag):
    for n in a:
        if a[n] is None:
            assert b[n] is None, (tag, n)
            continue
        assert torch.equal(a[n], b[n]), (tag, n, float((a[n].double() - b[n].double()).abs().max()))


@pytest.mark.parametrize("case", ["base", "large"])
def test_neighbour_independence_and_repeatability(rigs, case):
    """utterance b identical in two runs; its neighbours keep their lengths but get other waveforms, and the output gradient is zero
    on their rows.  Every gradient row of b and every parameter gradient must be bit-identical - the neighbours contribute exact
    zeros.  Two backward passes of one input give identical bits."""
    rig = rigs(case)
    B, R = rig.B, rig.pl.R
    base_wav = rig.wav(11)
    for b in sorted({0, B // 2, B - 1}):
        dh1 = rig.row_grad(12, rows_of=[b])
        runs, rows_of_b = [], []
        for other in (11, 13):
            w = rig.wav(other)
            w[b] = base_wav[b]
            rig.forward(w)
            runs.append(rig.backward(dh1=dh1, record=True))
            rows_of_b.append(_stage_rows(rig, b))
        if b == 0:                                # repeatability: the first input again
            rig.forward(base_wav)
            _grads_equal(runs[0], rig.backward(dh1=dh1), f"{case} repeat")
        a, c = runs
        rows = slice(b * R, (b + 1) * R)
        assert torch.equal(a["dx_layer"][rows], c["dx_layer"][rows]), (case, b)
        others = torch.ones(B * R, dtype=torch.bool, device=rig.dev)
        others[rows] = False
        assert float(a["dx_layer"][others].abs().max() if B > 1 else 0.0) == 0.0
        _grads_equal(a, c, f"{case} neighbours of {b}")
        assert len(rows_of_b[0]) == len(rows_of_b[1]) and len(rows_of_b[0]) > 20
        for (tag, x), (_, y) in zip(*rows_of_b):
            assert torch.equal(x, y), (case, b, tag)


@pytest.mark.parametrize("case", ["base", "large"])
def test_single_frame_support(rigs, case):
    """front end: a gradient at one frame only (the last valid frame of the longest utterance; the first frame of utterance 1).  Every
    stage must meet its fp64 criterion, whose bound is zero outside the frame's receptive field (structural zeros of the reference:
    other utterances, pad rows, rows beyond the windows) - so each of those elements must be exactly zero."""
    rig = rigs(case)
    B, R, D = rig.B, rig.pl.R, rig.arch.embed_dim
    longest = max(range(B), key=lambda b: rig.valid[b])
    for b, t in ((longest, rig.valid[longest] - 1), (1, 0)):
        dh0 = torch.zeros(B * R, D, device=rig.dev, dtype=torch.bfloat16)
        dh0[b * R + t] = torch.randn(D, generator=torch.Generator().manual_seed(15)).to(torch.bfloat16)
        rig.forward(rig.wav(14))
        rig.backward(dh0=dh0, record=True)
        rep = _Report(f"{case} frame {b}/{t}")
        _check_front(rep, rig, dh0)
        # the support really is confined: conv 1's input gradient is zero on every other utterance
        c = [c for c in rig.rec_f.calls if c.name.startswith("conv0_")][0]
        R0 = rig.pl.R_l[0]
        d0 = c.a[5][: B * R0].view(B, R0, -1)
        assert float(d0[torch.arange(B) != b].abs().max() if B > 1 else 0.0) == 0.0
        assert float(d0[b].abs().max()) > 0.0
    # one transformer layer: the gradient of hidden[1] at one frame; attention spreads it over b's valid keys only, so every other
    # utterance's rows and b's rows t >= valid_b stay exactly zero (and every stage meets its criterion, zero-bound elements exact)
    for b, t in ((longest, rig.valid[longest] - 1), (1, 0)):
        dh1 = torch.zeros(B * R, D, device=rig.dev, dtype=torch.bfloat16)
        dh1[b * R + t] = torch.randn(D, generator=torch.Generator().manual_seed(16)).to(torch.bfloat16)
        rig.forward(rig.wav(14))
        out = rig.backward(dh1=dh1, record=True)
        rep = _Report(f"{case} layer frame {b}/{t}")
        _check_layer(rep, rig, dh1)
        dx = out["dx_layer"].view(B, R, D)
        inside = torch.zeros(B, R, dtype=torch.bool, device=rig.dev)
        inside[b, : rig.valid[b]] = True
        assert float(dx[~inside].abs().max()) == 0.0 and float(dx[b, t].abs().max()) > 0.0


@pytest.mark.parametrize("case", ["base", "large"])
def test_pad_rows_are_never_mixed_in(rigs, case):
    """After the forward, rows the kernels are told are padding get +-1e4 (finite) in the saved activations; the backward must not
    change a bit.  Rows: every frame t >= valid_b of the row-local stage inputs (LayerNorm inputs, GEMM operands: their output gradient
    is exactly zero there), conv rows past the receptive field of the valid frames.  NOT overwritten: the attention's saved q / k / v,
    LSE and output at any row - sc_attn_bwd_bf16 only promises that query rows t >= q_rows carry dO = 0, and its dq kernel visits them
    (recomputing probabilities from q and lse2); the waveform (conv layer 0 recomputes from it; tests/test_gpu_frontend.py)."""
    rig = rigs(case)
    pl, a = rig.pl, rig.arch
    B, R = pl.B, pl.R
    w = rig.wav(16)
    dh1 = rig.row_grad(17)
    rig.forward(w)
    clean = rig.backward(dh1=dh1)
    rig.forward(w)
    g = torch.Generator(device="cpu").manual_seed(18)

    def junk(buf, pitch, keep_rows):
        v = buf[: B * pitch].view(B, pitch, -1)
        for b in range(B):
            n = v.shape[2]
            r = pitch - keep_rows[b]
            if r > 0:
                j = (torch.randint(0, 2, (r, n), generator=g).float() * 2 - 1) * 1e4
                v[b, keep_rows[b]:] = j.to(v.dtype).to(v.device)

    s = pl.train[0]
    for key in ("pre1", "x1", "u", "f", "pre2"):
        junk(s[key], R, rig.valid)
    junk(pl.hidden[0], R, rig.valid)
    st = rig.st
    junk(st["u_pos"], R, rig.valid)
    junk(st["pre"], R, rig.valid)
    junk(pl.feat_ln, R, rig.valid)
    need = list(rig.valid)                      # conv rows the valid frames read, layer by layer down
    for i in range(len(a.conv_kernels) - 1, -1, -1):
        junk(pl.conv[i], pl.R_l[i], need)
        if i >= 1:
            junk(st["u"][i], pl.R_l[i], need)
            if i in st["n"]:
                junk(st["n"][i], pl.R_l[i], need)
            k, s_ = a.conv_kernels[i], a.conv_strides[i]
            need = [(n - 1) * s_ + k if n > 0 else 0 for n in need]
    _grads_equal(clean, rig.backward(dh1=dh1), f"{case} pad junk")


@pytest.mark.parametrize("case", ["base", "large"])
def test_qkv_bias_gradient_layouts(rigs, case):
    """q / k / v bias gradients: the as_strided add (parameters' gradients in the optimiser's flat buffer, one stride apart) and the
    per-tensor loop give identical bits, and so does every other gradient"""
    rig = rigs(case)
    w, dh1 = rig.wav(19), rig.row_grad(20)
    rig.forward(w)
    loop = rig.backward(dh1=dh1)
    rig.forward(w)
    flat = rig.backward(dh1=dh1, flat_grads=True)
    ps = rig.tl.layer_parameters(0)
    # the product's condition for the as_strided add: q / k / v bias gradients contiguous in one storage, equally spaced
    tb = [ps[1].grad, ps[3].grad, ps[5].grad]
    step = (tb[1].data_ptr() - tb[0].data_ptr()) // 4
    assert step > 0 and tb[2].data_ptr() == tb[0].data_ptr() + 8 * step and all(
        t.is_contiguous() and t.untyped_storage().data_ptr() == tb[0].untyped_storage().data_ptr() for t in tb)
    _grads_equal(loop, flat, f"{case} bias layout")


@pytest.mark.parametrize("case", ["base_nodrop", "large"])
def test_whole_chain_vs_bf16_storage_control(rigs, case):
    """front end + one layer, every parameter gradient: the kernels add no more error than the storage format does -
    rel-L2(HIP, control) <= rel-L2(control, fp64), control = the fp64 chain with bf16 at the product's storage sites.  Dropout is off
    (base_nodrop; large has none): the masks are checked stage by stage above.  Sensitivity: removing the first window of utterance 1
    from the HIP conv 4 weight gradient must break the criterion."""
    rig = rigs(case)
    w = rig.wav(21)
    dh1 = rig.row_grad(22)
    rig.forward(w)
    hip = rig.backward(dh1=dh1, record=True)
    G = dh1.view(rig.B, rig.pl.R, -1)[:, : rig.pl.T].double()
    with torch.enable_grad():
        ctrl = _chain64(rig, w, G, emulate=True)
        ref = _chain64(rig, w, G, emulate=False)
    rows = []
    for n, gr in ctrl.items():
        if n.endswith("self_attn.k_proj.bias"):
            continue                      # exactly zero in exact arithmetic (softmax ignores a per-query shift): rel-L2 of noise
        if gr is None:                    # large (pre-LN): the encoder LayerNorm acts on an output the layers never read
            assert hip[n] is None or float(hip[n].abs().max()) == 0.0, n
            continue
        e_hc, e_cf = rel_l2(hip[n], gr), rel_l2(gr, ref[n])
        rows.append((n, e_hc, e_cf))
        print(f"[trainable-bwd] {case:>11s} whole chain {n:48s} rel-L2(HIP, control) {e_hc:9.3g}   rel-L2(control, fp64) {e_cf:9.3g}"
              f"   rel-L2(HIP, fp64) {rel_l2(hip[n], ref[n]):9.3g}")
    # + F32_RELL2: the stage criterion of one fp32 reduction, the kernels' own error where storage adds none (the layer's last bias
    # gradient is the column sum of the output gradient itself: control == fp64 there)
    bad = [r for r in rows if not r[1] <= r[2] + F32_RELL2]
    assert not bad, bad
    assert len(rows) >= 20
    # sensitivity: conv 4's weight gradient without one window of utterance 1 (its largest contribution)
    pl, C = rig.pl, rig.arch.conv_dim
    c = [c for c in rig.rec_f.calls if c.name == "wgrad_bf16"][3]                  # post_extract_proj, conv 6, 5, 4
    assert c.pa[2].shape == (C, 3 * C)
    du = c.a[0].double().view(rig.B, pl.R_l[4], C)
    X = pl.conv[3][: rig.B * pl.R_l[3]].double().view(rig.B, pl.R_l[3], C)
    m = int((du[1].norm(dim=1) * X[1, : 2 * pl.R_l[4]].view(pl.R_l[4], 2 * C).norm(dim=1)).argmax())
    one = torch.outer(du[1, m], X[1, 2 * m: 2 * m + 3].reshape(-1)).view(C, 3, C).permute(0, 2, 1)
    n = "feature_extractor.conv_layers.4.0.weight"
    e_bad = rel_l2(hip[n].double() - one, ctrl[n])
    print(f"[trainable-bwd] {case:>11s} whole chain sensitivity: conv 4 window {m} of utterance 1 removed: rel-L2(HIP', control) {e_bad:.3g}")
    assert e_bad > rel_l2(ctrl[n], ref[n]) + F32_RELL2, "whole chain: one-window error not rejected"
