"""GPU: the frozen HuBERT forward as the product runs it - FairseqSpeechEncoder_Hubert._encode (conv layers 1 .. 6, feature LayerNorm,
post_extract_proj, pos_conv, encoder LayerNorm, the encoder layers; post-LN base, pre-LN large) - stage by stage against float64,
element by element.

Nothing of the forward is restated: a recording proxy replaces the ``ops`` attribute of speechclip_plus_amd.speech_encoder, clones
every argument before and after each call and keeps the call itself for replays.  The per-op branch of _layers is taken when
``ops._timer is not None`` as speech_encoder sees it: the proxy answers that attribute with a sentinel while the real ops module keeps
None, so no timing event is recorded and the kernels are launched exactly as in production.  The float64 reference of a stage is
fairseq's definition (conv1d with the layer's stride, layer_norm, linear, the grouped pos_conv with padding 64 and SamePad, exact
erf-GELU, softmax attention with keys < valid) on the stage's own recorded bf16 inputs.  Conv layer 0 is covered by
tests/test_gpu_frontend.py.

Bounds: docs/parity.md ("Frozen HuBERT forward"); every constant below carries its derivation and was fixed before the first GPU
run.  On top of the stage checks: the encoder's bf16 working copies against the state dict, the bit-exact invariants (C++ layer driver
== op by op, pad rows never mixed in, repeatability, the GEMM tile families at more than 256 output tiles) and a sensitivity check per
criterion (a one-row, one-chunk, one-key, one-k-block or two-ulp error applied on the host to the kernel's result must be rejected)."""
import dataclasses
import inspect
import math

import numpy as np
import pytest
import torch

from test_gpu_trainable_bwd import BF16_RELL2, FTZ, KSEC, STORE, U, _passes, _Seq

pytestmark = pytest.mark.gpu

EPS = 1e-5
GELU_FIT = 3.5e-6      # |gelu_bf2 - x Phi(x)| in fp32 behind the bf16 store: pinned by test_bf16_site_gelu_against_the_exact_erf_gelu
GELU_LIP = 1.13        # max |d/dx x Phi(x)| = 1.129 (at x = sqrt(2)): what an error of the GELU's fp32 argument is multiplied by
K_EPI = 3              # fp32 operations on an accumulator besides its K products: it starts from the bias (one add), the dropout
#                        scale 1 / (1 - p) and the residual add - K_eff = K + 3 (MFMA 16x16x32 over K-tiles of 64, serial in k)
C_P = 1                # attention: the probabilities enter P.V as bf16(p), ONE rounding relative to p itself - the (possibly stale, by
#                        < 2^6) running max only scales p <= 64, far from bf16's range limits; the row sum adds the unrounded fp32 p
ATT_ACC = 2            # attention: fp32 accumulation over <= R keys of BOTH the numerator (P.V) and the row sum
EXP_ULP = 2            # v_exp_f32: 1 ulp = 2 U relative
SENTINEL = object()    # what the proxy answers for ops._timer on the per-op path


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# ---------------------------------------------------------------------------------------------------------------- recording proxy
def _cl(x):
    if isinstance(x, torch.Tensor):
        return x.detach().clone()
    if isinstance(x, (list, tuple)):
        return type(x)(_cl(v) for v in x)
    if isinstance(x, dict) and not any(isinstance(k, str) and k.startswith("l0_") for k in x):
        return {k: _cl(v) for k, v in x.items()}
    return x                    # the weight dict handed to hubert_layer_fwd (read-only) and plain objects are kept by reference


class _Call:
    def __init__(self, name, fn, raw, pre, post):
        self.name, self.fn, self.raw = name, fn, raw
        (self.a, self.kw), (self.pa, self.pkw) = pre, post

    def replay(self):
        self.fn(*self.raw[0], **self.raw[1])


class _FwdRec:
    """Stands in for ``ops`` inside speech_encoder.  Function calls are forwarded to the real module (whose own _timer stays None);
    while ``on`` their arguments are cloned before and after.  ``per_op``: answer ``_timer`` with a sentinel, so _layers takes the
    op-by-op branch instead of the one-call-per-layer driver."""

    def __init__(self, mod):
        self._m, self.calls, self.on, self.per_op = mod, [], False, True

    def __getattr__(self, name):
        if name == "_timer":
            assert self._m._timer is None
            return SENTINEL if self.per_op else None
        f = getattr(self._m, name)
        if not inspect.isfunction(f):
            return f

        def wrap(*a, **kw):
            if not self.on:
                return f(*a, **kw)
            pre = _cl((a, kw))
            r = f(*a, **kw)
            self.calls.append(_Call(name, f, (a, kw), pre, _cl((a, kw))))
            return r
        return wrap


# ---------------------------------------------------------------------------------------------------------------- the rig
# Lengths in samples.  48123 -> conv lengths 9623, 4811, 2405, 1202, 600, 300, T = 150 (odd at conv 0 - 2), chunk = L // T = 320, so an
# utterance's valid frames are ceil(len / 320): 20777 -> 65 (1 above a multiple of 64), 40601 -> 127 (1 below a multiple of 128),
# 1500 -> 5.  Segment layout: pitches 152, 72, 136, 8 (M = 368); uniform layout: R = 256 (M = 1024).  Neither reaches the 256-row
# persistent kernel (M < 512 or fewer than 192 tiles): their GEMMs run on the dispatcher's 128 x 128, 128 x 64 and 64 x 64 tiles.
# wide: 160000 -> T = 499, pitch 504 with ragged = False, M = 16 x 504 = 8064 = 32 M-tiles of 256 rows: fc1 and QKV have more than 256
# output tiles at either tile width (384 / 288 at 256 columns: several tiles per workgroup, the tile hand-over runs), conv 1 - 6
# 2016 .. 64 tiles, out_proj / fc2 96.  33333 -> T = 103 alone.
SMALL = [48123, 20777, 40601, 1500]
WIDE = [160000] * 12 + [159000, 120001, 80000, 150001]
CASES = {                              # (large, lengths, train)
    "base_small": (False, SMALL, False),
    "large_small": (True, SMALL, False),
    "base_wide": (False, WIDE, False),
    "base_B1": (False, [33333], False),
    "large_B1": (True, [33333], False),
    "base_train": (False, SMALL, True),
}
# layouts: "uniform" = B x R rows (what an encoder with unfrozen layers uses), "segment" = per-utterance pitches (the frozen encoder's
# default), "flat" = segment tables with every utterance at the padded length (ragged = False)


class _Lay:
    """rows of the batch in flight: first row, pitch, valid frames"""

    def __init__(self, pl, valid):
        B = pl.B
        if pl.seg is None:
            self.r0, self.pitch = [b * pl.R for b in range(B)], [pl.R] * B
        else:
            self.r0, self.pitch = list(pl.seg.row0_host[:-1]), list(pl.seg.pitch)
        self.valid, self.M, self.B, self.seg = list(valid), pl.M, B, pl.seg is not None
        self.max_pitch = max(self.pitch)

    def mask(self, upto, dev):
        m = torch.zeros(self.M, dtype=torch.bool, device=dev)
        for b in range(self.B):
            m[self.r0[b]: self.r0[b] + upto[b]] = True
        return m


class _Run:
    def __init__(self, rig, pl, calls):
        self.pl, self.calls = pl, calls
        T, chunk = pl.T, pl.L // pl.T
        valid = [min(T, -(-int(l) // chunk)) for l in rig.lens]                 # fairseq forward_padding_mask
        assert valid == pl.valid.cpu().tolist()
        self.lay = _Lay(pl, valid)
        self.hidden = pl.hidden.clone()
        self.scratch = {k: getattr(pl, k).clone() for k in ("qk", "ctx", "x1", "ffn", "pre")}
        self.scratch["vt"] = pl.vt.clone()


class _Rig:
    """the frozen encoder (two layers at the shipped widths, random weights) on one batch, driven through _encode"""

    def __init__(self, case, rec):
        from speechclip_plus_amd import random_hubert_state_dict
        from speechclip_plus_amd import speech_encoder as se
        large, lens, train = CASES[case]
        self.case, self.large, self.lens, self.rec = case, large, list(lens), rec
        name = "hubert_large_ll60k" if large else "hubert"
        self.arch = a = dataclasses.replace(se.ARCHS[name], layers=2)
        self.sd = random_hubert_state_dict(a, seed=97 + len(case))
        self.dev = torch.device("cuda:0")
        self.enc = se.FairseqSpeechEncoder_Hubert(name, arch=a, state_dict=self.sd, device="cuda:0")
        self.enc.train(train)
        assert self.enc._dropout_active() == train
        g = torch.Generator().manual_seed(5 + len(case))
        B, L = len(lens), max(lens)
        w = torch.zeros(B, L)
        for b, l in enumerate(lens):
            w[b, :l] = torch.randn(l, generator=g) * 0.5
        self.wav = w.to(self.dev)
        self.rows_used = {}                      # per plan: the most rows any run has laid out in it

    def run(self, layout, per_op=True, record=True):
        enc, rec = self.enc, self.rec
        uniform = layout == "uniform"
        enc._seg_mode = (lambda: False) if uniform else (lambda: True)          # the uniform B x R rows of an encoder with unfrozen layers
        rec.calls, rec.on, rec.per_op = [], record, per_op
        enc._drop_calls = 0                                                     # the same dropout seeds in every run
        try:
            pl = enc._encode(self.wav, self.lens, ragged=(layout == "segment"))
            torch.cuda.synchronize()
        finally:
            rec.on = False
        assert (pl.seg is None) == uniform
        self.rows_used[id(pl)] = max(self.rows_used.get(id(pl), 0), pl.M)
        return _Run(self, pl, rec.calls)


@pytest.fixture(scope="module")
def rigs():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from speechclip_plus_amd import speech_encoder as se
    mp = pytest.MonkeyPatch()
    rec = _FwdRec(se.ops)
    mp.setattr(se, "ops", rec)
    made = {}

    def get(case):
        if case not in made:
            made[case] = _Rig(case, rec)
        return made[case]

    yield get
    mp.undo()


# ---------------------------------------------------------------------------------------------------------------- criteria
class _Report:
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

    def show(self):
        for k, (r, e, w) in self.rows.items():
            print(f"[frozen-fwd] {self.tag:>22s} {k:36s} max err/bound {r:8.3g} at {w:14s} rel-L2 {e:9.3g}")


def _gemm_ref(A, W, bias, act=0, res=None, keep=None, p=0.0):
    """fp64 linear stage + its bound: STORE |ref| + KSEC U (K + K_EPI) (|A| @ |W|^T + |bias|) (x GELU_LIP + GELU_FIT behind a GELU).
    The residual is added in fp32 in front of the ONLY rounding (csrc/gemm_epilogue.inc, csrc/gemm_bf16.hip), dropout scales the fp32
    value in front of the residual add.  A dropped element has bound 0: it must be exactly the residual (or zero)."""
    A, W = A.double(), W.double()
    dot, mag = A @ W.t(), A.abs() @ W.abs().t()
    if bias is not None:
        dot, mag = dot + bias.double(), mag + bias.double().abs()
    err = KSEC * U * (A.shape[1] + K_EPI) * mag
    ref = dot
    if act == 1:
        ref, err = _gelu(dot), GELU_LIP * err + GELU_FIT
    z = torch.zeros((), dtype=torch.float64, device=ref.device)
    if keep is not None:
        ref, err = torch.where(keep, ref / (1.0 - p), z), torch.where(keep, err / (1.0 - p), z)
    if res is not None:
        ref = ref + res.double()
    bound = err + STORE * ref.abs()
    if keep is not None:
        bound = torch.where(keep, bound, z)
    return ref, bound


def _keep(rows, N, p, seed, dev, row_from=0):
    from test_gpu_kernels import _keep_mask
    idx = np.arange(row_from * N, (row_from + rows) * N, dtype=np.int64)
    return torch.from_numpy(_keep_mask(idx, seed, p)).view(rows, N).to(dev)


def _ln_ref(x, g, b, act=0):
    """layer_norm(eps 1e-5) in fp64 + its bound.  The kernel (csrc/rowops.hip) takes the two-pass mean / variance in fp32 over D
    channels: the mean is off by <= D U mean|x|, rstd by <= D U relative; y = xhat g + beta inherits |g| (|xhat| + rstd mean|x|) D U."""
    x, g, b = x.double(), g.double(), b.double()
    D = x.shape[1]
    mu = x.mean(1, keepdim=True)
    xc = x - mu
    rstd = ((xc * xc).mean(1, keepdim=True) + EPS).rsqrt()
    xh = xc * rstd
    ref = xh * g + b
    err = KSEC * D * U * (g.abs() * (xh.abs() + rstd * x.abs().mean(1, keepdim=True)) + b.abs())
    if act == 1:
        ref, err = _gelu(ref), GELU_LIP * err + GELU_FIT
    return ref, err + STORE * ref.abs()


def _vt_rows(vt, lay, D):
    """the V^T buffer ([B, H, 64, R], or per utterance [H, 64, pitch] back to back at D * row0) as rows [M, D]"""
    if not lay.seg:
        B, R = lay.B, lay.pitch[0]
        return vt.view(B, D, R).transpose(1, 2).reshape(B * R, D)
    flat = vt.reshape(-1)
    return torch.cat([flat[D * r0: D * (r0 + p)].view(D, p).t() for r0, p in zip(lay.r0, lay.pitch)])


def _attn_ref(c, lay, b, drop_query=None):
    """fp64 attention of utterance b over its pitch on the recorded q / k / V^T: softmax(scale q k^T, keys < valid) v per head, the
    probability dropout rebuilt on the host.  Returns ref [pitch, D], bound.  ``drop_query`` = (query, key): that key is removed from
    that query's softmax (sensitivity)."""
    from test_gpu_kernels import _keep_mask8
    qk, vt = c.a[0], c.a[1]
    H, D, scale = c.a[6], c.a[7], c.a[8]
    p_att, seed = c.kw.get("drop_p", 0.0), c.kw.get("drop_seed", 0)
    r0, P = lay.r0[b], lay.pitch[b]
    nv = max(1, min(lay.valid[b], P))
    dev = qk.device
    rows = qk[r0: r0 + P].double()
    q = rows[:, :D].view(P, H, 64).transpose(0, 1)
    k = rows[:, D:].view(P, H, 64).transpose(0, 1)
    v = _vt_rows(vt, lay, D)[r0: r0 + P].double().view(P, H, 64).transpose(0, 1)
    s = (q @ k.transpose(-1, -2)) * scale
    sa = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    ok = (torch.arange(P, device=dev)[None, None, :] < nv).expand(H, P, P).clone()
    if drop_query is not None:
        ok[:, drop_query[0], drop_query[1]] = False
    s = s.masked_fill(~ok, float("-inf"))
    smax = s.amax(-1, keepdim=True)
    Pm = torch.softmax(s, dim=-1)
    # the exponent fmaf(s, c, -m c) in the log2 domain and v_exp_f32: relative error of one probability (ln 2 x the absolute error of
    # the exponent, c ln 2 = scale): U (max|s| + |s - max| + 6 ln 2 [stale max] + 2 x 64 scale |q|.|k| [S = q k^T in fp32, K = 64] + 2)
    sm = s.masked_fill(~ok, 0.0)
    e = U * (sm.abs().amax(-1, keepdim=True) + (sm - smax).abs() + 6 * math.log(2.0) + KSEC * 64 * sa + EXP_ULP)
    e = e.masked_fill(~ok, 0.0)
    if p_att > 0:
        h = torch.arange(H, dtype=torch.int64)[:, None, None]
        qi = torch.arange(P, dtype=torch.int64)[None, :, None]
        ki = torch.arange(P, dtype=torch.int64)[None, None, :]
        if lay.seg:            # csrc/attention.hip drop_row: (h * rows + row0 + q) * max_pitch + key; uniform: ((b H + h) R + q) R + key
            idx = (h * lay.M + r0 + qi) * lay.max_pitch + ki
        else:
            idx = ((b * H + h) * P + qi) * P + ki
        keep, pa = _keep_mask8(idx.numpy().reshape(-1) & 0xffffffff, seed, p_att)
        Pm = Pm * (torch.from_numpy(keep).view(H, P, P).to(dev).double() / (1.0 - pa))
    ref = Pm @ v
    pv = Pm @ v.abs()
    exp_term = KSEC * ((Pm * e) @ v.abs() + (Pm * e).sum(-1, keepdim=True) * pv)
    bound = STORE * ref.abs() + C_P * STORE * pv + KSEC * ATT_ACC * P * U * pv + exp_term
    un = lambda t: t.transpose(0, 1).reshape(P, D)
    return un(ref), un(bound)


# ---------------------------------------------------------------------------------------------------------------- stage checks
def _rows_blocks(n, step):
    return [(i, min(n, i + step)) for i in range(0, n, step)]


def _check_conv(rep, rig, c, i):
    a = rig.arch
    C, k, s = a.conv_dim, a.conv_kernels[i], a.conv_strides[i]
    A, lda, W, ldw, Cb, ldc, M, N, K = c.a[:9]
    assert (lda, ldw, ldc, N, K) == (s * C, k * C, C, C, k * C) and c.kw["tap_c"] == (C if (k == 3 and s == 2) else 0)
    # fairseq Conv1d: out[t, co] = sum_{ci, j} w[co, ci, j] x[s t + j, ci] (+ bias), straight from the state dict
    Wf = rig.sd[f"feature_extractor.conv_layers.{i}.0.weight"].to(torch.bfloat16).to(A.device)            # [co][ci][tap]
    Wk = Wf.permute(0, 2, 1).reshape(C, k * C)                                                             # a window is [tap][ci]
    win = A.reshape(-1).as_strided((M, K), (lda, 1))
    got = c.pa[4]
    for lo, hi in _rows_blocks(M, 32768):
        ref, bound = _gemm_ref(win[lo:hi], Wk, c.kw["bias"], act=c.kw["act"])
        rep.check(f"conv {i} (k = {k}, s = {s})" + (" + GELU" if c.kw["act"] else ""), got[lo:hi], ref, bound, BF16_RELL2)
    assert torch.equal(got[M:], c.a[4][M:]), f"conv {i}: rows past M written"
    return got


def _check_ln(rep, c, stage):
    x, g, b = c.a[0], c.a[1], c.a[2]
    got = c.pkw["out"]
    for lo, hi in _rows_blocks(x.shape[0], 65536):
        ref, bound = _ln_ref(x[lo:hi], g, b, c.kw.get("act", 0))
        rep.check(stage, got[lo:hi], ref, bound, BF16_RELL2)
    return got


def _check_linear(rep, c, stage):
    x, w, bias = c.a[0], c.a[1], c.a[2]
    res, act = c.kw.get("residual"), c.kw.get("act", 0)
    p, seed = c.kw.get("drop_p", 0.0), c.kw.get("drop_seed", 0)
    got = c.pkw["out"]
    N = w.shape[0]
    for lo, hi in _rows_blocks(x.shape[0], 4096):
        keep = _keep(hi - lo, N, p, seed, x.device, row_from=lo) if p > 0 else None
        ref, bound = _gemm_ref(x[lo:hi], w, bias, act=act, res=None if res is None else res[lo:hi], keep=keep, p=p)
        rep.check(stage, got[lo:hi], ref, bound, BF16_RELL2)
    return got


def _check_qkv(rep, c, lay, stage):
    x, lda, W, ldw, qk0, ldc, M, N, K = c.a[:9]
    D = K
    assert (N, ldc, c.kw["n_split"]) == (3 * D, 2 * D, 2 * D) and M == lay.M
    qk, vt = c.pa[4], c.pkw["Ct"]
    vrows = _vt_rows(vt, lay, D)
    for lo, hi in _rows_blocks(M, 4096):
        ref, bound = _gemm_ref(x[lo:hi], W, c.kw["bias"])
        rep.check(stage + " q / k", qk[lo:hi], ref[:, : 2 * D], bound[:, : 2 * D], BF16_RELL2)
        rep.check(stage + " V^T", vrows[lo:hi], ref[:, 2 * D:], bound[:, 2 * D:], BF16_RELL2)
    assert torch.equal(vt.reshape(-1)[D * M:], c.kw["Ct"].reshape(-1)[D * M:]), "V^T: elements past the batch's rows written"
    return qk, vt


def _check_attn(rep, c, lay, stage):
    out = c.pa[3]
    for b in range(lay.B):
        ref, bound = _attn_ref(c, lay, b)
        r0, P = lay.r0[b], lay.pitch[b]
        rep.check(stage, out[r0: r0 + P], ref, bound, BF16_RELL2)
    return out


def _check_posconv(rep, rig, c_prep, c, lay):
    a, w = rig.arch, rig.enc._w
    D, G, Kp = a.embed_dim, a.pos_conv_groups, a.pos_conv_kernel
    Dg, halo = D // G, Kp // 2
    x, xz = c_prep.a[0], c_prep.pa[2]
    # prep: frames >= valid are zero, every other row is the input to the bit
    assert torch.equal(xz, torch.where(lay.mask(lay.valid, x.device)[:, None], x, torch.zeros_like(x))), "pos_conv prep: padded-frame mask"
    assert torch.equal(c.a[3], xz) and torch.equal(c.a[1], w["pos_w"])
    Wg = w["pos_w"].double().view(G, Dg, Kp, Dg).permute(0, 1, 3, 2)               # [g][co][ci][tap]
    bias = w["pos_b"].double()
    got = c.pa[4]
    for b in range(lay.B):
        r0, P = lay.r0[b], lay.pitch[b]
        xb = xz[r0: r0 + P].double()            # every row of the pitch: frames >= valid are zero, as are the frames past the pitch
        win = torch.nn.functional.pad(xb, (0, 0, halo, halo)).unfold(0, Kp, 1)[:P].reshape(P, G, Dg, Kp)      # SamePad drops the last frame
        u = torch.einsum("tgic,goic->tgo", win, Wg).reshape(P, D) + bias
        mag = torch.einsum("tgic,goic->tgo", win.abs(), Wg.abs()).reshape(P, D) + bias.abs()
        ref = xb + _gelu(u)
        bound = STORE * ref.abs() + GELU_LIP * KSEC * U * (Kp * Dg + K_EPI) * mag + GELU_FIT
        rep.check("pos_conv + GELU + residual", got[r0: r0 + P], ref, bound, BF16_RELL2)
    return got


def _check_chain(rep, rig, run):
    """every recorded call of one per-op forward, in the order the product issued them"""
    a, w, lay, pl = rig.arch, rig.enc._w, run.lay, run.pl
    ln_mode = a.extractor_mode == "layer_norm"
    train = rig.enc.training
    sq = _Seq(run.calls)
    sq.take("wav_prep_seg" if lay.seg else "wav_prep")
    sq.take(("conv0_layernorm_gelu" if ln_mode else "conv0_groupnorm_gelu") + ("_seg" if lay.seg else ""))     # tests/test_gpu_frontend.py
    prev = None
    for i in range(1, len(a.conv_kernels)):
        c = sq.take("gemm_raw")
        assert prev is None or torch.equal(c.a[0], prev)
        assert torch.equal(c.a[2], w[f"conv{i}_w"])
        prev = _check_conv(rep, rig, c, i)
        if ln_mode:
            c = sq.take("layernorm_bf16")
            assert torch.equal(c.a[0], prev[: c.a[0].shape[0]]) and c.kw["act"] == 1
            out = _check_ln(rep, c, f"conv {i} LayerNorm + GELU")
            prev = torch.cat([out, prev[out.shape[0]:]])
    c = sq.take("layernorm_bf16")
    assert torch.equal(c.a[0], prev[: lay.M])
    feat = _check_ln(rep, c, "feature LayerNorm")
    c = sq.take("linear_bf16")
    assert torch.equal(c.a[0], feat) and torch.equal(c.a[1], w["proj_w"])
    assert c.kw["drop_p"] == (a.dropout_input if train else 0.0)
    xp = _check_linear(rep, c, "post_extract_proj" + (" + dropout_input" if train else ""))
    c_prep = sq.take("posconv_prep_seg" if lay.seg else "posconv_prep")
    assert torch.equal(c_prep.a[0], xp)
    c = sq.take("posconv_seg" if lay.seg else "posconv")
    x = _check_posconv(rep, rig, c_prep, c, lay)
    p_res = a.dropout if train else 0.0
    if not a.layer_norm_first:
        c = sq.take("layernorm_bf16")
        assert torch.equal(c.a[0], x)
        x = _check_ln(rep, c, "encoder LayerNorm")
        if p_res > 0:
            c = sq.take("dropout_bf16")
            assert torch.equal(c.a[0], x)
            keep = _keep(x.shape[0], x.shape[1], c.a[1], c.a[2], x.device)
            ref = torch.where(keep, x.float() / (1 - c.a[1]), torch.zeros((), device=x.device)).to(torch.bfloat16)
            assert torch.equal(c.pkw["out"], ref), "encoder dropout mask"
            rep.rows.setdefault("encoder dropout (bitwise)", (0.0, 0.0, ""))
            x = c.pkw["out"]
    assert torch.equal(run.hidden[0], x)
    for i in range(a.layers):
        tag = f"layer {i} "
        if a.layer_norm_first:
            c = sq.take("layernorm_bf16")
            assert torch.equal(c.a[0], x)
            xin = _check_ln(rep, c, tag + "ln1")
        else:
            xin = x
        c = sq.take("gemm_raw")
        assert torch.equal(c.a[0], xin) and torch.equal(c.a[2], w[f"l{i}_qkv_w"])
        qk, vt = _check_qkv(rep, c, lay, tag + "QKV")
        c = sq.take("attn_fwd")
        assert torch.equal(c.a[0], qk) and torch.equal(c.a[1], vt) and c.kw["drop_p"] == (a.attention_dropout if train else 0.0)
        ctx = _check_attn(rep, c, lay, tag + "attention")
        c = sq.take("linear_bf16")
        assert torch.equal(c.a[0], ctx) and torch.equal(c.a[1], w[f"l{i}_o_w"]) and torch.equal(c.kw["residual"], x)
        assert c.kw["drop_p"] == p_res
        pre = _check_linear(rep, c, tag + "out_proj + residual")
        c = sq.take("layernorm_bf16")
        assert torch.equal(c.a[0], pre)
        x1 = _check_ln(rep, c, tag + ("ln2" if a.layer_norm_first else "ln1"))
        c = sq.take("linear_bf16")
        assert torch.equal(c.a[0], x1) and torch.equal(c.a[1], w[f"l{i}_fc1_w"]) and c.kw["act"] == 1
        f = _check_linear(rep, c, tag + "fc1 + GELU")
        c = sq.take("linear_bf16")
        assert torch.equal(c.a[0], f) and torch.equal(c.a[1], w[f"l{i}_fc2_w"]) and c.kw["drop_p"] == p_res
        assert torch.equal(c.kw["residual"], pre if a.layer_norm_first else x1)
        x = _check_linear(rep, c, tag + "fc2 + residual")
        if not a.layer_norm_first:
            c = sq.take("layernorm_bf16")
            assert torch.equal(c.a[0], x)
            x = _check_ln(rep, c, tag + "ln2")
        assert torch.equal(run.hidden[i + 1], x)
    assert sq.done()
    # rows past the rows any batch has laid out in the plan's capacity-sized buffers were never written (a fresh plan is zero)
    top = rig.rows_used[id(pl)]
    for k, v in pl._rows.items():
        assert float(v[top:].abs().max() if v.shape[0] > top else 0.0) == 0.0, k
    if top == lay.M:
        tail = pl._hidden[pl.NL * lay.M * pl.D:]
        assert float(tail.abs().max() if tail.numel() else 0.0) == 0.0


STAGE_RUNS = [("base_small", "uniform"), ("base_small", "segment"), ("large_small", "uniform"), ("large_small", "segment"),
              ("base_wide", "flat"), ("base_B1", "segment"), ("large_B1", "uniform"), ("base_train", "uniform"), ("base_train", "segment")]


@pytest.mark.parametrize("case,layout", STAGE_RUNS)
def test_stage_by_stage_vs_fp64(rigs, case, layout):
    """every stage of the frozen forward against its fp64 definition on its own recorded inputs, element by element"""
    rig = rigs(case)
    run = rig.run(layout)
    lay = run.lay
    if CASES[case][1] is SMALL:
        assert lay.valid == [150, 65, 127, 5]
        assert lay.pitch == ([152, 72, 136, 8] if layout == "segment" else [256] * 4)
    if case == "base_wide":
        M = lay.M
        assert -(-M // 256) * 12 > 256 and -(-M // 256) * 9 > 256, M             # fc1 / QKV: several tiles per workgroup
    rep = _Report(f"{case}/{layout}")
    try:
        _check_chain(rep, rig, run)
    finally:
        rep.show()


# ---------------------------------------------------------------------------------------------------------------- working copies
POS_STRADDLE_SHARE = {"base_small": 8.05e-6, "large_small": 7.51e-6}     # CPU rehearsal: 38 of 4718592 and 63 of 8388608 elements


def test_working_copies_match_the_state_dict(rigs):
    """Every entry of the encoder's weight dict that the forward reads == fairseq's definition on the state dict, rounded once to bf16
    (GEMM operands) or kept in fp32 (biases, norm vectors): torch.equal.  The weight-normed pos_conv weight g v / ||v|| (norm over
    dims 0, 1: weight_norm(dim = 2)) is evaluated in fp32 by _load_weights; against the bf16 rounding of the fp64 value it may differ
    where the two straddle a rounding boundary, by one bf16 ulp at most.  CPU rehearsal of _load_weights' arithmetic on the same
    seeds: 38 of 4718592 elements (base, 8.05e-6) and 63 of 8388608 (large, 7.51e-6) straddle; the cap is 4x that share."""
    for case in ("base_small", "large_small"):
        share = POS_STRADDLE_SHARE[case]
        rig = rigs(case)
        a, w = rig.arch, {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in rig.enc._w.items()}
        n_diff, numel, worst = _working_copies(a, rig.sd, w, rig.enc._load_weights, lambda: rig.enc._w["pos_w"].cpu())
        print(f"[frozen-fwd] {case}: weight-normed pos_conv, {n_diff} of {numel} elements off the fp64 rounding ({n_diff / numel:.3g}), "
              f"worst {worst:.3g} ulp")
        assert n_diff <= 4 * share * numel, (n_diff, numel)


def _working_copies(a, sd, w, load, pos_w):
    """-> (pos_conv elements that differ from the bf16 rounding of the fp64 weight norm, their number, the largest difference in ulps)"""
    bf = lambda t: t.to(torch.bfloat16)
    C = a.conv_dim
    eq = lambda k, t: torch.equal(w[k], t.contiguous())
    assert eq("conv0_w", sd["feature_extractor.conv_layers.0.0.weight"].reshape(C, a.conv_kernels[0]))
    ln_mode = a.extractor_mode == "layer_norm"
    for i in range(1, len(a.conv_kernels)):
        cw = sd[f"feature_extractor.conv_layers.{i}.0.weight"]
        k = a.conv_kernels[i]
        wk = w[f"conv{i}_w"].view(C, k, C)                        # [co][tap][ci]: the K order of a channels-last window
        for j in range(k):
            assert torch.equal(wk[:, j, :], bf(cw[:, :, j])), (i, j)
        if a.conv_bias:
            assert eq(f"conv{i}_bias", sd[f"feature_extractor.conv_layers.{i}.0.bias"])
        else:
            assert w[f"conv{i}_bias"] is None
        if ln_mode:
            assert eq(f"conv{i}_ln_g", sd[f"feature_extractor.conv_layers.{i}.2.1.weight"])
            assert eq(f"conv{i}_ln_b", sd[f"feature_extractor.conv_layers.{i}.2.1.bias"])
    assert eq("ln_feat_g", sd["layer_norm.weight"]) and eq("ln_feat_b", sd["layer_norm.bias"])
    assert eq("proj_w", bf(sd["post_extract_proj.weight"])) and eq("proj_b", sd["post_extract_proj.bias"])
    assert eq("pos_b", sd["encoder.pos_conv.0.bias"])
    assert eq("ln_enc_g", sd["encoder.layer_norm.weight"]) and eq("ln_enc_b", sd["encoder.layer_norm.bias"])
    D = a.embed_dim
    for i in range(a.layers):
        p = f"encoder.layers.{i}."
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
            assert torch.equal(w[f"l{i}_qkv_w"][j * D: (j + 1) * D], bf(sd[p + f"self_attn.{n}.weight"])), n
            assert torch.equal(w[f"l{i}_qkv_b"][j * D: (j + 1) * D], sd[p + f"self_attn.{n}.bias"]), n
        assert w[f"l{i}_qkv_w"].shape == (3 * D, D) and w[f"l{i}_qkv_b"].shape == (3 * D,)
        assert eq(f"l{i}_o_w", bf(sd[p + "self_attn.out_proj.weight"])) and eq(f"l{i}_o_b", sd[p + "self_attn.out_proj.bias"])
        assert eq(f"l{i}_fc1_w", bf(sd[p + "fc1.weight"])) and eq(f"l{i}_fc1_b", sd[p + "fc1.bias"])
        assert eq(f"l{i}_fc2_w", bf(sd[p + "fc2.weight"])) and eq(f"l{i}_fc2_b", sd[p + "fc2.bias"])
        assert eq(f"l{i}_ln1_g", sd[p + "self_attn_layer_norm.weight"]) and eq(f"l{i}_ln1_b", sd[p + "self_attn_layer_norm.bias"])
        assert eq(f"l{i}_ln2_g", sd[p + "final_layer_norm.weight"]) and eq(f"l{i}_ln2_b", sd[p + "final_layer_norm.bias"])
    # a plain pos_conv weight: [D, Dg, K] -> [g][co][tap][ci]
    G, Kp = a.pos_conv_groups, a.pos_conv_kernel
    Dg = D // G
    unpack = lambda t: t.view(G, Dg, Kp, Dg).permute(0, 1, 3, 2).reshape(D, Dg, Kp)
    assert torch.equal(unpack(w["pos_w"]), bf(sd["encoder.pos_conv.0.weight"]))
    # the checkpoint form: weight_g / weight_v through weight_norm(dim = 2)
    g = torch.Generator().manual_seed(3)
    sdn = {k: v for k, v in sd.items() if k != "encoder.pos_conv.0.weight"}
    sdn["encoder.pos_conv.0.weight_v"] = v = sd["encoder.pos_conv.0.weight"].clone()
    sdn["encoder.pos_conv.0.weight_g"] = gg = v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt() * (1.0 + 0.1 * torch.randn(1, 1, Kp, generator=g))
    load(sdn)
    got = unpack(pos_w())
    load(sd)
    v64, g64 = v.double(), gg.double()
    want = g64 * v64 / v64.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
    wb = want.to(torch.bfloat16)
    diff = got != wb
    ulp = want.abs().clamp_min(2.0 ** -126).log2().floor().exp2() * 2.0 ** -7                  # bf16 spacing at the fp64 value
    off = (got.double() - wb.double()).abs() / ulp
    assert float(off.max()) <= 1.0, "a pos_conv weight more than one bf16 ulp off the rounded fp64 value"
    return int(diff.sum()), diff.numel(), float(off.max())


# ---------------------------------------------------------------------------------------------------------------- invariants
def _same_run(a, b, tag, valid_only):
    lay = a.lay
    dev = a.hidden.device
    m = lay.mask(lay.valid, dev) if valid_only else torch.ones(lay.M, dtype=torch.bool, device=dev)
    for n in range(a.hidden.shape[0]):
        assert torch.equal(a.hidden[n], b.hidden[n]), (tag, "hidden", n)
    D = a.hidden.shape[2]
    for k in ("qk", "ctx", "x1", "ffn", "pre"):
        assert torch.equal(a.scratch[k][m], b.scratch[k][m]), (tag, k)
    assert torch.equal(_vt_rows(a.scratch["vt"], lay, D)[m], _vt_rows(b.scratch["vt"], lay, D)[m]), (tag, "vt")


@pytest.mark.parametrize("case", ["base_small", "large_small", "base_train", "base_wide"])
def test_layer_driver_equals_op_by_op(rigs, case):
    """ops.hubert_layer_fwd (one C-ABI call per layer, the default) against the op-by-op path: every hidden state and the scratch the
    driver leaves in the plan, bit for bit; uniform and segment layout, eval and train mode (same seeds)"""
    rig = rigs(case)
    for layout in (("flat",) if case == "base_wide" else ("uniform", "segment", "flat")):
        ops_run = rig.run(layout, per_op=True)
        assert "hubert_layer_fwd" not in [c.name for c in ops_run.calls]
        drv_run = rig.run(layout, per_op=False)
        assert [c.name for c in drv_run.calls].count("hubert_layer_fwd") == rig.arch.layers
        if CASES[case][2]:
            assert drv_run.calls[-1].a[13] == 0.1 and drv_run.calls[-1].a[14] == 0.1       # p_att, p_res live
            assert float((ops_run.hidden[0] == 0).float().mean()) > 0.05                     # the encoder dropout acted
        _same_run(ops_run, drv_run, f"{case}/{layout}", valid_only=True)


@pytest.mark.parametrize("case", ["base_small", "large_small"])
def test_repeatability(rigs, case):
    """two forwards of one batch: identical hidden states and scratch, every row, both layouts"""
    rig = rigs(case)
    for layout in ("uniform", "segment"):
        a = rig.run(layout, per_op=False, record=False)
        b = rig.run(layout, per_op=False, record=False)
        _same_run(a, b, f"{case}/{layout}", valid_only=False)


def _junk(buf, r0, lo, hi, g):
    if hi > lo:
        j = (torch.randint(0, 2, (hi - lo, buf.shape[1]), generator=g).float() * 2 - 1) * 1e4
        buf[r0 + lo: r0 + hi] = j.to(buf.dtype).to(buf.device)


@pytest.mark.parametrize("case", ["base_small", "large_small"])
def test_pad_rows_are_never_mixed_in(rigs, case):
    """Rows the kernels are told are padding get +-1e4 (finite); the recorded calls downstream are replayed on the plan's own buffers
    and every hidden state's valid rows must not change a bit: (1) frames >= valid of the layers' input, op by op and through the
    driver, (2) frames >= valid of the pos_conv input (its prep must mask them), (3) conv layer 0's rows past the receptive field of
    the valid frames."""
    rig = rigs(case)
    a = rig.arch
    g = torch.Generator().manual_seed(18)
    for layout in ("uniform", "segment"):
        for per_op in (True, False):
            run = rig.run(layout, per_op=per_op)
            pl, lay, calls = run.pl, run.lay, run.calls
            names = [c.name for c in calls]
            vm = lay.mask(lay.valid, rig.dev)
            i_pos = names.index("posconv_seg" if lay.seg else "posconv")
            i_layers = i_pos + (1 if a.layer_norm_first else 2)

            def replay(i0):
                for j in range(i0, len(calls)):
                    calls[j].replay()
                    if a.layer_norm_first and j == i_pos:
                        pl.hidden[0].copy_(pl.pre)
                torch.cuda.synchronize()

            def same(tag, first=0):
                for n in range(first, pl.hidden.shape[0]):
                    assert torch.equal(pl.hidden[n][vm], run.hidden[n][vm]), (case, layout, per_op, tag, n)

            replay(2)                                         # a plain replay reproduces the run
            assert torch.equal(pl.hidden, run.hidden)
            # (1) the layers' input
            for b in range(lay.B):
                _junk(pl.hidden[0], lay.r0[b], lay.valid[b], lay.pitch[b], g)
            replay(i_layers)
            same("layer input", first=1)
            # (2) the pos_conv input
            for b in range(lay.B):
                _junk(pl.x_proj, lay.r0[b], lay.valid[b], lay.pitch[b], g)
            replay(i_pos - 1)
            same("pos_conv input")
            # (3) conv layer 0's rows behind the valid frames' receptive field
            for b in range(lay.B):
                n = lay.valid[b]
                for i in range(len(a.conv_kernels) - 1, 0, -1):
                    n = (n - 1) * a.conv_strides[i] + a.conv_kernels[i]
                assert n < 64 * lay.pitch[b]
                _junk(pl.conv[0], 64 * lay.r0[b], n, 64 * lay.pitch[b], g)
            replay(2)
            same("conv rows")


def test_tile_families_agree_beyond_256_tiles(rigs):
    """wide case, recorded fc1 / QKV / out_proj operands: tile = 1 (128 x 128), 7 (256 x 192), 8 (256 x 256) and the cost model's
    choice give identical bits with more than 256 output tiles in flight (fc1, QKV: several tiles per workgroup)"""
    from speechclip_plus_amd import ops
    rig = rigs("base_wide")
    run = rig.run("flat")
    lay = run.lay
    qkv = [c for c in run.calls if c.name == "gemm_raw" and c.kw.get("Ct") is not None][0]
    lin = [c for c in run.calls if c.name == "linear_bf16"]
    o_proj, fc1 = lin[1], lin[2]
    assert fc1.kw["act"] == 1 and o_proj.kw.get("residual") is not None
    assert ops.gemm_tile_name(lay.M, 3072, 768, -1, 1) == "256x256"
    D = qkv.a[8]
    for tile in (0, 1, 7, 8):
        for c in (fc1, o_proj):
            kw = {k: v for k, v in c.kw.items() if k != "out"}
            out = ops.linear_bf16(*c.a, tile=tile, **kw)
            assert torch.equal(out, c.pkw["out"]), (tile, c.kw.get("act"))
        qk, vt = torch.zeros_like(qkv.a[4]), torch.zeros_like(qkv.kw["Ct"])
        ops.gemm_raw(*qkv.a[:4], qk, *qkv.a[5:], **dict(qkv.kw, Ct=vt, tile=tile))
        assert torch.equal(qk, qkv.pa[4]), tile
        assert torch.equal(_vt_rows(vt, lay, D), _vt_rows(qkv.pkw["Ct"], lay, D)), tile
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _rejected(tag, got, ref, bound):
    ok, ratio, e = _passes(got, ref, bound)
    print(f"[frozen-fwd] sensitivity {tag:62s} error / bound {ratio:8.3g}")
    assert not ok and ratio > 1.0, f"{tag}: not rejected (error / bound {ratio:.3g})"


def test_each_criterion_rejects_a_one_row_error(rigs):
    """The perturbations are applied on the host to the kernel's own result; the element-wise criterion alone (no rel-L2) must fail."""
    # ---- GEMM criterion, wide case: fc1 row 256 replaced by its neighbour across the 256-row tile boundary
    rig = rigs("base_wide")
    run = rig.run("flat")
    lin = [c for c in run.calls if c.name == "linear_bf16"]
    fc1 = lin[2]
    assert fc1.kw["act"] == 1
    ref, bound = _gemm_ref(fc1.a[0][:512], fc1.a[1], fc1.a[2], act=1)
    good = fc1.pkw["out"][:512]
    assert _passes(good, ref, bound)[0]
    bad = good.clone()
    bad[256] = good[255]
    _rejected("fc1 (wide): row 256 <- row 255", bad, ref, bound)
    # ---- one k-block of 64 missing from one output element (out_proj, wide): each of row 300's 768 elements on its own - the
    #      criterion has to resolve a TYPICAL element (the median), not the most favourable one; element (300, 401) is reported too
    c = lin[1]
    x, w = c.a[0][:512], c.a[1]
    ref, bound = _gemm_ref(x, w, c.a[2], res=c.kw["residual"][:512])
    good = c.pkw["out"][:512].double()
    assert _passes(good, ref, bound)[0]
    part = x[300, 128:192].double() @ w[:, 128:192].double().t()
    ratios = ((good[300] - part - ref[300]).abs() / (bound[300] + FTZ))
    med, share = float(ratios.median()), float((ratios > 1.0).double().mean())
    print(f"[frozen-fwd] sensitivity out_proj (wide): k-block 128..191 missing from ONE element of row 300: error / bound median "
          f"{med:.3g}, min {float(ratios.min()):.3g}, max {float(ratios.max()):.3g}, element 401 {float(ratios[401]):.3g}; "
          f"rejected on its own: {share:.3f} of the 768 elements")
    assert med > 1.0, f"a k-block missing from a typical element is not rejected (median error / bound {med:.3g})"
    # ---- one 8-column chunk on the N tail of the 192-wide tile.  No product launch of the cases above puts an N tail through the
    #      256-row kernel (base widths are multiples of 192 and 256; the large small case, M = 368, runs on the 64- / 128-row tiles),
    #      so the large out_proj operands (N = 1024 = 5 x 192 + 64, M = 368 = 256 + 112: N and M tails) are launched here with the
    #      256 x 192 tile forced, checked against fp64 with the stage's own criterion, and then perturbed
    from speechclip_plus_amd import ops
    rig = rigs("large_small")
    run = rig.run("segment")
    lay = run.lay
    lin = [c for c in run.calls if c.name == "linear_bf16"]
    c = lin[1]
    assert c.a[1].shape[0] == 1024 and c.kw.get("residual") is not None
    ref, bound = _gemm_ref(c.a[0], c.a[1], c.a[2], res=c.kw["residual"])
    good = ops.linear_bf16(c.a[0], c.a[1], c.a[2], residual=c.kw["residual"], tile=7)
    torch.cuda.synchronize()
    rep = _Report("large_small/tile 7")
    try:
        rep.check("out_proj + residual, 256 x 192 tile", good, ref, bound, BF16_RELL2)
    finally:
        rep.show()
    bad = good.clone()
    bad[100, 1016:1024] = good[100, 1008:1016]
    _rejected("out_proj (large, 256 x 192 tile): columns 1016..1023 <- 1008..1015 of one row", bad, ref, bound)
    # ---- attention: one key removed from one query's softmax - the last valid key, then key 0
    c = [c for c in run.calls if c.name == "attn_fwd"][0]
    b = 2                                                   # 127 valid frames
    r0, P, nv = lay.r0[b], lay.pitch[b], lay.valid[b]
    ref, bound = _attn_ref(c, lay, b)
    good = c.pa[3][r0: r0 + P].double()
    assert _passes(good, ref, bound)[0]
    for key in (nv - 1, 0):
        q = 40
        without = _attn_ref(c, lay, b, drop_query=(q, key))[0]
        bad = good.clone()
        bad[q] += without[q] - ref[q]
        _rejected(f"attention (large): key {key} missing from query {q}", bad, ref, bound)
    # ---- LayerNorm: one element off by 2 bf16 ulps
    c = [c for c in run.calls if c.name == "layernorm_bf16"][-1]
    ref, bound = _ln_ref(c.a[0], c.a[1], c.a[2], c.kw.get("act", 0))
    good = c.pkw["out"]
    assert _passes(good, ref, bound)[0]
    col = int(ref[10].abs().argmax())
    bad = good.clone()
    bits = bad.view(torch.int16)
    bits[10, col] += 2
    _rejected("LayerNorm (large): one element + 2 bf16 ulps", bad, ref, bound)
