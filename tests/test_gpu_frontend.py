"""GPU: the waveform front end (csrc/frontend.hip) entry point by entry point through ``ops.*``, against a float64 torch-CPU
restatement of the same operation: conv1d(stride 5) -> group_norm / layer_norm -> exact erf-GELU forward, torch.autograd backward.

Every forward batch mixes four signal kinds - noise, a quiet signal on a DC offset (1e-3 noise + 0.7: the cancellation case of the
Gram-matrix and closed-form statistics), silence, a loud utterance (amplitude ~30) - and the lengths where addressing goes wrong:
shorter than one conv window (no frame), exactly one window, len % 5 != 0, len == L, segments whose conv-0 row count is not a multiple
of the 128-row workgroup, batch size 1.  Samples of the caller's batch outside [off_b, off_b + len_b) hold large values: every kernel
that reads the caller's batch in place must mask them.

Backward bounds: derived in docs/parity.md ("conv layer 0 backward"), fixed before the first run; ``_bwd_bounds_*`` state them."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C = 512
EPS = 1e-5
U = 2.0 ** -24                 # fp32 unit roundoff
EPS_GELU_GRAD = 4e-6           # |gelu_grad_as - gelu'|: docs/parity.md
KINDS = ("noise", "dc", "silence", "loud")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _ops():
    from speechclip_plus_amd import ops
    return ops


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _signal(kind, n, g):
    x = torch.randn(n, generator=g)
    if kind == "dc":
        return x * 1e-3 + 0.7
    if kind == "silence":
        return torch.zeros(n)
    if kind == "loud":
        return x * 30.0
    return x


def _weights(seed, gamma_edges=False):
    g = torch.Generator().manual_seed(seed)
    w0 = torch.randn(C, 10, generator=g) * 0.3
    bias = torch.randn(C, generator=g) * 0.1
    gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    if gamma_edges:
        gam[::16] = 0.0                                                  # exact zeros
        gam[3::16] = 1e-3 * torch.sign(torch.randn(C // 16, generator=g))      # |gamma| << |beta|
        bet[3::16] = 0.5 * torch.sign(torch.randn(C // 16, generator=g))
        bet[::16] = 0.5
    return w0, bias, gam, bet


def _caller_batch(kinds, lens, L, offs, seed):
    """the caller's [B, W] batch: utterance b at [off_b, off_b + len_b), large values everywhere else (must never be read as samples)"""
    g = torch.Generator().manual_seed(seed)
    W = L + max(offs)
    wav = 50.0 + 10.0 * torch.randn(len(lens), W, generator=g)
    utt = []
    for b, (k, n, o) in enumerate(zip(kinds, lens, offs)):
        x = _signal(k, n, g)
        wav[b, o: o + n] = x
        utt.append(x)
    return wav, utt


def _frames(n):
    return max(0, (n - 10) // 5 + 1)


def _pitch(n, spr):
    return max(8, (n // spr + 2 + 7) // 8 * 8)


# lens / kinds: len < 10, exactly 10, len % 5 != 0, len == L; spr = 25 -> 5 conv-0 rows per segment row, segment row counts 40 .. 520
# (none a multiple of 128)
FWD_CASES = [
    ("mixed", list(KINDS) + ["noise", "dc", "loud"], [2400, 1203, 611, 2400, 7, 10, 1999], 25),
    ("kinds_at_L", list(KINDS), [3001, 3001, 3001, 3001], 35),
    ("batch1", ["noise"], [1237], 25),
]


def _segments(lens, spr, dev):
    ops = _ops()
    pitch = [_pitch(n, spr) for n in lens]
    return ops.RowSegments(pitch, [max(1, _frames(n)) for n in lens], dev), pitch


# ------------------------------------------------------------------------------------------------ 1: wav_prep_seg
@pytest.mark.parametrize("crop", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_wav_prep_seg_against_fp64(dev, case, normalize, crop):
    """each utterance's samples = the fp64 layer_norm over its own len (normalize) or the input bit for bit; silence normalises to
    exact zeros; every sample from len to the end of the utterance's segment is 0; nothing behind the last segment is written.
    Element bound of the normalised samples: (x - mean) rstd in fp32 with mean, rstd rounded once from fp64:
    4 u (rstd (|x| + |mean|) + |out|)."""
    ops = _ops()
    name, kinds, lens, spr = case
    L = max(lens)
    offs = [(37 * b + 5) % 23 for b in range(len(lens))] if crop else [0] * len(lens)
    wav, utt = _caller_batch(kinds, lens, L, offs, seed=11)
    seg, pitch = _segments(lens, spr, dev)
    sentinel = 1234.5
    flat = torch.full((spr * seg.rows + 16,), sentinel, device=dev)
    off_d = torch.tensor(offs, dtype=torch.int64, device=dev) if crop else None
    ops.wav_prep_seg(wav.to(dev), torch.tensor(lens, device=dev), flat, seg, spr, normalize, L=L, wav_off=off_d)
    got = flat.cpu()
    assert bool((got[spr * seg.rows:] == sentinel).all())
    for b, n in enumerate(lens):
        s0 = spr * seg.row0_host[b]
        o = got[s0: s0 + spr * pitch[b]]
        assert float(o[n:].abs().max()) == 0.0, b
        x = utt[b]
        if not normalize:
            assert torch.equal(o[:n], x), b
        elif kinds[b] == "silence":
            assert float(o[:n].abs().max()) == 0.0
        else:
            xd = x.double()
            ref = F.layer_norm(xd, (n,), eps=EPS)
            mean, rstd = xd.mean(), 1.0 / math.sqrt(float(xd.var(unbiased=False)) + EPS)
            bound = 4 * U * (rstd * (xd.abs() + abs(float(mean))) + ref.abs())
            err = (o[:n].double() - ref).abs()
            assert bool((err <= bound).all()), (name, b, float((err / bound).max()))


# ------------------------------------------------------------------------------------------------ forward references
def _ref_groupnorm(wav_pad64, T0, w0, gam, bet):
    y = F.conv1d(wav_pad64[:, None, : 5 * (T0 - 1) + 10], w0.double()[:, None], stride=5)
    return F.gelu(F.group_norm(y, C, gam.double(), bet.double(), EPS)).transpose(1, 2)        # (B, T0, C)


def _ref_layernorm(x64, w0, bias, gam, bet):
    """x64 [B, n] -> (B, T, C)"""
    y = F.conv1d(x64[:, None], w0.double()[:, None], None if bias is None else bias.double(), stride=5).transpose(1, 2)
    return F.gelu(F.layer_norm(y, (C,), gam.double(), bet.double(), EPS))


def _padded(utt, lens, width):
    wp = torch.zeros(len(lens), width)
    for b, (x, n) in enumerate(zip(utt, lens)):
        wp[b, :n] = x
    return wp


# ------------------------------------------------------------------------------------------------ 2: conv0_groupnorm_gelu_seg
@pytest.mark.parametrize("crop", [False, True])
@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_conv0_groupnorm_gelu_seg_against_fp64_and_uniform(dev, case, crop):
    """GroupNorm statistics over the batch's padded T0 on the zero-padded waveform (the caller's batch masked by wav_len / wav_off):
    rel-L2 < 5e-3 per utterance on its valid frames against fp64 (one bf16 store, test_frontend_conv0's bound), and bit-identical to
    the uniform-row launch (sc_conv0_gn_gelu without seg) on every frame whose window lies inside the utterance's segment."""
    ops = _ops()
    name, kinds, lens, spr = case
    L = max(lens)
    T0 = _frames(L)
    offs = [(53 * b + 3) % 31 for b in range(len(lens))] if crop else [0] * len(lens)
    wav, utt = _caller_batch(kinds, lens, L, offs, seed=12)
    w0, _, gam, bet = _weights(21)
    seg, pitch = _segments(lens, spr, dev)
    flat = torch.zeros(spr * seg.rows + 16, device=dev)
    lens_d = torch.tensor(lens, device=dev)
    off_d = torch.tensor(offs, dtype=torch.int64, device=dev) if crop else None
    ops.wav_prep_seg(wav.to(dev), lens_d, flat, seg, spr, False, L=L, wav_off=off_d)
    out = torch.full((seg.rows * spr // 5, C), float("nan"), device=dev, dtype=torch.bfloat16)
    wd = w0.to(dev), gam.to(dev), bet.to(dev)
    ops.conv0_groupnorm_gelu_seg(wav.to(dev) if crop else wav[:, :L].contiguous().to(dev), lens_d, flat, seg, spr, wd[0], wd[1], wd[2], T0,
                                 out, wav_off=off_d)
    # uniform rows on the zero-padded batch
    R0 = max(pitch) * spr // 5
    wav_pad = _padded(utt, lens, 5 * R0 + 64)
    out_u = torch.zeros(len(lens) * R0, C, device=dev, dtype=torch.bfloat16)
    ops.conv0_groupnorm_gelu(wav_pad.to(dev), wd[0], wd[1], wd[2], T0, R0, out_u)
    ref = _ref_groupnorm(wav_pad.double(), T0, w0, gam, bet)
    got, got_u = out.float().cpu(), out_u.view(len(lens), R0, C).float().cpu()
    for b, n in enumerate(lens):
        rows = pitch[b] * spr // 5
        r0 = seg.row0_host[b] * spr // 5
        ob = got[r0: r0 + rows]
        assert bool(torch.isfinite(ob).all()), b
        inside = rows - 1                                    # the last row's window reaches 5 samples past the segment
        assert torch.equal(ob[:inside], got_u[b, :inside]), (name, b)
        nv = _frames(n)
        if nv:
            e = rel_l2(ob[:nv], ref[b, :nv])
            print(f"{name} b{b} {kinds[b]} len {n}: rel-L2 {e:.3e}")
            assert e < 5e-3, (name, b, kinds[b], e)


# ------------------------------------------------------------------------------------------------ 3: conv0_layernorm_gelu_seg
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_conv0_layernorm_gelu_seg_against_fp64_and_uniform(dev, case, with_bias):
    """closed form (sc_set_option(2, 0)) and two-pass (sc_set_option(2, 1)) on ragged rows, the waveform normalised by wav_prep_seg
    as the large model's forward does: per utterance on its valid frames rel-L2 < 5e-3 against fp64 and at most 1.05x the two-pass
    kernel's error, all values finite, the two kernels within one bf16 ulp or 1e-6 of each other (the criteria of
    test_frontend_conv0_layer_norm_mode_closed_form_statistics), and each bit-identical to its uniform-row launch (sc_conv0_ln_gelu without seg)."""
    from speechclip_plus_amd._lib import lib
    ops = _ops()
    name, kinds, lens, spr = case
    L = max(lens)
    wav, utt = _caller_batch(kinds, lens, L, [0] * len(lens), seed=13)
    w0, bias, gam, bet = _weights(22)
    if not with_bias:
        bias = None
    seg, pitch = _segments(lens, spr, dev)
    flat = torch.zeros(spr * seg.rows + 16, device=dev)
    ops.wav_prep_seg(wav.to(dev), torch.tensor(lens, device=dev), flat, seg, spr, True, L=L)
    flat_h = flat.cpu()
    R0 = max(pitch) * spr // 5
    wav_pad = torch.zeros(len(lens), 5 * R0 + 64)
    for b in range(len(lens)):
        s0 = spr * seg.row0_host[b]
        wav_pad[b, : spr * pitch[b]] = flat_h[s0: s0 + spr * pitch[b]]
    wd = [t.to(dev) if t is not None else None for t in (w0, bias, gam, bet)]
    outs, outs_u = {}, {}
    for opt in (0, 1):
        lib().sc_set_option(2, opt)
        try:
            out = torch.full((seg.rows * spr // 5, C), float("nan"), device=dev, dtype=torch.bfloat16)
            ops.conv0_layernorm_gelu_seg(flat, seg, spr, *wd, out)
            out_u = torch.zeros(len(lens) * R0, C, device=dev, dtype=torch.bfloat16)
            ops.conv0_layernorm_gelu(wav_pad.to(dev), *wd, R0, out_u)
            outs[opt], outs_u[opt] = out.float().cpu(), out_u.view(len(lens), R0, C).float().cpu()
        finally:
            lib().sc_set_option(2, 0)
    for b, n in enumerate(lens):
        rows = pitch[b] * spr // 5
        r0 = seg.row0_host[b] * spr // 5
        ob = {o: outs[o][r0: r0 + rows] for o in (0, 1)}
        for o in (0, 1):
            assert bool(torch.isfinite(ob[o]).all()), (b, o)
            assert torch.equal(ob[o][: rows - 1], outs_u[o][b, : rows - 1]), (name, b, o)
        ulp = torch.maximum(ob[0].abs(), ob[1].abs()).clamp_min(2.0 ** -126).log2().floor().exp2() * 2.0 ** -7
        assert bool(((ob[0] - ob[1]).abs() <= torch.clamp(ulp, min=1e-6)).all()), (name, b)
        nv = _frames(n)
        if nv:
            ref = _ref_layernorm(flat_h[spr * seg.row0_host[b]:][: 5 * (nv - 1) + 10].double()[None], w0, bias, gam, bet)[0]
            e_new, e_old = rel_l2(ob[0][:nv], ref), rel_l2(ob[1][:nv], ref)
            print(f"{name} b{b} {kinds[b]} len {n}: closed form {e_new:.3e}, two-pass {e_old:.3e}")
            assert e_new < 5e-3 and e_new <= 1.05 * e_old + 1e-6, (name, b, kinds[b], e_new, e_old)


# ------------------------------------------------------------------------------------------------ 4: the fp32-output forms
U64 = 2.0 ** -53
GELU_SLOPE = 1.13              # max |gelu'| = 1.1290 (at x = sqrt 2): |gelu(n + dn) - gelu(n)| <= 1.13 |dn|, no higher-order term
SECOND_ORDER = 1.001           # products of two error terms: every relative term here is < 1e-4


def _gelu_erf_form_error(n):
    """|gelu_erf(n) - gelu(n)| for an exact fp32 argument n (csrc/sc_common.h; docs/parity.md): gelu = (h + |h|) - |h| erfc(|z|), h = n / 2;
    A&S 7.1.28 bounds erfc by 3e-7 absolute, its fp32 evaluation (6 Horner roundings x 16, four squarings x (8 + 4 + 2 + 1), rcp) by
    112 u relative, the rounding of z = |n| / sqrt 2 moves erfc by < u; the closing fma rounds once"""
    return 0.5 * n.abs() * (3e-7 + 112 * U * torch.erfc(n.abs() / math.sqrt(2.0)) + U) + U * F.gelu(n).abs()


def _f32_bound_groupnorm(x64, T0, w0, gam, bet):
    """(reference (B, T0, C), element bound) of conv0_groupnorm_gelu(out_f32=True); docs/parity.md, "conv layer 0, fp32 outputs"."""
    X = _windows(x64, T0)                                                  # [B, T, 10]
    w, g, be = w0.double(), gam.double()[None, :, None], bet.double()[None, :, None]
    y = torch.einsum("btj,cj->bct", X, w)
    absWX = torch.einsum("btj,cj->bct", X.abs(), w.abs())
    mu = y.mean(-1, keepdim=True)
    var = y.var(-1, unbiased=False, keepdim=True)
    rs = 1.0 / torch.sqrt(var + EPS)
    sc, sh = g * rs, be - mu * g * rs
    n = y * sc + sh
    # fp64 Gram statistics: at most T0 + 100 roundings on the way to scale / shift, charged on the sums of absolute values; the same
    # again for the fp64 reference's own statistics
    e64 = 2 * (T0 + 100) * U64
    d_mu = e64 * absWX.mean(-1, keepdim=True)
    d_var = e64 * ((absWX * absWX).mean(-1, keepdim=True) + 2 * mu.abs() * absWX.mean(-1, keepdim=True))
    d_rs = 0.5 * d_var / (var + EPS) + 4 * U64                             # relative
    d_sc = sc.abs() * (d_rs + U)                                           # rounded to fp32 once
    d_sh = sc.abs() * d_mu + (mu * sc).abs() * d_rs + U * sh.abs()
    d_y = 10 * U * absWX                                                   # the 10-FMA chain
    d_n = sc.abs() * d_y + y.abs() * d_sc + d_sh + U * n.abs()             # n = fma(y, sc, sh)
    bound = SECOND_ORDER * (GELU_SLOPE * d_n + _gelu_erf_form_error(n))
    return F.gelu(n).transpose(1, 2), bound.transpose(1, 2)


def _f32_bound_layernorm(x64, T0, w0, bias, gam, bet):
    """(reference (B, T0, C), element bound) of conv0_layernorm_gelu(out_f32=True): the two-pass kernel, statistics in fp32."""
    X = _windows(x64, T0)
    w, ga, be = w0.double(), gam.double(), bet.double()
    b0 = torch.zeros(C, dtype=torch.float64) if bias is None else bias.double()
    y = torch.einsum("btj,cj->btc", X, w) + b0
    d_y = 10 * U * (torch.einsum("btj,cj->btc", X.abs(), w.abs()) + b0.abs())          # the chain starts at the bias: 10 roundings
    m = y.mean(-1, keepdim=True)
    a = y - m
    var = (a * a).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = a * rstd
    n = ga * xh + be
    d_m = d_y.mean(-1, keepdim=True) + 14 * U * y.abs().mean(-1, keepdim=True)            # 8 serial adds + a 6-level wave tree
    d_a = d_y + d_m + U * a.abs()
    d_var = 2 * (a.abs() * d_a).mean(-1, keepdim=True) + 16 * U * var                       # squares, 8 adds, the tree, + eps
    d_rs = 0.5 * d_var / (var + EPS) + 2 * U                                                # relative; rsqrtf: 1 ulp
    d_xh = rstd * d_a + xh.abs() * (d_rs + U)
    d_n = ga.abs() * (d_xh + U * xh.abs()) + U * n.abs()
    bound = SECOND_ORDER * (GELU_SLOPE * d_n + _gelu_erf_form_error(n))
    return F.gelu(n), bound


@pytest.mark.parametrize("form", ["groupnorm", "layernorm", "layernorm_nobias"])
def test_conv0_fp32_outputs_against_fp64(dev, form):
    """out_f32=True of the two uniform conv-0 wrappers (the fp32 debug mode's kernels: same taps and affine, the 3e-7 erf-GELU form,
    unrounded stores) against fp64, every element within its derived bound (docs/parity.md, "conv layer 0, fp32 outputs").  B = 2 (noise,
    DC offset), T0 = R0 = 131: a full 128-row workgroup plus a 3-row one whose last wave iteration (4 rows, 2 in the LayerNorm kernel)
    is partial.  The flag does not leak: the bf16 call before and after the fp32 one give the same bits, out_f32=False or left out."""
    ops = _ops()
    T0 = R0 = 131
    kinds = ["noise", "dc"]
    B = len(kinds)
    g = torch.Generator().manual_seed(41)
    L = 5 * (T0 - 1) + 10
    wav = torch.zeros(B, L + 6)
    for b, k in enumerate(kinds):
        wav[b, :L] = _signal(k, L, g)
    w0, bias, gam, bet = _weights(23)
    if form == "layernorm_nobias":
        bias = None
    wd = wav.to(dev)
    if form == "groupnorm":
        td = [t.to(dev) for t in (w0, gam, bet)]
        run = lambda out, **kw: ops.conv0_groupnorm_gelu(wd, *td, T0, R0, out, **kw)
        ref, bound = _f32_bound_groupnorm(wav.double(), T0, w0, gam, bet)
        assert rel_l2(ref, _ref_groupnorm(wav.double(), T0, w0, gam, bet)) < 1e-9     # the bound's restatement is the file's reference
    else:
        td = [t.to(dev) if t is not None else None for t in (w0, bias, gam, bet)]
        run = lambda out, **kw: ops.conv0_layernorm_gelu(wd, *td, R0, out, **kw)
        ref, bound = _f32_bound_layernorm(wav.double(), T0, w0, bias, gam, bet)
        assert rel_l2(ref, _ref_layernorm(wav.double()[:, :L], w0, bias, gam, bet)) < 1e-12
    bf = [torch.full((B * R0, C), float("nan"), device=dev, dtype=torch.bfloat16) for _ in range(2)]
    out = torch.full((B * R0, C), float("nan"), device=dev, dtype=torch.float32)
    saved0 = run(bf[0])
    saved = run(out, out_f32=True)
    saved1 = run(bf[1], out_f32=False)
    assert torch.equal(bf[0].view(torch.int16), bf[1].view(torch.int16)) and bool(torch.isfinite(bf[0].float()).all())
    if form == "groupnorm":
        live = lambda s: (s[0], s[1], s[2].view(B, s[3], 66)[..., :65])          # scale, shift, the 65 written sums per chunk (66th: pad)
        for a_, b_, c_ in zip(live(saved0), live(saved), live(saved1)):
            assert torch.equal(a_, b_) and torch.equal(a_, c_)
    got = out.view(B, R0, C).cpu()
    assert bool(torch.isfinite(got).all())
    err = (got.double() - ref).abs()
    ratio = float((err / bound).max())
    print(f"{form}: max err / bound {ratio:.3e}, rel-L2 {rel_l2(got, ref):.3e}, largest bound {float(bound.max()):.3e}")
    assert bool((err <= bound).all()), (form, ratio)
    # one bf16 rounding of the fp32 result away from the bf16 path (whose GELU is the five-term fit, |error| <= 3.1e-6)
    assert rel_l2(bf[0].view(B, R0, C).float().cpu(), got) < 5e-3


# ------------------------------------------------------------------------------------------------ backward
def _gelu_d(n):
    """(gelu'(n), gelu''(n)) in fp64"""
    phi = torch.exp(-0.5 * n * n) / math.sqrt(2 * math.pi)
    return 0.5 * torch.erfc(-n / math.sqrt(2.0)) + n * phi, phi * (2.0 - n * n)


def _windows(x64, T0):
    """x64 [B, >= 5 (T0 - 1) + 10] -> X [B, T0, 10], X[b, t, j] = x[b, 5 t + j]"""
    return x64[:, : 5 * (T0 - 1) + 10].unfold(1, 10, 5)


def _bwd_bounds_groupnorm(x64, T0, w0, gam, bet, dy64, rpw):
    """element bounds of (dW0, dgamma, dbeta) for sc_conv0_gn_bwd; docs/parity.md, "conv layer 0 backward (GroupNorm)"."""
    B = x64.shape[0]
    X = _windows(x64, T0)                                                  # [B, T, 10]
    w, g, be = w0.double(), gam.double()[None, :, None], bet.double()[None, :, None]
    u = torch.einsum("btj,cj->bct", X, w)
    absWX = torch.einsum("btj,cj->bct", X.abs(), w.abs())
    mu = u.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(u.var(-1, unbiased=False, keepdim=True) + EPS)
    a = u - mu
    n = g * a * rs + be
    gp, gpp = _gelu_d(n)
    sc, sh = g * rs, be - mu * g * rs
    dy = dy64.transpose(1, 2)                                              # [B, C, T]
    dn = dy * gp
    dlt_n = U * (sc.abs() * (10 * absWX + u.abs()) + sh.abs() + n.abs())
    e_dn = dy.abs() * (gpp.abs() * dlt_n + EPS_GELU_GRAD) + U * dn.abs()
    dlt_a = U * (10 * absWX + mu.abs() + a.abs())                          # (u - mu) in fp32
    acc = U * (rpw + 2)
    A1, D = dn.sum(-1), (dn * a).sum(-1)                                   # [B, C]
    E_A1 = e_dn.sum(-1) + acc * dn.abs().sum(-1)
    E_D = (e_dn * a.abs() + dn.abs() * dlt_a).sum(-1) + acc * (dn * a).abs().sum(-1) + U * (dn * a).abs().sum(-1)
    V = torch.einsum("bct,btj->bcj", dn, X)
    E_V = torch.einsum("bct,btj->bcj", e_dn, X.abs()) + (acc + U) * torch.einsum("bct,btj->bcj", dn.abs(), X.abs())
    S = X.sum(1)[:, None, :]                                               # [B, 1, 10]
    K = torch.einsum("bct,btj->bcj", a, X)                                 # sum_t (u - mu) x_j = WG_j - mu S_j
    rs2, g2 = rs[..., 0], gam.double()[None, :]
    dW_b = g2[..., None] * rs2[..., None] * (V - A1[..., None] * S / T0 - D[..., None] * rs2[..., None] ** 2 * K / T0)
    E_dW = (g2.abs() * rs2)[..., None] * (E_V + (S.abs() / T0) * E_A1[..., None] + (rs2[..., None] ** 2) * (K.abs() / T0) * E_D[..., None]) \
        + U * dW_b.abs()
    E_dg = rs2 * E_D + U * (rs2 * D).abs()
    E_db = E_A1 + U * A1.abs()
    # fp32 column sum of the B per-utterance contributions
    E_dW = E_dW.sum(0) + U * B * dW_b.abs().sum(0)
    E_dg = E_dg.sum(0) + U * B * (rs2 * D).abs().sum(0)
    E_db = E_db.sum(0) + U * B * A1.abs().sum(0)
    return 2 * E_dW, 2 * E_dg, 2 * E_db


def _bwd_bounds_layernorm(x64, T0, w0, bias, gam, bet, dy64, rpw, nwc):
    """element bounds of (dW0, dbias, dgamma, dbeta) for sc_conv0_ln_bwd; docs/parity.md, "conv layer 0 backward (LayerNorm)"."""
    B = x64.shape[0]
    X = _windows(x64, T0)                                                  # [B, T, 10]
    w = w0.double()
    b0 = torch.zeros(C, dtype=torch.float64) if bias is None else bias.double()
    ga, be = gam.double(), bet.double()
    u = torch.einsum("btj,cj->btc", X, w) + b0
    Uc = torch.einsum("btj,cj->btc", X.abs(), w.abs()) + b0.abs()
    m = u.mean(-1, keepdim=True)
    a = u - m
    var = (a * a).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = a * rstd
    n = ga * xh + be
    gp, gpp = _gelu_d(n)
    dy = dy64                                                              # [B, T, C]
    dn = dy * gp
    d_u = U * 10 * Uc
    d_m = d_u.mean(-1, keepdim=True) + U * 14 * u.abs().mean(-1, keepdim=True)
    d_a = d_u + d_m + U * a.abs()
    d_var = 2 * (a.abs() * d_a).mean(-1, keepdim=True) + U * 16 * var
    d_rs = 0.5 * d_var / (var + EPS) + 2 * U                               # relative error of rstd
    d_xh = rstd * d_a + xh.abs() * (d_rs + U)
    d_n = ga.abs() * d_xh + U * n.abs()
    e_dn = dy.abs() * (gpp.abs() * d_n + EPS_GELU_GRAD) + U * dn.abs()
    g = dn * ga
    e_g = ga.abs() * e_dn + U * g.abs()
    m1, m2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    e_m1 = e_g.mean(-1, keepdim=True) + U * 14 * g.abs().mean(-1, keepdim=True)
    e_m2 = (e_g * xh.abs() + g.abs() * d_xh).mean(-1, keepdim=True) + U * 15 * (g * xh).abs().mean(-1, keepdim=True)
    du = rstd * (g - m1 - xh * m2)
    e_du = rstd * (e_g + e_m1 + xh.abs() * e_m2 + m2.abs() * d_xh) + du.abs() * d_rs + U * 4 * rstd * (g.abs() + m1.abs() + (xh * m2).abs())
    acc = U * (rpw + B * nwc + 2)                                          # fp32 rows of a wave chunk, then the fp32 column sum of B * nwc partials
    E_dg = (e_dn * xh.abs() + dn.abs() * d_xh).sum((0, 1)) + (acc + U) * (dn * xh).abs().sum((0, 1))
    E_db = e_dn.sum((0, 1)) + acc * dn.abs().sum((0, 1))
    E_dbias = e_du.sum((0, 1)) + acc * du.abs().sum((0, 1))
    E_dW = torch.einsum("btc,btj->cj", e_du, X.abs()) + (acc + U) * torch.einsum("btc,btj->cj", du.abs(), X.abs())
    return 2 * E_dW, 2 * E_dbias, 2 * E_dg, 2 * E_db


def _bwd_batch(kinds, T0, R0, seed):
    """zero-padded [B, ldw] batch whose utterances fill the T0 frames (the last one a few samples short), and bf16 dy [B * R0, C]"""
    g = torch.Generator().manual_seed(seed)
    L = 5 * (T0 - 1) + 10
    wav = torch.zeros(len(kinds), 5 * R0 + 64)
    for b, k in enumerate(kinds):
        n = L - (3 * b) % 5 if b else L
        wav[b, :n] = _signal(k, n, g)
    dy = torch.randn(len(kinds) * R0, C, generator=g).to(torch.bfloat16)
    return wav, dy


# (kinds, T0, R0): T0 == R0 not a multiple of nwc = 32 (rpw 7: the last three wave chunks own no row), T0 < R0, T0 < nwc, B = 1
BWD_SHAPES = [
    (list(KINDS), 203, 203),
    (["noise", "loud", "dc"], 150, 160),
    (["noise", "silence", "dc", "loud"], 7, 8),
    (["noise"], 1000, 1024),
]
NWC = 32


def _check_bwd(name, got, ref, bound, noise):
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all()), name
    ratio = float((err / bound.clamp_min(1e-300)).max())
    e = rel_l2(got, ref)
    print(f"{name}: max err / bound {ratio:.3e}, rel-L2 {e:.3e}")
    assert bool((err <= bound).all()), (name, ratio)
    if noise:
        assert e < 1e-4, (name, e)


def _groupnorm_bwd_run(dev, wav, dy, T0, R0, w0, gam, bet):
    ops = _ops()
    B = wav.shape[0]
    wd = wav.to(dev)
    W, G, Be = w0.to(dev), gam.to(dev), bet.to(dev)
    out = torch.empty(B * R0, C, device=dev, dtype=torch.bfloat16)
    saved = ops.conv0_groupnorm_gelu(wd, W, G, Be, T0, R0, out)
    return [t.clone().cpu() for t in ops.conv0_groupnorm_gelu_bwd(wd, W, G, Be, saved, dy.to(dev), T0, R0, nwc=NWC)]


def _groupnorm_autograd(wav, dy, T0, R0, w0, gam, bet):
    B = wav.shape[0]
    x64 = wav.double()
    W = w0.double().requires_grad_(True)
    G = gam.double().requires_grad_(True)
    Be = bet.double().requires_grad_(True)
    y = F.conv1d(x64[:, None, : 5 * (T0 - 1) + 10], W[:, None], stride=5)
    out = F.gelu(F.group_norm(y, C, G, Be, EPS))
    dy64 = dy.double().view(B, R0, C)[:, :T0]
    (out * dy64.transpose(1, 2)).sum().backward()
    return (W.grad, G.grad, Be.grad), x64, dy64


@pytest.mark.parametrize("shape", BWD_SHAPES, ids=[f"T0_{s[1]}_R0_{s[2]}_B{len(s[0])}" for s in BWD_SHAPES])
@pytest.mark.parametrize("gamma_edges", [False, True])
def test_conv0_groupnorm_gelu_bwd_against_fp64(dev, shape, gamma_edges):
    """dW0, dgamma, dbeta of sc_conv0_gn_bwd against fp64 autograd (same bf16 dy widened exactly, same fp32 weights): every element
    within its derived bound; rel-L2 < 1e-4 on a noise-only batch; rows T0 .. R0 of dy are not read (+-1e4 there changes no bit);
    two calls are bit-identical.  gamma_edges: channels with gamma == 0 exactly and with |gamma| = 1e-3 against |beta| = 0.5 (the
    former (sum dn n - beta sum dn) / gamma gave NaN / lost digits there) - same bounds, every value finite."""
    kinds, T0, R0 = shape
    w0, _, gam, bet = _weights(31, gamma_edges)
    wav, dy = _bwd_batch(kinds, T0, R0, seed=T0)
    dy_big = dy.view(len(kinds), R0, C).clone()
    if R0 > T0:
        dy_big[:, T0:] = (torch.randint(0, 2, (len(kinds), R0 - T0, C), generator=torch.Generator().manual_seed(1)) * 2 - 1) * 1e4
    dy_zero = dy.view(len(kinds), R0, C).clone()
    dy_zero[:, T0:] = 0
    got = _groupnorm_bwd_run(dev, wav, dy_big.view(-1, C), T0, R0, w0, gam, bet)
    again = _groupnorm_bwd_run(dev, wav, dy_big.view(-1, C), T0, R0, w0, gam, bet)
    zero = _groupnorm_bwd_run(dev, wav, dy_zero.view(-1, C), T0, R0, w0, gam, bet)
    for a, b, z in zip(got, again, zero):
        assert torch.equal(a, b) and torch.equal(a, z)
    ref, x64, dy64 = _groupnorm_autograd(wav, dy_zero.view(-1, C), T0, R0, w0, gam, bet)
    rpw = (T0 + NWC - 1) // NWC
    bounds = _bwd_bounds_groupnorm(x64, T0, w0, gam, bet, dy64, rpw)
    noise = set(kinds) == {"noise"}
    for nm, gv, rv, bd in zip(("dW0", "dgamma", "dbeta"), got, ref, bounds):
        _check_bwd(f"groupnorm {kinds} T0 {T0} R0 {R0} edges {gamma_edges} {nm}", gv, rv, bd, noise)
    if gamma_edges:
        assert float(got[0][::16].abs().max()) == 0.0                      # gamma == 0: dW0 is exactly 0 (the factor gamma / sigma)


@pytest.mark.parametrize("shape", BWD_SHAPES, ids=[f"T0_{s[1]}_R0_{s[2]}_B{len(s[0])}" for s in BWD_SHAPES])
@pytest.mark.parametrize("with_bias", [True, False])
def test_conv0_layernorm_gelu_bwd_against_fp64(dev, shape, with_bias):
    """dW0, dbias, dgamma, dbeta of sc_conv0_ln_bwd against fp64 autograd: every element within its derived bound; rel-L2 < 1e-4 on a
    noise-only batch; rows T0 .. R0 of dy are not read; two calls are bit-identical."""
    ops = _ops()
    kinds, T0, R0 = shape
    w0, bias, gam, bet = _weights(32)
    if not with_bias:
        bias = None
    wav, dy = _bwd_batch(kinds, T0, R0, seed=T0 + 1)
    B = len(kinds)
    dy_big = dy.view(B, R0, C).clone()
    if R0 > T0:
        dy_big[:, T0:] = (torch.randint(0, 2, (B, R0 - T0, C), generator=torch.Generator().manual_seed(2)) * 2 - 1) * 1e4
    dy_zero = dy.view(B, R0, C).clone()
    dy_zero[:, T0:] = 0
    wd = wav.to(dev)
    td = [t.to(dev) if t is not None else None for t in (w0, bias, gam, bet)]

    def run(d):
        return [t.clone().cpu() for t in ops.conv0_layernorm_gelu_bwd(wd, *td, d.reshape(-1, C).to(dev), T0, R0, nwc=NWC)]

    got, again, zero = run(dy_big), run(dy_big), run(dy_zero)
    for a, b, z in zip(got, again, zero):
        assert torch.equal(a, b) and torch.equal(a, z)
    x64 = wav.double()
    W = w0.double().requires_grad_(True)
    Bi = torch.zeros(C, dtype=torch.float64, requires_grad=True) if bias is None else bias.double().requires_grad_(True)
    G = gam.double().requires_grad_(True)
    Be = bet.double().requires_grad_(True)
    y = F.conv1d(x64[:, None, : 5 * (T0 - 1) + 10], W[:, None], Bi, stride=5).transpose(1, 2)
    out = F.gelu(F.layer_norm(y, (C,), G, Be, EPS))
    dy64 = dy_zero[:, :T0].double()
    (out * dy64).sum().backward()
    ref = (W.grad, Bi.grad, G.grad, Be.grad)
    rpw = (T0 + NWC - 1) // NWC
    bounds = _bwd_bounds_layernorm(x64, T0, w0, bias, gam, bet, dy64, rpw, NWC)
    noise = set(kinds) == {"noise"}
    for nm, gv, rv, bd in zip(("dW0", "dbias", "dgamma", "dbeta"), got, ref, bounds):
        _check_bwd(f"layernorm {kinds} T0 {T0} R0 {R0} bias {with_bias} {nm}", gv, rv, bd, noise)
