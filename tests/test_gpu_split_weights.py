"""GPU: the split-weight evaluation mode (docs/rounds/r09_split_weights.md): sc_gemm_bf16 with a_rep = 2 against float64 with the EXACT
fp32 weights, the tile families and the default path bit for bit, sc_hubert_layer_fwd(w_split = 1) against the per-op sequence, and
the small frozen encoder in eval mode with eval_weights = "split".

Bounds (fixed before the first GPU run).  A is bf16, W fp32; the kernel multiplies W_hi + W_lo with |W - W_hi - W_lo| <= 2^-17 |W|
(test_split_weights_cpu.py) and accumulates 2K exact bf16 x bf16 products in fp32, so for an fp32 output
    |err| <= (2^-17 + 2K 2^-24) sum_k |a| |w|
element by element, and the rms error is at most 1 / 64 of the rms error of the same launch with bf16(W) (the weight term falls by 2^8, 2^2
is left for the accumulation).  A bf16 output adds one bf16 rounding of the stored value, 2^-8 |y| (STORE of tests/test_gpu_trainable_bwd.py: the unit
roundoff of an 8-bit significand); the GELU (five-term fit, GELU_FIT from the
fp32 definition, slope <= GELU_LIP) is taken from tests/test_gpu_frozen_fwd.py."""
import math

import numpy as np
import pytest
import torch

import split_cases
from test_gpu_frozen_fwd import GELU_FIT, GELU_LIP
from test_gpu_model import LP_HIDDEN, rel_l2
from test_gpu_trainable_bwd import STORE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U_W, U_ACC = 2.0 ** -17, 2.0 ** -24
FAMILIES = (1, 2, 7, 8, 3, 13, 14, 15)
# (M, N, K, tap_c, lda): one logical / two physical tiles (prologue only); steady state of the double buffer; overlapping conv rows in the
# tap order; 12 and 48 logical tiles
SHAPES = [(264, 200, 64, 0, 64), (264, 200, 128, 0, 128), (520, 384, 192, 64, 128), (264, 200, 768, 0, 768), (64, 72, 3072, 0, 3072)]


def _ops():
    from speechclip_plus_amd import ops
    return ops


def _operands(M, N, K, lda, seed, batch=1):
    """A as the kernel reads it (rows of K elements every lda: they overlap when lda < K), W fp32 ~ N(0, 0.05^2)"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(batch, (M - 1) * lda + K, generator=g).to(torch.bfloat16)
    W = torch.randn(batch, N, K, generator=g) * 0.05
    A = torch.stack([buf[b].as_strided((M, K), (lda, 1)) for b in range(batch)])
    return buf.to(DEV), A.to(DEV), W.to(DEV)


def _launch(buf, M, N, K, lda, W, a_rep, tap_c=0, out_f32=True, tile=0, **kw):
    ops = _ops()
    C = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float32 if out_f32 else torch.bfloat16)
    ops.gemm_raw(buf, lda, W, W.shape[-1], C, N, M, N, K, out_f32=out_f32, tap_c=tap_c, tile=tile, a_rep=a_rep, **kw)
    return C


def _ref(A, W):
    """fp64 product and the magnitude sum the bounds scale with"""
    return A.double() @ W.double().t(), A.double().abs() @ W.double().abs().t()


@pytest.mark.parametrize("M,N,K,tap_c,lda", SHAPES)
def test_gemm_split_against_fp64(M, N, K, tap_c, lda):
    ops = _ops()
    buf, A, W = _operands(M, N, K, lda, seed=K + tap_c)
    buf, A, W = buf[0], A[0], W[0]
    ref, mag = _ref(A, W)
    bound = (U_W + 2 * K * U_ACC) * mag
    got = _launch(buf, M, N, K, lda, ops.split_weight_bf16(W), 2, tap_c)
    err = (got.double() - ref).abs()
    plain = _launch(buf, M, N, K, lda, W.to(torch.bfloat16).contiguous(), 0, tap_c)
    rms, rms_plain = err.pow(2).mean().sqrt().item(), (plain.double() - ref).pow(2).mean().sqrt().item()
    print(f"[split-gemm] {M}x{N}x{K} tap_c {tap_c}: max err/bound {(err / bound).max().item():.3g}, rms {rms:.3g} vs bf16(W) {rms_plain:.3g} "
          f"(ratio {rms_plain / rms:.0f})")
    assert bool((err <= bound).all()), f"largest err / bound {(err / bound).max().item():.3g}"
    assert rms <= rms_plain / 64, (rms, rms_plain)
    # bf16 output: the same accumulator behind one rounding
    got16 = _launch(buf, M, N, K, lda, ops.split_weight_bf16(W), 2, tap_c, out_f32=False)
    assert bool(((got16.double() - ref).abs() <= bound + STORE * (ref.abs() + bound)).all())   # the rounding acts on the computed value


def test_gemm_split_bias_gelu_residual():
    ops = _ops()
    M, N, K = 264, 200, 128
    buf, A, W = _operands(M, N, K, K, seed=11)
    buf, A, W = buf[0], A[0], W[0]
    g = torch.Generator().manual_seed(12)
    bias = (torch.randn(N, generator=g) * 0.1).to(DEV)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
    ref, mag = _ref(A, W)
    u = ref + bias.double()
    y = 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0))) + res.double()
    # fp32: bias add (the accumulator starts from it), the GELU's fit, the residual add; then the bf16 store
    pre = GELU_LIP * ((U_W + (2 * K + 1) * U_ACC) * (mag + bias.double().abs())) + GELU_FIT + 2 * U_ACC * y.abs()
    bound = pre + STORE * (y.abs() + pre)
    got = _launch(buf, M, N, K, K, ops.split_weight_bf16(W), 2, out_f32=False, bias=bias, act=1, residual=res, ldr=N)
    err = (got.double() - y).abs()
    assert bool((err <= bound).all()), f"largest err / bound {(err / bound).max().item():.3g}"


@pytest.mark.parametrize("layout", ["uniform", "segment"])
def test_gemm_split_transposed_store(layout):
    """the V^T store (columns >= n_split, per head, dh = 64): the same bits as the row-major store of the same launch without it"""
    ops = _ops()
    M, D, K = 264, 128, 128
    N = 3 * D
    buf, A, W = _operands(M, N, K, K, seed=21)
    Ws = ops.split_weight_bf16(W[0])
    plain = _launch(buf[0], M, N, K, K, Ws, 2, out_f32=False)
    C = torch.zeros(M, 2 * D, device=DEV, dtype=torch.bfloat16)
    vt = torch.zeros(M * D, device=DEV, dtype=torch.bfloat16)
    if layout == "uniform":
        R = 88                                                                # three utterances of 88 rows
        ops.gemm_raw(buf[0], K, Ws, 2 * K, C, 2 * D, M, N, K, Ct=vt, n_split=2 * D, R=R, dh=64, a_rep=2)
        v_rows = vt.view(M // R, D, R).transpose(1, 2).reshape(M, D)
    else:
        pitch = [56, 40, 168]
        seg = ops.RowSegments(pitch, pitch, DEV)
        ops.gemm_raw(buf[0], K, Ws, 2 * K, C, 2 * D, M, N, K, Ct=vt, n_split=2 * D, R=0, dh=64, seg=seg, a_rep=2)
        v_rows = torch.cat([vt[D * r0: D * (r0 + p)].view(D, p).t() for r0, p in zip(seg.row0_host[:-1], pitch)])
    torch.cuda.synchronize()
    assert torch.equal(C, plain[:, : 2 * D])
    assert torch.equal(v_rows, plain[:, 2 * D:])


def test_gemm_split_batched():
    ops = _ops()
    M, N, K, nb1, nb2 = 136, 72, 128, 2, 3
    nb = nb1 * nb2
    buf, A, W = _operands(M, N, K, K, seed=31, batch=nb)
    Ws = ops.split_weight_bf16(W)                                             # [6, N, 2K]
    C = torch.full((nb, M, N), float("nan"), device=DEV)
    ops.gemm_raw(buf, K, Ws, 2 * K, C, N, M, N, K, out_f32=True, nb1=nb1, nb2=nb2, sA=(nb2 * buf.stride(0), buf.stride(0)),
                 sW=(nb2 * N * 2 * K, N * 2 * K), sC=(nb2 * M * N, M * N), a_rep=2)
    for b in range(nb):
        ref, mag = _ref(A[b], W[b])
        err = (C[b].double() - ref).abs()
        assert bool((err <= (U_W + 2 * K * U_ACC) * mag).all()), b
        assert torch.equal(C[b], _launch(buf[b], M, N, K, K, Ws[b], 2)), b    # and the same bits as the launch on its own


@pytest.mark.parametrize("K,tap_c,lda", [(128, 0, 128), (192, 64, 128)])
def test_tile_families_agree_bitwise(K, tap_c, lda):
    ops = _ops()
    M, N = 520, 384
    buf, A, W = _operands(M, N, K, lda, seed=41 + K)
    Ws = ops.split_weight_bf16(W[0])
    auto = _launch(buf[0], M, N, K, lda, Ws, 2, tap_c)
    ref, mag = _ref(A[0], W[0])
    assert bool(((auto.double() - ref).abs() <= (U_W + 2 * K * U_ACC) * mag).all())
    for tile in FAMILIES:
        assert torch.equal(_launch(buf[0], M, N, K, lda, Ws, 2, tap_c, tile=tile), auto), tile


@pytest.mark.parametrize("M,N,K,tap_c,lda", SHAPES)
def test_default_path_untouched_by_a_rep_0_and_1(M, N, K, tap_c, lda):
    buf, A, W = _operands(M, N, K, lda, seed=51 + K)
    Wb = W[0].to(torch.bfloat16).contiguous()
    for out_f32 in (True, False):
        c0 = _launch(buf[0], M, N, K, lda, Wb, 0, tap_c, out_f32=out_f32)
        c1 = _launch(buf[0], M, N, K, lda, Wb, 1, tap_c, out_f32=out_f32)
        assert torch.equal(c0, c1)
        if out_f32:                                                           # and it is the bf16(W) product
            ref, mag = _ref(A[0], Wb)
            assert bool(((c0.double() - ref).abs() <= K * U_ACC * mag).all())


# ---------------------------------------------------------------------------------------------------------------- one-call layer
class _Scratch:
    def __init__(self, M, D, F, slack=64):
        z = lambda *s: torch.zeros(*s, device=DEV, dtype=torch.bfloat16)
        self.qk, self.vt, self.ctx, self.pre, self.x1, self.ffn = z(M + slack, 2 * D), z((M + slack) * D), z(M + slack, D), z(M + slack, D), z(M + slack, D), z(M + slack, F)


@pytest.mark.parametrize("pre_ln", [False, True])
@pytest.mark.parametrize("layout", ["padded", "segment"])
def test_layer_driver_with_w_split_equals_per_op(pre_ln, layout):
    ops = _ops()
    B, R, D, F, H = 3, 56, 128, 256, 2
    lens = [50, 37, 9]
    g = torch.Generator().manual_seed(61)
    f32 = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(DEV)
    w = {"l0_qkv_w": ops.split_weight_bf16(f32(3 * D, D, sc=D ** -0.5)), "l0_o_w": ops.split_weight_bf16(f32(D, D, sc=D ** -0.5)),
         "l0_fc1_w": ops.split_weight_bf16(f32(F, D, sc=D ** -0.5)), "l0_fc2_w": ops.split_weight_bf16(f32(D, F, sc=F ** -0.5)),
         "l0_qkv_b": f32(3 * D, sc=0.05), "l0_o_b": f32(D, sc=0.05), "l0_fc1_b": f32(F, sc=0.05), "l0_fc2_b": f32(D, sc=0.05)}
    for n in ("ln1", "ln2"):
        w[f"l0_{n}_g"], w[f"l0_{n}_b"] = 1.0 + f32(D, sc=0.1), f32(D, sc=0.1)
    if layout == "segment":
        pitch = [56, 40, 16]
        seg, M = ops.RowSegments(pitch, lens, DEV), sum(pitch)
    else:
        seg, M = None, B * R
    x = torch.zeros(M + 64, D, device=DEV, dtype=torch.bfloat16)
    x[:M] = torch.randn(M, D, generator=g).to(torch.bfloat16).to(DEV)
    x = x[:M]
    valid = torch.tensor(lens, device=DEV, dtype=torch.int32)
    # one call
    s1 = _Scratch(M, D, F)
    for k in ("qk", "ctx", "pre", "x1", "ffn"):
        setattr(s1, k, getattr(s1, k)[:M])
    out1 = torch.zeros(M, D, device=DEV, dtype=torch.bfloat16)
    ops.hubert_layer_fwd(x, out1, valid, w, 0, s1, B, R, max(lens), D, F, H, pre_ln, seg=seg, w_split=True)
    # op by op, a_rep = 2
    s2 = _Scratch(M, D, F)
    for k in ("qk", "ctx", "pre", "x1", "ffn"):
        setattr(s2, k, getattr(s2, k)[:M])
    out2 = torch.zeros(M, D, device=DEV, dtype=torch.bfloat16)
    attn_in = x
    if pre_ln:
        ops.layernorm_bf16(x, w["l0_ln1_g"], w["l0_ln1_b"], out=s2.x1)
        attn_in = s2.x1
    ops.gemm_raw(attn_in, D, w["l0_qkv_w"], 2 * D, s2.qk, 2 * D, M, 3 * D, D, bias=w["l0_qkv_b"], Ct=s2.vt, n_split=2 * D, R=R, dh=64, seg=seg, a_rep=2)
    ops.attn_fwd(s2.qk, s2.vt, valid, s2.ctx, B, R, H, D, 0.125, seg=seg)
    ops.linear_bf16(s2.ctx, w["l0_o_w"], w["l0_o_b"], out=s2.pre, residual=x, a_rep=2)
    if pre_ln:
        ops.layernorm_bf16(s2.pre, w["l0_ln2_g"], w["l0_ln2_b"], out=s2.x1)
        ops.linear_bf16(s2.x1, w["l0_fc1_w"], w["l0_fc1_b"], out=s2.ffn, act=1, a_rep=2)
        ops.linear_bf16(s2.ffn, w["l0_fc2_w"], w["l0_fc2_b"], out=out2, residual=s2.pre, a_rep=2)
    else:
        ops.layernorm_bf16(s2.pre, w["l0_ln1_g"], w["l0_ln1_b"], out=s2.x1)
        ops.linear_bf16(s2.x1, w["l0_fc1_w"], w["l0_fc1_b"], out=s2.ffn, act=1, a_rep=2)
        ops.linear_bf16(s2.ffn, w["l0_fc2_w"], w["l0_fc2_b"], out=s2.pre, residual=s2.x1, a_rep=2)
        ops.layernorm_bf16(s2.pre, w["l0_ln2_g"], w["l0_ln2_b"], out=out2)
    torch.cuda.synchronize()
    # rows an utterance's queries own (pad rows hold finite scratch in both runs; they are compared too: same kernels, same inputs)
    assert torch.isfinite(out1.float()).all()
    assert torch.equal(out1, out2)
    assert torch.equal(s1.ffn, s2.ffn) and torch.equal(s1.qk, s2.qk)
    # and the split weights are what was multiplied: the bf16 halves alone give other bits
    wb = dict(w)
    for k in ("qkv", "o", "fc1", "fc2"):
        s = w[f"l0_{k}_w"]
        wb[f"l0_{k}_w"] = s.view(s.shape[0], -1, 2, 64)[:, :, 0].reshape(s.shape[0], -1).contiguous()
    out3 = torch.zeros(M, D, device=DEV, dtype=torch.bfloat16)
    ops.hubert_layer_fwd(x, out3, valid, wb, 0, s2, B, R, max(lens), D, F, H, pre_ln, seg=seg)
    assert not torch.equal(out1, out3)


# ---------------------------------------------------------------------------------------------------------------- small encoder
def _small(case, eval_weights):
    from speechclip_plus_amd import speech_encoder as se
    name, a, sd, wav = split_cases.small_case(case)
    return se.FairseqSpeechEncoder_Hubert(name, arch=a, state_dict=sd, device=DEV, eval_weights=eval_weights), wav


def _states(enc, wav, uniform):
    enc._seg_mode = (lambda: False) if uniform else (lambda: True)
    with torch.no_grad():
        _, feat_len, hs = enc(wav.to(DEV), split_cases.LENS, feat_select_idx="last_hidden_state", return_hidden_states=True)
    torch.cuda.synchronize()
    return [h.float().cpu() for h in hs], [int(v) for v in feat_len.cpu().tolist()]


@pytest.fixture(scope="module")
def oracles():
    """the CPU references, computed once per case and shared: the fp32 oracle and the split emulation (all storage sites + w_split)"""
    made = {}

    def get(case):
        if case not in made:
            made[case] = (split_cases.oracle_states(case, "fp32"), split_cases.oracle_states(case, "split")[0])
        return made[case]
    return get


def _valid(h, feat_len):
    return torch.cat([h[b, :n] for b, n in enumerate(feat_len)])


@pytest.mark.parametrize("case", ["base_small", "large_small"])
@pytest.mark.parametrize("layout", ["uniform", "segment"])
def test_small_encoder_split_is_closer_to_fp32_and_train_mode_is_untouched(oracles, case, layout):
    uniform = layout == "uniform"
    enc_s, wav = _small(case, "split")
    enc_b = _small(case, "bf16")[0]
    (ref, fl), emu = oracles(case)
    hs_s, feat_len = _states(enc_s.eval(), wav, uniform)
    hs_b, _ = _states(enc_b.eval(), wav, uniform)
    assert feat_len == fl
    # every hidden state (the small encoders have two layers: three states) and the weighted sum against the split emulation, over the
    # valid frames, with the bound the shipped path's states meet against ITS emulation (LP_HIDDEN of tests/test_gpu_model.py, rel-L2)
    assert len(hs_s) == len(emu) == 3
    for n, (h, e) in enumerate(zip(hs_s, emu)):
        r = rel_l2(_valid(h, feat_len), _valid(e, feat_len))
        print(f"[split-encoder] {case} {layout}: hidden state {n} rel-L2 vs split emulation {r:.3g}")
        assert r <= LP_HIDDEN, (n, r)
    r = rel_l2(_valid(sum(hs_s) / 3, feat_len), _valid(sum(emu) / 3, feat_len))
    print(f"[split-encoder] {case} {layout}: weighted sum rel-L2 vs split emulation {r:.3g}")
    assert r <= LP_HIDDEN, r
    d_s, d_b = split_cases.dist(hs_s, ref, feat_len), split_cases.dist(hs_b, ref, feat_len)
    d_emu_split, d_emu_bf16 = np.load(split_cases.FIXTURE)[case]
    print(f"[split-encoder] {case} {layout}: d(HIP split) {d_s:.4g} (emulation {d_emu_split:.4g})  d(HIP bf16) {d_b:.4g} (emulation {d_emu_bf16:.4g})")
    assert d_s <= 1.25 * d_emu_split, (d_s, d_emu_split)          # HIP is as close to fp32 as the emulation is (the factor of test_gpu_recall.py)
    assert d_s < d_b, (d_s, d_b)
    # train mode (dropout held off so that two forwards can be compared): the split encoder runs the bf16 weights, bit for bit
    enc_s.train()
    enc_b.train()
    enc_s.hubert_dropout = enc_b.hubert_dropout = False
    t_s, _ = _states(enc_s, wav, uniform)
    t_b, _ = _states(enc_b, wav, uniform)
    assert all(torch.equal(x, y) for x, y in zip(t_s, t_b))
    assert not all(torch.equal(x, y) for x, y in zip(t_s, hs_s))
    e_b, _ = _states(enc_b.eval(), wav, uniform)
    assert all(torch.equal(x, y) for x, y in zip(e_b, hs_b))            # and going back to eval gives the first eval forward's bits


# ---------------------------------------------------------------------------------------------------------------- recall, 5000 utterances
@pytest.fixture(scope="module")
def hip_split_emb():
    """the product model with eval_weights = "split": unit embeddings of the 5000 utterances (one pass, shared by the two galleries)"""
    import recall_eval
    model = recall_eval.build_model(eval_weights="split")
    assert model.audio_encoder._split_active()
    return torch.nn.functional.normalize(recall_eval.hip_embeddings(model, 1000, recall_eval.BATCH), dim=-1)


@pytest.mark.parametrize("g,gallery", [("a", "recall_eval_natural.npz"), ("b", "recall_eval_natural_b.npz")])
def test_recall_with_split_weights_on_natural_margins(golden, hip_split_emb, g, gallery):
    """The pre-registered form of tests/test_gpu_recall.py::test_recall_on_natural_margins with the split emulation (every storage site
    + w_split, tests/golden/make_recall_splitw_fixture.py) in the place of the bf16 emulation: in both directions and at k = 1, 5, 10
    HIP-split's flips against fp32 come at the rate of the split emulation's (_same_rate, z = 3) and its flips against the split emulation
    are at most emu + 3 sqrt(vs_emu + emu); and the common shift of its unit embeddings against fp32 - what the mode exists to remove -
    is at most 1.25 x the split emulation's.  The recalls are asserted (inside the band the flip counts allow) only where the emulation
    itself is within 0.1 of fp32 at every k of both galleries; otherwise they are printed."""
    import recall_eval
    from test_gpu_recall import _same_rate
    fx, sp = golden(gallery), golden("recall_eval_splitemu.npz")
    a = hip_split_emb
    ids = torch.arange(1000).repeat_interleave(recall_eval.PER_ID)
    st = recall_eval.rank_stats(a, torch.from_numpy(fx["image"]), ids)
    shift = float((a.mean(0) - torch.from_numpy(sp["mean_unit_fp32"])).norm())
    print(f"[split-recall] {gallery}: common shift {shift:.5f} (split emulation {float(sp['shift_splitemu']):.5f})")
    assert shift <= 1.25 * float(sp["shift_splitemu"]), (shift, float(sp["shift_splitemu"]))
    flips = lambda x, y, k: int(((x < k) != (y < k)).sum())
    emu_close = True
    for gg, name in (("a", "recall_eval_natural.npz"), ("b", "recall_eval_natural_b.npz")):
        f2 = fx if gg == g else golden(name)
        for d in ("ai", "ia"):
            r32, rem = recall_eval.recalls(torch.from_numpy(f2[f"rank_{d}_fp32"]).long()), recall_eval.recalls(torch.from_numpy(sp[f"rank_{d}_splitemu_{gg}"]).long())
            emu_close = emu_close and all(abs(x - y) <= 0.1 + 1e-9 for x, y in zip(r32, rem))
    for d, n in (("ai", 5000), ("ia", 1000)):
        r32, rem, rh = torch.from_numpy(fx[f"rank_{d}_fp32"]).long(), torch.from_numpy(sp[f"rank_{d}_splitemu_{g}"]).long(), st[f"rank_{d}"].long()
        print(f"[split-recall] {gallery} {d}: HIP split {recall_eval.recalls(rh)}  split emulation {recall_eval.recalls(rem)}  fp32 {recall_eval.recalls(r32)}")
        for i, k in enumerate((1, 5, 10)):
            emu, vs_fp32, vs_emu = flips(rem, r32, k), flips(rh, r32, k), flips(rh, rem, k)
            print(f"[split-recall]   @{k}: flips emulation vs fp32 {emu}, HIP vs fp32 {vs_fp32}, HIP vs emulation {vs_emu}")
            assert _same_rate(vs_fp32, emu), (gallery, d, k, vs_fp32, emu)
            assert vs_emu <= emu + 3.0 * (vs_emu + emu) ** 0.5, (gallery, d, k, vs_emu, emu)
            if emu_close:
                assert abs(recall_eval.recalls(rh)[i] - recall_eval.recalls(r32)[i]) <= 0.1 + 100.0 * emu / n + 1e-9
