"""WavLM on the GPU: the gate kernel, the BIAS instances of the flash forward (both row layouts, with and without dropout) and the
frozen encoder end to end, each against the fp64 references of tests/wavlm_cases.py.  Figures are printed before they are asserted."""
import dataclasses

import pytest
import torch

import head_cases as hc
import wavlm_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from speechclip_plus_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------------------------------- gate
@pytest.mark.parametrize("rows", [1, 130, 777])
@pytest.mark.parametrize("H", [2, 12])
def test_gate_kernel(rows, H):
    """fp64 on the kernel's own bf16 inputs; every element within 4 x the fp32 yardstick's worst (head_cases.yard_bound)"""
    ops = _ops()
    g = torch.Generator().manual_seed(rows * 31 + H)
    x = (torch.randn(rows, H * 64, generator=g) * 1.5).to(torch.bfloat16)
    wg, bg = torch.randn(8, 64, generator=g) * 0.125, torch.randn(8, generator=g) * 0.3
    cst = 1.0 + 0.3 * torch.randn(H, generator=g)
    got = ops.wavlm_gate(x.to(DEV), wg.to(DEV), bg.to(DEV), cst.to(DEV), H)
    torch.cuda.synchronize()
    ref = wc.gate_ref(x.double(), wg.double(), bg.double(), cst.double(), H)
    yard = wc.gate_ref(x.float(), wg, bg, cst, H)
    rep = hc.Report()
    rep.yard(f"gate rows={rows} H={H}", "gate", got.cpu(), ref, yard, dims=())
    rep.done()
    # a wider row stride (the QKV GEMM's input may be a view) reads the same columns
    wide = torch.zeros(rows, H * 64 + 64, dtype=torch.bfloat16)
    wide[:, : H * 64] = x
    got2 = ops.wavlm_gate(wide.to(DEV)[:, : H * 64], wg.to(DEV), bg.to(DEV), cst.to(DEV), H)
    assert torch.equal(got, got2)


# ------------------------------------------------------------------------------------------------------------- biased attention
H_A, D_A, TMAX = 2, 128, 400
CASES = [(128, [128, 1, 37]), (256, [200, 256, 65]), (384, [300, 129, 64])]


def _attn_inputs(R, lens, spike):
    B = len(lens)
    g = torch.Generator().manual_seed(R)
    q, k, v = (torch.randn(B, R, D_A, generator=g).to(torch.bfloat16) for _ in range(3))
    gate = 0.5 + 2.0 * torch.rand(H_A, B * R, generator=g)                                  # (0.5, 2.5)
    table = wc.bias_table(torch.randn(wc.NUM_BUCKETS, H_A, generator=g), TMAX)              # the real bucket function over N(0, 1)
    if spike:
        # +8 at an offset that query 5 of utterance 0 / head 0 reaches in its LAST key tile: the running maximum jumps by
        # 8 x gate x log2(e) > 2^6's exponent there and the accumulators are rescaled
        gate[0, 5] = 2.0
        table[0, TMAX - 1 + (lens[0] - 10 - 5)] = 8.0
    return q, k, v, gate, table


def _reference(q, k, v, gate, table, lens, R, biased=True):
    B = len(lens)
    out = torch.zeros(B, R, D_A, dtype=torch.float64)
    for b in range(B):
        for h in range(H_A):
            cols = slice(h * 64, h * 64 + 64)
            out[b, :, cols] = wc.biased_attention_ref(q[b, :, cols].double(), k[b, :, cols].double(), v[b, :, cols].double(), 0.125,
                                                      gate[h, b * R: (b + 1) * R].double() if biased else None,
                                                      table[h].double() if biased else None, lens[b])
    return out


def _uniform(ops, q, k, v, lens, R, gate=None, table=None, drop_p=0.0, seed=0):
    B = len(lens)
    qk = torch.cat([q, k], dim=-1).reshape(B * R, 2 * D_A).contiguous().to(DEV)
    vt = v.view(B, R, H_A, 64).permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.zeros(B * R, D_A, device=DEV, dtype=torch.bfloat16)
    ops.attn_fwd(qk, vt, torch.tensor(lens, dtype=torch.int32, device=DEV), out, B, R, H_A, D_A, 0.125, drop_p=drop_p, drop_seed=seed,
                 gate=None if gate is None else gate.to(DEV), table=None if table is None else table.to(DEV))
    torch.cuda.synchronize()
    return out.cpu().view(B, R, D_A)


def _segments(ops, q, k, v, lens, gate, table, fill):
    """the same utterances in the ragged layout: pitch = the length rounded up to 8 rows, longest-first work list"""
    B, R = len(lens), q.shape[1]
    pitch = [(l + 7) // 8 * 8 for l in lens]
    seg = ops.RowSegments(pitch, lens, DEV)
    M, r0 = seg.rows, seg.row0_host
    qk = torch.zeros(M + 64, 2 * D_A, dtype=torch.bfloat16)
    vt = torch.zeros(D_A * (M + 64), dtype=torch.bfloat16)
    gs = torch.zeros(H_A, M)
    for b, p in enumerate(pitch):
        qk[r0[b]: r0[b] + p] = torch.cat([q[b, :p], k[b, :p]], dim=-1)
        vt[D_A * r0[b]: D_A * (r0[b] + p)] = v[b, :p].view(p, H_A, 64).permute(1, 2, 0).reshape(-1)
        gs[:, r0[b]: r0[b] + p] = gate[:, b * R: b * R + p]
    out = torch.full((M + 64, D_A), fill, dtype=torch.bfloat16).to(DEV)
    ops.attn_fwd(qk.to(DEV), vt.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), out, 0, 0, H_A, D_A, 0.125, seg=seg,
                 gate=gs.to(DEV), table=table.to(DEV))
    torch.cuda.synchronize()
    return out.cpu(), pitch, r0, M


@pytest.mark.parametrize("R,lens", CASES)
def test_biased_attention(R, lens):
    ops = _ops()
    q, k, v, gate, table = _attn_inputs(R, lens, spike=(R == 256))
    ref = _reference(q, k, v, gate, table, lens, R)
    got = _uniform(ops, q, k, v, lens, R, gate, table)
    plain = _uniform(ops, q, k, v, lens, R)
    e, m = wc.rel_l2(got, ref), float((got.double() - ref).abs().max())
    ep, mp = wc.rel_l2(plain, ref), float((plain.double() - ref).abs().max())
    print(f"WAVLM|attn uniform R={R}|biased rel_l2 {e:.3e} max {m:.3e}|plain kernel vs biased reference rel_l2 {ep:.3e} max {mp:.3e}")
    assert e < wc.ATTN_REL_L2 and m < wc.ATTN_MAX_ABS, (e, m)
    assert ep > wc.ATTN_REL_L2 and mp > wc.ATTN_MAX_ABS, "the plain kernel must MISS the biased reference"
    assert torch.equal(got, _uniform(ops, q, k, v, lens, R, gate, table)), "two runs are bit-identical"
    # segment layout, work list: the rows it shares with the uniform call are the same bits; nothing behind the last utterance is stored
    out, pitch, r0, M = _segments(ops, q, k, v, lens, gate, table, fill=7.0)
    for b, p in enumerate(pitch):
        rows = out[r0[b]: r0[b] + p]
        es, ms = wc.rel_l2(rows, ref[b, :p]), float((rows.double() - ref[b, :p]).abs().max())
        print(f"WAVLM|attn segments R={R} b={b} pitch={p}|rel_l2 {es:.3e} max {ms:.3e}")
        assert es < wc.ATTN_REL_L2 and ms < wc.ATTN_MAX_ABS, (b, es, ms)
        assert torch.equal(rows, got[b, :p]), f"utterance {b}: segment and uniform layouts differ"
    assert bool((out[M:] == 7.0).all()), "rows past the last pitch were stored"
    out2 = _segments(ops, q, k, v, lens, gate, table, fill=7.0)[0]
    assert torch.equal(out, out2)


def test_biased_attention_refuses_causal():
    ops = _ops()
    q, k, v, gate, table = _attn_inputs(128, [128], spike=False)
    qk = torch.cat([q, k], dim=-1).reshape(128, 2 * D_A).contiguous().to(DEV)
    vt = v.view(1, 128, H_A, 64).permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.zeros(128, D_A, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="causal"):
        ops.attn_fwd(qk, vt, torch.tensor([128], dtype=torch.int32, device=DEV), out, 1, 128, H_A, D_A, 0.125, causal=True,
                     gate=gate.to(DEV), table=table.to(DEV))


def test_biased_attention_dropout_mask_is_the_plain_one():
    """zero table, drop_p = 0.1, same seed: the biased instance keeps the element index and hash of the plain one, so the two differ
    by no more than they do without dropout (x 2 for bf16 rounding of differently ordered arithmetic); another mask would differ by
    orders of magnitude more (shown with another seed)"""
    ops = _ops()
    R, lens = 256, [200, 256, 65]
    q, k, v, gate, table = _attn_inputs(R, lens, spike=False)
    zero = torch.zeros_like(table)
    d0 = wc.rel_l2(_uniform(ops, q, k, v, lens, R, gate, zero), _uniform(ops, q, k, v, lens, R))
    a = _uniform(ops, q, k, v, lens, R, gate, zero, drop_p=0.1, seed=1234)
    b = _uniform(ops, q, k, v, lens, R, drop_p=0.1, seed=1234)
    d1 = wc.rel_l2(a, b)
    other = wc.rel_l2(a, _uniform(ops, q, k, v, lens, R, drop_p=0.1, seed=4321))
    print(f"WAVLM|attn dropout|biased vs plain p=0 {d0:.3e}|p=0.1 same seed {d1:.3e}|p=0.1 other seed {other:.3e}")
    assert d1 <= 2.0 * d0, (d1, d0)
    assert other > 100.0 * max(d0, 1e-6)


# ----------------------------------------------------------------------------------------------------------------- end to end
def _small_encoders(variant):
    from speechclip_plus_amd import speech_encoder as se
    fx, stable = wc.load_fixture(variant), variant == "stable"
    o_arch = wc.small_arch(stable)
    arch = se.HubertArch(embed_dim=128, ffn_dim=256, layers=2, heads=2, conv_dim=32, pos_conv_groups=2, layer_norm_first=stable,
                         extractor_mode="layer_norm" if stable else "default", conv_bias=stable, dropout=0.0, attention_dropout=0.0,
                         dropout_input=0.0, rel_pos_buckets=320)
    W = se.wavlm_state_dict_keys(fx["W"], arch)
    wavlm = se.FairseqSpeechEncoder_Hubert(name="wavlm_base", arch=arch, state_dict=W, device=DEV, feat_select_idx="weighted_sum").eval()
    hubert = se.FairseqSpeechEncoder_Hubert(name="hubert", arch=dataclasses.replace(arch, rel_pos_buckets=0), state_dict=W, device=DEV,
                                            feat_select_idx="weighted_sum").eval()
    return fx, o_arch, W, wavlm, hubert


def _enter_at_projection(enc, proj):
    """The conv front-end kernels are built for 512 channels (sc_conv0_gn_gelu / sc_conv0_ln_gelu, K % 64 of the conv GEMMs), the
    fixture has 32: its front end runs in the reference, and the HIP path enters at post_extract_proj's output - ``proj`` [B, T, D],
    stored in bf16 as the projection GEMM would - with everything from pos_conv on (prep, slab kernel, LayerNorm, every layer's GEMMs,
    gate, attention) on the kernels.  The WavLM encoder and the HuBERT yardstick enter the same way."""
    ops = _ops()
    a = enc.arch

    def front(pl, w, seeds, sd, p_in, p_res, padded=None, a_rep=0):
        seg, r0 = pl.seg, pl.seg.row0_host
        rows = torch.zeros(pl.M, a.embed_dim, dtype=torch.bfloat16)
        for b, p in enumerate(seg.pitch):
            n = min(p, proj.shape[1])
            rows[r0[b]: r0[b] + n] = proj[b, :n].to(torch.bfloat16)
        pl.x_proj.copy_(rows.to(DEV))
        ops.posconv_prep_seg(pl.x_proj, pl.valid, pl.xz, pl.xg, seg, a.embed_dim, a.pos_conv_groups, pl.halo)
        ops.posconv_seg(pl.xg, w["pos_w"], w["pos_b"], pl.xz, pl.pre, seg, a.embed_dim, a.pos_conv_groups, a.pos_conv_kernel)

    enc._frontend_frozen = front


@pytest.mark.parametrize("variant", ["post", "stable"])
def test_end_to_end_against_fp64(variant):
    """every hidden state (valid frames) and the weighted sum of wavlm_small, padded and ragged rows, against the fp64 restatement.
    Yardstick: the HuBERT path (parent kernels) on the same weights against ITS fp64 reference (the table zeroed); the WavLM error may be
    at most 1.5 x that at every state - the bias adds one fp32 product per score and nothing else."""
    fx, o_arch, W, wavlm, hubert = _small_encoders(variant)
    wav, lens = torch.from_numpy(fx["wav"]), fx["lens"].tolist()
    wavs = [wav[b, :l] for b, l in enumerate(lens)]
    dbg = {}
    ref, _, valid, feat_len = wc.wavlm_forward(W, o_arch, wavs, debug=dbg)
    for enc in (wavlm, hubert):
        _enter_at_projection(enc, dbg["proj"].float())
    ref_h, _, _, _ = wc.wavlm_forward(W, o_arch, wavs, zero_bias=True, final_ln=False)
    ws_ref = lambda hs: torch.stack([wc.valid_frames(h, feat_len) for h in hs]).mean(0)
    bad = []
    for ragged in (False, True):
        errs = {}
        for name, enc, r in (("wavlm", wavlm, ref), ("hubert", hubert, ref_h)):
            with torch.no_grad():
                pl = enc._encode(wav.to(DEV), lens, ragged=ragged)
                hs = [h.float().cpu() for h in enc._materialised_states(pl)]
                feat, fl = enc(wav.to(DEV), torch.tensor(lens))
            assert fl.tolist() == feat_len
            errs[name] = [wc.rel_l2(wc.valid_frames(h, valid), wc.valid_frames(x, valid)) for h, x in zip(hs, r)]
            errs[name].append(wc.rel_l2(wc.valid_frames(feat.float().cpu(), feat_len), ws_ref(r)))
        for n, (ew, eh) in enumerate(zip(errs["wavlm"], errs["hubert"])):
            what = f"state {n}" if n < len(ref) else "weighted sum"
            print(f"WAVLM|e2e {variant} {'ragged' if ragged else 'padded'}|{what}|wavlm {ew:.3e}|hubert yardstick {eh:.3e}|ratio {ew / eh:.2f}")
            if not ew <= 1.5 * eh:
                bad.append((ragged, what, ew, eh))
    assert not bad, bad


def test_model_forward_wavlm_base_two_layers():
    """wavlm_base at 2 layers, random weights, B = 2 x 2 s through KWClip_GeneralTransformer.forward in eval and in train mode (the
    frozen encoder's dropouts live, as in the reference's training step): finite loss, the reference's dict keys"""
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config
    from speechclip_plus_amd.speech_encoder import ARCHS
    torch.manual_seed(0)
    cfg = base_parallel_config()
    cfg.audio_encoder.type, cfg.audio_encoder.name = "s3prl_plus", "wavlm_base"
    cfg.audio_encoder.max_audio_len = -1
    model = KWClip_GeneralTransformer(cfg, device=DEV, hubert_arch=dataclasses.replace(ARCHS["wavlm_base"], layers=2))
    g = torch.Generator().manual_seed(1)
    batch = {"wav": torch.randn(2, 32000, generator=g).to(DEV), "wav_len": torch.tensor([32000, 25000]),
             "image": torch.randn(2, 512, generator=g).to(DEV), "id": torch.tensor([0, 1]).to(DEV)}
    for mode in (model.eval(), model.train()):
        with torch.set_grad_enabled(model.training):
            losses, log_metrics, others = mode(batch)
            out = model.compute_loss(losses)
        assert {"id", "image_feat", "parallel_audio_feat"} <= set(losses) and "cl_temp" in log_metrics
        assert {"id", "image_feat", "parallel_audio_feat", "cascaded_audio_feat", "vq_results", "keywords", "dsample_results", "keywords_len"} == set(others)
        assert torch.isfinite(out["loss"]).item() and others["parallel_audio_feat"].shape == (2, 512)
    model.eval()
    a = model(batch)[2]["parallel_audio_feat"]
    assert torch.equal(a, model(batch)[2]["parallel_audio_feat"])


def test_feature_extractor_s3prl_returns_13_wavlm_states():
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config
    cfg = base_parallel_config()
    cfg.audio_encoder.type, cfg.audio_encoder.name = "s3prl_plus", "wavlm_base"
    model = KWClip_GeneralTransformer(cfg, device=DEV).eval()
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        feat, hs = model.feature_extractor_s3prl([torch.randn(16000, generator=g).to(DEV), torch.randn(12000, generator=g).to(DEV)])
    assert len(hs) == 13 + 1 and all(h.shape == hs[0].shape for h in hs)      # 13 WavLM states, then the branch layer's (kwClip.py:965-997)
    assert hs[0].shape[-1] == 768 and all(bool(torch.isfinite(h.float()).all()) for h in hs)
