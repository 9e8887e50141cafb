"""WavLM on the host: the restatement of tests/wavlm_cases.py against transformers' WavLMModel (tests/golden/wavlm_small.npz), the
bucket table, the two key maps, the C ABI additions and the switches that are not built.  No GPU."""
import numpy as np
import pytest
import torch

import wavlm_cases as wc
from speechclip_plus_amd import _lib, speech_encoder as se
from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config

VARIANTS = ("post", "stable")


def _unilm_weights(fx, stable):
    return se.wavlm_state_dict_keys(fx["W"], wc.small_arch(stable))


@pytest.mark.parametrize("variant", VARIANTS)
def test_restatement_reproduces_hf(variant):
    """every hidden state and every gate of the padded batch, valid frames, at the bound of test_hubert_vs_hf"""
    fx, stable = wc.load_fixture(variant), variant == "stable"
    W = _unilm_weights(fx, stable)
    wav, lens = torch.from_numpy(fx["wav"]), fx["lens"].tolist()
    hidden, gates, valid, _ = wc.wavlm_forward(W, wc.small_arch(stable), [wav[b, :l] for b, l in enumerate(lens)], dtype=torch.float32)
    assert valid == fx["valid"].tolist()
    assert len(hidden) == fx["hidden"].shape[0] == 3
    for n, h in enumerate(hidden):
        np.testing.assert_allclose(wc.valid_frames(h, valid).numpy(), fx["hidden"][n], rtol=1e-3, atol=2e-5)
    for n, g in enumerate(gates):                      # [B, H, T] -> [H, sum(valid)]
        got = torch.cat([g[b, :, :v] for b, v in enumerate(valid)], dim=1)
        np.testing.assert_allclose(got.numpy(), fx["gates"][n], rtol=1e-3, atol=2e-5)


@pytest.mark.parametrize("variant", VARIANTS)
def test_bucket_table_equals_hf(variant):
    """the host table at T = 1000 is layer 0's position_bias: first row (offsets 0 .. 999) and first column (0 .. -999), exactly -
    the exact / logarithmic boundary at 80 and the clamp beyond 800 included"""
    fx = wc.load_fixture(variant)
    emb = fx["W"]["encoder.layers.0.attention.rel_attn_embed.weight"]
    tab = se.wavlm_bias_table(emb, 1000)
    assert tab.shape == (2, 1999)
    assert np.array_equal(tab[:, 999:].numpy(), fx["bias_row"])
    assert np.array_equal(tab[:, :1000].flip(1).numpy(), fx["bias_col"])
    idx = se.wavlm_bucket_index(1000)
    assert torch.equal(idx, wc.bucket_of_offsets(torch.arange(-999, 1000)))
    assert idx[999 + 79] == 160 + 79 and idx[999 + 80] == 160 + 80 and idx[999 - 79] == 79
    assert int(idx[999 + 800:].min()) == 319 and int(idx[: 999 - 799].max()) == 159     # clamped from 800 on


def test_both_key_maps_load_the_same_weights():
    fx = wc.load_fixture("post")
    arch = se.HubertArch(embed_dim=128, ffn_dim=256, layers=2, heads=2, conv_dim=32, pos_conv_groups=2, rel_pos_buckets=320)
    unilm = se.wavlm_state_dict_keys(fx["W"], arch)
    assert "encoder.layers.1.self_attn.grep_linear.weight" in unilm and "encoder.layers.0.self_attn.relative_attention_bias.weight" in unilm
    assert "encoder.layers.1.self_attn.grep_a" in unilm and not any("attention." in k or "feature_projection" in k for k in unilm)
    assert se.wavlm_state_dict_keys(unilm, arch).keys() == unilm.keys()            # unilm names pass through
    a = se.FairseqSpeechEncoder_Hubert(name="wavlm_base", arch=arch, state_dict=fx["W"], device="cpu")
    b = se.FairseqSpeechEncoder_Hubert(name="wavlm_base", arch=arch, state_dict=unilm, device="cpu")
    assert a._w.keys() == b._w.keys() and "rel_embed" in a._w and "l1_gate_w" in a._w
    for k, v in a._w.items():
        assert v is None and b._w[k] is None or torch.equal(v, b._w[k]), k


def test_abi_additions():
    lib = _lib.lib()
    assert lib.sc_abi_version() == 7
    # the library can run biased attention: the gate kernel, and the one attention entry takes the bias as arguments
    assert "sc_wavlm_gate_bf16" in _lib.SIGNATURES and lib.sc_wavlm_gate_bf16 is not None
    import os, re
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "speechclip_hip.h")).read()
    assert "int sc_wavlm_gate_bf16(" in header
    decl = re.search(r"int sc_attn_fwd_bf16\(([^;]*)\);", header)
    assert decl is not None
    for arg in ("const float* gate", "const float* table", "int32_t tmax"):
        assert arg in decl.group(1), arg
    assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES["sc_attn_fwd_bf16"])


def test_archs():
    for name in ("wavlm_base", "wavlm_base_plus"):
        a = se.ARCHS[name]
        assert (a.embed_dim, a.ffn_dim, a.layers, a.heads, a.layer_norm_first) == (768, 3072, 12, 12, False)
        assert a.rel_pos_buckets == 320 and a.rel_pos_max_distance == 800
    a = se.ARCHS["wavlm_large"]
    assert (a.embed_dim, a.ffn_dim, a.layers, a.heads, a.layer_norm_first, a.extractor_mode, a.normalize_wav) == (1024, 4096, 24, 16, True, "layer_norm", True)
    assert a.rel_pos_buckets == 320
    assert se.ARCHS["hubert_base"].rel_pos_buckets == 0 and se.HubertArch().rel_pos_max_distance == 800


def test_not_built_switches_raise(monkeypatch):
    mk = lambda **kw: se.S3prlSpeechEncoderPlus("wavlm_base", device="cpu", **kw)
    with pytest.raises(NotImplementedError, match="FROZEN"):
        mk(trainable=True)
    with pytest.raises(NotImplementedError, match="FROZEN"):
        mk(trainable=True, unfreeze_layers=[11])
    with pytest.raises(NotImplementedError, match="FROZEN"):
        mk(trainable=True, reinit_layers=[10, 11])
    with pytest.raises(NotImplementedError, match="split"):
        mk(eval_weights="split")
    enc = mk()
    with pytest.raises(NotImplementedError, match="split"):
        enc.set_eval_weights("split", state_dict={})
    monkeypatch.setattr(se, "_FUSED_LN", True)
    with pytest.raises(NotImplementedError, match="SC_FUSED_LN"):
        mk()
    monkeypatch.setattr(se, "_FUSED_LN", False)
    with pytest.raises(NotImplementedError, match="hubert_base"):
        se.S3prlSpeechEncoderPlus("hubert_base", device="cpu")
    with pytest.raises(NotImplementedError, match="wav2vec2"):
        se.S3prlSpeechEncoderPlus("wav2vec2", device="cpu")


# ------------------------------------------------------------------- rehearsal of tests/test_gpu_wavlm_stages.py's criteria
# H = 12, pitches 152 / 72 / 136 / 8, valid 150 / 65 / 127 / 5 (base_small, segment rows).  The kernel is stood in for by
# attn_cases.emulate_fwd_bias (its arithmetic order in torch fp32) on random bf16 operands with a gate from gate_ref in fp32 and a real
# bucket table: the reference alone has to stay inside the bound of docs/parity.md ("Attention on peaked and drifting scores", BIAS),
# and every wrong reference the GPU module plants has to be rejected by the element-wise criterion alone.
_REHEARSAL = {}


def _rehearsal(H=wc.STAGE_H):
    """operands, the fp32 gates of both layers' parameters on the same rows, the emulation's output and the fp64 reference per
    utterance (layer 1's parameters are the right ones): computed once, left unchanged"""
    if H not in _REHEARSAL:
        c = wc.rehearsal_operands(H=H)
        c["gates"] = [wc.gate_ref(c["x"].float(), *p, H) for p in c["gate_params"]]
        c["gates64"] = [wc.gate_ref(c["x"].double(), *p, H) for p in c["gate_params"]]
        c["emu"] = [wc.emulate_segment(c, c["gates"][1], b, v) for b, v in enumerate(wc.STAGE_VALID)]
        c["ref"] = [wc.segment_attention_ref(c["qk"], c["vt"], c["gates"][1], c["table"], c["r0"][b], c["pitch"][b], v, H, 0.125)
                    for b, v in enumerate(wc.STAGE_VALID)]
        _REHEARSAL[H] = c
    return _REHEARSAL[H]


def _share_rejected(c, gate=None, table=None):
    """share of the valid query rows of the four utterances that the element-wise criterion rejects when the reference is built from
    ``gate`` / ``table`` instead of the right ones, and the largest error / bound"""
    H = c["H"]
    rej = tot = 0
    worst = 0.0
    for b, v in enumerate(wc.STAGE_VALID):
        f = wc.segment_attention_ref(c["qk"], c["vt"], c["gates"][1] if gate is None else gate, c["table"] if table is None else table,
                                     c["r0"][b], c["pitch"][b], v, H, 0.125)
        rej += int(wc.rows_rejected(c["emu"][b], f["out"], f["bound"])[:v].sum())
        tot += v
        worst = max(worst, float(((c["emu"][b].double() - f["out"]).abs() / f["bound"]).max()))
    return rej / tot, worst


def test_rehearsal_unpacking_round_trip():
    c = _rehearsal()
    g = torch.Generator().manual_seed(1)
    v = torch.randn(c["M"], c["D"], generator=g).to(torch.bfloat16)
    vt = wc.pack_vt(v, c["r0"], c["pitch"], c["H"], slack=64)
    assert vt.numel() == c["D"] * (c["M"] + 64) and not bool(vt[c["D"] * c["M"]:].any())
    for r0, p in zip(c["r0"], c["pitch"]):
        assert torch.equal(wc.rows_of(wc.vt_segment(vt, r0, p, c["H"])), v[r0: r0 + p])
    assert torch.equal(wc.rows_of(wc.heads_of(v[:8], c["H"])), v[:8])
    assert c["table"].shape == (12, 2 * wc.STAGE_R - 1) and sum(wc.STAGE_PITCH) == c["M"] == 368
    # the shifted table holds the embedding of offset d + 1 where the right one holds offset d's
    sh = wc.table_shifted(c["rel"], wc.STAGE_R)
    assert sh.shape == c["table"].shape and torch.equal(sh[:, :-1], c["table"][:, 1:]) and not torch.equal(sh, c["table"])


def test_rehearsal_emulation_stays_within_the_bound():
    c = _rehearsal()
    for b, v in enumerate(wc.STAGE_VALID):
        f, got = c["ref"][b], c["emu"][b].double()
        ratio = float(((got - f["out"]).abs() / f["bound"]).max())
        e = wc.rel_l2(got, f["out"])
        print(f"WAVLM|rehearsal b={b} pitch={c['pitch'][b]} valid={v}|max error / bound {ratio:.3f}|rel-L2 {e:.3e}")
        assert got.shape == (12, c["pitch"][b], 64) and bool((got != f["out"]).any())
        assert ratio <= 1.0 and e <= 1e-2
    assert float(c["gates"][1].min()) > 0.9 and float(c["gates"][1].max()) < 3.1


def test_rehearsal_rejects_wrong_gate_parameters_and_tables():
    """layer 0's gate parameters on layer 1's rows, the table one offset off, heads 0 and 1 of the table exchanged (H = 12 and 16):
    the majority of the valid query rows is rejected, not one element"""
    c = _rehearsal()
    ok, worst = _share_rejected(c)
    assert ok == 0.0 and worst <= 1.0
    planted = [("gate of layer 0's parameters", c, dict(gate=c["gates64"][0])),
               ("table shifted by one offset", c, dict(table=wc.table_shifted(c["rel"], c["R"]))),
               ("table heads 0 / 1 exchanged, H = 12", c, dict(table=wc.table_heads_swapped(c["table"])))]
    c16 = _rehearsal(16)
    assert _share_rejected(c16)[0] == 0.0
    planted.append(("table heads 0 / 1 exchanged, H = 16", c16, dict(table=wc.table_heads_swapped(c16["table"]))))
    for tag, cc, kw in planted:
        share, worst = _share_rejected(cc, **kw)
        print(f"WAVLM|rehearsal sensitivity|{tag}|rows rejected {share:.3f}|max error / bound {worst:.3g}")
        assert share > 0.5, (tag, share)


def test_rehearsal_rejects_a_removed_key():
    c = _rehearsal()
    b, v, q = 0, wc.STAGE_VALID[0], 140
    f = c["ref"][b]
    key = wc.likeliest_key(f, q, 128, v)                  # the last key tile of 150 valid keys
    g = wc.segment_attention_ref(c["qk"], c["vt"], c["gates"][1], c["table"], c["r0"][b], c["pitch"][b], v, c["H"], 0.125, drop_key=key)
    assert torch.equal(g["out"][:, :q], f["out"][:, :q]) and not torch.equal(g["out"][key[0], q], f["out"][key[0], q])
    rej = wc.rows_rejected(c["emu"][b], g["out"], g["bound"])
    ratio = float(((c["emu"][b].double() - g["out"]).abs() / g["bound"])[key[0], q].max())
    print(f"WAVLM|rehearsal sensitivity|key {key[2]} (p = {float(f['P'][key]):.3f}) removed from query {q} head {key[0]}|error / bound {ratio:.3g}")
    assert bool(rej[q]) and int(rej.sum()) == 1


def test_rehearsal_gate_criterion_rejects_the_wrong_rows():
    """the gate taken from x where the encoder takes it from LayerNorm(x) (wavlm_large): test_gate_kernel's criterion sees it, and
    passes the fp32 evaluation of the right rows"""
    c = _rehearsal()
    p = c["gate_params"][0]
    g = torch.Generator().manual_seed(9)
    hidden = (c["x"].float() * (2.0 + 0.5 * torch.randn(c["D"], generator=g)) + 0.3 * torch.randn(c["D"], generator=g)).to(torch.bfloat16)
    ln = torch.nn.functional.layer_norm(hidden.float(), (c["D"],)).to(torch.bfloat16)
    got = wc.gate_ref(ln.float(), *p, c["H"]) * (1.0 + 2.0 ** -23)             # a stand-in kernel: fp32, one rounding off
    right, yard = wc.gate_ref(ln.double(), *p, c["H"]), wc.gate_ref(ln.float(), *p, c["H"])
    assert not wc.gate_criterion_rejects(got, right, yard)[0]
    wrong, wyard = wc.gate_ref(hidden.double(), *p, c["H"]), wc.gate_ref(hidden.float(), *p, c["H"])
    bad, lines = wc.gate_criterion_rejects(got, wrong, wyard)
    assert bad, lines


@pytest.mark.parametrize("typ", ["s3prl_plus", "FairseqHubert"])
def test_model_builds_from_a_wavlm_config(typ):
    cfg = base_parallel_config()
    cfg.audio_encoder.type, cfg.audio_encoder.name = typ, "wavlm_base"
    m = KWClip_GeneralTransformer(cfg, device="cpu")
    enc = m.audio_encoder
    assert isinstance(enc, se.S3prlSpeechEncoderPlus if typ == "s3prl_plus" else se.FairseqSpeechEncoder_Hubert)
    assert enc.out_dim == 768 and enc.downsample_rate == 320 and enc.upstream_model_hiddenstates_len == 13
    assert enc.arch.rel_pos_buckets == 320 and enc._w["rel_embed"].shape == (320, 12)
    assert [p.shape for p in enc.trainable_params()] == [torch.Size([13])]          # the weighted-sum weights alone
