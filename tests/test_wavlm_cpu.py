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
