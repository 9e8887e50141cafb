"""CPU: the split-weight evaluation mode (frozen GEMM weights as bf16 hi + lo, docs/rounds/r09_split_weights.md) - the interleave helper,
the library's argument rules for sc_gemm_args.a_rep / sc_hubert_layer_args.w_split (checked with null device pointers: nothing is
launched), and the constructor keyword / config key / NotImplementedError cases of the host."""
import ctypes

import pytest
import torch

from speechclip_plus_amd import _lib, ops

BK = 64


def _koff(kt, tap_c):
    """K-tile -> first k of the tile, the visiting order of the kernels (csrc/gemm256_bf16.hip: koff)"""
    if tap_c == 0:
        return kt * BK
    c, j = divmod(kt, 3)
    return (0 if j == 0 else (3 - j) * tap_c) + c * BK


def test_split_is_exact_in_fp32_and_carries_16_bits():
    g = torch.Generator().manual_seed(3)
    W = torch.randn(200, 768, generator=g) * 0.05
    ws = ops.split_weight_bf16(W)
    assert ws.dtype == torch.bfloat16 and tuple(ws.shape) == (200, 2 * 768) and ws.is_contiguous()
    t = ws.view(200, 768 // BK, 2, BK)
    hi, lo = t[:, :, 0].reshape(200, 768), t[:, :, 1].reshape(200, 768)
    assert torch.equal(hi, W.to(torch.bfloat16))
    assert torch.equal(lo, (W - hi.float()).to(torch.bfloat16))
    s32 = hi.float() + lo.float()
    assert torch.equal(s32.double(), hi.double() + lo.double())              # W_hi + W_lo == fp32(W_hi + W_lo)
    assert torch.equal(ops.split_weight_sum(ws), s32)
    assert bool(((W.double() - s32.double()).abs() <= 2.0 ** -17 * W.double().abs()).all())


@pytest.mark.parametrize("tap_c", [0, 64])
def test_layout_matches_the_kernels_offsets(tap_c):
    """physical K-tile kt multiplies the A tile at koff(kt / 2) with the W tile at 2 koff(kt / 2) + 64 (kt & 1): hi for even kt, lo for odd"""
    K = 192
    g = torch.Generator().manual_seed(4)
    W = torch.randn(16, K, generator=g)
    ws = ops.split_weight_bf16(W)
    hi = W.to(torch.bfloat16)
    lo = (W - hi.float()).to(torch.bfloat16)
    seen = []
    for kt in range(2 * K // BK):
        ka = _koff(kt // 2, tap_c)
        kw = 2 * ka + (kt & 1) * BK
        assert kw + BK <= 2 * K
        assert torch.equal(ws[:, kw: kw + BK], (lo if kt & 1 else hi)[:, ka: ka + BK]), (tap_c, kt)
        seen.append(ka)
    assert sorted(set(seen)) == [0, 64, 128] and all(seen.count(k) == 2 for k in set(seen))
    if tap_c:
        assert seen == [0, 0, 128, 128, 64, 64]                              # tap 0, tap 2, tap 1


def _gemm_args(**kw):
    a = _lib.GemmArgs()
    a.M, a.N, a.K, a.n_split, a.nb1, a.nb2 = 128, 128, 128, -1, 1, 1
    a.lda, a.ldw, a.ldc = 128, 256, 128                                      # ldw = 2K: what the split form needs
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _gemm_error(**kw):
    L = _lib.lib()
    rc = L.sc_gemm_bf16(ctypes.byref(_gemm_args(**kw)), None)
    assert rc != 0                                                           # null operands: never launched
    return L.sc_last_error().decode()


def test_library_accepts_a_rep_2_and_rejects_the_documented_combinations():
    assert "null operand" in _gemm_error()                                   # the baseline: only the operands are missing
    assert "null operand" in _gemm_error(a_rep=1)
    assert "null operand" in _gemm_error(a_rep=2)                            # a_rep = 2 on its own passes the argument rules
    assert "a_rep=3" in _gemm_error(a_rep=3)
    assert "a_rep=-1" in _gemm_error(a_rep=-1)
    e = _gemm_error(a_rep=2, tn=1)
    assert "a_rep = 2" in e and "TN" in e
    dummy = ctypes.c_void_p(64)                                              # never dereferenced: A / W / C stay null, so nothing is launched
    for field in ("ln_stats", "ln_colsum", "stats_out", "res_stats"):
        e = _gemm_error(a_rep=2, **{field: dummy})
        assert "a_rep = 2" in e and "LayerNorm folding" in e, (field, e)
    e = _gemm_error(a_rep=2, ldw=128)                                        # the [N, K] row stride with the [N, 2K] form
    assert "a_rep = 2" in e and "ldw=128" in e
    assert "null operand" in _gemm_error(a_rep=0, ldw=128)
    e = _gemm_error(a_rep=2, drop_p=0.1)
    assert "a_rep = 2" in e and "dropout" in e
    for tile in (32, 34):
        e = _gemm_error(a_rep=2, tile=tile)
        assert "a_rep = 2" in e and "diagnostic" in e


def test_layer_driver_rejects_w_split_with_fused_ln():
    L = _lib.lib()
    a = _lib.HubertLayerArgs()
    a.fused_ln, a.w_split = 1, 1
    assert L.sc_hubert_layer_fwd(ctypes.byref(a), None) != 0
    e = L.sc_last_error().decode()
    assert "w_split" in e and "fused_ln" in e
    a.fused_ln, a.w_split = 0, 2
    assert L.sc_hubert_layer_fwd(ctypes.byref(a), None) != 0
    assert "w_split=2" in L.sc_last_error().decode()
    a.w_split = 1                                                            # accepted: only the (null) pointers are missing, nothing is launched
    assert L.sc_hubert_layer_fwd(ctypes.byref(a), None) != 0
    assert "null pointer" in L.sc_last_error().decode()


def test_struct_sizes_and_field_slots_unchanged():
    L = _lib.lib()
    assert L.sc_abi_version() == 7
    assert ctypes.sizeof(_lib.GemmArgs) == 312 and L.sc_sizeof(0) == 312      # the parent's sizes
    assert ctypes.sizeof(_lib.HubertLayerArgs) == L.sc_sizeof(1)
    g = [n for n, _ in _lib.GemmArgs._fields_]
    assert "reserved3" not in g and g[g.index("aux_mode") + 1] == "a_rep" and g[g.index("a_rep") + 1] == "seg_chunk"
    h = [n for n, _ in _lib.HubertLayerArgs._fields_]
    assert "reserved2" not in h and h[-1] == "w_split" and h[-2] == "n_attn_work"


def _tiny_arch():
    import dataclasses
    from speechclip_plus_amd import speech_encoder as se
    return dataclasses.replace(se.ARCHS["hubert"], layers=1, embed_dim=128, ffn_dim=256, heads=2, conv_dim=64, pos_conv_groups=2)


def test_constructor_keyword_and_split_forms():
    from speechclip_plus_amd import random_hubert_state_dict
    from speechclip_plus_amd import speech_encoder as se
    a = _tiny_arch()
    sd = random_hubert_state_dict(a, seed=1)
    enc = se.FairseqSpeechEncoder_Hubert("hubert", arch=a, state_dict=sd, device="cpu")
    assert enc.eval_weights == "bf16" and enc._w_split is None and not enc._split_active()
    enc.eval()
    assert not enc._split_active()
    with pytest.raises(ValueError):
        enc.set_eval_weights("split")                                        # the fp32 weights are not kept: they have to be handed over
    with pytest.raises(ValueError):
        se.FairseqSpeechEncoder_Hubert("hubert", arch=a, state_dict=sd, device="cpu", eval_weights="fp32")
    sp = se.FairseqSpeechEncoder_Hubert("hubert", arch=a, state_dict=sd, device="cpu", eval_weights="split")
    assert sp.eval_weights == "split" and not sp._split_active()             # a fresh module is in train mode: untouched
    sp.eval()
    assert sp._split_active()
    sp.train()
    assert not sp._split_active()
    split_keys = [f"conv{i}_w" for i in range(1, 7)] + ["proj_w"] + [f"l0_{n}_w" for n in ("qkv", "o", "fc1", "fc2")]
    for k, v in sp._w.items():
        if k in split_keys:
            s = sp._w_split[k]
            assert s.dtype == torch.bfloat16 and s.shape[0] == v.shape[0] and s.shape[1] == 2 * v.shape[1], k
            assert torch.equal(s.view(s.shape[0], -1, 2, BK)[:, :, 0].reshape(v.shape), v), k      # the hi halves are the bf16 weights
        else:
            assert sp._w_split[k] is v, k                                    # everything else (conv 0, pos_conv, norms, biases) is shared
    fc1 = sd["encoder.layers.0.fc1.weight"]
    assert bool(((ops.split_weight_sum(sp._w_split["l0_fc1_w"]).double() - fc1.double()).abs() <= 2.0 ** -17 * fc1.double().abs()).all())
    enc.set_eval_weights("split", state_dict=sd)                             # the late switch builds the same forms
    assert all(torch.equal(enc._w_split[k], sp._w_split[k]) for k in split_keys)
    enc.set_eval_weights("bf16")
    assert enc.eval_weights == "bf16" and not enc._split_active()


def test_split_refuses_trainable_and_fused_ln(monkeypatch):
    from speechclip_plus_amd import random_hubert_state_dict
    from speechclip_plus_amd import speech_encoder as se
    a = _tiny_arch()
    sd = random_hubert_state_dict(a, seed=1)
    with pytest.raises(NotImplementedError, match="FROZEN"):
        se.FairseqSpeechEncoder_Hubert("hubert", arch=a, state_dict=sd, device="cpu", trainable=True, eval_weights="split")
    with pytest.raises(NotImplementedError, match="FROZEN"):
        se.FairseqSpeechEncoder_Hubert("hubert", arch=a, state_dict=sd, device="cpu", trainable=True, unfreeze_layers=[0], eval_weights="split")
    monkeypatch.setattr(se, "_FUSED_LN", True)
    with pytest.raises(NotImplementedError, match="SC_FUSED_LN"):
        se.FairseqSpeechEncoder_Hubert("hubert", arch=a, state_dict=sd, device="cpu", eval_weights="split")
    enc = se.FairseqSpeechEncoder_Hubert("hubert", arch=a, state_dict=sd, device="cpu")
    with pytest.raises(NotImplementedError, match="SC_FUSED_LN"):
        enc.set_eval_weights("split", state_dict=sd)


def test_config_key_and_model_switch():
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    from speechclip_plus_amd.config import load_config
    a = _tiny_arch()
    sd = random_hubert_state_dict(a, seed=1)
    cfg = base_parallel_config()
    assert "eval_weights" not in cfg.audio_encoder                           # off unless asked for
    cfg.audio_encoder.eval_weights = "split"
    model = KWClip_GeneralTransformer(cfg, device="cpu", hubert_state_dict=sd, hubert_arch=a)
    assert model.audio_encoder.eval_weights == "split" and model.audio_encoder._w_split is not None
    assert model.set_eval_weights("bf16") is model and model.audio_encoder.eval_weights == "bf16"
    model.set_eval_weights("split")
    assert model.eval().audio_encoder._split_active()
    plain = KWClip_GeneralTransformer(base_parallel_config(), device="cpu", hubert_state_dict=sd, hubert_arch=a)
    assert plain.audio_encoder.eval_weights == "bf16"
    plain.set_eval_weights("split", hubert_state_dict=sd)
    assert plain.audio_encoder.eval_weights == "split"
    bad = dict(base_parallel_config())
    bad["audio_encoder"] = dict(bad["audio_encoder"], eval_weights="fp16")
    with pytest.raises(ValueError, match="eval_weights"):
        load_config(bad, allow_synthetic_vocab=True)


@pytest.mark.parametrize("case", ["base_small", "large_small"])
def test_oracle_rehearsal_split_emulation_is_closer_to_fp32(case):
    """d(x) = rms distance of x's weighted-sum features from the fp32 oracle on the small encoders (tests/split_cases.py, committed
    seeds): the emulation with all storage sites + split weights sits closer than the one with bf16 weights - with room (a factor
    1.31 / 1.22) - and both distances are the ones stored for the GPU test."""
    import numpy as np
    import split_cases
    d_split, d_bf16 = split_cases.rehearse(case)
    assert d_split < d_bf16 / 1.15, (d_split, d_bf16)
    fx = np.load(split_cases.FIXTURE)[case]
    assert abs(fx[0] - d_split) <= 1e-3 * d_split and abs(fx[1] - d_bf16) <= 1e-3 * d_bf16, (fx, d_split, d_bf16)
