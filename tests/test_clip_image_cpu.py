"""CPU checks of the CLIP image tower (speechclip_plus_amd/clip_image.py): parameter names and shapes, the fixtures' weights and the
reference checkpoint's key map, the patch-GEMM padding, the FLOP count, input validation before any launch, the layer driver's
ctypes struct - and the fp32 restatement the GPU tests compare against, checked here against transformers' implementation."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from speechclip_plus_amd.clip_image import CLIP_IMAGE_ARCHS, CLIP_IMAGE_MEAN, CLIP_IMAGE_STD, ClipImageEncoder, patch_k
from test_gpu_clip_image import openai_vit_fp32

SMALL = dict(width=128, layers=2, heads=2, resolution=224, embed_dim=64)


def _fixture(patch):
    return dict(np.load(os.path.join(GOLDEN, f"clip_vision_p{patch}.npz")))


def _fixture_weights(fx):
    """int8 grid values times their power-of-two scale (tests/golden/make_golden_vision.py): exactly the weights transformers ran"""
    return {k[2:]: torch.from_numpy(fx[k].astype(np.float32) * fx["S_" + k[2:]]) for k in fx if k.startswith("Q_")}


def _pixels(fx):
    img = torch.from_numpy(fx["images"]).float() / 255.0
    return (img - torch.tensor(CLIP_IMAGE_MEAN).view(1, 3, 1, 1)) / torch.tensor(CLIP_IMAGE_STD).view(1, 3, 1, 1)


@pytest.mark.parametrize("name", ["ViT-B/32", "ViT-L/14"])
def test_state_dict_names_and_shapes(name):
    a = CLIP_IMAGE_ARCHS[name]
    W, L, P, E = a["width"], a["layers"], a["patch"], a["embed_dim"]
    g = 224 // P
    m = ClipImageEncoder(name, layers=1)          # one block: the names and shapes of every block are the same
    sd = m.state_dict()
    want = {"conv1.weight": (W, 3, P, P), "class_embedding": (W,), "positional_embedding": (1 + g * g, W), "ln_pre.weight": (W,),
            "ln_pre.bias": (W,), "ln_post.weight": (W,), "ln_post.bias": (W,), "proj": (W, E)}
    blk = {"attn.in_proj_weight": (3 * W, W), "attn.in_proj_bias": (3 * W,), "attn.out_proj.weight": (W, W), "attn.out_proj.bias": (W,),
           "ln_1.weight": (W,), "ln_1.bias": (W,), "mlp.c_fc.weight": (4 * W, W), "mlp.c_fc.bias": (4 * W,),
           "mlp.c_proj.weight": (W, 4 * W), "mlp.c_proj.bias": (W,), "ln_2.weight": (W,), "ln_2.bias": (W,)}
    want.update({f"transformer.resblocks.0.{k}": v for k, v in blk.items()})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert all(not p.requires_grad for p in m.parameters())
    assert m.heads * 64 == W and m.tokens == 1 + g * g and L == {"ViT-B/32": 12, "ViT-L/14": 24}[name]
    full = ClipImageEncoder(name) if name == "ViT-B/32" else None
    if full is not None:
        assert len(full.transformer.resblocks) == 12 and sum(p.numel() for p in full.parameters()) == 87849216


def test_pitch_and_patch_k_padding():
    assert patch_k(32) == 3072 and patch_k(14) == 640 and patch_k(16) == 768
    b32, l14 = ClipImageEncoder("ViT-B/32", layers=1), ClipImageEncoder("ViT-L/14", layers=1)
    assert (b32.tokens, b32.pitch, b32.Kp) == (50, 56, 3072)
    assert (l14.tokens, l14.pitch, l14.Kp) == (257, 264, 640)
    for P in range(1, 40):
        k = patch_k(P)
        assert k % 64 == 0 and 3 * P * P <= k < 3 * P * P + 64


@pytest.mark.parametrize("patch", [32, 14])
def test_fixture_weights_load_strict_and_restatement_matches_transformers(patch):
    """the fixture's openai-named weights load with strict=True, and the fp32 restatement of openai's VisionTransformer (the GPU tests'
    reference) reproduces transformers' CLIPVisionModelWithProjection on them"""
    fx = _fixture(patch)
    m = ClipImageEncoder(f"fixture-p{patch}", patch=patch, **SMALL)
    m.load_reference_state_dict(_fixture_weights(fx))
    for k, v in _fixture_weights(fx).items():
        assert torch.equal(m.state_dict()[k], v), k
    emb, hidden = openai_vit_fp32(m, _pixels(fx).double(), dtype=torch.float64)
    ref_e, ref_h = torch.from_numpy(fx["image_embeds"]).double(), torch.from_numpy(fx["last_hidden_state"]).double()
    assert (emb - ref_e).norm() / ref_e.norm() < 1e-5
    assert (hidden - ref_h).norm() / ref_h.norm() < 1e-3          # the hidden state is stored in fp16 (2^-11 relative per element)
    with pytest.raises(RuntimeError):             # strict: a missing key is refused
        sd = _fixture_weights(fx)
        del sd["proj"]
        m.load_reference_state_dict(sd)


def test_reference_checkpoint_visual_key_map():
    """clip.model.visual.* -> image_encoder.*, nothing else of the checkpoint goes to the tower; the default split is unchanged"""
    from speechclip_plus_amd import KWClip_GeneralTransformer
    fx = _fixture(32)
    ck = {"clip.model.visual." + k: v for k, v in _fixture_weights(fx).items()}
    ck["criterion.temperature"] = torch.tensor(0.07)
    ck["clip.model.logit_scale"] = torch.tensor(4.6)
    hubert, rest = KWClip_GeneralTransformer.split_reference_state_dict(ck)
    assert hubert == {} and set(rest) == {"criterion.temperature"}
    m = ClipImageEncoder("fixture", patch=32, **SMALL)
    pre = "clip.model.visual."
    m.load_reference_state_dict({k[len(pre):]: v for k, v in ck.items() if k.startswith(pre)})
    assert {"image_encoder." + k for k in m.state_dict()} == {"image_encoder." + k[len(pre):] for k in ck if k.startswith(pre)}


@pytest.mark.parametrize("name", ["ViT-B/32", "ViT-L/14"])
def test_flops_closed_form(name):
    a = CLIP_IMAGE_ARCHS[name]
    W, L, P, E = a["width"], a["layers"], a["patch"], a["embed_dim"]
    n = (224 // P) ** 2
    T = n + 1
    per_image = 2 * n * W * 3 * P * P + L * (2 * T * 12 * W * W + 4 * T * T * W) + 2 * W * E
    m = ClipImageEncoder(name, layers=1)
    m.arch["layers"] = L                       # the FLOP count of the full depth from the one-block container
    for B in (1, 8, 64):
        assert m.flops(B) == pytest.approx(B * per_image, rel=1e-12)
    if name == "ViT-L/14":                     # the issue's estimate: 24 * 24 * 1024^2 * 257 (the block GEMMs) ~ 155 GFLOP per image
        assert 155e9 < m.flops(1) < 165e9


def test_input_validation_before_any_launch():
    m = ClipImageEncoder("ViT-B/32", layers=1)
    with pytest.raises(ValueError):
        m(torch.zeros(3, 224, 224))                      # rank
    with pytest.raises(ValueError):
        m(torch.zeros(2, 1, 224, 224))                   # channels
    with pytest.raises(ValueError, match="interpolate"):
        m(torch.zeros(2, 3, 256, 256))                   # resolution
    with pytest.raises(ValueError, match="interpolate"):
        m(torch.zeros(2, 3, 224, 192))
    with pytest.raises(RuntimeError, match="device tensors only"):
        m(torch.zeros(2, 3, 224, 224))                   # CPU pixels
    with pytest.raises(NotImplementedError, match="forward-only"):
        ClipImageEncoder("ViT-B/32", layers=1, image_encoder_trainable=True)
    with pytest.raises(ValueError):
        ClipImageEncoder("ViT-H/14")


def test_model_builds_the_tower_as_a_frozen_submodule_on_request():
    """KWClip_GeneralTransformer(config, image_encoder="clip"): on the CPU only the construction (the tower's rules are checked on
    the GPU); a recipe asking for a trainable image tower is refused with the reason"""
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config
    cfg = base_parallel_config()
    cfg.clip["image_encoder_trainable"] = True
    with pytest.raises(NotImplementedError, match="forward-only"):
        KWClip_GeneralTransformer(cfg, image_encoder="clip", device="cpu")
    with pytest.raises(ValueError, match="'clip'"):
        KWClip_GeneralTransformer(base_parallel_config(), image_encoder="vit", device="cpu")


def test_layer_args_ffn_act_replaces_reserved():
    """sc_hubert_layer_args: ffn_act sits where the unused `reserved` slot was (right after pre_ln), the struct size is unchanged
    and the C side agrees (sc_sizeof)"""
    from speechclip_plus_amd import _lib
    H = _lib.HubertLayerArgs
    names = [f[0] for f in H._fields_]
    assert "reserved" not in names and names[names.index("pre_ln") + 1] == "ffn_act"
    assert H.ffn_act.offset == H.pre_ln.offset + 4 and H.ffn_act.size == 4
    assert H.ffn_act.offset == 3 * 8 + 7 * 4 and H.qkv_w.offset == H.ffn_act.offset + 4
    assert _lib.lib().sc_sizeof(1) == ctypes.sizeof(H)
    assert _lib.lib().sc_abi_version() == 7
