"""Fixtures of the CLIP image tower (tests/test_gpu_clip_image.py, tests/test_clip_image_cpu.py) from an independent implementation:
transformers' CLIPVisionModelWithProjection with a local config (no download) and seeded random weights, run in fp32 on the CPU.

Config: hidden 128, 2 heads (head_dim 64), intermediate 512, 2 layers, 224 px, patch 32 / 14, projection 64, quick_gelu, eps 1e-5.
Stored per patch size (clip_vision_p32.npz, clip_vision_p14.npz; compressed, about 0.5 MB each):
  Q_<name>, S_<name> the weights under openai/CLIP's ``visual.*`` names without the prefix (q / k / v concatenated into in_proj_*,
                     proj = visual_projection.weight^T) as int8 values (|Q| <= 15 for matrices, <= 127 for vectors) times a power-of-two
                     scale: weight = float32(Q) * S exactly.
                     The random weights are rounded to that grid BEFORE transformers runs, so the stored form is lossless
  images             uint8 [4, 3, 224, 224]: random 28 x 28 colour grids enlarged 8 x (blocks straddle the 14- and 32-pixel
                     patches); the tests normalise them with CLIP's published mean / std (as here)
  image_embeds       [4, 64] fp32  (un-normalised, = ln_post(class row) @ proj)
  last_hidden_state  [4, tokens, 128] fp16  (the last block's output, before ln_post; fp16 storage: 2^-11 relative)

    python tests/golden/make_golden_vision.py          (seconds on a CPU)
"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


def to_openai(sd: dict, layers: int) -> dict:
    v = "vision_model."
    out = {"class_embedding": sd[v + "embeddings.class_embedding"],
           "conv1.weight": sd[v + "embeddings.patch_embedding.weight"],
           "positional_embedding": sd[v + "embeddings.position_embedding.weight"],
           "ln_pre.weight": sd[v + "pre_layrnorm.weight"], "ln_pre.bias": sd[v + "pre_layrnorm.bias"],
           "ln_post.weight": sd[v + "post_layernorm.weight"], "ln_post.bias": sd[v + "post_layernorm.bias"],
           "proj": sd["visual_projection.weight"].t()}
    for i in range(layers):
        h, o = f"{v}encoder.layers.{i}.", f"transformer.resblocks.{i}."
        out[o + "attn.in_proj_weight"] = torch.cat([sd[h + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)
        out[o + "attn.in_proj_bias"] = torch.cat([sd[h + f"self_attn.{n}_proj.bias"] for n in "qkv"], 0)
        out[o + "attn.out_proj.weight"], out[o + "attn.out_proj.bias"] = sd[h + "self_attn.out_proj.weight"], sd[h + "self_attn.out_proj.bias"]
        out[o + "ln_1.weight"], out[o + "ln_1.bias"] = sd[h + "layer_norm1.weight"], sd[h + "layer_norm1.bias"]
        out[o + "ln_2.weight"], out[o + "ln_2.bias"] = sd[h + "layer_norm2.weight"], sd[h + "layer_norm2.bias"]
        out[o + "mlp.c_fc.weight"], out[o + "mlp.c_fc.bias"] = sd[h + "mlp.fc1.weight"], sd[h + "mlp.fc1.bias"]
        out[o + "mlp.c_proj.weight"], out[o + "mlp.c_proj.bias"] = sd[h + "mlp.fc2.weight"], sd[h + "mlp.fc2.bias"]
    return {k: t.detach().float().contiguous() for k, t in out.items()}


def from_openai(w: dict, layers: int) -> dict:
    """inverse of to_openai: openai names -> the transformers parameters"""
    v = "vision_model."
    out = {v + "embeddings.class_embedding": w["class_embedding"], v + "embeddings.patch_embedding.weight": w["conv1.weight"],
           v + "embeddings.position_embedding.weight": w["positional_embedding"],
           v + "pre_layrnorm.weight": w["ln_pre.weight"], v + "pre_layrnorm.bias": w["ln_pre.bias"],
           v + "post_layernorm.weight": w["ln_post.weight"], v + "post_layernorm.bias": w["ln_post.bias"],
           "visual_projection.weight": w["proj"].t()}
    for i in range(layers):
        h, o = f"{v}encoder.layers.{i}.", f"transformer.resblocks.{i}."
        for n, t in zip("qkv", w[o + "attn.in_proj_weight"].chunk(3, 0)):
            out[h + f"self_attn.{n}_proj.weight"] = t
        for n, t in zip("qkv", w[o + "attn.in_proj_bias"].chunk(3, 0)):
            out[h + f"self_attn.{n}_proj.bias"] = t
        for a, b in (("self_attn.out_proj", "attn.out_proj"), ("layer_norm1", "ln_1"), ("layer_norm2", "ln_2"), ("mlp.fc1", "mlp.c_fc"),
                     ("mlp.fc2", "mlp.c_proj")):
            out[h + a + ".weight"], out[h + a + ".bias"] = w[o + b + ".weight"], w[o + b + ".bias"]
    return out


def quantise(t: torch.Tensor):
    """-> (int8 Q, power-of-two scale S) with float32(Q) * S the nearest grid point to t: |Q| <= 15 for the matrices (they are the bulk
    of the file; 31 levels of a Gaussian keep it random), <= 127 for the vectors (LayerNorm weights near 1 keep their spread)"""
    qmax = 15 if t.dim() >= 2 else 127
    s = 2.0 ** float(np.ceil(np.log2(float(t.abs().max()) / qmax)))
    return torch.round(t / s).clamp(-qmax, qmax).to(torch.int8), np.float32(s)


def fixture_weights(fx: dict) -> dict:
    """the stored weights as fp32 tensors under openai's names (what the tests load)"""
    return {k[2:]: torch.from_numpy(fx[k].astype(np.float32) * fx["S_" + k[2:]]) for k in fx if k.startswith("Q_")}


def make(patch: int, seed: int) -> None:
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    layers = 2
    cfg = CLIPVisionConfig(hidden_size=128, intermediate_size=512, num_attention_heads=2, num_hidden_layers=layers, image_size=224,
                           patch_size=patch, projection_dim=64, hidden_act="quick_gelu", layer_norm_eps=1e-5, num_channels=3)
    model = CLIPVisionModelWithProjection(cfg).eval()
    with torch.no_grad():               # the default init leaves LayerNorms at (1, 0) and biases at 0: move every parameter off it
        for name, p in model.named_parameters():
            if "norm" in name or name.endswith("bias"):
                p.add_(0.05 * torch.randn_like(p))
            elif "embedding" in name:
                p.mul_(10.0)            # initializer_range 0.02 puts the embeddings far below the patch term
    w = to_openai(model.state_dict(), layers)
    qs = {k: quantise(t) for k, t in w.items()}
    grid = {k: q.float() * torch.tensor(s) for k, (q, s) in qs.items()}
    missing, unexpected = model.load_state_dict(from_openai(grid, layers), strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    g = torch.Generator().manual_seed(seed + 1)
    small = torch.randint(0, 256, (4, 3, 28, 28), generator=g, dtype=torch.uint8)
    images = small.repeat_interleave(8, dim=2).repeat_interleave(8, dim=3).contiguous()
    pix = (images.float() / 255.0 - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    with torch.no_grad():
        out = model(pixel_values=pix)
    fx = {}
    for k, (q, s) in qs.items():
        fx["Q_" + k], fx["S_" + k] = q.numpy(), np.asarray(s, dtype=np.float32)
    assert all(torch.equal(fixture_weights(fx)[k], grid[k]) for k in grid)
    fx["images"] = images.numpy()
    fx["image_embeds"] = out.image_embeds.float().numpy()
    fx["last_hidden_state"] = out.last_hidden_state.numpy().astype(np.float16)
    path = os.path.join(HERE, f"clip_vision_p{patch}.npz")
    np.savez_compressed(path, **fx)
    print(os.path.basename(path), os.path.getsize(path), "bytes",
          {k: v.shape for k, v in fx.items() if not k.startswith(("Q_", "S_"))})


if __name__ == "__main__":
    make(32, 32)
    make(14, 14)
