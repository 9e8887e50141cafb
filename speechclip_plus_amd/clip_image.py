"""Frozen CLIP image tower: normalised pixel batches [B, 3, 224, 224] -> image embeddings [B, E], as ClipModel.encode_image
(avssl/module/clip_official.py:202-211) runs openai/CLIP's VisionTransformer on every train / validation step of the shipped recipes
(``load_image: true``).

Architecture restated from the published model: conv1 (3 -> W, kernel = stride = P, no bias) over the 224 x 224 image, a learned
class embedding in front of the g^2 patches (g = 224 / P), learned positional_embedding [1 + g^2, W], ln_pre, ``layers`` pre-LN
residual blocks [ln_1 -> nn.MultiheadAttention(W, heads) ; ln_2 -> Linear(W, 4W) -> QuickGELU -> Linear(4W, W)], then ln_post on
the class row and ``@ proj`` [W, E].  ViT-B/32: W 768, 12 layers, 12 heads, P 32, E 512; ViT-L/14: W 1024, 24 layers, 16 heads,
P 14, E 768.  Parameter names are openai/CLIP's ``visual.*`` names without the prefix, so a reference checkpoint's
``clip.model.visual.*`` keys load with ``load_reference_state_dict`` (strict).

Forward only (the tower is frozen in every recipe, clip_official.py:116-119), eval mode, entirely on the library's kernels:
patchify (csrc/vit.hip) -> patch GEMM (sc_gemm_bf16, fp32 out) -> class / positional embedding + ln_pre (csrc/vit.hip) -> one
sc_hubert_layer_fwd per block (pre_ln = 1, ffn_act = 2: QuickGELU in the fc1 epilogue) over the images' ragged rows -> the class
rows (sc_rows_gather_bf16) -> ln_post (fp32 row LayerNorm) -> ``@ proj`` (exact-fp32 matrix-pipe GEMM).  The nn modules are
parameter containers with no arithmetic of their own: there is no stock-op or CPU path.

Raw images (a list of uint8 [H, W, 3] images of any size, or a packed ragged batch) are accepted wherever pixels are: CLIP's
resize + centre crop + normalise (ClipModel.prep_image, clip_official.py:153-166) runs on the device (image_prep.py,
csrc/image_prep.hip) and writes the patch GEMM's operand directly; ``prep_image`` returns the fp32 pixels themselves.
"""
import torch
from torch import nn

from ._lib import DEFINES
from .clip_text import ResidualAttentionBlock

CLIP_IMAGE_ARCHS = {"ViT-B/32": dict(width=768, layers=12, heads=12, patch=32, resolution=224, embed_dim=512),
                    "ViT-L/14": dict(width=1024, layers=24, heads=16, patch=14, resolution=224, embed_dim=768)}
CLIP_IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)       # the normalisation of CLIP's published preprocessing
CLIP_IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)
SEG_ROWS = DEFINES["SC_SEG_ROWS"]                            # 8: an image's row pitch is a multiple of this


def patch_k(patch: int) -> int:
    """columns of the patch GEMM's operand: 3 P^2 rounded up to 64 (the GEMM's K granularity; the extra columns are zero)"""
    return (3 * patch * patch + 63) // 64 * 64


class _VisionTransformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(width, heads) for _ in range(layers)])

    def forward(self, x):
        raise RuntimeError("the CLIP image transformer holds parameters only; ClipImageEncoder runs it on the HIP kernels")


class ClipImageEncoder(nn.Module):
    """openai/CLIP ``visual`` (VisionTransformer) of ``name``, frozen.  Without a checkpoint the weights are seeded random.
    ``layers``: a shallower tower of the same width (tests)."""

    def __init__(self, name: str = "ViT-B/32", device=None, seed: int = 1234, image_encoder_trainable: bool = False,
                 layers=None, **arch):
        super().__init__()
        if image_encoder_trainable:
            raise NotImplementedError("image_encoder_trainable = True: the CLIP image tower is built forward-only (frozen in every "
                                      "shipped recipe, clip_official.py:116-119); there is no backward through it")
        if name not in CLIP_IMAGE_ARCHS and not arch:
            raise ValueError(f"unknown CLIP image tower {name!r}: one of {sorted(CLIP_IMAGE_ARCHS)}")
        a = dict(CLIP_IMAGE_ARCHS.get(name, {}))
        a.update(arch)                                       # explicit dimensions (the golden fixtures' small towers)
        if layers is not None:
            a["layers"] = int(layers)
        W, P, S = a["width"], a["patch"], a["resolution"]
        if W % 64 or W // 64 != a["heads"] or S % P:
            raise ValueError(f"CLIP image tower {a}: head_dim must be 64 and the resolution a multiple of the patch size")
        self.name, self.arch = name, a
        self.width, self.heads, self.patch, self.resolution, self.embed_dim = W, a["heads"], P, S, a["embed_dim"]
        self.grid = S // P
        self.tokens = 1 + self.grid ** 2
        self.pitch = (self.tokens + SEG_ROWS - 1) // SEG_ROWS * SEG_ROWS       # 56 (B/32), 264 (L/14)
        self.Kp = patch_k(P)                                                    # 3072 (B/32), 640 (L/14)
        self.conv1 = nn.Conv2d(3, W, kernel_size=P, stride=P, bias=False)
        self.class_embedding = nn.Parameter(torch.empty(W))
        self.positional_embedding = nn.Parameter(torch.empty(self.tokens, W))
        self.ln_pre = nn.LayerNorm(W)
        self.transformer = _VisionTransformer(W, a["layers"], a["heads"])
        self.ln_post = nn.LayerNorm(W)
        self.proj = nn.Parameter(torch.empty(W, a["embed_dim"]))
        self._seed(seed)
        self.requires_grad_(False)
        self._seg_cache = {}
        self._ws_cache = (None, None)            # ((B, device), the blocks' scratch): one batch size at a time, as the encoder's plans
        if device is not None:
            self.to(device)

    def _seed(self, seed: int) -> None:
        """CLIP's published init scales, from one CPU generator (reproducible whatever the global RNG)"""
        g = torch.Generator(device="cpu").manual_seed(seed)
        W, L = self.width, self.arch["layers"]
        attn_std, proj_std, fc_std = W ** -0.5, (W ** -0.5) * ((2 * L) ** -0.5), (2 * W) ** -0.5
        with torch.no_grad():
            self.conv1.weight.copy_(torch.randn(self.conv1.weight.shape, generator=g) * (3 * self.patch ** 2) ** -0.5)
            self.class_embedding.copy_(torch.randn(W, generator=g) * W ** -0.5)
            self.positional_embedding.copy_(torch.randn(self.tokens, W, generator=g) * W ** -0.5)
            self.proj.copy_(torch.randn(W, self.embed_dim, generator=g) * W ** -0.5)
            for ln in [self.ln_pre, self.ln_post] + [m for blk in self.transformer.resblocks for m in (blk.ln_1, blk.ln_2)]:
                ln.weight.copy_(1.0 + 0.05 * torch.randn(W, generator=g))
                ln.bias.copy_(0.02 * torch.randn(W, generator=g))
            for blk in self.transformer.resblocks:
                blk.attn.in_proj_weight.copy_(torch.randn(3 * W, W, generator=g) * attn_std)
                blk.attn.in_proj_bias.copy_(0.02 * torch.randn(3 * W, generator=g))
                blk.attn.out_proj.weight.copy_(torch.randn(W, W, generator=g) * proj_std)
                blk.attn.out_proj.bias.copy_(0.02 * torch.randn(W, generator=g))
                blk.mlp.c_fc.weight.copy_(torch.randn(4 * W, W, generator=g) * fc_std)
                blk.mlp.c_fc.bias.copy_(0.02 * torch.randn(4 * W, generator=g))
                blk.mlp.c_proj.weight.copy_(torch.randn(W, 4 * W, generator=g) * proj_std)
                blk.mlp.c_proj.bias.copy_(0.02 * torch.randn(W, generator=g))

    # ------------------------------------------------------------------------------------------------ checkpoints / cost
    def load_reference_state_dict(self, sd: dict):
        """openai/CLIP ``visual.*`` weights (a reference checkpoint's ``clip.model.visual.*`` keys with that prefix stripped), strict."""
        return self.load_state_dict({k: v for k, v in sd.items()}, strict=True)

    def flops(self, B: int) -> float:
        """algorithmic FLOP of one forward over B images (2 x MACs from the shapes): patch embedding, per block QKV, scores, context,
        out_proj, fc1, fc2 over the real tokens, and the projection of the class rows (norms and activations not counted)"""
        W, T, L, E = self.width, self.tokens, self.arch["layers"], self.embed_dim
        patch = 2.0 * (self.grid ** 2) * W * 3 * self.patch ** 2
        block = 2.0 * T * (3 * W * W + W * W + 8 * W * W) + 2.0 * 2 * T * T * W
        return B * (patch + L * block + 2.0 * W * E)

    # ------------------------------------------------------------------------------------------------ device state
    def _weights(self, dev) -> dict:
        """bf16 GEMM weights (conv1 zero-padded to Kp columns) and fp32 vectors on ``dev``, (re)made when a parameter changes"""
        key = (str(dev), tuple((p.data_ptr(), p._version) for p in self.parameters()))
        if getattr(self, "_hip_key", None) != key:
            bf = lambda t: t.detach().to(device=dev, dtype=torch.bfloat16).contiguous()
            f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
            W = self.width
            c1 = torch.zeros(W, self.Kp, device=dev, dtype=torch.bfloat16)
            c1[:, : 3 * self.patch ** 2] = self.conv1.weight.detach().reshape(W, -1).to(device=dev, dtype=torch.bfloat16)
            w = {"conv1": c1, "cls": f32(self.class_embedding), "pos": f32(self.positional_embedding),
                 "ln_pre_g": f32(self.ln_pre.weight), "ln_pre_b": f32(self.ln_pre.bias),
                 "ln_post_g": f32(self.ln_post.weight), "ln_post_b": f32(self.ln_post.bias), "proj": f32(self.proj)}
            for i, blk in enumerate(self.transformer.resblocks):
                w[f"l{i}_qkv_w"], w[f"l{i}_qkv_b"] = bf(blk.attn.in_proj_weight), f32(blk.attn.in_proj_bias)
                w[f"l{i}_o_w"], w[f"l{i}_o_b"] = bf(blk.attn.out_proj.weight), f32(blk.attn.out_proj.bias)
                w[f"l{i}_fc1_w"], w[f"l{i}_fc1_b"] = bf(blk.mlp.c_fc.weight), f32(blk.mlp.c_fc.bias)
                w[f"l{i}_fc2_w"], w[f"l{i}_fc2_b"] = bf(blk.mlp.c_proj.weight), f32(blk.mlp.c_proj.bias)
                w[f"l{i}_ln1_g"], w[f"l{i}_ln1_b"] = f32(blk.ln_1.weight), f32(blk.ln_1.bias)
                w[f"l{i}_ln2_g"], w[f"l{i}_ln2_b"] = f32(blk.ln_2.weight), f32(blk.ln_2.bias)
            self._hip_weights, self._hip_key = w, key
        return self._hip_weights

    def segments(self, B: int, dev):
        """(RowSegments, valid_len [B] int32) of B images: pitch rows each, every image ``tokens`` keys; cached per (B, device)"""
        from . import ops
        key = (B, str(dev))
        if key not in self._seg_cache:
            seg = ops.RowSegments([self.pitch] * B, [self.tokens] * B, dev)
            self._seg_cache[key] = (seg, torch.full((B,), self.tokens, device=dev, dtype=torch.int32))
        return self._seg_cache[key]

    def check_images(self, images) -> None:
        """the input rules of forward, enforced before any launch"""
        if not isinstance(images, torch.Tensor):
            raise TypeError(f"images must be a tensor, got {type(images)}")
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"images must be [B, 3, {self.resolution}, {self.resolution}], got {tuple(images.shape)}")
        if images.shape[2] != self.resolution or images.shape[3] != self.resolution:
            raise ValueError(f"{self.name} takes {self.resolution} x {self.resolution} images (openai CLIP does not interpolate its "
                             f"positional embedding), got {tuple(images.shape[2:])}")
        if images.shape[0] < 1:
            raise ValueError("empty image batch")
        if not images.is_cuda:
            raise RuntimeError("the CLIP image tower runs on the HIP kernels: device tensors only")

    # ------------------------------------------------------------------------------------------------ raw images
    @staticmethod
    def _is_raw(images) -> bool:
        from .image_prep import RawImageBatch
        return isinstance(images, (list, tuple, RawImageBatch))

    def _raw(self, images):
        """list of raw images / (packed, image_hw) pair / RawImageBatch -> what image_prep.run takes, validated before any launch"""
        from . import image_prep
        if self.resolution != image_prep.N_PX:
            raise ValueError(f"raw-image input is CLIP's {image_prep.N_PX} x {image_prep.N_PX} preprocessing, this tower takes {self.resolution}")
        if isinstance(images, image_prep.RawImageBatch):
            raw = images
        elif isinstance(images, tuple) and len(images) == 2 and isinstance(images[0], torch.Tensor) and images[0].dim() == 1:
            raw = image_prep.RawImageBatch(images[0], images[1])
        else:
            raw = image_prep.as_entries(images)
        dev = self.positional_embedding.device
        if dev.type != "cuda":
            raise RuntimeError("the CLIP image tower runs on the HIP kernels: move it to the device first (raw images are resized there)")
        return raw, dev

    def prep_image(self, images) -> torch.Tensor:
        """ClipModel.prep_image (avssl/module/clip_official.py:153-166): a list of raw images - uint8 [H, W, 3] tensors (host or device),
        numpy arrays, PIL images (any mode: converted to RGB) or paths - or a packed raw batch (image_prep.RawImageBatch) -> fp32
        [B, 3, 224, 224] on the device: bicubic resize of the shorter side to 224, centre crop, /255, normalise, bit for bit what
        Pillow + torch give on the host (csrc/image_prep.hip).  No device synchronisation."""
        from . import image_prep
        raw, dev = self._raw(images)
        with torch.no_grad():
            return image_prep.run(raw, dev, pixels=True)[0]

    # ------------------------------------------------------------------------------------------------ forward
    def encode_hidden(self, images):
        """-> (X [B * pitch, W] bf16: the last block's output rows in the segment layout, segments).  Row b * pitch is image b's class
        token, rows b * pitch + 1 .. + g^2 its patches.  ``images``: normalised pixels [B, 3, S, S] on the device, or raw images (as
        prep_image takes them): those go raw -> the patch GEMM's operand directly, the fp32 image is never formed."""
        from . import ops
        if self._is_raw(images):
            from . import image_prep
            raw, dev = self._raw(images)
            B = len(raw)
            seg, _ = self.segments(B, dev)
            A = image_prep.run(raw, dev, pixels=False, seg=seg, patch=self.patch, Kp=self.Kp)[1]
            return self._encode_patches(A, B, dev)
        self.check_images(images)
        dev = images.device
        x = images if images.dtype == torch.float32 else images.float()
        if x.stride(3) != 1:
            x = x.contiguous()
        seg, _ = self.segments(images.shape[0], dev)
        A = ops.vit_patchify(x, seg, self.patch, self.Kp)
        return self._encode_patches(A, images.shape[0], dev)

    def _encode_patches(self, A: torch.Tensor, B: int, dev):
        """the tower from the patch GEMM's operand A [seg.rows, Kp] bf16 on"""
        from . import ops
        W, F = self.width, 4 * self.width
        w = self._weights(dev)
        seg, valid_len = self.segments(B, dev)
        rows = seg.rows
        G = torch.empty(rows, W, device=dev, dtype=torch.float32)
        ops.gemm_raw(A, self.Kp, w["conv1"], self.Kp, G, W, rows, W, self.Kp, out_f32=True)
        X = ops.vit_embed_ln(G, w["cls"], w["pos"], w["ln_pre_g"], w["ln_pre_b"], seg)
        Y = torch.empty_like(X)
        # the blocks' scratch, kept for the next batch of the same size: behind qk and vt it carries the zeroed slack that the
        # attention tiles read past the last image (tokens 50 / 257 at pitch 56 / 264: key tiles of 64 end 8 / 56 keys behind a row)
        key = (B, str(dev))
        if self._ws_cache[0] != key:
            self._ws_cache = (key, ops.hubert_layer_workspace(rows, W, F, dev))
        pl = self._ws_cache[1]
        for i in range(self.arch["layers"]):
            ops.hubert_layer_fwd(X, Y, valid_len, w, i, pl, B, self.pitch, self.tokens, W, F, self.heads, pre_ln=True, seg=seg, ffn_act=2)
            X, Y = Y, X
        return X, seg

    def forward(self, images) -> torch.Tensor:
        """[B, 3, S, S] normalised pixels on the device, or raw images (a list / packed raw batch, as prep_image takes them) -> fp32
        [B, E] image embeddings (not normalised, as encode_image)"""
        from . import ops
        with torch.no_grad():
            X, seg = self.encode_hidden(images)
            w = self._weights(X.device)
            cls_rows = ops.rows_gather(X, seg.row0[: seg.B])
            y, _, _ = ops.rowln_fwd(cls_rows, None, 0, w["ln_post_g"], w["ln_post_b"], self.ln_post.eps)
            return ops.sgemm_mfma(y, w["proj"], b_kmajor=True)
