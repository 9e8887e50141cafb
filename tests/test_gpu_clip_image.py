"""The frozen CLIP image tower on the GPU (speechclip_plus_amd/clip_image.py, csrc/vit.hip, the QuickGELU GEMM epilogue, the layer
driver's ffn_act).  Bounds fixed before any run (derivations in docs/parity.md, "CLIP image tower"):
  QuickGELU epilogue   every tile family bitwise equal; against bf16(quickgelu(fp32 GEMM output + bias)) - the library's own fp32
                       output of the same product (act = 0, out_f32), so that the accumulation is common and only the epilogue is
                       compared - every difference <= 1 bf16 ulp, in <= 1 % of the elements
  layer driver         sc_hubert_layer_fwd(pre_ln = 1, ffn_act = 2, seg) bitwise equal to the same entry points issued one by one
  patchify             bitwise equal to torch unfold -> permute -> bf16 (zero class / pad rows and K-pad columns)
  embed + ln_pre       <= 1 bf16 ulp per element against fp32 torch layer_norm(gemm + pos), plus the fp32 rounding of the affine
                       terms (2^-21 (|gamma xhat| + |beta|)) where gamma xhat and beta cancel; the plain 1-ulp bound fails on at most
                       1e-4 of the elements
  HF fixtures          rel-L2 < 2e-2 on image_embeds and on the non-pad rows of the last hidden state
  full size            rel-L2 < 2e-2 per embedding, cosine >= 0.999 per image, all finite, against the fp32 restatement below
  model level          pixels through the tower == the tower's embeddings passed as batch["image"], bitwise"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SMALL = dict(width=128, layers=2, heads=2, resolution=224, embed_dim=64)


def openai_vit_fp32(m, pixels: torch.Tensor, dtype=torch.float32):
    """Restatement of openai/CLIP's VisionTransformer.forward (conv1 -> class token + positional embedding -> ln_pre -> pre-LN
    residual blocks with QuickGELU MLPs -> ln_post on the class row -> @ proj) in plain torch at ``dtype`` on the pixels' device,
    from ClipImageEncoder ``m``'s parameters.  -> (embeddings [B, E], last block's output [B, tokens, W])."""
    dev = pixels.device
    p = {k: v.detach().to(device=dev, dtype=dtype) for k, v in m.state_dict().items()}
    x = pixels.to(dtype)
    B, W, H = x.shape[0], m.width, m.heads
    x = F.conv2d(x, p["conv1.weight"], stride=m.patch).reshape(B, W, -1).permute(0, 2, 1)
    x = torch.cat([p["class_embedding"].expand(B, 1, W), x], dim=1) + p["positional_embedding"]
    x = F.layer_norm(x, (W,), p["ln_pre.weight"], p["ln_pre.bias"], 1e-5)
    T = x.shape[1]
    for i in range(len(m.transformer.resblocks)):
        q = lambda n: p[f"transformer.resblocks.{i}.{n}"]
        h = F.layer_norm(x, (W,), q("ln_1.weight"), q("ln_1.bias"), 1e-5)
        qkv = (h @ q("attn.in_proj_weight").t() + q("attn.in_proj_bias")).view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
        att = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * 0.125, dim=-1) @ qkv[2]
        x = x + att.permute(0, 2, 1, 3).reshape(B, T, W) @ q("attn.out_proj.weight").t() + q("attn.out_proj.bias")
        h = F.layer_norm(x, (W,), q("ln_2.weight"), q("ln_2.bias"), 1e-5)
        u = h @ q("mlp.c_fc.weight").t() + q("mlp.c_fc.bias")
        x = x + (u * torch.sigmoid(1.702 * u)) @ q("mlp.c_proj.weight").t() + q("mlp.c_proj.bias")
    y = F.layer_norm(x[:, 0], (W,), p["ln_post.weight"], p["ln_post.bias"], 1e-5)
    return y @ p["proj"], x


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bf16_ulp(ref: torch.Tensor) -> torch.Tensor:
    """spacing of bf16 at the value (8 significant bits)"""
    return ref.double().abs().clamp(min=2.0 ** -126).log2().floor().exp2() * 2.0 ** -7


def _ops():
    from speechclip_plus_amd import ops
    return ops


def _pixels(fx, dev):
    from speechclip_plus_amd.clip_image import CLIP_IMAGE_MEAN, CLIP_IMAGE_STD
    img = torch.from_numpy(fx["images"]).float() / 255.0
    return ((img - torch.tensor(CLIP_IMAGE_MEAN).view(1, 3, 1, 1)) / torch.tensor(CLIP_IMAGE_STD).view(1, 3, 1, 1)).to(dev)


# ---------------------------------------------------------------------------------------------------- QuickGELU GEMM epilogue
@pytest.mark.parametrize("M,N,K,res,tiles", [
    (16896, 4096, 1024, False, (0, 1, 2, 3, 7, 8, 13, 14, 15)),     # ViT-L/14 fc1 at B = 64 (auto: the 256-row tile)
    (1733, 776, 1536, True, (0, 1, 2, 3, 7, 8, 13, 14, 15)),        # tails in every tile size, with a residual
    (300, 64, 1024, False, (0, 1, 3, 13, 14, 15)),                   # few rows, narrow output (auto: 64 x 64 / 128 x 64)
])
def test_quickgelu_epilogue_every_tile_family(M, N, K, res, tiles):
    ops = _ops()
    dev = "cuda"
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    W = (torch.randn(N, K, generator=g) * (2.0 / K) ** 0.5).to(torch.bfloat16).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    R = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev) if res else None
    first = None
    for t in tiles:
        C = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        ops.gemm_raw(A, K, W, K, C, N, M, N, K, bias=bias, residual=R, ldr=N if res else 0, act=2, tile=t)
        if first is None:
            first = C
        else:
            assert torch.equal(C, first), f"tile {t} differs from tile {tiles[0]}"
    # the fp32 GEMM output + bias of the same accumulation (tile-independent: the cross-tile equality above).  Against an independently
    # accumulated product the bound cannot hold where the pre-activation cancels to |u| ~ 1e-6: fp32 sums of K = 1024 terms differ from
    # the exact sum by up to ~8e-6 in torch and in the kernel alike (docs/parity.md)
    u = torch.empty(M, N, device=dev, dtype=torch.float32)
    ops.gemm_raw(A, K, W, K, u, N, M, N, K, bias=bias, act=0, out_f32=True)
    ref = u * torch.sigmoid(1.702 * u)
    if res:
        ref = ref + R.float()
    ref_bf = ref.to(torch.bfloat16)
    d = (first.double() - ref_bf.double()).abs()
    ulp = bf16_ulp(ref)
    assert bool((d <= ulp).all()), float((d / ulp).max())
    frac = float((d > 0).double().mean())
    assert frac <= 0.01, frac
    # and the product itself against torch's fp32 GEMM: bf16 storage only
    ut = A.float() @ W.float().t() + bias
    rt = ut * torch.sigmoid(1.702 * ut) + (R.float() if res else 0.0)
    assert rel_l2(first, rt) < 4e-3, rel_l2(first, rt)
    # not the identity and not the erf-GELU: the activation really is applied
    plain = ops.linear_bf16(A[:64], W, bias, act=0)
    assert not torch.equal(plain, first[:64]) or res


def test_quickgelu_refused_where_it_is_not_built():
    ops = _ops()
    A = torch.zeros(256, 64, device="cuda", dtype=torch.bfloat16)
    W = torch.zeros(256, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="dropout"):
        ops.linear_bf16(A, W, act=2, drop_p=0.1, drop_seed=1)
    with pytest.raises(RuntimeError, match="act"):
        ops.linear_bf16(A, W, act=5)


# ---------------------------------------------------------------------------------------------------- layer driver
@pytest.mark.parametrize("name,B", [("ViT-B/32", 5), ("ViT-L/14", 3)])
def test_layer_driver_quickgelu_matches_op_by_op(name, B):
    ops = _ops()
    from speechclip_plus_amd.clip_image import ClipImageEncoder
    m = ClipImageEncoder(name, layers=1, seed=5).cuda()
    dev = torch.device("cuda")
    w = m._weights(dev)
    seg, vl = m.segments(B, dev)
    D, F_, H, rows = m.width, 4 * m.width, m.heads, seg.rows
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(rows, D, generator=g).to(torch.bfloat16).to(dev)
    out = torch.empty_like(x)
    from types import SimpleNamespace
    # qk and vt with the zeroed slack the attention tiles read behind the last image (SC_ATTN_SLACK rows / elements)
    slack_qk = lambda: torch.zeros(rows + 64, 2 * D, device=dev, dtype=torch.bfloat16)[:rows]
    slack_vt = lambda: torch.zeros(rows * D + 64, device=dev, dtype=torch.bfloat16)[: rows * D].view(rows, D)
    pl = SimpleNamespace(qk=slack_qk(), vt=slack_vt(),
                         ctx=torch.empty(rows, D, device=dev, dtype=torch.bfloat16), pre=torch.empty(rows, D, device=dev, dtype=torch.bfloat16),
                         x1=torch.empty(rows, D, device=dev, dtype=torch.bfloat16), ffn=torch.empty(rows, F_, device=dev, dtype=torch.bfloat16))
    ops.hubert_layer_fwd(x, out, vl, w, 0, pl, B, m.pitch, m.tokens, D, F_, H, pre_ln=True, seg=seg, ffn_act=2)
    # the same entry points, one by one
    x1 = ops.layernorm_bf16(x, w["l0_ln1_g"], w["l0_ln1_b"])
    qk, vt = slack_qk(), slack_vt()
    ops.gemm_raw(x1, D, w["l0_qkv_w"], D, qk, 2 * D, rows, 3 * D, D, bias=w["l0_qkv_b"], Ct=vt, n_split=2 * D, R=m.pitch, dh=64, seg=seg)
    ctx = torch.empty(rows, D, device=dev, dtype=torch.bfloat16)
    ops.attn_fwd(qk, vt, vl, ctx, B, m.pitch, H, D, 0.125, seg=seg)
    pre = ops.linear_bf16(ctx, w["l0_o_w"], w["l0_o_b"], residual=x)
    x2 = ops.layernorm_bf16(pre, w["l0_ln2_g"], w["l0_ln2_b"])
    ffn = ops.linear_bf16(x2, w["l0_fc1_w"], w["l0_fc1_b"], act=2)
    ref = ops.linear_bf16(ffn, w["l0_fc2_w"], w["l0_fc2_b"], residual=pre)
    real = torch.cat([torch.arange(b * m.pitch, b * m.pitch + m.tokens) for b in range(B)]).to(dev)
    assert torch.equal(out[real], ref[real])
    assert torch.equal(pl.ffn[real], ffn[real])                       # the FC1 output of the driver is the QuickGELU one
    assert bool(torch.isfinite(out[real].float()).all())
    # ffn_act outside {0, 2}, and QuickGELU with the LayerNorm-folded form, are refused
    with pytest.raises(RuntimeError, match="ffn_act"):
        ops.hubert_layer_fwd(x, out, vl, w, 0, pl, B, m.pitch, m.tokens, D, F_, H, pre_ln=True, seg=seg, ffn_act=1)


# ---------------------------------------------------------------------------------------------------- patchify / embed + ln_pre
def _expected_patches(img, P, pitch, Kp):
    B, _, S, _ = img.shape
    gg = (S // P) ** 2
    pt = img.unfold(2, P, P).unfold(3, P, P).permute(0, 2, 3, 1, 4, 5).reshape(B, gg, 3 * P * P)
    A = torch.zeros(B, pitch, Kp, device=img.device, dtype=torch.bfloat16)
    A[:, 1: 1 + gg, : 3 * P * P] = pt.to(torch.bfloat16)
    return A.reshape(B * pitch, Kp)


@pytest.mark.parametrize("name", ["ViT-B/32", "ViT-L/14"])
def test_patchify_bitwise(name):
    ops = _ops()
    from speechclip_plus_amd.clip_image import ClipImageEncoder
    m = ClipImageEncoder(name, layers=1)
    dev = torch.device("cuda")
    B, S = 3, 224
    g = torch.Generator(device="cpu").manual_seed(3)
    seg, _ = m.segments(B, dev)
    views = {"contiguous": torch.randn(B, 3, S, S, generator=g).to(dev),
             "batch stride": torch.randn(2 * B, 3, S, S, generator=g).to(dev)[::2],
             "channel slice": torch.randn(B, 5, S, S, generator=g).to(dev)[:, 1:4],
             "row pitch": torch.randn(B, 3, S, S + 24, generator=g).to(dev)[..., 8: 8 + S]}
    for what, img in views.items():
        A = ops.vit_patchify(img, seg, m.patch, m.Kp)
        assert torch.equal(A, _expected_patches(img.contiguous(), m.patch, m.pitch, m.Kp)), what


@pytest.mark.parametrize("W,P", [(768, 32), (1024, 14), (128, 14)])
def test_embed_ln_pre_within_one_ulp(W, P):
    ops = _ops()
    from speechclip_plus_amd.clip_image import ClipImageEncoder
    m = ClipImageEncoder("t", width=W, layers=1, heads=W // 64, patch=P, resolution=224, embed_dim=64)
    dev = torch.device("cuda")
    B = 5
    seg, _ = m.segments(B, dev)
    g = torch.Generator(device="cpu").manual_seed(W + P)
    G = (torch.randn(seg.rows, W, generator=g) * 2.0 + 0.5).to(dev)
    cls, pos = torch.randn(W, generator=g).to(dev), (torch.randn(m.tokens, W, generator=g) * 0.3).to(dev)
    gamma, beta = (1.0 + 0.2 * torch.randn(W, generator=g)).to(dev), (0.1 * torch.randn(W, generator=g)).to(dev)
    X = ops.vit_embed_ln(G, cls, pos, gamma, beta, seg).view(B, m.pitch, W)
    e = G.view(B, m.pitch, W)[:, : m.tokens].double().clone()
    e[:, 0] = cls.double()
    e = e + pos.double()
    ref = F.layer_norm(e.float(), (W,), gamma, beta, 1e-5)
    d = (X[:, : m.tokens].double() - ref.double()).abs()
    ulp = bf16_ulp(ref)
    # near y = 0 the two fp32 evaluations of gamma xhat + beta differ by their own rounding, more than a bf16 ulp of the tiny result
    xhat = F.layer_norm(e.float(), (W,), None, None, 1e-5).double()
    fp32_terms = 2.0 ** -21 * ((xhat * gamma.double()).abs() + beta.double().abs())
    assert bool((d <= ulp + fp32_terms).all()), float(((d - fp32_terms) / ulp).max())
    assert float((d > ulp).double().mean()) <= 1e-4, float((d > ulp).double().mean())
    assert bool((X[:, m.tokens:] == 0).all())


# ---------------------------------------------------------------------------------------------------- whole tower
@pytest.mark.parametrize("patch", [32, 14])
def test_hf_fixture(golden, patch):
    from speechclip_plus_amd.clip_image import ClipImageEncoder
    fx = golden(f"clip_vision_p{patch}.npz")
    m = ClipImageEncoder("fixture", patch=patch, **SMALL)
    m.load_reference_state_dict({k[2:]: torch.from_numpy(fx[k].astype("float32") * fx["S_" + k[2:]]) for k in fx if k.startswith("Q_")})
    m = m.cuda()
    pix = _pixels(fx, "cuda")
    emb = m(pix)
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (4, 64)
    ref_e = torch.from_numpy(fx["image_embeds"])
    assert rel_l2(emb, ref_e) < 2e-2, rel_l2(emb, ref_e)
    X, seg = m.encode_hidden(pix)
    hid = X.view(4, m.pitch, m.width)[:, : m.tokens]
    ref_h = torch.from_numpy(fx["last_hidden_state"]).float()
    assert rel_l2(hid, ref_h) < 2e-2, rel_l2(hid, ref_h)
    assert torch.equal(m(pix), emb)                                   # cached weights / tables: the same bits again


@pytest.fixture(scope="module", params=["ViT-B/32", "ViT-L/14"])
def full_tower(request):
    from speechclip_plus_amd.clip_image import ClipImageEncoder
    return ClipImageEncoder(request.param, seed=2024).cuda()


@pytest.mark.parametrize("B", [8, 1, 65])
def test_full_size_against_fp32_restatement(full_tower, B):
    m = full_tower
    g = torch.Generator(device="cpu").manual_seed(B)
    pix = torch.randn(B, 3, 224, 224, generator=g).cuda()
    emb = m(pix)
    ref, _ = openai_vit_fp32(m, pix)
    assert tuple(emb.shape) == (B, m.embed_dim) and bool(torch.isfinite(emb).all())
    err = ((emb - ref).norm(dim=1) / ref.norm(dim=1)).cpu()
    cos = F.cosine_similarity(emb, ref, dim=1).cpu()
    assert float(err.max()) < 2e-2, (m.name, B, float(err.max()))
    assert float(cos.min()) >= 0.999, (m.name, B, float(cos.min()))


# ---------------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def clip_model():
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict, HubertArch
    sd = random_hubert_state_dict(HubertArch(), seed=7122)
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    torch.manual_seed(7122)
    model = KWClip_GeneralTransformer(cfg, device="cuda:0", hubert_state_dict=sd, image_encoder="clip").eval()
    return model, sd, cfg


def _batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    lens = [8000 - 700 * (b % 3) for b in range(B)]
    wav = torch.zeros(B, 8000)
    for b, l in enumerate(lens):
        wav[b, :l] = torch.randn(l, generator=g) * 0.3
    pix = torch.randn(B, 3, 224, 224, generator=g)
    return {"wav": wav.cuda(), "wav_len": torch.tensor(lens), "image": pix.cuda(), "id": (torch.arange(B) // 2).cuda()}


def test_model_pixels_equal_embeddings_bitwise(clip_model):
    model, _, _ = clip_model
    from speechclip_plus_amd.clip_image import ClipImageEncoder
    assert isinstance(model.image_encoder, ClipImageEncoder) and model.image_encoder.name == "ViT-B/32"
    assert all(k.startswith("image_encoder.") for k in model.state_dict() if "visual" in k or "conv1" in k)
    assert "image_encoder.proj" in model.state_dict()
    batch = _batch(4, 1)
    with torch.no_grad():
        losses_a, _, others_a = model(batch)
        emb = model.image_encoder(batch["image"])
        losses_b, _, others_b = model(dict(batch, image=emb))
        la, lb = model.compute_loss(losses_a)["loss"], model.compute_loss(losses_b)["loss"]
    assert torch.equal(others_a["image_feat"], others_b["image_feat"])
    assert torch.equal(la, lb) and bool(torch.isfinite(la))
    assert torch.equal(model.forward_image(emb), emb)                # 2-D embeddings still pass through


def test_model_validation_on_pixel_batches(clip_model):
    model, _, _ = clip_model
    outs = [model.validation_step_end(model.validation_step(_batch(6, 10 + i), i)) for i in range(2)]
    rec = model.validation_epoch_end(outs)
    assert rec is not None and all(o["image_feat"].shape == (6, 512) for o in outs)


def test_model_train_step_leaves_the_tower_frozen(clip_model):
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict, HubertArch
    from speechclip_plus_amd.train import ContrastiveTrainer
    _, sd, cfg = clip_model
    model = KWClip_GeneralTransformer(cfg, device="cuda:0", hubert_state_dict=sd, image_encoder="clip").train()
    tower = list(model.image_encoder.parameters())
    ids = {id(p) for p in tower}
    assert not any(id(p) in ids for p in model.getTrainableParams())
    before = [p.detach().clone() for p in tower]
    trainer = ContrastiveTrainer(model)
    loss = trainer.step(_batch(4, 3)).item()
    assert loss == loss
    assert all(p.grad is None and not p.requires_grad for p in tower)
    assert all(torch.equal(a, p) for a, p in zip(before, tower))


def test_from_reference_checkpoint_loads_the_visual_weights(clip_model):
    from speechclip_plus_amd import KWClip_GeneralTransformer
    from speechclip_plus_amd.clip_image import ClipImageEncoder
    model, sd, cfg = clip_model
    src = ClipImageEncoder("ViT-B/32", seed=99).cuda()              # a tower different from the model's own
    ck = {("audio_encoder.encoder." + k): v for k, v in sd.items()}
    ck.update({k: v for k, v in model.state_dict().items() if not k.startswith(("audio_encoder.encoder.", "image_encoder."))})
    ck.update({"clip.model.visual." + k: v for k, v in src.state_dict().items()})
    m2 = KWClip_GeneralTransformer.from_reference_checkpoint(cfg, ck, device="cuda:0", image_encoder="clip").eval()
    rep = m2._reference_load_report
    assert {"clip.model.visual." + k for k in src.state_dict()} <= set(rep["loaded"])
    assert not any(k.startswith("image_encoder.") for k in rep["not_in_checkpoint"])
    pix = _batch(3, 5)["image"]
    assert torch.equal(m2.image_encoder(pix), src(pix))
    # the default path still drops the visual keys
    m3 = KWClip_GeneralTransformer.from_reference_checkpoint(cfg, ck, device="cuda:0")
    assert m3.image_encoder is None and not any(k.startswith("clip.model.visual.") for k in m3._reference_load_report["loaded"])
