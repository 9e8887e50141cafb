"""Raw-image input on the GPU (speechclip_plus_amd/image_prep.py, csrc/image_prep.hip): CLIP's resize + crop + normalise on the device.
Everything here is held to EQUALITY - Pillow's 8-bit resampling is integer arithmetic and the normalisation is a table look-up:
  prep_image      == image_prep.reference_transform element for element, == the Pillow-made digests of tests/golden/image_prep.json,
                  and the same bits for a ragged batch of all cases as for each case alone
  operand A       the raw path's patch-GEMM operand == vit_patchify(prep_image(...)) bitwise, P = 32 and P = 14, zero pad rows / columns
  embeddings      forward(list) == forward(prep_image(list)) == model.forward_image(list) bitwise
  confinement     sentinels between the sources, a pre-filled intermediate and guard words behind every output stay as they were
  batch route     collate_general -> transfer_batch_to_device -> model.forward gives the tensor route's image_feat bitwise"""
import numpy as np
import pytest
import torch

from image_prep_cases import CASES, load_fixture, reference, sha256, source

pytestmark = pytest.mark.gpu

SMALL = dict(width=128, layers=2, heads=2, resolution=224, embed_dim=64)
EVERY = list(range(len(CASES)))
SOME = [0, 1, 3, 4, 5, 6, 8]                 # down- and upscale, both half-way crops, no pass, crop only: the embedding / route tests


def _images(idx):
    return [torch.from_numpy(source(i).copy()) for i in idx]


def _want_pixels(idx):
    return torch.from_numpy(np.stack([reference(i)[1] for i in idx]))


@pytest.fixture(scope="module")
def towers():
    from speechclip_plus_amd.clip_image import ClipImageEncoder
    return {32: ClipImageEncoder("ViT-B/32", layers=1, seed=5).cuda(), 14: ClipImageEncoder("fixture-p14", patch=14, seed=6, **SMALL).cuda()}


@pytest.fixture(scope="module")
def all_pixels(towers):
    """prep_image of every case as ONE ragged batch (shared, left unchanged)"""
    return towers[32].prep_image(_images(EVERY))


def test_prep_image_equals_the_twin_and_the_fixture(all_pixels):
    fx = load_fixture()
    got = all_pixels.cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(CASES), 3, 224, 224) and all_pixels.is_cuda
    want = _want_pixels(EVERY)
    total = 0
    for i, (w, h, kind) in enumerate(CASES):
        bad = torch.nonzero(got[i].view(torch.int32) != want[i].view(torch.int32))
        first = "" if len(bad) == 0 else f", first at (c, y, x) = {bad[0].tolist()}: {got[i][tuple(bad[0])]} != {want[i][tuple(bad[0])]}"
        print(f"case {i} {w} x {h} {kind}: {len(bad)} mismatches of {got[i].numel()}{first}")
        total += len(bad)
    assert total == 0, f"{total} mismatches against image_prep.reference_transform"
    for i in EVERY:
        assert sha256(got[i].numpy()) == fx["cases"][i]["f32_sha256"], f"case {i}: normalised values differ from Pillow + torch's digest"
    # the bytes behind the values (the LUT is injective per channel): Pillow's resized-and-cropped image
    from speechclip_plus_amd.image_prep import norm_lut
    lut = norm_lut()
    for i in EVERY:
        u8 = torch.stack([torch.searchsorted(lut[c].contiguous(), got[i, c].contiguous()) for c in range(3)], dim=-1).to(torch.uint8)
        assert sha256(u8.numpy()) == fx["cases"][i]["u8_sha256"], f"case {i}: resized bytes differ from Pillow {fx['pillow']}'s"


@pytest.mark.parametrize("i", EVERY)
def test_each_case_alone_gives_the_batch_bits(towers, all_pixels, i):
    one = towers[32].prep_image(_images([i]))
    assert tuple(one.shape) == (1, 3, 224, 224) and torch.equal(one[0], all_pixels[i])


def test_input_kinds_give_the_same_bits(towers, all_pixels):
    """numpy arrays, device tensors, PIL images and a packed raw batch on the host or on the device: one result"""
    from speechclip_plus_amd.image_prep import RawImageBatch, pack_host
    idx = [0, 4, 5, 6]
    m, want = towers[32], all_pixels[[0, 4, 5, 6]]
    mixed = [source(0), torch.from_numpy(source(4).copy()).cuda(), torch.from_numpy(source(5).copy()), torch.from_numpy(source(6).copy()).cuda()]
    assert torch.equal(m.prep_image(mixed), want)
    raw = pack_host(_images(idx))
    assert torch.equal(m.prep_image(raw), want)
    assert torch.equal(m.prep_image(RawImageBatch(raw.packed.cuda(), raw.hw)), want)
    try:
        from PIL import Image
    except ImportError:
        return
    assert torch.equal(m.prep_image([Image.fromarray(source(i), "RGB") for i in idx]), want)


@pytest.mark.parametrize("P", [32, 14])
def test_operand_a_equals_patchify_of_the_pixels(towers, all_pixels, P):
    from speechclip_plus_amd import image_prep, ops
    m = towers[P]
    dev = torch.device("cuda", torch.cuda.current_device())
    B = len(CASES)
    seg, _ = m.segments(B, dev)
    assert m.Kp == {32: 3072, 14: 640}[P]
    A = torch.full((seg.rows, m.Kp), float("nan"), device=dev, dtype=torch.bfloat16)          # every element must be written
    pix, A2 = image_prep.run(_images(EVERY), dev, pixels=False, seg=seg, patch=P, Kp=m.Kp, A=A)
    assert pix is None and A2 is A
    want = ops.vit_patchify(all_pixels, seg, P, m.Kp)
    assert torch.equal(A.view(torch.int16), want.view(torch.int16))
    A3 = A.view(B, m.pitch, m.Kp)
    gg = (224 // P) ** 2
    assert not A3[:, 0].any() and not A3[:, 1 + gg:].any() and not A3[:, :, 3 * P * P:].any()
    assert bool((A3[:, 1: 1 + gg, : 3 * P * P] != 0).any())
    # both outputs from one launch: the same bits
    pix, A4 = image_prep.run(_images(SOME), dev, pixels=True, seg=m.segments(len(SOME), dev)[0], patch=P, Kp=m.Kp)
    assert torch.equal(pix, all_pixels[SOME]) and torch.equal(A4.view(torch.int16), ops.vit_patchify(pix, m.segments(len(SOME), dev)[0], P, m.Kp).view(torch.int16))


@pytest.fixture(scope="module")
def model(towers):
    from speechclip_plus_amd import HubertArch, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    torch.manual_seed(7122)
    return KWClip_GeneralTransformer(cfg, device="cuda:0", hubert_state_dict=random_hubert_state_dict(HubertArch(), seed=7122),
                                     image_encoder=towers[32]).eval()


@pytest.mark.parametrize("P", [32, 14])
def test_embeddings_from_raw_images_equal_those_from_the_pixels(towers, all_pixels, model, P):
    m = towers[P]
    imgs = _images(SOME)
    pix = m.prep_image(imgs)
    assert torch.equal(pix, all_pixels[SOME])
    want = m(pix)
    got = m(imgs)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(SOME), m.embed_dim) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    X, seg = m.encode_hidden(imgs)
    assert torch.equal(X.view(torch.int16), m.encode_hidden(pix)[0].view(torch.int16))
    prev = model.image_encoder
    model.image_encoder = m
    try:
        assert torch.equal(model.forward_image(imgs), want)
        assert torch.equal(model.prep_image(imgs), pix)
    finally:
        model.image_encoder = prev


def test_confinement(towers, all_pixels):
    """sentinel bytes between the packed sources (so the sources start at odd offsets), the intermediate pre-filled with 0xAA, guard words
    behind the intermediate and both outputs: the same results, and nothing but the outputs is touched"""
    from speechclip_plus_amd import image_prep
    idx, GAP, GUARD = list(range(10)), 61, 4096
    m = towers[14]
    dev = torch.device("cuda", torch.cuda.current_device())
    parts, offsets, hw, at = [], [], [], 0
    for i in idx:
        parts.append(torch.full((GAP,), 0x5A, dtype=torch.uint8))
        at += GAP
        offsets.append(at)
        parts.append(torch.from_numpy(source(i).copy()).reshape(-1))
        at += parts[-1].numel()
        hw.append(tuple(source(i).shape[:2]))
    parts.append(torch.full((GAP,), 0x5A, dtype=torch.uint8))
    packed_host = torch.cat(parts)
    packed = packed_host.cuda()
    raw = image_prep.RawImageBatch(packed, hw, offsets)
    pl = image_prep.plan(hw, offsets)
    seg, _ = m.segments(len(idx), dev)
    mid_all = torch.full((pl.mid_bytes + GUARD,), 0xAA, dtype=torch.uint8, device=dev)
    out_all = torch.full((len(idx) * 3 * 224 * 224 + GUARD,), -7.0, dtype=torch.float32, device=dev)
    A_all = torch.full((seg.rows * m.Kp + GUARD,), -7.0, dtype=torch.bfloat16, device=dev)
    out = out_all[: len(idx) * 3 * 224 * 224].view(len(idx), 3, 224, 224)
    A = A_all[: seg.rows * m.Kp].view(seg.rows, m.Kp)
    image_prep.run(raw, dev, pixels=True, seg=seg, patch=14, Kp=m.Kp, out=out, A=A, mid=mid_all[: pl.mid_bytes])
    assert torch.equal(out, all_pixels[idx])
    plain = image_prep.run(_images(idx), dev, pixels=False, seg=seg, patch=14, Kp=m.Kp)[1]
    assert torch.equal(A.view(torch.int16), plain.view(torch.int16))
    assert bool((mid_all[pl.mid_bytes:] == 0xAA).all()) and bool((out_all[out.numel():] == -7.0).all()) and bool((A_all[A.numel():] == -7.0).all())
    assert torch.equal(packed.cpu(), packed_host)                           # the sources, sentinels included, are read-only


def test_two_runs_give_identical_bits(towers, all_pixels):
    m = towers[32]
    imgs = _images(EVERY)
    assert torch.equal(m.prep_image(imgs), all_pixels)
    a, b = m(imgs), m(imgs)
    assert torch.equal(a, b)


def test_batch_route_equals_the_tensor_route(towers, model):
    from speechclip_plus_amd.data import collate_general, transfer_batch_to_device
    g = torch.Generator().manual_seed(3)
    idx = SOME[:6]
    lens = [8000 - 700 * (b % 3) for b in range(len(idx))]
    rows = [{"wav": torch.randn(lens[b], generator=g) * 0.3, "image": torch.from_numpy(source(i).copy()), "id": b // 2} for b, i in enumerate(idx)]
    batch = collate_general(rows)
    assert batch["image"].dim() == 1 and batch["image_hw"].tolist() == [list(source(i).shape[:2]) for i in idx]
    on_dev = transfer_batch_to_device(batch, "cuda:0")
    assert on_dev["image"].is_cuda and on_dev["image_hw"].is_cuda and on_dev["image_hw"]._sc_host == batch["image_hw"]._sc_host
    pix = towers[32].prep_image(_images(idx))
    tensor_rows = [dict(r, image=pix[b].cpu()) for b, r in enumerate(rows)]
    on_dev_t = transfer_batch_to_device(collate_general(tensor_rows), "cuda:0")
    assert tuple(on_dev_t["image"].shape) == (len(idx), 3, 224, 224) and "image_hw" not in on_dev_t
    with torch.no_grad():
        _, _, others_raw = model(on_dev)
        _, _, others_t = model(on_dev_t)
    assert tuple(others_raw["image_feat"].shape) == (len(idx), 512) and bool(torch.isfinite(others_raw["image_feat"]).all())
    assert torch.equal(others_raw["image_feat"], others_t["image_feat"])
