"""CPU checks of the raw-image input (speechclip_plus_amd/image_prep.py): the resize / crop geometry and the numpy twin of the kernels
against the Pillow-made fixture (tests/golden/image_prep.json: equality, not a tolerance), the twin against Pillow directly where PIL
imports, the C ABI additions, every validation error before any launch, and the ragged-image packing of collate_general."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from image_prep_cases import CASES, load_fixture, make_source, reference, sha256, source
from speechclip_plus_amd import image_prep
from speechclip_plus_amd.clip_image import CLIP_IMAGE_MEAN, CLIP_IMAGE_STD, ClipImageEncoder
from speechclip_plus_amd.data import collate_general, transfer_batch_to_device

FX = load_fixture()


def test_fixture_covers_the_cases():
    assert [(c["w"], c["h"], c["kind"]) for c in FX["cases"]] == CASES and len(CASES) == 12
    assert FX["pillow"] and FX["n_px"] == 224
    for i, c in enumerate(FX["cases"]):
        assert sha256(source(i)) == c["source_sha256"], f"case {i}: the integer hash made other source pixels than the fixture's"


def test_geometry_equals_the_fixture():
    for c in FX["cases"]:
        assert list(image_prep.clip_resize_geometry(c["w"], c["h"])) == c["geometry"], c
    # the two half-way crops: Python's round goes to even
    assert image_prep.clip_resize_geometry(275, 206) == (299, 224, 38, 0)
    assert image_prep.clip_resize_geometry(61, 46) == (297, 224, 36, 0)
    assert image_prep.clip_resize_geometry(46, 61) == (224, 297, 0, 36)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_reference_transform_reproduces_both_digests(i):
    c = FX["cases"][i]
    u8, f32 = reference(i)
    assert u8.shape == (224, 224, 3) and u8.dtype == np.uint8 and f32.shape == (3, 224, 224) and f32.dtype == np.float32
    assert sha256(u8) == c["u8_sha256"], f"{c['w']} x {c['h']} {c['kind']}: resized bytes differ from Pillow {FX['pillow']}'s"
    assert sha256(f32) == c["f32_sha256"], f"{c['w']} x {c['h']} {c['kind']}: normalised values differ from ToTensor + Normalize"


def test_reference_transform_against_pillow_directly():
    """two sizes that are not in the fixture, element for element"""
    Image = pytest.importorskip("PIL.Image")
    for n, (w, h, kind) in enumerate([(640, 427, "noise"), (97, 211, "blocks")]):
        assert (w, h) not in [(c["w"], c["h"]) for c in FX["cases"]]
        src = make_source(w, h, kind, seed=100 + n)
        out_w, out_h, left, top = image_prep.clip_resize_geometry(w, h)
        want = np.array(Image.fromarray(src, "RGB").resize((out_w, out_h), Image.BICUBIC))[top: top + 224, left: left + 224]
        u8, f32 = image_prep.reference_transform(src)
        bad = np.argwhere(u8 != want)
        assert len(bad) == 0, f"{w} x {h}: {len(bad)} mismatches, first at {bad[0]}: {u8[tuple(bad[0])]} != {want[tuple(bad[0])]}"
        t = torch.from_numpy(want.copy()).permute(2, 0, 1).float().div(255)
        t = t.sub(torch.tensor(CLIP_IMAGE_MEAN).view(3, 1, 1)).div(torch.tensor(CLIP_IMAGE_STD).view(3, 1, 1))
        assert np.array_equal(f32.view(np.uint32), t.numpy().view(np.uint32))


def test_coefficient_tables():
    b, c = image_prep.pil_bicubic_coeffs(500, 298)
    assert b.shape == (298, 2) and c.shape == (298, 9) and b.dtype == np.int32 and c.dtype == np.int32       # ksize = ceil(2 * 500 / 298) * 2 + 1
    assert image_prep.pil_bicubic_coeffs(500, 298)[1] is c                                                   # cached
    assert image_prep.pil_bicubic_coeffs(2001, 224)[1].shape[1] == 37 and image_prep.pil_bicubic_coeffs(3000, 335)[1].shape[1] == 37
    assert image_prep.pil_bicubic_coeffs(46, 224)[1].shape[1] == 5                                           # upscale: support 2
    for n_in, n_out in ((500, 298), (46, 224), (2001, 224), (977, 7059)):
        b, c = image_prep.pil_bicubic_coeffs(n_in, n_out)
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] >= 1).all() and (b[:, 1] <= c.shape[1]).all()
        assert (np.abs(c.sum(axis=1) - (1 << 22)) <= c.shape[1]).all()                                       # a row sums to 1 up to rounding
        for i in (0, n_out // 2, n_out - 1):
            assert (c[i, b[i, 1]:] == 0).all()
    lut = image_prep.norm_lut()
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    for ch in range(3):
        want = torch.arange(256, dtype=torch.uint8).float().div(255).sub(CLIP_IMAGE_MEAN[ch]).div(CLIP_IMAGE_STD[ch])
        assert torch.equal(lut[ch], want)


def test_plan_tables_are_bounded():
    """what the kernels read: every tap inside the source / the intermediate, tables shared between images of one size"""
    hw = [(375, 500), (500, 375), (375, 500), (224, 224), (2001, 3000)]
    offsets = [7, 600000, 1200000, 1800000, 2000000]
    p = image_prep.plan(hw, offsets)
    assert p is image_prep.plan(hw, offsets) and p.tab.dtype == torch.int32 and p.tab.numel() == image_prep.plan_ints(hw)
    desc = p.tab[: 16 * len(hw)].numpy().view(np.int64).reshape(len(hw), 8)
    assert (desc[0, 5:] == desc[2, 5:]).all() and desc[0, 5] != desc[1, 5]
    mid_at = 0
    for b, (h, w) in enumerate(hw):
        off, sw, mid_off, rows, row0, ht, vt, ks = [int(v) for v in desc[b]]
        kh, kv = ks & 0xFFFFFFFF, ks >> 32
        assert (off, sw, mid_off) == (offsets[b], w, mid_at) and 1 <= kh <= 65 and 1 <= kv <= 65
        hb = p.tab[ht: ht + 448].view(224, 2).numpy()
        vb = p.tab[vt: vt + 448].view(224, 2).numpy()
        assert (hb[:, 0] >= 0).all() and (hb[:, 0] + hb[:, 1] <= w).all() and (hb[:, 1] <= kh).all() and (hb[:, 1] >= 1).all()
        assert (vb[:, 0] >= 0).all() and (vb[:, 0] + vb[:, 1] <= rows).all() and (vb[:, 1] <= kv).all() and (vb[:, 1] >= 1).all()
        assert row0 >= 0 and row0 + rows <= h and ht + 224 * (2 + kh) <= p.tab.numel() and vt + 224 * (2 + kv) <= p.tab.numel()
        mid_at += rows * 224 * 3
    assert p.mid_bytes == mid_at and p.max_rows == max(int(d[3]) for d in desc) and p.src_end == offsets[-1] + 3 * 2001 * 3000
    assert int(desc[3, 7]) == 1 | (1 << 32)                    # 224 x 224: both passes are the one-tap identity


def test_new_symbols_declared_bound_and_exported():
    from speechclip_plus_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    lib = _lib.lib()
    for name, nargs in (("sc_image_resample_h_u8", 10), ("sc_image_resample_v_norm", 13)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert len(_lib.SIGNATURES[name]) == nargs and getattr(lib, name) is not None
    assert "clip_official.py:153-166" in header and "base_dataset.py:93-106" in header
    assert "image_prep.hip" in build.SOURCES
    assert lib.sc_abi_version() == 7
    # host-side refusals, no launch: null pointers, neither output, odd P
    assert lib.sc_image_resample_h_u8(None, 1, None, None, None, 1, 1, 1, 224, None) != 0
    assert b"null pointer" in lib.sc_last_error()
    assert lib.sc_image_resample_v_norm(1 << 12, 8, 1 << 12, 1 << 12, 1 << 12, None, None, 0, None, 0, 1, 224, None) != 0
    assert b"neither output" in lib.sc_last_error()


def test_every_validation_error_is_raised_before_any_launch():
    m = ClipImageEncoder("ViT-B/32", layers=1)                       # on the CPU: a launch would fail differently (RuntimeError)
    ok = torch.zeros(30, 40, 3, dtype=torch.uint8)
    for call in (m, m.prep_image, m.encode_hidden):
        with pytest.raises(ValueError, match="non-empty"):
            call([])
        with pytest.raises(ValueError, match="uint8"):
            call([ok, torch.zeros(30, 40, 3)])                       # dtype
        with pytest.raises(ValueError, match="uint8"):
            call([np.zeros((30, 40, 3), dtype=np.int16)])
        with pytest.raises(ValueError, match="three interleaved channels"):
            call([torch.zeros(3, 30, 40, dtype=torch.uint8)])        # channels first
        with pytest.raises(ValueError, match="three interleaved channels"):
            call([torch.zeros(30, 40, dtype=torch.uint8)])
        with pytest.raises(ValueError, match="H, W >= 1"):
            call([torch.zeros(0, 40, 3, dtype=torch.uint8)])
        with pytest.raises(ValueError, match="ksize <= 65"):
            call([ok, torch.zeros(16 * 224 + 1, 16 * 224 + 1, 1, dtype=torch.uint8).expand(-1, -1, 3)])
        with pytest.raises(ValueError, match="tensors, numpy arrays, PIL images or paths"):
            call([ok, 3.5])
        with pytest.raises(RuntimeError, match="HIP kernels"):       # valid input, no device: refused, not computed on the CPU
            call([ok])
    image_prep.check_size(16 * 224, 16 * 224)                        # the limit itself passes: scale 16, ksize 65
    with pytest.raises(ValueError, match="ksize = 67"):
        image_prep.check_size(16 * 224 + 1, 16 * 224 + 1)
    # packed batches: sizes are host data, the buffer must hold every image
    with pytest.raises(ValueError, match="1-D uint8"):
        image_prep.RawImageBatch(torch.zeros(10, 3), [(1, 1)])
    with pytest.raises(ValueError, match="does not fit"):
        image_prep.RawImageBatch(torch.zeros(10, dtype=torch.uint8), [(2, 2)])
    with pytest.raises(ValueError, match="empty image batch"):
        image_prep.RawImageBatch(torch.zeros(10, dtype=torch.uint8), [])
    with pytest.raises(ValueError, match="H, W >= 1"):
        image_prep.RawImageBatch(torch.zeros(10, dtype=torch.uint8), [(0, 3)])
    # tensor inputs keep today's errors
    with pytest.raises(ValueError, match="interpolate"):
        m(torch.zeros(2, 3, 256, 256))
    with pytest.raises(TypeError):
        m("a.jpg")


def test_pil_images_are_converted_to_rgb(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    src = make_source(40, 30, "smooth", seed=3)
    grey = Image.fromarray(src[:, :, 0], "L")
    path = os.path.join(tmp_path, "a.png")
    Image.fromarray(src, "RGB").save(path)
    e = image_prep.as_entries([grey, Image.fromarray(src, "RGB"), path, src])
    assert all(t.dtype == torch.uint8 and tuple(t.shape) == (30, 40, 3) for t in e)
    assert torch.equal(e[0], torch.from_numpy(np.array(grey.convert("RGB")))) and torch.equal(e[1], torch.from_numpy(src))
    assert torch.equal(e[2], e[1]) and torch.equal(e[3], e[1])


def test_collate_packs_ragged_images_and_leaves_other_batches_alone():
    g = torch.Generator().manual_seed(0)
    imgs = [torch.from_numpy(make_source(w, h, "noise", seed=w)) for w, h in ((40, 30), (31, 50), (40, 30))]
    rows = [{"wav": torch.randn(100 + 10 * i, generator=g), "image": imgs[i], "id": i} for i in range(3)]
    out = collate_general(rows)
    assert out["image"].dtype == torch.uint8 and out["image"].dim() == 1 and out["image"].numel() == sum(t.numel() for t in imgs)
    assert torch.equal(out["image"], torch.cat([t.reshape(-1) for t in imgs]))
    assert out["image_hw"].dtype == torch.long and out["image_hw"].tolist() == [[30, 40], [50, 31], [30, 40]]
    assert out["image_hw"]._sc_host == [(30, 40), (50, 31), (30, 40)]
    assert list(out.keys()) == ["wav", "image", "image_hw", "id", "wav_len"]
    raw = image_prep.RawImageBatch(out["image"], out["image_hw"])
    assert raw.offsets == [0, 3600, 3600 + 4650] and len(raw) == 3
    moved = transfer_batch_to_device(out, "cpu")                   # the twin follows the tensor
    assert moved["image_hw"]._sc_host == out["image_hw"]._sc_host
    with pytest.raises(ValueError, match="ksize <= 65"):
        collate_general([{"image": torch.zeros(3600, 3600, 1, dtype=torch.uint8).expand(-1, -1, 3)}, {"image": imgs[0]}])
    # batches that work today come out byte-identical: embeddings, fp32 pixels, uint8 images of ONE size (stacked as before)
    for image in (lambda i: torch.randn(512, generator=g), lambda i: torch.randn(3, 8, 8, generator=g),
                  lambda i: torch.full((6, 5, 3), i, dtype=torch.uint8)):
        rows = [{"wav": torch.randn(50 + i, generator=g), "image": image(i), "id": 7 - i} for i in range(3)]
        out = collate_general(rows)
        assert list(out.keys()) == ["wav", "image", "id", "wav_len"] and "image_hw" not in out
        want = torch.stack([r["image"] for r in rows])
        assert out["image"].dtype == want.dtype and torch.equal(out["image"], want)
        assert out["id"].tolist() == [7, 6, 5] and out["wav_len"].tolist() == [50, 51, 52] and out["wav"].shape == (3, 52)
        for i, r in enumerate(rows):
            assert torch.equal(out["wav"][i, : 50 + i], r["wav"]) and not out["wav"][i, 50 + i:].any()
