"""What can be settled without a GPU about tests/clip_image_cases.py: the geometry of the cases, that the fp64 restatement of openai's
VisionTransformer reproduces the committed HF fixtures (at test_clip_image_cpu.py's tolerances), the q / k factor that keeps the softmax
of the cases from being flat, that an emulation of the product's arithmetic (fp32 torch, bf16 where the product stores) stays inside
every stage bound on b32 and l14 - so the bounds are satisfiable before any kernel runs -, that every planted error is rejected by the
element-wise criterion alone, and the emulation's distance from fp64 that the GPU module's whole-tower criterion refers to.  Figures are
printed before they are asserted."""
import os

import numpy as np
import pytest
import torch

import attn_cases as ac
import clip_image_cases as cc
from conftest import GOLDEN

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def runs():
    """case -> (emulated record, the product's weight dict, geometry, tower, pixels), made once"""
    made = {}

    def get(name):
        if name not in made:
            m = cc.make_tower(name)
            geo = cc.geometry(m, cc.CASES[name]["B"])
            w = dict(m._weights(CPU))
            pix = cc.pixels_of(name)
            made[name] = (cc.emulate(w, geo, pix), w, geo, m, pix)
        return made[name]
    return get


def test_case_table():
    for name, c in cc.CASES.items():
        m = cc.make_tower(name)
        geo = cc.geometry(m, c["B"])
        assert geo.rows == c["rows"] and geo.layers == c["layers"] and geo.H * 64 == geo.W, name
    b32, l14 = cc.geometry(cc.make_tower("b32"), 5), cc.geometry(cc.make_tower("l14"), 3)
    assert (b32.W, b32.H, b32.Kp, b32.tokens, b32.pitch) == (768, 12, 3072, 50, 56)
    assert (l14.W, l14.H, l14.Kp, l14.tokens, l14.pitch) == (1024, 16, 640, 257, 264)
    assert l14.tokens - 4 * 64 == 1 and l14.tokens - 2 * 128 == 1 and l14.pitch - l14.tokens == 7      # the 1-key tile, the 1-query block
    assert 64 - b32.pitch == 8                                                                          # the key tile ends 8 keys behind the image
    assert -(-4224 // 256) * (4096 // 256) == 272 > 256                                                 # l14_wide's fc1 tiles
    assert cc.make_tower("l14_one") is cc.make_tower("l14_wide")
    # the V^T layout round-trips, and decoding one image at another pitch is a different matrix
    v = torch.randn(l14.rows, l14.W).to(torch.bfloat16)
    assert torch.equal(cc.vt_rows(cc.encode_vt(v, l14), l14), v)
    wrong = cc.vt_rows(cc.encode_vt(v, l14), l14, wrong=(2, 256))
    assert torch.equal(wrong[: 2 * 264], v[: 2 * 264]) and torch.equal(wrong[2 * 264 + 256:], v[2 * 264 + 256:]) and not torch.equal(wrong, v)
    assert torch.equal(cc.rows_of(cc.heads_of(v, l14), l14), v)


def test_quickgelu_constants():
    """L = max |quickgelu'| on the grid and c(u) at the points the derivation names"""
    print(f"QGELU|L = {cc.QGELU_LIP:.6f}|c(0) = {float(cc.qgelu_err(torch.zeros(1, dtype=torch.float64))) / cc.U:.2f} U")
    assert 1.0998 < cc.QGELU_LIP < 1.1000
    u = torch.tensor([0.0, 40.0, -4.0], dtype=torch.float64)
    c = cc.qgelu_err(u) / cc.U
    assert float(c[0]) == 10.0 and abs(float(c[1]) - 8.0) < 1e-9 and 8.0 < float(c[2]) < 2 * (2 * 1.702 * 4 + 2 + 4)
    # the emulation's fp32 form and a correctly rounded fp32 form both sit inside c(u) |u| + one rounding of nothing else
    g = torch.Generator().manual_seed(1)
    u32 = (torch.randn(1 << 16, generator=g) * 3).float()
    f32 = u32 * (1.0 / (1.0 + torch.exp(-cc.ALPHA * u32)))
    err = (f32.double() - cc.qgelu64(u32.double())).abs()
    assert bool((err <= cc.qgelu_err(u32.double()) * u32.double().abs() + cc.FTZ).all())


@pytest.mark.parametrize("patch", [32, 14])
def test_fp64_restatement_matches_the_hf_fixtures(patch):
    """openai_vit64 on the fixture's weights (as they are: bf16_gemm off) against transformers' CLIPVisionModelWithProjection"""
    from speechclip_plus_amd.clip_image import CLIP_IMAGE_MEAN, CLIP_IMAGE_STD
    fx = dict(np.load(os.path.join(GOLDEN, f"clip_vision_p{patch}.npz")))
    sd = {k[2:]: torch.from_numpy(fx[k].astype(np.float32) * fx["S_" + k[2:]]) for k in fx if k.startswith("Q_")}
    img = torch.from_numpy(fx["images"]).float() / 255.0
    pix = (img - torch.tensor(CLIP_IMAGE_MEAN).view(1, 3, 1, 1)) / torch.tensor(CLIP_IMAGE_STD).view(1, 3, 1, 1)
    emb, hidden, pmax = cc.openai_vit64(sd, 2, patch, pix, bf16_gemm=False)
    ref_e, ref_h = torch.from_numpy(fx["image_embeds"]).double(), torch.from_numpy(fx["last_hidden_state"]).double()
    print(f"FIXTURE|p{patch}|embeddings {float((emb - ref_e).norm() / ref_e.norm()):.3e}|hidden {float((hidden - ref_h).norm() / ref_h.norm()):.3e}")
    assert (emb - ref_e).norm() / ref_e.norm() < 1e-5
    assert (hidden - ref_h).norm() / ref_h.norm() < 1e-3          # the hidden state is stored in fp16
    assert len(pmax) == 2 and tuple(pmax[0].shape) == (4, 2, hidden.shape[1])


def test_qk_factor():
    """per factor and layer: the median over the queries of the largest probability, fp64 reference; QK_FACTOR is the smallest factor
    that puts every layer of b32 and l14 into [0.3, 0.9]"""
    ok = {}
    for f in cc.FACTORS:
        meds = []
        for name in ("b32", "l14"):
            m = cc.make_tower(name, factor=f)
            _, _, pmax = cc.openai_vit64(m.state_dict(), m.heads, m.patch, cc.pixels_of(name))
            meds += [float(p.median()) for p in pmax]
            print(f"NOTFLAT|{name}|factor {f}|median of the largest probability per layer: " + ", ".join(f"{float(p.median()):.3f}" for p in pmax))
        ok[f] = all(cc.PMAX_LO <= x <= cc.PMAX_HI for x in meds)
    good = [f for f in cc.FACTORS if ok[f]]
    assert good and cc.QK_FACTOR == min(good), (ok, cc.QK_FACTOR)


@pytest.mark.parametrize("name", ["b32", "l14"])
def test_emulation_stays_inside_every_stage_bound(runs, name):
    rec, w, geo, m, pix = runs(name)
    rep = cc.Report()
    ratios = cc.check_record(rep, name + " (emulated)", rec, w, geo)
    assert all(v <= cc.tc.QGELU_SHARE for k, v in ratios.items() if k.endswith("share"))
    # emulate_attn is attn_cases.emulate_fwd, bit for bit (one image)
    L = rec["layers"][0]
    q, k, v = (cc.heads_of(t, geo)[: geo.H] for t in (L["qk"][:, : geo.W], L["qk"][:, geo.W:], cc.vt_rows(L["vt"], geo)))
    o, _ = ac.emulate_fwd(q, k, v, cc.key_mask(geo))
    assert torch.equal(o, cc.heads_of(L["ctx"], geo)[: geo.H])
    # the zero rows of the patch operand and the pad rows of the embedding
    assert float(rec["G"][cc.row0_of(geo)].abs().max()) == 0.0
    rep.done()


@pytest.mark.parametrize("name", ["b32", "l14"])
def test_every_planted_error_is_rejected(runs, name):
    rec, w, geo, m, pix = runs(name)
    got = cc.planted_suite(name + " (emulated)", rec, w, geo, fc1_row=(name == "l14"))
    print(f"PLANTS|{name}|" + ", ".join(f"{k}: {v:.3g}" for k, v in got.items()))
    assert len(got) == (8 if name == "l14" else 5)
    assert got.pop("attention plant, bounds moved") >= cc.PLANT_MOVES
    assert all(v > 1.0 for v in got.values()), got


@pytest.mark.parametrize("name", ["b32", "l14"])
def test_whole_tower_control(runs, name):
    """the emulation's distance from the fp64 tower per image: what the GPU module's criterion measures the HIP embeddings against"""
    rec, w, geo, m, pix = runs(name)
    ref, hidden, _ = cc.openai_vit64(m.state_dict(), m.heads, m.patch, pix)
    per, (_, d_emu, _) = cc.distances(rec["emb"], rec["emb"], ref)
    print(f"CONTROL|{name}|emulation to fp64 per image: " + ", ".join(f"{float(x):.3e}" for x in per[:, 1]) + f"|batch {d_emu:.3e}")
    last = rec["layers"][-1]["out"].view(geo.B, geo.pitch, geo.W)[:, : geo.tokens]
    print(f"CONTROL|{name}|last hidden rows rel-L2 {cc.rel_l2(last, hidden):.3e}")
    assert 0.0 < d_emu < 2e-2 and cc.rel_l2(last, hidden) < 2e-2
