"""GPU: the frozen CLIP image tower stage by stage against float64, element by element, on each launch's own operands.

``_sequence`` issues what ClipImageEncoder._encode_patches + forward issue, one entry point at a time through ``ops`` and keeping every
intermediate: vit_patchify, gemm_raw(out_f32), vit_embed_ln, per block layernorm_bf16, gemm_raw(seg=, Ct=, n_split=), attn_fwd(seg=),
linear_bf16(residual=), layernorm_bf16, linear_bf16(act = 2), linear_bf16(residual=), then rows_gather, rowln_fwd and
sgemm_mfma(b_kmajor).  Its last hidden rows and embeddings are first asserted bitwise equal to the product's (encode_hidden, forward),
which ties the stages to the product; a second call must give the same bits.  tests/clip_image_cases.py holds the cases, the fp64
references (run here in fp64 on the device), the bounds (docs/parity.md, "CLIP image tower / Stage by stage"; fixed before the first GPU
run), the emulation and the planted errors; tests/test_clip_image_cases_cpu.py shows on the CPU that the bounds are satisfiable.

Measured on one MI355X: the figures of the section's "Measured" table."""
import copy

import pytest
import torch

import clip_image_cases as cc

pytestmark = pytest.mark.gpu


def _sequence(m, pix):
    """the tower's launches one by one -> a record (clip_image_cases); ``u32`` is the fc1 product launched once more with act = 0 in fp32"""
    from speechclip_plus_amd import ops
    dev = pix.device
    w = m._weights(dev)
    B = pix.shape[0]
    seg, vl = m.segments(B, dev)
    D, F_, H, rows, Kp = m.width, 4 * m.width, m.heads, seg.rows, m.Kp
    A = ops.vit_patchify(pix, seg, m.patch, Kp)
    G = torch.empty(rows, D, device=dev, dtype=torch.float32)
    ops.gemm_raw(A, Kp, w["conv1"], Kp, G, D, rows, D, Kp, out_f32=True)
    X = ops.vit_embed_ln(G, w["cls"], w["pos"], w["ln_pre_g"], w["ln_pre_b"], seg)
    rec = dict(A=A, G=G, X0=X, layers=[])
    for i in range(m.arch["layers"]):
        # qk and vt with the zeroed slack the attention tiles read behind the last image (64 rows / 64 elements)
        qk = torch.zeros(rows + 64, 2 * D, device=dev, dtype=torch.bfloat16)[:rows]
        vt = torch.zeros(rows * D + 64, device=dev, dtype=torch.bfloat16)[: rows * D]
        h1 = ops.layernorm_bf16(X, w[f"l{i}_ln1_g"], w[f"l{i}_ln1_b"])
        ops.gemm_raw(h1, D, w[f"l{i}_qkv_w"], D, qk, 2 * D, rows, 3 * D, D, bias=w[f"l{i}_qkv_b"], Ct=vt.view(rows, D), n_split=2 * D,
                     R=m.pitch, dh=64, seg=seg)
        ctx = torch.empty(rows, D, device=dev, dtype=torch.bfloat16)
        ops.attn_fwd(qk, vt.view(rows, D), vl, ctx, B, m.pitch, H, D, 0.125, seg=seg)
        pre = ops.linear_bf16(ctx, w[f"l{i}_o_w"], w[f"l{i}_o_b"], residual=X)
        h2 = ops.layernorm_bf16(pre, w[f"l{i}_ln2_g"], w[f"l{i}_ln2_b"])
        ffn = ops.linear_bf16(h2, w[f"l{i}_fc1_w"], w[f"l{i}_fc1_b"], act=2)
        u32 = ops.linear_bf16(h2, w[f"l{i}_fc1_w"], w[f"l{i}_fc1_b"], act=0, out_f32=True)
        out = ops.linear_bf16(ffn, w[f"l{i}_fc2_w"], w[f"l{i}_fc2_b"], residual=pre)
        rec["layers"].append(dict(x=X, h1=h1, qk=qk, vt=vt, ctx=ctx, pre=pre, h2=h2, u32=u32, ffn=ffn, out=out))
        X = out
    rec["cls"] = ops.rows_gather(X, seg.row0[: seg.B])
    rec["y"], _, _ = ops.rowln_fwd(rec["cls"], None, 0, w["ln_post_g"], w["ln_post_b"], m.ln_post.eps)
    rec["emb"] = ops.sgemm_mfma(rec["y"], w["proj"], b_kmajor=True)
    torch.cuda.synchronize()
    return rec


def _flat(rec):
    return [rec[k] for k in ("A", "G", "X0", "cls", "y", "emb")] + [L[k] for L in rec["layers"] for k in sorted(L)]


@pytest.fixture(scope="module")
def runs():
    """case -> (record, the product's weight dict, geometry, tower, pixels), made once"""
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    dev = torch.device("cuda:0")
    made = {}

    def get(name):
        if name not in made:
            m = copy.deepcopy(cc.make_tower(name)).to(dev)
            pix = cc.pixels_of(name).to(dev)
            geo = cc.geometry(m, pix.shape[0])
            with torch.no_grad():
                rec = _sequence(m, pix)
                # first of all: these stages are the product's - the last hidden rows (real rows) and the embeddings, bit for bit
                Xp, _ = m.encode_hidden(pix)
                emb = m(pix)
            real = cc.real_rows(geo, dev)
            assert tuple(Xp.shape) == (geo.rows, geo.W) and geo.rows == cc.CASES[name]["rows"]
            assert torch.equal(rec["layers"][-1]["out"][real], Xp[real]), f"{name}: the sequence's last hidden rows are not encode_hidden's"
            assert torch.equal(rec["emb"], emb), f"{name}: the sequence's embeddings are not forward's"
            assert emb.dtype == torch.float32 and tuple(emb.shape) == (geo.B, geo.E)
            made[name] = (rec, m._weights(dev), geo, m, pix)
        return made[name]
    return get


@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_sequence_is_the_product_and_repeats(runs, name):
    """the stages are the product's (asserted by the fixture before anything else: last hidden rows and embeddings bitwise equal to
    encode_hidden / forward); the product once more and a second sequence give the same bits, the latter in every intermediate"""
    rec, w, geo, m, pix = runs(name)
    with torch.no_grad():
        emb = m(pix)
        again = _sequence(m, pix)
    assert torch.equal(rec["emb"], emb)
    assert torch.equal(rec["A"], cc.expected_patches(pix, geo))                  # the next stage's operand (bitwise, as test_patchify_bitwise)
    for a, b in zip(_flat(rec), _flat(again)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_stage_by_stage_vs_fp64(runs, name):
    """every launch against the fp64 definition of its operation on its own operands; the test fails once, with all its violations"""
    rec, w, geo, m, pix = runs(name)
    rep = cc.Report()
    ratios = cc.check_record(rep, name, rec, w, geo)
    print(f"STAGES|{name}|largest error / bound " + f"{max(v for k, v in ratios.items() if not k.endswith(('ulps', 'share'))):.3f}")
    rep.done()


def test_tile_families_agree_on_the_wide_case(runs):
    """l14_wide, the recorded fc1 (QuickGELU epilogue, 272 output tiles of 256 x 256), QKV and out_proj operands: tile = 1 (128 x 128),
    7 (256 x 192), 8 (256 x 256) and the cost model's choice give identical bits; the forced 256 x 192 launch of fc1 meets the fc1
    criterion against fp64 on its own.  The QKV launch has no 256 x 192 form at this width (n_split = 2048 is no multiple of 192): forcing
    it must be refused before anything is launched (docs/parity.md, "Findings")"""
    from speechclip_plus_amd import ops
    rec, w, geo, m, pix = runs("l14_wide")
    L = rec["layers"][0]
    rows, D = geo.rows, geo.W
    seg, _ = m.segments(geo.B, pix.device)
    assert ops.gemm_tile_name(rows, 4 * D, D, -1, 1) == "256x256" and -(-rows // 256) * (4 * D // 256) == 272
    rep = cc.Report()
    for tile in (1, 7, 8):
        f = ops.linear_bf16(L["h2"], w["l0_fc1_w"], w["l0_fc1_b"], act=2, tile=tile)
        assert torch.equal(f, L["ffn"]), tile
        if tile == 7:
            ref, bound, _ = cc.fc1_ref(L["h2"], w["l0_fc1_w"], w["l0_fc1_b"])
            cc.check(rep, "l14_wide", "fc1 + QuickGELU, 256 x 192 tile", f, ref, bound)
        o = ops.linear_bf16(L["ctx"], w["l0_o_w"], w["l0_o_b"], residual=L["x"], tile=tile)
        assert torch.equal(o, L["pre"]), tile
        qk = torch.zeros(rows + 64, 2 * D, device=pix.device, dtype=torch.bfloat16)[:rows]
        vt = torch.zeros(rows * D + 64, device=pix.device, dtype=torch.bfloat16)[: rows * D]
        qkv = lambda: ops.gemm_raw(L["h1"], D, w["l0_qkv_w"], D, qk, 2 * D, rows, 3 * D, D, bias=w["l0_qkv_b"], Ct=vt.view(rows, D),
                                   n_split=2 * D, R=m.pitch, dh=64, seg=seg, tile=tile)
        if tile == 7:       # n_split = 2048 = 10 x 192 + 128: a 192-wide tile would straddle the q / k | V^T split, the launch is refused
            with pytest.raises(RuntimeError, match="n_split"):
                qkv()
            continue
        qkv()
        assert torch.equal(qk, L["qk"]) and torch.equal(vt, L["vt"]), tile
    torch.cuda.synchronize()
    rep.done()


def test_each_criterion_rejects_its_planted_error(runs):
    """the eight planted errors, applied on the host to the kernels' own results (or as a changed reference): the element-wise criterion
    alone must reject each with error / bound > 1"""
    got = {}
    for name in ("b32", "l14"):
        rec, w, geo, m, pix = runs(name)
        r = cc.planted_suite(name, rec, w, geo, fc1_row=False)
        assert r.pop("attention plant, bounds moved") >= cc.PLANT_MOVES
        got.update({f"{name}: {k}": v for k, v in r.items()})
    rec, w, geo, m, pix = runs("l14_wide")
    got["l14_wide: 5 fc1 row"] = cc.plant_fc1_row(rec["layers"][0], w, 0)
    print("PLANTS|" + ", ".join(f"{k}: {v:.3g}" for k, v in got.items()))
    assert {k.split(": ")[1][0] for k in got} == set("12345678") and all(v > 1.0 for v in got.values()), got


@pytest.mark.parametrize("name", ["b32", "l14"])
def test_whole_tower_against_the_emulation_and_fp64(runs, name):
    """docs/parity.md's recall criterion (item 2) on the embeddings: the HIP tower sits no farther from the bf16-storage emulation than the
    emulation sits from the fp64 tower (openai's VisionTransformer on the same weights, GEMM weights as their bf16 copies).  The
    HIP-to-fp64 distance is printed per image."""
    rec, w, geo, m, pix = runs(name)
    with torch.no_grad():
        emu = cc.emulate(w, geo, pix)
        ref, hidden, _ = cc.openai_vit64(m.state_dict(), m.heads, m.patch, pix)
    per, (d_hip, d_emu, d_he) = cc.distances(rec["emb"], emu["emb"], ref)
    for b in range(geo.B):
        print(f"TOWER|{name} image {b}|HIP to fp64 {float(per[b, 0]):.3e}|emulation to fp64 {float(per[b, 1]):.3e}|HIP to emulation {float(per[b, 2]):.3e}")
    print(f"TOWER|{name}|batch: HIP to fp64 {d_hip:.3e}, emulation to fp64 {d_emu:.3e}, HIP to emulation {d_he:.3e}")
    assert bool(torch.isfinite(rec["emb"]).all())
    assert d_he <= d_emu, f"{name}: HIP to emulation {d_he:.3e} > emulation to fp64 {d_emu:.3e}"
