"""A valid output does not depend on the bytes a kernel reads but the mathematics excludes (docs/parity.md, "What a kernel reads and must
ignore"): keys at t >= valid_len, pad rows of a ragged utterance, the rows / elements a 64-key attention tile reads past an utterance or
past the buffer, and memory that nobody wrote.

  (a) sc_attn_fwd_bf16, both layouts, every instance: a clean run (excluded places zero), a run with FINITE_POISON under every mask of
      tests/poison_cases.py, a run with NONFINITE_POISON in the excluded K rows only, one with it in the q and the gate of the
      excluded rows -> out and lse2 of the rows t < len carry the bits of the clean run; the clean run itself is held against fp64
      with the bounds of tests/attn_cases.py.  (V^T must stay finite: 0 x NaN in the P.V product - the documented contract.)
  (b) sc_hubert_layer_fwd: pad rows of x drawn from N(0, 64^2), and the whole workspace except its documented finite slack
      pre-filled with NONFINITE_POISON -> out, ffn and qk on the valid rows carry the bits of the clean run.
  (c) whole paths once normally and once with torch.empty / empty_like / new_empty returning NaN: bit-equal valid rows and embeddings.

Values only: every operand carries its 64-row / 64-element slack inside its own tensor (tests/test_poison_cases_cpu.py checks the
largest index the contract allows against every allocation), so no case makes a kernel read outside the tensor it was given.  No
tolerance: every assertion is bit equality against a clean run, or a derived bound against fp64."""
import pytest
import torch

import attn_cases as ac
import poison_cases as pc
import wavlm_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 7.0
DROP_P, DROP_SEED = 0.1, 20260
_CACHE = {}


def _ops():
    from speechclip_plus_amd import ops
    return ops


def _heads(x, H):
    return x.double().view(x.shape[0], H, 64).transpose(0, 1)


# ================================================================================================================== (a) attention
def _case_operands(name):
    """operands and table of a geometry: built once, shared by its instances, never modified"""
    if name not in _CACHE:
        lay = pc.case_layout(name)
        ops_ = pc.operands(lay, seed=100 + sorted(pc.GEOMETRIES).index(name), tmax=pc.TMAX)
        table = wc.bias_table(torch.randn(wc.NUM_BUCKETS, lay.H, generator=torch.Generator().manual_seed(9)), pc.TMAX).float().contiguous()
        _CACHE[name] = (lay, ops_, table)
    return _CACHE[name]


def _attn(lay, qk, vt, gate, table, inst, use_work):
    """one launch -> out [rows, D] bf16, lse2 [H rows] fp32 on the CPU; the sentinel rows behind both are checked here"""
    ops = _ops()
    H, D, rows, B = lay.H, lay.D, lay.rows, len(lay.pitch)
    assert tuple(qk.shape) == (lay.qk_rows, 2 * D) and vt.numel() == lay.vt_numel and pc.within_allocation(lay)
    seg = None if lay.uniform else ops.RowSegments(lay.pitch, lay.lens, DEV)
    out = torch.full((rows + 8, D), SENT, dtype=torch.bfloat16, device=DEV)
    lse2 = torch.full((H * rows + 8,), SENT, dtype=torch.float32, device=DEV)
    kw = {"gate": gate.to(DEV), "table": table.to(DEV)} if inst == "bias" else {}
    ops.attn_fwd(qk.to(DEV), vt.to(DEV), torch.tensor(lay.lens, dtype=torch.int32, device=DEV), out, B, lay.pitch[0] if lay.uniform else 0, H, D,
                 0.125, lse2=lse2, causal=pc.CAUSAL_OF[inst], drop_p=DROP_P if inst == "drop" else 0.0, drop_seed=DROP_SEED, seg=seg,
                 use_work=use_work, **kw)
    torch.cuda.synchronize()
    out, lse2 = out.cpu(), lse2.cpu()
    assert bool((out[rows:] == SENT).all()) and bool((lse2[H * rows:] == SENT).all()), "sentinel rows behind the outputs were written"
    return out[:rows], lse2[: H * rows]


def _lse_rows(lay, lse2):
    """-> [H, rows]: the lse2 of either layout ([B, H, R] uniform, [H, rows] segment) by row of the batch"""
    if lay.uniform:
        B, R = len(lay.pitch), lay.pitch[0]
        return lse2.view(B, lay.H, R).transpose(0, 1).reshape(lay.H, B * R)
    return lse2.view(lay.H, lay.rows)


def _against_fp64(rep, tag, lay, ops_, table, inst, out, lse2):
    causal = pc.CAUSAL_OF[inst]
    lse = _lse_rows(lay, lse2)
    for b, (q, k, v, g) in enumerate(pc.cut_to_valid(lay, ops_["qk"], ops_["vt"], ops_["gate"])):
        n, r0 = q.shape[0], lay.row0[b]
        bias = ac.bias_matrix(g.double(), table.double(), n) if inst == "bias" else None
        f = ac.fwd_ref(_heads(q, lay.H), _heads(k, lay.H), _heads(v, lay.H), ac.key_mask(n, n, causal)[None], bias=bias)
        ac.check(rep, f"{tag} b={b}", "out", _heads(out[r0: r0 + n], lay.H), f["out"], f["bound"])
        ac.check(rep, f"{tag} b={b}", "lse2", lse[:, r0: r0 + n], f["lse2"], f["bound_lse"])


@pytest.mark.parametrize("name,inst,use_work", pc.attention_cases())
def test_attention_ignores_what_it_reads_but_excludes(name, inst, use_work):
    lay, ops_, table = _case_operands(name)
    tag = f"{name} {inst}{'' if use_work else ' no-work'}"
    rep = ac.Report()
    valid = lay.valid_rows
    clean_out, clean_lse = _attn(lay, ops_["qk"], ops_["vt"], ops_["gate"], table, inst, use_work)
    assert bool(torch.isfinite(clean_out[valid].float()).all()) and bool(torch.isfinite(_lse_rows(lay, clean_lse)[:, valid]).all())
    if inst != "drop":                       # the clean run against fp64 (not against the kernel's own output); dropout: attn_scores
        _against_fp64(rep, tag, lay, ops_, table, inst, clean_out, clean_lse)
    runs = {
        "finite poison under every mask": (pc.poison_bf16(ops_["qk"], lay.qk, pc.FINITE_POISON), pc.poison_bf16(ops_["vt"], lay.vt, pc.FINITE_POISON),
                                           pc.poison_f32(ops_["gate"], lay.gate, pc.FINITE_POISON)),
        "non-finite poison in the excluded K rows": (pc.poison_bf16(ops_["qk"], lay.k, pc.NONFINITE_POISON), ops_["vt"], ops_["gate"]),
        # beyond "finite": a pad query is one lane of every reduction, so its q and its gate may hold any bits as well
        "non-finite poison in the q and the gate of excluded rows": (pc.poison_bf16(ops_["qk"], lay.qk & ~lay.k, pc.NONFINITE_POISON), ops_["vt"],
                                                                      pc.poison_f32(ops_["gate"], lay.gate, pc.NONFINITE_POISON)),
    }
    for what, (qk, vt, gate) in runs.items():
        out, lse2 = _attn(lay, qk, vt, gate, table, inst, use_work)
        same_o = pc.bits_equal(out[valid], clean_out[valid])
        same_l = pc.bits_equal(_lse_rows(lay, lse2)[:, valid], _lse_rows(lay, clean_lse)[:, valid])
        nbad = int((out[valid].view(torch.int16) != clean_out[valid].view(torch.int16)).sum())
        print(f"POISON|{tag}|{what}|out bits equal {same_o} ({nbad} differ, {int(torch.isnan(out[valid].float()).sum())} NaN)|lse2 bits equal {same_l}")
        rep.require(tag, f"{what}: out of the rows t < len differs from the clean run in {nbad} elements", same_o)
        rep.require(tag, f"{what}: lse2 of the rows t < len differs from the clean run", same_l)
    rep.done()


# ================================================================================================================== (b) layer driver
D_L, F_L, H_L = 128, 256, 2


def _driver_weights():
    """the seeded weights of tests/test_gpu_split_weights.py::test_layer_driver_with_w_split_equals_per_op, as plain bf16 operands"""
    if "w" not in _CACHE:
        g = torch.Generator().manual_seed(61)
        f32 = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(DEV)
        bf = lambda t: t.to(torch.bfloat16).contiguous()
        D, F = D_L, F_L
        w = {"l0_qkv_w": bf(f32(3 * D, D, sc=D ** -0.5)), "l0_o_w": bf(f32(D, D, sc=D ** -0.5)), "l0_fc1_w": bf(f32(F, D, sc=D ** -0.5)),
             "l0_fc2_w": bf(f32(D, F, sc=F ** -0.5)), "l0_qkv_b": f32(3 * D, sc=0.05), "l0_o_b": f32(D, sc=0.05), "l0_fc1_b": f32(F, sc=0.05),
             "l0_fc2_b": f32(D, sc=0.05)}
        for n in ("ln1", "ln2"):
            w[f"l0_{n}_g"], w[f"l0_{n}_b"] = 1.0 + f32(D, sc=0.1), f32(D, sc=0.1)
        _CACHE["w"] = w
    return _CACHE["w"]


def _driver(lay, x, ws, pre_ln, ffn_act):
    """one sc_hubert_layer_fwd on the workspace ``ws`` (flat bf16, the documented layout) -> out, ffn, qk [rows, .] on the CPU"""
    from types import SimpleNamespace
    from speechclip_plus_amd._lib import lib
    ops = _ops()
    rows, D, F, H = lay.rows, D_L, F_L, H_L
    total, parts = pc.driver_workspace(rows, D, F)
    assert int(lib().sc_workspace_bytes(1, rows, D, F)) == 2 * total, "sc_workspace_bytes does not describe a workspace with the attention slack"
    assert ws.numel() == total and pc.within_allocation(lay)
    view = lambda name, cols: ws[parts[name][0]: parts[name][0] + parts[name][1]].view(rows, cols)
    pl = SimpleNamespace(qk=view("qk", 2 * D), vt=view("vt", D), ctx=view("ctx", D), pre=view("pre", D), x1=view("x1", D), ffn=view("ffn", F))
    seg = None if lay.uniform else ops.RowSegments(lay.pitch, lay.lens, DEV)
    out = torch.full((rows + 8, D), SENT, dtype=torch.bfloat16, device=DEV)
    valid = torch.tensor(lay.lens, device=DEV, dtype=torch.int32)
    ops.hubert_layer_fwd(x[:rows], out, valid, _driver_weights(), 0, pl, len(lay.pitch), lay.pitch[0], max(lay.lens), D, F, H, pre_ln, seg=seg,
                         ffn_act=ffn_act)
    torch.cuda.synchronize()
    assert bool((out[rows:] == SENT).all()), "rows behind the output were written"
    return out[:rows].cpu(), pl.ffn.cpu(), pl.qk.cpu()


@pytest.mark.parametrize("layout", list(pc.DRIVER_GEOMETRIES))
@pytest.mark.parametrize("ffn_act", [0, 2])
@pytest.mark.parametrize("pre_ln", [False, True])
def test_layer_driver_ignores_pad_rows_and_workspace_content(pre_ln, ffn_act, layout):
    lay = pc.case_layout(layout, pc.DRIVER_GEOMETRIES)
    rows, valid = lay.rows, lay.valid_rows
    g = torch.Generator().manual_seed(62)
    x = torch.zeros(rows + 64, D_L, dtype=torch.bfloat16)
    x[:rows][valid] = torch.randn(int(valid.sum()), D_L, generator=g).to(torch.bfloat16)
    x_pad = x.clone()
    x_pad[:rows][~valid] = (64.0 * torch.randn(rows - int(valid.sum()), D_L, generator=g)).to(torch.bfloat16)   # scratch of ordinary magnitude
    total, parts = pc.driver_workspace(rows, D_L, F_L)
    zero_ws = torch.zeros(total, dtype=torch.bfloat16)
    # everything the contract leaves open - qk, the rows behind it, vt, ctx, pre, x1, ffn - holds NaN / Inf; the 64 elements behind vt are 0
    keep = torch.zeros(total, dtype=torch.bool)
    keep[parts["vt_slack"][0]: parts["vt_slack"][0] + parts["vt_slack"][1]] = True
    dirty_ws = pc.poison_bf16(zero_ws, ~keep, pc.NONFINITE_POISON)
    assert int(torch.isfinite(dirty_ws.float()).sum()) == 64
    clean = _driver(lay, x.to(DEV), zero_ws.to(DEV), pre_ln, ffn_act)
    assert all(bool(torch.isfinite(t[valid].float()).all()) for t in clean)
    bad = []
    for what, xin, ws in (("pad rows of x ~ N(0, 64^2)", x_pad, zero_ws), ("workspace pre-filled with NaN / Inf", x, dirty_ws)):
        got = _driver(lay, xin.to(DEV), ws.to(DEV), pre_ln, ffn_act)
        for name, a, b in zip(("out", "ffn", "qk"), got, clean):
            same = pc.bits_equal(a[valid], b[valid])
            print(f"POISON|driver pre_ln={int(pre_ln)} ffn_act={ffn_act} {layout}|{what}|{name} bits equal {same} "
                  f"({int(torch.isnan(a[valid].float()).sum())} NaN of {a[valid].numel()})")
            if not same:
                bad.append((what, name))
    assert not bad, bad


# ================================================================================================================== (c) whole paths
def _normal_then_poisoned(fn):
    """fn() once normally and once with torch.empty / empty_like / new_empty returning NaN"""
    a = fn()
    torch.cuda.synchronize()
    with pc.poisoned_empty():
        b = fn()
        torch.cuda.synchronize()
    return a, b


def _tower(patch):
    from speechclip_plus_amd.clip_image import ClipImageEncoder
    from test_gpu_clip_image import SMALL
    return ClipImageEncoder("fixture", patch=patch, seed=17, **SMALL).cuda()


def _raw_images():
    from image_prep_cases import source
    return [torch.from_numpy(source(i).copy()) for i in (0, 4, 5)]


@pytest.mark.parametrize("kind,B", [("pixels", 1), ("pixels", 3), ("raw", 3)])
@pytest.mark.parametrize("patch", [32, 14])
def test_image_tower_does_not_depend_on_uninitialised_memory(patch, kind, B):
    """forward and encode_hidden (token rows) of the small tower: a normal run, then a poisoned run on the same module (its caches
    warm) and on a second module of the same seed whose FIRST forward happens inside the context (every cache built there)"""
    m, fresh = _tower(patch), _tower(patch)
    images = _raw_images() if kind == "raw" else torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B)).to(DEV)

    def run(mod):
        with torch.no_grad():
            X, _ = mod.encode_hidden(images)
            return mod(images).cpu(), X.view(B, mod.pitch, mod.width)[:, : mod.tokens].cpu()

    (emb, hid), (emb_p, hid_p) = _normal_then_poisoned(lambda: run(m))
    with pc.poisoned_empty():
        emb_f, hid_f = run(fresh)
        torch.cuda.synchronize()
    for what, e, h in (("warm module", emb_p, hid_p), ("fresh module", emb_f, hid_f)):
        print(f"POISON|image tower P={patch} {kind} B={B}|{what}|embeddings NaN {int(torch.isnan(e).sum())} of {e.numel()}|"
              f"token rows NaN {int(torch.isnan(h.float()).sum())} of {h.numel()}")
    assert bool(torch.isfinite(emb).all()) and bool(torch.isfinite(hid.float()).all())
    assert pc.bits_equal(emb_p, emb) and pc.bits_equal(hid_p, hid), "warm module: the poisoned run differs"
    assert pc.bits_equal(emb_f, emb) and pc.bits_equal(hid_f, hid), "fresh module: the poisoned run differs"


@pytest.mark.parametrize("variant", ["post", "stable"])
def test_speech_encoders_do_not_depend_on_uninitialised_memory(variant):
    """the two-layer WavLM and HuBERT encoders of tests/test_gpu_wavlm.py, padded and ragged: every hidden state on the valid frames
    and the weighted sum"""
    from test_gpu_wavlm import _enter_at_projection, _small_encoders
    fx, o_arch, W, wavlm, hubert = _small_encoders(variant)
    wav, lens = torch.from_numpy(fx["wav"]), fx["lens"].tolist()
    dbg = {}
    _, _, valid, feat_len = wc.wavlm_forward(W, o_arch, [wav[b, :l] for b, l in enumerate(lens)], debug=dbg)
    for name, enc in (("wavlm", wavlm), ("hubert", hubert)):
        _enter_at_projection(enc, dbg["proj"].float())
        for ragged in (False, True):
            def run():
                with torch.no_grad():
                    pl = enc._encode(wav.to(DEV), lens, ragged=ragged)
                    hs = [wc.valid_frames(h.cpu(), valid) for h in enc._materialised_states(pl)]
                    feat, fl = enc(wav.to(DEV), torch.tensor(lens))
                assert fl.tolist() == feat_len
                return hs + [wc.valid_frames(feat.cpu(), feat_len)]
            a, b = _normal_then_poisoned(run)
            same = [pc.bits_equal(x, y) for x, y in zip(a, b)]
            print(f"POISON|{name} {variant} {'ragged' if ragged else 'padded'}|states + weighted sum bit-equal: {same}")
            assert all(bool(torch.isfinite(x.float()).all()) for x in a)
            assert all(same), (name, ragged, same)


def test_encode_text_does_not_depend_on_uninitialised_memory(golden):
    """encode_text on the transformers fixture the HIP text tower is built for (clip_text_w128: head_dim 64; clip_text_w64 has
    head_dim 16, which sc_attn_fwd_bf16 refuses): both segment classes of its captions, bucketed and not"""
    from conftest import weights_from
    from speechclip_plus_amd import clip_text
    fx = golden("clip_text_w128.npz")
    W = {k[len("clip.model."):]: v for k, v in weights_from(fx).items()}
    V = W["token_embedding.weight"].shape[0]
    clip_text.CLIP_TEXT_ARCHS["hf-fixture-w128"] = dict(width=128, heads=int(fx["heads"]), layers=2, embed_dim=W["text_projection"].shape[1])
    try:
        vocab = torch.cat([torch.arange(V - 2), torch.tensor([clip_text.SOT_TOKEN, clip_text.EOT_TOKEN])])
        clip = clip_text.ClipModel("hf-fixture-w128", device="cuda:0", reduce_subword_embbedding=vocab).eval()
    finally:
        del clip_text.CLIP_TEXT_ARCHS["hf-fixture-w128"]
    clip.model.load_state_dict({k: v for k, v in W.items()}, strict=True)
    ids = torch.from_numpy(fx["ids"]).cuda()
    for bucket in (True, False):
        a, b = _normal_then_poisoned(lambda: clip.encode_text(ids, bucket=bucket).cpu())
        print(f"POISON|encode_text bucket={bucket}|NaN {int(torch.isnan(b).sum())} of {b.numel()}")
        assert bool(torch.isfinite(a).all()) and pc.bits_equal(a, b), bucket


def test_search_and_ranks_do_not_depend_on_uninitialised_memory():
    import rank_cases as rk
    import search_cases as sc_cases
    from speechclip_plus_amd import mutual_ranks, search
    q, gal = sc_cases.int_case(65, 129, 64, seed=65 + 129 + 64)
    qd, gd = q.float().to(DEV), gal.float().to(DEV)
    want = sc_cases.int_expected(q, gal, 10)
    for route in ("fused", None):
        a, b = _normal_then_poisoned(lambda: tuple(t.cpu() for t in search(qd, gd, 10, route=route)))
        assert torch.equal(a[1], want[1]) and torch.equal(a[0], want[0])
        assert pc.bits_equal(a[0], b[0]) and torch.equal(a[1], b[1]), route
    a_ids, b_ids = rk.caption_ids(65, 129, seed=65)
    a, b = _normal_then_poisoned(lambda: {k: v.cpu() for k, v in mutual_ranks(qd, gd, a_ids.to(DEV), b_ids.to(DEV)).items()})
    assert set(a) == set(b) and all(pc.bits_equal(a[k], b[k]) for k in a), [k for k in a if not pc.bits_equal(a[k], b[k])]
