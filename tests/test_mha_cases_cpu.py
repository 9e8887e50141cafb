"""CPU: the keyword attention block's test rig without a device (tests/mha_cases.py).  The real speechclip_plus_amd/mha_block.py runs
on the host over ``mha_cases.emu_ops`` - the kernels' arithmetic order in torch: fp32 accumulation K-tile by K-tile, bf16 at the storage
sites, the hash masks, ``gemm_raw`` through the call's own strides - under the same recording proxy and the same stage walkers as
tests/test_gpu_mha_block.py.  Shown here, before anything runs on a device: the emulation stays inside every bound of docs/parity.md
("Keyword attention block"), each planted error breaks its bound, the fp64 formulas equal fp64 autograd, and the host restatement of
the padded-head weight layout equals the unpadded module."""
import pytest
import torch

import mha_cases as mc


@pytest.fixture(scope="module")
def rig():
    from speechclip_plus_amd import mha_block
    mp = pytest.MonkeyPatch()
    emu = mc.emu_ops()
    rec = mc._Rec(emu)
    mp.setattr(mha_block, "ops", rec)
    yield mha_block, rec, emu, torch.device("cpu")
    mp.undo()


def test_cases_reach_their_paths():
    g = {n: mc.geom(c) for n, c in mc.CASES.items()}
    assert g["base_tn"].tn and g["base_tn"].Sp == 512 and g["tn_min"].tn and g["tn_min"].Sp == g["tn_min"].dh == 256
    assert not g["base_short"].tn and g["base_short"].dh % 256 == 0 and g["base_short"].Sp % 256 != 0
    assert (g["large8"].dh, g["large8"].D, g["large8"].padded) == (128, 1024, False)
    assert (g["pad96"].dh_true, g["pad96"].dh, g["pad96"].D, g["pad96"].Dm) == (96, 128, 256, 192)
    assert (g["pad8"].dh_true, g["pad8"].dh, g["pad8"].D) == (8, 64, 512)
    for n, c in mc.CASES.items():
        assert len(c["lens"]) == c["B"] and max(c["lens"]) == c["S"] and c["lens"][-1] < c["S"], n
        inp = mc.make_inputs(n, c)
        assert torch.equal(inp.x, mc.bfr(inp.x)) and bool((inp.dout[~inp.live] == 0).all())
    assert 1 in mc.CASES["tn_min"]["lens"] and 1 in mc.CASES["pad8"]["lens"]
    seen = {k for _, o in mc.STAGE_RUNS for k, v in o.items() if v is not False and v != 0.0} | {"rows"}
    assert {"rows", "rows_out", "acc", "p_att", "p_res", "mask", "dcls"} <= seen
    for n, o in mc.STAGE_RUNS:
        assert not (g[n].padded and o.get("acc")), "grad_target is off for padded heads"


@pytest.mark.parametrize("case,over", mc.STAGE_RUNS, ids=[f"{n}-{mc.mode_id(o)}" for n, o in mc.STAGE_RUNS])
def test_emulation_stays_inside_every_bound_and_planted_errors_break_them(rig, case, over):
    mb, rec, emu, dev = rig
    c = mc.CASES[case]
    inp = mc.make_inputs(case, c)
    r = mc.run_mha(mb, rec, c, inp, dev, mc.mode_of(over))
    rep = mc.Report(f"{case} {mc.mode_id(over)} (emulation)")
    st = mc.check_run(rep, emu, r, inp)
    rep.show()
    assert max(v[0] for v in rep.rows.values()) <= 1.0
    names = mc.assert_planted_rejected(st)
    assert len(names) == (6 if c["H"] > 1 else 5)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_encoder_emulation_stays_inside_every_bound(rig, p):
    mb, rec, emu, dev = rig
    inp = mc.make_inputs("ffn", mc.FFN_CASE)
    r = mc.run_encoder(mb, rec, mc.FFN_CASE, inp, dev, p)
    rep = mc.Report(f"ffn p={p} (emulation)")
    mc.check_encoder_run(rep, emu, r)
    rep.show()


def test_a_recorded_call_without_a_reference_fails(rig):
    mb, rec, emu, dev = rig
    c = mc.CASES["pad8"]
    inp = mc.make_inputs("pad8", c)
    r = mc.run_mha(mb, rec, c, inp, dev, mc.mode_of({}))
    r.bwd.append(r.bwd[-1])
    with pytest.raises(AssertionError, match="without a reference"):
        mc.check_run(mc.Report("extra call"), emu, r, inp)


@pytest.mark.parametrize("case", ["tn_min", "large8", "pad96", "pad8"])
def test_fp64_formulas_equal_fp64_autograd(case):
    """mha_graph (the definition the control chain is built on) against autograd of nn.MultiheadAttention + residual + LayerNorm"""
    c = mc.CASES[case]
    inp = mc.make_inputs(case, c)
    a = mc.graph_grads(mc.mha_graph, inp.x, inp.prm, c["H"], c["lens"], inp.dout, emulate=False)
    b = mc.nn_autograd(inp.x, inp.prm, c["H"], c["lens"], inp.dout)
    for n in a:
        if n == "bi":           # the key bias gradient is rounding noise around zero in both
            Dm = c["Dm"]
            assert float(a[n][Dm: 2 * Dm].abs().max()) < 1e-12 and float(b[n][Dm: 2 * Dm].abs().max()) < 1e-12
        for k, (u, v) in enumerate(zip(a[n].reshape(3, -1) if n == "bi" else [a[n]], b[n].reshape(3, -1) if n == "bi" else [b[n]])):
            if n == "bi" and k == 1:
                continue
            assert mc.rel_l2(u, v) < 1e-12, (n, mc.rel_l2(u, v))


@pytest.mark.parametrize("case", ["pad96", "pad8"])
def test_padded_head_layout_equals_the_unpadded_module(case):
    """attention through padded_weights (heads of dh columns, scale dh_true^-0.5, zero padding) == the unpadded definition in fp64,
    and the gradients of the padded copies, sliced as the block slices them, == the module's"""
    c = mc.CASES[case]
    G = mc.geom(c)
    inp = mc.make_inputs(case, c)
    B, S, Dm, H, dh, dt = G.B, G.S, G.Dm, G.H, G.dh, G.dh_true
    P = {k: v.double() for k, v in inp.prm.items()}
    Wi_p, bi_p, Wo_p = (t.clone().requires_grad_() for t in mc.padded_weights(P["Wi"], P["bi"], P["Wo"], H, dh))
    x = inp.x.double()
    qkv = x @ Wi_p.t() + bi_p
    q, k, v = (t.reshape(B, S, H, dh).transpose(1, 2) for t in qkv.split(G.D, dim=-1))
    pad = torch.arange(S)[None, :] >= torch.tensor(c["lens"])[:, None]
    Pm = torch.softmax(((q @ k.transpose(-1, -2)) * dt ** -0.5).masked_fill(pad[:, None, None, :], float("-inf")), -1)
    ctx = (Pm @ v).transpose(1, 2).reshape(B, S, G.D)
    out = torch.nn.functional.layer_norm(ctx @ Wo_p.t() + P["bo"] + x, (Dm,), P["g"], P["beta"], mc.EPS)
    (out * inp.dout.double()).sum().backward()
    ref = mc.graph_grads(mc.mha_graph, inp.x, inp.prm, H, c["lens"], inp.dout, emulate=False)
    assert mc.rel_l2(out.detach(), ref["out"]) < 1e-13
    gWi = Wi_p.grad.view(3, H, dh, Dm)
    assert mc.rel_l2(gWi[:, :, :dt].reshape(3 * Dm, Dm), ref["Wi"]) < 1e-12
    assert mc.rel_l2(Wo_p.grad.view(Dm, H, dh)[:, :, :dt].reshape(Dm, Dm), ref["Wo"]) < 1e-12
    gb = bi_p.grad.view(3, H, dh)[:, :, :dt].reshape(3, Dm)
    assert mc.rel_l2(gb[0], ref["bi"][:Dm]) < 1e-12 and mc.rel_l2(gb[2], ref["bi"][2 * Dm:]) < 1e-12
    # q / k padding meets zero columns of the other operand: its weight gradient is exactly zero; v padding meets zero columns of Wo_p
    assert float(gWi[:2, :, dt:].abs().max()) == 0.0


@pytest.mark.parametrize("case", ["tn_min", "pad96"])
def test_whole_block_criterion_on_the_emulation(rig, case):
    """rel-L2(emulation, control) <= rel-L2(control, fp64) + F32_RELL2 for the output, the input gradient and every parameter gradient"""
    mb, rec, emu, dev = rig
    c = mc.CASES[case]
    inp = mc.make_inputs(case, c)
    r = mc.run_mha(mb, rec, c, inp, dev, mc.mode_of({}))
    hip = dict(r.grads, out=r.out, x=r.dx)
    ctrl = mc.graph_grads(mc.mha_graph, inp.x, inp.prm, c["H"], c["lens"], inp.dout, emulate=True)
    ref = mc.nn_autograd(inp.x, inp.prm, c["H"], c["lens"], inp.dout)
    rows = mc.whole_block_rows(hip, ctrl, ref, c["Dm"])
    for n, e_hc, e_cf in rows:
        print(f"[mha-block] {case:>10s} whole block (emulation) {n:6s} rel-L2(emu, control) {e_hc:9.3g}   rel-L2(control, fp64) {e_cf:9.3g}")
    bad = [x for x in rows if not x[1] <= x[2] + mc.F32_RELL2]
    assert not bad, bad
    assert len(rows) == 8


def test_encoder_graph_equals_the_stock_encoder_in_fp64():
    """encoder_graph (the fp64 definition behind the feed-forward case's control) against nn.TransformerEncoder itself"""
    c = mc.FFN_CASE
    inp = mc.make_inputs("ffn", c)
    a = mc.graph_grads(mc.encoder_graph, inp.x, inp.prm, c["H"], c["lens"], inp.dout, emulate=False)
    enc = mc.build_encoder(c, inp.prm, torch.device("cpu"), 0.0).double()
    x = inp.x.double().requires_grad_()
    pad = torch.arange(c["S"])[None, :] >= torch.tensor(c["lens"])[:, None]
    out = enc.model(x, src_key_padding_mask=pad)
    (out * inp.dout.double()).sum().backward()
    assert mc.rel_l2(a["out"], out.detach()) < 1e-12 and mc.rel_l2(a["x"], x.grad) < 1e-12
    for n, p in mc.encoder_params(enc).items():
        if n != "bi":
            assert mc.rel_l2(a[n], p.grad) < 1e-11, n
