"""GPU: the keyword attention block of the cascaded+ / hybrid+ recipes - speechclip_plus_amd/mha_block.py, MhaNormFn / FfnNormFn /
LayerNormFn as MultiheadAttentionAndNorm.forward / forward_rows and TransformerEncoder.forward run them - stage by stage against
float64, forward and backward.

Nothing of the block is restated on the device: a recording proxy replaces ``mha_block.ops`` and clones every argument before and
after each call; tests/mha_cases.py walks the recorded calls and compares each with the fp64 definition of that stage BY MEANING
(per utterance and head of the recorded qkv, never the call's strides), so the addressing written in mha_block.py is under test.  The
cases reach the TN form of dV / dK at the base recipe's own sequence length, the transposing form, hybrid+ large (8 x 128), zero-padded
heads (96 -> 128, 8 -> 64), the in-place modes of the train step (``rows``, ``rows_out``, accumulation into a flat gradient buffer)
and both dropout sites.  Bounds: docs/parity.md ("Keyword attention block"), fixed before the first GPU run and shown to hold for
the CPU emulation in tests/test_mha_cases_cpu.py."""
import copy

import pytest
import torch

import mha_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from speechclip_plus_amd import mha_block, ops
    mp = pytest.MonkeyPatch()
    rec = mc._Rec(ops)
    mp.setattr(mha_block, "ops", rec)
    yield mha_block, rec, ops, torch.device("cuda:0")
    mp.undo()


_cache = {}


def _run(rig, case, over, **kw):
    """one run per (case, mode), shared by the tests that only read it"""
    mb, rec, ops, dev = rig
    key = (case, mc.mode_id(over)) if not kw else None
    if key in _cache:
        return _cache[key]
    c = mc.CASES[case]
    inp = mc.make_inputs(case, c)
    r = mc.run_mha(mb, rec, c, inp, dev, mc.mode_of(over), **kw)
    if key is not None:
        _cache[key] = (r, inp)
    return r, inp


@pytest.mark.parametrize("case,over", mc.STAGE_RUNS, ids=[f"{n}-{mc.mode_id(o)}" for n, o in mc.STAGE_RUNS])
def test_stage_by_stage_vs_fp64(rig, case, over):
    """every recorded call of the forward and the backward against its fp64 definition; the walker fails on a call it has no
    reference for and asserts from the recorded arguments that the intended branch (TN / transposing, len_mask, acc, rows_out) was
    taken.  Then the sensitivity checks: errors planted on the host into the kernels' own results must each fail the element-wise
    criterion alone."""
    mb, rec, ops, dev = rig
    r, inp = _run(rig, case, over)
    rep = mc.Report(f"{case} {mc.mode_id(over)}")
    try:
        st = mc.check_run(rep, ops, r, inp)
    finally:
        rep.show()
    mode, G = r.mode, r.G
    names = {c.name for c in r.fwd + r.bwd}
    assert ("derived_pair" in names) == (not G.padded) and ("rows_zero_pad" in names) == (mode.rows_out is not None)
    assert any(c.kw.get("tn") for c in r.bwd if c.name == "gemm_raw") == G.tn
    if mode.rows is not None:       # the block read the buffer in place: its first product's A operand is no padded copy
        assert r.buf is not None and torch.equal(r.fwd[2].a[0], r.buf[mode.rows: mode.rows + G.M])
    if mode.p_res > 0:
        assert "dropout_bf16" in names
    for name in mc.assert_planted_rejected(st):
        print(f"[mha-block] {case:>10s} {mc.mode_id(over)}: rejected - {name}")
    # structural zeros of the in-place layouts
    if mode.rows is not None:
        lens = torch.tensor(G.lens, device=dev)
        s = torch.arange(G.Sp, device=dev)[None, :]
        off = mode.rows
        dead = (s < off) | (s >= off + lens[:, None])
        assert bool((r.dx[dead] == 0).all()), "rows mode: dx outside the live rows (leading off rows, pad rows)"
    if mode.rows_out is not None:
        n_cls, lead, trail = mode.rows_out, mb.ROWS_LEAD, mb.ROWS_TRAIL
        assert bool((r.out[:, :n_cls] == 0).all()) and bool((r.out[:, G.S:] == 0).all())
        assert bool((st.flat[:lead] == 0).all()) and bool((st.flat[lead + G.M:] == 0).all()) and st.flat.shape[0] == lead + G.M + trail
        if n_cls:
            assert torch.equal(r.cls, st.out_rows.view(G.B, G.Sp, G.Dm)[:, 0].float())
    if G.padded:                     # the sliced-away padding: gradients in the module's shapes
        assert r.grads["Wi"].shape == (3 * G.Dm, G.Dm) and r.grads["bi"].shape == (3 * G.Dm,) and r.grads["Wo"].shape == (G.Dm, G.Dm)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_encoder_layer_stage_by_stage_vs_fp64(rig, p):
    """TransformerEncoder.forward: MhaNormFn with the residual dropout, FfnNormFn (forward and backward) and LayerNormFn"""
    mb, rec, ops, dev = rig
    inp = mc.make_inputs("ffn", mc.FFN_CASE)
    r = mc.run_encoder(mb, rec, mc.FFN_CASE, inp, dev, p)
    rep = mc.Report(f"ffn p={p}")
    try:
        mc.check_encoder_run(rep, ops, r)
    finally:
        rep.show()
    assert ("dropout_bf16" in {c.name for c in r.fwd}) == (p > 0)
    if p == 0.0:
        _cache["ffn"] = (r, inp)


def _criterion(tag, rows, n_min):
    for n, e_hc, e_cf in rows:
        print(f"[mha-block] {tag:>10s} whole block {n:6s} rel-L2(HIP, control) {e_hc:9.3g}   rel-L2(control, fp64) {e_cf:9.3g}")
    bad = [x for x in rows if not x[1] <= x[2] + mc.F32_RELL2]
    assert not bad, bad
    assert len(rows) == n_min


@pytest.mark.parametrize("case", list(mc.CASES))
def test_whole_block_vs_bf16_storage_control(rig, case):
    """output, input gradient and every parameter gradient of MultiheadAttentionAndNorm.forward: the kernels add no more error than
    the storage format does - rel-L2(HIP, control) <= rel-L2(control, fp64) + F32_RELL2; fp64 = autograd of nn.MultiheadAttention +
    residual + LayerNorm on the unpadded module, control = the fp64 definition with bf16 at the product's storage sites"""
    mb, rec, ops, dev = rig
    r, inp = _run(rig, case, {})
    c = mc.CASES[case]
    hip = dict(r.grads, out=r.out, x=r.dx)
    x, prm, dout = inp.x.to(dev), {k: v.to(dev) for k, v in inp.prm.items()}, inp.dout.to(dev)
    ctrl = mc.graph_grads(mc.mha_graph, x, prm, c["H"], c["lens"], dout, emulate=True)
    ref = mc.nn_autograd(x, prm, c["H"], c["lens"], dout)
    _criterion(case, mc.whole_block_rows(hip, ctrl, ref, c["Dm"]), 8)
    # sensitivity: the in_proj weight gradient without the contribution of one frame of utterance 1
    dq = [cc for cc in r.bwd if cc.name == "wgrad_bf16"][1]
    G = r.G
    full = torch.outer(dq.a[0][G.Sp].double(), dq.a[1][G.Sp].double())
    one = full.view(3, G.H, G.dh, G.Dm)[:, :, : G.dh_true].reshape(3 * G.Dm, G.Dm) if G.padded else full
    e_bad = mc.rel_l2(hip["Wi"].double() - one, ctrl["Wi"])
    assert e_bad > mc.rel_l2(ctrl["Wi"], ref["Wi"]) + mc.F32_RELL2, "whole block: one-frame error not rejected"


def test_whole_encoder_layer_vs_bf16_storage_control(rig):
    mb, rec, ops, dev = rig
    c = mc.FFN_CASE
    if "ffn" not in _cache:
        inp = mc.make_inputs("ffn", c)
        _cache["ffn"] = (mc.run_encoder(mb, rec, c, inp, dev, 0.0), inp)
    r, inp = _cache["ffn"]
    hip = dict(r.grads, out=r.out, x=r.dx)
    x, prm, dout = inp.x.to(dev), {k: v.to(dev) for k, v in inp.prm.items()}, inp.dout.to(dev)
    ctrl = mc.graph_grads(mc.encoder_graph, x, prm, c["H"], c["lens"], dout, emulate=True)
    ref = mc.graph_grads(mc.encoder_graph, x, prm, c["H"], c["lens"], dout, emulate=False)
    _criterion("ffn", mc.whole_block_rows(hip, ctrl, ref, c["Dm"]), 16)


def _outputs(calls):
    out = []
    for i, c in enumerate(calls):
        for tag, v in (("ret", c.ret), ("args", c.pa), ("kw", tuple(c.pkw.values()))):
            for j, t in enumerate(v if isinstance(v, (tuple, list)) else (v,)):
                for k, u in enumerate(t if isinstance(t, (tuple, list)) else (t,)):
                    if isinstance(u, torch.Tensor):
                        out.append((f"{i} {c.name} {tag} {j}.{k}", u))
    return out


@pytest.mark.parametrize("case", ["base_tn", "large8", "tn_min"])
def test_bitwise_invariants(rig, case):
    """repeatability of every recorded output; neighbour reordering; rows mode == plain mode on a copy of the same rows; +-1e4 pad
    rows == zero pad rows; rows_out frames == the plain path's bf16 output rows; acc mode against the returned-gradient mode"""
    mb, rec, ops, dev = rig
    c = mc.CASES[case]
    G = mc.geom(c)
    B, S, Sp, Dm = G.B, G.S, G.Sp, G.Dm
    plain, inp = _run(rig, case, {})
    # ---- two runs: identical bits in every recorded output that the kernels wrote
    again = mc.run_mha(mb, rec, c, inp, dev, mc.mode_of({}))
    for (ta, a), (tb, b) in zip(_outputs(plain.fwd + plain.bwd), _outputs(again.fwd + again.bwd)):
        if "gemm_raw args" in ta and a.shape == (G.M, 3 * G.D):
            continue                                   # dqkv between its three products: the columns not yet written are uninitialised
        assert ta == tb and torch.equal(a, b), ta
    assert torch.equal(plain.out, again.out) and torch.equal(plain.dx, again.dx)
    for n in plain.grads:
        assert torch.equal(plain.grads[n], again.grads[n]), n
    # ---- utterance b keeps its bits when its neighbours are reordered
    perm = list(range(1, B)) + [0]
    c2 = dict(c, lens=[c["lens"][i] for i in perm])
    inp2 = copy.copy(inp)
    inp2.x, inp2.dout, inp2.dcls = inp.x[perm], inp.dout[perm], inp.dcls[perm]
    moved = mc.run_mha(mb, rec, c2, inp2, dev, mc.mode_of({}))
    for i, b in enumerate(perm):
        assert torch.equal(moved.out[i], plain.out[b]) and torch.equal(moved.dx[i], plain.dx[b]), (i, b)
    # ---- rows mode == plain mode fed a copy of the same rows; +-1e4 pad rows == zero pad rows
    for off in (0, 1):
        rows, _ = _run(rig, case, dict(rows=off))
        assert torch.equal(rows.out, plain.out), f"rows off={off}: out"
        assert torch.equal(rows.dx[:, off: off + S].float(), plain.dx), f"rows off={off}: dx"
        zero = mc.run_mha(mb, rec, c, inp, dev, mc.mode_of(dict(rows=off, junk=0.0)))
        assert torch.equal(zero.out, rows.out) and torch.equal(zero.dx, rows.dx), f"rows off={off}: pad-row junk reached a live row"
        for n in rows.grads:
            assert torch.equal(zero.grads[n], rows.grads[n]), f"rows off={off}: pad-row junk reached the gradient of {n}"
    # ---- rows_out frames == the plain path's bf16 output rows
    for n_cls in (0, 1):
        ro, _ = _run(rig, case, dict(rows_out=n_cls))
        assert torch.equal(ro.out[:, n_cls: S], plain.out[:, n_cls:].to(torch.bfloat16)), f"rows_out n_cls={n_cls}"
        assert bool((ro.out[:, :n_cls] == 0).all()) and bool((ro.out[:, S:] == 0).all())
        if n_cls:
            assert torch.equal(ro.cls, plain.out[:, 0])
    # ---- acc mode: out and dx bitwise; parameter gradients: the beta path adds the slices' sum s to the target in one fp32 addition
    # (csrc/headtail.hip: v = sum; v += beta * C), so post = fl(pre + s) and post - pre is s behind one rounding at |post| - not
    # bitwise, but within that rounding's share of the stage bound, KSEC u (|pre| + |post|)
    acc, _ = _run(rig, case, dict(acc=True))
    assert torch.equal(acc.out, plain.out) and torch.equal(acc.dx, plain.dx)
    for n in plain.grads:
        pre = acc.pre[n].double()
        post = pre + acc.grads[n].double()
        bound = mc.KSEC * mc.U * (pre.abs() + post.abs())
        d = (acc.grads[n].double() - plain.grads[n].double()).abs()
        print(f"[mha-block] {case:>10s} acc vs returned gradient {n:5s} max diff / bound {float((d / (bound + mc.FTZ)).max()):.3g}"
              f"   bitwise {bool(torch.equal(acc.grads[n], plain.grads[n]))}")
        assert bool((d <= bound).all()), n
