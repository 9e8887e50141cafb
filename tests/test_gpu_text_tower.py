"""GPU: the frozen CLIP text tower as the product runs it - clip_text_hip.KeywordTowerFn / TextTowerFn over tower_forward and
tower_backward - stage by stage against float64, element by element, forward and input gradient, every layer.

Nothing of the forward or backward is restated and nothing is added to the product: a recording proxy replaces the ``ops`` attribute
of speechclip_plus_amd.clip_text_hip (tests/test_gpu_frozen_fwd.py's _FwdRec with ``per_op`` off, here also keeping what a call
returned), clones every argument before and after each call, and the recorded calls are turned into the stages of
tests/text_tower_cases.py, which holds the cases, the fp64 references, the bounds (docs/parity.md, "Frozen CLIP text tower"; fixed
before the first GPU run) and the planted errors.  On top of the stage checks: the prompt kernels and the working copies bit for bit,
exact zeros in every gradient row behind an EOT or in a pad sequence, causal independence under +-100 noise in those rows,
repeatability, KeywordTowerFn == TextTowerFn, the placement of a sequence inside an attention block, a sensitivity check per criterion
and the per-sequence end-to-end error against the bf16-storage control.

Measured on one MI355X (the figures docs/parity.md tabulates): see the section's "Measured" table."""
import inspect

import pytest
import torch

import attn_cases as ac
import text_tower_cases as tc
from test_gpu_frozen_fwd import _FwdRec, _cl
from test_gpu_trainable_bwd import _Seq

pytestmark = pytest.mark.gpu

END_TO_END = 1.5        # err_HIP <= 1.5 err_ctl per sequence: both carry independent rounding noise of the same size over thousands of
#                         elements, so the ratio concentrates near 1; a lost keyword or a lost layer moves it by an order of magnitude


class _Rec(_FwdRec):
    """_FwdRec (every argument cloned before and after the call) that also keeps a clone of what the call returned: the tower's
    kernels return fresh tensors instead of filling ``out=`` arguments"""

    def __getattr__(self, name):
        w = _FwdRec.__getattr__(self, name)
        if not inspect.isfunction(w):
            return w

        def keep(*a, **kw):
            n = len(self.calls)
            r = w(*a, **kw)
            if len(self.calls) == n + 1:
                self.calls[n].ret = _cl(r)
            return r
        return keep


class _Ctx:
    def __init__(self, cth, rec):
        self.cth, self.rec, self.dev = cth, rec, torch.device("cuda:0")
        self._clips, self._runs = {}, {}

    def clip(self, W):
        if W not in self._clips:
            self._clips[W] = tc.make_clip(W).to(self.dev)
        return self._clips[W]

    def consts(self, W):
        clip = self.clip(W)
        tok, pos = clip._prompt_constants(self.dev)
        return clip, clip._tower_weights(self.dev), tok, pos

    def keyword(self, W, heads, kw, counts, d_rows, n_pos, record=True):
        """one KeywordTowerFn forward + backward -> dict(calls, rows, dk)"""
        clip, weights, tok, pos = self.consts(W)
        kw = kw.to(self.dev).clone().requires_grad_()
        self.rec.calls, self.rec.on = [], record
        try:
            rows = self.cth.KeywordTowerFn.apply(kw, counts.to(self.dev), tok, pos, weights, heads, n_pos, clip.eot_clamped)
            rows.backward(d_rows.to(self.dev))
            torch.cuda.synchronize()
        finally:
            self.rec.on = False
        return dict(calls=self.rec.calls, rows=rows.detach(), dk=kw.grad.detach())

    def text(self, W, heads, x, dy, record=True):
        clip, weights, _, _ = self.consts(W)
        x = x.to(self.dev).clone().requires_grad_()
        self.rec.calls, self.rec.on = [], record
        try:
            y = self.cth.TextTowerFn.apply(x, weights, heads)
            y.backward(dy.to(self.dev))
            torch.cuda.synchronize()
        finally:
            self.rec.on = False
        return dict(calls=self.rec.calls, y=y.detach(), dx=x.grad.detach())

    def run(self, name):
        """the case's recorded run, made once: + stages, misc (the calls around the tower), inputs, the dead-row mask"""
        if name not in self._runs:
            c, inp = tc.CASES[name], tc.case_inputs(name)
            n_pos = tc.n_pos_of(name)
            assert self.cth._geometry(c["B"], n_pos)[:3] == (c["SEG"], c["Bp"], c["M"]), name
            if c["path"] == "keyword":
                r = self.keyword(c["W"], c["heads"], inp["keywords"], inp["counts"], inp["d_rows"], n_pos)
                counts = inp["counts"].tolist()
            else:
                r = self.text(c["W"], c["heads"], inp["x"], inp["dy"])
                counts = [n_pos - 2] * c["B"]                                  # every row below T is live
            r["stages"], r["misc"] = _stages(r["calls"], c["SEG"], c["heads"], c["path"] == "keyword", n_pos)
            r.update(inp=inp, counts=counts, live=tc.live_rows(counts, c["Bp"], c["SEG"], self.dev), n_pos=n_pos)
            self._runs[name] = r
        return self._runs[name]


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from speechclip_plus_amd import clip_text_hip as cth
    if cth.FOLD_LN:
        pytest.skip("SC_TOWER_FOLD_LN=1: the LayerNorms run in the GEMM prologues; the stages of this module are the default chain's")
    mp = pytest.MonkeyPatch()
    rec = _Rec(cth.ops)
    mp.setattr(cth, "ops", rec)
    yield _Ctx(cth, rec)
    mp.undo()


# ---------------------------------------------------------------------------------------------------------------- calls -> stages
def _tile(M, N, K, n_cu):
    """the tile sc_gemm_bf16's cost model picks for a plain launch below the 256-row kernel's threshold (csrc/gemm_bf16.hip)"""
    t64, t128 = -(-M // 64) * -(-N // 64), -(-M // 128) * -(-N // 128)
    assert not (M >= 512 and N >= 192 and -(-M // 256) * -(-N // 256) >= 192)
    return "64x64x4" if (K >= 512 and t64 <= 2 * n_cu) else "128x64" if t128 <= 2 * n_cu else "128x128"


def _stages(calls, SEG, heads, keyword, n_pos):
    """Walks the recorded calls in the order the product issued them, asserts that every call read what the call before it wrote
    (torch.equal) and that the backward read what the forward saved, and returns the stages + the calls around the tower."""
    eq = torch.equal
    sq, st, misc, fwd = _Seq(calls), [], {}, []
    lin_bias = lambda c: c.a[2] if len(c.a) > 2 else None
    X = None
    if keyword:
        misc["assemble"] = c = sq.take("prompt_assemble")
        X = c.ret[0]
    n_layers = sum(c.name == "layernorm_bf16" for c in calls) // 2
    assert n_layers == tc.LAYERS
    for li in range(n_layers):
        t = f"layer {li} "
        c = sq.take("layernorm_bf16")
        assert (X is None or eq(c.a[0], X)) and c.kw["eps"] == tc.EPS
        Xl, h = c.a[0], c.ret
        M, W = Xl.shape
        NB = M // 128
        st.append(dict(kind="ln", name=t + "ln_1", x=Xl, g=c.a[1], b=c.a[2], got=h))
        c = sq.take("linear_bf16")
        assert eq(c.a[0], h) and not c.kw
        qkv = c.ret
        st.append(dict(kind="gemm", name=t + "QKV", A=h, W=c.a[1], bias=lin_bias(c), got=qkv))
        if SEG == 32:
            c = sq.take("attn32_fwd")
            assert eq(c.a[0], qkv) and c.a[1] == heads and c.a[2] == 0.125
            att, lse2 = c.ret, None
        else:
            c = sq.take("head_transpose")
            assert eq(c.a[0], qkv[:, 2 * W:])
            vt = c.ret
            assert eq(vt, qkv[:, 2 * W:].view(NB, 128, heads, 64).permute(0, 2, 3, 1)), "head_transpose: not the transpose, bit for bit"
            c = sq.take("attn_fwd")
            assert eq(c.a[0], qkv[:, : 2 * W]) and eq(c.a[1], vt) and c.kw["causal"] == (1 if SEG == 128 else SEG)
            assert c.a[2].tolist() == [128] * NB and tuple(c.a[4:9]) == (NB, 128, heads, W, 0.125)
            att, lse2 = c.pa[3], c.pkw["lse2"]
        st.append(dict(kind="attn_fwd", name=t + "attention", qkv=qkv, SEG=SEG, out=att, lse2=lse2))
        c = sq.take("linear_bf16")
        assert eq(c.a[0], att) and eq(c.kw["residual"], Xl)
        X2 = c.ret
        st.append(dict(kind="gemm", name=t + "out_proj + residual", A=att, W=c.a[1], bias=lin_bias(c), res=Xl, got=X2))
        c = sq.take("layernorm_bf16")
        assert eq(c.a[0], X2)
        h2 = c.ret
        st.append(dict(kind="ln", name=t + "ln_2", x=X2, g=c.a[1], b=c.a[2], got=h2))
        c = sq.take("linear_bf16")
        assert eq(c.a[0], h2) and c.kw["act"] == 2 and c.kw["aux_mode"] == 1
        u, f = c.pkw["aux"], c.ret
        st.append(dict(kind="fc1", name=t + "fc1", A=h2, W=c.a[1], bias=lin_bias(c), u=u, f=f))
        c = sq.take("linear_bf16")
        assert eq(c.a[0], f) and eq(c.kw["residual"], X2)
        X = c.ret
        st.append(dict(kind="gemm", name=t + "fc2 + residual", A=f, W=c.a[1], bias=lin_bias(c), res=X2, got=X))
        fwd.append((Xl, qkv, att, lse2, X2, u))
    misc["out"] = X
    dX = None
    if keyword:
        misc["gather"] = c = sq.take("rows_gather")
        assert eq(c.a[0], X)
        misc["scatter"] = c = sq.take("rows_scatter")
        dX = c.ret
    for li in range(n_layers - 1, -1, -1):
        t = f"layer {li} bwd "
        Xl, qkv, att, lse2, X2, u = fwd[li]
        c = sq.take("linear_bf16")
        assert (dX is None or eq(c.a[0], dX)) and c.kw["act"] == 2 and c.kw["aux_mode"] == 2 and eq(c.kw["aux"], u) and len(c.a) == 2
        dX, du = c.a[0], c.ret
        misc.setdefault("dX_in", dX)
        st.append(dict(kind="aux2", name=t + "fc2 dgrad x QuickGELU'", A=dX, W=c.a[1], u=u, got=du))
        c = sq.take("linear_bf16")
        assert eq(c.a[0], du) and len(c.a) == 2 and not c.kw
        dh2 = c.ret
        st.append(dict(kind="gemm", name=t + "fc1 dgrad", A=du, W=c.a[1], got=dh2))
        c = sq.take("layernorm_bwd")
        assert eq(c.a[0], X2) and eq(c.a[1], dh2) and eq(c.kw["dres"], dX) and c.a[3] == tc.EPS and set(c.kw) == {"dres"}
        dX2 = c.ret
        st.append(dict(kind="ln_bwd", name=t + "ln_2' + dres", x=X2, dy=dh2, g=c.a[2], dres=dX, got=dX2))
        c = sq.take("linear_bf16")
        assert eq(c.a[0], dX2) and len(c.a) == 2 and not c.kw
        datt = c.ret
        st.append(dict(kind="gemm", name=t + "out_proj dgrad", A=dX2, W=c.a[1], got=datt))
        M, W = Xl.shape
        if SEG == 32:
            c = sq.take("attn32_bwd")
            assert eq(c.a[0], qkv) and eq(c.a[1], datt)
            dqkv = c.ret
        else:
            c = sq.take("attn_bwd")
            assert all(eq(c.a[i], qkv[:, i * W: (i + 1) * W]) for i in range(3)) and eq(c.a[3], att) and eq(c.a[4], datt) and eq(c.a[5], lse2)
            assert c.kw["causal"] == (1 if SEG == 128 else SEG) and c.kw["q_rows"] == (128 if SEG < 128 else n_pos)
            dqkv = torch.cat([c.pa[7], c.pa[8], c.pa[9]], dim=1)
        st.append(dict(kind="attn_bwd", name=t + "attention", qkv=qkv, dout=datt, SEG=SEG, dqkv=dqkv))
        c = sq.take("linear_bf16")
        assert eq(c.a[0], dqkv) and len(c.a) == 2 and not c.kw
        dh1 = c.ret
        st.append(dict(kind="gemm", name=t + "QKV dgrad", A=dqkv, W=c.a[1], got=dh1))
        c = sq.take("layernorm_bwd")
        assert eq(c.a[0], Xl) and eq(c.a[1], dh1) and eq(c.kw["dres"], dX2)
        dX = c.ret
        st.append(dict(kind="ln_bwd", name=t + "ln_1' + dres", x=Xl, dy=dh1, g=c.a[2], dres=dX2, got=dX))
    misc["dX_out"] = dX
    if keyword:
        misc["assemble_bwd"] = c = sq.take("prompt_assemble_bwd")
        assert eq(c.a[0], dX)
    assert sq.done()
    return st, misc


# ---------------------------------------------------------------------------------------------------------------- stage by stage
@pytest.mark.parametrize("name", list(tc.CASES))
def test_stage_by_stage_vs_fp64(ctx, name):
    """every recorded call of the forward and the backward, every layer, against its fp64 definition on its own recorded inputs; the
    test fails once, with all its violations"""
    from speechclip_plus_amd import ops
    r = ctx.run(name)
    c = tc.CASES[name]
    rep = tc.Report()
    n_cu = ops._num_cus()
    for st in r["stages"]:
        if st["kind"] in ("gemm", "fc1", "aux2"):
            (M, K), N = st["A"].shape, st["W"].shape[0]
            print(f"TILE|{name}|{st['name']}|{M} x {N} x {K}|{_tile(M, N, K, n_cu)}")
        tc.check_stage(rep, name, st)
    if n_cu == 256:         # the tile instances the case table names (the cost model depends on the CU count)
        tiles = {st["name"]: _tile(st["A"].shape[0], st["W"].shape[0], st["A"].shape[1], n_cu) for st in r["stages"] if st["kind"] in ("gemm", "fc1", "aux2")}
        if name == "A":
            assert set(tiles.values()) == {"64x64x4"}, tiles
        if name == "B":
            wide = {k for k, v in tiles.items() if v == "128x64"}
            assert wide == {f"layer {i} {s}" for i in (0, 1) for s in ("QKV", "fc1", "bwd fc2 dgrad x QuickGELU'")}, tiles
            assert set(tiles.values()) == {"128x64", "64x64x4"}, tiles
    # the tower's output and input gradient as the autograd function hands them on
    if c["path"] == "keyword":
        rep.require(name, "KeywordTowerFn's rows are not the output's EOT rows", torch.equal(r["rows"], r["misc"]["gather"].ret))
        rep.require(name, "KeywordTowerFn's gradient is not prompt_assemble_bwd's", torch.equal(r["dk"], r["misc"]["assemble_bwd"].ret))
    else:
        B, T, SEG = c["B"], c["T"], c["SEG"]
        rep.require(name, "TextTowerFn's output is not the rows below T", torch.equal(r["y"], r["misc"]["out"].view(c["Bp"], SEG, -1)[:B, :T].float()))
        rep.require(name, "TextTowerFn's gradient is not the rows below T", torch.equal(r["dx"], r["misc"]["dX_out"].view(c["Bp"], SEG, -1)[:B, :T].float()))
    rep.done()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_prompt_kernels_bit_exact(ctx, name):
    """prompt_assemble, rows_gather, rows_scatter and prompt_assemble_bwd against the element-wise formulation, bit for bit (SEG 32, 64
    and 128: cases C and D are the ones no other test reaches)"""
    r = ctx.run(name)
    c, inp, m = tc.CASES[name], r["inp"], r["misc"]
    _, _, tok, pos = ctx.consts(c["W"])
    dev = ctx.dev
    kw, counts = inp["keywords"].to(dev), inp["counts"]
    X, eot = tc.assemble_ref(kw, counts, tok, pos, c["Bp"], c["SEG"], r["n_pos"])
    a = m["assemble"]
    assert tuple(a.a[4:7]) == (c["Bp"], c["SEG"], r["n_pos"])
    assert torch.equal(a.ret[1], eot) and torch.equal(a.ret[0], X)
    assert torch.equal(m["gather"].ret, m["out"][eot.long()].float())
    want = torch.zeros(c["M"], c["W"], device=dev, dtype=torch.bfloat16)
    want[eot.long()] = inp["d_rows"].to(dev).to(torch.bfloat16)
    assert tuple(m["scatter"].a[2:4]) == (c["M"], c["SEG"]) and torch.equal(m["scatter"].ret, want)
    dX = m["dX_out"].view(c["Bp"], c["SEG"], c["W"])
    dk = torch.zeros(c["B"], c["N"], c["W"], device=dev)
    for b, n in enumerate(counts.tolist()):
        dk[b, :n] = dX[b, 1: n + 1].float()
    assert torch.equal(m["assemble_bwd"].ret, dk)
    assert int(ctx.clip(c["W"]).eot_clamped) == 0


def test_working_copies_match_the_weights(ctx):
    """every working copy of prepare_weights == bf16(weight) / bf16(weight.t()), contiguous; biases and LayerNorm vectors in fp32"""
    for W in (512, 768):
        clip, weights, _, _ = ctx.consts(W)
        bf = lambda t: t.detach().to(torch.bfloat16)
        for w, blk in zip(weights, clip.model.transformer.resblocks):
            for n, src in (("wqkv", blk.attn.in_proj_weight), ("wo", blk.attn.out_proj.weight), ("w1", blk.mlp.c_fc.weight), ("w2", blk.mlp.c_proj.weight)):
                a, aT = getattr(w, n), getattr(w, n + "T")
                assert a.is_contiguous() and aT.is_contiguous() and torch.equal(a, bf(src)) and torch.equal(aT, bf(src).t()), (W, n)
            for n, src in (("bqkv", blk.attn.in_proj_bias), ("bo", blk.attn.out_proj.bias), ("b1", blk.mlp.c_fc.bias), ("b2", blk.mlp.c_proj.bias),
                           ("g1", blk.ln_1.weight), ("be1", blk.ln_1.bias), ("g2", blk.ln_2.weight), ("be2", blk.ln_2.bias)):
                assert getattr(w, n).dtype == torch.float32 and torch.equal(getattr(w, n), src.detach()), (W, n)
            assert (w.eps1, w.eps2) == (tc.EPS, tc.EPS)


# ---------------------------------------------------------------------------------------------------------------- exact zeros
@pytest.mark.parametrize("name", list(tc.CASES))
def test_dead_rows_carry_exactly_zero_gradient(ctx, name):
    """clip_text_hip's promise, at every layer of the backward and in every recorded gradient tensor: every row behind its sequence's EOT
    (rows n_pos .. SEG - 1 included) and every row of a pad sequence is exactly zero, and everything is finite.  Case E (a dense dy on
    the rows below T): the rows T .. SEG - 1."""
    r = ctx.run(name)
    rep = tc.Report()
    live = r["live"]
    assert int((~live).sum()) > 0
    n = 0
    for st in r["stages"]:
        if " bwd " in st["name"]:
            n += 1
            tc.check_dead_rows(rep, name, st["name"], st["dqkv"] if st["kind"] == "attn_bwd" else st["got"], live)
    assert n == 7 * tc.LAYERS
    tc.check_dead_rows(rep, name, "the gradient that enters the tower", r["misc"]["dX_in"], live)
    for st in r["stages"]:                                             # the forward stays finite on every row
        for k in ("got", "out", "u", "f"):
            if k in st and " bwd " not in st["name"]:
                rep.require(name, f"{st['name']}: not finite", bool(torch.isfinite(st[k].float()).all()))
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- causal independence
def _tower(ctx, name, X, dX):
    """the recorded tower_forward / tower_backward once more, on the given rows -> (every layer's output, the input gradient)"""
    c = tc.CASES[name]
    _, weights, _, _ = ctx.consts(c["W"])
    _, _, _, causal = ctx.cth._geometry(c["B"], tc.n_pos_of(name))
    out, saved = ctx.cth.tower_forward(X.clone(), weights, c["heads"], causal)
    outs = [s[0] for s in saved[1:]] + [out]
    g = ctx.cth.tower_backward(dX.clone(), weights, saved, c["heads"], causal, 128 if c["SEG"] < 128 else tc.n_pos_of(name))
    torch.cuda.synchronize()
    return outs, g


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_causal_independence(ctx, name):
    """every row behind a sequence's EOT and every row of a pad sequence overwritten with finite +-100 noise: the rows up to the EOT keep
    their bits in every layer's output and in the input gradient, which stays exactly zero behind them"""
    r = ctx.run(name)
    live, m = r["live"], r["misc"]
    X, dX = m["assemble"].ret[0], m["scatter"].ret
    outs, g = _tower(ctx, name, X, dX)
    assert torch.equal(outs[-1], m["out"]) and torch.equal(g, m["dX_out"])            # the replay reproduces the recorded run
    gen = torch.Generator().manual_seed(77)
    noise = ((torch.randint(0, 2, tuple(X.shape), generator=gen).float() * 2 - 1) * 100 * (0.5 + torch.rand(tuple(X.shape), generator=gen)))
    Xn = torch.where(live[:, None], X, noise.to(ctx.dev).to(torch.bfloat16))
    assert bool((Xn[~live].float().abs() >= 50).all())
    outs_n, g_n = _tower(ctx, name, Xn, dX)
    for li, (a, b) in enumerate(zip(outs, outs_n)):
        assert torch.equal(a[live], b[live]), f"{name}: layer {li}'s live rows changed with the rows behind the EOT"
        assert bool(torch.isfinite(b.float()).all())
    assert torch.equal(g[live], g_n[live]), f"{name}: the input gradient's live rows changed"
    assert float(g_n[~live].float().abs().max()) == 0.0 and bool(torch.isfinite(g_n.float()).all())


# ---------------------------------------------------------------------------------------------------------------- other invariants
@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_repeatability_and_keyword_fn_equals_text_fn(ctx, name):
    """two runs give identical bits (forward rows, input gradient); KeywordTowerFn == TextTowerFn on the element-wise prompt at
    T = n_pos, bitwise, on the EOT rows and on the keyword gradient"""
    r = ctx.run(name)
    c, inp = tc.CASES[name], r["inp"]
    again = ctx.keyword(c["W"], c["heads"], inp["keywords"], inp["counts"], inp["d_rows"], r["n_pos"], record=False)
    assert torch.equal(again["rows"], r["rows"]) and torch.equal(again["dk"], r["dk"])
    _, _, tok, pos = ctx.consts(c["W"])
    x = tc.prompt_fp32(inp["keywords"].to(ctx.dev), inp["counts"], tok, pos, r["n_pos"])
    dy = torch.zeros_like(x)
    for b, n in enumerate(r["counts"]):
        dy[b, n + 1] = inp["d_rows"][b].to(ctx.dev)
    t = ctx.text(c["W"], c["heads"], x, dy, record=False)
    for b, n in enumerate(r["counts"]):
        assert torch.equal(t["y"][b, n + 1], r["rows"][b]), (name, b)
        assert torch.equal(t["dx"][b, 1: n + 1], r["dk"][b, :n]), (name, b)
        assert float(r["dk"][b, n:].abs().max() if n < c["N"] else 0.0) == 0.0


def _placed(ctx, W, heads, N, n, slot, B, seed):
    """a prompt of n keywords in slot ``slot`` of a batch of B (the others: other keywords, other counts) -> recorded run"""
    g = torch.Generator().manual_seed(seed)
    kw = torch.randn(B, N, W, generator=torch.Generator().manual_seed(seed + 1)) * 0.02
    mine = torch.randn(N, W, generator=g) * 0.02
    d = torch.randn(B, W, generator=torch.Generator().manual_seed(seed + 2))
    d_mine = torch.randn(W, generator=g)
    kw[slot], d[slot] = mine, d_mine
    counts = torch.tensor([(n + 3 * (b + 1)) % (N + 1) for b in range(B)], dtype=torch.int64)
    counts[slot] = n
    r = ctx.keyword(W, heads, kw, counts, d, min(77, N + 2))
    r["slot"], r["n"] = slot, n
    return r


def test_placement_in_the_block_seg32(ctx):
    """SEG = 32: a sequence alone (B = 1) and the same sequence in slot 3 of a four-sequence block give identical bits, forward and
    gradient - attn32_* is one wave per (sequence, head), and no GEMM, LayerNorm or epilogue depends on the row's position"""
    a = _placed(ctx, 512, 8, 8, 6, 0, 1, 900)
    b = _placed(ctx, 512, 8, 8, 6, 3, 4, 900)
    assert torch.equal(a["rows"][0], b["rows"][3]) and torch.equal(a["dk"][0], b["dk"][3])
    assert float(a["dk"][0, :6].abs().max()) > 0


def test_placement_in_the_block_seg64(ctx):
    """SEG = 64: the same sequence as the first and as the second segment of a 128-row attention block.  The flash kernel walks other key
    blocks for the second segment, so the attention outputs are compared within the sum of the two bounds (layer 0, whose inputs must
    agree to the bit); whether the bits agree is printed, nothing more is asserted."""
    a = _placed(ctx, 512, 8, 40, 37, 0, 1, 901)
    b = _placed(ctx, 512, 8, 40, 37, 1, 2, 901)
    sa, _ = _stages(a["calls"], 64, 8, True, 42)
    sb, _ = _stages(b["calls"], 64, 8, True, 42)
    A = {s["name"]: s for s in sa}["layer 0 attention"]
    Bs = {s["name"]: s for s in sb}["layer 0 attention"]
    assert torch.equal(A["qkv"][:64], Bs["qkv"][64:128])
    fa, _ = tc.attn_fwd_stage_ref(A["qkv"], 64)
    fb, _ = tc.attn_fwd_stage_ref(Bs["qkv"], 64)
    oa, ob = tc.split_heads(A["out"], 128)[:8, :64], tc.split_heads(Bs["out"], 128)[:8, 64:]
    bound = fa["bound"][:8, :64] + fb["bound"][:8, 64:]
    rep = tc.Report()
    ac.check(rep, "placement SEG 64", "layer 0 attention, first against second segment", oa, ob, bound)
    print(f"PLACEMENT|SEG 64|layer 0 attention bits agree: {torch.equal(oa, ob)}|EOT rows agree: {torch.equal(a['rows'][0], b['rows'][1])}|"
          f"d keywords agree: {torch.equal(a['dk'][0], b['dk'][1])}")
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def test_each_criterion_rejects_its_planted_error(ctx):
    """every planted error of text_tower_cases.planted_suite on the device results of cases B (SEG 32, the recipe's row count) and C
    (SEG 64): the element-wise criterion alone must reject each"""
    for name in ("B", "C"):
        r = ctx.run(name)
        got = tc.planted_suite(r["stages"], name, tc.CASES[name]["SEG"], r["counts"])
        assert len(got) == 7 and all(v > 1.0 for v in got.values()), got
    # case A: attn32_fwd / attn32_bwd on the three-key prompt of the issue (count 1)
    r = ctx.run("A")
    got = tc.planted_suite(r["stages"], "A", 32, r["counts"])
    assert len(got) == 7 and all(v > 1.0 for v in got.values()), got


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_end_to_end_per_sequence(ctx, name):
    """EOT output row and d keywords of each sequence: rel-L2(HIP, fp64) <= 1.5 rel-L2(control, fp64) of the same sequence, the control
    being the fp64 chain with a bf16 rounding wherever the product stores bf16; a sequence whose reference gradient is exactly zero
    (count 0) must have an exactly zero result.  Both figures are printed per sequence."""
    r = ctx.run(name)
    c, m = tc.CASES[name], r["misc"]
    lw = tc.layer_weights(ctx.clip(c["W"]), ctx.dev)
    X, dX = m["assemble"].ret[0], m["scatter"].ret
    ref, gref, _ = tc.tower64(X, dX, lw, c["heads"], c["SEG"], rounded=False)
    ctl, gctl, _ = tc.tower64(X, dX, lw, c["heads"], c["SEG"], rounded=True)
    eot = m["assemble"].ret[1].tolist()
    rep = tc.Report()
    worst = [0.0, 0.0]
    for b, n in enumerate(r["counts"]):
        rows = slice(b * c["SEG"] + 1, b * c["SEG"] + 1 + n)
        eh, ec = tc.seq_rel_l2(r["rows"][b], ref[eot[b]]), tc.seq_rel_l2(ctl[eot[b]], ref[eot[b]])
        gh, gc = tc.seq_rel_l2(r["dk"][b, :n], gref[rows]), tc.seq_rel_l2(gctl[rows], gref[rows])
        print(f"E2E|{name} seq {b} count {n}|EOT row HIP {eh:.3e} control {ec:.3e} ratio {eh / ec:.3f}|"
              f"d keywords HIP {gh:.3e} control {gc:.3e}" + (f" ratio {gh / gc:.3f}" if gc > 0 else " (exactly zero)"))
        worst = [max(worst[0], eh / ec), max(worst[1], gh / gc if gc > 0 else 0.0)]
        rep.require(name, f"seq {b}: EOT row rel-L2 {eh:.3e} > {END_TO_END} x control {ec:.3e}", eh <= END_TO_END * ec)
        rep.require(name, f"seq {b} (count {n}): d keywords rel-L2 {gh:.3e} > {END_TO_END} x control {gc:.3e}", gh <= END_TO_END * gc)
        rep.require(name, f"seq {b}: gradient behind the keyword count not zero", n == c["N"] or float(r["dk"][b, n:].abs().max()) == 0.0)
    print(f"E2E|{name}|largest HIP / control: EOT row {worst[0]:.3f}, d keywords {worst[1]:.3f}")
    rep.done()
