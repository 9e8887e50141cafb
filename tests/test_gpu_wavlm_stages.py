"""GPU: the frozen WavLM forward as the product runs it - FairseqSpeechEncoder_Hubert._encode on wavlm_base (post-LN, 12 heads) and
wavlm_large (pre-LN, 16 heads, LayerNorm convs, encoder.layer_norm on the output) at the shipped widths, two layers, random weights -
stage by stage against float64, element by element, on the operands each kernel received.

The rig is tests/test_gpu_frozen_fwd.py's (imported, not copied): the recording proxy in place of speech_encoder's ``ops``, the
stage checks and their bounds.  WavLM's layers run op by op by construction, so the proxy leaves ``_timer`` alone: the launches are
production's.  Every stage WavLM shares with HuBERT goes through the imported checks; new here are the table, the gate
(wavlm_cases.gate_ref, test_gate_kernel's criterion), the biased attention (attn_cases.fwd_ref with bias = gate x table, the BIAS
bound of docs/parity.md "Attention on peaked and drifting scores", as it stands) and the encoder's output LayerNorm of the pre-LN
order.  Only the two layouts a WavLM encoder can reach run: "segment" (ragged = True) and "flat" (ragged = False).

On top: bit-exact invariants (ragged == padded, repeatability, pad rows, plan and table re-use, replaced weights) and a
sensitivity check per new criterion.  docs/parity.md, "Frozen WavLM forward"."""
import dataclasses

import pytest
import torch

import head_cases as hc
import wavlm_cases as wc
from test_gpu_frozen_fwd import (BF16_RELL2, SMALL, _FwdRec, _Report, _Rig, _Seq, _check_conv, _check_linear, _check_ln, _check_posconv,
                                 _check_qkv, _junk, _keep, _vt_rows)

pytestmark = pytest.mark.gpu

# Lengths in samples; the chunk is L // T = 320 everywhere.  SMALL: 150 / 65 / 127 / 5 valid frames, segment pitches 152 / 72 / 136 / 8
# (M = 368), flat 4 x 152; the plan is the 64000-sample bucket's, R = 200, table [H, 399].  10 s: 160000 -> T = 499 and 82000 -> 257
# valid frames (one above a multiple of 64 and of 128), pitches 504 / 264: 8 key tiles, 4 query blocks, table [12, 1007].
TEN_S = [160000, 82000]
CASES = {                              # (arch, lengths, train)
    "base_small": ("wavlm_base", SMALL, False),
    "large_small": ("wavlm_large", SMALL, False),
    "base_10s": ("wavlm_base", TEN_S, False),
    "base_B1": ("wavlm_base", [33333], False),
    "base_train": ("wavlm_base", SMALL, True),
}
REL = "encoder.layers.0.self_attn.relative_attention_bias.weight"


class _WavRig(_Rig):
    """_Rig with a WavLM encoder; ``share``: another rig whose encoder (and weights) this one drives with its own batch"""

    def __init__(self, case, rec, seed=None, share=None):
        from speechclip_plus_amd import speech_encoder as se
        name, lens, train = CASES[case]
        self.case, self.large, self.lens, self.rec = case, name == "wavlm_large", list(lens), rec
        self.dev = torch.device("cuda:0")
        if share is None:
            self.arch = a = dataclasses.replace(se.ARCHS[name], layers=2)
            self.sd = se.random_wavlm_state_dict(a, seed=(97 + len(case)) if seed is None else seed)
            self.enc = se.FairseqSpeechEncoder_Hubert(name, arch=a, state_dict=self.sd, device="cuda:0")
            self.enc.train(train)
            self.rows_used = {}
        else:
            assert share.enc.name == name and share.enc.training == train
            self.arch, self.sd, self.enc, self.rows_used = share.arch, share.sd, share.enc, share.rows_used
        assert self.enc._dropout_active() == train
        g = torch.Generator().manual_seed(5 + len(case))
        w = torch.zeros(len(lens), max(lens))
        for b, l in enumerate(lens):
            w[b, :l] = torch.randn(l, generator=g) * 0.5
        self.wav = w.to(self.dev)

    def run(self, layout, record=True):
        assert layout in ("segment", "flat")          # the uniform B x R rows are out of a WavLM encoder's reach
        if self.enc.training:                         # the dropout seeds are a function of torch's seed: the same masks in every process
            torch.manual_seed(4242)
        run = super().run(layout, per_op=False, record=record)
        run.gate = run.pl.gate_rows(self.arch.heads, run.pl.M).clone()
        return run


@pytest.fixture(scope="module")
def rigs():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from speechclip_plus_amd import speech_encoder as se
    mp = pytest.MonkeyPatch()
    rec = _FwdRec(se.ops)
    mp.setattr(se, "ops", rec)
    made = {}

    def get(case, **kw):
        if kw:
            return _WavRig(case, rec, **kw)
        if case not in made:
            made[case] = _WavRig(case, rec)
        return made[case]

    yield get
    mp.undo()
    _WALKED.clear()


# ---------------------------------------------------------------------------------------------------------------- new stage checks
def _dev_f32(t, dev):
    return t.detach().float().contiguous().to(dev)


def _gate_refs(x, params, H):
    """fp64 reference and fp32 yardstick (torch on the CPU, as test_gate_kernel takes them) of the gate on the recorded rows"""
    x = x.cpu()
    wg, bg, cst = (p.detach().cpu().float().reshape(s) for p, s in zip(params, ((8, 64), (8,), (-1,))))
    return wc.gate_ref(x.double(), wg.double(), bg.double(), cst.double(), H), wc.gate_ref(x.float(), wg, bg, cst, H)


def _gate_params(sd, i):
    p = f"encoder.layers.{i}.self_attn."
    return sd[p + "grep_linear.weight"], sd[p + "grep_linear.bias"], sd[p + "grep_a"].reshape(-1)


def _check_gate(grep, rig, c, i, xin, tag):
    H = rig.arch.heads
    x, wg, bg, cst = c.a[:4]
    assert torch.equal(x, xin), f"{tag}: the gate reads other rows than the QKV GEMM"
    for got, want, n in zip((wg, bg, cst), _gate_params(rig.sd, i), ("grep_linear.weight", "grep_linear.bias", "grep_a")):
        assert torch.equal(got, _dev_f32(want, got.device).reshape(got.shape)), f"{tag}: {n} is not layer {i}'s"
    assert c.a[4] == H
    got = c.pkw["out"]
    assert got.shape == (H, x.shape[0])
    ref, yard = _gate_refs(x, (wg, bg, cst), H)
    grep.yard(f"{rig.case} {tag}", "gate", got.cpu(), ref, yard, dims=())
    return got


def _drop_of(c, lay):
    p = c.kw.get("drop_p", 0.0)
    return (lay.M, lay.max_pitch, c.kw.get("drop_seed", 0), p) if p > 0 else None


def _attn_refs(c, lay, H):
    """attn_cases.fwd_ref per utterance over its pitch, on the call's recorded operands"""
    return [wc.segment_attention_ref(c.a[0], c.a[1], c.kw["gate"], c.kw["table"], lay.r0[b], lay.pitch[b], lay.valid[b], H, c.a[8],
                                     drop=_drop_of(c, lay)) for b in range(lay.B)]


def _check_attn(rep, c, lay, H, stage):
    out = c.pa[3]
    refs = _attn_refs(c, lay, H)
    for b, f in enumerate(refs):
        r0, P = lay.r0[b], lay.pitch[b]
        rep.check(stage, out[r0: r0 + P].cpu(), wc.rows_of(f["out"]), wc.rows_of(f["bound"]), BF16_RELL2)
    return out, refs


def _walk(rep, grep, rig, run):
    """every recorded call of one forward, in the order the product issued them -> per layer the gate call, the attention call and
    its references"""
    a, w, lay, pl, sd = rig.arch, rig.enc._w, run.lay, run.pl, rig.sd
    H, dev = a.heads, rig.dev
    ln_mode = a.extractor_mode == "layer_norm"
    train = rig.enc.training
    assert lay.seg
    sq = _Seq(run.calls)
    sq.take("wav_prep_seg")
    sq.take("conv0_layernorm_gelu_seg" if ln_mode else "conv0_groupnorm_gelu_seg")            # tests/test_gpu_frontend.py
    prev = None
    for i in range(1, len(a.conv_kernels)):
        c = sq.take("gemm_raw")
        assert prev is None or torch.equal(c.a[0], prev)
        assert torch.equal(c.a[2], w[f"conv{i}_w"])
        prev = _check_conv(rep, rig, c, i)
        if ln_mode:
            c = sq.take("layernorm_bf16")
            assert torch.equal(c.a[0], prev[: c.a[0].shape[0]]) and c.kw["act"] == 1
            out = _check_ln(rep, c, f"conv {i} LayerNorm + GELU")
            prev = torch.cat([out, prev[out.shape[0]:]])
    c = sq.take("layernorm_bf16")
    assert torch.equal(c.a[0], prev[: lay.M])
    feat = _check_ln(rep, c, "feature LayerNorm")
    c = sq.take("linear_bf16")
    assert torch.equal(c.a[0], feat) and torch.equal(c.a[1], w["proj_w"])
    assert c.kw["drop_p"] == (a.dropout_input if train else 0.0)
    xp = _check_linear(rep, c, "post_extract_proj" + (" + dropout_input" if train else ""))
    c_prep = sq.take("posconv_prep_seg")
    assert torch.equal(c_prep.a[0], xp)
    c = sq.take("posconv_seg")
    x = _check_posconv(rep, rig, c_prep, c, lay)
    p_res = a.dropout if train else 0.0
    if not a.layer_norm_first:
        c = sq.take("layernorm_bf16")
        assert torch.equal(c.a[0], x)
        x = _check_ln(rep, c, "encoder LayerNorm")
        if p_res > 0:
            c = sq.take("dropout_bf16")
            assert torch.equal(c.a[0], x)
            keep = _keep(x.shape[0], x.shape[1], c.a[1], c.a[2], x.device)
            ref = torch.where(keep, x.float() / (1 - c.a[1]), torch.zeros((), device=x.device)).to(torch.bfloat16)
            assert torch.equal(c.pkw["out"], ref), "encoder dropout mask"
            rep.rows.setdefault("encoder dropout (bitwise)", (0.0, 0.0, ""))
            x = c.pkw["out"]
    assert torch.equal(run.hidden[0], x)
    # (1) the table: the fp32 bucket embedding of layer 0 gathered by offset for the plan's R, the same bits for every layer
    table = wc.bias_table(sd[REL].float(), pl.R).to(dev)
    assert table.shape == (H, 2 * pl.R - 1)
    layers = []
    for i in range(a.layers):
        tag = f"layer {i} "
        if a.layer_norm_first:
            c = sq.take("layernorm_bf16")
            assert torch.equal(c.a[0], x) and torch.equal(c.a[1], w[f"l{i}_ln1_g"])
            xin = _check_ln(rep, c, tag + "ln1")
        else:
            xin = x
        c = sq.take("gemm_raw")
        assert torch.equal(c.a[0], xin) and torch.equal(c.a[2], w[f"l{i}_qkv_w"])
        qk, vt = _check_qkv(rep, c, lay, tag + "QKV")
        # (2) the gate: the QKV GEMM's rows, layer i's parameters
        c_gate = sq.take("wavlm_gate")
        gate = _check_gate(grep, rig, c_gate, i, xin, tag + "gate")
        # (3) the biased attention
        c = sq.take("attn_fwd")
        assert torch.equal(c.a[0], qk) and torch.equal(c.a[1], vt) and c.kw["drop_p"] == (a.attention_dropout if train else 0.0)
        assert c.kw["table"].shape == (H, 2 * pl.R - 1) and torch.equal(c.kw["table"], table), tag + "table"
        assert torch.equal(c.kw["gate"], gate), tag + "the attention's gate is not the gate kernel's output"
        assert c.kw["seg"] is pl.seg and (c.a[6], c.a[7]) == (H, a.embed_dim)
        ctx, refs = _check_attn(rep, c, lay, H, tag + "biased attention")
        layers.append({"gate": c_gate, "attn": c, "refs": refs, "hidden": x})
        c = sq.take("linear_bf16")
        assert torch.equal(c.a[0], ctx) and torch.equal(c.a[1], w[f"l{i}_o_w"]) and torch.equal(c.kw["residual"], x)
        assert c.kw["drop_p"] == p_res
        pre = _check_linear(rep, c, tag + "out_proj + residual")
        c = sq.take("layernorm_bf16")
        assert torch.equal(c.a[0], pre)
        x1 = _check_ln(rep, c, tag + ("ln2" if a.layer_norm_first else "ln1"))
        c = sq.take("linear_bf16")
        assert torch.equal(c.a[0], x1) and torch.equal(c.a[1], w[f"l{i}_fc1_w"]) and c.kw["act"] == 1
        f = _check_linear(rep, c, tag + "fc1 + GELU")
        c = sq.take("linear_bf16")
        assert torch.equal(c.a[0], f) and torch.equal(c.a[1], w[f"l{i}_fc2_w"]) and c.kw["drop_p"] == p_res
        assert torch.equal(c.kw["residual"], pre if a.layer_norm_first else x1)
        x = _check_linear(rep, c, tag + "fc2 + residual")
        if not a.layer_norm_first:
            c = sq.take("layernorm_bf16")
            assert torch.equal(c.a[0], x)
            x = _check_ln(rep, c, tag + "ln2")
        if not (a.layer_norm_first and i + 1 == a.layers):
            assert torch.equal(run.hidden[i + 1], x)
    if a.layer_norm_first:
        # (4) pre-LN order: the encoder's output is encoder.layer_norm of the last layer's, in place in hidden[layers]
        c = sq.take("layernorm_bf16")
        assert torch.equal(c.a[0], x)
        assert torch.equal(c.a[1], _dev_f32(sd["encoder.layer_norm.weight"], dev)) and torch.equal(c.a[2], _dev_f32(sd["encoder.layer_norm.bias"], dev))
        x = _check_ln(rep, c, "encoder.layer_norm (output)")
        assert torch.equal(run.hidden[a.layers], x)
    assert sq.done(), f"call {sq.i} of {len(sq.c)}: {sq.c[sq.i].name} after the last stage"
    assert torch.equal(run.gate, layers[-1]["gate"].pkw["out"])
    # rows past the rows any batch has laid out in the plan's capacity-sized buffers were never written (a fresh plan is zero)
    top = rig.rows_used[id(pl)]
    for k, v in pl._rows.items():
        assert float(v[top:].abs().max() if v.shape[0] > top else 0.0) == 0.0, k
    return layers


_WALKED = {}


def _walked(rigs, case, layout):
    """one recorded forward per (case, layout) with its stage checks and references: computed once, shared, left unchanged"""
    key = (case, layout)
    if key not in _WALKED:
        rig = rigs(case)
        run = rig.run(layout)
        rep, grep = _Report(f"{case}/{layout}"), hc.Report()
        try:
            layers = _walk(rep, grep, rig, run)
        finally:
            rep.show()
        grep.done()
        _WALKED[key] = (rig, run, layers)
    return _WALKED[key]


STAGE_RUNS = [("base_small", "segment"), ("base_small", "flat"), ("large_small", "segment"), ("large_small", "flat"),
              ("base_10s", "segment"), ("base_B1", "segment"), ("base_train", "segment"), ("base_train", "flat")]


@pytest.mark.parametrize("case,layout", STAGE_RUNS)
def test_stage_by_stage_vs_fp64(rigs, case, layout):
    """every stage of the frozen WavLM forward against its fp64 definition on its own recorded inputs, element by element"""
    rig = rigs(case)
    a = rig.arch
    if CASES[case][2]:
        assert rig.enc._dropout_active() and min(a.dropout_input, a.dropout, a.attention_dropout) > 0.0
    rig, run, layers = _walked(rigs, case, layout)
    lay, pl = run.lay, run.pl
    assert (a.heads, a.layer_norm_first) == ((16, True) if rig.large else (12, False)) and len(layers) == 2
    if CASES[case][1] is SMALL:
        assert lay.valid == [150, 65, 127, 5]
        assert lay.pitch == ([152, 72, 136, 8] if layout == "segment" else [152] * 4)
        assert pl.R == wc.STAGE_R and lay.M == (368 if layout == "segment" else 608)
    if case == "base_10s":
        assert lay.valid == [499, 257] and lay.pitch == [504, 264] and pl.R == 504
        assert tuple(layers[0]["attn"].kw["table"].shape) == (12, 2 * 504 - 1)
        assert -(-lay.valid[0] // 64) == 8 and -(-lay.pitch[0] // 128) == 4          # key tiles, query blocks
    if case == "base_B1":
        assert lay.valid == [103] and pl.T == 103
    if CASES[case][2]:
        assert float((run.hidden[0] == 0).float().mean()) > 0.05                       # the encoder dropout acted
        assert layers[0]["attn"].kw["drop_p"] == a.attention_dropout


# ---------------------------------------------------------------------------------------------------------------- invariants
@pytest.mark.parametrize("case", ["base_small", "large_small"])
def test_ragged_equals_padded(rigs, case):
    """the valid frames of every hidden state: segment rows (per-utterance pitches) == flat rows (every utterance at T)"""
    rig = rigs(case)
    s, f = rig.run("segment", record=False), rig.run("flat", record=False)
    assert s.lay.pitch != f.lay.pitch and s.lay.valid == f.lay.valid
    for n in range(s.hidden.shape[0]):
        for b, v in enumerate(s.lay.valid):
            assert torch.equal(s.hidden[n][s.lay.r0[b]: s.lay.r0[b] + v], f.hidden[n][f.lay.r0[b]: f.lay.r0[b] + v]), (case, n, b)
    for b, v in enumerate(s.lay.valid):                                                # the last layer's gate of the valid frames
        assert torch.equal(s.gate[:, s.lay.r0[b]: s.lay.r0[b] + v], f.gate[:, f.lay.r0[b]: f.lay.r0[b] + v]), (case, "gate", b)


@pytest.mark.parametrize("case", ["base_small", "large_small"])
def test_repeatability(rigs, case):
    """two forwards of one batch: identical hidden states and gate buffers, every row, both layouts"""
    rig = rigs(case)
    for layout in ("segment", "flat"):
        a, b = rig.run(layout, record=False), rig.run(layout, record=False)
        assert torch.equal(a.hidden, b.hidden) and torch.equal(a.gate, b.gate), (case, layout)
        for k in a.scratch:
            assert torch.equal(a.scratch[k], b.scratch[k]), (case, layout, k)


@pytest.mark.parametrize("case", ["base_small", "large_small"])
def test_pad_rows_are_never_mixed_in(rigs, case):
    """+-1e4 in the frames >= valid of the layers' input and in the gate entries of those rows; the recorded layer calls are replayed
    on the plan's own buffers and the valid rows of every hidden state must not change a bit"""
    rig = rigs(case)
    a = rig.arch
    g = torch.Generator().manual_seed(18)
    for layout in ("segment", "flat"):
        run = rig.run(layout)
        pl, lay, calls = run.pl, run.lay, run.calls
        names = [c.name for c in calls]
        vm = lay.mask(lay.valid, rig.dev)
        i_layers = names.index("posconv_seg") + (1 if a.layer_norm_first else 2)
        assert names[i_layers] == ("layernorm_bf16" if a.layer_norm_first else "gemm_raw") and "wavlm_gate" not in names[:i_layers]

        def replay():
            for j in range(i_layers, len(calls)):
                calls[j].replay()
            torch.cuda.synchronize()

        replay()                                          # a plain replay reproduces the run
        assert torch.equal(pl.hidden, run.hidden)
        gate = pl.gate_rows(a.heads, pl.M)
        for b in range(lay.B):
            _junk(pl.hidden[0], lay.r0[b], lay.valid[b], lay.pitch[b], g)
            _junk(gate.t(), lay.r0[b], lay.valid[b], lay.pitch[b], g)
        assert float(pl.hidden[0][~vm].abs().min()) == 1e4 - 16 and float(gate[:, ~vm].abs().min()) == 1e4    # bf16(1e4) = 9984
        replay()
        assert torch.equal(pl.hidden[0][vm], run.hidden[0][vm])
        for n in range(1, pl.hidden.shape[0]):
            assert torch.equal(pl.hidden[n][vm], run.hidden[n][vm]), (case, layout, n)
        assert torch.equal(pl.gate_rows(a.heads, pl.M)[:, vm], run.gate[:, vm])


def test_plan_and_table_reuse(rigs):
    """base_small, then base_B1 (another T, another plan, another table) on the SAME encoder, then base_small again"""
    small = rigs("base_small")
    first = small.run("segment", record=False)
    other = rigs("base_B1", share=small)
    assert other.enc is small.enc
    b1 = other.run("segment")
    assert b1.pl is not first.pl and b1.pl.T == 103 and first.pl.T == 150 and (b1.pl.B, first.pl.B) == (1, 4)
    tabs = [c.kw["table"] for c in b1.calls if c.name == "attn_fwd"]
    assert len(tabs) == 2 and all(torch.equal(t, wc.bias_table(small.sd[REL].float(), b1.pl.R).to(small.dev)) for t in tabs)
    third = small.run("segment", record=False)
    assert third.pl is first.pl
    assert torch.equal(third.hidden, first.hidden) and torch.equal(third.gate, first.gate)


def test_replaced_weights(rigs):
    """a second state dict loaded into an encoder that has already run (_load_weights, the constructor's own path - the encoder
    has no other): its next forward == a freshly built encoder's on that state dict; nothing of the first weights (the plan's table,
    the gate's working copies, a plan buffer) survives"""
    from speechclip_plus_amd import speech_encoder as se
    used = rigs("base_small", seed=311)
    before = used.run("segment", record=False)
    sd2 = se.random_wavlm_state_dict(used.arch, seed=733)
    used.enc._load_weights(sd2)
    used.sd = sd2
    after = used.run("segment")
    fresh = rigs("base_small", seed=733).run("segment", record=False)
    assert after.pl is before.pl and not torch.equal(after.hidden[2], before.hidden[2])
    tabs = [c.kw["table"] for c in after.calls if c.name == "attn_fwd"]
    assert all(torch.equal(t, wc.bias_table(sd2[REL].float(), after.pl.R).to(used.dev)) for t in tabs)
    assert torch.equal(after.hidden, fresh.hidden) and torch.equal(after.gate, fresh.gate)


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def _share(tag, c, lay, H, gate=None, table=None):
    """the kernel's own output against a deliberately wrong reference: share of the valid query rows that the element-wise criterion
    rejects, largest error / bound"""
    out = c.pa[3]
    rej = tot = 0
    worst = 0.0
    for b in range(lay.B):
        r0, P, v = lay.r0[b], lay.pitch[b], lay.valid[b]
        f = wc.segment_attention_ref(c.a[0], c.a[1], c.kw["gate"] if gate is None else gate, c.kw["table"] if table is None else table,
                                     r0, P, v, H, c.a[8], drop=_drop_of(c, lay))
        got = wc.heads_of(out[r0: r0 + P].cpu(), H)
        rej += int(wc.rows_rejected(got, f["out"], f["bound"])[:v].sum())
        tot += v
        worst = max(worst, float(((got.double() - f["out"]).abs() / f["bound"]).max()))
    print(f"[wavlm-fwd] sensitivity {tag:64s} rows rejected {rej:4d} of {tot:4d}   max error / bound {worst:8.3g}")
    return rej / tot, worst


def test_wrong_gate_parameters_and_tables_are_rejected(rigs):
    """attention of layer 1 against references with (a) the gate of layer 0's parameters on layer 1's rows, (b) the table one offset
    off (j - i + 1), (c) heads 0 and 1 of the table exchanged, at H = 12 and at H = 16: the majority of the valid query rows fails"""
    rig, run, layers = _walked(rigs, "base_small", "segment")
    lay, H = run.lay, rig.arch.heads
    c = layers[1]["attn"]
    share, worst = _share("base layer 1: the right reference", c, lay, H)
    assert share == 0.0 and worst <= 1.0
    wrong_gate = _gate_refs(layers[1]["gate"].a[0], _gate_params(rig.sd, 0), H)[0]
    planted = [("base layer 1: gate of layer 0's parameters", dict(gate=wrong_gate)),
               ("base layer 1: table shifted by one offset", dict(table=wc.table_shifted(rig.sd[REL].float(), run.pl.R))),
               ("base layer 1: table heads 0 / 1 exchanged (H = 12)", dict(table=wc.table_heads_swapped(c.kw["table"].cpu())))]
    for tag, kw in planted:
        assert _share(tag, c, lay, H, **kw)[0] > 0.5, tag
    rig, run, layers = _walked(rigs, "large_small", "segment")
    c = layers[1]["attn"]
    assert rig.arch.heads == 16 and _share("large: the right reference", c, run.lay, 16)[0] == 0.0
    assert _share("large layer 1: table heads 0 / 1 exchanged (H = 16)", c, run.lay, 16, table=wc.table_heads_swapped(c.kw["table"].cpu()))[0] > 0.5


def test_gate_from_the_unnormalised_rows_is_rejected(rigs):
    """wavlm_large: the gate reference taken from hidden[i] instead of ln1(hidden[i]) - the gate criterion must fail"""
    rig, run, layers = _walked(rigs, "large_small", "segment")
    for i, L in enumerate(layers):
        c = L["gate"]
        got = c.pkw["out"].cpu()
        assert not torch.equal(L["hidden"], c.a[0])
        ok_ref, ok_yard = _gate_refs(c.a[0], c.a[1:4], 16)
        assert not wc.gate_criterion_rejects(got, ok_ref, ok_yard)[0]
        ref, yard = _gate_refs(L["hidden"], c.a[1:4], 16)
        bad, lines = wc.gate_criterion_rejects(got, ref, yard)
        e = float(hc.row_errors(got, ref, ()).max())
        print(f"[wavlm-fwd] sensitivity large layer {i}: gate reference from hidden[{i}], not ln1: error {e:.3g} / bound {hc.yard_bound(float(hc.row_errors(yard, ref, ()).max())):.3g}")
        assert bad, lines


def test_a_removed_key_of_the_last_tile_is_rejected(rigs):
    """base_10s: one key of key tile 7 (keys 448 .. 498) removed from one query of the last query block (rows 384 ..)"""
    rig, run, layers = _walked(rigs, "base_10s", "segment")
    lay, H = run.lay, rig.arch.heads
    c, f = layers[0]["attn"], layers[0]["refs"][0]
    r0, P, v, q = lay.r0[0], lay.pitch[0], lay.valid[0], 450
    key = wc.likeliest_key(f, q, 448, v)
    assert 448 <= key[2] < v and q >= 384
    g = wc.segment_attention_ref(c.a[0], c.a[1], c.kw["gate"], c.kw["table"], r0, P, v, H, c.a[8], drop_key=key)
    got = wc.heads_of(c.pa[3][r0: r0 + P].cpu(), H)
    assert not bool(wc.rows_rejected(got, f["out"], f["bound"]).any())
    rej = wc.rows_rejected(got, g["out"], g["bound"])
    ratio = float(((got.double() - g["out"]).abs() / g["bound"])[key[0], q].max())
    print(f"[wavlm-fwd] sensitivity base_10s: key {key[2]} (p = {float(f['P'][key]):.3g}) removed from query {q}, head {key[0]}: error / bound {ratio:.3g}")
    assert bool(rej[q]) and int(rej.sum()) == 1


def test_segment_unpacking_is_the_rigs(rigs):
    """wavlm_cases.vt_segment reads the recorded V^T as tests/test_gpu_frozen_fwd.py's _vt_rows does"""
    rig, run, layers = _walked(rigs, "base_small", "segment")
    lay, H = run.lay, rig.arch.heads
    vt = layers[0]["attn"].a[1]
    rows = _vt_rows(vt, lay, H * 64)
    for b in range(lay.B):
        assert torch.equal(wc.rows_of(wc.vt_segment(vt, lay.r0[b], lay.pitch[b], H)), rows[lay.r0[b]: lay.r0[b] + lay.pitch[b]])
