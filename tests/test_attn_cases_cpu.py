"""What can be settled without a GPU about tests/attn_cases.py: the constructed cases reach the rescale counts they record, the
torch emulation of the kernels' arithmetic order stays below every derived bound on every case (so the bounds are satisfiable before
any kernel runs), and each planted error is rejected by the element-wise criterion.  Figures are printed before they are asserted."""
import pytest
import torch

import attn_cases as ac

# what every case records (attn_cases.build: c["rescales"], per query, from the host evaluation of the rule on the fp64 block maxima):
# per utterance the largest count over the queries of head 0 / head 2 (profile reversed) ...
RESCALES = {"stair55": [(5, 3), (3, 1), (2, 1), (1, 0)], "stair65": [(7, 3), (3, 1), (3, 1), (1, 0)], "stair09": [(1, 0), (1, 0), (0, 0), (0, 0)],
            "ramp": [(3, 1), (1, 0), (0, 0), (3, 1)], "desc": [(11, 11), (5, 5), (7, 7), (3, 3)], "spike": [(0, 1), (0, 1), (1, 1), (1, 1)],
            "twin": [(0, 1), (0, 0), (0, 1), (0, 0)], "stair55_off": [(3, 2), (3, 1), (1, 0), (2, 1)], "control": [(0, 0)] * 4}
# ... and the utterances in which EVERY 32-query wave of head 0 holds a query with 0 and a query with >= 2 rescales (the others are
# too short for two rescales: 33 / 65 keys)
MIXED = {"stair55": [0, 1, 2], "stair65": [0, 1, 2], "ramp": [0, 3], "stair55_off": [0, 1, 3]}
SEG_RUNS = [("ramp", 32, [128, 127, 128]), ("ramp", 64, [128, 127, 128]), ("stair65", 64, [256, 256])]
DROP_P, DROP_SEED = 0.1, 0x5eed1234


def _utt(c, b):
    return tuple(ac.heads(c[n][b]) for n in "qkv")


def _trace(c, b, causal=0):
    q, k, v = _utt(c, b)
    f = ac.fwd_ref(q, k, v, ac.key_mask(c["R"], c["lens"][b], causal)[None])
    return f, ac.rescale_trace(f["x"])


@pytest.mark.parametrize("name", list(ac.CASES))
def test_cases_reach_their_recorded_rescale_counts(name):
    c = ac.build(name)
    mixed = []
    for b in range(c["B"]):
        f, (cnt, margin, _) = _trace(c, b)                 # the rule on the reference's own masked scores
        assert torch.equal(cnt, c["rescales"][b]) and torch.equal(margin, c["margin"][b])
        print(f"ATTN|{name} b={b} keys={c['lens'][b]}|rescales after the first block, head 0 / 1 / 2: max {[int(cnt[h].max()) for h in range(3)]}|"
              f"margin {[round(float(margin[h].min()), 3) for h in range(3)]}")
        assert (int(cnt[0].max()), int(cnt[2].max())) == RESCALES[name][b], (name, b)
        if c["kind"] != "control":
            assert float(margin[[0, 2]].min()) >= ac.MARGIN, (name, b, float(margin[[0, 2]].min()))
            t, g = c["t"][b, [0, 2]], c["gains"][b]
            assert ac.bf16_exact(t) and ac.bf16_exact(g)
            if c["kind"] != "desc":
                assert bool(((t * 8) % 1 == 0).all() and ((g * 8) % 1 == 0).all())
        waves = cnt[0].view(-1, 32)
        if bool((waves.amin(1) == 0).all() and (waves.amax(1) >= 2).all()):
            mixed.append(b)
    if name in ac.DRIFTING:
        assert mixed == MIXED[name], (name, mixed)


def test_spike_rows_are_one_hot():
    c = ac.build("spike")
    for b, nv in enumerate(c["lens"]):
        f, _ = _trace(c, b)
        hot = c["gains"][b] == 2 * ac.A_GAIN
        for hi, h in enumerate((0, 2)):
            js = ac.SPIKE_KEYS[hi][b]
            j = min(nv - 1, js) if js >= 0 else nv - 1
            assert float((1.0 - f["P"][h, hot, j]).abs().max()) < 1e-12
            q, k, v = _utt(c, b)
            assert float((f["out"][h, hot] - v[h, j]).abs().max()) < 1e-10


def test_manual_backward_formulas_equal_autograd():
    c = ac.build("stair65")
    q, k, v = _utt(c, 1)
    dout = torch.randn(ac.H, c["R"], ac.DH, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    r = ac.bwd_ref(q, k, v, dout, ac.key_mask(c["R"], c["lens"][1])[None].expand(ac.H, -1, -1))
    for n in ("dq", "dk", "dv"):
        assert float((r[n] - r["manual_" + n]).abs().max()) <= 1e-12 * max(1.0, float(r[n].abs().max()))


def _dout(c, b, seed=0):
    g = torch.Generator().manual_seed(77 + b + seed)
    d = torch.randn(c["R"], ac.D, generator=g).to(torch.bfloat16)
    d[c["lens"][b]:] = 0
    return d


def _rehearse(rep, c, b, causal=0, drop=False, bwd=True):
    """the emulated forward (+ backward, fed the emulation's own out and lse2) of utterance b against fp64"""
    R, nv = c["R"], c["lens"][b]
    q, k, v = _utt(c, b)
    mask = ac.key_mask(R, nv, causal)[None].expand(ac.H, -1, -1)
    mult, keep, thr8 = None, None, 0
    if drop:
        mult, pa = ac.drop_mult(ac.drop_index_uniform(b, R), DROP_SEED, DROP_P)
        keep, thr8 = mult > 0, int(round(pa * 256))
    f = ac.fwd_ref(q, k, v, mask, mult=mult)
    f["mult"] = mult
    o, l = ac.emulate_fwd(q, k, v, mask, keep=keep, thr8=thr8)
    tag = f"{c['name']} b={b} causal={causal} drop={int(drop)} restart={c.get('restart', 0)}"
    ratios = [ac.check(rep, "rehearsal " + tag, "out", o, f["out"], f["bound"]), ac.check(rep, "rehearsal " + tag, "lse2", l, f["lse2"], f["bound_lse"])]
    flat = ac.within(l, f["lse2"], f["bound_lse_flat"])[1]
    print(f"ATTN|rehearsal {tag}|lse2 error over the flat-logarithm form of the bound (printed only): {flat:.3f}")
    if drop and c["kind"] == "spike":
        # a dropped probability contributes exactly nothing: a one-hot row that lost its spike key is left with the e^-40 tail
        hit = ac.dropped_spike_rows(f, c["gains"][b])
        ratios.append(int(hit.sum()))
        rep.require(tag, "the spike of a row whose spike key is dropped leaked into the output",
                    float(o.double()[hit].abs().max() if bool(hit.any()) else 0.0) < 1e-12)
    if bwd:
        dout = ac.heads(_dout(c, b))
        ep, dd = ac.flash_bwd_errors(f, dout)
        r = ac.bwd_ref(q, k, v, dout, mask, mult=mult, ep=ep, ddelta=dd)
        got = ac.emulate_bwd(q, k, v, o, dout, l, mask, keep=keep, thr8=thr8)
        for n, g_ in zip(("dq", "dk", "dv"), got):
            ratios.append(ac.check(rep, "rehearsal " + tag, n, g_, r[n], r["bound_" + n]))
    return ratios


@pytest.mark.parametrize("name", list(ac.CASES))
def test_rehearsal_keeps_every_bound(name):
    rep = ac.Report()
    c = ac.build(name)
    n_hit = 0
    for b in range(c["B"]):
        for causal in (0, 1):
            _rehearse(rep, c, b, causal=causal)
        if c["kind"] in ("stair55", "stair65", "stair09", "spike"):
            r = _rehearse(rep, c, b, drop=True)
            n_hit += r[2] if c["kind"] == "spike" else 0
    if c["kind"] == "spike":
        print(f"ATTN|spike drop|one-hot rows whose spike key is dropped: {n_hit}")
        assert n_hit > 0
    rep.done()


@pytest.mark.parametrize("name,restart,lens", SEG_RUNS)
def test_rehearsal_segment_causal(name, restart, lens):
    rep = ac.Report()
    c = ac.build(name, restart=restart, lens=lens)
    for b in range(c["B"]):
        _rehearse(rep, c, b, causal=restart, bwd=(restart == 32))
        _, (cnt, _, _) = _trace(c, b, causal=restart)
        assert int(cnt[0].max()) == (1 if restart == 64 else 0)
    rep.done()


@pytest.mark.parametrize("name", list(ac.BIAS_CASES))
def test_rehearsal_bias(name):
    rep = ac.Report()
    c = ac.build_bias(name)
    R = c["R"]
    most = 0
    for b, nv in enumerate(c["lens"]):
        q, k, v = _utt(c, b)
        mask = ac.key_mask(R, nv)[None].expand(ac.H, -1, -1)
        gate = c["gate"][:, b * R: (b + 1) * R]
        bias = ac.bias_matrix(gate.double(), c["table"].double(), R)
        for drop in (False, True):
            mult, keep, thr8 = None, None, 0
            if drop:
                mult, pa = ac.drop_mult(ac.drop_index_uniform(b, R), DROP_SEED, DROP_P)
                keep, thr8 = mult > 0, int(round(pa * 256))
            f = ac.fwd_ref(q, k, v, mask, bias=bias, mult=mult)
            o, l = ac.emulate_fwd_bias(q, k, v, mask, gate, c["table"], keep=keep, thr8=thr8)
            ac.check(rep, f"rehearsal {name} b={b} drop={int(drop)}", "out", o, f["out"], f["bound"])
            ac.check(rep, f"rehearsal {name} b={b} drop={int(drop)}", "lse2", l, f["lse2"], f["bound_lse"])
        cnt, margin, _ = ac.rescale_trace(f["x"])
        most = max(most, int(cnt[0].max()))
        assert float(margin[[0, 2]].min()) >= ac.MARGIN
    print(f"ATTN|{name}|most rescales after block 0 on head 0: {most}")
    assert most >= 2
    rep.done()


SHORT_KINDS = ("spike0", "spike31", "ramp", "desc")


def short_case(kind, nseq):
    """32-key versions of the profiles for the one-wave kernels: qkv [nseq 32, 3 D] bf16, causal inside each 32-row sequence"""
    g = torch.Generator().manual_seed(40 + SHORT_KINDS.index(kind) + nseq)
    M = 32 * nseq
    q, k = (0.05 * torch.randn(M, ac.H, ac.DH, generator=g, dtype=torch.float64) for _ in range(2))
    v = torch.randn(M, ac.H, ac.DH, generator=g, dtype=torch.float64)
    q[:, 1], k[:, 1] = torch.randn(M, ac.DH, generator=g, dtype=torch.float64), torch.randn(M, ac.DH, generator=g, dtype=torch.float64)
    j = torch.arange(32, dtype=torch.float64)
    t = {"spike0": ac.SPIKE_T * (j == 0), "spike31": ac.SPIKE_T * (j == 31), "ramp": 0.25 * j, "desc": -4.0 * j}[kind].double()
    gains = torch.cat([ac.wave_gains(32, g) for _ in range(nseq)])
    for h in (0, 2):
        q[:, h, 0] = gains
        k[:, h, 0] = (t if h == 0 else t.flip(0)).repeat(nseq)
    return torch.cat([x.reshape(M, ac.D) for x in (q, k, v)], dim=1).to(torch.bfloat16)


@pytest.mark.parametrize("kind", SHORT_KINDS)
def test_rehearsal_short_kernels(kind):
    rep = ac.Report()
    qkv = short_case(kind, 5)
    mask = ac.key_mask(32, 32, causal=1)[None]
    for s_, plen in zip(range(5), (1, 27, 32, 27, 1)):
        q, k, v = (ac.heads(qkv[32 * s_: 32 * s_ + 32, i * ac.D: (i + 1) * ac.D]) for i in range(3))
        f = ac.fwd_ref(q, k, v, mask)
        ac.check(rep, f"rehearsal short {kind} seq={s_}", "out", ac.emulate_short_fwd(q, k, v, mask), f["out"], f["bound"])
        dout = torch.randn(32, ac.D, generator=torch.Generator().manual_seed(s_)).to(torch.bfloat16)
        dout[plen:] = 0
        dout = ac.heads(dout)
        ep, dd = ac.short_bwd_errors(f, dout, v)
        r = ac.bwd_ref(q, k, v, dout, mask.expand(ac.H, -1, -1), ep=ep, ddelta=dd, R_acc=32)
        for n, g_ in zip(("dq", "dk", "dv"), ac.emulate_short_bwd(q, k, v, dout, mask)):
            ac.check(rep, f"rehearsal short {kind} seq={s_}", n, g_, r[n], r["bound_" + n])
    rep.done()


# ------------------------------------------------------------------------------------------------------------------- planted errors
def planted(name="stair65", b=0):
    """-> the fp64 reference of utterance b and the planted results (a) - (d) as (what, h, query, out row, lse2 value)"""
    c = ac.build(name)
    q, k, v = _utt(c, b)
    mask = ac.key_mask(c["R"], c["lens"][b])[None]
    f = ac.fwd_ref(q, k, v, mask)
    cnt, _, dec = ac.rescale_trace(f["x"])
    i_hot = int((c["gains"][b] == 2 * ac.A_GAIN).nonzero()[5])          # rescales at every block
    i_zero = int((c["gains"][b] == 0).nonzero()[5])                     # never rescales after block 0
    assert bool(dec[3][0, i_hot]) and bool(dec[6][0, i_hot]) and int(cnt[0, i_zero]) == 0
    out = []
    fa = ac.fwd_ref(q, k, v, mask, drop_key=(0, i_hot, c["lens"][b] - 1))
    out.append(("a: one key removed", 0, i_hot, fa["out"][0, i_hot], fa["lse2"][0, i_hot]))
    ob, lb = ac.plant_missed_rescale(q, k, v, mask, 0, i_hot, 6)
    out.append(("b: missed rescale", 0, i_hot, ob, lb))
    oc, lc = ac.plant_wrong_rescale(q, k, v, mask, 0, i_zero, 3, 6.5)
    out.append(("c: wave-mate's alpha", 0, i_zero, oc, lc))
    out.append(("d: lse2 off by 1e-3", 0, i_zero, f["out"][0, i_zero], f["lse2"][0, i_zero] + 1e-3))
    return f, out


def apply_planted(f, h, i, o_row, l_val, out=None, lse=None):
    out = (f["out"] if out is None else out).double().clone()
    lse = (f["lse2"] if lse is None else lse).double().clone()
    out[h, i], lse[h, i] = o_row, l_val
    return out, lse


def test_planted_errors_are_rejected():
    f, plants = planted()
    for what, h, i, o_row, l_val in plants:
        out, lse = apply_planted(f, h, i, o_row, l_val)
        ok_o, r_o, _ = ac.within(out, f["out"], f["bound"])
        ok_l, r_l, _ = ac.within(lse, f["lse2"], f["bound_lse"])
        print(f"ATTN|planted {what}|out error / bound {r_o:.3g}|lse2 error / bound {r_l:.3g}|whole-tensor rel-L2 out {ac.rel_l2(out, f['out']):.3e} "
              f"lse2 {ac.rel_l2(lse, f['lse2']):.3e}|allclose(1e-3, 2e-2) on lse2: {torch.allclose(lse, f['lse2'], rtol=1e-3, atol=2e-2)}")
        assert not (ok_o and ok_l), what
        if what[0] in "bd":        # the criteria the suite had let these through
            assert ac.rel_l2(out, f["out"]) < 1.5e-2 and (what[0] == "b" or torch.allclose(lse, f["lse2"], rtol=1e-3, atol=2e-2))
    # (e): one masked key block of a causal = 32 query let through
    c = ac.build("ramp", restart=32, lens=[128, 127, 128])
    q, k, v = _utt(c, 0)
    mask = ac.key_mask(128, 128, 32)[None].expand(ac.H, -1, -1).clone()
    f = ac.fwd_ref(q, k, v, mask)
    i = int((c["gains"][0][64:96] == 0).nonzero()[0]) + 64
    mask[0, i, 32:64] = True
    fe = ac.fwd_ref(q, k, v, mask)
    out, lse = apply_planted(f, 0, i, fe["out"][0, i], fe["lse2"][0, i])
    ok_o, r_o, _ = ac.within(out, f["out"], f["bound"])
    ok_l, r_l, _ = ac.within(lse, f["lse2"], f["bound_lse"])
    print(f"ATTN|planted e: a masked block let through|out error / bound {r_o:.3g}|lse2 error / bound {r_l:.3g}")
    assert not ok_o and not ok_l
