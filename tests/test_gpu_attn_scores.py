"""The attention kernels per query against fp64 on peaked and drifting scores: attn_fwd_kernel in all its instances (plain, dropout,
gated relative-position bias; uniform and segment rows; causal 0 / 1 / 32 / 64), attn_bwd_dq_kernel / attn_bwd_dkv_kernel in both entry
forms, attn32_fwd_kernel / attn32_bwd_kernel.

Cases, fp64 references, bounds and planted errors come from tests/attn_cases.py; tests/test_attn_cases_cpu.py shows on the CPU that
an emulation of the kernels' arithmetic order keeps every bound used here.  Every comparison is element by element (docs/parity.md,
"Attention on peaked and drifting scores"); rel-L2 is printed only.  Every figure is printed as a ``PARITY|...`` line before anything is
asserted, and a test fails once with all its violations."""
import pytest
import torch

import attn_cases as ac
from test_attn_cases_cpu import DROP_P, DROP_SEED, SEG_RUNS, SHORT_KINDS, _dout, _utt, apply_planted, planted, short_case

pytestmark = pytest.mark.gpu
SENT = 7.0
DEV = "cuda"
_REF = {}


def _ops():
    from speechclip_plus_amd import ops
    return ops


def _ref(c, b, causal=0, drop=None, bias=False):
    """fp64 reference of utterance b, computed once per (case, options) and left unchanged.  drop = None / 'uniform' / (r0, pitch, rows,
    max_pitch) for the element index of the segment layout"""
    key = (c["name"], c.get("restart", 0), tuple(c["lens"]), b, causal, drop, bias)
    if key not in _REF:
        R = c["R"]
        q, k, v = _utt(c, b)
        mask = ac.key_mask(R, c["lens"][b], causal)[None].expand(ac.H, -1, -1)
        mult = None
        if drop == "uniform":
            mult = ac.drop_mult(ac.drop_index_uniform(b, R), DROP_SEED, DROP_P)[0]
        elif drop is not None:
            r0, p, rows, mp = drop
            mult = torch.zeros(ac.H, R, R, dtype=torch.float64)          # rows / keys past the pitch: not compared, masked
            mult[:, :p, :p] = ac.drop_mult(ac.drop_index_segment(r0, p, rows, mp), DROP_SEED, DROP_P)[0]
        bm = ac.bias_matrix(c["gate"][:, b * R: (b + 1) * R].double(), c["table"].double(), R) if bias else None
        f = ac.fwd_ref(q, k, v, mask, bias=bm, mult=mult)
        f["mult"] = mult
        _REF[key] = f
    return _REF[key]


def _uniform(c, causal=0, drop=False, bias=False, order=None):
    """-> out [B, R, D] bf16, lse2 [B, H, R] fp32 on the CPU; ``order``: the utterances in another batch order"""
    ops = _ops()
    B, R = c["B"], c["R"]
    order = list(range(B)) if order is None else order
    q, k, v = (c[n][order] for n in "qkv")
    qk = torch.cat([q, k], dim=-1).reshape(B * R, 2 * ac.D).contiguous().to(DEV)
    vt = v.view(B, R, ac.H, 64).permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.full((B * R + 8, ac.D), SENT, dtype=torch.bfloat16, device=DEV)
    lse2 = torch.full((B * ac.H * R + 8,), SENT, dtype=torch.float32, device=DEV)
    kw = {}
    if bias:
        gate = c["gate"].view(ac.H, B, R)[:, order].reshape(ac.H, B * R).contiguous()
        kw = {"gate": gate.to(DEV), "table": c["table"].to(DEV)}
    ops.attn_fwd(qk, vt, torch.tensor([c["lens"][b] for b in order], dtype=torch.int32, device=DEV), out, B, R, ac.H, ac.D, ac.SCALE,
                 lse2=lse2, causal=causal, drop_p=DROP_P if drop else 0.0, drop_seed=DROP_SEED, **kw)
    torch.cuda.synchronize()
    out, lse2 = out.cpu(), lse2.cpu()
    assert bool((out[B * R:] == SENT).all()) and bool((lse2[B * ac.H * R:] == SENT).all()), "rows past the batch written"
    return out[: B * R].view(B, R, ac.D), lse2[: B * ac.H * R].view(B, ac.H, R)


def _segments(c, use_work=True, causal=0, drop=False, bias=False):
    """the same utterances in the segment layout, pitch = the length rounded up to 8 rows -> out [M + 64, D], lse2 [H, M], pitch, r0, seg"""
    ops = _ops()
    R, lens = c["R"], c["lens"]
    pitch = [(n + 7) // 8 * 8 for n in lens]
    seg = ops.RowSegments(pitch, lens, DEV)
    M, r0 = seg.rows, seg.row0_host
    qk = torch.zeros(M + 64, 2 * ac.D, dtype=torch.bfloat16)
    vt = torch.zeros(ac.D * (M + 64), dtype=torch.bfloat16)
    gs = torch.zeros(ac.H, M)
    for b, p in enumerate(pitch):
        qk[r0[b]: r0[b] + p] = torch.cat([c["q"][b, :p], c["k"][b, :p]], dim=-1)
        vt[ac.D * r0[b]: ac.D * (r0[b] + p)] = c["v"][b, :p].view(p, ac.H, 64).permute(1, 2, 0).reshape(-1)
        if bias:
            gs[:, r0[b]: r0[b] + p] = c["gate"][:, b * R: b * R + p]
    out = torch.full((M + 64, ac.D), SENT, dtype=torch.bfloat16, device=DEV)
    lse2 = torch.full((ac.H * M + 8,), SENT, dtype=torch.float32, device=DEV)
    kw = {"gate": gs.to(DEV), "table": c["table"].to(DEV)} if bias else {}
    ops.attn_fwd(qk.to(DEV), vt.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), out, 0, 0, ac.H, ac.D, ac.SCALE, lse2=lse2,
                 causal=causal, drop_p=DROP_P if drop else 0.0, drop_seed=DROP_SEED, seg=seg, use_work=use_work, **kw)
    torch.cuda.synchronize()
    out, lse2 = out.cpu(), lse2.cpu()
    assert bool((out[M:] == SENT).all()) and bool((lse2[ac.H * M:] == SENT).all()), "rows past the last pitch written"
    return out, lse2[: ac.H * M].view(ac.H, M), pitch, r0, seg


def _cmp_uniform(rep, c, tag, out, lse2, causal=0, drop=None, bias=False):
    worst = 0.0
    for b in range(c["B"]):
        f = _ref(c, b, causal, drop, bias)
        worst = max(worst, ac.check(rep, f"{tag} b={b}", "out", ac.heads(out[b]), f["out"], f["bound"]),
                    ac.check(rep, f"{tag} b={b}", "lse2", lse2[b], f["lse2"], f["bound_lse"]))
    return worst


def _cmp_segments(rep, c, tag, res, causal=0, drop=False, bias=False):
    out, lse2, pitch, r0, seg = res
    for b, p in enumerate(pitch):
        f = _ref(c, b, causal, (r0[b], p, seg.rows, seg.max_pitch) if drop else None, bias)
        ac.check(rep, f"{tag} b={b}", "out", ac.heads(out[r0[b]: r0[b] + p]), f["out"][:, :p], f["bound"][:, :p])
        ac.check(rep, f"{tag} b={b}", "lse2", lse2[:, r0[b]: r0[b] + p], f["lse2"][:, :p], f["bound_lse"][:, :p])


def _same(rep, tag, what, a, b):
    """bit for bit: the same shape, dtype and bit pattern"""
    ok = a.shape == b.shape and a.dtype == b.dtype
    if ok:
        bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
        ok = bool((a.contiguous().view(bits) == b.contiguous().view(bits)).all())
    rep.require(tag, what + ": bits differ", ok)


# ---------------------------------------------------------------------------------------------------------------- forward, plain
@pytest.mark.parametrize("name", list(ac.CASES))
def test_forward_plain_both_layouts(name):
    """uniform rows, segment rows with and without the work table, causal 0 and 1, every query row below R (below the pitch) against
    fp64; the bitwise invariants of the per-query rescale decision"""
    rep = ac.Report()
    c = ac.build(name)
    B = c["B"]
    for causal in (0, 1):
        out, lse2 = _uniform(c, causal)
        _cmp_uniform(rep, c, f"{name} uniform causal={causal}", out, lse2, causal)
        sw = _segments(c, True, causal)
        sn = _segments(c, False, causal)
        _cmp_segments(rep, c, f"{name} segments work causal={causal}", sw, causal)
        _cmp_segments(rep, c, f"{name} segments no-work causal={causal}", sn, causal)
        tag = f"{name} bits causal={causal}"
        _same(rep, tag, "with / without the work table: out", sw[0], sn[0])
        _same(rep, tag, "with / without the work table: lse2", sw[1], sn[1])
        for b, p in enumerate(sw[2]):
            r0 = sw[3][b]
            _same(rep, tag, f"utterance {b}: uniform / segment out", out[b, :p], sw[0][r0: r0 + p])
            _same(rep, tag, f"utterance {b}: uniform / segment lse2", lse2[b, :, :p], sw[1][:, r0: r0 + p])
        out2, lse22 = _uniform(c, causal)
        _same(rep, tag, "two runs: out", out, out2)
        _same(rep, tag, "two runs: lse2", lse2, lse22)
        order = list(reversed(range(B)))
        outr, lser = _uniform(c, causal, order=order)
        for pos, b in enumerate(order):
            _same(rep, tag, f"utterance {b} among reordered neighbours: out", out[b], outr[pos])
            _same(rep, tag, f"utterance {b} among reordered neighbours: lse2", lse2[b], lser[pos])
    rep.done()


@pytest.mark.parametrize("name,restart,lens", SEG_RUNS)
def test_forward_segment_causal(name, restart, lens):
    """causal = 32 / 64 in the uniform layout, the profile restarted per segment: key blocks before a query's segment are fully masked
    (the running maximum stays at its floor), the segment itself drifts"""
    rep = ac.Report()
    c = ac.build(name, restart=restart, lens=lens)
    out, lse2 = _uniform(c, restart)
    _cmp_uniform(rep, c, f"{name} causal={restart}", out, lse2, restart)
    rep.done()


@pytest.mark.parametrize("name", ["stair55", "stair65", "stair09", "spike"])
def test_forward_dropout(name):
    """drop_p = 0.1: a dropped probability contributes exactly nothing (the reference's product with the host mask), lse2 is that of the
    undropped scores, a row whose spike key is dropped stays within its bound"""
    rep = ac.Report()
    c = ac.build(name)
    out, lse2 = _uniform(c, 0, drop=True)
    _cmp_uniform(rep, c, f"{name} uniform drop", out, lse2, 0, "uniform")
    _cmp_segments(rep, c, f"{name} segments drop", _segments(c, True, 0, drop=True), 0, drop=True)
    for b in range(c["B"]):
        f = _ref(c, b)
        ac.check(rep, f"{name} drop b={b}", "lse2 vs the undropped scores", lse2[b], f["lse2"], f["bound_lse"])
    if name == "spike":
        # a dropped probability contributes exactly nothing: a one-hot row that lost its spike key is left with the e^-40 tail
        n_dropped = 0
        for b in range(c["B"]):
            hit = ac.dropped_spike_rows(_ref(c, b, 0, "uniform"), c["gains"][b])
            n_dropped += int(hit.sum())
            rep.require(f"{name} drop b={b}", "the spike of a row whose spike key is dropped leaked into the output",
                        float(ac.heads(out[b])[hit].abs().max() if bool(hit.any()) else 0.0) < 1e-12)
        print(f"ATTN|spike drop|one-hot rows whose spike key is dropped: {n_dropped}")
        rep.require(name, "no one-hot row lost its spike key: the case does not reach that path", n_dropped > 0)
    rep.done()


@pytest.mark.parametrize("name", list(ac.BIAS_CASES))
def test_forward_bias(name):
    """BIAS = 1 with Tmax = R: the drift comes from gate x table; uniform and segment rows, with and without dropout; valid = 65 at
    R = 384 and valid = R clamp a q-block's table window at both ends of the head's table"""
    rep = ac.Report()
    c = ac.build_bias(name)
    for drop in (False, True):
        out, lse2 = _uniform(c, 0, drop=drop, bias=True)
        _cmp_uniform(rep, c, f"{name} uniform drop={int(drop)}", out, lse2, 0, "uniform" if drop else None, True)
        res = _segments(c, True, 0, drop=drop, bias=True)
        _cmp_segments(rep, c, f"{name} segments drop={int(drop)}", res, 0, drop=drop, bias=True)
        if not drop:
            for b, p in enumerate(res[2]):
                _same(rep, name, f"utterance {b}: uniform / segment out", out[b, :p], res[0][res[3][b]: res[3][b] + p])
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- backward
def _backward(rep, c, tag, causal=0, drop=False, given_kT=False):
    ops = _ops()
    B, R = c["B"], c["R"]
    qkv = torch.cat([c[n].reshape(B * R, ac.D) for n in "qkv"], dim=1).contiguous().to(DEV)
    q, k, v = qkv[:, : ac.D], qkv[:, ac.D: 2 * ac.D], qkv[:, 2 * ac.D:]
    vl = torch.tensor(c["lens"], dtype=torch.int32, device=DEV)
    vt = ops.head_transpose(v, B, R, ac.H)
    out = torch.zeros(B * R, ac.D, device=DEV, dtype=torch.bfloat16)
    lse2 = torch.empty(B, ac.H, R, device=DEV, dtype=torch.float32)
    kw = {"drop_p": DROP_P, "drop_seed": DROP_SEED} if drop else {}
    ops.attn_fwd(qkv[:, : 2 * ac.D], vt, vl, out, B, R, ac.H, ac.D, ac.SCALE, lse2=lse2, causal=causal, **kw)
    dout = torch.stack([_dout(c, b) for b in range(B)])
    dqkv = torch.full((B * R, 3 * ac.D), SENT, device=DEV, dtype=torch.bfloat16)
    ops.attn_bwd(q, k, v, out, dout.reshape(B * R, ac.D).to(DEV), lse2, vl, dqkv[:, : ac.D], dqkv[:, ac.D: 2 * ac.D], dqkv[:, 2 * ac.D:],
                 B, R, ac.H, ac.SCALE, causal=causal, kT=ops.head_transpose(k, B, R, ac.H) if given_kT else None, **kw)
    torch.cuda.synchronize()
    got = dqkv.cpu().view(B, R, 3, ac.D)
    for b in range(B):
        nv = c["lens"][b]
        f = _ref(c, b, causal, "uniform" if drop else None)
        d = ac.heads(dout[b])
        ep, dd = ac.flash_bwd_errors(f, d)
        qh, kh, vh = _utt(c, b)
        r = ac.bwd_ref(qh, kh, vh, d, f["mask"], mult=f["mult"], ep=ep, ddelta=dd)
        for i, n in enumerate(("dq", "dk", "dv")):
            ac.check(rep, f"{tag} b={b}", n, ac.heads(got[b, :, i]), r[n], r["bound_" + n])
        rep.require(f"{tag} b={b}", "a pad query's dq or a masked key's dk / dv is not exactly zero", bool((got[b, nv:] == 0).all()))


@pytest.mark.parametrize("name", list(ac.CASES))
def test_backward(name):
    """dq / dk / dv fed the kernel's own out and lse2: fused entry (causal 0), given kT (causal 1), the forward's drop seed"""
    rep = ac.Report()
    c = ac.build(name)
    _backward(rep, c, f"{name} bwd fused causal=0")
    _backward(rep, c, f"{name} bwd kT causal=1", causal=1, given_kT=True)
    if c["kind"] in ("stair55", "stair65", "stair09", "spike"):
        _backward(rep, c, f"{name} bwd fused drop", drop=True)
        _backward(rep, c, f"{name} bwd kT drop", drop=True, given_kT=True)
    rep.done()


def test_backward_segment_causal():
    rep = ac.Report()
    name, restart, lens = SEG_RUNS[0]
    c = ac.build(name, restart=restart, lens=lens)
    _backward(rep, c, f"{name} bwd fused causal=32", causal=32)
    _backward(rep, c, f"{name} bwd kT causal=32", causal=32, given_kT=True)
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- one-wave kernels
@pytest.mark.parametrize("kind", SHORT_KINDS)
def test_short_kernels(kind):
    """attn32_fwd / attn32_bwd at nseq 1, 5, 64 against fp64 per sequence, d out zeroed behind prompt lengths 1 / 27 / 32; the forward
    also against attn_fwd(causal = 32) on the same rows, within the sum of the two bounds"""
    ops = _ops()
    rep = ac.Report()
    mask = ac.key_mask(32, 32, causal=1)[None]
    for nseq in (1, 5, 64):
        M = 32 * nseq
        qkv = short_case(kind, nseq)
        plen = [(1, 27, 32)[s % 3] for s in range(nseq)]
        dout = torch.randn(M, ac.D, generator=torch.Generator().manual_seed(nseq)).to(torch.bfloat16)
        for s, n in enumerate(plen):
            dout[32 * s + n: 32 * s + 32] = 0
        qd = qkv.to(DEV)
        out = ops.attn32_fwd(qd, ac.H, ac.SCALE).cpu()
        dqkv = ops.attn32_bwd(qd, dout.to(DEV), ac.H, ac.SCALE).cpu()
        # the flash kernel on the same rows: one utterance of M rows, causal inside 32-row segments (64 rows / elements of slack)
        qk = torch.zeros(M + 64, 2 * ac.D, dtype=torch.bfloat16)
        qk[:M] = qkv[:, : 2 * ac.D]
        vt = torch.zeros(ac.D * M + 64, dtype=torch.bfloat16)
        vt[: ac.D * M] = qkv[:, 2 * ac.D:].view(M, ac.H, 64).permute(1, 2, 0).reshape(-1)
        flash = torch.zeros(M, ac.D, dtype=torch.bfloat16, device=DEV)
        ops.attn_fwd(qk.to(DEV), vt.to(DEV), torch.tensor([M], dtype=torch.int32, device=DEV), flash, 1, M, ac.H, ac.D, ac.SCALE, causal=32)
        torch.cuda.synchronize()
        flash = flash.cpu()
        # every sequence at once: [nseq H, 32, 64], the fp64 reference and its bounds vectorised over (sequence, head)
        sq = lambda x: x.double().view(nseq, 32, ac.H, 64).permute(0, 2, 1, 3).reshape(nseq * ac.H, 32, 64)
        q, k, v = (sq(qkv[:, i * ac.D: (i + 1) * ac.D]) for i in range(3))
        f = ac.fwd_ref(q, k, v, mask)
        tag = f"short {kind} nseq={nseq}"
        ac.check(rep, tag, "out", sq(out), f["out"], f["bound"])
        ac.check(rep, tag, "out vs attn_fwd(causal = 32)", sq(out), sq(flash), 2 * f["bound"])
        d = sq(dout)
        ep, dd = ac.short_bwd_errors(f, d, v)
        r = ac.bwd_ref(q, k, v, d, f["mask"], ep=ep, ddelta=dd, R_acc=32)
        for i, n in enumerate(("dq", "dk", "dv")):
            ac.check(rep, tag, n, sq(dqkv[:, i * ac.D: (i + 1) * ac.D]), r[n], r["bound_" + n])
        rep.require(tag, "a gradient row behind a prompt's d out is not finite", bool(torch.isfinite(dqkv.float()).all()))
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def test_planted_errors_on_the_device_result_are_rejected():
    """(b) a missed rescale, (d) lse2 off by 1e-3, (e) a masked key block let through - planted into the kernel's own output"""
    f, plants = planted()
    c = ac.build("stair65")
    out, lse2 = _uniform(c, 0)
    dev_out, dev_lse = ac.heads(out[0]), lse2[0].double()
    assert ac.within(dev_out, f["out"], f["bound"])[0] and ac.within(dev_lse, f["lse2"], f["bound_lse"])[0]
    for what, h, i, o_row, l_val in plants:
        if what[0] not in "bd":
            continue
        o, l = apply_planted(f, h, i, o_row.to(torch.bfloat16).double(), float(l_val), out=dev_out, lse=dev_lse)
        ok_o, r_o, _ = ac.within(o, f["out"], f["bound"])
        ok_l, r_l, _ = ac.within(l, f["lse2"], f["bound_lse"])
        print(f"ATTN|device + planted {what}|out error / bound {r_o:.3g}|lse2 error / bound {r_l:.3g}")
        assert not (ok_o and ok_l), what
    name, restart, lens = SEG_RUNS[0]
    c = ac.build(name, restart=restart, lens=lens)
    out, lse2 = _uniform(c, restart)
    fr = _ref(c, 0, restart)
    q, k, v = _utt(c, 0)
    i = int((c["gains"][0][64:96] == 0).nonzero()[0]) + 64
    mask = fr["mask"].clone()
    mask[0, i, 32:64] = True
    fe = ac.fwd_ref(q, k, v, mask)
    o, l = apply_planted(fr, 0, i, fe["out"][0, i].to(torch.bfloat16).double(), float(fe["lse2"][0, i]), out=ac.heads(out[0]), lse=lse2[0].double())
    ok_o, r_o, _ = ac.within(o, fr["out"], fr["bound"])
    ok_l, r_l, _ = ac.within(l, fr["lse2"], fr["bound_lse"])
    print(f"ATTN|device + planted e|out error / bound {r_o:.3g}|lse2 error / bound {r_l:.3g}")
    assert not ok_o and not ok_l
