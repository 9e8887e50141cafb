"""The keyword branch's own kernels against fp64: continuous integrate-and-fire (csrc/cif.hip: fire kernels in both forms and both
row layouts, bookkeeping, tail, weight head, row zeroing), the keyword quantiser's row kernels and the keyword BatchNorm
(csrc/vq.hip), the row softmax of the attention block (csrc/softmax.hip).

Inputs, references and bounds come from tests/kw_cases.py (seeded; fp64 references, every backward by autograd on the fp64
forward; the same functions in fp32 on the CPU are the yardstick).  Every kernel is compared on its own inputs; the error is taken
per row of a quantity's natural grouping.  Bounds (docs/parity.md, "Keyword branch kernels"): sums of products ``k u sum |a_i b_i|``
with k from the code; quantities through exp / log / rsqrt / division ``max(4 x the yardstick's error on the case, 2^-23)``;
discrete quantities exactly, against the device's own fp32 inputs and against fp64 where the fp64 decision has margin.  Every
figure is printed as a ``PARITY|case|quantity|error|yardstick|bound`` line before anything is asserted, and a test fails once
with all its violations."""
import ctypes

import pytest
import torch

import kw_cases as kc

pytestmark = pytest.mark.gpu
SENT = 7.0                                   # sentinel of the buffers a kernel must not touch


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _ops():
    from speechclip_plus_amd import ops
    return ops


def _lib():
    from speechclip_plus_amd import _lib
    return _lib.lib()


def _rc(rc, what):
    from speechclip_plus_amd._lib import check
    check(rc, what)


def _exact(rep, name, what, got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    n = int((got != want).sum()) if got.shape == want.shape else -1
    print(f"PARITY|{name}|{what} (exact)|{float(n):.3e}|-|0.000e+00")
    rep.require(name, f"{what}: {n} elements differ", n == 0)


def _within(rep, name, what, got, ref, elem_bound):
    """|got - ref| <= elem_bound element by element; prints the largest error / bound"""
    d = (got.detach().double().cpu() - ref.detach().double().cpu()).abs()
    b = elem_bound.detach().double().cpu()
    r = torch.where(d == 0, torch.zeros_like(d), d / b.clamp_min(1e-300))
    i = int(r.argmax())
    print(f"PARITY|{name}|{what}|{float(d.flatten()[i]):.3e}|-|{float(b.flatten()[i]):.3e}")
    rep.require(name, f"{what}: error {float(d.flatten()[i]):.3e} > bound {float(b.flatten()[i]):.3e}", bool((d <= b).all()))


# ================================================================================================================ CIF: fire kernels
def _fire_rows(dev, c, g, T, zhi, out32, dx32, pa32, pb32, rep, name):
    """the _rows entry points on bf16 frames inside a sentinel-filled buffer of a larger row pitch"""
    ops, L = _ops(), _lib()
    B, S, C, thr = c["B"], c["S"], c["C"], c["thr"]
    P = 1 + S + zhi + 2
    full = torch.full((B, P, C), SENT, device=dev, dtype=torch.bfloat16)
    full[:, 1: 1 + S] = c["x"].to(dev).to(torch.bfloat16)
    dfull = torch.full((B, P, C), SENT, device=dev, dtype=torch.bfloat16)
    alpha, csum = c["alpha"].to(dev), c["csum"].to(dev)
    nblk = (C + 255) // 256
    out = torch.full((B, T + 1, C), SENT, device=dev)
    pa, pb = torch.full((nblk, B, S), SENT, device=dev), torch.full((nblk, B, S), SENT, device=dev)
    x0, d0 = full.view(-1)[C:], dfull.view(-1)[C:]
    _rc(L.sc_cif_fwd_rows(ops._p(x0), 1, P * C, ops._p(alpha), ops._p(csum), ops._p(out), B, S, C, T, thr, ops._stream()), "sc_cif_fwd_rows")
    _rc(L.sc_cif_bwd_rows(ops._p(x0), 1, P * C, ops._p(alpha), ops._p(csum), ops._p(g), ops._p(d0), 1, P * C, 1, zhi, ops._p(pa), ops._p(pb),
                          B, S, C, T, thr, ops._stream()), "sc_cif_bwd_rows")
    rep.equal(name, "out, bf16 rows vs fp32 frames", out, out32)
    rep.equal(name, "pa, bf16 rows vs fp32 frames", pa, pa32)
    rep.equal(name, "pb, bf16 rows vs fp32 frames", pb, pb32)
    d = dfull.float()
    _exact(rep, name, "dx rows: zlo / zhi rows zero", torch.cat([d[:, :1], d[:, 1 + S: 1 + S + zhi]], 1), torch.zeros(B, 1 + zhi, C))
    _exact(rep, name, "dx rows: nothing written behind S + zhi", d[:, 1 + S + zhi:], torch.full((B, 2, C), SENT))
    _within(rep, name, "dx rows vs fp32 dx (one bf16 rounding)", d[:, 1: 1 + S], dx32, kc.UB * dx32.double().abs().cpu() + 1e-38)


@pytest.mark.parametrize("S,C", kc.FIRE_SWEEP)
def test_cif_fire_kernels(dev, S, C):
    """sc_cif_fwd / sc_cif_bwd in both kernel forms (one wave per slot / per 8 frames, and the sequential walk of
    sc_set_option(6, 1)), and the _rows forms: S through the one-pass ballot search, its 64 / 65 boundary, a partial last 8-frame
    block and the LDS limit; thr 1 / 0.75 / 0.7; T = 0, 3, 75."""
    ops, L = _ops(), _lib()
    rep = kc.Report()
    try:
        for thr in kc.FIRE_THR:
            c = kc.fire_case(S, C, thr)
            x, alpha, csum = c["x"].to(dev), c["alpha"].to(dev), c["csum"].to(dev)
            for T in kc.FIRE_T:
                name = f"fire S={S} C={C} thr={thr} T={T}"
                g = kc.fire_grad(c, T)
                gd = g.to(dev)
                args = (c["x"], c["alpha"], c["csum"], g)
                auto = kc.fire_autograd(*args, c["thr"], T)
                f64 = kc.fire_formula(*(t.double() for t in args), c["thr"], T)
                ref = dict(auto, pa=f64["pa"], pb=f64["pb"])
                yard = kc.fire_formula(*args, c["thr"], T)
                yard["pa_sum"], yard["pb_sum"] = yard["pa"].double().sum(0), yard["pb"].double().sum(0)
                bounds = kc.fire_bounds(*args, c["thr"], T)
                got = {}
                for opt in (0, 1):
                    L.sc_set_option(6, opt)
                    out = ops.cif_fwd(x, alpha, csum, T, c["thr"])
                    dx, pa, pb = ops.cif_bwd(x, alpha, csum, gd, T, c["thr"])
                    got[opt] = {"out": out, "dx": dx, "pa": pa, "pb": pb}
                    if opt == 0 or T == 3:
                        _fire_rows(dev, c, gd, T, 3 if opt == 0 else 0, out, dx, pa, pb, rep, name + f" form={opt}")
                L.sc_set_option(6, 0)
                for q in ("out", "dx", "pa", "pb"):
                    rep.equal(name, f"{q}, slot / frame form vs sequential form", got[0][q], got[1][q])
                q0 = dict(got[0], pa_sum=got[0]["pa"].double().sum(0), pb_sum=got[0]["pb"].double().sum(0))
                kc.fire_checks(rep, name, q0, ref, yard, bounds)
                right, _ = kc.fire_indices(c["csum"], c["thr"], T)
                past = torch.arange(T + 1)[None] > right[:, -1:]
                rep.require(name, "a slot past the last fire is not exactly zero", bool((got[0]["out"].cpu()[past] == 0).all()))
    finally:
        L.sc_set_option(6, 0)
    rep.done()


def test_cif_refusals(dev):
    """S = 2049, C = 6, thr = 0, a misaligned x and x_bf16 != dx_bf16 are refused on the host with an error that names the
    argument; nothing is launched: the sentinel-filled outputs stay as they were."""
    ops, L = _ops(), _lib()
    B, S, C, T = 2, 16, 8, 3
    mk = lambda *sh: torch.full(sh, SENT, device=dev)
    x, alpha, csum, g = mk(B, 2052, C), mk(B, 2052), mk(B, 2052), mk(B, T + 1, C)
    out, dx, pa, pb = mk(B, T + 1, C), mk(B, 2052, C), mk(1, B, 2052), mk(1, B, 2052)
    p, st = ops._p, ops._stream()
    rep = kc.Report()

    def refused(what, rc, word):
        msg = L.sc_last_error().decode()
        print(f"REFUSAL|{what}|rc={rc}|{msg}")
        rep.require("refusals", f"{what}: accepted", rc != 0)
        rep.require("refusals", f"{what}: the error '{msg}' does not name {word}", word in msg)

    fwd = lambda xp, S_, C_, thr: L.sc_cif_fwd_rows(xp, 0, S_ * C_, p(alpha), p(csum), p(out), B, S_, C_, T, thr, st)
    bwd = lambda xp, xb, db, S_, C_, thr: L.sc_cif_bwd_rows(xp, xb, S_ * C_, p(alpha), p(csum), p(g), p(dx), db, S_ * C_, 0, 0, p(pa), p(pb),
                                                             B, S_, C_, T, thr, st)
    refused("fwd S=2049", fwd(p(x), 2049, C, 1.0), "S=2049")
    refused("bwd S=2049", bwd(p(x), 0, 0, 2049, C, 1.0), "S=2049")
    refused("fwd C=6", fwd(p(x), S, 6, 1.0), "C=6")
    refused("bwd C=6", bwd(p(x), 0, 0, S, 6, 1.0), "C=6")
    refused("fwd thr=0", fwd(p(x), S, C, 0.0), "thr=0")
    refused("bwd thr=0", bwd(p(x), 0, 0, S, C, 0.0), "thr=0")
    off = ctypes.c_void_p(x.data_ptr() + 4)
    refused("fwd misaligned x", fwd(off, S, C, 1.0), "alignment")
    refused("bwd misaligned x", bwd(off, 0, 0, S, C, 1.0), "alignment")
    refused("bwd x_bf16 != dx_bf16", bwd(p(x), 1, 0, S, C, 1.0), "dtype")
    flags = torch.zeros(8, dtype=torch.int32, device=dev)
    i64 = torch.zeros(B, dtype=torch.int64, device=dev)
    u8 = torch.zeros(B, 2052, dtype=torch.uint8, device=dev)
    refused("prepare S=2049", L.sc_cif_prepare(p(alpha), 2052, p(u8), 2052, None, 0, B, 2049, 1.0, 1e-5, 75, T, p(dx), p(x), p(csum), p(pa), p(pb),
                                               p(i64), p(u8), p(flags), st), "S=2049")
    torch.cuda.synchronize()
    for t in (out, dx, pa, pb, x, csum):
        rep.require("refusals", "an output was written", bool((t == SENT).all()))
    rep.require("refusals", "flags were written", int(flags.abs().sum()) == 0)
    rep.done()


# ================================================================================================================ CIF: bookkeeping
def _strided(dev, t, ld, fill):
    buf = torch.full((t.shape[0], ld), fill, device=dev, dtype=t.dtype)
    buf[:, : t.shape[1]] = t.to(dev)
    return buf[:, : t.shape[1]]


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("thr", [1.0, 0.7])
def test_cif_prepare(dev, thr, scale):
    """sc_cif_prepare on a strided alpha_raw and a pad of its own stride: a_clip exact, quantity / csum within one ulp of the fp64
    sum / scan of the fp32 weights, ratio within 4 ulp, alpha exact given the device's ratio, fired / feat_len exactly from the
    device's csum and (unscaled) from fp64, all eight flag words - over two calls, the second without a positive utterance."""
    ops = _ops()
    c = kc.prepare_case(thr, scale)
    B, S, T = c["B"], c["S"], c["T"]
    a_d, pad_d = _strided(dev, c["a_raw"].contiguous(), 256, 9.0), _strided(dev, c["pad"].contiguous(), 264, True)
    assert a_d.stride(0) == 256 and pad_d.stride(0) == 264
    flags = torch.zeros(8, dtype=torch.int32, device=dev)
    flags[2], flags[7] = 77, -5
    tgt = c["target"].to(dev) if scale else None
    r = ops.cif_prepare(a_d, pad_d, tgt, scale, c["thr"], c["eps"], c["max_feat"], T, flags)
    g = {k: v.cpu() for k, v in r.items()}
    args = (c["pad"], c["target"], c["thr"], c["eps"], scale, c["max_feat"], T)
    r64, r32 = kc.prepare_ref(c["a_raw"].double(), *args), kc.prepare_ref(c["a_raw"], *args)
    name = f"prepare thr={thr} scale={scale}"
    rep = kc.Report()
    _exact(rep, name, "a_clip", g["a_clip"], r64["a_clip"].float())
    _within(rep, name, "quantity (1 ulp)", g["quantity"], r64["quantity"], kc.ULP * r64["quantity"].abs())
    _within(rep, name, "ratio (4 ulp)", g["ratio"], r64["ratio"], 4 * kc.ULP * r64["ratio"].abs())
    _exact(rep, name, "alpha = fp32(a_clip ratio)", g["alpha"], g["a_clip"] * g["ratio"][:, None])
    scan = g["alpha"].double().cumsum(-1)
    _within(rep, name, "csum (1 ulp of the fp64 scan of the fp32 weights)", g["csum"], scan, kc.ULP * scan.abs())
    # discrete, (1): from the csum the kernel wrote, fp32 floor(c / thr)
    right, left = kc.fire_indices(g["csum"], c["thr"], T)
    _exact(rep, name, "fired from the device's csum", g["fired"].bool(), right > left)
    cap = min(c["max_feat"], T)
    fl1 = torch.floor(kc.div32(g["csum"][:, -1], c["thr"])).clamp(1, cap).long()
    _exact(rep, name, "feat_len from the device's csum", g["feat_len"], fl1)
    if scale:
        want = c["target"].clamp(1, cap)
        want[3] = 1
        _exact(rep, name, "feat_len = clip(target) (all-zero utterance: 1)", g["feat_len"], want)
    else:                                    # (2): against fp64 from the raw inputs where the decision has margin
        ok_len = (kc.decision_margin(r64["total"], c["thr"]) > kc.COUNT_MARGIN) | (r64["total"] == 0)
        ok = (kc.decision_margin(r64["csum"], c["thr"]) > kc.COUNT_MARGIN) | (r64["csum"] == 0)
        ok = ok & torch.cat([torch.ones_like(ok[:, :1]), ok[:, :-1]], 1) | c["pad"] | (r64["a_clip"] == 0)
        rep.require(name, "more than 1 % of the rows lack margin", bool(ok_len.all()) and float((~ok).float().mean()) <= kc.EXCLUDE_CAP)
        _exact(rep, name, "feat_len vs fp64", g["feat_len"], r64["feat_len"])
        _exact(rep, name, "fired vs fp64 (margin rows)", g["fired"].bool()[ok], r64["fired"][ok])
    rep.yard(name, "alpha vs fp64", g["alpha"], r64["alpha"], r32["alpha"], (1,))
    # second call: every utterance all-zero -> flags[3]; the cumulative words keep counting
    zero = torch.zeros(2, S, device=dev)
    ops.cif_prepare(zero, torch.zeros(2, S, dtype=torch.bool, device=dev), torch.tensor([2, 3], device=dev) if scale else None, scale, c["thr"],
                    c["eps"], c["max_feat"], T, flags)
    pos = int((r64["quantity"] > 0).sum())
    mism = int((r64["feat_len"] != c["target"].clamp(1, c["max_feat"])).sum()) if scale else 0
    want_flags = [pos, mism + (2 if scale else 0), 77, 1, 0, 0, (B - pos + 2) if scale else 0, -5]
    print(f"FLAGS|{name}|{flags.tolist()}|{want_flags}")
    rep.require(name, f"flags {flags.tolist()} != {want_flags}", flags.tolist() == want_flags)
    rep.done()


@pytest.mark.parametrize("kind", kc.COUNT_KINDS)
@pytest.mark.parametrize("S", kc.COUNT_S)
def test_cif_count_property(dev, S, kind):
    """The property the design rests on: the scaled weights sum to target + 1e-5, so feat_len == clip(target, 1, 75) without a host
    read - targets 1 .. 75 in one call, the clamped targets 0 and 80 in a second.  Rows that kw_cases.count_shortfalls names (the
    fp64 sum of the fp32-scaled weights itself below the target) are reported and left out by name."""
    ops = _ops()
    rep = kc.Report()
    for targets in (list(range(1, 76)), [0, 80]):
        a, t = kc.count_case(S, kind, targets)
        short = kc.count_shortfalls(a, t)
        flags = torch.zeros(8, dtype=torch.int32, device=dev)
        r = ops.cif_prepare(a.to(dev), torch.zeros(a.shape, dtype=torch.bool, device=dev), t.to(dev), True, 1.0, kc.f32(1e-5), 75, 75, flags)
        fl, want = r["feat_len"].cpu(), t.clamp(1, 75)
        keep = torch.ones(len(targets), dtype=torch.bool)
        keep[short] = False
        name = f"count S={S} {kind} targets={targets[0]}..{targets[-1]}"
        print(f"COUNT|{name}|shortfalls {short}|device mismatches {(fl != want).nonzero().flatten().tolist()}|flags[1]={int(flags[1])}")
        _exact(rep, name, "feat_len == clip(target, 1, 75)", fl[keep], want[keep])
        rep.require(name, f"flags[1] = {int(flags[1])} beyond the named shortfalls", int(flags[1]) == int((fl != want)[~keep].sum()))
    rep.done()


@pytest.mark.parametrize("with_gq", [False, True])
@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("nblk", [1, 2, 3, 4])
def test_cif_prepare_bwd(dev, nblk, scale, with_gq):
    """sc_cif_prepare_bwd on given fp32 pa / pb against autograd through clip -> mask -> quantity -> scaling -> cumsum, a_raw
    inside [0, 1] with both ends (the precondition in include/speechclip_hip.h).  The all-zero utterance: finite, and d quantity
    alone on its frames (0 / 0 before the guard in cif_prepare_bwd_kernel)."""
    ops = _ops()
    c = kc.prepare_bwd_case(nblk, scale, with_gq)
    auto, r = kc.prepare_bwd_autograd(c["a_raw"], c["pad"], c["target"], c["thr"], c["eps"], scale, c["pa"].double().sum(0),
                                      c["pb"].double().sum(0), c["gq"])
    inp = [r[k].float() for k in ("a_clip", "ratio", "quantity")]
    pad_d = _strided(dev, c["pad"].contiguous(), c["pad"].shape[1] + 5, True)
    da = ops.cif_prepare_bwd(c["pa"].to(dev), c["pb"].to(dev), inp[0].to(dev), pad_d, inp[1].to(dev), inp[2].to(dev),
                             c["gq"].to(dev) if with_gq else None, scale).cpu()
    yard = kc.prepare_bwd_formula(c["pa"], c["pb"], inp[0], c["pad"], inp[1], inp[2], c["gq"], scale)
    bd = kc.prepare_bwd_bound(c["pa"], c["pb"], inp[0], c["pad"], inp[1], inp[2], c["gq"], scale)
    name = f"prepare_bwd nblk={nblk} scale={scale} gq={with_gq}"
    rep = kc.Report()
    rep.derived(name, "da", da, auto, bd, (1,), yard)
    _exact(rep, name, "da on padded frames", da[c["pad"]], torch.zeros(int(c["pad"].sum())))
    z = c["zero_row"]
    rep.require(name, "da of the all-zero utterance is not finite", bool(torch.isfinite(da[z]).all()))
    if scale:
        want = (c["gq"][z] if with_gq else torch.zeros(())) * (~c["pad"][z]).float()
        _exact(rep, name, "da of the all-zero utterance == gq", da[z], want.expand_as(da[z]))
    rep.done()


@pytest.mark.parametrize("T", [3, 75])
def test_cif_tail(dev, T):
    """sc_cif_tail on its own: tail weights 1e-3 below and above tail_thr, a count already at 75 and a count of T."""
    ops = _ops()
    c = kc.tail_case(T)
    args = (c["feat_len"], c["thr"], c["tail_thr"], c["max_feat"], T)
    r64 = kc.tail_ref(c["alpha"].double(), c["csum"].double(), c["out"].double(), *args)
    r32 = kc.tail_ref(c["alpha"], c["csum"], c["out"], *args)
    fl, out = c["feat_len"].to(dev), c["out"].to(dev).clone()
    factor, extend = ops.cif_tail(c["alpha"].to(dev), c["csum"].to(dev), fl, out, T, c["thr"], c["tail_thr"], c["max_feat"])
    name = f"tail T={T}"
    rep = kc.Report()
    _exact(rep, name, "extend", extend.bool(), r64["extend"])
    _exact(rep, name, "feat_len (in place)", fl, r64["feat_len"])
    rep.yard(name, "factor", factor, r64["factor"], r32["factor"], ())
    rep.yard(name, "out", out, r64["out"], r32["out"], (2,))
    o = out.cpu()
    for b in range(o.shape[0]):
        rep.require(name, f"rows >= feat_len of utterance {b} are not exactly zero", float(o[b, int(r64['feat_len'][b]):].abs().sum()) == 0)
    rep.done()


@pytest.mark.parametrize("p1,p2", kc.HEAD_P)
@pytest.mark.parametrize("rows,C", kc.HEAD_SHAPES)
def test_cif_weight_head(dev, rows, C, p1, p2):
    """sc_cif_head_fwd / _bwd / _bwd_rows with ldy > C: alpha and dy per row (the sigmoid path: yardstick rule; the bf16 dy one
    rounding more), dw per column and db from the fp64 sum of the kernel's partials (derived)."""
    ops, L = _ops(), _lib()
    c = kc.whead_case(rows, C)
    auto = kc.whead_autograd(c, p1, p2)
    m1f, m2f = kc.whead_masks(rows, C, p1, p2, torch.float32)
    a32 = auto["alpha"].float()
    yard = dict(kc.whead_bwd_formula(c["y"], c["w"], a32, c["dalpha"], m1f, m2f), alpha=kc.whead_fwd(c["y"], c["w"], c["b"], m1f, m2f))
    bd = kc.whead_sum_bounds(c, a32, p1, p2)
    s1, s2 = kc.HEAD_SEEDS
    y = _strided(dev, c["y"], C + 8, SENT)
    w, b, da = c["w"].to(dev), c["b"].to(dev), c["dalpha"].to(dev)
    alpha = ops.cif_head_fwd(y, w, b, p1, s1, p2, s2)
    name = f"whead rows={rows} C={C} p=({p1}, {p2})"
    rep = kc.Report()
    rep.yard(name, "alpha", alpha, auto["alpha"], yard["alpha"], ())
    nblk, p, st = kc.HEAD_NBLK, ops._p, ops._stream()
    ad = a32.to(dev)
    for bf in (0, 1):
        dy = torch.full((rows, C + 4), SENT, device=dev, dtype=torch.bfloat16 if bf else torch.float32)
        pw, pb = torch.full((nblk, C), SENT, device=dev), torch.full((nblk,), SENT, device=dev)
        if bf:
            rc = L.sc_cif_head_bwd_rows(p(y), y.stride(0), p(w), p(ad), p(da), p(dy), 1, dy.stride(0), p(pw), p(pb), nblk, rows, C, p1, s1, p2, s2, st)
        else:
            rc = L.sc_cif_head_bwd(p(y), y.stride(0), p(w), p(ad), p(da), p(dy), dy.stride(0), p(pw), p(pb), nblk, rows, C, p1, s1, p2, s2, st)
        _rc(rc, "sc_cif_head_bwd")
        tag = " (bf16 rows)" if bf else ""
        if bf:
            e = kc.row_errors(dy[:, :C].float(), auto["dy"], (1,))
            yb = kc.yard_bound(float(kc.row_errors(yard["dy"], auto["dy"], (1,)).max())) + kc.UB
            print(f"PARITY|{name}|dy{tag}|{float(e.max()):.3e}|-|{yb:.3e}")
            rep.require(name, f"dy{tag}: {float(e.max()):.3e} > {yb:.3e}", float(e.max()) <= yb)
        else:
            rep.yard(name, "dy", dy[:, :C], auto["dy"], yard["dy"], (1,))
        _exact(rep, name, f"dy{tag}: columns behind C untouched", dy[:, C:].float(), torch.full((rows, 4), SENT))
        rep.derived(name, "dw" + tag, pw.double().sum(0), auto["dw"], bd["dw"], (), yard["dw"])
        rep.derived(name, "db" + tag, pb.double().sum().reshape(1), auto["db"], bd["db"], (), yard["db"])
    rep.done()


@pytest.mark.parametrize("lead,B,P,head,stop,trail,D", kc.ZERO_PAD_CASES)
def test_rows_zero_pad(dev, lead, B, P, head, stop, trail, D):
    """sc_rows_zero_pad_bf16: exactly the named rows are zero, every other byte is untouched (B = 0, head = 0, stop = P, D = 8 / 768)"""
    ops, L = _ops(), _lib()
    n = lead + B * P + trail
    g = torch.Generator().manual_seed(n + D)
    src = (torch.randn(n + 2, D, generator=g) + 3).to(torch.bfloat16)
    buf = src.to(dev).clone()
    _rc(L.sc_rows_zero_pad_bf16(ops._p(buf), lead, B, max(P, 1), head, stop, trail, D, ops._stream()), "sc_rows_zero_pad_bf16")
    z = torch.cat([kc.zero_pad_rows(lead, B, P, head, stop, trail), torch.zeros(2, dtype=torch.bool)])
    want = src.clone()
    want[z] = 0
    rep = kc.Report()
    _exact(rep, f"zero_pad {(lead, B, P, head, stop, trail, D)}", "buffer bits", buf.cpu().view(torch.int16), want.view(torch.int16))
    rep.done()


# ================================================================================================================ quantiser
@pytest.mark.parametrize("Nk,Et", kc.PREP_SHAPES)
def test_vq_prep_and_norm_bwd(dev, Nk, Et):
    """sc_vq_prep_f32 (16-byte and element load paths, a row stride above Et, a zero row and a row below eps) and
    sc_vq_norm_bwd_f32 (both branches) per row."""
    ops = _ops()
    kw = kc.vq_prep_case(Nk, Et)
    kd = _strided(dev, kw.contiguous(), Et + 4, SENT)
    r64, r32 = kc.vq_prep_ref(kw.double()), kc.vq_prep_ref(kw)
    kwn_T, rnorm = ops.vq_prep(kd, kc.VQ_EPS)
    name = f"vq_prep Nk={Nk} Et={Et}"
    rep = kc.Report()
    rep.yard(name, "rnorm", rnorm, r64["rnorm"], r32["rnorm"], ())
    live = torch.ones(Nk, dtype=torch.bool)
    if Nk >= 3:
        live[1] = False
        _exact(rep, name, "rnorm of a zero row and of a row below eps = 1 / eps", rnorm[1:3].cpu(), r32["rnorm"][1:3])
        _exact(rep, name, "the zero row stays zero", kwn_T[:, 1].cpu(), torch.zeros(Et))
    rep.yard(name, "kwn rows", kwn_T[:, :Nk].t()[live], r64["kwn"][live], r32["kwn"][live], (1,))
    _exact(rep, name, "columns Nk .. ldt zero", kwn_T[:, Nk:].cpu(), torch.zeros(Et, kwn_T.shape[1] - Nk))
    dy = torch.randn(Nk, Et, generator=torch.Generator().manual_seed(1))
    auto = kc.norm_bwd_autograd(kw, dy)
    rn32 = r64["rnorm"].float()
    dx = ops.vq_norm_bwd(kd, rn32.to(dev), _strided(dev, dy, Et + 12, SENT), kc.VQ_EPS)
    rep.yard(name, "norm_bwd dx", dx, auto, kc.norm_bwd_formula(kw, rn32, dy), (1,))
    rep.done()


@pytest.mark.parametrize("V", kc.ROWSTATS_V)
def test_vq_rowstats_soft_bwd(dev, V):
    """sc_vq_rowstats (ldx > V; three temperatures, three mask sets; a masked raw maximum, bit-equal maxima in two live columns,
    an all-equal row), sc_vq_gather_f32 / sc_vq_onehot_f32 exactly, sc_vq_soft_bwd in both output types with Vpad = V and V rounded
    up to 128, NaN in the masked t.  Soft backward: rows whose largest softmax weight is above 0.75 cancel in t - <s, t> and are
    held to the derived bound alone; every other row to the yardstick rule, the yardstick taken over those rows."""
    ops, L = _ops(), _lib()
    x64 = kc.rowstats_case(V)
    x32 = x64.float()
    Nk = x32.shape[0]
    rep = kc.Report()
    p, st = ops._p, ops._stream()
    for cols in kc.ROWSTATS_MASKS:
        xm64, xm32 = kc.mask_cols(x64, cols), kc.mask_cols(x32, cols)
        ok = kc.argmax_margin(xm64)
        for temp in kc.ROWSTATS_TEMP:
            name = f"rowstats V={V} mask={cols} temp={temp}"
            xd = _strided(dev, x32, V + 7, SENT)
            idx, lse_t, lse_1, ent = ops.vq_rowstats(xd, V, temp, cols)
            r64, r32 = kc.rowstats_ref(xm32.double(), temp), kc.rowstats_ref(xm32, temp)
            _exact(rep, name, "x with the masked columns -inf in place", xd.cpu(), xm32)
            _exact(rep, name, "idx from the fp32 scores (first index)", idx, r32["idx"])
            rep.require(name, "more than 1 % of the rows lack margin", float((~ok).float().mean()) <= kc.EXCLUDE_CAP)
            _exact(rep, name, "idx vs fp64 (margin rows)", idx.cpu()[ok], kc.first_argmax(xm64)[ok])
            for q, v in (("lse_t", lse_t), ("lse_1", lse_1), ("ent", ent)):
                rep.yard(name, q, v, r64[q], r32[q], ())
            # soft backward on the fp64 lse_t rounded once; t holds NaN where the mask is
            t = torch.randn(Nk, V, generator=torch.Generator().manual_seed(2))
            auto = kc.soft_bwd_autograd(xm32, t, temp)
            lt32 = r64["lse_t"].float()
            yard = kc.soft_bwd_formula(xm32, lt32, t, temp)
            own = kc.soft_bwd_bound(xm32, lt32, t, temp)
            cancel = kc.soft_bwd_cancel_rows(xm32, lt32, temp)        # held to the derived bound alone; the others to the yardstick rule
            tn = t.clone()
            tn[:, [c_ for c_ in cols if c_ < V]] = float("nan")
            xmd, td = _strided(dev, xm32, V + 7, SENT), _strided(dev, tn, V + 3, SENT)
            for Vpad in (V, -(-V // 128) * 128):
                for bf in (False, True):
                    dx = ops.vq_soft_bwd(xmd, lt32.to(dev), td, V, temp, bf, Vpad)
                    tag = f"soft_bwd Vpad={Vpad} {'bf16' if bf else 'fp32'}"
                    kc.soft_bwd_check(rep, name, tag, dx[:, :V].float(), auto, yard, own, cancel, kc.UB if bf else 0.0)
                    _exact(rep, name, tag + " pad columns zero", dx[:, V:].float().cpu(), torch.zeros(Nk, Vpad - V))
    table = torch.randn(V, 12, generator=torch.Generator().manual_seed(3))
    idx_h = torch.cat([torch.tensor([V - 1, 0]), torch.arange(Nk - 2) % V])
    _exact(rep, f"gather V={V}", "rows", ops.vq_gather(table.to(dev), idx_h.to(dev)), table[idx_h])
    _exact(rep, f"onehot V={V}", "rows", ops.vq_onehot(idx_h.to(dev), V), torch.nn.functional.one_hot(idx_h, V).float())
    rep.done()


@pytest.mark.parametrize("Nk", kc.PERP_NK)
def test_vq_perplexity(dev, Nk):
    """sc_vq_perplexity on the fp64 lse_1 rounded once, Nk = 1 (15 of 16 chunks empty), 17 (two rows a chunk, the last chunk one)
    and 300 (19 rows a chunk), each with nchunk 16 and with nchunk above Nk; the argmax histogram, every row on one token, every
    row on its own token; the workspace used twice (the kernel clears the histogram).  Both figures are exp(-H) of a sum of size
    log V and may meet kw_cases.perplexity_bound instead of the yardstick rule."""
    ops, L = _ops(), _lib()
    p, st = ops._p, ops._stream()
    V = kc.PERP_V
    xm32, l1, sets = kc.perplexity_case(Nk)
    xmd, l1_d = _strided(dev, xm32, V + 7, SENT), l1.to(dev)
    both = torch.ones(2, dtype=torch.bool)                    # code and prob perplexity: each is the exponential of such a sum
    rep = kc.Report()
    for tag in kc.PERP_HIST:
        idx_h = sets[tag]
        assert idx_h.dtype == torch.int64 and idx_h.numel() == Nk and 0 <= int(idx_h.min()) and int(idx_h.max()) < V    # indexed unchecked
        idx_d = idx_h.to(dev)                                 # named: the library is given raw pointers, the tensors must outlive the call
        for nchunk in kc.perplexity_chunks(Nk):
            name = f"perplexity Nk={Nk} {tag} nchunk={nchunk}"
            partial = torch.full((nchunk, V), SENT, device=dev)
            hist = torch.full((V + 64,), 12345, device=dev, dtype=torch.int32)
            out = torch.full((2,), SENT, device=dev)
            for _ in range(2):
                _rc(L.sc_vq_perplexity(p(xmd), xmd.stride(0), Nk, V, p(idx_d), p(l1_d), p(partial), nchunk, p(hist), p(out), st),
                    "sc_vq_perplexity")
            ref = kc.perplexity_ref(xm32.double(), idx_h, l1.double())
            rep.yard(name, "code / prob perplexity", out, ref, kc.perplexity_ref(xm32, idx_h, l1), (),
                     kc.perplexity_bound(xm32, idx_h, l1, nchunk) * ref.abs(), both)
    rep.done()


# ================================================================================================================ BatchNorm
@pytest.mark.parametrize("N,E", kc.BN_SHAPES)
def test_keyword_batchnorm(dev, N, E):
    """sc_bn_rows_fwd / _bwd with strided x / dy / y / dx: N below, at and above the 128 row lanes (1600: the product's), a
    channel of mean 100 and a constant channel; two training steps (running estimates, the unbiased factor at N = 2), the eval
    forward from them, the backward on the fp64 statistics rounded once."""
    ops, L = _ops(), _lib()
    c = kc.bn_case(N, E)
    d = lambda k: c[k].double()
    p, st = ops._p, ops._stream()
    gam, bet = c["gamma"].to(dev), c["beta"].to(dev)
    rm, rv = c["rm0"].to(dev).clone(), c["rv0"].to(dev).clone()
    rm64, rv64, rm32, rv32 = d("rm0"), d("rv0"), c["rm0"], c["rv0"]
    name = f"bn N={N} E={E}"
    rep = kc.Report()
    for step, key in enumerate(("x", "x2")):
        xd = _strided(dev, c[key], E + 3, SENT)
        y = torch.full((N, E + 5), SENT, device=dev)
        sm, sr = torch.empty(E, device=dev), torch.empty(E, device=dev)
        _rc(L.sc_bn_rows_fwd(p(xd), xd.stride(0), N, E, p(gam), p(bet), p(rm), p(rv), 1, kc.BN_MOM, kc.BN_EPS, p(y), y.stride(0), p(sm), p(sr), st),
            "sc_bn_rows_fwd")
        r64 = kc.bn_train_ref(d(key), d("gamma"), d("beta"), rm64, rv64)
        r32 = kc.bn_train_ref(c[key], c["gamma"], c["beta"], rm32, rv32)
        if step == 0:
            bd = kc.bn_sum_bounds(c, r64["save_mean"].float(), r64["save_rstd"].float())
            rep.derived(name, "save_mean", sm, r64["save_mean"], bd["save_mean"], (), r32["save_mean"])
        rep.yard(name, f"save_rstd step {step}", sr, r64["save_rstd"], r32["save_rstd"], ())
        fold = kc.bn_fold_rows(r64["save_mean"], r64["save_rstd"])   # y = fma(x, g, b) cancels where |mean| > 2 sigma: its derived bound
        rep.yard(name, f"y step {step}", y[:, :E], r64["y"], r32["y"], (0,),
                 kc.bn_y_bound(c[key], c["gamma"], c["beta"], r64["save_mean"], r64["save_rstd"]), fold)
        _exact(rep, name, "y: columns behind E untouched", y[:, E:], torch.full((N, 5), SENT))
        rm64, rv64, rm32, rv32 = r64["run_mean"], r64["run_var"], r32["run_mean"], r32["run_var"]
    rep.derived(name, "run_mean after two steps", rm, rm64, kc.bn_run_mean_bound(c), (), rm32)
    rep.yard(name, "run_var after two steps", rv, rv64, rv32, ())
    # eval forward from the fp64 running estimates rounded once
    rme, rve = rm64.float(), rv64.float()
    xd = _strided(dev, c["x"], E + 3, SENT)
    y = torch.full((N, E + 5), SENT, device=dev)
    rme_d, rve_d = rme.to(dev), rve.to(dev)
    _rc(L.sc_bn_rows_fwd(p(xd), xd.stride(0), N, E, p(gam), p(bet), p(rme_d), p(rve_d), 0, kc.BN_MOM, kc.BN_EPS, p(y), y.stride(0), None,
                         None, st), "sc_bn_rows_fwd")
    rep.yard(name, "y eval", y[:, :E], kc.bn_eval_ref(d("x"), d("gamma"), d("beta"), rme.double(), rve.double()),
             kc.bn_eval_ref(c["x"], c["gamma"], c["beta"], rme, rve), (0,),
             kc.bn_y_bound(c["x"], c["gamma"], c["beta"], rme, (rve.double() + kc.BN_EPS).rsqrt()),
             kc.bn_fold_rows(rme, (rve.double() + kc.BN_EPS).rsqrt()))
    # backward on the first step's fp64 statistics rounded once
    r64 = kc.bn_train_ref(d("x"), d("gamma"), d("beta"), d("rm0"), d("rv0"))
    mean32, rstd32 = r64["save_mean"].float(), r64["save_rstd"].float()
    auto = kc.bn_autograd(c)
    yard = kc.bn_bwd_formula(c["x"], c["dy"], c["gamma"], mean32, rstd32)
    bd = kc.bn_sum_bounds(c, mean32, rstd32)
    dyd = _strided(dev, c["dy"], E + 9, SENT)
    dx = torch.full((N, E + 5), SENT, device=dev)
    dg, db = torch.empty(E, device=dev), torch.empty(E, device=dev)
    mean_d, rstd_d = mean32.to(dev), rstd32.to(dev)
    _rc(L.sc_bn_rows_bwd(p(xd), xd.stride(0), p(dyd), dyd.stride(0), N, E, p(gam), p(mean_d), p(rstd_d), p(dx), dx.stride(0), p(dg),
                         p(db), st), "sc_bn_rows_bwd")
    rep.yard(name, "dx", dx[:, :E], auto["dx"], yard["dx"], (0,))
    _exact(rep, name, "dx: columns behind E untouched", dx[:, E:], torch.full((N, 5), SENT))
    rep.derived(name, "dgamma", dg, auto["dgamma"], bd["dgamma"], (), yard["dgamma"])
    rep.derived(name, "dbeta", db, auto["dbeta"], bd["dbeta"], (), yard["dbeta"])
    rep.done()


# ================================================================================================================ softmax
def _softmax_case(dev, rep, c, name, backward=True):
    ops, L = _ops(), _lib()
    rows, n, rpb, scale = c["rows"], c["n"], kc.SOFTMAX_RPB, c["scale"]
    sd, md = c["scores"].to(dev), c["mask"].to(dev).to(torch.uint8).contiguous()
    P64, P32y = kc.softmax_ref(c["scores"].double(), c["mask"], rpb, scale), kc.softmax_ref(c["scores"], c["mask"], rpb, scale)
    P32 = torch.full((rows, n), SENT, device=dev)
    _rc(L.sc_softmax_fwd_f32(ops._p(sd), ops._p(md), ops._p(P32), rows, n, rpb, scale, ops._stream()), "sc_softmax_fwd_f32")
    rep.yard(name, "P fp32", P32, P64, P32y, (1,))
    P32c = P32.cpu()
    _exact(rep, name, "fully masked batch: zeros", P32c[rpb: 2 * rpb], torch.zeros(rpb, n))
    one = torch.zeros(rpb, n)
    one[:, n - 1] = 1.0
    _exact(rep, name, "single live key: exactly 1", P32c[2 * rpb: 3 * rpb], one)
    for p in (0.0, 0.25):
        P, Pd = ops.softmax_fwd(sd, md, rpb, scale, p, kc.SOFTMAX_SEED)
        _within(rep, name, f"P bf16 vs P fp32 (one bf16 rounding) p={p}", P.float(), P32c, kc.UB * P32c.double().abs())
        keep = kc.softmax_keep(rows, n, p)
        if p > 0:
            # the kernel scales the unrounded probability and rounds once: bf16(P32 / (1 - p)) where kept, 0 where dropped
            want = torch.where(keep, P32c * torch.tensor(1.0 / (1.0 - p), dtype=torch.float32), torch.zeros(())).to(torch.bfloat16)
            _exact(rep, name, f"Pd = keep P / (1 - p), bits p={p}", Pd.cpu().view(torch.int16), want.view(torch.int16))
            _within(rep, name, f"Pd vs the stored P (one bf16 rounding) p={p}", Pd.float(), P.float().cpu().double() * keep / (1 - p),
                    2.02 * kc.UB * P.float().cpu().double() / (1 - p))
        if backward:
            Pb = P.float().cpu()
            dS = ops.softmax_bwd(c["dP"].to(dev), P, scale, p, kc.SOFTMAX_SEED)
            ref = kc.softmax_bwd_formula(c["dP"].double(), Pb.double(), scale, keep, p)
            yard = kc.bf16_values(kc.softmax_bwd_formula(c["dP"], Pb, scale, keep, p))
            rep.derived(name, f"dS p={p}", dS.float(), ref, kc.softmax_bwd_bound(c["dP"], Pb, scale, keep, p), (1,), yard)


@pytest.mark.parametrize("scale", kc.SOFTMAX_SCALE)
@pytest.mark.parametrize("n", kc.SOFTMAX_N)
def test_softmax_rows(dev, n, scale):
    """sc_softmax_fwd_f32, sc_softmax_fwd (P, Pd) and sc_softmax_bwd at every template instance and its edges (n = 516 .. 768: four
    chunks with an empty fourth), rows_per_batch = 5, a fully masked batch and a batch with one live key, p = 0 and 0.25.  The dS
    reference is the softmax-backward formula in fp64 evaluated at the bf16 P the kernel is given (a rounded P is no softmax of any
    scores, so autograd cannot be run at it); tests/test_kw_cases_cpu.py shows formula == autograd at the exact fp64 P."""
    rep = kc.Report()
    _softmax_case(dev, rep, kc.softmax_case(n, scale), f"softmax n={n} scale={scale}")
    rep.done()


def test_softmax_grid_stride_loop(dev):
    """66000 rows: 464 more than the 16384 workgroups x 4 waves of the largest grid, so the row loop of the first 464 waves takes a
    second trip"""
    rows, n = kc.SOFTMAX_LONG
    rep = kc.Report()
    _softmax_case(dev, rep, kc.softmax_case(n, 0.37, rows=rows), f"softmax rows={rows} n={n}")
    rep.done()


def test_softmax_refusals(dev):
    ops, L = _ops(), _lib()
    p, st = ops._p, ops._stream()
    s = torch.full((4, 1032), SENT, device=dev)
    m = torch.zeros(4, 1032, dtype=torch.uint8, device=dev)
    P = torch.full((4, 1032), SENT, device=dev, dtype=torch.bfloat16)
    Pd = P.clone()
    rep = kc.Report()
    calls = (("n=6", lambda: L.sc_softmax_fwd(p(s), p(m), p(P), None, 4, 6, 1, 1.0, 0.0, 0, st), "n=6"),
             ("n=1028", lambda: L.sc_softmax_fwd(p(s), p(m), p(P), None, 4, 1028, 1, 1.0, 0.0, 0, st), "n=1028"),
             ("Pd with p=0", lambda: L.sc_softmax_fwd(p(s), p(m), p(P), p(Pd), 4, 8, 1, 1.0, 0.0, 0, st), "Pd"),
             ("f32 n=6", lambda: L.sc_softmax_fwd_f32(p(s), p(m), p(s), 4, 6, 1, 1.0, st), "n=6"),
             ("bwd n=1028", lambda: L.sc_softmax_bwd(p(s), p(P), p(Pd), 4, 1028, 1.0, 0.0, 0, st), "n=1028"))
    for what, call, word in calls:
        rc = call()
        msg = L.sc_last_error().decode()                      # read after each call: the library keeps the last error only
        print(f"REFUSAL|{what}|rc={rc}|{msg}")
        rep.require("softmax refusals", f"{what}: accepted", rc != 0)
        rep.require("softmax refusals", f"{what}: the error '{msg}' does not name {word}", word in msg)
    torch.cuda.synchronize()
    rep.require("softmax refusals", "an output was written", bool((P == SENT).all()) and bool((Pd == SENT).all()) and bool((s == SENT).all()))
    rep.done()
