"""Properties of the builders, references and criteria in tests/kw_cases.py that tests/test_gpu_kw_kernels.py relies on: no GPU
needed.  Every reference runs in both dtypes; each hand-written backward formula equals autograd in fp64 to 1e-12; the fp32
yardstick meets every derived bound against fp64; the reference alone stays inside the exclusion cap of the discrete rules; the
cases have the coverage the GPU tests assume; a row moved by 1.5 x its bound is rejected."""
import pytest
import torch

import kw_cases as kc

AUTOGRAD_TOL = 1e-12
CPU_FIRE = [(S, C) for S, C in kc.FIRE_SWEEP if S * C <= 129 * 768]          # all nine thr x T; the widest case once (test_fire_widest_case_once)


def _close(a, b):
    return kc.rel_l2(a, b) <= AUTOGRAD_TOL


# ------------------------------------------------------------------------------------------------------------------ CIF: fire
def test_fire_sweep_covers_the_kernel_paths():
    S_ = [S for S, _ in kc.FIRE_SWEEP]
    assert 64 in S_ and 65 in S_ and kc.MAXS in S_ and any(S < 64 for S in S_) and any(S % 8 for S in S_ if S > 8)
    assert any(C > 256 and C % 256 for _, C in kc.FIRE_SWEEP) and any(C == 1024 for _, C in kc.FIRE_SWEEP)
    for thr in kc.FIRE_THR:
        c = kc.fire_case(129, 768, thr)
        t = c["thr"]
        assert c["lens"].tolist() == [129, 1, 86, 65] and float(c["alpha"][0].max()) >= 2 * t
        assert bool((c["alpha"][0, :129] == 0).any()) and float(c["alpha"][1].sum()) < t
        assert c["csum"][3, 1].item() == t and c["csum"][3, 2].item() == 2 * t and c["csum"][3, 3].item() == 4 * t      # exact landings
        for b in range(4):
            assert float(c["alpha"][b, int(c["lens"][b]):].abs().sum()) == 0
        assert float(c["csum"][0, -1]) > 4 * t                               # T = 3 clips, and a frame fires across the clipped boundary
        right, left = kc.fire_indices(c["csum"], t, 75)
        assert int((right - left).max()) >= 2                                # a multi-fire frame
        assert torch.equal(c["x"].to(torch.bfloat16).float(), c["x"])
    assert float(kc.fire_case(499, 1024, 1.0)["csum"][0, -1]) > 76           # the clip at T = 75 engages


@pytest.mark.parametrize("S,C", CPU_FIRE)
def test_fire_formula_is_autograd_and_yardstick_is_within_bounds(S, C):
    rep = kc.Report()
    for thr in kc.FIRE_THR:
        c = kc.fire_case(S, C, thr)
        for T in kc.FIRE_T:
            g = kc.fire_grad(c, T)
            args = (c["x"], c["alpha"], c["csum"], g)
            auto = kc.fire_autograd(*args, c["thr"], T)
            f64 = kc.fire_formula(*(t.double() for t in args), c["thr"], T)
            assert _close(f64["out"], auto["out"]) and _close(f64["dx"], auto["dx"])
            assert _close(f64["pa"].sum(0), auto["pa_sum"]) and _close(f64["pb"].sum(0), auto["pb_sum"])
            yard = kc.fire_formula(*args, c["thr"], T)
            yard["pa_sum"], yard["pb_sum"] = yard["pa"].double().sum(0), yard["pb"].double().sum(0)
            ref = dict(f64, pa_sum=auto["pa_sum"], pb_sum=auto["pb_sum"])
            kc.fire_checks(rep, f"cpu fire S={S} C={C} thr={thr} T={T}", yard, ref, yard, kc.fire_bounds(*args, c["thr"], T))
            right, _ = kc.fire_indices(c["csum"], c["thr"], T)
            for b in range(4):                                               # slots past the last fire: exactly zero
                assert float(f64["out"][b, int(right[b, -1]) + 1:].abs().sum()) == 0
    rep.done()


def test_fire_widest_case_once():
    """(499, 1024): four channel blocks at a large S, one thr / T combination (the clip at T = 75 engaged, thr = 0.7)"""
    c = kc.fire_case(499, 1024, 0.7)
    T = 75
    g = kc.fire_grad(c, T)
    args = (c["x"], c["alpha"], c["csum"], g)
    auto = kc.fire_autograd(*args, c["thr"], T)
    f64 = kc.fire_formula(*(t.double() for t in args), c["thr"], T)
    assert f64["pa"].shape[0] == 4
    assert _close(f64["out"], auto["out"]) and _close(f64["dx"], auto["dx"])
    assert _close(f64["pa"].sum(0), auto["pa_sum"]) and _close(f64["pb"].sum(0), auto["pb_sum"])
    yard = kc.fire_formula(*args, c["thr"], T)
    yard["pa_sum"], yard["pb_sum"] = yard["pa"].double().sum(0), yard["pb"].double().sum(0)
    rep = kc.Report()
    kc.fire_checks(rep, "cpu fire S=499 C=1024 thr=0.7 T=75", yard, dict(f64, pa_sum=auto["pa_sum"], pb_sum=auto["pb_sum"]), yard,
                   kc.fire_bounds(*args, c["thr"], T))
    rep.done()


def test_fire_bound_rejects_a_moved_row():
    c = kc.fire_case(65, 260, 0.7)
    g = kc.fire_grad(c, 3)
    args = (c["x"], c["alpha"], c["csum"], g)
    ref = kc.fire_formula(*(t.double() for t in args), c["thr"], 3)
    bd = kc.fire_bounds(*args, c["thr"], 3)
    for q in ("out", "dx", "pa"):
        bad = ref[q].clone()
        i = (0, 0) if q == "out" else (0, int(c["alpha"][0].argmax())) if q == "dx" else (1, 0, int(c["alpha"][0].argmax()))
        assert float(bd[q][i].max()) > 0
        bad[i] += 1.5 * (bd[q][i].max() if q != "pa" else bd[q][i])
        rep = kc.Report()
        rep.derived("moved", q, bad, ref[q], bd[q], kc.FIRE_DIMS[q])
        assert len(rep.bad) == 1, q
        rep = kc.Report()
        rep.derived("exact", q, ref[q], ref[q], bd[q], kc.FIRE_DIMS[q])
        assert not rep.bad


# ------------------------------------------------------------------------------------------------------------------ CIF: bookkeeping
@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("thr", [1.0, 0.7])
def test_prepare_reference_both_dtypes_and_exclusion_cap(thr, scale):
    c = kc.prepare_case(thr, scale)
    a, pad = c["a_raw"], c["pad"]
    assert a.stride(0) > c["S"] and pad.stride(0) > c["S"] and pad.stride(0) != a.stride(0)
    assert float(a.min()) < 0 and float(a.max()) > 1
    args = (pad, c["target"], c["thr"], c["eps"], scale, c["max_feat"], c["T"])
    r64, r32 = kc.prepare_ref(a.double(), *args), kc.prepare_ref(a, *args)
    assert torch.equal(r64["a_clip"].float(), r32["a_clip"])                 # clip and mask are exact
    assert float(r64["quantity"][3]) == 0 and float(r64["alpha"][3].abs().sum()) == 0 and int(r64["feat_len"][3]) == 1
    assert float((r32["csum"].double() - r64["csum"]).abs().max()) < 1e-4
    if scale:
        want = c["target"].clamp(1, min(c["max_feat"], c["T"]))
        want[3] = 1
        assert torch.equal(r64["feat_len"], want)
    else:                                                                    # the discrete rule (2): the reference alone is inside the cap
        ok_len = (kc.decision_margin(r64["total"], c["thr"]) > kc.COUNT_MARGIN) | (r64["total"] == 0)       # an all-zero utterance is exact
        ok_frame = (kc.decision_margin(r64["csum"], c["thr"]) > kc.COUNT_MARGIN) | (r64["csum"] == 0)
        ok_frame = ok_frame & torch.cat([torch.ones_like(ok_frame[:, :1]), ok_frame[:, :-1]], 1) | pad | (r64["a_clip"] == 0)
        assert bool(ok_len.all()) and float((~ok_frame).float().mean()) <= kc.EXCLUDE_CAP
        assert torch.equal(r32["feat_len"], r64["feat_len"])
        assert torch.equal(r32["fired"][ok_frame], r64["fired"][ok_frame])


@pytest.mark.parametrize("kind", kc.COUNT_KINDS)
@pytest.mark.parametrize("S", kc.COUNT_S)
def test_count_property_of_the_fp32_scaling(S, kind):
    """The fp64 sum of the fp32-scaled weights against the target: rows that fall short are the arithmetic's, named by
    count_shortfalls; every other row gives clip(target, 1, 75) under fp32 floor()."""
    for targets in (list(range(1, 76)), [0, 80]):
        a, t = kc.count_case(S, kind, targets)
        assert float(a.min()) >= 0 and float(a.max()) <= 1 and bool((a.sum(-1) > 0).all())
        if kind == "wide":
            assert float(a[a > 0].min()) < 1e-3
        tot = kc.count_fp32_total(a, t)
        short = kc.count_shortfalls(a, t)
        print(f"COUNT|S={S} {kind} targets={targets[0]}..{targets[-1]}|min margin {float((tot - t.clamp(0, 80).double()).min()):.3e}"
              f"|shortfalls {short}")
        fl = torch.floor(kc.div32(tot.float(), 1.0)).clamp(1, 75).long()
        keep = torch.ones(len(targets), dtype=torch.bool)
        keep[short] = False
        assert torch.equal(fl[keep], t.clamp(1, 75)[keep])
        assert len(short) <= 0.05 * len(targets) + 1


@pytest.mark.parametrize("with_gq", [False, True])
@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("nblk", [1, 2, 3, 4])
def test_prepare_bwd_formula_is_autograd(nblk, scale, with_gq):
    c = kc.prepare_bwd_case(nblk, scale, with_gq)
    assert float(c["a_raw"].min()) == 0 and float(c["a_raw"].max()) == 1      # the precondition: inside [0, 1], both ends included
    auto, r = kc.prepare_bwd_autograd(c["a_raw"], c["pad"], c["target"], c["thr"], c["eps"], scale, c["pa"].double().sum(0),
                                      c["pb"].double().sum(0), c["gq"])
    gq64 = c["gq"].double() if with_gq else None
    f64 = kc.prepare_bwd_formula(c["pa"].double(), c["pb"].double(), r["a_clip"], c["pad"], r["ratio"], r["quantity"], gq64, scale)
    assert _close(f64, auto)
    z = c["zero_row"]
    want = (gq64[z] if with_gq else torch.zeros(())) * (~c["pad"][z]).double()
    assert bool(torch.isfinite(auto).all()) and (not scale or torch.equal(auto[z], want.expand_as(auto[z])))
    assert float(auto[c["pad"]].abs().sum()) == 0
    inp = [r[k].float() for k in ("a_clip", "ratio", "quantity")]
    yard = kc.prepare_bwd_formula(c["pa"], c["pb"], inp[0], c["pad"], inp[1], inp[2], c["gq"], scale)
    bd = kc.prepare_bwd_bound(c["pa"], c["pb"], inp[0], c["pad"], inp[1], inp[2], c["gq"], scale)
    rep = kc.Report()
    rep.derived(f"cpu prepare_bwd nblk={nblk} scale={scale} gq={with_gq}", "da", yard, auto, bd, (1,))
    bad = auto.clone()
    bad[1, 7] += 1.5 * bd[1].max()
    n = len(rep.bad)
    rep.derived("moved", "da", bad, auto, bd, (1,))
    assert n == 0 and len(rep.bad) == 1, rep.bad


@pytest.mark.parametrize("T", [3, 75])
def test_tail_cases_are_unambiguous(T):
    c = kc.tail_case(T)
    args = (c["feat_len"], c["thr"], c["tail_thr"], c["max_feat"], T)
    r64 = kc.tail_ref(c["alpha"].double(), c["csum"].double(), c["out"].double(), *args)
    r32 = kc.tail_ref(c["alpha"], c["csum"], c["out"], *args)
    assert float((r64["tw"] - c["tail_thr"]).abs().min()) > 0.9e-3
    assert r64["extend"].tolist() == [False, True, False, True, True] and torch.equal(r32["extend"], r64["extend"])
    assert int(c["feat_len"][-1]) == min(T, 75) and torch.equal(r32["feat_len"], r64["feat_len"])
    assert int(r64["feat_len"][-1]) == min(T + 1, 75)
    for b in range(5):
        assert float(r64["out"][b, int(r64["feat_len"][b]):].abs().sum()) == 0
    assert float(kc.row_errors(r32["out"], r64["out"], (2,)).max()) < 1e-6 and float(kc.row_errors(r32["factor"], r64["factor"], ()).max()) < 1e-6


@pytest.mark.parametrize("p1,p2", kc.HEAD_P)
@pytest.mark.parametrize("rows,C", kc.HEAD_SHAPES)
def test_weight_head_formula_is_autograd(rows, C, p1, p2):
    c = kc.whead_case(rows, C)
    auto = kc.whead_autograd(c, p1, p2)
    m1, m2 = kc.whead_masks(rows, C, p1, p2, torch.float64)
    f64 = kc.whead_bwd_formula(c["y"].double(), c["w"].double(), auto["alpha"], c["dalpha"].double(), m1, m2)
    assert all(_close(f64[k], auto[k]) for k in ("dy", "dw", "db"))
    a32 = auto["alpha"].float()
    m1f, m2f = kc.whead_masks(rows, C, p1, p2, torch.float32)
    yard = kc.whead_bwd_formula(c["y"], c["w"], a32, c["dalpha"], m1f, m2f)
    bd = kc.whead_sum_bounds(c, a32, p1, p2, chain=rows)                      # the bound as derived, for a plain fp32 sum over the rows
    rep = kc.Report()
    rep.derived(f"cpu whead rows={rows} C={C}", "dw", yard["dw"], auto["dw"], bd["dw"], ())
    rep.derived(f"cpu whead rows={rows} C={C}", "db", yard["db"], auto["db"], bd["db"], ())
    rep.done()                                                                 # (dy goes by the yardstick rule: nothing derived to meet)
    for q, i in (("dw", C // 2), ("db", 0)):
        bad = auto[q].clone()
        bad[i] += 1.5 * kc.whead_sum_bounds(c, a32, p1, p2)[q][i]              # the device's bound (its own, shorter chains)
        rep = kc.Report()
        rep.derived("moved", q, bad, auto[q], kc.whead_sum_bounds(c, a32, p1, p2)[q], ())
        assert len(rep.bad) == 1, q
    if p1 > 0:
        assert abs(float((m1 > 0).double().mean()) - (1 - p1)) < 0.1 or rows * C < 2048


def test_zero_pad_rows_cover_the_edges():
    cs = kc.ZERO_PAD_CASES
    assert any(c[1] == 0 for c in cs) and any(c[3] == 0 for c in cs) and any(c[4] == c[2] for c in cs) and {c[6] for c in cs} >= {8, 768}
    for lead, B, P, head, stop, trail, D in cs:
        z = kc.zero_pad_rows(lead, B, P, head, stop, trail)
        assert int(z.sum()) == lead + B * (head + P - stop) + trail


# ------------------------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("Nk,Et", kc.PREP_SHAPES)
def test_vq_prep_and_norm_bwd_references(Nk, Et):
    kw = kc.vq_prep_case(Nk, Et)
    assert kw.stride(0) > Et
    r64, r32 = kc.vq_prep_ref(kw.double()), kc.vq_prep_ref(kw)
    assert float(kc.row_errors(r32["kwn"], r64["kwn"], (1,)).max()) < 1e-6
    if Nk >= 3:
        assert float(r32["rnorm"][1]) == float(r32["rnorm"][2]) == float(1.0 / torch.tensor(kc.VQ_EPS, dtype=torch.float32))
    dy = torch.randn(Nk, Et, generator=torch.Generator().manual_seed(1))
    auto = kc.norm_bwd_autograd(kw, dy)
    f64 = kc.norm_bwd_formula(kw.double(), r64["rnorm"], dy.double())
    assert _close(f64, auto)
    if Nk >= 3:
        assert _close(auto[1], dy[1].double() / kc.VQ_EPS) and _close(auto[2], dy[2].double() / kc.VQ_EPS)      # the clamped branch


@pytest.mark.parametrize("V", kc.ROWSTATS_V)
def test_rowstats_references_and_argmax_cap(V):
    x64 = kc.rowstats_case(V)
    x32 = x64.float()
    assert x32[1, 1] == x32[1, 4] and float(x32[1].max()) == float(x32[1, 1]) and int((x32[1] == x32[1].max()).sum()) == 2
    assert int(x32[0].argmax()) == 0 and all(1 not in cols and 4 not in cols for cols in kc.ROWSTATS_MASKS)       # the tie stays live
    for cols in kc.ROWSTATS_MASKS:
        xm64, xm32 = kc.mask_cols(x64, cols), kc.mask_cols(x32, cols)
        ok = kc.argmax_margin(xm64)
        assert float((~ok).float().mean()) <= kc.EXCLUDE_CAP
        for temp in kc.ROWSTATS_TEMP:
            r64, r32 = kc.rowstats_ref(xm32.double(), temp), kc.rowstats_ref(xm32, temp)
            assert torch.equal(r64["idx"], r32["idx"]) and torch.equal(kc.first_argmax(xm64)[ok], r32["idx"][ok])
            assert int(r32["idx"][1]) == 1                                   # the first of the two bit-equal maxima, at every V
            if 0 in cols:
                assert int(r32["idx"][0]) != 0
            for q in ("lse_t", "lse_1", "ent"):
                assert bool(torch.isfinite(r32[q]).all()) and float(kc.row_errors(r32[q], r64[q], ()).max()) < 1e-4, (q, temp)
            t = torch.randn(x32.shape, generator=torch.Generator().manual_seed(2))
            auto = kc.soft_bwd_autograd(xm32, t, temp)
            tn = t.double().clone()
            tn[:, list(c for c in cols if c < V)] = float("nan")             # the formula ignores what t holds in masked columns
            f64 = kc.soft_bwd_formula(xm32.double(), kc.rowstats_ref(xm32.double(), temp)["lse_t"], tn, temp)
            assert _close(f64, auto), (cols, temp)
            # the fp32 formula on the rounded lse_t: inside the derived bound on every row.  The rows whose largest weight is above
            # 0.75 go by that bound alone, the others by the yardstick rule with the yardstick taken over them only: that figure
            # stays at the 1e-5 level, and in either group a row moved by 1.5 x its bound is rejected
            lt32 = kc.rowstats_ref(xm32.double(), temp)["lse_t"].float()
            yard, own = kc.soft_bwd_formula(xm32, lt32, t, temp), kc.soft_bwd_bound(xm32, lt32, t, temp)
            cancel = kc.soft_bwd_cancel_rows(xm32, lt32, temp)
            name = f"cpu soft_bwd V={V} mask={cols} temp={temp}"
            rep = kc.Report()
            rep.derived(name, "dx", yard, auto, own, (1,))
            kc.soft_bwd_check(rep, name, "dx", yard, auto, yard, own, cancel)
            rep.done()
            ey = kc.row_errors(yard, auto, (1,))
            if bool((~cancel).any()):
                assert float(ey[~cancel].max()) < 3e-5, float(ey[~cancel].max())
            if temp == 1.0:
                assert not bool(cancel.any()) or V == 5
            for group in (cancel, ~cancel):
                if not bool(group.any()):
                    continue
                r = int(group.nonzero()[0])
                rule = kc.yard_bound(float(ey[~cancel].max())) if bool((~cancel).any()) else 0.0
                b = float(own[r].max()) if bool(cancel[r]) else rule * float(auto[r].abs().max())
                bad = auto.clone()
                bad[r, int(auto[r].abs().argmax())] += 1.5 * b
                rep = kc.Report()
                kc.soft_bwd_check(rep, "moved", "dx", bad, auto, yard, own, cancel)
                assert len(rep.bad) == 1, (cols, temp, bool(cancel[r]))
    assert V != 5 or bool(cancel.any())                      # two live columns 1.8 / 0.03 apart: the case the finding is about


@pytest.mark.parametrize("Nk", kc.PERP_NK)
def test_perplexity_cases(Nk):
    """The chunking the three sizes are there for, the reference in both dtypes, the yardstick inside perplexity_bound, a value
    moved by 1.5 x the larger of the two criteria rejected."""
    V = kc.PERP_V
    xm32, l1, sets = kc.perplexity_case(Nk)
    assert set(sets) == set(kc.PERP_HIST) and V >= max(kc.PERP_NK) + 3 and V > 256 and V % 256
    rpc = -(-Nk // 16)
    used, last = -(-Nk // rpc), Nk - (-(-Nk // rpc) - 1) * rpc
    assert (Nk, rpc, used, last) in ((1, 1, 1, 1), (17, 2, 9, 1), (300, 19, 16, 15))
    assert kc.perplexity_chunks(Nk)[0] == 16 and kc.perplexity_chunks(Nk)[1] > Nk
    assert int(sets["one token"].unique().numel()) == 1 and int(sets["all different"].unique().numel()) == Nk
    assert bool(torch.isinf(xm32[:, [0, 2, 3]]).all()) and float((l1.double() - kc.rowstats_ref(xm32.double(), 1.0)["lse_1"]).abs().max()) < 1e-6
    both = torch.ones(2, dtype=torch.bool)
    for tag, idx in sets.items():
        assert idx.dtype == torch.int64 and 0 <= int(idx.min()) and int(idx.max()) < V and not bool(torch.isinf(xm32[0, idx]).any())
        pp64, pp32 = kc.perplexity_ref(xm32.double(), idx, l1.double()), kc.perplexity_ref(xm32, idx, l1)
        if tag == "one token":
            assert abs(float(pp64[0]) - 1) < 1e-6
        if tag == "all different":
            assert abs(float(pp64[0]) - Nk) < 1e-3 * Nk
        for nchunk in kc.perplexity_chunks(Nk):
            pb = kc.perplexity_bound(xm32, idx, l1, nchunk)
            e = kc.row_errors(pp32, pp64, ())
            assert bool((e <= pb).all()) and float(pb.max()) < (1e-4 if nchunk == 16 else 2e-4), (tag, nchunk, e, pb)     # (303 partials in order)
            moved = pp64 * (1 + 1.5 * torch.maximum(pb, torch.full_like(pb, kc.yard_bound(float(e.max())))))
            rep = kc.Report()
            rep.yard("moved", "perplexity", moved, pp64, pp32, (), pb * pp64.abs(), both)
            assert len(rep.bad) == 1
            rep = kc.Report()
            rep.yard("yardstick", "perplexity", pp32, pp64, pp32, (), pb * pp64.abs(), both)
            rep.done()


# ------------------------------------------------------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("N,E", kc.BN_SHAPES)
def test_bn_formula_is_autograd_and_yardstick_is_within_bounds(N, E):
    assert any(n > kc.BN_RL for n, _ in kc.BN_SHAPES) and any(n == kc.BN_RL + 1 for n, _ in kc.BN_SHAPES)
    c = kc.bn_case(N, E)
    d = lambda k: c[k].double()
    r64 = kc.bn_train_ref(d("x"), d("gamma"), d("beta"), d("rm0"), d("rv0"))
    auto = kc.bn_autograd(c)
    f64 = kc.bn_bwd_formula(d("x"), d("dy"), d("gamma"), r64["save_mean"], r64["save_rstd"])
    assert all(_close(f64[k], auto[k]) for k in ("dx", "dgamma", "dbeta"))
    assert abs(float(r64["save_mean"][0]) - 100) < 3 and float(r64["save_rstd"][1]) == float((torch.tensor(kc.BN_EPS, dtype=torch.float64)).rsqrt())
    if N == 2:
        var = ((d("x") - r64["save_mean"]) ** 2).mean(0)
        assert _close(r64["run_var"], 0.9 * d("rv0") + 0.1 * var * 2.0)      # the unbiased factor N / (N - 1) = 2
    mean32, rstd32 = r64["save_mean"].float(), r64["save_rstd"].float()
    r32 = kc.bn_train_ref(c["x"], c["gamma"], c["beta"], c["rm0"], c["rv0"])
    y32 = kc.bn_bwd_formula(c["x"], c["dy"], c["gamma"], mean32, rstd32)
    bd = kc.bn_sum_bounds(c, mean32, rstd32)
    rep = kc.Report()
    name = f"cpu bn N={N} E={E}"
    rep.derived(name, "save_mean", r32["save_mean"], r64["save_mean"], bd["save_mean"], ())
    rep.derived(name, "dbeta", y32["dbeta"], auto["dbeta"], bd["dbeta"], ())
    rep.derived(name, "dgamma", y32["dgamma"], auto["dgamma"], bd["dgamma"], ())
    rep.done()
    # run_mean after two steps (x, then x2): the fp32 chain inside its derived bound; a channel moved by 1.5 x is rejected
    s1 = kc.bn_train_ref(c["x"], c["gamma"], c["beta"], c["rm0"], c["rv0"])
    s2 = kc.bn_train_ref(c["x2"], c["gamma"], c["beta"], s1["run_mean"], s1["run_var"])
    t1 = kc.bn_train_ref(d("x"), d("gamma"), d("beta"), d("rm0"), d("rv0"))
    t2 = kc.bn_train_ref(d("x2"), d("gamma"), d("beta"), t1["run_mean"], t1["run_var"])
    rb = kc.bn_run_mean_bound(c)
    rep.derived(name, "run_mean", s2["run_mean"], t2["run_mean"], rb, ())
    rep.done()
    bad = t2["run_mean"].clone()
    bad[3] += 1.5 * rb[3]
    rep.derived("moved", "run_mean", bad, t2["run_mean"], rb, ())
    assert len(rep.bad) == 1
    rep.bad.pop()
    bad = auto["dgamma"].clone()
    bad[2] += 1.5 * bd["dgamma"][2]
    rep.derived("moved", "dgamma", bad, auto["dgamma"], bd["dgamma"], ())
    assert len(rep.bad) == 1
    # y: the folded form fma(x, g, b) in fp32 stays inside bn_y_bound, misses the yardstick rule on the mean-100 and constant
    # channels, and a channel moved by 1.5 x max(yardstick rule, its bound) is still rejected
    g32 = c["gamma"] * rstd32
    folded = c["x"] * g32 + (c["beta"] - mean32 * g32)
    yb = kc.bn_y_bound(c["x"], c["gamma"], c["beta"], r64["save_mean"], r64["save_rstd"])
    fold = kc.bn_fold_rows(r64["save_mean"], r64["save_rstd"])
    assert bool(fold[0]) and bool(fold[1]) and int(fold.sum()) < E       # the mean-100 and the constant channel, never every channel
    rep = kc.Report()
    rep.yard(name, "y folded", folded, r64["y"], r32["y"], (0,), yb, fold)
    rep.done()
    if N == 1600:                                            # the product's row count: the folded form misses the yardstick rule alone
        rep.yard(name, "y folded, yardstick rule alone", folded, r64["y"], r32["y"], (0,))
        assert len(rep.bad) == 1
    e_rule = kc.yard_bound(float(kc.row_errors(r32["y"], r64["y"], (0,)).max()))
    plain = int((~fold).nonzero()[0])
    for ch, b in ((0, max(e_rule * float(r64["y"][:, 0].abs().max()), float(yb[:, 0].max()))),      # a named channel: the larger of the two
                  (plain, e_rule * float(r64["y"][:, plain].abs().max()))):                          # any other: the yardstick rule alone
        bad = r64["y"].clone()
        bad[:, ch] += 1.5 * b
        rep = kc.Report()
        rep.yard("moved", "y", bad, r64["y"], r32["y"], (0,), yb, fold)
        assert len(rep.bad) == 1, ch


# ------------------------------------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("scale", kc.SOFTMAX_SCALE)
@pytest.mark.parametrize("n", kc.SOFTMAX_N)
def test_softmax_references(n, scale):
    assert any(516 <= m <= 768 for m in kc.SOFTMAX_N) and kc.SOFTMAX_LONG[0] > 65536
    c = kc.softmax_case(n, scale)
    rpb = kc.SOFTMAX_RPB
    P64, P32 = kc.softmax_ref(c["scores"].double(), c["mask"], rpb, c["scale"]), kc.softmax_ref(c["scores"], c["mask"], rpb, c["scale"])
    assert float(P64[rpb: 2 * rpb].abs().sum()) == 0 and float(P32[rpb: 2 * rpb].abs().sum()) == 0             # the fully masked batch
    assert bool((P32[2 * rpb: 3 * rpb, n - 1] == 1).all()) and float(P32[2 * rpb: 3 * rpb, : n - 1].abs().sum()) == 0
    live = torch.ones(c["rows"], dtype=torch.bool)
    live[rpb: 2 * rpb] = False
    assert float((P64[live].sum(-1) - 1).abs().max()) < 1e-12
    assert float(kc.row_errors(P32, P64, (1,)).max()) < 1e-5
    rep = kc.Report()
    for p in (0.0, 0.25):
        keep = kc.softmax_keep(c["rows"], n, p)
        Pa, dS = kc.softmax_bwd_autograd(c["scores"], c["mask"], rpb, c["scale"], c["dP"], keep, p)
        assert _close(kc.softmax_bwd_formula(c["dP"].double(), Pa, c["scale"], keep, p), dS)
        Pb = kc.bf16_values(P64.float())                                     # the bf16 P the backward kernel is given
        ref = kc.softmax_bwd_formula(c["dP"].double(), Pb.double(), c["scale"], keep, p)
        yard = kc.bf16_values(kc.softmax_bwd_formula(c["dP"], Pb, c["scale"], keep, p))
        bd = kc.softmax_bwd_bound(c["dP"], Pb, c["scale"], keep, p)
        rep.derived(f"cpu softmax n={n} scale={scale} p={p}", "dS", yard, ref, bd, (1,))
        if n >= 72 and p == 0.0:
            bad = ref.clone()
            bad[0] += 1.5 * bd[0].max()
            k = len(rep.bad)
            rep.derived("moved", "dS", bad, ref, bd, (1,))
            assert len(rep.bad) == k + 1
            rep.bad.pop()
    rep.done()


def test_yardstick_rule_rejects_a_moved_row():
    """max(4 x yardstick, 2^-23): a row moved by 1.5 x that bound fails, the yardstick itself passes"""
    c = kc.softmax_case(260, 0.37)
    P64, P32 = kc.softmax_ref(c["scores"].double(), c["mask"], kc.SOFTMAX_RPB, c["scale"]), kc.softmax_ref(c["scores"], c["mask"], kc.SOFTMAX_RPB, c["scale"])
    b = kc.yard_bound(float(kc.row_errors(P32, P64, (1,)).max()))
    rep = kc.Report()
    rep.yard("yard", "P", P32, P64, P32, (1,))
    assert not rep.bad
    bad = P64.clone()
    bad[0, 130] += 1.5 * b * float(P64[0].max())
    rep.yard("moved", "P", bad, P64, P32, (1,))
    assert len(rep.bad) == 1
