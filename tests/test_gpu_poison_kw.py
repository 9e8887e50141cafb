"""The keyword side of the model and the loss-side buffers do not depend on the bytes a kernel reads but the mathematics excludes
(docs/parity.md, "What a kernel reads and must ignore", subsection "Keyword side"): the quantiser's padded rows and columns, frames
behind an utterance's length and slots behind its keyword count in CIF, masked keys of the row softmax and of the constant-query
pool, keyword rows behind the count in the prompt, caller-owned buffers reused across calls and chunks, the criteria's workspaces
and the rings of the negative queue.

  (a) every kernel by value: a clean run (excluded places zero) against runs with FINITE_POISON and with NONFINITE_POISON in the
      excluded places -> the valid outputs carry the clean run's bits, the promised zeros are exact zeros; the clean run itself is held
      against the fp64 restatement the project has for that kernel (tests/kw_cases.py, kwpool_cases.py, vq_modes_cases.py).  Where a
      contract says "finite" the non-finite run is left out for that region alone, and the case says so.  One planted check per mask:
      the same poison in ONE element the mathematics reads changes the output.
  (b) whole forward paths of the three keyword recipes under poisoned_empty: warm module, fresh module.
  (c) whole train steps: twice, torch.empty = NaN on a warm and on a fresh model, after a step on a LARGER batch (more keywords,
      longer utterances), with the branch's dropout on, and with the quantiser soft at a learnable temperature.
  (d) the four criteria under poisoned_empty and the model's queue / bank across a wrap of the rings.

Values only: every operand carries its padding inside its own tensor (tests/test_poison_cases_cpu.py holds the largest index each
contract allows against every allocation).  No tolerance: every assertion is bit equality against a clean run, an exact zero, or a
bound the case files derive."""
import dataclasses

import numpy as np
import pytest
import torch

import kw_cases as kc
import kwpool_cases as kp
import poison_cases as pc
import vq_modes_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TEMP = 0.1
SEED = 4242
_CACHE = {}
POISONS = (("finite poison", pc.FINITE_POISON), ("non-finite poison", pc.NONFINITE_POISON))


def _ops():
    from speechclip_plus_amd import ops
    return ops


def _poison(t, mask, patterns):
    return pc.poison_bf16(t, mask, patterns) if t.dtype == torch.bfloat16 else pc.poison_f32(t, mask, patterns)


def _view(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(rep, tag, what, got, clean, names=None):
    """every entry of ``got`` carries the bits of ``clean``: one POISON line (differing elements, NaN count) before anything is required"""
    names = list(clean) if names is None else names
    diff = {n: int((_view(got[n]) != _view(clean[n])).sum()) if got[n].shape == clean[n].shape else -1 for n in names}
    nan = sum(int(torch.isnan(got[n].float()).sum()) for n in names if got[n].is_floating_point())
    print(f"POISON|{tag}|{what}|{len(names)} outputs, {sum(1 for v in diff.values() if v)} differ ({sum(abs(v) for v in diff.values())} elements)|NaN {nan}")
    for n, v in diff.items():
        rep.require(tag, f"{what}: {n} differs from the clean run in {v} elements", v == 0)
    return not any(diff.values())


def _changed(tag, what, got, clean, names):
    """the planted check: at least one of ``names`` no longer carries the clean run's bits"""
    moved = pc.changed(got, clean, names)
    print(f"POISON|{tag}|planted: {what}|outputs that changed: {moved}")
    return bool(moved)


# ================================================================================================================== (a) quantiser
def _quantiser_case(Nk, V):
    """keywords near table rows (a decided argmax), the table, and the device operands of the score product - built once per shape"""
    if (Nk, V) not in _CACHE:
        ops = _ops()
        Et = pc.KW_ET
        lay = pc.quantiser_layout(Nk, V, Et)
        g = torch.Generator().manual_seed(Nk * 7 + V)
        table = torch.randn(V, Et, generator=g)
        kw = table[torch.randint(4, V, (Nk,), generator=g)] + 0.8 * torch.randn(Nk, Et, generator=g)
        t = torch.zeros(lay.Nkp, lay.Vp)
        t[:Nk, :V] = torch.randn(Nk, V, generator=g)
        wn = table / table.norm(dim=-1, keepdim=True).clamp_min(1e-8)
        kw_d, wn_d = kw.to(DEV), wn.to(DEV).contiguous()
        with pc.poisoned_empty():           # the padded outputs come from torch.empty = NaN: the zeros below are the kernels' own
            kwn_T, rnorm = ops.vq_prep(kw_d)
            c = {"lay": lay, "table": table, "kw": kw, "t": t, "wn": wn, "rnorm": rnorm,
                 "kw_split": ops.split3_bf16(kw_d, 0, row_scale=rnorm).cpu(), "kwn_T": kwn_T.cpu(),
                 "table_split": ops.split3_bf16(wn_d, 1, rows_pad=128).cpu(), "norm_T": torch.zeros(Et, lay.Vp)}
            torch.cuda.synchronize()
        c["norm_T"][:, :V] = wn.t()
        # the kernels write their own padding as zeros (vq.hip:64, :89-95): the clean operands ARE zero under every mask
        assert tuple(c["kw_split"].shape) == (lay.Nkp, 6 * lay.Ep) and tuple(c["table_split"].shape) == (lay.Vp, 6 * lay.Ep)
        assert bool((c["kw_split"][lay.kw_split] == 0).all()) and bool((c["table_split"][lay.table_split] == 0).all())
        assert bool((c["kwn_T"][lay.kwn_T] == 0).all())
        _CACHE[(Nk, V)] = c
    return _CACHE[(Nk, V)]


def _scores(lay, kw_split, table_split, kwn_T, norm_T):
    """both score products on the given operands -> {"split": cos [Nkp, Vp] of the bf16 GEMM over the six K-blocks, "fp32": of the
    exact-fp32 GEMM} on the device"""
    ops = _ops()
    for name, (last, numel) in pc.quantiser_read_extent(lay).items():
        assert last < numel, name
    A, TS = kw_split.to(DEV), table_split.to(DEV)
    K6 = A.shape[1]
    assert A.numel() == lay.Nkp * K6 and TS.numel() == lay.Vp * K6
    cos = torch.zeros(lay.Nkp, lay.Vp, device=DEV)
    ops.gemm_raw(A, K6, TS, K6, cos, lay.Vp, lay.Nkp, lay.Vp, K6, out_f32=True)
    return {"split": cos, "fp32": ops.sgemm_mfma(kwn_T.to(DEV), norm_T.to(DEV), a_kmajor=True, b_kmajor=True)}


def _row_kernels(c, cos, t, s_rows=None, w_cols=None, s_plant=None, w_plant=None):
    """every row kernel of the quantiser and both selections on x = cos[:Nk] (a copy: sc_vq_rowstats writes the mask into it) ->
    dict of CPU tensors.  ``s_rows`` / ``w_cols``: patterns for rows >= Nk of the soft split and for the pad columns of the soft table."""
    ops = _ops()
    lay = c["lay"]
    Nk, V, Vp, Et = lay.Nk, lay.V, lay.Vp, lay.Et
    cos = cos.to(DEV).clone()
    assert tuple(cos.shape) == (lay.Nkp, Vp) and tuple(t.shape) == (lay.Nkp, Vp)
    x, td = cos[:Nk], t.to(DEV)[:Nk]
    table_d = c["table"].to(DEV)
    out = {}
    idx, lse_t, lse_1, ent = ops.vq_rowstats(x, V, TEMP)
    out.update(idx=idx, lse_t=lse_t, lse_1=lse_1, ent=ent, masked=x[:, :V].clone(), ppl=ops.vq_perplexity(x, V, idx, lse_1))
    out["gather"], out["onehot"] = ops.vq_gather(table_d, idx), ops.vq_onehot(idx, V)
    out["soft_bwd"] = ops.vq_soft_bwd(x, lse_t, td, V, TEMP, True, Vp)
    W = ops.vq_soft_table(table_d, Vp)
    if w_cols is not None:
        W = _poison(W.cpu(), lay.w_split, w_cols).to(DEV)
    if w_plant is not None:
        W = pc.plant(W.cpu(), w_plant).to(DEV)
    for noise in (False, True):
        n = "_g" if noise else ""
        idx2, stats = ops.vq_noisy_rowstats(x, V, TEMP, SEED, noise)
        out["idx" + n + "2"], out["stats" + n] = idx2, stats
        out["s" + n] = ops.vq_soft_prob(x, stats, V, TEMP, SEED, noise)
        split = ops.vq_soft_split(x, stats, V, TEMP, Vp, SEED, noise)
        assert tuple(split.shape) == (lay.Nkp, 3 * Vp)
        if s_rows is not None:
            split = _poison(split.cpu(), lay.s_split, s_rows).to(DEV)
        if s_plant is not None:
            split = pc.plant(split.cpu(), s_plant).to(DEV)
        out["kw_soft" + n] = ops.vq_soft_product(split, W, Et)[:Nk]
        dx, dtemp = ops.vq_soft_bwd2(x, stats, td, V, TEMP, True, Vp, SEED, noise, want_dtemp=True)
        out["dx" + n], out["dtemp" + n] = dx, dtemp
        out["dx32" + n] = ops.vq_soft_bwd2(x, stats, td, V, TEMP, False, Vp, SEED, noise)[0]
    for k in pc.KW_TOPK:
        fn = ops.topk_rows if k <= 32 else ops.topk_rows_wide
        out[f"top{k}_vals"], out[f"top{k}_idx"] = fn(x, V, k)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in out.items()}


def _t32(tau):
    return float(np.float32(tau))


def _quantiser_against_fp64(rep, tag, c, sc, got):
    """the clean run against fp64: the split product as close to fp64 as the exact-fp32 product (tests/test_gpu_tail_kernels.py), the
    row statistics by the yardstick rule of tests/kw_cases.py, the soft family by the bounds of tests/vq_modes_cases.py"""
    lay = c["lay"]
    Nk, V = lay.Nk, lay.V
    kwn = (c["kw"].to(DEV) * c["rnorm"][:, None]).double().cpu()
    ref = kwn @ c["wn"].double().t()
    e_split = float((sc["split"][:Nk, :V].double().cpu() - ref).abs().max())
    e_fp32 = float((sc["fp32"][:Nk, :V].double().cpu() - ref).abs().max())
    print(f"PARITY|{tag}|cos, split product vs fp64|{e_split:.3e}|{e_fp32:.3e}|{2.0 * e_fp32 + 1e-7:.3e}")
    rep.require(tag, f"cos: split product error {e_split:.3e} > 2 x {e_fp32:.3e} + 1e-7", e_split <= 2.0 * e_fp32 + 1e-7)
    xm32 = got["masked"]
    rep.require(tag, "the special columns of x are not -inf", bool(torch.isneginf(xm32[:, list(vc.SPECIAL)]).all()))
    r64, r32 = kc.rowstats_ref(xm32.double(), TEMP), kc.rowstats_ref(xm32, TEMP)
    rep.require(tag, "idx is not the first argmax of the fp32 scores", torch.equal(got["idx"], r32["idx"]))
    for q in ("lse_t", "lse_1"):
        rep.yard(tag, q, got[q], r64[q], r32[q], ())
    # the yardstick rule, as tests/test_gpu_kw_kernels.py applies it; at kw_cases.ENT_FEW_ROWS (5 rows of V = 8112: too few rows for
    # the yardstick to sample the common shift of a row's probabilities) a row may meet kw_cases.rowstats_ent_bound instead
    few = (Nk, V) == kc.ENT_FEW_ROWS
    rep.yard(tag, "ent", got["ent"], r64["ent"], r32["ent"], (), kc.rowstats_ent_bound(xm32) if few else None,
             torch.ones(Nk, dtype=torch.bool) if few else None)
    nchunk = max(1, min(16, Nk))
    pref = kc.perplexity_ref(xm32.double(), got["idx"], got["lse_1"].double())
    rep.yard(tag, "code / prob perplexity", got["ppl"], pref, kc.perplexity_ref(xm32, got["idx"], got["lse_1"]), (),
             kc.perplexity_bound(xm32, got["idx"], got["lse_1"], nchunk) * pref.abs(), torch.ones(2, dtype=torch.bool))
    rep.require(tag, "gather is not table[idx]", torch.equal(got["gather"], c["table"][got["idx"]]))
    rep.require(tag, "onehot is not the one-hot of idx", torch.equal(got["onehot"], torch.nn.functional.one_hot(got["idx"], V).float()))
    x = xm32.double().numpy()
    tau = _t32(TEMP)
    table = c["table"].double().numpy()
    t = c["t"][:Nk, :V].double().numpy()
    for noise in (False, True):
        n = "_g" if noise else ""
        g = vc.gumbel(Nk, V, SEED) if noise else None
        f = vc.forward(x, tau, False, g, table)
        m, ls = vc.row_statistics(x if g is None else x + g, tau)
        bm, bls = vc.rowstats_bounds(x, tau, noise, V)
        st = got["stats" + n].double().numpy()
        rm, rls = float((np.abs(st[0] - m) / bm).max()), float((np.abs(st[1] - ls) / bls).max())
        E_s = vc.prob_rel_bound(x, tau, noise, V)
        rs = float((np.abs(got["s" + n].double().numpy() - f["s"]) / (E_s * f["s"] + 2.0 ** -126)).max())
        rk = float((np.abs(got["kw_soft" + n].double().numpy() - f["keywords"]) / vc.keyword_bound(f["s"], table, E_s, V)).max())
        _, rdx, _, _ = vc.backward(f["s"], f["z"], t, tau)
        rd = float((np.abs(got["dx32" + n][:, :V].double().numpy() - rdx) / (vc.dx_bound(f["s"], t, tau, E_s, V) + 2.0 ** -126)).max())
        # the bf16 form is the fp32 form rounded once, to nearest even: the same bits as torch's conversion
        rep.require(tag, f"noise={noise}: the bf16 dx is not the rounded fp32 dx", pc.bits_equal(got["dx" + n], got["dx32" + n].to(torch.bfloat16)))
        for q, r in (("max", rm), ("log sum", rls), ("s", rs), ("soft keywords", rk), ("dx", rd)):
            print(f"PARITY|{tag} noise={noise}|{q}: error / bound|{r:.3e}|-|1.000e+00")
            rep.require(tag, f"noise={noise}: {q} error / bound {r:.3f} > 1", r <= 1.0)
        rep.require(tag, f"noise={noise}: s of a special column is not exactly 0", bool((got["s" + n][:, list(vc.SPECIAL)] == 0).all()))
    for k in pc.KW_TOPK:
        want = torch.topk(xm32, min(k, V), dim=-1)
        rep.require(tag, f"top-{k} values are not torch.topk's", torch.equal(got[f"top{k}_vals"][:, : min(k, V)], want.values))


@pytest.mark.parametrize("V", pc.KW_V)
@pytest.mark.parametrize("Nk", pc.KW_NK)
def test_quantiser_ignores_its_padding(Nk, V):
    """Regions (docs/parity.md): 1 rows >= Nk of the keyword split and the matching columns of kwn_T; 2 rows >= V of the table split
    and the matching columns of the normalised table; 3 cos[:, V:] and cos[Nk:, :] (and t under the same mask and in the special
    columns) handed to the row kernels and the selections; rows >= Nk of the soft split (any bits) and the pad columns of the soft
    table - "finite" there: the soft split holds exact zeros in its own pad columns and the product is 0 x w."""
    c = _quantiser_case(Nk, V)
    lay = c["lay"]
    tag = f"quantiser Nk={Nk} V={V}"
    rep = kc.Report()
    valid = lambda sc: {k: v[:Nk, :V].cpu() for k, v in sc.items()}
    clean_sc = _scores(lay, c["kw_split"], c["table_split"], c["kwn_T"], c["norm_T"])
    clean_cos = valid(clean_sc)
    tmask = lay.cos.clone()
    tmask[:, list(vc.SPECIAL)] = True
    clean = _row_kernels(c, clean_sc["split"], c["t"])
    assert all(bool(torch.isfinite(v.float()).all()) for k, v in clean.items() if k not in ("masked",) and not k.endswith("_vals"))
    _quantiser_against_fp64(rep, tag, c, clean_sc, clean)
    for what, pat in POISONS:
        ks, kt = _poison(c["kw_split"], lay.kw_split, pat), _poison(c["kwn_T"], lay.kwn_T, pat)
        ts, nt = _poison(c["table_split"], lay.table_split, pat), _poison(c["norm_T"], lay.norm_T, pat)
        _same(rep, tag, f"{what}, region 1: keyword rows >= Nk", valid(_scores(lay, ks, c["table_split"], kt, c["norm_T"])), clean_cos)
        _same(rep, tag, f"{what}, region 2: table rows >= V", valid(_scores(lay, c["kw_split"], ts, c["kwn_T"], nt)), clean_cos)
        both = _scores(lay, ks, ts, kt, nt)
        _same(rep, tag, f"{what}, regions 1 + 2", valid(both), clean_cos)
        finite = pat is pc.FINITE_POISON
        # region 3, twice: the score matrix the poisoned products wrote, and the clean one with the patterns put into its padding
        for src, cos in (("as the poisoned products wrote it", both["split"].cpu()),
                         ("patterns in cos[:, V:] and cos[Nk:, :]", _poison(clean_sc["split"].cpu(), lay.cos, pat))):
            got = _row_kernels(c, cos, _poison(c["t"], tmask, pat), s_rows=pat, w_cols=pat if finite else None)
            _same(rep, tag, f"{what}, region 3 ({src}; soft table pad columns {'poisoned' if finite else 'clean: finite only'})", got, clean)
            for n in ("soft_bwd", "dx", "dx_g", "dx32", "dx32_g"):
                rep.require(tag, f"{what}: {n} is not exactly zero in the columns >= V", bool((got[n][:, V:] == 0).all()))
    # planted: the same poison in ONE element the mathematics reads
    first = torch.zeros(lay.Nkp, lay.Vp, dtype=torch.bool)
    first[Nk - 1, V - 1] = True                                 # the last valid score: one column in front of the pad columns
    rep.require(tag, "planted NaN in the last valid score changed nothing",
                _changed(tag, "cos[Nk - 1, V - 1]", _row_kernels(c, pc.plant(clean_sc["split"].cpu(), first), c["t"]), clean, ["lse_t", "top5_idx", "s"]))
    row = torch.zeros(lay.Nkp, 6 * lay.Ep, dtype=torch.bool)
    row[Nk - 1] = True                                          # the last valid keyword row of the split
    planted = _scores(lay, _poison(c["kw_split"], row, pc.NONFINITE_POISON), c["table_split"], pc.plant(c["kwn_T"], ~lay.kwn_T & (torch.arange(lay.Nkp) == Nk - 1)[None]), c["norm_T"])
    rep.require(tag, "planted poison in the last valid keyword row changed nothing", _changed(tag, "keyword row Nk - 1", valid(planted), clean_cos, ["split"]))
    rep.require(tag, "planted poison in the last valid keyword row changed nothing (fp32 product)", _changed(tag, "kwn_T column Nk - 1", valid(planted), clean_cos, ["fp32"]))
    trow = torch.zeros(lay.Vp, 6 * lay.Ep, dtype=torch.bool)
    trow[V - 1] = True                                          # region 2: the last valid table row of the split, column V - 1 of norm_T
    planted = _scores(lay, c["kw_split"], _poison(c["table_split"], trow, pc.NONFINITE_POISON), c["kwn_T"],
                      pc.plant(c["norm_T"], ~lay.norm_T & (torch.arange(lay.Vp) == V - 1)[None]))
    rep.require(tag, "planted poison in the last valid table row changed nothing", _changed(tag, "table row V - 1", valid(planted), clean_cos, ["split"]))
    rep.require(tag, "planted poison in the last valid table row changed nothing (fp32 product)", _changed(tag, "norm_T column V - 1", valid(planted), clean_cos, ["fp32"]))
    srow = torch.zeros(lay.Nkp, 3 * lay.Vp, dtype=torch.bool)
    srow[Nk - 1, 1] = True                                      # a live row of the soft split (block hi, a live column)
    rep.require(tag, "planted NaN in a live row of the soft split changed nothing",
                _changed(tag, "s_split[Nk - 1]", _row_kernels(c, clean_sc["split"].cpu(), c["t"], s_plant=srow), clean, ["kw_soft", "kw_soft_g"]))
    wcol = torch.zeros(lay.Et, 3 * lay.Vp, dtype=torch.bool)
    wcol[0, V - 1] = True                                       # the last live column of the soft table: one in front of its pad columns
    rep.require(tag, "planted NaN in the last live column of the soft table changed nothing",
                _changed(tag, "w_split[0, V - 1]", _row_kernels(c, clean_sc["split"].cpu(), c["t"], w_plant=wcol), clean, ["kw_soft", "kw_soft_g"]))
    rep.done()


# ================================================================================================================== (a) CIF
def _cif_run(c, x, alpha, csum, g, T=pc.CIF_T):
    """sc_cif_fwd, sc_cif_bwd (the slot / frame kernels and the sequential walk must agree) and sc_cif_tail on a copy of out"""
    from speechclip_plus_amd._lib import lib
    ops = _ops()
    for name, (last, numel) in pc.cif_read_extent(c, T).items():
        assert last < numel, name
    xd, ad, cd, gd = (t.contiguous().to(DEV) for t in (x, alpha, csum, g))
    assert tuple(xd.shape) == (c["B"], c["S"], c["C"]) and tuple(gd.shape) == (c["B"], T + 1, c["C"])
    res = {}
    try:
        for opt in (0, 1):
            lib().sc_set_option(6, opt)
            out = ops.cif_fwd(xd, ad, cd, T, 1.0)
            dx, pa, pb = ops.cif_bwd(xd, ad, cd, gd, T, 1.0)
            res[opt] = {"out": out, "dx": dx, "pa": pa, "pb": pb}
    finally:
        lib().sc_set_option(6, 0)
    # the partials' only consumer, on the partials as the backward wrote them (pad frames included)
    da = ops.cif_prepare_bwd(res[0]["pa"], res[0]["pb"], c["a_clip"].to(DEV), c["pad"].to(DEV), c["ratio"].to(DEV), c["quantity"].to(DEV),
                             c["gq"].to(DEV), True)
    fl = c["last"].clamp(min=1).to(DEV)
    tail = res[0]["out"].clone()
    factor, extend = ops.cif_tail(ad, cd, fl, tail, T, 1.0, 0.5, 75)
    torch.cuda.synchronize()
    r = {k: v.cpu() for k, v in res[0].items()}
    r.update({k + "_seq": v.cpu() for k, v in res[1].items()}, tail=tail.cpu(), feat_len=fl.cpu(), factor=factor.cpu(), extend=extend.cpu(),
             da=da.cpu())
    return r


def _cif_valid(c, r, T=pc.CIF_T):
    """what the contract promises: out on the slots up to the last one a frame lands in, dx / pa / pb on the frames t < len, the tail's
    results"""
    keep_s, keep_f = ~pc.slot_mask(c["last"], T), ~c["pad"]
    v = {}
    for sfx in ("", "_seq"):
        v["out" + sfx] = r["out" + sfx][keep_s]
        v["dx" + sfx] = r["dx" + sfx][keep_f]
        v["pa" + sfx], v["pb" + sfx] = r["pa" + sfx][:, keep_f], r["pb" + sfx][:, keep_f]
    v.update(tail=r["tail"], feat_len=r["feat_len"], factor=r["factor"], extend=r["extend"], da=r["da"])
    return v


def test_cif_ignores_frames_behind_the_length_and_slots_behind_the_count():
    """Regions: x on the frames t >= len - "finite": their weight alpha is an exact 0 and the walk forms 0 x x (cif.hip:111, :263-266),
    so the non-finite run is left out for x; pa of those frames is x . g[left] - Inf or NaN under the finite poison - and
    sc_cif_prepare_bwd, its only consumer, runs on it here: da of the valid frames keeps its bits (this round's second fix: the scaling
    term selects on a_clip != 0 instead of forming 0 x pa); g on the slots behind the slot the last frame lands in (the keyword count) - any bits.
    alpha and csum of the frames t >= len are OPERANDS (0 and the running total: the kernels take no length): sc_cif_prepare writes
    them from the pad mask, and what it must ignore there is alpha_raw - any bits.  Slot ``count`` itself is read: the weight left over
    behind the last fire lands there (1e-5 with the target scaling), and the planted check shows it."""
    ops = _ops()
    c = pc.cif_case()
    T, tag = pc.CIF_T, f"cif S={pc.CIF_S} C={pc.CIF_C} lens {list(pc.CIF_LENS)} targets {list(pc.CIF_TARGETS)}"
    rep = kc.Report()
    gen = torch.Generator().manual_seed(91)
    behind = pc.slot_mask(c["last"], T)                            # strictly behind the count
    g = torch.randn(c["B"], T + 1, c["C"], generator=gen) * (~behind)[..., None]
    xmask, gmask = pc.row_mask(c["pad"].reshape(-1), c["C"]).view(c["B"], c["S"], c["C"]), pc.row_mask(behind.reshape(-1), c["C"]).view(c["B"], T + 1, c["C"])
    assert int(xmask.sum()) > 0 and int(gmask.sum()) > 0 and bool((c["alpha"][c["pad"]] == 0).all())
    raw = _cif_run(c, c["x"], c["alpha"], c["csum"], g)
    clean = _cif_valid(c, raw)
    # the clean run against fp64 (tests/kw_cases.py: derived bounds), the two kernel forms against each other
    args = (c["x"], c["alpha"], c["csum"], g)
    auto = kc.fire_autograd(*args, 1.0, T)
    f64 = kc.fire_formula(*(t.double() for t in args), 1.0, T)
    yard = kc.fire_formula(*args, 1.0, T)
    yard["pa_sum"], yard["pb_sum"] = yard["pa"].double().sum(0), yard["pb"].double().sum(0)
    q0 = {k: raw[k] for k in ("out", "dx", "pa", "pb")}
    q0.update(pa_sum=raw["pa"].double().sum(0), pb_sum=raw["pb"].double().sum(0))
    kc.fire_checks(rep, tag, q0, dict(auto, pa=f64["pa"], pb=f64["pb"]), yard, kc.fire_bounds(*args, 1.0, T))
    for q in ("out", "dx", "pa", "pb"):
        rep.equal(tag, f"{q}, slot / frame form vs sequential form", raw[q], raw[q + "_seq"])
    pargs = (raw["pa"], raw["pb"], c["a_clip"], c["pad"], c["ratio"], c["quantity"], c["gq"], True)
    rep.derived(tag, "da (sc_cif_prepare_bwd on the kernel's own partials)", raw["da"], kc.prepare_bwd_formula(*(t.double() if torch.is_tensor(t) and t.is_floating_point() else t for t in pargs)),
                kc.prepare_bwd_bound(*pargs), (1,), kc.prepare_bwd_formula(*pargs))
    rep.require(tag, "da of a frame t >= len is not exactly zero on the clean run", bool((raw["da"][c["pad"]] == 0).all()))
    rep.require(tag, "out behind the last slot a frame lands in is not exactly zero", bool((raw["out"][behind] == 0).all()))
    rep.require(tag, "dx of a frame t >= len is not exactly zero on the clean run", bool((raw["dx"][c["pad"]] == 0).all()))
    tr = kc.tail_ref(c["alpha"].double(), c["csum"].double(), raw["out"].double(), c["last"].clamp(min=1), 1.0, 0.5, 75, T)
    rep.require(tag, "tail: extend / feat_len differ from fp64", torch.equal(raw["extend"].bool(), tr["extend"]) and torch.equal(raw["feat_len"], tr["feat_len"]))
    for b in range(c["B"]):
        rep.require(tag, f"tail: rows >= feat_len of utterance {b} are not exactly zero", float(raw["tail"][b, int(raw["feat_len"][b]):].abs().sum()) == 0)
    runs = [("finite poison in x of the frames t >= len (finite only: 0 x x)", _poison(c["x"], xmask, pc.FINITE_POISON), g)]
    for what, pat in POISONS:
        runs.append((f"{what} in g behind the count", c["x"], _poison(g, gmask, pat)))
    runs.append(("finite poison in x, non-finite in g", runs[0][1], _poison(g, gmask, pc.NONFINITE_POISON)))
    for what, x, gg in runs:
        with pc.poisoned_empty():
            got = _cif_run(c, x, c["alpha"], c["csum"], gg)
        _same(rep, tag, what, _cif_valid(c, got), clean)
        rep.require(tag, f"{what}: out behind the last slot is not exactly zero", bool((got["out"][behind] == 0).all()))
        rep.require(tag, f"{what}: da of a frame t >= len is not exactly zero", bool((got["da"][c["pad"]] == 0).all()))
        if x is not c["x"]:
            print(f"POISON|{tag}|{what}|pa of the frames t >= len: {int((~torch.isfinite(got['pa'][:, c['pad']])).sum())} of {got['pa'][:, c['pad']].numel()} not finite")
        if gg is g:
            rep.require(tag, f"{what}: dx of a frame t >= len is not exactly zero", bool((got["dx"][c["pad"]] == 0).all()))
    # sc_cif_prepare: alpha_raw of the padded frames, any bits -> alpha exactly 0 there, every output the clean run's
    a_raw = (torch.rand(c["B"], c["S"], generator=gen) * (~c["pad"])).contiguous()
    tgt = torch.tensor(pc.CIF_TARGETS)

    def prepare(a):
        flags = torch.zeros(8, dtype=torch.int32, device=DEV)
        r = ops.cif_prepare(a.to(DEV), c["pad"].to(DEV), tgt.to(DEV), True, 1.0, kc.f32(1e-5), 75, T, flags)
        return {k: v.cpu() for k, v in r.items()}
    pclean = prepare(a_raw)
    p64 = kc.prepare_ref(a_raw.double(), c["pad"], tgt, 1.0, kc.f32(1e-5), True, 75, T)
    rep.require(tag, "prepare: a_clip / feat_len differ from fp64", torch.equal(pclean["a_clip"], p64["a_clip"].float()) and torch.equal(pclean["feat_len"], p64["feat_len"]))
    rep.yard(tag, "prepare: alpha vs fp64", pclean["alpha"], p64["alpha"], kc.prepare_ref(a_raw, c["pad"], tgt, 1.0, kc.f32(1e-5), True, 75, T)["alpha"], (1,))
    for what, pat in POISONS:
        with pc.poisoned_empty():
            got = prepare(_poison(a_raw, c["pad"], pat))
        _same(rep, tag, f"prepare: {what} in alpha_raw of the padded frames", got, pclean)
        rep.require(tag, f"prepare, {what}: alpha of a padded frame is not exactly zero", bool((got["alpha"][c["pad"]] == 0).all()))
    # planted, one per mask: a frame IN FRONT of the length, the slot AT the count, a live frame of alpha_raw
    b = 2                                                          # lens 37, count 3
    one = torch.zeros_like(xmask)
    one[b, pc.CIF_LENS[b] - 1] = True
    rep.require(tag, "planted NaN in x of the last valid frame changed nothing",
                _changed(tag, "x[b, len - 1]", _cif_valid(c, _cif_run(c, pc.plant(c["x"], one), c["alpha"], c["csum"], g)), clean, ["out", "pa"]))
    at = torch.zeros_like(gmask)
    at[b, int(c["last"][b])] = True
    rep.require(tag, "planted NaN in g AT the count changed nothing (the slot the left-over weight lands in is read)",
                _changed(tag, "g[b, count]", _cif_valid(c, _cif_run(c, c["x"], c["alpha"], c["csum"], pc.plant(g, at))), clean, ["dx"]))
    # sc_cif_prepare_bwd on its own: pa of the frames t >= len holds any bits (pb there is an operand: the backward writes 0, no fire)
    dargs = lambda pa: (pa.to(DEV), raw["pb"].to(DEV), c["a_clip"].to(DEV), c["pad"].to(DEV), c["ratio"].to(DEV), c["quantity"].to(DEV), c["gq"].to(DEV), True)
    pmask = c["pad"][None].expand_as(raw["pa"]).contiguous()
    assert bool((raw["pb"][pmask] == 0).all())
    for what, pat in POISONS:
        with pc.poisoned_empty():
            got = {"da": ops.cif_prepare_bwd(*dargs(_poison(raw["pa"], pmask, pat))).cpu()}
        _same(rep, tag, f"prepare_bwd: {what} in pa of the frames t >= len", got, {"da": raw["da"]})
    vp = torch.zeros_like(pmask)
    vp[0, b, pc.CIF_LENS[b] - 1] = True
    rep.require(tag, "planted NaN in pa of the last valid frame changed nothing",
                _changed(tag, "pa[0, b, len - 1]", {"da": ops.cif_prepare_bwd(*dargs(pc.plant(raw["pa"], vp))).cpu()}, {"da": raw["da"]}, ["da"]))
    live = torch.zeros_like(c["pad"])
    live[b, pc.CIF_LENS[b] - 1] = True
    rep.require(tag, "planted value in alpha_raw of the last valid frame changed nothing", _changed(tag, "alpha_raw[b, len - 1]", prepare(pc.plant(a_raw, live, 0.5)), pclean, ["alpha"]))
    rep.done()


# ================================================================================================================== (a) masked keys
def _softmax_run(scores, mask, dP, p):
    ops = _ops()
    H, T, n = pc.KEY_H, pc.KEY_T, pc.KEY_N
    B = mask.shape[0]
    for name, (last, numel) in pc.key_read_extent(B, H, n, 8, 8, T + 1, pc.KEY_D).items():
        assert last < numel, name
    sd, md = scores.contiguous().to(DEV), mask.to(torch.uint8).contiguous().to(DEV)
    assert tuple(sd.shape) == (B * H * T, n) and tuple(md.shape) == (B, n)
    P, Pd = ops.softmax_fwd(sd, md, H * T, 0.125, p, kc.SOFTMAX_SEED)
    dS = ops.softmax_bwd(dP.contiguous().to(DEV), P, 0.125, p, kc.SOFTMAX_SEED)
    torch.cuda.synchronize()
    return {"P": P.cpu(), "Pd": Pd.cpu(), "dS": dS.cpu()}


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_row_softmax_ignores_masked_keys(p):
    """sc_softmax_fwd / sc_softmax_bwd, D = 256 (head_dim 128, scale 0.125 is the test's own), H = 2, T = 70 queries, n = 72 keys,
    lengths 70 / 1 / 37: the scores of masked keys and dP of masked keys (what the GEMM in front forms from the V row of a pad frame)
    hold any bits -> P and dS of masked keys are exactly 0, the live keys carry the clean run's bits.  (Before this round the backward
    formed 0 x dP: with dropout, dP / (1 - p) of a large finite value overflowed to Inf and the whole row's dS became NaN.)"""
    H, T, n, lens = pc.KEY_H, pc.KEY_T, pc.KEY_N, list(pc.KEY_LENS)
    B, rows = len(lens), len(lens) * H * T
    tag = f"softmax H={H} T={T} n={n} lens {lens} p={p}"
    rep = kc.Report()
    g = torch.Generator().manual_seed(72)
    mask = pc.key_mask(lens, n)
    mrow = mask.repeat_interleave(H * T, dim=0)
    scores = ((torch.rand(rows, n, generator=g) * 2 - 1) * 30.0) * ~mrow
    dP = torch.randn(rows, n, generator=g) * ~mrow
    clean = _softmax_run(scores, mask, dP, p)
    # the clean run against fp64 (tests/kw_cases.py)
    P64, P32 = kc.softmax_ref(scores.double(), mask, H * T, kc.f32(0.125)), kc.softmax_ref(scores, mask, H * T, kc.f32(0.125))
    e = (clean["P"].double() - P64).abs()
    e32 = kc.yard_bound(float(kc.row_errors(P32, P64, (1,)).max())) * P64.amax(-1, keepdim=True)       # the fp32 probability: yardstick rule
    bound = e32 + kc.UB * (P64 + e32)                                                                    # and its one bf16 rounding
    print(f"PARITY|{tag}|P bf16 vs fp64|{float(e.max()):.3e}|-|{float(bound.max()):.3e}")
    rep.require(tag, "P: beyond one bf16 rounding of the yardstick rule", bool((e <= bound).all()))
    keep = kc.softmax_keep(rows, n, p)
    Pb = clean["P"].float()
    rep.derived(tag, "dS", clean["dS"].float(), kc.softmax_bwd_formula(dP.double(), Pb.double(), kc.f32(0.125), keep, p),
                kc.softmax_bwd_bound(dP, Pb, kc.f32(0.125), keep, p), (1,))
    for what, pat in POISONS:
        with pc.poisoned_empty():
            got = _softmax_run(_poison(scores, mrow, pat), mask, _poison(dP, mrow, pat), p)
        _same(rep, tag, f"{what} in the scores and dP of masked keys", {k: v[~mrow] for k, v in got.items()}, {k: v[~mrow] for k, v in clean.items()})
        for k in ("P", "Pd", "dS"):
            rep.require(tag, f"{what}: {k} of a masked key is not exactly zero", bool((got[k][mrow] == 0).all()))
    one = torch.zeros_like(mrow)
    one[2 * H * T + 3, pc.KEY_LENS[2] - 1] = True                  # the last live key of a row of the 37-key utterance
    rep.require(tag, "planted NaN in a live score changed nothing", _changed(tag, "scores[row, len - 1]", _softmax_run(pc.plant(scores, one), mask, dP, p), clean, ["P"]))
    rep.require(tag, "planted NaN in dP of a live key changed nothing", _changed(tag, "dP[row, len - 1]", _softmax_run(scores, mask, pc.plant(dP, one), p), clean, ["dS"]))
    flipped = mask.clone()
    flipped[2, pc.KEY_LENS[2] - 1] = True                          # the key mask itself: the last live key of that utterance masked
    rep.require(tag, "masking one more key changed nothing", _changed(tag, "key_mask[b, len - 1]", _softmax_run(scores, flipped, dP, p), clean, ["P", "dS"]))
    rep.done()


def _pool_run(case, X, mult):
    ops = _ops()
    Xd = X.to(torch.bfloat16).to(DEV)
    a, c, crow, flen = (case[k].to(DEV) for k in ("a", "c", "crow", "flen"))
    md = mult.to(DEV)
    p, m, psum = ops.kw_pool_fwd(Xd, a, c, crow, flen, case["row0"], md, want_psum=True)
    dX, da, dc = ops.kw_pool_bwd(Xd, a, crow, flen, case["row0"], p, case["dm"].to(DEV), md, case["cbias"].to(DEV))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in (("p", p), ("m", m), ("psum", psum), ("dX", dX), ("da", da), ("dc", dc))}


def test_constant_query_pool_ignores_rows_outside_the_frames():
    """sc_kw_pool_fwd / sc_kw_pool_bwd, D = 256, 8 queries, T = 70 frames behind one CLS slot, lengths 70 / 1 / 37 (and 0: the
    constant keys alone): X outside [row0, row0 + flen) - the CLS slot included - and the multiplier's entries of those keys hold any
    bits; the score and partial buffers of the call come from torch.empty = NaN.  p of those keys and dX of those rows: exactly 0."""
    case = dict(kp.pool_case(pc.KEY_D, 8, 8, pc.KEY_T + 1, 1))
    case["flen"] = torch.tensor(list(pc.KEY_LENS) + [0], dtype=torch.int32)
    B, R, C = case["B"], case["R"], case["C"]
    tag = f"kw_pool D={pc.KEY_D} Q=8 R={R} flen {case['flen'].tolist()}"
    rep = kc.Report()
    out_rows = pc.pool_frames_mask(case["flen"], R, case["row0"])
    assert torch.equal(~out_rows, kp.valid_mask(case)[:, C:])
    xmask = pc.row_mask(out_rows.reshape(-1), pc.KEY_D).view(B, R, pc.KEY_D)
    kmask = torch.cat([torch.zeros(B, C, dtype=torch.bool), out_rows], 1)[:, None].expand(B, 8, C + R).contiguous()
    X0 = case["X"] * ~xmask
    m0 = case["mult"] * ~kmask
    clean = _pool_run(case, X0, m0)
    fails = kp.check(tag, clean, kp.pool_ref(case, case["mult"], case["cbias"]), {}, [])
    rep.require(tag, f"the clean run misses the fp64 criterion: {fails}", not fails)
    for what, pat in POISONS:
        with pc.poisoned_empty():
            got = _pool_run(case, _poison(X0.to(torch.bfloat16), xmask, pat).float(), _poison(m0, kmask, pat))
        _same(rep, tag, f"{what} in X outside the frames and in the multiplier of those keys, torch.empty = NaN", got, clean)
        rep.require(tag, f"{what}: p of a key outside the frames is not exactly zero", bool((got["p"][kmask] == 0).all()))
        rep.require(tag, f"{what}: dX of a row outside the frames is not exactly zero", bool((got["dX"][xmask] == 0).all()))
    one = torch.zeros_like(xmask)
    one[2, case["row0"] + pc.KEY_LENS[2] - 1, 5] = True            # the last frame of the 37-frame utterance
    rep.require(tag, "planted NaN in the last frame changed nothing", _changed(tag, "X[b, row0 + flen - 1]", _pool_run(case, pc.plant(X0, one), m0), clean, ["p", "m"]))
    mone = torch.zeros_like(kmask)
    mone[2, 0, C + case["row0"] + pc.KEY_LENS[2] - 1] = True       # the multiplier of that frame's key, query 0
    rep.require(tag, "planted NaN in the multiplier of a live key changed nothing", _changed(tag, "mult[b, 0, last frame]", _pool_run(case, X0, pc.plant(m0, mone)), clean, ["m", "psum"]))
    rep.done()


# ================================================================================================================== (a) prompt
def _prompt_run(kw, count, tok, pos, dX, Bp):
    ops = _ops()
    B, N, W = kw.shape
    SEG, n_pos = pc.PROMPT_SEG, pc.PROMPT_NPOS
    for name, (last, numel) in pc.prompt_read_extent(B, Bp, N, W, SEG, n_pos, count.tolist()).items():
        assert last < numel, name
    cd = count.to(DEV)
    X, eot = ops.prompt_assemble(kw.contiguous().to(DEV), cd, tok.to(DEV), pos.to(DEV), Bp, SEG, n_pos)
    dk = ops.prompt_assemble_bwd(dX.contiguous().to(DEV), cd, B, N, SEG, n_pos)
    torch.cuda.synchronize()
    return {"X": X.cpu().view(Bp, SEG, W), "eot": eot.cpu(), "dk": dk.cpu()}


def test_prompt_ignores_keyword_rows_behind_the_count():
    """sc_prompt_assemble / sc_prompt_assemble_bwd: keyword rows j >= count[b] hold any bits (prompt.hip:36 reads t - 1 < count only),
    so do the rows of dX the backward does not gather (prompt.hip:104: j + 1 >= count + 1) -> the prompt rows up to EOT carry the
    clean run's bits and equal bf16(e + pos) exactly, rows behind n_pos and pad samples are exactly zero, dk behind the count is zero."""
    N, W, SEG, n_pos, counts = pc.PROMPT_N, pc.PROMPT_W, pc.PROMPT_SEG, pc.PROMPT_NPOS, list(pc.PROMPT_COUNTS)
    B, Bp = len(counts), len(counts) + 1
    tag = f"prompt N={N} W={W} SEG={SEG} n_pos={n_pos} counts {counts}"
    rep = kc.Report()
    g = torch.Generator().manual_seed(16)
    count = torch.tensor(counts)
    behind = pc.prompt_mask(counts, N)
    kmask = pc.row_mask(behind.reshape(-1), W).view(B, N, W)
    kw = torch.randn(B, N, W, generator=g) * ~kmask
    tok, pos = torch.randn(3, W, generator=g), torch.randn(n_pos, W, generator=g)
    # dX rows the backward gathers: b SEG + j + 1, j < count
    dmask = torch.ones(Bp, SEG, dtype=torch.bool)
    for b, n in enumerate(counts):
        dmask[b, 1: 1 + min(n, n_pos - 1)] = False
    dmask = pc.row_mask(dmask.reshape(-1), W)
    dX = (torch.randn(Bp * SEG, W, generator=g) * ~dmask).to(torch.bfloat16)
    clean = _prompt_run(kw, count, tok, pos, dX, Bp)
    # the clean run against its exact statement
    want = torch.zeros(Bp, SEG, W)
    for b, n in enumerate(counts):
        e = torch.cat([tok[:1], kw[b, :n], tok[1:2], tok[2:3].expand(n_pos - n - 2, W)])[:n_pos]
        want[b, :n_pos] = e + pos
    rep.require(tag, "X is not bf16(e + pos) / zero behind n_pos and in pad samples", pc.bits_equal(clean["X"], want.to(torch.bfloat16)))
    rep.require(tag, "eot_row", clean["eot"].tolist() == [b * SEG + n + 1 for b, n in enumerate(counts)])
    wdk = torch.zeros(B, N, W)
    for b, n in enumerate(counts):
        wdk[b, :n] = dX.view(Bp, SEG, W)[b, 1: 1 + n].float()
    rep.require(tag, "dk is not the gathered rows / zero behind the count", pc.bits_equal(clean["dk"], wdk))
    for what, pat in POISONS:
        with pc.poisoned_empty():
            got = _prompt_run(_poison(kw, kmask, pat), count, tok, pos, _poison(dX, dmask, pat), Bp)
        _same(rep, tag, f"{what} in the keyword rows behind the count and in the rows of dX that are not gathered", got, clean)
        rep.require(tag, f"{what}: rows behind n_pos are not exactly zero", bool((got["X"][:, n_pos:] == 0).all()) and bool((got["X"][B:] == 0).all()))
        rep.require(tag, f"{what}: dk behind the count is not exactly zero", bool((got["dk"][kmask] == 0).all()))
    one = torch.zeros_like(kmask)
    one[2, counts[2] - 1, 0] = True                                # the last keyword in front of the count
    rep.require(tag, "planted NaN in the last keyword in front of the count changed nothing",
                _changed(tag, "keywords[b, count - 1]", _prompt_run(pc.plant(kw, one), count, tok, pos, dX, Bp), clean, ["X"]))
    done = torch.zeros(Bp * SEG, W, dtype=torch.bool)
    done[2 * SEG + counts[2], 0] = True                            # the last row of dX the backward gathers for that sample
    rep.require(tag, "planted NaN in a gathered row of dX changed nothing",
                _changed(tag, "dX[b SEG + count]", _prompt_run(kw, count, tok, pos, pc.plant(dX.float(), done).to(torch.bfloat16), Bp), clean, ["dk"]))
    rep.done()


# ================================================================================================================== (b), (c) the recipes
KW_MODELS = ("cascaded+ base", "hybrid+ large", "cascaded base")
SHORT = 320                     # samples: one valid frame
LENS_B = [20880, 6100, SHORT, 9000]          # 65 frames (1 above a multiple of 64), 18, 1, 27 -> keyword targets 3, 1, 0, 1
LENS_A = [40000, 33000, 26000, 30000]        # 124, 102, 81, 93 frames -> targets 6, 5, 4, 5: every cached buffer larger and fuller


def _build(kind, soft=False):
    """the recipe at reduced depth (HuBERT 2 / 1 / 1 layers, CLIP text tower 2 / 1 / 1 layers), max_audio_len = -1, dropout off;
    ``soft``: the quantiser in soft mode with a learnable temperature"""
    from speechclip_plus_amd import (KWClip_GeneralTransformer, cascaded_base_config, cascaded_plus_base_config, hybrid_plus_large_config,
                                     random_hubert_state_dict, set_dropout)
    from speechclip_plus_amd.speech_encoder import ARCHS
    large = kind.startswith("hybrid")
    layers = 2 if kind.startswith("cascaded+") else 1
    arch = dataclasses.replace(ARCHS["hubert_large_ll60k" if large else "hubert"], layers=layers)
    sd = random_hubert_state_dict(arch, seed=29)
    torch.manual_seed(29)
    cfg = {"cascaded+ base": cascaded_plus_base_config, "hybrid+ large": hybrid_plus_large_config, "cascaded base": cascaded_base_config}[kind]()
    cfg.audio_encoder.max_audio_len = -1
    cfg.clip.layers = layers
    if soft:
        cfg.model_settings.cascaded_branch.vq.args = {"temp": "learnable=0.1", "time_first": True, "use_gumbel": False, "hard": False}
    model = set_dropout(KWClip_GeneralTransformer(cfg, device="cuda:0", hubert_state_dict=sd, hubert_arch=arch), False)
    with torch.no_grad():
        model.audio_encoder.weightedsum_layer.weights.copy_(torch.tensor([0.3, -0.2, 0.5][: layers + 1]))
        if hasattr(model.cascaded_branch, "downsampling"):
            model.cascaded_branch.downsampling.weight_proj[1].bias.add_(-0.5)
    return model


def _batch(kind, lens, seed):
    g = torch.Generator().manual_seed(seed)
    B, E = len(lens), 768 if kind.startswith("hybrid") else 512
    wav = torch.zeros(B, max(lens))
    for b, l in enumerate(lens):
        wav[b, :l] = torch.randn(l, generator=g) * 0.5
    return {"wav": wav.cuda(), "wav_len": torch.tensor(lens), "image": torch.randn(B, E, generator=g).cuda(), "id": torch.tensor([0, 1, 1, 2][:B]).cuda()}


def _valid_slots(t, lens):
    """[B, N, ...] -> the slots in front of lens[b] (None: a fixed count, every slot)"""
    if lens is None:
        return t
    keep = torch.arange(t.shape[1])[None] < lens.cpu()[:, None]
    return t[keep]


def _forward_paths(model, batch):
    """encode_speech, model(batch), extract_keywords, detokenize_keywords and the neighbour path at a chunk of 128 rows over more
    than 128 keyword rows (the score and split buffers are reused) -> dict of CPU tensors: what the mathematics defines"""
    from speechclip_plus_amd.keyword_neighbors import keyword_neighbors
    lens = batch["wav_len"].tolist()
    wavs = [batch["wav"][b, :l] for b, l in enumerate(lens)]
    res = {}
    with torch.no_grad():
        es = model.encode_speech(wavs)
        _, _, o = model(batch)
        ek = model.extract_keywords(wavs)
        kl = o["keywords_len"]
        if kl is not None:
            assert torch.equal(kl.cpu(), ek["dsample_results"]["dsample_feats_length"].cpu())
            res["keywords_len"] = kl.cpu()
        for src, d in (("encode_speech", es), ("forward", o)):
            for k in ("cascaded_audio_feat", "parallel_audio_feat"):
                if d[k] is not None:
                    res[f"{src} {k}"] = d[k].float().cpu()
            res[f"{src} keywords"] = _valid_slots(d["keywords"].float().cpu(), kl)
            res[f"{src} token ids"] = _valid_slots(d["vq_results"]["targets"].reshape(d["keywords"].shape[:2]).cpu(), kl)
        N = o["keywords"].shape[1]
        res["extract_keywords token ids"] = _valid_slots(torch.tensor(ek["vq_results"]["targets"]).view(len(lens), N), kl)
        entries = model.detokenize_keywords([o], K=5)
        flat = [[float(v) for pair in e["neighbors"][k] for v in pair] for e in entries for k in sorted(e["neighbors"])]
        res["detokenize_keywords"] = torch.tensor(flat, dtype=torch.float64)
        rows = int(kl.sum()) if kl is not None else len(lens) * N
        reps = 1 + 200 // max(rows, 1)
        vals, idx = keyword_neighbors(o["keywords"].repeat(reps, 1, 1), model.clip.model.token_embedding.weight, 5,
                                      None if kl is None else kl.repeat(reps), chunk_rows=128)
        assert rows * reps > 128, "the chunk buffers are reused at least once"
        res["neighbours, chunks of 128: values"], res["neighbours, chunks of 128: ids"] = vals.cpu(), idx.cpu()
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("kind", KW_MODELS)
def test_keyword_forward_paths_do_not_depend_on_uninitialised_memory(kind):
    """eval mode, four utterances (one of a single valid frame, one of 65 frames): a normal run, a run with torch.empty = NaN on the warm
    module, and the FIRST run of a fresh module of the same seed under torch.empty = NaN (every cache and derived table built there)"""
    model, batch = _build(kind).eval(), _batch(kind, LENS_B, 41)
    with torch.no_grad():
        fl = model.forward_audio(batch["wav"], batch["wav_len"])[1].tolist()
    assert 1 in fl and any(n % 64 == 1 and n > 1 for n in fl), fl
    clean = _forward_paths(model, batch)
    assert all(bool(torch.isfinite(v).all()) for k, v in clean.items() if v.is_floating_point() and "neighbours" not in k)
    rep = kc.Report()
    with pc.poisoned_empty():
        warm = _forward_paths(model, batch)
    _same(rep, f"forward paths {kind}", "torch.empty = NaN, warm module", warm, clean)
    del model
    with pc.poisoned_empty():
        first = _forward_paths(_build(kind).eval(), batch)
    _same(rep, f"forward paths {kind}", "torch.empty = NaN, first run of a fresh module", first, clean)
    rep.done()


def _step(model, batch):
    """model(batch), compute_loss, backward -> {"loss": ..., parameter name: grad} on the CPU.  The dropout masks are functions of
    torch's seed and of three call counters: all three are put back before every step."""
    from speechclip_plus_amd import mha_block, ops
    model.zero_grad(set_to_none=True)
    torch.manual_seed(31)
    model.audio_encoder._drop_calls = 0
    ops._mult_calls[0] = 0
    mha_block._calls = 0
    loss = model.compute_loss(model(batch)[0])["loss"]
    loss.backward()
    torch.cuda.synchronize()
    res = {"loss": loss.detach().float().cpu().reshape(1)}
    res.update({n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None})
    model.zero_grad(set_to_none=True)
    return res


# leg -> (recipe, the branch's dropout on, the quantiser soft with a learnable temperature)
TRAIN_LEGS = {"cascaded+ base": ("cascaded+ base", False, False), "hybrid+ large": ("hybrid+ large", False, False),
              "cascaded base": ("cascaded base", False, False), "cascaded+ base, branch dropout": ("cascaded+ base", True, False),
              "cascaded+ base, soft quantiser, learnable temperature": ("cascaded+ base", False, True)}
# the parameters of the branch that must be among the compared gradients, by a fragment of their names
BRANCH_PARAMS = {"cascaded+ base": ("downsampling.conv", "linear_proj", "bn_layer", "self_att", "criterion.temperature"),
                 "hybrid+ large": ("downsampling.conv", "linear_proj", "bn_layer", "self_att", "cascaded_branch.cls", "criterion.temperature"),
                 # cascaded base: spchclp_c.yaml fixes the temperature (temperature_trainable: false) - no such parameter; asserted below
                 "cascaded base": ("linear_proj", "bn_layer", "self_att", "cascaded_branch.cls")}


@pytest.mark.parametrize("leg", list(TRAIN_LEGS))
def test_keyword_train_step_does_not_depend_on_unwritten_memory_or_history(leg):
    """loss and every p.grad of one train step, bit for bit: a second clean step (the precondition), torch.empty = NaN on the warm
    model, the step after a step on a batch A with MORE keywords and longer utterances, the second step after A, and the first step of
    a fresh model under torch.empty = NaN.  Nothing is excluded from the bit comparison."""
    from speechclip_plus_amd import set_dropout
    kind, dropout, soft = TRAIN_LEGS[leg]

    def build():
        m = _build(kind, soft).train()
        if dropout:
            set_dropout(m.cascaded_branch, True)
        return m
    model = build()
    B, A = _batch(kind, LENS_B, 41), _batch(kind, LENS_A, 42)
    clean = _step(model, B)
    assert all(bool(torch.isfinite(t.float()).all()) for t in clean.values()), [n for n, t in clean.items() if not bool(torch.isfinite(t.float()).all())]
    want = BRANCH_PARAMS[kind] + (("vector_quantizer.curr_temp",) if soft else ())
    assert bool(model.criterion.temperature_trainable) == ("criterion.temperature" in want), "a trainable temperature is among the compared gradients"
    for frag in want:
        hit = [n for n in clean if frag in n and float(clean[n].float().abs().max()) > 0]
        assert hit, f"no parameter named *{frag}* has a non-zero gradient among {sorted(clean)}"
    rep = kc.Report()
    tag = f"train step {leg}"
    _same(rep, tag, "a second clean step", _step(model, B), clean)
    with pc.poisoned_empty():
        warm = _step(model, B)
    _same(rep, tag, "torch.empty = NaN, warm model", warm, clean)
    other = _step(model, A)
    assert all(bool(torch.isfinite(t.float()).all()) for t in other.values())
    for what in ("the step after a step on a larger batch", "the second step after a step on a larger batch"):
        _same(rep, tag, what, _step(model, B), clean)
    del model
    with pc.poisoned_empty():
        first = _step(build(), B)
    _same(rep, tag, "torch.empty = NaN, first step of a fresh model", first, clean)
    rep.done()


# ================================================================================================================== (d) criteria and rings
LOSS_SHAPE = (130, 100, 1000, 40)          # 130 x 100 features: 3 x 3 tiles of 64 (SupConLoss: 260 contrast rows, 5 x 5 tiles); 1000 extras


def _criterion_run(name):
    import neg_loss_cases as nc
    import queue_loss_cases as qc
    from speechclip_plus_amd.losses import MaskedContrastiveLoss, SigmoidContrastiveLoss, SupConLoss
    c = (nc if name == "masked, bank" else qc).make_case(*LOSS_SHAPE)
    to = lambda k: c[k].to(DEV)
    a, b, ids = to("A").requires_grad_(True), to("B").requires_grad_(True), to("ids")
    if name.startswith("masked"):
        crit = MaskedContrastiveLoss(temperature=0.07, temperature_trainable=True).to(DEV)
        extra = {"masked, plain": {}, "masked, bank": lambda: dict(bank=to("bank"), bank_ids=to("bank_ids"), neg_idx=to("neg_idx")),
                 "masked, queue": lambda: dict(queue_A=to("queue_A"), queue_B=to("queue_B"), queue_ids=to("queue_ids"))}[name]
        loss = crit(a, b, ids, **(extra() if callable(extra) else extra))
    elif name == "supcon":
        crit = SupConLoss().to(DEV)
        loss = crit(feat_A=a, feat_B=b, index=ids)
    else:
        crit = SigmoidContrastiveLoss().to(DEV)
        loss = crit(a, b, ids)
    loss.backward()
    torch.cuda.synchronize()
    res = {"loss": loss.detach().cpu().reshape(1), "dA": a.grad.cpu(), "dB": b.grad.cpu()}
    res.update({f"d {n}": p.grad.detach().cpu().reshape(-1) for n, p in crit.named_parameters()})
    return res


@pytest.mark.parametrize("name", ["masked, plain", "masked, bank", "masked, queue", "supcon", "sigmoid"])
def test_criteria_do_not_depend_on_uninitialised_memory(name):
    clean = _criterion_run(name)
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in clean.values()), clean.keys()
    assert len(clean) >= 4, "the scalar gradients are among the compared results"
    rep = kc.Report()
    with pc.poisoned_empty():
        got = _criterion_run(name)
    _same(rep, f"criterion {name} {LOSS_SHAPE[0]} x {LOSS_SHAPE[1]}", "torch.empty = NaN", got, clean)
    rep.done()


def _ring_sequence(poisoned):
    """a bare model (compute_loss reads config, criterion and the rings only), set_negative_queue(300), four train-mode compute_loss
    calls of 130 rows each - 0, 130, 260 queued rows, then the wrap - and one call with a negative bank instead.  ``poisoned``: every
    ring row holds NaN until a batch is written there (the rings are allocated as zeros: the rows beyond n_valid are given the NaN
    here), under torch.empty = NaN from the first call on."""
    import contextlib
    import neg_loss_cases as nc
    import queue_loss_cases as qc
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    res = {}
    with (pc.poisoned_empty() if poisoned else contextlib.nullcontext()):
        model = KWClip_GeneralTransformer.__new__(KWClip_GeneralTransformer)
        torch.nn.Module.__init__(model)
        model.config = base_parallel_config()
        model.criterion = MaskedContrastiveLoss(**model.config.cl_loss.args).to(DEV)
        model._device, model.subword_embd_dim = torch.device("cuda:0"), 100
        model.train()
        model.set_negative_queue(300)
        q = model._neg_queue
        if poisoned:
            for ring in (q["image"], q["speech"]["parallel"]):
                ring.fill_(float("nan"))
        for i in range(4):
            c = qc.make_case(130, 100, 0, 40, seed=1 + i % 2)
            a = c["A"].to(DEV).requires_grad_(True)
            loss = model.compute_loss({"id": c["ids"].to(DEV), "image_feat": c["B"].to(DEV), "parallel_audio_feat": a})["loss"]
            loss.backward()
            res[f"queue call {i}: loss"], res[f"queue call {i}: dA"] = loss.detach().cpu().reshape(1), a.grad.cpu()
            res[f"queue call {i}: head, n_valid"] = torch.tensor([q["head"], q["n_valid"]])
        res["rings once full"] = torch.cat([q["image"], q["speech"]["parallel"]]).cpu()
        model.clear_negative_queue()
        c = nc.make_case(*LOSS_SHAPE)
        model.set_negative_bank(c["bank"].to(DEV) * 3.0, c["bank_ids"].to(DEV), 32)
        a = c["A"].to(DEV).requires_grad_(True)
        loss = model.compute_loss({"id": c["ids"].to(DEV), "image_feat": c["B"].to(DEV), "parallel_audio_feat": a})["loss"]
        loss.backward()
        res["bank: loss"], res["bank: dA"] = loss.detach().cpu().reshape(1), a.grad.cpu()
        torch.cuda.synchronize()
    return res


def test_model_queue_and_bank_do_not_depend_on_ring_rows_nobody_wrote():
    clean, got = _ring_sequence(False), _ring_sequence(True)
    assert [clean[f"queue call {i}: head, n_valid"].tolist() for i in range(4)] == [[0, 0], [130, 130], [260, 260], [90, 300]]
    assert float(clean["queue call 1: loss"]) != float(clean["queue call 3: loss"]), "the queue changes the loss"
    rep = kc.Report()
    _same(rep, "model queue(300) x 4 calls + bank", "ring rows beyond n_valid = NaN, torch.empty = NaN from the first call on", got, clean)
    for k, v in got.items():
        rep.require("model queue / bank", f"{k} is not finite", bool(torch.isfinite(v.double()).all()))
    rep.done()
