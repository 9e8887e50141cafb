"""Properties of the builders, references and criteria in tests/head_cases.py that tests/test_gpu_parallel_head.py relies on: no GPU
needed.  The fp32 yardstick meets every derived bound against fp64 (and a derived sanity bound where the device is held to 4 x the
yardstick), the cases have the coverage and the numerical range the GPU tests assume, and each per-row criterion rejects a one-row
error that a whole-tensor rel-L2 at the former 1e-4 lets through."""
import pytest
import torch

import head_cases as hc

OLD_REL_L2 = 1e-4


def _pool(D, H, R, train_p=None):
    c = hc.train_case(D, H, R, train_p) if train_p else hc.pool_case(D, H, R)
    mult, cbias = (c["mult"], c["cbias"]) if train_p else (None, None)
    ref, inp = hc.pool_reference(c, mult, cbias)
    return c, ref, inp, hc.pool_yardstick(c, inp, mult, cbias), hc.pool_bounds(c, inp, mult, cbias), mult, cbias


def test_sweep_covers_every_template_instance_and_tail():
    sweep = hc.POOL_SWEEP
    assert {hc.nch(D) for D, _, _ in sweep} == {1, 2, 3, 4}
    assert {H for D, H, _ in sweep if D % 64 == 0} == {1, 2, 4, 8, 16}                 # NH of the pool kernels; 16 = two score passes
    assert any(R < 16 for _, _, R in sweep)
    assert any(R % 8 and R % 16 and R % 32 and R % 64 for _, _, R in sweep)
    assert any(R % 64 and (R % 64) % 4 for _, _, R in sweep)                            # a clamped row inside a wave's group of 4
    assert all(D % 64 == 0 for D, _, _ in sweep)             # 320 = 5 x 64 included: every case runs all three kernels
    for _, _, R in sweep:
        lens = hc.pool_lengths(R)
        assert lens[0] == R and lens[1] == 1 and lens[2] % 32 and 1 <= lens[2] <= R and lens[3] == R // 2 + 1
    assert set(hc.TRAIN_CASES) <= set(sweep)
    assert hc.pool_lds_limits(8) == (1792, 896) and hc.pool_lds_limits(16) == (768, 384) and hc.pool_lds_limits(1) == (16128, 8064)
    assert sorted({D // H for _, D, H in hc.VALUE_BIAS_CASES}) == [64, 96, 128, 768]
    assert any(D > 256 for _, D, _ in hc.VALUE_BIAS_CASES) and any(B > 64 for B, _, _ in hc.VALUE_BIAS_CASES)


@pytest.mark.parametrize("D,H,R", hc.POOL_SWEEP)
def test_pool_cases_are_well_conditioned(D, H, R):
    """Every (b, h) row has a live key; the softmax arguments stay where fp32 exp neither overflows nor flushes (|s - max| < 80:
    exp(-87.3) is the smallest normal); X holds bf16 values and zeros past the length."""
    c = hc.pool_case(D, H, R)
    live = hc.live_mask(c["lens"], R)
    assert bool(live.any(-1).all()) and int(live.sum()) == sum(hc.pool_lengths(R))
    assert torch.equal(c["X"].to(torch.bfloat16).float(), c["X"]) and float(c["X"][~live].abs().max() if (~live).any() else 0) == 0
    s = hc.scores_ref(c["X"].double(), c["a"].double()).masked_fill(~live[:, None, :], float("-inf"))
    span = (s.amax(-1, keepdim=True) - s)[live[:, None, :].expand_as(s)]
    assert float(span.max()) < 80 and float(s[live[:, None, :].expand_as(s)].abs().max()) < 80
    assert float(hc.weight_eps(s, c["lens"]).max()) < 128 * hc.U          # the exp term of the m bound stays at the 1e-5 level


@pytest.mark.parametrize("p", hc.TRAIN_P)
@pytest.mark.parametrize("D,H,R", hc.TRAIN_CASES)
def test_dropout_patterns(D, H, R, p):
    """Multipliers are 0 or 1 / (1 - p), keep 50 % .. 95 % of the live weights and at least one per row; dm and cbias are the value
    path's Wv_h^T dctx_h and dctx_h . bv_h."""
    c = hc.train_case(D, H, R, p)
    mult = c["mult"]
    live = hc.live_mask(c["lens"], R)[:, None, :].expand_as(mult)
    vals = mult.unique().tolist()
    assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] * (1.0 - p) - 1.0) < 1e-6
    frac = float(((mult > 0) & live).sum()) / float(live.sum())
    assert 0.5 <= frac <= 0.95, frac
    assert bool(((mult > 0) & live).any(-1).all())
    dh = D // H
    dm = torch.einsum("bhj,hjk->bhk", c["dctx"].double().view(-1, H, dh), c["Wv"].double().view(H, dh, D))
    assert float((c["dm"].double() - dm).abs().max()) <= hc.U * float(dm.abs().max())
    assert torch.equal(c["mult"], hc.train_case(D, H, R, p)["mult"])


@pytest.mark.parametrize("D,H,R,train_p", [s + (None,) for s in hc.POOL_SWEEP] + [s + (p,) for s in hc.TRAIN_CASES for p in hc.TRAIN_P])
def test_pool_yardstick_is_within_the_derived_bounds(D, H, R, train_p):
    c, ref, inp, yard, bounds, mult, cbias = _pool(D, H, R, train_p)
    rep = hc.Report()
    name = f"cpu D={D} H={H} R={R} p={train_p}"
    hc.pool_checks(rep, name, c, yard, ref, yard, bounds, mult)
    if "dX" in yard:                                         # held to 4 x the yardstick on the device: the yardstick itself is sane
        rep.derived(name, "dX (yardstick sanity)", yard["dX"], ref["dX"], bounds["dX"], hc.POOL_DIMS["dX"])
        e = hc.weight_eps(inp["scores"], c["lens"])
        rep.derived(name, "p (yardstick sanity)", yard["p"], ref["p"], e[..., None] * ref["p"], hc.POOL_DIMS["p"])
        # the hand-written backward formula and autograd agree in fp64 (the formula is the yardstick's, autograd the reference's)
        auto = hc.pool_autograd(c["X"], c["a"], c["dm"], c["lens"], mult, cbias)
        b64 = hc.pool_bwd_ref(c["X"].double(), auto["p"], auto["dp"], c["dm"].double(), c["a"].double(), c["lens"], mult,
                              cbias.double() if cbias is not None else None)
        assert hc.rel_l2(b64["dX"], auto["dX"]) < 1e-13 and hc.rel_l2(b64["da_part"].sum(0), auto["da"]) < 1e-13
    rep.done()


def test_dx_fallback_applies_to_dropped_key_rows_only():
    """The derived bound is an alternative for the dX rows of keys that some head drops, nowhere else: without multipliers no row
    has it, and a row of kept keys moved past 4 x the yardstick fails even where its derived bound is larger."""
    c, ref, inp, yard, bounds, mult, _ = _pool(64, 1, 40, 0.1)
    rows = hc.dropped_key_rows(c, mult)
    assert bool(rows.any()) and not bool(rows.all()) and not bool(hc.dropped_key_rows(c, None).any())
    own = hc.row_bounds(bounds["dX"], ref["dX"], (2,))
    yb = hc.yard_bound(float(hc.row_errors(yard["dX"], ref["dX"], (2,)).max()))
    live = hc.live_mask(c["lens"], c["R"])
    cand = (live & ~rows & (own > 2 * yb)).nonzero()
    assert len(cand), "no kept row whose derived bound exceeds the yardstick bound"
    b, s_ = cand[0].tolist()
    bad = yard["dX"].clone().double()
    bad[b, s_] += 1.5 * yb * ref["dX"][b, s_].abs().max()
    rep = hc.Report()
    rep.yard("fallback", "dX", bad, ref["dX"], yard["dX"], (2,), bounds["dX"], rows)
    assert len(rep.bad) == 1


@pytest.mark.parametrize("q", ["p", "m", "dX", "da", "scores"])
def test_per_row_criterion_rejects_a_one_row_error(q):
    """The yardstick's result with one (b, h) or (b, s) row moved by three units of its bound fails the per-row criterion, while the
    whole-tensor rel-L2 of the former tests stays below 1e-4."""
    c, ref, inp, yard, bounds, mult, _ = _pool(768, 8, 320, 0.1)
    dims = hc.POOL_DIMS[q]
    bad = yard[q].clone().double()
    if q in hc.POOL_DERIVED:
        step = 3.0 * bounds[q]
    else:
        step = 3.0 * hc.yard_bound(float(hc.row_errors(yard[q], ref[q], dims).max())) * ref[q].abs().amax(dims, keepdim=True).expand_as(ref[q])
        if q == "dX":                                        # a dropped key's row may also meet its own derived bound
            step = torch.maximum(step, 3.0 * bounds[q].amax(dims, keepdim=True).expand_as(ref[q]))
    row = (2, 3) if q in ("p", "m") else (3,) if q == "da" else (2, slice(None), 5) if q == "scores" else (2, 7)      # b = 2: the odd length
    bad[row] += step[row]
    rep = hc.Report()
    if q in hc.POOL_DERIVED:
        rep.derived("mutation", q, bad, ref[q], bounds[q], dims)
    else:
        rep.yard("mutation", q, bad, ref[q], yard[q], dims, bounds.get(q), hc.dropped_key_rows(c, mult) if q == "dX" else None)
    assert len(rep.bad) == 1, rep.bad
    assert hc.rel_l2(bad, ref[q]) < OLD_REL_L2
    ok = hc.Report()
    (ok.derived("mutation", q, yard[q], ref[q], bounds[q], dims) if q in hc.POOL_DERIVED else ok.yard("mutation", q, yard[q], ref[q], yard[q], dims))
    assert not ok.bad


def test_row_errors_zero_rows_and_nan():
    ref = torch.tensor([[1.0, -2.0], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64)
    got = torch.tensor([[1.0, -2.5], [0.0, 0.0], [0.0, 1e-30]], dtype=torch.float64)
    assert hc.row_errors(got, ref, (1,)).tolist() == [0.25, 0.0, float("inf")]
    got[0, 0] = float("nan")
    assert hc.row_errors(got, ref, (1,))[0] == float("inf")


@pytest.mark.parametrize("B,D,H", hc.VALUE_BIAS_CASES)
def test_value_bias_yardstick(B, D, H):
    c = hc.value_bias_case(B, D, H)
    ref, yard, bounds = hc.value_bias_ref(c, torch.float64), hc.value_bias_ref(c, torch.float32), hc.value_bias_bounds(c)
    rep = hc.Report()
    rep.derived("cpu value_bias", "cbias", yard["cbias"], ref["cbias"], bounds["cbias"], ())
    v = lambda t: t.view(H, D // H)
    rep.derived("cpu value_bias", "gbv", v(yard["gbv"]), v(ref["gbv"]), v(bounds["gbv"]), (1,))
    rep.done()
    assert float(c["gbv0"].abs().min()) > 0                  # accumulation on top of non-zero contents
    moved = yard["gbv"].clone().double()
    moved[5] += 3 * bounds["gbv"].max()
    bad = hc.Report()
    bad.derived("mutation", "gbv", v(moved), v(ref["gbv"]), v(bounds["gbv"]), (1,))
    assert bad.bad and hc.rel_l2(moved, ref["gbv"]) < OLD_REL_L2


@pytest.mark.parametrize("nblk,NL", hc.SOFTMAX_REDUCE_CASES)
def test_softmax_reduce_yardstick(nblk, NL):
    part, w = hc.softmax_reduce_case(nblk, NL)
    ref = hc.softmax_reduce_ref(part.double(), w.double())
    rep = hc.Report()
    rep.derived("cpu softmax_reduce", "out", hc.softmax_reduce_ref(part, w), ref, hc.softmax_reduce_bound(part, w), (0,))
    rep.done()
    if NL == 1:
        assert float(ref.abs().max()) == 0.0                  # w = 1: d - w d, exactly zero
    else:
        assert abs(float(ref.sum())) < 1e-6 * float(ref.abs().sum())                  # a softmax backward sums to zero (w sums to 1 in fp32)


# ---------------------------------------------------------------------------------------------------------------- row tail
def _tail(B, D, F_, E):
    c = hc.tail_case(B, D, F_, E)
    ref, inp = hc.tail_reference(c, torch.float64)
    S = {"x_W1": hc.rt_slices(B, F_, D), "sliced": hc.rt_slices(B, D, F_), "ctx": hc.rt_slices(B, D // hc.TAIL_H, D, hc.TAIL_H)}
    return c, ref, inp, hc.tail_reference(c, torch.float32, inp), hc.tail_bounds(c, inp, S)


def test_tail_cases_cover_the_tiles_and_the_row_groups():
    Bs = {B for B, _, _, _ in hc.TAIL_CASES}
    assert Bs == {1, 7, 65, 130} and min(Bs) < 8 and any(64 < B <= 128 for B in Bs) and any(B > 128 for B in Bs)
    assert {(D, F_, E) for _, D, F_, E in hc.TAIL_CASES} == {(768, 3072, 512), (1024, 4096, 768)}
    for B, D, F_, E in hc.TAIL_CASES:
        for K in (D, F_):                                       # S = 8 is a legal split of both contractions: no empty slice
            assert hc.rt_kc(K, 8) * 7 < K
        assert hc.rt_slices(B, F_, D) > 1 and hc.rt_slices(B, D, F_) > 1
    assert set(hc.TAIL_DERIVED) | set(hc.TAIL_YARD) == set(_tail(1, 768, 3072, 512)[1])


@pytest.mark.parametrize("B,D,F_,E", hc.TAIL_CASES)
def test_tail_yardstick_is_within_the_derived_bounds(B, D, F_, E):
    """The derived quantities of the fp32 yardstick meet their bounds; the others (LayerNorm, GELU, unit rows) are within 64 u per
    row of fp64, the size the device is then held to 4 x of; the dropout sites keep 70 % .. 95 % and zero rows stay zero."""
    c, ref, inp, yard, bounds = _tail(B, D, F_, E)
    rep = hc.Report()
    hc.tail_checks(rep, f"cpu tail B={B} D={D}", yard, ref, yard, bounds)
    rep.done()
    for q in hc.TAIL_YARD:
        assert float(hc.row_errors(yard[q], ref[q], hc.tail_dims(q)).max()) < 64 * hc.U, q
    assert 0.7 < float(hc.keep_rows(B, F_, hc.SEED_F, hc.P_F).float().mean()) < 0.8
    assert 0.8 < float(hc.keep_rows(B, D, hc.SEED_D, hc.P_D).float().mean()) < 0.95
    assert float(c["dgam0"].abs().min()) > 0 and float(c["gb0"].abs().min()) > 0          # accumulation onto non-zero contents


@pytest.mark.parametrize("q", ["gemm_split", "gemm_sliced", "gW", "h_dm", "ln1_out", "lnb_dx", "elem2", "l2_e", "lnb_dgamma"])
def test_tail_per_row_criterion_rejects_a_one_row_error(q):
    """One element of row b (of a column sum: one element) of the yardstick moved by three units of the row's bound: the per-row
    criterion fails, the whole-tensor rel-L2 of test_rowtail_ops (1e-6 / 1e-5) or the former 1e-4 does not see it."""
    c, ref, inp, yard, bounds = _tail(130, 768, 3072, 512)
    dims = hc.tail_dims(q)
    bad = yard[q].clone().double()
    at = (77, 5) if dims else (77,)
    if q in hc.TAIL_DERIVED:
        bad[at] += 3.0 * (bounds[q][77].amax() if dims else bounds[q][77])
    else:
        bad[at] += 3.0 * hc.yard_bound(float(hc.row_errors(yard[q], ref[q], dims).max())) * ref[q][77].abs().amax()
    rep = hc.Report()
    hc.tail_checks(rep, "mutation", {q: bad}, ref, yard, bounds)
    assert len(rep.bad) == 1, rep.bad
    assert hc.rel_l2(bad, ref[q]) < OLD_REL_L2
    if q != "gemm_sliced":                     # K = 3072 in 8 slices: 3 k u = 7e-5 of sum |a b| on one element is 1.6e-5 of the tensor
        assert hc.rel_l2(bad, ref[q]) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- whole head
@pytest.mark.parametrize("train", [False, True])
def test_head_oracle_is_dtype_generic_and_the_yardstick_is_small(train):
    """oracle.parallel_branch_forward runs in fp64 and fp32 alike (head_reference asserts the output dtype); the fp32 oracle is
    within 1e-5 of fp64 in every quantity at the base width, so 4 x its error replaces the former 1e-2 / 3e-2 by three orders of
    magnitude; padded frames have an exactly zero gradient; the key part of in_proj_bias is zero up to fp64 rounding."""
    d, h, f, E = hc.HEAD_CASES[0]
    W = hc.head_weights(d, f, E)
    assert torch.equal(W["cls"], hc.bf16_values(W["cls"]))
    feat, lens, gout = hc.head_inputs(d, E)
    assert torch.equal(feat, hc.bf16_values(feat)) and lens.tolist() == [100, 37, 1] and feat.shape == (3, 100, d)
    drop = hc.head_drop_fn(*hc.head_host_masks(d, h, f)) if train else None
    ref = hc.head_reference(W, feat, lens, gout, h, drop)
    yard = hc.head_reference(W, feat, lens, gout, h, drop, dtype=torch.float32)
    rep = hc.Report()
    hc.head_checks(rep, "cpu head", yard, ref, yard)
    rep.done()
    for q in ref:
        if not q.endswith("[k]"):
            assert float(hc.row_errors(yard[q], ref[q], hc.head_dims(q, ref[q])).max()) < 1e-5, q
    dead = ~hc.live_mask(lens.to(torch.int32), hc.HEAD_T)
    assert float(ref["d_feat"][dead].abs().max()) == 0.0
    # one frame's gradient moved by three units of the bound: rejected per row, invisible to the former 3e-2
    bad = {"d_feat": yard["d_feat"].clone().double()}
    bad["d_feat"][1, 20] += 3 * hc.yard_bound(float(hc.row_errors(yard["d_feat"], ref["d_feat"], (2,)).max())) * ref["d_feat"][1, 20].abs().max()
    r2 = hc.Report()
    hc.head_checks(r2, "mutation", bad, ref, yard)
    assert len(r2.bad) == 1 and hc.rel_l2(bad["d_feat"], ref["d_feat"]) < OLD_REL_L2
