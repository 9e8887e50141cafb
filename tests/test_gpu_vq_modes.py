"""The quantiser's soft / Gumbel / learnable-temperature modes on the HIP kernels of csrc/vq.hip (under ops.vq_* and
vector_quantizers.SimpleVectorQuantizer) against the fp64 restatement of tests/vq_modes_cases.py.

Bounds, fixed before the first run (U = 2^-24; every formula is a function in vq_modes_cases.py with its derivation):
  noise         |g_dev - g| <= 4 U (1 + |g|)                                      two precise logarithms, 1 ulp = 2 U each
  row stats     |m_dev - m| <= dy,  |ls_dev - ls| <= 2 dy / tau + (ceil(V / 256) + 70) U   dy = U [4 (1 + G) + X + G] with noise, else 0
  s             |s_dev - s| <= E_s s + 2^-126                                     E_s = U [4 dy / (U tau) + ceil(V / 256) + 404];
                                                                                  below the smallest normal a value has no 24 bits
  (a fixed temperature reaches the kernels as an fp32 number: the fp64 side uses that number)
  keywords      |kw_dev - s64 . table64| <= (3 * 2^-18 + E_s + 2 U (K_eff + 3)) (s . |table|),  K_eff = 3 Vp / S + S: S serial slices
  dx            dx_bound: (2 E_s + (ceil(V / 256) + 13) U) s (|t| + <s, |t|>) / tau   (+ 2^-9 of that for the bf16 form)
  d tau         dtau_bound: the accumulation charged on sum |dz z| / tau, plus the two factors' own errors
  d kw          through quantize_keywords the chain has four bf16 operands (g, the table, dx, the normalised table): see _dkw_bound
  hard values   exactly one-hot; masked columns exactly 0; two calls the same bits.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import vq_modes_cases as vc

pytestmark = pytest.mark.gpu
U = vc.U
NEW_MODES = ((False, False), (True, True), (True, False))          # (use_gumbel, hard) beside the default (False, True)


@functools.lru_cache(maxsize=None)
def _scores(Nk, V):
    if (Nk, V) == (15, 50):
        import os
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vq_modes.npz"))
        return z["x"].reshape(15, 50).astype(np.float32)
    return (0.3 * np.random.default_rng(Nk * 31 + V).standard_normal((Nk, V))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _table(V, Et):
    return np.random.default_rng(V + Et).standard_normal((V, Et)).astype(np.float32)


def _next_seed():
    """the seed the next ops.next_mult_seed() call returns, without moving the counter"""
    from speechclip_plus_amd import ops
    c = ops._mult_calls[0]
    s = ops.next_mult_seed()
    ops._mult_calls[0] = c
    return s


def _np(t):
    return t.detach().double().cpu().numpy()


def _t32(tau):
    """the temperature as the kernels receive it: an fp32 number"""
    return float(np.float32(tau))


# ---------------------------------------------------------------------------------------------------- noise
@pytest.mark.parametrize("Nk,V", [(3, 50), (5, 777), (130, 1000)])
def test_noise_against_the_twin(Nk, V):
    from speechclip_plus_amd import ops
    for seed in (99, 0xDEADBEEF):
        g = vc.gumbel(Nk, V, seed)
        got = _np(ops.vq_gumbel(Nk, V, seed, "cuda"))
        ratio = float((np.abs(got - g) / vc.noise_bound(g)).max())
        print(f"noise ({Nk}, {V}) seed {seed:#x}: largest error / bound = {ratio:.3f}")
        assert np.isfinite(got).all() and ratio <= 1.0


# ---------------------------------------------------------------------------------------------------- noisy row statistics
def test_noisy_rowstats_on_the_margin_case():
    from speechclip_plus_amd import ops
    x, g, margin = vc.margin_case()
    xd = torch.from_numpy(x).float().cuda()
    want = vc.first_argmax(x + g)
    for tau in (0.1, 1.0):
        for noise in (True, False):
            idx, stats = ops.vq_noisy_rowstats(xd, 1000, tau, 99, noise)
            y = x + g if noise else x
            assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want if noise else vc.first_argmax(x))   # all 300
            m, ls = vc.row_statistics(y, _t32(tau))
            bm, bls = vc.rowstats_bounds(x, _t32(tau), noise, 1000)
            rm, rls = float((np.abs(_np(stats[0]) - m) / bm).max()), float((np.abs(_np(stats[1]) - ls) / bls).max())
            print(f"margin case tau {tau} noise {noise}: max error / bound {rm:.3f}, log-sum error / bound {rls:.3f}")
            assert rm <= 1.0 and rls <= 1.0
    assert not torch.isinf(xd[:, 1]).any() and torch.isinf(xd[:, 0]).all()                   # the scores are read, never written


def test_noisy_rowstats_tie_rule():
    """Equal perturbed scores: the noise keeps 23 bits of its hash word, so among the 8112 columns of a row some pairs share their g
    bit for bit (about four pairs per row).  With every other column at -inf and the same score on such a pair, x + g ties exactly:
    the lower column must win, as in sc_vq_rowstats, whichever lane or wave holds it."""
    from speechclip_plus_amd import ops
    V, rows = 8112, []
    for seed in range(1, 40):
        w = vc.noise_words(1, V, seed)[0] >> np.uint32(9)
        w[list(vc.SPECIAL)] = np.arange(3, dtype=np.uint32) + np.uint32(1 << 30)            # never part of a pair
        order = np.argsort(w, kind="stable")
        same = np.nonzero(w[order][1:] == w[order][:-1])[0]
        for i in same:
            rows.append((seed, int(order[i]), int(order[i + 1])))
        if len(rows) >= 6:
            break
    assert len(rows) >= 6
    for seed, lo, hi in rows[:6]:
        assert lo < hi
        x = torch.full((1, V), float("-inf"))
        x[0, lo] = x[0, hi] = 0.25
        idx, stats = ops.vq_noisy_rowstats(x.cuda(), V, 0.5, seed)
        g = vc.gumbel(1, V, seed)[0]
        assert g[lo] == g[hi] and int(idx[0]) == lo, (seed, lo, hi, int(idx[0]))
        assert abs(float(stats[0, 0]) - (0.25 + g[lo])) <= 1e-5 and abs(float(stats[1, 0]) - np.log(2.0)) <= 4 * U
    x = torch.full((2, 300), 0.5).cuda()                                                    # and without noise in the way: a flat row
    x[:, list(vc.SPECIAL)] = float("-inf")
    assert ops.vq_rowstats(x, 300, 1.0)[0].tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------------- dense subword_prob
@pytest.mark.parametrize("use_gumbel,hard", ((False, True),) + NEW_MODES)
@pytest.mark.parametrize("tau", [0.01, 0.1, 1.0])
@pytest.mark.parametrize("Nk,V", [(15, 50), (130, 1000), (7, 8112)])
def test_dense_subword_prob_in_the_four_modes(Nk, V, tau, use_gumbel, hard):
    from speechclip_plus_amd.vector_quantizers import SimpleVectorQuantizer
    x = vc.masked(_scores(Nk, V))
    vq = SimpleVectorQuantizer(temp=f"fixed={tau}", use_gumbel=use_gumbel, hard=hard).cuda().train()
    torch.manual_seed(5)
    seed = _next_seed()
    r = vq(torch.from_numpy(_scores(Nk, V)).cuda().view(1, Nk, V).clone())
    g = vc.gumbel(Nk, V, seed) if use_gumbel else None
    f = vc.forward(x, _t32(tau), hard, g)
    prob = _np(r["subword_prob"]).reshape(Nk, V)
    assert np.isfinite(prob).all() and np.all(prob[:, list(vc.SPECIAL)] == 0.0)
    y = np.sort(x if g is None else x + g, axis=-1)
    safe = (y[:, -1] - y[:, -2]) > (1e-4 if use_gumbel else 0.0)           # the device's x + g carries up to 4 U (1 + |g|) + U |x + g|
    assert safe.mean() >= 0.9
    assert np.array_equal(r["targets"].reshape(-1).cpu().numpy()[safe], f["targets"][safe])
    if hard:
        assert np.array_equal(prob[safe], f["prob"][safe])
        assert set(np.unique(prob)) == {0.0, 1.0} and np.all(prob.sum(-1) == 1.0)
    else:
        E_s = vc.prob_rel_bound(x, _t32(tau), use_gumbel, V)
        ratio = float((np.abs(prob - f["s"]) / (E_s * f["s"] + 2.0 ** -126)).max())
        print(f"s ({Nk}, {V}) tau {tau} gumbel {use_gumbel}: E_s {E_s:.2e}, largest error / bound = {ratio:.3f}")
        assert ratio <= 1.0 and np.abs(prob.sum(-1) - 1.0).max() <= E_s + (np.ceil(V / 256.0) + 8) * U
    assert r["temp"] == tau and r["num_vars"] == V


# ---------------------------------------------------------------------------------------------------- soft keywords
def _soft_keywords(x, table, tau, seed, noise, plant=None):
    """ops-level soft product on masked scores x [Nk, V] (numpy, -inf in the special columns); ``plant``: a planted error."""
    from speechclip_plus_amd import ops
    Nk, V = x.shape
    Et = table.shape[1]
    Vp = -(-V // 128) * 128
    xd = torch.from_numpy(x).float().cuda()
    if plant == "noise_row":                              # row n of the scores meets the noise of row n + 1
        xd = torch.cat([xd[-1:], xd[:-1]])
    stats = ops.vq_noisy_rowstats(xd, V, tau, seed, noise)[1]
    A = ops.vq_soft_split(xd, stats, V, tau, Vp, seed, noise)
    W = ops.vq_soft_table(torch.from_numpy(table).cuda(), Vp)
    assert A.shape == (-(-Nk // 128) * 128, 3 * Vp) and W.shape == (Et, 3 * Vp)
    blocks = A.view(A.shape[0], 3, Vp)
    assert float(blocks[Nk:].float().abs().max()) == 0.0 and float(blocks[:, :, V:].float().abs().max() if Vp > V else 0.0) == 0.0
    assert torch.equal(blocks[:, 0], blocks[:, 1])
    if plant == "lo_hi":
        blocks[:, 2] = 0
    if plant == "column":
        r = Nk // 2
        blocks[r, :, int(blocks[r, 0].float().argmax())] = 0
    out = _np(ops.vq_soft_product(A, W, Et)[:Nk])
    return np.concatenate([out[1:], out[:1]]) if plant == "noise_row" else out


def _violations(got, ref, bound):
    return int((np.abs(got - ref) > bound).sum()), float((np.abs(got - ref) / bound).max())


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("Et", [8, 512])
@pytest.mark.parametrize("V", [50, 1000, 8112])
@pytest.mark.parametrize("Nk", [6, 130])
def test_soft_keywords_against_fp64(Nk, V, Et, noise):
    tau, seed = 0.1, 4242
    x, table = vc.masked(_scores(Nk, V)), _table(V, Et)
    f = vc.forward(x, _t32(tau), False, vc.gumbel(Nk, V, seed) if noise else None, table)
    E_s = vc.prob_rel_bound(x, _t32(tau), noise, V)
    bound = vc.keyword_bound(f["s"], table.astype(np.float64), E_s, V)
    bad, ratio = _violations(_soft_keywords(x, table, tau, seed, noise), f["keywords"], bound)
    print(f"keywords ({Nk}, {V}, {Et}) noise {noise}: E_s {E_s:.2e} K_eff {vc.keyword_k_eff(V)}, largest error / bound = {ratio:.3f}")
    assert bad == 0, ratio


@pytest.mark.parametrize("plant,noise", [("lo_hi", False), ("lo_hi", True), ("column", False), ("column", True), ("noise_row", True)])
def test_planted_errors_in_the_soft_product_are_rejected(plant, noise):
    Nk, V, Et, tau, seed = 130, 1000, 8, 0.1, 4242
    x, table = vc.masked(_scores(Nk, V)), _table(V, Et)
    f = vc.forward(x, _t32(tau), False, vc.gumbel(Nk, V, seed) if noise else None, table)
    bound = vc.keyword_bound(f["s"], table.astype(np.float64), vc.prob_rel_bound(x, _t32(tau), noise, V), V)
    assert _violations(_soft_keywords(x, table, tau, seed, noise), f["keywords"], bound)[0] == 0
    bad, ratio = _violations(_soft_keywords(x, table, tau, seed, noise, plant=plant), f["keywords"], bound)
    print(f"planted {plant} noise {noise}: {bad} elements outside the bound, largest error / bound = {ratio:.1f}")
    assert bad > 0


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("V", [50, 1000])
def test_soft_keywords_at_a_cold_temperature_are_the_gather(V, noise):
    """tau = 1e-3: a row whose top-2 margin exceeds 40 tau has s = one-hot to e^-40, so the soft product must return table[argmax]
    within the split's 3 * 2^-18 and the accumulation term of |table[argmax]| (+ V e^-40 max |table| for the other columns)."""
    Nk, Et, tau, seed = 130, 8, 1e-3, 77
    x, table = vc.masked(_scores(Nk, V)), _table(V, Et).astype(np.float64)
    y = x + vc.gumbel(Nk, V, seed) if noise else x
    top = np.sort(y, axis=-1)
    safe = (top[:, -1] - top[:, -2]) / tau > 40.0 + 1.0
    assert safe.sum() >= 10
    got = _soft_keywords(x, table.astype(np.float32), tau, seed, noise)
    rows = table[vc.first_argmax(y)]
    bound = (3.0 * 2.0 ** -18 + 2.0 * U * (vc.keyword_k_eff(V) + 3)) * np.abs(rows) + V * np.exp(-40.0) * np.abs(table).max()
    assert np.all(np.abs(got - rows)[safe] <= bound[safe])


# ---------------------------------------------------------------------------------------------------- gradients
def _dense_step(vq, x32, t32):
    from speechclip_plus_amd import ops  # noqa: F401
    xd = torch.from_numpy(x32).cuda().requires_grad_()
    r = vq((xd * 1.0).view(1, *x32.shape))
    (r["subword_prob"].view(x32.shape) * torch.from_numpy(t32).cuda()).sum().backward()
    gt = vq.curr_temp.grad.clone() if isinstance(vq.curr_temp, torch.nn.Parameter) else None
    vq.zero_grad()
    return xd.grad.clone(), gt, r


@pytest.mark.parametrize("use_gumbel,hard", ((False, True),) + NEW_MODES)
@pytest.mark.parametrize("Nk,V", [(15, 50), (130, 1000)])
def test_dense_gradients_to_the_scores_and_the_temperature(Nk, V, use_gumbel, hard):
    """d x and d tau of the module-level forward with a learnable temperature (every mode, the default one included: a learnable
    temperature in training is new there too)."""
    from speechclip_plus_amd import ops
    from speechclip_plus_amd.vector_quantizers import SimpleVectorQuantizer
    tau = 0.1
    x32 = _scores(Nk, V)
    t32 = np.random.default_rng(V).standard_normal((Nk, V)).astype(np.float32)
    vq = SimpleVectorQuantizer(temp=f"learnable={tau}", use_gumbel=use_gumbel, hard=hard).cuda().train()
    tau = float(vq.curr_temp.item())
    torch.manual_seed(9)
    c0, seed = ops._mult_calls[0], _next_seed()
    dx, dtau, r = _dense_step(vq, x32, t32)
    ops._mult_calls[0] = c0
    dx2, dtau2, _ = _dense_step(vq, x32, t32)
    assert torch.equal(dx, dx2) and torch.equal(dtau, dtau2) and dtau.shape == (1,)                     # two calls, the same bits
    x = vc.masked(x32)
    f = vc.forward(x, tau, hard, vc.gumbel(Nk, V, seed) if use_gumbel else None)
    t = t32.astype(np.float64)
    _, rdx, rdtau, _ = vc.backward(f["s"], f["z"], t, tau)
    E_s = vc.prob_rel_bound(x, tau, use_gumbel, V)
    got = _np(dx)
    assert np.all(got[:, list(vc.SPECIAL)] == 0.0) and np.isfinite(got).all()
    ratio = float((np.abs(got - rdx) / (vc.dx_bound(f["s"], t, tau, E_s, V) + 2.0 ** -126)).max())
    b_tau, charged = vc.dtau_bound(x, f["s"], f["z"], t, tau, E_s, V, use_gumbel)
    r_tau = abs(float(dtau) - rdtau) / b_tau
    print(f"dense ({Nk}, {V}) gumbel {use_gumbel} hard {hard}: dx error / bound {ratio:.3f}; d tau {float(dtau):.6g} vs {rdtau:.6g}, "
          f"error / bound {r_tau:.3f} (bound / charged sum {b_tau / charged:.2e})")
    assert ratio <= 1.0 and r_tau <= 1.0 and np.isfinite(float(dtau)) and float(dtau) != 0.0


def _dkw_bound(kw, table, s, tau, gout, E_s, V):
    """Element-wise bound of d kw through quantize_keywords.  The chain: t = g . table^T with g and the table rounded to bf16 (2^-9
    each, products exact, fp32 accumulation over Et) -> dx in bf16 (dx_bound, bf16 form, with the error of t carried through the linear
    map t -> dz) -> dx . Tn with Tn the normalised table in bf16 (2^-9), fp32 accumulation over V in slices -> the normalisation's
    backward in fp32.  Every step's error is pushed through the absolute values of the steps behind it."""
    h = 2.0 ** -9
    Et = table.shape[1]
    tn = table / np.maximum(np.linalg.norm(table, axis=-1, keepdims=True), 1e-8)
    t_abs = np.abs(gout) @ np.abs(table).T
    d_t = (2.0 * h + h * h + (Et + 64) * U) * t_abs
    t = gout @ table.T
    lin = lambda e: s * (e + (s * e).sum(-1, keepdims=True)) / tau                       # |dz(e)| / tau for an error e >= 0 of t
    d_dx = vc.dx_bound(s, t, tau, E_s, V, bf16=True) + (1.0 + h) * lin(d_t)
    dx_abs = lin(np.abs(t))
    K = 128 * (-(-V // 128)) // 16 + 16
    d_dkwn = d_dx @ np.abs(tn) + (h + 2.0 * K * U) * (dx_abs @ np.abs(tn))
    n = np.maximum(np.linalg.norm(kw, axis=-1, keepdims=True), 1e-8)
    yv = np.abs(kw) / n
    back = lambda e: (e + yv * (yv * e).sum(-1, keepdims=True)) / n
    dkwn_abs = dx_abs @ np.abs(tn)
    return back(d_dkwn) + (Et + 16) * U * back(dkwn_abs)


@pytest.mark.parametrize("use_gumbel,hard", NEW_MODES)
@pytest.mark.parametrize("V,Et", [(50, 8), (1000, 64)])
def test_keyword_gradients_through_quantize_keywords(V, Et, use_gumbel, hard):
    """quantize_keywords in every new mode, temperature learnable: keywords, d kw and d tau against fp64 ON THE DEVICE'S SCORES (the
    cosine product has its own tests; what is new starts at the scores); a hard-mode model allocates no soft table."""
    from speechclip_plus_amd import ops
    from speechclip_plus_amd.vector_quantizers import SimpleVectorQuantizer
    B, N = 2, 65
    Nk = B * N
    table32 = _table(V, Et)
    rng = np.random.default_rng(V * 3 + Et)
    kw32 = (table32[rng.integers(4, V, Nk)] + 0.8 * rng.standard_normal((Nk, Et))).astype(np.float32)
    gout32 = rng.standard_normal((Nk, Et)).astype(np.float32)
    vq = SimpleVectorQuantizer(temp="learnable=0.1", use_gumbel=use_gumbel, hard=hard).cuda().train()
    tau = float(vq.curr_temp.item())
    table_d = torch.from_numpy(table32).cuda()

    def step():
        kw = torch.from_numpy(kw32).cuda().view(B, N, Et).requires_grad_()
        r, out = vq.quantize_keywords(kw, table_d)
        out.backward(torch.from_numpy(gout32).cuda().view(B, N, Et))
        gt = vq.curr_temp.grad.clone()
        vq.zero_grad()
        return r, out.detach(), kw.grad.clone(), gt
    torch.manual_seed(21)
    c0, seed = ops._mult_calls[0], _next_seed()
    r, out, dkw, dtau = step()
    assert ops._mult_calls[0] == c0 + (1 if use_gumbel else 0)
    ops._mult_calls[0] = c0
    r2, out2, dkw2, dtau2 = step()
    assert torch.equal(out, out2) and torch.equal(dkw, dkw2) and torch.equal(dtau, dtau2) and torch.equal(r["targets"], r2["targets"])
    tb = vq._tables["tables"]
    assert (tb._soft_T is None) == hard
    # the device's masked scores: read back through the module-level kernels on the same keywords
    cos = ops.cosine_scores_split(torch.from_numpy(kw32).cuda(), ops.vq_prep(torch.from_numpy(kw32).cuda())[1], tb.norm_split, tb.Vp)
    ops.vq_rowstats(cos[:Nk], V, tau, vc.SPECIAL)
    x = _np(cos[:Nk, :V])
    g = vc.gumbel(Nk, V, seed) if use_gumbel else None
    table, gout = table32.astype(np.float64), gout32.astype(np.float64)
    f = vc.forward(x, tau, hard, g, table)
    y = np.sort(x if g is None else x + g, axis=-1)
    safe = (y[:, -1] - y[:, -2]) > (1e-4 if use_gumbel else 0.0)          # the device's x + g is an fp32 sum: near-ties may fall either way
    assert safe.mean() >= 0.9
    assert np.array_equal(r["targets"].reshape(-1).cpu().numpy()[safe], f["targets"][safe])
    E_s = vc.prob_rel_bound(x, tau, use_gumbel, V)
    if hard:
        assert np.array_equal(_np(out).reshape(Nk, Et)[safe], table[f["targets"]][safe])
        assert np.array_equal(_np(r["subword_prob"]).reshape(Nk, V)[safe], f["prob"][safe])
    else:
        assert _violations(_np(out).reshape(Nk, Et), f["keywords"], vc.keyword_bound(f["s"], table, E_s, V))[0] == 0
        sp = _np(r["subword_prob"]).reshape(Nk, V)
        assert float((np.abs(sp - f["s"]) / (E_s * f["s"] + 2.0 ** -126)).max()) <= 1.0
    t = gout @ table.T
    _, rdx, rdtau, _ = vc.backward(f["s"], f["z"], t, tau)
    tn = table / np.maximum(np.linalg.norm(table, axis=-1, keepdims=True), 1e-8)
    kw = kw32.astype(np.float64)
    n = np.maximum(np.linalg.norm(kw, axis=-1, keepdims=True), 1e-8)
    yv = kw / n
    dkwn = rdx @ tn
    ref = (dkwn - yv * (yv * dkwn).sum(-1, keepdims=True)) / n
    ratio = float((np.abs(_np(dkw).reshape(Nk, Et) - ref) / _dkw_bound(kw, table, f["s"], tau, gout, E_s, V)).max())
    # d tau: t reaches the kernel with the relative error of two bf16 operands, on top of dtau_bound
    b_tau, charged = vc.dtau_bound(x, f["s"], f["z"], t, tau, E_s, V, use_gumbel)
    t_abs = np.abs(gout) @ np.abs(table).T
    az = np.where(f["s"] > 0, np.abs(f["z"]), 0.0)
    b_tau += (2.0 ** -8 + 2.0 ** -18 + (Et + 64) * U) * (f["s"] * (t_abs + (f["s"] * t_abs).sum(-1, keepdims=True)) * az).sum() / tau
    r_tau = abs(float(dtau) - rdtau) / b_tau
    print(f"quantize_keywords V {V} Et {Et} gumbel {use_gumbel} hard {hard}: d kw error / bound {ratio:.3f}, d tau {float(dtau):.6g} vs "
          f"{rdtau:.6g} error / bound {r_tau:.3f}")
    assert ratio <= 1.0 and r_tau <= 1.0 and float(dtau) != 0.0


# ---------------------------------------------------------------------------------------------------- unchanged paths
def test_the_default_mode_issues_todays_calls_and_draws_no_seed():
    from speechclip_plus_amd import ops
    from speechclip_plus_amd.vector_quantizers import SPECIAL_TOKENS, SimpleVectorQuantizer, VocabTables
    V, Et, B, N = 1000, 64, 2, 65
    Nk = B * N
    table = torch.from_numpy(_table(V, Et)).cuda()
    g = torch.Generator().manual_seed(3)
    kw0 = torch.randn(B, N, Et, generator=g).cuda()
    gout = torch.randn(B, N, Et, generator=g).cuda()
    c0 = ops._mult_calls[0]
    vq = SimpleVectorQuantizer(temp="fixed=0.1").cuda().train()
    kw = kw0.clone().requires_grad_()
    r, out = vq.quantize_keywords(kw, table)
    out.backward(gout)
    assert ops._mult_calls[0] == c0 and vq._tables["tables"]._soft_T is None
    # the sequence as it stood before the modes were added, issued by hand
    tb = VocabTables(table)
    k2 = kw0.reshape(Nk, Et).contiguous()
    _, rnorm = ops.vq_prep(k2)
    cos = ops.cosine_scores_split(k2, rnorm, tb.norm_split, tb.Vp)
    idx, lse_t, lse_1, ent = ops.vq_rowstats(cos[:Nk], V, 0.1, SPECIAL_TOKENS)
    ppl = ops.vq_perplexity(cos[:Nk], V, idx, lse_1)
    want = ops.vq_gather(tb.table, idx)
    assert torch.equal(out.reshape(Nk, Et), want) and torch.equal(r["targets"].reshape(-1), idx)
    assert torch.equal(r["prob_perplexity"], ppl[1]) and torch.equal(r["code_perplexity"], ppl[0])
    assert torch.equal(r["ent_per_t"], ent.view(B, N).mean(dim=0))
    Nkp, Vp = cos.shape
    gb = torch.zeros(Nkp, tb.Etp, device="cuda", dtype=torch.bfloat16)
    gb[:Nk, :Et] = gout.reshape(Nk, Et)
    t = torch.empty(Nkp, Vp, device="cuda", dtype=torch.float32)
    ops.gemm_raw(gb, tb.Etp, tb.table_bf16, tb.Etp, t, Vp, Nkp, Vp, tb.Etp, out_f32=True)
    dx = torch.zeros(Nkp, Vp, device="cuda", dtype=torch.bfloat16)
    dx[:Nk] = ops.vq_soft_bwd(cos[:Nk], lse_t, t[:Nk], V, 0.1, out_bf16=True, Vpad=Vp)
    S, Kc = tb.splits, Vp // tb.splits
    part = torch.empty(S, Nkp, Et, device="cuda", dtype=torch.float32)
    ops.gemm_raw(dx, Vp, tb.norm_T_bf16, Vp, part, Et, Nkp, Et, Kc, out_f32=True, nb1=S, sA=(Kc, 0), sW=(Kc, 0), sC=(Nkp * Et, 0))
    dkwn = torch.empty(Nkp, Et, device="cuda", dtype=torch.float32)
    ops.colsum(part, Nkp * Et, S, Nkp * Et, dkwn)
    assert torch.equal(kw.grad.reshape(Nk, Et), ops.vq_norm_bwd(k2, rnorm, dkwn[:Nk]))
    # sc_vq_soft_bwd2 without noise is sc_vq_soft_bwd: the same formula, the precise exponential instead of the fast one
    d2, _ = ops.vq_soft_bwd2(cos[:Nk], ops.vq_noisy_rowstats(cos[:Nk], V, 0.1, noise=False)[1], t[:Nk], V, 0.1, out_bf16=False)
    d1 = ops.vq_soft_bwd(cos[:Nk], lse_t, t[:Nk], V, 0.1, out_bf16=False)
    assert float((d2 - d1).abs().max()) <= 2.0 ** -16 * float(d1.abs().max())       # the fast exponential's error at |a| ~ 20 tau^-1


@pytest.mark.parametrize("temp", ["fixed=0.1", "learnable=0.1"])
def test_eval_mode_gives_the_defaults_bits_in_every_mode(temp):
    from speechclip_plus_amd import ops
    from speechclip_plus_amd.vector_quantizers import SimpleVectorQuantizer
    V, Et = 1000, 64
    table = torch.from_numpy(_table(V, Et)).cuda()
    kw = torch.randn(2, 65, Et, generator=torch.Generator().manual_seed(4)).cuda()
    x = torch.from_numpy(_scores(130, 1000)).cuda().view(2, 65, 1000)
    c0 = ops._mult_calls[0]
    base = SimpleVectorQuantizer(temp="fixed=0.1").cuda().eval()
    r0, out0 = base.quantize_keywords(kw, table)
    d0 = base(x.clone())
    for use_gumbel, hard in NEW_MODES + ((False, True),):
        vq = SimpleVectorQuantizer(temp=temp, use_gumbel=use_gumbel, hard=hard).cuda().eval()
        r, out = vq.quantize_keywords(kw, table)
        d = vq(x.clone())
        assert torch.equal(out, out0) and not out.requires_grad
        for k in ("targets", "code_perplexity", "prob_perplexity", "ent_per_t", "diversity_loss", "subword_prob"):
            assert torch.equal(r[k], r0[k]) and torch.equal(d[k], d0[k]), k
    assert ops._mult_calls[0] == c0


# ---------------------------------------------------------------------------------------------------- the launch sequences
RECORDED_OPS = ("vq_prep", "sgemm_mfma", "cosine_scores_split", "vq_rowstats", "vq_perplexity", "vq_noisy_rowstats", "vq_gather", "vq_onehot",
                "vq_soft_prob", "vq_soft_split", "vq_soft_table", "vq_soft_product", "vq_soft_bwd", "vq_soft_bwd2", "gemm_raw", "colsum",
                "vq_norm_bwd")
CONFIGURATIONS = {"default": {}, "soft": {"hard": False}, "gumbel_hard": {"use_gumbel": True, "hard": True}, "learnable": {"temp": "learnable=0.1"}}
MODE_ONLY = {"vq_noisy_rowstats", "vq_soft_bwd2", "vq_soft_split", "vq_soft_prob", "vq_soft_table"}
KW_FRONT = ["vq_prep", "cosine_scores_split", "vq_rowstats", "vq_perplexity"]
KW_BACK = ["gemm_raw", "colsum", "vq_norm_bwd"]
# What the two nodes called before they took the mode as an argument (recorded with record_sequences on that code, one class per
# entry point and mode family then): forward calls, "|", backward calls.
KEYWORD_SEQUENCES = {
    "default": KW_FRONT + ["vq_gather", "|", "gemm_raw", "vq_soft_bwd"] + KW_BACK,
    "soft": KW_FRONT + ["vq_noisy_rowstats", "vq_soft_split", "vq_soft_table", "vq_soft_product", "|", "gemm_raw", "vq_soft_bwd2"] + KW_BACK,
    "gumbel_hard": KW_FRONT + ["vq_noisy_rowstats", "vq_gather", "|", "gemm_raw", "vq_soft_bwd2"] + KW_BACK,
    "learnable": KW_FRONT + ["vq_noisy_rowstats", "vq_gather", "|", "gemm_raw", "vq_soft_bwd2"] + KW_BACK,
    "eval": KW_FRONT + ["vq_gather", "|"],
}
DENSE_SEQUENCES = {
    "default": ["vq_rowstats", "vq_perplexity", "vq_onehot", "|", "vq_soft_bwd"],
    "soft": ["vq_rowstats", "vq_perplexity", "vq_noisy_rowstats", "vq_soft_prob", "|", "vq_soft_bwd2"],
    "gumbel_hard": ["vq_rowstats", "vq_perplexity", "vq_noisy_rowstats", "vq_onehot", "|", "vq_soft_bwd2"],
    "learnable": ["vq_rowstats", "vq_perplexity", "vq_noisy_rowstats", "vq_onehot", "|", "vq_soft_bwd2"],
    "eval": ["vq_rowstats", "vq_perplexity", "vq_onehot", "|"],
}


def record_sequences(setattr_):
    """-> (keyword sequences, dense sequences): the ``ops`` functions quantize_keywords (V = 50 table, 6 keyword rows) and forward(x)
    (a (2, 3, 50) score tensor) call, in order, per configuration; calls one recorded function makes to another are its own business
    and are not recorded.  ``setattr_(ops, name, wrapper)`` installs the recorder (monkeypatch.setattr)."""
    from speechclip_plus_amd import ops
    from speechclip_plus_amd.vector_quantizers import SimpleVectorQuantizer
    log, depth = [], [0]

    def recorder(name, fn):
        @functools.wraps(fn)
        def wrapper(*args, **kwargs):
            if depth[0] == 0:
                log.append(name)
            depth[0] += 1
            try:
                return fn(*args, **kwargs)
            finally:
                depth[0] -= 1
        return wrapper
    V, Et = 50, 8
    table = torch.from_numpy(_table(V, Et)).cuda()
    kw0 = torch.randn(2, 3, Et, generator=torch.Generator().manual_seed(11)).cuda()
    x0 = torch.from_numpy(_scores(15, V)[:6].reshape(2, 3, V).copy()).cuda()
    quantizers = {name: SimpleVectorQuantizer(**{"temp": "fixed=0.1", **args}).cuda().train() for name, args in CONFIGURATIONS.items()}
    quantizers["eval"] = SimpleVectorQuantizer(temp="fixed=0.1").cuda().eval()
    for name in RECORDED_OPS:
        setattr_(ops, name, recorder(name, getattr(ops, name)))
    keyword, dense = {}, {}
    for name, vq in quantizers.items():
        kw = kw0.clone().requires_grad_(vq.training)
        _, out = vq.quantize_keywords(kw, table)
        log.append("|")
        if vq.training:
            out.sum().backward()
        keyword[name], log[:] = list(log), []
        x = x0.clone().requires_grad_(vq.training)
        r = vq(x * 1.0)
        log.append("|")
        if vq.training:
            (r["subword_prob"] * x0).sum().backward()
        dense[name], log[:] = list(log), []
    return keyword, dense


def test_the_launch_sequences_are_the_ones_before_the_nodes_were_folded(monkeypatch):
    from speechclip_plus_amd import ops
    c0 = ops._mult_calls[0]
    try:
        keyword, dense = record_sequences(monkeypatch.setattr)
    finally:
        ops._mult_calls[0] = c0
    assert keyword == KEYWORD_SEQUENCES and dense == DENSE_SEQUENCES
    for seq in (keyword["default"], keyword["eval"], dense["default"], dense["eval"]):
        assert not MODE_ONLY & set(seq)
    assert keyword["eval"][-1] == "|" and dense["eval"][-1] == "|"                       # eval records no backward call


# ---------------------------------------------------------------------------------------------------- sampling
@pytest.mark.parametrize("seed", vc.SAMPLING_SEEDS)
def test_sampled_tokens_follow_the_softmax_on_the_device(seed):
    from speechclip_plus_amd import ops
    Nk, V = 65536, 16
    x = vc.masked(np.tile(np.linspace(-1.0, 1.0, V), (Nk, 1)))
    idx, _ = ops.vq_noisy_rowstats(torch.from_numpy(x).float().cuda(), V, 1.0, seed)
    counts = np.bincount(idx.cpu().numpy(), minlength=V)
    _, expect, sigma = vc.sampling_counts(seed)
    live = sigma > 0
    dev = float(np.abs((counts - expect)[live] / sigma[live]).max())
    print(f"device sampling seed {seed:#x}: largest deviation {dev:.2f} sigma")
    assert counts[list(vc.SPECIAL)].sum() == 0 and counts.sum() == Nk and dev <= 4.0


# ---------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def model_setup():
    from speechclip_plus_amd import KWClip_GeneralTransformer, cascaded_base_config, random_hubert_state_dict
    from speechclip_plus_amd.speech_encoder import ARCHS
    arch = dataclasses.replace(ARCHS["hubert"], layers=2)
    torch.manual_seed(42)
    cfg = cascaded_base_config()
    cfg.audio_encoder.max_audio_len = -1
    cfg.model_settings.cascaded_branch.vq.args.temp = "learnable=0.1"
    cfg.model_settings.cascaded_branch.vq.args.hard = False
    model = KWClip_GeneralTransformer(cfg, device="cuda:0", hubert_state_dict=random_hubert_state_dict(arch, seed=42), hubert_arch=arch).train()
    g = torch.Generator().manual_seed(7)
    lens = [24000, 17000, 20000, 24000]
    wav = torch.zeros(len(lens), max(lens))
    for b, n in enumerate(lens):
        wav[b, :n] = torch.randn(n, generator=g) * 0.5
    batch = {"wav": wav.cuda(), "wav_len": torch.tensor(lens), "image": torch.randn(len(lens), 512, generator=g).cuda(),
             "id": torch.tensor([0, 1, 1, 2]).cuda()}
    return model, batch


def _train_step(model, batch, seed):
    from speechclip_plus_amd import mha_block, ops
    torch.manual_seed(seed)
    # the three call counters the stateless dropout (and Gumbel) seeds are derived from, beside torch's seed
    ops._mult_calls[0], mha_block._calls, model.audio_encoder._drop_calls = 0, 0, 0
    model.zero_grad(set_to_none=True)
    bn = model.cascaded_branch.bn_layer.bn_layer
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    losses_, _, others = model(batch)
    out = model.compute_loss(losses_)
    out["loss"].backward()
    bn.load_state_dict(state)                                        # every step starts from the same running statistics
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad and p.grad is not None}
    return out["loss"].detach().clone(), others["vq_results"]["targets"].clone(), others["keywords"].detach().clone(), grads


def test_model_train_step_with_soft_keywords_and_a_learnable_temperature(model_setup):
    model, batch = model_setup
    vq = model.cascaded_branch.vector_quantizer
    assert (vq.hard, vq.use_gumbel, vq.temp_type) == (False, False, "learnable")
    assert any(p is vq.curr_temp for p in model.getTrainableParams())
    loss, targets, kws, grads = _train_step(model, batch, 1)
    assert torch.isfinite(loss) and torch.isfinite(kws).all()
    trainable = {n for n, p in model.named_parameters() if any(p is q for q in model.getTrainableParams())}
    assert "cascaded_branch.vector_quantizer.curr_temp" in trainable and "audio_encoder.weightedsum_layer.weights" in trainable
    assert trainable <= set(grads), sorted(trainable - set(grads))                   # every trainable parameter gets a gradient
    assert all(torch.isfinite(g).all() for g in grads.values())
    gt = grads["cascaded_branch.vector_quantizer.curr_temp"]
    assert gt.shape == (1,) and torch.isfinite(gt).all() and float(gt) != 0.0
    tb = vq._tables["tables"]
    assert tb._soft_T is not None and tb._soft_T.shape == (512, 3 * tb.Vp)
    # soft keywords are mixtures of table rows, not rows: no keyword equals its argmax row
    rows = tb.table[targets.reshape(-1)]
    assert float((kws.reshape(-1, 512).float() - rows).norm() / rows.norm()) > 1e-3


def test_model_train_step_with_gumbel_is_reproducible_and_seeded(model_setup):
    model, batch = model_setup
    vq = model.cascaded_branch.vector_quantizer
    vq.use_gumbel = True
    try:
        for hard in (True, False):
            vq.hard = hard
            a = _train_step(model, batch, 1)
            b = _train_step(model, batch, 1)
            c = _train_step(model, batch, 2)
            assert torch.isfinite(a[0]) and all(torch.isfinite(g).all() for g in a[3].values())
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
            assert set(a[3]) == set(b[3]) and all(torch.equal(a[3][n], b[3][n]) for n in a[3])
            assert not torch.equal(a[1], c[1])                          # another seed samples other tokens
            gt = a[3]["cascaded_branch.vector_quantizer.curr_temp"]
            assert torch.isfinite(gt).all() and float(gt) != 0.0
            if hard:
                tb = vq._tables["tables"]
                rows = tb.table[a[1].reshape(-1)]
                assert float((a[2].reshape(-1, 512).float() - rows).norm() / rows.norm()) < 1e-5
    finally:
        vq.use_gumbel, vq.hard = False, False
