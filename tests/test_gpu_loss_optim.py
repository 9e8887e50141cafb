"""The end of the train step against fp64: MaskedContrastiveLoss on sc_infonce_fwd / sc_infonce_grad at multi-tile, ragged and
option-bearing shapes, and the fused clip + Adam launch (sc_sumsq_f32, sc_adam_f32: ops.sumsq / ops.adam_step under optim.FlatAdam) on buffers that stride, misalign and pad.

Inputs and references come from tests/loss_cases.py (seeded; fp64 = oracle.loss_ref under torch autograd, and a plain fp64 Adam).
Bounds (docs/parity.md, "Contrastive loss and flat Adam"):
  * temperature 0.07: logits 2e-5, log-sum-exps 5e-5, loss 2e-5 max(1, |loss|), all absolute; gradients max |g - g64| / max |g64|
    <= 2e-4 each.
  * temperature 0.01: min(4 x the error of the fp32 oracle on the CPU against fp64, 7 x the bounds above).  The fp32 oracle's error
    is printed for every other loss case too, as a yardstick only.
  * sumsq: relative error <= 2 k 2^-24, k = the longest chain of additions of the launch geometry.
  * Adam p / m / v / update: 4 x the error of fp32 torch.optim.Adam on the CPU against the fp64 restatement, each relative to the
    quantity's largest magnitude over the run.
Every figure is printed as a ``PARITY|case|quantity|error|yardstick|bound`` line before anything is asserted."""
import pytest
import torch

import loss_cases as lc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _ops():
    from speechclip_plus_amd import ops
    return ops


def _report(case, quantity, err, yardstick, bound):
    ys = "-" if yardstick is None else f"{yardstick:.3e}"
    print(f"PARITY|{case}|{quantity}|{err:.3e}|{ys}|{bound:.3e}")
    return [] if err <= bound else [f"{case}: {quantity} error {err:.3e} > bound {bound:.3e} (yardstick {ys})"]


# ---------------------------------------------------------------------------------------------------------------- loss
def _module_run(dev, A, Bm, ids, temperature=0.07, scale=1.0, **kw):
    """MaskedContrastiveLoss(...)(A, B, ids) and backward() on the device -> loss, dA, dB, [dT, log_inv_temp]."""
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    kw = dict(kw)
    trainable = kw.pop("trainable", False)
    crit = MaskedContrastiveLoss(temperature=temperature, temperature_trainable=trainable, **kw).to(dev)
    a, b = A.to(dev).requires_grad_(True), Bm.to(dev).requires_grad_(True)
    loss = crit(a, b, ids.to(dev) if ids is not None else None)
    (loss if scale == 1.0 else scale * loss).backward()
    out = {"loss": loss.detach(), "dA": a.grad, "dB": b.grad}
    if trainable:
        out.update(dT=crit.temperature.grad, log_inv_temp=crit.temperature.detach())
    return out


def _ops_run(dev, A, Bm, ids, temperature=0.07, margin=0.0, dcl=False, a2b=True, b2a=True, trainable=False):
    """ops.infonce_fwd -> loss, logits, lse_row, lse_col (the forward takes the inverse temperature as a device scalar)."""
    it = torch.full((1,), 1.0 / temperature, device=dev)
    loss, logits, lr, lcol = _ops().infonce_fwd(A.to(dev), Bm.to(dev), ids.to(dev) if ids is not None else None, it, margin, dcl, a2b, b2a)
    return {"loss": loss.reshape(()), "logits": logits, "lse_row": lr, "lse_col": lcol}


def _errors(got, ref):
    e = {}
    for k in got:
        if k in ("dA", "dB", "dT"):
            e[k] = lc.scale_rel_err(got[k], ref[k])
        elif k in ("loss", "logits", "lse_row", "lse_col"):
            e[k] = lc.max_abs_err(got[k], ref[k])
    return e


def _base_bounds(ref, factor=1.0):
    return {"loss": factor * lc.TOL_LOSS * max(1.0, abs(float(ref["loss"]))), "logits": factor * lc.TOL_LOGITS,
            "lse_row": factor * lc.TOL_LSE, "lse_col": factor * lc.TOL_LSE, "dA": factor * lc.TOL_GRAD, "dB": factor * lc.TOL_GRAD,
            "dT": factor * lc.TOL_GRAD}


def _check(case, got, ref, yard=None, yard_bound=False):
    """``got`` against the fp64 ``ref``.  ``yard``: the fp32 oracle's results, whose error is printed next to the device's;
    ``yard_bound``: the bound is min(4 x that error, 7 x base) instead of the base bounds."""
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (case, k)
    err = _errors(got, ref)
    yerr = _errors({k: yard[k] for k in err}, ref) if yard is not None else {}
    bounds = _base_bounds(ref)
    if yard_bound:
        cap = _base_bounds(ref, 7.0)
        bounds = {k: min(4.0 * yerr[k], cap[k]) for k in err}
    bad = []
    for k in err:
        bad += _report(case, k, err[k], yerr.get(k), bounds[k])
    return bad


def _both_paths(dev, case, A, Bm, ids, temperature=0.07, scale=1.0, yard=False, **kw):
    """The module path (loss, gradients) and the forward entry (logits, log-sum-exps) of one case against fp64."""
    mod = _module_run(dev, A, Bm, ids, temperature, scale, **kw)
    ref = lc.loss_reference(A, Bm, ids, temperature, scale=scale, log_inv_temp=mod.pop("log_inv_temp", None), **kw)
    y = lc.loss_reference(A, Bm, ids, temperature, scale=scale, dtype=torch.float32, **kw)      # printed; the bound only where ``yard``
    bad = _check(case + " module", mod, ref, y, yard)
    fwd = _ops_run(dev, A, Bm, ids, temperature, **kw)
    bad += _check(case + " forward", fwd, ref, y, yard)
    return bad, mod, fwd


@pytest.mark.parametrize("with_ids", [True, False], ids=["ids", "noindex"])
@pytest.mark.parametrize("Bg,E", lc.SHAPE_SWEEP)
def test_loss_shape_sweep(dev, Bg, E, with_ids):
    """Default options from one row to 16 x 16 tiles, E from one float4 to twelve K-tiles (68 and 100: a partial last K-tile, 4, 20,
    68, 100: not a multiple of 16), with ``ids = arange // 5`` and with ``index=None``."""
    A, Bm = lc.make_pair(Bg, E, seed=Bg * 1000 + E)
    ids = lc.ids_div5(Bg) if with_ids else None
    bad, mod, fwd = _both_paths(dev, f"sweep Bg={Bg} E={E} {'ids' if with_ids else 'noindex'}", A, Bm, ids)
    assert not bad, bad
    if Bg == 1 or (with_ids and Bg <= 5):          # -l + log(exp(l)): the oracle's 0 and zeros, exactly
        assert float(mod["loss"]) == 0.0 and float(fwd["loss"]) == 0.0
        assert float(mod["dA"].abs().max()) == 0.0 and float(mod["dB"].abs().max()) == 0.0


@pytest.mark.parametrize("Bg", [130, 200])
@pytest.mark.parametrize("name", list(lc.VARIANTS))
def test_loss_variants_multi_tile(dev, name, Bg):
    """margin / dcl / one-sided / trainable temperature at 3 x 3 and 4 x 4 ragged tiles: the margin on the diagonal of every diagonal
    tile, the ``!dcl`` diagonal test in off-diagonal tiles, d loss / d log(1 / T)."""
    A, Bm = lc.make_pair(Bg, 100, seed=Bg + len(name))
    bad, _, _ = _both_paths(dev, f"variant {name} Bg={Bg}", A, Bm, lc.ids_div5(Bg), **lc.VARIANTS[name])
    assert not bad, bad


@pytest.mark.parametrize("permuted", [False, True], ids=["aligned", "permuted"])
def test_loss_tile_without_negatives(dev, permuted):
    """dcl with groups of 70 ids at Bg = 200: tile (0, 0) has no negative for any of its rows and columns (partial max -inf, which
    the merge has to skip); the permuted ids scatter the same groups over all tiles."""
    Bg = 200
    ids = lc.ids_empty_tile_permuted(Bg) if permuted else lc.ids_empty_tile(Bg)
    A, Bm = lc.make_pair(Bg, 100, seed=70 + permuted)
    bad, _, _ = _both_paths(dev, f"empty tile {'permuted' if permuted else 'aligned'}", A, Bm, ids, dcl=True)
    assert not bad, bad


def test_loss_wide_ids(dev):
    """Negative ids and ids that differ only above bit 31: bit for bit the result of the same grouping labelled 0 .. k - 1."""
    Bg = 130
    ids = lc.wide_ids(Bg)
    A, Bm = lc.make_pair(Bg, 100, seed=31)
    bad, mod, fwd = _both_paths(dev, "wide ids", A, Bm, ids)
    _, mod2, fwd2 = _both_paths(dev, "wide ids relabelled", A, Bm, lc.relabel(ids))
    assert not bad, bad
    for a, b in ((mod, mod2), (fwd, fwd2)):
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_loss_large_logits(dev):
    """Fixed temperature 0.01 (inverse 100, CLIP's ceiling), Bg = 200, E = 64: finite, and within min(4 x the fp32 oracle's own error
    against fp64, 7 x the 0.07 bounds)."""
    A, Bm = lc.make_pair(200, 64, seed=100)
    bad, _, _ = _both_paths(dev, "temperature 0.01", A, Bm, lc.ids_div5(200), temperature=0.01, yard=True)
    assert not bad, bad


def test_loss_scaled_before_backward(dev):
    """(0.25 * loss).backward(), as accumulate_grad_batches does: the incoming gradient reaches sc_infonce_grad as gscale."""
    A, Bm = lc.make_pair(130, 100, seed=25)
    ids = lc.ids_div5(130)
    mod = _module_run(dev, A, Bm, ids, scale=0.25)
    full, y = lc.loss_reference(A, Bm, ids), lc.loss_reference(A, Bm, ids, scale=0.25, dtype=torch.float32)
    ref = {"loss": full["loss"], "dA": 0.25 * full["dA"], "dB": 0.25 * full["dB"]}
    bad = _check("scaled 0.25", mod, ref, y)
    assert not bad, bad


ROUNDS = [(200, 1), (200, 2), (200, 3), (130, 4), (200, 5)]


@pytest.mark.parametrize("path", ["module", "forward"])
def test_loss_workspace_reuse(dev, path):
    """Launch after launch on one stream and one (device, stream, Bg) workspace with different data: the ticket word has to come back
    to zero and no partial of an earlier launch may survive.  The forward path runs its second round with margin + dcl."""
    bad = []
    for r, (Bg, seed) in enumerate(ROUNDS):                          # all on the current stream
        A, Bm = lc.make_pair(Bg, 100, seed=seed)
        ids = lc.ids_div5(Bg)
        kw = dict(margin=0.3, dcl=True) if (path == "forward" and r == 1) else {}
        ref, y = lc.loss_reference(A, Bm, ids, **kw), lc.loss_reference(A, Bm, ids, dtype=torch.float32, **kw)
        got = _module_run(dev, A, Bm, ids, **kw) if path == "module" else _ops_run(dev, A, Bm, ids, **kw)
        bad += _check(f"reuse {path} round {r} Bg={Bg}", got, ref, y)
    assert not bad, bad


def test_loss_is_bitwise_repeatable(dev):
    """docs/kernels.md: fixed-order reductions.  16 x 16 tiles arrive at the ticket in any order; the result may not depend on it."""
    A, Bm = lc.make_pair(1000, 68, seed=8)
    ids = lc.ids_div5(1000)
    runs = [{**_module_run(dev, A, Bm, ids), **{"fwd_" + k: v for k, v in _ops_run(dev, A, Bm, ids).items()}} for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert torch.equal(runs[0]["loss"], runs[0]["fwd_loss"])


# ---------------------------------------------------------------------------------------------------------------- optimiser
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("n", list(lc.ADAM_SIZES))
def test_sumsq_vs_fp64(dev, n, aligned):
    """sc_sumsq_f32 + the merge of its partials against an fp64 sum: 16-byte body with a scalar tail, and the scalar branch of a
    buffer four bytes off.  Every term is >= 0, so the relative error is at most (chain of additions) x 2^-24, doubled for the
    squares' own rounding."""
    buf = lc.sumsq_values(n, seed=n).to(dev)
    x = buf[1:].clone() if aligned else buf[1:]
    assert x.numel() == n and x.is_contiguous() and (x.data_ptr() % 16 == 0) == aligned
    part = _ops().sumsq(x)
    assert part.numel() == lc.SUMSQ_BLOCKS
    got = lc.merge_partials_fp32(part)
    ref = float((x.double().cpu() ** 2).sum())
    k = lc.sumsq_chain(n, aligned)
    bad = _report(f"sumsq n={n} {'aligned' if aligned else 'misaligned'}", "sum", abs(got - ref) / ref, None, 2 * k * U)
    assert not bad, bad


def _flat_views(opt, buf):
    return [buf[off: off + p.numel()] for p, off in zip(opt.params, opt.offsets)]


@pytest.mark.parametrize("hyper", list(lc.ADAM_HYPER))
@pytest.mark.parametrize("total", list(lc.ADAM_SIZES))
def test_flat_adam_vs_fp64(dev, total, hyper):
    """FlatAdam (sumsq + clip + Adam in one launch pair) against the fp64 restatement: parameters, both moment buffers and the
    per-step update of the parameter that starts in [-1e-3, 1e-3]; 20 steps on the warm-up / decay schedule, then two steps from
    step_count 9 999 (3 steps at 7.6 M elements).  One and three elements are pooled over 16 seeds: the errors are the largest over
    all 16 runs, on both sides of the 4 x (fp32 torch's error on one element of one run can be 0, which bounds nothing)."""
    from speechclip_plus_amd.optim import FlatAdam, ALIGN
    wd, clip, _ = lc.ADAM_HYPER[hyper]
    big = total > 1_000_000
    steps = [0, 1, 2] if big else list(range(20)) + [9999, 10000]
    num = {q: [0.0, 0.0] for q in ("p", "m", "v", "update")}         # [device, fp32 torch]: max |x - x64| over the run
    den = {q: 0.0 for q in num}                                      # max |x64| over the run
    bad = []
    for seed in (range(16) if total <= 3 else [total % 1000]):
        ps = lc.adam_params(total, seed)
        dps = [torch.nn.Parameter(p.to(dev)) for p in ps]
        opt = FlatAdam(dps, lr=lc.ADAM_LR, betas=lc.ADAM_BETAS, eps=lc.ADAM_EPS, weight_decay=wd, max_grad_norm=clip)
        ref = lc.AdamRef64(ps, weight_decay=wd, max_grad_norm=clip)
        t32 = lc.TorchAdam(ps, weight_decay=wd, max_grad_norm=clip)
        assert opt.size % ALIGN == 0 and opt.size >= total
        pad = torch.ones(opt.size, dtype=torch.bool, device=dev)
        for v in _flat_views(opt, pad):
            v.fill_(False)
        assert int(pad.sum()) == opt.size - total
        for s in steps:
            if s == 9999:
                opt.step_count = ref.step_count = 9999
                t32.set_step_count(9999)
            gs = lc.adam_grads(total, hyper, min(s, 25), seed)
            lr = lc.adam_lr(min(s, 25))
            opt.zero_grad()
            for p, g in zip(dps, gs):
                p.grad.copy_(g.to(dev))
            before = [dps[0].detach().double().cpu(), ref.p[0].clone(), t32.p[0].double()]   # the update is taken in fp64: exact
            if clip > 0 and s in (0, 1):                             # the clipped norm is the norm over the real gradients
                ssq = lc.merge_partials_fp32(_ops().sumsq(opt.flat_g))
                want = sum(float((g.double() ** 2).sum()) for g in gs)
                bad += _report(f"adam n={total} {hyper} step {s}", "flat_g sumsq", abs(ssq - want) / want, None,
                               2 * lc.sumsq_chain(opt.size, True) * U)
            opt.step(lr=lr)
            ref.step(gs, lr)
            t32.step(gs, lr)
            got = {"p": [p.detach().cpu() for p in dps], "m": [x.cpu() for x in _flat_views(opt, opt.m)],
                   "v": [x.cpu() for x in _flat_views(opt, opt.v)], "update": [dps[0].detach().double().cpu() - before[0]]}
            yard = {"p": t32.p, "m": t32.m, "v": t32.v, "update": [t32.p[0].double() - before[2]]}
            want = {"p": ref.p, "m": ref.m, "v": ref.v, "update": [ref.p[0] - before[1]]}
            for q in num:
                for i, side in enumerate((got, yard)):
                    num[q][i] = max(num[q][i], max(float((x.double() - r).abs().max()) for x, r in zip(side[q], want[q])))
                den[q] = max(den[q], max(float(r.abs().max()) for r in want[q]))
        assert opt.step_count == steps[-1] + 1
        for name, buf in (("flat_p", opt.flat_p), ("m", opt.m), ("v", opt.v), ("flat_g", opt.flat_g)):
            if opt.size > total:
                assert float(buf[pad].abs().max()) == 0.0, (name, "padding moved")
    for q in num:
        bad += _report(f"adam n={total} {hyper}", q, num[q][0] / den[q], num[q][1] / den[q], 4.0 * num[q][1] / den[q])
    assert not bad, bad
