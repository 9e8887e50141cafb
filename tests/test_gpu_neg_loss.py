"""The contrastive loss with a negative bank (csrc/infonce_neg.hip: sc_infonce_neg_fwd / sc_infonce_neg_grad under
MaskedContrastiveLoss.forward(..., bank=, bank_ids=, neg_idx=) and model.set_negative_bank) against fp64.

Inputs and the fp64 reference come from tests/neg_loss_cases.py: lc.make_pair rows, ids = arange // 5, a bank of unit Gaussian rows
whose first min(Bg, N / 2) rows are the batch's own B rows under the batch's ids, lists = the true top M among rows with another id.
Bounds (docs/parity.md, "Contrastive loss with a negative bank"): the project's own at temperature 0.07 - x 2e-5, log-sum-exps 5e-5,
loss 2e-5 max(1, |loss|), all absolute; gradients max |g - g64| / max |g64| <= 2e-4 - and at 0.01 min(4 x the error of the fp32 form
of the reference expression on the CPU, 7 x those).  ``used`` and everything stated "bit for bit" is compared with ==.
Every figure is printed as a ``PARITY|case|quantity|error|yardstick|bound`` line before anything is asserted."""
import functools

import pytest
import torch

import loss_cases as lc
import neg_loss_cases as nc

pytestmark = pytest.mark.gpu


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


@functools.lru_cache(maxsize=None)
def _case(shape, with_ids=True):
    return nc.make_case(*shape, with_ids=with_ids)


def _to(dev, t):
    return t.to(dev) if t is not None else None


def _module_run(dev, c, temperature=0.07, scale=1.0, **kw):
    """MaskedContrastiveLoss(...)(A, B, ids, bank=, bank_ids=, neg_idx=) and backward() -> loss, dA, dB, used, [dT, log_inv_temp]"""
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    kw = dict(kw)
    trainable = kw.pop("trainable", False)
    crit = MaskedContrastiveLoss(temperature=temperature, temperature_trainable=trainable, **kw).to(dev)
    a, b = c["A"].to(dev).requires_grad_(True), c["B"].to(dev).requires_grad_(True)
    loss = crit(a, b, _to(dev, c["ids"]), bank=c["bank"].to(dev), bank_ids=_to(dev, c["bank_ids"]), neg_idx=c["neg_idx"].to(dev))
    (loss if scale == 1.0 else scale * loss).backward()
    out = {"loss": loss.detach(), "dA": a.grad, "dB": b.grad, "used": crit.last_used}
    if trainable:
        out.update(dT=crit.temperature.grad, log_inv_temp=crit.temperature.detach())
    return out


def _plain_run(dev, c, temperature=0.07, **kw):
    """the same criterion without the keywords, and ops.infonce_fwd's lse_row"""
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    crit = MaskedContrastiveLoss(temperature=temperature, **kw).to(dev)
    a, b = c["A"].to(dev).requires_grad_(True), c["B"].to(dev).requires_grad_(True)
    loss = crit(a, b, _to(dev, c["ids"]))
    loss.backward()
    it = torch.full((1,), 1.0 / temperature, device=dev)
    lse_row = _ops().infonce_fwd(c["A"].to(dev), c["B"].to(dev), _to(dev, c["ids"]), it, kw.get("margin", 0.0), kw.get("dcl", False),
                                 kw.get("a2b", True), kw.get("b2a", True))[2]
    return {"loss": loss.detach(), "dA": a.grad, "dB": b.grad, "lse_row": lse_row}


def _ops_run(dev, c, temperature=0.07, margin=0.0, dcl=False, a2b=True, b2a=True, trainable=False, bank=None, neg_idx=None):
    """ops.infonce_fwd, then ops.infonce_neg_fwd -> loss, lse_row (extended), x, used"""
    ops = _ops()
    it = torch.full((1,), 1.0 / temperature, device=dev)
    A, ids = c["A"].to(dev), _to(dev, c["ids"])
    _, logits, lr, lcol = ops.infonce_fwd(A, c["B"].to(dev), ids, it, margin, dcl, a2b, b2a)
    bank = c["bank"].to(dev) if bank is None else bank
    neg_idx = c["neg_idx"].to(dev) if neg_idx is None else neg_idx
    loss, lse_ext, x, used = ops.infonce_neg_fwd(A, bank, neg_idx, ids, _to(dev, c["bank_ids"]), it, lr, lcol, logits, a2b, b2a)
    return {"loss": loss.reshape(()), "lse_row": lse_ext, "x": x, "used": used}


def _errors(got, ref):
    e = {}
    for k in got:
        if k in ("dA", "dB", "dT"):
            e[k] = lc.scale_rel_err(got[k], ref[k])
        elif k in ("loss", "lse_row"):
            e[k] = lc.max_abs_err(got[k], ref[k])
        elif k == "x":
            e[k] = nc.x_err(got[k], ref[k])
    return e


def _base_bounds(ref, factor=1.0):
    return {"loss": factor * lc.TOL_LOSS * max(1.0, abs(float(ref["loss"]))), "x": factor * lc.TOL_LOGITS, "lse_row": factor * lc.TOL_LSE,
            "dA": factor * lc.TOL_GRAD, "dB": factor * lc.TOL_GRAD, "dT": factor * lc.TOL_GRAD}


def _check(case, got, ref, yard, yard_bound=False):
    for k, v in got.items():
        if k not in ("x", "used", "log_inv_temp"):
            assert bool(torch.isfinite(v).all()), (case, k)
    err = _errors(got, ref)
    yerr = _errors({k: yard[k] for k in err}, ref)
    bounds = _base_bounds(ref)
    if yard_bound:
        cap = _base_bounds(ref, 7.0)
        bounds = {k: min(4.0 * yerr[k], cap[k]) for k in err}
    bad = []
    for k in err:
        bad += _report(case, k, err[k], yerr.get(k), bounds[k])
    if "used" in got:
        assert torch.equal(got["used"].cpu(), ref["used"]), (case, "used")
    return bad


def _both_paths(dev, case, c, temperature=0.07, yard=False, **kw):
    mod = _module_run(dev, c, temperature, **kw)
    args = (c["A"], c["B"], c["ids"], c["bank"], c["bank_ids"], c["neg_idx"], temperature)
    ref = nc.neg_loss_reference(*args, log_inv_temp=mod.pop("log_inv_temp", None), **kw)
    y = nc.neg_loss_reference(*args, dtype=torch.float32, **kw)
    bad = _check(case + " module", mod, ref, y, yard)
    fwd = _ops_run(dev, c, temperature, **kw)
    bad += _check(case + " forward", fwd, ref, y, yard)
    return bad, mod, fwd, ref


def _same_bits(a, b, keys=None):
    for k in keys or a:
        assert torch.equal(a[k], b[k]) or (a[k].dtype.is_floating_point and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))), k


# ------------------------------------------------------------------------------------------------------------ 1: the sweep
@pytest.mark.parametrize("shape", nc.SHAPE_SWEEP, ids=lambda s: "x".join(map(str, s)))
def test_neg_loss_shape_sweep(dev, shape):
    """One row (no in-batch negative: the denominator is the extras alone) to 8 x 8 tiles; E at one to three 16-byte pieces per lane
    and off a whole piece; M below one group of four, off a group, off a chunk and at the limit of 1024."""
    c = _case(shape)
    bad, mod, fwd, ref = _both_paths(dev, "sweep " + "x".join(map(str, shape)), c)
    assert not bad, bad
    if shape[0] == 1:
        plain = _plain_run(dev, c)
        print(f"PARITY|sweep 1x4x3x2|plain loss|{float(plain['loss']):.4f}|-|-")
        print(f"PARITY|sweep 1x4x3x2|extended loss|{float(mod['loss']):.4f}|-|-")
        # the plain loss is -l + log(e^l) = 0 exactly; the extended one is log(1 + sum_n e^{x_n - l}), a thousand bounds above it
        assert float(plain["loss"]) == 0.0 and float(ref["loss"]) > 1000 * lc.TOL_LOSS and int(mod["used"][0]) == 2
    if shape == nc.MAIN:                                  # the extras are no rounding matter: a test that loses them cannot pass
        plain = lc.loss_reference(c["A"], c["B"], c["ids"])
        assert float(ref["loss"]) - float(plain["loss"]) > 0.1


@pytest.mark.parametrize("shape", [(5, 1000, 40, 6), (5, 1028, 40, 6)], ids=lambda s: "x".join(map(str, s)))
def test_neg_loss_wide_rows(dev, shape):
    """The two forward paths the sweep's widths do not reach: four 16-byte pieces per lane with a partial last piece (E = 1000), and
    past 1024 the kernel that streams the rows piece by piece (E = 1028: five column blocks in the backward, the last of one lane)."""
    bad, _, _, _ = _both_paths(dev, "wide rows " + "x".join(map(str, shape)), _case(shape))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ 2: every slot empty
@pytest.mark.parametrize("shape", [(130, 100, 1000, 40), (64, 512, 6000, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_all_slots_empty_is_the_plain_call(dev, shape):
    c = dict(_case(shape))
    c["neg_idx"] = torch.full_like(c["neg_idx"], -1)
    mod, plain = _module_run(dev, c), _plain_run(dev, c)
    fwd = _ops_run(dev, c)
    _same_bits(mod, plain, ("loss", "dA", "dB"))
    _same_bits(fwd, plain, ("loss", "lse_row"))
    assert int(mod["used"].abs().max()) == 0 and int(fwd["used"].abs().max()) == 0
    assert bool(torch.isneginf(fwd["x"]).all())


# ------------------------------------------------------------------------------------------------------------ 3: slots that must not count
@pytest.mark.parametrize("nan_rows", [False, True], ids=["finite", "nan_rows"])
def test_inadmissible_slots_equal_empty_slots(dev, nan_rows):
    """A third of the slots overwritten with -1, -7, N, 2^40, rows under the anchor's own id and rows under another batch row's id:
    every output has the bits of the run with those slots at -1 - also with NaN bank rows behind the id-masked slots."""
    Bg, E, N, M = nc.MAIN
    c = dict(_case(nc.MAIN))
    g = torch.Generator().manual_seed(3)
    hit = torch.rand(Bg, M, generator=g) < 1 / 3
    kind = torch.randint(0, 6, (Bg, M), generator=g)
    n_own = min(Bg, N // 2)                                                   # bank rows 0 .. n_own - 1 carry the batch's ids
    own = (torch.arange(Bg) // 5 * 5)[:, None].expand(Bg, M)                  # a bank row under the anchor's own id
    other = ((torch.arange(Bg)[:, None] + 5 + torch.randint(0, Bg - 10, (Bg, M), generator=g)) % n_own)   # ... under another row's id
    assert bool((c["bank_ids"][own] == c["ids"][:, None]).all()) and bool((c["bank_ids"][other] != c["ids"][:, None]).all())
    junk = torch.stack([torch.full((Bg, M), v, dtype=torch.int64) for v in (-1, -7, N, 2 ** 40)] + [own, other])
    dirty, clean = c["neg_idx"].clone(), c["neg_idx"].clone()
    dirty[hit] = junk.gather(0, kind[None])[0][hit]
    clean[hit] = -1
    bank = c["bank"].clone()
    if nan_rows:
        bank[:n_own] = float("nan")                     # every row an id-masked slot points at
        clean[(clean >= 0) & (clean < n_own)] = -1      # the true lists hold such rows too: id-masked in one run, empty in the other
    outs = []
    for idx in (dirty, clean):
        cc = dict(c, neg_idx=idx, bank=bank)
        outs.append((_module_run(dev, cc), _ops_run(dev, cc)))
    for k in (0, 1):
        _same_bits(outs[0][k], outs[1][k])
        for name, v in outs[0][k].items():
            if name != "x":
                assert bool(torch.isfinite(v.float()).all()), name
    ref = nc.neg_loss_reference(c["A"], c["B"], c["ids"], bank, c["bank_ids"], dirty)
    assert torch.equal(outs[0][1]["used"].cpu(), ref["used"])
    assert lc.max_abs_err(outs[0][0]["loss"], ref["loss"]) <= lc.TOL_LOSS * max(1.0, abs(float(ref["loss"])))


# ------------------------------------------------------------------------------------------------------------ 4: variants
@pytest.mark.parametrize("name", ["margin", "dcl", "a2b", "margin_dcl_trainT"])
def test_neg_loss_variants(dev, name):
    """margin / dcl / b2a=False / trainable temperature (dT against fp64) at Bg = 130"""
    bad, _, _, _ = _both_paths(dev, f"variant {name}", _case(nc.MAIN), **lc.VARIANTS[name])
    assert not bad, bad


def test_neg_loss_needs_a2b(dev):
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    c = _case(nc.MAIN)
    crit = MaskedContrastiveLoss(a2b=False).to(dev)
    with pytest.raises(ValueError, match="a2b"):
        crit(c["A"].to(dev), c["B"].to(dev), c["ids"].to(dev), bank=c["bank"].to(dev), bank_ids=c["bank_ids"].to(dev),
             neg_idx=c["neg_idx"].to(dev))


# ------------------------------------------------------------------------------------------------------------ 5: no in-batch negative
def test_dcl_all_ids_equal_extras_alone(dev):
    """dcl with one id for the whole batch: every in-batch partial is -inf; four valid slots per anchor keep every output finite."""
    Bg, E, N, M = 70, 100, 200, 6
    A, Bm = lc.make_pair(Bg, E, seed=70)
    ids = torch.zeros(Bg, dtype=torch.int64)
    bank, _ = nc.make_bank(Bm, None, N, seed=71)
    bank_ids = 1 + torch.arange(N, dtype=torch.int64)
    neg_idx = torch.full((Bg, M), -1, dtype=torch.int64)
    neg_idx[:, :4] = nc.true_lists(A, bank, ids, bank_ids, 4)
    c = {"A": A, "B": Bm, "ids": ids, "bank": bank, "bank_ids": bank_ids, "neg_idx": neg_idx}
    mod = _module_run(dev, c, dcl=True, b2a=False)
    args = (A, Bm, ids, bank, bank_ids, neg_idx)
    ref = nc.neg_loss_reference(*args, dcl=True, b2a=False)
    y = nc.neg_loss_reference(*args, dcl=True, b2a=False, dtype=torch.float32)
    bad = _check("dcl one id module", mod, ref, y)
    bad += _check("dcl one id forward", _ops_run(dev, c, dcl=True, b2a=False), ref, y)
    assert not bad, bad
    assert int(mod["used"].min()) == 4 and int(mod["used"].max()) == 4


# ------------------------------------------------------------------------------------------------------------ 6: temperature 0.01
def test_neg_loss_temperature_001(dev):
    bad, _, _, _ = _both_paths(dev, "T=0.01", _case(nc.MAIN), temperature=0.01, yard=True)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ 7: repeatability
@pytest.mark.parametrize("shape", [(130, 100, 1000, 40), (200, 64, 5000, 256)], ids=lambda s: "x".join(map(str, s)))
def test_repeatable_bits(dev, shape):
    c = _case(shape)
    first = (_module_run(dev, c), _ops_run(dev, c))
    again = (_module_run(dev, c), _ops_run(dev, c))
    torch.randn(257, 129, device=dev) @ torch.randn(129, 65, device=dev)           # an unrelated launch in between
    third = (_module_run(dev, c), _ops_run(dev, c))
    for other in (again, third):
        for k in (0, 1):
            _same_bits(first[k], other[k])


# ------------------------------------------------------------------------------------------------------------ 8: operand forms
def test_strided_bank_and_sliced_lists(dev):
    """A bank that is a row-strided view is read in place; a ``neg_idx`` that is a column slice is copied: both give the contiguous
    call's bits.  A bank that requires grad is refused."""
    c = _case(nc.MAIN)
    Bg, E, N, M = nc.MAIN
    base = (_module_run(dev, c), _ops_run(dev, c))
    wide = torch.full((N, E + 28), float("nan"), device=dev)
    wide[:, :E] = c["bank"].to(dev)
    view = wide[:, :E]
    lists = torch.full((Bg, M + 3), 7, dtype=torch.int64, device=dev)
    lists[:, 1: M + 1] = c["neg_idx"].to(dev)
    sl = lists[:, 1: M + 1]
    assert not view.is_contiguous() and not sl.is_contiguous()
    _same_bits(_ops_run(dev, c, bank=view, neg_idx=sl), base[1])
    _same_bits(_module_run(dev, dict(c, bank=view, neg_idx=sl)), base[0])
    every_other = torch.zeros(2 * N, E, device=dev)
    every_other[::2] = c["bank"].to(dev)
    _same_bits(_ops_run(dev, c, bank=every_other[::2]), base[1])
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    with pytest.raises(ValueError, match="requires_grad"):
        MaskedContrastiveLoss().to(dev)(c["A"].to(dev), c["B"].to(dev), c["ids"].to(dev), bank=c["bank"].to(dev).requires_grad_(True),
                                        bank_ids=c["bank_ids"].to(dev), neg_idx=c["neg_idx"].to(dev))


# ------------------------------------------------------------------------------------------------------------ 9: through the miner
def test_end_to_end_through_the_miner(dev):
    import speechclip_plus_amd as sc
    c = dict(_case((130, 100, 1000, 40)))
    A, ids = c["A"].to(dev), c["ids"].to(dev)
    index = sc.GalleryIndex(c["bank"].to(dev), ids=c["bank_ids"].to(dev))
    neg_idx = sc.hard_negatives(A, index, ids, None, 32)[1]
    c["neg_idx"] = neg_idx.cpu()
    mod = _module_run(dev, c)
    args = (c["A"], c["B"], c["ids"], c["bank"], c["bank_ids"], c["neg_idx"])
    ref, y = nc.neg_loss_reference(*args), nc.neg_loss_reference(*args, dtype=torch.float32)
    bad = _check("miner module", mod, ref, y)
    assert not bad, bad
    holds_batch_image = ((c["neg_idx"] >= 0) & (c["neg_idx"] < 130)).any(1)          # bank rows 0 .. 129 are the batch's images
    assert bool((c["neg_idx"] >= 0).all())
    assert bool(holds_batch_image.any())
    used = mod["used"].cpu()
    assert bool((used[holds_batch_image] < 32).all()) and bool((used[~holds_batch_image] == 32).all())


# ------------------------------------------------------------------------------------------------------------ 10: the model
def _bare_model(dev):
    """compute_loss reads ``config``, ``criterion`` and the bank only: no encoder is built"""
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    model = KWClip_GeneralTransformer.__new__(KWClip_GeneralTransformer)
    torch.nn.Module.__init__(model)
    model.config = base_parallel_config()
    model.criterion = MaskedContrastiveLoss(**model.config.cl_loss.args).to(dev)
    return model


def test_model_compute_loss_with_a_bank(dev):
    import speechclip_plus_amd as sc
    c = _case((130, 100, 1000, 40))
    model = _bare_model(dev)
    feats = {"id": c["ids"].to(dev), "image_feat": c["B"].to(dev), "parallel_audio_feat": c["A"].to(dev)}
    model.train()
    plain = model.compute_loss(feats)["loss"]
    model.set_negative_bank(c["bank"].to(dev) * 3.0, c["bank_ids"].to(dev), 32)          # the setter normalises the rows
    rows, bank_ids, index, k = model._neg_bank
    assert k == 32 and lc.max_abs_err(rows, c["bank"]) < 1e-6
    with_bank = model.compute_loss(feats)["loss"]
    neg_idx = sc.hard_negatives(feats["parallel_audio_feat"], index, feats["id"], None, 32)[1]
    by_hand = model.criterion(feats["parallel_audio_feat"], feats["image_feat"], feats["id"], bank=rows, bank_ids=bank_ids, neg_idx=neg_idx)
    w = float(model.config.model_settings.get("parallel_objective_weight", 0.0))
    by_hand = by_hand if w == 1.0 else w * by_hand
    assert float(with_bank) == float(by_hand) and float(with_bank) != float(plain)
    model.eval()
    assert float(model.compute_loss(feats)["loss"]) == float(plain)
    model.train()
    model.clear_negative_bank()
    assert float(model.compute_loss(feats)["loss"]) == float(plain)
