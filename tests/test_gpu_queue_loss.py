"""The contrastive loss with a cross-batch queue (csrc/infonce_queue.hip: sc_infonce_queue_fwd / sc_infonce_queue_grad under
MaskedContrastiveLoss(..., queue_A=, queue_B=, queue_ids=) and model.set_negative_queue) against fp64.

Inputs and the reference come from tests/queue_loss_cases.py; the fp64 expression is evaluated on the device.  Bounds (docs/parity.md,
"Contrastive loss with a cross-batch queue"): each is the larger of the project's own constant for this arithmetic - x 2e-5,
log-sum-exps 5e-5, loss 2e-5 max(1, |loss|), all absolute; gradients max |g - g64| / max |g64| <= 2e-4 - and 4 x the error of the
fp32 form of the same expression on the CPU against fp64, computed here for the case at hand.  ``used`` and everything stated "bit
for bit" is compared with ==.  Every figure is printed as a ``PARITY|case|quantity|error|yardstick|bound`` line before anything is
asserted."""
import dataclasses
import functools

import pytest
import torch

import loss_cases as lc
import queue_loss_cases as qc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SWEEP_VARIANTS = dict(qc.VARIANTS, no_ids={})


def _ops():
    from speechclip_plus_amd import ops
    return ops


def _report(case, quantity, err, yardstick, bound):
    print(f"PARITY|{case}|{quantity}|{err:.3e}|{yardstick:.3e}|{bound:.3e}")
    return [] if err <= bound else [f"{case}: {quantity} error {err:.3e} > bound {bound:.3e} (yardstick {yardstick:.3e})"]


@functools.lru_cache(maxsize=None)
def _case(shape, with_ids=True):
    return qc.make_case(*shape, with_ids=with_ids)


def _to(t):
    return t.to(DEV) if t is not None else None


def _args(c):
    return c["A"], c["B"], c["ids"], c["queue_A"], c["queue_B"], c["queue_ids"]


def _module_run(c, temperature=0.07, trainable=True, queue=True, **kw):
    """MaskedContrastiveLoss(...)(A, B, ids, queue_A=, queue_B=, queue_ids=) and backward() -> loss, dA, dB, used_A, used_B, [dT,
    log_inv_temp]; ``queue`` False leaves the keywords out"""
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    crit = MaskedContrastiveLoss(temperature=temperature, temperature_trainable=trainable, **kw).to(DEV)
    a, b = c["A"].to(DEV).requires_grad_(True), c["B"].to(DEV).requires_grad_(True)
    q = dict(queue_A=_to(c["queue_A"]), queue_B=_to(c["queue_B"]), queue_ids=_to(c["queue_ids"])) if queue else {}
    loss = crit(a, b, _to(c["ids"]), **q)
    loss.backward()
    out = {"loss": loss.detach(), "dA": a.grad, "dB": b.grad}
    if queue:
        out.update(used_A=crit.last_queue_used[0], used_B=crit.last_queue_used[1])
    if trainable:
        out.update(dT=crit.temperature.grad, log_inv_temp=crit.temperature.detach())
    return out


def _ops_run(c, temperature=0.07, margin=0.0, dcl=False, a2b=True, b2a=True):
    """ops.infonce_fwd, the score products, then ops.infonce_queue_fwd -> loss, lse_row, lse_col (extended), x_A, x_B, used_A, used_B"""
    ops = _ops()
    it = torch.full((1,), 1.0 / temperature, device=DEV)
    A, Bm, ids = c["A"].to(DEV), c["B"].to(DEV), _to(c["ids"])
    loss, logits, lr, lcol = ops.infonce_fwd(A, Bm, ids, it, margin, dcl, a2b, b2a)
    x_A = ops.queue_scores(A, c["queue_B"].to(DEV)) if a2b else None
    x_B = ops.queue_scores(Bm, c["queue_A"].to(DEV)) if b2a else None
    loss, lr, lcol, uA, uB = ops.infonce_queue_fwd(x_A, x_B, ids, _to(c["queue_ids"]), it, loss, lr, lcol, logits, A.shape[1], a2b, b2a)
    out = {"loss": loss.reshape(()), "lse_row": lr, "lse_col": lcol, "used_A": uA, "used_B": uB}
    if a2b:
        out["x_A"] = x_A
    if b2a:
        out["x_B"] = x_B
    return out


def _errors(got, ref):
    e = {}
    for k in got:
        if k in ("dA", "dB", "dT"):
            e[k] = qc.grad_err(got[k], ref[k])
        elif k in ("loss", "lse_row", "lse_col"):
            e[k] = lc.max_abs_err(got[k], ref[k])
        elif k in ("x_A", "x_B"):
            e[k] = qc.x_err(got[k], ref[k])
    return e


def _floors(ref):
    return {"loss": lc.TOL_LOSS * max(1.0, abs(float(ref["loss"]))), "x_A": lc.TOL_LOGITS, "x_B": lc.TOL_LOGITS, "lse_row": lc.TOL_LSE,
            "lse_col": lc.TOL_LSE, "dA": lc.TOL_GRAD, "dB": lc.TOL_GRAD, "dT": lc.TOL_GRAD}


def _check(case, got, ref, yard):
    for k, v in got.items():
        if k not in ("x_A", "x_B", "used_A", "used_B", "log_inv_temp"):
            assert bool(torch.isfinite(v).all()), (case, k)
    err = _errors(got, ref)
    yerr = _errors({k: yard[k] for k in err}, ref)
    floors = _floors(ref)
    bad = []
    for k in err:
        bad += _report(case, k, err[k], yerr[k], max(floors[k], 4.0 * yerr[k]))
    for k in ("used_A", "used_B"):
        if k in got:
            assert torch.equal(got[k].cpu(), ref[k].cpu()), (case, k)
    return bad


# ------------------------------------------------------------------------------------------------------------ 1: the sweep
@pytest.mark.parametrize("variant", list(SWEEP_VARIANTS))
@pytest.mark.parametrize("temperature", qc.TEMPERATURES)
@pytest.mark.parametrize("shape", qc.SHAPE_SWEEP, ids=lambda s: "x".join(map(str, s)))
def test_sweep_against_fp64(shape, temperature, variant):
    """x, both extended statistics, the loss, used_A / used_B (ops level) and the loss, dA, dB, dT (autograd through the module, the
    temperature trainable) against the fp64 expression on the device"""
    kw = SWEEP_VARIANTS[variant]
    c = _case(shape, with_ids=variant != "no_ids")
    case = f"{'x'.join(map(str, shape))} T{temperature} {variant}"
    mod = _module_run(c, temperature, **kw)
    lit = mod.pop("log_inv_temp")
    ref = qc.queue_loss_reference(*_args(c), temperature, trainable=True, log_inv_temp=lit, device=DEV, **kw)
    yard = qc.queue_loss_reference(*_args(c), temperature, trainable=True, log_inv_temp=lit, dtype=torch.float32, **kw)
    bad = _check(case + " module", mod, ref, yard)
    # the ops-level forward runs at the constant temperature 1 / T, the module at exp(fp32 log(1 / T)): its own reference
    ref0 = qc.queue_loss_reference(*_args(c), temperature, device=DEV, **kw)
    yard0 = qc.queue_loss_reference(*_args(c), temperature, dtype=torch.float32, **kw)
    bad += _check(case + " forward", _ops_run(c, temperature, **kw), ref0, yard0)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ 2: bit for bit
def _same_bits(x, y):
    assert set(x) == set(y)
    for k in x:
        assert torch.equal(x[k], y[k]), k


@pytest.mark.parametrize("kw", [{}, dict(margin=0.2, dcl=True), dict(b2a=False), dict(a2b=False)], ids=["default", "margin_dcl", "a2b", "b2a"])
def test_an_empty_queue_is_the_plain_call(kw):
    c = _case((130, 100, 1000, 40))
    plain = _module_run(c, queue=False, **kw)
    empty = dict(c, queue_A=c["queue_A"][:0], queue_B=c["queue_B"][:0], queue_ids=c["queue_ids"][:0])
    got = _module_run(empty, **kw)
    assert int(got.pop("used_A").sum()) == 0 and int(got.pop("used_B").sum()) == 0
    _same_bits(got, plain)
    assert float(plain["dA"].abs().max()) > 0 and float(plain["dT"].abs()) > 0
    # every entry masked (one id everywhere): the kernels run, and still leave the plain call's loss and statistics
    if not kw.get("dcl"):
        one = dict(c, ids=torch.full_like(c["ids"], 7), queue_ids=torch.full_like(c["queue_ids"], 7))
        ops = _ops()
        it = torch.full((1,), 1.0 / 0.07, device=DEV)
        o = {k: v for k, v in kw.items() if k in ("a2b", "b2a")}
        p = ops.infonce_fwd(one["A"].to(DEV), one["B"].to(DEV), one["ids"].to(DEV), it, kw.get("margin", 0.0), False, **o)
        got = _ops_run(one, **kw)
        assert torch.equal(got["loss"], p[0].reshape(())) and torch.equal(got["lse_row"], p[2]) and torch.equal(got["lse_col"], p[3])
        assert int(got["used_A"].sum()) == 0 and int(got["used_B"].sum()) == 0
        for k in ("x_A", "x_B"):
            assert k not in got or bool(torch.isneginf(got[k]).all())


def test_a_queue_of_one_anchors_id_leaves_that_anchor_alone():
    c = dict(_case((130, 100, 1000, 40)))
    anchor = 17
    c["ids"] = torch.arange(130)                                       # every anchor its own id: only row 17 is masked
    c["queue_ids"] = torch.full_like(c["queue_ids"], anchor)
    ops = _ops()
    it = torch.full((1,), 1.0 / 0.07, device=DEV)
    plain = ops.infonce_fwd(c["A"].to(DEV), c["B"].to(DEV), c["ids"].to(DEV), it)
    got = _ops_run(c)
    others = torch.arange(130) != anchor
    for k, p in (("lse_row", plain[2]), ("lse_col", plain[3])):
        assert float(got[k][anchor]) == float(p[anchor]), k
        assert bool((got[k].cpu()[others] > p.cpu()[others]).all()), k
    for k in ("used_A", "used_B"):
        assert int(got[k][anchor]) == 0 and bool((got[k].cpu()[others] == 1000).all()), k
    for k in ("x_A", "x_B"):
        assert bool(torch.isneginf(got[k][anchor]).all()) and bool(torch.isfinite(got[k].cpu()[others]).all()), k


@pytest.mark.parametrize("shape", [(65, 768, 4097, 50), (256, 512, 16384, 6000)], ids=lambda s: "x".join(map(str, s)))
def test_two_calls_give_the_same_bits(shape):
    c = _case(shape)
    _same_bits(_module_run(c, margin=0.2), _module_run(c, margin=0.2))
    _same_bits(_ops_run(c), _ops_run(c))


def test_the_backward_runs_once_and_a_one_sided_loss_needs_one_queue():
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    c = _case((5, 8, 3, 3))
    crit = MaskedContrastiveLoss().to(DEV)
    a = c["A"].to(DEV).requires_grad_(True)
    loss = crit(a, c["B"].to(DEV), c["ids"].to(DEV), queue_A=c["queue_A"].to(DEV), queue_B=c["queue_B"].to(DEV), queue_ids=c["queue_ids"].to(DEV))
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="runs once per forward"):   # the scores have become the weights
        loss.backward()
    for kw, own in ((dict(b2a=False), "queue_B"), (dict(a2b=False), "queue_A")):
        both = _module_run(c, **kw)
        one = MaskedContrastiveLoss(temperature_trainable=True, **kw).to(DEV)
        loss = one(c["A"].to(DEV), c["B"].to(DEV), c["ids"].to(DEV), queue_ids=c["queue_ids"].to(DEV), **{own: c[own].to(DEV)})
        assert torch.equal(loss.detach(), both["loss"]), kw
    with pytest.raises(ValueError, match="requires_grad"):
        crit(a, c["B"].to(DEV), c["ids"].to(DEV), queue_A=c["queue_A"].to(DEV), queue_B=c["queue_B"].to(DEV).requires_grad_(True),
             queue_ids=c["queue_ids"].to(DEV))


def test_a_row_strided_queue_is_read_in_place():
    c = _case((130, 100, 1000, 40))
    base = _module_run(c)
    wide = torch.full((1000, 104), float("nan"), device=DEV)           # the ring as a view of wider rows, NaN beside it
    wide[:, :100] = c["queue_B"].to(DEV)
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    crit = MaskedContrastiveLoss(temperature_trainable=True).to(DEV)
    a, b = c["A"].to(DEV).requires_grad_(True), c["B"].to(DEV).requires_grad_(True)
    loss = crit(a, b, c["ids"].to(DEV), queue_A=c["queue_A"].to(DEV), queue_B=wide[:, :100], queue_ids=c["queue_ids"].to(DEV))
    loss.backward()
    assert torch.equal(loss.detach(), base["loss"]) and torch.equal(a.grad, base["dA"]) and torch.equal(b.grad, base["dB"])


# ------------------------------------------------------------------------------------------------------------ 3: the model
def _bare_model(E):
    """compute_loss reads ``config``, ``criterion`` and the rings only: no encoder is built"""
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    model = KWClip_GeneralTransformer.__new__(KWClip_GeneralTransformer)
    torch.nn.Module.__init__(model)
    model.config = base_parallel_config()
    model.criterion = MaskedContrastiveLoss(**model.config.cl_loss.args).to(DEV)
    model._device, model.subword_embd_dim = DEV, E
    return model


def _feats(shape, seed):
    c = qc.make_case(*shape, seed=seed)
    return {"id": c["ids"].to(DEV), "image_feat": c["B"].to(DEV), "parallel_audio_feat": c["A"].to(DEV).requires_grad_(True)}


def test_model_compute_loss_with_a_queue():
    shape = (130, 100, 0, 40)
    model = _bare_model(100)
    first, second = _feats(shape, 1), _feats(shape, 2)
    model.train()
    plain1 = model.compute_loss(first)["loss"]
    model.set_negative_queue(300)
    q = model._neg_queue
    for ring in (q["image"], q["speech"]["parallel"]):                 # rows beyond n_valid reach nothing
        ring.fill_(float("nan"))
    got1 = model.compute_loss(first)["loss"]
    got1.backward()
    assert torch.equal(got1, plain1) and int(model.criterion.last_queue_used[0].sum()) == 0          # the first call sees an empty queue
    got2 = model.compute_loss(second)["loss"]
    got2.backward()
    assert (q["head"], q["n_valid"]) == (130, 130) and bool(torch.isfinite(got2))
    assert bool(torch.isfinite(second["parallel_audio_feat"].grad).all())
    a = second["parallel_audio_feat"].detach().clone().requires_grad_(True)
    by_hand = model.criterion(a, second["image_feat"], second["id"], queue_A=first["parallel_audio_feat"].detach(),
                              queue_B=first["image_feat"], queue_ids=first["id"])
    by_hand.backward()
    assert torch.equal(got2, by_hand) and torch.equal(a.grad, second["parallel_audio_feat"].grad)
    plain2 = model.criterion(second["parallel_audio_feat"].detach(), second["image_feat"], second["id"]).detach()
    assert float(got2.detach()) > float(plain2) + 1e-3
    model.eval()
    assert torch.equal(model.compute_loss(second)["loss"].detach(), plain2) and (q["head"], q["n_valid"]) == (130, 130)
    model.train()
    got3 = model.compute_loss(first)["loss"]                           # 260 rows: first's and second's
    assert (q["head"], q["n_valid"]) == (260, 260) and bool(torch.isfinite(got3))
    got4 = model.compute_loss(second)["loss"]                          # 390 rows wrap: the ring is full, NaN rows all overwritten
    assert (q["head"], q["n_valid"]) == (90, 300) and bool(torch.isfinite(got4))
    assert bool(torch.isfinite(q["image"]).all()) and bool(torch.isfinite(q["speech"]["parallel"]).all())
    model.clear_negative_queue()
    assert torch.equal(model.compute_loss(first)["loss"], plain1)


def test_two_trainer_steps_on_a_two_term_recipe():
    """hybrid+ at reduced depth: one speech ring per branch term, two ContrastiveTrainer steps with a queue - no in-place-modification
    error, a finite loss, the rings filled from the gathered batch"""
    from speechclip_plus_amd import set_dropout, KWClip_GeneralTransformer, hybrid_plus_large_config, random_hubert_state_dict
    from speechclip_plus_amd.speech_encoder import ARCHS
    from speechclip_plus_amd.train import ContrastiveTrainer
    arch = dataclasses.replace(ARCHS["hubert_large_ll60k"], layers=1)
    torch.manual_seed(5)
    cfg = hybrid_plus_large_config()
    cfg.audio_encoder.max_audio_len = -1
    cfg.clip.layers = 1
    model = set_dropout(KWClip_GeneralTransformer(cfg, device="cuda:0", hubert_state_dict=random_hubert_state_dict(arch, seed=5),
                                                  hubert_arch=arch).train(), False)
    keys = set(model.state_dict().keys())
    model.set_negative_queue(6)
    q = model._neg_queue
    assert set(q["speech"]) == {"cascaded", "parallel"} and q["image"].shape == (6, 768) and set(model.state_dict().keys()) == keys
    g = torch.Generator().manual_seed(6)
    lens = [12000, 9000, 12000, 8000]
    wav = torch.zeros(4, max(lens))
    for b, n in enumerate(lens):
        wav[b, :n] = torch.randn(n, generator=g) * 0.5
    batch = {"wav": wav.cuda(), "wav_len": torch.tensor(lens), "image": torch.randn(4, 768, generator=g).cuda(),
             "id": torch.tensor([0, 0, 1, 2]).cuda()}
    trainer = ContrastiveTrainer(model)
    l1 = trainer.step(batch)
    assert (q["head"], q["n_valid"]) == (0, 0) and q["pending"] is not None
    l2 = trainer.step(batch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(l1)) and bool(torch.isfinite(l2)) and (q["head"], q["n_valid"]) == (4, 4)
    used_A, used_B = model.criterion.last_queue_used
    assert used_A.cpu().tolist() == [2, 2, 3, 3] and used_B.cpu().tolist() == [2, 2, 3, 3]           # the queue holds ids 0, 0, 1, 2
    assert q["ids"][:4].cpu().tolist() == [0, 0, 1, 2]
    casc, par = q["speech"]["cascaded"][:4], q["speech"]["parallel"][:4]
    for ring in (casc, par, q["image"][:4]):
        assert float((ring.norm(dim=1) - 1).abs().max()) < 1e-4       # the unit rows of step 1
    assert not torch.equal(casc, par)
    l3 = trainer.step(batch)                                           # rows 4, 5 and 0, 1: the batch straddles the end
    assert bool(torch.isfinite(l3)) and (q["head"], q["n_valid"]) == (2, 6)
