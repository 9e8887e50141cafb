"""SigmoidContrastiveLoss on the HIP kernels of csrc/sigmoid_loss.hip (sc_sigmoid_loss_fwd / sc_sigmoid_loss_grad) against fp64.

Inputs, the fp64 reference (the formulas, no autograd) and the bounds come from tests/sigmoid_loss_cases.py; the bounds are the project's
own (tests/loss_cases.py) carried over: scores TOL_X(t) = 2e-5 max(1, 0.07 t); |loss - loss64| <= TOL_X(t) sum |g64| + 2e-5 max(1, loss64);
max |G / (gscale t) - g64| <= 2e-4 max |g64| with every ignored entry exactly 0; dA, dB max |d - d64| / max |d64| <= 2e-4; d t and d b
2e-4 of the sum of their absolute summands; the counts equal the reference's integers.  Everything stated "bit for bit" is compared with
torch.equal.  Every figure is printed as a ``PARITY|case|quantity|error|bound`` line before anything is asserted."""
import functools
import math

import pytest
import torch

import loss_cases as lc
import sigmoid_loss_cases as sg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _report(case, quantity, err, bound):
    print(f"PARITY|{case}|{quantity}|{err:.3e}|{bound:.3e}")
    return [] if err <= bound else [f"{case}: {quantity} error {err:.3e} > bound {bound:.3e}"]


def _to(t):
    return t.to(DEV) if t is not None else None


@functools.lru_cache(maxsize=None)
def _ref(shape, idset, mode, t, b, widen=None):
    """fp64 at the fp32 value of t that the kernels see; computed once per case and shared.  ``widen``: the inputs rounded to that dtype first"""
    A, Bm = sg.inputs(shape)
    if widen is not None:
        A, Bm = A.to(widen).float(), Bm.to(widen).float()
    return sg.reference(A, Bm, sg.make_ids(idset, shape[0]), t, b, mode)


def _crit(t, b, mode="ignore", learnable=True):
    from speechclip_plus_amd.losses import SigmoidContrastiveLoss
    crit = SigmoidContrastiveLoss(temperature=1.0 / t, bias=b, learnable=learnable, same_id=mode).to(DEV)
    return crit, float(crit.logit_scale.detach().exp())             # torch's own exp on the device: the t of the forward, to the bit


def _module_run(A, Bm, ids, t, b, mode="ignore", scale=1.0, dtype=None):
    """SigmoidContrastiveLoss(...)(A, Bm, ids) and backward() -> dict(loss, dA, dB, dt, db, t, counts); dt = d logit_scale / t"""
    crit, t_used = _crit(t, b, mode)
    a, bm = (x.to(DEV) if dtype is None else x.to(DEV).to(dtype) for x in (A, Bm))
    a.requires_grad_(True), bm.requires_grad_(True)
    loss = crit(a, bm, _to(ids))
    (loss if scale == 1.0 else scale * loss).backward()
    return {"loss": loss.detach(), "dA": a.grad, "dB": bm.grad, "dls": crit.logit_scale.grad, "db": crit.logit_bias.grad,
            "dt": crit.logit_scale.grad.double() / t_used, "t": t_used, "counts": crit.last_counts}


def _ops_run(A, Bm, ids, t, b, mode="ignore", gscale=1.0):
    """ops by hand -> dict(loss, s, x, counts, G, g, dscale_part, dbias_part, dA, dB, dt, db)"""
    from speechclip_plus_amd import ops
    a, bm, ids = A.to(DEV), Bm.to(DEV), _to(ids)
    tt, bb, gs = (torch.tensor([v], dtype=torch.float32, device=DEV) for v in (t, b, gscale))
    loss, s, counts = ops.sigmoid_loss_fwd(a, bm, ids, tt, bb, mode)
    G, dsp, dbp = ops.sigmoid_loss_grad(s, ids, gs, tt, bb, mode)
    return {"loss": loss.reshape(()), "s": s, "x": float(tt) * s.double() + b, "counts": counts, "G": G, "g": G.double() / (gscale * float(tt)),
            "dscale_part": dsp, "dbias_part": dbp, "dA": ops.sgemm_mfma(G, bm, b_kmajor=True),
            "dB": ops.sgemm_mfma(G, a, a_kmajor=True, b_kmajor=True), "dt": dsp.sum(), "db": dbp.sum()}


def _check(case, got, ref, t, keys):
    bound, err = sg.bounds(ref, t), sg.errors({k: got[k] for k in keys}, ref)
    fails = []
    for k in keys:
        fails += _report(case, k, err[k], bound[k])
    return fails


@pytest.mark.parametrize("case", sg.CASES, ids=sg.case_id)
def test_loss_counts_and_gradients_vs_fp64(case):
    """through ``ops`` (scores, loss, G element-wise, the ignored entries, counts, d t, d b, the two products) and through the module
    (loss, dA, dB, d t, d b in their own dtypes and shapes), at the t each of them sees"""
    shape, idset, mode, setting = case
    B = shape[0]
    A, Bm = sg.inputs(shape)
    ids = sg.make_ids(idset, B)
    t, b = sg.SETTINGS[setting]
    name = sg.case_id(case)
    ref = _ref(shape, idset, mode, t, b)
    got = _ops_run(A, Bm, ids, t, b, mode)
    fails = _check(name + "/ops", got, ref, t, ("x", "loss", "g", "dA", "dB", "dt", "db"))
    _, w, same = sg.pair_tables(B, ids, mode)
    ignored = got["G"].cpu()[w == 0]
    print(f"PARITY|{name}/ops|ignored entries of G|{float(ignored.abs().max()) if ignored.numel() else 0.0:.3e}|0.000e+00")
    print(f"PARITY|{name}/ops|counts|{got['counts'].tolist()}|{ref['counts'].tolist()}")
    mod = _module_run(A, Bm, ids, t, b, mode)
    mref = _ref(shape, idset, mode, mod["t"], b)
    # exp(log t) in fp32: log t <= 4.61 is stored to half an ulp, 2.4e-7, which is relative in t; the exp adds a few ulp of t, 6e-8 each
    fails += _report(name, "t of the module", abs(mod["t"] - t), 6e-7 * t)
    fails += _check(name + "/module", mod, mref, mod["t"], ("loss", "dA", "dB", "dt", "db"))
    print(f"PARITY|{name}/module|counts|{mod['counts'].tolist()}|{mref['counts'].tolist()}")
    assert not fails, "\n".join(fails)
    assert ignored.numel() == int(ref["counts"][2]) and (ignored.numel() == 0 or float(ignored.abs().max()) == 0.0)
    for c in (got["counts"], mod["counts"]):
        assert c.dtype == torch.int32 and c.shape == (3,) and c.is_cuda and torch.equal(c.cpu().long(), ref["counts"])
    assert mod["loss"].shape == () and mod["dls"].shape == () and mod["db"].shape == () and mod["dA"].dtype == torch.float32
    assert all(bool(torch.isfinite(got[k]).all()) for k in ("loss", "s", "G", "dscale_part", "dbias_part", "dA", "dB"))
    assert all(bool(torch.isfinite(mod[k]).all()) for k in ("loss", "dA", "dB", "dls", "db"))
    if setting == "saturated":
        assert float(got["x"].max()) > 130.0 and not math.isfinite(float(torch.tensor(float(got["x"].max()), dtype=torch.float32).exp()))


def test_the_empty_tile_contributes_exactly_nothing_but_its_diagonal():
    """ids_empty_tile at (200, 512), "ignore": in tile (0, 0) every off-diagonal pair has weight 0 - G is exactly 0 there, the loss is the
    one of the same batch with the tile's off-diagonal dots moved (they cannot reach it), bit for bit"""
    from speechclip_plus_amd import ops
    shape = sg.EMPTY_TILE_SHAPE
    A, Bm = sg.inputs(shape)
    ids = lc.ids_empty_tile(shape[0])
    t, b = sg.SETTINGS["trained"]
    got = _ops_run(A, Bm, ids, t, b)
    tile = got["G"][:lc.TILE, :lc.TILE].cpu()
    off = ~torch.eye(lc.TILE, dtype=torch.bool)
    assert float(tile[off].abs().max()) == 0.0 and float(tile[~off].abs().min()) > 0.0
    # rows 0 .. 63 of B rotated among themselves, except where they meet their own anchor: only ignored pairs of tile (0, 0) move
    s2 = got["s"].clone()
    s2[:lc.TILE, :lc.TILE] = torch.where(off.to(DEV), s2[:lc.TILE, :lc.TILE].roll(1, 1), s2[:lc.TILE, :lc.TILE])
    tt, bb, gs = (torch.tensor([v], dtype=torch.float32, device=DEV) for v in (t, b, 1.0))
    G2, dsp2, dbp2 = ops.sigmoid_loss_grad(s2, _to(ids), gs, tt, bb)
    assert torch.equal(G2, got["G"]) and torch.equal(dsp2, got["dscale_part"]) and torch.equal(dbp2, got["dbias_part"])


def test_wide_int64_ids_are_compared_on_all_64_bits():
    """ids that are negative or differ only above bit 31: the same bits as the same grouping relabelled 0 .. k - 1, in every mode that
    reads them, and not the bits of what a 32-bit compare would see"""
    A, Bm = sg.inputs(sg.WIDE_SHAPE)
    wide = lc.wide_ids(sg.WIDE_SHAPE[0])
    t, b = sg.SETTINGS["trained"]
    keys = ("loss", "dA", "dB", "dls", "db", "counts")
    for mode in ("ignore", "positive"):
        a = _module_run(A, Bm, wide, t, b, mode)
        r = _module_run(A, Bm, lc.relabel(wide), t, b, mode)
        low = _module_run(A, Bm, wide & 0xFFFFFFFF, t, b, mode)
        assert all(torch.equal(a[k], r[k]) for k in keys), mode
        assert not torch.equal(a["loss"], low["loss"]) and not torch.equal(a["counts"], low["counts"]), mode
    for ids in (lc.ids_div5(130), lc.ids_empty_tile(130)):
        a, r = _module_run(A, Bm, ids, t, b), _module_run(A, Bm, lc.relabel(ids + 2 ** 40), t, b)
        assert all(torch.equal(a[k], r[k]) for k in keys)


def test_two_calls_give_identical_bits_and_the_module_is_ops_by_hand():
    for shape, mode in (((65, 68), "ignore"), ((130, 100), "positive"), ((512, 768), "ignore"), ((64, 64), "negative")):
        A, Bm = sg.inputs(shape)
        ids = lc.ids_div5(shape[0])
        t, b = sg.SETTINGS["trained"]
        m1, m2 = _module_run(A, Bm, ids, t, b, mode), _module_run(A, Bm, ids, t, b, mode)
        assert all(torch.equal(m1[k], m2[k]) for k in ("loss", "dA", "dB", "dls", "db", "counts")), (shape, mode)
        o1, o2 = _ops_run(A, Bm, ids, m1["t"], b, mode), _ops_run(A, Bm, ids, m1["t"], b, mode)
        assert all(torch.equal(o1[k], o2[k]) for k in ("loss", "s", "counts", "G", "dscale_part", "dbias_part", "dA", "dB")), (shape, mode)
        assert all(torch.equal(m1[k], o1[k]) for k in ("loss", "dA", "dB", "db", "counts")), (shape, mode)
        assert torch.equal(m1["dls"], o1["dt"] * torch.tensor(m1["t"], dtype=torch.float32, device=DEV))     # torch's exp backward: d t times t


def test_without_ids_the_three_modes_agree_bit_for_bit():
    for shape in ((5, 8), (65, 68), (130, 100)):
        A, Bm = sg.inputs(shape)
        t, b = sg.SETTINGS["trained"]
        runs = [_ops_run(A, Bm, None, t, b, mode) for mode in sg.MODES]
        for r in runs[1:]:
            assert all(torch.equal(r[k], runs[0][k]) for k in ("loss", "s", "counts", "G", "dscale_part", "dbias_part")), shape
        assert runs[0]["counts"].tolist() == [shape[0], shape[0] * (shape[0] - 1), 0]


def test_gscale_two_gives_exactly_twice():
    for shape, mode in (((65, 68), "ignore"), ((130, 100), "positive")):
        A, Bm = sg.inputs(shape)
        ids = lc.ids_div5(shape[0])
        t, b = sg.SETTINGS["trained"]
        one, two = _ops_run(A, Bm, ids, t, b, mode, gscale=1.0), _ops_run(A, Bm, ids, t, b, mode, gscale=2.0)
        assert all(torch.equal(two[k], 2 * one[k]) for k in ("G", "dscale_part", "dbias_part")), shape
        assert torch.equal(two["loss"], one["loss"]) and float(one["G"].abs().max()) > 0
        m1, m2 = _module_run(A, Bm, ids, t, b, mode), _module_run(A, Bm, ids, t, b, mode, scale=2.0)     # ... and so through autograd
        assert all(torch.equal(m2[k], 2 * m1[k]) for k in ("dA", "dB", "dls", "db")), shape


def test_a_second_backward_returns_the_same_numbers():
    A, Bm = sg.inputs((65, 68))
    crit, _ = _crit(*sg.SETTINGS["trained"])
    a, bm = A.to(DEV).requires_grad_(True), Bm.to(DEV).requires_grad_(True)
    loss = crit(a, bm, lc.ids_div5(65).to(DEV))
    first = torch.autograd.grad(loss, (a, bm, crit.logit_scale, crit.logit_bias), retain_graph=True)
    second = torch.autograd.grad(loss, (a, bm, crit.logit_scale, crit.logit_bias))
    assert all(torch.equal(x, y) for x, y in zip(first, second)) and float(first[0].abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_half_precision_features_get_gradients_in_their_dtype(dtype):
    """The features are widened on the way in, so the reference is fp64 on the widened inputs and the fp32 quantities keep their
    bounds; dA and dB are rounded once more, to ``dtype``: at most half an ulp of each entry, eps / 2 of the largest on top of TOL_GRAD."""
    shape, idset, mode = (130, 100), "div5", "ignore"
    A, Bm = sg.inputs(shape)
    t, b = sg.SETTINGS["trained"]
    got = _module_run(A, Bm, sg.make_ids(idset, shape[0]), t, b, mode, dtype=dtype)
    assert got["dA"].dtype == dtype and got["dB"].dtype == dtype and got["dA"].shape == shape
    assert got["dls"].dtype == torch.float32 and got["db"].dtype == torch.float32 and got["loss"].dtype == torch.float32
    ref = _ref(shape, idset, mode, got["t"], b, widen=dtype)
    bound, err = sg.bounds(ref, got["t"]), sg.errors({k: got[k] for k in ("loss", "dA", "dB", "dt", "db")}, ref)
    name = f"130x100-div5-ignore-trained/{str(dtype).split('.')[1]}"
    fails = []
    for k in ("loss", "dt", "db"):
        fails += _report(name, k, err[k], bound[k])
    for k in ("dA", "dB"):
        fails += _report(name, k, err[k], bound[k] + torch.finfo(dtype).eps / 2)
    assert not fails, "\n".join(fails)
    assert torch.equal(got["counts"].cpu().long(), ref["counts"])


def test_rows_behind_b_are_never_read():
    """A and B padded behind row B with 1e30 and NaN, ids with a value that would join a group: nothing changes"""
    from speechclip_plus_amd import ops
    B, E = 65, 68
    A, Bm = (x.to(DEV) for x in sg.inputs((B, E)))
    pad = torch.cat([torch.full((70, E), 1e30, device=DEV), torch.full((70, E), float("nan"), device=DEV)], 0)
    Ap, Bp = torch.cat([A, pad], 0), torch.cat([Bm, pad], 0)
    ids = lc.ids_div5(B).to(DEV)
    idp = torch.cat([ids, torch.zeros(140, dtype=torch.int64, device=DEV)])
    tt, bb = (torch.tensor([v], dtype=torch.float32, device=DEV) for v in sg.SETTINGS["trained"])
    plain = ops.sigmoid_loss_fwd(A, Bm, ids, tt, bb)
    padded = ops.sigmoid_loss_fwd(Ap[:B], Bp[:B], idp[:B], tt, bb)
    assert Ap[:B].data_ptr() == Ap.data_ptr()                                              # views: the pad rows stand right behind row B
    assert all(torch.equal(x, y) for x, y in zip(plain, padded)) and bool(torch.isfinite(padded[0]).all())


# ---------------------------------------------------------------------------------------------------- model level
def _tiny_model(seed=3):
    import dataclasses
    from speechclip_plus_amd import Config, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict, set_dropout
    from speechclip_plus_amd.speech_encoder import ARCHS
    arch = dataclasses.replace(ARCHS["hubert"], layers=1)
    torch.manual_seed(seed)
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    # the recipe's first step runs at lr 1e-4 / 5000 = 2e-8, and Adam's first update is lr in size: under half an ulp of log 10 = 2.30
    # (1.2e-7) and of -10 (4.8e-7), so neither fp32 scalar could move.  No warm-up: the step is 1e-4
    cfg.audio_encoder.scheduler.warmup = 1
    cfg.cl_loss = Config({"type": "SigmoidContrastiveLoss", "args": {"temperature": 0.1, "bias": -10.0, "learnable": True, "same_id": "ignore"}})
    model = KWClip_GeneralTransformer(cfg, device=DEV, hubert_state_dict=random_hubert_state_dict(arch, seed=seed), hubert_arch=arch)
    return set_dropout(model.train(), False)


def _input_dict(B=12, E=512, seed=9):
    g = torch.Generator().manual_seed(seed)
    norm = torch.nn.functional.normalize
    return {"id": torch.tensor([0, 1, 1, 2, 3, 3, 3, 4, 5, 6, 0, 7]).to(DEV),
            "image_feat": norm(torch.randn(B, E, generator=g), dim=-1).to(DEV),
            "parallel_audio_feat": norm(torch.randn(B, E, generator=g), dim=-1).to(DEV).requires_grad_(True)}


def test_the_model_trains_with_the_sigmoid_loss():
    """compute_loss is the criterion called alone on the same features, bit for bit; both scalars get a gradient; cl_bias is logged; a
    negative queue is refused by name at the first train-mode compute_loss; one ContrastiveTrainer step moves both scalars"""
    from speechclip_plus_amd.losses import SigmoidContrastiveLoss
    from speechclip_plus_amd.train import ContrastiveTrainer
    model = _tiny_model()
    crit = model.criterion
    assert isinstance(crit, SigmoidContrastiveLoss)
    d = _input_dict()
    out = model.compute_loss(d)
    out["loss"].backward()
    dls, db, dA = crit.logit_scale.grad.clone(), crit.logit_bias.grad.clone(), d["parallel_audio_feat"].grad.clone()
    assert torch.equal(out["loss"], out["p_cl_loss"]) and float(dls.abs()) > 0 and float(db.abs()) > 0 and float(dA.abs().max()) > 0
    assert crit.last_counts.tolist() == [12, 12 * 11 - 10, 10]                             # the id groups {0, 10}, {1, 2}, {4, 5, 6}: 2 + 2 + 6 pairs
    crit.logit_scale.grad = crit.logit_bias.grad = None
    a = d["parallel_audio_feat"].detach().clone().requires_grad_(True)
    direct = crit(a, d["image_feat"], d["id"])
    direct.backward()
    assert torch.equal(direct, out["loss"]) and torch.equal(a.grad, dA)
    assert torch.equal(crit.logit_scale.grad, dls) and torch.equal(crit.logit_bias.grad, db)
    crit.logit_scale.grad = crit.logit_bias.grad = None
    model.set_negative_queue(16)
    try:
        with pytest.raises(ValueError, match="MaskedContrastiveLoss"):
            model.compute_loss(_input_dict())
    finally:
        model.clear_negative_queue()
    assert bool(torch.isfinite(model.compute_loss(_input_dict())["loss"]))
    g = torch.Generator().manual_seed(17)
    batch = {"wav": torch.randn(4, 8000, generator=g).cuda(), "wav_len": torch.tensor([8000, 6000, 8000, 5000]),
             "image": torch.randn(4, 512, generator=g).cuda(), "id": torch.tensor([0, 1, 1, 2]).cuda()}
    logged = model.training_step(batch)["log_metrics"]                     # the step's log: both scalars, as device tensors
    assert isinstance(logged["cl_bias"], torch.Tensor) and float(logged["cl_bias"]) == -10.0 and abs(float(logged["cl_temp"]) - 0.1) < 1e-6
    trainer = ContrastiveTrainer(model)                                    # the flat Adam over getTrainableParams(), the replicated criterion
    for p in (crit.logit_scale, crit.logit_bias):
        assert any(q is p for q in trainer.opt.params) and any(q is p for q in trainer.replicated)
    s0, b0 = crit.logit_scale.detach().clone(), crit.logit_bias.detach().clone()
    loss = trainer.step(batch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(trainer.opt.flat_p).all())
    assert float(crit.logit_scale.grad.abs()) > 0 and float(crit.logit_bias.grad.abs()) > 0
    assert not torch.equal(crit.logit_scale.detach(), s0) and not torch.equal(crit.logit_bias.detach(), b0)
