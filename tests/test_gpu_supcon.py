"""SupConLoss on the HIP kernels of csrc/supcon.hip (sc_supcon_fwd / sc_supcon_grad under losses.SupConLoss) against fp64.

Inputs and the fp64 reference come from tests/supcon_cases.py (unit rows with a shared component per sample; the loss and its gradients
from the formulas), the fixtures from the reference implementation (tests/golden/supcon.npz).  Bounds are the project's own at
temperature 0.07 (tests/loss_cases.py): logits 2e-5, log-sum-exps 5e-5, |loss - loss64| <= 2e-5 / base_temperature (the bound on the mean
of the per-row terms times the factor the loss applies), gradients max |g - g64| / max |g64| <= 2e-4, and |dT - dT64| <= 2e-4 sum_ij
|g_ij l_ij| / T (the absolute summands of dT).  Everything stated "bit for bit" is compared with torch.equal.
Every figure is printed as a ``PARITY|case|quantity|error|bound`` line before anything is asserted."""
import functools
import math

import pytest
import torch

import supcon_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _report(case, quantity, err, bound):
    print(f"PARITY|{case}|{quantity}|{err:.3e}|{bound:.3e}")
    return [] if err <= bound else [f"{case}: {quantity} error {err:.3e} > bound {bound:.3e}"]


def _to(t):
    return t.to(DEV) if t is not None else None


@functools.lru_cache(maxsize=None)
def _features(shape):
    return sc.make_features(*shape, seed=sum(shape))


@functools.lru_cache(maxsize=None)
def _ref(shape, labelled, mode, base_temperature):
    """fp64 at the module's own fp32 temperature value; computed once per case and shared"""
    f = _features(shape)
    T = float(torch.tensor(0.07, dtype=torch.float32))
    return sc.reference(f, sc.labels_div5(shape[0]) if labelled else None, None, T=T, base_temperature=base_temperature, mode=mode)


def _module_run(features, labels=None, mask=None, scale=1.0, **kw):
    """SupConLoss(**kw)(features, labels, mask) and backward() -> dict(loss, dfeatures, [dT, T])"""
    from speechclip_plus_amd.losses import SupConLoss
    crit = SupConLoss(**kw).to(DEV)
    f = features.to(DEV).requires_grad_(True)
    loss = crit(f, labels=_to(labels), mask=_to(mask))
    (loss if scale == 1.0 else scale * loss).backward()
    out = {"loss": loss.detach(), "dfeatures": f.grad}
    if crit.learnable_temperature:
        out.update(dT=crit.temperature.grad, T=crit.temperature.detach())
    return out


def _check(case, got, ref, base_temperature, dT64=None, abs_gl=None):
    fails = _report(case, "loss", abs(float(got["loss"]) - float(ref["loss"])), sc.TOL_LOSS / base_temperature)
    fails += _report(case, "dfeatures", sc.scale_rel_err(got["dfeatures"], ref["dfeatures"]), sc.TOL_GRAD)
    if "dT" in got:
        dT64 = float(ref["dT"]) if dT64 is None else dT64
        abs_gl = float(ref["abs_gl"]) if abs_gl is None else abs_gl
        assert got["dT"].shape == (1,)
        fails += _report(case, "dT", abs(float(got["dT"]) - dT64), sc.TOL_GRAD * abs_gl)
    return fails


CASES = [(shape, labelled) for shape in sc.SHAPES for labelled in (False, True) if labelled or shape[1] >= 2]


@pytest.mark.parametrize("shape, labelled", CASES, ids=[f"{'x'.join(map(str, s))}-{'div5' if lab else 'nolabels'}" for s, lab in CASES])
def test_loss_and_gradients_vs_fp64(shape, labelled):
    from speechclip_plus_amd import ops
    bsz, V, E = shape
    f = _features(shape)
    labels = sc.labels_div5(bsz) if labelled else None
    fails = []
    for mode in sc.MODES:
        Na = V * bsz if mode == "all" else bsz
        for bt in sc.BASE_TEMPERATURES:
            case = f"{bsz}x{V}x{E}/{'div5' if labelled else 'nolabels'}/{mode}/bt{bt}"
            ref = _ref(shape, labelled, mode, bt)
            got = _module_run(f, labels, temperature=0.07, contrast_mode=mode, base_temperature=bt)
            assert float(got["T"]) == float(torch.tensor(0.07, dtype=torch.float32))
            fails += _check(case, got, ref, bt)
            if shape == (1, 2, 4):                   # one non-self column, the positive: everything vanishes
                assert float(got["loss"]) == 0.0 and float(got["dfeatures"].abs().max()) == 0.0 and float(got["dT"]) == 0.0
        # the forward's own outputs, once per mode
        C = torch.cat(torch.unbind(f, 1), 0).contiguous().to(DEV)
        it = (1.0 / torch.tensor([0.07], device=DEV))
        loss, logits, lse, possum, poscnt = ops.supcon_fwd(C, Na, bsz, _to(labels), None, it, 0.07)
        ref = _ref(shape, labelled, mode, 0.07)
        case = f"{bsz}x{V}x{E}/{'div5' if labelled else 'nolabels'}/{mode}"
        assert logits.shape == (Na, V * bsz) and lse.shape == possum.shape == poscnt.shape == (Na,)
        fails += _report(case, "logits", float((logits.double().cpu() - ref["logits"]).abs().max()), sc.TOL_LOGITS)
        if V * bsz > 1:
            fails += _report(case, "lse", float((lse.double().cpu() - ref["lse"]).abs().max()), sc.TOL_LSE)
        assert torch.equal(poscnt.double().cpu(), ref["poscnt"])                          # counts of 0 / 1 weights: exact
        fails += _report(case, "possum", float(((possum.double().cpu() - ref["possum"]).abs() / ref["poscnt"]).max()), sc.TOL_LOGITS)
    assert not fails, "\n".join(fails)


def test_wide_int64_labels_are_compared_on_all_64_bits():
    """ids that are negative or differ only above bit 31: the same bits as the same grouping relabelled 0 .. k - 1"""
    from loss_cases import relabel
    f = _features((65, 2, 20))
    wide = sc.wide_ids(65)
    assert int((wide >> 32).ne(0).sum()) > 0 and len(torch.unique(wide)) > 3
    for mode in sc.MODES:
        a = _module_run(f, wide, contrast_mode=mode)
        b = _module_run(f, relabel(wide), contrast_mode=mode)
        low = _module_run(f, wide & 0xFFFFFFFF, contrast_mode=mode)                       # what a 32-bit compare would see
        assert all(torch.equal(a[k], b[k]) for k in ("loss", "dfeatures", "dT"))
        assert not torch.equal(a["loss"], low["loss"])


def test_the_mask_of_label_equality_gives_the_labels_bits():
    f = _features((33, 2, 68))
    labels = sc.labels_div5(33)
    mask = (labels[:, None] == labels[None, :]).float()
    for mode in sc.MODES:
        a = _module_run(f, labels, contrast_mode=mode)
        b = _module_run(f, None, mask, contrast_mode=mode)
        assert all(torch.equal(a[k], b[k]) for k in ("loss", "dfeatures", "dT"))
    eye = _module_run(f, None, torch.eye(33))
    none = _module_run(f)
    assert all(torch.equal(eye[k], none[k]) for k in ("loss", "dfeatures", "dT"))


@pytest.mark.parametrize("name", [n for n in sc.GOLDEN_CASES if n not in sc.NAN_CASES])
def test_fixtures_of_the_reference_implementation(name):
    gold = sc.load_golden()
    mode, T, bt, learnable = sc.GOLDEN_CASES[name][4:8]
    f, labels, mask = sc.golden_inputs(name)
    assert torch.equal(f, torch.from_numpy(gold[f"{name}/features"]))
    got = _module_run(f, labels, mask, temperature=T, contrast_mode=mode, base_temperature=bt, learnable_temperature=learnable)
    helper = sc.reference(f, labels, mask, T=float(gold[f"{name}/T"].reshape(-1)[0]), base_temperature=bt, mode=mode)
    ref = {"loss": float(gold[f"{name}/loss64"]), "dfeatures": torch.from_numpy(gold[f"{name}/dfeatures64"])}
    assert ("dT" in got) == learnable
    dT64 = float(gold[f"{name}/dtemperature64"].reshape(-1)[0]) if learnable else None
    fails = _check(name, got, ref, bt, dT64, float(helper["abs_gl"]))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", sc.NAN_CASES)
def test_an_anchor_without_a_positive_gives_a_nan_loss(name):
    mode, T, bt, learnable = sc.GOLDEN_CASES[name][4:8]
    f, labels, mask = sc.golden_inputs(name)
    got = _module_run(f, labels, mask, temperature=T, contrast_mode=mode, base_temperature=bt, learnable_temperature=learnable)
    assert math.isnan(float(got["loss"]))


def test_two_calls_give_identical_bits():
    for shape, mode in (((65, 2, 768), "all"), ((100, 3, 64), "one"), ((512, 2, 100), "all")):
        f = _features(shape)
        labels = sc.labels_div5(shape[0])
        a = _module_run(f, labels, contrast_mode=mode)
        b = _module_run(f, labels, contrast_mode=mode)
        assert all(torch.equal(a[k], b[k]) for k in ("loss", "dfeatures", "dT")), (shape, mode)


def test_rows_behind_n_are_never_read():
    """C padded behind row N with 1e30 (and NaN): nothing changes, in the forward's outputs or in G"""
    from speechclip_plus_amd import ops
    bsz, V, E = 33, 2, 68
    N = bsz * V
    C = torch.cat(torch.unbind(_features((bsz, V, E)), 1), 0).contiguous().to(DEV)
    padded = torch.cat([C, torch.full((70, E), 1e30, device=DEV), torch.full((70, E), float("nan"), device=DEV)], 0)
    labels = sc.labels_div5(bsz).to(DEV)
    it, gs = torch.full((1,), 1.0 / 0.07, device=DEV), torch.ones(1, device=DEV)
    for Na in (N, bsz):
        plain = ops.supcon_fwd(C, Na, bsz, labels, None, it, 0.07)
        pad = ops.supcon_fwd(padded[:N], Na, bsz, labels, None, it, 0.07)
        assert padded[:N].data_ptr() == padded.data_ptr()                                  # a view: the pad rows stand right behind row N
        assert all(torch.equal(a, b) for a, b in zip(plain, pad)) and bool(torch.isfinite(pad[0]).all())
        G, dot = ops.supcon_grad(pad[1], pad[2], pad[4], bsz, labels, None, gs, it, 0.07)
        assert bool(torch.isfinite(G).all()) and bool(torch.isfinite(dot).all())


def test_the_adapter_is_the_call_on_the_stacked_features():
    """forward(feat_A=, feat_B=, index=) == forward(stack((feat_A, feat_B), 1), labels=index): loss and both gradients, bit for bit"""
    from speechclip_plus_amd.losses import SupConLoss
    f = _features((33, 2, 68))
    ids = sc.labels_div5(33).to(DEV)
    for mode in sc.MODES:
        outs = []
        for adapter in (True, False):
            crit = SupConLoss(contrast_mode=mode).to(DEV)
            a, b = f[:, 0].to(DEV).requires_grad_(True), f[:, 1].to(DEV).requires_grad_(True)
            loss = crit(feat_A=a, feat_B=b, index=ids) if adapter else crit(torch.stack((a, b), 1), labels=ids)
            loss.backward()
            outs.append((loss.detach(), a.grad, b.grad, crit.temperature.grad))
        assert all(torch.equal(x, y) for x, y in zip(*outs)), mode
        assert float(outs[0][1].abs().max()) > 0 and float(outs[0][2].abs().max()) > 0


def test_half_precision_features_get_gradients_in_their_dtype():
    from speechclip_plus_amd.losses import SupConLoss
    f = _features((33, 2, 68)).to(DEV)
    crit = SupConLoss().to(DEV)
    h = f.bfloat16().requires_grad_(True)
    crit(h, labels=sc.labels_div5(33).to(DEV)).backward()
    assert h.grad.dtype == torch.bfloat16 and h.grad.shape == h.shape and bool(torch.isfinite(h.grad.float()).all())
    f4 = f.reshape(33, 2, 17, 4).clone().requires_grad_(True)                             # trailing dimensions are flattened
    f3 = f.clone().requires_grad_(True)
    l4, l3 = crit(f4), crit(f3)
    l4.backward()
    l3.backward()
    assert torch.equal(l4, l3) and torch.equal(f4.grad.reshape(33, 2, 68), f3.grad)


# ---------------------------------------------------------------------------------------------------- model level
def _tiny_model(seed=3):
    import dataclasses
    from speechclip_plus_amd import Config, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict, set_dropout
    from speechclip_plus_amd.speech_encoder import ARCHS
    arch = dataclasses.replace(ARCHS["hubert"], layers=1)
    torch.manual_seed(seed)
    cfg = base_parallel_config()
    cfg.audio_encoder.max_audio_len = -1
    cfg.cl_loss = Config({"type": "SupConLoss", "args": {"temperature": 0.07, "contrast_mode": "all", "base_temperature": 0.07,
                                                         "learnable_temperature": True}})
    model = KWClip_GeneralTransformer(cfg, device=DEV, hubert_state_dict=random_hubert_state_dict(arch, seed=seed), hubert_arch=arch)
    return set_dropout(model.train(), False)


@pytest.fixture(scope="module")
def model():
    return _tiny_model()


def _input_dict(B=12, E=512, seed=9):
    g = torch.Generator().manual_seed(seed)
    norm = torch.nn.functional.normalize
    return {"id": torch.tensor([0, 1, 1, 2, 3, 3, 3, 4, 5, 6, 0, 7]).to(DEV),
            "image_feat": norm(torch.randn(B, E, generator=g), dim=-1).to(DEV),
            "parallel_audio_feat": norm(torch.randn(B, E, generator=g), dim=-1).to(DEV).requires_grad_(True)}


def test_compute_loss_is_the_criterion_on_the_stacked_features(model):
    from speechclip_plus_amd.losses import SupConLoss
    assert isinstance(model.criterion, SupConLoss)
    d = _input_dict()
    model.criterion.temperature.grad = None
    out = model.compute_loss(d)
    out["loss"].backward()
    dT, dA = model.criterion.temperature.grad.clone(), d["parallel_audio_feat"].grad.clone()
    assert torch.equal(out["loss"], out["p_cl_loss"]) and dT.shape == (1,) and float(dT.abs()) > 0 and float(dA.abs().max()) > 0
    model.criterion.temperature.grad = None
    a = d["parallel_audio_feat"].detach().clone().requires_grad_(True)
    direct = model.criterion(torch.stack((a, d["image_feat"]), 1), labels=d["id"])
    direct.backward()
    assert torch.equal(direct, out["loss"]) and torch.equal(a.grad, dA) and torch.equal(model.criterion.temperature.grad, dT)
    model.criterion.temperature.grad = None


def test_compute_loss_with_a_negative_bank_names_the_loss_that_has_them(model):
    g = torch.Generator().manual_seed(4)
    model.set_negative_bank(torch.randn(64, 512, generator=g).to(DEV), torch.arange(100, 164).to(DEV), 4)
    try:
        with pytest.raises(ValueError, match="MaskedContrastiveLoss"):
            model.compute_loss(_input_dict())
    finally:
        model.clear_negative_bank()
    assert bool(torch.isfinite(model.compute_loss(_input_dict())["loss"]))


def test_one_train_step_and_one_optimiser_step():
    model = _tiny_model()
    g = torch.Generator().manual_seed(17)
    B, L = 4, 8000
    batch = {"wav": torch.randn(B, L, generator=g).cuda(), "wav_len": torch.tensor([8000, 6000, 8000, 5000]),
             "image": torch.randn(B, 512, generator=g).cuda(), "id": torch.tensor([0, 1, 1, 2]).cuda()}
    from speechclip_plus_amd.train import ContrastiveTrainer
    trainer = ContrastiveTrainer(model)                                    # the flat Adam over getTrainableParams(), the replicated criterion
    assert any(p is model.criterion.temperature for p in trainer.opt.params)
    assert any(p is model.criterion.temperature for p in trainer.replicated)
    t0 = model.criterion.temperature.detach().clone()
    loss = trainer.step(batch)                                             # forward, backward, clip + Adam
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(trainer.opt.flat_g).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.getTrainableParams())
    assert float(model.criterion.temperature.grad.abs()) > 0
    assert bool(torch.isfinite(trainer.opt.flat_p).all()) and not torch.equal(model.criterion.temperature.detach(), t0)
    assert bool(torch.isfinite(trainer.step(batch)))                       # and the next step runs on the moved temperature
