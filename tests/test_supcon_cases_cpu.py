"""tests/supcon_cases.py against the fixtures the reference implementation of SupConLoss produced (tests/golden/supcon.npz, written by
tests/golden/make_golden_supcon.py): the helper's fp64 formulas reproduce the reference's fp64 autograd, and the reference's own fp32 run
stays inside the bounds the GPU tests hold the kernels to - a condition on the inputs, not a measurement of the kernels.  No GPU."""
import math

import numpy as np
import pytest
import torch

import supcon_cases as sc

FINITE_CASES = [n for n in sc.GOLDEN_CASES if n not in sc.NAN_CASES]


@pytest.fixture(scope="module")
def gold():
    return sc.load_golden()


def _ref(gold, name):
    mode, _, base_temperature = sc.GOLDEN_CASES[name][4:7]
    f = torch.from_numpy(gold[f"{name}/features"])
    labels = torch.from_numpy(gold[f"{name}/labels"]) if f"{name}/labels" in gold.files else None
    mask = torch.from_numpy(gold[f"{name}/mask"]) if f"{name}/mask" in gold.files else None
    return sc.reference(f, labels, mask, T=float(gold[f"{name}/T"].reshape(-1)[0]), base_temperature=base_temperature, mode=mode)


def test_the_fixture_holds_every_case_and_the_inputs_the_helper_builds(gold):
    for name, (bsz, V, E, labelling, _, T, _, learnable) in sc.GOLDEN_CASES.items():
        f, labels, mask = sc.golden_inputs(name)
        assert gold[f"{name}/features"].shape == (bsz, V, E) and np.array_equal(gold[f"{name}/features"], f.numpy())
        assert (f"{name}/labels" in gold.files) == (labels is not None) and (f"{name}/mask" in gold.files) == (mask is not None)
        if labels is not None:
            assert gold[f"{name}/labels"].dtype == np.int64 and np.array_equal(gold[f"{name}/labels"], labels.numpy())
        if mask is not None:
            assert np.array_equal(gold[f"{name}/mask"], mask.numpy())
        t = float(gold[f"{name}/T"].reshape(-1)[0])
        assert t == (float(np.float32(T)) if learnable else T)               # the module's own value: float32(0.07) is not 0.07
        assert (f"{name}/dtemperature64" in gold.files) == learnable
    m = gold["mask_all/mask"]
    assert not np.array_equal(m, m.T) and len(np.unique(m)) > 2               # asymmetric, weights other than 0 and 1


@pytest.mark.parametrize("name", FINITE_CASES)
def test_the_helper_reproduces_the_references_fp64_numbers(gold, name):
    r = _ref(gold, name)
    loss64 = float(gold[f"{name}/loss64"])
    print(f"SUPCON|{name}|loss {abs(float(r['loss']) - loss64):.3e} of {abs(loss64):.3e}")
    assert abs(float(r["loss"]) - loss64) <= 1e-6 * abs(loss64)
    d64 = torch.from_numpy(gold[f"{name}/dfeatures64"])
    err = sc.scale_rel_err(r["dfeatures"], d64)
    print(f"SUPCON|{name}|dfeatures {err:.3e}")
    assert err <= 1e-6
    if sc.GOLDEN_CASES[name][7]:
        dT64 = float(gold[f"{name}/dtemperature64"].reshape(-1)[0])
        print(f"SUPCON|{name}|dT {abs(float(r['dT']) - dT64):.3e} of {abs(dT64):.3e}, sum |g l| / T {float(r['abs_gl']):.3e}")
        assert abs(float(r["dT"]) - dT64) <= 1e-6 * float(r["abs_gl"])


@pytest.mark.parametrize("name", FINITE_CASES)
def test_the_references_own_fp32_run_is_inside_the_gpu_bounds(gold, name):
    base_temperature = sc.GOLDEN_CASES[name][6]
    r = _ref(gold, name)
    e_loss = abs(float(gold[f"{name}/loss32"]) - float(gold[f"{name}/loss64"]))
    e_grad = sc.scale_rel_err(torch.from_numpy(gold[f"{name}/dfeatures32"]), torch.from_numpy(gold[f"{name}/dfeatures64"]))
    print(f"SUPCON|{name}|reference fp32 vs fp64: loss {e_loss:.3e} (bound {sc.TOL_LOSS / base_temperature:.3e}), dfeatures {e_grad:.3e}")
    assert e_loss <= sc.TOL_LOSS / base_temperature and e_grad <= sc.TOL_GRAD
    if sc.GOLDEN_CASES[name][7]:
        e_T = abs(float(gold[f"{name}/dtemperature32"].reshape(-1)[0]) - float(gold[f"{name}/dtemperature64"].reshape(-1)[0]))
        print(f"SUPCON|{name}|reference fp32 vs fp64: dT {e_T:.3e} (bound {sc.TOL_GRAD * float(r['abs_gl']):.3e})")
        assert e_T <= sc.TOL_GRAD * float(r["abs_gl"])


@pytest.mark.parametrize("name", sc.NAN_CASES)
def test_an_anchor_without_a_positive_gives_nan_in_the_reference_and_in_the_helper(gold, name):
    assert math.isnan(float(gold[f"{name}/loss32"])) and math.isnan(float(gold[f"{name}/loss64"]))
    r = _ref(gold, name)
    assert math.isnan(float(r["loss"])) and int((r["poscnt"] == 0).sum()) >= 1


def test_the_single_pair_case_is_zero():
    """(1, 2, 4): one non-self column per anchor, which is its positive - loss, gradients and dT vanish"""
    r = sc.reference(sc.make_features(1, 2, 4, 0), T=0.07, base_temperature=0.07)
    assert abs(float(r["loss"])) < 1e-12 and float(r["dfeatures"].abs().max()) < 1e-12 and float(r["abs_gl"]) < 1e-12


def test_modes_and_shapes_of_the_reference():
    f = sc.make_features(5, 3, 8, 1)
    a, o = sc.reference(f, sc.labels_div5(5), mode="all"), sc.reference(f, sc.labels_div5(5), mode="one")
    assert a["logits"].shape == (15, 15) and o["logits"].shape == (5, 15) and torch.equal(a["logits"][:5], o["logits"])
    assert a["dfeatures"].shape == f.shape and torch.allclose(f.norm(dim=-1), torch.ones(5, 3), atol=1e-6)
    assert torch.equal(o["poscnt"], torch.full((5,), 14.0, dtype=torch.float64))       # one label group: every other row is a positive
