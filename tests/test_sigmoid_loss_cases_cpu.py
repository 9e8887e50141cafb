"""The cases of the pairwise sigmoid loss (tests/sigmoid_loss_cases.py), the checks that need no GPU: the helper's fp64 formulas against
fp64 torch autograd over F.binary_cross_entropy_with_logits, and the conditions that make the GPU sweep's bounds bite - re-asserted on
the fp64 reference and on a plain fp32 torch evaluation.  They are properties of the cases, not measurements of the kernels."""
import pytest
import torch
import torch.nn.functional as F

import loss_cases as lc
import sigmoid_loss_cases as sg

TRAINED = sg.SETTINGS["trained"]


def _ref(case, **kw):
    shape, idset, mode, setting = case
    A, Bm = sg.inputs(shape)
    t, b = sg.SETTINGS[setting]
    return sg.reference(A, Bm, sg.make_ids(idset, shape[0]), t, b, mode, **kw)


@pytest.mark.parametrize("case", sg.CASES, ids=sg.case_id)
def test_the_formulas_are_autograd_over_bce_with_logits(case):
    """an independent definition: F.binary_cross_entropy_with_logits(x, target, weight, reduction="sum") / B with torch autograd in fp64"""
    shape, idset, mode, setting = case
    B = shape[0]
    A, Bm = sg.inputs(shape)
    t0, b0 = sg.SETTINGS[setting]
    ref = _ref(case)
    a, bm = A.double().requires_grad_(True), Bm.double().requires_grad_(True)
    t, b = torch.tensor(t0, dtype=torch.float64, requires_grad=True), torch.tensor(b0, dtype=torch.float64, requires_grad=True)
    z, w, _ = sg.pair_tables(B, sg.make_ids(idset, B), mode)
    x = t * (a @ bm.t()) + b
    x.retain_grad()
    loss = F.binary_cross_entropy_with_logits(x, (z + 1) / 2, weight=w, reduction="sum") / B
    loss.backward()
    loss = loss.detach()

    def rel(got, want):
        return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)
    assert abs(float(loss) - float(ref["loss"])) <= 1e-12 * abs(float(loss))
    assert rel(ref["g"], x.grad) <= 1e-12 and rel(ref["dA"], a.grad) <= 1e-12 and rel(ref["dB"], bm.grad) <= 1e-12
    assert rel(ref["dt"], t.grad) <= 1e-12 and rel(ref["db"], b.grad) <= 1e-12
    assert int(ref["counts"].sum()) == B * B and int(ref["counts"][0]) >= B
    if idset == "none" or mode == "negative":
        assert ref["counts"].tolist() == [B, B * B - B, 0]


@pytest.mark.parametrize("case", sg.CASES, ids=sg.case_id)
def test_a_plain_fp32_evaluation_stays_inside_every_bound(case):
    """what the arithmetic of the format gives: the bounds ask nothing that fp32 cannot deliver"""
    t = sg.SETTINGS[case[3]][0]
    ref, f32 = _ref(case), _ref(case, dtype=torch.float32)
    bound, err = sg.bounds(ref, t), sg.errors(f32, ref)
    for k in ("x", "loss", "g", "dA", "dB", "dt", "db"):
        print(f"CASE|{sg.case_id(case)}|{k}|{err[k]:.3e}|{bound[k]:.3e}")
    assert all(err[k] <= bound[k] for k in bound), {k: (err[k], bound[k]) for k in bound if err[k] > bound[k]}
    assert torch.equal(f32["counts"], ref["counts"])


@pytest.mark.parametrize("shape", [(65, 68), (130, 100), (512, 768)], ids=lambda s: "x".join(map(str, s)))
def test_at_the_trained_setting_the_id_mask_moves_far_more_than_the_bounds(shape):
    """(1 / 0.07, -5) with ids_div5: dropping the mask moves the fp64 loss by >= 100 loss bounds and puts a median of >= 10 TOL_GRAD
    max |g| into the entries of g that must be 0.  At (10, -10) the same mask moves g by a fraction of TOL_GRAD: that setting proves
    the mask through the counts only."""
    A, Bm = sg.inputs(shape)
    ids = lc.ids_div5(shape[0])
    t, b = TRAINED
    masked, plain = sg.reference(A, Bm, ids, t, b, "ignore"), sg.reference(A, Bm, None, t, b)
    bound = sg.bounds(masked, t)
    _, w, same = sg.pair_tables(shape[0], ids, "ignore")
    move = abs(float(plain["loss"]) - float(masked["loss"]))
    median = float(plain["g"][same].abs().median())
    print(f"CASE|{shape}|loss move {move:.3e}|bound {bound['loss']:.3e}|median g {median / bound['g']:.1f} TOL_GRAD")
    assert move >= 100 * bound["loss"] and median >= 10 * bound["g"]
    assert float(masked["g"][same].abs().max()) == 0.0 and int(masked["counts"][2]) == int(same.sum()) > 0
    t, b = sg.SETTINGS["default"]
    masked, plain = sg.reference(A, Bm, ids, t, b, "ignore"), sg.reference(A, Bm, None, t, b)
    assert float(plain["g"][same].abs().median()) < sg.bounds(masked, t)["g"]              # ... and not at the defaults
    assert not torch.equal(masked["counts"], plain["counts"])


@pytest.mark.parametrize("shape", [s for s in sg.SHAPES if s[0] >= 5], ids=lambda s: "x".join(map(str, s)))
def test_positive_against_ignore_moves_the_loss_by_at_least_12(shape):
    A, Bm = sg.inputs(shape)
    ids = lc.ids_div5(shape[0])
    t, b = TRAINED
    pos, ign = sg.reference(A, Bm, ids, t, b, "positive"), sg.reference(A, Bm, ids, t, b, "ignore")
    print(f"CASE|{shape}|positive {float(pos['loss']):.4f}|ignore {float(ign['loss']):.4f}")
    assert float(pos["loss"]) - float(ign["loss"]) >= 12.0
    assert int(pos["counts"][0]) == int(ign["counts"][0]) + int(ign["counts"][2]) and int(pos["counts"][2]) == 0


def test_the_saturated_setting_overflows_the_naive_form_only():
    """(100, +100) at (65, 68): x reaches 137, exp(max x) is not finite in fp32, the stable fp32 evaluation is finite and inside the bounds"""
    A, Bm = sg.inputs(sg.SATURATED_SHAPE)
    t, b = sg.SETTINGS["saturated"]
    ref, f32 = sg.reference(A, Bm, None, t, b), sg.reference(A, Bm, None, t, b, dtype=torch.float32)
    assert float(ref["x"].max()) > 130.0 and not bool(torch.isfinite(f32["x"].max().exp()))
    masked = sg.reference(A, Bm, lc.ids_div5(sg.SATURATED_SHAPE[0]), t, b, "ignore")
    print(f"CASE|saturated|loss without ids {float(ref['loss']):.2f}|with ids_div5, ignore {float(masked['loss']):.2f}")
    assert abs(float(masked["loss"]) - 6006.86) < 0.01                                      # the figure of the case as the sweep runs it
    assert all(bool(torch.isfinite(f32[k]).all()) for k in ("loss", "g", "dA", "dB", "dt", "db"))
    bound, err = sg.bounds(ref, t), sg.errors(f32, ref)
    assert all(err[k] <= bound[k] for k in bound)


def test_the_empty_tile_and_the_wide_ids_are_what_their_names_say():
    B = sg.EMPTY_TILE_SHAPE[0]
    _, w, same = sg.pair_tables(B, lc.ids_empty_tile(B), "ignore")
    tile = w[:lc.TILE, :lc.TILE]
    assert float((tile - torch.eye(lc.TILE, dtype=torch.float64)).abs().max()) == 0.0       # tile (0, 0): the diagonal alone is weighted
    assert float(w[:lc.TILE, 2 * lc.TILE:].min()) == 1.0                                   # ... and other tiles are not empty
    wide = lc.wide_ids(sg.WIDE_SHAPE[0])
    low = wide & 0xFFFFFFFF
    same_wide, same_low = sg.pair_tables(len(wide), wide, "ignore")[2], sg.pair_tables(len(wide), low, "ignore")[2]
    assert int((wide >> 32).ne(0).sum()) > 0 and int(wide.lt(0).sum()) > 0
    assert int(same_low.sum()) > int(same_wide.sum()) > 0                                  # a 32-bit compare would merge groups
    assert torch.equal(sg.pair_tables(len(wide), lc.relabel(wide), "ignore")[2], same_wide)
    A, Bm = sg.inputs(sg.WIDE_SHAPE)
    t, b = TRAINED
    a, c = sg.reference(A, Bm, wide, t, b), sg.reference(A, Bm, low, t, b)
    assert abs(float(a["loss"]) - float(c["loss"])) >= 100 * sg.bounds(a, t)["loss"]
