"""Properties of the builders in tests/loss_cases.py that tests/test_gpu_loss_optim.py relies on: no GPU needed."""
import math

import pytest
import torch

import loss_cases as lc


def test_shape_sweep_covers_every_batch_and_width():
    Bgs, Es = {1, 2, 63, 64, 65, 130, 200, 512, 1000}, {4, 20, 64, 68, 100, 768}
    assert {b for b, _ in lc.SHAPE_SWEEP} == Bgs and {e for _, e in lc.SHAPE_SWEEP} == Es
    for b in Bgs:
        assert len({e for bb, e in lc.SHAPE_SWEEP if bb == b}) >= 2, b
    for e in Es:
        assert any(ee == e and b in lc.RAGGED_MULTI_TILE for b, ee in lc.SHAPE_SWEEP), e
        assert e % 4 == 0                                         # the kernel's 16-byte operand loads
    assert any(e % 16 for _, e in lc.SHAPE_SWEEP)
    for b in lc.RAGGED_MULTI_TILE:
        assert b > lc.TILE and b % lc.TILE


@pytest.mark.parametrize("with_ids", [True, False])
def test_shape_sweep_gradients_have_a_scale(with_ids):
    """max |g - g64| / max |g64| needs a gradient that fp32 can resolve: every sweep case either has an analytically zero gradient
    (checked for exact zeros on the device) or a softmax that is not saturated.  (Bg, E) = (2, 4) is not in the sweep for that reason:
    at this seed its fp64 loss is 8e-9 and max |dA| 1.7e-7, below fp32's resolution of p - 1 (the fp32 oracle is 0.44 off there)."""
    for Bg, E in lc.SHAPE_SWEEP:
        if Bg > 200:
            continue                                              # hundreds of negatives per row: never saturated
        A, Bm = lc.make_pair(Bg, E, seed=Bg * 1000 + E)
        r = lc.loss_reference(A, Bm, lc.ids_div5(Bg) if with_ids else None)
        zero = Bg == 1 or (with_ids and Bg <= 5)
        for k in ("dA", "dB"):
            assert (float(r[k].abs().max()) < lc.ZERO_GRAD) == zero, (Bg, E, k)
        assert zero or float(r["loss"]) > 1e-3, (Bg, E, float(r["loss"]))


def test_pairs_are_unit_rows_with_a_correlated_partner():
    A, Bm = lc.make_pair(130, 100, seed=3)
    assert A.dtype == torch.float32 and torch.allclose(A.norm(dim=-1), torch.ones(130), atol=1e-6)
    assert torch.allclose(Bm.norm(dim=-1), torch.ones(130), atol=1e-6)
    cos = A.double() @ Bm.double().t()
    assert float(cos.diag().mean()) > float(cos.mean()) + 0.03
    A2, _ = lc.make_pair(130, 100, seed=3)
    assert torch.equal(A, A2)


def test_batch_of_one_is_zero_in_the_oracle():
    A, Bm = lc.make_pair(1, 768, seed=1)
    for ids in (torch.zeros(1, dtype=torch.int64), None):
        r = lc.loss_reference(A, Bm, ids)
        assert abs(float(r["loss"])) < 1e-14                      # -l + log(exp(l)): zero up to fp64 rounding
        assert float(r["dA"].abs().max()) < 1e-14 and float(r["dB"].abs().max()) < 1e-14


@pytest.mark.parametrize("permuted", [False, True])
def test_empty_tile_ids(permuted):
    """dcl, Bg = 200, groups of 70: a 64 x 64 tile without any negative for its rows, yet negatives for every row and column over the
    whole batch and finite fp64 log-sum-exps (the case with no negatives at all is out of scope: the reference returns inf)."""
    Bg = 200
    ids = lc.ids_empty_tile_permuted(Bg) if permuted else lc.ids_empty_tile(Bg)
    assert sorted(torch.bincount(ids).tolist()) == [60, 70, 70]
    neg = lc.neg_mask(Bg, ids, dcl=True)
    empty = lc.rows_without_negatives_per_tile(neg)
    if not permuted:
        assert (0, 0, 64, 64) in empty                            # tile (0, 0): all one id
        assert not bool(lc.neg_mask(Bg, ids, dcl=False)[:64, :64].sum(1).eq(0).any())    # without dcl the diagonal is a negative
    else:
        assert (0, 0, 64, 64) not in empty and not torch.equal(ids, lc.ids_empty_tile(Bg))
    assert bool((neg.sum(1) > 0).all()) and bool((neg.sum(0) > 0).all())
    A, Bm = lc.make_pair(Bg, 100, seed=7)
    r = lc.loss_reference(A, Bm, ids, dcl=True)
    assert bool(torch.isfinite(r["lse_row"]).all()) and bool(torch.isfinite(r["lse_col"]).all())
    assert math.isfinite(float(r["loss"])) and bool(torch.isfinite(r["dA"]).all())


def test_wide_ids_relabel_to_the_same_loss_in_fp64():
    Bg = 130
    ids = lc.wide_ids(Bg)
    assert set(ids.tolist()) == set(lc.WIDE_ID_VALUES) and ids.dtype == torch.int64
    small = lc.relabel(ids)
    assert int(small.min()) == 0 and int(small.max()) == len(lc.WIDE_ID_VALUES) - 1
    assert torch.equal(ids[:, None] == ids[None, :], small[:, None] == small[None, :])
    # 32-bit truncation would merge groups: 2^32 and 2^40 with each other, 2^32 + 1 with 1
    low = ids & 0xFFFFFFFF
    assert not torch.equal(low[:, None] == low[None, :], ids[:, None] == ids[None, :])
    A, Bm = lc.make_pair(Bg, 100, seed=9)
    r1, r2 = lc.loss_reference(A, Bm, ids), lc.loss_reference(A, Bm, small)
    for k in ("loss", "dA", "dB", "lse_row", "lse_col"):
        assert torch.equal(r1[k], r2[k]), k


def test_loss_reference_lse_is_the_loss():
    """The helper's log-sum-exps and logits are the quantities inside the oracle's loss, for every option set."""
    A, Bm = lc.make_pair(130, 20, seed=2)
    ids = lc.ids_div5(130)
    for name, kw in lc.VARIANTS.items():
        r = lc.loss_reference(A, Bm, ids, **kw)
        d = r["logits"].diag()
        a2b, b2a = kw.get("a2b", True), kw.get("b2a", True)
        loss = ((r["lse_row"] - d).mean() if a2b else 0) + ((r["lse_col"] - d).mean() if b2a else 0)
        loss = loss / 2 if a2b and b2a else loss
        assert abs(float(loss) - float(r["loss"])) < 1e-12, name
        assert ("dT" in r) == bool(kw.get("trainable"))
    r1, r4 = lc.loss_reference(A, Bm, ids), lc.loss_reference(A, Bm, ids, scale=0.25)
    assert torch.allclose(r4["dA"], 0.25 * r1["dA"], rtol=1e-14, atol=0)


@pytest.mark.parametrize("hyper", list(lc.ADAM_HYPER))
def test_adam_restatement_equals_torch_adam_on_doubles(hyper):
    total = 1023
    wd, clip, _ = lc.ADAM_HYPER[hyper]
    ps = [p.double() for p in lc.adam_params(total, seed=4)]
    ref = lc.AdamRef64(ps, weight_decay=wd, max_grad_norm=clip)
    tor = lc.TorchAdam(ps, weight_decay=wd, max_grad_norm=clip)
    clipped = []
    for s in list(range(20)) + [9999, 10000]:
        if s == 9999:
            ref.step_count = 9999
            tor.set_step_count(9999)
        gs = lc.adam_grads(total, hyper, min(s, 25), seed=4)
        lr = lc.adam_lr(min(s, 25))
        ref.step(gs, lr)
        tor.step(gs, lr)
        clipped.append(clip > 0 and ref.grad_norm + 1e-6 > clip)
        for q in ("p", "m", "v"):
            assert lc.cat_err(getattr(tor, q), getattr(ref, q)) < 1e-12, (hyper, s, q)
    if hyper == "wd_clip4_alternating":
        assert clipped == [bool(min(s, 25) % 2) for s in list(range(20)) + [9999, 10000]]
    if hyper == "clip1e-3_tiny":
        assert all(clipped)
        assert abs(clip / ref.grad_norm - clip / (ref.grad_norm + 1e-6)) / (clip / ref.grad_norm) > 1e-4      # the + 1e-6 matters


@pytest.mark.parametrize("total", list(lc.ADAM_SIZES))
def test_adam_clip_is_on_and_off_at_every_size(total):
    """The global norm of the fp32 gradients is what ADAM_HYPER sets, whatever the size and the seed: 12 / 1 against max_norm 4 on
    alternate steps, 2e-3 against 1e-3 where the + 1e-6 of the coefficient shows."""
    steps = range(3) if total > 1_000_000 else range(4)
    for seed in (range(16) if total <= 3 else [total % 1000]):
        for s in steps:
            n = lc.grad_norm64(lc.adam_grads(total, "wd_clip4_alternating", s, seed))
            assert n == pytest.approx(12.0 if s % 2 else 1.0, rel=1e-6) and (n + 1e-6 > 4.0) == bool(s % 2)
            assert lc.grad_norm64(lc.adam_grads(total, "clip1e-3_tiny", s, seed)) == pytest.approx(2e-3, rel=1e-6)
        assert all(g.dtype == torch.float32 for g in lc.adam_grads(total, "plain", 0, seed))


def test_adam_sizes_are_odd_tensors():
    for total, ns in lc.ADAM_SIZES.items():
        assert sum(ns) == total and all(n % 2 for n in ns) and 1 <= len(ns) <= 4
    assert 600001 > lc.ADAM_MAX_BLOCKS * 256                      # more elements than adam_kernel has threads
    ps = lc.adam_params(21513, seed=1)
    assert float(ps[0].abs().max()) <= 1e-3 and float(ps[1].abs().max()) > 1
    assert [lc.adam_lr(s) for s in range(3)] == pytest.approx([lc.ADAM_LR * (s + 1) / 5 for s in range(3)], rel=1e-12)
    assert lc.adam_lr(20) < lc.adam_lr(6) < lc.adam_lr(4)          # warm-up over 5 steps, then the decay


def test_sumsq_chain_and_merge():
    # 1 M floats on 1024 x 256 threads: a full vector pass (2 + 1), no tail, trees 6 + 2, 16 partials per lane + 6
    assert lc.sumsq_chain(1 << 20, aligned=True) == 3 + 8 + 16 + 6
    assert lc.sumsq_chain(1 << 20, aligned=False) == 4 + 8 + 16 + 6
    assert lc.sumsq_chain(3, aligned=True) == 1 + 8 + 16 + 6
    assert lc.sumsq_chain(1023, aligned=True) == 2 + 1 + 1 + 8 + 16 + 6
    part = torch.arange(1024, dtype=torch.float32)
    assert lc.merge_partials_fp32(part) == float(part.double().sum())
    x = lc.sumsq_values(100000, seed=1)
    assert 1e-4 <= float(x.abs().min()) and float(x.abs().max()) <= 1e2 and float(x.abs().max() / x.abs().min()) > 1e5
