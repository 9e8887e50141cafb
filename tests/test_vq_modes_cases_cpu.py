"""tests/vq_modes_cases.py (the host restatement of the quantiser's soft / Gumbel / learnable-temperature modes) against the
reference module's fixtures (tests/golden/vq_modes.npz), against torch's F.gumbel_softmax on a given noise, and the noise twin against
the library's sc_hash32; then the two conditions the GPU tests lean on: the sampled tokens follow softmax(x), and the margin case's
smallest top-2 margin dwarfs the device noise's error.  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vq_modes_cases as vc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vq_modes.npz")


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN)
    d = {k: z[k] for k in z.files}
    d["x2"] = vc.masked(d["x"].reshape(15, 50))
    d["t"] = d["gk"].reshape(15, 8).astype(np.float64) @ d["emb"].astype(np.float64).T           # d subword_prob
    return d


@pytest.mark.parametrize("tag,hard", [("soft_fixed", False), ("hard_learn", True), ("soft_learn", False), ("hard_learn_fin", True),
                                      ("soft_learn_fin", False)])
def test_the_helper_reproduces_the_reference_fixtures(fx, tag, hard):
    """The fixture is the reference's fp32 run: the fp64 restatement agrees to fp32 rounding.  Tolerances measured when the fixture was
    made: subword_prob 1.1e-7 absolute (values <= 1), gradient to x 2.3e-6 absolute at max |gx| = 24.3 (9.5e-8 relative), the
    temperature gradient 3e-6 relative; asserted at 4 U, 4 U max |gx| x 15 terms and 1e-5."""
    f = vc.forward(fx["x2"], 0.1, hard, table=fx["emb"])
    dz, dx, dtau, _ = vc.backward(f["s"], f["z"], fx["t"], 0.1)
    assert np.array_equal(f["targets"], fx[tag + "_targets"].reshape(-1))
    assert np.abs(f["prob"] - fx[tag + "_prob"].reshape(15, 50)).max() <= 4 * vc.U
    gx = fx[tag + "_gx"].reshape(15, 50).astype(np.float64)
    assert np.all(gx[:, list(vc.SPECIAL)] == 0.0) and np.all(dx[:, list(vc.SPECIAL)] == 0.0)
    assert np.abs(dx - gx).max() <= 60 * vc.U * np.abs(gx).max()
    if tag.endswith("_learn"):
        # a CORRECTION, not a match: the reference's own curr_temp.grad is NaN under the -inf mask (0 * inf in x / temp's backward)
        assert np.isnan(fx[tag + "_gtemp"]).all() and np.isfinite(dtau)
    if tag.endswith("_fin"):
        ref = float(fx[tag + "_gtemp"][0])
        assert np.isfinite(ref) and abs(dtau - ref) <= 1e-5 * abs(ref), (dtau, ref)


def test_eval_mode_of_a_soft_module_is_the_hard_one_hot(fx):
    f = vc.eval_forward(fx["x2"])
    assert np.array_equal(f["prob"], fx["ev_soft_prob"].reshape(15, 50)) and np.array_equal(f["targets"], fx["ev_soft_targets"].reshape(-1))
    assert set(np.unique(f["prob"])) == {0.0, 1.0} and np.all(f["prob"].sum(-1) == 1.0)


@pytest.mark.parametrize("hard", [False, True])
def test_the_formula_is_torchs_gumbel_softmax_on_the_same_noise(fx, hard):
    """F.gumbel_softmax draws g = -log(Exp(1)) from torch's generator: reseed, draw the same g, and the helper's table row
    (softmax((x + g) / tau), hard: one-hot of argmax(x + g) with the soft gradient) is torch's value and gradient."""
    tau = 0.5
    x = torch.from_numpy(fx["x2"]).requires_grad_()
    torch.manual_seed(7)
    g = -torch.empty_like(x, memory_format=torch.legacy_contiguous_format).exponential_().log()
    torch.manual_seed(7)
    y = F.gumbel_softmax(x, tau=tau, hard=hard)
    t = torch.from_numpy(fx["t"])
    (y * t).sum().backward()
    f = vc.forward(fx["x2"], tau, hard, g=g.numpy())
    _, dx, _, _ = vc.backward(f["s"], f["z"], fx["t"], tau)
    assert np.abs(f["prob"] - y.detach().numpy()).max() <= 1e-14
    assert np.array_equal(f["targets"], y.detach().numpy().argmax(-1))
    assert np.abs(dx - x.grad.numpy()).max() <= 1e-12 * np.abs(dx).max()


def test_the_twins_words_are_the_librarys():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()
    words = np.concatenate([np.arange(64, dtype=np.uint32), np.array([0xffffffff, 0x80000000, 0x9E3779B1, 12345678], dtype=np.uint32)])
    assert [int(w) for w in vc.hash32(words)] == [lib.sc_hash32(int(w)) for w in words]
    w = vc.noise_words(3, 50, 0xDEADBEEF)
    assert int(w[2, 7]) == lib.sc_hash32((2 * 50 + 7) ^ 0xDEADBEEF)
    e = 1663 * 19787 + 19786                                                        # the last element of the largest recipe shape
    assert int(vc.hash32(np.array([e ^ 5], dtype=np.uint32))[0]) == lib.sc_hash32(e ^ 5)


def test_the_noise_is_finite_and_in_range():
    for seed in (0, 1, 99, 0xffffffff):
        w = vc.noise_words(257, 1000, seed)
        u = vc.uniform(w)
        assert u.min() >= 2.0 ** -24 and u.max() <= 1.0 - 2.0 ** -24
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u)             # exact in fp32
        g = vc.gumbel(257, 1000, seed)
        assert np.isfinite(g).all() and g.min() >= vc.G_MIN and g.max() <= vc.G_MAX
    lo, hi = -np.log(-np.log(2.0 ** -24)), -np.log(-np.log(1.0 - 2.0 ** -24))
    assert vc.G_MIN <= lo and hi <= vc.G_MAX


@pytest.mark.parametrize("seed", vc.SAMPLING_SEEDS)
def test_sampling_condition_on_the_twin(seed):
    """65536 draws of argmax(x + g) follow softmax(x) within 4 sigma per token (measured: at most 2.31 sigma over the five seeds); no
    masked column is ever chosen."""
    counts, expect, sigma = vc.sampling_counts(seed)
    assert counts[list(vc.SPECIAL)].sum() == 0 and counts.sum() == 65536
    live = sigma > 0
    dev = np.abs((counts - expect)[live] / sigma[live]).max()
    print(f"seed {seed:#x}: largest deviation {dev:.2f} sigma")
    assert dev <= 4.0


def test_margin_condition():
    x, g, margin = vc.margin_case()
    err = float(vc.noise_bound(g).max())
    print(f"smallest top-2 margin {margin:.3e}, device noise error at most {err:.3e}")
    assert 6.0e-3 < margin < 7.0e-3 and err < 4.4e-6 and margin > 1000 * err
