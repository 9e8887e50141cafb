"""csrc/kwpool.hip (sc_kw_pool_fwd / sc_kw_pool_bwd) against fp64 on the same bf16 X: the constant-query pooling of the fixed-keyword
cascaded branch.  Inputs, the restatement and the criterion are in tests/kwpool_cases.py: relative L2 <= 2e-4 per (utterance, query)
for p / m / psum, per utterance for dX, per query for da / dc; a bf16 dX gets one 2^-8 rounding on top.  Every figure is printed as a
``PARITY|case|quantity|error|bound`` line before anything is asserted."""
import pytest
import torch

import kwpool_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _run(dev, case, mult=None, cbias=None, dx_dtype=torch.float32, X=None):
    from speechclip_plus_amd import ops
    Xd = (case["X"] if X is None else X).to(torch.bfloat16).to(dev)
    a, c, crow, flen = (case[k].to(dev) for k in ("a", "c", "crow", "flen"))
    md = mult.to(dev) if mult is not None else None
    p, m, psum = ops.kw_pool_fwd(Xd, a, c, crow, flen, case["row0"], md, want_psum=True)
    dX, da, dc = ops.kw_pool_bwd(Xd, a, crow, flen, case["row0"], p, case["dm"].to(dev), md,
                                 cbias.to(dev) if cbias is not None else None, dx_dtype=dx_dtype)
    return {"p": p, "m": m, "psum": psum, "dX": dX, "da": da, "dc": dc}


def _done(failures):
    assert not failures, "\n".join(f"{n} {k}: {e:.3e} > {b:.3e}" for n, k, e, b in failures)


@pytest.mark.parametrize("row0", kc.KERNEL_ROW0)
@pytest.mark.parametrize("R", kc.KERNEL_R)
@pytest.mark.parametrize("Q,C", kc.KERNEL_QC)
@pytest.mark.parametrize("D", kc.KERNEL_D)
def test_pool_against_fp64(dev, D, Q, C, R, row0):
    """Forward and backward, eval form (no multiplier) and train form (multiplier with zeros + the psum gradient), fp32 and bf16 dX.
    flen = 0, 1, 65, R - row0: a softmax over the constant keys alone, one frame, a frame count off every tile, the full buffer."""
    case = kc.pool_case(D, Q, C, R, row0)
    name = f"D={D} Q={Q} C={C} R={R} row0={row0}"
    fails = []
    ref = kc.pool_ref(case)
    got = _run(dev, case)
    kc.check(name + " eval", got, ref, {}, fails)
    reft = kc.pool_ref(case, case["mult"], case["cbias"])
    gott = _run(dev, case, case["mult"], case["cbias"])
    kc.check(name + " train", gott, reft, {}, fails)
    # a multiplier leaves p itself alone: the same bits as without
    assert torch.equal(gott["p"], got["p"])
    gotb = _run(dev, case, case["mult"], case["cbias"], dx_dtype=torch.bfloat16)
    assert gotb["dX"].dtype == torch.bfloat16
    kc.check(name + " train bf16 dX", {"dX": gotb["dX"]}, reft, {"dX": kc.FP32_BOUND + kc.BF16_ROUND}, fails)
    kc.check(name + " train bf16 dX", {k: gotb[k] for k in ("da", "dc")}, reft, {}, fails)
    for k in ("p", "m", "psum"):
        assert torch.equal(gotb[k], gott[k]), k
    # zeros behind flen, and in the CLS slot in front of the frames
    valid = kc.valid_mask(case).to(dev)
    assert (got["p"][~valid[:, None].expand_as(got["p"])] == 0).all()
    assert (got["dX"][~valid[:, C:]] == 0).all() and (gotb["dX"][~valid[:, C:]] == 0).all()
    _done(fails)


def test_pool_peaked_scores(dev):
    """The scores of query 0 span +-60 on the longest utterance: the maximum is subtracted before the exponential, so the result is a
    clean one-hot (no NaN, no overflow), and forward and backward meet the same bound as everywhere else."""
    case = kc.pool_case(768, 8, 8, 200, 1, peaked=True)
    ref = kc.pool_ref(case, case["mult"], case["cbias"])
    s = torch.cat([case["c"][0].double(), case["X"][3, 1:].double() @ case["a"][0].double()])
    assert float(s.max() - s.min()) > 60.0
    got = _run(dev, case, case["mult"], case["cbias"])
    for v in got.values():
        assert torch.isfinite(v).all()
    assert float(ref["p"][3, 0].max()) > 0.9 and int(got["p"][3, 0].argmax()) == int(ref["p"][3, 0].argmax())
    fails = []
    kc.check("peaked", got, ref, {}, fails)
    _done(fails)


def test_pool_ignores_rows_outside_the_frames_and_repeats(dev):
    """NaN in every row of X outside [row0, row0 + flen) - row 0 (the CLS slot) included - and in the multiplier's entries of those rows:
    every output keeps its bits.  Two calls on the same inputs: the same bits (no atomics)."""
    for Q, R, row0 in ((9, 200, 1), (8, 128, 0)):
        case = kc.pool_case(768, Q, Q, R, row0)
        clean = _run(dev, case, case["mult"], case["cbias"])
        again = _run(dev, case, case["mult"], case["cbias"])
        valid = kc.valid_mask(case)
        Xn = case["X"].clone()
        Xn[~valid[:, Q:]] = float("nan")
        mn = case["mult"].clone()
        mn[~valid[:, None].expand_as(mn)] = float("nan")
        dirty = _run(dev, case, mn, case["cbias"], X=Xn)
        for k in clean:
            assert torch.equal(clean[k], again[k]), ("two calls", k)
            assert torch.equal(clean[k], dirty[k]), ("NaN outside the frames", k)


def test_pool_multiplier_semantics(dev):
    """m and psum follow p * mult: with the kernel's own p, sum_j (p mult)_j key_j in fp64 reproduces m and psum; p is unchanged."""
    case = kc.pool_case(768, 9, 9, 200, 1)
    got = _run(dev, case, case["mult"], case["cbias"])
    plain = _run(dev, case)
    assert torch.equal(got["p"], plain["p"])
    assert (case["mult"] == 0).any()
    w = got["p"].double().cpu() * case["mult"].double()
    C = case["C"]
    m = w[..., :C] @ case["crow"].double() + torch.einsum("bqr,brd->bqd", w[..., C:],
                                                         torch.nan_to_num(case["X"].double()) * kc.valid_mask(case)[:, C:, None])
    fails = []
    kc.check("mult", {"m": got["m"], "psum": got["psum"]}, {"m": m, "psum": w.sum(-1)}, {}, fails)
    _done(fails)


def test_criterion_sees_a_dropped_key(dev):
    """Sensitivity: the kernel's own result with the last valid frame of one utterance, or constant key 0, taken out on the host
    must fail the criterion."""
    case = kc.pool_case(768, 8, 8, 200, 1)
    ref = kc.pool_ref(case)
    got = _run(dev, case)
    C, row0 = case["C"], case["row0"]
    X, p = case["X"].double(), got["p"].double().cpu()
    b = 3
    last = row0 + int(case["flen"][b]) - 1
    m_frame = got["m"].double().cpu().clone()
    m_frame[b] -= p[b, :, C + last, None] * X[b, last][None]
    fails = kc.check("dropped last frame", {"m": m_frame}, ref, {}, [])
    assert fails, "the criterion does not see a dropped frame"
    m_const = got["m"].double().cpu().clone()
    m_const -= p[:, :, 0, None] * case["crow"].double()[0]
    fails = kc.check("dropped constant key 0", {"m": m_const}, ref, {}, [])
    assert fails, "the criterion does not see a dropped constant key"
    # and the untouched result passes
    _done(kc.check("untouched", {"m": got["m"]}, ref, {}, []))


def test_pool_refuses_what_it_cannot_run(dev):
    """Past the LDS limit, D off 64 and Q / C past 16: an error with the numbers, no launch."""
    from speechclip_plus_amd import ops
    rmax = ops.kw_pool_max_rows(16, 16, backward=False)
    assert 200 < rmax < 4096
    B, D = 1, 64

    def call(Q, C, R, D=D):
        X = torch.zeros(B, R, D, device=dev, dtype=torch.bfloat16)
        z = lambda *s: torch.zeros(*s, device=dev)
        return ops.kw_pool_fwd(X, z(Q, D), z(Q, C), z(C, D), torch.zeros(B, dtype=torch.int32, device=dev), 0)

    call(16, 16, rmax)
    with pytest.raises(RuntimeError, match="LDS"):
        call(16, 16, rmax + 1)
    with pytest.raises(RuntimeError, match="1..16"):
        call(17, 16, 64)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        call(8, 8, 64, D=96)
