"""The contrastive loss with a negative bank, the checks that need no GPU: the two new entries declared / bound / exported, their C
argument checks, the host layers' refusals in their order (format errors before device errors, all before a launch), the fp64
reference expression against oracle.loss_ref, and the unchanged signature of the plain call."""
import inspect
import os
import re

import pytest
import torch

import loss_cases as lc
import neg_loss_cases as nc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("sc_infonce_neg_fwd", "sc_infonce_neg_grad")


class _OnDevice(torch.Tensor):
    """a tensor that says it is on the device; the checks under test raise before anything reads it"""
    is_cuda = True


# ---------------------------------------------------------------------------------------------------- declared, bound, exported
def test_symbols_declared_bound_and_exported():
    from speechclip_plus_amd import _lib, build, ops
    header = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    declared = set(re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "sc_infonce_neg_workspace_floats" in declared and hasattr(lib, "sc_infonce_neg_workspace_floats")
    assert lib.sc_abi_version() == 7                                   # the change is additive
    assert "infonce_neg.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "infonce_neg.hip"))
    assert callable(ops.infonce_neg_fwd) and callable(ops.infonce_neg_grad)


def _entries():
    """both C entries as f(Bg, E, N, M, stride, a2b) with null pointers throughout"""
    from speechclip_plus_amd import _lib
    lib = _lib.lib()

    def fwd(Bg, E, N, M, stride, a2b=1):
        return lib.sc_infonce_neg_fwd(None, None, stride, None, None, None, None, None, None, None, Bg, E, N, M, a2b, 1, None, None, None,
                                      None, None, None)

    def grad(Bg, E, N, M, stride, a2b=1):
        return lib.sc_infonce_neg_grad(None, stride, None, None, None, None, None, Bg, E, N, M, a2b, 1, None, None, None)
    return lib, (("sc_infonce_neg_fwd", fwd), ("sc_infonce_neg_grad", grad))


def test_argument_checks_need_no_device():
    lib, entries = _entries()
    for name, f in entries:
        for E in (0, 6, 101, -4):
            assert f(3, E, 10, 2, 128) == -1 and name.encode() in lib.sc_last_error() and b"E %" in lib.sc_last_error(), (name, E)
        for M in (0, -1, 1025):
            assert f(3, 64, 10, M, 64) == -1 and b"1 <= M <= 1024" in lib.sc_last_error(), (name, M)
        for N in (-1, 2 ** 31, 2 ** 40):
            assert f(3, 64, N, 2, 64) == -1 and b"N < 2^31" in lib.sc_last_error(), (name, N)
        for stride in (60, 66, 0):
            assert f(3, 64, 10, 2, stride) == -1 and b"16-byte rows" in lib.sc_last_error(), (name, stride)
        assert f(3, 64, 10, 2, 64, a2b=0) == -1 and b"a2b" in lib.sc_last_error()
        assert f(-1, 64, 10, 2, 64) == -1
        assert f(3, 64, 10, 2, 64) == -1 and b"null pointer" in lib.sc_last_error()      # everything else passed: the operands are missing
        assert f(0, 64, 10, 2, 64) == 0 and f(0, 64, 0, 1024, 68) == 0                   # no anchor: a no-op, nothing is touched
        assert f(0, 6, 10, 2, 64) == -1 and f(0, 64, 10, 0, 64) == -1                    # ... behind the range checks
    ws = lib.sc_infonce_neg_workspace_floats                      # 3 floats per (anchor, chunk); chunks of 64 slots, of 32 / 16 while
    assert ws(64, 1024) == 3 * 64 * 16 and ws(512, 64) == 3 * 512 and ws(200, 256) == 3 * 200 * 4     # ... under 512 workgroups
    assert ws(64, 32) == 3 * 64 * 2 and ws(64, 256) == 3 * 64 * 8 and ws(1, 2) == 3 and ws(0, 2) == 0 and ws(4, 1025) == 0


# ---------------------------------------------------------------------------------------------------- refusals and their order
def _operands(Bg=4, E=8, N=6, M=3, on_device=False):
    t = {"A": torch.zeros(Bg, E), "B": torch.zeros(Bg, E), "ids": torch.zeros(Bg, dtype=torch.int64), "bank": torch.zeros(N, E),
         "bank_ids": torch.ones(N, dtype=torch.int64), "neg_idx": torch.zeros(Bg, M, dtype=torch.int64)}
    return {k: v.as_subclass(_OnDevice) if on_device else v for k, v in t.items()}


def _crit(**kw):
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    return MaskedContrastiveLoss(**kw)


def _call(crit, t, **over):
    t = {**t, **over}
    return crit(t["A"], t["B"], t["ids"], bank=t["bank"], bank_ids=t["bank_ids"], neg_idx=t["neg_idx"])


def test_module_refusals_come_before_any_launch_in_order():
    """Every operand below is a host tensor (or says it is on the device and holds no device memory): a launch would fail, so each
    refusal is raised before one.  Each case carries every LATER defect too: the earlier refusal wins."""
    t = _operands()
    crit, one_sided = _crit(), _crit(a2b=False)
    grad_bank = t["bank"].clone().requires_grad_(True)
    bad_M = torch.zeros(4, 1025, dtype=torch.int64)
    with pytest.raises(ValueError, match="ids on one side only"):                        # ... and no lists, a2b off, grad bank, CPU
        _call(one_sided, t, bank_ids=None, neg_idx=None, bank=grad_bank)
    with pytest.raises(ValueError, match="ids on one side only"):
        _call(crit, t, ids=None)
    with pytest.raises(ValueError, match="bank and neg_idx come together"):              # a bank without lists
        _call(one_sided, t, neg_idx=None, bank=grad_bank)
    with pytest.raises(ValueError, match="bank and neg_idx come together"):              # lists without a bank
        _call(crit, t, bank=None)
    with pytest.raises(ValueError, match="bank must be torch.float32"):                  # dtypes and shapes
        _call(one_sided, t, bank=t["bank"].double(), neg_idx=bad_M)
    with pytest.raises(ValueError, match="must share E"):
        _call(crit, t, bank=torch.zeros(6, 12))
    with pytest.raises(ValueError, match="neg_idx must be torch.int64"):
        _call(crit, t, neg_idx=t["neg_idx"].int())
    with pytest.raises(ValueError, match=r"neg_idx has shape \(3, 3\), expected \(4, M\)"):
        _call(crit, t, neg_idx=t["neg_idx"][:3])
    with pytest.raises(ValueError, match=r"bank_ids has shape \(5,\), expected \(6,\)"):
        _call(crit, t, bank_ids=t["bank_ids"][:5])
    with pytest.raises(ValueError, match="ids must be torch.int64"):
        _call(crit, t, ids=t["ids"].int())
    with pytest.raises(ValueError, match="1 <= M <= 1024"):                              # M, ahead of a2b / grad bank / CPU
        _call(one_sided, t, neg_idx=bad_M, bank=grad_bank)
    with pytest.raises(ValueError, match="1 <= M <= 1024"):
        _call(crit, t, neg_idx=torch.zeros(4, 0, dtype=torch.int64))
    with pytest.raises(ValueError, match="a2b=False"):                                   # a2b, ahead of grad bank / CPU
        _call(one_sided, t, bank=grad_bank)
    with pytest.raises(ValueError, match="requires_grad"):                               # grad bank, ahead of CPU
        _call(crit, t, bank=grad_bank)
    with pytest.raises(RuntimeError, match="MaskedContrastiveLoss runs on the HIP kernels: device tensors only"):
        _call(crit, t)
    dev = _operands(on_device=True)
    with pytest.raises(RuntimeError, match=r"device tensors only \(bank_ids\)"):         # the ids alone on the host are enough
        _call(crit, dev, bank_ids=t["bank_ids"])


def test_ops_refusals_come_before_any_launch_in_order():
    from speechclip_plus_amd import ops
    t = _operands()
    it = torch.ones(1)
    lse, logits = torch.zeros(4), torch.zeros(4, 4)

    def fwd(a2b=True, **over):
        u = {**t, **over}
        return ops.infonce_neg_fwd(u["A"], u["bank"], u["neg_idx"], u["ids"], u["bank_ids"], it, lse, lse, logits, a2b, True)

    def grad(a2b=True, **over):
        u = {**t, **over}
        return ops.infonce_neg_grad(u["A"], u["bank"], u["neg_idx"], torch.zeros(4, 3), lse, it, it, a2b, True, torch.zeros(4, 8), torch.zeros(4))
    with pytest.raises(ValueError, match="infonce_neg_fwd: ids on one side only"):
        fwd(a2b=False, bank_ids=None, neg_idx=torch.zeros(4, 0, dtype=torch.int64))
    for f, name in ((fwd, "infonce_neg_fwd"), (grad, "infonce_neg_grad")):
        with pytest.raises(ValueError, match=f"{name}: neg_idx must be torch.int64"):
            f(a2b=False, neg_idx=t["neg_idx"].float())
        with pytest.raises(ValueError, match=f"{name}: A must be torch.float32"):
            f(A=t["A"].half())
        with pytest.raises(ValueError, match="multiple of 4"):
            f(A=torch.zeros(4, 6), bank=torch.zeros(6, 6))
        with pytest.raises(ValueError, match=f"{name}: 1 <= M <= 1024"):
            f(a2b=False, neg_idx=torch.zeros(4, 2000, dtype=torch.int64))
        with pytest.raises(ValueError, match="a2b=False"):
            f(a2b=False, bank=t["bank"].clone().requires_grad_(True))
        with pytest.raises(ValueError, match="requires_grad"):
            f(bank=t["bank"].clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match=f"{name} runs on the HIP kernels: device tensors only"):
            f()


# ---------------------------------------------------------------------------------------------------- the reference expression
@pytest.mark.parametrize("name", [None] + list(k for k in lc.VARIANTS if k != "b2a"))
def test_reference_with_empty_lists_is_the_oracle(name):
    """all slots empty (-1, out of range, id-masked): loss and gradients of the helper's fp64 expression equal oracle.loss_ref's"""
    kw = lc.VARIANTS[name] if name else {}
    c = nc.make_case(*nc.MAIN)
    N = c["bank"].shape[0]
    empty = torch.full_like(c["neg_idx"], -1)
    empty[:, 1::3] = N
    empty[:, 2::3] = (torch.arange(130) // 5 * 5)[:, None]                 # bank rows under the anchor's own id
    got = nc.neg_loss_reference(c["A"], c["B"], c["ids"], c["bank"], c["bank_ids"], empty, **kw)
    ref = lc.loss_reference(c["A"], c["B"], c["ids"], **kw)
    assert int(got["used"].max()) == 0
    for k in ("loss", "dA", "dB", "lse_row", "lse_col") + (("dT",) if "dT" in ref else ()):
        assert torch.equal(got[k], ref[k]), k


def test_reference_counts_the_extras():
    c = nc.make_case(*nc.MAIN)
    got = nc.neg_loss_reference(c["A"], c["B"], c["ids"], c["bank"], c["bank_ids"], c["neg_idx"])
    plain = lc.loss_reference(c["A"], c["B"], c["ids"])
    assert float(got["loss"]) - float(plain["loss"]) > 0.1
    ok = nc.slot_mask(c["neg_idx"], 1000, c["ids"], c["bank_ids"])
    assert 0 < int((~ok).sum()) < ok.numel()                               # mined lists do hold the batch's own images
    assert bool((got["lse_row"] > plain["lse_row"]).all())


# ---------------------------------------------------------------------------------------------------- the plain call
def test_forward_without_the_keywords_is_the_old_signature():
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    from speechclip_plus_amd import KWClip_GeneralTransformer
    sig = inspect.signature(MaskedContrastiveLoss.forward)
    names = list(sig.parameters)
    assert names == ["self", "feat_A", "feat_B", "index", "bank", "bank_ids", "neg_idx"]
    assert sig.parameters["index"].default is None and sig.parameters["index"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    for k in names[4:]:
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default is None
    assert MaskedContrastiveLoss().last_used is None
    assert callable(KWClip_GeneralTransformer.set_negative_bank) and callable(KWClip_GeneralTransformer.clear_negative_bank)
