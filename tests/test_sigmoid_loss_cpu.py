"""SigmoidContrastiveLoss without a GPU: the three C entry points of csrc/sigmoid_loss.hip are declared once in a header of their own,
bound with its types and exported by every library build, beside the other two headers as they were and at the same ABI version; the
C argument checks come before any HIP call; constructor, state dict and the two ValueErrors; ``sigmoid_loss_operands`` refuses in its
order, all before a launch; the bank and the queue are refused by name; the model builds with ``cl_loss.type: SigmoidContrastiveLoss``
and trains both scalars."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sc_sigmoid_loss_fwd", "sc_sigmoid_loss_grad", "sc_sigmoid_loss_workspace_floats")
GIB = 1 << 30


class _OnDevice(torch.Tensor):
    """a tensor that says it is on the device; the checks under test raise before anything reads it"""
    is_cuda = True


# ---------------------------------------------------------------------------------------------------- declared, bound, exported
def test_symbols_declared_once_bound_and_exported():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import _header, _lib, build, losses, ops
    fns = _lib.SIGMOID_HEADER.functions
    header = open(os.path.join(ROOT, "include", "speechclip_hip_sigmoid.h")).read()
    declared = re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", _header._COMMENT.sub(" ", header))
    assert sorted(declared) == sorted(NAMES) == sorted(_lib.SIGMOID_HEADER.functions)       # these three, once each
    assert not _lib.SIGMOID_HEADER.structs and not _lib.SIGMOID_HEADER.defines             # prototypes only
    assert 'extern "C"' in header and "avssl" not in header                                # nothing of the reference to cite
    assert not set(NAMES) & (set(_lib.HEADER.functions) | set(_lib.QUEUE_HEADER.functions))
    v, i32 = ctypes.c_void_p, ctypes.c_int32
    assert fns["sc_sigmoid_loss_workspace_floats"] == (ctypes.c_int64, [i32])
    assert fns["sc_sigmoid_loss_fwd"] == (i32, [v, v, i32, i32, v, i32, v, v, v, v, v, v, v])
    assert fns["sc_sigmoid_loss_grad"] == (i32, [v, i32, v, i32, v, v, v, v, v, v, v])
    for path in (_lib.LIB_PATH, _lib.DIAG_LIB_PATH, _lib.GELU_EXACT_LIB_PATH):             # every build exports and binds them
        cdll = _lib._load(path)
        for name in NAMES:
            restype, argtypes = fns[name]
            fn = getattr(cdll, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes, (path, name)
    assert _lib.lib().sc_abi_version() == 7 and len(_lib.HEADER.functions) == 139 and len(_lib.QUEUE_HEADER.functions) == 3
    assert "sigmoid_loss.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "sigmoid_loss.hip"))
    assert callable(ops.sigmoid_loss_fwd) and callable(ops.sigmoid_loss_grad) and callable(ops.sigmoid_loss_operands)
    assert ops.SIGMOID_MAX_DOT_BYTES == GIB                            # the C side's twin is pinned by the argument checks below
    assert sc.SigmoidContrastiveLoss is losses.SigmoidContrastiveLoss and "SigmoidContrastiveLoss" in sc.__all__


def test_c_argument_checks_need_no_device():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()
    one = 16                                                           # a non-null, 16-byte aligned address that is never dereferenced

    def fwd(B=8, E=8, mode=0, A=one, Bm=one, out=one):
        return lib.sc_sigmoid_loss_fwd(A, Bm, B, E, None, mode, one, one, out, out, out, out, None)

    def grad(B=8, mode=0, s=one, out=one):
        return lib.sc_sigmoid_loss_grad(s, B, None, mode, one, one, one, out, out, out, None)
    big = 16400                                                        # 16400^2 * 4 bytes > 1 GiB >= 16384^2 * 4
    for B in (0, -3):                                                  # each call carries every LATER defect too: the earlier check wins
        assert fwd(B=B, E=6, mode=5, A=None) == -1 and b"sc_sigmoid_loss_fwd: B >= 1" in lib.sc_last_error()
        assert grad(B=B, mode=5, s=None) == -1 and b"sc_sigmoid_loss_grad: B >= 1" in lib.sc_last_error()
    for E in (0, 6, 101, -4):
        assert fwd(E=E, mode=5, B=big, A=None) == -1 and b"E %" in lib.sc_last_error(), E
    for mode in (-1, 3):
        assert fwd(mode=mode, B=big, A=None) == -1 and b"same_id" in lib.sc_last_error()
        assert grad(mode=mode, B=big, s=None) == -1 and b"same_id" in lib.sc_last_error()
    assert fwd(B=big, A=None) == -1 and b"1073741824" in lib.sc_last_error() and b"1 GiB" in lib.sc_last_error()
    assert grad(B=big, s=None) == -1 and b"1073741824" in lib.sc_last_error() and b"1 GiB" in lib.sc_last_error()
    assert fwd(A=None, Bm=one + 4) == -1 and b"null" in lib.sc_last_error()
    assert fwd(out=None) == -1 and b"null" in lib.sc_last_error()
    assert grad(s=None) == -1 and b"null" in lib.sc_last_error() and grad(out=None) == -1 and b"null" in lib.sc_last_error()
    assert fwd(A=one + 4) == -1 and b"aligned" in lib.sc_last_error()
    assert fwd(Bm=one + 8) == -1 and b"aligned" in lib.sc_last_error()
    ws = lib.sc_sigmoid_loss_workspace_floats                          # per tile the sum and three counts, then the ticket word + padding
    assert ws(1) == 8 and ws(64) == 8 and ws(65) == 4 * 4 + 4 and ws(130) == 4 * 9 + 4 and ws(512) == 4 * 64 + 4
    assert ws(16384) == 4 * 256 * 256 + 4                              # exactly 1 GiB of dots is served
    assert ws(0) == -1 and b"B >= 1" in lib.sc_last_error()
    assert ws(big) == -1 and b"1 GiB" in lib.sc_last_error()


# ---------------------------------------------------------------------------------------------------- the module
def test_constructor_state_dict_and_the_two_value_errors():
    from speechclip_plus_amd.losses import SigmoidContrastiveLoss
    crit = SigmoidContrastiveLoss()
    assert (crit.learnable, crit.same_id) == (True, "ignore") and crit.last_counts is None
    for p in (crit.logit_scale, crit.logit_bias):
        assert isinstance(p, torch.nn.Parameter) and p.shape == () and p.dtype == torch.float32
    assert crit.logit_scale.item() == float(torch.tensor(math.log(10.0), dtype=torch.float32)) and crit.logit_bias.item() == -10.0
    assert list(crit.state_dict()) == ["logit_scale", "logit_bias"] and len(list(crit.parameters())) == 2
    assert abs(crit.current_temperature - 0.1) < 1e-7 and isinstance(crit.current_temperature, float)
    t, b = crit.temperature_for_logging, crit.bias_for_logging
    assert all(isinstance(x, torch.Tensor) and x.dim() == 0 and not x.requires_grad for x in (t, b))
    assert abs(float(t) - 0.1) < 1e-7 and float(b) == -10.0
    fixed = SigmoidContrastiveLoss(temperature=0.07, bias=-5.0, learnable=False, same_id="positive")
    assert list(fixed.parameters()) == [] and list(fixed.state_dict()) == ["logit_scale", "logit_bias"] and fixed.same_id == "positive"
    assert all(x.shape == () and not x.requires_grad for x in fixed.state_dict().values())
    assert isinstance(fixed.temperature_for_logging, float) and isinstance(fixed.bias_for_logging, float)
    assert abs(fixed.temperature_for_logging - 0.07) < 1e-7 and fixed.bias_for_logging == -5.0
    fixed.load_state_dict({"logit_scale": torch.tensor(math.log(20.0)), "logit_bias": torch.tensor(-3.0)})
    assert abs(fixed.temperature_for_logging - 0.05) < 1e-7 and fixed.bias_for_logging == -3.0 and abs(fixed.current_temperature - 0.05) < 1e-7
    crit.load_state_dict(fixed.state_dict())                                              # the keys are the same either way
    assert abs(crit.current_temperature - 0.05) < 1e-7 and float(crit.bias_for_logging) == -3.0
    with pytest.raises(ValueError, match="same_id 'some'"):
        SigmoidContrastiveLoss(same_id="some")
    with pytest.raises(ValueError, match="same_id None"):
        SigmoidContrastiveLoss(same_id=None)


def test_the_bank_and_the_queue_are_refused_by_name():
    from speechclip_plus_amd.losses import SigmoidContrastiveLoss
    crit = SigmoidContrastiveLoss()
    A, ids = torch.zeros(6, 8), torch.arange(6)
    for kw in (dict(bank=torch.zeros(4, 8)), dict(neg_idx=torch.zeros(6, 2, dtype=torch.int64)), dict(bank_ids=torch.zeros(4, dtype=torch.int64)),
               dict(queue_A=torch.zeros(0, 8)), dict(queue_B=torch.zeros(4, 8)), dict(queue_ids=torch.zeros(4, dtype=torch.int64))):
        with pytest.raises(ValueError, match="MaskedContrastiveLoss"):
            crit(A.double(), A, ids, **kw)                                                 # ... ahead of the dtype of the batch
    with pytest.raises(ValueError, match="MaskedContrastiveLoss"):
        crit(feat_A=A, feat_B=A, index=ids, queue_A=A, queue_B=A, queue_ids=ids)
    with pytest.raises(RuntimeError, match="SigmoidContrastiveLoss runs on the HIP kernels: device tensors only"):
        crit(feat_A=A, feat_B=A, index=ids)                                               # everything in order: the first thing that needs the device
    with pytest.raises(RuntimeError, match="device tensors only"):
        crit(A.bfloat16(), A.half())                                                      # half-precision features are the module's to widen


# ---------------------------------------------------------------------------------------------------- refusals and their order
def test_operand_refusals_come_before_any_launch_in_order():
    """Every operand is a host tensor (or says it is on the device and holds no device memory): a launch would fail, so each refusal is
    raised before one.  Each case carries every LATER defect too: the earlier refusal wins."""
    from speechclip_plus_amd import ops
    A, ids = torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64)
    big = torch.zeros(1, 4).expand(16400, 4)                                               # no memory behind it

    def call(A=A, B=A, ids=ids, same_id="ignore"):
        return ops.sigmoid_loss_operands("sigmoid_loss_operands", A, B, ids, same_id)
    # 1. dtypes and shapes of the batch
    with pytest.raises(ValueError, match="A must be a 2-D tensor"):
        call(A=torch.zeros(8), B=A.double(), ids=ids.int(), same_id="some")
    with pytest.raises(ValueError, match="B must be a 2-D tensor"):
        call(B=torch.zeros(4, 8, 1), ids=ids.int(), same_id="some")
    with pytest.raises(ValueError, match="A must be torch.float32, not torch.float64"):
        call(A=A.double(), B=torch.zeros(5, 8), ids=ids.int(), same_id="some")
    with pytest.raises(ValueError, match="B must be torch.float32, not torch.float16"):
        call(B=torch.zeros(5, 8).half(), ids=ids.int(), same_id="some")
    with pytest.raises(ValueError, match="multiple of 4"):
        call(A=torch.zeros(4, 6), B=torch.zeros(5, 6), ids=ids.int(), same_id="some")
    with pytest.raises(ValueError, match="at least one row"):
        call(A=torch.zeros(0, 8), B=torch.zeros(5, 8), ids=ids.int(), same_id="some")
    # 2. one shape
    with pytest.raises(ValueError, match=r"A \(4, 8\) and B \(5, 8\) must be one shape"):
        call(B=torch.zeros(5, 8), ids=ids.int(), same_id="some")
    with pytest.raises(ValueError, match=r"must be one shape"):
        call(B=torch.zeros(4, 12), ids=ids[:3], same_id="some")
    # 3. the id vector
    with pytest.raises(ValueError, match="ids must be torch.int64"):
        call(ids=ids.int(), same_id="some")
    with pytest.raises(ValueError, match=r"ids has shape \(3,\), expected \(4,\)"):
        call(ids=ids[:3], same_id="some")
    with pytest.raises(ValueError, match="ids must be a tensor"):
        call(ids=[0, 1, 2, 3], same_id="some")
    # 4. the mode string
    with pytest.raises(ValueError, match="same_id 'some' is none of 'ignore', 'positive', 'negative'"):
        call(A=big, B=big, ids=None, same_id="some")
    with pytest.raises(ValueError, match="same_id 0"):
        call(same_id=0)
    # 5. the size limit, stated
    with pytest.raises(ValueError, match=r"above the limit of 1073741824 \(1 GiB\)"):
        call(A=big, B=big, ids=None)
    # 6. the device, last
    with pytest.raises(RuntimeError, match=r"sigmoid_loss_operands runs on the HIP kernels: device tensors only \(A\)"):
        call()
    dev = A.as_subclass(_OnDevice)
    with pytest.raises(RuntimeError, match=r"device tensors only \(B\)"):
        call(A=dev)
    with pytest.raises(RuntimeError, match=r"device tensors only \(ids\)"):                # the ids alone on the host are enough
        call(A=dev, B=dev)
    assert [call(A=dev, B=dev, ids=None, same_id=m) for m in ("ignore", "positive", "negative")] == [0, 1, 2]
    ok = torch.zeros(1, 4).expand(16384, 4).as_subclass(_OnDevice)                         # exactly 1 GiB of dots is served
    assert call(A=ok, B=ok, ids=None) == 0


def test_fwd_and_grad_refuse_before_any_launch():
    from speechclip_plus_amd import ops
    A, one = torch.zeros(4, 8), torch.ones(1)
    with pytest.raises(ValueError, match="A must be torch.float32"):
        ops.sigmoid_loss_fwd(A.half(), A.half(), None, one, one)
    with pytest.raises(ValueError, match="same_id 'some'"):
        ops.sigmoid_loss_fwd(A, A, None, one, one, "some")
    with pytest.raises(RuntimeError, match="device tensors only"):
        ops.sigmoid_loss_fwd(A, A, None, one, one)
    dev = A.as_subclass(_OnDevice)
    with pytest.raises(ValueError, match="scale must be a one-element torch.float32"):
        ops.sigmoid_loss_fwd(dev, dev, None, torch.ones(2), one)
    with pytest.raises(ValueError, match="bias must be a one-element torch.float32"):
        ops.sigmoid_loss_fwd(dev, dev, None, one, -10.0)
    s = torch.zeros(4, 4)
    for args, msg in [((s.double(), None, one, one, one), "s must be"), ((torch.zeros(4, 5), None, one, one, one), "s must be"),
                      ((s, torch.zeros(3, dtype=torch.int64), one, one, one), "ids has shape"), ((s, None, one, one, one, "some"), "same_id 'some'"),
                      ((s.as_subclass(_OnDevice), None, torch.ones(2), one, one), "gscale must be")]:
        with pytest.raises(ValueError, match=msg):
            ops.sigmoid_loss_grad(*args)
    with pytest.raises(RuntimeError, match="device tensors only"):
        ops.sigmoid_loss_grad(s, None, one, one, one)


# ---------------------------------------------------------------------------------------------------- the model
def test_the_model_builds_with_the_sigmoid_loss_and_trains_both_scalars():
    import dataclasses
    from speechclip_plus_amd import Config, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    from speechclip_plus_amd import speech_encoder as se
    from speechclip_plus_amd.losses import SigmoidContrastiveLoss
    arch = dataclasses.replace(se.ARCHS["hubert"], layers=1, embed_dim=128, ffn_dim=256, heads=2, conv_dim=64, pos_conv_groups=2)

    def build(args):
        cfg = base_parallel_config()
        cfg.cl_loss = Config({"type": "SigmoidContrastiveLoss", "args": args})
        return KWClip_GeneralTransformer(cfg, device="cpu", hubert_state_dict=random_hubert_state_dict(arch, seed=1), hubert_arch=arch)
    model = build({"temperature": 0.1, "bias": -10.0, "learnable": True, "same_id": "ignore"})
    crit = model.criterion
    assert isinstance(crit, SigmoidContrastiveLoss)
    assert {"criterion.logit_scale", "criterion.logit_bias"} <= set(model.state_dict())
    for p in (crit.logit_scale, crit.logit_bias):
        assert any(q is p for q in model.getTrainableParams())
        assert any(q is p for q in crit.parameters() if q.requires_grad)                   # train.py's replicated set
    fixed = build({"learnable": False, "same_id": "negative"})
    assert list(fixed.criterion.parameters()) == [] and {"criterion.logit_scale", "criterion.logit_bias"} <= set(fixed.state_dict())
    assert not any(q is fixed.criterion.logit_scale or q is fixed.criterion.logit_bias for q in fixed.getTrainableParams())
    assert fixed.criterion.same_id == "negative" and fixed.criterion.bias_for_logging == -10.0
