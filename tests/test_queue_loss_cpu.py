"""The contrastive loss with a cross-batch queue, the checks that need no GPU: the new entries declared / bound / exported and their C
argument checks, the fp64 reference expression against oracle.loss_ref and against F.cross_entropy, the conditions that make the GPU
sweep's bounds bite (the queue and its id mask move the loss by far more than the bounds), the host layers' refusals in their order
(format errors before device errors, all before a launch), and the ring logic of model.set_negative_queue on a model built on the CPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import loss_cases as lc
import queue_loss_cases as qc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("sc_infonce_queue_fwd", "sc_infonce_queue_grad", "sc_infonce_queue_workspace_floats")


class _OnDevice(torch.Tensor):
    """a tensor that says it is on the device; the checks under test raise before anything reads it"""
    is_cuda = True


# ---------------------------------------------------------------------------------------------------- declared, bound, exported
def test_symbols_declared_bound_and_exported():
    from speechclip_plus_amd import _header, _lib, build, ops
    header = open(os.path.join(ROOT, "include", "speechclip_hip_queue.h")).read()
    declared = re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", _header._COMMENT.sub(" ", header))
    assert sorted(declared) == sorted(NAMES) == sorted(_lib.QUEUE_HEADER.functions)      # the side header holds these three, once each
    assert "avssl/module/losses.py:185-245" in header
    lib = _lib.lib()
    for path in (_lib.LIB_PATH, _lib.DIAG_LIB_PATH, _lib.GELU_EXACT_LIB_PATH):           # every build exports and binds them
        cdll = _lib._load(path)
        for name in NAMES:
            restype, argtypes = _lib.QUEUE_HEADER.functions[name]
            fn = getattr(cdll, name)
            assert restype is ctypes.c_int32 and fn.restype is restype and list(fn.argtypes) == argtypes, (path, name)
    assert not set(NAMES) & set(_lib.HEADER.functions) and lib.sc_abi_version() == 7     # speechclip_hip.h is as it was; additive
    assert "infonce_queue.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "infonce_queue.hip"))
    assert callable(ops.infonce_queue_fwd) and callable(ops.infonce_queue_grad) and callable(ops.queue_operands)
    assert ops.QUEUE_MAX_SCORES == 2 ** 26                             # the C side's twin is pinned by the argument checks below


def test_argument_checks_need_no_device():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()

    def fwd(Bg, E, Nq, ldx, a2b=1, b2a=1, ids=None, qids=None):
        return lib.sc_infonce_queue_fwd(None, None, ldx, ids, qids, None, None, None, None, Bg, E, Nq, a2b, b2a, None, None, None, None, None,
                                        None, None)

    def grad(Bg, Nq, ldx, a2b=1, b2a=1):
        return lib.sc_infonce_queue_grad(None, None, ldx, None, None, None, None, Bg, Nq, a2b, b2a, None, None)
    for E in (0, 6, 101, -4):
        assert fwd(3, E, 8, 8) == -1 and b"sc_infonce_queue_fwd" in lib.sc_last_error() and b"E %" in lib.sc_last_error(), E
    for name, f in (("fwd", lambda *a, **k: fwd(a[0], 64, *a[1:], **k)), ("grad", grad)):
        assert f(3, -1, 8) == -1 and b"0 <= Nq" in lib.sc_last_error(), name
        assert f(-1, 8, 8) == -1, name
        assert f(2 ** 13, 2 ** 13 + 1, 2 ** 13 + 4) == -1 and b"2^26" in lib.sc_last_error(), name          # one row of scores too many
        for ldx in (7, 9, 10, 4):
            assert f(3, 8, ldx) == -1 and b"16-byte rows" in lib.sc_last_error(), (name, ldx)
        assert f(3, 8, 8, a2b=0, b2a=0) == -1 and b"a2b | b2a" in lib.sc_last_error(), name
        assert f(3, 8, 8) == -1 and b"null pointer" in lib.sc_last_error(), name                            # everything else passed
        assert f(0, 8, 8) == 0 and f(3, 0, 0) == 0 and f(0, 0, 4) == 0, name                                # nothing to do: no launch
        assert f(0, 8, 7) == -1, name                                                                      # ... behind the range checks
    one = (ctypes.c_int64 * 4)()
    assert fwd(3, 64, 4, 4, ids=one) == -1 and b"come together" in lib.sc_last_error()                      # ids on one side only
    assert fwd(3, 64, 4, 4, qids=one) == -1 and b"come together" in lib.sc_last_error()
    ws = lib.sc_infonce_queue_workspace_floats        # 3 floats per (anchor, chunk, side); chunks of 4096 columns, of 2048 / 1024 while
    assert ws(512, 16384) == 6 * 512 * 4 and ws(64, 4096) == 6 * 64 * 4 and ws(64, 4097) == 6 * 64 * 5      # ... under 512 workgroups
    assert ws(256, 16384) == 6 * 256 * 4 and ws(130, 1000) == 6 * 130 and ws(1, 3) == 6 and ws(0, 8) == 0 and ws(8, 0) == 0
    assert ws(2 ** 13, 2 ** 13 + 1) == -1 and b"2^26" in lib.sc_last_error()


# ---------------------------------------------------------------------------------------------------- the reference expression
def _args(c):
    return c["A"], c["B"], c["ids"], c["queue_A"], c["queue_B"], c["queue_ids"]


@pytest.mark.parametrize("name", [None] + list(lc.VARIANTS))
def test_reference_with_an_empty_queue_is_the_oracle(name):
    """no rows, or every entry masked: loss and gradients of the helper's fp64 expression equal oracle.loss_ref's"""
    kw = lc.VARIANTS[name] if name else {}
    c = qc.make_case(130, 100, 1000, 40)
    ref = lc.loss_reference(c["A"], c["B"], c["ids"], **kw)
    empty = dict(c, queue_A=c["queue_A"][:0], queue_B=c["queue_B"][:0], queue_ids=c["queue_ids"][:0])
    one_id = dict(c, ids=torch.full_like(c["ids"], 7), queue_ids=torch.full_like(c["queue_ids"], 7))
    ref_one = lc.loss_reference(c["A"], c["B"], one_id["ids"], **kw)
    cases = [(empty, ref)] + ([] if kw.get("dcl") else [(one_id, ref_one)])       # one id and dcl: no negative at all, the loss is inf
    for case, r in cases:
        got = qc.queue_loss_reference(*_args(case), **kw)
        assert int(got["used_A"].max()) == 0 and int(got["used_B"].max()) == 0
        for k in ("loss", "lse_row", "lse_col", "dA", "dB") + (("dT",) if "dT" in r else ()):     # fp64 on both sides: rounding only
            assert bool(torch.isfinite(got[k]).all()) and lc.max_abs_err(got[k], r[k]) <= 1e-13 * max(1.0, float(r[k].abs().max())), k


@pytest.mark.parametrize("shape", [(5, 8, 3, 3), (130, 100, 1000, 40)])
def test_reference_one_sided_is_cross_entropy_over_the_wider_row(shape):
    """b2a off, no ids, no margin, no dcl: the loss is F.cross_entropy(cat([logits, x_A], 1), arange(Bg)) - an independent definition"""
    c = qc.make_case(*shape, with_ids=False)
    for T in qc.TEMPERATURES:
        got = qc.queue_loss_reference(*_args(c), temperature=T, b2a=False)
        a, b, q = c["A"].double().requires_grad_(True), c["B"].double().requires_grad_(True), c["queue_B"].double()
        ce = F.cross_entropy(torch.cat([a @ b.t() / T, a @ q.t() / T], 1), torch.arange(shape[0]))
        ce.backward()
        ce = ce.detach()
        assert abs(float(got["loss"]) - float(ce)) <= 1e-12 * max(1.0, abs(float(ce)))
        assert lc.scale_rel_err(got["dA"], a.grad) <= 1e-12 and lc.scale_rel_err(got["dB"], b.grad) <= 1e-12


@pytest.mark.parametrize("shape", qc.SHAPE_SWEEP, ids=lambda s: "x".join(map(str, s)))
def test_the_cases_make_the_bounds_bite(shape):
    """At every shape and both temperatures the queue moves the fp64 loss by >= 1e-3, and at the three masked shapes dropping the id
    mask over the queue moves it by >= 1e-2: a kernel that loses the extras or the mask cannot pass the sweep's 2e-5 loss bound."""
    c = qc.make_case(*shape)
    for T in qc.TEMPERATURES:
        with_q = float(qc.queue_loss_reference(*_args(c), temperature=T)["loss"])
        plain = float(lc.loss_reference(c["A"], c["B"], c["ids"], temperature=T)["loss"])
        print(f"CASE|{shape}|T {T}|plain {plain:.6f}|queue {with_q:.6f}")
        assert with_q - plain >= 1e-3, (shape, T, with_q, plain)
        if shape in qc.MASK_SHAPES:
            unmasked = float(qc.queue_loss_reference(*_args(c), temperature=T, mask_queue=False)["loss"])
            print(f"CASE|{shape}|T {T}|without the mask {unmasked:.6f}")
            assert unmasked - with_q >= 1e-2, (shape, T, unmasked, with_q)
    adm = qc.admitted(c["ids"], c["queue_ids"], shape[0], shape[2])
    if shape == (5, 8, 3, 3):
        assert int((~adm).sum()) == 6                                  # 40 % of the 15 entries are masked
    if shape == (1, 4, 3, 2):
        assert float(lc.loss_reference(c["A"], c["B"], c["ids"])["loss"]) == 0.0
    assert bool(adm.any(1).all())                                      # every anchor keeps an entry: the dcl loss stays finite at Bg = 1


# ---------------------------------------------------------------------------------------------------- refusals and their order
def _operands(Bg=4, E=8, Nq=6, on_device=False):
    t = {"A": torch.zeros(Bg, E), "B": torch.zeros(Bg, E), "ids": torch.zeros(Bg, dtype=torch.int64), "queue_A": torch.zeros(Nq, E),
         "queue_B": torch.zeros(Nq, E), "queue_ids": torch.ones(Nq, dtype=torch.int64)}
    return {k: v.as_subclass(_OnDevice) if on_device else v for k, v in t.items()}


def _crit(**kw):
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    return MaskedContrastiveLoss(**kw)


def _call(crit, t, **over):
    t = {**t, **over}
    return crit(t["A"], t["B"], t["ids"], queue_A=t["queue_A"], queue_B=t["queue_B"], queue_ids=t["queue_ids"])


def test_module_refusals_come_before_any_launch_in_order():
    """Every operand below is a host tensor (or says it is on the device and holds no device memory): a launch would fail, so each
    refusal is raised before one.  Each case carries every LATER defect too: the earlier refusal wins."""
    t = _operands()
    crit = _crit()
    grad_q = t["queue_B"].clone().requires_grad_(True)
    with pytest.raises(ValueError, match="a bank or a queue, not both"):                 # ... and one-sided ids, a grad queue, CPU
        crit(t["A"], t["B"], None, bank=torch.zeros(6, 8), neg_idx=torch.zeros(4, 2, dtype=torch.int64), queue_B=grad_q,
             queue_ids=t["queue_ids"])
    with pytest.raises(ValueError, match="ids on one side only"):                        # ... and a missing queue, a grad queue, CPU
        _call(crit, t, ids=None, queue_A=None, queue_B=grad_q)
    with pytest.raises(ValueError, match="ids on one side only"):
        _call(crit, t, queue_ids=None)
    with pytest.raises(ValueError, match="B must be torch.float32"):                     # dtypes and shapes of the batch
        _call(crit, t, B=t["B"].double(), queue_A=None)
    with pytest.raises(ValueError, match="multiple of 4"):
        _call(crit, dict(t, A=torch.zeros(4, 6), B=torch.zeros(4, 6)))
    with pytest.raises(ValueError, match="a2b is on and queue_B is missing"):            # a missing queue, ahead of the other's dtype
        _call(crit, t, queue_B=None, queue_A=t["queue_A"].double())
    with pytest.raises(ValueError, match="b2a is on and queue_A is missing"):
        _call(crit, t, queue_A=None, queue_B=grad_q)
    with pytest.raises(ValueError, match="queue_A must be torch.float32"):
        _call(crit, t, queue_A=t["queue_A"].half(), queue_B=grad_q)
    with pytest.raises(ValueError, match="queue_B must be a 2-D tensor"):
        _call(crit, t, queue_B=torch.zeros(6))
    with pytest.raises(ValueError, match=r"queue_B \(6, 12\) must share E = 8"):
        _call(crit, t, queue_B=torch.zeros(6, 12))
    with pytest.raises(ValueError, match="one ring position, one length"):
        _call(crit, t, queue_A=torch.zeros(5, 8), queue_B=grad_q)
    with pytest.raises(ValueError, match=r"queue_ids has shape \(5,\), expected \(6,\)"):
        _call(crit, t, queue_ids=t["queue_ids"][:5], queue_B=grad_q)
    with pytest.raises(ValueError, match="ids must be torch.int64"):
        _call(crit, t, ids=t["ids"].int())
    with pytest.raises(ValueError, match="requires_grad"):                               # a grad queue, ahead of CPU
        _call(crit, t, queue_B=grad_q)
    with pytest.raises(RuntimeError, match="MaskedContrastiveLoss runs on the HIP kernels: device tensors only"):
        _call(crit, t)
    dev = _operands(on_device=True)
    with pytest.raises(RuntimeError, match=r"device tensors only \(queue_ids\)"):        # the ids alone on the host are enough
        _call(crit, dev, queue_ids=t["queue_ids"])
    # a one-sided loss needs only the queue of its own side, and ignores the other
    with pytest.raises(RuntimeError, match=r"device tensors only \(A\)"):
        _call(_crit(b2a=False), t, queue_A=None)
    with pytest.raises(RuntimeError, match=r"device tensors only \(A\)"):
        _call(_crit(a2b=False), t, queue_B=grad_q)
    with pytest.raises(ValueError, match="a2b is on and queue_B is missing"):
        _call(_crit(b2a=False), t, queue_B=None)


def test_the_limit_on_the_scores_is_stated():
    from speechclip_plus_amd import ops
    big = torch.zeros(1, 4).expand(2 ** 13 + 1, 4).as_subclass(_OnDevice)                # no memory behind either
    anchors = torch.zeros(1, 4).expand(2 ** 13, 4).as_subclass(_OnDevice)
    with pytest.raises(ValueError, match=r"at most 2\^26 \(67108864, 256 MiB of fp32\)"):
        ops.queue_operands("queue_operands", anchors, anchors, big, big, None, None, True, True)
    with pytest.raises(ValueError, match="a2b and b2a are both off"):
        ops.queue_operands("queue_operands", anchors, anchors, big, big, None, None, False, False)


def test_supcon_refuses_the_queue():
    from speechclip_plus_amd.losses import SupConLoss
    t = _operands()
    for kw in (dict(queue_A=t["queue_A"]), dict(queue_B=t["queue_B"]), dict(queue_ids=t["queue_ids"])):
        with pytest.raises(ValueError, match="MaskedContrastiveLoss"):
            SupConLoss()(feat_A=t["A"], feat_B=t["B"], index=t["ids"], **kw)


def test_forward_keeps_its_parameters_and_the_call_takes_the_queue():
    from speechclip_plus_amd.losses import MaskedContrastiveLoss
    assert list(inspect.signature(MaskedContrastiveLoss.forward).parameters) == ["self", "feat_A", "feat_B", "index", "bank", "bank_ids", "neg_idx"]
    call = inspect.signature(MaskedContrastiveLoss.__call__).parameters
    for k in ("queue_A", "queue_B", "queue_ids"):
        assert call[k].kind is inspect.Parameter.KEYWORD_ONLY and call[k].default is None
    crit = MaskedContrastiveLoss()
    with pytest.raises(ValueError, match="ids on one side only"):      # a refused call leaves nothing behind for the next one
        crit(torch.zeros(2, 4), torch.zeros(2, 4), None, queue_B=torch.zeros(3, 4), queue_ids=torch.zeros(3, dtype=torch.int64))
    assert crit._queue == (None, None, None)
    assert MaskedContrastiveLoss().last_queue_used is None


# ---------------------------------------------------------------------------------------------------- the ring
class _Recorder(torch.nn.Module):
    """stands in for the criterion: keeps copies of what compute_loss hands it"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, feat_A, feat_B, index=None, **kw):
        self.calls.append({k: v.clone() for k, v in kw.items()})
        return (feat_A * feat_B).sum()


def _bare_model(E, two_terms=False):
    """compute_loss reads ``config``, ``criterion`` and the rings only: no encoder is built"""
    from speechclip_plus_amd import KWClip_GeneralTransformer, base_parallel_config
    model = KWClip_GeneralTransformer.__new__(KWClip_GeneralTransformer)
    torch.nn.Module.__init__(model)
    model.config = base_parallel_config()
    if two_terms:
        model.config.model_settings.cascaded_objective_weight = 1.0
    model.criterion = _Recorder()
    model._device, model.subword_embd_dim = torch.device("cpu"), E
    return model


def _batch(n, E, start, two_terms=False):
    """rows whose every element is their own serial number (+ 0.5 on the image side, + 0.25 on the cascaded side), ids = 100 + serial"""
    serial = torch.arange(start, start + n, dtype=torch.float32)[:, None].expand(n, E)
    d = {"id": 100 + torch.arange(start, start + n), "image_feat": serial + 0.5, "parallel_audio_feat": serial.clone()}
    if two_terms:
        d["cascaded_audio_feat"] = serial + 0.25
    return d


def test_ring_fill_wrap_and_clear():
    E = 4
    model = _bare_model(E)
    keys = set(model.state_dict().keys())
    model.set_negative_queue(10)
    assert set(model.state_dict().keys()) == keys and not list(model.buffers())          # plain attributes: the keys stay the reference's
    q = model._neg_queue
    assert set(q["speech"]) == {"parallel"} and q["image"].shape == (10, E) and q["ids"].dtype == torch.int64
    model.train()
    calls = model.criterion.calls
    model.compute_loss(_batch(4, E, 0))                                # sees nothing; stashes serials 0 .. 3
    assert calls[-1]["queue_A"].shape == (0, E) and calls[-1]["queue_ids"].shape == (0,) and (q["head"], q["n_valid"]) == (0, 0)
    model.compute_loss(_batch(4, E, 4))                                # sees 0 .. 3
    assert (q["head"], q["n_valid"]) == (4, 4)
    assert calls[-1]["queue_A"][:, 0].tolist() == [0, 1, 2, 3] and calls[-1]["queue_B"][:, 0].tolist() == [0.5, 1.5, 2.5, 3.5]
    assert calls[-1]["queue_ids"].tolist() == [100, 101, 102, 103]                       # ids follow rows
    model.eval()
    before = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in q.items() if k in ("image", "ids", "head", "n_valid")}
    model.compute_loss(_batch(4, E, 50))                               # eval mode: neither read nor written, nothing stashed
    assert calls[-1] == {} and (q["head"], q["n_valid"]) == (4, 4) and torch.equal(q["image"], before["image"])
    model.train()
    model.compute_loss(_batch(4, E, 8))                                # sees 0 .. 7 (the stash of the last TRAIN call)
    assert (q["head"], q["n_valid"]) == (8, 8) and calls[-1]["queue_A"][:, 0].tolist() == list(range(8))
    model.compute_loss(_batch(4, E, 12))                               # 8 .. 11 straddle the end: rows 8, 9 and 0, 1
    assert (q["head"], q["n_valid"]) == (2, 10)
    assert calls[-1]["queue_A"][:, 0].tolist() == [10, 11, 2, 3, 4, 5, 6, 7, 8, 9]
    assert calls[-1]["queue_ids"].tolist() == [110, 111, 102, 103, 104, 105, 106, 107, 108, 109]
    assert calls[-1]["queue_B"][:, 0].tolist() == [10.5, 11.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, 8.5, 9.5]
    model.compute_loss(_batch(25, E, 16))                              # writes 12 .. 15; stashes a batch longer than the ring
    assert (q["head"], q["n_valid"]) == (6, 10)
    model.compute_loss(_batch(1, E, 41))                               # ... of which the last ten rows stay: 31 .. 40 from row 6 on
    assert (q["head"], q["n_valid"]) == (6, 10)
    assert calls[-1]["queue_A"][:, 0].tolist() == [35, 36, 37, 38, 39, 40, 31, 32, 33, 34]
    model.clear_negative_queue()
    model.compute_loss(_batch(4, E, 0))
    assert calls[-1] == {} and model._neg_queue is None
    model.set_negative_queue(3)                                        # a fresh ring starts empty
    model.compute_loss(_batch(2, E, 0))
    assert calls[-1]["queue_B"].shape == (0, E)


def test_one_speech_ring_per_branch_term():
    E = 4
    model = _bare_model(E, two_terms=True)
    model.set_negative_queue(6)
    assert set(model._neg_queue["speech"]) == {"cascaded", "parallel"}
    model.train()
    model.compute_loss(_batch(3, E, 0, two_terms=True))
    model.compute_loss(_batch(3, E, 3, two_terms=True))
    casc, par = model.criterion.calls[-2:]                             # compute_loss's order: cascaded, then parallel
    assert casc["queue_A"][:, 0].tolist() == [0.25, 1.25, 2.25] and par["queue_A"][:, 0].tolist() == [0, 1, 2]
    assert torch.equal(casc["queue_B"], par["queue_B"]) and torch.equal(casc["queue_ids"], par["queue_ids"])


def test_bank_and_queue_exclude_each_other_and_sizes_are_checked():
    model = _bare_model(4)
    with pytest.raises(ValueError, match="size >= 1"):
        model.set_negative_queue(0)
    model.set_negative_queue(8)
    with pytest.raises(ValueError, match="a bank or a queue, not both"):
        model.set_negative_bank(torch.zeros(4, 4), torch.zeros(4, dtype=torch.int64), 2)
    model.clear_negative_queue()
    model._neg_bank = object()                                         # a bank is set (building one needs the device)
    with pytest.raises(ValueError, match="a bank or a queue, not both"):
        model.set_negative_queue(8)
    model.clear_negative_bank()
    model.set_negative_queue(8)
    model.train()
    with pytest.raises(ValueError, match="rows of width 4"):
        model.compute_loss(_batch(2, 8, 0))
