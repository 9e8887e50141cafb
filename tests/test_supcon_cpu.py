"""SupConLoss without a GPU: the C entry points of csrc/supcon.hip are declared in include/speechclip_hip.h, bound from it and
exported by every library build, additive to the functions the header had, at the same ABI version; constructor and state dict are the
reference's; every refusal - the module's ValueErrors, ops' operand checks, the C argument checks - comes before any launch; the
model builds with ``cl_loss.type: SupConLoss`` and trains its temperature."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sc_supcon_fwd", "sc_supcon_grad", "sc_supcon_workspace_floats")
GIB = 1 << 30


# ---------------------------------------------------------------------------------------------------- declared, bound, exported
def _declared(text):
    return re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_symbols_declared_in_the_header_bound_and_exported():
    import speechclip_plus_amd as sc
    from speechclip_plus_amd import _lib, build, losses, ops
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    assert set(NEW_SYMBOLS) <= set(_declared(text)) and set(NEW_SYMBOLS) <= set(_lib.HEADER.functions)
    assert "losses.py:8-123" in text and 'extern "C"' in text
    assert {"sc_supcon_fwd", "sc_supcon_grad"} <= set(_lib.SIGNATURES) and "sc_supcon_workspace_floats" not in _lib.SIGNATURES
    assert _lib.HEADER.functions["sc_supcon_workspace_floats"] == (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32])
    assert _lib.DEFINES["SC_SUPCON_MAX_LOGIT_BYTES"] == GIB and ops.SUPCON_MAX_LOGIT_BYTES == GIB
    v, f = ctypes.c_void_p, ctypes.c_float
    i32 = ctypes.c_int32
    assert _lib.SIGNATURES["sc_supcon_fwd"] == [v, i32, i32, i32, i32, v, v, v, f, v, v, v, v, v, v, v]
    assert _lib.SIGNATURES["sc_supcon_grad"] == [v, v, v, i32, i32, i32, v, v, v, v, f, v, v, v]
    for path in (_lib.LIB_PATH, _lib.DIAG_LIB_PATH, _lib.GELU_EXACT_LIB_PATH):           # all three link the same objects
        cdll = _lib._load(path)
        for name in NEW_SYMBOLS:
            restype, argtypes = _lib.HEADER.functions[name]
            fn = getattr(cdll, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes, (path, name)
    assert "supcon.hip" in build.SOURCES
    assert callable(ops.supcon_fwd) and callable(ops.supcon_grad)
    assert sc.SupConLoss is losses.SupConLoss and "SupConLoss" in sc.__all__ and "MaskedContrastiveLoss" in sc.__all__


def test_one_header_declares_them_once_and_the_abi_version_stays():
    """The loss's three and the quantiser modes' five entry points are declared exactly once, in the one header, beside the 131
    functions it had; no side header and no second table is left; the additions did not move the ABI version."""
    from speechclip_plus_amd import _lib
    eight = NEW_SYMBOLS + ("sc_vq_gumbel_f32", "sc_vq_noisy_rowstats", "sc_vq_soft_prob_f32", "sc_vq_soft_split_bf16", "sc_vq_soft_bwd2")
    declared = _declared(open(_lib.HEADER_PATH).read())
    assert all(declared.count(name) == 1 for name in eight)
    fns = list(_lib.HEADER.functions)
    assert len(fns) == 139 == len(set(declared)) and set(fns) == set(declared)
    assert len(set(fns) - set(eight)) == 131 and sorted(fns[-8:]) == sorted(eight)           # the former 131, then the two blocks
    assert _lib.DEFINES == {"SC_SEG_ROWS": 8, "SC_ATTN_SLACK": 64, "SC_CONV0_NSTAT": 66, "SC_WS_INFONCE": 0, "SC_WS_HUBERT_LAYER": 1,
                            "SC_SUPCON_MAX_LOGIT_BYTES": GIB}
    assert _lib.HEADER_PATH.endswith("speechclip_hip.h")
    assert not hasattr(_lib, "SUPCON_HEADER") and not hasattr(_lib, "VQ_HEADER")
    assert not os.path.exists(os.path.join(ROOT, "include", "speechclip_hip_supcon.h"))
    assert not os.path.exists(os.path.join(ROOT, "include", "speechclip_hip_vq.h"))
    assert _lib.lib().sc_abi_version() == 7


# ---------------------------------------------------------------------------------------------------- the C argument checks
def test_c_argument_checks_need_no_device():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()
    one = 16                                                         # a non-null, 16-byte aligned address that is never dereferenced

    def fwd(N=8, Na=8, bsz=4, E=8, labels=None, mask=None, C=one, out=one, bt=0.07):
        return lib.sc_supcon_fwd(C, N, Na, bsz, E, labels, mask, one, bt, out, out, out, out, out, out, None)

    def grad(N=8, Na=8, bsz=4, labels=None, mask=None, logits=one, bt=0.07):
        return lib.sc_supcon_grad(logits, one, one, N, Na, bsz, labels, mask, one, one, bt, one, one, None)
    assert fwd(E=6) == -1 and b"E %" in lib.sc_last_error()
    assert fwd(E=0) == -1 and b"E=0" in lib.sc_last_error()
    assert fwd(C=None) == -1 and b"null" in lib.sc_last_error()
    assert fwd(out=None) == -1 and b"null" in lib.sc_last_error()
    assert fwd(C=one + 4) == -1 and b"aligned" in lib.sc_last_error()
    assert fwd(N=8, Na=12) == -1 and b"Na" in lib.sc_last_error()
    assert fwd(N=8, Na=-1) == -1 and b"Na" in lib.sc_last_error()
    assert fwd(N=10, Na=10, bsz=4) == -1 and b"bsz" in lib.sc_last_error()
    assert fwd(bsz=0) == -1 and b"bsz" in lib.sc_last_error()
    assert fwd(labels=one, mask=one) == -1 and b"both" in lib.sc_last_error()
    assert fwd(bt=0.0) == -1 and b"base_temperature" in lib.sc_last_error()
    big = 16400                                                      # 16400^2 * 4 bytes > 1 GiB >= 16384^2 * 4
    assert fwd(N=big, Na=big, bsz=big) == -1 and b"1073741824" in lib.sc_last_error() and b"1 GiB" in lib.sc_last_error()
    assert fwd(N=0, Na=0, C=None, out=None) == 0                     # N = 0 launches nothing: no pointer is looked at
    assert grad(logits=None) == -1 and b"null" in lib.sc_last_error()
    assert grad(N=8, Na=9) == -1 and b"Na" in lib.sc_last_error()
    assert grad(N=big, Na=big, bsz=big) == -1 and b"1 GiB" in lib.sc_last_error()
    assert grad(labels=one, mask=one) == -1 and b"both" in lib.sc_last_error()
    assert grad(N=0, Na=0, logits=None) == 0
    ws = lib.sc_supcon_workspace_floats
    assert ws(0, 0) == 0 and ws(64, 64) == 4 * 64 + 4 and ws(100, 300) == 4 * 5 * 100 + 4 and ws(130, 130) == 4 * 3 * 130 + 4
    assert ws(12, 8) == -1 and b"Na" in lib.sc_last_error()
    assert ws(big, big) == -1 and b"1 GiB" in lib.sc_last_error()
    assert ws(16384, 16384) == 4 * 256 * 16384 + 4                   # exactly 1 GiB of logits is served


# ---------------------------------------------------------------------------------------------------- ops: operand checks first
def test_ops_refuse_bad_operands_before_any_launch():
    from speechclip_plus_amd import ops
    C, it = torch.zeros(8, 8), torch.ones(1)
    bad = [
        (dict(C=torch.zeros(8)), "C must be a 2-D"), (dict(C=C.double()), "C must be torch.float32"),
        (dict(C=torch.zeros(8, 6)), "multiple of 4"), (dict(C=torch.zeros(8, 16)[:, ::2]), "C must be contiguous"),
        (dict(bsz=3), "bsz 3"), (dict(bsz=0), "bsz 0"), (dict(Na=9), "Na 9"), (dict(Na=-1), "Na -1"),
        (dict(labels=torch.zeros(4, dtype=torch.int64), mask=torch.zeros(4, 4)), "labels and mask are both given"),
        (dict(labels=torch.zeros(4, dtype=torch.int32)), "labels must be torch.int64"), (dict(labels=torch.zeros(5, dtype=torch.int64)), "labels has shape"),
        (dict(mask=torch.zeros(4, 4, dtype=torch.float64)), "mask must be a torch.float32"), (dict(mask=torch.zeros(4, 5)), "mask has shape"),
        (dict(inv_temp=torch.ones(2)), "inv_temp must be"), (dict(inv_temp=0.07), "inv_temp must be"),
        (dict(base_temperature=0.0), "base_temperature"),
    ]
    for kw, msg in bad:
        args = dict(C=C, Na=8, bsz=4, labels=None, mask=None, inv_temp=it, base_temperature=0.07)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.supcon_fwd(**args)
    with pytest.raises(ValueError, match="1 GiB"):
        ops.supcon_operands("supcon_fwd", torch.zeros(16400, 4), 16400, 16400, None, None)
    with pytest.raises(RuntimeError, match="device tensors only"):   # CPU tensors are refused like every other op's
        ops.supcon_fwd(C, 8, 4, None, None, it)
    lg, v = torch.zeros(8, 8), torch.zeros(8)
    for args, msg in [((lg.double(), v, v, 4, None, None, it, it), "logits must be"), ((lg, v[:4], v, 4, None, None, it, it), "lse has shape"),
                      ((lg, v, v, 3, None, None, it, it), "bsz 3"), ((lg, v, v, 4, None, None, torch.ones(2), it), "gscale must be"),
                      ((lg, v, v, 4, torch.zeros(4, dtype=torch.int64), torch.zeros(4, 4), it, it), "both given"),
                      ((lg, v, v, 4, None, torch.zeros(4, 3), it, it), "mask must be")]:
        with pytest.raises(ValueError, match=msg):
            ops.supcon_grad(*args)
    with pytest.raises(RuntimeError, match="device tensors only"):
        ops.supcon_grad(lg, v, v, 4, None, None, it, it)


# ---------------------------------------------------------------------------------------------------- the module
def test_constructor_and_state_dict_are_the_references():
    from speechclip_plus_amd.losses import SupConLoss
    crit = SupConLoss()
    assert (crit.contrast_mode, crit.base_temperature, crit.learnable_temperature) == ("all", 0.07, True)
    assert isinstance(crit.temperature, torch.nn.Parameter) and crit.temperature.shape == (1,) and crit.temperature.dtype == torch.float32
    assert crit.temperature.item() == float(torch.tensor(0.07, dtype=torch.float32))         # T itself, not log(1 / T)
    assert list(crit.state_dict()) == ["temperature"] and crit.state_dict()["temperature"].shape == (1,)
    assert crit.current_temperature == crit.temperature.item()
    t = crit.temperature_for_logging
    assert isinstance(t, torch.Tensor) and t.dim() == 0 and not t.requires_grad and float(t) == crit.temperature.item()
    fixed = SupConLoss(temperature=0.1, contrast_mode="one", base_temperature=0.2, learnable_temperature=False)
    assert fixed.temperature == 0.1 and list(fixed.parameters()) == [] and list(fixed.state_dict()) == []
    assert fixed.current_temperature == 0.1 and fixed.temperature_for_logging == 0.1 and fixed.contrast_mode == "one"
    crit.load_state_dict({"temperature": torch.tensor([0.05])})                               # the reference's key and shape load
    assert abs(crit.current_temperature - 0.05) < 1e-8


def test_every_value_error_is_raised_before_any_launch():
    """CPU tensors throughout: a launch (or ops' own device check, a RuntimeError) would show as another exception."""
    from speechclip_plus_amd.losses import SupConLoss
    crit = SupConLoss()
    f = torch.zeros(6, 2, 8)
    labels = torch.arange(6)
    with pytest.raises(ValueError, match="at least 3 dimensions"):
        crit(f[:, 0])
    with pytest.raises(ValueError, match="both `labels` and `mask`"):
        crit(f, labels=labels, mask=torch.eye(6))
    with pytest.raises(ValueError, match="Num of labels"):
        crit(f, labels=labels[:5])
    with pytest.raises(ValueError, match="Unknown mode: some"):
        SupConLoss(contrast_mode="some")(f)
    with pytest.raises(ValueError, match="Unknown mode"):
        SupConLoss(contrast_mode="some")(feat_A=f[:, 0], feat_B=f[:, 1], index=labels)
    for kw in (dict(bank=torch.zeros(4, 8)), dict(neg_idx=torch.zeros(6, 2, dtype=torch.int64)), dict(bank_ids=torch.zeros(4, dtype=torch.int64)),
               dict(bank=torch.zeros(4, 8), bank_ids=torch.zeros(4, dtype=torch.int64), neg_idx=torch.zeros(6, 2, dtype=torch.int64))):
        with pytest.raises(ValueError, match="MaskedContrastiveLoss"):
            crit(feat_A=f[:, 0], feat_B=f[:, 1], index=labels, **kw)
    with pytest.raises(ValueError, match="Num of labels"):
        crit(feat_A=f[:, 0], feat_B=f[:, 1], index=labels[:5])
    with pytest.raises(ValueError, match="features"):
        crit()
    with pytest.raises(ValueError, match="not both"):
        crit(f, feat_A=f[:, 0], feat_B=f[:, 1])
    with pytest.raises(ValueError, match="one shape"):
        crit(feat_A=f[:, 0], feat_B=f[:5, 1])
    with pytest.raises(RuntimeError, match="device tensors only"):       # everything is in order: the first thing that needs the device
        crit(f, labels=labels)


# ---------------------------------------------------------------------------------------------------- the model
def _tiny_model(loss_args):
    import dataclasses
    from speechclip_plus_amd import Config, KWClip_GeneralTransformer, base_parallel_config, random_hubert_state_dict
    from speechclip_plus_amd import speech_encoder as se
    arch = dataclasses.replace(se.ARCHS["hubert"], layers=1, embed_dim=128, ffn_dim=256, heads=2, conv_dim=64, pos_conv_groups=2)
    cfg = base_parallel_config()
    cfg.cl_loss = Config({"type": "SupConLoss", "args": loss_args})
    return cfg, KWClip_GeneralTransformer(cfg, device="cpu", hubert_state_dict=random_hubert_state_dict(arch, seed=1), hubert_arch=arch), arch


def test_the_model_builds_with_supconloss_and_trains_its_temperature():
    from speechclip_plus_amd import KWClip_GeneralTransformer, random_hubert_state_dict
    from speechclip_plus_amd.losses import SupConLoss
    cfg, model, arch = _tiny_model({"temperature": 0.07, "contrast_mode": "all", "base_temperature": 0.07, "learnable_temperature": True})
    assert isinstance(model.criterion, SupConLoss) and "criterion.temperature" in model.state_dict()
    assert any(p is model.criterion.temperature for p in model.getTrainableParams())
    assert any(p is model.criterion.temperature for p in model.criterion.parameters() if p.requires_grad)    # train.py's replicated set
    # a checkpoint of the reference carries criterion.temperature with shape [1]: it loads by name and shape
    sd = {k: v.clone() for k, v in model.state_dict().items() if not k.startswith("audio_encoder.")}
    sd["criterion.temperature"] = torch.tensor([0.033])
    sd.update({"audio_encoder.encoder." + k: v for k, v in random_hubert_state_dict(arch, seed=1).items()})
    again = KWClip_GeneralTransformer.from_reference_checkpoint(cfg, sd, device="cpu", hubert_arch=arch)
    assert abs(again.criterion.temperature.item() - 0.033) < 1e-8 and "criterion.temperature" in again._reference_load_report["loaded"]
    _, fixed, _ = _tiny_model({"temperature": 0.1, "contrast_mode": "one", "learnable_temperature": False})
    assert fixed.criterion.temperature == 0.1 and fixed.criterion.contrast_mode == "one"
    assert "criterion.temperature" not in fixed.state_dict()
