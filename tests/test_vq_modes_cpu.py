"""The quantiser's soft / Gumbel / learnable-temperature modes without a GPU: the C entry points (csrc/vq.hip) are declared in
include/speechclip_hip.h, bound from it and exported by every library build, additive to the functions the header had, at the same ABI
version; the constructor takes every mode; every refusal - the module's, ops' operand checks, the C argument
checks - comes before any launch; a table holds no soft operand until a soft call asks for it."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sc_vq_gumbel_f32", "sc_vq_noisy_rowstats", "sc_vq_soft_prob_f32", "sc_vq_soft_split_bf16", "sc_vq_soft_bwd2")


def _declared(text):
    return re.findall(r"\b(sc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_symbols_declared_in_the_header_bound_and_exported():
    from speechclip_plus_amd import _lib, build, ops
    text = open(os.path.join(ROOT, "include", "speechclip_hip.h")).read()
    assert set(NEW_SYMBOLS) <= set(_declared(text)) and set(NEW_SYMBOLS) <= set(_lib.HEADER.functions) and set(NEW_SYMBOLS) <= set(_lib.SIGNATURES)
    assert "my_vector_quantizer.py:124-137" in text and 'extern "C"' in text
    v, f, i32, i64, u32 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
    assert _lib.SIGNATURES["sc_vq_gumbel_f32"] == [v, i64, i32, i32, u32, v]
    assert _lib.SIGNATURES["sc_vq_noisy_rowstats"] == [v, i64, i32, i32, f, u32, i32, v, v, v, v]
    assert _lib.SIGNATURES["sc_vq_soft_prob_f32"] == [v, i64, v, v, i32, i32, f, u32, i32, v, i64, v]
    assert _lib.SIGNATURES["sc_vq_soft_split_bf16"] == [v, i64, v, v, i32, i32, f, u32, i32, v, i32, i32, v]
    assert _lib.SIGNATURES["sc_vq_soft_bwd2"] == [v, i64, v, v, v, i64, i32, i32, i32, f, u32, i32, v, i64, i32, v, v]
    for path in (_lib.LIB_PATH, _lib.DIAG_LIB_PATH, _lib.GELU_EXACT_LIB_PATH):           # all three link the same objects
        cdll = _lib._load(path)
        for name in NEW_SYMBOLS:
            restype, argtypes = _lib.HEADER.functions[name]
            fn = getattr(cdll, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes, (path, name)
    assert "vq.hip" in build.SOURCES and "vq_modes.hip" not in build.SOURCES
    for name in ("vq_gumbel", "vq_noisy_rowstats", "vq_soft_prob", "vq_soft_split", "vq_soft_table", "vq_soft_product", "vq_soft_bwd2"):
        assert callable(getattr(ops, name))


def test_one_header_declares_them_once_and_the_abi_version_stays():
    """The modes' five and the supervised contrastive loss's three entry points are declared exactly once, in the one header, beside
    the 131 functions it had; no side header and no second table is left; the additions did not move the ABI version."""
    from speechclip_plus_amd import _lib
    eight = NEW_SYMBOLS + ("sc_supcon_fwd", "sc_supcon_grad", "sc_supcon_workspace_floats")
    declared = _declared(open(_lib.HEADER_PATH).read())
    assert all(declared.count(name) == 1 for name in eight)
    fns = list(_lib.HEADER.functions)
    assert len(fns) == 139 == len(set(declared)) and set(fns) == set(declared)
    assert len(set(fns) - set(eight)) == 131 and sorted(fns[-8:]) == sorted(eight)           # the former 131, then the two blocks
    assert _lib.DEFINES == {"SC_SEG_ROWS": 8, "SC_ATTN_SLACK": 64, "SC_CONV0_NSTAT": 66, "SC_WS_INFONCE": 0, "SC_WS_HUBERT_LAYER": 1,
                            "SC_SUPCON_MAX_LOGIT_BYTES": 1 << 30}
    assert not hasattr(_lib, "SUPCON_HEADER") and not hasattr(_lib, "VQ_HEADER")
    assert not os.path.exists(os.path.join(ROOT, "include", "speechclip_hip_supcon.h"))
    assert not os.path.exists(os.path.join(ROOT, "include", "speechclip_hip_vq.h"))
    assert _lib.lib().sc_abi_version() == 7


@pytest.mark.parametrize("use_gumbel", [False, True])
@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("temp", ["fixed=0.1", "learnable=0.1", "[2.0, 0.5, 0.999995]"])
def test_the_constructor_takes_every_mode(use_gumbel, hard, temp):
    from speechclip_plus_amd.vector_quantizers import SimpleVectorQuantizer
    vq = SimpleVectorQuantizer(temp=temp, use_gumbel=use_gumbel, hard=hard)
    assert (vq.use_gumbel, vq.hard) == (use_gumbel, hard)
    if temp.startswith("learnable"):
        assert isinstance(vq.curr_temp, torch.nn.Parameter) and vq.curr_temp.shape == (1,) and list(vq.state_dict()) == ["curr_temp"]
        assert [n for n, _ in vq.named_parameters()] == ["curr_temp"]
    elif temp.startswith("fixed"):
        assert list(vq.parameters()) == [] and float(vq.curr_temp) == float(torch.tensor(0.1))
    else:
        assert vq.temp_type == "scheduled" and vq.curr_temp == 2.0
        vq.set_num_updates(10 ** 7)
        assert vq.curr_temp == 0.5
    vq.train()
    default, temp_t, seed = vq._mode() if (not use_gumbel) else (None, None, None)     # a Gumbel call draws a seed: not here
    if not use_gumbel:
        assert seed == 0 and default == (hard and not temp.startswith("learnable")) and (temp_t is not None) == temp.startswith("learnable")
    assert vq.eval()._mode() == (True, None, 0)                                        # eval: the shipped quantiser in every mode


def test_the_seed_is_drawn_only_by_a_gumbel_training_call():
    from speechclip_plus_amd import ops
    from speechclip_plus_amd.vector_quantizers import SimpleVectorQuantizer
    before = ops._mult_calls[0]
    try:
        for hard in (False, True):
            for temp in ("fixed=0.1", "learnable=0.1"):
                SimpleVectorQuantizer(temp=temp, use_gumbel=False, hard=hard).train()._mode()
                SimpleVectorQuantizer(temp=temp, use_gumbel=True, hard=hard).eval()._mode()
        assert ops._mult_calls[0] == before
        torch.manual_seed(3)
        vq = SimpleVectorQuantizer(temp="fixed=0.1", use_gumbel=True, hard=False).train()
        s1, s2 = vq._mode()[2], vq._mode()[2]
        assert ops._mult_calls[0] == before + 2 and s1 != s2 and 0 <= s1 < 1 << 32
    finally:
        ops._mult_calls[0] = before


def test_a_temperature_at_or_below_zero_is_refused_before_any_launch():
    from speechclip_plus_amd.vector_quantizers import SimpleVectorQuantizer
    for temp in ("fixed=0.0", "learnable=-0.1", "[0.0, 0.0, 0.5]"):
        with pytest.raises(ValueError, match="must be positive"):
            SimpleVectorQuantizer(temp=temp, hard=False)._temp()
    with pytest.raises(RuntimeError, match="device tensors only"):                     # everything else in order: CPU tensors are refused
        SimpleVectorQuantizer(temp="fixed=0.1", hard=False, use_gumbel=True)(torch.zeros(2, 3, 8))
    with pytest.raises(RuntimeError, match="device tensors only"):
        SimpleVectorQuantizer(temp="learnable=0.1").quantize_keywords(torch.zeros(2, 3, 8), torch.zeros(10, 8))


def test_c_argument_checks_need_no_device():
    from speechclip_plus_amd import _lib
    lib = _lib.lib()
    one = 16                                                         # a non-null, aligned address that is never dereferenced

    def err(rc, word):
        return rc == -1 and word in lib.sc_last_error()
    assert err(lib.sc_vq_gumbel_f32(None, 8, 2, 8, 0, None), b"null")
    assert err(lib.sc_vq_gumbel_f32(one, 8, 0, 8, 0, None), b"positive")
    assert err(lib.sc_vq_gumbel_f32(one, 4, 2, 8, 0, None), b"ldg")
    assert err(lib.sc_vq_gumbel_f32(one, 1 << 20, 1 << 16, 1 << 16, 0, None), b"32-bit noise index")
    assert err(lib.sc_vq_noisy_rowstats(one, 8, 2, 8, 0.1, 0, 1, None, one, one, None), b"null")
    assert err(lib.sc_vq_noisy_rowstats(one, 8, 2, 8, 0.1, 0, 1, one, one, None, None), b"null")
    assert err(lib.sc_vq_noisy_rowstats(one, 8, 2, 8, 0.0, 0, 1, one, one, one, None), b"temp")
    assert err(lib.sc_vq_noisy_rowstats(one, 4, 2, 8, 0.1, 0, 0, one, one, one, None), b"ldx")
    assert err(lib.sc_vq_noisy_rowstats(one, 1 << 20, 1 << 16, 1 << 16, 0.1, 0, 1, one, one, one, None), b"32-bit noise index")
    assert err(lib.sc_vq_soft_prob_f32(one, 8, None, one, 2, 8, 0.1, 0, 0, one, 8, None), b"null")
    assert err(lib.sc_vq_soft_prob_f32(one, 8, one, one, 2, 8, -1.0, 0, 0, one, 8, None), b"temp")
    assert err(lib.sc_vq_soft_prob_f32(one, 8, one, one, 2, 8, 0.1, 0, 0, one, 7, None), b"lds")
    assert err(lib.sc_vq_soft_prob_f32(one, 8, one, one, 70000, 8, 0.1, 0, 0, one, 8, None), b"65535")
    assert err(lib.sc_vq_soft_split_bf16(one, 8, one, one, 2, 8, 0.1, 0, 0, None, 128, 64, None), b"null")
    assert err(lib.sc_vq_soft_split_bf16(one, 8, one, one, 2, 8, 0.1, 0, 0, one, 1, 64, None), b"Nkp")
    assert err(lib.sc_vq_soft_split_bf16(one, 8, one, one, 2, 8, 0.1, 0, 0, one, 128, 6, None), b"Vp")
    assert err(lib.sc_vq_soft_split_bf16(one, 8, one, one, 2, 8, 0.1, 0, 0, one, 128, 10, None), b"Vp")
    assert err(lib.sc_vq_soft_split_bf16(one, 8, one, one, 2, 8, 0.1, 0, 0, one + 2, 128, 64, None), b"aligned")
    assert err(lib.sc_vq_soft_bwd2(one, 8, one, one, None, 8, 2, 8, 8, 0.1, 0, 0, one, 8, 0, None, None), b"null")
    assert err(lib.sc_vq_soft_bwd2(one, 8, one, one, one, 8, 2, 8, 4, 0.1, 0, 0, one, 8, 0, None, None), b"Vpad")
    assert err(lib.sc_vq_soft_bwd2(one, 8, one, one, one, 8, 2, 8, 16, 0.1, 0, 0, one, 8, 0, None, None), b"ldd")
    assert err(lib.sc_vq_soft_bwd2(one, 8, one, one, one, 8, 2, 8, 8, 0.0, 0, 1, one, 8, 1, one, None), b"temp")


def test_ops_refuse_bad_operands_before_any_launch():
    from speechclip_plus_amd import ops
    x, v = torch.zeros(4, 8), torch.zeros(2, 4)
    bad = [((torch.zeros(8), v, 8, 0.1), "x must be a 2-D"), ((x.double(), v, 8, 0.1), "x must be torch.float32"),
           ((x, v, 9, 0.1), "at least V = 9"), ((x.t().contiguous().t(), v, 4, 0.1), "unit column stride"),
           ((x, v, 8, 0.0), "temp must be positive"), ((x, v[:, :3], 8, 0.1), "stats must be"), ((x, v.double(), 8, 0.1), "stats must be")]
    for args, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ops.vq_soft_prob(*args)
    with pytest.raises(ValueError, match="Vp = 100"):
        ops.vq_soft_split(x, v, 8, 0.1, 100)
    with pytest.raises(ValueError, match="t must be"):
        ops.vq_soft_bwd2(x, v, torch.zeros(4, 7), 8, 0.1, False)
    with pytest.raises(ValueError, match="Vpad = 4"):
        ops.vq_soft_bwd2(x, v, x, 8, 0.1, False, Vpad=4)
    with pytest.raises(ValueError, match="below 2\\^32"):
        ops.vq_gumbel(1 << 16, 1 << 16, 0, "cuda")
    for call in (lambda: ops.vq_soft_prob(x, v, 8, 0.1), lambda: ops.vq_noisy_rowstats(x, 8, 0.1, 1), lambda: ops.vq_soft_split(x, v, 8, 0.1, 64),
                 lambda: ops.vq_soft_bwd2(x, v, x, 8, 0.1, False), lambda: ops.vq_gumbel(4, 8, 0, "cpu")):
        with pytest.raises(RuntimeError, match="device tensors only"):                 # CPU tensors are refused like every other op's
            call()


def test_a_table_holds_no_soft_operand_until_asked():
    from speechclip_plus_amd.vector_quantizers import VocabTables
    tb = object.__new__(VocabTables)                                 # the constructor needs the device; the lazy slot does not
    tb._soft_T, tb.table, tb.Vp = None, torch.randn(5, 4), 128
    calls = []
    from speechclip_plus_amd import ops
    real = ops.vq_soft_table
    ops.vq_soft_table = lambda table, Vp: calls.append(Vp) or real(table, Vp)
    try:
        assert tb._soft_T is None and calls == []
        W = tb.soft_table()
        assert tb.soft_table() is W and calls == [128]               # built once, on the first request
    finally:
        ops.vq_soft_table = real
    assert W.shape == (4, 3 * 128) and W.dtype == torch.bfloat16
    hi, lo = W[:, :5].float(), W[:, 128:133].float()
    assert torch.equal(W[:, 256:261], W[:, :5]) and float(W[:, 5:128].abs().max()) == 0.0 and float(W[:, 133:256].abs().max()) == 0.0
    assert float((hi + lo - tb.table.t()).abs().max()) <= 2.0 ** -17 * float(tb.table.abs().max())
    import inspect
    src = inspect.getsource(VocabTables.__init__)
    assert "self._soft_T = None" in src and "vq_soft_table" not in src
