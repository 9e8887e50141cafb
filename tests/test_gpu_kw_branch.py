"""The fixed-keyword branch head on the device: Kw_BatchNorm against the reference module's recorded results
(tests/golden/kw_bn_fixed.npz) and MultiheadAttentionAndNorm.query_forward - the pooled route on csrc/kwpool.hip - against the fp64
restatement through nn.MultiheadAttention (tests/kwpool_cases.py) and against the full-sequence route on the same inputs.

Bounds.  The pooled route and the BatchNorm kernels are fp32 on inputs both sides share (the bf16 features): relative L2 <= 2e-4
(kwpool_cases.FP32_BOUND), per (utterance, keyword) for the output, per tensor for a gradient; the weighted-sum logits see the bf16
dX rows: + 2^-8.  The full-sequence route multiplies bf16 operands and stores q / k / v, probabilities, context and the pre-norm sum
in bf16: up to eight roundings of 2^-8 = 3.1e-2 on the output; its gradients meet the project's bound for the bf16 paths, 6e-2
(tests/test_gpu_recipes.py)."""
import os

import numpy as np
import pytest
import torch

import kwpool_cases as kc

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FULL_OUT_BOUND, FULL_GRAD_BOUND = 8 * 2.0 ** -8, 6e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _rel(got, ref, dims=None):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    if dims is None:
        return float((got - ref).norm() / ref.norm())
    return float(((got - ref).pow(2).sum(dims).sqrt() / ref.pow(2).sum(dims).sqrt()).max())


# ------------------------------------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("kind", ("eachKw", "same"))
def test_kw_batchnorm_module_against_the_reference_fixture(dev, kind):
    from speechclip_plus_amd.vector_quantizers import Kw_BatchNorm
    z = np.load(os.path.join(ROOT, "tests", "golden", "kw_bn_fixed.npz"))
    t = lambda k: torch.from_numpy(z[k]).to(dev)
    m = Kw_BatchNorm(kw_num=8, kw_dim=16, batchnorm_type=kind, init_bias=t("init_bias").cpu(), init_scale=t("init_scale").cpu(),
                     std_scale=float(z["std_scale"]), learnable=True, parallel=kind == "eachKw").to(dev)
    with torch.no_grad():
        m.bn_layer.weight.copy_(t(f"{kind}.weight"))
        m.bn_layer.bias.copy_(t(f"{kind}.bias"))
    m.train()
    x1 = t("x1").clone().requires_grad_(True)
    y1 = m(x1)
    y1.backward(t("dy"))
    m(t("x2"))
    errs = {"y1": _rel(y1, t(f"{kind}.y1")), "dx1": _rel(x1.grad, t(f"{kind}.dx1")),
            "dweight": _rel(m.bn_layer.weight.grad, t(f"{kind}.dweight")), "dbias": _rel(m.bn_layer.bias.grad, t(f"{kind}.dbias")),
            "running_mean": _rel(m.bn_layer.running_mean, t(f"{kind}.running_mean")),
            "running_var": _rel(m.bn_layer.running_var, t(f"{kind}.running_var"))}
    assert int(m.bn_layer.num_batches_tracked) == int(z[f"{kind}.num_batches_tracked"]) == 2
    m.eval()
    rm = m.bn_layer.running_mean.clone()
    x2 = t("x2").clone().requires_grad_(True)
    ye = m(x2)
    ye.backward(t("dy"))
    errs["y_eval"] = _rel(ye, t(f"{kind}.y_eval"))
    assert torch.equal(rm, m.bn_layer.running_mean) and int(m.bn_layer.num_batches_tracked) == 2       # eval leaves the buffers alone
    # eval gradient: the running statistics are constants -> a scale per (slot, channel)
    w, rv = t(f"{kind}.weight").double(), t(f"{kind}.running_var").double()
    scale = w / torch.sqrt(rv + 1e-5)
    scale = scale.view(16, 8).t() if kind == "eachKw" else scale
    errs["dx_eval"] = _rel(x2.grad, t("dy").double() * scale)
    for k, v in errs.items():
        print(f"PARITY|kw_bn {kind}|{k}|{v:.3e}|{kc.FP32_BOUND:.3e}", flush=True)
    bad = {k: v for k, v in errs.items() if not v <= kc.FP32_BOUND}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ query_forward
def _module(dev, w, D, H):
    from speechclip_plus_amd import MultiheadAttentionAndNorm
    m = MultiheadAttentionAndNorm(d_model=D, nhead=H, dropout=0.1).to(dev)
    att, norm = m.multihead_attn_layer, m.attentionBlock_Norm
    with torch.no_grad():
        att.in_proj_weight.copy_(w["in_proj_weight"])
        att.in_proj_bias.copy_(w["in_proj_bias"])
        att.out_proj.weight.copy_(w["out_proj.weight"])
        att.out_proj.bias.copy_(w["out_proj.bias"])
        norm.weight.copy_(w["ln.weight"])
        norm.bias.copy_(w["ln.bias"])
    cls = torch.nn.Parameter(w["cls"].clone().to(dev))
    return m.eval(), cls


def _params(m, cls):
    att, norm = m.multihead_attn_layer, m.attentionBlock_Norm
    return {"cls": cls, "in_proj_weight": att.in_proj_weight, "in_proj_bias": att.in_proj_bias, "out_proj.weight": att.out_proj.weight,
            "out_proj.bias": att.out_proj.bias, "ln.weight": norm.weight, "ln.bias": norm.bias}


def _zero(ps):
    for p in ps.values():
        p.grad = None


CASES = (("handle", 768, 1, 8, 150, (150, 1, 65, 100)),          # the encoder's buffer, read in place (row 0 = the free CLS slot)
         ("plain", 1024, 1, 9, 70, (70, 1, 37)),                 # a plain feature tensor; 9 queries (the hybrid's count)
         ("plain", 128, 2, 8, 70, (70, 2, 65)))                  # two heads: K H = 16 vectors


@pytest.mark.parametrize("layout,D,H,K,T,lens", CASES)
def test_query_forward_against_fp64_and_the_full_sequence_route(dev, layout, D, H, K, T, lens):
    from speechclip_plus_amd import WeightedSumLayer
    g = torch.Generator().manual_seed(D + K)
    B = len(lens)
    w = kc.branch_weights(D, H, K, seed=D + H)
    m, cls = _module(dev, w, D, H)
    ps = _params(m, cls)
    lens_t = torch.tensor(lens)
    G = torch.randn(B, K, D, generator=g)
    if layout == "handle":
        NL, R = 3, 192
        hidden = torch.randn(NL, B * R, D, generator=g).to(torch.bfloat16).to(dev)
        ws = WeightedSumLayer(NL).to(dev)
        with torch.no_grad():
            ws.weights.copy_(torch.tensor([0.3, -0.2, 0.5]))
        make = lambda: ws.forward_padded(hidden, B, R, T, D)
        feat0 = make()
        assert feat0._sc_handle.src.shape == (B, R, D)
        feat_vals = feat0.detach().float().cpu()
    else:
        feat_vals = torch.randn(B, T, D, generator=g).to(torch.bfloat16).float()
        make = lambda: feat_vals.to(dev).requires_grad_(True)
    # ---- fp64 restatement on the same bf16 features
    out_ref, leaves = kc.branch_ref(w, feat_vals, lens_t, H)
    (out_ref * G.double()).sum().backward()
    ref_g = {k: leaves[k].grad for k in ps}
    if layout == "handle":
        hd = hidden.double().cpu().view(NL, B, R, D)[:, :, :T]          # (frame t of the sum lands in row t + 1 of the buffer)
        wsoft = torch.softmax(torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64), 0)
        d_n = (hd * leaves["feat"].grad[None]).sum((1, 2, 3))
        ref_g["ws"] = wsoft * (d_n - (wsoft * d_n).sum())
    else:
        ref_g["feat"] = leaves["feat"].grad
    # ---- pooled route
    errs, fails = {}, []

    def run(path):
        _zero(ps)
        m.query_path = path
        feat = make()
        if layout == "handle":
            ws.weights.grad = None
        out = m.query_forward(cls, feat, lens_t.to(dev))
        (out * G.to(dev)).sum().backward()
        grads = {k: p.grad.clone() for k, p in ps.items()}
        if layout == "handle":
            grads["ws"] = ws.weights.grad.clone()
        else:
            grads["feat"] = feat.grad.clone()
        return out.detach(), grads

    out_p, g_p = run("pooled")
    assert out_p.dtype == torch.float32 and out_p.shape == (B, K, D)
    errs["out"] = (_rel(out_p, out_ref, (2,)), kc.FP32_BOUND)
    for k, v in g_p.items():
        errs["d " + k] = (_rel(v, ref_g[k]), kc.FP32_BOUND + (kc.BF16_ROUND if k == "ws" else 0.0))
    out_f, g_f = run("full")
    errs["full out"] = (_rel(out_f, out_ref, (2,)), FULL_OUT_BOUND)
    for k, v in g_f.items():
        errs["full d " + k] = (_rel(v, ref_g[k]), FULL_GRAD_BOUND)
    errs["pooled vs full out"] = (_rel(out_p, out_f, (2,)), FULL_OUT_BOUND + kc.FP32_BOUND)
    for k, (e, b) in errs.items():
        print(f"PARITY|query {layout} D={D} H={H} K={K}|{k}|{e:.3e}|{b:.3e}", flush=True)
        if not e <= b:
            fails.append((k, e, b))
    assert not fails, fails
    # bk shifts every score of a query alike: its gradient is exactly zero on the pooled route
    assert (g_p["in_proj_bias"][D: 2 * D] == 0).all()


@pytest.mark.parametrize("D,H,K,T,lens", ((768, 1, 8, 70, (70, 33, 1)), (128, 2, 8, 70, (70, 2, 65))))
def test_query_forward_train_mode_against_fp64(dev, D, H, K, T, lens):
    """Train mode: nn.MultiheadAttention's dropout on the attention weights.  The multiplier the node draws is a function of torch's
    seed and a call counter, so the same call materialises it for the fp64 restatement (kwpool_cases.branch_rows_mult, held here
    against the nn.MultiheadAttention form without a multiplier).  Forward and every gradient - the multiplier over K H rows, the
    value bias through sum(p mult), its path back into the attention weights, d cls through p mult - meet the pooled route's
    bound; the same seed repeats the bits."""
    from speechclip_plus_amd import ops
    B = len(lens)
    w = kc.branch_weights(D, H, K, seed=D + 7)
    m, cls = _module(dev, w, D, H)
    ps = _params(m, cls)
    g = torch.Generator().manual_seed(D)
    feat_vals = torch.randn(B, T, D, generator=g).to(torch.bfloat16).float()
    G = torch.randn(B, K, D, generator=g)
    lens_t = torch.tensor(lens)
    a, _ = kc.branch_ref(w, feat_vals, lens_t, H)
    b, _ = kc.branch_ref(w, feat_vals, lens_t, H, mult=torch.ones(B, K * H, K + T))
    assert _rel(b, a) < 1e-12                                               # the written-out restatement is nn.MultiheadAttention's
    m.train()
    torch.manual_seed(5)
    n0 = ops._mult_calls[0]
    n = B * K * H * (K + T)
    mult = ops.dropout_mult(((n + 7) // 8 * 8,), 0.1, dev)[:n].view(B, K * H, K + T).cpu()
    assert (mult == 0).any() and abs(float(mult.mean()) - 1.0) < 0.05
    outs = []
    for _ in range(2):
        ops._mult_calls[0] = n0
        _zero(ps)
        feat = feat_vals.to(dev).requires_grad_(True)
        out = m.query_forward(cls, feat, lens_t.to(dev))
        (out * G.to(dev)).sum().backward()
        outs.append(out.detach())
    assert torch.equal(outs[0], outs[1])
    out_ref, leaves = kc.branch_ref(w, feat_vals, lens_t, H, mult=mult)
    (out_ref * G.double()).sum().backward()
    errs = {"out": _rel(outs[0], out_ref, (2,)), "d feat": _rel(feat.grad, leaves["feat"].grad)}
    for k, p in ps.items():
        errs["d " + k] = _rel(p.grad, leaves[k].grad)
    for k, e in errs.items():
        print(f"PARITY|query train D={D} H={H} K={K}|{k}|{e:.3e}|{kc.FP32_BOUND:.3e}", flush=True)
    bad = {k: e for k, e in errs.items() if not e <= kc.FP32_BOUND}
    assert not bad, bad
    m.eval()
    assert not torch.equal(m.query_forward(cls, feat_vals.to(dev), lens_t.to(dev)), outs[0])


def test_query_forward_falls_back_to_the_full_sequence_route(dev):
    """K x heads > 16, and a row count past the kernel's LDS limit (ops.kw_pool_max_rows), take the full-sequence route: the result
    meets that route's bound against fp64, and no pooling entry is called."""
    from speechclip_plus_amd import ops
    cases = ((256, 4, 8, 40, (40, 7)),                                       # 32 vectors: past the kernel's 16
             (128, 2, 8, ops.kw_pool_max_rows(16, 8, backward=True) + 1, (300, 9)))          # 16 vectors, one row too many
    assert 64 < cases[1][3] < 1024
    calls = []
    orig = ops.kw_pool_fwd
    ops.kw_pool_fwd = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        for D, H, K, T, lens in cases:
            w = kc.branch_weights(D, H, K, seed=4)
            m, cls = _module(dev, w, D, H)
            f = torch.randn(2, T, D, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).float()
            out_ref, _ = kc.branch_ref(w, f, torch.tensor(lens), H)
            out = m.query_forward(cls, f.to(dev), torch.tensor(lens, device=dev))
            assert _rel(out, out_ref, (2,)) <= FULL_OUT_BOUND
        assert not calls
        w = kc.branch_weights(128, 2, 8, seed=4)                             # one row fewer: the pooled route
        m, cls = _module(dev, w, 128, 2)
        m.query_forward(cls, torch.zeros(1, cases[1][3] - 1, 128, device=dev), torch.tensor([5], device=dev))
        assert calls
    finally:
        ops.kw_pool_fwd = orig
