"""Helpers of tests/test_gpu_attn_scores.py (not collected on their own): seeded score constructions, fp64 references, derived bounds,
a torch emulation of the kernels' arithmetic order and planted errors for the attention kernels - attn_fwd_kernel in all its
instances (csrc/attention.hip), attn_bwd_dq_kernel / attn_bwd_dkv_kernel (csrc/attention_bwd.hip), attn32_fwd_kernel /
attn32_bwd_kernel (csrc/attn_short.hip).  Nothing here needs a GPU; tests/test_attn_cases_cpu.py pins the cases' properties, shows
that the emulation keeps every bound and that every planted error breaks one.

Scores are CONSTRUCTED: channel 0 of a structured head carries q[i, 0] = g_i and k[j, 0] = t_j (multiples of 1/8 that bf16 holds
exactly), channels 1 .. 63 carry N(0, 0.05) noise, v is N(0, 1).  With dh = 64 and scale = 1/8 the log2-domain score is
x_ij = g_i t_j C + noise, C = scale log2(e) = 0.18034.  The gains of a 32-query wave are a seeded shuffle of {0, +a, -a, +2a}, a = 4:
the same key block holds queries whose running maximum must be rescaled and queries that must multiply by exactly 1.  Head 0 carries
the profile, head 1 is plain N(0, 1), head 2 carries the profile reversed over the utterance's valid keys.

Bounds (docs/parity.md, "Attention on peaked and drifting scores") use the project's constants: U = 2^-24, one bf16 store 2^-8,
second-order factor 2, 2^-106 of absolute slack for flushed subnormals."""
import math

import numpy as np
import torch

from head_cases import Report, rel_l2  # noqa: F401

U = 2.0 ** -24
STORE = 2.0 ** -8
KSEC = 2
FTZ = 2.0 ** -106
C_P = 1                 # the probabilities enter P.V as bf16(p): one rounding relative to p, whatever the (stale) maximum
ATT_ACC = 2             # fp32 accumulation over the keys of both the numerator and the row sum
ATT_ROUND = 3           # backward: P, dS and the stored O are bf16 inside the kernels
EXP_ULP = 2             # v_exp_f32: 1 ulp = 2 U relative
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634

H, DH = 3, 64
D = H * DH
SCALE = 0.125
C32 = float(np.float32(SCALE) * np.float32(LOG2E))      # the kernels' c: scale * 1.4426950408889634f in fp32 (scale a power of two)
A_GAIN = 4.0
GAINS = (0.0, A_GAIN, -A_GAIN, 2 * A_GAIN)
GROW = 6.0              # csrc/attention.hip: grow = (m_cand - m_run) * cs > 6
MARGIN = 0.25
FLOOR_M = -1e30
SPIKE_T = 40.0          # g t scale = 8 x 40 / 8 = 40 nats at the largest gain
OFF_Q, OFF_K = 32.0, 52.0   # channel 1 of the offset case: 32 x 52 C = 300.08 in the log2 domain, the same for every (query, key)

# name -> (profile, R, key lengths): H = 3, B <= 4, R in {128, 256, 384}, lengths from {1, 33, 64, 65, 127, 128, 129, 200, 256, 384}
CASES = {
    "stair55": ("stair55", 384, [384, 200, 129, 65]),
    "stair65": ("stair65", 256, [256, 127, 128, 33]),
    "stair09": ("stair09", 384, [384, 256, 64, 1]),
    "ramp": ("ramp", 128, [128, 65, 33, 127]),
    "desc": ("desc", 384, [384, 200, 256, 129]),
    "spike": ("spike", 256, [256, 200, 129, 65]),
    "twin": ("twin", 256, [256, 129, 200, 128]),
    "stair55_off": ("stair55", 256, [256, 200, 65, 129]),
    "control": ("control", 128, [128, 1, 33, 64]),
}
STEP = {"stair55": 3.75, "stair65": 4.5, "stair09": 0.625}      # t per 32-key block: x 2a C = 5.41 / 6.49 / 0.90 per block
DRIFTING = ("stair55", "stair65", "ramp", "stair55_off")        # mixed waves: some query with 0 and some with >= 2 rescales
SPIKE_KEYS = ((0, 31, 32, 63), (64, -1, -1, 64))                 # head 0 / head 2, per utterance; -1 = valid - 1


def bf16_exact(t):
    return bool((t.to(torch.bfloat16).to(t.dtype) == t).all())


def profile(kind, n):
    """t_j, j < n (fp64 values that bf16 holds exactly)"""
    j = torch.arange(n, dtype=torch.float64)
    blk = torch.div(j, 32, rounding_mode="floor")
    if kind in STEP:
        t = STEP[kind] * blk
    elif kind == "ramp":
        t = 0.125 * (j % 32) + 4.5 * blk               # block maximum at the block's last key, 6.49 per block at the largest gain
    elif kind == "desc":
        t = -0.375 * j                                 # maximum at key 0; at the largest gain exp2 underflows from key 277 on
    elif kind == "twin":
        t = torch.zeros(n, dtype=torch.float64)
        t[10] = SPIKE_T
        if n > 100:
            t[100] = SPIKE_T                           # exactly equal maxima in key tiles 0 and 1
    else:
        raise KeyError(kind)
    return t.to(torch.bfloat16).double()


def wave_gains(R, g):
    """[R]: every 32-query wave holds each of {0, +a, -a, +2a} eight times, in a seeded order"""
    base = torch.tensor(GAINS, dtype=torch.float64).repeat(8)
    return torch.cat([base[torch.randperm(32, generator=g)] for _ in range(R // 32)])


def build(name, restart=0, lens=None, causal=0):
    """-> dict: q, k, v [B, R, D] bf16 (CPU), lens, R, gains [B, R] fp64, t [B, H, R] fp64 (NaN on the control head), and per
    query the record of the decision rule on the fp64 block maxima under the key-length mask (``causal``: the mask the record is
    taken under): rescales [B, H, R] (after the first block with a visible key) and margin [B, H, R] (smallest |growth - 6|).
    ``restart`` = 32 / 64: the profile starts again every ``restart`` keys (segment-causal packing: every segment drifts)."""
    kind, R, case_lens = CASES[name]
    lens = list(case_lens if lens is None else lens)
    B = len(lens)
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name) * 7 + restart)
    q = 0.05 * torch.randn(B, R, H, DH, generator=g, dtype=torch.float64)
    k = 0.05 * torch.randn(B, R, H, DH, generator=g, dtype=torch.float64)
    v = torch.randn(B, R, H, DH, generator=g, dtype=torch.float64)
    ctl = [1] if kind != "control" else [0, 1, 2]
    for h in ctl:
        q[:, :, h] = torch.randn(B, R, DH, generator=g, dtype=torch.float64)
        k[:, :, h] = torch.randn(B, R, DH, generator=g, dtype=torch.float64)
    gains = torch.stack([wave_gains(R, g) for _ in range(B)])
    t = torch.full((B, H, R), float("nan"), dtype=torch.float64)
    if kind != "control":
        for b, nv in enumerate(lens):
            for h in (0, 2):
                if kind == "spike":
                    tj = torch.zeros(R, dtype=torch.float64)
                    js = SPIKE_KEYS[h // 2][b]
                    tj[min(nv - 1, js) if js >= 0 else nv - 1] = SPIKE_T
                else:
                    n = restart if restart else R
                    tj = profile(kind, n).repeat(R // n)
                    if h == 2:                          # reversed over the valid keys (per segment when restarted)
                        if restart:
                            tj = profile(kind, n).flip(0).repeat(R // n)
                        else:
                            tj = torch.cat([tj[:nv].flip(0), tj[nv:]])
                t[b, h] = tj
                q[b, :, h, 0] = gains[b]
                k[b, :, h, 0] = tj
                if name.endswith("_off"):
                    q[b, :, h, 1] = OFF_Q
                    k[b, :, h, 1] = OFF_K
    bf = lambda x: x.reshape(B, R, D).to(torch.bfloat16)
    c = {"name": name, "kind": kind, "R": R, "B": B, "lens": lens, "q": bf(q), "k": bf(k), "v": bf(v), "gains": gains, "t": t,
         "restart": restart}
    c["rescales"], c["margin"] = record_rescales(c, causal)
    return c


def record_rescales(c, causal=0):
    """per query of every utterance and head: the rescale count and the smallest distance of a decision from the threshold, from the
    log2-domain scores of the bf16 operands in fp64"""
    cnt, mar = [], []
    for b, nv in enumerate(c["lens"]):
        q, k = heads(c["q"][b]), heads(c["k"][b])
        x = ((q @ k.transpose(-1, -2)) * (SCALE * LOG2E)).masked_fill(~key_mask(c["R"], nv, causal)[None], float("-inf"))
        n, m, _ = rescale_trace(x)
        cnt.append(n)
        mar.append(m)
    return torch.stack(cnt), torch.stack(mar)


def dropped_spike_rows(f, gains):
    """[H, R] bool: one-hot rows (largest gain, structured heads) whose spike key the dropout mask removed - the reference of such a
    row is what the e^-40 tail leaves, below 1e-15"""
    hit = ((f["mult"] == 0) & (f["P"] > 0.5)).any(-1) & (gains == 2 * A_GAIN)[None]
    hit[1] = False
    return hit


def heads(x):
    """[R, D] -> [H, R, 64] fp64"""
    return x.double().view(x.shape[0], H, DH).transpose(0, 1)


def rows(x):
    """[H, R, 64] -> [R, D]"""
    return x.transpose(0, 1).reshape(x.shape[1], -1)


def key_mask(R, nv, causal=0, nq=None):
    """[nq or R, R] bool: key j < nv; causal 1: j <= i; causal 32 / 64: also j >= the start of i's aligned segment"""
    i = torch.arange(R if nq is None else nq)[:, None]
    j = torch.arange(R)[None, :]
    m = (j < max(1, min(nv, R))).expand(i.shape[0], R).clone()
    if causal:
        m &= j <= i
    if causal > 1:
        m &= j >= (i // causal) * causal
    return m


def drop_mult(idx, seed, p):
    """keep / (1 - p_applied) in fp64 for the element indices ``idx`` (any shape, int64) + the applied rate round(256 p) / 256"""
    from test_gpu_kernels import _keep_mask8
    keep, pa = _keep_mask8(idx.numpy().reshape(-1) & 0xffffffff, seed, p)
    return torch.from_numpy(keep).view(idx.shape).double() / (1.0 - pa), pa


def drop_index_uniform(b, R, nh=H):
    """csrc/attention.hip drop_row, uniform rows: ((b H + h) R + q) R + key"""
    h, qi, ki = (torch.arange(n, dtype=torch.int64) for n in (nh, R, R))
    return ((b * nh + h[:, None, None]) * R + qi[None, :, None]) * R + ki[None, None, :]


def drop_index_segment(r0, pitch, rows_total, max_pitch, nh=H):
    """segment rows: (h rows_total + row0 + q) max_pitch + key"""
    h, qi, ki = (torch.arange(n, dtype=torch.int64) for n in (nh, pitch, pitch))
    return (h[:, None, None] * rows_total + r0 + qi[None, :, None]) * max_pitch + ki[None, None, :]


def bias_matrix(gate, table, R):
    """gate [H, R], table [H, 2 Tmax - 1] -> gate[h, i] table[h, Tmax - 1 + j - i], [H, R, R] (dtype of the arguments)"""
    tmax = (table.shape[1] + 1) // 2
    idx = tmax - 1 + torch.arange(R)[None, :] - torch.arange(R)[:, None]
    return gate[:, :, None] * table[:, idx]


# ================================================================================================================== fp64 references
def fwd_ref(q, k, v, mask, scale=SCALE, bias=None, mult=None, drop_key=None):
    """q, k, v [H, R, 64] fp64, mask [H or 1, R, R], bias [H, R, R] in natural units, mult = keep / (1 - p).  -> dict: out [H, R, 64],
    lse2 [H, R] (undropped scores), their element-wise bounds, x = the masked log2-domain scores, P (undropped), e.
    ``drop_key`` = (h, query, key): that key is removed from that query's softmax (planted error a)."""
    nk = q.shape[1]
    s = (q @ k.transpose(-1, -2)) * scale
    sa = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    z = s if bias is None else s + bias
    mask = mask.expand_as(z).clone()
    if drop_key is not None:
        mask[drop_key] = False
    zm = z.masked_fill(~mask, float("-inf"))
    zmax = zm.amax(-1, keepdim=True)
    P = torch.softmax(zm, dim=-1)
    lse2 = torch.logsumexp(zm, dim=-1) * LOG2E
    z0 = z.masked_fill(~mask, 0.0)
    # relative error of one probability = the absolute error of its natural-log exponent.  Plain: fma(s, c, -fl(m c)) and v_exp_f32:
    # U (max|s| [fl(m c)] + |s - max| + 6 ln 2 [fma result, stale max] + 2 x 64 scale |q|.|k| [S in fp32, K = 64] + 2 [v_exp_f32]).
    # BIAS: x = fma(s, c, gate . fl(table log2 e)) is rounded once more (U |x|) and the bias carries two roundings (2 U |gate table|)
    e = z0.abs().amax(-1, keepdim=True) + (z0 - zmax).abs() + 6 * LN2 + KSEC * 64 * sa + EXP_ULP
    if bias is not None:
        e = e + z0.abs() + 2 * bias.abs()
    e = (U * e).masked_fill(~mask, 0.0)
    Pm = P if mult is None else P * mult
    ref, pv = Pm @ v, Pm @ v.abs()
    # the row sum is taken over the UNDROPPED probabilities: its error is sum P e, also where the keys that carry it are dropped
    exp_term = KSEC * ((Pm * e) @ v.abs() + (P * e).sum(-1, keepdim=True) * pv)
    bound = STORE * ref.abs() + C_P * STORE * pv + KSEC * ATT_ACC * nk * U * pv + exp_term + FTZ
    xmax2 = zmax.squeeze(-1) * LOG2E
    # lse2 = fl(m cs + v_log_f32(l)), l = sum of the unrounded p (relative error <= max e + 2 nk U); |log2 l| <= |lse2 - max| + 6
    bl = (KSEC * nk * U + e.amax(-1)) / LN2 + U * (lse2.abs() + xmax2.abs() + 6) + 2 * U * ((lse2 - xmax2).abs() + 7)
    # printed only (docs/parity.md): the same with a flat 2 U for the logarithm and no allowance for the stale maximum
    bl_flat = (KSEC * nk * U + e.amax(-1)) / LN2 + U * (lse2.abs() + xmax2.abs()) + 2 * U
    return {"out": ref, "bound": bound, "lse2": lse2, "bound_lse": bl, "bound_lse_flat": bl_flat, "x": zm * LOG2E, "P": P, "e": e,
            "mask": mask, "pv": pv}


def bwd_ref(q, k, v, dout, mask, scale=SCALE, mult=None, ep=None, ddelta=None, R_acc=None):
    """fp64 dq / dk / dv [H, R, 64] by autograd + bounds of the form 2^-8 |ref| + 3 2^-8 mag + 2 R U mag, plus 2 x the same
    magnitudes weighted with ``ep`` [H, R, R] (relative error of the recomputed P) and ``ddelta`` [H, R, 1] (error of delta)."""
    R_acc = q.shape[1] if R_acc is None else R_acc
    qa, ka, va = (t.detach().clone().requires_grad_() for t in (q, k, v))
    zm = ((qa @ ka.transpose(-1, -2)) * scale).masked_fill(~mask, float("-inf"))
    Pa = torch.softmax(zm, dim=-1)
    ((Pa if mult is None else Pa * mult) @ va).backward(dout)
    with torch.no_grad():
        P = Pa.detach()
        one = torch.ones_like(P) if mult is None else mult
        Pd = P * one
        O = Pd @ v
        dP = (dout @ v.transpose(-1, -2)) * one
        delta = (P * dP).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        man = ((dS @ k) * scale, (dS.transpose(-1, -2) @ q) * scale, Pd.transpose(-1, -2) @ dout)
        dPm = (dout.abs() @ v.abs().transpose(-1, -2)) * one
        dSm = P * (dPm + (dout.abs() * O.abs()).sum(-1, keepdim=True) + delta.abs())
        mags = [(dSm @ k.abs()) * scale, (dSm.transpose(-1, -2) @ q.abs()) * scale, Pd.transpose(-1, -2) @ dout.abs()]
        if ep is not None:
            dSe = dSm * ep + (0.0 if ddelta is None else P * ddelta)
            extra = [(dSe @ k.abs()) * scale, (dSe.transpose(-1, -2) @ q.abs()) * scale, (Pd * ep).transpose(-1, -2) @ dout.abs()]
        else:
            extra = [torch.zeros_like(m) for m in mags]
    out = {}
    for n, ref, m, x, mn in zip(("dq", "dk", "dv"), (qa.grad, ka.grad, va.grad), mags, extra, man):
        out[n] = ref
        out["bound_" + n] = STORE * ref.abs() + ATT_ROUND * STORE * m + KSEC * R_acc * U * m + KSEC * x + FTZ
        out["manual_" + n] = mn
    return out


def flash_bwd_errors(f, dout):
    """ep, ddelta of the flash backward fed the kernel's own lse2 and out: P = exp2(fma(s, c, -lse2)) - ln 2 U (|s c| + |lse2| + 2) - and
    the forward's lse2 bound (a whole row of P scales with it); delta = sum dO . O inherits the forward's output bound"""
    x0 = f["x"].masked_fill(~f["mask"], 0.0)
    ep = LN2 * (U * (x0.abs() + f["lse2"].abs()[..., None] + 2) + f["bound_lse"][..., None])
    return ep.masked_fill(~f["mask"], 0.0), (dout.abs() * f["bound"]).sum(-1, keepdim=True)


def short_bwd_errors(f, dout, v):
    """attn32_bwd recomputes maximum and sum: P = exp2(x - mx) / sum carries the forward's exponent error, the sum's (2 x 32 U + max e)
    and the division (2 U); delta = sum_j P dP in fp32"""
    ep = (f["e"] + (KSEC * 32 * U + f["e"].amax(-1, keepdim=True)) + 2 * U).masked_fill(~f["mask"], 0.0)
    dPm = dout.abs() @ v.abs().transpose(-1, -2)
    return ep, (f["P"] * (ep + KSEC * 32 * U) * dPm).sum(-1, keepdim=True)


# ================================================================================================================== the decision rule
def rescale_trace(x):
    """Host evaluation of the deferred-rescale rule on log2-domain scores x [..., Q, K] (-inf = masked), 32 keys at a time:
    -> (number of rescales after the first block with a visible key [..., Q], smallest |growth - 6| over those decisions,
    the list of per-block decisions [..., Q] bool)"""
    K = x.shape[-1]
    m_run = torch.full(x.shape[:-1], FLOOR_M, dtype=torch.float64)
    count = torch.zeros(x.shape[:-1], dtype=torch.int64)
    margin = torch.full(x.shape[:-1], float("inf"), dtype=torch.float64)
    decisions = []
    for k0 in range(0, K, 32):
        mloc = x[..., k0: k0 + 32].amax(-1)
        m_cand = torch.maximum(m_run, mloc)
        growth = m_cand - m_run
        grow = growth > GROW
        later = m_run > FLOOR_M
        count += (grow & later).long()
        margin = torch.minimum(margin, torch.where(later, (growth - GROW).abs(), margin))
        decisions.append(grow & later)
        m_run = torch.where(grow, m_cand, m_run)
    return count, margin, decisions


# ================================================================================================================== emulation
def _f32(x):
    return x.to(torch.float32)


def emulate_fwd(q, k, v, mask, keep=None, thr8=0):
    """The forward kernel's arithmetic order in torch fp32: fp32 scores from the bf16 operands, 32-key blocks, the per-query stale-max
    rule, exp2 in fp32 of fma(x, cs, -fl(m cs)), the row sum over the unrounded p, bf16 P into an fp32 P.V, one multiply by 1 / l (times
    256 / (256 - thr8) under dropout), bf16 store.  q, k, v [H, R, 64] (bf16 values), keep [H, R, R] bool.
    -> out [H, R, 64] bf16, lse2 [H, R] fp32"""
    q, k, v = _f32(q), _f32(k), _f32(v)
    return _emulate_blocks(q @ k.transpose(-1, -2), C32, v, mask, keep, thr8)


def bias_log2_f32(gate, table, R):
    """the biased kernel's addend in fp32, as natural units x log2 e: gate . fl(table . 1.4426950f)"""
    return bias_matrix(_f32(gate), _f32(table) * np.float32(LOG2E), R)


def emulate_fwd_bias(q, k, v, mask, gate, table, keep=None, thr8=0):
    """BIAS = 1: x = fma(s, c, gate . fl(table log2 e)) in the log2 domain, then the same blocks with the factor c replaced by 1"""
    q, k, v = _f32(q), _f32(k), _f32(v)
    R = q.shape[1]
    b2 = bias_log2_f32(gate, table, R)
    s = q @ k.transpose(-1, -2)
    xs = _f32(s.double() * C32 + b2.double())
    return _emulate_blocks(xs, 1.0, v, mask, keep, thr8)


def _emulate_blocks(xs, cs, v, mask, keep, thr8):
    cs32 = torch.tensor(cs, dtype=torch.float32)
    xs = xs.masked_fill(~mask.expand_as(xs), float("-inf"))
    Hh, R = xs.shape[0], xs.shape[1]
    m_run = torch.full((Hh, R), FLOOR_M, dtype=torch.float32)
    l = torch.zeros(Hh, R, dtype=torch.float32)
    o = torch.zeros(Hh, R, DH, dtype=torch.float32)
    for k0 in range(0, xs.shape[2], 32):
        xb = xs[..., k0: k0 + 32]
        m_cand = torch.maximum(m_run, xb.amax(-1))
        grow = (m_cand - m_run) * cs32 > 6.0
        m_new = torch.where(grow, m_cand, m_run)
        alpha = torch.exp2((m_run - m_new) * cs32)
        l, o, m_run = l * alpha, o * alpha[..., None], m_new
        mc = m_run * cs32
        p = torch.exp2(_f32(xb.double() * cs - mc.double()[..., None]))
        l = l + p.sum(-1)
        pb = p.to(torch.bfloat16).float()
        if keep is not None:
            pb = pb * keep[..., k0: k0 + 32]
        o = o + pb @ v[:, k0: k0 + 32]
    inv = (np.float32(256.0) / np.float32(256 - thr8) if thr8 else np.float32(1.0)) / l
    return (o * inv[..., None]).to(torch.bfloat16), m_run * cs32 + torch.log2(l)


def emulate_bwd(q, k, v, o_bf, dout, lse2, mask, scale=SCALE, keep=None, thr8=0):
    """The backward kernels' order: fp32 S and dP from bf16 operands, delta = sum dO . O on the STORED bf16 O, P = exp2(fma(s, c, -lse2)),
    bf16 P and dS into fp32 products, bf16 store.  -> dq, dk, dv [H, R, 64] bf16"""
    q, k, v, o_bf, dout = (_f32(t) for t in (q, k, v, o_bf, dout))
    s = q @ k.transpose(-1, -2)
    dp = dout @ v.transpose(-1, -2)
    ds_ = np.float32(256.0) / np.float32(256 - thr8) if thr8 else np.float32(1.0)
    if keep is not None:
        dp = torch.where(keep, dp * ds_, torch.zeros_like(dp))
    delta = (dout * o_bf).sum(-1, keepdim=True)
    P = torch.exp2(_f32(s.double() * C32 - _f32(lse2).double()[..., None]))
    P = torch.where(mask.expand_as(P), P, torch.zeros_like(P))
    dS = (P * (dp - delta)).to(torch.bfloat16).float()
    Pr = P if keep is None else torch.where(keep, P * ds_, torch.zeros_like(P))
    Pr = Pr.to(torch.bfloat16).float()
    sc = np.float32(scale)
    bf = lambda t: t.to(torch.bfloat16)
    return bf((dS @ k) * sc), bf((dS.transpose(-1, -2) @ q) * sc), bf(Pr.transpose(-1, -2) @ dout)


def emulate_short_fwd(q, k, v, mask, scale=SCALE):
    """attn32_fwd_kernel: x = fl(s c), one maximum, p = exp2(x - mx), bf16 p, one multiply by 1 / sum"""
    q, k, v = _f32(q), _f32(k), _f32(v)
    c = np.float32(scale) * np.float32(LOG2E)
    x = ((q @ k.transpose(-1, -2)) * c).masked_fill(~mask.expand(q.shape[0], -1, -1), float("-inf"))
    p = torch.exp2(x - x.amax(-1, keepdim=True))
    inv = 1.0 / p.sum(-1, keepdim=True)
    return ((p.to(torch.bfloat16).float() @ v) * inv).to(torch.bfloat16)


def emulate_short_bwd(q, k, v, dout, mask, scale=SCALE):
    q, k, v, dout = (_f32(t) for t in (q, k, v, dout))
    c = np.float32(scale) * np.float32(LOG2E)
    x = ((q @ k.transpose(-1, -2)) * c).masked_fill(~mask.expand(q.shape[0], -1, -1), float("-inf"))
    P = torch.exp2(x - x.amax(-1, keepdim=True))
    P = P * (1.0 / P.sum(-1, keepdim=True))
    dp = dout @ v.transpose(-1, -2)
    delta = (P * dp).sum(-1, keepdim=True)
    sb = (np.float32(scale) * P * (dp - delta)).to(torch.bfloat16).float()
    pb = P.to(torch.bfloat16).float()
    bf = lambda t: t.to(torch.bfloat16)
    return bf(sb @ k), bf(sb.transpose(-1, -2) @ q), bf(pb.transpose(-1, -2) @ dout)


# ================================================================================================================== planted errors
def plant_missed_rescale(q, k, v, mask, h, i, t):
    """(b): the output and lse2 of query (h, i) when its numerator and row sum accumulated before key block t are NOT multiplied by
    alpha at block t (fp64; alpha = 2^-(growth of the maximum at block t)) -> out row [64], lse2 value"""
    x = ((q[h, i] @ k[h].t()) * SCALE * LOG2E).masked_fill(~mask[h if mask.shape[0] > 1 else 0, i], float("-inf"))
    m_old, m_new = x[: 32 * t].max(), x[: 32 * (t + 1)].max()
    w = torch.exp2(x - x.max())
    w[: 32 * t] = w[: 32 * t] * torch.exp2(m_new - m_old)          # the early terms keep the weight they had under the old maximum
    return (w @ v[h]) / w.sum(), x.max() + torch.log2(w.sum())


def plant_wrong_rescale(q, k, v, mask, h, i, t, growth):
    """(c): query (h, i) needed no rescale at block t but was given its wave-mate's alpha = 2^-growth"""
    x = ((q[h, i] @ k[h].t()) * SCALE * LOG2E).masked_fill(~mask[h if mask.shape[0] > 1 else 0, i], float("-inf"))
    w = torch.exp2(x - x.max())
    w[: 32 * t] = w[: 32 * t] * 2.0 ** -growth
    return (w @ v[h]) / w.sum(), x.max() + torch.log2(w.sum())


def within(got, ref, bound):
    """element-wise criterion -> (ok, largest error / bound, flat index of it)"""
    d = (got.double() - ref.double()).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    i = int(r.argmax())
    return bool((d <= bound).all()), float(r.flatten()[i]), i


def check(rep, case, what, got, ref, bound):
    """prints PARITY|case|quantity|error|rel-L2 (printed only)|bound at the element with the largest error / bound, then records"""
    ok, ratio, i = within(got, ref, bound)
    err = float((got.double() - ref.double()).abs().flatten()[i])
    line = f"PARITY|{case}|{what} @{i}|{err:.3e}|{rel_l2(got, ref):.3e}|{float(bound.flatten()[i]):.3e}|ratio {ratio:.3f}"
    print(line)
    rep.lines.append(line)
    rep.require(case, f"{what}: error {err:.3e} > bound {float(bound.flatten()[i]):.3e} at flat index {i}", ok)
    return ratio


# ================================================================================================================== bias cases
# WavLM's gate[h, i] table[h, Tmax - 1 + j - i]: q . k is noise only, the drift comes from the table (fp32) times gates of mixed sign
# {0, +1, -1, +2}.  Tmax = R, the smallest the kernels accept.  name -> (R, key lengths)
BIAS_CASES = {"bias_stair": (384, [384, 65, 200]), "bias_ramp": (256, [256, 129, 33])}


def build_bias(name):
    """-> dict like build() plus gate [H, B R] fp32, table [H, 2 R - 1] fp32.  Head 0: the table is a staircase of 2.25 per 32 offsets
    (6.49 per key block in the log2 domain at gate 2) or a ramp of 5 / 32 per offset; head 2: the same reversed; head 1: N(0, 1) table,
    gates in (0.5, 2.5)"""
    R, lens = BIAS_CASES[name]
    B = len(lens)
    g = torch.Generator().manual_seed(500 + sorted(BIAS_CASES).index(name))
    q, k = (0.05 * torch.randn(B, R, D, generator=g, dtype=torch.float64) for _ in range(2))
    v = torch.randn(B, R, D, generator=g, dtype=torch.float64)
    gains = torch.stack([wave_gains(R, g) for _ in range(B)]) / A_GAIN
    gate = torch.stack([gains.reshape(-1), 0.5 + 2.0 * torch.rand(B * R, generator=g, dtype=torch.float64), gains.reshape(-1)])
    d = torch.arange(2 * R - 1, dtype=torch.float64)
    prof = 2.25 * torch.div(d, 32, rounding_mode="floor") if name == "bias_stair" else 0.15625 * d
    table = torch.stack([prof, torch.randn(2 * R - 1, generator=g, dtype=torch.float64), prof.flip(0)])
    bf = lambda x: x.to(torch.bfloat16)
    return {"name": name, "R": R, "B": B, "lens": list(lens), "q": bf(q), "k": bf(k), "v": bf(v), "gate": gate.float().contiguous(),
            "table": table.float().contiguous(), "gains": gains}
