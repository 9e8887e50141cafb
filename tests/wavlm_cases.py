"""References for the WavLM tests (tests/test_wavlm_cpu.py, tests/test_gpu_wavlm.py, tests/test_gpu_wavlm_stages.py): one function per quantity, generic in dtype -
the fp64 call is the reference, the fp32 call the yardstick.  Shared stages (conv extractor, padding mask, length rules) come from
``oracle``; what WavLM adds to HuBERT - the bucket table, the gate, the biased softmax, the encoder with them - is restated here
from microsoft/unilm wavlm/modules.py ``MultiheadAttention`` and transformers ``WavLMAttention`` (the two agree formula by formula).

State-dict names are unilm's / s3prl's (encoder.layers.N.self_attn.{q,k,v,out}_proj, grep_linear, grep_a, relative_attention_bias)."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle.hubert_ref import HubertArch, fold_weight_norm, forward_padding_mask, preprocess_input
from oracle.lengths import fairseq_valid_frames, feat_len_rule

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavlm_small.npz")
NUM_BUCKETS, MAX_DISTANCE = 320, 800

# the kernel's own bounds (tests/test_gpu_kernels.py::test_attention)
ATTN_REL_L2, ATTN_MAX_ABS = 1.5e-2, 0.08


def small_arch(stable: bool) -> HubertArch:
    """the fixture's geometry: hidden 128, 2 heads of 64, 2 layers, FFN 256, conv_dim 32, pos_conv 128 taps in 2 groups of 64"""
    return HubertArch(embed_dim=128, ffn_dim=256, layers=2, heads=2, conv_dim=32, extractor_mode="layer_norm" if stable else "default",
                      conv_bias=stable, layer_norm_first=stable, pos_conv_groups=2)


def load_fixture(variant: str) -> dict:
    """-> dict(W = HF-named fp32 weights, wav [B, L] (float16 values), lens, valid, hidden [NL + 1, sum(valid), D] and gates
    [NL, H, sum(valid)] (valid frames, utterance after utterance), bias_row / bias_col [H, 1000]) of ``variant`` in ("post", "stable")"""
    fx = np.load(GOLDEN)
    p = variant + "_"
    out = {k[len(p):]: fx[k] for k in fx.files if k.startswith(p) and not k.startswith(p + "W_")}
    out["W"] = {k[len(p) + 2:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(p + "W_")}
    out["wav"], out["lens"] = fx["wav"].astype(np.float32), fx["lens"]
    for k in [k for k in out if k.startswith("posv_")]:          # pos_conv's direction tensor: [128, 4, 128] int8 / 32, tiled x 16 (the generator)
        out["W"][k[5:]] = (torch.from_numpy(out.pop(k)).float() / 32.0).repeat(1, 16, 1)
    return out


def valid_frames(t: torch.Tensor, valid) -> torch.Tensor:
    """[..., B, T, D] -> [..., sum(valid), D]: the fixture's layout"""
    return torch.cat([t[..., b, :v, :] for b, v in enumerate(valid)], dim=-2)


def conv_feature_extractor(W, arch: HubertArch, x: torch.Tensor) -> torch.Tensor:
    """oracle.hubert_ref.conv_feature_extractor in x's dtype (the oracle's casts its GroupNorm input to fp32, so it cannot serve as the
    fp64 reference): (B, L) -> (B, C, T)"""
    x = x.unsqueeze(1)
    for i, s_ in enumerate(arch.conv_strides):
        pre = f"feature_extractor.conv_layers.{i}."
        x = F.conv1d(x, W[pre + "0.weight"], W.get(pre + "0.bias"), stride=s_)
        if arch.extractor_mode == "default" and i == 0:
            x = F.group_norm(x, arch.conv_dim, W[pre + "2.weight"], W[pre + "2.bias"], 1e-5)
        elif arch.extractor_mode == "layer_norm":
            x = F.layer_norm(x.transpose(1, 2), (arch.conv_dim,), W[pre + "2.1.weight"], W[pre + "2.1.bias"], 1e-5).transpose(1, 2)
        x = F.gelu(x)
    return x


# ------------------------------------------------------------------------------------------------------------------- bucket table
def bucket_of_offsets(d: torch.Tensor, num_buckets: int = NUM_BUCKETS, max_distance: int = MAX_DISTANCE) -> torch.Tensor:
    """WavLM ``_relative_positions_bucket`` of the int64 offsets d = key - query.  The log is torch's, in fp32, over the whole tensor, as
    every public implementation takes it: the reference for this discrete decision IS that expression (the fixture holds its result)."""
    nb = num_buckets // 2
    max_exact = nb // 2
    a = d.abs()
    large = max_exact + torch.log(a.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)
    large = torch.clamp(large.to(torch.long), max=nb - 1)
    return (d > 0).long() * nb + torch.where(a < max_exact, a, large)


def bias_table(rel_embed: torch.Tensor, T: int) -> torch.Tensor:
    """[H, 2 T - 1] in rel_embed's dtype: entry T - 1 + d = embedding of the bucket of offset d"""
    return rel_embed.index_select(0, bucket_of_offsets(torch.arange(-(T - 1), T))).t().contiguous()


# --------------------------------------------------------------------------------------------------------------------------- gate
def gate_ref(x: torch.Tensor, wg: torch.Tensor, bg: torch.Tensor, const: torch.Tensor, H: int) -> torch.Tensor:
    """x [rows, H * 64] -> [H, rows]: a (b const[h] - 1) + 2, a / b = sigmoid of the 4-sums of wg . x_head + bg; in x's dtype"""
    rows = x.shape[0]
    p = F.linear(x.reshape(rows, H, 64), wg.to(x.dtype), bg.to(x.dtype))             # [rows, H, 8]
    ab = torch.sigmoid(p.reshape(rows, H, 2, 4).sum(-1))
    return (ab[..., 0] * (ab[..., 1] * const.to(x.dtype)[None, :] - 1.0) + 2.0).t().contiguous()


# --------------------------------------------------------------------------------------------------------------- biased attention
def biased_attention_ref(q, k, v, scale, gate, table, n_valid: int):
    """One (utterance, head): q / k / v [R, 64], gate [R], table [2 Tmax - 1] -> [R, 64]; keys >= n_valid masked; dtype of q.
    gate / table None: the plain softmax."""
    R = q.shape[0]
    s = (q @ k.t()) * scale
    if gate is not None:
        tmax = (table.numel() + 1) // 2
        i = torch.arange(R)
        s = s + gate[:, None] * table[(tmax - 1) + i[None, :] - i[:, None]]
    s[:, n_valid:] = float("-inf")
    return torch.softmax(s, dim=-1) @ v


# ----------------------------------------------------------------------------------------------------------------------- encoder
def wavlm_forward(W, arch: HubertArch, wavs, dtype=torch.float64, zero_bias: bool = False, final_ln: bool = True, debug=None):
    """The frozen WavLM encoder as s3prl's upstream runs it (pad, chunk-rule key mask, every layer's input + the encoder's output),
    in ``dtype``.  W: unilm-named weights.  -> (hidden states [NL + 1] of [B, T, D], gates [NL] of [B, H, T], valid frames, feat_len).
    ``zero_bias``: the relative-position table zeroed = HuBERT arithmetic on the same weights (the yardstick's reference);
    ``final_ln`` False: the pre-LN order's last state as the HuBERT path hands it out (layer_results, no encoder.layer_norm)."""
    W = {k: v.to(dtype) for k, v in W.items()}
    if "encoder.pos_conv.0.weight" not in W:
        W["encoder.pos_conv.0.weight"] = fold_weight_norm(W["encoder.pos_conv.0.weight_g"], W["encoder.pos_conv.0.weight_v"])
    padded, mask = preprocess_input([w.to(dtype) for w in wavs], arch.normalize_wav)
    padded = padded.to(dtype)
    D, H = arch.embed_dim, arch.heads
    feats = conv_feature_extractor(W, arch, padded).transpose(1, 2)
    feats = F.layer_norm(feats, (arch.conv_dim,), W["layer_norm.weight"], W["layer_norm.bias"], 1e-5)
    B, T = feats.shape[:2]
    pm = forward_padding_mask(T, mask)
    x = F.linear(feats, W["post_extract_proj.weight"], W["post_extract_proj.bias"])
    if debug is not None:
        debug["proj"] = x.clone()              # post_extract_proj's output, every padded frame
    x = x.masked_fill(pm.unsqueeze(-1), 0.0)
    xc = F.conv1d(x.transpose(1, 2), W["encoder.pos_conv.0.weight"], W["encoder.pos_conv.0.bias"], padding=arch.pos_conv_kernel // 2,
                  groups=arch.pos_conv_groups)[:, :, :-1]
    x = x + F.gelu(xc).transpose(1, 2)
    if not arch.layer_norm_first:
        x = F.layer_norm(x, (D,), W["encoder.layer_norm.weight"], W["encoder.layer_norm.bias"], 1e-5)
    table = bias_table(W["encoder.layers.0.self_attn.relative_attention_bias.weight"], T)                  # [H, 2 T - 1]
    if zero_bias:
        table = torch.zeros_like(table)
    i = torch.arange(T)
    pos_bias = table[:, (T - 1) + i[None, :] - i[:, None]]                                                  # [H, T, T]
    hidden, gates = [x], []
    for n in range(arch.layers):
        p = f"encoder.layers.{n}."
        ln = lambda name, t: F.layer_norm(t, (D,), W[p + name + ".weight"], W[p + name + ".bias"], 1e-5)
        h_in = ln("self_attn_layer_norm", x) if arch.layer_norm_first else x
        g = gate_ref(h_in.reshape(B * T, D), W[p + "self_attn.grep_linear.weight"], W[p + "self_attn.grep_linear.bias"],
                     W[p + "self_attn.grep_a"].reshape(-1), H).reshape(H, B, T).transpose(0, 1)           # [B, H, T]
        gates.append(g)
        q, k, v = (F.linear(h_in, W[p + f"self_attn.{m}_proj.weight"], W[p + f"self_attn.{m}_proj.bias"]).view(B, T, H, 64).transpose(1, 2)
                   for m in "qkv")
        s = (q * 64 ** -0.5) @ k.transpose(-1, -2) + g.unsqueeze(-1) * pos_bias.unsqueeze(0)
        s = s.masked_fill(pm[:, None, None, :], float("-inf"))
        o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, D)
        att = F.linear(o, W[p + "self_attn.out_proj.weight"], W[p + "self_attn.out_proj.bias"])
        ffn = lambda t: F.linear(F.gelu(F.linear(t, W[p + "fc1.weight"], W[p + "fc1.bias"])), W[p + "fc2.weight"], W[p + "fc2.bias"])
        if not arch.layer_norm_first:
            x = ln("self_attn_layer_norm", x + att)
            x = ln("final_layer_norm", x + ffn(x))
        else:
            x = x + att
            x = x + ffn(ln("final_layer_norm", x))
        hidden.append(x)
    if arch.layer_norm_first and final_ln:     # the encoder's output, not the last layer's: encoder.layer_norm applied
        hidden[-1] = F.layer_norm(x, (D,), W["encoder.layer_norm.weight"], W["encoder.layer_norm.bias"], 1e-5)
    lens = [len(w) for w in wavs]
    return hidden, gates, fairseq_valid_frames(lens, padded.shape[1], T), feat_len_rule(lens, T, arch.downsample_rate)


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-300))


# ------------------------------------------------------------------------------------ the product's attention call, segment rows
# What tests/test_gpu_wavlm_stages.py records of one ``attn_fwd`` call of the frozen encoder - qk [M, 2 D] bf16 rows, the flat V^T
# buffer (per utterance [H, 64, pitch] back to back at D * row0), gate [H, M] fp32, table [H, 2 R - 1] fp32 - turned into
# attn_cases.fwd_ref calls, one per utterance over its pitch.  Device-agnostic: everything is taken to the CPU in fp64.
STAGE_H, STAGE_PITCH, STAGE_VALID, STAGE_R = 12, (152, 72, 136, 8), (150, 65, 127, 5), 200   # base_small: R of the plan's 64000-sample bucket


def heads_of(x, H):
    """[P, H * 64] -> [H, P, 64]"""
    return x.reshape(x.shape[0], H, 64).transpose(0, 1)


def rows_of(x):
    """[H, P, 64] -> [P, H * 64]"""
    return x.transpose(0, 1).reshape(x.shape[1], -1)


def vt_segment(vt, r0, pitch, H):
    """utterance at row ``r0`` of the flat V^T buffer -> v [H, pitch, 64]"""
    D = H * 64
    return vt.reshape(-1)[D * r0: D * (r0 + pitch)].view(H, 64, pitch).transpose(1, 2)


def pack_vt(v_rows, r0s, pitches, H, slack=0):
    """the inverse (the QKV GEMM's store): v rows [M, H * 64] -> the flat buffer, ``slack`` rows of zeros behind"""
    D = H * 64
    out = torch.zeros(D * (v_rows.shape[0] + slack), dtype=v_rows.dtype)
    for r0, p in zip(r0s, pitches):
        out[D * r0: D * (r0 + p)] = v_rows[r0: r0 + p].view(p, H, 64).permute(1, 2, 0).reshape(-1)
    return out


def segment_attention_ref(qk, vt, gate, table, r0, pitch, valid, H, scale, drop=None, drop_key=None):
    """attn_cases.fwd_ref of the utterance at rows r0 .. r0 + pitch: keys < valid, bias = gate[h, i] table[h, Tmax - 1 + j - i], fp64.
    ``drop`` = (rows of the batch, largest pitch, seed, p): the probability dropout rebuilt from the segment layout's element index;
    ``drop_key`` = (h, query, key) removed from that query's softmax.  -> fwd_ref's dict (out / bound [H, pitch, 64])"""
    import attn_cases as ac
    D = H * 64
    cpu64 = lambda t: t.detach().double().cpu()
    rows = cpu64(qk[r0: r0 + pitch])
    q, k = heads_of(rows[:, :D], H), heads_of(rows[:, D: 2 * D], H)
    v = cpu64(vt_segment(vt, r0, pitch, H))
    bias = ac.bias_matrix(cpu64(gate[:, r0: r0 + pitch]), cpu64(table), pitch)
    mult = None
    if drop is not None:
        rows_total, max_pitch, seed, p = drop
        mult = ac.drop_mult(ac.drop_index_segment(r0, pitch, rows_total, max_pitch, nh=H), seed, p)[0]
    return ac.fwd_ref(q, k, v, ac.key_mask(pitch, valid)[None], scale, bias=bias, mult=mult, drop_key=drop_key)


def rows_rejected(got, ref, bound):
    """[H, P, 64] each -> [P] bool: the query rows with an element outside its bound (the element-wise criterion alone)"""
    d = (got.detach().double().cpu() - ref).abs()
    return (~(d <= bound)).any(2).any(0)


def table_shifted(rel_embed, R):
    """the table read one offset off: entry R - 1 + d holds the embedding of offset d + 1 (j - i + 1)"""
    return bias_table(rel_embed, R + 1)[:, 2:].contiguous()


def table_heads_swapped(table, a=0, b=1):
    t = table.clone()
    t[a], t[b] = table[b], table[a]
    return t


def likeliest_key(f, query, lo, hi):
    """(h, query, key): the key in lo .. hi - 1 and the head whose reference probability for ``query`` is largest - removing a key
    moves the output by about its probability, and only a key that carries some is a fair planted error"""
    p = f["P"][:, query, lo:hi]
    h, j = divmod(int(p.argmax()), hi - lo)
    return h, query, lo + j


def gate_criterion_rejects(got, ref, yard):
    """test_gate_kernel's criterion (head_cases.Report.yard: every element within 4 x the fp32 evaluation's worst) -> (rejected, lines)"""
    import head_cases as hc
    rep = hc.Report()
    rep.yard("sensitivity", "gate", got, ref, yard, dims=())
    return bool(rep.bad), rep.lines


def rehearsal_operands(H=STAGE_H, pitches=STAGE_PITCH, R=STAGE_R, seed=0):
    """Random operands in the recorded call's form, for the CPU rehearsal: LayerNorm-like bf16 rows x [M, D], qk [M + 64, 2 D] and the
    packed V^T of N(0, 1) bf16 values, two layers' gate parameters as random_wavlm_state_dict draws them, a real bucket table"""
    g = torch.Generator().manual_seed(4100 + 7 * H + seed)
    D, M = H * 64, sum(pitches)
    r0s = [sum(pitches[:b]) for b in range(len(pitches))]
    x = torch.randn(M, D, generator=g).to(torch.bfloat16)
    qk = torch.zeros(M + 64, 2 * D, dtype=torch.bfloat16)
    qk[:M] = torch.randn(M, 2 * D, generator=g).to(torch.bfloat16)
    vt = pack_vt(torch.randn(M, D, generator=g).to(torch.bfloat16), r0s, pitches, H, slack=64)
    gp = [(torch.randn(8, 64, generator=g) * 0.125, torch.randn(8, generator=g) * 0.1, 1.0 + 0.3 * torch.randn(H, generator=g)) for _ in range(2)]
    rel = torch.randn(NUM_BUCKETS, H, generator=g)
    return {"H": H, "D": D, "M": M, "r0": r0s, "pitch": list(pitches), "x": x, "qk": qk, "vt": vt, "gate_params": gp, "rel": rel,
            "table": bias_table(rel, R), "R": R}


def emulate_segment(c, gate, b, valid):
    """attn_cases.emulate_fwd_bias (the kernel's arithmetic order in torch fp32) on utterance b of rehearsal_operands -> [H, pitch, 64] bf16"""
    import attn_cases as ac
    H, D, r0, P = c["H"], c["D"], c["r0"][b], c["pitch"][b]
    rows = c["qk"][r0: r0 + P]
    return ac.emulate_fwd_bias(heads_of(rows[:, :D], H), heads_of(rows[:, D:], H), vt_segment(c["vt"], r0, P, H),
                               ac.key_mask(P, valid)[None], gate[:, r0: r0 + P], c["table"])[0]
