"""Helpers of tests/test_gpu_poison.py and tests/test_gpu_poison_bwd.py (not collected on their own; pure torch, no device code): the bit
patterns, the layouts and the masks of the places a kernel READS but the mathematics EXCLUDES (docs/parity.md, "What a kernel reads
and must ignore"; the backward's regions and cases are at the end of the file).

For sc_attn_fwd_bf16 both row layouts share one addressing: utterance b owns ``pitch[b]`` rows at ``row0[b]`` of ``qk`` and the
per-utterance ``[H, 64, pitch[b]]`` block at element ``D * row0[b]`` of the flat ``vt`` (uniform rows: every pitch = R).  A layout here
carries its slack INSIDE the tensors: ``slack`` rows behind the last utterance in ``qk`` and ``slack`` elements behind the last
utterance in ``vt``, so that no read the contract allows leaves the tensor (``read_extent`` computes the largest indices;
tests/test_poison_cases_cpu.py compares them with the allocation for every case the GPU tests run).

The masks mark pad rows (t >= len inside a pitch, all 2 D columns: the q of a pad query and the k of a masked key), pad columns of
every V^T ``d`` row, the gate of pad rows, and the slack.  They are the exact complement of what an fp64 reference reads."""
import contextlib
from types import SimpleNamespace

import torch

FINITE_POISON = (0x7F7F, 0xFF7F, 0x0001, 0x8001)        # bf16: +- the largest finite value, +- the smallest denormal
NONFINITE_POISON = (0x7FC0, 0x7F80, 0xFF80, 0xFFC1)     # bf16: quiet NaN, +Inf, -Inf, a NaN with payload (tests/test_gpu_parallel_head.py)
KT = 64                 # keys per LDS tile of attn_fwd_kernel (csrc/attention.hip:29)
WAVE_Q = 32             # queries per wave (csrc/attention.hip:110-111)
SLACK = 64              # rows of qk / elements of vt behind the last utterance that the contract asks for


# ================================================================================================================== layouts and masks
def layout(pitch, lens, H, slack=SLACK, uniform=False):
    """-> SimpleNamespace: pitch, lens, row0 [B + 1], rows, H, D, slack, uniform, the tensor sizes ``qk_rows`` (= rows + slack) and
    ``vt_numel`` (= D rows + slack), and the boolean masks ``qk`` [qk_rows, 2 D], ``k`` (the k columns of ``qk`` only), ``vt``
    [vt_numel], ``gate`` [H, rows], ``valid_rows`` [rows] (the complement of the pad rows)."""
    pitch, lens = [int(p) for p in pitch], [int(n) for n in lens]
    assert len(pitch) == len(lens) and all(p > 0 and p % 8 == 0 for p in pitch) and all(1 <= n <= p for p, n in zip(pitch, lens))
    D = 64 * H
    row0 = [0]
    for p in pitch:
        row0.append(row0[-1] + p)
    rows = row0[-1]
    valid = torch.zeros(rows, dtype=torch.bool)
    vt = torch.zeros(D * rows + slack, dtype=torch.bool)
    for b, (p, n) in enumerate(zip(pitch, lens)):
        valid[row0[b]: row0[b] + n] = True
        blk = vt[D * row0[b]: D * (row0[b] + p)].view(D, p)            # [H, 64, pitch]: one row per (head, d)
        blk[:, n:] = True
    vt[D * rows:] = True
    qk = torch.ones(rows + slack, 2 * D, dtype=torch.bool)
    qk[:rows][valid] = False
    k = qk.clone()
    k[:, :D] = False
    return SimpleNamespace(pitch=pitch, lens=lens, row0=row0, rows=rows, H=H, D=D, slack=slack, uniform=uniform, qk_rows=rows + slack,
                           vt_numel=D * rows + slack, qk=qk, k=k, vt=vt, gate=(~valid)[None].expand(H, rows).clone(), valid_rows=valid)


def uniform_layout(R, lens, H, slack=SLACK):
    """uniform rows: utterance b at row b R, vt [B, H, 64, R] (+ slack)"""
    return layout([R] * len(lens), lens, H, slack, uniform=True)


def segment_layout(pitch, lens, H, slack=SLACK):
    """ragged rows (sc_segments): a pitch per utterance, vt = per utterance [H, 64, pitch] back to back (+ slack)"""
    return layout(pitch, lens, H, slack, uniform=False)


def read_extent(lay):
    """The largest indices the read contract of sc_attn_fwd_bf16 allows for this layout -> (q row, k row, vt element, gate column):
      q rows   a wave loads 32 query rows, the last wave of an utterance up to row 32 ceil(pitch / 32) - 1 (attention.hip:110-120)
      k rows   whole 64-key tiles up to 64 ceil(n / 64) - 1, n = max(1, min(len, pitch)) (attention.hip:112-113, 131-144, 158-160;
               ``causal`` only lowers n for the q-blocks in front of the last one)
      vt       the same key range of every (head, d) row: D row0 + (h 64 + d) pitch + key (attention.hip:130-132, 139, 142)
      gate     column min(row0 + query, rows - 1) (attention.hip:167)"""
    q_row = k_row = vt_el = gate_col = -1
    for b, (p, n) in enumerate(zip(lay.pitch, lay.lens)):
        r0 = lay.row0[b]
        n = max(1, min(n, p))
        last_key = (n + KT - 1) // KT * KT - 1
        q_last = (p + WAVE_Q - 1) // WAVE_Q * WAVE_Q - 1
        q_row = max(q_row, r0 + q_last)
        k_row = max(k_row, r0 + last_key)
        vt_el = max(vt_el, lay.D * r0 + (lay.D - 1) * p + last_key)
        gate_col = max(gate_col, min(r0 + q_last, lay.rows - 1))
    return q_row, k_row, vt_el, gate_col


def within_allocation(lay):
    """every read of ``read_extent`` stays inside the tensors of ``lay``"""
    q_row, k_row, vt_el, gate_col = read_extent(lay)
    return q_row < lay.qk_rows and k_row < lay.qk_rows and vt_el < lay.vt_numel and gate_col < lay.rows


# ================================================================================================================== bit patterns
def pattern(n, patterns, start=0):
    """[n] int16: the 16-bit patterns cycled from ``start``"""
    p = torch.tensor([v - 0x10000 if v >= 0x8000 else v for v in patterns], dtype=torch.int16)
    return p[(torch.arange(n) + start) % len(patterns)]


def poison_bf16(t, mask, patterns):
    """a copy of the bf16 tensor ``t`` with the patterns, cycled, under the boolean ``mask`` (same shape)"""
    assert t.dtype == torch.bfloat16 and mask.shape == t.shape
    bits = t.contiguous().clone().view(torch.int16)
    bits[mask] = pattern(int(mask.sum()), patterns)
    return bits.view(torch.bfloat16)


def poison_f32(t, mask, patterns):
    """fp32: the bf16 patterns in the upper half-word (+- 3.39e38, +- 2^-133; NaN / Inf for the non-finite set)"""
    assert t.dtype == torch.float32 and mask.shape == t.shape
    bits = t.contiguous().clone().view(torch.int32)
    bits[mask] = pattern(int(mask.sum()), patterns).to(torch.int32) << 16
    return bits.view(torch.float32)


def bits_equal(a, b):
    """same shape, dtype and bit pattern (NaN payloads and the sign of zero count)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return bool((a.contiguous().view(view) == b.contiguous().view(view)).all())


# ================================================================================================================== operands
def operands(lay, seed, tmax=0):
    """seeded N(0, 1) q / k / v on the valid rows, zeros on pad rows and slack -> dict: qk [qk_rows, 2 D] bf16, vt [vt_numel] bf16 (the
    transposed v), per utterance q / k / v [len, D] bf16 (what a reference reads); with ``tmax``: gate [H, rows] in (0.5, 2.5) on the
    valid rows, 0 on pad rows (fp32), and tmax for the caller's table"""
    g = torch.Generator().manual_seed(seed)
    D, H = lay.D, lay.H
    qk = torch.zeros(lay.qk_rows, 2 * D, dtype=torch.bfloat16)
    vt = torch.zeros(lay.vt_numel, dtype=torch.bfloat16)
    utt = []
    for b, (p, n) in enumerate(zip(lay.pitch, lay.lens)):
        r0 = lay.row0[b]
        q, k, v = (torch.randn(n, D, generator=g).to(torch.bfloat16) for _ in range(3))
        qk[r0: r0 + n] = torch.cat([q, k], dim=-1)
        vt[D * r0: D * (r0 + p)].view(D, p)[:, :n] = v.t()
        utt.append((q, k, v))
    out = {"qk": qk, "vt": vt, "utt": utt}
    if tmax:
        gate = torch.zeros(H, lay.rows)
        gate[:, lay.valid_rows] = 0.5 + 2.0 * torch.rand(H, int(lay.valid_rows.sum()), generator=g)
        out["gate"] = gate
    return out


def cut_to_valid(lay, qk, vt, gate=None):
    """what the fp64 reference is given: per utterance q, k, v [len, D] (and gate [H, len]) cut out of the layout's tensors"""
    D = lay.D
    res = []
    for b, (p, n) in enumerate(zip(lay.pitch, lay.lens)):
        r0 = lay.row0[b]
        v = vt[D * r0: D * (r0 + p)].view(D, p)[:, :n].t()
        item = (qk[r0: r0 + n, :D], qk[r0: r0 + n, D:], v)
        res.append(item + ((gate[:, r0: r0 + n],) if gate is not None else ()))
    return res


# ================================================================================================================== the cases of test_gpu_poison.py
H_ATT = 2
TMAX = 400                                                   # >= the largest pitch (264)
# name -> (uniform, pitch, lens)
GEOMETRIES = {
    "uniform R=56": (True, [56, 56, 56], [50, 50, 50]),       # ViT-B/32: the over-read lands in the next image and in the slack
    "uniform R=264": (True, [264, 264], [257, 257]),          # ViT-L/14: one valid key in the last tile
    "uniform R=128": (True, [128, 128, 128], [128, 1, 37]),
    "segment 56x3": (False, [56, 56, 56], [50, 50, 50]),
    "segment 264/8/136": (False, [264, 8, 136], [257, 1, 129]),
}
INSTANCES = ("plain", "drop", "causal", "bias")
DRIVER_GEOMETRIES = {"padded": (True, [56, 56, 56], [50, 37, 9]), "segment": (False, [56, 40, 16], [50, 37, 9])}


def attention_cases():
    """-> list of (geometry name, instance, use_work): every geometry x instance, the ragged three-utterance geometry with and
    without the work list, and causal = 32 at uniform R = 128"""
    cases = []
    for name, (uniform, _, _) in GEOMETRIES.items():
        for inst in INSTANCES:
            cases.append((name, inst, True))
            if name == "segment 264/8/136":
                cases.append((name, inst, False))
    cases.append(("uniform R=128", "causal32", True))
    return cases


def case_layout(name, table=GEOMETRIES):
    uniform, pitch, lens = table[name]
    return layout(pitch, lens, H_ATT, SLACK, uniform=uniform)


CAUSAL_OF = {"plain": 0, "drop": 0, "bias": 0, "causal": 1, "causal32": 32}


# ================================================================================================================== layer driver workspace
def driver_workspace(rows, D, F, slack=SLACK):
    """The workspace sc_workspace_bytes(SC_WS_HUBERT_LAYER, rows, D, F) describes (include/speechclip_hip.h), in bf16 elements:
    -> (total, {name: (offset, numel)}) for qk, qk_slack, vt, vt_slack, ctx, pre, x1, ffn, in that order"""
    parts = (("qk", rows * 2 * D), ("qk_slack", slack * 2 * D), ("vt", rows * D), ("vt_slack", slack), ("ctx", rows * D),
             ("pre", rows * D), ("x1", rows * D), ("ffn", rows * F))
    off, table = 0, {}
    for name, n in parts:
        table[name] = (off, n)
        off += n
    return off, table


# ================================================================================================================== torch.empty
@contextlib.contextmanager
def poisoned_empty():
    """For the duration: torch.empty, torch.empty_like and Tensor.new_empty return floating tensors filled with NaN (other dtypes
    untouched), so a result that depends on memory nobody wrote shows.  The originals are restored on every way out."""
    orig = (torch.empty, torch.empty_like, torch.Tensor.new_empty)

    def wrap(fn):
        def poisoned(*args, **kwargs):
            t = fn(*args, **kwargs)
            if isinstance(t, torch.Tensor) and t.is_floating_point() and t.numel():
                with torch.no_grad():
                    t.fill_(float("nan"))
            return t
        poisoned.__wrapped__ = fn
        return poisoned

    torch.empty, torch.empty_like, torch.Tensor.new_empty = wrap(orig[0]), wrap(orig[1]), wrap(orig[2])
    try:
        yield
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = orig


# ================================================================================================================== backward: regions
# sc_attn_bwd_bf16 / sc_attn_bwd_fused_bf16 (csrc/attention_bwd.hip), uniform rows, R % 128 == 0.  A row t of utterance b is a KEY of
# one of four regions and a QUERY of one of four (docs/parity.md, "Backward"); n = valid_len[b], up = ceil to a multiple:
#   keys      valid [0, n) | tail32 [n, up32(n)) | tail128 [up32(n), up128(n)) | padded [up128(n), R)
#   queries   valid [0, n) | q_pad  [n, q_rows)  | q_blk   [q_rows, up32(q_rows)) | q_far [up32(q_rows), R)
BWD_KEY_REGIONS = ("valid", "tail32", "tail128", "padded")
BWD_QUERY_REGIONS = ("valid", "q_pad", "q_blk", "q_far")
# name -> (R, lens, q_rows): the smallest geometries that reach every branch (tests/test_gpu_poison_bwd.py names them)
BWD_GEOMETRIES = {"R=128": (128, [128, 1, 37], 128), "R=256": (256, [200, 129, 65], 200)}
BWD_INSTANCES = ("plain", "drop", "causal")
BWD_ENTRIES = ("fused", "unfused")
ORDINARY = 64.0                                              # the N(0, 64^2) scratch of test_layer_driver_ignores_pad_rows_and_workspace_content


def _up(n, m):
    return (n + m - 1) // m * m


def bwd_layout(R, lens, q_rows, H=H_ATT):
    """-> SimpleNamespace: B, R, lens, q_rows, H, D, rows = B R and one boolean [rows] mask per region name (``key`` / ``query``
    dicts); ``valid`` is the same mask in both"""
    lens = [int(n) for n in lens]
    assert R % 128 == 0 and all(1 <= n <= R for n in lens) and max(lens) <= q_rows <= R
    B = len(lens)
    t = torch.arange(R)
    key = {n: torch.zeros(B, R, dtype=torch.bool) for n in BWD_KEY_REGIONS}
    query = {n: torch.zeros(B, R, dtype=torch.bool) for n in BWD_QUERY_REGIONS}
    for b, n in enumerate(lens):
        key["valid"][b] = t < n
        key["tail32"][b] = (t >= n) & (t < _up(n, 32))
        key["tail128"][b] = (t >= _up(n, 32)) & (t < _up(n, 128))
        key["padded"][b] = t >= _up(n, 128)
        query["valid"][b] = t < n
        query["q_pad"][b] = (t >= n) & (t < q_rows)
        query["q_blk"][b] = (t >= max(n, q_rows)) & (t < _up(q_rows, 32))
        query["q_far"][b] = t >= _up(q_rows, 32)
    flat = lambda d: {n: m.reshape(-1) for n, m in d.items()}
    return SimpleNamespace(B=B, R=R, lens=lens, q_rows=q_rows, H=H, D=64 * H, rows=B * R, key=flat(key), query=flat(query),
                           valid=key["valid"].reshape(-1))


def bwd_case_layout(name):
    return bwd_layout(*BWD_GEOMETRIES[name])


def row_mask(rows_mask, cols):
    """[rows] -> [rows, cols]"""
    return rows_mask[:, None].expand(-1, cols).contiguous()


def col_mask_T(lay, rows_mask):
    """[B R] -> [B, H, 64, R]: the columns of a per-head transposed copy (sc_head_transpose_bf16) that hold those rows"""
    return rows_mask.view(lay.B, 1, 1, lay.R).expand(lay.B, lay.H, 64, lay.R).contiguous()


def stat_mask(lay, rows_mask):
    """[B R] -> [B, H, R]: lse2 / delta of those rows"""
    return rows_mask.view(lay.B, 1, lay.R).expand(lay.B, lay.H, lay.R).contiguous()


def head_transpose(x, lay):
    """host form of sc_head_transpose_bf16: [B R, H 64] -> [B, H, 64, R]"""
    return x.view(lay.B, lay.R, lay.H, 64).permute(0, 2, 3, 1).contiguous()


def bwd_operands(lay, seed):
    """seeded N(0, 1) q / k / v / dout [B R, D] bf16 on the valid rows, exact zeros elsewhere, and ``scratch`` [B R, D] bf16 ~ N(0, 64^2)
    (what a region of class "finite and of ordinary magnitude" is given)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n in ("q", "k", "v", "dout"):
        t = torch.zeros(lay.rows, lay.D)
        t[lay.valid] = torch.randn(int(lay.valid.sum()), lay.D, generator=g)
        out[n] = t.to(torch.bfloat16)
    out["scratch"] = (ORDINARY * torch.randn(lay.rows, lay.D, generator=g)).to(torch.bfloat16)
    return out


def put(t, mask, src):
    """a copy of ``t`` with the elements of ``src`` under ``mask`` (same shapes)"""
    t = t.clone()
    t[mask] = src[mask]
    return t


def bwd_read_extent(lay):
    """The largest row of an utterance that csrc/attention_bwd.hip touches, per kernel -> dict (all must be < R; R % 128 == 0 is what
    makes it so, attention_bwd.hip:523):
      dq_query   every row of the utterance: R - 1 (:89-107, no use of q_rows)
      dq_key     whole 64-key tiles of K, V and K^T up to 64 ceil(n / 64) - 1 (:138-159)
      dkv_key    the 128 keys of every workgroup: R - 1 (:251-275)
      dkv_query  whole 64-row tiles of q, dout, q^T, dout^T, lse2, delta up to 64 ceil(q_rows / 64) - 1 (:288-311)
      prep       the transposes and delta: every row, R - 1 (:416-433, :465-503)"""
    n = max(max(1, min(v, lay.R)) for v in lay.lens)
    return {"dq_query": lay.R - 1, "dq_key": _up(n, 64) - 1, "dkv_key": lay.R - 1, "dkv_query": _up(lay.q_rows, 64) - 1, "prep": lay.R - 1}


# ================================================================================================================== backward: row reducers
REDUCER_LENS = [128, 1, 37]                                  # rows = 3 x 128, valid rows per block of 128
REDUCER_PITCH = 128
REDUCERS = ("wgrad_tn", "wgrad_transposing", "wgrad_list", "colsum", "ln_acc", "ln_acc_drop_sum", "ln_dres", "posconv_wgrad", "wsum_seg")
SHORT_PROMPTS = [32, 1, 17]                                  # sc_attn32_bwd_bf16: prompt rows of the three 32-row sequences


def reducer_valid(pitch=REDUCER_PITCH, lens=REDUCER_LENS):
    """[len(lens) pitch] bool: rows t < len of every block"""
    t = torch.arange(pitch)
    return torch.cat([t < n for n in lens])


def short_valid(prompts=SHORT_PROMPTS):
    return reducer_valid(32, prompts)


# ================================================================================================================== keyword side
# tests/test_gpu_poison_kw.py (docs/parity.md, "What a kernel reads and must ignore", subsection "Keyword side").  Every layout below
# carries its padding INSIDE its tensors; ``*_read_extent`` gives, per operand, (the largest element index a kernel's contract allows,
# the allocation's numel) and tests/test_poison_cases_cpu.py holds the first below the second for every case the GPU tests run.
KW_NK = (5, 130)                # keywords: Nkp = 128 and 256 (130 = 2 above a 128-row tile)
KW_V = (200, 8112)              # vocabularies: Vp = 256 and 8192, both with pad columns
KW_ET = 64
KW_TOPK = (5, 40)               # sc_topk_rows_f32 (k <= 32) and sc_topk_rows_wide_f32


def roundup(n, m):
    return (n + m - 1) // m * m


def quantiser_layout(Nk, V, Et=KW_ET):
    """The padded operands of the keyword quantiser (vector_quantizers.VocabTables, ops.vq_prep / split3_bf16 / cosine_scores_split /
    vq_soft_split / vq_soft_table) -> SimpleNamespace with Nk, V, Et, Nkp, Vp (both rounded up to 128), Ep (Et rounded up to 64) and
    the boolean masks of the padding:
      kw_split [Nkp, 6 Ep]   rows >= Nk                  kwn_T [Et, Nkp]   columns >= Nk
      table_split [Vp, 6 Ep] rows >= V                   norm_T [Et, Vp]   columns >= V
      cos [Nkp, Vp]          rows >= Nk or columns >= V (cos_rows / cos_cols apart)
      s_split [Nkp, 3 Vp]    rows >= Nk                  w_split [Et, 3 Vp] columns >= V of each of the three K-blocks"""
    Nkp, Vp, Ep = roundup(Nk, 128), roundup(V, 128), roundup(Et, 64)
    r, v = torch.arange(Nkp) >= Nk, torch.arange(Vp) >= V
    cos_rows, cos_cols = r[:, None].expand(Nkp, Vp).contiguous(), v[None].expand(Nkp, Vp).contiguous()
    return SimpleNamespace(Nk=Nk, V=V, Et=Et, Nkp=Nkp, Vp=Vp, Ep=Ep, kw_split=row_mask(r, 6 * Ep), kwn_T=r[None].expand(Et, Nkp).contiguous(),
                           table_split=row_mask(v, 6 * Ep), norm_T=v[None].expand(Et, Vp).contiguous(), cos_rows=cos_rows, cos_cols=cos_cols, cos=cos_rows | cos_cols,
                           s_split=row_mask(r, 3 * Vp), w_split=v.repeat(3)[None].expand(Et, 3 * Vp).contiguous())


def quantiser_read_extent(lay, k=max(KW_TOPK)):
    """operand -> (largest element index read, numel):
      the two GEMMs read whole operands (sc_gemm_bf16 on [Nkp, 6 Ep] x [Vp, 6 Ep], csrc/vq.hip:171 on [Et, Nkp] x [Et, Vp]; the soft
      product on [Nkp, 3 Vp] x [Et, 3 Vp]): last element of each;
      the row kernels (vq.hip:283-325 rowstats, :329-340 colprob, :461-487 noisy rowstats, :498-505 soft prob, :508-530 soft split,
      :533-568 soft bwd2, :398-421 soft bwd) and the selections (topk.hip:20-26, topk_wide.hip:149) walk rows < Nk, columns < V of
      a matrix of row pitch Vp: element (Nk - 1) Vp + V - 1"""
    K6, K3 = 6 * lay.Ep, 3 * lay.Vp
    return {"kw_split": (lay.Nkp * K6 - 1, lay.Nkp * K6), "table_split": (lay.Vp * K6 - 1, lay.Vp * K6),
            "kwn_T": (lay.Et * lay.Nkp - 1, lay.Et * lay.Nkp), "norm_T": (lay.Et * lay.Vp - 1, lay.Et * lay.Vp),
            "s_split": (lay.Nkp * K3 - 1, lay.Nkp * K3), "w_split": (lay.Et * K3 - 1, lay.Et * K3),
            "cos": ((lay.Nk - 1) * lay.Vp + lay.V - 1, lay.Nkp * lay.Vp)}


# ---- CIF (csrc/cif.hip): B utterances of S frames, C channels, T + 1 slots
CIF_S, CIF_C, CIF_T = 90, 24, 6
CIF_LENS = (90, 1, 37, 64)      # S itself, one frame, off every 8-frame batch, on one
CIF_TARGETS = (6, 0, 3, 1)      # keyword counts the weights are scaled to (0: an utterance that never fires)


def frame_mask(lens, S):
    """[B, S] bool: frames t >= len"""
    return torch.arange(S)[None] >= torch.as_tensor(lens)[:, None]


def slot_mask(last, T, at=False):
    """[B, T + 1] bool: the slots behind ``last[b]`` (``at``: that slot too)"""
    return torch.arange(T + 1)[None] >= (torch.as_tensor(last)[:, None] + (0 if at else 1))


def cif_case(lens=CIF_LENS, targets=CIF_TARGETS, S=CIF_S, C=CIF_C, seed=90):
    """alpha / csum as sc_cif_prepare forms them with apply_scaling (the weights of utterance b sum to target + 1e-5, csum = the fp64
    scan rounded once; exactly 0 / constant on the frames t >= len), frames x of values bf16 holds, zero on the frames t >= len ->
    dict with alpha, csum, x, pad [B, S] (t >= len), last [B] = the slot the last frame lands in (= the keyword count), and the
    operands sc_cif_prepare_bwd takes beside pa / pb: a_clip (the weights before the scaling, 0 on the frames t >= len), ratio,
    quantity, gq [B]"""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    pad = frame_mask(lens, S)
    a = torch.rand(B, S, generator=g).double() * (~pad)
    q = a.sum(-1, keepdim=True)
    a_clip, quantity = a.float(), q[:, 0].float()
    ratio = ((torch.tensor(targets).double() + 1e-5) / q[:, 0]).float()
    a = (a * (torch.tensor(targets).double()[:, None] + 1e-5) / q).float()
    csum = a.double().cumsum(-1).float()
    x = torch.randn(B, S, C, generator=g).to(torch.bfloat16).float() * (~pad)[..., None]
    last = torch.floor(csum[:, -1]).long().clamp(0, CIF_T)
    return {"alpha": a.contiguous(), "csum": csum.contiguous(), "x": x.contiguous(), "pad": pad, "last": last, "lens": list(lens),
            "B": B, "S": S, "C": C, "a_clip": a_clip.contiguous(), "ratio": ratio, "quantity": quantity,
            "gq": torch.randn(B, generator=g)}


def cif_read_extent(c, T=CIF_T):
    """operand -> (largest element index read, numel): every frame kernel walks all S frames of every utterance (cif.hip:99-126,
    :156-200, :258-270, :297-325) and the slots 0 .. right of the last frame <= T of g (cif.hip:158-182, :308-316); the tail walks
    the S weights (cif.hip:491-500) and slot feat_len <= T of out (:506-509)"""
    B, S, C = c["B"], c["S"], c["C"]
    return {"x": (B * S * C - 1, B * S * C), "alpha": (B * S - 1, B * S), "csum": (B * S - 1, B * S),
            "g": ((B - 1) * (T + 1) * C + int(c["last"].max()) * C + C - 1, B * (T + 1) * C), "out": (B * (T + 1) * C - 1, B * (T + 1) * C)}


# ---- masked keys: the row softmax of the attention block (csrc/softmax.hip) and the constant-query pool (csrc/kwpool.hip)
KEY_LENS = (70, 1, 37)
KEY_T, KEY_N, KEY_H, KEY_D = 70, 72, 2, 256          # n = 72: the frames' pitch, a multiple of 8 above T


def key_mask(lens, n):
    """[B, n] bool: keys k >= len (the pad keys between T and n included)"""
    return frame_mask(lens, n)


def pool_frames_mask(flen, R, row0):
    """[B, R] bool: the rows of X that are no frame of the utterance (the CLS slot in front of row0, rows behind row0 + flen)"""
    r = torch.arange(R)[None]
    fl = torch.as_tensor(flen).long()[:, None]
    return (r < row0) | (r >= row0 + fl)


def key_read_extent(B, H, n, Q, C, R, D):
    """softmax: whole rows of scores / dP / P [B H T, n] and of the mask [B, n] (softmax.hip:30-38, :94-100); pool: whole X [B, R, D]
    rows are addressed only inside [row0, row0 + flen) (kwpool.hip:22-80, :83-180), p / mult [B, Q, C + R] whole"""
    rows = B * H * KEY_T
    return {"scores": (rows * n - 1, rows * n), "mask": (B * n - 1, B * n), "X": (B * R * D - 1, B * R * D),
            "p": (B * Q * (C + R) - 1, B * Q * (C + R))}


# ---- keyword prompt (csrc/prompt.hip)
PROMPT_N, PROMPT_W, PROMPT_SEG, PROMPT_NPOS = 6, 64, 16, 10
PROMPT_COUNTS = (6, 0, 3, 1)


def prompt_mask(count, N):
    """[B, N] bool: keyword rows j >= count[b]"""
    return torch.arange(N)[None] >= torch.as_tensor(count)[:, None]


def prompt_read_extent(B, Bp, N, W, SEG, n_pos, count):
    """keywords [B, N, W]: rows j < min(count, N) only (prompt.hip:36: t < index, zero past N); dX [Bp SEG, W]: rows b SEG + j + 1 for
    j + 1 < min(count + 1, n_pos) (prompt.hip:104-106)"""
    c = max(min(int(v), N) for v in count)
    return {"keywords": ((B - 1) * N * W + c * W - 1, B * N * W), "dX": (((B - 1) * SEG + min(c, n_pos - 1)) * W + W - 1, Bp * SEG * W)}


def plant(t, mask, value=float("nan")):
    """a copy of ``t`` with ``value`` in the FIRST element ``mask`` marks - the planted check of a mask: put where the mathematics does
    read, it must change the output; an empty mask plants nothing, and the caller's comparison must then report "unchanged" """
    t = t.clone()
    idx = mask.reshape(-1).nonzero()
    if idx.numel():
        t.view(-1)[int(idx[0])] = value
    return t


def changed(got, clean, names):
    """the planted check's verdict: the names among ``names`` whose tensors no longer carry the clean run's bits (an empty list: the
    plant reached nothing - the caller must fail)"""
    return [n for n in names if not bits_equal(got[n], clean[n])]
