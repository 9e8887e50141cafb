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
    view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
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
