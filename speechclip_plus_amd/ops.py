"""Tensor-level wrappers over the C ABI (raw device pointers, current HIP stream).

torch is used here only for device memory and streams.  Every function requires device tensors and the
built extension; nothing falls back to eager PyTorch or the CPU.
"""
import ctypes
from typing import Optional

import torch

from ._lib import DEFINES, RtGemmArgs, RtLnArgs, RtLnBwdArgs, GemmArgs, HubertLayerArgs, Segments, check, diag_lib, lib


def _p(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    if t is None:
        return ctypes.c_void_p(0)
    if not t.is_cuda:
        raise RuntimeError("speechclip_plus_amd ops need device (HIP) tensors; there is no CPU path")
    return ctypes.c_void_p(t.data_ptr())


def _seg(seg: Optional["RowSegments"]):
    """the ``seg`` argument of an entry point that takes either row layout: NULL = uniform rows"""
    return seg.ref() if seg is not None else None


def aligned16(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself when its storage offset is 16-byte aligned, else a fresh copy (trainable parameters are views into the
    optimiser's flat buffer at 4-byte granularity; kernels that load 16 bytes per lane need aligned bases)."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class RowSegments:
    """Ragged row layout of one batch (``sc_segments``, include/speechclip_hip.h): utterance b owns rows [row0[b], row0[b + 1]) -
    its own pitch, a multiple of 8 rows - of every activation buffer of the encoder.  Built on the host from the batch's lengths
    (``host_tables``: pure python, tested on the CPU) and uploaded in one pinned, asynchronous copy.

    ``pitch`` [B] rows per utterance; ``keys`` [B] the key count that sorts the attention work list (longest first)."""

    GRAN = DEFINES["SC_SEG_ROWS"]      # 8: pitches are multiples of this; one chunk-table entry per GRAN rows

    def __init__(self, pitch, keys, device, storage: Optional[torch.Tensor] = None, keys_known: bool = True):
        host, self.row0_host, self.n_work = self.host_tables(pitch, keys, keys_known)
        self.pitch = [int(p) for p in pitch]
        self.B, self.rows, self.max_pitch = len(self.pitch), self.row0_host[-1], max(self.pitch)
        n = host.numel()
        if storage is not None:
            assert storage.dtype == torch.int32 and storage.numel() >= n and storage.data_ptr() % 16 == 0
            dev = storage[:n]
            dev.copy_(host.pin_memory(), non_blocking=True)
        else:
            dev = host.pin_memory().to(device, non_blocking=True)
        nch = self.rows // self.GRAN
        self.chunk = dev[: 4 * nch]                              # 16-byte entries first: they stay 16-byte aligned
        self.work = dev[4 * nch: 4 * nch + 4 * self.n_work]
        self.row0 = dev[4 * nch + 4 * self.n_work:]
        self._dev = dev
        self.c = Segments()
        self.c.row0, self.c.chunk = _p(self.row0), _p(self.chunk)
        self.c.B, self.c.rows, self.c.max_pitch = self.B, self.rows, self.max_pitch

    @classmethod
    def table_ints(cls, B: int, max_rows: int) -> int:
        """upper bound of the table size in int32 (storage for a plan: B utterances, at most ``max_rows`` rows)"""
        return 4 * (max_rows // cls.GRAN) + B + 1 + 4 * B * ((max_rows + 127) // 128 + 1)

    @classmethod
    def host_tables(cls, pitch, keys, keys_known: bool = True):
        """-> (int32 tensor [chunk table | attention work list | row0], row0 as a python list, number of work items).
        chunk[c] = (first row, pitch, utterance, 0) of the utterance that owns rows 8 c .. 8 c + 7; work = one int4 item per
        128-query block, (utterance | q-block << 16, first row, pitch, key count or -1), longest utterance first (its workgroups run
        longest: start them first).  ``keys_known`` False: the key counts only order the list (the kernel reads valid_len)."""
        import numpy as np
        B, G = len(pitch), cls.GRAN
        p = np.asarray([int(x) for x in pitch], dtype=np.int64)
        assert B < 65536 and (p > 0).all() and (p % G == 0).all()
        row0 = np.concatenate([[0], np.cumsum(p)])
        per = np.stack([row0[:-1], p, np.arange(B), np.zeros(B, dtype=np.int64)], axis=1)         # one entry per utterance
        chunk = np.repeat(per, p // G, axis=0).reshape(-1)
        order = sorted(range(B), key=lambda b: (-int(keys[b]), b))
        work = [(b | (qb << 16), int(row0[b]), int(p[b]), int(keys[b]) if keys_known else -1)
                for b in order for qb in range((int(p[b]) + 127) // 128)]
        tab = np.concatenate([chunk, np.asarray(work, dtype=np.int64).reshape(-1), row0]).astype(np.int32)
        return torch.from_numpy(tab), [int(x) for x in row0], len(work)

    def ref(self):
        return ctypes.byref(self.c)


class KernelTimer:
    """Optional per-launch HIP-event timing (bench.py): events are recorded on the stream the kernel is
    launched on; ``work`` is the ALGORITHMIC flop (or byte) count the caller attributes to the launch."""

    def __init__(self):
        self.records = {}
        self.tagged = {}

    def add(self, name, start, end, work, tag=None):
        self.records.setdefault(name, []).append((start, end, work))
        if tag is not None:
            self.tagged.setdefault(tag, []).append((start, end, work))

    def summary_by_tag(self):
        return {tag: {"launches": len(r), "ms": sum(s.elapsed_time(e) for s, e, _ in r), "work": float(sum(w for _, _, w in r))}
                for tag, r in self.tagged.items()}

    def summary(self):
        out = {}
        for name, recs in self.records.items():
            ms = sum(s.elapsed_time(e) for s, e, _ in recs)
            out[name] = {"launches": len(recs), "ms": ms, "work": float(sum(w for _, _, w in recs))}
        return out


_timer: Optional[KernelTimer] = None


def set_timer(t: Optional[KernelTimer]) -> None:
    global _timer
    _timer = t


def gemm_tile_name(M: int, N: int, K: int, n_split: int, batch: int, tile: int = 0) -> str:
    """Mirror of the tile selection in sc_gemm_bf16 (csrc/gemm_bf16.hip), for reporting only."""
    if tile == 0:
        if N <= 64 and n_split < 0:
            tile = 3
        elif M >= 512 and N >= 192 and ((M + 255) // 256) * ((N + 255) // 256) * batch >= 192 and (n_split < 0 or n_split % 64 == 0):
            tile = 2
        else:
            tile = 1
    return {1: "128x128", 2: "256x256", 3: "128x64", 7: "256x256", 8: "256x256", 9: "128x256_duo", 10: "128x256_duo", 11: "128x256_duo"}.get(tile, "diag")


def gemm_raw(A: torch.Tensor, lda: int, W: torch.Tensor, ldw: int, C: torch.Tensor, ldc: int, M: int, N: int, K: int,
             bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, ldr: int = 0, act: int = 0,
             out_f32: bool = False, Ct: Optional[torch.Tensor] = None, n_split: int = -1, R: int = 0, dh: int = 0,
             nb1: int = 1, nb2: int = 1, sA=(0, 0), sW=(0, 0), sC=(0, 0), sBias=(0, 0), sR=(0, 0),
             alg_rows: Optional[int] = None, tile: int = 0, drop_p: float = 0.0, drop_seed: int = 0, tap_c: int = 0,
             ln_stats: Optional[torch.Tensor] = None, ln_ns: int = 0, ln_colsum: Optional[torch.Tensor] = None,
             res_stats: Optional[torch.Tensor] = None, res_ns: int = 0, res_gamma: Optional[torch.Tensor] = None,
             res_beta: Optional[torch.Tensor] = None, stats_out: Optional[torch.Tensor] = None, ln_eps: float = 0.0,
             tn: bool = False, k_total: int = 0, aux: Optional[torch.Tensor] = None, aux_mode: int = 0,
             seg: Optional["RowSegments"] = None, a_rep: int = 0) -> int:
    """C = epi(A . W^T); see sc_gemm_args in include/speechclip_hip.h.  Pointers are the tensors' data_ptr()
    (pass a sliced view to offset).  ``alg_rows``: rows that are algorithmic work (excludes layout padding),
    used only by the optional KernelTimer.  ``ln_*`` / ``res_*`` / ``stats_out``: LayerNorm folded into the GEMM (row-statistics
    buffers are [M, 8, 2] fp32); returns the number of statistics strips written per row (0 without ``stats_out``).
    ``a_rep`` = 2: ``W`` is the [N, 2K] hi / lo interleave of ``split_weight_bf16`` and every A tile is read twice (``K`` stays A's)."""
    assert A.dtype == torch.bfloat16 and W.dtype == torch.bfloat16
    assert C.dtype == (torch.float32 if out_f32 else torch.bfloat16)
    if bias is not None:
        assert bias.dtype == torch.float32
        bias = aligned16(bias)          # sc_gemm_bf16 reads the bias in 16-byte groups; trainable biases are 4-byte-aligned views
    if residual is not None:
        assert residual.dtype == torch.bfloat16
    a = GemmArgs()
    a.A, a.lda, a.W, a.ldw, a.C, a.ldc = _p(A), lda, _p(W), ldw, _p(C), ldc
    a.M, a.N, a.K = M, N, K
    a.bias, a.residual, a.ldr = _p(bias), _p(residual), ldr
    a.act, a.out_f32 = act, int(out_f32)
    a.Ct, a.n_split, a.R, a.dh = _p(Ct), n_split, R, dh
    a.nb1, a.nb2 = nb1, nb2
    a.sA1, a.sA2 = sA
    a.sW1, a.sW2 = sW
    a.sC1, a.sC2 = sC
    a.sBias1, a.sBias2 = sBias
    a.sR1, a.sR2 = sR
    a.tile = tile
    a.drop_p, a.drop_seed = float(drop_p), int(drop_seed) & 0xffffffff
    a.tap_c = int(tap_c)
    a.k_total = int(k_total)
    a.a_rep = int(a_rep)
    if aux_mode == 3:       # forward-only twin of mode 1: the activation of the rounded pre-activation, which is not stored
        assert aux is None and Ct is None
        a.aux_mode = 3
    elif aux_mode:          # activation fused with a second [M, N] bf16 operand of C's row stride (sc_gemm_args.aux_mode)
        assert aux is not None and aux.dtype == torch.bfloat16 and Ct is None and aux.stride(0) == ldc and aux.stride(1) == 1
        a.Ct, a.aux_mode = _p(aux), int(aux_mode)
    a.tn = int(tn)          # C[m, n] = sum_r A[r, m] W[r, n]: both operands row-indexed by the reduction (weight gradients)
    if seg is not None:     # ragged rows: the transposed (V^T) store looks its utterance up per 32-row chunk
        assert M == seg.rows
        a.seg_chunk = _p(seg.chunk)
    strips = 0
    if ln_colsum is not None and ln_stats is None and stats_out is None:
        # LayerNorm in the GEMM's prologue (128- / 64-row tiles, round 6): A holds raw rows, W = W0 diag(gamma), bias = c_n, the row
        # statistics are computed by the kernel (csrc/gemm_bf16.hip: ln_self)
        assert ln_colsum.dtype == torch.float32 and ln_colsum.is_contiguous() and ln_colsum.numel() == N and ln_eps > 0.0 and K <= 1024
        a.ln_colsum, a.ln_eps = _p(ln_colsum), float(ln_eps)
    if ln_stats is not None or stats_out is not None:
        for t in (ln_stats, ln_colsum, res_stats, res_gamma, res_beta, stats_out):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
        a.ln_stats, a.ln_ns, a.ln_colsum = _p(ln_stats), int(ln_ns), _p(ln_colsum)
        a.res_stats, a.res_ns, a.res_gamma, a.res_beta = _p(res_stats), int(res_ns), _p(res_gamma), _p(res_beta)
        a.stats_out, a.ln_eps = _p(stats_out), float(ln_eps)
        if stats_out is not None:
            assert stats_out.numel() >= M * 16
            strips = int(diag_lib().sc_gemm_stats_strips(ctypes.byref(a)))
    # diagnostic tile ids and the opt-in LayerNorm-folded GEMMs exist in the diagnostics library only (the product library refuses them)
    L = diag_lib() if (tile in (32, 34) or ln_stats is not None or stats_out is not None) else lib()
    if _timer is None:
        check(L.sc_gemm_bf16(ctypes.byref(a), _stream()), "sc_gemm_bf16", L)
        return strips
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    check(L.sc_gemm_bf16(ctypes.byref(a), _stream()), "sc_gemm_bf16", L)
    ev1.record()
    rows = (M if alg_rows is None else alg_rows) * nb1 * nb2
    _timer.add("gemm_bf16_" + gemm_tile_name(M, N, K, n_split, nb1 * nb2, 2 if (tile == 0 and strips + ln_ns > 0) else tile), ev0, ev1,
               2.0 * rows * N * K, tag=f"M{M} N{N} K{K} lda{lda} act{act} res{int(residual is not None)} z{nb1 * nb2}")
    return strips


def hubert_layer_fwd(x: torch.Tensor, out: torch.Tensor, valid_len: torch.Tensor, w: dict, i: int, pl, B: int, R: int, T: int, D: int,
                     F_: int, H: int, pre_ln: bool, p_attn: float = 0.0, p_res: float = 0.0, seeds=(0, 0, 0), fused=None,
                     seg: Optional["RowSegments"] = None, ffn_act: int = 0, w_split: bool = False) -> None:
    """One frozen HuBERT encoder layer in ONE C-ABI call (sc_hubert_layer_fwd: QKV -> attention -> out_proj -> LN -> FC1 -> FC2 ->
    LN on the caller's stream).  ``w``: the encoder's weight dict (keys l{i}_*), ``pl``: its plan (scratch buffers).
    ``fused`` = (x_stats or None, x_ns, out_stats): the LayerNorm-free form (the LayerNorms folded into the GEMMs; ``out`` receives
    raw rows + statistics); x_stats None = ``x`` is an ordinary, materialised input (layer 0).  ``ffn_act``: FC1 activation, 0 erf-GELU,
    2 QuickGELU (the CLIP image tower's blocks, clip_image.py).  ``w_split``: the four GEMM weights in ``w`` are the [N, 2K] hi / lo
    interleaves of ``split_weight_bf16`` (evaluation; not with ``fused``)."""
    a = HubertLayerArgs()
    a.ffn_act = int(ffn_act)
    a.w_split = int(bool(w_split))
    a.x, a.out, a.valid_len = _p(x), _p(out), _p(valid_len)
    a.B, a.R, a.T, a.D, a.F, a.H, a.pre_ln = B, R, T, D, F_, H, int(pre_ln)
    a.qkv_w, a.o_w, a.fc1_w, a.fc2_w = _p(w[f"l{i}_qkv_w"]), _p(w[f"l{i}_o_w"]), _p(w[f"l{i}_fc1_w"]), _p(w[f"l{i}_fc2_w"])
    a.qkv_b, a.o_b, a.fc1_b, a.fc2_b = _p(w[f"l{i}_qkv_b"]), _p(w[f"l{i}_o_b"]), _p(w[f"l{i}_fc1_b"]), _p(w[f"l{i}_fc2_b"])
    a.ln1_g, a.ln1_b, a.ln2_g, a.ln2_b = _p(w[f"l{i}_ln1_g"]), _p(w[f"l{i}_ln1_b"]), _p(w[f"l{i}_ln2_g"]), _p(w[f"l{i}_ln2_b"])
    a.eps, a.p_attn, a.p_res = 1e-5, float(p_attn), float(p_res)
    a.seed_attn, a.seed_o, a.seed_fc2 = (int(s) & 0xffffffff for s in seeds)
    a.qk, a.vt, a.ctx, a.pre, a.x1, a.ffn = _p(pl.qk), _p(pl.vt), _p(pl.ctx), _p(pl.pre), _p(pl.x1), _p(pl.ffn)
    if seg is not None:
        a.seg = ctypes.pointer(seg.c)
        a.attn_work, a.n_attn_work = _p(seg.work), seg.n_work
    if fused is not None:
        x_stats, x_ns, out_stats = fused
        a.fused_ln = 1
        a.fc1_w, a.fc1_b, a.fc1_colsum = _p(w[f"l{i}_fc1_wf"]), _p(w[f"l{i}_fc1_cf"]), _p(w[f"l{i}_fc1_sf"])
        a.stats1, a.out_stats = _p(pl.stats1), _p(out_stats)
        if x_stats is not None:
            a.x_stats, a.x_ns = _p(x_stats), int(x_ns)
            a.x_ln_g, a.x_ln_b = _p(w[f"l{i - 1}_ln2_g"]), _p(w[f"l{i - 1}_ln2_b"])
            a.qkv_w, a.qkv_b, a.qkv_colsum = _p(w[f"l{i}_qkv_wf"]), _p(w[f"l{i}_qkv_cf"]), _p(w[f"l{i}_qkv_sf"])
    L = diag_lib() if fused is not None else lib()       # the LayerNorm-free form runs on the diagnostics library's GEMMs (opt-in)
    check(L.sc_hubert_layer_fwd(ctypes.byref(a), _stream()), "sc_hubert_layer_fwd", L)


ATTN_SLACK = DEFINES["SC_ATTN_SLACK"]     # 64: rows behind qk / elements behind vt that a 64-key attention tile may read past the last utterance


def hubert_layer_workspace(rows: int, D: int, F_: int, device):
    """The scratch of ``hubert_layer_fwd`` for ``rows`` rows as ONE allocation of sc_workspace_bytes(SC_WS_HUBERT_LAYER) bytes, laid out
    as the header documents it: qk [rows + 64, 2 D] | vt [rows D + 64] | ctx | pre | x1 [rows, D] | ffn [rows, F].  The 64 rows behind
    qk and the 64 elements behind vt are what the attention kernel reads past the last utterance: no kernel writes them, they are
    zeroed here, once (0 x NaN in the P.V product is NaN); everything else is left as the allocator hands it out - the layer writes
    it before it reads it.  -> namespace(qk, vt, ctx, pre, x1, ffn) of [rows, .] views for the ``pl`` argument."""
    from types import SimpleNamespace
    n = int(lib().sc_workspace_bytes(DEFINES["SC_WS_HUBERT_LAYER"], rows, D, F_)) // 2
    ws = torch.empty(n, device=device, dtype=torch.bfloat16)
    pl, off = {}, 0
    for name, cols, slack in (("qk", 2 * D, ATTN_SLACK * 2 * D), ("vt", D, ATTN_SLACK), ("ctx", D, 0), ("pre", D, 0), ("x1", D, 0), ("ffn", F_, 0)):
        pl[name] = ws[off: off + rows * cols].view(rows, cols)
        off += rows * cols
        if slack:
            ws[off: off + slack].zero_()
            off += slack
    assert off == n, (off, n)
    return SimpleNamespace(ws=ws, **pl)


def gemm_stats_strips(M: int, N: int) -> int:
    """Row-statistics strips a producer GEMM [M, N] writes (one per N-tile of the width the dispatcher picks)."""
    a = GemmArgs()
    a.M, a.N, a.K, a.n_split, a.nb1, a.nb2 = int(M), int(N), 64, -1, 1, 1
    return int(diag_lib().sc_gemm_stats_strips(ctypes.byref(a)))


def linear_bf16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, act: int = 0, out_f32: bool = False,
                alg_rows: Optional[int] = None, tile: int = 0, drop_p: float = 0.0, drop_seed: int = 0,
                aux: Optional[torch.Tensor] = None, aux_mode: int = 0, ln_colsum: Optional[torch.Tensor] = None, ln_eps: float = 0.0,
                a_rep: int = 0) -> torch.Tensor:
    """y[M, N] = epi(x[M, K] . w[N, K]^T) for contiguous 2-D operands.  ``aux`` / ``aux_mode`` (small problems, 128-row tiles):
    1 = also store the pre-activation into ``aux`` and return act(it); 2 = return (x . w^T) * act'(aux); 3 = the values of 1, nothing
    stored (``aux`` None).
    ``ln_colsum`` / ``ln_eps``: y = epi(LayerNorm(x) . w0^T) with the LayerNorm in the GEMM's prologue - ``w`` = w0 diag(gamma),
    ``ln_colsum[n]`` = sum_k w[n, k], ``bias[n]`` = sum_k beta[k] w0[n, k] + bias0[n] (``fold_layernorm``); K <= 1024.
    ``a_rep`` = 2: ``w`` is the [N, 2K] hi / lo interleave of ``split_weight_bf16``."""
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == (2 * K if a_rep == 2 else K) and x.stride(1) == 1 and w.stride(1) == 1
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    gemm_raw(x, x.stride(0), w, w.stride(0), out, out.stride(0), M, N, K, bias=bias, residual=residual,
             ldr=residual.stride(0) if residual is not None else 0, act=act, out_f32=out_f32, alg_rows=alg_rows, tile=tile,
             drop_p=drop_p, drop_seed=drop_seed, aux=aux, aux_mode=aux_mode, ln_colsum=ln_colsum, ln_eps=ln_eps, a_rep=a_rep)
    return out


SPLIT_BK = 64       # K-tile of the GEMM kernels: the granularity of the hi / lo interleave


def split_weight_bf16(w: torch.Tensor) -> torch.Tensor:
    """fp32 weight [..., N, K] (K % 64 == 0) -> the [..., N, 2K] bf16 operand of sc_gemm_args.a_rep = 2: W_hi = bf16(W),
    W_lo = bf16(W - W_hi), interleaved by 64-column K-tile [hi tile 0 | lo tile 0 | hi tile 1 | ...].  W_hi + W_lo is exact in fp32 and
    carries ~16 significant bits of W.  Plain torch, on whatever device ``w`` lives (run once per weight, on load)."""
    w = w.detach().float()
    K = w.shape[-1]
    assert K % SPLIT_BK == 0, f"split_weight_bf16: K={K} must be a multiple of {SPLIT_BK}"
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    lead = w.shape[:-1]
    both = torch.stack((hi.reshape(*lead, K // SPLIT_BK, SPLIT_BK), lo.reshape(*lead, K // SPLIT_BK, SPLIT_BK)), dim=-2)
    return both.reshape(*lead, 2 * K).contiguous()


def split_weight_sum(ws: torch.Tensor) -> torch.Tensor:
    """The fp32 weight W_hi + W_lo (exact) that a [..., N, 2K] interleave of ``split_weight_bf16`` stands for."""
    lead, K2 = ws.shape[:-1], ws.shape[-1]
    t = ws.float().reshape(*lead, K2 // (2 * SPLIT_BK), 2, SPLIT_BK)
    return (t[..., 0, :] + t[..., 1, :]).reshape(*lead, K2 // 2)


def fold_layernorm(w0: torch.Tensor, bias0: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """(w, ln_colsum, bias) for linear_bf16(..., ln_colsum=...): LayerNorm(x) w0^T + bias0 = rstd (x w^T - mean ln_colsum) + bias with
    w = bf16(w0 diag(gamma)), ln_colsum = the row sums of the bf16 values the kernel multiplies, bias = bias0 + w0 beta (fp32)."""
    w0f = w0.detach().float()
    w = (w0f * gamma.detach().float()[None, :]).to(torch.bfloat16).contiguous()
    colsum = w.float().sum(dim=1).contiguous()
    c = w0f @ beta.detach().float()
    if bias0 is not None:
        c = c + bias0.detach().float()
    return w, colsum, c.contiguous()


def attn_fwd(qk: torch.Tensor, vt: torch.Tensor, valid_len: torch.Tensor, out: torch.Tensor, B: int, R: int, H: int,
             D: int, scale: float, alg_flops: float = 0.0, lse2: Optional[torch.Tensor] = None, causal: bool = False,
             drop_p: float = 0.0, drop_seed: int = 0, seg: Optional["RowSegments"] = None, use_work: bool = True,
             gate: Optional[torch.Tensor] = None, table: Optional[torch.Tensor] = None) -> None:
    """``seg``: ragged rows (B / R are then ignored; vt = per utterance [H, 64, pitch] back to back, as gemm_raw(seg=...) writes it).
    ``gate`` [H, rows] / ``table`` [H, 2 Tmax - 1] fp32 (both or neither): WavLM's gated relative-position bias
    gate[h, i] * table[h, Tmax - 1 + j - i] on the scaled scores (``wavlm_gate`` writes the gate).  One entry point: sc_attn_fwd_bf16."""
    assert qk.dtype == torch.bfloat16 and vt.dtype == torch.bfloat16 and out.dtype == torch.bfloat16
    assert valid_len.dtype == torch.int32
    assert (gate is None) == (table is None), "attn_fwd: gate and table come together"
    if _timer is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    tmax = 0
    if gate is not None:
        rows = seg.rows if seg is not None else B * R
        assert gate.dtype == torch.float32 and gate.is_contiguous() and gate.shape == (H, rows), (gate.shape, H, rows)
        assert table.dtype == torch.float32 and table.is_contiguous() and table.dim() == 2 and table.shape[0] == H and table.shape[1] % 2 == 1
        tmax = (table.shape[1] + 1) // 2
    work, nwork = (seg.work, seg.n_work) if seg is not None and use_work else (None, 0)
    check(lib().sc_attn_fwd_bf16(_p(qk), qk.stride(0), _p(vt), _p(valid_len), _p(out), out.stride(0), _seg(seg), _p(work), nwork, B, R, H, D,
                                 float(scale), _p(gate), _p(table), tmax, _p(lse2), int(causal), float(drop_p), int(drop_seed) & 0xffffffff,
                                 _stream()), "sc_attn_fwd_bf16")
    if _timer is not None:
        ev1.record()
        _timer.add("attn_fwd_relbias" if gate is not None else "attn_fwd", ev0, ev1, float(alg_flops))


def wavlm_gate(x: torch.Tensor, wg: torch.Tensor, bg: torch.Tensor, const: torch.Tensor, H: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """WavLM's gate of the relative-position bias for every (head, row) of ``x`` [rows, >= H 64] bf16 -> ``out`` [H, rows] fp32:
    a (b const[h] - 1) + 2 with a, b = sigmoid of the two 4-sums of wg [8, 64] . x_head + bg [8] (sc_wavlm_gate_bf16)."""
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1 and x.shape[1] >= 64 * H
    for t, n in ((wg, 512), (bg, 8), (const, H)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, (t.shape, n)
    rows = x.shape[0]
    if out is None:
        out = torch.empty(H, rows, device=x.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (H, rows)
    check(lib().sc_wavlm_gate_bf16(_p(x), x.stride(0), _p(wg), _p(bg), _p(const), _p(out), rows, H, _stream()), "sc_wavlm_gate_bf16")
    return out


def head_transpose(x: torch.Tensor, B: int, R: int, H: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """xT[b, h, d, t] = x[b R + t, h 64 + d]; ``x`` may be a column slice of a wider row-major buffer."""
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    if out is None:
        out = torch.empty(B, H, 64, R, device=x.device, dtype=torch.bfloat16)
    check(lib().sc_head_transpose_bf16(_p(x), x.stride(0), _p(out), B, R, H, _stream()), "sc_head_transpose_bf16")
    return out


def attn32_fwd(qkv: torch.Tensor, heads: int, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Causal attention of 32-row sequences (sc_attn32_fwd_bf16): qkv [nseq 32, 3 heads 64] bf16 -> [nseq 32, heads 64]"""
    M, W3 = qkv.shape
    W = heads * 64
    assert qkv.dtype == torch.bfloat16 and qkv.stride(1) == 1 and W3 == 3 * W and M % 32 == 0
    if out is None:
        out = torch.empty(M, W, device=qkv.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.stride(1) == 1 and tuple(out.shape) == (M, W)
    check(lib().sc_attn32_fwd_bf16(_p(qkv), qkv.stride(0), _p(out), out.stride(0), M // 32, heads, float(scale), _stream()), "sc_attn32_fwd_bf16")
    return out


def attn32_bwd(qkv: torch.Tensor, dout: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """-> d qkv [nseq 32, 3 heads 64] bf16 (sc_attn32_bwd_bf16: from qkv and d out alone)"""
    M, W3 = qkv.shape
    W = heads * 64
    assert qkv.dtype == torch.bfloat16 and qkv.stride(1) == 1 and W3 == 3 * W and M % 32 == 0
    assert dout.dtype == torch.bfloat16 and dout.stride(1) == 1 and tuple(dout.shape) == (M, W)
    dqkv = torch.empty(M, 3 * W, device=qkv.device, dtype=torch.bfloat16)
    check(lib().sc_attn32_bwd_bf16(_p(qkv), qkv.stride(0), _p(dout), dout.stride(0), _p(dqkv), 3 * W, M // 32, heads, float(scale), _stream()),
          "sc_attn32_bwd_bf16")
    return dqkv


def attn_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse2: torch.Tensor,
             valid_len: torch.Tensor, dq: torch.Tensor, dk: torch.Tensor, dv: torch.Tensor, B: int, R: int, H: int, scale: float,
             causal: bool = False, kT: Optional[torch.Tensor] = None, q_rows: Optional[int] = None, drop_p: float = 0.0,
             drop_seed: int = 0) -> None:
    """q, k, v, out, dout, dq, dk, dv: [B R, H 64] views (column slices of wider buffers allowed); query rows t >= q_rows
    (default R) must carry dout = 0.  ``drop_p`` / ``drop_seed``: those of the forward (attn_fwd) when it dropped probabilities."""
    for t in (q, k, v, out, dout, dq, dk, dv):
        assert t.dtype == torch.bfloat16 and t.stride(1) == 1
    delta = torch.empty(B, H, R, device=q.device, dtype=torch.float32)
    args = lambda qT, kT, doT: (_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out), out.stride(0), _p(dout), dout.stride(0),
                                _p(qT), _p(kT), _p(doT), _p(lse2), _p(delta), _p(valid_len), _p(dq), dq.stride(0), _p(dk), dk.stride(0),
                                _p(dv), dv.stride(0), B, R, H, R if q_rows is None else q_rows, float(scale), int(causal), float(drop_p),
                                int(drop_seed) & 0xffffffff, _stream())
    if kT is None:          # the three per-head transposes and delta in one preparation launch inside the call
        T3 = torch.empty(3, B, H, 64, R, device=q.device, dtype=torch.bfloat16)
        check(lib().sc_attn_bwd_fused_bf16(*args(T3[0], T3[1], T3[2])), "sc_attn_bwd_fused_bf16")
        return
    qT = head_transpose(q, B, R, H)
    doT = head_transpose(dout, B, R, H)
    check(lib().sc_attn_bwd_bf16(*args(qT, kT, doT)), "sc_attn_bwd_bf16")


def layernorm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, eps: float, dres: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, want_param_grads: bool = False, acc=None, drop=None, sum_acc: Optional[torch.Tensor] = None):
    """dx = LN'(x)(dy) (+ dres) for bf16 rows; with ``want_param_grads`` also returns (dgamma, dbeta) fp32.
    ``acc`` = (dgamma_target, dbeta_target): the parameter gradients are ADDED to these fp32 [D] tensors by the reduction itself (no
    temporaries, no add launches); returns dx only.
    ``drop`` = (p, seed): also returns F.dropout(dx) with the stateless mask of element row * D + col (the residual branch's operand) -
    result (dx, dx_dropped); ``sum_acc`` fp32 [D]: the column sums of that dropped copy (of dx without ``drop``) are ADDED to it (the
    branch's bias gradient; needs ``acc`` / ``want_param_grads``).  One pass (sc_layernorm_bwd_drop_bf16)."""
    want_param_grads = want_param_grads or acc is not None
    rows, D = x.shape
    assert x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16 and gamma.dtype == torch.float32
    if out is None:
        out = torch.empty(rows, D, device=x.device, dtype=torch.bfloat16)
    dg = db = ds = None
    n_part = 0
    if want_param_grads:
        n_part = min(1024, (rows + 3) // 4)             # one partial row per workgroup (its four waves are added in LDS)
        dg = torch.empty(n_part, D, device=x.device, dtype=torch.float32)
        db = torch.empty(n_part, D, device=x.device, dtype=torch.float32)
    ext = drop is not None or sum_acc is not None
    out_drop = None
    if ext:
        p, seed = drop if drop is not None else (0.0, 0)
        if p > 0.0:
            out_drop = torch.empty(rows, D, device=x.device, dtype=torch.bfloat16)
        if sum_acc is not None:
            assert want_param_grads, "the column sums ride on the parameter-gradient partials"
            ds = torch.empty(n_part, D, device=x.device, dtype=torch.float32)
        check(lib().sc_layernorm_bwd_drop_bf16(_p(x), x.stride(0), _p(dy), dy.stride(0), _p(gamma), _p(dres), 0 if dres is None else dres.stride(0),
                                               _p(out), out.stride(0), rows, D, float(eps), _p(dg), _p(db), n_part, _p(out_drop),
                                               D if out_drop is not None else 0, float(p), int(seed) & 0xffffffff, _p(ds), _stream()),
              "sc_layernorm_bwd_drop_bf16")
        if sum_acc is not None:
            colsum(ds, D, n_part, D, sum_acc, beta=1.0)
        if out_drop is None:
            out_drop = out
    else:
        check(lib().sc_layernorm_bwd_bf16(_p(x), x.stride(0), _p(dy), dy.stride(0), _p(gamma), _p(dres), 0 if dres is None else dres.stride(0),
                                          _p(out), out.stride(0), rows, D, float(eps), _p(dg), _p(db), n_part, _stream()),
              "sc_layernorm_bwd_bf16")
    res = (out, out_drop) if drop is not None else out
    if not want_param_grads:
        return res
    if acc is not None:
        colsum(dg, D, n_part, D, acc[0], beta=1.0)
        colsum(db, D, n_part, D, acc[1], beta=1.0)
        return res
    g, b = torch.empty(D, device=x.device, dtype=torch.float32), torch.empty(D, device=x.device, dtype=torch.float32)
    colsum(dg, D, n_part, D, g)
    colsum(db, D, n_part, D, b)
    return (res, g, b) if drop is not None else (out, g, b)


def transpose_bf16(x: torch.Tensor, out: Optional[torch.Tensor] = None, colsum_partial: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[rows, cols] (row stride >= cols) -> contiguous [cols, rows]; rows and cols multiples of 8.  ``colsum_partial``
    ([ceil(rows / 64), cols] fp32) receives the per-64-row-block column sums of x (first stage of a bias gradient)."""
    rows, cols = x.shape
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    if out is None:
        out = torch.empty(cols, rows, device=x.device, dtype=torch.bfloat16)
    check(lib().sc_transpose_bf16(_p(x), x.stride(0), _p(out), out.stride(0), rows, cols, _p(colsum_partial), _stream()),
          "sc_transpose_bf16")
    return out


_cus = []


def _num_cus() -> int:
    if not _cus:
        _cus.append(int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count))
    return _cus[0]


_derived = {}


def derived(param: torch.Tensor, tag: str, fn):
    """``fn(param.detach())`` cached per parameter VERSION (bf16 working copies, transposed copies of trainable weights: computed once
    per optimiser step instead of once per call).  The key carries optim.param_generation() because the fused Adam kernel writes the
    masters through a raw pointer (no ``_version`` bump).  Entries hold only a weak reference to their parameter and die with it."""
    import weakref
    from .optim import param_generation
    if not isinstance(param, torch.nn.Parameter):       # a temporary: its id / address can be recycled for different contents
        return fn(param.detach())
    key = (id(param), tag)
    ver = (param.data_ptr(), param._version, param_generation(), tuple(param.shape))
    hit = _derived.get(key)
    if hit is not None and hit[0]() is param and hit[1] == ver:
        return hit[2]
    val = fn(param.detach())
    if len(_derived) > 512:                             # drop the entries of parameters that no longer exist
        for k in [k for k, v in _derived.items() if v[0]() is None]:
            del _derived[k]
    _derived[key] = (weakref.ref(param), ver, val)
    return val


def bf16_copy(t: torch.Tensor) -> torch.Tensor:
    """contiguous bf16 copy of ``t`` (any float dtype, any strides - a permuted / transposed / flipped view) in ONE copy kernel;
    ``t.to(bfloat16).contiguous()`` on a strided view is a cast launch plus a layout launch"""
    out = torch.empty(t.shape, dtype=torch.bfloat16, device=t.device)
    out.copy_(t.detach())
    return out


def weight_copies(w: torch.Tensor, want: str = "both"):
    """bf16 working copies of an fp32 [N, K] weight in ONE launch (sc_cast_transpose_f32_bf16): -> (bf16(w) [N, K], bf16(w)^T [K, N]);
    ``want`` "plain" / "T" / "both" (the entry not asked for is None).  Falls back to torch for shapes / dtypes the kernel does not take."""
    w = w.detach()
    N, K = w.shape
    if not (w.is_cuda and w.dtype == torch.float32 and w.stride(1) == 1 and w.stride(0) % 4 == 0 and N % 4 == 0 and K % 4 == 0 and w.data_ptr() % 16 == 0):
        wb = w.to(torch.bfloat16).contiguous()
        return (wb if want != "T" else None), (wb.t().contiguous() if want != "plain" else None)
    y = torch.empty(N, K, device=w.device, dtype=torch.bfloat16) if want != "T" else None
    yT = torch.empty(K, N, device=w.device, dtype=torch.bfloat16) if want != "plain" else None
    check(lib().sc_cast_transpose_f32_bf16(_p(w), w.stride(0), _p(y), K, _p(yT), N, N, K, _stream()), "sc_cast_transpose_f32_bf16")
    return y, yT


def derived_pair(param: torch.Tensor):
    """(bf16 copy, transposed bf16 copy) of a trainable 2-D weight, both cached per parameter version (``derived``) and produced by
    one launch when neither is cached."""
    pair = derived(param, "bf16_pair", lambda t: weight_copies(t, "both"))
    return pair


def len_mask(lens: torch.Tensor, n: int, add: int = 0) -> torch.Tensor:
    """bool [B, n]: True where k >= lens[b] + add (sc_len_mask_u8); the lengths ride along as ``._sc_lens`` = (lens, add) so that a
    consumer can rebuild the mask at another pitch, or read the lengths back, without a reduction over the mask"""
    assert lens.dtype == torch.int64 and lens.dim() == 1 and lens.is_contiguous()
    B = lens.shape[0]
    m = torch.empty(B, n, device=lens.device, dtype=torch.uint8)
    check(lib().sc_len_mask_u8(_p(lens), int(add), _p(m), B, int(n), _stream()), "sc_len_mask_u8")
    m = m.view(torch.bool)
    m._sc_lens = (lens, int(add))
    return m


_shared_streams = {}


def shared_stream(name: str, device=None, priority: int = 0) -> "torch.cuda.Stream":
    """ONE HIP stream per (role, device) and process.  The runtime multiplexes streams onto a handful of hardware queues; two streams
    that land on the same queue run one after the other.  Roles that are meant to run side by side ("encoder", "optimiser",
    "allreduce", "head_aux") therefore keep the streams they got first, instead of every model / trainer instance drawing new ones (the
    fourth model built in one process lost the encoder / tail overlap that way)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (name, idx)
    st = _shared_streams.get(key)
    if st is None:
        from . import warn_if_hw_queues_short
        warn_if_hw_queues_short()               # the first side stream of the process: say so once if the hardware queues cannot carry it
        # priority < 0: a high-priority stream gets a hardware queue of its own priority class - not one of the few normal-priority
        # queues the other roles share (the "h2d" copy stream: queued on the encoder's hardware queue, a batch's copy would start
        # only when the encoder in front of it has finished)
        st = _shared_streams[key] = torch.cuda.Stream(device=idx, priority=priority)
    return st


def grad_target(p):
    """``p.grad`` if a backward may ADD its result into it directly (the optimiser's flat gradient buffer: fp32, dense, p's shape) -
    the producing kernel's own reduction then accumulates (beta = 1) and the autograd node returns None for that input, which saves
    the temporary and the AccumulateGrad add launch per parameter.  None (p.grad unset / foreign): return the gradient as usual."""
    g = getattr(p, "grad", None)
    if g is None or not isinstance(p, torch.nn.Parameter) or not p.requires_grad:
        return None
    # ONLY the optimiser's own flat gradient buffer (optim.FlatAdam tags the views it hands out): adding into any other .grad would
    # bypass tensor / post-accumulate-grad hooks and write .grad under torch.autograd.grad, which must not touch it
    if not getattr(g, "_sc_flat", False):
        return None
    return g if (g.dtype == torch.float32 and g.is_contiguous() and g.shape == p.shape and g.device == p.device) else None


def invalidate_derived() -> None:
    """Forget every cached derived copy (after writing parameters through ``.data``, which bumps no version counter)."""
    _derived.clear()


def colsum_bf16(x: torch.Tensor, out: torch.Tensor, beta: float = 0.0) -> None:
    """out[c] = beta out[c] + sum_r x[r, c]  (bf16 rows -> fp32; bias gradients): row-block partials, then sc_colsum_f32 in block order."""
    rows, cols = x.shape
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1 and out.dtype == torch.float32
    nblk = max(1, min(512, rows // 64))
    part = torch.empty(nblk, cols, device=x.device, dtype=torch.float32)
    check(lib().sc_colsum_bf16(_p(x), x.stride(0), rows, cols, _p(part), nblk, _stream()), "sc_colsum_bf16")
    colsum(part, cols, nblk, cols, out, beta=beta)


def wgrad_bf16(dy: torch.Tensor, x: torch.Tensor, gW, gb: Optional[torch.Tensor] = None, beta: float = 1.0) -> None:
    """gW[N, K] = beta gW + dy[rows, N]^T x[rows, K]  (fp32, contiguous) ;  gb[N] = beta gb + colsum(dy).
    ``gW`` may be a LIST of fp32 contiguous tensors that together hold the N rows in order (q / k / v projection weights of one fused
    QKV product): the slice reduction writes each block straight into its tensor.

    The contraction runs over the rows.  N, K multiples of 256: the TN form of sc_gemm_bf16 reads both operands in place (row-major,
    any row stride - also the overlapping-row im2col view of a conv input), split along the rows into fp32 partials that
    sc_colsum_f32 adds in slice order.  Other shapes (grouped pos_conv: 48 columns): both operands are transposed first."""
    rows, N = dy.shape
    K = x.shape[1]
    blocks = None
    if isinstance(gW, (list, tuple)):
        blocks = list(gW)
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.shape[1] == K for t in blocks) and sum(t.shape[0] for t in blocks) == N
        gW = None
    else:
        assert gW.dtype == torch.float32 and gW.is_contiguous() and tuple(gW.shape) == (N, K)
    assert x.shape[0] == rows and rows % 64 == 0
    assert dy.stride(1) == 1 and x.stride(1) == 1
    tiles = ((N + 255) // 256) * ((K + 255) // 256)
    tn_ok = N % 256 == 0 and K % 256 == 0 and dy.stride(0) % 8 == 0 and x.stride(0) % 8 == 0
    if blocks is not None and not tn_ok:                     # generic shapes: one temporary, then block adds
        tmp = torch.empty(N, K, device=dy.device, dtype=torch.float32)
        wgrad_bf16(dy, x, tmp, None, beta=0.0)
        r = 0
        for t in blocks:
            if beta == 0.0:
                t.copy_(tmp[r: r + t.shape[0]])
            else:
                t.mul_(beta).add_(tmp[r: r + t.shape[0]])
            r += t.shape[0]
        if gb is not None:
            colsum_bf16(dy, gb, beta=beta)
        return
    if tn_ok:
        kt = rows // 64
        S = max(1, min(_num_cus() // tiles, kt // 4))     # one round of workgroups; slices of whole K-tiles, the last one shorter
        Kc = -(-kt // S) * 64
        S = -(-rows // Kc)
        part = gW if (S == 1 and beta == 0.0 and gW is not None) else torch.empty(S, N, K, device=dy.device, dtype=torch.float32)
        gemm_raw(dy, dy.stride(0), x, x.stride(0), part, K, N, K, Kc, out_f32=True, nb1=S, sA=(Kc * dy.stride(0), 0),
                 sW=(Kc * x.stride(0), 0), sC=(N * K, 0), tn=True, k_total=rows)
        if blocks is not None:
            r = 0
            for t in blocks:                                   # rows r .. r + n of every slice are one contiguous run of n K floats
                n = t.shape[0]
                colsum(part.view(S, N * K)[:, r * K:], N * K, S, n * K, t, beta=beta)
                r += n
        elif part is not gW:
            colsum(part, N * K, S, N * K, gW, beta=beta)
        if gb is not None:
            colsum_bf16(dy, gb, beta=beta)
        return
    pb = torch.empty((rows + 63) // 64, N, device=dy.device, dtype=torch.float32) if gb is not None else None
    S = max(1, min(256 // max(tiles, 1), rows // 512))
    # the slices must be equal and multiples of 64 rows: the transposed operands are laid out with the row count padded up to
    # 64 * S and the pad columns zeroed (rows = B * 499 has no useful divisor; one un-split GEMM over 32k rows would leave most
    # of the chip idle)
    rows_pad = -(-rows // (64 * S)) * (64 * S)
    dyT = torch.empty(N, rows_pad, device=dy.device, dtype=torch.bfloat16)
    xT = torch.empty(K, rows_pad, device=dy.device, dtype=torch.bfloat16)
    if rows_pad != rows:
        dyT[:, rows:].zero_()
        xT[:, rows:].zero_()
    transpose_bf16(dy, out=dyT, colsum_partial=pb)
    transpose_bf16(x, out=xT)
    Kc = rows_pad // S
    part = torch.empty(S, N, K, device=dy.device, dtype=torch.float32)
    gemm_raw(dyT, rows_pad, xT, rows_pad, part, K, N, K, Kc, out_f32=True, nb1=S, sA=(Kc, 0), sW=(Kc, 0), sC=(N * K, 0))
    colsum(part, N * K, S, N * K, gW, beta=beta)
    if gb is not None:                      # second stage of the bias gradient (first stage: the transpose of dy above)
        colsum(pb, N, pb.shape[0], N, gb, beta=beta)


def posconv_wgrad(du: torch.Tensor, xg: torch.Tensor, G: int, rows: int, Dg: int, Kp: int) -> torch.Tensor:
    """gw [G, Dg, Kp Dg] fp32 = the grouped pos_conv weight gradient (sc_posconv_wgrad_bf16): du / xg are [G, rows, Dg] slabs given by
    their first element (du advanced by the halo, see the header); row slices reduced in order by sc_colsum_f32."""
    assert du.dtype == torch.bfloat16 and xg.dtype == torch.bfloat16 and rows % 128 == 0
    Z = 4
    while (rows // 128) % Z:
        Z -= 1
    n = G * Dg * Kp * Dg
    part = torch.empty(Z, n, device=du.device, dtype=torch.float32)
    check(lib().sc_posconv_wgrad_bf16(_p(du), _p(xg), _p(part), G, rows, Dg, Kp, Z, _stream()), "sc_posconv_wgrad_bf16")
    if Z == 1:
        return part.view(G, Dg, Kp * Dg)
    gw = torch.empty(G, Dg, Kp * Dg, device=du.device, dtype=torch.float32)
    colsum(part, n, Z, n, gw)
    return gw


def dropout_bf16(x: torch.Tensor, p: float, seed: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.dropout(x, p) on bf16 rows with the stateless hash mask (element row * D + col); in place when out is x."""
    rows, D = x.shape
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    if out is None:
        out = torch.empty_like(x)
    check(lib().sc_dropout_bf16(_p(x), x.stride(0), _p(out), out.stride(0), rows, D, float(p), int(seed) & 0xffffffff, _stream()),
          "sc_dropout_bf16")
    return out


_mult_calls = [0]


def next_mult_seed() -> int:
    """Seed of the next fp32 dropout site: a function of torch's seed and a call counter (reproducible under torch.manual_seed, no
    device RNG state).  A site is either materialised (``dropout_mult``) or evaluated inside its consumer kernel (rt_* ops below) -
    the keep bit of element i is the same either way."""
    _mult_calls[0] += 1
    return ((torch.initial_seed() * 0x9E3779B1) ^ (_mult_calls[0] * 0x85EBCA6B)) & 0xffffffff


def dropout_mult(shape, p: float, device, seed: Optional[int] = None) -> torch.Tensor:
    """fp32 multiplier of F.dropout(., p) for a tensor of ``shape`` (numel a multiple of 8): keep ? 1 / (1 - p) : 0, one launch."""
    n = 1
    for d in shape:
        n *= int(d)
    out = torch.empty(n, device=device, dtype=torch.float32)
    if seed is None:
        seed = next_mult_seed()
    check(lib().sc_dropout_mult_f32(_p(out), n, float(p), seed, _stream()), "sc_dropout_mult_f32")
    return out.view(*shape)


def cif_fwd(x: torch.Tensor, alpha: torch.Tensor, csum: torch.Tensor, T: int, thr: float) -> torch.Tensor:
    """integrate-and-fire accumulation: x [B,S,C] fp32, alpha / csum [B,S] fp32 -> out [B,T+1,C] (see sc_cif_fwd)."""
    B, S, C = x.shape
    for t in (x, alpha, csum):
        assert t.dtype == torch.float32 and t.is_contiguous()
    out = torch.empty(B, T + 1, C, device=x.device, dtype=torch.float32)
    check(lib().sc_cif_fwd(_p(x), _p(alpha), _p(csum), _p(out), B, S, C, T, float(thr), _stream()), "sc_cif_fwd")
    return out


def cif_bwd(x: torch.Tensor, alpha: torch.Tensor, csum: torch.Tensor, g: torch.Tensor, T: int, thr: float):
    """-> (dx [B,S,C], pa, pb [nblk,B,S]): per-channel-block partials of d alpha (direct part) and d csum (sc_cif_prepare_bwd adds
    them up)."""
    B, S, C = x.shape
    assert g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == (B, T + 1, C)
    nblk = (C + 255) // 256
    dx = torch.empty_like(x)
    pa = torch.empty(nblk, B, S, device=x.device, dtype=torch.float32)
    pb = torch.empty(nblk, B, S, device=x.device, dtype=torch.float32)
    check(lib().sc_cif_bwd(_p(x), _p(alpha), _p(csum), _p(g), _p(dx), _p(pa), _p(pb), B, S, C, T, float(thr), _stream()), "sc_cif_bwd")
    return dx, pa, pb


def cif_prepare(alpha_raw: torch.Tensor, pad: torch.Tensor, target: Optional[torch.Tensor], apply_scaling: bool, thr: float, eps: float,
                max_feat: int, T: int, flags: torch.Tensor) -> dict:
    """CIF bookkeeping of one batch on the device (sc_cif_prepare): alpha_raw [B,S] fp32 (row stride free), pad [B,S] uint8 / bool."""
    B, S = alpha_raw.shape
    assert alpha_raw.dtype == torch.float32 and alpha_raw.stride(1) == 1 and pad.element_size() == 1 and pad.stride(1) == 1
    assert flags.dtype == torch.int32 and flags.numel() >= 8
    if target is not None:
        assert target.dtype == torch.int64 and target.is_contiguous() and target.numel() == B
    dev = alpha_raw.device
    f = lambda *sh: torch.empty(*sh, device=dev, dtype=torch.float32)
    r = dict(a_clip=f(B, S), alpha=f(B, S), csum=f(B, S), quantity=f(B), ratio=f(B),
             feat_len=torch.empty(B, device=dev, dtype=torch.int64), fired=torch.empty(B, S, device=dev, dtype=torch.uint8))
    check(lib().sc_cif_prepare(_p(alpha_raw), alpha_raw.stride(0), _p(pad), pad.stride(0), _p(target), int(bool(apply_scaling)), B, S,
                               float(thr), float(eps), int(max_feat), int(T), _p(r["a_clip"]), _p(r["alpha"]), _p(r["csum"]),
                               _p(r["quantity"]), _p(r["ratio"]), _p(r["feat_len"]), _p(r["fired"]), _p(flags), _stream()),
          "sc_cif_prepare")
    return r


def cif_prepare_bwd(pa: torch.Tensor, pb: torch.Tensor, a_clip: torch.Tensor, pad: torch.Tensor, ratio: torch.Tensor,
                    quantity: torch.Tensor, gq: Optional[torch.Tensor], scaled: bool) -> torch.Tensor:
    nblk, B, S = pa.shape
    da = torch.empty(B, S, device=pa.device, dtype=torch.float32)
    if gq is not None:
        assert gq.dtype == torch.float32 and gq.is_contiguous()
    check(lib().sc_cif_prepare_bwd(_p(pa), _p(pb), nblk, B, S, _p(a_clip), _p(pad), pad.stride(0), _p(ratio), _p(quantity), _p(gq),
                                   int(bool(scaled)), _p(da), _stream()), "sc_cif_prepare_bwd")
    return da


def cif_tail(alpha: torch.Tensor, csum: torch.Tensor, feat_len: torch.Tensor, out: torch.Tensor, T: int, thr: float, tail_thr: float,
             max_feat: int):
    """in place on ``feat_len`` and ``out`` [B,T+1,C]; returns (factor [B] fp32, extend [B] uint8)."""
    B, S = alpha.shape
    C = out.shape[2]
    assert tuple(out.shape) == (B, T + 1, C) and out.is_contiguous() and feat_len.dtype == torch.int64
    factor = torch.empty(B, device=alpha.device, dtype=torch.float32)
    extend = torch.empty(B, device=alpha.device, dtype=torch.uint8)
    check(lib().sc_cif_tail(_p(alpha), _p(csum), B, S, C, int(T), float(thr), float(tail_thr), int(max_feat), _p(feat_len), _p(out),
                            _p(factor), _p(extend), _stream()), "sc_cif_tail")
    return factor, extend


# ---- keyword -> sub-word vector quantiser (csrc/vq.hip) ---------------------------------------------------------------
def vq_prep(kw: torch.Tensor, eps: float = 1e-8):
    """kw [Nk, Et] fp32 -> (kwn_T [Et, Nkp] fp32 normalised + transposed, Nkp = roundup(Nk, 128); rnorm [Nk])."""
    Nk, Et = kw.shape
    assert kw.dtype == torch.float32 and kw.stride(1) == 1
    Nkp = (Nk + 127) // 128 * 128
    kwn_T = torch.empty(Et, Nkp, device=kw.device, dtype=torch.float32)
    rnorm = torch.empty(Nk, device=kw.device, dtype=torch.float32)
    check(lib().sc_vq_prep_f32(_p(kw), kw.stride(0), Nk, Et, float(eps), _p(kwn_T), Nkp, _p(rnorm), _stream()), "sc_vq_prep_f32")
    return kwn_T, rnorm


def split3_bf16(x: torch.Tensor, side: int, row_scale: Optional[torch.Tensor] = None, rows_pad: int = 128, cols_pad: int = 64,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [R, E] fp32 (* row_scale [R]) -> its three-way bf16 split as the six K-blocks of an fp32-accurate product on the bf16 matrix
    pipe (sc_split3_bf16): [Rp, 6 Ep] bf16, Rp / Ep = R / E rounded up to ``rows_pad`` / ``cols_pad``; side 0 and side 1 pair up.
    ``out``: a caller-owned [Rp, 6 Ep] bf16 buffer to write into (keyword_neighbors reuses one across chunks)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and side in (0, 1)
    R, E = x.shape
    Rp, Ep = -(-R // rows_pad) * rows_pad, -(-E // cols_pad) * cols_pad
    if out is None:
        out = torch.empty(Rp, 6 * Ep, device=x.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (Rp, 6 * Ep) and out.is_contiguous()
    check(lib().sc_split3_bf16(_p(x), x.stride(0), _p(row_scale), R, E, _p(out), Rp, Ep, side, _stream()), "sc_split3_bf16")
    return out


def cosine_scores_split(kw: torch.Tensor, rnorm: Optional[torch.Tensor], table_split: torch.Tensor, Vp: int,
                        out: Optional[torch.Tensor] = None, split_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cos [Nkp, Vp] fp32 = (kw * rnorm) . table_n^T to fp32 accuracy: ONE bf16 GEMM over the six K-blocks of the three-way splits
    (``table_split`` = split3_bf16(normalised table, side 1), rows padded to Vp).  ``out`` [Nkp, Vp] fp32 / ``split_out`` [Nkp, K6]
    bf16: caller-owned buffers for the scores and the split of ``kw`` (none allocated here then)."""
    A = split3_bf16(kw, 0, row_scale=rnorm, out=split_out)
    K6 = A.shape[1]
    assert table_split.shape == (Vp, K6), (table_split.shape, Vp, K6)
    cos = torch.empty(A.shape[0], Vp, device=kw.device, dtype=torch.float32) if out is None else out
    assert cos.dtype == torch.float32 and tuple(cos.shape) == (A.shape[0], Vp) and cos.is_contiguous()
    gemm_raw(A, K6, table_split, K6, cos, Vp, A.shape[0], Vp, K6, out_f32=True)
    return cos


def sgemm_mfma(A: torch.Tensor, Bm: torch.Tensor, a_kmajor: bool = False, b_kmajor: bool = False, bias: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C [M, N] = A . B^T (+ bias) in exact fp32 on the matrix pipe.  A: [M, K] (or [K, M] with a_kmajor), B: [N, K] (nn.Linear
    layout; or [K, N] with b_kmajor); any M, N, K."""
    assert A.dtype == torch.float32 and Bm.dtype == torch.float32
    assert (A.stride(1) == 1 or A.shape[1] == 1) and (Bm.stride(1) == 1 or Bm.shape[1] == 1)
    K, M = A.shape if a_kmajor else A.shape[::-1]
    K2, N = Bm.shape if b_kmajor else Bm.shape[::-1]
    assert K == K2, (A.shape, Bm.shape)
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.stride(1) == 1
    if _timer is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    S = int(lib().sc_sgemm_mfma_slices(M, N, K))          # few output tiles x long K: slices of the contraction, added in order
    if S > 1:
        part = torch.empty(S, M, N, device=A.device, dtype=torch.float32)
        check(lib().sc_sgemm_mfma_f32_split(_p(A), A.stride(0), int(a_kmajor), _p(Bm), Bm.stride(0), int(b_kmajor), _p(out), out.stride(0),
                                            M, N, K, _p(bias), _p(part), S, _stream()), "sc_sgemm_mfma_f32_split")
    else:
        check(lib().sc_sgemm_mfma_f32(_p(A), A.stride(0), int(a_kmajor), _p(Bm), Bm.stride(0), int(b_kmajor), _p(out), out.stride(0), M, N, K,
                                      _p(bias), _stream()), "sc_sgemm_mfma_f32")
    if _timer is not None:
        ev1.record()
        _timer.add("sgemm_mfma_f32", ev0, ev1, 2.0 * M * N * K)
    return out


def _lists_out(rows: int, k: int, dev, vals: Optional[torch.Tensor], idx: Optional[torch.Tensor]):
    """the output pair of a selection entry, (vals [rows, k] fp32, idx [rows, k] int32): allocated on ``dev`` where None, the caller's
    own (contiguous) checked otherwise"""
    if vals is None:
        vals = torch.empty(rows, k, device=dev, dtype=torch.float32)
    if idx is None:
        idx = torch.empty(rows, k, device=dev, dtype=torch.int32)
    assert vals.dtype == torch.float32 and idx.dtype == torch.int32 and vals.is_contiguous() and idx.is_contiguous()
    assert tuple(vals.shape) == (rows, k) and tuple(idx.shape) == (rows, k)
    return vals, idx


def topk_rows(scores: torch.Tensor, V: int, k: int, vals: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None):
    """scores [rows, >= V] fp32 (unit column stride, any row pitch and base alignment) -> (vals [rows, k] fp32, idx [rows, k] int32): the
    k largest of the first V columns of every row, best first - ties to the lower column, NaN above every number, -inf / -1 behind
    the V-th entry when V < k (sc_topk_rows_f32, csrc/topk.hip).  ``vals`` / ``idx``: caller-owned contiguous outputs."""
    assert scores.dtype == torch.float32 and scores.dim() == 2 and (scores.stride(1) == 1 or scores.shape[1] == 1)
    rows = scores.shape[0]
    assert scores.shape[1] >= V, (scores.shape, V)
    ld = scores.stride(0) if rows > 1 else max(V, 1)
    vals, idx = _lists_out(rows, k, scores.device, vals, idx)
    check(lib().sc_topk_rows_f32(_p(scores) if rows else ctypes.c_void_p(0), ld, rows, V, k, _p(vals) if rows else ctypes.c_void_p(0),
                                 _p(idx) if rows else ctypes.c_void_p(0), _stream()), "sc_topk_rows_f32")
    return vals, idx


def search_slabs(nQ: int, N: int, k: int) -> int:
    """Slabs the gallery axis of ``search_topk`` is cut into for (nQ, N, k) (sc_search_slabs)."""
    return int(lib().sc_search_slabs(int(nQ), int(N), int(k)))


def search_topk(q_split: torch.Tensor, g_split: torch.Tensor, nQ: int, N: int, k: int, slabs: Optional[int] = None,
                vals: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None):
    """The k best of N gallery rows for each of nQ queries, selection fused into the score GEMM (sc_search_topk_bf16, csrc/search.hip):
    ``q_split`` = split3_bf16(queries, 0) [>= roundup(nQ, 128), 6 Ep], ``g_split`` = split3_bf16(gallery, 1) [>= roundup(N, 128), 6 Ep]
    -> (vals [nQ, k] fp32, idx [nQ, k] int32), best first in ``topk_rows``' order (ties to the lower gallery row, NaN first, -inf / -1
    behind the N-th entry).  The scores are those of ``cosine_scores_split``; no [nQ, N] matrix is written.  ``slabs``: how many slabs
    the gallery axis is cut into (None: sc_search_slabs); the result does not depend on it.  More than one slab: the per-slab lists
    [nQ, S, k] are merged by ``topk_rows`` and one gather.  ``vals`` / ``idx``: caller-owned contiguous outputs."""
    return _search_lists("search_topk", q_split, g_split, nQ, N, k, slabs, vals, idx)


def _search_operands(name: str, q: torch.Tensor, g: torch.Tensor, nQ: int, N: int) -> int:
    """the bf16 operand pair of the scan ``name`` (``search_topk`` / ``search_coarse`` and their filtered forms), checked: contiguous
    [>= roundup(nQ, 128), K] / [>= roundup(N, 128), K] on the device -> K"""
    if not (q.is_cuda and g.is_cuda):
        raise RuntimeError(f"{name} runs on the HIP kernels: no CPU path")
    assert q.dtype == torch.bfloat16 and g.dtype == torch.bfloat16 and q.dim() == 2 and g.dim() == 2
    assert q.is_contiguous() and g.is_contiguous()
    K = q.shape[1]
    assert g.shape[1] == K, (q.shape, g.shape)
    assert q.shape[0] >= -(-nQ // 128) * 128 and g.shape[0] >= -(-N // 128) * 128, (q.shape, nQ, g.shape, N)
    return K


def _search_lists(name: str, q: torch.Tensor, g: torch.Tensor, nQ: int, N: int, k: int, slabs: Optional[int], vals, idx):
    """``search_topk`` / ``search_coarse`` (``name``; the C entry is sc_<name>_bf16): the per-slab lists [nQ, S, k], merged by ``topk_rows``
    and one gather when S > 1"""
    nQ, N, k = int(nQ), int(N), int(k)
    K = _search_operands(name, q, g, nQ, N)
    dev = q.device
    vals, idx = _lists_out(nQ, k, dev, vals, idx)
    S = search_slabs(nQ, N, k) if slabs is None else int(slabs)
    if S == 1 or nQ == 0:
        pv, pi = vals, idx
    else:
        pv = torch.empty(nQ, S * k, device=dev, dtype=torch.float32)
        pi = torch.empty(nQ, S * k, device=dev, dtype=torch.int32)
    null, entry = ctypes.c_void_p(0), f"sc_{name}_bf16"
    check(getattr(lib(), entry)(_p(q) if nQ else null, _p(g) if N else null, nQ, N, K, k, S, _p(pv) if nQ else null, _p(pi) if nQ else null,
                                _stream()), entry)
    if pv is not vals:
        _, pos = topk_rows(pv, S * k, k, vals=vals)
        torch.gather(pi, 1, pos.long(), out=idx)
    return vals, idx


def _search_words(name: str, q: torch.Tensor, g: torch.Tensor, nQ: int, N: int, k: int, q_ids, g_ids, live, slabs: Optional[int],
                  merge: bool, vals=None, idx=None):
    """``search_topk_filtered`` / ``search_coarse_filtered`` (``name``; the C entry is sc_<name>_bf16): the per-slab list words
    part [nQ, max(S, 1), k] int64 -> ``merge``: ``search_merge``'s lists of them in ``vals`` / ``idx`` (checked before the launch), else part"""
    nQ, N, k = int(nQ), int(N), int(k)
    K = _search_operands(name, q, g, nQ, N)
    dev = q.device
    q_ids, g_ids, live = filter_operands(name, nQ, N, q_ids, g_ids, live, dev)
    if merge:
        vals, idx = _lists_out(nQ, k, dev, vals, idx)
    S = search_slabs(nQ, N, k) if slabs is None else int(slabs)
    part = torch.empty(nQ, max(S, 1), k, device=dev, dtype=torch.int64)
    null, entry = ctypes.c_void_p(0), f"sc_{name}_bf16"
    check(getattr(lib(), entry)(_p(q) if nQ else null, _p(g) if N else null, nQ, N, K, k, S, _p(q_ids) if nQ and N else null,
                                _p(g_ids) if nQ and N else null, _p(live) if N else null, _p(part) if nQ else null, _stream()), entry)
    return search_merge(part, k, vals=vals, idx=idx) if merge else part


def check_filter_tensor(name: str, what: str, t, n: int, dtypes=(torch.int64,)) -> None:
    """``t`` as a filter operand ``what`` of ``name``: a contiguous tensor [n] of one of ``dtypes`` (where it lives: ``filter_operands``)"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: {what} must be a tensor")
    if t.dtype not in dtypes:
        raise ValueError(f"{name}: {what} must be {' or '.join(str(d) for d in dtypes)}, not {t.dtype}")
    if t.dim() != 1 or t.numel() != n:
        raise ValueError(f"{name}: {what} has shape {tuple(t.shape)}, expected ({n},)")
    if not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be contiguous")


def filter_operands(name: str, nQ: int, N: int, q_ids, g_ids, live, dev, names=("q_ids", "g_ids", "live")):
    """The filter operands of the filtered entries, checked before any launch: ``q_ids`` [nQ] / ``g_ids`` [N] int64 (both or neither),
    ``live`` [N] bool or uint8, all contiguous and on the device ``dev`` (None: any one device is taken).  Format errors are reported
    before device errors.  -> (q_ids, g_ids, live as uint8), each a tensor or None.  ``names``: what the caller calls them."""
    if (q_ids is None) != (g_ids is None):
        raise ValueError(f"{name}: ids on one side only - give {names[0]} and {names[1]}, or neither")
    given = [(what, t, n, dtypes) for what, t, n, dtypes in ((names[0], q_ids, nQ, (torch.int64,)), (names[1], g_ids, N, (torch.int64,)),
                                                             (names[2], live, N, (torch.bool, torch.uint8))) if t is not None]
    for what, t, n, dtypes in given:
        check_filter_tensor(name, what, t, n, dtypes)
    for what, t, _, _ in given:
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on the HIP kernels: device tensors only ({what})")
        if dev is not None and t.device != dev:
            raise ValueError(f"{name}: {what} is on {t.device}, the operands on {dev}")
    if live is not None and live.dtype == torch.bool:
        live = live.view(torch.uint8)                     # the same bytes: True is 1
    return q_ids, g_ids, live


def topk_rows_filtered(scores: torch.Tensor, V: int, k: int, q_ids: Optional[torch.Tensor] = None, g_ids: Optional[torch.Tensor] = None,
                       live: Optional[torch.Tensor] = None, vals: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None):
    """``topk_rows`` over the admissible columns only (sc_topk_rows_filtered_f32, csrc/search_filter.hip): column j is admissible for
    row i iff j < V, ``live`` is None or live[j] != 0, and the ids are None or g_ids[j] != q_ids[i] (``q_ids`` [rows] / ``g_ids`` [V]
    int64, both or neither; ``live`` [V] bool or uint8).  -> (vals [rows, k] fp32, idx [rows, k] int32), ``topk_rows``' order over the
    admissible columns, -inf / -1 behind the last of them; an admissible -inf keeps its column.  ``scores`` is not modified."""
    if not scores.is_cuda:
        raise RuntimeError("topk_rows_filtered runs on the HIP kernels: no CPU path")
    assert scores.dtype == torch.float32 and scores.dim() == 2 and (scores.stride(1) == 1 or scores.shape[1] == 1)
    rows, V, k = scores.shape[0], int(V), int(k)
    assert scores.shape[1] >= V, (scores.shape, V)
    q_ids, g_ids, live = filter_operands("topk_rows_filtered", rows, V, q_ids, g_ids, live, scores.device)
    ld = scores.stride(0) if rows > 1 else max(V, 1)
    vals, idx = _lists_out(rows, k, scores.device, vals, idx)
    null = ctypes.c_void_p(0)
    check(lib().sc_topk_rows_filtered_f32(_p(scores) if rows else null, ld, rows, V, k, _p(q_ids), _p(g_ids), _p(live),
                                          _p(vals) if rows else null, _p(idx) if rows else null, _stream()), "sc_topk_rows_filtered_f32")
    return vals, idx


def topk_rows_wide(scores: torch.Tensor, V: int, k: int, *, q_ids: Optional[torch.Tensor] = None, g_ids: Optional[torch.Tensor] = None,
                   live: Optional[torch.Tensor] = None, vals: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None):
    """``topk_rows`` / ``topk_rows_filtered`` for k up to 1024 (sc_topk_rows_wide_f32, csrc/topk_wide.hip; meant for 33 <= k <= 1024,
    1 <= k accepted): scores [rows, >= V] fp32 (unit column stride, any row pitch and base alignment) -> (vals [rows, k] fp32, idx
    [rows, k] int32), the k best eligible columns of every row, best first in ``topk_rows``' order - larger value first, ties to the
    lower column (-0 == +0), NaN above every number, -inf / -1 behind the last eligible column; vals are the matrix's own bits.
    Column j is eligible for row i iff j < V, ``live`` is None or live[j] != 0, and the ids are None or g_ids[j] != q_ids[i]
    (``q_ids`` [rows] / ``g_ids`` [V] int64, both or neither; ``live`` [V] bool or uint8); an eligible -inf keeps its column.
    ``scores`` is not modified.  ``vals`` / ``idx``: caller-owned contiguous outputs."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2:
        raise ValueError("topk_rows_wide: scores must be a [rows, >= V] tensor")
    if not scores.is_cuda:
        raise RuntimeError("topk_rows_wide runs on the HIP kernels: no CPU path")
    if scores.dtype != torch.float32:
        raise ValueError(f"topk_rows_wide: scores must be torch.float32, not {scores.dtype}")
    rows, V, k = scores.shape[0], int(V), int(k)
    if not (scores.stride(1) == 1 or scores.shape[1] == 1):
        raise ValueError("topk_rows_wide: scores must have unit column stride")
    if not 1 <= V <= scores.shape[1]:
        raise ValueError(f"topk_rows_wide: scores has shape {tuple(scores.shape)}, expected at least ({rows}, {V}) with V >= 1")
    if not 1 <= k <= 1024:
        raise RuntimeError(f"topk_rows_wide: 1 <= k <= 1024 (k {k})")
    q_ids, g_ids, live = filter_operands("topk_rows_wide", rows, V, q_ids, g_ids, live, scores.device)
    ld = scores.stride(0) if rows > 1 else max(V, 1)
    if vals is None:
        vals = torch.empty(rows, k, device=scores.device, dtype=torch.float32)
    if idx is None:
        idx = torch.empty(rows, k, device=scores.device, dtype=torch.int32)
    for what, t, dtype in (("vals", vals, torch.float32), ("idx", idx, torch.int32)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"topk_rows_wide: {what} must be a tensor")
        if t.dtype != dtype:
            raise ValueError(f"topk_rows_wide: {what} must be {dtype}, not {t.dtype}")
        if tuple(t.shape) != (rows, k):
            raise ValueError(f"topk_rows_wide: {what} has shape {tuple(t.shape)}, expected ({rows}, {k})")
        if not t.is_contiguous():
            raise ValueError(f"topk_rows_wide: {what} must be contiguous")
        if t.device != scores.device:
            raise ValueError(f"topk_rows_wide: {what} is on {t.device}, the operands on {scores.device}")
    null = ctypes.c_void_p(0)
    check(lib().sc_topk_rows_wide_f32(_p(scores) if rows else null, ld, rows, V, k, _p(q_ids), _p(g_ids), _p(live),
                                      _p(vals) if rows else null, _p(idx) if rows else null, _stream()), "sc_topk_rows_wide_f32")
    return vals, idx


def search_merge(part: torch.Tensor, k: int, vals: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None):
    """part [nQ, S, k] int64 - the per-slab list words ``search_topk_filtered``'s kernel writes (key << 32 | ~row, best first, 0 = no
    entry) -> (vals [nQ, k] fp32, idx [nQ, k] int32): per query the k largest words, decoded; -inf / -1 where a query has fewer than
    k entries (sc_search_merge_u64).  A real -inf is an entry and ranks ahead of every filler, whichever slab holds it."""
    if not part.is_cuda:
        raise RuntimeError("search_merge runs on the HIP kernels: no CPU path")
    assert part.dtype == torch.int64 and part.dim() == 3 and part.is_contiguous() and part.shape[2] == int(k), (part.dtype, part.shape, k)
    nQ, S, k = part.shape[0], part.shape[1], int(k)
    vals, idx = _lists_out(nQ, k, part.device, vals, idx)
    null = ctypes.c_void_p(0)
    check(lib().sc_search_merge_u64(_p(part) if nQ else null, nQ, S, k, _p(vals) if nQ else null, _p(idx) if nQ else null, _stream()),
          "sc_search_merge_u64")
    return vals, idx


def search_merge_lists(part_vals: torch.Tensor, part_idx: torch.Tensor, row0: torch.Tensor, k: int, *, vals: Optional[torch.Tensor] = None,
                       idx: Optional[torch.Tensor] = None):
    """part_vals [S, nQ, k] fp32 / part_idx [S, nQ, k] int32 - per shard s of a gallery the list ``search`` returns for it (best first, a
    row of the shard, -1 = no entry) -, row0 [S] int64 on the device = the global row of every shard's row 0 -> (vals [nQ, k] fp32,
    idx [nQ, k] int32 global rows): per query the k best entries over all S lists under the order contract on GLOBAL rows, the values'
    own 32 bits kept, -inf / -1 behind the last entry (sc_search_merge_lists_f32, csrc/search_merge_wide.hip).  1 <= k <= 1024.  The
    shard stride is taken from the tensors: both must have the strides (>= nQ k, k, 1), so ``buf[:, q0:q1]`` of a [S, nQall, k] buffer
    merges without a copy.  ``vals`` / ``idx``: caller-owned contiguous outputs."""
    k = int(k)
    for what, t, dtype in (("part_vals", part_vals, torch.float32), ("part_idx", part_idx, torch.int32), ("row0", row0, torch.int64)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"search_merge_lists: {what} must be a tensor")
        if t.dtype != dtype:
            raise ValueError(f"search_merge_lists: {what} must be {dtype}, not {t.dtype}")
    if part_vals.dim() != 3 or part_vals.shape[2] != k or part_idx.shape != part_vals.shape:
        raise ValueError(f"search_merge_lists: part_vals {tuple(part_vals.shape)} / part_idx {tuple(part_idx.shape)} must both be [S, nQ, {k}]")
    S, nQ = part_vals.shape[0], part_vals.shape[1]
    if not 1 <= k <= 1024 or S < 1:
        raise ValueError(f"search_merge_lists: 1 <= k <= 1024 and S >= 1 (k {k}, S {S})")
    if row0.dim() != 1 or row0.numel() != S or not row0.is_contiguous():
        raise ValueError(f"search_merge_lists: row0 has shape {tuple(row0.shape)}, expected a contiguous ({S},)")
    stride = nQ * k
    if nQ > 0:
        for what, t in (("part_vals", part_vals), ("part_idx", part_idx)):
            if t.stride(2) != 1 or (nQ > 1 and t.stride(1) != k) or (S > 1 and t.stride(0) < nQ * k):
                raise ValueError(f"search_merge_lists: {what} has strides {t.stride()}, expected (>= {nQ * k}, {k}, 1)")
        if S > 1:
            stride = part_vals.stride(0)
            if part_idx.stride(0) != stride:
                raise ValueError(f"search_merge_lists: part_vals and part_idx differ in their shard stride ({stride}, {part_idx.stride(0)})")
    if not (part_vals.is_cuda and part_idx.is_cuda and row0.is_cuda):
        raise RuntimeError("search_merge_lists runs on the HIP kernels: no CPU path")
    vals, idx = _lists_out(nQ, k, part_vals.device, vals, idx)
    null = ctypes.c_void_p(0)
    check(lib().sc_search_merge_lists_f32(_p(part_vals) if nQ else null, _p(part_idx) if nQ else null, stride, _p(row0), nQ, S, k,
                                          _p(vals) if nQ else null, _p(idx) if nQ else null, _stream()), "sc_search_merge_lists_f32")
    return vals, idx


def search_topk_filtered(q_split: torch.Tensor, g_split: torch.Tensor, nQ: int, N: int, k: int, q_ids: Optional[torch.Tensor] = None,
                         g_ids: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None, slabs: Optional[int] = None,
                         vals: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None):
    """``search_topk`` over the admissible gallery rows only (sc_search_topk_filtered_bf16 + sc_search_merge_u64,
    csrc/search_filter.hip): gallery row j is admissible for query i iff j < N, ``live`` is None or live[j] != 0, and the ids are None
    or g_ids[j] != q_ids[i] (``q_ids`` [nQ] / ``g_ids`` [N] int64, both or neither, all 64 bits compared; ``live`` [N] bool or uint8).
    Operands, scores and order are ``search_topk``'s; an inadmissible row never appears, -inf / -1 stand behind the last admissible
    row, and an admissible row scoring a real -inf ranks ahead of them.  ``slabs``: None = sc_search_slabs; any S >= 1 is legal here
    (a slab may hold no admissible row at all) and the result does not depend on it.  The per-slab lists [nQ, S, k] are 64-bit
    words, merged and decoded by ``search_merge``.  ``vals`` / ``idx``: caller-owned contiguous outputs."""
    return _search_words("search_topk_filtered", q_split, g_split, nQ, N, k, q_ids, g_ids, live, slabs, True, vals, idx)


def rows_bf16(x: torch.Tensor, row_scale: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """x [R, E] fp32 (* row_scale [R]) -> (out [Rp, Ep] bf16, norms [3, R] fp32), Rp / Ep = R / E rounded up to 128 / 64
    (sc_rows_bf16, csrc/search_compact.hip): the rows rounded to bf16 (nearest even), zero outside [R, E], and per row the 2-norms of
    the scaled row, of its bf16 image and of their difference, each accumulated in fp64.  ``out``: a caller-owned [Rp, Ep] bf16 buffer."""
    if not x.is_cuda:
        raise RuntimeError("rows_bf16 runs on the HIP kernels: no CPU path")
    assert x.dtype == torch.float32 and x.dim() == 2 and (x.stride(1) == 1 or x.shape[1] == 1)
    R, E = x.shape
    Rp, Ep = -(-R // 128) * 128, -(-E // 64) * 64
    if out is None:
        out = torch.empty(Rp, Ep, device=x.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (Rp, Ep) and out.is_contiguous()
    norms = torch.empty(3, R, device=x.device, dtype=torch.float32)
    if row_scale is not None:
        assert row_scale.dtype == torch.float32 and tuple(row_scale.shape) == (R,) and row_scale.is_contiguous()
    if R:
        check(lib().sc_rows_bf16(_p(x), x.stride(0) if R > 1 else E, _p(row_scale), R, E, _p(out), Rp, Ep, _p(norms), _stream()), "sc_rows_bf16")
    return out, norms


def search_coarse(q_bf16: torch.Tensor, g_bf16: torch.Tensor, nQ: int, N: int, D: int, slabs: Optional[int] = None,
                  vals: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None):
    """The D best of N gallery rows for each of nQ queries by their bf16 x bf16 scores (sc_search_coarse_bf16, csrc/search_compact.hip):
    ``q_bf16`` = rows_bf16(queries) [>= roundup(nQ, 128), Ep], ``g_bf16`` = rows_bf16(gallery) [>= roundup(N, 128), Ep] ->
    (vals [nQ, D] fp32, idx [nQ, D] int32), best first in ``topk_rows``' order (ties to the lower gallery row, NaN first, -inf / -1
    behind the N-th entry).  ``slabs``: None = sc_search_slabs(nQ, N, D); the result does not depend on it.  More than one slab: the
    per-slab lists [nQ, S, D] are merged by ``topk_rows`` and one gather, as ``search_topk`` merges them."""
    return _search_lists("search_coarse", q_bf16, g_bf16, nQ, N, D, slabs, vals, idx)


def search_rerank(q: torch.Tensor, q_scale: Optional[torch.Tensor], rows: torch.Tensor, g_scale: Optional[torch.Tensor],
                  cand_idx: torch.Tensor, cand_vals: torch.Tensor, eps: torch.Tensor, k: int, vals: Optional[torch.Tensor] = None,
                  idx: Optional[torch.Tensor] = None, certified: Optional[torch.Tensor] = None):
    """Exact re-rank of coarse candidates (sc_search_rerank_f32, csrc/search_compact.hip): ``q`` [nQ, E] / ``rows`` [N, E] fp32 (unit
    column stride, any pitch), ``q_scale`` [nQ] / ``g_scale`` [N] or None, ``cand_idx`` / ``cand_vals`` [nQ, D] int32 / fp32 (best
    first, -1 = no candidate), ``eps`` [nQ] fp32 -> (vals [nQ, k] fp32, idx [nQ, k] int32, certified [nQ] uint8): the k best
    candidates by their inner product accumulated in fp64 (rows scaled in fp32 first), and 1 where no row outside the candidates can
    belong to the list: every value finite and (N <= D or e_k - |e_k| 2^-23 > cand_vals[:, D - 1] + eps)."""
    return _search_rerank("search_rerank", q, q_scale, rows, g_scale, cand_idx, cand_vals, eps, k, vals, idx, certified)


def _search_rerank(name: str, q, q_scale, rows, g_scale, cand_idx, cand_vals, eps, k: int, vals, idx, certified):
    """``search_rerank`` / ``search_rerank_filtered`` (``name``; the C entry is sc_<name>_f32): the same operands, checks and outputs"""
    if not (q.is_cuda and rows.is_cuda and cand_idx.is_cuda):
        raise RuntimeError(f"{name} runs on the HIP kernels: no CPU path")
    assert q.dtype == torch.float32 and rows.dtype == torch.float32 and q.dim() == 2 and rows.dim() == 2
    assert (q.stride(1) == 1 or q.shape[1] == 1) and (rows.stride(1) == 1 or rows.shape[1] == 1)
    nQ, E = q.shape
    N = rows.shape[0]
    assert rows.shape[1] == E, (q.shape, rows.shape)
    D, k = int(cand_idx.shape[1]), int(k)
    assert cand_idx.dtype == torch.int32 and cand_vals.dtype == torch.float32 and cand_idx.is_contiguous() and cand_vals.is_contiguous()
    assert tuple(cand_idx.shape) == (nQ, D) and tuple(cand_vals.shape) == (nQ, D) and 1 <= k <= D <= 32, (cand_idx.shape, cand_vals.shape, k)
    assert eps.dtype == torch.float32 and tuple(eps.shape) == (nQ,) and eps.is_contiguous()
    for s, n in ((q_scale, nQ), (g_scale, N)):
        assert s is None or (s.dtype == torch.float32 and tuple(s.shape) == (n,) and s.is_contiguous())
    vals, idx = _lists_out(nQ, k, q.device, vals, idx)
    if certified is None:
        certified = torch.empty(nQ, device=q.device, dtype=torch.uint8)
    assert certified.dtype == torch.uint8 and certified.is_contiguous() and tuple(certified.shape) == (nQ,)
    if nQ:
        entry = f"sc_{name}_f32"
        check(getattr(lib(), entry)(_p(q), q.stride(0) if nQ > 1 else E, _p(q_scale), _p(rows) if N else ctypes.c_void_p(0),
                                    rows.stride(0) if N > 1 else E, _p(g_scale), _p(cand_idx), _p(cand_vals), _p(eps), nQ, N, E, D, k,
                                    _p(vals), _p(idx), _p(certified), _stream()), entry)
    return vals, idx, certified


def search_coarse_filtered(q_bf16: torch.Tensor, g_bf16: torch.Tensor, nQ: int, N: int, D: int, q_ids: Optional[torch.Tensor] = None,
                           g_ids: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None, slabs: Optional[int] = None):
    """``search_coarse`` over the admissible gallery rows only (sc_search_coarse_filtered_bf16, csrc/search_compact_filter.hip):
    gallery row j is admissible for query i iff j < N, ``live`` is None or live[j] != 0, and the ids are None or g_ids[j] != q_ids[i]
    (``q_ids`` [nQ] / ``g_ids`` [N] int64, both or neither, all 64 bits compared; ``live`` [N] bool or uint8).  Operands and scores are
    ``search_coarse``'s: an admissible row carries the same fp32 bits.  -> part [nQ, S, D] int64, the per-slab list words
    (key << 32 | ~row, best first, 0 = no entry); ``search_merge(part, D)`` merges and decodes them (S = 1 included).  ``slabs``:
    None = sc_search_slabs(nQ, N, D); any S >= 1 is legal (a slab may hold no admissible row) and the merged lists do not depend on it."""
    return _search_words("search_coarse_filtered", q_bf16, g_bf16, nQ, N, D, q_ids, g_ids, live, slabs, False)


def search_rerank_filtered(q: torch.Tensor, q_scale: Optional[torch.Tensor], rows: torch.Tensor, g_scale: Optional[torch.Tensor],
                           cand_idx: torch.Tensor, cand_vals: torch.Tensor, eps: torch.Tensor, k: int, vals: Optional[torch.Tensor] = None,
                           idx: Optional[torch.Tensor] = None, certified: Optional[torch.Tensor] = None):
    """``search_rerank`` with the certificate over the admissible rows (sc_search_rerank_filtered_f32, csrc/search_compact_filter.hip):
    the same operands - ``cand_idx`` / ``cand_vals`` [nQ, D] the merged lists of ``search_coarse_filtered``, -1 = no candidate - and the
    same fp64 re-rank; certified = 1 where every value is finite and (the query has fewer than D candidates, so every admissible row
    is one, or e_k - |e_k| 2^-23 > cand_vals[:, D - 1] + eps).  ``eps`` must bound |exact - coarse| over the rows that can be admissible."""
    return _search_rerank("search_rerank_filtered", q, q_scale, rows, g_scale, cand_idx, cand_vals, eps, k, vals, idx, certified)


def _rank_key_value(key: torch.Tensor) -> torch.Tensor:
    """the uint32 keys of csrc/rank.hip (held as int32 bits) -> the fp32 values they stand for; key 0 (no candidate) -> -inf"""
    bits = torch.where(key < 0, key & 0x7fffffff, ~key)                # key >= 2^31: a value >= 0 with its sign bit set; below: the complement
    return torch.where(key == 0, torch.full_like(bits, -8388608), bits).view(torch.float32)   # 0xff800000 = -inf


def rank_counts(a_split: torch.Tensor, b_split: torch.Tensor, a_ids: torch.Tensor, b_ids: torch.Tensor, nA: int, nB: int,
                slabs: Optional[int] = None):
    """For the nA rows of A against the nB rows of B, candidate j being correct for query i iff a_ids[i] == b_ids[j]
    (sc_rank_counts_bf16, csrc/rank.hip): -> (best_a [nA] fp32, ahead_a [nA] int32, best_b [nB] fp32, ahead_b [nB] int32).  ``best`` is
    the largest score over a query's correct, non-NaN candidates (-inf: none) and ``ahead`` counts the candidates scoring above it
    plus the wrong ones that tie with it or are NaN - A's rows as queries over B's rows in ``_a``, the other way round in ``_b``.
    ``a_split`` = split3_bf16(A, 0) [>= roundup(nA, 128), 6 Ep], ``b_split`` = split3_bf16(B, 1) [>= roundup(nB, 128), 6 Ep]; the scores are
    those of ``search_topk`` / ``cosine_scores_split`` and no [nA, nB] matrix is written.  ``slabs``: how many slabs B's rows are cut
    into (None: sc_search_slabs(nA, nB, 1)); the result does not depend on it, nor on the run."""
    nA, nB = int(nA), int(nB)
    K6, S, _ = _rank_part_operands("rank_counts", a_split, b_split, a_ids, b_ids, nA, nB, (), None, slabs)
    out = torch.zeros(2 * (nA + nB), device=a_split.device, dtype=torch.int32)    # the kernel's four outputs, zeroed in one fill
    key_a, key_b, ahead_a, ahead_b = out[:nA], out[nA: nA + nB], out[nA + nB: 2 * nA + nB], out[2 * nA + nB:]
    if nA and nB:
        check(lib().sc_rank_counts_bf16(_p(a_split), _p(b_split), _p(a_ids), _p(b_ids), nA, nB, K6, S, _p(key_a), _p(key_b), _p(ahead_a),
                                        _p(ahead_b), _stream()), "sc_rank_counts_bf16")
    return _rank_key_value(key_a), ahead_a, _rank_key_value(key_b), ahead_b


def _rank_part_operands(name: str, a_split, b_split, a_ids, b_ids, nA: int, nB: int, counts, b_live, slabs):
    """The operand checks of ``rank_counts`` / ``rank_best`` / ``rank_ahead`` (``name``), those of the caller's accumulators ``counts``
    (pairs of (tensor, rows): int32, contiguous, on the device) and of ``b_live`` -> (K6, S, the mask as uint8 or None)"""
    every = (a_split, b_split, a_ids, b_ids) + tuple(t for t, _ in counts) + (() if b_live is None else (b_live,))
    if not all(t.is_cuda for t in every):
        raise RuntimeError(f"{name} runs on the HIP kernels: no CPU path")
    assert a_split.dtype == torch.bfloat16 and b_split.dtype == torch.bfloat16 and a_split.dim() == 2 and b_split.dim() == 2
    assert a_split.is_contiguous() and b_split.is_contiguous()
    K6 = a_split.shape[1]
    assert b_split.shape[1] == K6, (a_split.shape, b_split.shape)
    assert a_split.shape[0] >= -(-nA // 128) * 128 and b_split.shape[0] >= -(-nB // 128) * 128, (a_split.shape, nA, b_split.shape, nB)
    assert a_ids.dtype == torch.int64 and b_ids.dtype == torch.int64 and a_ids.is_contiguous() and b_ids.is_contiguous()
    assert tuple(a_ids.shape) == (nA,) and tuple(b_ids.shape) == (nB,), (a_ids.shape, nA, b_ids.shape, nB)
    for t, rows in counts:
        assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (rows,), (name, t.dtype, t.shape, rows)
    if b_live is not None:
        assert b_live.dtype in (torch.bool, torch.uint8) and b_live.is_contiguous() and tuple(b_live.shape) == (nB,), (b_live.dtype, b_live.shape, nB)
        b_live = b_live.view(torch.uint8)
    return K6, (search_slabs(nA, nB, 1) if slabs is None else int(slabs)), b_live


def rank_best(a_split: torch.Tensor, b_split: torch.Tensor, a_ids: torch.Tensor, b_ids: torch.Tensor, nA: int, nB: int,
              key_a: torch.Tensor, key_b: torch.Tensor, *, b_live: Optional[torch.Tensor] = None, slabs: Optional[int] = None) -> None:
    """The first phase of ``rank_counts`` for one (A range, B range) pair, ACCUMULATED (sc_rank_best_bf16, csrc/rank.hip):
    key_a [nA] / key_b [nB] int32 (the kernel's uint32 keys; ``_rank_key_value`` decodes them, 0 = none) take the maximum of what
    they hold and the pair's largest key over correct, non-NaN candidates.  ``b_live`` [nB] bool / uint8 or None: a row of B with
    b_live == 0 is no candidate and no query, and its slot of ``key_b`` is not touched.  The caller zeroes the keys once, calls this
    for every pair, then ``rank_ahead`` for every pair; operands, scores and ``slabs`` are ``rank_counts``'."""
    nA, nB = int(nA), int(nB)
    K6, S, live = _rank_part_operands("rank_best", a_split, b_split, a_ids, b_ids, nA, nB, ((key_a, nA), (key_b, nB)), b_live, slabs)
    if nA and nB:
        check(lib().sc_rank_best_bf16(_p(a_split), _p(b_split), _p(a_ids), _p(b_ids), _p(live), nA, nB, K6, S, _p(key_a), _p(key_b),
                                      _stream()), "sc_rank_best_bf16")


def rank_ahead(a_split: torch.Tensor, b_split: torch.Tensor, a_ids: torch.Tensor, b_ids: torch.Tensor, nA: int, nB: int,
               key_a: torch.Tensor, key_b: torch.Tensor, ahead_a: torch.Tensor, ahead_b: torch.Tensor, *,
               b_live: Optional[torch.Tensor] = None, slabs: Optional[int] = None) -> None:
    """The second phase of ``rank_counts`` for one pair, ACCUMULATED (sc_rank_ahead_bf16, csrc/rank.hip): reads the final keys
    ``key_a`` [nA] / ``key_b`` [nB] (``rank_best`` over EVERY pair) and adds to ahead_a [nA] / ahead_b [nB] int32 the pair's
    candidates that rank ahead under ``rank_counts``' rule.  ``b_live`` as in ``rank_best``: a dead row's ``ahead_b`` is not touched."""
    nA, nB = int(nA), int(nB)
    K6, S, live = _rank_part_operands("rank_ahead", a_split, b_split, a_ids, b_ids, nA, nB,
                                      ((key_a, nA), (key_b, nB), (ahead_a, nA), (ahead_b, nB)), b_live, slabs)
    if nA and nB:
        check(lib().sc_rank_ahead_bf16(_p(a_split), _p(b_split), _p(a_ids), _p(b_ids), _p(live), nA, nB, K6, S, _p(key_a), _p(key_b),
                                       _p(ahead_a), _p(ahead_b), _stream()), "sc_rank_ahead_bf16")


def topk_rescore_cos(kw: torch.Tensor, table: torch.Tensor, idx: torch.Tensor, vals: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """vals[r, j] <- cos(kw[r], table[idx[r, j]]) accumulated in fp64 (sc_topk_rescore_cos_f32): kw [rows, E], table [V, E] fp32, idx /
    vals [rows, k] int32 / fp32 contiguous (idx as ops.topk_rows wrote it; -1 -> -inf)."""
    rows, E = kw.shape
    assert kw.dtype == torch.float32 and table.dtype == torch.float32 and kw.stride(1) == 1 and table.stride(1) == 1 and table.shape[1] == E
    assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and idx.is_contiguous() and vals.is_contiguous()
    assert idx.shape == vals.shape and idx.shape[0] == rows
    if rows:
        check(lib().sc_topk_rescore_cos_f32(_p(kw), kw.stride(0), _p(table), table.stride(0), table.shape[0], E, float(eps), _p(idx), rows,
                                            idx.shape[1], _p(vals), _stream()), "sc_topk_rescore_cos_f32")
    return vals


def vq_rowstats(x: torch.Tensor, V: int, temp: float, mask_cols=(0, 2, 3)):
    """x [Nk, >= V] fp32 (masked columns overwritten with -inf) -> idx [Nk] int64, lse_t, lse_1, ent [Nk] fp32."""
    Nk = x.shape[0]
    assert x.dtype == torch.float32 and x.stride(1) == 1 and x.shape[1] >= V
    dev = x.device
    idx = torch.empty(Nk, device=dev, dtype=torch.int64)
    lse_t, lse_1, ent = (torch.empty(Nk, device=dev, dtype=torch.float32) for _ in range(3))
    cols = [int(c) for c in mask_cols if 0 <= int(c) < V]
    assert len(cols) <= 4
    arr = (ctypes.c_int32 * 4)(*(cols + [-1] * (4 - len(cols))))
    check(lib().sc_vq_rowstats(_p(x), x.stride(0), Nk, V, float(temp), arr, len(cols), _p(idx), _p(lse_t), _p(lse_1), _p(ent), _stream()),
          "sc_vq_rowstats")
    return idx, lse_t, lse_1, ent


def vq_perplexity(x: torch.Tensor, V: int, idx: torch.Tensor, lse_1: torch.Tensor, nchunk: int = 16) -> torch.Tensor:
    """-> [code_perplexity, prob_perplexity] (fp32, device)."""
    Nk = x.shape[0]
    nchunk = max(1, min(nchunk, Nk))
    partial = torch.empty(nchunk, V, device=x.device, dtype=torch.float32)
    hist = torch.empty(V + 64, device=x.device, dtype=torch.int32)       # + 64 words: the entropy partials of the workgroups
    out = torch.empty(2, device=x.device, dtype=torch.float32)
    check(lib().sc_vq_perplexity(_p(x), x.stride(0), Nk, V, _p(idx), _p(lse_1), _p(partial), nchunk, _p(hist), _p(out), _stream()),
          "sc_vq_perplexity")
    return out


def vq_gather(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    Nk, Et = idx.numel(), table.shape[1]
    assert table.dtype == torch.float32 and table.stride(1) == 1 and idx.dtype == torch.int64
    out = torch.empty(Nk, Et, device=table.device, dtype=torch.float32)
    check(lib().sc_vq_gather_f32(_p(table), table.stride(0), _p(idx), _p(out), Et, Nk, Et, _stream()), "sc_vq_gather_f32")
    return out


def vq_onehot(idx: torch.Tensor, V: int) -> torch.Tensor:
    out = torch.empty(idx.numel(), V, device=idx.device, dtype=torch.float32)
    check(lib().sc_vq_onehot_f32(_p(idx), _p(out), V, idx.numel(), V, _stream()), "sc_vq_onehot_f32")
    return out


def vq_soft_bwd(x: torch.Tensor, lse_t: torch.Tensor, t: torch.Tensor, V: int, temp: float, out_bf16: bool, Vpad: Optional[int] = None):
    """dx [Nk, Vpad] = softmax(x / temp)(t - <softmax, t>) / temp; x, t [Nk, >= V] fp32."""
    Nk = x.shape[0]
    Vpad = V if Vpad is None else Vpad
    assert x.dtype == torch.float32 and t.dtype == torch.float32 and x.stride(1) == 1 and t.stride(1) == 1
    dx = torch.empty(Nk, Vpad, device=x.device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    check(lib().sc_vq_soft_bwd(_p(x), x.stride(0), _p(lse_t), _p(t), t.stride(0), Nk, V, Vpad, float(temp), _p(dx), Vpad,
                               int(out_bf16), _stream()), "sc_vq_soft_bwd")
    return dx


def vq_norm_bwd(kw: torch.Tensor, rnorm: torch.Tensor, dy: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    Nk, Et = kw.shape
    assert kw.dtype == torch.float32 and dy.dtype == torch.float32 and kw.stride(1) == 1 and dy.stride(1) == 1
    dx = torch.empty(Nk, Et, device=kw.device, dtype=torch.float32)
    check(lib().sc_vq_norm_bwd_f32(_p(kw), kw.stride(0), _p(rnorm), _p(dy), dy.stride(0), float(eps), _p(dx), Et, Nk, Et, _stream()),
          "sc_vq_norm_bwd_f32")
    return dx


def vq_mode_operands(name: str, x, V: int, temp, stats=None, mats=()) -> None:
    """The operands of the quantiser's soft / Gumbel kernels (csrc/vq.hip, behind the row statistics), checked before any launch - format errors first,
    "device tensors only" last: x [Nk, >= V] fp32 with unit column stride and Nk V < 2^32 (the noise index is 32 bits wide), temp a
    positive float, ``stats`` the contiguous [2, Nk] fp32 row statistics of vq_noisy_rowstats, ``mats`` = (name, tensor) pairs of
    [Nk, >= V] fp32 matrices."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{name}: x must be a 2-D tensor")
    if x.dtype != torch.float32:
        raise ValueError(f"{name}: x must be torch.float32, not {x.dtype}")
    Nk, V = x.shape[0], int(V)
    if Nk == 0 or V <= 0 or x.shape[1] < V or x.stride(1) != 1:
        raise ValueError(f"{name}: x {tuple(x.shape)} must have rows, at least V = {V} > 0 columns and unit column stride")
    if Nk * V >= 1 << 32:
        raise ValueError(f"{name}: x has {Nk} rows of V = {V} scores: Nk * V must stay below 2^32 (the noise index is 32 bits wide)")
    if not float(temp) > 0.0:
        raise ValueError(f"{name}: temp must be positive, not {temp}")
    if stats is not None and (not isinstance(stats, torch.Tensor) or stats.dtype != torch.float32 or tuple(stats.shape) != (2, Nk)
                              or not stats.is_contiguous()):
        raise ValueError(f"{name}: stats must be a contiguous torch.float32 tensor of shape (2, {Nk}) (vq_noisy_rowstats)")
    for what, t in mats:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != Nk or t.shape[1] < V or t.stride(1) != 1:
            raise ValueError(f"{name}: {what} must be a torch.float32 matrix [{Nk}, >= {V}] with unit column stride")
    given = [("x", x)] + ([("stats", stats)] if stats is not None else []) + list(mats)
    for what, t in given:
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on the HIP kernels: device tensors only ({what})")
    for what, t in given:
        if t.device != x.device:
            raise ValueError(f"{name}: {what} is on {t.device}, x on {x.device}")


def vq_gumbel(Nk: int, V: int, seed: int, device) -> torch.Tensor:
    """g [Nk, V] fp32 = -log(-log u), u from sc_hash32((n V + v) ^ seed): the noise the Gumbel kernels evaluate in place, materialised
    (sc_vq_gumbel_f32) for host twins and torch yardsticks."""
    Nk, V = int(Nk), int(V)
    if Nk <= 0 or V <= 0 or Nk * V >= 1 << 32:
        raise ValueError(f"vq_gumbel: Nk = {Nk} and V = {V} must be positive with Nk * V below 2^32")
    if torch.device(device).type != "cuda":
        raise RuntimeError("vq_gumbel runs on the HIP kernels: device tensors only")
    g = torch.empty(Nk, V, device=device, dtype=torch.float32)
    check(lib().sc_vq_gumbel_f32(_p(g), V, Nk, V, int(seed) & 0xffffffff, _stream()), "sc_vq_gumbel_f32")
    return g


def vq_noisy_rowstats(x: torch.Tensor, V: int, temp: float, seed: int = 0, noise: bool = True):
    """x [Nk, >= V] fp32, masked (vq_rowstats ran) -> idx [Nk] int64 = first argmax(x + g), stats [2, Nk] fp32 = (max (x + g),
    log sum exp((x + g - max) / temp)): LSE((x + g) / temp) = stats[0] / temp + stats[1], kept apart for the soft kernels.
    ``noise`` false: the same statistics of x itself."""
    vq_mode_operands("vq_noisy_rowstats", x, V, temp)
    Nk = x.shape[0]
    idx = torch.empty(Nk, device=x.device, dtype=torch.int64)
    stats = torch.empty(2, Nk, device=x.device, dtype=torch.float32)
    check(lib().sc_vq_noisy_rowstats(_p(x), x.stride(0), Nk, V, float(temp), int(seed) & 0xffffffff, int(bool(noise)), _p(idx),
                                     _p(stats[0]), _p(stats[1]), _stream()), "sc_vq_noisy_rowstats")
    return idx, stats


def vq_soft_prob(x: torch.Tensor, stats: torch.Tensor, V: int, temp: float, seed: int = 0, noise: bool = False) -> torch.Tensor:
    """s [Nk, V] fp32 = softmax((x + g) / temp) (g = 0 without ``noise``), exactly 0 in masked columns; ``stats`` [2, Nk] =
    vq_noisy_rowstats' for the same (temp, seed, noise)."""
    if isinstance(x, torch.Tensor) and x.shape[0] > 65535:
        raise ValueError(f"vq_soft_prob: x has {x.shape[0]} rows, at most 65535")
    vq_mode_operands("vq_soft_prob", x, V, temp, stats=stats)
    Nk = x.shape[0]
    s = torch.empty(Nk, V, device=x.device, dtype=torch.float32)
    check(lib().sc_vq_soft_prob_f32(_p(x), x.stride(0), _p(stats[0]), _p(stats[1]), Nk, V, float(temp), int(seed) & 0xffffffff, int(bool(noise)), _p(s), V,
                                    _stream()), "sc_vq_soft_prob_f32")
    return s


def vq_soft_split(x: torch.Tensor, stats: torch.Tensor, V: int, temp: float, Vp: int, seed: int = 0, noise: bool = False,
                  rows_pad: int = 128) -> torch.Tensor:
    """The same s as bf16 hi + lo in the three K-blocks [hi | hi | lo] of the soft product: [Nkp, 3 Vp] bf16, zero outside [Nk, V]."""
    Vp = int(Vp)
    if Vp < V or Vp % 64 != 0:
        raise ValueError(f"vq_soft_split: Vp = {Vp} must be a multiple of 64 at or above V = {V}")
    vq_mode_operands("vq_soft_split", x, V, temp, stats=stats)
    Nk = x.shape[0]
    Nkp = -(-Nk // rows_pad) * rows_pad
    out = torch.empty(Nkp, 3 * Vp, device=x.device, dtype=torch.bfloat16)
    check(lib().sc_vq_soft_split_bf16(_p(x), x.stride(0), _p(stats[0]), _p(stats[1]), Nk, V, float(temp), int(seed) & 0xffffffff, int(bool(noise)), _p(out),
                                      Nkp, Vp, _stream()), "sc_vq_soft_split_bf16")
    return out


def vq_soft_table(table: torch.Tensor, Vp: int) -> torch.Tensor:
    """table [V, Et] fp32 -> its transposed bf16 split [Et, 3 Vp] = [hi | lo | hi] (hi = bf16(table), lo = bf16(table - hi); zero in the
    columns V .. Vp - 1 of every block): the W operand of ``vq_soft_product``.  Built once per table, off the step's path."""
    V, Et = table.shape
    tT = table.detach().float().t()
    hi = tT.to(torch.bfloat16)
    lo = (tT - hi.float()).to(torch.bfloat16)
    W = torch.zeros(Et, 3, Vp, device=table.device, dtype=torch.bfloat16)
    W[:, 0, :V], W[:, 1, :V], W[:, 2, :V] = hi, lo, hi
    return W.view(Et, 3 * Vp)


def vq_soft_slices(Vp: int) -> int:
    """Equal slices (multiples of 64, at most 16) of the soft product's contraction of 3 Vp."""
    units = 3 * Vp // 64
    return max(s for s in range(1, 17) if units % s == 0)


def vq_soft_product(s_split: torch.Tensor, w_split: torch.Tensor, Et: int) -> torch.Tensor:
    """keywords [Nkp, Et] fp32 = s . table over the K-blocks [hi | hi | lo] x [hi | lo | hi]: hi hi + hi lo + lo hi, every bf16 product
    exact in fp32, as ONE batched bf16 GEMM cut along the contraction into fp32 partials that sc_colsum_f32 adds in slice order."""
    assert s_split.dtype == torch.bfloat16 and w_split.dtype == torch.bfloat16 and s_split.is_contiguous() and w_split.is_contiguous()
    Nkp, K3 = s_split.shape
    assert w_split.shape == (Et, K3) and K3 % 192 == 0, (tuple(w_split.shape), Et, K3)
    S = vq_soft_slices(K3 // 3)
    Kc = K3 // S
    part = torch.empty(S, Nkp, Et, device=s_split.device, dtype=torch.float32)
    gemm_raw(s_split, K3, w_split, K3, part, Et, Nkp, Et, Kc, out_f32=True, nb1=S, sA=(Kc, 0), sW=(Kc, 0), sC=(Nkp * Et, 0))
    out = torch.empty(Nkp, Et, device=s_split.device, dtype=torch.float32)
    colsum(part, Nkp * Et, S, Nkp * Et, out)
    return out


def vq_soft_bwd2(x: torch.Tensor, stats: torch.Tensor, t: torch.Tensor, V: int, temp: float, out_bf16: bool, Vpad: Optional[int] = None,
                 seed: int = 0, noise: bool = False, want_dtemp: bool = False):
    """-> (dx [Nk, Vpad] = s (t - <s, t>) / temp with s = softmax((x + g) / temp), dtemp [1] = -(1 / temp) sum dz z or None): the row
    terms of d temp are added in index order by sc_colsum_f32."""
    Vpad = V if Vpad is None else int(Vpad)
    if Vpad < V:
        raise ValueError(f"vq_soft_bwd2: Vpad = {Vpad} is below V = {V}")
    vq_mode_operands("vq_soft_bwd2", x, V, temp, stats=stats, mats=(("t", t),))
    Nk = x.shape[0]
    dx = torch.empty(Nk, Vpad, device=x.device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    rows = torch.empty(Nk, device=x.device, dtype=torch.float32) if want_dtemp else None
    check(lib().sc_vq_soft_bwd2(_p(x), x.stride(0), _p(stats[0]), _p(stats[1]), _p(t), t.stride(0), Nk, V, Vpad, float(temp), int(seed) & 0xffffffff,
                                int(bool(noise)), _p(dx), Vpad, int(out_bf16), _p(rows), _stream()), "sc_vq_soft_bwd2")
    dtemp = None
    if want_dtemp:
        dtemp = torch.empty(1, device=x.device, dtype=torch.float32)
        colsum(rows, 1, Nk, 1, dtemp)
    return dx, dtemp


def bn_rows_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, run_mean: torch.Tensor, run_var: torch.Tensor,
                training: bool, momentum: float, eps: float):
    """BatchNorm over the rows of x [N, E] fp32 -> (y, save_mean, save_rstd); running estimates updated in place when training."""
    N, E = x.shape
    assert x.dtype == torch.float32 and x.stride(1) == 1
    for t in (gamma, beta, run_mean, run_var):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == E
    y = torch.empty(N, E, device=x.device, dtype=torch.float32)
    sm = torch.empty(E, device=x.device, dtype=torch.float32) if training else None
    sr = torch.empty(E, device=x.device, dtype=torch.float32) if training else None
    check(lib().sc_bn_rows_fwd(_p(x), x.stride(0), N, E, _p(gamma), _p(beta), _p(run_mean), _p(run_var), int(training), float(momentum),
                               float(eps), _p(y), E, _p(sm), _p(sr), _stream()), "sc_bn_rows_fwd")
    return y, sm, sr


def bn_rows_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, save_mean: torch.Tensor, save_rstd: torch.Tensor):
    N, E = x.shape
    assert dy.dtype == torch.float32 and dy.stride(1) == 1 and tuple(dy.shape) == (N, E)
    dx = torch.empty(N, E, device=x.device, dtype=torch.float32)
    dg = torch.empty(E, device=x.device, dtype=torch.float32)
    db = torch.empty(E, device=x.device, dtype=torch.float32)
    check(lib().sc_bn_rows_bwd(_p(x), x.stride(0), _p(dy), dy.stride(0), N, E, _p(gamma), _p(save_mean), _p(save_rstd), _p(dx), E,
                               _p(dg), _p(db), _stream()), "sc_bn_rows_bwd")
    return dx, dg, db


def bn_eachkw_fwd(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, run_mean: torch.Tensor, run_var: torch.Tensor,
                  training: bool, momentum: float, eps: float):
    """Fixed-count keyword BatchNorm: x [B, K, Ed] fp32, one statistic per (slot k, channel d) over B, parameters and running
    buffers [Ed * K] indexed d * K + k (the reference checkpoint's layout) -> (y, save_mean, save_rstd)."""
    B, K, Ed = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    for t in (gamma, beta, run_mean, run_var):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == K * Ed
    y = torch.empty_like(x)
    sm = torch.empty(K * Ed, device=x.device, dtype=torch.float32) if training else None
    sr = torch.empty(K * Ed, device=x.device, dtype=torch.float32) if training else None
    check(lib().sc_bn_eachkw_fwd(_p(x), B, K, Ed, _p(gamma), _p(beta), _p(run_mean), _p(run_var), int(training), float(momentum),
                                 float(eps), _p(y), _p(sm), _p(sr), _stream()), "sc_bn_eachkw_fwd")
    return y, sm, sr


def bn_eachkw_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, save_mean: torch.Tensor, save_rstd: torch.Tensor):
    B, K, Ed = x.shape
    assert dy.dtype == torch.float32 and dy.is_contiguous() and dy.shape == x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(K * Ed, device=x.device, dtype=torch.float32)
    db = torch.empty(K * Ed, device=x.device, dtype=torch.float32)
    check(lib().sc_bn_eachkw_bwd(_p(x), _p(dy), B, K, Ed, _p(gamma), _p(save_mean), _p(save_rstd), _p(dx), _p(dg), _p(db), _stream()),
          "sc_bn_eachkw_bwd")
    return dx, dg, db


def softmax_fwd(scores: torch.Tensor, key_mask: torch.Tensor, rows_per_batch: int, scale: float, drop_p: float = 0.0,
                drop_seed: int = 0):
    """P = softmax(scale * scores | key mask) as bf16 (+ the dropped copy in train mode); scores fp32 [..., n] contiguous,
    key_mask uint8 / bool [batches, n] (non-zero = padded key).  Returns (P, Pd) with Pd = P when drop_p == 0."""
    n = scores.shape[-1]
    rows = scores.numel() // n
    assert scores.dtype == torch.float32 and scores.is_contiguous() and key_mask.is_contiguous() and key_mask.element_size() == 1
    assert key_mask.shape[-1] == n and rows == key_mask.numel() // n * rows_per_batch
    P = torch.empty(scores.shape, device=scores.device, dtype=torch.bfloat16)
    Pd = torch.empty_like(P) if drop_p > 0.0 else None
    check(lib().sc_softmax_fwd(_p(scores), _p(key_mask), _p(P), _p(Pd), rows, n, rows_per_batch, float(scale), float(drop_p),
                               int(drop_seed) & 0xffffffff, _stream()), "sc_softmax_fwd")
    return P, (Pd if Pd is not None else P)


def softmax_bwd(dP: torch.Tensor, P: torch.Tensor, scale: float, drop_p: float = 0.0, drop_seed: int = 0) -> torch.Tensor:
    """dS = scale * P (dP' - rowsum(P dP')) as bf16, dP' = the dropout backward of dP (same mask as softmax_fwd)."""
    n = dP.shape[-1]
    rows = dP.numel() // n
    assert dP.dtype == torch.float32 and P.dtype == torch.bfloat16 and dP.is_contiguous() and P.is_contiguous() and P.shape == dP.shape
    dS = torch.empty_like(P)
    check(lib().sc_softmax_bwd(_p(dP), _p(P), _p(dS), rows, n, float(scale), float(drop_p), int(drop_seed) & 0xffffffff, _stream()),
          "sc_softmax_bwd")
    return dS


def act_bf16(u: torch.Tensor, act: int, df: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act 1 = erf-GELU, 2 = QuickGELU; with ``df``: df * act'(u)."""
    assert u.dtype == torch.bfloat16 and u.is_contiguous() and (df is None or (df.dtype == torch.bfloat16 and df.is_contiguous()))
    if out is None:
        out = torch.empty_like(u)
    check(lib().sc_act_bf16(_p(u), _p(df), _p(out), u.numel(), act, _stream()), "sc_act_bf16")
    return out


def layernorm_bf16(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, out: Optional[torch.Tensor] = None,
                   eps: float = 1e-5, act: int = 0) -> torch.Tensor:
    assert x.dim() == 2 and x.dtype == torch.bfloat16 and x.stride(1) == 1
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32
    if out is None:
        out = torch.empty_like(x)
    check(lib().sc_layernorm_bf16(_p(x), x.stride(0), _p(gamma), _p(beta), _p(out), out.stride(0), x.shape[0],
                                  x.shape[1], float(eps), act, _stream()), "sc_layernorm_bf16")
    return out


def _wav_window(wav: torch.Tensor, L: Optional[int], wav_off: Optional[torch.Tensor]) -> int:
    """host-side shape contract of the kernels that read the caller's [B, ld] batch in place: unit sample stride, a padded length
    L <= the row width, int64 offsets on the batch's device (their range is the caller's contract: off_b + len_b <= width)"""
    assert wav.dim() == 2 and wav.stride(1) == 1 and wav.dtype == torch.float32, (wav.shape, wav.stride(), wav.dtype)
    L = wav.shape[1] if L is None else int(L)
    assert 0 < L <= wav.shape[1] and (wav.shape[0] == 1 or wav.stride(0) >= wav.shape[1]), (L, wav.shape, wav.stride())
    if wav_off is not None:
        assert wav_off.dtype == torch.int64 and wav_off.device == wav.device and wav_off.numel() == wav.shape[0] and wav_off.is_contiguous()
    return L


def wav_prep(wav: torch.Tensor, wav_len: torch.Tensor, out: torch.Tensor, normalize: bool, L: Optional[int] = None,
             wav_off: Optional[torch.Tensor] = None) -> None:
    """L / wav_off: the in-forward crop - utterance b is wav[b, off_b : off_b + len_b], padded length L (sc_wav_prep, uniform rows)"""
    assert wav_len.dtype == torch.int64 and out.dtype == torch.float32
    L = _wav_window(wav, L, wav_off)
    check(lib().sc_wav_prep(_p(wav), wav.stride(0), _p(wav_len), _p(wav_off), _p(out), out.stride(0), None, 0, wav.shape[0], L, int(normalize),
                            _stream()), "sc_wav_prep")


def wav_prep_seg(wav: torch.Tensor, wav_len: torch.Tensor, out_flat: torch.Tensor, seg: "RowSegments", samples_per_row: int,
                 normalize: bool, L: Optional[int] = None, wav_off: Optional[torch.Tensor] = None) -> None:
    """waveform into the ragged layout: utterance b at sample samples_per_row * row0[b] of ONE flat fp32 buffer (sc_wav_prep with seg);
    L / wav_off as in wav_prep"""
    assert wav_len.dtype == torch.int64 and out_flat.dtype == torch.float32
    assert out_flat.numel() >= samples_per_row * seg.rows + 16
    L = _wav_window(wav, L, wav_off)
    check(lib().sc_wav_prep(_p(wav), wav.stride(0), _p(wav_len), _p(wav_off), _p(out_flat), 0, seg.ref(), samples_per_row, seg.B, L,
                            int(normalize), _stream()), "sc_wav_prep")


def _conv0_groupnorm_gelu(stats_wav: torch.Tensor, wav_len: Optional[torch.Tensor], wav_off: Optional[torch.Tensor], x: torch.Tensor,
                          seg: Optional["RowSegments"], samples_per_row: int, w0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                          T0: int, R0: int, out: torch.Tensor, eps: float, nchunk: int, out_f32: bool = False):
    """stats -> finalize -> gn_gelu of both row layouts: the GroupNorm statistics of stats_wav over t < T0 (wav_len None: the prepared
    batch; else the caller's, masked by wav_len / wav_off), then the activation of the prepared waveform x (seg None: [B, ldw] rows)"""
    B, C = stats_wav.shape[0], w0.shape[0]
    partial = torch.empty(B * nchunk * DEFINES["SC_CONV0_NSTAT"], device=stats_wav.device, dtype=torch.float64)
    scale = torch.empty(B, C, device=stats_wav.device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    L = lib()
    check(L.sc_conv0_stats(_p(stats_wav), stats_wav.stride(0), _p(wav_len), _p(wav_off), B, T0, nchunk, _p(partial), _stream()), "sc_conv0_stats")
    check(L.sc_conv0_finalize(_p(partial), nchunk, _p(w0), _p(gamma), _p(beta), B, C, T0, float(eps), _p(scale), _p(shift), _stream()),
          "sc_conv0_finalize")
    check(L.sc_conv0_gn_gelu(_p(x), 0 if seg is not None else x.stride(0), seg.ref() if seg is not None else None, samples_per_row, _p(w0),
                             _p(scale), _p(shift), _p(out), int(out_f32), B, R0, C, _stream()), "sc_conv0_gn_gelu")
    return scale, shift, partial, nchunk


def conv0_groupnorm_gelu_seg(wav: torch.Tensor, wav_len: torch.Tensor, wav_flat: torch.Tensor, seg: "RowSegments", samples_per_row: int,
                             w0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, T0: int, out: torch.Tensor, eps: float = 1e-5,
                             nchunk: int = 8, wav_off: Optional[torch.Tensor] = None) -> None:
    """conv layer 0 + GroupNorm + GELU on ragged rows.  The GroupNorm statistics run over the PADDED batch length T0 (fairseq feeds the
    zero-padded batch, speech_encoder_plus.py:75) and come straight from the caller's [B, L] batch masked by wav_len; the activation is
    written for the rows of the segment layout only."""
    _wav_window(wav, None, wav_off)
    _conv0_groupnorm_gelu(wav, wav_len, wav_off, wav_flat, seg, samples_per_row, w0, gamma, beta, T0, 0, out, eps, nchunk)


def conv0_layernorm_gelu_seg(wav_flat: torch.Tensor, seg: "RowSegments", samples_per_row: int, w0: torch.Tensor, bias: Optional[torch.Tensor],
                             gamma: torch.Tensor, beta: torch.Tensor, out: torch.Tensor, eps: float = 1e-5) -> None:
    check(lib().sc_conv0_ln_gelu(_p(wav_flat), 0, seg.ref(), samples_per_row, _p(w0), _p(bias), _p(gamma), _p(beta), float(eps), _p(out), 0,
                                 seg.B, 0, w0.shape[0], _stream()), "sc_conv0_ln_gelu")


def conv0_groupnorm_gelu(wav_pad: torch.Tensor, w0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, T0: int,
                         R0: int, out: torch.Tensor, eps: float = 1e-5, nchunk: int = 8, out_f32: bool = False):
    """conv layer 0 + GroupNorm(C groups) over t < T0 + GELU -> out[B*R0, C] bf16 (channels-last; out_f32: the fp32 debug mode's
    unrounded fp32).  Returns what the backward (conv0_groupnorm_gelu_bwd) needs: (scale, shift, Gram statistics, nchunk)."""
    assert out.dtype == (torch.float32 if out_f32 else torch.bfloat16)
    return _conv0_groupnorm_gelu(wav_pad, None, None, wav_pad, None, 0, w0, gamma, beta, T0, R0, out, eps, nchunk, out_f32)


def conv0_groupnorm_gelu_bwd(wav_pad: torch.Tensor, w0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, saved, dy: torch.Tensor,
                             T0: int, R0: int, eps: float = 1e-5, nwc: int = 32):
    """Parameter gradients of conv layer 0 + GroupNorm + GELU (sc_conv0_gn_bwd): dy [B*R0, C] bf16 -> (dW0 [C, 10], dgamma [C], dbeta [C])."""
    scale, shift, stats, nchunk = saved
    B, C = wav_pad.shape[0], w0.shape[0]
    dev = wav_pad.device
    partial = torch.empty(B, nwc, C, 12, device=dev, dtype=torch.float32)
    contrib = torch.empty(B, C * 12, device=dev, dtype=torch.float32)
    check(lib().sc_conv0_gn_bwd(_p(wav_pad), wav_pad.stride(0), _p(w0), _p(scale), _p(shift), _p(dy), _p(stats), nchunk, _p(gamma), _p(beta),
                                B, T0, R0, C, float(eps), _p(partial), nwc, _p(contrib), _stream()), "sc_conv0_gn_bwd")
    tot = torch.empty(C * 12, device=dev, dtype=torch.float32)
    colsum(contrib, C * 12, B, C * 12, tot)
    tot = tot.view(C, 12)
    return tot[:, :10], tot[:, 10], tot[:, 11]


def conv0_layernorm_gelu(wav_pad: torch.Tensor, w0: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor,
                         beta: torch.Tensor, R0: int, out: torch.Tensor, eps: float = 1e-5, out_f32: bool = False) -> None:
    """conv layer 0 (+bias) + LayerNorm over channels + GELU ("layer_norm" extractor mode) -> out[B*R0, 512] bf16 (out_f32: the fp32
    debug mode's unrounded fp32)."""
    assert out.dtype == (torch.float32 if out_f32 else torch.bfloat16)
    B, C = wav_pad.shape[0], w0.shape[0]
    check(lib().sc_conv0_ln_gelu(_p(wav_pad), wav_pad.stride(0), None, 0, _p(w0), _p(bias), _p(gamma), _p(beta), float(eps), _p(out),
                                 int(out_f32), B, R0, C, _stream()), "sc_conv0_ln_gelu")


def conv0_layernorm_gelu_bwd(wav_pad: torch.Tensor, w0: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor,
                             dy: torch.Tensor, T0: int, R0: int, eps: float = 1e-5, nwc: int = 32):
    """Parameter gradients of conv layer 0 (+bias) + LayerNorm + GELU (sc_conv0_ln_bwd): dy [B*R0, 512] bf16 ->
    (dW0 [C, 10], dbias [C], dgamma [C], dbeta [C])."""
    B, C = wav_pad.shape[0], w0.shape[0]
    dev = wav_pad.device
    partial = torch.empty(B * nwc, C * 16, device=dev, dtype=torch.float32)
    check(lib().sc_conv0_ln_bwd(_p(wav_pad), wav_pad.stride(0), _p(w0), _p(bias), _p(gamma), _p(beta), float(eps), _p(dy), B, T0, R0, C,
                                _p(partial), nwc, _stream()), "sc_conv0_ln_bwd")
    tot = torch.empty(C * 16, device=dev, dtype=torch.float32)
    colsum(partial, C * 16, B * nwc, C * 16, tot)
    tot = tot.view(C, 16)
    return tot[:, :10], tot[:, 10], tot[:, 11], tot[:, 12]


def posconv_prep(x: torch.Tensor, valid_len: torch.Tensor, xz: torch.Tensor, xg: torch.Tensor, B: int, R: int, D: int,
                 G: int, halo: int) -> None:
    check(lib().sc_posconv_prep(_p(x), _p(valid_len), _p(xz), _p(xg), None, B, R, D, G, halo, _stream()), "sc_posconv_prep")


def posconv_prep_seg(x: torch.Tensor, valid_len: torch.Tensor, xz: torch.Tensor, xg: torch.Tensor, seg: "RowSegments", D: int, G: int,
                     halo: int) -> None:
    """ragged rows: xg = flat [G, rows + 2 halo B, D / G] slab buffer (numel at least that), utterance b at slab row row0[b] + 2 halo b"""
    assert xg.numel() >= (seg.rows + 2 * halo * seg.B) * D
    check(lib().sc_posconv_prep(_p(x), _p(valid_len), _p(xz), _p(xg), seg.ref(), 0, 0, D, G, halo, _stream()), "sc_posconv_prep")


def _posconv(xg, w, bias, residual, out, seg, B, R, D, G, Kp, Rp, alg_rows) -> None:
    """sc_posconv_bf16 in its timer bracket; ``alg_rows``: the rows the launch is credited with"""
    assert xg.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and out.dtype == torch.bfloat16
    if _timer is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    check(lib().sc_posconv_bf16(_p(xg), _p(w), _p(bias), _p(residual), _p(out), _seg(seg), B, R, D, G, Kp, Rp, _stream()), "sc_posconv_bf16")
    if _timer is not None:
        ev1.record()
        _timer.add("posconv", ev0, ev1, 2.0 * alg_rows * D * Kp * (D // G))


def posconv_seg(xg: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], residual: Optional[torch.Tensor], out: torch.Tensor,
                seg: "RowSegments", D: int, G: int, Kp: int, alg_rows: Optional[int] = None) -> None:
    """``posconv`` on ragged rows: the slab layout of ``posconv_prep_seg``, out / residual rows row0[b] + t"""
    _posconv(xg, w, bias, residual, out, seg, 0, 0, D, G, Kp, 0, seg.rows if alg_rows is None else alg_rows)


def posconv(xg: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], residual: Optional[torch.Tensor], out: torch.Tensor,
            B: int, R: int, D: int, G: int, Kp: int, alg_rows: Optional[int] = None) -> None:
    """HuBERT positional convolution + bias + GELU + residual on the slab layout of ``posconv_prep`` (sc_posconv_bf16):
    xg [G, B, Rp, D/G] bf16, w [G, D/G, Kp*D/G] bf16 tap-major, out / residual [B*R, D] bf16."""
    assert xg.is_contiguous() and w.is_contiguous() and out.is_contiguous() and xg.shape[0] == G and xg.shape[1] == B
    _posconv(xg, w, bias, residual, out, None, B, R, D, G, Kp, xg.shape[2], B * (R if alg_rows is None else alg_rows))


class LazyStates:
    """Hidden states kept RAW (in front of their LayerNorm) with row statistics (speech_encoder: LayerNorm folded into the encoder
    GEMMs): ``stats`` [NL, B*R, 8, 2] fp32, ``gamma`` / ``beta`` [NL, D] fp32, layers >= ``first_lazy`` are raw, ``ns`` valid strips."""

    def __init__(self, stats, gamma, beta, first_lazy: int, ns: int, eps: float):
        self.stats, self.gamma, self.beta, self.first_lazy, self.ns, self.eps = stats, gamma, beta, int(first_lazy), int(ns), float(eps)


def wsum_fwd(h: torch.Tensor, w_softmax: torch.Tensor, out: torch.Tensor, B: int, R: int, D: int, row_off: int,
             normalize: bool = False, lazy: Optional[LazyStates] = None, seg: Optional["RowSegments"] = None) -> None:
    """``seg``: h [NL, seg.rows, D] in the ragged layout -> out [B, R, D] uniform (every row written, zero outside the utterances)"""
    NL = h.shape[0]
    if seg is not None:
        assert lazy is None and h.shape[1] == seg.rows and B == seg.B
    if lazy is not None:
        assert not normalize
        check(lib().sc_wsum_lazy_fwd(_p(h), _p(w_softmax), NL, _p(out), B, R, D, row_off, _p(lazy.stats), _p(lazy.gamma), _p(lazy.beta),
                                     lazy.first_lazy, lazy.ns, lazy.eps, _stream()), "sc_wsum_lazy_fwd")
        return
    assert h.dtype == torch.bfloat16 and w_softmax.dtype == torch.float32 and out.dtype == torch.bfloat16
    check(lib().sc_wsum_fwd(_p(h), _p(w_softmax), NL, _p(out), _seg(seg), B, R, D, row_off, int(normalize), _stream()), "sc_wsum_fwd")


def wsum_bwd(h: torch.Tensor, g: torch.Tensor, B: int, R: int, D: int, row_off: int, nblk: int = 1024,
             normalize: bool = False, lazy: Optional[LazyStates] = None) -> torch.Tensor:
    """returns d(softmaxed weights)[NL] up to a common shift: <g, h_n - h_last> (sc_wsum_bwd: the callers' softmax projection
    w_n (d_n - sum_m w_m d_m) does not see the shift, and the fp32 sums keep the digits the projection needs)."""
    NL = h.shape[0]
    assert g.dtype == torch.float32
    part = torch.empty(nblk, NL, device=h.device, dtype=torch.float32)
    if lazy is not None:
        assert not normalize
        check(lib().sc_wsum_lazy_bwd(_p(h), _p(g), NL, _p(part), nblk, B, R, D, row_off, _p(lazy.stats), _p(lazy.gamma), _p(lazy.beta),
                                     lazy.first_lazy, lazy.ns, lazy.eps, _stream()), "sc_wsum_lazy_bwd")
        return part.sum(0)
    check(lib().sc_wsum_bwd(_p(h), _p(g), NL, _p(part), nblk, None, B, R, D, row_off, int(normalize), _stream()), "sc_wsum_bwd")
    return part.sum(0)


def cls_scores(X: torch.Tensor, vec: torch.Tensor, per_batch: bool, B: int, R: int, D: int, H: int) -> torch.Tensor:
    scores = torch.empty(B, H, R, device=X.device, dtype=torch.float32)
    assert vec.dtype == torch.float32 and vec.is_contiguous()
    check(lib().sc_cls_scores(_p(X), _p(vec), H * D if per_batch else 0, _p(scores), B, R, D, H, _stream()), "sc_cls_scores")
    return scores


def cls_pool_fwd(X: torch.Tensor, scores: torch.Tensor, lens: torch.Tensor, B: int, R: int, D: int, H: int,
                 mult: Optional[torch.Tensor] = None, want_psum: bool = False):
    """``mult`` [B,H,R] fp32 = dropout multipliers of the attention weights (0 or 1/(1-p)); p is returned un-masked.  ``want_psum``:
    also sum_s p mult [B,H] (the weight of the value bias when dropped weights no longer sum to 1)."""
    p = torch.empty(B, H, R, device=X.device, dtype=torch.float32)
    m = torch.empty(B, H, D, device=X.device, dtype=torch.float32)
    psum = torch.empty(B, H, device=X.device, dtype=torch.float32) if want_psum else None
    if mult is not None:
        assert mult.shape == (B, H, R) and mult.dtype == torch.float32 and mult.is_contiguous()
    check(lib().sc_cls_pool_fwd(_p(X), _p(scores), _p(lens), _p(p), _p(m), B, R, D, H, _p(mult), _p(psum), _stream()), "sc_cls_pool_fwd")
    return (p, m, psum) if want_psum else (p, m)


def cls_pool_bwd(X: torch.Tensor, p: torch.Tensor, dp: torch.Tensor, dm: torch.Tensor, a: torch.Tensor, lens: torch.Tensor,
                 B: int, R: int, D: int, H: int, mult: Optional[torch.Tensor] = None, cbias: Optional[torch.Tensor] = None):
    """``cbias`` [B,H]: ``dp`` is the raw X . dm and the kernel forms (dp + cbias) * mult itself; otherwise dp arrives in that form."""
    dX = torch.empty(B, R, D, device=X.device, dtype=torch.float32)
    da = torch.empty(B, H, D, device=X.device, dtype=torch.float32)
    check(lib().sc_cls_pool_bwd(_p(X), _p(p), _p(dp), _p(dm), _p(a), _p(lens), _p(dX), _p(da), B, R, D, H, _p(mult), _p(cbias), _stream()),
          "sc_cls_pool_bwd")
    return dX, da


def kw_pool_max_rows(Q: int, C: int, backward: bool = True) -> int:
    """Largest R (rows of X per utterance) sc_kw_pool_fwd / _bwd accept for Q queries and C constant keys (LDS-bound)."""
    return int(lib().sc_kw_pool_max_rows(int(Q), int(C), int(backward)))


def kw_pool_fwd(X: torch.Tensor, a: torch.Tensor, c: torch.Tensor, crow: torch.Tensor, flen: torch.Tensor, row0: int,
                mult: Optional[torch.Tensor] = None, want_psum: bool = False):
    """Constant-query pooling (csrc/kwpool.hip): X [B, R, D] bf16 with the frames of utterance b at rows row0 .. row0 + flen[b] - 1,
    a [Q, D], c [Q, C] (scores of the C constant keys), crow [C, D] (their rows), flen int32 [B] -> p [B, Q, C + R] (before ``mult``),
    m [B, Q, D] (, psum [B, Q] = sum p mult)."""
    B, R, D = X.shape
    Q, C = c.shape
    assert X.dtype == torch.bfloat16 and X.is_contiguous() and flen.dtype == torch.int32 and flen.numel() == B
    for t, shape in ((a, (Q, D)), (c, (Q, C)), (crow, (C, D))):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, (tuple(t.shape), shape)
    if mult is not None:
        assert tuple(mult.shape) == (B, Q, C + R) and mult.dtype == torch.float32 and mult.is_contiguous()
    scores = torch.empty(B, Q, R, device=X.device, dtype=torch.float32)
    p = torch.empty(B, Q, C + R, device=X.device, dtype=torch.float32)
    m = torch.empty(B, Q, D, device=X.device, dtype=torch.float32)
    psum = torch.empty(B, Q, device=X.device, dtype=torch.float32) if want_psum else None
    check(lib().sc_kw_pool_fwd(_p(X), _p(a), _p(c), _p(crow), _p(flen), _p(scores), _p(p), _p(m), _p(psum), _p(mult), B, R, D, Q, C,
                               int(row0), _stream()), "sc_kw_pool_fwd")
    return (p, m, psum) if want_psum else (p, m)


def kw_pool_bwd(X: torch.Tensor, a: torch.Tensor, crow: torch.Tensor, flen: torch.Tensor, row0: int, p: torch.Tensor, dm: torch.Tensor,
                mult: Optional[torch.Tensor] = None, cbias: Optional[torch.Tensor] = None, dx_dtype: torch.dtype = torch.float32):
    """-> dX [B, R, D] (``dx_dtype`` fp32 or bf16; zero outside the frames), da [Q, D], dc [Q, C].  ``cbias`` [B, Q]: gradient of psum."""
    B, R, D = X.shape
    Q, C = a.shape[0], crow.shape[0]
    assert tuple(p.shape) == (B, Q, C + R) and p.is_contiguous() and dm.dtype == torch.float32 and dm.is_contiguous()
    assert tuple(dm.shape) == (B, Q, D) and dx_dtype in (torch.float32, torch.bfloat16)
    if cbias is not None:
        assert cbias.dtype == torch.float32 and cbias.is_contiguous() and cbias.numel() == B * Q
    dev = X.device
    dpw = torch.empty(B, Q, R, device=dev, dtype=torch.float32)
    dX = torch.empty(B, R, D, device=dev, dtype=dx_dtype)
    da_part = torch.empty(B, Q, D, device=dev, dtype=torch.float32)
    dc_part = torch.empty(B, Q, C, device=dev, dtype=torch.float32)
    da = torch.empty(Q, D, device=dev, dtype=torch.float32)
    dc = torch.empty(Q, C, device=dev, dtype=torch.float32)
    check(lib().sc_kw_pool_bwd(_p(X), _p(a), _p(crow), _p(flen), _p(p), _p(mult), _p(dm), _p(cbias), _p(dpw), _p(dX),
                               int(dx_dtype == torch.bfloat16), _p(da_part), _p(dc_part), _p(da), _p(dc), B, R, D, Q, C, int(row0),
                               _stream()), "sc_kw_pool_bwd")
    return dX, da, dc


def sgemm(A: torch.Tensor, sai: int, sak: int, Bm: torch.Tensor, sbj: int, sbk: int, M: int, N: int, K: int,
          alpha: float = 1.0, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C[i, j] = alpha sum_k A[i sai + k sak] Bm[j sbj + k sbk] (+ bias[j]): the loss's logits / gradient products.  Routed through
    sc_sgemm_f32_ex so that the few-tile case (Bg = 64 per GPU: one 64 x 64 tile) is split along K over the chip."""
    assert A.dtype == torch.float32 and Bm.dtype == torch.float32
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    sgemm_ex(A, (sai, sak, 0), Bm, (sbj, sbk, 0), out, out.stride(0), M, N, K, alpha=alpha, bias=bias)
    return out


_INFONCE_WS = {}


def _infonce_workspace(Bg: int, device) -> torch.Tensor:
    """Per (device, stream, Bg) workspace of sc_infonce_fwd; zeroed once (it holds the ticket word, which every launch resets)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream, Bg)
    ws = _INFONCE_WS.get(key)
    if ws is None:
        ws = _INFONCE_WS[key] = torch.zeros(int(lib().sc_infonce_workspace_floats(Bg)), device=device, dtype=torch.float32)
    return ws


def infonce_fwd(A: torch.Tensor, Bm: torch.Tensor, ids: Optional[torch.Tensor], inv_temp: torch.Tensor, margin: float = 0.0,
                dcl: bool = False, a2b: bool = True, b2a: bool = True):
    """-> (loss [1], logits [Bg, Bg], lse_row [Bg], lse_col [Bg]); A, B [Bg, E] fp32 contiguous, inv_temp a device scalar tensor."""
    Bg, E = A.shape
    assert A.dtype == torch.float32 and Bm.dtype == torch.float32 and A.is_contiguous() and Bm.is_contiguous() and Bm.shape == A.shape
    assert inv_temp.dtype == torch.float32 and inv_temp.is_cuda and inv_temp.numel() == 1
    if ids is not None:
        assert ids.dtype == torch.int64 and ids.is_contiguous()
    A, Bm = aligned16(A), aligned16(Bm)
    dev = A.device
    logits = torch.empty(Bg, Bg, device=dev, dtype=torch.float32)
    lse_row, lse_col = torch.empty(Bg, device=dev, dtype=torch.float32), torch.empty(Bg, device=dev, dtype=torch.float32)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    ws = _infonce_workspace(Bg, dev)
    check(lib().sc_infonce_fwd(_p(A), _p(Bm), Bg, E, _p(ids), _p(inv_temp), float(margin), int(dcl), int(a2b), int(b2a), _p(logits),
                               _p(lse_row), _p(lse_col), _p(loss), _p(ws), _stream()), "sc_infonce_fwd")
    return loss, logits, lse_row, lse_col


def infonce_grad(logits: torch.Tensor, ids: Optional[torch.Tensor], lse_row: torch.Tensor, lse_col: torch.Tensor,
                 gscale: torch.Tensor, inv_temp: torch.Tensor, margin: float = 0.0, dcl: bool = False, a2b: bool = True,
                 b2a: bool = True):
    """-> (G [Bg, Bg] = inv_temp * gscale * dloss/dlogits, dot [Bg] with sum(dot) = d loss / d inv_temp * gscale)."""
    Bg = logits.shape[0]
    G = torch.empty_like(logits)
    dot = torch.empty(Bg, device=logits.device, dtype=torch.float32)
    check(lib().sc_infonce_grad(_p(logits), _p(ids), _p(lse_row), _p(lse_col), Bg, _p(gscale), _p(inv_temp), float(margin), int(dcl),
                                int(a2b), int(b2a), _p(G), _p(dot), _stream()), "sc_infonce_grad")
    return G, dot


NEG_MAX_M = 1024                   # the longest list per anchor (hard_negatives' own limit)


def neg_operands(name: str, A, bank, neg_idx, ids, bank_ids, a2b: bool = True) -> None:
    """The operands of the loss with a negative bank, checked before any launch, in ``search``'s order - format errors first, "device
    tensors only" last: ids on one side only; dtypes and shapes (A [Bg, E] / bank [N, E] fp32 with E % 4 == 0, neg_idx [Bg, M] int64,
    ids [Bg] / bank_ids [N] int64 contiguous); 1 <= M <= 1024; a2b; a bank that requires grad; the device."""
    if (ids is None) != (bank_ids is None):
        raise ValueError(f"{name}: ids on one side only - give the batch's ids and bank_ids, or neither")
    for what, t in (("A", A), ("bank", bank)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{name}: {what} must be a 2-D tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: {what} must be torch.float32, not {t.dtype}")
    Bg, E = A.shape
    N = bank.shape[0]
    if bank.shape[1] != E or E % 4 != 0 or E == 0:
        raise ValueError(f"{name}: A {tuple(A.shape)} and bank {tuple(bank.shape)} must share E, a multiple of 4")
    if N >= 2 ** 31:
        raise ValueError(f"{name}: the bank has {N} rows, at most 2^31 - 1 are served")
    if not isinstance(neg_idx, torch.Tensor):
        raise ValueError(f"{name}: neg_idx must be a tensor")
    if neg_idx.dtype != torch.int64:
        raise ValueError(f"{name}: neg_idx must be torch.int64, not {neg_idx.dtype}")
    if neg_idx.dim() != 2 or neg_idx.shape[0] != Bg:
        raise ValueError(f"{name}: neg_idx has shape {tuple(neg_idx.shape)}, expected ({Bg}, M)")
    if ids is not None:
        check_filter_tensor(name, "ids", ids, Bg)
        check_filter_tensor(name, "bank_ids", bank_ids, N)
    M = neg_idx.shape[1]
    if not 1 <= M <= NEG_MAX_M:
        raise ValueError(f"{name}: 1 <= M <= {NEG_MAX_M} (neg_idx has M = {M} slots per anchor)")
    if not a2b:
        raise ValueError(f"{name}: the extra negatives enter the a2b denominator - with a2b=False they have none to enter")
    if bank.requires_grad:
        raise ValueError(f"{name}: the bank is constant - it gets no gradient (bank.requires_grad is set)")
    given = [("A", A), ("bank", bank), ("neg_idx", neg_idx)] + ([("ids", ids), ("bank_ids", bank_ids)] if ids is not None else [])
    for what, t in given:
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on the HIP kernels: device tensors only ({what})")
    for what, t in given:
        if t.device != A.device:
            raise ValueError(f"{name}: {what} is on {t.device}, A on {A.device}")


def bank_rows(bank: torch.Tensor) -> torch.Tensor:
    """``bank`` as the kernels read it: rows of unit element stride at a row stride that is a multiple of 4 floats, 16-byte aligned (a
    row-strided view is read in place; anything else is copied once)"""
    N, E = bank.shape
    if not (bank.stride(1) == 1 and (N <= 1 or (bank.stride(0) % 4 == 0 and bank.stride(0) >= E))):
        bank = bank.contiguous()
    return aligned16(bank)


def infonce_neg_fwd(A: torch.Tensor, bank: torch.Tensor, neg_idx: torch.Tensor, ids: Optional[torch.Tensor], bank_ids: Optional[torch.Tensor],
                    inv_temp: torch.Tensor, lse_row: torch.Tensor, lse_col: torch.Tensor, logits: torch.Tensor, a2b: bool = True,
                    b2a: bool = True):
    """The plain call's a2b denominator extended by the bank rows ``neg_idx`` [Bg, M] names (sc_infonce_neg_fwd, csrc/infonce_neg.hip):
    ``lse_row`` / ``lse_col`` / ``logits`` are ``infonce_fwd``'s outputs for the same A, B, ids and options -> (loss [1], lse_row_ext [Bg],
    x [Bg, M] = inv_temp <A_i, bank[r]> with -inf where the slot takes no part, used [Bg] int32).  A slot takes part iff 0 <= r < N and,
    with ids, bank_ids[r] is the id of no batch row.  ``bank`` may be a row-strided view (read in place); a non-contiguous ``neg_idx`` is
    copied."""
    neg_operands("infonce_neg_fwd", A, bank, neg_idx, ids, bank_ids, a2b)
    Bg, E = A.shape
    N, M = bank.shape[0], neg_idx.shape[1]
    assert A.is_contiguous() and inv_temp.dtype == torch.float32 and inv_temp.is_cuda and inv_temp.numel() == 1
    assert logits.shape == (Bg, Bg) and logits.is_contiguous() and lse_row.shape == (Bg,) and lse_col.shape == (Bg,)
    assert logits.dtype == lse_row.dtype == lse_col.dtype == torch.float32 and lse_row.is_contiguous() and lse_col.is_contiguous()
    A, bank, neg_idx = aligned16(A), bank_rows(bank), neg_idx.contiguous()
    dev = A.device
    x = torch.empty(Bg, M, device=dev, dtype=torch.float32)
    used = torch.empty(Bg, device=dev, dtype=torch.int32)
    lse_ext = torch.empty(Bg, device=dev, dtype=torch.float32)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    ws_floats = int(lib().sc_infonce_neg_workspace_floats(Bg, M))
    if ws_floats < 0:
        check(ws_floats, "sc_infonce_neg_workspace_floats")
    ws = torch.empty(ws_floats, device=dev, dtype=torch.float32)
    check(lib().sc_infonce_neg_fwd(_p(A), _p(bank), bank.stride(0) if N > 1 else E, _p(neg_idx), _p(ids), _p(bank_ids), _p(inv_temp),
                                   _p(lse_row), _p(lse_col), _p(logits), Bg, E, N, M, int(a2b), int(b2a), _p(x), _p(used), _p(lse_ext),
                                   _p(loss), _p(ws), _stream()), "sc_infonce_neg_fwd")
    return loss, lse_ext, x, used


def infonce_neg_grad(A: torch.Tensor, bank: torch.Tensor, neg_idx: torch.Tensor, x: torch.Tensor, lse_row_ext: torch.Tensor,
                     gscale: torch.Tensor, inv_temp: torch.Tensor, a2b: bool, b2a: bool, dA: torch.Tensor, dot: torch.Tensor):
    """The extras' share of the gradient, accumulated IN PLACE (sc_infonce_neg_grad): ``dA`` [Bg, E] (holding G . B of ``infonce_grad``
    run on ``lse_row_ext``) += c inv_temp sum_n p_in bank[r_in] and ``dot`` [Bg] += c sum_n p_in x_in / inv_temp, p_in = e^{x_in -
    lse_row_ext_i}, c = gscale / (Bg n_dir).  ``x`` is ``infonce_neg_fwd``'s (its -inf entries are the empty slots).  -> (dA, dot)"""
    neg_operands("infonce_neg_grad", A, bank, neg_idx, None, None, a2b)
    Bg, E = A.shape
    N, M = bank.shape[0], neg_idx.shape[1]
    assert x.shape == (Bg, M) and x.dtype == torch.float32 and x.is_contiguous() and lse_row_ext.shape == (Bg,)
    assert dA.shape == (Bg, E) and dA.dtype == torch.float32 and dA.is_contiguous() and dot.shape == (Bg,) and dot.is_contiguous()
    bank, neg_idx = bank_rows(bank), neg_idx.contiguous()
    check(lib().sc_infonce_neg_grad(_p(bank), bank.stride(0) if N > 1 else E, _p(neg_idx), _p(x), _p(lse_row_ext), _p(gscale),
                                    _p(inv_temp), Bg, E, N, M, int(a2b), int(b2a), _p(dA), _p(dot), _stream()), "sc_infonce_neg_grad")
    return dA, dot


QUEUE_MAX_SCORES = 1 << 26         # scores [Bg, Nq] fp32 per side (256 MiB): csrc/infonce_queue.hip refuses more


def queue_operands(name: str, A, B, queue_A, queue_B, ids, queue_ids, a2b: bool = True, b2a: bool = True) -> None:
    """The operands of the loss with a cross-batch queue, checked before any launch, in ``neg_operands``' order - format errors first,
    "device tensors only" last: ids on one side only; dtypes and shapes (A, B [Bg, E] fp32 with E % 4 == 0); the queue of every enabled
    side given (``queue_B`` [Nq, E] for a2b, ``queue_A`` [Nq, E] for b2a; a queue for a side that is off is ignored) as a 2-D fp32 tensor
    of width E, both of one length; ids [Bg] / queue_ids [Nq] int64 contiguous; Bg Nq within QUEUE_MAX_SCORES; a queue that requires
    grad; the device."""
    if (ids is None) != (queue_ids is None):
        raise ValueError(f"{name}: ids on one side only - give the batch's ids and queue_ids, or neither")
    for what, t in (("A", A), ("B", B)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{name}: {what} must be a 2-D tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: {what} must be torch.float32, not {t.dtype}")
    Bg, E = A.shape
    if B.shape != A.shape or E % 4 != 0 or E == 0:
        raise ValueError(f"{name}: A {tuple(A.shape)} and B {tuple(B.shape)} must be one shape [Bg, E], E a multiple of 4")
    if not (a2b or b2a):
        raise ValueError(f"{name}: a2b and b2a are both off")
    queues = ([("queue_B", queue_B, "a2b")] if a2b else []) + ([("queue_A", queue_A, "b2a")] if b2a else [])
    for what, t, side in queues:
        if t is None:
            raise ValueError(f"{name}: {side} is on and {what} is missing - every enabled side needs its queue")
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{name}: {what} must be a 2-D tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: {what} must be torch.float32, not {t.dtype}")
        if t.shape[1] != E:
            raise ValueError(f"{name}: {what} {tuple(t.shape)} must share E = {E} with A")
    Nq = queues[0][1].shape[0]
    if len(queues) == 2 and queues[1][1].shape[0] != Nq:
        raise ValueError(f"{name}: queue_A has {queue_A.shape[0]} rows and queue_B {queue_B.shape[0]} - one ring position, one length")
    if ids is not None:
        check_filter_tensor(name, "ids", ids, Bg)
        check_filter_tensor(name, "queue_ids", queue_ids, Nq)
    if Bg * Nq > QUEUE_MAX_SCORES:
        raise ValueError(f"{name}: Bg Nq = {Bg} x {Nq} scores per side, at most 2^26 ({QUEUE_MAX_SCORES}, 256 MiB of fp32) are served")
    for what, t, _ in queues:
        if t.requires_grad:
            raise ValueError(f"{name}: the queue is constant - it gets no gradient ({what}.requires_grad is set)")
    given = [("A", A), ("B", B)] + [(w, t) for w, t, _ in queues] + ([("ids", ids), ("queue_ids", queue_ids)] if ids is not None else [])
    for what, t in given:
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on the HIP kernels: device tensors only ({what})")
    for what, t in given:
        if t.device != A.device:
            raise ValueError(f"{name}: {what} is on {t.device}, A on {A.device}")


def queue_scores(anchors: torch.Tensor, queue: torch.Tensor) -> torch.Tensor:
    """The raw dot products [Bg, Nq] of the anchors against the queue's rows on the exact-fp32 GEMM, as a view of a buffer whose rows
    are whole 16-byte pieces (leading dimension Nq rounded up to 4): what ``infonce_queue_fwd`` takes over."""
    Bg, Nq = anchors.shape[0], queue.shape[0]
    ldx = (Nq + 3) // 4 * 4
    x = torch.empty(Bg, ldx, device=anchors.device, dtype=torch.float32)[:, :Nq]
    if Bg and Nq:
        sgemm_mfma(anchors, bank_rows(queue), out=x)
    return x


def _queue_x(name: str, x: Optional[torch.Tensor], Bg: int, Nq: int):
    """-> the leading dimension of a score buffer (``queue_scores``' form)"""
    assert x.dtype == torch.float32 and x.dim() == 2 and tuple(x.shape) == (Bg, Nq), (name, tuple(x.shape), (Bg, Nq))
    ldx = x.stride(0)
    assert (x.stride(1) == 1 or Nq <= 1) and ldx >= Nq and ldx % 4 == 0 and x.data_ptr() % 16 == 0, f"{name}: rows of whole 16-byte pieces"
    assert x.untyped_storage().nbytes() - x.storage_offset() * 4 >= Bg * ldx * 4, f"{name}: the last row's pad columns lie outside the storage"
    return ldx


def infonce_queue_fwd(x_A: Optional[torch.Tensor], x_B: Optional[torch.Tensor], ids: Optional[torch.Tensor],
                      queue_ids: Optional[torch.Tensor], inv_temp: torch.Tensor, loss: torch.Tensor, lse_row: torch.Tensor,
                      lse_col: torch.Tensor, logits: torch.Tensor, E: int, a2b: bool = True, b2a: bool = True):
    """The plain call's denominators extended by a cross-batch queue (sc_infonce_queue_fwd, csrc/infonce_queue.hip).  ``x_A`` / ``x_B``
    [Bg, Nq] are ``queue_scores(A, queue_B)`` / ``queue_scores(B, queue_A)`` (the one of a side that is off may be None) and are
    rewritten IN PLACE: inv_temp x where the entry is admitted - no ids, or queue_ids[q] != ids[i] - and -inf elsewhere.  ``loss`` /
    ``lse_row`` / ``lse_col`` / ``logits`` are ``infonce_fwd``'s outputs for the same A, B, ids and options.
    -> (loss [1], lse_row_ext [Bg], lse_col_ext [Bg], used_A [Bg] int32, used_B [Bg] int32).  An empty queue or batch launches nothing
    and returns the plain statistics themselves."""
    Bg = logits.shape[0]
    assert (a2b or b2a) and (x_A is not None or not a2b) and (x_B is not None or not b2a)
    x_A, x_B = x_A if a2b else None, x_B if b2a else None
    Nq = (x_A if a2b else x_B).shape[1]
    if (ids is None) != (queue_ids is None):
        raise ValueError("infonce_queue_fwd: ids on one side only - give the batch's ids and queue_ids, or neither")
    if Bg * Nq > QUEUE_MAX_SCORES:
        raise ValueError(f"infonce_queue_fwd: Bg Nq = {Bg} x {Nq} scores per side, at most 2^26 ({QUEUE_MAX_SCORES}, 256 MiB of fp32) are served")
    assert inv_temp.dtype == torch.float32 and inv_temp.is_cuda and inv_temp.numel() == 1
    assert logits.shape == (Bg, Bg) and logits.is_contiguous() and lse_row.shape == (Bg,) and lse_col.shape == (Bg,)
    assert logits.dtype == lse_row.dtype == lse_col.dtype == torch.float32 and lse_row.is_contiguous() and lse_col.is_contiguous()
    dev = logits.device
    used_A, used_B = torch.zeros(Bg, device=dev, dtype=torch.int32), torch.zeros(Bg, device=dev, dtype=torch.int32)
    if Bg == 0 or Nq == 0:
        return loss, lse_row, lse_col, used_A, used_B
    ldx = [_queue_x("infonce_queue_fwd", x, Bg, Nq) for x in (x_A, x_B) if x is not None]
    assert len(set(ldx)) == 1, "infonce_queue_fwd: x_A and x_B of one leading dimension"
    if ids is not None:
        check_filter_tensor("infonce_queue_fwd", "ids", ids, Bg)
        check_filter_tensor("infonce_queue_fwd", "queue_ids", queue_ids, Nq)
    lse_row_ext, lse_col_ext = torch.empty_like(lse_row), torch.empty_like(lse_col)
    loss_ext = torch.empty(1, device=dev, dtype=torch.float32)
    ws_floats = int(lib().sc_infonce_queue_workspace_floats(Bg, Nq))
    if ws_floats < 0:
        check(ws_floats, "sc_infonce_queue_workspace_floats")
    ws = torch.empty(ws_floats, device=dev, dtype=torch.float32)
    check(lib().sc_infonce_queue_fwd(_p(x_A), _p(x_B), ldx[0], _p(ids), _p(queue_ids), _p(inv_temp), _p(lse_row), _p(lse_col), _p(logits), Bg,
                                     int(E), Nq, int(a2b), int(b2a), _p(lse_row_ext), _p(lse_col_ext), _p(used_A), _p(used_B), _p(loss_ext),
                                     _p(ws), _stream()), "sc_infonce_queue_fwd")
    return loss_ext, lse_row_ext, lse_col_ext, used_A, used_B


def infonce_queue_grad(x_A: Optional[torch.Tensor], x_B: Optional[torch.Tensor], lse_row_ext: torch.Tensor, lse_col_ext: torch.Tensor,
                       gscale: torch.Tensor, inv_temp: torch.Tensor, a2b: bool, b2a: bool, dot: torch.Tensor):
    """The extras' weights, IN PLACE (sc_infonce_queue_grad): ``x_A`` / ``x_B`` as ``infonce_queue_fwd`` left them become w = c inv_temp
    e^{x - lse_ext}, c = gscale / (Bg n_dir), exactly 0 where x was -inf - so dA += w_A . queue_B and dB += w_B . queue_A need no
    further scaling - and ``dot`` [Bg] (``infonce_grad``'s, run on the extended statistics) += c sum_q p x / inv_temp over both sides.
    -> (w_A, w_B, dot)"""
    Bg = lse_row_ext.shape[0]
    assert (a2b or b2a) and (x_A is not None or not a2b) and (x_B is not None or not b2a)
    x_A, x_B = x_A if a2b else None, x_B if b2a else None
    Nq = (x_A if a2b else x_B).shape[1]
    if Bg == 0 or Nq == 0:
        return x_A, x_B, dot
    ldx = [_queue_x("infonce_queue_grad", x, Bg, Nq) for x in (x_A, x_B) if x is not None]
    assert len(set(ldx)) == 1, "infonce_queue_grad: x_A and x_B of one leading dimension"
    assert lse_row_ext.shape == lse_col_ext.shape == dot.shape == (Bg,) and dot.dtype == torch.float32 and dot.is_contiguous()
    assert lse_row_ext.is_contiguous() and lse_col_ext.is_contiguous() and gscale.numel() == 1 and inv_temp.numel() == 1
    check(lib().sc_infonce_queue_grad(_p(x_A), _p(x_B), ldx[0], _p(lse_row_ext), _p(lse_col_ext), _p(gscale), _p(inv_temp), Bg, Nq, int(a2b),
                                      int(b2a), _p(dot), _stream()), "sc_infonce_queue_grad")
    return x_A, x_B, dot


_SUPCON_WS = {}
SUPCON_MAX_LOGIT_BYTES = DEFINES["SC_SUPCON_MAX_LOGIT_BYTES"]      # 1 GiB of logits [Na, N] fp32


def supcon_operands(name: str, C, Na: int, bsz: int, labels, mask, inv_temp=None) -> None:
    """The operands of the supervised contrastive loss, checked before any launch - format errors first, "device tensors only" last:
    C [N, E] fp32 with E % 4 == 0 and N a whole number of views of bsz samples; 0 <= Na <= N; labels [bsz] int64 or mask [bsz, bsz]
    fp32 (one of them or neither), contiguous; Na N 4 bytes of logits within SUPCON_MAX_LOGIT_BYTES; inv_temp a one-element fp32 tensor."""
    if not isinstance(C, torch.Tensor) or C.dim() != 2:
        raise ValueError(f"{name}: C must be a 2-D tensor")
    if C.dtype != torch.float32:
        raise ValueError(f"{name}: C must be torch.float32, not {C.dtype}")
    N, E = C.shape
    if E == 0 or E % 4 != 0:
        raise ValueError(f"{name}: C {tuple(C.shape)} must have E > 0, a multiple of 4")
    if not C.is_contiguous():
        raise ValueError(f"{name}: C must be contiguous")
    if bsz <= 0 or N % bsz != 0:
        raise ValueError(f"{name}: bsz {bsz} must be positive and divide the {N} rows of C (N = views x bsz)")
    if not 0 <= Na <= N:
        raise ValueError(f"{name}: Na {Na} must lie in 0 .. N = {N}")
    if labels is not None and mask is not None:
        raise ValueError(f"{name}: labels and mask are both given - one of them or neither")
    if labels is not None:
        check_filter_tensor(name, "labels", labels, bsz)
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.float32:
            raise ValueError(f"{name}: mask must be a torch.float32 tensor")
        if tuple(mask.shape) != (bsz, bsz) or not mask.is_contiguous():
            raise ValueError(f"{name}: mask has shape {tuple(mask.shape)}, expected a contiguous ({bsz}, {bsz})")
    if Na * N * 4 > SUPCON_MAX_LOGIT_BYTES:
        raise ValueError(f"{name}: the logits [{Na}, {N}] fp32 take {Na * N * 4} bytes, above the limit of {SUPCON_MAX_LOGIT_BYTES} (1 GiB)")
    if inv_temp is not None and (not isinstance(inv_temp, torch.Tensor) or inv_temp.dtype != torch.float32 or inv_temp.numel() != 1):
        raise ValueError(f"{name}: inv_temp must be a one-element torch.float32 tensor (a device scalar)")
    given = [("C", C)] + [(w, t) for w, t in (("labels", labels), ("mask", mask), ("inv_temp", inv_temp)) if t is not None]
    for what, t in given:
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on the HIP kernels: device tensors only ({what})")
    for what, t in given:
        if t.device != C.device:
            raise ValueError(f"{name}: {what} is on {t.device}, C on {C.device}")


def _supcon_workspace(Na: int, N: int, device) -> torch.Tensor:
    """Per (device, stream, Na, N) workspace of sc_supcon_fwd; zeroed once HERE (it ends in the ticket word, which every launch resets)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream, Na, N)
    ws = _SUPCON_WS.get(key)
    if ws is None:
        ws = _SUPCON_WS[key] = torch.zeros(int(lib().sc_supcon_workspace_floats(Na, N)), device=device, dtype=torch.float32)
    return ws


def supcon_fwd(C: torch.Tensor, Na: int, bsz: int, labels: Optional[torch.Tensor], mask: Optional[torch.Tensor], inv_temp: torch.Tensor,
               base_temperature: float = 0.07):
    """Supervised contrastive loss on the contrast rows C [N, E] = cat(unbind(features, 1), 0), anchors = rows 0 .. Na - 1 (sc_supcon_fwd,
    csrc/supcon.hip) -> (loss [1], logits [Na, N], lse [Na], possum [Na] = sum_j w_ij l_ij, poscnt [Na] = sum_j w_ij).  ``labels``
    [bsz] int64 or ``mask`` [bsz, bsz] fp32 or neither (the identity); ``inv_temp`` a device scalar tensor.  N = 0 or Na = 0 launches
    nothing (the loss of no anchor is NaN, as the mean of nothing)."""
    Na, bsz = int(Na), int(bsz)
    if float(base_temperature) == 0.0:
        raise ValueError("supcon_fwd: base_temperature is 0")
    supcon_operands("supcon_fwd", C, Na, bsz, labels, mask, inv_temp)
    C = aligned16(C)
    N, E = C.shape
    dev = C.device
    logits = torch.empty(Na, N, device=dev, dtype=torch.float32)
    lse, possum, poscnt = (torch.empty(Na, device=dev, dtype=torch.float32) for _ in range(3))
    if N == 0 or Na == 0:
        return torch.full((1,), float("nan"), device=dev), logits, lse, possum, poscnt
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    ws = _supcon_workspace(Na, N, dev)
    check(lib().sc_supcon_fwd(_p(C), N, Na, bsz, E, _p(labels), _p(mask), _p(inv_temp), float(base_temperature), _p(logits), _p(lse),
                              _p(possum), _p(poscnt), _p(loss), _p(ws), _stream()), "sc_supcon_fwd")
    return loss, logits, lse, possum, poscnt


def supcon_grad(logits: torch.Tensor, lse: torch.Tensor, poscnt: torch.Tensor, bsz: int, labels: Optional[torch.Tensor],
                mask: Optional[torch.Tensor], gscale: torch.Tensor, inv_temp: torch.Tensor, base_temperature: float = 0.07):
    """-> (G [Na, N] = inv_temp * gscale * dloss/dlogits, dot [Na] with sum(dot) = gscale * d loss / d inv_temp) from ``supcon_fwd``'s
    logits, lse and poscnt (sc_supcon_grad).  dC = [G . C ; 0] + G^T . C[:Na] on ``sgemm_mfma``."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("supcon_grad: logits must be a contiguous 2-D torch.float32 tensor")
    Na, N = logits.shape
    bsz = int(bsz)
    if bsz <= 0 or N % bsz != 0 or Na > N:
        raise ValueError(f"supcon_grad: logits {tuple(logits.shape)} must be [Na <= N, N] with bsz {bsz} > 0 dividing N")
    for what, t in (("lse", lse), ("poscnt", poscnt)):
        check_filter_tensor("supcon_grad", what, t, Na, (torch.float32,))
    for what, t in (("gscale", gscale), ("inv_temp", inv_temp)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1:
            raise ValueError(f"supcon_grad: {what} must be a one-element torch.float32 tensor (a device scalar)")
    if labels is not None and mask is not None:
        raise ValueError("supcon_grad: labels and mask are both given - one of them or neither")
    if labels is not None:
        check_filter_tensor("supcon_grad", "labels", labels, bsz)
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.float32 or tuple(mask.shape) != (bsz, bsz)
                             or not mask.is_contiguous()):
        raise ValueError(f"supcon_grad: mask must be a contiguous torch.float32 tensor of shape ({bsz}, {bsz})")
    if float(base_temperature) == 0.0:
        raise ValueError("supcon_grad: base_temperature is 0")
    for what, t in (("logits", logits), ("lse", lse), ("poscnt", poscnt), ("gscale", gscale), ("inv_temp", inv_temp), ("labels", labels),
                    ("mask", mask)):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"supcon_grad runs on the HIP kernels: device tensors only ({what})")
    G = torch.empty_like(logits)
    dot = torch.empty(Na, device=logits.device, dtype=torch.float32)
    if N > 0 and Na > 0:
        check(lib().sc_supcon_grad(_p(logits), _p(lse), _p(poscnt), N, Na, bsz, _p(labels), _p(mask), _p(gscale), _p(inv_temp),
                                   float(base_temperature), _p(G), _p(dot), _stream()), "sc_supcon_grad")
    return G, dot


_SIGMOID_WS = {}
SIGMOID_MAX_DOT_BYTES = 1 << 30    # 1 GiB of dots [B, B] fp32: csrc/sigmoid_loss.hip refuses more (its header holds prototypes only)
SIGMOID_SAME_ID = {"ignore": 0, "positive": 1, "negative": 2}     # what a same-id pair off the diagonal is: sc_sigmoid_loss_fwd's same_id


def sigmoid_loss_operands(name: str, A, B, ids, same_id, half_ok: bool = False) -> int:
    """The operands of the pairwise sigmoid loss, checked before any launch in ``neg_operands``' order - format errors first, "device
    tensors only" last: dtypes and shapes of the batch (A, B 2-D fp32 - with ``half_ok`` also fp16 / bf16, which the module widens -
    with at least one row and E % 4 == 0); A and B of one shape; ids [B] int64 contiguous; the mode string; B B 4 bytes of dots within
    SIGMOID_MAX_DOT_BYTES; the device.  -> the mode as sc_sigmoid_loss_fwd takes it."""
    dtypes = (torch.float32, torch.float16, torch.bfloat16) if half_ok else (torch.float32,)
    for what, t in (("A", A), ("B", B)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{name}: {what} must be a 2-D tensor")
        if t.dtype not in dtypes:
            raise ValueError(f"{name}: {what} must be {' or '.join(str(d) for d in dtypes)}, not {t.dtype}")
    Bg, E = A.shape
    if Bg < 1 or E == 0 or E % 4 != 0:
        raise ValueError(f"{name}: A {tuple(A.shape)} must have at least one row and E > 0, a multiple of 4")
    if A.shape != B.shape:
        raise ValueError(f"{name}: A {tuple(A.shape)} and B {tuple(B.shape)} must be one shape [B, E]")
    if ids is not None:
        check_filter_tensor(name, "ids", ids, Bg)
    if not isinstance(same_id, str) or same_id not in SIGMOID_SAME_ID:
        raise ValueError(f"{name}: same_id {same_id!r} is none of {', '.join(repr(k) for k in SIGMOID_SAME_ID)}")
    if Bg * Bg * 4 > SIGMOID_MAX_DOT_BYTES:
        raise ValueError(f"{name}: the dots [{Bg}, {Bg}] fp32 take {Bg * Bg * 4} bytes, above the limit of {SIGMOID_MAX_DOT_BYTES} (1 GiB)")
    given = [("A", A), ("B", B)] + ([("ids", ids)] if ids is not None else [])
    for what, t in given:
        if not t.is_cuda:
            raise RuntimeError(f"{name} runs on the HIP kernels: device tensors only ({what})")
    for what, t in given:
        if t.device != A.device:
            raise ValueError(f"{name}: {what} is on {t.device}, A on {A.device}")
    return SIGMOID_SAME_ID[same_id]


def _sigmoid_scalars(name: str, dev, **scalars) -> None:
    for what, t in scalars.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1:
            raise ValueError(f"{name}: {what} must be a one-element torch.float32 tensor (a device scalar)")
    for what, t in scalars.items():
        if not t.is_cuda or t.device != dev:
            raise RuntimeError(f"{name} runs on the HIP kernels: device tensors only ({what}), on the operands' device")


def _sigmoid_workspace(Bg: int, device) -> torch.Tensor:
    """Per (device, stream, B) workspace of sc_sigmoid_loss_fwd; zeroed once HERE (it ends in the ticket word, which every launch resets)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream, Bg)
    ws = _SIGMOID_WS.get(key)
    if ws is None:
        ws = _SIGMOID_WS[key] = torch.zeros(int(lib().sc_sigmoid_loss_workspace_floats(Bg)), device=device, dtype=torch.float32)
    return ws


def sigmoid_loss_fwd(A: torch.Tensor, Bm: torch.Tensor, ids: Optional[torch.Tensor], scale: torch.Tensor, bias: torch.Tensor,
                     same_id: str = "ignore"):
    """Pairwise sigmoid loss of the batch (sc_sigmoid_loss_fwd, csrc/sigmoid_loss.hip) -> (loss [1], s [B, B] the RAW dots <A_i, B_j>,
    counts [3] int32 = positives, negatives, ignored).  A, B [B, E] fp32 contiguous unit rows; ``scale`` = t > 0 and ``bias`` = b
    one-element device tensors (x = t s + b); ``same_id``: what an off-diagonal pair of equal ids is - "ignore", "positive", "negative"."""
    mode = sigmoid_loss_operands("sigmoid_loss_fwd", A, Bm, ids, same_id)
    if not A.is_contiguous() or not Bm.is_contiguous():
        raise ValueError("sigmoid_loss_fwd: A and B must be contiguous")
    _sigmoid_scalars("sigmoid_loss_fwd", A.device, scale=scale, bias=bias)
    A, Bm = aligned16(A), aligned16(Bm)
    Bg, E = A.shape
    dev = A.device
    s = torch.empty(Bg, Bg, device=dev, dtype=torch.float32)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    counts = torch.empty(3, device=dev, dtype=torch.int32)
    ws = _sigmoid_workspace(Bg, dev)
    check(lib().sc_sigmoid_loss_fwd(_p(A), _p(Bm), Bg, E, _p(ids), mode, _p(scale), _p(bias), _p(s), _p(loss), _p(counts), _p(ws),
                                    _stream()), "sc_sigmoid_loss_fwd")
    return loss, s, counts


def sigmoid_loss_grad(s: torch.Tensor, ids: Optional[torch.Tensor], gscale: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor,
                      same_id: str = "ignore"):
    """-> (G [B, B] = gscale t dloss/dx, exactly 0 where a pair is ignored; dscale_part [B], dbias_part [B] with sum(dscale_part) =
    gscale d loss / d t and sum(dbias_part) = gscale d loss / d b) from ``sigmoid_loss_fwd``'s dots (sc_sigmoid_loss_grad).
    dA = G . B and dB = G^T . A on ``sgemm_mfma``."""
    if not isinstance(s, torch.Tensor) or s.dim() != 2 or s.dtype != torch.float32 or not s.is_contiguous() or s.shape[0] != s.shape[1] \
            or s.shape[0] < 1:
        raise ValueError("sigmoid_loss_grad: s must be a contiguous square 2-D torch.float32 tensor with at least one row")
    Bg = s.shape[0]
    if ids is not None:
        check_filter_tensor("sigmoid_loss_grad", "ids", ids, Bg)
    if not isinstance(same_id, str) or same_id not in SIGMOID_SAME_ID:
        raise ValueError(f"sigmoid_loss_grad: same_id {same_id!r} is none of {', '.join(repr(k) for k in SIGMOID_SAME_ID)}")
    if Bg * Bg * 4 > SIGMOID_MAX_DOT_BYTES:
        raise ValueError(f"sigmoid_loss_grad: the dots [{Bg}, {Bg}] fp32 take {Bg * Bg * 4} bytes, above the limit of "
                         f"{SIGMOID_MAX_DOT_BYTES} (1 GiB)")
    for what, t in (("s", s), ("ids", ids)):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"sigmoid_loss_grad runs on the HIP kernels: device tensors only ({what})")
    _sigmoid_scalars("sigmoid_loss_grad", s.device, gscale=gscale, scale=scale, bias=bias)
    G = torch.empty_like(s)
    dscale_part, dbias_part = (torch.empty(Bg, device=s.device, dtype=torch.float32) for _ in range(2))
    check(lib().sc_sigmoid_loss_grad(_p(s), Bg, _p(ids), SIGMOID_SAME_ID[same_id], _p(gscale), _p(scale), _p(bias), _p(G), _p(dscale_part),
                                     _p(dbias_part), _stream()), "sc_sigmoid_loss_grad")
    return G, dscale_part, dbias_part


def sumsq(x: torch.Tensor, nblk: int = 1024) -> torch.Tensor:
    part = torch.empty(nblk, device=x.device, dtype=torch.float32)
    check(lib().sc_sumsq_f32(_p(x), x.numel(), _p(part), nblk, _stream()), "sc_sumsq_f32")
    return part


def adam_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, lr: float, beta1: float, beta2: float,
              eps: float, weight_decay: float, step: int, gn_partial: Optional[torch.Tensor], max_norm: float) -> None:
    nblk = gn_partial.numel() if gn_partial is not None else 0
    # the betas cross as doubles: 1 - beta and the bias corrections are formed in double on the host side of the entry point
    check(lib().sc_adam_f32(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, float(beta1), float(beta2), eps, weight_decay, step,
                            _p(gn_partial), nblk, max_norm, _stream()), "sc_adam_f32")


# ---- fp32 one-row-per-utterance head tail (csrc/headtail.hip) ------------------------------------------------------
_SPLITK_WS = {}


def _splitk_workspace(device) -> torch.Tensor:
    """Scratch for split-K partial sums, one buffer per (device, stream): calls on one stream are serialised, calls on different
    streams (the head's parameter-only backward half, the trainer's prefetch) must not share it."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _SPLITK_WS.get(key)
    if ws is None:
        ws = _SPLITK_WS[key] = torch.empty(8 << 20, device=device, dtype=torch.float32)
    return ws


def sgemm_ex(A: torch.Tensor, sa, Bm: torch.Tensor, sb, C: torch.Tensor, ldc: int, M: int, N: int, K: int, nbatch: int = 1,
             scz: int = 0, alpha: float = 1.0, beta: float = 0.0, bias: Optional[torch.Tensor] = None, sbiasz: int = 0) -> None:
    """C[z][i,j] = alpha sum_k A[z][i*sa0 + k*sa1] Bm[z][j*sb0 + k*sb1] (+ bias[z][j]) + beta C[z][i,j];
    sa / sb = (row stride, k stride, batch stride) in elements; pointers are the tensors' data_ptr()."""
    assert A.dtype == torch.float32 and Bm.dtype == torch.float32 and C.dtype == torch.float32
    ws = _splitk_workspace(A.device)
    check(lib().sc_sgemm_f32_ex(_p(A), sa[0], sa[1], sa[2], _p(Bm), sb[0], sb[1], sb[2], _p(C), ldc, scz, M, N, K, nbatch,
                                float(alpha), float(beta), _p(bias), sbiasz, _p(ws), ws.numel(), _stream()), "sc_sgemm_f32_ex")


def rowln_fwd(x: torch.Tensor, res: Optional[torch.Tensor], res_stride: int, gamma: torch.Tensor, beta: torch.Tensor, eps: float):
    rows, D = x.shape
    y, xhat = torch.empty_like(x), torch.empty_like(x)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    check(lib().sc_rowln_f32_fwd(_p(x), _p(res), res_stride, _p(gamma), _p(beta), _p(y), _p(xhat), _p(rstd), rows, D, float(eps),
                                 _stream()), "sc_rowln_f32_fwd")
    return y, xhat, rstd


def rowln_bwd(dy: torch.Tensor, xhat: torch.Tensor, gamma: torch.Tensor, rstd: torch.Tensor, dgamma_acc: torch.Tensor,
              dbeta_acc: torch.Tensor) -> torch.Tensor:
    rows, D = dy.shape
    dx = torch.empty_like(dy)
    check(lib().sc_rowln_f32_bwd(_p(dy), _p(xhat), _p(gamma), _p(rstd), _p(dx), _p(dgamma_acc), _p(dbeta_acc), rows, D, _stream()),
          "sc_rowln_f32_bwd")
    return dx


def gelu_f32(u: torch.Tensor, df: Optional[torch.Tensor] = None) -> torch.Tensor:
    out = torch.empty_like(u)
    check(lib().sc_gelu_f32(_p(u), _p(df), _p(out), u.numel(), _stream()), "sc_gelu_f32")
    return out


def colsum(x: torch.Tensor, ld: int, rows: int, cols: int, out: torch.Tensor, alpha: float = 1.0, beta: float = 0.0) -> None:
    check(lib().sc_colsum_f32(_p(x), ld, rows, cols, _p(out), float(alpha), float(beta), _stream()), "sc_colsum_f32")


def headmask(q: torch.Tensor, Qm: torch.Tensor, H: int, D: int, dh: int, gather: bool) -> None:
    check(lib().sc_headmask_f32(_p(q), _p(Qm), H, D, dh, int(gather), _stream()), "sc_headmask_f32")


# ---------------------------------------------------------------------------------------------- row tail of the head (csrc/rowtail.hip)
class Slices:
    """A [rows, cols] fp32 matrix given as ``ns`` partial slices [ns, rows, cols] that its consumer adds in order (a split product of
    sc_rt_gemm; ns = 1: an ordinary matrix)."""

    def __init__(self, t: torch.Tensor):
        assert t.dim() == 3 and t.dtype == torch.float32 and t.is_contiguous()
        self.t, self.ns, self.rows, self.cols = t, t.shape[0], t.shape[1], t.shape[2]

    def total(self) -> torch.Tensor:          # (tests / debugging: the consumer kernels never materialise this)
        return self.t.sum(0)


def rt_gemm(A, Bm: torch.Tensor, M: int, N: int, K: int, *, a_kmajor: bool = False, b_kmajor: bool = False, lda: Optional[int] = None,
            ldb: Optional[int] = None, a_bias: Optional[torch.Tensor] = None, a_rowscale: Optional[torch.Tensor] = None, a_group: int = 1,
            split: bool = False, out: Optional[torch.Tensor] = None, ldc: Optional[int] = None, alpha: float = 1.0, beta: float = 0.0,
            bias: Optional[torch.Tensor] = None, act: int = 0, U: Optional[torch.Tensor] = None, drop_p: float = 0.0, drop_seed: int = 0,
            gb: Optional[torch.Tensor] = None, nbatch: int = 1, a_z: int = 0, b_z: int = 0, c_z: int = 0, bias_z: int = 0, gb_z: int = 0):
    """C = epi(alpha A . B^T) (sc_rt_gemm).  ``A``: a tensor or ``Slices`` (row-major [M, K]; or [K, M] with a_kmajor), ``Bm`` [N, K] (or
    [K, N] with b_kmajor).  ``split`` = True: the contraction is split over the chip and a ``Slices`` of raw partial products comes back
    (its consumer adds them, with the bias); otherwise the epilogue runs and the [M, N] result (``out`` or a fresh tensor) is returned."""
    a = RtGemmArgs()
    if isinstance(A, Slices):
        assert not a_kmajor
        a.A, a.a_ns, a.a_slice = _p(A.t), A.ns, A.rows * A.cols
        lda = A.cols if lda is None else lda
    else:
        assert A.dtype == torch.float32
        a.A, a.a_ns, a.a_slice = _p(A), 1, 0
        lda = A.stride(0) if lda is None else lda
    assert Bm.dtype == torch.float32
    a.lda, a.a_z, a.a_kmajor = int(lda), int(a_z), int(a_kmajor)
    a.a_bias, a.a_rowscale, a.a_group = _p(a_bias), _p(a_rowscale), int(a_group)
    a.a_nscale = int(a_rowscale.shape[-1]) if a_rowscale is not None else 0
    a.B, a.ldb, a.b_z, a.b_kmajor, a.nbatch = _p(Bm), int(Bm.stride(0) if ldb is None else ldb), int(b_z), int(b_kmajor), int(nbatch)
    a.M, a.N, a.K = int(M), int(N), int(K)
    a.alpha, a.beta = float(alpha), float(beta)
    dev = Bm.device
    if split:
        S = int(lib().sc_rt_gemm_slices(M, N, K, nbatch))
        assert nbatch == 1 or c_z > 0
        res = torch.empty(S, M, N if nbatch == 1 else ldc, device=dev, dtype=torch.float32)
        a.C, a.ldc, a.c_slice, a.c_z, a.S = _p(res), res.shape[2], M * res.shape[2], int(c_z), S
        check(lib().sc_rt_gemm(ctypes.byref(a), _stream()), "sc_rt_gemm")
        return Slices(res)
    if out is None:
        out = torch.empty(M, N, device=dev, dtype=torch.float32)
    a.C, a.ldc, a.c_slice, a.c_z, a.S = _p(out), int(out.stride(0) if ldc is None else ldc), 0, int(c_z), 1
    a.U = _p(U)
    a.bias, a.bias_z, a.act = _p(bias), int(bias_z), int(act)
    a.drop_p, a.drop_seed = float(drop_p), int(drop_seed) & 0xffffffff
    a.gb, a.gb_z = _p(gb), int(gb_z)
    check(lib().sc_rt_gemm(ctypes.byref(a), _stream()), "sc_rt_gemm")
    return out


def rt_ln_fwd(y: Slices, bias, res, res_stride: int, g1, b1, eps1: float, g2=None, b2=None, eps2: float = 0.0, drop_p: float = 0.0,
              drop_seed: int = 0):
    """z = (sum_s y_s + bias) * dropout + res ; LN1 [; LN2] -> (out1, xhat1, rstd1[, out2, xhat2, rstd2])."""
    rows, D = y.rows, y.cols
    dev = y.t.device
    f = lambda *sh: torch.empty(*sh, device=dev, dtype=torch.float32)
    a = RtLnArgs()
    a.y, a.y_slice, a.ns, a.rows, a.D = _p(y.t), rows * D, y.ns, rows, D
    a.bias, a.drop_p, a.drop_seed = _p(bias), float(drop_p), int(drop_seed) & 0xffffffff
    a.res, a.res_stride = _p(res), int(res_stride)
    o1, h1, r1 = f(rows, D), f(rows, D), f(rows)
    a.g1, a.b1, a.eps1, a.out1, a.xhat1, a.rstd1 = _p(g1), _p(b1), float(eps1), _p(o1), _p(h1), _p(r1)
    outs = (o1, h1, r1)
    if g2 is not None:
        o2, h2, r2 = f(rows, D), f(rows, D), f(rows)
        a.g2, a.b2, a.eps2, a.out2, a.xhat2, a.rstd2 = _p(g2), _p(b2), float(eps2), _p(o2), _p(h2), _p(r2)
        outs = outs + (o2, h2, r2)
    check(lib().sc_rt_ln_fwd(ctypes.byref(a), _stream()), "sc_rt_ln_fwd")
    return outs


def rt_ln_bwd(dy: Slices, add, xhat, gamma, rstd, dgamma_acc, dbeta_acc, want_masked: bool = False, drop_p: float = 0.0, drop_seed: int = 0):
    """LayerNorm backward over a sliced incoming gradient (+ ``add``); returns dx (and dx * dropout multiplier when asked)."""
    rows, D = dy.rows, dy.cols
    a = RtLnBwdArgs()
    dx = torch.empty(rows, D, device=dy.t.device, dtype=torch.float32)
    dxm = torch.empty_like(dx) if want_masked else None
    a.dy, a.dy_slice, a.ns, a.rows, a.D = _p(dy.t), rows * D, dy.ns, rows, D
    a.add, a.xhat, a.gamma, a.rstd, a.dx, a.dx_masked = _p(add), _p(xhat), _p(gamma), _p(rstd), _p(dx), _p(dxm)
    a.drop_p, a.drop_seed, a.dgamma, a.dbeta = float(drop_p), int(drop_seed) & 0xffffffff, _p(dgamma_acc), _p(dbeta_acc)
    check(lib().sc_rt_ln_bwd(ctypes.byref(a), _stream()), "sc_rt_ln_bwd")
    return (dx, dxm) if want_masked else dx


def rt_l2norm_fwd(y: Slices, bias, keep_x: bool = True):
    """x = sum_s y_s + bias ; e = x / |x| -> (x or None, e, 1 / |x|)."""
    rows, D = y.rows, y.cols
    dev = y.t.device
    x = torch.empty(rows, D, device=dev, dtype=torch.float32) if keep_x else None
    e = torch.empty(rows, D, device=dev, dtype=torch.float32)
    rn = torch.empty(rows, device=dev, dtype=torch.float32)
    check(lib().sc_rt_l2norm_fwd(_p(y.t), rows * D, y.ns, _p(bias), _p(x), _p(e), _p(rn), rows, D, _stream()), "sc_rt_l2norm_fwd")
    return x, e, rn


def rt_l2norm_bwd(g: torch.Tensor, e: torch.Tensor, rn: torch.Tensor) -> torch.Tensor:
    rows, D = e.shape
    dx = torch.empty_like(e)
    g = g.float().contiguous()
    check(lib().sc_rt_l2norm_bwd(_p(g), _p(e), _p(rn), _p(dx), rows, D, _stream()), "sc_rt_l2norm_bwd")
    return dx


def rt_elem(y: Slices, mode: int, bias=None, rowscale=None, group: int = 1, u: Optional[torch.Tensor] = None, drop_p: float = 0.0,
            drop_seed: int = 0):
    """mode 0: sum_s y_s + bias * rowscale -> out ; 1: -> (u, gelu(u) * dropout) ; 2: (sum_s y_s) * dropout * gelu'(u) -> out."""
    rows, D = y.rows, y.cols
    out = torch.empty(rows, D, device=y.t.device, dtype=torch.float32)
    if mode == 1:
        u = torch.empty_like(out)
    nscale = int(rowscale.shape[-1]) if rowscale is not None else 0
    check(lib().sc_rt_elem(_p(y.t), rows * D, y.ns, _p(bias), _p(rowscale), int(group), nscale, _p(out), _p(u), rows, D, int(mode), float(drop_p),
                           int(drop_seed) & 0xffffffff, _stream()), "sc_rt_elem")
    return (u, out) if mode == 1 else out


def rt_value_bias_bwd(dctx: torch.Tensor, bv: torch.Tensor, psum: torch.Tensor, gbv_acc: torch.Tensor, H: int) -> torch.Tensor:
    """-> cbias [B,H] = sum_j dctx[b,h,j] bv[h,j] ; gbv_acc[h,j] += sum_b dctx[b,h,j] psum[b,h]  (one launch)"""
    B, D = dctx.shape
    cb = torch.empty(B, H, device=dctx.device, dtype=torch.float32)
    check(lib().sc_rt_value_bias_bwd(_p(dctx), _p(bv), _p(psum), _p(cb), _p(gbv_acc), B, D, H, _stream()), "sc_rt_value_bias_bwd")
    return cb


def wsum_bwd_logits(h: torch.Tensor, g: torch.Tensor, w_soft: torch.Tensor, B: int, R: int, D: int, row_off: int, nblk: int = 1024,
                    normalize: bool = False, lazy: Optional[LazyStates] = None, seg: Optional["RowSegments"] = None) -> torch.Tensor:
    """Gradient of the weighted-sum LOGITS in two launches: the partial sums <g, h_n - h_last> per block (sc_wsum_bwd) and their
    reduction fused with the softmax backward w_n (d_n - sum_m w_m d_m) (sc_rt_softmax_bwd_reduce)."""
    NL = h.shape[0]
    assert g.dtype in (torch.float32, torch.bfloat16) and g.is_contiguous()      # bf16: as the attention block's GEMM wrote it
    flags = int(normalize) | (2 if g.dtype == torch.bfloat16 else 0)
    part = torch.empty(nblk, NL, device=h.device, dtype=torch.float32)
    if seg is not None:
        assert lazy is None and h.shape[1] == seg.rows and B == seg.B
    if lazy is not None:
        assert not normalize
        if g.dtype != torch.float32:
            g = g.float()
        check(lib().sc_wsum_lazy_bwd(_p(h), _p(g), NL, _p(part), nblk, B, R, D, row_off, _p(lazy.stats), _p(lazy.gamma), _p(lazy.beta),
                                     lazy.first_lazy, lazy.ns, lazy.eps, _stream()), "sc_wsum_lazy_bwd")
    else:
        check(lib().sc_wsum_bwd(_p(h), _p(g), NL, _p(part), nblk, _seg(seg), B, R, D, row_off, flags, _stream()), "sc_wsum_bwd")
    out = torch.empty(NL, device=h.device, dtype=torch.float32)
    check(lib().sc_rt_softmax_bwd_reduce(_p(part), nblk, NL, _p(w_soft), _p(out), _stream()), "sc_rt_softmax_bwd_reduce")
    return out


def cif_head_fwd(y: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, p1: float, seed1: int, p2: float, seed2: int) -> torch.Tensor:
    """alpha [rows] = sigmoid(bias + sum_c w[c] m2 relu(m1 y[row, c]))  (sc_cif_head_fwd; y [rows, C] fp32 contiguous)"""
    rows, C = y.shape
    alpha = torch.empty(rows, device=y.device, dtype=torch.float32)
    check(lib().sc_cif_head_fwd(_p(y), y.stride(0), _p(w), _p(bias), _p(alpha), rows, C, float(p1), int(seed1) & 0xffffffff, float(p2),
                                int(seed2) & 0xffffffff, _stream()), "sc_cif_head_fwd")
    return alpha


def cif_head_bwd(y: torch.Tensor, w: torch.Tensor, alpha: torch.Tensor, dalpha: torch.Tensor, p1: float, seed1: int, p2: float, seed2: int,
                 nblk: int = 512, dy_out: Optional[torch.Tensor] = None, acc=None):
    """-> dy [rows, C], dw [C], db [1]; ``acc`` = (gw, gb) fp32 gradient buffers of C and 1 elements the two reductions ADD into
    (-> dy, None, None)"""
    rows, C = y.shape
    dy = torch.empty_like(y) if dy_out is None else dy_out             # dy_out: bf16 [rows, C] rows (what the conv's dgrad GEMM reads)
    assert dy.dtype in (torch.float32, torch.bfloat16) and dy.stride(1) == 1 and tuple(dy.shape) == (rows, C)
    pw = torch.empty(nblk, C, device=y.device, dtype=torch.float32)
    pb = torch.empty(nblk, device=y.device, dtype=torch.float32)
    check(lib().sc_cif_head_bwd_rows(_p(y), y.stride(0), _p(w), _p(alpha), _p(dalpha), _p(dy), int(dy.dtype == torch.bfloat16), dy.stride(0), _p(pw),
                                     _p(pb), nblk, rows, C, float(p1), int(seed1) & 0xffffffff, float(p2), int(seed2) & 0xffffffff, _stream()),
          "sc_cif_head_bwd")
    if acc is not None:
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in acc) and acc[0].numel() == C and acc[1].numel() == 1
        colsum(pw, C, nblk, C, acc[0], beta=1.0)
        colsum(pb.view(nblk, 1), 1, nblk, 1, acc[1], beta=1.0)
        return dy, None, None
    dw = torch.empty(C, device=y.device, dtype=torch.float32)
    db = torch.empty(1, device=y.device, dtype=torch.float32)
    colsum(pw, C, nblk, C, dw)
    colsum(pb.view(nblk, 1), 1, nblk, 1, db)
    return dy, dw, db


def conv_overlap_add(dcols: torch.Tensor, C: int, u: Optional[torch.Tensor] = None, act: int = 1) -> torch.Tensor:
    """dcols [M, 3C] bf16 (window gradients of a k = 3 / stride 2 conv) -> input-row gradients [2M, C] bf16 (sc_conv_overlap_add_bf16);
    ``u`` [2M, C] bf16: also through the activation below, dx * act'(u) (sc_conv_overlap_add_act_bf16)"""
    M = dcols.shape[0]
    assert dcols.dtype == torch.bfloat16 and dcols.is_contiguous() and dcols.shape[1] == 3 * C
    dx = torch.empty(2 * M, C, device=dcols.device, dtype=torch.bfloat16)
    if u is not None:
        assert u.dtype == torch.bfloat16 and u.is_contiguous() and u.numel() >= 2 * M * C
        check(lib().sc_conv_overlap_add_act_bf16(_p(dcols), _p(u), _p(dx), M, C, int(act), _stream()), "sc_conv_overlap_add_act_bf16")
    else:
        check(lib().sc_conv_overlap_add_bf16(_p(dcols), _p(dx), M, C, _stream()), "sc_conv_overlap_add_bf16")
    return dx


# ---- keyword prompt of the cascaded branches in the text tower's packed rows (csrc/prompt.hip) ------------------------------------------
def prompt_assemble(keywords: torch.Tensor, count: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, Bp: int, SEG: int, n_pos: int,
                    clamped: Optional[torch.Tensor] = None):
    """keywords [B, N, W] fp32 (last two dims dense), count [B] int64, tok [3, W] (SOT, EOT, token 0), pos [>= n_pos, W] ->
    X [Bp * SEG, W] bf16 (prefix rows of [SOT, kw.., EOT, 0..] + pos; zero elsewhere), eot_row [B] int32 (rows of X)"""
    B, N, W = keywords.shape
    assert keywords.dtype == torch.float32 and keywords.stride(2) == 1 and (N == 0 or keywords.stride(1) == W)
    assert count.dtype == torch.int64 and count.is_contiguous() and tok.dtype == torch.float32 and tok.is_contiguous() and tuple(tok.shape) == (3, W)
    assert pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[0] >= n_pos and pos.shape[1] == W
    X = torch.empty(Bp * SEG, W, device=keywords.device, dtype=torch.bfloat16)
    eot_row = torch.empty(B, device=keywords.device, dtype=torch.int32)
    check(lib().sc_prompt_assemble(_p(keywords), keywords.stride(0) if B > 1 else N * W, _p(count), _p(tok), _p(pos), _p(X), _p(eot_row),
                                   _p(clamped), B, Bp, N, W, SEG, n_pos, _stream()), "sc_prompt_assemble")
    return X, eot_row


def text_assemble(ids: torch.Tensor, table: torch.Tensor, pos: torch.Tensor, Bp: int, SEG: int, n_pos: int, out: Optional[torch.Tensor] = None,
                  bad: Optional[torch.Tensor] = None):
    """ids [B, L <= 77] int64 (unit column stride, any row stride), table [V, W] fp32 (rows dense), pos [>= n_pos, W] fp32 ->
    X [Bp * SEG, W] bf16 (rows b SEG + t = table[ids[b, t]] + pos[t] for t < n_pos; zero elsewhere), eot_row [B] int32 (rows of X at the
    first position of each caption's largest id, clamped to n_pos - 1), bad [1] int64 (clamps + ids outside [0, V), which embed as
    zero) - sc_text_assemble.  ``out``: X's storage; ``bad``: a counter to add to instead of a fresh zero."""
    B, L = ids.shape
    V, W = table.shape
    assert ids.dtype == torch.int64 and ids.stride(1) == 1 and (B == 1 or ids.stride(0) >= L)
    assert table.dtype == torch.float32 and table.stride(1) == 1 and table.stride(0) >= W
    assert pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[0] >= n_pos and pos.shape[1] == W
    if out is None:
        out = torch.empty(Bp * SEG, W, device=ids.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (Bp * SEG, W)
    eot_row = torch.empty(B, device=ids.device, dtype=torch.int32)
    if bad is None:
        bad = torch.zeros(1, device=ids.device, dtype=torch.int64)
    assert bad.dtype == torch.int64 and bad.numel() == 1
    check(lib().sc_text_assemble(_p(ids), ids.stride(0) if B > 1 else L, _p(table), table.stride(0), _p(pos), _p(out), _p(eot_row), _p(bad),
                                 B, Bp, L, V, W, SEG, n_pos, _stream()), "sc_text_assemble")
    return out, eot_row, bad


def prompt_assemble_bwd(dX: torch.Tensor, count: torch.Tensor, B: int, N: int, SEG: int, n_pos: int) -> torch.Tensor:
    """dX [>= B * SEG, W] bf16 -> dkeywords [B, N, W] fp32 (rows behind a sample's keyword count: zero)"""
    W = dX.shape[1]
    assert dX.dtype == torch.bfloat16 and dX.is_contiguous()
    dk = torch.empty(B, N, W, device=dX.device, dtype=torch.float32)
    if N > 0:
        check(lib().sc_prompt_assemble_bwd(_p(dX), _p(count), _p(dk), N * W, B, N, W, SEG, n_pos, _stream()), "sc_prompt_assemble_bwd")
    return dk


def rows_gather(X: torch.Tensor, row: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b] = float(X[row[b]]): X [M, W] bf16 contiguous, row [B] int32"""
    assert X.dtype == torch.bfloat16 and X.is_contiguous() and row.dtype == torch.int32
    if out is None:
        out = torch.empty(row.numel(), X.shape[1], device=X.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (row.numel(), X.shape[1])
    check(lib().sc_rows_gather_bf16(_p(X), _p(row), _p(out), row.numel(), X.shape[1], _stream()), "sc_rows_gather_bf16")
    return out


def vit_patchify(images: torch.Tensor, seg: "RowSegments", P: int, Kp: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A [seg.rows, Kp] bf16: the patch GEMM's operand of CLIP's conv1 (sc_vit_patchify_bf16).  images: fp32 [B, 3, S, S] on the
    device whose pixel rows are contiguous (any batch / channel / row stride); class, pad rows and columns >= 3 P^2 are zero."""
    assert images.dtype == torch.float32 and images.dim() == 4 and images.shape[1] == 3 and images.stride(3) == 1
    assert images.shape[0] == seg.B and images.shape[2] == images.shape[3]
    if out is None:
        out = torch.empty(seg.rows, Kp, device=images.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (seg.rows, Kp)
    sb, sc, sy, _ = images.stride()
    check(lib().sc_vit_patchify_bf16(_p(images), sb, sc, sy, _p(out), Kp, seg.ref(), images.shape[2], P, _stream()), "sc_vit_patchify_bf16")
    return out


def vit_embed_ln(G: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, seg: "RowSegments",
                 eps: float = 1e-5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """X [seg.rows, W] bf16 = ln_pre(class / patch embedding + positional embedding) (sc_vit_embed_ln_bf16); G = the patch GEMM's fp32
    output [seg.rows, W], pos [tokens, W]; pad rows are zero."""
    rows, W = G.shape
    for t in (G, cls, pos, gamma, beta):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert rows == seg.rows and cls.numel() == W and pos.shape[1] == W and gamma.numel() == W and beta.numel() == W
    if out is None:
        out = torch.empty(rows, W, device=G.device, dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and tuple(out.shape) == (rows, W)
    check(lib().sc_vit_embed_ln_bf16(_p(G), _p(aligned16(cls)), _p(aligned16(pos)), _p(aligned16(gamma)), _p(aligned16(beta)), _p(out),
                                     seg.ref(), pos.shape[0], W, float(eps), _stream()), "sc_vit_embed_ln_bf16")
    return out


def image_resample_h(src: torch.Tensor, tab: torch.Tensor, mid: torch.Tensor, plan) -> torch.Tensor:
    """mid (uint8, plan.mid_bytes) <- the horizontal pass of CLIP's bicubic resize over the packed raw images ``src`` (1-D uint8), only the
    crop window's columns and the source rows its vertical pass reads (sc_image_resample_h_u8).  ``tab``: the plan's descriptor /
    coefficient tables on the device (image_prep.Plan)."""
    for t, dt in ((src, torch.uint8), (mid, torch.uint8), (tab, torch.int32)):
        assert t.dtype == dt and t.dim() == 1 and t.is_contiguous()
    assert tab.numel() == plan.tab.numel() and mid.numel() >= plan.mid_bytes and src.numel() >= plan.src_end and tab.data_ptr() % 8 == 0
    check(lib().sc_image_resample_h_u8(_p(src), src.numel(), _p(tab), _p(tab), _p(mid), mid.numel(), plan.B, plan.max_rows, plan.n_px, _stream()),
          "sc_image_resample_h_u8")
    return mid


def image_resample_v_norm(mid: torch.Tensor, tab: torch.Tensor, lut: torch.Tensor, plan, out: Optional[torch.Tensor] = None,
                          A: Optional[torch.Tensor] = None, seg: Optional["RowSegments"] = None, P: int = 0, Kp: int = 0):
    """The vertical pass over ``mid`` + the normalisation look-up (sc_image_resample_v_norm) into ``out`` fp32 [B, 3, S, S] and / or
    ``A`` [seg.rows, Kp] bf16 - what vit_patchify makes of ``out``, bit for bit - whichever is given."""
    S, B = plan.n_px, plan.B
    assert mid.dtype == torch.uint8 and mid.is_contiguous() and mid.numel() >= plan.mid_bytes
    assert tab.dtype == torch.int32 and tab.numel() == plan.tab.numel() and tab.data_ptr() % 8 == 0
    assert lut.dtype == torch.float32 and lut.is_contiguous() and tuple(lut.shape) == (3, 256)
    assert out is not None or A is not None
    if out is not None:
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, 3, S, S)
    if A is not None:
        assert seg is not None and seg.B == B and min(seg.pitch) >= 1 + (S // P) ** 2
        assert A.dtype == torch.bfloat16 and A.is_contiguous() and tuple(A.shape) == (seg.rows, Kp)
    check(lib().sc_image_resample_v_norm(_p(mid), mid.numel(), _p(tab), _p(tab), _p(lut), _p(out), _p(A), Kp, seg.ref() if A is not None else None,
                                         P, B, S, _stream()), "sc_image_resample_v_norm")
    return out, A


def audio_resample(src: torch.Tensor, desc: torch.Tensor, table: Optional[torch.Tensor], first: Optional[torch.Tensor], P: int, Q: int,
                   taps: int, tile: int, out: torch.Tensor) -> torch.Tensor:
    """out [rows, Lout] fp32 <- the utterances of ONE source rate that ``desc`` (int64 [n, 5]: byte offset, frames, channels, n_out,
    output row) names in the packed PCM ``src`` (1-D int16 or fp32), converted, down-mixed and resampled to 16 kHz; zeros behind each
    n_out (sc_audio_resample).  ``table`` [Q, taps] fp32 / ``first`` [Q] int32: audio_prep.resample_table; None at P = Q = 1."""
    assert src.dim() == 1 and src.is_contiguous() and src.dtype in (torch.int16, torch.float32) and src.numel() > 0
    assert desc.dtype == torch.int64 and desc.dim() == 2 and desc.shape[1] == 5 and desc.is_contiguous() and desc.shape[0] >= 1
    assert out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.shape[1] >= 1 and out.stride(0) >= out.shape[1]
    if P == 1 and Q == 1:
        table = first = None
    else:
        assert table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == (Q, taps)
        assert first.dtype == torch.int32 and first.is_contiguous() and tuple(first.shape) == (Q,)
    check(lib().sc_audio_resample(_p(src), src.numel() * src.element_size(), int(src.dtype == torch.int16), _p(desc), desc.shape[0], _p(table),
                                  _p(first), P, Q, taps, tile, _p(out), out.stride(0), out.shape[0], out.shape[1], _stream()), "sc_audio_resample")
    return out


def rows_scatter(d: torch.Tensor, row: torch.Tensor, M: int, SEG: int) -> torch.Tensor:
    """dX [M, W] bf16: zero except dX[row[b]] = bf16(d[b]) (row[b] inside segment b of SEG rows)"""
    B, W = d.shape
    assert d.dtype == torch.float32 and d.is_contiguous() and row.dtype == torch.int32
    dX = torch.empty(M, W, device=d.device, dtype=torch.bfloat16)
    check(lib().sc_rows_scatter_bf16(_p(d), _p(row), _p(dX), M, B, W, SEG, _stream()), "sc_rows_scatter_bf16")
    return dX


# ---- CIF on the rows of the attention block in front of it (bf16, the block's pitch; csrc/cif.hip) ------------------------------------
def cif_fwd_rows(full: torch.Tensor, head: int, S: int, alpha: torch.Tensor, csum: torch.Tensor, T: int, thr: float) -> torch.Tensor:
    """full [B, P, C] bf16 contiguous, frames of utterance b = its rows head .. head + S - 1 -> out [B, T + 1, C] fp32"""
    B, P, C = full.shape
    assert full.dtype == torch.bfloat16 and full.is_contiguous() and head + S <= P
    assert alpha.dtype == torch.float32 and alpha.is_contiguous() and csum.is_contiguous() and tuple(alpha.shape) == (B, S)
    out = torch.empty(B, T + 1, C, device=full.device, dtype=torch.float32)
    x0 = full.view(-1)[head * C:]
    check(lib().sc_cif_fwd_rows(_p(x0), 1, P * C, _p(alpha), _p(csum), _p(out), B, S, C, T, float(thr), _stream()), "sc_cif_fwd_rows")
    return out


def cif_bwd_rows(full: torch.Tensor, head: int, S: int, alpha: torch.Tensor, csum: torch.Tensor, g: torch.Tensor, T: int, thr: float,
                 tail_rows: int = 0):
    """-> (d full [B, P, C] bf16: the frames' gradient, zero in every other row, pa, pb [nblk, B, S]); ``tail_rows``: d full is the
    head of a flat buffer with that many more (zero) rows behind it"""
    B, P, C = full.shape
    assert g.dtype == torch.float32 and g.is_contiguous() and tuple(g.shape) == (B, T + 1, C)
    nblk = (C + 255) // 256
    if tail_rows:
        flat = torch.empty(B * P + tail_rows, C, device=full.device, dtype=full.dtype)
        flat[B * P:].zero_()
        dfull = flat[: B * P].view(B, P, C)
    else:
        dfull = torch.empty_like(full)
    pa = torch.empty(nblk, B, S, device=full.device, dtype=torch.float32)
    pb = torch.empty(nblk, B, S, device=full.device, dtype=torch.float32)
    check(lib().sc_cif_bwd_rows(_p(full.view(-1)[head * C:]), 1, P * C, _p(alpha), _p(csum), _p(g), _p(dfull.view(-1)[head * C:]), 1, P * C, head,
                                P - head - S, _p(pa), _p(pb), B, S, C, T, float(thr), _stream()), "sc_cif_bwd_rows")
    return dfull, pa, pb


def rows_zero_pad(flat: torch.Tensor, lead: int, B: int, P: int, head: int, stop: int, trail: int) -> None:
    """flat [lead + B P + trail, D] bf16: zero the rows that are not frames (see sc_rows_zero_pad_bf16)"""
    assert flat.dtype == torch.bfloat16 and flat.is_contiguous() and flat.shape[0] == lead + B * P + trail
    check(lib().sc_rows_zero_pad_bf16(_p(flat), lead, B, P, head, stop, trail, flat.shape[1], _stream()), "sc_rows_zero_pad_bf16")


def wsum_share(dX: torch.Tensor, w: torch.Tensor, prev: Optional[torch.Tensor], B: int, R: int, T: int, row_off: int = 1) -> torch.Tensor:
    """[B R, D] bf16 = (prev or 0) + bf16(w * dX[b, t + row_off]) for the frames t < T (sc_wsum_share_bf16): dX fp32 [B, R, D], w a
    one-element fp32 device tensor (one softmax weight of the weighted sum)"""
    D = dX.shape[-1]
    assert dX.dtype == torch.float32 and dX.is_contiguous() and w.dtype == torch.float32 and w.numel() == 1
    assert prev is None or (prev.dtype == torch.bfloat16 and prev.is_contiguous() and prev.numel() == B * R * D)
    out = torch.empty(B * R, D, device=dX.device, dtype=torch.bfloat16)
    check(lib().sc_wsum_share_bf16(_p(dX), _p(w), _p(prev), _p(out), B, R, T, D, row_off, _stream()), "sc_wsum_share_bf16")
    return out


def transpose_batched_bf16(x0: torch.Tensor, sx: int, n: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """n equally shaped [rows, cols] bf16 matrices, matrix z = ``sx`` elements after matrix z - 1 (``x0`` = the first, dense rows) ->
    out [n, cols, rows] (one launch, sc_transpose_batched_bf16)"""
    rows, cols = x0.shape
    assert x0.dtype == torch.bfloat16 and x0.stride(1) == 1
    if out is None:
        out = torch.empty(n, cols, rows, device=x0.device, dtype=torch.bfloat16)
    check(lib().sc_transpose_batched_bf16(_p(x0), x0.stride(0), sx, _p(out), rows, cols * rows, rows, cols, n, _stream()), "sc_transpose_batched_bf16")
    return out
