"""Keyword -> CLIP sub-word vector quantiser and keyword BatchNorm of the cascaded+/hybrid+ branches on the library's kernels
(csrc/vq.hip; scope rows a11 / f3).

What the reference computes (avssl/model/kw_branches.py:158-197, avssl/module/speechclip_c_modules/my_vector_quantizer.py:64-165):
cosine of every projected keyword against every token embedding of the reduced vocabulary, the special tokens {0, 2, 3} masked
to -inf, ``argmax`` -> one-hot, and in training the straight-through estimator ``hard + soft - soft.detach()`` with
``soft = softmax(x / temp)``; then ``keywords = subword_prob @ token_embedding``.

How it runs here (``SimpleVectorQuantizer.quantize_keywords``, called by GeneralBranch.vq_audio_features):

    forward   kw -> normalise + transpose (sc_vq_prep_f32) -> cosine scores in exact fp32 on the matrix pipe (sc_sgemm_mfma_f32:
              the scores pick a discrete token, so no reduced-precision operand) -> one row pass (sc_vq_rowstats: mask, argmax,
              LSE(x / temp), LSE(x), entropy) -> perplexities (sc_vq_perplexity) -> keywords = table[argmax] (sc_vq_gather_f32:
              the value of ``hard @ table``; the dense (Nk, V) one-hot is never built)
    backward  t = g . table^T (bf16 MFMA GEMM, fp32 out) -> dx = soft (t - <soft, t>) / temp (sc_vq_soft_bwd, bf16) ->
              d cos-side = dx . normalised table (bf16 MFMA GEMM, split along the vocabulary) -> through the normalisation
              (sc_vq_norm_bwd_f32).  The reference trains under precision-16 autocast; gradients here are bf16 operands with
              fp32 accumulation.

The other training modes (the same two nodes, ``_KeywordVQFn`` / ``_VQDenseFn``, with a mode; kernels behind the row statistics in
csrc/vq.hip, prototypes in include/speechclip_hip.h):
``use_gumbel`` perturbs the scores with g = -log(-log u), a stateless hash of (seed, row, column) that every kernel evaluates again
(targets and the one-hot from argmax(x + g), soft = softmax((x + g) / temp)); ``hard = False`` makes ``subword_prob`` the softmax
itself, keywords = soft . table as one bf16 GEMM over the K-blocks [hi | hi | lo] x [hi | lo | hi] (every product exact in fp32, fp32
partials along the vocabulary added in slice order); ``temp = "learnable=..."`` returns d temp = -(1 / temp) sum dz z to ``curr_temp``.
Eval mode of every configuration, and training with use_gumbel false, hard true and no temperature gradient, issue the calls above.

``SimpleVectorQuantizer.forward(x)`` keeps the reference's module-level signature on a given score tensor (dense
``subword_prob`` with the same straight-through gradient, same kernels).  Same constructor keywords and result-dict keys.
There is no CPU path: these modules take device tensors only (the CPU restatement of this maths is oracle/cascaded_ref.py).
"""
import ast
import logging
from typing import Optional

import torch
import torch.nn as nn

from . import ops

logger = logging.getLogger(__name__)

__all__ = ["SimpleVectorQuantizer", "Kw_BatchNorm_dynamic", "VocabTables"]

SPECIAL_TOKENS = (0, 2, 3)        # my_vector_quantizer.py:64 default prob_msk
# the cosine scores on the fp32 matrix pipe (sc_sgemm_mfma_f32, rounds 2-5) instead of the three-way bf16 split product: A/B and tests
EXACT_FP32_SCORES = False


def _roundup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class VocabTables:
    """Derived copies of the frozen token table, built once per table version: the normalised table K-major in fp32 (the exact-fp32
    score GEMM of the debug / A-B path), its three-way bf16 split (the score GEMM of the product path), the table in bf16
    (``g . table^T``) and the normalised table K-major in bf16 (``dx . normalised table``)."""

    def __init__(self, weight: torch.Tensor):
        w = weight.detach().float().contiguous()
        V, Et = w.shape
        self.V, self.Et, self.Vp = V, Et, _roundup(V, 128)
        self.table = w
        wn = w / w.norm(dim=-1, keepdim=True).clamp_min(1e-8)                       # F.normalize(emb, dim=-1, eps=1e-8)
        self.norm_T = torch.zeros(Et, self.Vp, device=w.device, dtype=torch.float32)
        self.norm_T[:, :V] = wn.t()
        self.Etp = _roundup(Et, 64)                                                 # K of the bf16 GEMM g . table^T
        self.table_bf16 = torch.zeros(self.Vp, self.Etp, device=w.device, dtype=torch.bfloat16)
        self.table_bf16[:V, :Et] = w
        self.norm_T_bf16 = self.norm_T.to(torch.bfloat16)
        # round 6: the normalised table as three bf16 addends in the six-K-block layout (ops.split3_bf16): the cosine scores are then ONE
        # bf16 GEMM with fp32-accurate results (every bf16 x bf16 product is exact in fp32) instead of an fp32 GEMM on the fp32 matrix pipe
        self.norm_split = ops.split3_bf16(wn.contiguous(), 1, rows_pad=128)
        assert self.norm_split.shape[0] == self.Vp
        units = self.Vp // 64
        self.splits = max(s for s in range(1, 17) if units % s == 0)                # equal vocabulary slices, multiples of 64
        self._soft_T = None

    def soft_table(self) -> torch.Tensor:
        """The table transposed and split, [Et, 3 Vp] bf16 = [hi | lo | hi]: the W operand of the soft product ``s . table``
        (ops.vq_soft_product).  Built on the first soft call: a hard-mode model never allocates it."""
        if self._soft_T is None:
            self._soft_T = ops.vq_soft_table(self.table, self.Vp)
        return self._soft_T

    @staticmethod
    def of(weight: torch.Tensor, cache: dict) -> "VocabTables":
        key = (weight.data_ptr(), weight._version, tuple(weight.shape), weight.device)
        if cache.get("key") != key:
            cache["key"], cache["tables"] = key, VocabTables(weight)
        return cache["tables"]


class VQResult(dict):
    """Result dict of the fused path: ``subword_prob`` (a dense (B, N, V) one-hot nobody on the path reads - the keywords are
    gathered) is materialised on first access only."""

    _soft = None        # soft modes: (scores, row statistics, temp, seed, noise) - subword_prob is then softmax((x + g) / temp), not the one-hot

    def __missing__(self, key):
        if key == "subword_prob":
            bsz, tsz, V = self._shape
            if self._soft is not None:
                x, stats, temp, seed, noise = self._soft
                self[key] = ops.vq_soft_prob(x, stats, V, temp, seed, noise).view(bsz, tsz, V)
            else:
                self[key] = ops.vq_onehot(self["targets"].reshape(-1), V).view(bsz, tsz, V)
            return self[key]
        raise KeyError(key)


# A call's ``mode``: None is the shipped default (argmax of the scores, hard one-hot, no gradient to a temperature: sc_vq_rowstats' fused
# lse_t and sc_vq_soft_bwd); otherwise (use_gumbel, hard, seed), on sc_vq_noisy_rowstats' (max, log sum) and sc_vq_soft_bwd2.


def _row_statistics(x, V: int, temp: float, mask):
    """The front half every call shares, on scores x [Nk, >= V] (masked in place): -> (idx, lse_t, ent, ppl).  ent and ppl come from
    the unperturbed scores in every mode."""
    idx, lse_t, lse_1, ent = ops.vq_rowstats(x, V, temp, mask)
    return idx, lse_t, ent, ops.vq_perplexity(x, V, idx, lse_1)


def _soft_bwd(x, stat, t, V: int, temp: float, mode, want_dtemp: bool, out_bf16: bool, Vpad=None):
    """-> (dx = soft (t - <soft, t>) / temp, d temp or None) on the statistics the forward of this mode saved."""
    if mode is None:
        return ops.vq_soft_bwd(x, stat, t, V, temp, out_bf16=out_bf16, Vpad=Vpad), None
    use_gumbel, _, seed = mode
    return ops.vq_soft_bwd2(x, stat, t, V, temp, out_bf16=out_bf16, Vpad=Vpad, seed=seed, noise=use_gumbel, want_dtemp=want_dtemp)


class _KeywordVQFn(torch.autograd.Function):
    """kw [Nk, Et] fp32, temp_t = the temperature parameter [1] when it takes a gradient (else None) -> (keywords [Nk, Et], idx [Nk] =
    the targets, ent [Nk], ppl [2], scores [Nkp, Vp], stats [2, Nk] or None in the default mode); gradients to kw and, as a [1]
    tensor, to temp_t.  hard: keywords = table[idx] (the exact one-hot's product; the straight-through term is value-neutral, the dense
    (Nk, V) one-hot is never built); soft: keywords = s . table on the split-bf16 product (ops.vq_soft_product)."""

    @staticmethod
    def forward(ctx, kw, temp_t, tb: VocabTables, temp: float, training: bool, mode):
        Nk, Et = kw.shape
        kw = kw.detach().float().contiguous()
        kwn_T, rnorm = ops.vq_prep(kw)
        if EXACT_FP32_SCORES:
            cos = ops.sgemm_mfma(kwn_T, tb.norm_T, a_kmajor=True, b_kmajor=True)                               # [Nkp, Vp] fp32
        else:
            cos = ops.cosine_scores_split(kw, rnorm, tb.norm_split, tb.Vp)                                     # [Nkp, Vp] fp32, fp32-accurate
        x = cos[:Nk]
        idx, lse_t, ent, ppl = _row_statistics(x, tb.V, temp, SPECIAL_TOKENS)
        use_gumbel, hard, seed = mode or (False, True, 0)
        stat = lse_t
        if mode is not None:               # the argmax and the (max, log sum) [2, Nk] of the scores this mode softmaxes
            idx, stat = ops.vq_noisy_rowstats(x, tb.V, temp, seed, use_gumbel)
        if hard:
            out = ops.vq_gather(tb.table, idx)
        else:
            out = ops.vq_soft_product(ops.vq_soft_split(x, stat, tb.V, temp, tb.Vp, seed, use_gumbel), tb.soft_table(), Et)[:Nk]
        ctx.tb, ctx.temp, ctx.training, ctx.mode, ctx.want_dtemp = tb, temp, training, mode, temp_t is not None
        if training:
            ctx.save_for_backward(kw, rnorm, cos, stat)
        stats = None if mode is None else stat
        ctx.mark_non_differentiable(*(t for t in (idx, ent, ppl, cos, stats) if t is not None))
        return out, idx, ent, ppl, cos, stats

    @staticmethod
    def backward(ctx, g, *_):
        if not ctx.training:               # inference: subword_prob is the hard one-hot, nothing flows back
            return None, None, None, None, None, None
        kw, rnorm, cos, stat = ctx.saved_tensors
        tb = ctx.tb
        dkw, dtemp = _keyword_backward(kw, rnorm, cos, tb, g, lambda x, t, Vp: _soft_bwd(
            x, stat, t, tb.V, ctx.temp, ctx.mode, ctx.want_dtemp, out_bf16=True, Vpad=Vp))
        return dkw, dtemp, None, None, None, None


def _keyword_backward(kw, rnorm, cos, tb: VocabTables, g, soft_bwd):
    """The gradient chain of ``quantize_keywords`` in every training mode: t = g . table^T -> (dx, d temp) = soft_bwd(scores, t, Vp) ->
    dx . normalised table, cut along the vocabulary -> through the normalisation.  -> (d kw, d temp)"""
    Nk, Et = kw.shape
    Nkp, Vp = cos.shape
    dev = kw.device
    gb = torch.zeros(Nkp, tb.Etp, device=dev, dtype=torch.bfloat16)
    gb[:Nk, :Et] = g
    t = torch.empty(Nkp, Vp, device=dev, dtype=torch.float32)
    ops.gemm_raw(gb, tb.Etp, tb.table_bf16, tb.Etp, t, Vp, Nkp, Vp, tb.Etp, out_f32=True)     # d subword_prob = g . table^T
    dx = torch.zeros(Nkp, Vp, device=dev, dtype=torch.bfloat16) if Nkp != Nk else None
    dxv, dtemp = soft_bwd(cos[:Nk], t[:Nk], Vp)
    if dx is None:
        dx = dxv
    else:
        dx[:Nk] = dxv
    S = tb.splits
    Kc = Vp // S
    part = torch.empty(S, Nkp, Et, device=dev, dtype=torch.float32)
    ops.gemm_raw(dx, Vp, tb.norm_T_bf16, Vp, part, Et, Nkp, Et, Kc, out_f32=True, nb1=S, sA=(Kc, 0), sW=(Kc, 0), sC=(Nkp * Et, 0))
    dkwn = torch.empty(Nkp, Et, device=dev, dtype=torch.float32)
    ops.colsum(part, Nkp * Et, S, Nkp * Et, dkwn)
    return ops.vq_norm_bwd(kw, rnorm, dkwn[:Nk]), dtemp


class _VQDenseFn(torch.autograd.Function):
    """The module-level API on a given score matrix x [Nk, V] (masked in place): dense subword_prob = the exact one-hot of argmax(x + g)
    (hard) or s = softmax((x + g) / temp) (soft), gradient dx = s (t - <s, t>) / temp in both, d temp as a [1] tensor to temp_t."""

    @staticmethod
    def forward(ctx, x, temp_t, temp: float, prob_msk, training: bool, mode):
        Nk, V = x.shape
        idx, lse_t, ent, ppl = _row_statistics(x, V, temp, prob_msk)
        use_gumbel, hard, seed = mode or (False, True, 0)
        stat = lse_t
        if mode is not None:               # the argmax and the (max, log sum) [2, Nk] of the scores this mode softmaxes
            idx, stat = ops.vq_noisy_rowstats(x, V, temp, seed, use_gumbel)
        prob = ops.vq_onehot(idx, V) if hard else ops.vq_soft_prob(x, stat, V, temp, seed, use_gumbel)
        ctx.temp, ctx.training, ctx.mode, ctx.want_dtemp = temp, training, mode, temp_t is not None
        if training:
            ctx.save_for_backward(x, stat)
        ctx.mark_non_differentiable(idx, ent, ppl)
        return prob, idx, ent, ppl

    @staticmethod
    def backward(ctx, g, *_):
        if not ctx.training:
            return None, None, None, None, None, None
        x, stat = ctx.saved_tensors
        dx, dtemp = _soft_bwd(x, stat, g.float().contiguous(), x.shape[1], ctx.temp, ctx.mode, ctx.want_dtemp, out_bf16=False)
        return dx, dtemp, None, None, None, None


class SimpleVectorQuantizer(nn.Module):
    def __init__(self, temp, groundTruthPerplexity=None, time_first=True, use_gumbel=False, hard=True):
        super().__init__()
        self.time_first, self.use_gumbel, self.hard = time_first, bool(use_gumbel), bool(hard)
        if isinstance(temp, str):
            if temp.startswith("learnable="):
                self.temp_type = "learnable"
                self.curr_temp = nn.parameter.Parameter(torch.FloatTensor([ast.literal_eval(temp[len("learnable="):])]))
            elif temp.startswith("fixed="):
                self.temp_type = "fixed"
                self._fixed_temp = float(ast.literal_eval(temp[len("fixed="):]))
                self.register_buffer("curr_temp", torch.FloatTensor([self._fixed_temp]))
            else:
                self.temp_type = "scheduled"
                sched = ast.literal_eval(temp)
                assert len(sched) == 3, f"{sched}, {len(sched)}"
                self.max_temp, self.min_temp, self.temp_decay = sched
                self.curr_temp = self.max_temp
        self.codebook_indices = None
        self.groundTruthPerplexity = groundTruthPerplexity
        self._tables = {}

    def set_num_updates(self, num_updates):
        if self.temp_type == "scheduled":
            self.curr_temp = max(self.max_temp * self.temp_decay ** num_updates, self.min_temp)

    def _temp(self) -> float:
        """The temperature of this call as a host float, read ONCE per forward: a learnable temperature costs one ``.item()`` (a device
        sync) here, the sync the reference has at my_vector_quantizer.py:123 (``result["temp"] = self.curr_temp.item()``).  A
        temperature at or below zero is a ValueError before any launch."""
        if self.temp_type == "fixed":
            temp = self._fixed_temp
        elif self.temp_type == "learnable":
            temp = float(self.curr_temp.item())
        else:
            temp = float(self.curr_temp)
        if not temp > 0.0:
            raise ValueError(f"SimpleVectorQuantizer: the temperature is {temp}; it must be positive")
        return temp

    def _mode(self):
        """-> (default, temp_t, seed).  ``default``: this call is the shipped quantiser's (eval mode of every configuration; training
        with use_gumbel false, hard true and no gradient to a temperature) and issues exactly the calls it always has.  Otherwise
        ``temp_t`` is the temperature parameter when it takes a gradient (else None) and ``seed`` the Gumbel seed: one
        ``ops.next_mult_seed()`` per call, drawn only when training with use_gumbel, so no other mode moves the dropout seed stream."""
        temp_t = self.curr_temp if (self.temp_type == "learnable" and self.training and torch.is_grad_enabled()
                                    and self.curr_temp.requires_grad) else None
        if not self.training or (self.hard and not self.use_gumbel and temp_t is None):
            return True, None, 0
        return False, temp_t, (ops.next_mult_seed() if self.use_gumbel else 0)

    def _result(self, bsz, tsz, V, idx, ent, ppl, temp) -> VQResult:
        r = VQResult(num_vars=V)
        r._shape = (bsz, tsz, V)
        if bsz * tsz == 1:
            # my_vector_quantizer.py:90 squeezes the (1, V) one-hot: its "mean over rows" becomes the mean over the vocabulary
            p = torch.full((), 1.0 / V, device=idx.device)
            r["code_perplexity"] = torch.exp(-(p * torch.log(p + 1e-7)))
        else:
            r["code_perplexity"] = ppl[0]
        r["prob_perplexity"] = ppl[1]
        r["ent_per_t"] = ent.view(bsz, tsz).mean(dim=0)
        r["temp"] = temp
        if self.groundTruthPerplexity is not None:
            gt = float(self.groundTruthPerplexity)
            r["diversity_loss"] = (r["prob_perplexity"] - gt) ** 2 / (V - gt) ** 2
        else:
            r["diversity_loss"] = (V - r["prob_perplexity"]) / V
        r["targets"] = idx.view(bsz, tsz, 1)
        return r

    def forward(self, x, prob_msk=[0, 2, 3], produce_targets=True):
        """my_vector_quantizer.py:64-165 on a score tensor (B, T, V) (or (B, V, T) when not time_first); the masked columns of
        ``x`` are overwritten with -inf like the reference's in-place add."""
        if not x.is_cuda:
            raise RuntimeError("SimpleVectorQuantizer runs on the HIP kernels: device tensors only (CPU restatement: oracle/)")
        if not self.time_first:
            x = x.transpose(1, 2)
        bsz, tsz, fsz = x.shape
        x2 = x.reshape(bsz * tsz, fsz)
        if x2.dtype != torch.float32 or x2.stride(1) != 1:
            x2 = x2.float().contiguous()
        temp = self._temp()
        default, temp_t, seed = self._mode()
        mode = None if default else (self.use_gumbel, self.hard, seed)
        prob, idx, ent, ppl = _VQDenseFn.apply(x2, temp_t, temp, tuple(prob_msk), self.training, mode)
        r = self._result(bsz, tsz, fsz, idx, ent, ppl, temp)
        r["subword_prob"] = prob.view(bsz, tsz, fsz)
        if not produce_targets:
            del r["targets"]
        return r

    def quantize_keywords(self, keywords: torch.Tensor, token_table: torch.Tensor):
        """Fused cosine -> mask -> argmax / straight-through -> ``@ token_table`` (kw_branches.py:158-197):
        keywords (B, N, Et) projected keyword embeddings, token_table (V, Et) frozen -> (result dict, quantised keywords)."""
        if not keywords.is_cuda:
            raise RuntimeError("SimpleVectorQuantizer runs on the HIP kernels: device tensors only (CPU restatement: oracle/)")
        assert not token_table.requires_grad
        tb = VocabTables.of(token_table, self._tables)
        bsz, tsz, Et = keywords.shape
        temp = self._temp()
        default, temp_t, seed = self._mode()
        mode = None if default else (self.use_gumbel, self.hard, seed)
        out, idx, ent, ppl, cos, stats = _KeywordVQFn.apply(keywords.reshape(bsz * tsz, Et), temp_t, tb, temp, self.training, mode)
        r = self._result(bsz, tsz, tb.V, idx, ent, ppl, temp)
        if mode is not None and not self.hard:     # subword_prob, if anybody asks, is the dense softmax of these scores
            r._soft = (cos[:bsz * tsz], stats, temp, seed, self.use_gumbel)
        return r, out.reshape(bsz, tsz, Et).to(keywords.dtype)


class _KwBNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, run_mean, run_var, training: bool, momentum: float, eps: float):
        x = x.detach().float().contiguous()
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        y, sm, sr = ops.bn_rows_fwd(x, g, b, run_mean, run_var, training, momentum, eps)
        ctx.training = training
        if training:
            ctx.save_for_backward(x, g, sm, sr)
        else:
            ctx.save_for_backward(g, run_var.detach().clone())
            ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.float().contiguous()
        if ctx.training:
            x, g, sm, sr = ctx.saved_tensors
            dx, dg, db = ops.bn_rows_bwd(x, dy, g, sm, sr)
            return dx, dg, db, None, None, None, None, None
        g, rv = ctx.saved_tensors                      # inference statistics are constants: a per-channel scale
        return dy * (g * torch.rsqrt(rv + ctx.eps)), None, None, None, None, None, None, None


class Kw_BatchNorm_dynamic(nn.Module):
    """BatchNorm1d over keyword embeddings, initialised from the CLIP token-embedding mean / std (kw_bn.py:167-228).
    ``bn_layer`` holds the parameters and running statistics under the reference's state-dict names; the arithmetic runs on
    sc_bn_rows_fwd / _bwd."""

    def __init__(self, kw_dim: int, init_bias: torch.Tensor, init_scale: torch.Tensor, std_scale: int = 1,
                 learnable: bool = True) -> None:
        super().__init__()
        assert std_scale > 0, f"std scale must > 0, but input std scale is {std_scale}"
        self.kw_dim, self.learnable, self.std_scale = kw_dim, learnable, std_scale
        self.bn_layer = nn.BatchNorm1d(kw_dim)
        self.bn_layer.weight.data.copy_(init_scale * std_scale)
        self.bn_layer.bias.data.copy_(init_bias)
        self.bn_layer.weight.requires_grad = learnable
        self.bn_layer.bias.requires_grad = learnable

    def forward(self, keywords: torch.Tensor) -> torch.Tensor:
        assert keywords.dim() == 3
        if not keywords.is_cuda:
            raise RuntimeError("Kw_BatchNorm_dynamic runs on the HIP kernels: device tensors only (CPU restatement: oracle/)")
        bn = self.bn_layer
        B, N, E = keywords.shape
        training = self.training
        if training:
            bn.num_batches_tracked.add_(1)
        y = _KwBNFn.apply(keywords.reshape(B * N, E), bn.weight, bn.bias, bn.running_mean, bn.running_var, training,
                          float(bn.momentum), float(bn.eps))
        return y.view(B, N, E).to(keywords.dtype)


class _KwBNEachFn(torch.autograd.Function):
    """The fixed-count form on sc_bn_eachkw_fwd / _bwd: x [B, K, E], parameters and buffers [E * K] at index d * K + k."""

    @staticmethod
    def forward(ctx, x, gamma, beta, run_mean, run_var, training: bool, momentum: float, eps: float):
        x = x.detach().float().contiguous()
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        y, sm, sr = ops.bn_eachkw_fwd(x, g, b, run_mean, run_var, training, momentum, eps)
        ctx.training = training
        if training:
            ctx.save_for_backward(x, g, sm, sr)
        else:
            ctx.save_for_backward(g, run_var.detach().clone())
            ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.float().contiguous()
        if ctx.training:
            x, g, sm, sr = ctx.saved_tensors
            dx, dg, db = ops.bn_eachkw_bwd(x, dy, g, sm, sr)
            return dx, dg, db, None, None, None, None, None
        g, rv = ctx.saved_tensors                      # inference statistics are constants: a scale per (slot, channel), stored [E, K]
        B, K, E = dy.shape
        return dy * (g * torch.rsqrt(rv + ctx.eps)).view(E, K).t(), None, None, None, None, None, None, None


class Kw_BatchNorm(nn.Module):
    """BatchNorm for a fixed number of keywords (kw_bn.py:8-164), initialised from the CLIP token-embedding mean / std.
    ``eachKw`` + ``parallel``: nn.BatchNorm1d(kw_dim * kw_num) over keywords.permute(0, 2, 1).reshape(B, -1) - one statistic per
    (keyword slot k, channel d) over the batch, parameters and running buffers stored at d * kw_num + k as a reference checkpoint
    holds them; read in that layout by sc_bn_eachkw_fwd / _bwd (no permuted copy per step).  ``same``: one nn.BatchNorm1d(kw_dim) over
    every keyword position (sc_bn_rows_*).  ``bn_layer`` carries the reference's state-dict names."""

    def __init__(self, kw_num: int, kw_dim: int, batchnorm_type: str, init_bias: torch.Tensor, init_scale: torch.Tensor,
                 std_scale: int = 1, learnable: bool = True, parallel: bool = False) -> None:
        super().__init__()
        self.batchnorm_type, self.kw_num, self.kw_dim = batchnorm_type, kw_num, kw_dim
        self.learnable, self.parallel = learnable, parallel
        self.std_scale = std_scale if isinstance(std_scale, list) else [std_scale] * kw_num
        if batchnorm_type == "eachKw":
            if not parallel:
                raise NotImplementedError("Kw_BatchNorm: eachKw with parallel = false (kw_num separate BatchNorm1d modules, state-dict "
                                          "keys bn_layers.*) is selected by no shipped recipe and is not built")
            self.bn_layer = nn.BatchNorm1d(kw_dim * kw_num)
            self.bn_layer.weight.data.copy_((init_scale * self.std_scale[0]).repeat(kw_num))
            self.bn_layer.bias.data.copy_(init_bias.repeat(kw_num))
        elif batchnorm_type == "same":
            self.bn_layer = nn.BatchNorm1d(kw_dim)
            self.bn_layer.weight.data.copy_(init_scale * self.std_scale[0])
            self.bn_layer.bias.data.copy_(init_bias)
        else:
            raise NotImplementedError(f"Kw_BatchNorm: batchnorm_type = {batchnorm_type!r} (eachKw or same)")
        self.bn_layer.weight.requires_grad = learnable
        self.bn_layer.bias.requires_grad = learnable

    def forward(self, keywords: torch.Tensor, seq_lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        assert keywords.dim() == 3 and keywords.shape[2] == self.kw_dim
        if seq_lens is not None:
            raise NotImplementedError("Kw_BatchNorm: seq_lens (a ragged keyword count) is the dynamic module's case: Kw_BatchNorm_dynamic")
        assert keywords.shape[1] == self.kw_num
        if not keywords.is_cuda:
            raise RuntimeError("Kw_BatchNorm runs on the HIP kernels: device tensors only (CPU restatement: tests/kwpool_cases.py)")
        bn = self.bn_layer
        B, K, E = keywords.shape
        training = self.training
        if training:
            bn.num_batches_tracked.add_(1)
        args = (bn.weight, bn.bias, bn.running_mean, bn.running_var, training, float(bn.momentum), float(bn.eps))
        if self.batchnorm_type == "eachKw":
            y = _KwBNEachFn.apply(keywords, *args)
        else:
            y = _KwBNFn.apply(keywords.reshape(B * K, E), *args).view(B, K, E)
        return y.to(keywords.dtype)
