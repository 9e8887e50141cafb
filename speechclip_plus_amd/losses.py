"""MaskedContrastiveLoss (avssl/module/losses.py:129-245) on the HIP loss kernels.

Same constructor (temperature, temperature_trainable, margin, dcl, a2b, b2a - every option built), ``forward(feat_A, feat_B,
index=None) -> scalar`` (keywords ``bank`` / ``bank_ids`` / ``neg_idx``: mined negatives from a constant bank beside the batch, see
``forward``), ``current_temperature`` and the ``temperature`` parameter / attribute (log(1/T) when trainable, 1/T
otherwise).  No MAX_EYE = 256 cap (losses.py:126: the reference cannot run B > 256; the masks are computed in-kernel from
``index``).  Forward = one launch (csrc/loss_optim.hip: sc_infonce_fwd); the temperature reaches the kernels as a DEVICE scalar,
so a trainable temperature costs no host synchronisation in the step.
"""
import numpy as np
import torch
from torch import nn

from . import ops


class _InfoNCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat_A, feat_B, inv_temp, index, margin, dcl, a2b, b2a):
        A = feat_A.detach().float().contiguous()
        Bm = feat_B.detach().float().contiguous()
        it = inv_temp.detach().float().reshape(1).contiguous()
        ids = index.contiguous() if index is not None else None
        loss, logits, lse_row, lse_col = ops.infonce_fwd(A, Bm, ids, it, margin, dcl, a2b, b2a)
        ctx.save_for_backward(A, Bm, logits, lse_row, lse_col, it, ids if ids is not None else torch.empty(0))
        ctx.has_ids = ids is not None
        ctx.opts = (margin, dcl, a2b, b2a)
        return loss.reshape(())            # (a fresh [1] buffer of this call: no copy)

    @staticmethod
    def backward(ctx, g):
        A, Bm, logits, lse_row, lse_col, it, ids = ctx.saved_tensors
        ids = ids if ctx.has_ids else None
        G, dot = ops.infonce_grad(logits, ids, lse_row, lse_col, g.float().reshape(1).contiguous(), it, *ctx.opts)
        dA = dB = dT = None
        if ctx.needs_input_grad[0]:
            dA = ops.sgemm_mfma(G, Bm, b_kmajor=True)                          # G . B     (G already carries inv_temp)
        if ctx.needs_input_grad[1]:
            dB = ops.sgemm_mfma(G, A, a_kmajor=True, b_kmajor=True)            # G^T . A
        if ctx.needs_input_grad[2]:
            dT = dot.sum()                                                     # d loss / d inv_temp (device scalar)
        return dA, dB, dT, None, None, None, None, None


class _InfoNCENegFn(torch.autograd.Function):
    """``_InfoNCEFn`` with the a2b denominator extended by rows of a constant bank (csrc/infonce_neg.hip): the plain forward, then the
    extension; backward = ``infonce_grad`` on the extended lse_row, the two products, then the extras' accumulation into dA and dot."""

    @staticmethod
    def forward(ctx, feat_A, feat_B, inv_temp, index, margin, dcl, a2b, b2a, bank, bank_ids, neg_idx, holder):
        A = feat_A.detach().float().contiguous()
        Bm = feat_B.detach().float().contiguous()
        it = inv_temp.detach().float().reshape(1).contiguous()
        ids = index.contiguous() if index is not None else None
        bank, neg_idx = ops.bank_rows(bank), neg_idx.contiguous()              # copies, where any are needed, are made once for both passes
        _, logits, lse_row, lse_col = ops.infonce_fwd(A, Bm, ids, it, margin, dcl, a2b, b2a)
        loss, lse_ext, x, used = ops.infonce_neg_fwd(A, bank, neg_idx, ids, bank_ids, it, lse_row, lse_col, logits, a2b, b2a)
        holder.last_used = used
        ctx.save_for_backward(A, Bm, logits, lse_ext, lse_col, it, ids if ids is not None else torch.empty(0), bank, neg_idx, x)
        ctx.has_ids = ids is not None
        ctx.opts = (margin, dcl, a2b, b2a)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        A, Bm, logits, lse_ext, lse_col, it, ids, bank, neg_idx, x = ctx.saved_tensors
        ids = ids if ctx.has_ids else None
        gscale = g.float().reshape(1).contiguous()
        G, dot = ops.infonce_grad(logits, ids, lse_ext, lse_col, gscale, it, *ctx.opts)
        dA = dB = dT = None
        want_dA, want_dT = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        if want_dA:
            dA = ops.sgemm_mfma(G, Bm, b_kmajor=True)                          # G . B: the in-batch share
        if want_dA or want_dT:
            acc = dA if want_dA else torch.zeros_like(A)
            ops.infonce_neg_grad(A, bank, neg_idx, x, lse_ext, gscale, it, ctx.opts[2], ctx.opts[3], acc, dot)
        if ctx.needs_input_grad[1]:
            dB = ops.sgemm_mfma(G, A, a_kmajor=True, b_kmajor=True)            # G^T . A: no extra term; it moves through lse_ext
        if want_dT:
            dT = dot.sum()
        return (dA, dB, dT) + (None,) * 9


class MaskedContrastiveLoss(nn.Module):
    def __init__(self, temperature: float = 0.07, temperature_trainable: bool = False, margin: float = 0.0,
                 dcl: bool = False, a2b: bool = True, b2a: bool = True):
        super().__init__()
        assert a2b or b2a, "Cannot set both `a2b` and `b2a` to False."
        self.temperature_trainable = temperature_trainable
        self.margin, self.dcl, self.a2b, self.b2a = float(margin), bool(dcl), bool(a2b), bool(b2a)
        if temperature_trainable:
            self.temperature = nn.Parameter(torch.ones([]) * np.log(1 / temperature))
        else:
            self.temperature = 1 / temperature
        self._inv_temp_dev = {}
        self.last_used = None          # int32 [Bg] device tensor: slots per anchor that took part in the last call with a bank

    @property
    def current_temperature(self) -> float:
        if self.temperature_trainable:
            temp = self.temperature.data.cpu().detach().float().exp().item()
        else:
            temp = self.temperature
        return float(temp)

    @property
    def temperature_for_logging(self):
        """``current_temperature`` without the device -> host synchronisation of ``.item()``: a 0-dim device tensor when the
        temperature is trainable (loggers accept tensors), the python float otherwise."""
        if self.temperature_trainable:
            return self.temperature.detach().float().exp()
        return float(self.temperature)

    def forward(self, feat_A: torch.Tensor, feat_B: torch.Tensor, index: torch.LongTensor = None, *, bank: torch.Tensor = None,
                bank_ids: torch.LongTensor = None, neg_idx: torch.LongTensor = None) -> torch.Tensor:
        """``bank`` [N, E] fp32 (constant: no gradient, a bank that requires grad is refused), ``bank_ids`` [N] int64 (with ``index``,
        both or neither) and ``neg_idx`` [Bg, M] int64, 1 <= M <= 1024, in the form ``hard_negatives`` returns: per anchor, bank rows
        added as plain negatives (no margin) to the feat_A -> feat_B denominator.  Slot (i, n), r = neg_idx[i, n], takes part iff
        0 <= r < N and, with ids, bank_ids[r] is the id of NO row of the batch - the false negative and the image that already stands in
        the batch are left out, as are the -1 tails.  ``bank`` and ``neg_idx`` come together; without them the call is the plain
        loss.  With ``a2b=False`` the extras have no denominator to enter: a ValueError.  ``last_used`` [Bg] int32 (a device tensor, no
        sync) counts the slots that took part in the last call."""
        assert feat_A.shape == feat_B.shape, (feat_A.shape, feat_B.shape)
        if index is not None:
            assert index.shape[0] == feat_A.shape[0], (index.shape, feat_A.shape)
        with_bank = bank is not None or neg_idx is not None or bank_ids is not None
        if with_bank:                                      # every refusal before a launch
            if (index is None) != (bank_ids is None):
                raise ValueError("MaskedContrastiveLoss: ids on one side only - give index and bank_ids, or neither")
            if bank is None or neg_idx is None:
                raise ValueError("MaskedContrastiveLoss: bank and neg_idx come together (a bank without lists, or lists without a bank)")
            ops.neg_operands("MaskedContrastiveLoss", feat_A, bank, neg_idx, index, bank_ids, self.a2b)
        if self.temperature_trainable:
            inv_temp = torch.exp(self.temperature)
        else:                                              # constant: one device scalar per device, built once
            inv_temp = self._inv_temp_dev.get(feat_A.device)
            if inv_temp is None:
                inv_temp = self._inv_temp_dev[feat_A.device] = torch.full((1,), float(self.temperature), device=feat_A.device)
        # losses.py:219-220 subtracts the margin only ``if self.margin > 0.0``: a negative margin is the plain loss
        if with_bank:
            return _InfoNCENegFn.apply(feat_A, feat_B, inv_temp, index, max(self.margin, 0.0), self.dcl, self.a2b, self.b2a, bank, bank_ids,
                                       neg_idx, self)
        return _InfoNCEFn.apply(feat_A, feat_B, inv_temp, index, max(self.margin, 0.0), self.dcl, self.a2b, self.b2a)
