"""MaskedContrastiveLoss (avssl/module/losses.py:129-245) on the HIP loss kernels.

Same constructor (temperature, temperature_trainable, margin, dcl, a2b, b2a - every option built), ``forward(feat_A, feat_B,
index=None) -> scalar`` (keywords ``bank`` / ``bank_ids`` / ``neg_idx``: mined negatives from a constant bank beside the batch, see
``forward``; the module's call also takes ``queue_A`` / ``queue_B`` / ``queue_ids``: a cross-batch queue of past embeddings,
negatives in both directions), ``current_temperature`` and the ``temperature`` parameter / attribute (log(1/T) when trainable, 1/T
otherwise).  No MAX_EYE = 256 cap (losses.py:126: the reference cannot run B > 256; the masks are computed in-kernel from
``index``).  Forward = one launch (csrc/loss_optim.hip: sc_infonce_fwd); the temperature reaches the kernels as a DEVICE scalar,
so a trainable temperature costs no host synchronisation in the step.

SupConLoss (avssl/module/losses.py:8-123), the module's other class, follows below on csrc/supcon.hip: same-id pairs as positives.

SigmoidContrastiveLoss, this project's addition (the reference has no such loss), stands last, on csrc/sigmoid_loss.hip: the pairwise
sigmoid loss with a learnable scale and bias, every pair a decision of its own.
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


class _InfoNCEQueueFn(torch.autograd.Function):
    """``_InfoNCEFn`` with BOTH denominators extended by a cross-batch queue (csrc/infonce_queue.hip) as one node: the plain forward, the
    one or two score products on the exact-fp32 GEMM, then the extension; backward = ``infonce_grad`` on the extended statistics, the two
    in-batch products, the weights in place of the scores, then the one or two queue products.  The scores are consumed by the backward
    (they become the weights), so the node runs backward once."""

    @staticmethod
    def forward(ctx, feat_A, feat_B, inv_temp, index, margin, dcl, a2b, b2a, queue_A, queue_B, queue_ids, holder):
        A = ops.aligned16(feat_A.detach().float().contiguous())
        Bm = ops.aligned16(feat_B.detach().float().contiguous())
        it = inv_temp.detach().float().reshape(1).contiguous()
        ids = index.contiguous() if index is not None else None
        qA = ops.bank_rows(queue_A.detach()) if b2a else None                  # the image anchors' extras: past speech rows
        qB = ops.bank_rows(queue_B.detach()) if a2b else None                  # the speech anchors' extras: past image rows
        loss, logits, lse_row, lse_col = ops.infonce_fwd(A, Bm, ids, it, margin, dcl, a2b, b2a)
        x_A = ops.queue_scores(A, qB) if a2b else None
        x_B = ops.queue_scores(Bm, qA) if b2a else None
        loss, lse_row, lse_col, used_A, used_B = ops.infonce_queue_fwd(x_A, x_B, ids, queue_ids, it, loss, lse_row, lse_col, logits,
                                                                        A.shape[1], a2b, b2a)
        holder.last_queue_used = (used_A, used_B)
        none = torch.empty(0)
        ctx.save_for_backward(A, Bm, logits, lse_row, lse_col, it, ids if ids is not None else none, qA if b2a else none,
                              qB if a2b else none, x_A if a2b else none, x_B if b2a else none)
        ctx.has_ids = ids is not None
        ctx.opts = (margin, dcl, a2b, b2a)
        ctx.consumed = False
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        A, Bm, logits, lse_row, lse_col, it, ids, qA, qB, x_A, x_B = ctx.saved_tensors
        margin, dcl, a2b, b2a = ctx.opts
        if ctx.consumed:
            raise RuntimeError("MaskedContrastiveLoss with a queue: the backward turns the saved scores into the weights in place and "
                               "runs once per forward")
        ctx.consumed = True
        ids = ids if ctx.has_ids else None
        gscale = g.float().reshape(1).contiguous()
        G, dot = ops.infonce_grad(logits, ids, lse_row, lse_col, gscale, it, margin, dcl, a2b, b2a)
        dA = dB = dT = None
        want_dA, want_dB, want_dT = ctx.needs_input_grad[:3]
        if want_dA:
            dA = ops.sgemm_mfma(G, Bm, b_kmajor=True)                          # G . B: the in-batch share
        if want_dB:
            dB = ops.sgemm_mfma(G, A, a_kmajor=True, b_kmajor=True)            # G^T . A
        Nq = (x_A if a2b else x_B).shape[1]
        if Nq > 0 and A.shape[0] > 0 and (want_dA or want_dB or want_dT):
            w_A, w_B, dot = ops.infonce_queue_grad(x_A if a2b else None, x_B if b2a else None, lse_row, lse_col, gscale, it, a2b, b2a, dot)
            if want_dA and a2b:
                dA += ops.sgemm_mfma(w_A, qB, b_kmajor=True)                   # w_A . queue_B (w already carries c inv_temp)
            if want_dB and b2a:
                dB += ops.sgemm_mfma(w_B, qA, b_kmajor=True)                   # w_B . queue_A
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
        self._queue = (None, None, None)   # (queue_A, queue_B, queue_ids) of the call in progress: see __call__
        self.last_queue_used = None    # (used_A, used_B), int32 [Bg] device tensors: queue entries admitted per anchor, last call with a queue

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

    def __call__(self, *args, queue_A: torch.Tensor = None, queue_B: torch.Tensor = None, queue_ids: torch.LongTensor = None, **kwargs):
        """``criterion(feat_A, feat_B, index=None, *, bank=, bank_ids=, neg_idx=, queue_A=, queue_B=, queue_ids=)``: ``forward``'s own
        arguments and the cross-batch queue's three keywords (described under ``forward``).  ``forward`` keeps the parameter list it has
        had since the bank - code that inspects it sees no change - so the queue travels beside it, in ``_queue``, for the length of this
        call: hooks run as for any module; one criterion object is not called from two threads at once."""
        if queue_A is None and queue_B is None and queue_ids is None:
            return super().__call__(*args, **kwargs)
        self._queue = (queue_A, queue_B, queue_ids)
        try:
            return super().__call__(*args, **kwargs)
        finally:
            self._queue = (None, None, None)

    def forward(self, feat_A: torch.Tensor, feat_B: torch.Tensor, index: torch.LongTensor = None, *, bank: torch.Tensor = None,
                bank_ids: torch.LongTensor = None, neg_idx: torch.LongTensor = None) -> torch.Tensor:
        """``bank`` [N, E] fp32 (constant: no gradient, a bank that requires grad is refused), ``bank_ids`` [N] int64 (with ``index``,
        both or neither) and ``neg_idx`` [Bg, M] int64, 1 <= M <= 1024, in the form ``hard_negatives`` returns: per anchor, bank rows
        added as plain negatives (no margin) to the feat_A -> feat_B denominator.  Slot (i, n), r = neg_idx[i, n], takes part iff
        0 <= r < N and, with ids, bank_ids[r] is the id of NO row of the batch - the false negative and the image that already stands in
        the batch are left out, as are the -1 tails.  ``bank`` and ``neg_idx`` come together; without them the call is the plain
        loss.  With ``a2b=False`` the extras have no denominator to enter: a ValueError.  ``last_used`` [Bg] int32 (a device tensor, no
        sync) counts the slots that took part in the last call.

        ``queue_A`` / ``queue_B`` [Nq, E] fp32 (past feat_A / feat_B rows, unit-normalised by the caller; constants: no gradient, a queue
        that requires grad is refused) and ``queue_ids`` [Nq] int64 (with ``index``, both or neither): a cross-batch queue, plain
        negatives (no margin) in BOTH directions - queue_B joins the feat_A -> feat_B denominator, queue_A the feat_B -> feat_A one.
        Entry (i, q) is admitted iff there are no ids or queue_ids[q] != index[i]: a queued item is a false negative only for the anchor
        that has its id.  A direction that is off needs no queue; an enabled one without its queue is a ValueError, as is a bank
        together with a queue.  An empty queue (Nq = 0) is the plain loss to the bit.  ``last_queue_used`` = (used_A, used_B), [Bg] int32
        device tensors (no sync), counts the entries admitted per anchor in the last call.  The three are keywords of the module's CALL
        (``__call__``), not of this method."""
        queue_A, queue_B, queue_ids = self._queue
        assert feat_A.shape == feat_B.shape, (feat_A.shape, feat_B.shape)
        if index is not None:
            assert index.shape[0] == feat_A.shape[0], (index.shape, feat_A.shape)
        with_bank = bank is not None or neg_idx is not None or bank_ids is not None
        with_queue = queue_A is not None or queue_B is not None or queue_ids is not None
        if with_bank and with_queue:
            raise ValueError("MaskedContrastiveLoss: extra negatives come from a bank or a queue, not both")
        if with_bank:                                      # every refusal before a launch
            if (index is None) != (bank_ids is None):
                raise ValueError("MaskedContrastiveLoss: ids on one side only - give index and bank_ids, or neither")
            if bank is None or neg_idx is None:
                raise ValueError("MaskedContrastiveLoss: bank and neg_idx come together (a bank without lists, or lists without a bank)")
            ops.neg_operands("MaskedContrastiveLoss", feat_A, bank, neg_idx, index, bank_ids, self.a2b)
        if with_queue:
            ops.queue_operands("MaskedContrastiveLoss", feat_A, feat_B, queue_A, queue_B, index, queue_ids, self.a2b, self.b2a)
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
        if with_queue:
            return _InfoNCEQueueFn.apply(feat_A, feat_B, inv_temp, index, max(self.margin, 0.0), self.dcl, self.a2b, self.b2a, queue_A,
                                         queue_B, queue_ids, self)
        return _InfoNCEFn.apply(feat_A, feat_B, inv_temp, index, max(self.margin, 0.0), self.dcl, self.a2b, self.b2a)


class _SupConFn(torch.autograd.Function):
    """The whole of SupConLoss as ONE node.  ``views``: either ``features`` [bsz, V, E] alone or V tensors [bsz, E] (view v = rows v bsz ..
    of the contrast matrix); forward = sc_supcon_fwd, backward = sc_supcon_grad and the two feature products on the exact-fp32 GEMM."""

    @staticmethod
    def forward(ctx, inv_temp, labels, mask, anchor_views, base_temperature, *views):
        if len(views) == 1 and views[0].dim() == 3:                            # cat(unbind(features, 1), 0): row r = features[r % bsz, r // bsz]
            bsz, V, E = views[0].shape
            C = views[0].detach().float().transpose(0, 1).reshape(V * bsz, E)
        else:
            bsz, V = views[0].shape[0], len(views)
            C = torch.cat([v.detach().float() for v in views], 0)
        it = inv_temp.detach().float().reshape(1).contiguous()
        Na = anchor_views * bsz
        loss, logits, lse, _, poscnt = ops.supcon_fwd(C, Na, bsz, labels, mask, it, base_temperature)
        none = torch.empty(0)
        ctx.save_for_backward(C, logits, lse, poscnt, it, labels if labels is not None else none, mask if mask is not None else none)
        ctx.has = (labels is not None, mask is not None)
        ctx.it_shape = inv_temp.shape
        ctx.geom = (bsz, V, Na, base_temperature, [(v.dim(), v.dtype) for v in views])
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        C, logits, lse, poscnt, it, labels, mask = ctx.saved_tensors
        bsz, V, Na, base_temperature, views = ctx.geom
        labels, mask = labels if ctx.has[0] else None, mask if ctx.has[1] else None
        G, dot = ops.supcon_grad(logits, lse, poscnt, bsz, labels, mask, g.float().reshape(1).contiguous(), it, base_temperature)
        dT = dot.sum().reshape(ctx.it_shape) if ctx.needs_input_grad[0] else None   # d loss / d inv_temp (device scalar)
        dviews = [None] * len(views)
        if any(ctx.needs_input_grad[5:]):
            dC = ops.sgemm_mfma(G, C[:Na], a_kmajor=True, b_kmajor=True)       # G^T . C[:Na]  [N, E]   (G already carries inv_temp)
            dC[:Na] += ops.sgemm_mfma(G, C, b_kmajor=True)                     # G . C         [Na, E]: the anchors' own rows
            if len(views) == 1 and views[0][0] == 3:
                dviews = [dC.view(V, bsz, -1).transpose(0, 1).to(views[0][1])]
            else:
                dviews = [dC[v * bsz: (v + 1) * bsz].to(dt) if need else None
                          for v, ((_, dt), need) in enumerate(zip(views, ctx.needs_input_grad[5:]))]
        return (dT, None, None, None, None) + tuple(dviews)


class SupConLoss(nn.Module):
    """Supervised contrastive loss (Khosla et al., https://arxiv.org/abs/2004.11362; avssl/module/losses.py:8-123) on the HIP kernels of
    csrc/supcon.hip: samples that share a label are POSITIVES of one another - speech-image, speech-speech and image-image - where
    MaskedContrastiveLoss only takes them out of the negatives.  Without labels and mask it is the SimCLR loss.

    The reference's constructor and state: ``temperature`` is an ``nn.Parameter`` of shape [1] holding T itself when
    ``learnable_temperature`` (its state-dict key and shape), the python float otherwise; ``current_temperature`` as there.  The loss's
    factor is 1 / base_temperature (not T / base_temperature), as in the reference's text.  An anchor without a positive (one view and a
    label nobody shares, or a zero row of ``mask``) gives 0 / 0: a NaN loss, as the reference's - there is no host check and no
    synchronisation.  1 / T is formed by torch on the device, the node returns its gradient and autograd does the rest."""

    def __init__(self, temperature=0.07, contrast_mode="all", base_temperature=0.07, learnable_temperature=True):
        super().__init__()
        self.learnable_temperature = learnable_temperature
        if learnable_temperature:
            self.temperature = nn.Parameter(torch.FloatTensor([temperature]))
        else:
            self.temperature = temperature
        self.contrast_mode = contrast_mode
        self.base_temperature = base_temperature
        self._inv_temp_dev = {}

    @property
    def current_temperature(self):
        if self.learnable_temperature:
            return self.temperature.item()
        return self.temperature

    @property
    def temperature_for_logging(self):
        """``current_temperature`` without the device -> host synchronisation of ``.item()``: a 0-dim device tensor when the temperature
        is learnable (loggers accept tensors), the python float otherwise."""
        if self.learnable_temperature:
            return self.temperature.detach().float().reshape(())
        return float(self.temperature)

    def forward(self, features=None, labels=None, mask=None, *, feat_A=None, feat_B=None, index=None, bank=None, bank_ids=None,
                neg_idx=None, queue_A=None, queue_B=None, queue_ids=None):
        """With ``features`` [bsz, n_views, ...] (trailing dimensions flattened), ``labels`` [bsz] or ``mask`` [bsz, bsz] (float, may be
        asymmetric, any weights; no gradient) it is the reference's call, with the reference's ValueErrors.

        With ``feat_A`` / ``feat_B`` [bsz, E] and ``index`` it is the call ``compute_loss`` makes of every criterion: ``features =
        stack((feat_A, feat_B), 1)``, ``labels = index``.  Speech (feat_A) is view 0, so ``contrast_mode="one"`` anchors on speech only.
        This adapter is this project's decision: the reference's compute_loss passes ``feat_A=, feat_B=, index=`` to whatever criterion
        the yaml names, which its own SupConLoss.forward(features, labels, mask) answers with a TypeError - the reference cannot train
        with the class it ships.  Mined negatives (``bank`` / ``bank_ids`` / ``neg_idx``) and the cross-batch
        queue (``queue_A`` / ``queue_B`` / ``queue_ids``) stay MaskedContrastiveLoss's: a ValueError."""
        if bank is not None or bank_ids is not None or neg_idx is not None:
            raise ValueError("SupConLoss takes no negative bank (bank / bank_ids / neg_idx): mined negatives are MaskedContrastiveLoss's")
        if queue_A is not None or queue_B is not None or queue_ids is not None:
            raise ValueError("SupConLoss takes no negative queue (queue_A / queue_B / queue_ids): the cross-batch queue is "
                             "MaskedContrastiveLoss's")
        if features is None:
            if feat_A is None or feat_B is None:
                raise ValueError("SupConLoss: give `features` [bsz, n_views, ...], or feat_A and feat_B")
            if labels is not None or mask is not None:
                raise ValueError("SupConLoss: with feat_A / feat_B the labels come as `index`")
            if feat_A.dim() != 2 or feat_A.shape != feat_B.shape:
                raise ValueError(f"SupConLoss: feat_A {tuple(feat_A.shape)} and feat_B {tuple(feat_B.shape)} must be one shape [bsz, E]")
            views, labels = (feat_A, feat_B), index
            batch_size, n_views = feat_A.shape[0], 2
        else:
            if feat_A is not None or feat_B is not None or index is not None:
                raise ValueError("SupConLoss: give `features` or feat_A / feat_B / index, not both")
            if len(features.shape) < 3:
                raise ValueError("`features` needs to be [bsz, n_views, ...],at least 3 dimensions are required")
            if len(features.shape) > 3:
                features = features.reshape(features.shape[0], features.shape[1], -1)
            views = (features,)
            batch_size, n_views = features.shape[0], features.shape[1]
        if labels is not None and mask is not None:
            raise ValueError("Cannot define both `labels` and `mask`")
        if labels is not None:
            labels = labels.contiguous().view(-1)
            if labels.shape[0] != batch_size:
                raise ValueError("Num of labels does not match num of features")
            labels = labels.to(torch.int64)
        elif mask is not None:
            mask = mask.detach().float().contiguous()
        if self.contrast_mode == "one":
            anchor_views = 1
        elif self.contrast_mode == "all":
            anchor_views = n_views
        else:
            raise ValueError("Unknown mode: {}".format(self.contrast_mode))
        dev = views[0].device
        if self.learnable_temperature:
            inv_temp = self.temperature.reciprocal()
        else:                                              # constant: one device scalar per device, built once
            inv_temp = self._inv_temp_dev.get(dev)
            if inv_temp is None:
                inv_temp = self._inv_temp_dev[dev] = torch.full((1,), 1.0 / float(self.temperature), device=dev)
        return _SupConFn.apply(inv_temp, labels, mask, anchor_views, float(self.base_temperature), *views)


class _SigmoidLossFn(torch.autograd.Function):
    """The whole of SigmoidContrastiveLoss as ONE node over (feat_A, feat_B, t, b): forward = sc_sigmoid_loss_fwd, backward =
    sc_sigmoid_loss_grad, the two feature products on the exact-fp32 GEMM and the sums of the rows' d t / d b terms.  Nothing saved is
    written by the backward, so a second backward through the node returns the same numbers."""

    @staticmethod
    def forward(ctx, feat_A, feat_B, scale, bias, index, same_id, holder):
        A = ops.aligned16(feat_A.detach().float().contiguous())               # half-precision features are widened on the way in
        Bm = ops.aligned16(feat_B.detach().float().contiguous())
        t = scale.detach().float().reshape(1).contiguous()
        b = bias.detach().float().reshape(1).contiguous()
        ids = index.contiguous() if index is not None else None
        loss, s, counts = ops.sigmoid_loss_fwd(A, Bm, ids, t, b, same_id)
        holder.last_counts = counts
        ctx.save_for_backward(A, Bm, s, t, b, ids if ids is not None else torch.empty(0))
        ctx.has_ids = ids is not None
        ctx.same_id = same_id
        ctx.meta = (feat_A.dtype, feat_B.dtype, scale.shape, scale.dtype, bias.shape, bias.dtype)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        A, Bm, s, t, b, ids = ctx.saved_tensors
        dtype_A, dtype_B, t_shape, t_dtype, b_shape, b_dtype = ctx.meta
        ids = ids if ctx.has_ids else None
        G, dscale_part, dbias_part = ops.sigmoid_loss_grad(s, ids, g.float().reshape(1).contiguous(), t, b, ctx.same_id)
        dA = dB = dt = db = None
        if ctx.needs_input_grad[0]:
            dA = ops.sgemm_mfma(G, Bm, b_kmajor=True).to(dtype_A)              # G . B     (G already carries t)
        if ctx.needs_input_grad[1]:
            dB = ops.sgemm_mfma(G, A, a_kmajor=True, b_kmajor=True).to(dtype_B)   # G^T . A
        if ctx.needs_input_grad[2]:
            dt = dscale_part.sum().reshape(t_shape).to(t_dtype)               # d loss / d t (device scalar)
        if ctx.needs_input_grad[3]:
            db = dbias_part.sum().reshape(b_shape).to(b_dtype)
        return dA, dB, dt, db, None, None, None


class SigmoidContrastiveLoss(nn.Module):
    """Pairwise sigmoid loss of SigLIP (Zhai et al. 2023, https://arxiv.org/abs/2303.15343) on the HIP kernels of csrc/sigmoid_loss.hip:
    every (speech, image) pair of the gathered batch is a binary decision of its own, ``x_ij = t <A_i, B_j> + b`` against ``z_ij`` = +1
    on the diagonal and -1 off it, ``loss = (1 / B) sum_ij w_ij softplus(-z_ij x_ij)`` - no softmax, no denominator over the batch.

    ``same_id`` says what an off-diagonal pair whose items share an id (``index``) is: ``"ignore"`` (w = 0: MaskedContrastiveLoss's view of
    it, the default), ``"positive"`` (z = +1: SupConLoss's view) or ``"negative"`` (plain SigLIP).  Without ``index`` the three coincide.
    The normalisation is by B alone, so a row whose every negative is ignored is legal and contributes its positive term.

    ``logit_scale`` holds log(1 / temperature) and ``logit_bias`` holds ``bias``: 0-dim ``nn.Parameter``s when ``learnable``, buffers
    otherwise, in the state dict under those names either way.  ``t = exp(logit_scale)`` is formed by torch on the device, the node
    returns d loss / d t and d loss / d b and autograd does the rest: no host synchronisation in the step."""

    def __init__(self, temperature: float = 0.1, bias: float = -10.0, learnable: bool = True, same_id: str = "ignore"):
        super().__init__()
        if same_id not in ops.SIGMOID_SAME_ID:
            raise ValueError(f"SigmoidContrastiveLoss: same_id {same_id!r} is none of {', '.join(repr(k) for k in ops.SIGMOID_SAME_ID)}")
        if not float(temperature) > 0.0:
            raise ValueError(f"SigmoidContrastiveLoss: temperature {temperature} must be positive")
        self.learnable, self.same_id = bool(learnable), same_id
        scale, bias = torch.ones([]) * np.log(1 / temperature), torch.ones([]) * float(bias)
        if self.learnable:
            self.logit_scale, self.logit_bias = nn.Parameter(scale), nn.Parameter(bias)
        else:
            self.register_buffer("logit_scale", scale)
            self.register_buffer("logit_bias", bias)
            self._host_values()
        self.last_counts = None        # int32 [3] device tensor: positives, negatives, ignored pairs of the last call

    def _host_values(self):
        """the constants as python floats (not learnable only), read once here and again after a state dict is loaded"""
        self._temperature_host = float((-self.logit_scale.detach().float()).exp())
        self._bias_host = float(self.logit_bias.detach())

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        if not self.learnable:
            self._host_values()

    @property
    def current_temperature(self) -> float:
        return float((-self.logit_scale.detach().float()).exp())

    @property
    def temperature_for_logging(self):
        """1 / t without a device -> host synchronisation: a 0-dim device tensor when learnable (loggers accept tensors), the python
        float otherwise."""
        if self.learnable:
            return (-self.logit_scale.detach().float()).exp()
        return self._temperature_host

    @property
    def bias_for_logging(self):
        """b, as ``temperature_for_logging`` gives 1 / t"""
        if self.learnable:
            return self.logit_bias.detach().float().reshape(())
        return self._bias_host

    def forward(self, feat_A: torch.Tensor, feat_B: torch.Tensor, index: torch.LongTensor = None, *, bank=None, bank_ids=None,
                neg_idx=None, queue_A=None, queue_B=None, queue_ids=None) -> torch.Tensor:
        """``feat_A`` / ``feat_B`` [B, E] unit rows (fp32, or fp16 / bf16: widened on the way in, gradients in their own dtype), ``index``
        [B] int64 or None: the call ``compute_loss`` makes of every criterion.  Mined negatives (``bank`` / ``bank_ids`` / ``neg_idx``) and
        the cross-batch queue (``queue_A`` / ``queue_B`` / ``queue_ids``) stay MaskedContrastiveLoss's: a ValueError.  ``last_counts``
        [3] int32 (a device tensor, no sync) holds the positives, negatives and ignored pairs of the last call."""
        if bank is not None or bank_ids is not None or neg_idx is not None:
            raise ValueError("SigmoidContrastiveLoss takes no negative bank (bank / bank_ids / neg_idx): mined negatives are "
                             "MaskedContrastiveLoss's")
        if queue_A is not None or queue_B is not None or queue_ids is not None:
            raise ValueError("SigmoidContrastiveLoss takes no negative queue (queue_A / queue_B / queue_ids): the cross-batch queue is "
                             "MaskedContrastiveLoss's")
        ops.sigmoid_loss_operands("SigmoidContrastiveLoss", feat_A, feat_B, index, self.same_id, half_ok=True)
        return _SigmoidLossFn.apply(feat_A, feat_B, self.logit_scale.exp(), self.logit_bias, index, self.same_id, self)
