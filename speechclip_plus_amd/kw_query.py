"""The K keyword rows of the fixed-keyword cascaded branch, forward and backward, without the full-sequence attention.

What the reference computes (avssl/model/kw_branches.py:365-374 over MultiheadAttentionAndNorm, TransformerModels.py:120-126):
``LN(MHA(src, src, src, mask) + src)[:, :K]`` with ``src = [cls_1..cls_K ; feat]``.  Only the K rows of the learned queries are
kept and those queries are parameters, so (csrc/kwpool.hip) per query k and head h

    q = Wq cls + bq ;  a_kh = dh^-1/2 Wk_h^T q_kh ;  c = a cls^T          (parameters only: cached per parameter version)
    p = softmax([c_kh ; a_kh . X[b, t]]) ;  m[b,kh] = sum_j p_j cls_j + sum_t p_t X[b,t]
    ctx_k = concat_h(Wv_h m[b,kh] + bv_h sum(p mult)) ;  out_k = LN(cls_k + Wo ctx_k + bo)

(bk shifts every score of a query alike and cancels in the softmax, so it receives a zero gradient, as in the reference.)  The
K-row chain runs in fp32 on the master weights (sc_sgemm_f32_ex, sc_rowln_f32_*).  One autograd node; the block's parameters are
inputs of the node and get their gradients as its return values (mha_block.MhaNormFn's convention), the weighted-sum logits get
theirs through the encoder handle (head_tail.ParallelHeadFn's), a plain ``feat`` its own.

Train mode applies nn.MultiheadAttention's dropout to the attention weights (a [B, K H, K + R] multiplier consumed by the kernel)."""
import torch

from . import ops


def _f(*shape, dev):
    return torch.empty(*shape, device=dev, dtype=torch.float32)


def kw_query(module, cls: torch.Tensor):
    """(x0 [K, D], q [K, D], Qm [K H, D], a [K H, D], c [K H, K]): the queries folded into the key projection.  Parameters only, so
    cached per parameter version like head_tail.cls_query."""
    from .optim import param_generation
    att = module.multihead_attn_layer
    key = (param_generation(), cls.data_ptr(), cls._version, att.in_proj_weight.data_ptr(), att.in_proj_weight._version,
           att.in_proj_bias._version)
    cache = getattr(module, "_sc_kw_query", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    D, H = att.embed_dim, att.num_heads
    dh = D // H
    K = cls.shape[-2]
    dev = cls.device
    Wi, bi = att.in_proj_weight.detach(), att.in_proj_bias.detach()
    x0 = cls.detach().reshape(K, D).float().contiguous()
    q = _f(K, D, dev=dev)
    ops.sgemm_ex(x0, (D, 1, 0), Wi[:D], (D, 1, 0), q, D, K, D, D, bias=bi[:D])
    if H == 1:
        Qm = q
    else:
        Qm = _f(K * H, D, dev=dev)
        for k in range(K):
            ops.headmask(q[k: k + 1], Qm[k * H: (k + 1) * H], H, D, dh, gather=False)
    a = _f(K * H, D, dev=dev)
    ops.sgemm_ex(Qm, (D, 1, 0), Wi[D: 2 * D], (1, D, 0), a, D, K * H, D, D, alpha=dh ** -0.5)
    c = _f(K * H, K, dev=dev)
    ops.sgemm_ex(a, (D, 1, 0), x0, (D, 1, 0), c, K, K * H, K, D)
    val = (x0, q, Qm, a, c)
    module._sc_kw_query = (key, val)
    return val


class KwQueryFn(torch.autograd.Function):
    """inputs : cls [1, K, D], in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, LayerNorm weight, bias (parameters),
                ws_weights (weighted-sum logits or None), feat (plain path or None), then constants: the block module, the encoder
                handle, X [B, R, D] bf16, flen int32 [B], row0
       output : [B, K, D] fp32"""

    @staticmethod
    def forward(ctx, cls, Wi, bi, Wo, bo, g, beta, ws_weights, feat, module, handle, X, flen, row0):
        att, norm = module.multihead_attn_layer, module.attentionBlock_Norm
        D, H = att.embed_dim, att.num_heads
        dh = D // H
        K = cls.shape[-2]
        Q = K * H
        X = X.detach()
        B, R, _ = X.shape
        dev = X.device
        x0, q, Qm, a, c = kw_query(module, cls)
        Wi_, bi_ = Wi.detach(), bi.detach()
        pd = float(att.dropout) if module.training else 0.0
        mult = None
        if pd > 0:
            n = B * Q * (K + R)
            mult = ops.dropout_mult(((n + 7) // 8 * 8,), pd, dev)[:n].view(B, Q, K + R)
        p, m, psum = ops.kw_pool_fwd(X, a, c, x0, flen, row0, mult, want_psum=True)
        # ---- value projection per head: cx[(b,k), h] = Wv_h m[b, k H + h] + bv_h sum(p mult)   (eval: the weights sum to 1)
        BK = B * K
        cx = _f(BK, D, dev=dev)
        ops.sgemm_ex(m, (H * D, 1, D), Wi_[2 * D:], (D, 1, dh * D), cx, D, BK, dh, D, nbatch=H, scz=dh,
                     bias=bi_[2 * D:] if mult is None else None, sbiasz=dh)
        if mult is not None:
            cx.view(BK, H, dh).addcmul_(psum.view(BK, H, 1), bi_[2 * D:].view(1, H, dh))
        attn = _f(BK, D, dev=dev)
        ops.sgemm_ex(cx, (D, 1, 0), Wo.detach(), (D, 1, 0), attn, D, BK, D, D, bias=bo.detach())
        res = x0.repeat(B, 1)                                    # row (b, k) adds cls_k
        out, xhat, rstd = ops.rowln_fwd(attn, res, D, g.detach().float().contiguous(), beta.detach().float().contiguous(), norm.eps)
        ctx.mod, ctx.handle, ctx.dims, ctx.row0 = module, handle, (B, R, D, H, K), row0
        ctx.feat_meta = None if feat is None else (feat.shape, feat.dtype)
        ctx.mult = mult
        ctx.save_for_backward(X, flen, x0, q, Qm, a, p, m, psum, cx, xhat, rstd, Wi_, Wo.detach(), g.detach().float().contiguous())
        return out.view(B, K, D)

    @staticmethod
    def backward(ctx, d_out):
        X, flen, x0, q, Qm, a, p, m, psum, cx, xhat, rstd, Wi, Wo, g = ctx.saved_tensors
        B, R, D, H, K = ctx.dims
        row0, mult = ctx.row0, ctx.mult
        dh, Q, BK = D // H, K * H, B * K
        dev = X.device
        Wq, Wk, Wv = Wi[:D], Wi[D: 2 * D], Wi[2 * D:]
        gWi, gbi = _f(3 * D, D, dev=dev), torch.zeros(3 * D, device=dev, dtype=torch.float32)
        gWo, gbo = _f(D, D, dev=dev), _f(D, dev=dev)
        dg, dbeta = torch.zeros(D, device=dev, dtype=torch.float32), torch.zeros(D, device=dev, dtype=torch.float32)
        dy = d_out.float().contiguous().view(BK, D)
        # ---- LayerNorm over (cls_k + attn): d attn = dz, d cls_k += sum_b dz[(b,k)]
        dz = ops.rowln_bwd(dy, xhat, g, rstd, dg, dbeta)
        d_x0 = _f(K, D, dev=dev)
        ops.colsum(dz, K * D, B, K * D, d_x0)
        # ---- out_proj
        ops.sgemm_ex(dz, (1, D, 0), cx, (1, D, 0), gWo, D, D, D, BK)
        ops.colsum(dz, D, BK, D, gbo)
        dcx = _f(BK, D, dev=dev)
        ops.sgemm_ex(dz, (D, 1, 0), Wo, (1, D, 0), dcx, D, BK, D, D)
        # ---- value projection: Wv_h += dcx_h^T m_h ; bv_h += sum dcx_h psum ; dm_h = dcx_h Wv_h
        ops.sgemm_ex(dcx, (1, D, dh), m, (1, H * D, D), gWi[2 * D:], D, dh, D, BK, nbatch=H, scz=dh * D)
        cbias = None
        if mult is not None:                  # dropped weights do not sum to 1: the bias path reaches the attention weights
            cbias = ops.rt_value_bias_bwd(dcx, ctx.mod.multihead_attn_layer.in_proj_bias.detach()[2 * D:].contiguous(),
                                          psum.view(BK, H), gbi[2 * D:], H).view(B, Q)
        else:
            ops.colsum(dcx, D, BK, D, gbi[2 * D:])
        dm = _f(B, Q, D, dev=dev)
        ops.sgemm_ex(dcx, (D, 1, dh), Wv, (1, D, dh * D), dm, H * D, BK, D, dh, nbatch=H, scz=D)
        # ---- pooling backward (two sweeps over X); the weighted-sum sweep takes bf16 rows
        hd = ctx.handle
        if hd is not None:
            hd.check_fresh()
        to_ws = hd is not None and ctx.needs_input_grad[7]
        plain = hd is not None and hd.lazy is None and hd.layers_bwd is None and ctx.feat_meta is None
        dX, da, dc = ops.kw_pool_bwd(X, a, x0, flen, row0, p, dm, mult, cbias,
                                     dx_dtype=torch.bfloat16 if (to_ws and plain) else torch.float32)
        # ---- the constant keys: rows (d cls += sum w dm) and scores c = a cls^T
        w = p[:, :, :K] if mult is None else p[:, :, :K] * mult[:, :, :K]
        w = w.reshape(B * Q, K).contiguous()
        ops.sgemm_ex(w, (1, K, 0), dm, (1, D, 0), d_x0, D, K, D, B * Q, beta=1.0)
        ops.sgemm_ex(dc, (K, 1, 0), x0, (1, D, 0), da, D, Q, D, K, beta=1.0)
        ops.sgemm_ex(dc, (1, K, 0), a, (1, D, 0), d_x0, D, K, D, Q, beta=1.0)
        # ---- a = s Qm Wk ;  q = Wq cls + bq   (bk receives exactly zero)
        s = dh ** -0.5
        ops.sgemm_ex(Qm, (1, D, 0), da, (1, D, 0), gWi[D: 2 * D], D, D, D, Q, alpha=s)
        dQm = _f(Q, D, dev=dev)
        ops.sgemm_ex(da, (D, 1, 0), Wk, (D, 1, 0), dQm, D, Q, D, D, alpha=s)
        if H == 1:
            dq = dQm
        else:
            dq = _f(K, D, dev=dev)
            for k in range(K):
                ops.headmask(dq[k: k + 1], dQm[k * H: (k + 1) * H], H, D, dh, gather=True)
        ops.sgemm_ex(dq, (1, D, 0), x0, (1, D, 0), gWi[:D], D, D, D, K)
        ops.colsum(dq, D, K, D, gbi[:D])
        ops.sgemm_ex(dq, (D, 1, 0), Wq, (1, D, 0), d_x0, D, K, D, D, beta=1.0)
        d_ws, d_feat = None, None
        if to_ws:
            d_ws = ops.wsum_bwd_logits(hd.hidden, dX, hd.w_soft, B, R, D, 1, normalize=hd.normalize, lazy=hd.lazy, seg=hd.seg)
        if hd is not None and hd.layers_bwd is not None:           # unfrozen HuBERT layers: continue the chain below the weighted sum
            hd.layers_bwd(dX, hd.w_soft)
        if hd is not None:
            hd.release()
        if ctx.feat_meta is not None and ctx.needs_input_grad[8]:
            shape, dtype = ctx.feat_meta
            d_feat = dX[:, row0: row0 + shape[1]].to(dtype)
        return (d_x0.view(1, K, D), gWi, gbi, gWo, gbo, dg, dbeta, d_ws, d_feat, None, None, None, None, None)
