"""Frozen CLIP text tower as the cascaded branches use it: mirror of ClipModel.encode_keywords
(avssl/module/clip_official.py:222-279) over a restatement of openai/CLIP's text transformer (requirements.txt:4,
unpinned; the `clip` package and its weights are not available offline).

Architecture restated from the published model: token_embedding (V x W), learned positional_embedding (77 x W),
`layers` pre-LN residual blocks [ln_1 -> causal nn.MultiheadAttention(W, heads) ; ln_2 -> Linear(W, 4W) -> QuickGELU
(x * sigmoid(1.702 x)) -> Linear(4W, W)], ln_final, text_projection (W x E).  ViT-B/32: W = 512, 8 heads, 12 layers,
E = 512; ViT-L/14: W = 768, 12 heads, 12 layers, E = 768.  Parameter names follow openai/CLIP's state dict
(``model.token_embedding.weight``, ``model.transformer.resblocks.{i}.attn.in_proj_weight``, ...) so a real
checkpoint can be loaded with ``load_state_dict``.  The gradient flows THROUGH the frozen tower to the keyword embeddings:
the transformer blocks run on the library's kernels (clip_text_hip.py: bf16 GEMMs, causal attention forward and backward,
LayerNorm / QuickGELU forward and backward), ``ln_final`` and ``text_projection`` act on the B end-of-text rows only, in fp32
(row LayerNorm kernel + exact-fp32 matrix-pipe GEMM).  The nn modules below are PARAMETER CONTAINERS under openai/CLIP's names:
they have no arithmetic of their own - there is no stock-op or CPU path (a trainable text tower, which no shipped recipe uses,
raises).
"""
from collections import OrderedDict
from typing import Optional, Union

import torch
from torch import nn

CLIP_TEXT_ARCHS = {"ViT-B/32": dict(width=512, heads=8, layers=12, embed_dim=512),
                   "ViT-L/14": dict(width=768, heads=12, layers=12, embed_dim=768)}
SOT_TOKEN, EOT_TOKEN, CLIP_VOCAB, CONTEXT_LEN = 49406, 49407, 49408, 77


def _no_eager(what: str):
    raise RuntimeError(f"{what} holds the CLIP text tower's parameters only; the arithmetic runs on the HIP kernels through "
                       "ClipModel.encode_keywords (speechclip_plus_amd has no stock-op / CPU path)")


class QuickGELU(nn.Module):
    def forward(self, x: torch.Tensor):
        _no_eager("QuickGELU")


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model: int, n_head: int):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = nn.LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([("c_fc", nn.Linear(d_model, d_model * 4)), ("gelu", QuickGELU()),
                                              ("c_proj", nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = nn.LayerNorm(d_model)

    def forward(self, x: torch.Tensor, attn_mask: torch.Tensor = None):
        _no_eager("ResidualAttentionBlock")


class _TextTransformer(nn.Module):
    def __init__(self, width: int, layers: int, heads: int):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.ModuleList([ResidualAttentionBlock(width, heads) for _ in range(layers)])

    def forward(self, x: torch.Tensor, attn_mask: torch.Tensor = None):
        _no_eager("the text transformer")


class _ClipTextCore(nn.Module):
    """Holds the text-side parameters under openai/CLIP's names."""

    def __init__(self, vocab: int, width: int, heads: int, layers: int, embed_dim: int, seed: int = 1234):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, width)
        self.positional_embedding = nn.Parameter(torch.empty(CONTEXT_LEN, width))
        self.transformer = _TextTransformer(width, layers, heads)
        self.ln_final = nn.LayerNorm(width)
        self.text_projection = nn.Parameter(torch.empty(width, embed_dim))
        g = torch.Generator(device="cpu").manual_seed(seed)
        with torch.no_grad():            # CLIP's published init scales
            self.token_embedding.weight.copy_(torch.randn(vocab, width, generator=g) * 0.02)
            self.positional_embedding.copy_(torch.randn(CONTEXT_LEN, width, generator=g) * 0.01)
            self.text_projection.copy_(torch.randn(width, embed_dim, generator=g) * width ** -0.5)


class _EotHeadFn(torch.autograd.Function):
    """``ln_final`` + ``@ text_projection`` on the B end-of-text rows (clip_official.py:270-277), fp32, frozen parameters:
    sc_rowln_f32_fwd / _bwd and the exact-fp32 matrix-pipe GEMM; gradient w.r.t. the rows only."""

    @staticmethod
    def forward(ctx, rows, gamma, beta, eps, proj):
        from . import ops
        x = rows.detach().float().contiguous()
        g, b = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        y, xhat, rstd = ops.rowln_fwd(x, None, 0, g, b, eps)
        P = proj.detach().float().contiguous()                       # [W, E]: K-major for out = y @ P
        ctx.save_for_backward(xhat, rstd, g, P)
        return ops.sgemm_mfma(y, P, b_kmajor=True)

    @staticmethod
    def backward(ctx, d_out):
        from . import ops
        xhat, rstd, g, P = ctx.saved_tensors
        dy = ops.sgemm_mfma(d_out.float().contiguous(), P)           # dy[b, w] = sum_e d_out[b, e] P[w, e]
        scratch = torch.zeros(2, g.numel(), device=g.device, dtype=torch.float32)      # the frozen affine's gradient: discarded
        return ops.rowln_bwd(dy, xhat, g, rstd, scratch[0], scratch[1]), None, None, None, None


class ClipModel(nn.Module):
    """Text half of avssl/module/clip_official.py:ClipModel (image tower: out of scope, embeddings are inputs)."""

    def __init__(self, name: str = "ViT-B/32", device: str = "cuda", image_encoder_trainable: bool = False,
                 text_encoder_trainable: bool = False, reduce_subword_embbedding: Optional[Union[str, torch.Tensor]] = None,
                 layers: Optional[int] = None, seed: int = 1234, **kwargs):
        super().__init__()
        assert name in CLIP_TEXT_ARCHS, name
        a = dict(CLIP_TEXT_ARCHS[name])
        if layers is not None:
            a["layers"] = layers
        self.name, self.device = name, device
        self.text_encoder_trainable = text_encoder_trainable
        self.model = _ClipTextCore(CLIP_VOCAB, a["width"], a["heads"], a["layers"], a["embed_dim"], seed)
        self.out_dim = a["width"]
        # keyword counts that pointed behind the keyword tensor and were clamped by encode_keywords (device counter, read on request)
        self.register_buffer("eot_clamped", torch.zeros((), dtype=torch.int64), persistent=False)
        # ids outside the table and end-of-text positions behind the prefix that sc_text_assemble met (encode_text checks the range on
        # the host first: stays 0 unless that check is bypassed)
        self.register_buffer("text_bad", torch.zeros(1, dtype=torch.int64), persistent=False)
        self.tokenizer = None                    # attach a BPE tokenizer (openai/CLIP's SimpleTokenizer interface) for prep_text
        self.selected_text_emb_ids = None
        if reduce_subword_embbedding is not None:
            # clip_official.py:63-108: keep only the sub-words seen in the captions.  Accepts the reference's .npy path
            # (columns id, frequency) or a 1-D tensor of original token ids.
            if isinstance(reduce_subword_embbedding, str):
                import numpy as np
                ids = torch.from_numpy(np.load(reduce_subword_embbedding)[:, 0].astype("int64"))
            else:
                ids = reduce_subword_embbedding.long().cpu()
            self.selected_text_emb_ids = ids
            self.model.token_embedding = nn.Embedding.from_pretrained(self.model.token_embedding.weight.detach()[ids])
            self.original2Reduced = {int(o): n for n, o in enumerate(ids.tolist())}
            self.reducedl2Original = {n: int(o) for n, o in enumerate(ids.tolist())}
            self.startOfTxt_reduced = self.original2Reduced[SOT_TOKEN]
            self.endOfTxt_reduced = self.original2Reduced[EOT_TOKEN]
        if not text_encoder_trainable:
            for p in self.model.parameters():
                p.requires_grad = False
        self.to(device)

    def _check_tower(self) -> None:
        core = self.model
        heads = core.transformer.resblocks[0].attn.num_heads
        if self.text_encoder_trainable:
            raise NotImplementedError("text_encoder_trainable: no shipped recipe trains the CLIP text tower; only the frozen tower "
                                      "(forward + input gradient) is built")
        if core.transformer.width != 64 * heads:
            raise NotImplementedError(f"text tower head_dim {core.transformer.width // heads}: the attention kernels are built for 64")

    def _tower_weights(self, dev):
        """bf16 (+ transposed) copies of the frozen tower's weights, (re)converted when a checkpoint is loaded or the module moves"""
        from .clip_text_hip import prepare_weights
        core = self.model
        key = (dev, tuple((p.data_ptr(), p._version) for p in core.transformer.parameters()))
        if getattr(self, "_hip_key", None) != key:
            self._hip_weights, self._hip_key = prepare_weights(core.transformer, dev), key
        return self._hip_weights

    def _transformer(self, x: torch.Tensor) -> torch.Tensor:
        """(B, T <= 77, W) -> (B, T, W) on the library's bf16 kernels, forward and input gradient (clip_text_hip.TextTowerFn).  The
        tower is frozen in every shipped recipe (clip_official.py:113-134) and both published towers have head_dim 64."""
        if not x.is_cuda:
            raise RuntimeError("the CLIP text tower runs on the HIP kernels: device tensors only")
        self._check_tower()
        from .clip_text_hip import TextTowerFn
        return TextTowerFn.apply(x, self._tower_weights(x.device), self.model.transformer.resblocks[0].attn.num_heads)

    def update_device(self, device):
        self.device = device

    def to(self, *args, **kwargs):
        super().to(*args, **kwargs)
        self.device = self.model.token_embedding.weight.device
        return self

    def _prompt_constants(self, dev):
        """(tok [3, W] = embeddings of SOT, EOT and token 0; pos [77, W]) as fp32 device tensors, per parameter version"""
        emb, posp = self.model.token_embedding.weight, self.model.positional_embedding
        key = (str(dev), emb.data_ptr(), emb._version, posp.data_ptr(), posp._version)
        if getattr(self, "_prompt_key", None) != key:
            sot, eot = (SOT_TOKEN, EOT_TOKEN) if self.selected_text_emb_ids is None else (self.startOfTxt_reduced, self.endOfTxt_reduced)
            tok = emb.detach()[torch.tensor([sot, eot, 0], device=emb.device)].to(device=dev, dtype=torch.float32).contiguous()
            self._prompt_const = (tok, posp.detach().to(device=dev, dtype=torch.float32).contiguous())
            self._prompt_key = key
        return self._prompt_const

    def encode_keywords(self, keywords: torch.Tensor, keyword_num: Union[int, torch.Tensor]) -> torch.Tensor:
        """clip_official.py:222-279: [SOT, kw_1 .. kw_n, EOT, 0 ...] -> text transformer -> EOT row @ text_projection."""
        if not isinstance(keywords, torch.Tensor):
            raise TypeError(f"Unknown keywords type {type(keywords)}")
        bsz = keywords.size(0)
        dev = keywords.device
        ln = self.model.ln_final
        if isinstance(keyword_num, torch.Tensor):
            # per-sample keyword counts (the CIF branches): prompt assembly, the tower's padding and the end-of-text gather are
            # single launches around the tower (clip_text_hip.KeywordTowerFn, csrc/prompt.hip).  The tower is causal and only the
            # end-of-text row is read: positions behind the LAST end-of-text token of the batch cannot influence any output, and
            # keywords.shape[1] is the batch's largest keyword count (sized on the host), so the prefix [SOT, kw_1 .. kw_N, EOT] =
            # N + 2 positions is all the transformer sees.  A count that points behind the keyword tensor (a caller error the
            # reference reports as a shape mismatch on the host) is clamped into the prefix and counted in ``eot_clamped`` instead of
            # indexing out of bounds on the device.
            if not keywords.is_cuda:
                raise RuntimeError("the CLIP text tower runs on the HIP kernels: device tensors only")
            self._check_tower()
            from .clip_text_hip import KeywordTowerFn
            n_pos = min(CONTEXT_LEN, keywords.shape[1] + 2)
            tok, pos = self._prompt_constants(dev)
            heads = self.model.transformer.resblocks[0].attn.num_heads
            rows = KeywordTowerFn.apply(keywords, keyword_num.to(dev), tok, pos, self._tower_weights(dev), heads, n_pos, self.eot_clamped)
            return _EotHeadFn.apply(rows, ln.weight, ln.bias, ln.eps, self.model.text_projection)
        sot, eot = (SOT_TOKEN, EOT_TOKEN) if self.selected_text_emb_ids is None else (self.startOfTxt_reduced, self.endOfTxt_reduced)
        text = torch.zeros([bsz, CONTEXT_LEN], device=dev, dtype=torch.long)
        text[:, 0] = sot
        text[:, keyword_num + 1] = eot
        x = self.model.token_embedding(text)
        x = torch.cat([x[:, :1], keywords, x[:, 1 + keyword_num:]], dim=1)
        x = x + self.model.positional_embedding
        n_pos = min(CONTEXT_LEN, int(keyword_num) + 2)          # the causal prefix up to the end-of-text position
        x = self._transformer(x[:, :n_pos])
        return _EotHeadFn.apply(x[:, 1 + keyword_num], ln.weight, ln.bias, ln.eps, self.model.text_projection)

    # ------------------------------------------------------------------------------------------------- captions
    def to_reduced_ids(self, text: torch.Tensor) -> torch.Tensor:
        """ORIGINAL CLIP token ids -> ids of the reduced table through one lookup tensor (a new tensor: the caller's is not written;
        clip_official.py:178-181 / kwClip.py:518-524 loop over every element in Python).  An id that is not in the reduced vocabulary
        raises ValueError - at once for host ids; device ids come back with -1 in its place and encode_text, which reads the id range
        anyway, raises for it (``_original``), so that the mapping costs no host read of its own.  Full vocabulary: ``text`` itself."""
        if self.selected_text_emb_ids is None:
            return text
        lut = getattr(self, "_o2r_lut", None)
        if lut is None or lut.device != text.device:
            lut = torch.full((CLIP_VOCAB + 1,), -1, dtype=torch.int64)           # last entry: every id outside the CLIP vocabulary
            lut[self.selected_text_emb_ids] = torch.arange(self.selected_text_emb_ids.numel())
            lut = self._o2r_lut = lut.to(text.device)
        t = text.long()
        out = lut[torch.where((t < 0) | (t >= CLIP_VOCAB), CLIP_VOCAB, t)]
        missing = t[out < 0] if not t.is_cuda else t[:0]
        if missing.numel():
            raise ValueError(f"token id {int(missing[0])} is not in the reduced vocabulary ({self.selected_text_emb_ids.numel()} sub-words)")
        return out

    def prep_text(self, sents: list) -> torch.Tensor:
        """clip_official.py:168-182 (clip.tokenize): sentences -> [B, 77] int64 ids of the table in use, [SOT, BPE ids, EOT, 0 ...].
        The BPE vocabulary is not part of this package: ``self.tokenizer`` must have been attached (``encode(str) -> list of ids``,
        openai/CLIP's SimpleTokenizer)."""
        if getattr(self, "tokenizer", None) is None:
            raise RuntimeError("prep_text needs a tokenizer: attach one as `clip.tokenizer` (openai/CLIP's SimpleTokenizer interface; "
                               "INTEGRATION.md) or pass token ids to encode_text / forward_text")
        if isinstance(sents, str):
            sents = [sents]
        res = torch.zeros(len(sents), CONTEXT_LEN, dtype=torch.int64)
        for i, sent in enumerate(sents):
            toks = [SOT_TOKEN] + list(self.tokenizer.encode(sent)) + [EOT_TOKEN]
            if len(toks) > CONTEXT_LEN:
                raise RuntimeError(f"Input {sent} is too long for context length {CONTEXT_LEN}")
            res[i, : len(toks)] = torch.tensor(toks, dtype=torch.int64)
        return self.to_reduced_ids(res)

    def encode_text(self, text: torch.Tensor, bucket: bool = True, _original: Optional[torch.Tensor] = None) -> torch.Tensor:
        """clip_official.py:213-220 -> openai/CLIP ``encode_text``: text [B, L <= 77] integer ids OF THE TABLE IN USE (reduced ids when
        the vocabulary is reduced) -> [B, embed_dim] fp32, token_embedding + positional_embedding -> transformer -> ln_final -> the row
        at ``text.argmax(-1)`` @ text_projection.  Forward-only, under no_grad (the tower is frozen).  The tower is causal and only the
        end-of-text row is read, so every caption runs on its own prefix at its own segment class (clip_text_hip.text_buckets;
        ``bucket`` False: the whole batch at the class of its longest caption - the baseline the bucketing is measured against).
        ``text`` may live on the host: the end-of-text positions are then computed there and only the ids are uploaded; for device ids
        the positions and the id range come back in one small copy."""
        if not isinstance(text, torch.Tensor):
            raise TypeError(f"Unknown text type {type(text)}")
        if text.dim() != 2 or text.shape[1] > CONTEXT_LEN or text.shape[1] < 1 or text.shape[0] < 1:
            raise ValueError(f"Incorrect text tensor shape {tuple(text.shape)}: [B, L <= {CONTEXT_LEN}] token ids")
        if text.dtype.is_floating_point or text.dtype.is_complex or text.dtype == torch.bool:
            raise TypeError(f"text must hold integer token ids, got {text.dtype}")
        self._check_tower()
        emb = self.model.token_embedding.weight
        V, B = emb.shape[0], text.shape[0]
        with torch.no_grad():
            t = text.detach().to(torch.int64)
            stats = torch.cat([t.argmax(dim=-1), t.amin().reshape(1), t.amax().reshape(1)]).tolist()   # device ids: the one copy to the host
            eot_pos, lo, hi = stats[:B], stats[B], stats[B + 1]
            if lo < 0 and _original is not None:         # ids mapped by to_reduced_ids on the device: name the caller's id
                raise ValueError(f"token id {int(_original[t < 0][0])} is not in the reduced vocabulary ({V} sub-words)")
            if lo < 0 or hi >= V:
                raise ValueError(f"token id {lo if lo < 0 else hi} is outside the token table in use [0, {V})")
            dev = emb.device
            if not emb.is_cuda:
                raise RuntimeError("the CLIP text tower runs on the HIP kernels: device tensors only")
            from . import ops
            from .clip_text_hip import text_rows
            t = t.to(dev)
            if t.stride(1) != 1:
                t = t.contiguous()
            table = ops.aligned16(emb.detach() if emb.dtype == torch.float32 else emb.detach().float())
            if table.stride(1) != 1 or table.stride(0) % 4:
                table = table.contiguous()
            heads = self.model.transformer.resblocks[0].attn.num_heads
            rows, order = text_rows(t, eot_pos, table, self._prompt_constants(dev)[1], self._tower_weights(dev), heads, bucket=bucket,
                                    bad=self.text_bad)
            ln = self.model.ln_final
            out = _EotHeadFn.apply(rows, ln.weight, ln.bias, ln.eps, self.model.text_projection)
            if order is not None:                        # back to input order
                out = torch.empty_like(out).index_copy_(0, order, out)
            return out
