"""Keyword detokenisation: for every keyword embedding the K nearest rows of the CLIP token table, on the device.

What the reference computes (avssl/util/model_utils.py:41-252, called by kwClip.py:295-443 at every validation epoch that logs):
``F.cosine_similarity`` of a [rows, E, 1] tensor against [1, E, V] (or ``keywords @ pinv(table^T)^T``) and ``torch.topk``, batch by
batch on the CPU, then every neighbour decoded next to the gold caption.  The paper's keyword hit rate is computed from that output.

How it runs here:

    keyword_neighbors   rows in chunks -> cosine scores to fp32 accuracy on the bf16 matrix pipe (VocabTables + ops.cosine_scores_split:
                        the quantiser's own score path; exact-fp32 ops.sgemm_mfma for ``pseudo_inverse``) into ONE reused score
                        buffer -> per-row top-K (ops.topk_rows, csrc/topk.hip) -> (vals [B, N, K] fp32, idx [B, N, K] int64)
    extract_fixed_keyword_neighbors / extract_dynamic_keyword_neighbors
                        the reference's functions (same argument names, same result list) on keyword_neighbors with one
                        device-to-host copy of (vals, idx) per call; ``neighbors_to_entries`` is their host half
    keyword_statistics  mean / std / norm per keyword slot, kw_mean_mse, kw_std_mse (kwClip.py:325-353) on the device
    keyword_hit_rate    integer ops on (B, N, K) x (B, 77): does one of a keyword's K neighbours occur in the caption

There is no CPU path for the scores and the selection: device tensors only.  The host halves (result structure, id mapping,
hit rate) are plain torch / python and are tested without a GPU.
"""
from collections import defaultdict
from typing import Callable, List, Optional, Sequence, Union

import torch

__all__ = ["keyword_neighbors", "extract_fixed_keyword_neighbors", "extract_dynamic_keyword_neighbors", "neighbors_to_entries",
           "TokenDecoder", "keyword_statistics", "keyword_hit_rate", "default_chunk_rows", "SCORE_SCRATCH_BYTES"]

# Score scratch of one chunk.  Chosen from the MI355X's 256 MiB Infinity Cache: the GEMM writes a chunk's scores and the selection
# reads them once, so a chunk whose scores fit the cache is read back from it instead of from HBM.  Half the cache, not all of it:
# the GEMM streams the split token table through the same cache while it writes (6 x 2 bytes x E per vocabulary row: 50 MB at
# V = 8 112 / E = 512, 183 MB at 19 787 / 768, 303 MB at 49 408 / 512).
SCORE_SCRATCH_BYTES = 128 << 20
SOT_TOKEN, EOT_TOKEN, PAD_TOKEN = 49406, 49407, 0          # CLIP's <|startoftext|>, <|endoftext|> and the caption padding
_DEFAULT_CACHE: dict = {}


def _roundup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def default_chunk_rows(V: int, scratch_bytes: int = SCORE_SCRATCH_BYTES) -> int:
    """Rows per chunk whose fp32 scores ([rows, V rounded up to 128]) fit ``scratch_bytes``: a multiple of 128 (the GEMM's row
    tile), at least 128.  4096 rows at V = 8 112, 1664 at 19 787, 640 at 49 408."""
    return max(128, scratch_bytes // (4 * _roundup(V, 128)) // 128 * 128)


def _tables(token_table: torch.Tensor, tables):
    from .vector_quantizers import VocabTables
    if isinstance(tables, VocabTables):
        assert (tables.V, tables.Et) == tuple(token_table.shape), ((tables.V, tables.Et), token_table.shape)
        return tables
    return VocabTables.of(token_table, _DEFAULT_CACHE if tables is None else tables)


def _pinv(tb) -> torch.Tensor:
    """pinv(table^T) [V, E]: fp64 on the host, once per table version (kept on the VocabTables, which is rebuilt per version)."""
    p = getattr(tb, "_pinv", None)
    if p is None:
        p = torch.linalg.pinv(tb.table.detach().double().cpu().t()).float().contiguous().to(tb.table.device)
        tb._pinv = p
    return p


def keyword_neighbors(keywords: torch.Tensor, token_table: torch.Tensor, K: int, keywords_len: Optional[torch.Tensor] = None,
                      retrieve_method: str = "cosine", tables=None, chunk_rows: Optional[int] = None):
    """keywords [B, N, E] (or [rows, E]), token_table [V, E] -> (vals [B, N, K] fp32, idx [B, N, K] int64), best first, on the device.

    ``retrieve_method``: "cosine" (model_utils.py:91-95; no special-token masking, as the reference) or "pseudo_inverse"
    (:79-89: ``keywords @ pinv(table^T)^T``, the pseudo-inverse computed once per table version in fp64 on the host).
    ``keywords_len`` [B]: slots at or past an utterance's count are not scored and come back as -inf / -1 (the reference scores
    them and throws them away).  ``tables``: a VocabTables of ``token_table`` or the cache dict one is kept in (the quantiser's
    ``_tables``); None: a module-level cache.  ``chunk_rows``: rows scored per pass, rounded up to a multiple of 128; the default
    (``default_chunk_rows``) is the largest chunk whose fp32 scores fit SCORE_SCRATCH_BYTES = 128 MiB, half the 256 MiB Infinity
    Cache, so the selection reads what the GEMM just wrote from the cache whatever the epoch size.  One score buffer and one
    split-operand buffer are allocated per call and reused by every chunk.  Ties and NaN: the order of ops.topk_rows.  The order is
    the order of the fp32 score matrix; for "cosine" the returned values are then re-evaluated for the K selected columns with fp64
    accumulation (ops.topk_rescore_cos), so two neighbours closer than the matrix's accumulation error (below 1e-6 away from a
    score of 1) can appear in either order next to exact values."""
    from . import ops
    if retrieve_method not in ("cosine", "pseudo_inverse"):
        raise NotImplementedError(retrieve_method)
    if not keywords.is_cuda or not token_table.is_cuda:
        raise RuntimeError("keyword_neighbors runs on the HIP kernels: device tensors only")
    squeeze = keywords.dim() == 2
    if squeeze:
        keywords = keywords.unsqueeze(0)
    B, N, E = keywords.shape
    V = token_table.shape[0]
    assert token_table.shape[1] == E, (token_table.shape, keywords.shape)
    assert 1 <= K <= 32, f"K = {K}: the selection kernel keeps at most 32 neighbours"
    dev = keywords.device
    kw = keywords.detach().reshape(B * N, E).float().contiguous()
    sel = None
    if keywords_len is not None:
        lens = torch.as_tensor(keywords_len, device=dev).long()
        assert lens.shape == (B,), (lens.shape, B)
        sel = (torch.arange(N, device=dev).unsqueeze(0) < lens.unsqueeze(1)).reshape(-1).nonzero().squeeze(1)
        kw = kw.index_select(0, sel)
    R = kw.shape[0]
    vals = torch.empty(R, K, device=dev, dtype=torch.float32)
    idx = torch.empty(R, K, device=dev, dtype=torch.int32)
    if R > 0:
        tb = _tables(token_table, tables)
        chunk = default_chunk_rows(V) if chunk_rows is None else max(128, _roundup(int(chunk_rows), 128))
        chunk = min(chunk, _roundup(R, 128))
        scores = torch.empty(chunk, tb.Vp, device=dev, dtype=torch.float32)          # the one score scratch of the call
        if retrieve_method == "cosine":
            _, rnorm = ops.vq_prep(kw)                                                # 1 / max(|kw|, 1e-8): the quantiser's normalisation
            split = torch.empty(chunk, tb.norm_split.shape[1], device=dev, dtype=torch.bfloat16)
        else:
            pinv = _pinv(tb)
        for r0 in range(0, R, chunk):
            r1 = min(R, r0 + chunk)
            rp = _roundup(r1 - r0, 128)
            if retrieve_method == "cosine":
                ops.cosine_scores_split(kw[r0:r1], rnorm[r0:r1], tb.norm_split, tb.Vp, out=scores[:rp], split_out=split[:rp])
            else:
                ops.sgemm_mfma(kw[r0:r1], pinv, out=scores[: r1 - r0, :V])
            ops.topk_rows(scores[: r1 - r0], V, K, vals=vals[r0:r1], idx=idx[r0:r1])
        if retrieve_method == "cosine":
            # the score matrix is accumulated in fp32 over 6 E products: a few 1e-6 low at a score of 1 (a quantised keyword against its
            # own token).  It decides the ORDER; the values written next to the tokens are re-evaluated with fp64 accumulation
            ops.topk_rescore_cos(kw, tb.table, idx, vals)
    idx = idx.long()
    if sel is not None:
        full_v = torch.full((B * N, K), float("-inf"), device=dev, dtype=torch.float32)
        full_i = torch.full((B * N, K), -1, device=dev, dtype=torch.int64)
        full_v.index_copy_(0, sel, vals)
        full_i.index_copy_(0, sel, idx)
        vals, idx = full_v, full_i
    vals, idx = vals.view(B, N, K), idx.view(B, N, K)
    return (vals[0], idx[0]) if squeeze else (vals, idx)


# ------------------------------------------------------------------------------------------------ host half: the reference's result
class TokenDecoder:
    """model_utils.py:17-28 (SpeechCLIPDecoder) without the hard dependency on a BPE tokenizer: reduced index -> original CLIP
    token id (``clip.reducedl2Original`` when the vocabulary is reduced) -> ``decode(id)`` if given, else
    ``clip.tokenizer.decoder[id]`` if the CLIP wrapper has a tokenizer, else the original token id itself."""

    def __init__(self, clip=None, decode: Optional[Callable[[int], object]] = None):
        self.index_mapping = None
        if clip is not None and getattr(clip, "selected_text_emb_ids", None) is not None:
            self.index_mapping = clip.reducedl2Original
        tok = getattr(clip, "tokenizer", None) if clip is not None else None
        self._table = getattr(tok, "decoder", None)
        self._decode = decode

    def original_id(self, token_id: int) -> int:
        return int(self.index_mapping[token_id]) if self.index_mapping is not None else int(token_id)

    def decode(self, token_id: int):
        o = self.original_id(int(token_id))
        if self._decode is not None:
            return self._decode(o)
        if self._table is not None:
            return self._table[o]
        return o


def neighbors_to_entries(vals, idx, gold_texts: Sequence, counts: Sequence[int], decoder: TokenDecoder) -> List[dict]:
    """Host tensors vals / idx [U, N, K] -> the reference's list: one ``{"gold": ..., "neighbors": {"keyword_i": [[token, score],
    ...]}}`` per utterance u, with ``counts[u]`` keywords (model_utils.py:108-125 / :238-250)."""
    vals_l, idx_l = vals.tolist(), idx.tolist()
    out = []
    for u, gold in enumerate(gold_texts):
        neighbors = defaultdict(list)
        for kw_i in range(int(counts[u])):
            neighbors["keyword_{}".format(kw_i)] = [[decoder.decode(i), v] for i, v in zip(idx_l[u][kw_i], vals_l[u][kw_i])]
        out.append({"gold": gold, "neighbors": neighbors})
    return out


def _device_of(model, *tensors) -> torch.device:
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device(getattr(model, "device", "cuda"))


def _device_neighbors(model, token_table: torch.Tensor) -> Callable:
    """keyword_neighbors on the quantiser's own VocabTables cache when ``token_table`` IS the model's token table (no second set of
    derived tables), else on the module-level cache."""
    vq = getattr(getattr(model, "cascaded_branch", None), "vector_quantizer", None)
    own = getattr(getattr(getattr(model, "clip", None), "model", None), "token_embedding", None)
    tables = getattr(vq, "_tables", None) if own is not None and own.weight.data_ptr() == token_table.data_ptr() else None

    def fn(keywords, table, K, keywords_len, retrieve_method):
        return keyword_neighbors(keywords, table, K, keywords_len, retrieve_method, tables=tables)
    return fn


def extract_fixed_keyword_neighbors(model, K: int, retrieve_method: str, tokenEmbeddings: torch.Tensor,
                                    keywordEmbeddings: torch.Tensor, gold_texts: list, decode: Optional[Callable] = None,
                                    _neighbors: Optional[Callable] = None) -> List[dict]:
    """model_utils.py:41-127: K neighbours of a fixed number of keywords (``model.keyword_num``) per utterance.
    keywordEmbeddings [U, keyword_num, E] (any shape that views to it).  One difference on purpose: the reference labels entry
    ``i + x`` with ``gold_texts[x]`` (the caption of the x-th utterance of the FIRST batch, :122); here it is ``gold_texts[i + x]``
    (docs/parity.md).  ``decode``: original CLIP token id -> what the entry holds (see TokenDecoder)."""
    n = len(gold_texts)
    E = int(model.subword_embd_dim)
    kw = keywordEmbeddings.reshape(-1, int(model.keyword_num), E)[:n]
    assert kw.shape[0] == n, (kw.shape, n)
    fn = _neighbors
    if fn is None:
        dev = _device_of(model, tokenEmbeddings, keywordEmbeddings)
        kw, tokenEmbeddings = kw.to(dev), tokenEmbeddings.to(dev)
        fn = _device_neighbors(model, tokenEmbeddings)
    vals, idx = fn(kw, tokenEmbeddings, K, None, retrieve_method)
    host = torch.cat([vals.double(), idx.double()], dim=-1).cpu()              # one device-to-host copy (ids < 2^53: exact)
    return neighbors_to_entries(host[..., :K].float(), host[..., K:].long(), list(gold_texts), [int(model.keyword_num)] * n,
                                TokenDecoder(getattr(model, "clip", None), decode))


def extract_dynamic_keyword_neighbors(model, K: int, retrieve_method: str, outputs, tokenEmbeddings: torch.Tensor,
                                      keywordEmbeddings_list: List[List[torch.Tensor]], gold_texts: list, kwEmbedLengths: list,
                                      decode: Optional[Callable] = None, _neighbors: Optional[Callable] = None) -> List[dict]:
    """model_utils.py:130-252: K neighbours of a dynamic number of keywords per utterance (the CIF recipes).
    ``keywordEmbeddings_list[b]``: the keyword tensors [bsz, max count, E] of validation batch b (one per device under
    DataParallel); ``gold_texts`` / ``kwEmbedLengths``: one entry per utterance, ``model.config.data.dev_batch_size`` per batch.
    Only the first ``kwEmbedLengths[u]`` slots of an utterance are scored (the reference scores all and reads those)."""
    batch_size = int(model.config.data.dev_batch_size)
    E = int(model.subword_embd_dim)
    rows, golds, counts, row_sel, base = [], [], [], [], 0
    for b_idx, i in zip(range(len(outputs)), range(0, len(gold_texts), batch_size)):
        gold_b, len_b = gold_texts[i: i + batch_size], kwEmbedLengths[i: i + batch_size]
        in_batch = 0
        for emb in keywordEmbeddings_list[b_idx]:
            bsz, max_len = emb.shape[:2]
            rows.append(emb.reshape(bsz * max_len, E))
            for x in range(bsz):
                c = int(len_b[in_batch + x])
                assert c <= max_len, (c, max_len)
                golds.append(gold_b[in_batch + x])
                counts.append(c)
                row_sel.extend(range(base + x * max_len, base + x * max_len + c))
            base += bsz * max_len
            in_batch += bsz
    decoder = TokenDecoder(getattr(model, "clip", None), decode)
    if not row_sel:
        return neighbors_to_entries(torch.zeros(len(golds), 0, K), torch.zeros(len(golds), 0, K), golds, counts, decoder)
    fn = _neighbors
    kw = torch.cat(rows, dim=0)
    if fn is None:
        dev = _device_of(model, tokenEmbeddings, kw)
        kw, tokenEmbeddings = kw.to(dev), tokenEmbeddings.to(dev)
        fn = _device_neighbors(model, tokenEmbeddings)
    kw = kw.index_select(0, torch.tensor(row_sel, dtype=torch.long).to(kw.device))
    vals, idx = fn(kw.unsqueeze(0), tokenEmbeddings, K, None, retrieve_method)
    host = torch.cat([vals.double(), idx.double()], dim=-1).cpu()[0]           # one device-to-host copy
    n_max = max(counts)
    v = torch.full((len(golds), max(n_max, 1), K), float("-inf"))
    ix = torch.full((len(golds), max(n_max, 1), K), -1, dtype=torch.long)
    r = 0
    for u, c in enumerate(counts):
        v[u, :c], ix[u, :c] = host[r: r + c, :K].float(), host[r: r + c, K:].long()
        r += c
    return neighbors_to_entries(v, ix, golds, counts, decoder)


# ------------------------------------------------------------------------------------------------ statistics and hit rate
def keyword_statistics(keywords: torch.Tensor, token_table: torch.Tensor, keywords_len: Optional[torch.Tensor] = None) -> dict:
    """kwClip.py:325-353 on the device: keywords [U, N, E], keywords_len [U] (None: every slot counts) ->
    ``{"mean" | "std" | "norm": {"kw_i": scalar, ..., "kw": scalar over every valid keyword}, "kw_mean_mse", "kw_std_mse"}``.
    mean / std (unbiased, over utterances) / L2 norm per slot i are taken over the utterances that have slot i.  kw_mean_mse /
    kw_std_mse: L2 distance between the keywords' per-channel mean / std and the token table's (what the reference's
    ``torch.norm(a, b, p=2)`` is written to mean: its second positional argument is ``p``; docs/parity.md)."""
    U, N, E = keywords.shape
    kw = keywords.detach().float()
    dev = kw.device
    if keywords_len is None:
        mask = torch.ones(U, N, device=dev, dtype=torch.bool)
    else:
        mask = torch.arange(N, device=dev).unsqueeze(0) < torch.as_tensor(keywords_len, device=dev).long().unsqueeze(1)
    m = mask.unsqueeze(-1).float()
    cnt = m.sum(0)                                               # [N, 1]
    mean_e = (kw * m).sum(0) / cnt
    var_e = (((kw - mean_e) ** 2) * m).sum(0) / (cnt - 1)
    norm = (kw.norm(p=2, dim=-1) * mask.float()).sum(0) / cnt.squeeze(-1)
    stats = {"mean": {}, "std": {}, "norm": {}}
    mean_s, std_s = mean_e.mean(-1), var_e.sqrt().mean(-1)
    for i in range(N):
        stats["mean"][f"kw_{i}"], stats["std"][f"kw_{i}"], stats["norm"][f"kw_{i}"] = mean_s[i], std_s[i], norm[i]
    allk = kw[mask]                                              # [valid keywords, E]
    stats["mean"]["kw"], stats["std"]["kw"] = allk.mean(0).mean(), allk.std(0).mean()
    stats["norm"]["kw"] = allk.norm(p=2, dim=-1).mean()
    tab = token_table.detach().float().to(dev)
    stats["kw_mean_mse"] = torch.norm(allk.mean(0) - tab.mean(0), p=2)
    stats["kw_std_mse"] = torch.norm(allk.std(0) - tab.std(0), p=2)
    return stats


def keyword_hit_rate(idx: torch.Tensor, gold_text: torch.Tensor, reduced_to_original: Optional[torch.Tensor] = None) -> dict:
    """idx [B, N, K] neighbour ids (-1: unscored slot), gold_text [B, L] caption token ids (CLIP's 77-wide tokenisation) ->
    ``{"per_slot": [N], "mean": scalar, "hits": [B, N] bool, "valid": [B, N] bool}``.  A keyword hits if one of its K neighbours'
    ORIGINAL token ids (``reduced_to_original`` [V]: ``clip.selected_text_emb_ids`` when the vocabulary is reduced) occurs among
    the utterance's caption ids; <|startoftext|>, <|endoftext|> and the padding id never count.  Rates are over the scored
    keywords (a slot nobody has: nan).  Integer ops only; stays on torch like the other length and mask arithmetic."""
    B, N, K = idx.shape
    gold = gold_text.reshape(B, -1).to(idx.device).long()
    valid_n = idx >= 0
    orig = idx.clamp(min=0)
    if reduced_to_original is not None:
        orig = reduced_to_original.to(idx.device).long()[orig]
    gold_ok = (gold != PAD_TOKEN) & (gold != SOT_TOKEN) & (gold != EOT_TOKEN)
    match = (orig.reshape(B, N * K, 1) == gold.unsqueeze(1)) & gold_ok.unsqueeze(1)          # [B, N K, L]
    hits = (match.any(-1).view(B, N, K) & valid_n).any(-1)
    valid = valid_n.any(-1)
    per_slot = (hits & valid).sum(0).float() / valid.sum(0).float()
    mean = (hits & valid).sum().float() / valid.sum().float()
    return {"per_slot": per_slot, "mean": mean, "hits": hits, "valid": valid}
