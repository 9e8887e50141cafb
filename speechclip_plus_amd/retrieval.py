"""Recall@k of the validation epoch - same signature and result dictionaries as the reference's ``mutualRetrieval``
(avssl/module/retrieval.py:6-121; scores built at avssl/model/kwClip.py:447-482).

The reference sorts every score row and looks the answers up in rank order.  Here no row is sorted: a query hits at k iff fewer
than k candidates score strictly above its best-scoring correct candidate, so one masked row maximum and one comparison count per
direction give every k at once (on the device the scores live on).

Degenerate scores: the reference leaves exact float ties between a correct and a wrong candidate to the order of an
unstable ``argsort`` - collapsed embeddings (all scores equal) then score about chance - and sorts NaN first.  Here a tie counts
AGAINST the query (a wrong candidate with the same score as the best correct one is ahead of it), a NaN candidate is ahead of
everything (where the reference's sort puts it) and a query whose best correct score is not finite is a miss at every k: a
diverged or collapsed model reports recall near 0, never 100, so a "keep the best validation recall" monitor cannot latch onto it."""
from typing import Dict, Optional, Sequence, Tuple, Union

import torch

__all__ = ["mutualRetrieval", "GalleryIndex", "search", "mutual_ranks", "recall_from_ranks", "mutual_recall", "CompactGalleryIndex",
           "search_compact", "compact_eps", "hard_negatives", "ShardedGalleryIndex", "search_sharded"]


def _recall(score: torch.Tensor, query_ids: torch.Tensor, cand_ids: torch.Tensor, ks: Sequence[int], cand_title: str) -> Dict[str, float]:
    """score [Q, C]; a candidate c is correct for query q iff cand_ids[c] == query_ids[q] (an image with several captions has
    several correct candidates; one of them inside the top k is a hit)."""
    correct = cand_ids.unsqueeze(0) == query_ids.unsqueeze(1)
    nan = torch.isnan(score)
    best = score.masked_fill(~correct | nan, float("-inf")).amax(dim=1, keepdim=True)
    # wrong candidates ahead of the best correct one: higher score, equal score (ties count against the query), or NaN
    ahead = (score > best).sum(dim=1) + (((score == best) | nan) & ~correct).sum(dim=1)
    # a query without a correct candidate, or whose best correct score is not finite (-inf: none / all NaN; +inf: overflow): never a hit
    ok = correct.any(dim=1) & torch.isfinite(best.squeeze(1))
    ahead = torch.where(ok, ahead, torch.full_like(ahead, score.shape[1]))
    out = {}
    for k in ks:
        if k > score.shape[1]:
            print(f"recall@{k} asks for more than the {score.shape[1]} {cand_title} candidates there are; counted over all of them")
        out[f"recall@{k}"] = 100.0 * (ahead < k).float().mean().item()
    return out


def _mean_results(results_AB: dict, results_BA: dict) -> dict:
    """the third dictionary of every result triple: the mean of the two directions, key by key"""
    return {key: 0.5 * (results_AB[key] + results_BA[key]) for key in results_AB}


def mutualRetrieval(score_per_A: torch.Tensor, score_per_B: torch.Tensor, AB_answers: torch.Tensor,
                    BA_answers: torch.Tensor, recall_at: list, modality_A_title: str = "audio",
                    modality_B_title: str = "image") -> Tuple[dict, dict, dict]:
    nA, nB = AB_answers.numel(), BA_answers.numel()
    if AB_answers.dim() != 1 or BA_answers.dim() != 1:
        raise AssertionError("answers must be 1-d id vectors")
    if tuple(score_per_A.shape) != (nA, nB) or tuple(score_per_B.shape) != (nB, nA):
        raise AssertionError(f"score shapes {tuple(score_per_A.shape)} / {tuple(score_per_B.shape)} do not match {nA} x {nB} answers")
    a_ids = AB_answers.to(score_per_A.device)
    b_ids = BA_answers.to(score_per_A.device)
    results_AB = _recall(score_per_A, a_ids, b_ids, recall_at, modality_B_title)
    results_BA = _recall(score_per_B.to(score_per_A.device), b_ids, a_ids, recall_at, modality_A_title)
    return results_AB, results_BA, _mean_results(results_AB, results_BA)


# ------------------------------------------------------------------------------------------------ gallery search
# What the reference does with its ranking: torch.argsort(score, descending=True) of the whole [nQ, N] matrix
# (avssl/module/retrieval.py:45-46, scores from avssl/model/kwClip.py:447-482), read off into recall figures and dropped.  ``search``
# returns the first k entries of every row of that ranking - items and scores - without the matrix: ops.search_topk selects inside
# the score GEMM's epilogue (csrc/search.hip).
_INDEX_CHUNK_ROWS = 16384          # gallery / query rows split per pass (a multiple of 128)


def _up128(x: int) -> int:
    """x rounded up to the kernels' 128-row tile"""
    return -(-x // 128) * 128


def _rows_f32(x: torch.Tensor) -> torch.Tensor:
    """fp32 rows with unit column stride (any row pitch: the split kernel takes one)"""
    x = x.detach().float()
    return x if x.stride(1) == 1 else x.contiguous()


def _split_rows(x: torch.Tensor, side: int, cosine: bool, out: torch.Tensor) -> None:
    """x [R, E] fp32 -> out[: roundup(R, 128)] = its three-way bf16 split (ops.split3_bf16); ``cosine``: rows scaled by
    1 / max(|x|, 1e-8) (ops.vq_prep's rnorm as the split's row_scale)."""
    from . import ops
    rnorm = ops.vq_prep(x)[1] if cosine else None
    ops.split3_bf16(x, side, row_scale=rnorm, out=out[: _up128(x.shape[0])])


def _split_in_chunks(x: torch.Tensor, side: int, cosine: bool) -> torch.Tensor:
    """x [R, E] -> its split [roundup(R, 128), 6 Ep] bf16 (``_split_rows``), made in chunks of ``_INDEX_CHUNK_ROWS`` rows so that no second
    fp32 copy of a large ``x`` exists"""
    R, E = x.shape
    out = torch.empty(_up128(R), 6 * -(-E // 64) * 64, device=x.device, dtype=torch.bfloat16)
    for r0 in range(0, R, _INDEX_CHUNK_ROWS):
        _split_rows(_rows_f32(x[r0: r0 + _INDEX_CHUNK_ROWS]), side, cosine, out[r0:])
    return out


FUSED_MIN_GALLERY = 131072


def default_route(nQ: int, N: int) -> str:
    """"fused" (csrc/search.hip) or "composition" (ops.cosine_scores_split into a 128 MiB score scratch + ops.topk_rows, what
    keyword_neighbors runs) for nQ queries against N gallery rows.  Measured (docs/rounds/r13_search.md): the fused kernel wins where
    whole score rows stop fitting the scratch in useful numbers - a large gallery - and loses below, where the composition's GEMM
    runs on the 256-row tiles and the score matrix stays in the Infinity Cache."""
    return "fused" if N >= FUSED_MIN_GALLERY or N == 0 else "composition"


class _LiveRows:
    """``live`` / ``remove`` / ``restore`` / ``n_live`` of a built index (GalleryIndex, CompactGalleryIndex): the rows' data is never
    touched, ``live`` is None (every row takes part) or a bool [N] device tensor changed in place"""

    def _init_rows(self, gallery: torch.Tensor, cosine: bool, ids: Optional[torch.Tensor]) -> None:
        """the constructors' checks of ``gallery`` [N, E] and ``ids`` [N], under the class's own name -> N, E, Ep, ids, live, cosine"""
        name = type(self).__name__
        if not isinstance(gallery, torch.Tensor) or gallery.dim() != 2:
            raise ValueError(f"{name}: gallery must be a [N, E] tensor")
        if not gallery.is_cuda:
            raise RuntimeError(f"{name} runs on the HIP kernels: device tensors only")
        self.N, self.E = int(gallery.shape[0]), int(gallery.shape[1])
        assert self.E >= 1, gallery.shape
        if ids is not None:
            from . import ops
            ops.filter_operands(name, self.N, self.N, ids, ids, None, gallery.device, names=("ids", "ids", "live"))
        self.ids, self.live = ids, None
        self.cosine = bool(cosine)
        self.Ep = -(-self.E // 64) * 64

    def __len__(self) -> int:
        return self.N

    def _rows_arg(self, rows) -> torch.Tensor:
        """row numbers (a tensor or a sequence of ints) -> int64 on the index's device, every one inside [0, N)"""
        rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= self.N):
            raise IndexError(f"{type(self).__name__}: rows outside [0, {self.N})")
        return rows.to(self.device)

    def _live_changed(self) -> None:
        """``live`` has just been written"""

    def remove(self, rows):
        """Take gallery rows ``rows`` out of every later search (``live[rows] = False``, in place; the rows' data is not touched)."""
        rows = self._rows_arg(rows)
        if self.live is None:
            self.live = torch.ones(self.N, device=self.device, dtype=torch.bool)
        self.live[rows] = False
        self._live_changed()
        return self

    def restore(self, rows=None):
        """Put ``rows`` back (None: every row; ``live`` becomes None again, so a search runs exactly as before any ``remove``)."""
        if rows is None:
            self.live = None
            self._live_changed()
        elif self.live is not None:
            self.live[self._rows_arg(rows)] = True
            self._live_changed()
        else:
            self._rows_arg(rows)                                      # nothing is removed; the rows are still checked
        return self

    @property
    def n_live(self) -> int:
        return self.N if self.live is None else int(self.live.sum())


class GalleryIndex(_LiveRows):
    """A gallery [N, E] prepared for ``search``: the side-1 three-way bf16 split of its rows ([roundup(N, 128), 6 Ep] bf16, Ep = E
    rounded up to 64: 12 Ep bytes per gallery row), built in chunks of rows so that no second fp32 copy of a large gallery is made.
    ``cosine=True``: every row is scaled by 1 / max(|g|, 1e-8) on the way in, so the scores against unit (or ``cosine=True``)
    queries are cosines.  Build once, search with any number of query batches.

    ``ids``: int64 [N] ids of the rows (kept as ``index.ids``, a device tensor, or None): ``search(..., query_ids=...)`` then leaves
    out every row whose id equals the query's.  ``index.live``: None (every row takes part) or a bool [N] device tensor;
    ``remove(rows)`` / ``restore(rows=None)`` change it in place - the split is never touched, so taking rows out of a built index
    (a NaN row, a withdrawn item) costs one small copy, and ``search`` skips them.  ``n_live`` counts the rows that take part."""

    def __init__(self, gallery: torch.Tensor, cosine: bool = False, ids: Optional[torch.Tensor] = None):
        self._init_rows(gallery, cosine, ids)
        self.split = _split_in_chunks(gallery, 1, self.cosine)

    @property
    def device(self) -> torch.device:
        return self.split.device


def _search_filter(queries: torch.Tensor, gallery, query_ids, gallery_ids, live, name: str = "search"):
    """The filter of a ``search`` / ``search_compact`` call, checked before anything is launched (ops.filter_operands): ``gallery_ids`` /
    ``live`` default to an index's own.  -> (query_ids, gallery_ids, live), all None when the call has no filter."""
    from . import ops
    own = isinstance(gallery, (GalleryIndex, CompactGalleryIndex))
    if gallery_ids is None and query_ids is not None and own:
        gallery_ids = gallery.ids
    if live is None and own:
        live = gallery.live
    nQ, N = queries.shape[0], (gallery.N if own else gallery.shape[0])
    return ops.filter_operands(name, nQ, N, query_ids, gallery_ids, live, gallery.device if gallery.device.type == "cuda" else None,
                               names=("query_ids", "gallery_ids", "live"))


def search(queries: torch.Tensor, gallery: Union[torch.Tensor, GalleryIndex, "CompactGalleryIndex"], k: int, cosine: bool = False,
           slabs: Optional[int] = None, route: Optional[str] = None, *, query_ids: Optional[torch.Tensor] = None,
           gallery_ids: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """queries [nQ, E], gallery [N, E] (or a GalleryIndex of it) -> (vals [nQ, k] fp32, idx [nQ, k] int64): for every query the k
    gallery rows with the largest inner product, best first, on the device.  ``cosine=True`` scales query and gallery rows by
    1 / max(|x|, 1e-8) first (a GalleryIndex carries its own choice; the flag then applies to the queries).  1 <= k <= 1024.
    k <= 32 runs the routes below.  32 < k <= 1024 ("wide", csrc/topk_wide.hip): always the composition route's scores, selected by
    ``ops.topk_rows_wide`` under the same order and filter rules; ``default_route`` is not consulted, ``route="fused"`` or ``slabs=`` is a
    ValueError (the fused kernel keeps 32 rows per query), so is a CompactGalleryIndex (its certificate is built on 32 candidates:
    use a GalleryIndex) and a gallery of more than 262 144 rows (128 query rows of scores must fit the 128 MiB scratch).

    Order: larger score first, the lower gallery index first among equal scores, NaN above every number; fewer than k gallery rows:
    -inf / -1 behind them.  ``vals`` are the kernel's fp32 scores: the three-way bf16 splits of both rows multiplied on the bf16
    matrix pipe, six K-blocks summed in fp32.  Accuracy: with Ep = E rounded up to 64, a score differs from the exact inner product
    by at most (6 Ep + 8) 2^-24 sum_i |q_i| |g_i|; the returned order is the order of those fp32 scores, so two gallery rows whose
    exact scores are closer than twice that bound can come back in either order, and a row within twice the bound of the k-th best
    may take its place.  Non-finite inputs: an infinity becomes NaN in the split, so a row with a NaN or an infinity scores NaN
    against every query and ranks first.  ``route``: None = ``default_route`` picks by the gallery size - "fused" (csrc/search.hip:
    the selection runs in the score GEMM's epilogue, the [nQ, N] score matrix is never written, queries go in chunks of 16384
    rows) or "composition" (the same score GEMM into one 128 MiB scratch per chunk of queries + ops.topk_rows; faster on small
    galleries); both give the same lists.  ``slabs``: slabs of the gallery axis of the fused kernel (tests; implies "fused"; the
    result does not depend on it).  A CompactGalleryIndex as ``gallery``: ``search_compact(queries, gallery, k)[:2]`` - the same lists
    from the bf16 copy, with re-rank scores as ``vals`` (see there).

    Filter (csrc/search_filter.hip): gallery row j is ADMISSIBLE for query i iff j < N, ``live`` is absent or live[j] != 0, and ids
    are absent or gallery_ids[j] != query_ids[i].  ``query_ids`` [nQ] / ``gallery_ids`` [N]: int64, contiguous, on the device, all
    64 bits compared, negative values legal, both or neither; ``live`` [N]: bool (or uint8).  ``gallery_ids`` / ``live`` default to
    the GalleryIndex's own ``ids`` / ``live``.  The result is the order above over the admissible rows only: an inadmissible row never
    appears whatever its score (NaN included), -inf / -1 stand behind the last admissible row, an admissible row has the same fp32
    bits as without the filter, and one whose score is a real -inf ranks ahead of the fillers.  Both routes run with a filter and
    ``default_route`` picks as before.  Without ids and without a live mask the call runs exactly the unfiltered code.  A
    CompactGalleryIndex with any filter ARGUMENT is a ValueError: the filtered compact call returns its certificate, so it is
    ``search_compact``'s; without filter arguments the index's own removed rows are honoured."""
    k = int(k)
    wide = k > 32                                     # the wide selection: the composition route's scores, ops.topk_rows_wide
    if k > WIDE_MAX_K:
        raise ValueError(f"search: 1 <= k <= {WIDE_MAX_K} (k {k})")
    if isinstance(gallery, CompactGalleryIndex):      # the compact route (below): exact lists through the certificate and its fallback
        if wide:
            raise ValueError(f"search: k = {k} on a CompactGalleryIndex - its certificate is built on at most 32 candidates per query "
                             "(k <= depth <= 32); build a GalleryIndex of the gallery for 32 < k <= 1024")
        if query_ids is not None or gallery_ids is not None or live is not None:
            raise ValueError("search: a CompactGalleryIndex takes no filter arguments here - the filtered call returns its certificate "
                             "(restated over the admissible rows), so it is search_compact(queries, index, k, query_ids=..., "
                             "gallery_ids=..., live=...); search(queries, index, k) honours the index's own removed rows")
        if route is not None:
            raise ValueError("search: route applies to a GalleryIndex or a tensor, not to a CompactGalleryIndex")
        return search_compact(queries, gallery, k, cosine=cosine, slabs=slabs)[:2]
    if wide and (route == "fused" or slabs is not None):
        raise ValueError(f"search: k = {k} with route=\"fused\" / slabs= - the fused kernel keeps at most 32 gallery rows per query; "
                         "32 < k <= 1024 runs the composition route (route=None or \"composition\")")
    if wide and route not in (None, "composition"):
        raise ValueError(f"search: route = {route!r} (\"fused\" or \"composition\")")
    if not isinstance(queries, torch.Tensor) or queries.dim() != 2:
        raise ValueError("search: queries must be a [nQ, E] tensor")
    own = isinstance(gallery, GalleryIndex)
    filtered = query_ids is not None or gallery_ids is not None or live is not None or (own and gallery.live is not None)
    if (wide or filtered) and not own and not (isinstance(gallery, torch.Tensor) and gallery.dim() == 2):
        raise ValueError("search: gallery must be a [N, E] tensor or a GalleryIndex")
    if filtered:                                      # format errors come before device errors
        query_ids, gallery_ids, live = _search_filter(queries, gallery, query_ids, gallery_ids, live)
    g_cuda = gallery.split.is_cuda if own else (isinstance(gallery, torch.Tensor) and gallery.is_cuda)
    if not queries.is_cuda or not g_cuda:
        raise RuntimeError("search runs on the HIP kernels: device tensors only")
    N = gallery.N if own else int(gallery.shape[0])
    if wide and N > wide_max_gallery():
        raise ValueError(f"search: k = {k} against {N} gallery rows - 128 query rows of scores no longer fit the score scratch; "
                         f"32 < k <= {WIDE_MAX_K} serves at most N = {wide_max_gallery()} gallery rows (k <= 32 has no such limit)")
    index = gallery if own else GalleryIndex(gallery, cosine=cosine)
    assert queries.shape[1] == index.E, (queries.shape, index.E)
    if not 1 <= k <= WIDE_MAX_K:
        raise ValueError(f"search: 1 <= k <= {WIDE_MAX_K} (k {k})")
    if wide:                                          # ``default_route`` is not consulted
        route = "composition"
    elif route is None:
        route = "fused" if slabs is not None else default_route(queries.shape[0], index.N)
    if route not in ("fused", "composition"):
        raise ValueError(f"search: route = {route!r} (\"fused\" or \"composition\")")
    return _search_chunks(queries, index, k, cosine, slabs, route, query_ids, gallery_ids, live)


WIDE_MAX_K = 1024                  # csrc/topk_wide.hip sorts the list in 8 KiB of LDS


def wide_max_gallery() -> int:
    """The largest gallery ``search`` serves at k > 32: 128 query rows (one row tile of the score GEMM) of fp32 scores, the gallery axis
    rounded up to 128, must fit the 128 MiB score scratch of the composition route -> 262 144 rows."""
    from .keyword_neighbors import SCORE_SCRATCH_BYTES
    return SCORE_SCRATCH_BYTES // (4 * 128) // 128 * 128


def _search_chunks(queries: torch.Tensor, index: GalleryIndex, k: int, cosine: bool, slabs: Optional[int], route: str,
                   query_ids: Optional[torch.Tensor], gallery_ids: Optional[torch.Tensor], live: Optional[torch.Tensor]):
    """``search`` on checked operands: the queries in chunks of rows through one query-split buffer and, on the composition route, one
    score scratch.  The selection is the fused kernel's (ops.search_topk, with a filter ops.search_topk_filtered) or, on the scores
    of ops.cosine_scores_split, ops.topk_rows / ops.topk_rows_filtered / (k > 32) ops.topk_rows_wide."""
    from . import ops
    nQ, N, dev = queries.shape[0], index.N, queries.device
    wide, filtered = k > 32, query_ids is not None or live is not None
    vals = torch.empty(nQ, k, device=dev, dtype=torch.float32)
    idx = torch.empty(nQ, k, device=dev, dtype=torch.int32)
    if wide and nQ > 0 and N == 0:                                        # no gallery row: fillers only (nothing to score)
        vals.fill_(float("-inf"))
        idx.fill_(-1)
    elif nQ > 0:
        q = _rows_f32(queries)
        if route == "composition" and N > 0:
            from .keyword_neighbors import default_chunk_rows
            chunk = min(default_chunk_rows(N), _up128(nQ))
            scores = torch.empty(chunk, index.split.shape[0], device=dev, dtype=torch.float32)   # the one score scratch of the call
        else:
            chunk = min(_INDEX_CHUNK_ROWS, _up128(nQ))
            scores = None
        split = torch.empty(chunk, 6 * index.Ep, device=dev, dtype=torch.bfloat16)       # the one query-split buffer of the call
        for r0 in range(0, nQ, chunk):
            r1 = min(nQ, r0 + chunk)
            out = {"vals": vals[r0:r1], "idx": idx[r0:r1]}
            if filtered or wide:
                out.update(q_ids=None if query_ids is None else query_ids[r0:r1], g_ids=gallery_ids, live=live)
            if scores is None:
                _split_rows(q[r0:r1], 0, cosine, split)
                select = ops.search_topk_filtered if filtered else ops.search_topk
                select(split, index.split, r1 - r0, N, k, slabs=slabs, **out)
            else:
                rp = _up128(r1 - r0)
                rnorm = ops.vq_prep(q[r0:r1])[1] if cosine else None
                ops.cosine_scores_split(q[r0:r1], rnorm, index.split, index.split.shape[0], out=scores[:rp], split_out=split[:rp])
                select = ops.topk_rows_wide if wide else ops.topk_rows_filtered if filtered else ops.topk_rows
                select(scores[: r1 - r0], N, k, **out)
    return vals, idx.long()


def hard_negatives(A: torch.Tensor, B: Union[torch.Tensor, GalleryIndex, "CompactGalleryIndex"], a_ids: torch.Tensor,
                   b_ids: Optional[torch.Tensor], k: int, cosine: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Hard-negative mining: for every anchor A[i] the k highest-scoring rows of B that are WRONG for it - rows j with
    b_ids[j] != a_ids[i] - as (vals [nA, k] fp32, idx [nA, k] int64), hardest first.  ``a_ids`` [nA] / ``b_ids`` [nB]: int64 device
    tensors (the ids ``mutual_ranks`` takes to decide what is correct); ``b_ids`` None: the ids of the GalleryIndex ``B``.  This is
    ``search(A, B, k, cosine, query_ids=a_ids, gallery_ids=b_ids)``: scores, order, ties and tails are ``search``'s, an anchor with
    fewer than k wrong rows ends in -inf / -1, and a removed row of an index (``live``) is never mined.  ``B`` a CompactGalleryIndex:
    the same lists through ``search_compact(..., query_ids=a_ids, gallery_ids=b_ids)`` and its exact fallback (vals are the re-rank's).
    1 <= k <= 1024 on a tensor or a GalleryIndex (k > 32: ``search``'s wide selection, at most 262 144 rows in ``B``); k <= 32 on a
    CompactGalleryIndex.  ``B`` a ShardedGalleryIndex built with ``ids=`` (``b_ids`` None): ``search_sharded(A, B, k, cosine,
    query_ids=a_ids)`` - the same lists with global rows, any number of rows in ``B``, collective when the index is distributed."""
    if isinstance(B, ShardedGalleryIndex):                            # the shards bring their ids: search_sharded, the same lists
        if a_ids is None or b_ids is not None or B.ids is None:
            raise ValueError("hard_negatives: a ShardedGalleryIndex takes a_ids and its own ids (build it with ids=, pass b_ids=None)")
        return search_sharded(A, B, k, cosine=cosine, query_ids=a_ids)
    if a_ids is None:
        raise ValueError("hard_negatives: a_ids is required (without ids every row is a negative: that is search)")
    if b_ids is None and not (isinstance(B, (GalleryIndex, CompactGalleryIndex)) and B.ids is not None):
        raise ValueError("hard_negatives: b_ids is required unless B is a GalleryIndex or a CompactGalleryIndex built with ids=")
    if isinstance(B, CompactGalleryIndex):
        return search_compact(A, B, k, cosine=cosine, query_ids=a_ids, gallery_ids=b_ids)[:2]
    return search(A, B, k, cosine=cosine, query_ids=a_ids, gallery_ids=b_ids)


# ------------------------------------------------------------------------------------------------ sharded gallery search
# ``search`` serves one GalleryIndex on one device, and at k > 32 at most ``wide_max_gallery()`` rows of it.  A ShardedGalleryIndex is
# consecutive row ranges of one logical gallery, each a GalleryIndex - cut from one tensor on this device, or one range per rank of a
# process group.  ``search_sharded`` runs ``search`` per shard and merges the k-entry lists exactly (csrc/search_merge_wide.hip): a score
# depends only on its query row, its gallery row and the fixed K order, so the result equals ``search`` on the whole gallery bit for bit.
SHARD_LISTS_BYTES = 256 << 20      # the partial lists of one chunk of queries, S * chunk * k * 8 bytes, stay under this


def _exchange_counts(mine: Sequence[int], dev, group) -> list:
    """a few ints of every rank -> [W][len(mine)] on every rank (one all_gather_into_tensor)"""
    import torch.distributed as dist
    W = dist.get_world_size(group)
    m = torch.tensor(list(mine), device=dev, dtype=torch.int64)
    every = torch.empty(W * m.numel(), device=dev, dtype=torch.int64)
    dist.all_gather_into_tensor(every, m, group=group)
    return every.view(W, m.numel()).tolist()


class ShardedGalleryIndex(_LiveRows):
    """Consecutive row ranges of one gallery [N, E], each a GalleryIndex, for ``search_sharded``.

    Local form, ``ShardedGalleryIndex(gallery, shard_rows=None, cosine=False, ids=None)``: ``gallery`` [N, E] on the device is cut into
    shards of ``shard_rows`` rows (None: ``wide_max_gallery()``, the most ``search`` serves at k > 32; any positive int is legal, the
    last shard may be short).  Every shard is built as a GalleryIndex is - in chunks of rows, no second fp32 copy of the gallery.
    The default is the FEWEST shards, not the fastest call at k > 32: ``search`` scores as many query rows at a time as its 128 MiB
    scratch holds of a shard's rows, 128 at 262 144; ``shard_rows=65536`` ran 1 024 x 1 000 000 x 512 at k = 100 in 8.3 ms against 21.2 ms
    (docs/rounds/r21_sharded_search.md).

    Distributed form, ``ShardedGalleryIndex(rows, cosine=False, ids=None, group=pg)``: COLLECTIVE over the process group ``pg``
    (torch.distributed).  ``rows`` [n_rank, E] are this rank's rows of the gallery (0 rows are legal), ``ids`` this rank's ids; the global
    gallery is the ranks' rows in rank order, so this rank's ``row0`` is the sum of the lower ranks' counts (exchanged once, here).  E
    must be equal on every rank (a ValueError on every rank otherwise).

    ``N`` (``len(index)``): the global row count.  ``E``, ``cosine``, ``shards`` (the GalleryIndex objects on this device), ``row0`` (the
    global row of each of them), ``n_live`` (live rows of the whole gallery; in the distributed form reading it is collective).
    ``remove(rows)`` / ``restore(rows=None)`` take GLOBAL rows, as on a GalleryIndex (IndexError outside [0, N)); in the distributed
    form every rank passes the same rows and applies those in its range.  ``ids``: the constructor's argument (None: the index takes no
    ``query_ids``); the shards hold their slices of it and their own ``live`` masks."""

    def __init__(self, gallery: torch.Tensor, shard_rows: Optional[int] = None, cosine: bool = False, ids: Optional[torch.Tensor] = None,
                 group=None):
        if isinstance(gallery, (CompactGalleryIndex, GalleryIndex)) or (
                isinstance(gallery, (list, tuple)) and any(isinstance(s, CompactGalleryIndex) for s in gallery)):
            raise ValueError("ShardedGalleryIndex: built from the gallery's rows, every shard a GalleryIndex - a CompactGalleryIndex cannot "
                             "be a shard (its lists are certified on 32 candidates, its values are re-rank scores)")
        self._init_rows(gallery, cosine, ids)
        self.group = group
        n = self.N
        if group is None:
            shard_rows = wide_max_gallery() if shard_rows is None else int(shard_rows)
            if shard_rows < 1:
                raise ValueError(f"ShardedGalleryIndex: shard_rows must be a positive int (shard_rows {shard_rows})")
            self.row0 = list(range(0, max(n, 1), shard_rows))
            self.shards = [GalleryIndex(gallery[r0: r0 + shard_rows], cosine=cosine, ids=None if ids is None else ids[r0: r0 + shard_rows])
                           for r0 in self.row0]
            starts = self.row0
        else:
            import torch.distributed as dist
            if shard_rows is not None:
                raise ValueError("ShardedGalleryIndex: shard_rows applies to the local form; with group= every rank's rows are one shard")
            W, rank = dist.get_world_size(group), dist.get_rank(group)
            counts, Es, has = (list(col) for col in zip(*_exchange_counts([n, self.E, int(ids is not None)], gallery.device, group)))
            if len(set(Es)) != 1:
                raise ValueError(f"ShardedGalleryIndex: E differs between the ranks ({Es})")
            if len(set(has)) != 1:
                raise ValueError(f"ShardedGalleryIndex: ids on some ranks only ({has})")
            starts = [sum(counts[:r]) for r in range(W)]
            self.N = sum(counts)
            self.row0 = [starts[rank]]
            self.shards = [GalleryIndex(gallery, cosine=cosine, ids=ids)]
        if self.N >= 2 ** 31 - 1:
            raise ValueError(f"ShardedGalleryIndex: {self.N} rows - a global row must be below 2^31 - 1")
        self._starts = torch.tensor(starts, device=gallery.device, dtype=torch.int64)     # row0 of every list the merge sees

    @property
    def device(self) -> torch.device:
        return self.shards[0].device

    def _per_shard(self, rows: torch.Tensor):
        """global rows (checked, on the device) -> (shard, its own rows of them) for every shard on this device that has any"""
        for r0, shard in zip(self.row0, self.shards):
            own = rows[(rows >= r0) & (rows < r0 + shard.N)] - r0
            if own.numel():
                yield shard, own

    def remove(self, rows):
        """Take the GLOBAL gallery rows ``rows`` out of every later search (the shards' ``live`` masks; the rows' data is not touched)."""
        for shard, own in self._per_shard(self._rows_arg(rows)):
            shard.remove(own)
        return self

    def restore(self, rows=None):
        """Put the GLOBAL rows ``rows`` back (None: every row, and every shard searches exactly as before any ``remove``)."""
        if rows is None:
            for shard in self.shards:
                shard.restore()
        else:
            for shard, own in self._per_shard(self._rows_arg(rows)):
                shard.restore(own)
        return self

    @property
    def n_live(self) -> int:
        n = sum(shard.n_live for shard in self.shards)
        if self.group is not None:
            import torch.distributed as dist
            total = torch.tensor([n], device=self.device, dtype=torch.int64)
            dist.all_reduce(total, group=self.group)
            n = int(total)
        return n


def _gather_rows(x: torch.Tensor, counts: Sequence[int], group) -> torch.Tensor:
    """x [counts[rank], ...] on every rank -> the ranks' rows in rank order [sum(counts), ...] on every rank: one all_gather_into_tensor
    of blocks padded to the largest count (the collective wants equal sizes), the padding cut away"""
    import torch.distributed as dist
    W, top = len(counts), max(counts)
    block = torch.zeros((top,) + tuple(x.shape[1:]), device=x.device, dtype=x.dtype)
    block[: x.shape[0]] = x
    every = torch.empty((W * top,) + tuple(x.shape[1:]), device=x.device, dtype=x.dtype)      # rank-major along dim 0: the collective's layout
    dist.all_gather_into_tensor(every, block, group=group)
    every = every.view((W, top) + tuple(x.shape[1:]))
    return torch.cat([every[r, : counts[r]] for r in range(W)], dim=0)


def search_sharded(queries: torch.Tensor, index: ShardedGalleryIndex, k: int, cosine: bool = False, *,
                   query_ids: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """queries [nQ, E], a ShardedGalleryIndex -> (vals [nQ, k] fp32, idx [nQ, k] int64 GLOBAL gallery rows), 1 <= k <= 1024: what
    ``search(queries, GalleryIndex(whole gallery), k, cosine, query_ids=...)`` returns - the same rows in the same places, the same 32
    bits in every value - for every partition into shards, also where ``search`` itself stops (k > 32 on more than 262 144 rows; a
    gallery spread over the ranks of a process group).  ``cosine`` applies to the queries (the index carries its own choice).
    ``query_ids`` [nQ] int64: a gallery row whose id equals the query's is left out (the index must have been built with ``ids=``); the
    shards' removed rows are never returned.

    Per chunk of queries: ``search`` on every shard - so scores, filter, order and tails are ``search``'s, with its scratch, one shard at
    a time -, the lists stacked [S, chunk, k], one ``ops.search_merge_lists``.  The chunk keeps the stacked lists, S * chunk * k * 8
    bytes, under ``SHARD_LISTS_BYTES`` (256 MiB).

    Distributed index: the call is COLLECTIVE.  Every rank passes its OWN queries (the counts may differ, 0 is legal), the same k, and
    ids on every rank or on none.  The counts are exchanged, queries and ids all-gathered, every rank searches its shard for all of
    them, the partial lists are all-gathered ([W, nQall, k], rank-major: the merge's layout) and every rank merges the slice of its own
    queries.  The chunk loop's trip count comes from the global query count, so every rank runs the same collectives."""
    from . import ops
    k = int(k)
    if not 1 <= k <= WIDE_MAX_K:
        raise ValueError(f"search_sharded: 1 <= k <= {WIDE_MAX_K} (k {k})")
    if not isinstance(index, ShardedGalleryIndex):
        raise ValueError("search_sharded: index must be a ShardedGalleryIndex (a tensor or a GalleryIndex goes to search)")
    if not isinstance(queries, torch.Tensor) or queries.dim() != 2:
        raise ValueError("search_sharded: queries must be a [nQ, E] tensor")
    nQ = queries.shape[0]
    if query_ids is not None:
        if index.ids is None:
            raise ValueError("search_sharded: query_ids on a ShardedGalleryIndex built without ids=")
        ops.check_filter_tensor("search_sharded", "query_ids", query_ids, nQ)
    if not queries.is_cuda or (query_ids is not None and not query_ids.is_cuda):
        raise RuntimeError("search_sharded runs on the HIP kernels: device tensors only")
    assert queries.shape[1] == index.E, (queries.shape, index.E)
    if k > 32 and any(shard.N > wide_max_gallery() for shard in index.shards):
        raise ValueError(f"search_sharded: k = {k} on shards of more than {wide_max_gallery()} rows - search serves 32 < k <= {WIDE_MAX_K} "
                         f"on at most that many; build the index with shard_rows <= {wide_max_gallery()}")
    dev = queries.device
    own0, own1 = 0, nQ                                                # this rank's queries among all of them
    if index.group is not None:
        import torch.distributed as dist
        counts, has = (list(col) for col in zip(*_exchange_counts([nQ, int(query_ids is not None)], dev, index.group)))
        if len(set(has)) != 1:
            raise ValueError(f"search_sharded: query_ids on some ranks only ({has})")
        own0 = sum(counts[: dist.get_rank(index.group)])
        own1 = own0 + nQ
        queries = _gather_rows(_rows_f32(queries), counts, index.group)
        if query_ids is not None:
            query_ids = _gather_rows(query_ids, counts, index.group)
    nAll, S = queries.shape[0], int(index._starts.numel())
    vals = torch.empty(nQ, k, device=dev, dtype=torch.float32)
    idx = torch.empty(nQ, k, device=dev, dtype=torch.int32)
    if nAll == 0:
        return vals, idx.long()
    chunk = min(max(SHARD_LISTS_BYTES // (S * k * 8), 1), nAll)
    pv = torch.empty(S * chunk * k, device=dev, dtype=torch.float32)  # the stacked lists of the call
    pi = torch.empty(S * chunk * k, device=dev, dtype=torch.int32)
    for c0 in range(0, nAll, chunk):
        c1 = min(nAll, c0 + chunk)
        n = c1 - c0
        lv, li = pv[: S * n * k].view(S, n, k), pi[: S * n * k].view(S, n, k)
        qc, ic = queries[c0:c1], None if query_ids is None else query_ids[c0:c1]
        if index.group is None:
            for s, shard in enumerate(index.shards):
                v, i = search(qc, shard, k, cosine=cosine, query_ids=ic)
                lv[s].copy_(v)
                li[s].copy_(i)
        else:
            v, i = search(qc, index.shards[0], k, cosine=cosine, query_ids=ic)
            dist.all_gather_into_tensor(lv.view(S * n, k), v.contiguous(), group=index.group)      # [W n, k]: rank-major, the merge's layout
            dist.all_gather_into_tensor(li.view(S * n, k), i.int().contiguous(), group=index.group)
        a, b = max(c0, own0), min(c1, own1)
        if a < b:
            ops.search_merge_lists(lv[:, a - c0: b - c0], li[:, a - c0: b - c0], index._starts, k, vals=vals[a - own0: b - own0],
                                   idx=idx[a - own0: b - own0])
    return vals, idx.long()


# ------------------------------------------------------------------------------------------------ compact gallery search
# A GalleryIndex costs 12 Ep bytes per gallery row and six K-blocks per score.  The compact index keeps ONE bf16 copy (2 Ep bytes per
# row) for a coarse top-D scan (csrc/search_compact.hip), re-ranks the D candidates exactly from the fp32 rows and certifies, per
# query, that no row outside the candidates can belong to the answer; a query without the certificate goes through ``search``.
_FALLBACK_CHUNK_ROWS = 131072      # gallery rows per temporary GalleryIndex of the exact fallback


def compact_eps(q_norms: torch.Tensor, gmax: float, gtmax: float, dmax: float, Ep: int) -> torch.Tensor:
    """The bound on |exact - coarse| of a query against ANY gallery row, in fp64: ``q_norms`` [3, nQ] = (|q'|, |q~|, |q' - q~|) as
    ``ops.rows_bf16`` reports them (q' the scaled fp32 row, q~ its bf16 image), ``gmax`` / ``gtmax`` / ``dmax`` the largest |g'|, |g~|
    and |g' - g~| over the gallery, ``Ep`` the padded row length.  With exact - coarse_true = sum (q' - q~) g' + sum q~ (g' - g~),
    Cauchy-Schwarz on both sums and the fp32 accumulation of Ep products in the project's usual form:

        eps = (|q' - q~| gmax + |q~| dmax + (Ep + 8) 2^-24 |q~| gtmax) (1 + 2^-20)

    (the last factor covers the fp32 roundings of the norms and of eps itself).  -> [nQ] fp64 on ``q_norms``' device."""
    n = q_norms.double()
    return (n[2] * float(gmax) + n[1] * float(dmax) + (Ep + 8) * 2.0 ** -24 * n[1] * float(gtmax)) * (1.0 + 2.0 ** -20)


class CompactGalleryIndex(_LiveRows):
    """A gallery [N, E] prepared for ``search_compact``: ``coarse`` = its rows rounded to bf16 ([roundup(N, 128), Ep] bf16, Ep = E
    rounded up to 64: 2 Ep bytes per gallery row, a sixth of a GalleryIndex), built in chunks of rows; ``rows`` = the fp32 gallery the
    exact re-rank reads - kept BY REFERENCE when it is already fp32 on the device with unit column stride (the caller must not modify
    it afterwards), one fp32 copy otherwise; ``rnorm`` [N] = 1 / max(|g|, 1e-8) for ``cosine=True`` (the scores against unit or
    ``cosine=True`` queries are then cosines), else None; ``gmax`` / ``gtmax`` / ``dmax`` = the largest norm of a scaled row, of its
    bf16 image and of their difference (``compact_eps``); ``nbytes`` = what the index itself allocated.

    ``ids`` / ``live`` / ``remove(rows)`` / ``restore(rows=None)`` / ``n_live``: as on a GalleryIndex (the same checks and errors).
    ``search_compact`` skips a removed row, and ``gmax`` / ``gtmax`` / ``dmax`` are taken over the LIVE rows only - removing a NaN or
    huge row makes ``compact_eps`` finite and small again, so the index certifies as if the row had never been there.  For that the
    per-row norms ``ops.rows_bf16`` reports are kept as ``norms`` [3, N] fp32 from the first time a row is dead (the first ``remove``
    or the first ``search_compact(..., live=)``: one more pass over the fp32 rows, 12 N bytes added to ``nbytes``); an index that
    never had a dead row holds nothing more than before.  ``restore()`` brings the three bounds of the whole gallery back bit for bit."""

    def __init__(self, gallery: torch.Tensor, cosine: bool = False, ids: Optional[torch.Tensor] = None):
        from . import ops
        self._init_rows(gallery, cosine, ids)
        self.norms = None
        self.rows = _rows_f32(gallery)
        held = self.rows.data_ptr() == gallery.data_ptr() and gallery.dtype == torch.float32
        self.coarse = torch.empty(_up128(self.N), self.Ep, device=gallery.device, dtype=torch.bfloat16)
        self.rnorm = torch.empty(self.N, device=gallery.device, dtype=torch.float32) if self.cosine else None
        top = torch.zeros(3, device=gallery.device, dtype=torch.float32)
        for r0 in range(0, self.N, _INDEX_CHUNK_ROWS):
            r1 = min(self.N, r0 + _INDEX_CHUNK_ROWS)
            x = self.rows[r0:r1]
            scale = None
            if self.cosine:
                self.rnorm[r0:r1] = ops.vq_prep(x)[1]
                scale = self.rnorm[r0:r1]
            _, norms = ops.rows_bf16(x, scale, out=self.coarse[r0: r0 + _up128(r1 - r0)])
            top = torch.maximum(top, norms.amax(dim=1))               # amax / maximum carry a NaN on
        self._top_all = tuple(float(v) for v in top.tolist())         # the bounds over the whole gallery: what restore() brings back
        self.gmax, self.gtmax, self.dmax = self._top_all
        self.nbytes = self.coarse.numel() * 2 + (self.rnorm.numel() * 4 if self.cosine else 0) + (0 if held else self.rows.numel() * 4)

    @property
    def device(self) -> torch.device:
        return self.coarse.device

    def _row_norms(self) -> torch.Tensor:
        """``norms`` [3, N] fp32, computed on first use: ``ops.rows_bf16`` over the fp32 rows again, in the constructor's chunks and
        with its scales (the same bits the constructor's maxima were taken from), the bf16 images going to a scratch buffer"""
        if self.norms is None:
            from . import ops
            norms = torch.empty(3, self.N, device=self.device, dtype=torch.float32)
            scratch = torch.empty(min(_up128(self.N), _INDEX_CHUNK_ROWS), self.Ep, device=self.device, dtype=torch.bfloat16)
            for r0 in range(0, self.N, _INDEX_CHUNK_ROWS):
                r1 = min(self.N, r0 + _INDEX_CHUNK_ROWS)
                scale = self.rnorm[r0:r1] if self.cosine else None
                norms[:, r0:r1] = ops.rows_bf16(self.rows[r0:r1], scale, out=scratch[: _up128(r1 - r0)])[1]
            self.norms = norms
            self.nbytes += norms.numel() * 4
        return self.norms

    def _bounds(self, live: Optional[torch.Tensor]) -> Tuple[float, float, float]:
        """(gmax, gtmax, dmax) over the rows with live[j] != 0 (None: every row; no such row: zeros).  A dead row's norms do not
        enter, whatever they are; a live NaN row still makes its bound NaN.  The host reads three floats."""
        if live is None:
            return self._top_all
        if self.N == 0:
            return (0.0, 0.0, 0.0)
        norms = self._row_norms()
        top = torch.where((live != 0).unsqueeze(0), norms, torch.zeros((), device=norms.device, dtype=norms.dtype)).amax(dim=1)
        return tuple(float(v) for v in top.tolist())

    def _live_changed(self) -> None:
        self.gmax, self.gtmax, self.dmax = self._bounds(self.live)


def _exact_fallback(q: torch.Tensor, index: CompactGalleryIndex, k: int, cosine: bool, query_ids: Optional[torch.Tensor] = None,
                    gallery_ids: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None):
    """q [nU, E] fp32 -> (vals [nU, k] fp32, idx [nU, k] int32) by ``search`` against the fp32 rows, the gallery in chunks of
    ``_FALLBACK_CHUNK_ROWS`` rows (a temporary GalleryIndex each; ``gallery_ids`` / ``live`` sliced per chunk, ``query_ids`` [nU] the
    uncertified queries' own), the per-chunk lists merged in index order and the k survivors re-scored by ``ops.search_rerank``.
    Without a filter only the last chunk can end in fillers, so position order keeps the tie rule.  With a filter ANY chunk can, so
    the fillers are moved behind every entry first (a stable sort on one bit: the entries keep their chunk order, which is index
    order); ``ops.topk_rows`` then breaks a tie by position - equal scores keep the lower gallery row first, and a real -inf, an
    entry, stands ahead of every filler."""
    from . import ops
    nU, dev = q.shape[0], q.device
    pv, pi = [], []
    for c0 in range(0, max(index.N, 1), _FALLBACK_CHUNK_ROWS):
        c1 = min(index.N, c0 + _FALLBACK_CHUNK_ROWS)
        v, i = search(q, GalleryIndex(index.rows[c0:c1], cosine=index.cosine), k, cosine=cosine, query_ids=query_ids,
                      gallery_ids=None if gallery_ids is None else gallery_ids[c0:c1], live=None if live is None else live[c0:c1])
        pv.append(v)
        pi.append(torch.where(i >= 0, i + c0, i))
    if len(pv) == 1:
        cv, ci = pv[0], pi[0].int()
    else:
        allv, alli = torch.cat(pv, dim=1), torch.cat(pi, dim=1)
        if query_ids is not None or live is not None:
            _, order = torch.sort((alli < 0).to(torch.int8), dim=1, stable=True)
            allv, alli = torch.gather(allv, 1, order), torch.gather(alli, 1, order)
        cv, pos = ops.topk_rows(allv, allv.shape[1], k)
        ci = torch.gather(alli, 1, pos.long()).int()
    q_scale = ops.vq_prep(q)[1] if cosine else None
    vals, idx, _ = ops.search_rerank(q, q_scale, index.rows, index.rnorm, ci.contiguous(), cv.contiguous(),
                                     torch.zeros(nU, device=dev, dtype=torch.float32), k)
    return vals, idx


def search_compact(queries: torch.Tensor, gallery: Union[torch.Tensor, CompactGalleryIndex], k: int, cosine: bool = False, depth: int = 32,
                   fallback: str = "exact", slabs: Optional[int] = None, *, query_ids: Optional[torch.Tensor] = None,
                   gallery_ids: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """queries [nQ, E], gallery [N, E] (or a CompactGalleryIndex of it) -> (vals [nQ, k] fp32, idx [nQ, k] int64, certified [nQ] bool):
    ``search``'s lists from a bf16 copy of the gallery.  1 <= k <= depth <= 32.  Per query: the ``depth`` best rows by the bf16 x bf16
    score (one K-block instead of six), re-ranked by their inner products accumulated in fp64 from the fp32 rows, and the certificate
    ``certified``: the k-th exact value lies above the last candidate's coarse value by more than ``compact_eps``, so no row outside
    the candidates can belong to the list, not even by a tie.  Order and tails are ``search``'s (larger first, lower gallery row among
    equals, NaN on top, -inf / -1 behind the N-th entry).  ``vals`` are the re-rank scores - the fp64 sum rounded once, closer to the
    exact inner product than ``search``'s fp32 scores - so where ``search`` orders two rows by rounding noise the lists may differ.
    ``cosine=True`` scales query and gallery rows by 1 / max(|x|, 1e-8) (an index carries its own choice; the flag then applies to the
    queries).  Queries go in chunks of 16384 rows through one reused bf16 buffer.

    ``fallback="exact"`` (default): the mask is read on the host - the one synchronisation of the call - and every uncertified query
    is searched again by ``search`` against the fp32 rows, in gallery chunks of 131072 rows, and re-scored the same way; their
    ``certified`` stays False.  This costs a PASS OVER THE WHOLE GALLERY (a three-way split of every chunk included) whenever any row
    is uncertified.  ``fallback="none"``: no synchronisation; an uncertified row holds the best k of its candidates.  ``slabs``:
    at most so many slabs of the coarse kernel's gallery axis (tests; empty slabs are dropped, the result does not depend on it).

    Filter (csrc/search_compact_filter.hip): gallery row j is ADMISSIBLE for query i iff j < N, ``live`` is absent or live[j] != 0, and
    ids are absent or gallery_ids[j] != query_ids[i] - ``search``'s rule and operands (int64 ids, both or neither, all 64 bits
    compared; ``live`` bool or uint8; checked before anything is launched).  ``gallery_ids`` defaults to the index's ``ids``; the
    effective mask is the index's ``live`` AND the argument.  The result is the contract above over the admissible rows only: an
    inadmissible row never appears, whatever its score (NaN and inf included), and it spoils nothing.  The certificate is restated
    over them: the candidates are the ``depth`` best ADMISSIBLE rows by coarse score; a query with fewer than ``depth`` candidates has
    every admissible row among them and is certified (its tail is -inf / -1; with no admissible row the empty list is the exact
    answer), every other one by the inequality above, and ``compact_eps`` takes the gallery's three norms over the LIVE rows (a
    superset of every query's admissible rows, so ids do not enter the bounds) - a removed NaN or huge row no longer costs every
    query its certificate.  The exact fallback runs the filtered ``search`` per gallery chunk with the same ids and mask.  A call
    without ids and without ``live=`` on an index with nothing removed runs exactly the unfiltered code."""
    from . import ops
    if not isinstance(queries, torch.Tensor) or queries.dim() != 2:
        raise ValueError("search_compact: queries must be a [nQ, E] tensor")
    own = isinstance(gallery, CompactGalleryIndex)
    filtered = query_ids is not None or gallery_ids is not None or live is not None or (own and gallery.live is not None)
    call_live = live
    if filtered:
        if not own and not (isinstance(gallery, torch.Tensor) and gallery.dim() == 2):
            raise ValueError("search_compact: gallery must be a [N, E] tensor or a CompactGalleryIndex")
        query_ids, gallery_ids, live = _search_filter(queries, gallery, query_ids, gallery_ids, live, name="search_compact")
    g_cuda = gallery.coarse.is_cuda if own else (isinstance(gallery, torch.Tensor) and gallery.is_cuda)
    if not queries.is_cuda or not g_cuda:
        raise RuntimeError("search_compact runs on the HIP kernels: device tensors only")
    if fallback not in ("exact", "none"):
        raise ValueError(f"search_compact: fallback = {fallback!r} (\"exact\" or \"none\")")
    index = gallery if own else CompactGalleryIndex(gallery, cosine=cosine)
    nQ, E = queries.shape
    assert E == index.E, (queries.shape, index.E)
    k, D = int(k), int(depth)
    assert 1 <= k <= D <= 32, f"k = {k}, depth = {D}: 1 <= k <= depth <= 32"
    bounds = (index.gmax, index.gtmax, index.dmax)                    # the index's own mask (or none): its bounds are kept up to date
    if call_live is not None:                                         # a mask of the call: the effective mask (uint8) and its bounds
        if index.live is not None:
            live = ((live != 0) & index.live).view(torch.uint8)
        bounds = index._bounds(live)
    dev = queries.device
    vals = torch.empty(nQ, k, device=dev, dtype=torch.float32)
    idx = torch.empty(nQ, k, device=dev, dtype=torch.int32)
    cert = torch.empty(nQ, device=dev, dtype=torch.uint8)
    if nQ == 0:
        return vals, idx.long(), cert.bool()
    q = _rows_f32(queries)
    if slabs is not None and filtered:                                # any number of slabs is legal: an empty one writes no entry
        slabs = max(int(slabs), 1)
    elif slabs is not None:    # at most ``slabs`` slabs of whole column tiles, none of them empty (sc_search_slabs' rule)
        nT = max(-(-index.N // 128), 1)
        slabs = -(-nT // -(-nT // max(min(int(slabs), nT), 1)))
    chunk = min(_INDEX_CHUNK_ROWS, _up128(nQ))
    qbuf = torch.empty(chunk, index.Ep, device=dev, dtype=torch.bfloat16)                # the one query buffer of the call
    for r0 in range(0, nQ, chunk):
        r1 = min(nQ, r0 + chunk)
        qc = q[r0:r1]
        q_scale = ops.vq_prep(qc)[1] if cosine else None
        q16, norms = ops.rows_bf16(qc, q_scale, out=qbuf[: _up128(r1 - r0)])
        eps = compact_eps(norms, *bounds, index.Ep).float()
        if filtered:                                                  # the candidates and the certificate over the admissible rows
            part = ops.search_coarse_filtered(q16, index.coarse, r1 - r0, index.N, D, q_ids=None if query_ids is None else query_ids[r0:r1],
                                              g_ids=gallery_ids, live=live, slabs=slabs)
            cv, ci = ops.search_merge(part, D)
            rerank = ops.search_rerank_filtered
        else:
            cv, ci = ops.search_coarse(q16, index.coarse, r1 - r0, index.N, D, slabs=slabs)
            rerank = ops.search_rerank
        rerank(qc, q_scale, index.rows, index.rnorm, ci, cv, eps, k, vals=vals[r0:r1], idx=idx[r0:r1], certified=cert[r0:r1])
    cert = cert.bool()
    if fallback == "exact":
        todo = torch.nonzero(~cert).squeeze(1)                        # the host reads the mask here
        if todo.numel():
            fv, fi = _exact_fallback(q[todo].contiguous(), index, k, cosine, None if query_ids is None else query_ids[todo], gallery_ids, live)
            vals[todo] = fv
            idx[todo] = fi
    return vals, idx.long(), cert


# ------------------------------------------------------------------------------------------------ ranks without the score matrix
# What ``_recall`` needs of a query is one integer: how many candidates are ahead of its best correct candidate.  csrc/rank.hip
# produces that integer for every row AND every column in the epilogue of the score GEMM ``search`` runs, so recall at any k, median
# and mean rank in both directions come from two integer vectors and no [nA, nB] array exists (avssl/module/retrieval.py:45-121 on
# the scores of avssl/model/kwClip.py:447-482).
def _never_hits(ahead: torch.Tensor, best: torch.Tensor, n_candidates: int) -> torch.Tensor:
    """the finishing rule of the rank kernel's counts: a query whose ``best`` is not finite - key 0 (no correct, non-NaN, live
    candidate) came back as -inf; +inf: an overflowed score - gets ``ahead`` = the number of candidates.  -> int64"""
    return torch.where(torch.isfinite(best), ahead.long(), torch.full((), n_candidates, dtype=torch.int64, device=ahead.device))


def mutual_ranks(A: torch.Tensor, B: Union[torch.Tensor, GalleryIndex], a_ids: torch.Tensor, b_ids: torch.Tensor, cosine: bool = False,
                 slabs: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """A [nA, E], B [nB, E] (or a GalleryIndex of it), a_ids [nA], b_ids [nB] integer ids; row j of B is a correct candidate for row i
    of A (and the other way round) iff a_ids[i] == b_ids[j].  -> {"ahead_AB" [nA] int64, "ahead_BA" [nB] int64, "best_AB" [nA] fp32,
    "best_BA" [nB] fp32} on the device: ``best`` is the score of a query's best correct candidate (-inf: it has none, or only NaN
    ones) and ``ahead`` the number of candidates ranked ahead of it by ``_recall``'s rule: a higher score, or a wrong candidate with
    the same score (ties count against the query) or a NaN score.  A query without a correct candidate, or whose best correct score is
    not finite, gets ``ahead`` = the number of candidates: it never hits.  rank = ahead + 1.

    Scores are ``search``'s: the three-way bf16 splits of both rows multiplied on the bf16 matrix pipe, six K-blocks summed in fp32,
    within (6 Ep + 8) 2^-24 sum_i |a_i| |b_i| of the exact inner product (Ep = E rounded up to 64); an infinity in a row becomes NaN
    in the split.  ``cosine=True`` scales the rows of A and B by 1 / max(|x|, 1e-8) first (a GalleryIndex carries its own choice).
    A is split once, in chunks of rows like a GalleryIndex (12 Ep bytes per row, no second fp32 copy).  ``slabs``: slabs of B's rows
    in the kernel (tests); the result is bitwise independent of it and of the run."""
    from . import ops
    if not isinstance(A, torch.Tensor) or A.dim() != 2:
        raise ValueError("mutual_ranks: A must be a [nA, E] tensor")
    b_cuda = B.split.is_cuda if isinstance(B, GalleryIndex) else (isinstance(B, torch.Tensor) and B.is_cuda)
    if not A.is_cuda or not b_cuda:
        raise RuntimeError("mutual_ranks runs on the HIP kernels: device tensors only")
    index = B if isinstance(B, GalleryIndex) else GalleryIndex(B, cosine=cosine)
    nA, E = A.shape
    nB = index.N
    assert E == index.E, (A.shape, index.E)
    if a_ids.dim() != 1 or b_ids.dim() != 1 or a_ids.numel() != nA or b_ids.numel() != nB:
        raise AssertionError(f"ids {tuple(a_ids.shape)} / {tuple(b_ids.shape)} do not match {nA} x {nB} rows")
    dev = A.device
    a_ids = a_ids.to(device=dev, dtype=torch.int64).contiguous()
    b_ids = b_ids.to(device=dev, dtype=torch.int64).contiguous()
    a_split = _split_in_chunks(A, 0, cosine)
    best_a, ahead_a, best_b, ahead_b = ops.rank_counts(a_split, index.split, a_ids, b_ids, nA, nB, slabs=slabs)
    return {"ahead_AB": _never_hits(ahead_a, best_a, nB), "ahead_BA": _never_hits(ahead_b, best_b, nA), "best_AB": best_a, "best_BA": best_b}


def recall_from_ranks(ahead: torch.Tensor, n_candidates: int, ks: Sequence[int], cand_title: str = "") -> Dict[str, float]:
    """ahead [Q] (candidates ahead of each query's best correct one; ``n_candidates`` for a query that never hits) -> recall@k in per
    cent for every k of ``ks`` as ``_recall`` reports it (a hit iff ahead < k, any k), and with rank = ahead + 1 ``median_rank`` (the
    mean of the two middle ranks when Q is even) and ``mean_rank``."""
    out = {}
    for k in ks:
        if k > n_candidates:
            print(f"recall@{k} asks for more than the {n_candidates} {cand_title + ' ' if cand_title else ''}candidates there are; counted over all of them")
        out[f"recall@{k}"] = 100.0 * (ahead < k).float().mean().item()
    Q = ahead.numel()
    if Q == 0:
        out["median_rank"] = out["mean_rank"] = float("nan")
        return out
    rank = torch.sort(ahead.reshape(-1).double() + 1.0).values
    out["median_rank"] = 0.5 * (rank[(Q - 1) // 2] + rank[Q // 2]).item()
    out["mean_rank"] = rank.mean().item()
    return out


def _recall_triple(ahead_ab: torch.Tensor, ahead_ba: torch.Tensor, n_b: int, n_a: int, recall_at: list, title_b: str, title_a: str,
                   rank_stats: bool) -> Tuple[dict, dict, dict]:
    """the two directions' ``ahead`` vectors, candidate counts and candidate titles -> ``mutualRetrieval``'s (A -> B, B -> A, mean)
    dictionaries, with ``median_rank`` and ``mean_rank`` in each under ``rank_stats``"""
    results_AB = recall_from_ranks(ahead_ab, n_b, recall_at, title_b)
    results_BA = recall_from_ranks(ahead_ba, n_a, recall_at, title_a)
    if not rank_stats:
        for res in (results_AB, results_BA):
            del res["median_rank"], res["mean_rank"]
    return results_AB, results_BA, _mean_results(results_AB, results_BA)


def mutual_recall(A: torch.Tensor, B: Union[torch.Tensor, GalleryIndex], AB_answers: torch.Tensor, BA_answers: torch.Tensor,
                  recall_at: list, modality_A_title: str = "audio", modality_B_title: str = "image", cosine: bool = False,
                  slabs: Optional[int] = None, rank_stats: bool = False) -> Tuple[dict, dict, dict]:
    """``mutualRetrieval``'s three dictionaries (A -> B, B -> A, their mean) from the embeddings instead of the score matrices:
    ``mutual_recall(A, B, ...)`` reports what ``mutualRetrieval(A @ B.t(), (A @ B.t()).t(), ...)`` reports, on ``mutual_ranks``' scores
    and without the [nA, nB] matrix.  ``AB_answers`` [nA] / ``BA_answers`` [nB]: the ids of A's and B's rows.  ``rank_stats=True``
    adds ``median_rank`` and ``mean_rank`` (rank = ahead + 1) to every dictionary.  The scores differ from a torch matmul's in the last
    bits (see ``mutual_ranks``): two candidates whose exact scores are closer than twice that bound may rank in either order."""
    if AB_answers.dim() != 1 or BA_answers.dim() != 1:
        raise AssertionError("answers must be 1-d id vectors")
    ranks = mutual_ranks(A, B, AB_answers, BA_answers, cosine=cosine, slabs=slabs)
    return _recall_triple(ranks["ahead_AB"], ranks["ahead_BA"], BA_answers.numel(), AB_answers.numel(), recall_at, modality_B_title,
                          modality_A_title, rank_stats)


# ------------------------------------------------------------------------------------------------ ranks over a sharded gallery
# ``mutual_ranks`` wants all of A and all of B in one GalleryIndex.  csrc/rank.hip also runs its two phases as accumulating entries
# per (A, shard) pair: every shard's "best" first - between ranks the row keys meet in an all-reduce(MAX) -, then every shard's
# "ahead".  A score depends only on its row of A, its row of B and the fixed K order, so the ranks are those of the whole gallery,
# exactly: integers, no tolerance.
def mutual_ranks_sharded(A: torch.Tensor, index: ShardedGalleryIndex, a_ids: torch.Tensor, cosine: bool = False) -> dict:
    """``mutual_ranks`` of A [nA, E] (ids ``a_ids`` [nA] int64) against a ShardedGalleryIndex built with ``ids=``: row j of the gallery
    is a correct candidate of row i of A iff index.ids[j] == a_ids[i].  -> {"ahead_AB" [nA] int64, "best_AB" [nA] fp32, "ahead_BA" [N]
    int64, "best_BA" [N] fp32, "n_A", "n_B_live"}: ``mutual_ranks``' vectors on the whole gallery for every partition into shards,
    exactly.  Removed rows of the index are no candidates and no queries: they carry ahead_BA = -1 and best_BA = -inf.  A query
    without a correct live candidate, or whose best is not finite, gets ``ahead`` = the number of candidates: ``n_B_live`` for
    A -> B, ``n_A`` for B -> A.  ``cosine`` applies to A (the index carries its own choice).

    A is split once; ops.rank_best runs over every shard with the shard's ids and ``live`` mask, then ops.rank_ahead over every
    shard (csrc/rank.hip).  No [nA, N] matrix exists.

    Distributed index (``index.group``): the call is COLLECTIVE.  Every rank passes its OWN rows of A and their ids (the counts may
    differ, 0 is legal); they are all-gathered, every rank runs "best" for all of A against its shard, the row keys are combined by
    all_reduce(MAX) - as unsigned values in int64 -, "ahead" runs with the global keys and the row counts are combined by
    all_reduce(SUM).  The column results are complete on the rank that holds the rows, because it saw all of A.  Every rank
    returns the A -> B entries of its own queries and the B -> A entries of its own gallery rows; ``n_A`` is the global query count."""
    from . import ops
    if not isinstance(index, ShardedGalleryIndex):
        raise ValueError("mutual_ranks_sharded: index must be a ShardedGalleryIndex (a tensor or a GalleryIndex goes to mutual_ranks)")
    if index.ids is None:
        raise ValueError("mutual_ranks_sharded: a ShardedGalleryIndex built without ids= (the ids say which row is correct)")
    if not isinstance(A, torch.Tensor) or A.dim() != 2:
        raise ValueError("mutual_ranks_sharded: A must be a [nA, E] tensor")
    nA = A.shape[0]
    ops.check_filter_tensor("mutual_ranks_sharded", "a_ids", a_ids, nA)
    if not A.is_cuda or not a_ids.is_cuda:
        raise RuntimeError("mutual_ranks_sharded runs on the HIP kernels: device tensors only")
    assert A.shape[1] == index.E, (A.shape, index.E)
    dev, group = A.device, index.group
    own0 = 0
    if group is not None:
        import torch.distributed as dist
        counts = [c[0] for c in _exchange_counts([nA], dev, group)]
        own0 = sum(counts[: dist.get_rank(group)])
        if sum(counts):                                               # the same on every rank: so are the collectives below
            A = _gather_rows(_rows_f32(A), counts, group)
            a_ids = _gather_rows(a_ids, counts, group)
    nAll = A.shape[0]
    a_split = _split_in_chunks(A, 0, cosine)
    off = [0]
    for shard in index.shards:
        off.append(off[-1] + shard.N)
    n_loc = off[-1]                                                   # gallery rows on this device
    out = torch.zeros(2 * (nAll + n_loc), device=dev, dtype=torch.int32)      # keys and counts of the call, zeroed in one fill
    key_a, ahead_a, key_b, ahead_b = out[:nAll], out[nAll: 2 * nAll], out[2 * nAll: 2 * nAll + n_loc], out[2 * nAll + n_loc:]
    for shard, o in zip(index.shards, off):
        ops.rank_best(a_split, shard.split, a_ids, shard.ids, nAll, shard.N, key_a, key_b[o: o + shard.N], b_live=shard.live)
    if group is not None and nAll:
        # uint32 keys in int32 storage: a signed MAX would put every key of a positive score (>= 2^31) below the others
        wide = key_a.long() & 0xFFFFFFFF
        dist.all_reduce(wide, op=dist.ReduceOp.MAX, group=group)
        key_a.copy_(torch.where(wide >= 2 ** 31, wide - 2 ** 32, wide))
    for shard, o in zip(index.shards, off):
        ops.rank_ahead(a_split, shard.split, a_ids, shard.ids, nAll, shard.N, key_a, key_b[o: o + shard.N], ahead_a, ahead_b[o: o + shard.N],
                       b_live=shard.live)
    ahead_a = ahead_a.long()
    if group is not None and nAll:
        dist.all_reduce(ahead_a, op=dist.ReduceOp.SUM, group=group)
    n_live = index.n_live
    best_a, best_b = ops._rank_key_value(key_a), ops._rank_key_value(key_b)
    ahead_a, ahead_b = _never_hits(ahead_a, best_a, n_live), _never_hits(ahead_b, best_b, nAll)
    if any(shard.live is not None for shard in index.shards):
        live = torch.cat([torch.ones(shard.N, device=dev, dtype=torch.bool) if shard.live is None else shard.live for shard in index.shards])
        ahead_b = torch.where(live, ahead_b, torch.full((), -1, dtype=torch.int64, device=dev))     # best_b is -inf there: its key was never written
    return {"ahead_AB": ahead_a[own0: own0 + nA], "best_AB": best_a[own0: own0 + nA], "ahead_BA": ahead_b, "best_BA": best_b,
            "n_A": nAll, "n_B_live": n_live}


def mutual_recall_sharded(A: torch.Tensor, index: ShardedGalleryIndex, AB_answers: torch.Tensor, recall_at: list,
                          modality_A_title: str = "audio", modality_B_title: str = "image", cosine: bool = False,
                          rank_stats: bool = False) -> Tuple[dict, dict, dict]:
    """``mutual_recall``'s three dictionaries over the whole set from ``mutual_ranks_sharded``: A -> B over all queries, B -> A over
    the live rows of the gallery (``AB_answers`` [nA] int64: the ids of A's rows; the gallery's are ``index.ids``).  Distributed
    index: COLLECTIVE; the two ``ahead`` vectors are all-gathered, so every rank returns the same dictionaries."""
    ranks = mutual_ranks_sharded(A, index, AB_answers, cosine=cosine)
    ahead_ab, ahead_ba = ranks["ahead_AB"], ranks["ahead_BA"]
    if index.group is not None:
        counts = _exchange_counts([ahead_ab.numel(), ahead_ba.numel()], ahead_ab.device, index.group)
        if sum(c[0] for c in counts):
            ahead_ab = _gather_rows(ahead_ab.contiguous(), [c[0] for c in counts], index.group)
        if sum(c[1] for c in counts):
            ahead_ba = _gather_rows(ahead_ba.contiguous(), [c[1] for c in counts], index.group)
    ahead_ba = ahead_ba[ahead_ba >= 0]                                # a removed row is no query
    return _recall_triple(ahead_ab, ahead_ba, ranks["n_B_live"], ranks["n_A"], recall_at, modality_B_title, modality_A_title, rank_stats)
