// Gallery search (gfx950): for every query the k best gallery rows, with the selection fused into the score GEMM's epilogue - the
// [nQ, N] score matrix never exists in memory.
//   replaces: torch.argsort(score, descending=True) of the whole score matrix (avssl/module/retrieval.py:45-46) on the scores of
//             avssl/model/kwClip.py:447-482, where only the first max(recall_at) entries of a row are ever looked at.
//
// Scores: the arithmetic of ops.cosine_scores_split.  Both operands are the three-way bf16 splits sc_split3_bf16 writes (queries
// side 0, gallery side 1, rows padded to 128, K6 = 6 Ep columns); a score is the fp32 sum of the six K-blocks, K-tiles in increasing
// order: search_tile.h's tile at K = K6.
//
// Grid: row tiles of 128 queries x S column slabs of the gallery; a slab is ``tiles`` whole column tiles of 128 gallery rows.  The
// kernel is search_kernels.h's search_scan_kernel<false>: after a tile's K loop the waves scan the scores in LDS into a row's list of
// k sorted words.  Columns >= N are excluded by their index.
//
// Order contract (search_common.h): larger value first, lower gallery index first among equal values (-0 == +0), NaN above every
// number, lower index first among NaNs, fewer than k columns: the tail is -inf / -1.  The value written is the key mapped back:
// a zero comes back as +0 and every NaN as the default NaN.
//
// Every (row tile, slab) writes its k candidates to part_vals / part_idx [nQ, S, k]; the caller merges the S lists of a row with
// sc_topk_rows_f32 over [nQ, S k] (position order = lower slab first = lower columns first, and only the last slab's list can end in
// -inf / -1 fillers because every other slab holds 128 >= k valid columns per tile) and one gather of the indices.  S = 1: the lists
// are the result.  No atomics; a score's arithmetic does not depend on S, so neither does the result.
#include "search_kernels.h"

#include <algorithm>

extern "C" int sc_search_slabs(int32_t nQ, int32_t N, int32_t k) {
    (void)k;                                                          // whole 128-column tiles hold >= 32 >= k columns each
    if (nQ <= 0 || N <= 0) return 1;
    const int64_t nM = ((int64_t)nQ + BM - 1) / BM, nT = ((int64_t)N + BN - 1) / BN;
    const int64_t cus = sc_num_cus();
    if (nM >= cus) return 1;                                          // the row tiles alone cover the chip
    // at most two workgroups per CU (what fits at k <= 16), rounded DOWN: a few workgroups over one round cost a whole second round
    // (8 192 x 262 144 x 768: 23.8 ms at 64 x 8 workgroups, 31.8 ms at 64 x 12)
    const int64_t want = std::min<int64_t>(std::max<int64_t>(2 * cus / nM, 1), nT);
    const int64_t tiles = (nT + want - 1) / want;
    return (int)((nT + tiles - 1) / tiles);                           // whole tiles per slab, the last slab not empty
}

extern "C" int sc_search_topk_bf16(const sc_bf16* q_split, const sc_bf16* g_split, int32_t nQ, int32_t N, int32_t K6, int32_t k, int32_t S,
                                   float* part_vals, int32_t* part_idx, void* stream) {
    SC_CHECK(nQ >= 0 && N >= 0, "sc_search_topk_bf16: nQ >= 0, N >= 0 (nQ %d, N %d)", nQ, N);
    SC_CHECK(k >= 1 && k <= 32, "sc_search_topk_bf16: 1 <= k <= 32 (k %d)", k);
    SC_CHECK(K6 > 0 && K6 % 384 == 0, "sc_search_topk_bf16: K6=%d must be 6 Ep with Ep a multiple of 64", K6);
    SC_CHECK(S >= 1, "sc_search_topk_bf16: S >= 1 (S %d)", S);
    const int64_t nT = ((int64_t)N + BN - 1) / BN;
    const int64_t tiles = std::max<int64_t>((nT + S - 1) / S, 1);
    // every slab but the last must hold at least k valid columns (the merge relies on fillers only at the very end): with whole
    // 128-column tiles that is "the last slab is not empty" - then every earlier slab is made of full tiles
    SC_CHECK(S == 1 || (int64_t)(S - 1) * tiles < nT,
             "sc_search_topk_bf16: S=%d slabs of %lld column tiles leave a slab before the last with fewer than k columns (N %d: %lld tiles)", S,
             (long long)tiles, N, (long long)nT);
    if (nQ == 0) return 0;
    SC_CHECK(part_vals && part_idx, "sc_search_topk_bf16: null output");
    SC_CHECK(N == 0 || (q_split && g_split), "sc_search_topk_bf16: null operand");
    SC_CHECK(((uintptr_t)q_split % 16) == 0 && ((uintptr_t)g_split % 16) == 0, "sc_search_topk_bf16: operands must be 16-byte aligned");
    const int64_t nM = ((int64_t)nQ + BM - 1) / BM;
    SC_CHECK(nM * S < ((int64_t)1 << 31), "sc_search_topk_bf16: %lld workgroups", (long long)(nM * S));
    SearchScanArgs a{};
    a.q = (const uint16_t*)q_split;
    a.g = (const uint16_t*)g_split;
    a.nQ = nQ; a.N = N; a.K = K6; a.k = k; a.S = S; a.tiles = (int)tiles;
    a.part_vals = part_vals;
    a.part_idx = part_idx;
    return search_scan_launch<false>(a, nM * S, "search", (hipStream_t)stream);
}
