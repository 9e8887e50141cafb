// Filtered gallery search (gfx950): search.hip's top-k and topk.hip's row selection over the ADMISSIBLE gallery rows only.
//   replaces: score.masked_fill(mask, -inf) + torch.topk over the whole [nQ, N] score matrix - what excluding a query's own item and
//             its sibling captions, mining the k highest-scoring wrong items of an anchor, or dropping removed gallery rows costs on
//             the scores of avssl/model/kwClip.py:447-482 (ranked by avssl/module/retrieval.py:45-46).
//
// Rule (include/speechclip_hip.h states it once for every layer): gallery row j is admissible for query i iff j < N, live is NULL or
// live[j] != 0, and the ids are NULL or g_ids[j] != q_ids[i] (int64, all 64 bits).  The result is csrc/topk.hip's order contract over
// the admissible rows: larger score first, lower gallery row first among equal scores (-0 == +0), NaN above every number, -inf / -1
// behind the last admissible row.  An inadmissible row never appears whatever its score; an admissible row keeps the fp32 bits the
// unfiltered kernels give it; a real -inf ranks ahead of every filler.
//
//   sc_search_topk_filtered_bf16  search_kernels.h's search_scan_kernel<true> on search.hip's operands (K = K6): the admissibility test
//                                 sits in front of the k-th-key test, so an inadmissible column never pays for an insertion.  With a
//                                 filter ANY slab can hold fewer than k admissible columns, so the per-slab lists leave as the 64-bit
//                                 words themselves (0 = no entry).
//   sc_search_merge_u64           one wave per query: the k largest of its S k words, decoded.  Words of distinct columns are
//                                 distinct, so the order is total; a real -inf has key 0x007fffff > 0 and sorts above a filler
//                                 wherever its slab is.
//   sc_topk_rows_filtered_f32     topk_rows.h's row selection - topk.hip's - with the RowFilter policy over a score matrix: a column is
//                                 tested for admissibility only once its key would enter the lane's list, so the ids are read for
//                                 candidates, not for every score.  The score matrix is not modified.
// No atomics, nothing allocated, fixed-order reductions: same input, same bits, for every S.
#include "search_kernels.h"
#include "topk_rows.h"

#include <algorithm>

namespace {

// One wave per query row: the k largest of its n = S k words by k passes of a 64-lane maximum over the words below the last one
// taken (the words of a row are distinct but for the zeros, and n is a few hundred: the row stays in cache), then decoded.
__global__ __launch_bounds__(256) void search_merge_kernel(const uint64_t* __restrict__ part, int nQ, int n, int k, float* __restrict__ vals,
                                                           int32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= nQ) return;                                     // whole waves leave together: no barrier below
    const uint64_t* __restrict__ w = part + (int64_t)r * n;
    uint64_t prev = 0ull, out = 0ull;
    for (int p = 0; p < k; ++p) {
        uint64_t best = 0ull;
        for (int i = lane; i < n; i += 64) {
            const uint64_t x = w[i];
            if ((p == 0 || x < prev) && x > best) best = x;  // p == 0: the all-ones word (NaN at column 0) is a legal entry
        }
        best = wave_max_u64(best);
        if (best == 0ull) break;                             // fewer than k entries: wave-uniform
        if (lane == p) out = best;
        prev = best;
    }
    if (lane < k) {
        const int64_t o = (int64_t)r * k + lane;
        vals[o] = tk_value(tk_word_key(out));                // no entry: -inf
        idx[o] = tk_word_col(out);                           // no entry: ~0 = -1
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void topk_rows_filtered_kernel(const float* __restrict__ scores, int64_t ld, int rows, int V, int k,
                                                                 const int64_t* __restrict__ q_ids, const int64_t* __restrict__ g_ids,
                                                                 const uint8_t* __restrict__ live, float* __restrict__ vals,
                                                                 int32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                   // whole waves leave together: no barrier below
    RowFilter f;
    f.g_ids = g_ids;
    f.live = live;
    f.qid = g_ids ? q_ids[r] : 0;
    topk_select_row<VEC>(scores + (int64_t)r * ld, V, k, lane, f, vals + (int64_t)r * k, idx + (int64_t)r * k);
}

}  // namespace

extern "C" int sc_search_topk_filtered_bf16(const sc_bf16* q_split, const sc_bf16* g_split, int32_t nQ, int32_t N, int32_t K6, int32_t k,
                                            int32_t S, const int64_t* q_ids, const int64_t* g_ids, const uint8_t* live, uint64_t* part,
                                            void* stream) {
    SC_CHECK(nQ >= 0 && N >= 0, "sc_search_topk_filtered_bf16: nQ >= 0, N >= 0 (nQ %d, N %d)", nQ, N);
    SC_CHECK(k >= 1 && k <= 32, "sc_search_topk_filtered_bf16: 1 <= k <= 32 (k %d)", k);
    SC_CHECK(K6 > 0 && K6 % 384 == 0, "sc_search_topk_filtered_bf16: K6=%d must be 6 Ep with Ep a multiple of 64", K6);
    SC_CHECK(S >= 1, "sc_search_topk_filtered_bf16: S >= 1 (S %d)", S);
    SC_CHECK((q_ids == nullptr) == (g_ids == nullptr) || nQ == 0 || N == 0,
             "sc_search_topk_filtered_bf16: ids on one side only (q_ids %s, g_ids %s): give both or neither", q_ids ? "given" : "NULL",
             g_ids ? "given" : "NULL");
    if (nQ == 0) return 0;
    SC_CHECK(part, "sc_search_topk_filtered_bf16: null output");
    SC_CHECK(N == 0 || (q_split && g_split), "sc_search_topk_filtered_bf16: null operand");
    SC_CHECK(((uintptr_t)q_split % 16) == 0 && ((uintptr_t)g_split % 16) == 0,
             "sc_search_topk_filtered_bf16: operands must be 16-byte aligned");
    SC_CHECK(((uintptr_t)q_ids % 8) == 0 && ((uintptr_t)g_ids % 8) == 0 && ((uintptr_t)part % 8) == 0,
             "sc_search_topk_filtered_bf16: ids and part must be 8-byte aligned");
    const int64_t nM = ((int64_t)nQ + BM - 1) / BM;
    const int64_t nT = ((int64_t)N + BN - 1) / BN;
    const int64_t tiles = std::max<int64_t>((nT + S - 1) / S, 1);     // a slab past the last tile writes an empty list: the merge copes
    SC_CHECK(nM * S < ((int64_t)1 << 31), "sc_search_topk_filtered_bf16: %lld workgroups", (long long)(nM * S));
    SearchScanArgs a{};
    a.q = (const uint16_t*)q_split;
    a.g = (const uint16_t*)g_split;
    a.nQ = nQ; a.N = N; a.K = K6; a.k = k; a.S = S; a.tiles = (int)tiles;
    const bool ids = q_ids && g_ids;
    a.q_ids = ids ? q_ids : nullptr;
    a.g_ids = ids ? g_ids : nullptr;
    a.live = N > 0 ? live : nullptr;
    a.part = part;
    return search_scan_launch<true>(a, nM * S, "search_filter", (hipStream_t)stream);
}

extern "C" int sc_search_merge_u64(const uint64_t* part, int32_t nQ, int32_t S, int32_t k, float* vals, int32_t* idx, void* stream) {
    SC_CHECK(nQ >= 0, "sc_search_merge_u64: nQ >= 0 (nQ %d)", nQ);
    SC_CHECK(k >= 1 && k <= 32, "sc_search_merge_u64: 1 <= k <= 32 (k %d)", k);
    SC_CHECK(S >= 1 && (int64_t)S * k < ((int64_t)1 << 31), "sc_search_merge_u64: S >= 1 and S k < 2^31 (S %d)", S);
    if (nQ == 0) return 0;
    SC_CHECK(part && vals && idx, "sc_search_merge_u64: null pointer");
    SC_CHECK(((uintptr_t)part % 8) == 0, "sc_search_merge_u64: part must be 8-byte aligned");
    hipLaunchKernelGGL(search_merge_kernel, dim3((unsigned)((nQ + 3) / 4)), dim3(256), 0, (hipStream_t)stream, part, nQ, S * k, k, vals, idx);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_topk_rows_filtered_f32(const float* scores, int64_t ld, int32_t rows, int32_t V, int32_t k, const int64_t* q_ids,
                                         const int64_t* g_ids, const uint8_t* live, float* vals, int32_t* idx, void* stream) {
    SC_CHECK(rows >= 0 && V >= 1 && ld >= V, "sc_topk_rows_filtered_f32: rows >= 0, V >= 1, ld >= V (rows %d, V %d, ld %lld)", rows, V,
             (long long)ld);
    SC_CHECK(k >= 1 && k <= 32, "sc_topk_rows_filtered_f32: 1 <= k <= 32 (k %d)", k);
    SC_CHECK((q_ids == nullptr) == (g_ids == nullptr) || rows == 0,
             "sc_topk_rows_filtered_f32: ids on one side only (q_ids %s, g_ids %s): give both or neither", q_ids ? "given" : "NULL",
             g_ids ? "given" : "NULL");
    if (rows == 0) return 0;
    SC_CHECK(scores && vals && idx, "sc_topk_rows_filtered_f32: null pointer");
    SC_CHECK(((uintptr_t)q_ids % 8) == 0 && ((uintptr_t)g_ids % 8) == 0, "sc_topk_rows_filtered_f32: ids must be 8-byte aligned");
    const bool vec = (((uintptr_t)scores) & 15) == 0 && (ld & 3) == 0;
    const dim3 grid((rows + 3) / 4), block(256);
    if (vec)
        hipLaunchKernelGGL(topk_rows_filtered_kernel<true>, grid, block, 0, (hipStream_t)stream, scores, ld, rows, V, k, q_ids, g_ids, live, vals,
                           idx);
    else
        hipLaunchKernelGGL(topk_rows_filtered_kernel<false>, grid, block, 0, (hipStream_t)stream, scores, ld, rows, V, k, q_ids, g_ids, live, vals,
                           idx);
    SC_LAUNCH_CHECK();
    return 0;
}
