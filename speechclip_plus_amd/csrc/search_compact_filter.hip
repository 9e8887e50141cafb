// Filtered compact gallery search (gfx950): search_compact.hip's coarse top-D scan and exact re-rank over the ADMISSIBLE gallery rows
// only, with the certificate restated over them.
//   replaces: score.masked_fill(mask, -inf) + torch.argsort over the whole [nQ, N] score matrix (avssl/module/retrieval.py:45-46 on
//             the scores of avssl/model/kwClip.py:447-482) when a query's own item, its sibling captions or removed gallery rows must
//             stay out of the ranking - on the 2 Ep bytes per gallery row of the compact index.
//
// Rule (include/speechclip_hip.h states it once for every layer): gallery row j is admissible for query i iff j < N, live is NULL or
// live[j] != 0, and the ids are NULL or g_ids[j] != q_ids[i] (int64, all 64 bits).
//
//   sc_search_coarse_filtered_bf16  search_kernels.h's search_scan_kernel<true> at K = Ep: sc_search_coarse_bf16's operands, arithmetic
//                                   and K-tile order, so an admissible row carries the same fp32 bits.  The admissibility test sits
//                                   in front of the D-th-key test and no LDS is spent on ids (at D = 32 the ring and the lists
//                                   already take 98 304 B).  With a filter ANY slab can hold fewer than D admissible columns, so the
//                                   per-slab lists leave as the 64-bit words of the LDS lists themselves (key << 32 | ~column, 0 = no
//                                   entry): sc_search_merge_u64 merges and decodes them.
//   sc_search_rerank_filtered_f32   search_kernels.h's search_rerank_kernel<true>: sc_search_rerank_f32 with the certificate over
//                                   the admissible rows.  The candidates are a query's D best ADMISSIBLE rows, so "fewer than D
//                                   candidates" means every admissible row is one - that clause stands where the unfiltered kernel
//                                   has N <= D.
// No atomics, nothing allocated, fixed-order reductions: same input, same bits, for every S.
#include "search_kernels.h"

#include <algorithm>

extern "C" int sc_search_coarse_filtered_bf16(const sc_bf16* q_bf16, const sc_bf16* g_bf16, int32_t nQ, int32_t N, int32_t Ep, int32_t D,
                                              int32_t S, const int64_t* q_ids, const int64_t* g_ids, const uint8_t* live, uint64_t* part,
                                              void* stream) {
    SC_CHECK(nQ >= 0 && N >= 0, "sc_search_coarse_filtered_bf16: nQ >= 0, N >= 0 (nQ %d, N %d)", nQ, N);
    SC_CHECK(D >= 1 && D <= SEARCH_MAXK, "sc_search_coarse_filtered_bf16: 1 <= D <= 32 (D %d)", D);
    SC_CHECK(Ep > 0 && Ep % 64 == 0, "sc_search_coarse_filtered_bf16: Ep=%d must be a multiple of 64", Ep);
    SC_CHECK(S >= 1, "sc_search_coarse_filtered_bf16: S >= 1 (S %d)", S);
    SC_CHECK((q_ids == nullptr) == (g_ids == nullptr) || nQ == 0 || N == 0,
             "sc_search_coarse_filtered_bf16: ids on one side only (q_ids %s, g_ids %s): give both or neither", q_ids ? "given" : "NULL",
             g_ids ? "given" : "NULL");
    if (nQ == 0) return 0;
    SC_CHECK(part, "sc_search_coarse_filtered_bf16: null output");
    SC_CHECK(N == 0 || (q_bf16 && g_bf16), "sc_search_coarse_filtered_bf16: null operand");
    SC_CHECK(((uintptr_t)q_bf16 % 16) == 0 && ((uintptr_t)g_bf16 % 16) == 0,
             "sc_search_coarse_filtered_bf16: operands must be 16-byte aligned");
    SC_CHECK(((uintptr_t)q_ids % 8) == 0 && ((uintptr_t)g_ids % 8) == 0 && ((uintptr_t)part % 8) == 0,
             "sc_search_coarse_filtered_bf16: ids and part must be 8-byte aligned");
    const int64_t nM = ((int64_t)nQ + BM - 1) / BM;
    const int64_t nT = ((int64_t)N + BN - 1) / BN;
    const int64_t tiles = std::max<int64_t>((nT + S - 1) / S, 1);     // a slab past the last tile writes an empty list: the merge copes
    SC_CHECK(nM * S < ((int64_t)1 << 31), "sc_search_coarse_filtered_bf16: %lld workgroups", (long long)(nM * S));
    SearchScanArgs a{};
    a.q = (const uint16_t*)q_bf16;
    a.g = (const uint16_t*)g_bf16;
    a.nQ = nQ; a.N = N; a.K = Ep; a.k = D; a.S = S; a.tiles = (int)tiles;
    const bool ids = q_ids && g_ids;
    a.q_ids = ids ? q_ids : nullptr;
    a.g_ids = ids ? g_ids : nullptr;
    a.live = N > 0 ? live : nullptr;
    a.part = part;
    return search_scan_launch<true>(a, nM * S, "search_coarse_filtered", (hipStream_t)stream);
}

extern "C" int sc_search_rerank_filtered_f32(const float* q, int64_t ldq, const float* q_scale, const float* rows, int64_t ldr,
                                             const float* g_scale, const int32_t* cand_idx, const float* cand_vals, const float* eps,
                                             int32_t nQ, int32_t N, int32_t E, int32_t D, int32_t k, float* vals, int32_t* idx,
                                             uint8_t* certified, void* stream) {
    return search_rerank<true>("sc_search_rerank_filtered_f32", q, ldq, q_scale, rows, ldr, g_scale, cand_idx, cand_vals, eps, nQ, N, E, D, k,
                               vals, idx, certified, stream);
}
