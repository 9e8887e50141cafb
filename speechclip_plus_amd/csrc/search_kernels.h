// The two kernels the gallery-search entry points share (gfx950), each written once:
//   search_scan_kernel<FILTER>      the fused top-k: search_tile.h's score tile with a list scan behind it.  Serves sc_search_topk_bf16
//                                   and sc_search_coarse_bf16 (FILTER = false) and their _filtered twins (FILTER = true); the split
//                                   and the plain bf16 operands differ only in the row width K.
//   search_rerank_kernel<FILTERED>  the exact fp64 re-rank of up to 32 candidates with the certificate; serves sc_search_rerank_f32
//                                   and sc_search_rerank_filtered_f32, which differ in one clause of the certificate.
// Both have internal linkage: a translation unit that launches an instantiation owns its copy and the LDS attribute of that copy.
//
// List scan.  After a tile's K loop the scores lie in LDS and the waves scan them: a wave owns 32 rows, a lane reads columns lane and
// lane + 64 of a row (conflict free), maps them to the sortable key and tests them against the key of the row's current k-th entry;
// only a row with a passing column pays for insertions, and a candidate overtaken by an earlier insertion of the same pass is dropped
// on one scalar compare.  A row's list is k sorted words (tk_word: key << 32 | ~column) in LDS: the wave loads it one entry per lane
// and inserts a candidate with one wave shift (every lane keeps its entry, takes the candidate, or takes its lower neighbour's
// entry) - no runtime-indexed register array.  Columns >= N are excluded by their index: the zero padding rows of the operand score
// 0, and NaN against a NaN query.  No atomics; a score's arithmetic does not depend on S, so neither does the result.
//
// FILTER adds three things.  After a tile's K loop a lane loads the id and the live byte of its two columns (nothing at or past N is
// read); a wave keeps the ids of its 32 query rows one per lane and reads the row's id into a scalar register, so the admissibility
// test is part of the ballot predicate in front of the k-th-key test: an inadmissible column never pays for an insertion and no LDS
// is spent on ids.  And the lists leave as the words themselves (0 = no entry) for sc_search_merge_u64, because with a filter ANY
// slab can hold fewer than k admissible columns; without one only the last slab can (the entry points check it), so the lists leave
// decoded, -inf / -1 fillers at the very end, and sc_topk_rows_f32 can merge them by position.
#pragma once
#include "search_tile.h"

namespace {

constexpr int SEARCH_MAXK = 32;                     // list depth: one entry per lane of half a wave

struct SearchScanArgs {
    const uint16_t* q;       // [roundup(nQ, 128), K] bf16
    const uint16_t* g;       // [roundup(N, 128), K] bf16
    int nQ, N, K, k, S, tiles;
    float* part_vals;        // [nQ, S, k]            FILTER = false: the lists, decoded
    int32_t* part_idx;
    const int64_t* q_ids;    // [nQ] or NULL (with g_ids)   FILTER = true
    const int64_t* g_ids;    // [N] or NULL
    const uint8_t* live;     // [N] or NULL
    uint64_t* part;          // [nQ, S, k] list words, best first; 0 = no entry
};

inline int search_scan_lds_bytes(int k) { return RING_BYTES + BM * k * 8; }

template <bool FILTER>
__global__ __launch_bounds__(256) void search_scan_kernel(const SearchScanArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int k = p.k;
    const bool has_ids = FILTER && p.g_ids != nullptr;
    const TileBlock blk(p.nQ, p.N, p.tiles);
    const int m0 = blk.m0;
    const ScoreTile tile(p.q, p.g, m0, p.K);
    const int lane = tile.lane, wave = tile.wave;

    float* const Cs = (float*)smem;
    uint64_t* const lists = (uint64_t*)(smem + RING_BYTES);           // [BM][k], best first; 0 = no entry (-inf / -1)

    // a wave owns the lists of its 32 rows: no other wave touches them, so no barrier orders these stores
    for (int i = lane; i < 32 * k; i += 64) lists[wave * 32 * k + i] = 0ull;

    // the ids of this wave's 32 query rows, row rr in lane rr: read back per row into scalar registers (no LDS beside the lists)
    uint32_t qid_lo = 0u, qid_hi = 0u;
    if (has_ids && lane < 32 && m0 + wave * 32 + lane < p.nQ) {
        const uint64_t v = (uint64_t)p.q_ids[m0 + wave * 32 + lane];
        qid_lo = (uint32_t)v;
        qid_hi = (uint32_t)(v >> 32);
    }
    const int rows_here = min(32, p.nQ - m0 - wave * 32);             // wave-uniform; <= 0: nothing to scan

    for (int t = blk.t_begin; t < blk.t_end; ++t) {
        const int n0 = t * BN;
        f32x4 acc[FM][FN];
        tile.scores(smem, n0, acc);

        // ---- this lane's two columns of the tile: in range and, FILTER, live, with their ids (no DMA is in flight here; the loads
        // complete under the score stores and their barrier).  g_ids / live are [N], not padded: nothing at or past N is read
        const int c0 = n0 + lane, c1 = n0 + 64 + lane;
        bool ok0 = c0 < p.N, ok1 = c1 < p.N;
        uint64_t gid0 = 0ull, gid1 = 0ull;
        if (has_ids) {
            if (ok0) gid0 = (uint64_t)p.g_ids[c0];
            if (ok1) gid1 = (uint64_t)p.g_ids[c1];
        }
        if (FILTER && p.live) {
            if (ok0) ok0 = p.live[c0] != 0;
            if (ok1) ok1 = p.live[c1] != 0;
        }

        tile.store(Cs, acc, [](float s) { return s; });

        // ---- selection: wave w scans rows 32 w .. 32 w + 31 of the tile ----------------------------------------------------
        for (int rr = 0; rr < rows_here; ++rr) {
            const int r = wave * 32 + rr;
            bool a0 = ok0, a1 = ok1;
            if (has_ids) {                                            // the row's id, wave-uniform
                const uint64_t qid = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)qid_hi, rr) << 32) |
                                     (uint32_t)__builtin_amdgcn_readlane((int)qid_lo, rr);
                a0 = a0 && gid0 != qid;
                a1 = a1 && gid1 != qid;
            }
            const uint32_t key0 = tk_key(Cs[r * BN + lane]), key1 = tk_key(Cs[r * BN + 64 + lane]);
            const uint32_t kth = tk_word_key(lists[r * k + k - 1]);
            // admissible first, then strict: a score equal to the k-th entry's has a higher column than it and stays out
            uint64_t m_lo = __ballot(a0 && key0 > kth), m_hi = __ballot(a1 && key1 > kth);
            if ((m_lo | m_hi) == 0ull) continue;
            uint64_t e = lane < k ? lists[r * k + lane] : 0ull;
            uint32_t kth_now = kth;                                   // wave-uniform: follows the list as it fills
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                uint64_t m = h ? m_hi : m_lo;
                const uint32_t keyh = h ? key1 : key0;
                while (m) {
                    const int j = __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t ck = (uint32_t)__builtin_amdgcn_readlane((int)keyh, j);
                    if (ck <= kth_now) continue;                      // overtaken by an insertion of this pass
                    const uint64_t c = tk_word(ck, n0 + h * 64 + j);
                    const uint64_t up = ((uint64_t)wave_shr1((uint32_t)(e >> 32)) << 32) | wave_shr1((uint32_t)e);
                    // entries above the candidate stay; the first one below takes it; the rest move down one place
                    e = e > c ? e : ((lane == 0 || up > c) ? c : up);
                    kth_now = (uint32_t)__builtin_amdgcn_readlane((int)tk_word_key(e), k - 1);
                }
            }
            if (lane < k) lists[r * k + lane] = e;
        }
        __syncthreads();   // the next tile's DMA overwrites the score tile
    }

    // ---- this slab's list of every row: FILTER - as words, any slab may hold fewer than k entries and the merge must see which are
    // real; else decoded
    if (lane < k) {
        for (int rr = 0; rr < rows_here; ++rr) {
            const int r = wave * 32 + rr;
            const uint64_t e = lists[r * k + lane];
            const int64_t o = ((int64_t)(m0 + r) * p.S + blk.slab) * k + lane;
            if (FILTER) {
                p.part[o] = e;
            } else {
                p.part_vals[o] = tk_value(tk_word_key(e));
                p.part_idx[o] = tk_word_col(e);                       // no entry: ~0 = -1
            }
        }
    }
}

// nwg = row tiles x S workgroups; ``what`` names the caller in the one error this can raise
template <bool FILTER>
int search_scan_launch(const SearchScanArgs& a, int64_t nwg, const char* what, hipStream_t stream) {
    static sc_lds_attr_once attr;
    if (hipError_t e = sc_set_max_lds_once(attr, search_scan_kernel<FILTER>, search_scan_lds_bytes(SEARCH_MAXK)); e != hipSuccess) {
        sc_set_error("hipFuncSetAttribute(%s): %s", what, hipGetErrorString(e));
        return -3;
    }
    hipLaunchKernelGGL(search_scan_kernel<FILTER>, dim3((unsigned)nwg), dim3(256), search_scan_lds_bytes(a.k), stream, a);
    SC_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------ exact re-rank + certificate
// One workgroup per query: a wave per candidate gathers the fp32 row and accumulates the product with the query in fp64 (both rows
// scaled in fp32 first, as sc_rows_bf16 scales them), then wave 0 ranks the D candidates by (exact key, ~row) with one comparison
// count per lane and evaluates the certificate in fp64.
struct RerankArgs {
    const float* q;          // [nQ, E], pitch ldq
    const float* q_scale;    // [nQ] or null
    const float* rows;       // [N, E], pitch ldr
    const float* g_scale;    // [N] or null
    const int32_t* cand_idx; // [nQ, D]
    const float* cand_vals;  // [nQ, D]
    const float* eps;        // [nQ]
    int64_t ldq, ldr;
    int N, E, D, k;
    float* vals;             // [nQ, k]
    int32_t* idx;            // [nQ, k]
    uint8_t* certified;      // [nQ]
};

// FILTERED: the candidates are a query's D best ADMISSIBLE rows and the certificate is stated over those
template <bool FILTERED>
__global__ __launch_bounds__(256) void search_rerank_kernel(const RerankArgs p) {
    __shared__ float ex[SEARCH_MAXK];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t qi = blockIdx.x;
    const int D = p.D, k = p.k;
    const float* __restrict__ qrow = p.q + qi * p.ldq;
    const float qs = p.q_scale ? p.q_scale[qi] : 1.f;
    const int32_t* const ci = p.cand_idx + qi * D;

    for (int j = wave; j < D; j += 4) {
        const int col = ci[j];                                        // wave-uniform
        float e = -INFINITY;
        if (col >= 0 && col < p.N) {                                  // anything else is a filler: nothing is read
            const float* __restrict__ grow = p.rows + (int64_t)col * p.ldr;
            const float gs = p.g_scale ? p.g_scale[col] : 1.f;
            double acc = 0.0;
            for (int i = lane; i < p.E; i += 64) {
                const float a = qrow[i] * qs, b = grow[i] * gs;       // the fp32 rows the coarse operands were rounded from
                acc = fma((double)a, (double)b, acc);
            }
            e = (float)wave_sum_d(acc);
        }
        if (lane == 0) ex[j] = e;
    }
    __syncthreads();
    if (wave != 0) return;

    // ---- wave 0: lane j holds candidate j; rank = how many candidates are ahead of it in (exact key, ~row) order -------------
    const bool have = lane < D;
    const int col = have ? ci[lane] : -1;
    const bool valid = have && col >= 0 && col < p.N;
    const float e = valid ? ex[lane] : -INFINITY;
    const float cv = valid ? p.cand_vals[qi * D + lane] : 0.f;
    const uint32_t key = valid ? tk_key(e) : TK_EMPTY;
    const uint32_t low = valid ? ~(uint32_t)col : 0u;
    int rank = 0;
    for (int i = 0; i < D; ++i) {
        const uint32_t ki = (uint32_t)__shfl((int)key, i), li = (uint32_t)__shfl((int)low, i);
        const bool ahead = ki > key || (ki == key && (li > low || (li == low && i < lane)));
        rank += ahead ? 1 : 0;
    }
    if (have && rank < k) {
        p.vals[qi * k + rank] = tk_value(key);
        p.idx[qi * k + rank] = valid ? col : -1;
    }
    // ---- the certificate, in fp64 ------------------------------------------------------------------------------------------
    const float eps = p.eps[qi];
    const bool finite_all = __ballot(valid && !(isfinite(e) && isfinite(cv))) == 0ull && isfinite(eps);
    const int n_valid = __popcll(__ballot(valid));
    const uint64_t at_k = __ballot(have && rank == k - 1);            // exactly one lane: the ranks are a permutation of 0 .. D - 1
    const float e_k = __shfl(e, __builtin_ctzll(at_k | (1ull << 63)));
    const float t = p.cand_vals[qi * D + D - 1];
    int cert = 0;
    if (finite_all) {
        if (FILTERED) {                                               // over the admissible rows
            if (n_valid < D)
                cert = 1;                                             // every admissible row is a candidate (none at all included)
            else
                cert = ((double)e_k - fabs((double)e_k) * 0x1p-23 > (double)t + (double)eps) ? 1 : 0;
        } else {
            if (p.N <= D)
                cert = 1;                                             // every gallery row is a candidate
            else if (n_valid == D)
                cert = ((double)e_k - fabs((double)e_k) * 0x1p-23 > (double)t + (double)eps) ? 1 : 0;
        }
    }
    if (lane == 0) p.certified[qi] = (uint8_t)cert;
}

// the whole entry point but its name: ``fn`` goes in front of every message
template <bool FILTERED>
int search_rerank(const char* fn, const float* q, int64_t ldq, const float* q_scale, const float* rows, int64_t ldr, const float* g_scale,
                  const int32_t* cand_idx, const float* cand_vals, const float* eps, int32_t nQ, int32_t N, int32_t E, int32_t D, int32_t k,
                  float* vals, int32_t* idx, uint8_t* certified, void* stream) {
    SC_CHECK(nQ >= 0 && N >= 0 && E >= 1 && ldq >= E && ldr >= E, "%s: bad shape (nQ %d, N %d, E %d, ldq %lld, ldr %lld)", fn, nQ, N, E,
             (long long)ldq, (long long)ldr);
    SC_CHECK(D >= 1 && D <= SEARCH_MAXK && k >= 1 && k <= D, "%s: 1 <= k <= D <= 32 (k %d, D %d)", fn, k, D);
    if (nQ == 0) return 0;
    SC_CHECK(q && cand_idx && cand_vals && eps && vals && idx && certified && (N == 0 || rows), "%s: null pointer", fn);
    RerankArgs a;
    a.q = q; a.q_scale = q_scale; a.rows = rows; a.g_scale = g_scale;
    a.cand_idx = cand_idx; a.cand_vals = cand_vals; a.eps = eps;
    a.ldq = ldq; a.ldr = ldr;
    a.N = N; a.E = E; a.D = D; a.k = k;
    a.vals = vals; a.idx = idx; a.certified = certified;
    hipLaunchKernelGGL(search_rerank_kernel<FILTERED>, dim3((unsigned)nQ), dim3(256), 0, (hipStream_t)stream, a);
    SC_LAUNCH_CHECK();
    return 0;
}

}  // namespace
