// Filtered compact gallery search (gfx950): search_compact.hip's coarse top-D scan and exact re-rank over the ADMISSIBLE gallery rows
// only, with the certificate restated over them.
//   replaces: score.masked_fill(mask, -inf) + torch.argsort over the whole [nQ, N] score matrix (avssl/module/retrieval.py:45-46 on
//             the scores of avssl/model/kwClip.py:447-482) when a query's own item, its sibling captions or removed gallery rows must
//             stay out of the ranking - on the 2 Ep bytes per gallery row of the compact index.
//
// Rule (include/speechclip_hip.h states it once for every layer): gallery row j is admissible for query i iff j < N, live is NULL or
// live[j] != 0, and the ids are NULL or g_ids[j] != q_ids[i] (int64, all 64 bits).
//
//   sc_search_coarse_filtered_bf16  sc_search_coarse_bf16's kernel written again (same operands, K loop, tile, XCD remap, arithmetic and
//                                   K-tile order: an admissible row carries the same fp32 bits).  After a tile's K loop a lane loads
//                                   the id and the live byte of its two columns (lane, lane + 64; nothing at or past N is read); a
//                                   wave keeps the ids of its 32 query rows one per lane and reads the row's id with v_readlane, so
//                                   the admissibility test is part of the ballot predicate in front of the D-th-key test and no LDS
//                                   is spent on ids (at D = 32 the ring and the lists already take 98 304 B).  With a filter ANY
//                                   slab can hold fewer than D admissible columns, so the per-slab lists leave as the 64-bit words
//                                   of the LDS lists themselves (key << 32 | ~column, 0 = no entry): sc_search_merge_u64 merges and
//                                   decodes them.
//   sc_search_rerank_filtered_f32   sc_search_rerank_f32 with the certificate over the admissible rows: the candidates are a query's D
//                                   best ADMISSIBLE rows, so "fewer than D candidates" means every admissible row is one - that
//                                   clause stands where the unfiltered kernel has N <= D.
// No atomics, nothing allocated, fixed-order reductions: same input, same bits, for every S.
#include "sc_common.h"

#include <algorithm>

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int ROWB = BK * 2;                        // bytes per LDS tile row
constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB;
constexpr int RING_BYTES = 2 * (A_BYTES + B_BYTES);
static_assert(RING_BYTES == BM * BN * 4, "the fp32 score tile lies exactly over the two-stage ring");
constexpr int TM = 64, TN = 64, FM = 4, FN = 4;     // per-wave tile, 16 x 16 fragments
constexpr int MAXD = 32;

constexpr uint32_t TK_EMPTY = 0u;            // below every real key (-inf maps to 0x007fffff)
constexpr uint32_t TK_NAN = 0xffffffffu;     // above +inf (0xff800000)

// fp32 -> uint32 with the order of the contract (the mapping of csrc/topk.hip): a < b as floats <=> key(a) < key(b); -0 and +0
// share a key; every NaN is TK_NAN
__device__ __forceinline__ uint32_t tk_key(float v) {
    const uint32_t u = __float_as_uint(v);
    uint32_t k = u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
    if ((u & 0x7fffffffu) > 0x7f800000u) k = TK_NAN;
    if (k == 0x7fffffffu) k = 0x80000000u;
    return k;
}
__device__ __forceinline__ float tk_value(uint32_t k) {
    if (k == TK_EMPTY) return -INFINITY;
    if (k == TK_NAN) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ void glds16(const void* g, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// lane i <- lane i - 1 over the whole wave (DPP wave_shr:1); lane 0 gets 0 and is handled by the caller
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);
}

// ------------------------------------------------------------------------------------------ coarse fused top-D, filtered
struct CoarseFilterArgs {
    const uint16_t* q;       // [roundup(nQ, 128), Ep] bf16
    const uint16_t* g;       // [roundup(N, 128), Ep] bf16
    int nQ, N, Ep, D, S, tiles;
    const int64_t* q_ids;    // [nQ] or NULL (with g_ids)
    const int64_t* g_ids;    // [N] or NULL
    const uint8_t* live;     // [N] or NULL
    uint64_t* part;          // [nQ, S, D] list words, best first; 0 = no entry
};

__global__ __launch_bounds__(256) void search_coarse_filtered_kernel(const CoarseFilterArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int k = p.D;
    const bool has_ids = p.g_ids != nullptr;

    // ---- block -> (row tile, slab): XCD remap (bijective; blocks b, b + 8, ... share an L2), then row tiles fastest, so the
    // workgroups of a slab walk the same gallery tiles side by side
    const int nM = (p.nQ + BM - 1) / BM;
    const int nT = (p.N + BN - 1) / BN;
    int L;
    {
        const int nwg = gridDim.x, bid = blockIdx.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    const int slab = L / nM, m_tile = L - slab * nM;
    const int m0 = m_tile * BM;
    const int t_begin = min(nT, slab * p.tiles), t_end = min(nT, t_begin + p.tiles);   // a slab past the last tile is empty

    char* const As = smem;
    char* const Bs = smem + 2 * A_BYTES;
    float* const Cs = (float*)smem;
    uint64_t* const lists = (uint64_t*)(smem + RING_BYTES);           // [BM][D], best first; 0 = no entry

    // a wave owns the lists of its 32 rows: no other wave touches them, so no barrier orders these stores
    for (int i = lane; i < 32 * k; i += 64) lists[wave * 32 * k + i] = 0ull;

    // the ids of this wave's 32 query rows, row rr in lane rr: read back per row into scalar registers (no LDS beside the lists)
    uint32_t qid_lo = 0u, qid_hi = 0u;
    if (has_ids && lane < 32 && m0 + wave * 32 + lane < p.nQ) {
        const uint64_t v = (uint64_t)p.q_ids[m0 + wave * 32 + lane];
        qid_lo = (uint32_t)v;
        qid_hi = (uint32_t)(v >> 32);
    }

    // ---- DMA source pointers of the query tile (per lane; the swizzle lives in the source address) ----------------------
    constexpr int A_INST = BM / 32, B_INST = BN / 32;
    const uint16_t* a_src[A_INST];
#pragma unroll
    for (int i = 0; i < A_INST; ++i) {
        const int row = (i * 4 + wave) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        a_src[i] = p.q + (int64_t)(m0 + row) * p.Ep + c * 8;          // rows are padded to 128: in bounds
    }
    int a_off[FM][2], b_off[FN][2];
#pragma unroll
    for (int mi = 0; mi < FM; ++mi) {
        const int row = wm * TM + mi * 16 + (lane & 15);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) a_off[mi][kk] = row * ROWB + (((kk * 4 + (lane >> 4)) ^ ((row >> 1) & 7)) << 4);
    }
#pragma unroll
    for (int ni = 0; ni < FN; ++ni) {
        const int row = wn * TN + ni * 16 + (lane & 15);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) b_off[ni][kk] = row * ROWB + (((kk * 4 + (lane >> 4)) ^ ((row >> 1) & 7)) << 4);
    }
    const int nk = p.Ep / BK;

    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = t * BN;
        const uint16_t* b_src[B_INST];
#pragma unroll
        for (int i = 0; i < B_INST; ++i) {
            const int row = (i * 4 + wave) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            b_src[i] = p.g + (int64_t)(n0 + row) * p.Ep + c * 8;      // gallery rows are padded to 128: in bounds
        }
        auto stage = [&](int buf, int kt) {
#pragma unroll
            for (int i = 0; i < A_INST; ++i) glds16(a_src[i] + kt * BK, As + buf * A_BYTES + (i * 4 + wave) * 1024);
#pragma unroll
            for (int i = 0; i < B_INST; ++i) glds16(b_src[i] + kt * BK, Bs + buf * B_BYTES + (i * 4 + wave) * 1024);
        };
        f32x4 acc[FM][FN];
#pragma unroll
        for (int mi = 0; mi < FM; ++mi)
#pragma unroll
            for (int ni = 0; ni < FN; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

        stage(0, 0);
        __syncthreads();   // hipcc drains the DMA (vmcnt(0)) in front of the barrier
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) stage(buf ^ 1, kt + 1);
            const char* as = As + buf * A_BYTES;
            const char* bs = Bs + buf * B_BYTES;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8 af[FM], bfr[FN];
#pragma unroll
                for (int mi = 0; mi < FM; ++mi) af[mi] = *(const bf16x8*)(as + a_off[mi][kk]);
#pragma unroll
                for (int ni = 0; ni < FN; ++ni) bfr[ni] = *(const bf16x8*)(bs + b_off[ni][kk]);
#pragma unroll
                for (int mi = 0; mi < FM; ++mi)
#pragma unroll
                    for (int ni = 0; ni < FN; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
            }
            __syncthreads();
        }

        // ---- this lane's two columns of the tile: in range, live, and their ids (no DMA is in flight here; the loads complete
        // under the score stores and the barrier below).  g_ids / live are [N], not padded: nothing at or past N is read
        const int c0 = n0 + lane, c1 = n0 + 64 + lane;
        bool ok0 = c0 < p.N, ok1 = c1 < p.N;
        uint64_t gid0 = 0ull, gid1 = 0ull;
        if (has_ids) {
            if (ok0) gid0 = (uint64_t)p.g_ids[c0];
            if (ok1) gid1 = (uint64_t)p.g_ids[c1];
        }
        if (p.live) {
            if (ok0) ok0 = p.live[c0] != 0;
            if (ok1) ok1 = p.live[c1] != 0;
        }

        // ---- scores -> LDS tile (every wave is past the ring: the K loop ends in a barrier) ------------------------------
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
            const int nl = wn * TN + ni * 16 + (lane & 15);
#pragma unroll
            for (int mi = 0; mi < FM; ++mi) {
                const int ml = wm * TM + mi * 16 + 4 * (lane >> 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) Cs[(ml + r) * BN + nl] = acc[mi][ni][r];
            }
        }
        __syncthreads();

        // ---- selection: wave w scans rows 32 w .. 32 w + 31 of the tile ----------------------------------------------------
        const int rows_here = min(32, p.nQ - m0 - wave * 32);         // wave-uniform; <= 0: nothing to scan
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
            const uint32_t kth = (uint32_t)(lists[r * k + k - 1] >> 32);
            // admissible first, then strict: a score equal to the D-th entry's has a higher column than it and stays out
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
                    const uint64_t c = ((uint64_t)ck << 32) | (uint32_t)~(uint32_t)(n0 + h * 64 + j);
                    const uint64_t up = ((uint64_t)wave_shr1((uint32_t)(e >> 32)) << 32) | wave_shr1((uint32_t)e);
                    // entries above the candidate stay; the first one below takes it; the rest move down one place
                    e = e > c ? e : ((lane == 0 || up > c) ? c : up);
                    kth_now = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(e >> 32), k - 1);
                }
            }
            if (lane < k) lists[r * k + lane] = e;
        }
        __syncthreads();   // the next tile's DMA overwrites the score tile
    }

    // ---- this slab's list of every row, as words: any slab may hold fewer than D entries, so the merge must see which are real
    const int rows_here = min(32, p.nQ - m0 - wave * 32);
    if (lane < k) {
        for (int rr = 0; rr < rows_here; ++rr) {
            const int r = wave * 32 + rr;
            p.part[((int64_t)(m0 + r) * p.S + slab) * k + lane] = lists[r * k + lane];
        }
    }
}

inline int lds_bytes(int D) { return RING_BYTES + BM * D * 8; }

// ------------------------------------------------------------------------------------------ exact re-rank + certificate
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

__global__ __launch_bounds__(256) void search_rerank_filtered_kernel(const RerankArgs p) {
    __shared__ float ex[MAXD];
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
    // ---- the certificate over the admissible rows, in fp64 ---------------------------------------------------------------------
    const float eps = p.eps[qi];
    const bool finite_all = __ballot(valid && !(isfinite(e) && isfinite(cv))) == 0ull && isfinite(eps);
    const int n_valid = __popcll(__ballot(valid));
    const uint64_t at_k = __ballot(have && rank == k - 1);            // exactly one lane: the ranks are a permutation of 0 .. D - 1
    const float e_k = __shfl(e, __builtin_ctzll(at_k | (1ull << 63)));
    const float t = p.cand_vals[qi * D + D - 1];
    int cert = 0;
    if (finite_all) {
        if (n_valid < D)
            cert = 1;                                                 // every admissible row is a candidate (none at all included)
        else
            cert = ((double)e_k - fabs((double)e_k) * 0x1p-23 > (double)t + (double)eps) ? 1 : 0;
    }
    if (lane == 0) p.certified[qi] = (uint8_t)cert;
}

}  // namespace

extern "C" int sc_search_coarse_filtered_bf16(const sc_bf16* q_bf16, const sc_bf16* g_bf16, int32_t nQ, int32_t N, int32_t Ep, int32_t D,
                                              int32_t S, const int64_t* q_ids, const int64_t* g_ids, const uint8_t* live, uint64_t* part,
                                              void* stream) {
    SC_CHECK(nQ >= 0 && N >= 0, "sc_search_coarse_filtered_bf16: nQ >= 0, N >= 0 (nQ %d, N %d)", nQ, N);
    SC_CHECK(D >= 1 && D <= MAXD, "sc_search_coarse_filtered_bf16: 1 <= D <= 32 (D %d)", D);
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
    static sc_lds_attr_once attr;
    if (hipError_t e = sc_set_max_lds_once(attr, search_coarse_filtered_kernel, lds_bytes(MAXD)); e != hipSuccess) {
        sc_set_error("hipFuncSetAttribute(search_coarse_filtered): %s", hipGetErrorString(e));
        return -3;
    }
    CoarseFilterArgs a;
    a.q = (const uint16_t*)q_bf16;
    a.g = (const uint16_t*)g_bf16;
    a.nQ = nQ; a.N = N; a.Ep = Ep; a.D = D; a.S = S; a.tiles = (int)tiles;
    const bool ids = q_ids && g_ids;
    a.q_ids = ids ? q_ids : nullptr;
    a.g_ids = ids ? g_ids : nullptr;
    a.live = N > 0 ? live : nullptr;
    a.part = part;
    hipLaunchKernelGGL(search_coarse_filtered_kernel, dim3((unsigned)(nM * S)), dim3(256), lds_bytes(D), (hipStream_t)stream, a);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_search_rerank_filtered_f32(const float* q, int64_t ldq, const float* q_scale, const float* rows, int64_t ldr,
                                             const float* g_scale, const int32_t* cand_idx, const float* cand_vals, const float* eps,
                                             int32_t nQ, int32_t N, int32_t E, int32_t D, int32_t k, float* vals, int32_t* idx,
                                             uint8_t* certified, void* stream) {
    SC_CHECK(nQ >= 0 && N >= 0 && E >= 1 && ldq >= E && ldr >= E,
             "sc_search_rerank_filtered_f32: bad shape (nQ %d, N %d, E %d, ldq %lld, ldr %lld)", nQ, N, E, (long long)ldq, (long long)ldr);
    SC_CHECK(D >= 1 && D <= MAXD && k >= 1 && k <= D, "sc_search_rerank_filtered_f32: 1 <= k <= D <= 32 (k %d, D %d)", k, D);
    if (nQ == 0) return 0;
    SC_CHECK(q && cand_idx && cand_vals && eps && vals && idx && certified && (N == 0 || rows), "sc_search_rerank_filtered_f32: null pointer");
    RerankArgs a;
    a.q = q; a.q_scale = q_scale; a.rows = rows; a.g_scale = g_scale;
    a.cand_idx = cand_idx; a.cand_vals = cand_vals; a.eps = eps;
    a.ldq = ldq; a.ldr = ldr;
    a.N = N; a.E = E; a.D = D; a.k = k;
    a.vals = vals; a.idx = idx; a.certified = certified;
    hipLaunchKernelGGL(search_rerank_filtered_kernel, dim3((unsigned)nQ), dim3(256), 0, (hipStream_t)stream, a);
    SC_LAUNCH_CHECK();
    return 0;
}
