// Gallery search (gfx950): for every query the k best gallery rows, with the selection fused into the score GEMM's epilogue - the
// [nQ, N] score matrix never exists in memory.
//   replaces: torch.argsort(score, descending=True) of the whole score matrix (avssl/module/retrieval.py:45-46) on the scores of
//             avssl/model/kwClip.py:447-482, where only the first max(recall_at) entries of a row are ever looked at.
//
// Scores: the arithmetic of ops.cosine_scores_split.  Both operands are the three-way bf16 splits sc_split3_bf16 writes (queries
// side 0, gallery side 1, rows padded to 128, K6 = 6 Ep columns); a score is the fp32 sum of the six K-blocks on
// v_mfma_f32_16x16x32_bf16, K-tiles in increasing order.  The K loop is the one of gemm_bf16.hip's 128 x 128 tile written again: 256
// threads = 2 x 2 waves, LDS-DMA staging into two buffers, 16-byte chunk index XOR ((row >> 1) & 7) applied on the global source
// address, one barrier per K-tile.
//
// Grid: row tiles of 128 queries x S column slabs of the gallery; a slab is ``tiles`` whole column tiles of 128 gallery rows and a
// workgroup walks them in increasing column order.  After a tile's K loop the accumulators go to the LDS tile (over the staging ring,
// as the GEMM's epilogue does) and the waves scan it: a wave owns 32 rows, a lane reads columns lane and lane + 64 of a row (conflict
// free), maps them to the sortable key of csrc/topk.hip and tests them against the key of the row's current k-th entry; only a row
// with a passing column pays for insertions, and a candidate overtaken by an earlier insertion of the same pass is dropped on one
// scalar compare.  A row's list is k sorted 64-bit words (key << 32 | ~column) in LDS: the wave loads it
// one entry per lane and inserts a candidate with one wave shift (every lane keeps its entry, takes the candidate, or takes its lower
// neighbour's entry) - no runtime-indexed register array.  (key, ~column) is a total order over distinct columns, so equal scores
// keep the lower column in front whatever order they arrive in.  Columns >= N are excluded by their index: the zero padding rows of
// the split operand score 0, and NaN against a NaN query.
//
// Order contract = csrc/topk.hip's: larger value first, lower gallery index first among equal values (-0 == +0), NaN above every
// number, lower index first among NaNs, fewer than k columns: the tail is -inf / -1.  The value written is the key mapped back:
// a zero comes back as +0 and every NaN as the default NaN.
//
// Every (row tile, slab) writes its k candidates to part_vals / part_idx [nQ, S, k]; the caller merges the S lists of a row with
// sc_topk_rows_f32 over [nQ, S k] (position order = lower slab first = lower columns first, and only the last slab's list can end in
// -inf / -1 fillers because every other slab holds 128 >= k valid columns per tile) and one gather of the indices.  S = 1: the lists
// are the result.  No atomics; a score's arithmetic does not depend on S, so neither does the result.
#include "sc_common.h"

#include <algorithm>

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int ROWB = BK * 2;                        // bytes per LDS tile row
constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB;
constexpr int RING_BYTES = 2 * (A_BYTES + B_BYTES);
static_assert(RING_BYTES == BM * BN * 4, "the fp32 score tile lies exactly over the two-stage ring");
constexpr int TM = 64, TN = 64, FM = 4, FN = 4;     // per-wave tile, 16 x 16 fragments

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

// lane i <- lane i - 1 over the whole wave (DPP wave_shr:1, an ALU move: no LDS round trip); lane 0 gets 0 and is handled by the caller
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);
}

struct SearchArgs {
    const uint16_t* q;       // [roundup(nQ, 128), K6] side-0 split
    const uint16_t* g;       // [roundup(N, 128), K6] side-1 split
    int nQ, N, K6, k, S, tiles;
    float* part_vals;        // [nQ, S, k]
    int32_t* part_idx;
};

__global__ __launch_bounds__(256) void search_topk_kernel(const SearchArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int k = p.k;

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
    const int t_begin = slab * p.tiles, t_end = min(nT, t_begin + p.tiles);

    char* const As = smem;
    char* const Bs = smem + 2 * A_BYTES;
    float* const Cs = (float*)smem;
    uint64_t* const lists = (uint64_t*)(smem + RING_BYTES);           // [BM][k], best first; 0 = no entry (-inf / -1)

    // a wave owns the lists of its 32 rows: no other wave touches them, so no barrier orders these stores
    for (int i = lane; i < 32 * k; i += 64) lists[wave * 32 * k + i] = 0ull;

    // ---- DMA source pointers of the query tile (per lane; the swizzle lives in the source address) ----------------------
    constexpr int A_INST = BM / 32, B_INST = BN / 32;
    const uint16_t* a_src[A_INST];
#pragma unroll
    for (int i = 0; i < A_INST; ++i) {
        const int row = (i * 4 + wave) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        a_src[i] = p.q + (int64_t)(m0 + row) * p.K6 + c * 8;          // rows are padded to 128: in bounds
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
    const int nk = p.K6 / BK;

    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = t * BN;
        const uint16_t* b_src[B_INST];
#pragma unroll
        for (int i = 0; i < B_INST; ++i) {
            const int row = (i * 4 + wave) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            b_src[i] = p.g + (int64_t)(n0 + row) * p.K6 + c * 8;      // gallery rows are padded to 128: in bounds
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
        const bool ok0 = n0 + lane < p.N, ok1 = n0 + 64 + lane < p.N;
        const int rows_here = min(32, p.nQ - m0 - wave * 32);         // wave-uniform; <= 0: nothing to scan
        for (int rr = 0; rr < rows_here; ++rr) {
            const int r = wave * 32 + rr;
            const uint32_t key0 = tk_key(Cs[r * BN + lane]), key1 = tk_key(Cs[r * BN + 64 + lane]);
            const uint32_t kth = (uint32_t)(lists[r * k + k - 1] >> 32);
            // strict: a score equal to the k-th entry's has a higher column than it and stays out
            uint64_t m_lo = __ballot(ok0 && key0 > kth), m_hi = __ballot(ok1 && key1 > kth);
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

    // ---- this slab's k candidates of every row -------------------------------------------------------------------------------
    const int rows_here = min(32, p.nQ - m0 - wave * 32);
    if (lane < k) {
        for (int rr = 0; rr < rows_here; ++rr) {
            const int r = wave * 32 + rr;
            const uint64_t e = lists[r * k + lane];
            const int64_t o = ((int64_t)(m0 + r) * p.S + slab) * k + lane;
            p.part_vals[o] = tk_value((uint32_t)(e >> 32));
            p.part_idx[o] = (int32_t)~(uint32_t)e;                    // no entry: ~0 = -1
        }
    }
}

inline int lds_bytes(int k) { return RING_BYTES + BM * k * 8; }

}  // namespace

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
    static sc_lds_attr_once attr;
    if (hipError_t e = sc_set_max_lds_once(attr, search_topk_kernel, lds_bytes(32)); e != hipSuccess) {
        sc_set_error("hipFuncSetAttribute(search): %s", hipGetErrorString(e));
        return -3;
    }
    SearchArgs a;
    a.q = (const uint16_t*)q_split;
    a.g = (const uint16_t*)g_split;
    a.nQ = nQ; a.N = N; a.K6 = K6; a.k = k; a.S = S; a.tiles = (int)tiles;
    a.part_vals = part_vals;
    a.part_idx = part_idx;
    hipLaunchKernelGGL(search_topk_kernel, dim3((unsigned)(nM * S)), dim3(256), lds_bytes(k), (hipStream_t)stream, a);
    SC_LAUNCH_CHECK();
    return 0;
}
