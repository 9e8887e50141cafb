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
//   sc_search_topk_filtered_bf16  search.hip's kernel written again (same operands, K loop, tile, XCD remap, list words
//                                 key << 32 | ~column, slabs of whole column tiles).  After a tile's K loop a lane loads the id and
//                                 the live byte of its two columns (lane, lane + 64; nothing at or past N is read); a wave keeps
//                                 the ids of its 32 query rows one per lane and reads the row's id into a scalar register, so the
//                                 admissibility test is part of the ballot predicate in front of the k-th-key test: an
//                                 inadmissible column never pays for an insertion.  With a filter ANY slab can hold fewer than k
//                                 admissible columns, so the per-slab lists leave as the 64-bit words themselves (0 = no entry).
//   sc_search_merge_u64           one wave per query: the k largest of its S k words, decoded.  Words of distinct columns are
//                                 distinct, so the order is total; a real -inf has key 0x007fffff > 0 and sorts above a filler
//                                 wherever its slab is.
//   sc_topk_rows_filtered_f32     topk.hip's kernel written again over a score matrix: a column is tested for admissibility only
//                                 once its key would enter the lane's list, so the ids are read for candidates, not for every
//                                 score.  The score matrix is not modified.
// No atomics, nothing allocated, fixed-order reductions: same input, same bits, for every S.
#include "sc_common.h"

#include <algorithm>

namespace {

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

// 64-lane maximum of a 64-bit word, the same value in every lane
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t best) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o);
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, o);
        const uint64_t q = ((uint64_t)hi << 32) | lo;
        best = q > best ? q : best;
    }
    return best;
}

// ====================================================================================================== fused kernel
constexpr int BM = 128, BN = 128, BK = 64;
constexpr int ROWB = BK * 2;                        // bytes per LDS tile row
constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB;
constexpr int RING_BYTES = 2 * (A_BYTES + B_BYTES);
static_assert(RING_BYTES == BM * BN * 4, "the fp32 score tile lies exactly over the two-stage ring");
constexpr int TM = 64, TN = 64, FM = 4, FN = 4;     // per-wave tile, 16 x 16 fragments

__device__ __forceinline__ void glds16(const void* g, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// lane i <- lane i - 1 over the whole wave (DPP wave_shr:1); lane 0 gets 0 and is handled by the caller
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);
}

struct FilterSearchArgs {
    const uint16_t* q;       // [roundup(nQ, 128), K6] side-0 split
    const uint16_t* g;       // [roundup(N, 128), K6] side-1 split
    int nQ, N, K6, k, S, tiles;
    const int64_t* q_ids;    // [nQ] or NULL (with g_ids)
    const int64_t* g_ids;    // [N] or NULL
    const uint8_t* live;     // [N] or NULL
    uint64_t* part;          // [nQ, S, k] list words, best first; 0 = no entry
};

__global__ __launch_bounds__(256) void search_topk_filtered_kernel(const FilterSearchArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int k = p.k;
    const bool has_ids = p.g_ids != nullptr;

    // ---- block -> (row tile, slab): XCD remap (bijective; blocks b, b + 8, ... share an L2), then row tiles fastest
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
    uint64_t* const lists = (uint64_t*)(smem + RING_BYTES);           // [BM][k], best first; 0 = no entry

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

    // ---- this slab's list of every row, as words: any slab may hold fewer than k entries, so the merge must see which are real
    const int rows_here = min(32, p.nQ - m0 - wave * 32);
    if (lane < k) {
        for (int rr = 0; rr < rows_here; ++rr) {
            const int r = wave * 32 + rr;
            p.part[((int64_t)(m0 + r) * p.S + slab) * k + lane] = lists[r * k + lane];
        }
    }
}

inline int lds_bytes(int k) { return RING_BYTES + BM * k * 8; }

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
        vals[o] = tk_value((uint32_t)(out >> 32));           // no entry: -inf
        idx[o] = (int32_t)~(uint32_t)out;                    // no entry: ~0 = -1
    }
}

// ====================================================================================================== row selection
struct RowFilter {
    const int64_t* g_ids;    // [V] or NULL
    const uint8_t* live;     // [V] or NULL
    int64_t qid;             // this row's id (g_ids != NULL)

    __device__ __forceinline__ bool admissible(int col) const {
        bool ok = true;
        if (live) ok = live[col] != 0;
        if (g_ids) ok = ok && g_ids[col] != qid;
        return ok;
    }
};

// the float a group is tested against: the value of the lane's fourth-best key, NaN when the list is not full or its tail is a NaN
// (every group then takes the exact path)
__device__ __forceinline__ float tk_threshold(uint32_t k) {
    if (k == TK_EMPTY || k == TK_NAN) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

struct Top4 {
    uint32_t k0, k1, k2, k3;     // keys, best first; TK_EMPTY = no entry
    int c0, c1, c2, c3;
    float thr;

    __device__ __forceinline__ void clear() {
        k0 = k1 = k2 = k3 = TK_EMPTY;
        c0 = c1 = c2 = c3 = -1;
        thr = tk_threshold(TK_EMPTY);
    }
    // strict: an equal key stays behind the entries already listed (they have lower columns)
    __device__ __forceinline__ void insert(uint32_t key, int col) {
        const bool g0 = key > k0, g1 = key > k1, g2 = key > k2, g3 = key > k3;
        k3 = g2 ? k2 : (g3 ? key : k3);  c3 = g2 ? c2 : (g3 ? col : c3);
        k2 = g1 ? k1 : (g2 ? key : k2);  c2 = g1 ? c1 : (g2 ? col : c2);
        k1 = g0 ? k0 : (g1 ? key : k1);  c1 = g0 ? c0 : (g1 ? col : c1);
        k0 = g0 ? key : k0;              c0 = g0 ? col : c0;
    }
    __device__ __forceinline__ void pop() {
        k0 = k1; k1 = k2; k2 = k3; k3 = TK_EMPTY;
        c0 = c1; c1 = c2; c2 = c3; c3 = -1;
        thr = tk_threshold(TK_EMPTY);
    }
};

// columns of group g of a lane, in increasing order: VEC - the 16-byte word lane + 64 g; else four elements 64 columns apart
template <bool VEC>
__device__ __forceinline__ int tk_col(int lane, int g, int j) {
    return VEC ? 4 * (lane + 64 * g) + j : lane + 64 * (4 * g + j);
}

template <bool VEC>
__device__ __forceinline__ void tk_load(const float* __restrict__ row, int lane, int g, float (&a)[4]) {
    if (VEC) {
        const f32x4 v = *(const f32x4*)(row + tk_col<true>(lane, g, 0));
        a[0] = v[0]; a[1] = v[1]; a[2] = v[2]; a[3] = v[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = row[tk_col<false>(lane, g, j)];
    }
}

// one group of four columns into the list.  REFILL: only pairs that rank after (lk, lc), counted in ``seen``.  A column's id and
// live byte are read only when its key would enter the list (or, REFILL, ranks after the last popped pair): always a column < V
template <bool VEC, bool REFILL>
__device__ __forceinline__ void tk_group(Top4& t, const RowFilter& f, const float (&a)[4], int lane, int g, int nvalid, uint32_t lk, int lc,
                                         int& seen) {
    if (!REFILL && nvalid == 4 && a[0] <= t.thr && a[1] <= t.thr && a[2] <= t.thr && a[3] <= t.thr) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t key = tk_key(a[j]);
        const int col = tk_col<VEC>(lane, g, j);
        bool take = j < nvalid;
        if (REFILL)
            take = take && (key < lk || (key == lk && col > lc));
        else
            take = take && key > t.k3;                       // anything else would leave the list as it is
        if (take) take = f.admissible(col);
        if (REFILL) seen += take ? 1 : 0;
        if (take) t.insert(key, col);
    }
    t.thr = tk_threshold(t.k3);
}

// all columns of this lane, in increasing order, four groups of loads in flight
template <bool VEC, bool REFILL>
__device__ __forceinline__ void tk_scan(Top4& t, const RowFilter& f, const float* __restrict__ row, int V, int lane, uint32_t lk, int lc,
                                        int& seen) {
    int g = 0;
    for (; tk_col<VEC>(lane, g + 3, 3) < V; g += 4) {
        float a0[4], a1[4], a2[4], a3[4];
        tk_load<VEC>(row, lane, g, a0);
        tk_load<VEC>(row, lane, g + 1, a1);
        tk_load<VEC>(row, lane, g + 2, a2);
        tk_load<VEC>(row, lane, g + 3, a3);
        tk_group<VEC, REFILL>(t, f, a0, lane, g, 4, lk, lc, seen);
        tk_group<VEC, REFILL>(t, f, a1, lane, g + 1, 4, lk, lc, seen);
        tk_group<VEC, REFILL>(t, f, a2, lane, g + 2, 4, lk, lc, seen);
        tk_group<VEC, REFILL>(t, f, a3, lane, g + 3, 4, lk, lc, seen);
    }
    for (; tk_col<VEC>(lane, g, 0) < V; ++g) {
        float a[4];
        int nvalid = 4;
        if (tk_col<VEC>(lane, g, 3) < V) {
            tk_load<VEC>(row, lane, g, a);
        } else {           // the row's last columns: element loads, nothing at or past V is touched
            nvalid = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = tk_col<VEC>(lane, g, j);
                const bool ok = c < V;
                a[j] = ok ? row[c] : 0.f;
                nvalid += ok ? 1 : 0;      // columns increase with j: the valid ones are the first nvalid
            }
        }
        tk_group<VEC, REFILL>(t, f, a, lane, g, nvalid, lk, lc, seen);
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
    const float* __restrict__ row = scores + (int64_t)r * ld;
    RowFilter f;
    f.g_ids = g_ids;
    f.live = live;
    f.qid = g_ids ? q_ids[r] : 0;
    Top4 t;
    t.clear();
    int seen = 0;
    tk_scan<VEC, false>(t, f, row, V, lane, 0u, 0, seen);
    // columns this lane owns (admissible or not): more than the list holds -> an empty list is not the end of the lane
    const int owned = VEC ? ((V + 3) / 4 > lane ? 4 * (((V + 3) / 4 - lane + 63) / 64) : 0) : (V > lane ? (V - lane + 63) / 64 : 0);
    bool more = owned > 4;
    int out_c = -1;
    for (int p = 0; p < k; ++p) {
        const uint64_t mine = t.k0 == TK_EMPTY ? 0ull : ((uint64_t)t.k0 << 32) | (uint32_t)~(uint32_t)t.c0;
        const uint64_t best = wave_max_u64(mine);
        if (best == 0ull) break;                             // fewer than k admissible columns: wave-uniform
        if (lane == p) out_c = (int)~(uint32_t)best;
        if (mine == best) {                                  // columns are unique: exactly one lane
            const uint32_t lk = t.k0;
            const int lc = t.c0;
            t.pop();
            if (t.k0 == TK_EMPTY && more) {
                int cnt = 0;
                tk_scan<VEC, true>(t, f, row, V, lane, lk, lc, cnt);
                more = cnt > 4;
            }
        }
    }
    if (lane < k) {
        const int64_t o = (int64_t)r * k + lane;
        vals[o] = out_c >= 0 ? row[out_c] : -INFINITY;       // the matrix's own bits; a real -inf keeps its column
        idx[o] = out_c;
    }
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
    static sc_lds_attr_once attr;
    if (hipError_t e = sc_set_max_lds_once(attr, search_topk_filtered_kernel, lds_bytes(32)); e != hipSuccess) {
        sc_set_error("hipFuncSetAttribute(search_filter): %s", hipGetErrorString(e));
        return -3;
    }
    FilterSearchArgs a;
    a.q = (const uint16_t*)q_split;
    a.g = (const uint16_t*)g_split;
    a.nQ = nQ; a.N = N; a.K6 = K6; a.k = k; a.S = S; a.tiles = (int)tiles;
    const bool ids = q_ids && g_ids;
    a.q_ids = ids ? q_ids : nullptr;
    a.g_ids = ids ? g_ids : nullptr;
    a.live = N > 0 ? live : nullptr;
    a.part = part;
    hipLaunchKernelGGL(search_topk_filtered_kernel, dim3((unsigned)(nM * S)), dim3(256), lds_bytes(k), (hipStream_t)stream, a);
    SC_LAUNCH_CHECK();
    return 0;
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
