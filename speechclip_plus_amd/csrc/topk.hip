// Per-row top-K over an fp32 score matrix (gfx950): the selection behind keyword detokenisation (keyword_neighbors.py) - for every
// keyword embedding the K nearest rows of the CLIP token table.  The scores come from the quantiser's own score path
// (sc_split3_bf16 + sc_gemm_bf16); this file only selects.
//   sc_topk_rows_f32         scores [rows, ld] fp32, V valid columns -> vals [rows, k] fp32, idx [rows, k] int32, best first
//   sc_topk_rescore_cos_f32  vals[row, r] = cos(kw[row], table[idx[row, r]]) with fp64 accumulation: the score matrix is accumulated in
//                            fp32 over 6 E products (a few 1e-6 low at a score of 1, measured); what is REPORTED next to a token is exact
//
// The output is discrete, so the order is a contract: larger value first, among equal values the lower column first (a stable
// descending sort; -0 == +0), NaN above every number (torch.topk's rank), lower column first among NaNs.  V < k: the tail is
// -inf / -1.  No atomics, no LDS, fixed-order reductions: same input, same bits.
//
// One wave per row (four rows per 256-thread workgroup, no barrier).  A lane owns every 64th group of four columns - a 16-byte load
// when the row base is 16-byte aligned and the pitch a multiple of four floats, four element loads 64 columns apart otherwise - and
// walks them in increasing column order.  It keeps its four best as (sortable key, column) in NAMED registers (a runtime-indexed
// register array would go to scratch), inserted by an unrolled strict compare-exchange: strict + increasing columns = the lower
// column stays in front among equal values.  A group is first tested against the lane's fourth-best as FLOATS (!(v <= t): one
// compare per element; NaN and an unfilled list fail it on purpose) and only a group with a candidate pays for keys and insertion.
// The wave then pops the global best k times: a 64-lane max over (key << 32 | ~column).  Four per lane is not a bound on the
// answer: a lane whose list runs empty while it still owns unlisted columns re-scans ITS columns for the next four that rank after
// its last popped pair before the next pop (rare on continuous scores - k of 64 lanes' best - and exact on tie-heavy rows).
// Every score is read once (re-scans aside) -> bandwidth-bound; the k values are re-read at the end so the caller gets the
// matrix's own bits (-0, NaN payloads).
#include "sc_common.h"

namespace {

constexpr uint32_t TK_EMPTY = 0u;            // below every real key (-inf maps to 0x007fffff)
constexpr uint32_t TK_NAN = 0xffffffffu;     // above +inf (0xff800000)

// fp32 -> uint32 with the order of the contract: a < b as floats <=> key(a) < key(b); -0 and +0 share a key; every NaN is TK_NAN
__device__ __forceinline__ uint32_t tk_key(float v) {
    const uint32_t u = __float_as_uint(v);
    uint32_t k = u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
    if ((u & 0x7fffffffu) > 0x7f800000u) k = TK_NAN;
    if (k == 0x7fffffffu) k = 0x80000000u;
    return k;
}

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

// one group of four columns into the list.  REFILL: only pairs that rank after (lk, lc), counted in ``seen``
template <bool VEC, bool REFILL>
__device__ __forceinline__ void tk_group(Top4& t, const float (&a)[4], int lane, int g, int nvalid, uint32_t lk, int lc, int& seen) {
    if (!REFILL && nvalid == 4 && a[0] <= t.thr && a[1] <= t.thr && a[2] <= t.thr && a[3] <= t.thr) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t key = tk_key(a[j]);
        const int col = tk_col<VEC>(lane, g, j);
        bool take = j < nvalid;
        if (REFILL) {
            take = take && (key < lk || (key == lk && col > lc));
            seen += take ? 1 : 0;
        }
        if (take) t.insert(key, col);
    }
    t.thr = tk_threshold(t.k3);
}

// all columns of this lane, in increasing order, four groups of loads in flight
template <bool VEC, bool REFILL>
__device__ __forceinline__ void tk_scan(Top4& t, const float* __restrict__ row, int V, int lane, uint32_t lk, int lc, int& seen) {
    int g = 0;
    for (; tk_col<VEC>(lane, g + 3, 3) < V; g += 4) {
        float a0[4], a1[4], a2[4], a3[4];
        tk_load<VEC>(row, lane, g, a0);
        tk_load<VEC>(row, lane, g + 1, a1);
        tk_load<VEC>(row, lane, g + 2, a2);
        tk_load<VEC>(row, lane, g + 3, a3);
        tk_group<VEC, REFILL>(t, a0, lane, g, 4, lk, lc, seen);
        tk_group<VEC, REFILL>(t, a1, lane, g + 1, 4, lk, lc, seen);
        tk_group<VEC, REFILL>(t, a2, lane, g + 2, 4, lk, lc, seen);
        tk_group<VEC, REFILL>(t, a3, lane, g + 3, 4, lk, lc, seen);
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
        tk_group<VEC, REFILL>(t, a, lane, g, nvalid, lk, lc, seen);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ scores, int64_t ld, int rows, int V, int k,
                                                        float* __restrict__ vals, int32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                   // whole waves leave together: no barrier below
    const float* __restrict__ row = scores + (int64_t)r * ld;
    Top4 t;
    t.clear();
    int seen = 0;
    tk_scan<VEC, false>(t, row, V, lane, 0u, 0, seen);
    // columns this lane owns: more than the list holds -> an empty list is not the end of the lane
    const int owned = VEC ? ((V + 3) / 4 > lane ? 4 * (((V + 3) / 4 - lane + 63) / 64) : 0) : (V > lane ? (V - lane + 63) / 64 : 0);
    bool more = owned > 4;
    int out_c = -1;
    for (int p = 0; p < k; ++p) {
        const uint64_t mine = t.k0 == TK_EMPTY ? 0ull : ((uint64_t)t.k0 << 32) | (uint32_t)~(uint32_t)t.c0;
        uint64_t best = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o);
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)best, o);
            const uint64_t q = ((uint64_t)hi << 32) | lo;
            best = q > best ? q : best;
        }
        if (best == 0ull) break;                             // fewer than k columns: wave-uniform
        if (lane == p) out_c = (int)~(uint32_t)best;
        if (mine == best) {                                  // columns are unique: exactly one lane
            const uint32_t lk = t.k0;
            const int lc = t.c0;
            t.pop();
            if (t.k0 == TK_EMPTY && more) {
                int cnt = 0;
                tk_scan<VEC, true>(t, row, V, lane, lk, lc, cnt);
                more = cnt > 4;
            }
        }
    }
    if (lane < k) {
        const int64_t o = (int64_t)r * k + lane;
        vals[o] = out_c >= 0 ? row[out_c] : -INFINITY;
        idx[o] = out_c;
    }
}

// One wave per selected (row, rank): the cosine of kw[row] and table[idx] with fp64 accumulation of the three sums, rounded once.
__global__ __launch_bounds__(256) void topk_rescore_cos_kernel(const float* __restrict__ kw, int64_t ldk, const float* __restrict__ table,
                                                               int64_t ldt, int V, int E, float eps, const int32_t* __restrict__ idx,
                                                               int64_t n, int k, float* __restrict__ vals) {
    const int lane = threadIdx.x & 63;
    const int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= n) return;
    const int col = idx[o];
    if (col < 0 || col >= V) {       // no such neighbour (or not an index of this table): nothing is read
        if (lane == 0) vals[o] = -INFINITY;
        return;
    }
    const float* __restrict__ a = kw + (o / k) * ldk;
    const float* __restrict__ b = table + (int64_t)col * ldt;
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (int e = lane; e < E; e += 64) {
        const double x = (double)a[e], y = (double)b[e];
        ab = fma(x, y, ab);
        aa = fma(x, x, aa);
        bb = fma(y, y, bb);
    }
    ab = wave_sum_d(ab);
    aa = wave_sum_d(aa);
    bb = wave_sum_d(bb);
    if (lane == 0) vals[o] = (float)(ab / (fmax(sqrt(aa), (double)eps) * fmax(sqrt(bb), (double)eps)));
}

}  // namespace

extern "C" int sc_topk_rescore_cos_f32(const float* kw, int64_t ldk, const float* table, int64_t ldt, int32_t V, int32_t E, float eps,
                                       const int32_t* idx, int32_t rows, int32_t k, float* vals, void* stream) {
    SC_CHECK(rows >= 0 && V >= 1 && E >= 1 && k >= 1 && ldk >= E && ldt >= E, "sc_topk_rescore_cos_f32: bad shape (rows %d, V %d, E %d, k %d)",
             rows, V, E, k);
    if (rows == 0) return 0;
    SC_CHECK(kw && table && idx && vals, "sc_topk_rescore_cos_f32: null pointer");
    const int64_t n = (int64_t)rows * k;
    hipLaunchKernelGGL(topk_rescore_cos_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, kw, ldk, table, ldt, V, E, eps,
                       idx, n, k, vals);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_topk_rows_f32(const float* scores, int64_t ld, int32_t rows, int32_t V, int32_t k, float* vals, int32_t* idx,
                                void* stream) {
    SC_CHECK(rows >= 0 && V >= 1 && ld >= V, "sc_topk_rows_f32: rows >= 0, V >= 1, ld >= V (rows %d, V %d, ld %lld)", rows, V, (long long)ld);
    SC_CHECK(k >= 1 && k <= 32, "sc_topk_rows_f32: 1 <= k <= 32 (k %d)", k);
    if (rows == 0) return 0;
    SC_CHECK(scores && vals && idx, "sc_topk_rows_f32: null pointer");
    const bool vec = (((uintptr_t)scores) & 15) == 0 && (ld & 3) == 0;
    const dim3 grid((rows + 3) / 4), block(256);
    if (vec)
        hipLaunchKernelGGL(topk_rows_kernel<true>, grid, block, 0, (hipStream_t)stream, scores, ld, rows, V, k, vals, idx);
    else
        hipLaunchKernelGGL(topk_rows_kernel<false>, grid, block, 0, (hipStream_t)stream, scores, ld, rows, V, k, vals, idx);
    SC_LAUNCH_CHECK();
    return 0;
}
