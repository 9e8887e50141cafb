// Wide per-row top-K over an fp32 score matrix (gfx950): 33 <= k <= 1024 (1 <= k accepted, so that it can be held against topk.hip),
// with search_filter.hip's admissibility rule as nullable operands.  The selection behind search / hard_negatives / retrieve at k > 32:
// the scores come from the composition route's score GEMM (sc_split3_bf16 + sc_gemm_bf16 into the score scratch); this file only selects.
//   sc_topk_rows_wide_f32   scores [rows, ld] fp32, V valid columns, q_ids [rows] / g_ids [V] int64 or both NULL, live [V] bytes or NULL
//                           -> vals [rows, k] fp32, idx [rows, k] int32, best first
//
// The order is topk.hip's contract: larger value first, among equal values the lower column first (a stable descending sort;
// -0 == +0), NaN above every number, lower column first among NaNs.  Fewer than k eligible columns: the tail is -inf / -1.  vals are
// the matrix's own bits (-0, NaN payloads), re-read at the end.  Column j is ELIGIBLE iff j < V, live is NULL or live[j] != 0, and
// the ids are NULL or g_ids[j] != q_ids[row]; an ineligible column behaves as absent, an eligible real -inf ranks ahead of every
// filler.  No float atomics; the integer LDS atomics below only count and hand out slots of a buffer that is sorted afterwards on
// distinct words, so the same input gives the same bits.
//
// One 256-thread workgroup per row, four steps:
//   1. SELECT.  An exact radix select over the 32-bit keys (search_common.h's tk_key: no column has key 0, so the word 0 is free to
//      mean "no entry"), most significant digit first, 11 + 11 + 10 bits: a 2048-bin LDS histogram per pass (ds_add, no return), a block scan over the bins from the top, the bin holding the kk-th key
//      (kk = min(k, eligible columns)) fixes the digit.  After three passes T is the kk-th key itself, ``need`` the number of
//      columns with key == T that belong to the list and ``cnt`` how many such columns the row has.  Passes two and three test
//      admissibility only for columns whose key carries the prefix, so a filter costs its id / live loads once, not per pass.
//   2. ADMIT.  One more pass puts key << 32 | ~column of every eligible column with key > T into an 8 KiB LDS buffer at a slot
//      from an LDS counter (their order is irrelevant: step 3 sorts).  The columns with key == T: when need == cnt all of them
//      are in and take slots the same way; otherwise the pass runs in increasing column order - every thread owns four
//      consecutive columns of a 1024-column chunk, a block prefix count over the chunk's ties gives each its rank among the
//      row's ties, and exactly the first ``need`` are admitted.  Nothing is buffered per tie, so a row of N equal scores is no
//      special case (the chunk loop stops counting once ``need`` ties are in).
//   3. SORT.  A bitonic sort of the kk words (padded with 0 = no entry to a power of two) in LDS, descending.  Words of distinct
//      columns are distinct: the order is total, and ~column puts the lower column first among equal keys.
//   4. STORE.  idx = the column, vals = the row re-read at it; -inf / -1 behind the kk-th entry.
// The row is read four times (16-byte loads when the row base is 16-byte aligned and the pitch a multiple of four floats, element
// loads 256 columns apart otherwise; columns at or past V are never touched); at the sizes the score scratch holds it stays in the
// Infinity Cache.  No runtime-indexed register arrays.
#include "search_common.h"

namespace {

constexpr int TW_THREADS = 256;
constexpr int TW_BINS = 2048;                // 11 bits per pass (the last pass has 10: its upper 1024 bins stay zero)
constexpr int TW_PER_THREAD = TW_BINS / TW_THREADS;
constexpr int TW_KMAX = 1024;

struct WideFilter {
    const int64_t* __restrict__ g_ids;       // nullptr: no id test
    const uint8_t* __restrict__ live;        // nullptr: every column lives
    int64_t qid;
    __device__ __forceinline__ bool ok(int c) const {
        bool e = true;
        if (live) e = live[c] != 0;
        if (g_ids) e = e && g_ids[c] != qid;
        return e;
    }
};

struct WideShared {
    int hist[TW_BINS];
    uint64_t words[TW_KMAX];
    int wsum[2][4];                          // per-wave totals of the block scans (two buffers: one barrier per ordered chunk)
    int sel[4];                              // digit, remaining, count of the selected bin, total
    int slots;                               // next free slot of ``words`` for the unordered admissions
};

// every column c < V of the row, in no particular order, four loads in flight: f(value, column)
template <bool VEC, class F>
__device__ __forceinline__ void tw_for_each(const float* __restrict__ row, int V, int tid, F&& f) {
    if (VEC) {
        const int nfull = V >> 2;            // whole groups of four columns; the up to three columns behind them: element loads
        int g = tid;
        for (; g + 3 * TW_THREADS < nfull; g += 4 * TW_THREADS) {
            const f32x4 a = *(const f32x4*)(row + 4 * g);
            const f32x4 b = *(const f32x4*)(row + 4 * (g + TW_THREADS));
            const f32x4 c = *(const f32x4*)(row + 4 * (g + 2 * TW_THREADS));
            const f32x4 d = *(const f32x4*)(row + 4 * (g + 3 * TW_THREADS));
#pragma unroll
            for (int j = 0; j < 4; ++j) f(a[j], 4 * g + j);
#pragma unroll
            for (int j = 0; j < 4; ++j) f(b[j], 4 * (g + TW_THREADS) + j);
#pragma unroll
            for (int j = 0; j < 4; ++j) f(c[j], 4 * (g + 2 * TW_THREADS) + j);
#pragma unroll
            for (int j = 0; j < 4; ++j) f(d[j], 4 * (g + 3 * TW_THREADS) + j);
        }
        for (; g < nfull; g += TW_THREADS) {
            const f32x4 a = *(const f32x4*)(row + 4 * g);
#pragma unroll
            for (int j = 0; j < 4; ++j) f(a[j], 4 * g + j);
        }
        const int c = 4 * nfull + tid;
        if (c < V) f(row[c], c);
    } else {
        int c = tid;
        for (; c + 3 * TW_THREADS < V; c += 4 * TW_THREADS) {
            const float a0 = row[c], a1 = row[c + TW_THREADS], a2 = row[c + 2 * TW_THREADS], a3 = row[c + 3 * TW_THREADS];
            f(a0, c);
            f(a1, c + TW_THREADS);
            f(a2, c + 2 * TW_THREADS);
            f(a3, c + 3 * TW_THREADS);
        }
        for (; c < V; c += TW_THREADS) f(row[c], c);
    }
}

__device__ __forceinline__ int tw_wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(v, o);
        if (lane >= o) v += n;
    }
    return v;
}

// The histogram is complete (a barrier lies behind the last ds_add).  Walks the bins from the top: the bin that holds the rem-th
// entry (rem clamped to the total) -> s.sel = {digit, rem inside the bin, the bin's count, total}; the histogram is zero again and
// every thread may read s.sel when this returns.  Thread t owns the bins 2047 - 8 t down to 2040 - 8 t.
__device__ __forceinline__ void tw_select(WideShared& s, int tid, int rem) {
    const int lane = tid & 63, wave = tid >> 6;
    const int hi = TW_BINS - 1 - TW_PER_THREAD * tid;
    int mine = 0;
#pragma unroll
    for (int i = 0; i < TW_PER_THREAD; ++i) mine += s.hist[hi - i];
    const int incl = tw_wave_incl_scan(mine, lane);
    if (lane == 63) s.wsum[0][wave] = incl;
    __syncthreads();
    const int w0 = s.wsum[0][0], w1 = s.wsum[0][1], w2 = s.wsum[0][2], w3 = s.wsum[0][3];
    const int total = w0 + w1 + w2 + w3;
    const int above = incl - mine + (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0);
    rem = rem < total ? rem : total;
    if (tid == 0 && total == 0) {
        s.sel[0] = 0; s.sel[1] = 0; s.sel[2] = 0; s.sel[3] = 0;
    }
    if (above < rem && rem <= above + mine) {        // exactly one thread when total > 0
        int acc = above;
#pragma unroll
        for (int i = 0; i < TW_PER_THREAD; ++i) {
            const int h = s.hist[hi - i];
            if (acc < rem && rem <= acc + h) {
                s.sel[0] = hi - i;
                s.sel[1] = rem - acc;
                s.sel[2] = h;
                s.sel[3] = total;
            }
            acc += h;
        }
    }
#pragma unroll
    for (int i = 0; i < TW_PER_THREAD; ++i) s.hist[hi - i] = 0;
    __syncthreads();
}

template <bool VEC>
__global__ __launch_bounds__(TW_THREADS) void topk_rows_wide_kernel(const float* __restrict__ scores, int64_t ld, int V, int k,
                                                                    const int64_t* __restrict__ q_ids, const int64_t* __restrict__ g_ids,
                                                                    const uint8_t* __restrict__ live, float* __restrict__ vals,
                                                                    int32_t* __restrict__ idx) {
    __shared__ WideShared s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    const float* __restrict__ row = scores + r * ld;
    float* __restrict__ out_v = vals + r * k;
    int32_t* __restrict__ out_i = idx + r * k;
    WideFilter f;
    f.g_ids = g_ids;
    f.live = live;
    f.qid = g_ids ? q_ids[r] : 0;

#pragma unroll
    for (int i = 0; i < TW_PER_THREAD; ++i) s.hist[tid + TW_THREADS * i] = 0;
    if (tid == 0) s.slots = 0;
    __syncthreads();

    // ---- 1. select: T = the kk-th largest key over the eligible columns
    tw_for_each<VEC>(row, V, tid, [&](float v, int c) {
        if (f.ok(c)) atomicAdd(&s.hist[tk_key(v) >> 21], 1);
    });
    __syncthreads();
    tw_select(s, tid, k);
    const int kk = s.sel[3] < k ? s.sel[3] : k;          // entries of the list
    if (kk == 0) {                                       // no eligible column: block-uniform
        for (int p = tid; p < k; p += TW_THREADS) {
            out_v[p] = -INFINITY;
            out_i[p] = -1;
        }
        return;
    }
    const uint32_t p1 = (uint32_t)s.sel[0];
    int rem = s.sel[1];
    __syncthreads();                                     // s.sel is read: the next select may write it
    tw_for_each<VEC>(row, V, tid, [&](float v, int c) {
        const uint32_t key = tk_key(v);
        if ((key >> 21) == p1 && f.ok(c)) atomicAdd(&s.hist[(key >> 10) & 0x7ffu], 1);
    });
    __syncthreads();
    tw_select(s, tid, rem);
    const uint32_t p2 = (p1 << 11) | (uint32_t)s.sel[0];
    rem = s.sel[1];
    __syncthreads();
    tw_for_each<VEC>(row, V, tid, [&](float v, int c) {
        const uint32_t key = tk_key(v);
        if ((key >> 10) == p2 && f.ok(c)) atomicAdd(&s.hist[key & 0x3ffu], 1);
    });
    __syncthreads();
    tw_select(s, tid, rem);
    const uint32_t T = (p2 << 10) | (uint32_t)s.sel[0];
    const int need = s.sel[1];                           // columns with key == T in the list (>= 1)
    const int cnt = s.sel[2];                            // columns with key == T in the row
    const int above = kk - need;                         // columns with key > T

    // the sort's buffer: P words, "no entry" until a column is admitted (kk .. P - 1 stay so: the padding)
    int P = 2;
    while (P < kk) P <<= 1;
    for (int i = tid; i < P; i += TW_THREADS) s.words[i] = 0ull;
    __syncthreads();

    // ---- 2. admit
    if (need == cnt) {                                   // every tie is in: no order to keep
        tw_for_each<VEC>(row, V, tid, [&](float v, int c) {
            const uint32_t key = tk_key(v);
            if (key >= T && f.ok(c)) {
                const int slot = atomicAdd(&s.slots, 1);
                if (slot < kk) s.words[slot] = ((uint64_t)key << 32) | (uint32_t)~(uint32_t)c;
            }
        });
    } else {                                             // the first ``need`` ties by column: chunks of 1024 columns, four per thread
        int tie_base = 0;                                // ties in the chunks behind: block-uniform
        for (int c0 = 0; c0 < V; c0 += 4 * TW_THREADS) {
            const int c = c0 + 4 * tid;
            float a[4];
            if (VEC && c + 3 < V) {
                const f32x4 q = *(const f32x4*)(row + c);
                a[0] = q[0]; a[1] = q[1]; a[2] = q[2]; a[3] = q[3];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = c + j < V ? row[c + j] : 0.f;
            }
            const bool ties = tie_base < need;           // block-uniform: the barrier below is taken by all or none
            uint64_t w[4];
            bool tie[4];
            int ntie = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t key = tk_key(a[j]);
                const bool in = c + j < V && (key > T || (ties && key == T)) && f.ok(c + j);
                w[j] = ((uint64_t)key << 32) | (uint32_t)~(uint32_t)(c + j);
                tie[j] = in && key == T;
                ntie += tie[j] ? 1 : 0;
                if (in && key > T) {
                    const int slot = atomicAdd(&s.slots, 1);
                    if (slot < above) s.words[slot] = w[j];
                }
            }
            if (ties) {
                const int par = (c0 >> 10) & 1;
                const int incl = tw_wave_incl_scan(ntie, lane);
                if (lane == 63) s.wsum[par][wave] = incl;
                __syncthreads();
                const int w0 = s.wsum[par][0], w1 = s.wsum[par][1], w2 = s.wsum[par][2], w3 = s.wsum[par][3];
                int pos = tie_base + incl - ntie + (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (tie[j]) {
                        if (pos < need) s.words[above + pos] = w[j];
                        ++pos;
                    }
                }
                tie_base += w0 + w1 + w2 + w3;
            }
        }
    }

    // ---- 3. sort the P words, descending
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = tid; i < (P >> 1); i += TW_THREADS) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const uint64_t x = s.words[lo], y = s.words[hi];
                const bool desc = (lo & size) == 0;
                if ((x < y) == desc) {
                    s.words[lo] = y;
                    s.words[hi] = x;
                }
            }
        }
    }
    __syncthreads();

    // ---- 4. store: the matrix's own bits; a real -inf keeps its column
    for (int p = tid; p < k; p += TW_THREADS) {
        int c = -1;
        if (p < kk) c = (int)~(uint32_t)s.words[p];
        if ((uint32_t)c >= (uint32_t)V) c = -1;          // "no entry" (never among the first kk words); nothing outside the row is read
        out_v[p] = c >= 0 ? row[c] : -INFINITY;
        out_i[p] = c;
    }
}

}  // namespace

extern "C" int sc_topk_rows_wide_f32(const float* scores, int64_t ld, int32_t rows, int32_t V, int32_t k, const int64_t* q_ids,
                                     const int64_t* g_ids, const uint8_t* live, float* vals, int32_t* idx, void* stream) {
    SC_CHECK(rows >= 0 && V >= 1 && ld >= V, "sc_topk_rows_wide_f32: rows >= 0, V >= 1, ld >= V (rows %d, V %d, ld %lld)", rows, V,
             (long long)ld);
    SC_CHECK(V <= (1 << 30), "sc_topk_rows_wide_f32: V <= 2^30 (V %d)", V);
    SC_CHECK(k >= 1 && k <= TW_KMAX, "sc_topk_rows_wide_f32: 1 <= k <= 1024 (k %d)", k);
    SC_CHECK((q_ids == nullptr) == (g_ids == nullptr) || rows == 0,
             "sc_topk_rows_wide_f32: ids on one side only (q_ids %s, g_ids %s): give both or neither", q_ids ? "given" : "NULL",
             g_ids ? "given" : "NULL");
    if (rows == 0) return 0;
    SC_CHECK(scores && vals && idx, "sc_topk_rows_wide_f32: null pointer");
    SC_CHECK(((uintptr_t)q_ids % 8) == 0 && ((uintptr_t)g_ids % 8) == 0, "sc_topk_rows_wide_f32: ids must be 8-byte aligned");
    SC_CHECK(((uintptr_t)scores % 4) == 0 && ((uintptr_t)vals % 4) == 0 && ((uintptr_t)idx % 4) == 0,
             "sc_topk_rows_wide_f32: scores, vals and idx must be 4-byte aligned");
    const bool vec = (((uintptr_t)scores) & 15) == 0 && (ld & 3) == 0;
    const dim3 grid((unsigned)rows), block(TW_THREADS);
    if (vec)
        hipLaunchKernelGGL(topk_rows_wide_kernel<true>, grid, block, 0, (hipStream_t)stream, scores, ld, V, k, q_ids, g_ids, live, vals, idx);
    else
        hipLaunchKernelGGL(topk_rows_wide_kernel<false>, grid, block, 0, (hipStream_t)stream, scores, ld, V, k, q_ids, g_ids, live, vals, idx);
    SC_LAUNCH_CHECK();
    return 0;
}
