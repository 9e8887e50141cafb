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
// One wave per row (four rows per 256-thread workgroup, no barrier): topk_rows.h's selection with no filter - four candidates per
// lane in named registers, a float pre-test per group of four columns, k pops of a 64-lane maximum, a re-scan for a lane that runs
// empty.  Every score is read once (re-scans aside) -> bandwidth-bound.
#include "topk_rows.h"

namespace {

template <bool VEC>
__global__ __launch_bounds__(256) void topk_rows_kernel(const float* __restrict__ scores, int64_t ld, int rows, int V, int k,
                                                        float* __restrict__ vals, int32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                   // whole waves leave together: no barrier below
    topk_select_row<VEC>(scores + (int64_t)r * ld, V, k, lane, NoRowFilter{}, vals + (int64_t)r * k, idx + (int64_t)r * k);
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
