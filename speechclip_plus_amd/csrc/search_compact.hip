// Compact gallery search (gfx950): one bf16 copy of the gallery scanned by a coarse fused top-D kernel, an exact fp64 re-rank of the
// D <= 32 candidates from the fp32 rows, and a per-query certificate that no row outside the candidates can belong to the answer.
//   replaces: the same ranking as csrc/search.hip - torch.argsort(score, descending=True) of the whole score matrix
//             (avssl/module/retrieval.py:45-46) on the scores of avssl/model/kwClip.py:447-482 - with 2 Ep bytes per gallery row
//             instead of the 12 Ep of the three-way split, and K = Ep instead of 6 Ep per score.
//
//   sc_rows_bf16           x [R, E] fp32 (* row_scale) -> out [Rp, Ep] bf16 (round to nearest even, zero outside [R, E]) and
//                          norms [3, R]: |x'|, |x~|, |x' - x~| of the scaled row x', its bf16 image x~ and the residual, each sum of
//                          squares in fp64, rounded once.  One wave per row, one pass, 16-byte loads where the rows allow them.
//   sc_search_coarse_bf16  search_kernels.h's search_scan_kernel<false> - csrc/search.hip's kernel - on plain bf16 operands: K = Ep, lists
//                          of D words.  Same order contract, same slab rule, no atomics.  The K loop is a sixth of search.hip's, so
//                          the scan is a larger share of a tile's period; at D = 32 the lists (32 KiB) and the ring (64 KiB) leave
//                          room for one workgroup per CU, at D <= 16 for two.
//   sc_search_rerank_f32   search_kernels.h's search_rerank_kernel<false>: the exact scores of the D candidates from the fp32 rows in
//                          fp64, ranked by (exact key, ~row), and the certificate: every gallery row is a candidate (N <= D), or the
//                          list is full and its k-th exact score clears the coarse D-th score by more than the bound eps.
#include "search_kernels.h"

#include <algorithm>

namespace {

// ------------------------------------------------------------------------------------------ rows -> bf16 + the three norms
// One wave per output row (4 rows per workgroup); a lane converts 4 consecutive columns per step.  x' - x~ is exact in fp32 (the
// difference of a value and its rounding), so the three sums of squares see the exact operands.
__global__ __launch_bounds__(256) void rows_bf16_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ row_scale, int R,
                                                        int E, uint16_t* __restrict__ out, int Rp, int Ep, float* __restrict__ norms, int vec) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= Rp) return;                                              // wave-uniform
    uint16_t* const o = out + (int64_t)r * Ep;
    if (r >= R) {
        for (int c = lane * 4; c < Ep; c += 256) *(uint2*)(o + c) = make_uint2(0u, 0u);
        return;
    }
    const float* const xr = x + (int64_t)r * ldx;
    const float s = row_scale ? row_scale[r] : 1.f;
    double n_x = 0.0, n_b = 0.0, n_d = 0.0;
    for (int c = lane * 4; c < Ep; c += 256) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && c + 3 < E) {
            const float4 t = *(const float4*)(xr + c);
            v[0] = t.x * s; v[1] = t.y * s; v[2] = t.z * s; v[3] = t.w * s;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j < E) v[j] = xr[c + j] * s;
        }
        const uint32_t lo = pack2bf(v[0], v[1]), hi = pack2bf(v[2], v[3]);
        *(uint2*)(o + c) = make_uint2(lo, hi);
        const float b[4] = {bflo(lo), bfhi(lo), bflo(hi), bfhi(hi)};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double xd = (double)v[j], bd = (double)b[j], dd = (double)(v[j] - b[j]);
            n_x = fma(xd, xd, n_x);
            n_b = fma(bd, bd, n_b);
            n_d = fma(dd, dd, n_d);
        }
    }
    n_x = wave_sum_d(n_x);
    n_b = wave_sum_d(n_b);
    n_d = wave_sum_d(n_d);
    if (lane == 0) {
        norms[r] = (float)sqrt(n_x);
        norms[(int64_t)R + r] = (float)sqrt(n_b);
        norms[2 * (int64_t)R + r] = (float)sqrt(n_d);
    }
}

}  // namespace

extern "C" int sc_rows_bf16(const float* x, int64_t ldx, const float* row_scale, int32_t R, int32_t E, sc_bf16* out, int32_t Rp, int32_t Ep,
                            float* norms, void* stream) {
    SC_CHECK(R >= 0 && E >= 1 && Rp >= R && Rp % 128 == 0 && Ep >= E && Ep % 64 == 0 && ldx >= E,
             "sc_rows_bf16: R=%d E=%d Rp=%d Ep=%d ldx=%lld (Rp %% 128 == 0, Ep %% 64 == 0, Rp >= R, Ep >= E, ldx >= E)", R, E, Rp, Ep,
             (long long)ldx);
    if (Rp == 0) return 0;
    SC_CHECK(out && (R == 0 || (x && norms)), "sc_rows_bf16: null pointer");
    SC_CHECK(((uintptr_t)out % 8) == 0, "sc_rows_bf16: out must be 8-byte aligned");
    const int vec = (((uintptr_t)x % 16) == 0 && ldx % 4 == 0) ? 1 : 0;
    hipLaunchKernelGGL(rows_bf16_kernel, dim3((unsigned)(Rp / 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, row_scale, R, E, (uint16_t*)out, Rp,
                       Ep, norms, vec);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_search_coarse_bf16(const sc_bf16* q_bf16, const sc_bf16* g_bf16, int32_t nQ, int32_t N, int32_t Ep, int32_t D, int32_t S,
                                     float* part_vals, int32_t* part_idx, void* stream) {
    SC_CHECK(nQ >= 0 && N >= 0, "sc_search_coarse_bf16: nQ >= 0, N >= 0 (nQ %d, N %d)", nQ, N);
    SC_CHECK(D >= 1 && D <= SEARCH_MAXK, "sc_search_coarse_bf16: 1 <= D <= 32 (D %d)", D);
    SC_CHECK(Ep > 0 && Ep % 64 == 0, "sc_search_coarse_bf16: Ep=%d must be a multiple of 64", Ep);
    SC_CHECK(S >= 1, "sc_search_coarse_bf16: S >= 1 (S %d)", S);
    const int64_t nT = ((int64_t)N + BN - 1) / BN;
    const int64_t tiles = std::max<int64_t>((nT + S - 1) / S, 1);
    // every slab but the last must hold at least D valid columns (the merge relies on fillers only at the very end): with whole
    // 128-column tiles that is "the last slab is not empty" - then every earlier slab is made of full tiles
    SC_CHECK(S == 1 || (int64_t)(S - 1) * tiles < nT,
             "sc_search_coarse_bf16: S=%d slabs of %lld column tiles leave a slab before the last with fewer than D columns (N %d: %lld tiles)", S,
             (long long)tiles, N, (long long)nT);
    if (nQ == 0) return 0;
    SC_CHECK(part_vals && part_idx, "sc_search_coarse_bf16: null output");
    SC_CHECK(N == 0 || (q_bf16 && g_bf16), "sc_search_coarse_bf16: null operand");
    SC_CHECK(((uintptr_t)q_bf16 % 16) == 0 && ((uintptr_t)g_bf16 % 16) == 0, "sc_search_coarse_bf16: operands must be 16-byte aligned");
    const int64_t nM = ((int64_t)nQ + BM - 1) / BM;
    SC_CHECK(nM * S < ((int64_t)1 << 31), "sc_search_coarse_bf16: %lld workgroups", (long long)(nM * S));
    SearchScanArgs a{};
    a.q = (const uint16_t*)q_bf16;
    a.g = (const uint16_t*)g_bf16;
    a.nQ = nQ; a.N = N; a.K = Ep; a.k = D; a.S = S; a.tiles = (int)tiles;
    a.part_vals = part_vals;
    a.part_idx = part_idx;
    return search_scan_launch<false>(a, nM * S, "search_coarse", (hipStream_t)stream);
}

extern "C" int sc_search_rerank_f32(const float* q, int64_t ldq, const float* q_scale, const float* rows, int64_t ldr, const float* g_scale,
                                    const int32_t* cand_idx, const float* cand_vals, const float* eps, int32_t nQ, int32_t N, int32_t E,
                                    int32_t D, int32_t k, float* vals, int32_t* idx, uint8_t* certified, void* stream) {
    return search_rerank<false>("sc_search_rerank_f32", q, ldq, q_scale, rows, ldr, g_scale, cand_idx, cand_vals, eps, nQ, N, E, D, k, vals, idx,
                                certified, stream);
}
