// Constant-query attention pooling of the fixed-keyword cascaded branch (avssl/model/kw_branches.py:349-382 over
// MultiheadAttentionAndNorm, TransformerModels.py:120-126) without materialising Q / K / V.
//
// The branch keeps only the K keyword rows of LN(MHA([cls_1..cls_K ; frames]) + .), and those K queries are parameters.  As in
// clspool.hip the query is folded into the key projection (a_q = dh^-1/2 Wk^T q_q, host side), so per utterance b and query q
//   s      = [ c[q, 0..C) ; a_q . X[b, row0 + t] , t < flen[b] ]        c = a . cls^T: the constant (CLS) rows are keys too
//   p      = softmax(s) ;  w = p * mult                                   (mult: attention dropout, NULL = none)
//   m[b,q] = sum_j w_j crow[j] + sum_t w_t X[b, row0 + t] ;  psum[b,q] = sum w
// Differences from clspool.hip: any Q, C in 1..16 (not only powers of two), C constant keys that live outside X (fp32 rows), the
// frames at a row offset, flen = 0 allowed, and rows of X outside the frames are never loaded (NaN there cannot reach an output).
// Two sweeps over X per direction: kw_scores_kernel (X . vec^T), then the pooling / gradient kernel.  No atomics: the batch sums
// of da / dc are a fixed-order loop over per-utterance partials.
#include "sc_common.h"

namespace {

constexpr int KW_MAXQ = 16;

// scores[b, q0 + q, s] = vec[b?, q0 + q, :] . X[b, s, :] for the frame rows row0 <= s < row0 + flen[b] only (other entries of
// `scores` are left untouched and never read).  One wave per row, lanes across D, the NQ vectors in registers.
template <int NQ, int NCH>     // NCH: 4-element chunks per lane (D <= 256 NCH)
__global__ __launch_bounds__(256) void kw_scores_kernel(const uint16_t* __restrict__ X, const float* __restrict__ vec,
                                                        int64_t vec_bstride, const int32_t* __restrict__ flen,
                                                        float* __restrict__ scores, int R, int D, int Q, int q0, int row0) {
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = max(0, min(flen[b], R - row0));
    constexpr int ROWS = 64, RPW = ROWS / 4;
    if (blockIdx.x * ROWS >= row0 + n || (int)(blockIdx.x + 1) * ROWS <= row0) return;      // no frame row in this block
    const int nchunks = D >> 2;
    const float* vb = vec + (int64_t)b * vec_bstride + (int64_t)q0 * D;
    f32x4 vr[NQ][NCH];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = lane + 64 * c;
            vr[q][c] = ch < nchunks ? *(const f32x4*)(vb + (int64_t)q * D + ch * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    const int s0 = blockIdx.x * ROWS + wave * RPW;
#pragma unroll
    for (int g = 0; g < RPW; g += 4) {
        uint2 u[4][NCH];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = s0 + g + r;
            const bool ok = s >= row0 && s < row0 + n;              // wave-uniform
            const uint16_t* xr = X + ((int64_t)b * R + (ok ? s : 0)) * D;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int ch = lane + 64 * c;
                u[r][c] = (ok && ch < nchunks) ? *(const uint2*)(xr + ch * 4) : uint2{0u, 0u};
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = s0 + g + r;
            if (s < row0 || s >= row0 + n) continue;
            float acc[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const float x0 = bflo(u[r][c].x), x1 = bfhi(u[r][c].x), x2 = bflo(u[r][c].y), x3 = bfhi(u[r][c].y);
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc[q] += x0 * vr[q][c][0] + x1 * vr[q][c][1] + x2 * vr[q][c][2] + x3 * vr[q][c][3];
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const float t = wave_sum(acc[q]);
                if (lane == 0) scores[((int64_t)b * Q + q0 + q) * R + s] = t;
            }
        }
    }
}

// index i of the C + R wide probability row: i < C = constant key i, else row i - C of X
__device__ __forceinline__ bool kw_valid(int i, int C, int row0, int n) { return i < C || (i >= C + row0 && i < C + row0 + n); }

// grid (D/64, B): softmax over the C constant keys and the n frames (redundant per block, tiny), then
// m[b,q,d] = sum_j w[q,j] crow[j,d] + sum_t w[q,t] X[b,row0+t,d] for this block's 64 columns.
template <int QP>     // Q padded to 1, 2, 4, 8, 16
__global__ __launch_bounds__(256) void kw_pool_fwd_kernel(const uint16_t* __restrict__ X, const float* __restrict__ scores,
                                                          const float* __restrict__ c, const float* __restrict__ crow,
                                                          const int32_t* __restrict__ flen, float* __restrict__ p,
                                                          float* __restrict__ m, int R, int D, int Q, int C, int row0,
                                                          const float* __restrict__ mult, float* __restrict__ psum) {
    extern __shared__ float sm[];            // w[Q][C + R] then red[4][Q][64]
    const int P = C + R;
    float* ps = sm;
    float* red = sm + Q * P;
    const int b = blockIdx.y, d0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = max(0, min(flen[b], R - row0));
    for (int q = wave; q < Q; q += 4) {
        const float* sr = scores + ((int64_t)b * Q + q) * R + row0;
        const float* cr = c + (int64_t)q * C;
        float mx = -INFINITY;
        for (int j = lane; j < C + n; j += 64) mx = fmaxf(mx, j < C ? cr[j] : sr[j - C]);
        mx = wave_max(mx);
        float sum = 0.f;
        for (int j = lane; j < C + n; j += 64) {
            const float e = __expf((j < C ? cr[j] : sr[j - C]) - mx);
            ps[q * P + (j < C ? j : j + row0)] = e;
            sum += e;
        }
        sum = wave_sum(sum);
        const float inv = 1.0f / sum;
        float kept = 0.f;
        const int64_t prow = ((int64_t)b * Q + q) * P;
        // normalise with the lane mapping of the loop above: a lane reads back only what it wrote itself
        for (int j = lane; j < C + n; j += 64) {
            const int i = j < C ? j : j + row0;
            const float v = ps[q * P + i] * inv;
            // attention-weight dropout (train mode): the pooling uses p * mult (mult = 0 or 1 / (1 - p_drop)), p itself is kept
            const float w = mult ? v * mult[prow + i] : v;
            ps[q * P + i] = w;
            kept += w;
            if (blockIdx.x == 0) p[prow + i] = v;
        }
        // zeros in the CLS slot in front of the frames and behind flen (entries no lane touched above)
        for (int i = C + lane; i < P; i += 64) {
            if (i < C + row0 || i >= C + row0 + n) {
                ps[q * P + i] = 0.f;
                if (blockIdx.x == 0) p[prow + i] = 0.f;
            }
        }
        if (psum) {                          // sum p mult: the weight of the value bias (dropped weights no longer sum to 1)
            kept = wave_sum(kept);
            if (blockIdx.x == 0 && lane == 0) psum[(int64_t)b * Q + q] = kept;
        }
    }
    __syncthreads();
    // a lane owns 8 columns (one 16-byte load per row) of every 8th row of its wave
    float acc[QP][8];
#pragma unroll
    for (int q = 0; q < QP; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[q][e] = 0.f;
    const int cchunk = lane & 7, rsub = lane >> 3;
    const uint16_t* xc = X + (int64_t)b * R * D + d0 + cchunk * 8;
    const float* pw = ps + C;
    for (int s = row0 + wave * 8 + rsub; s < row0 + n; s += 32) {
        const uint4 u = *(const uint4*)(xc + (int64_t)s * D);
        const float x[8] = {bflo(u.x), bfhi(u.x), bflo(u.y), bfhi(u.y), bflo(u.z), bfhi(u.z), bflo(u.w), bfhi(u.w)};
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            if (q < Q) {
                const float w = pw[q * P + s];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[q][e] = fmaf(w, x[e], acc[q][e]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        if (q < Q) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = acc[q][e];
                v += __shfl_xor(v, 8);
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (rsub == 0) red[(wave * Q + q) * 64 + cchunk * 8 + e] = v;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < Q * 64; i += 256) {
        const int q = i >> 6, d = i & 63;
        float v = (red[(0 * Q + q) * 64 + d] + red[(1 * Q + q) * 64 + d]) + (red[(2 * Q + q) * 64 + d] + red[(3 * Q + q) * 64 + d]);
        for (int j = 0; j < C; ++j) v = fmaf(ps[q * P + j], crow[(int64_t)j * D + d0 + d], v);
        m[((int64_t)b * Q + q) * D + d0 + d] = v;
    }
}

__device__ __forceinline__ void kw_store4(float* dst, const f32x4& g) { *(f32x4*)dst = g; }
__device__ __forceinline__ void kw_store4(uint16_t* dst, const f32x4& g) { *(uint2*)dst = uint2{pack2bf(g[0], g[1]), pack2bf(g[2], g[3])}; }

// grid (D/64, B).  dw_i = dm_q . key_i + cbias ; dp = dw * mult ; ds = p (dp - sum p dp)
//   dX[b,s,d] = sum_q w dm[b,q,d] + ds a[q,d] (frame rows; every other row of the R is written as zero)
//   da_part[b,q,d] = sum_t ds X ;  dc_part[b,q,j] = ds of constant key j
// dpw [B,Q,R]: dm . X on the frame rows (kw_scores_kernel); the constant keys' dm . crow[j] is formed here.
template <int QP, typename DXT>
__global__ __launch_bounds__(256) void kw_pool_bwd_kernel(const uint16_t* __restrict__ X, const float* __restrict__ p,
                                                          const float* __restrict__ dpw, const float* __restrict__ dm,
                                                          const float* __restrict__ a, const float* __restrict__ crow,
                                                          const int32_t* __restrict__ flen, DXT* __restrict__ dX,
                                                          float* __restrict__ da_part, float* __restrict__ dc_part, int R, int D,
                                                          int Q, int C, int row0, const float* __restrict__ mult,
                                                          const float* __restrict__ cbias) {
    extern __shared__ float sm[];            // w[Q][P] (p * mult), ds[Q][P], red[4][Q][64]
    const int P = C + R;
    float* ps = sm;
    float* dss = sm + Q * P;
    float* red = sm + 2 * Q * P;
    const int b = blockIdx.y, d0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = max(0, min(flen[b], R - row0));
    for (int q = wave; q < Q; q += 4) {
        const int64_t prow = ((int64_t)b * Q + q) * P;
        const float* pr = p + prow;
        const float* mr = mult ? mult + prow : nullptr;
        const float* dpr = dpw + ((int64_t)b * Q + q) * R;
        const float* dmr = dm + ((int64_t)b * Q + q) * D;
        float dwc = 0.f;                     // lane j < C: dm_q . crow[j]
        for (int j = 0; j < C; ++j) {
            float t = 0.f;
            for (int d = lane; d < D; d += 64) t = fmaf(dmr[d], crow[(int64_t)j * D + d], t);
            t = wave_sum(t);
            if (lane == j) dwc = t;
        }
        const float cb = cbias ? cbias[(int64_t)b * Q + q] : 0.f;
        float dot = 0.f;
        for (int i = lane; i < P; i += 64)
            if (kw_valid(i, C, row0, n)) dot += pr[i] * (((i < C ? dwc : dpr[i - C]) + cb) * (mr ? mr[i] : 1.f));
        dot = wave_sum(dot);
        for (int i = lane; i < P; i += 64) {
            const bool ok = kw_valid(i, C, row0, n);
            float w = 0.f, ds = 0.f;
            if (ok) {
                const float pv = pr[i], mu = mr ? mr[i] : 1.f;
                w = pv * mu;
                ds = pv * (((i < C ? dwc : dpr[i - C]) + cb) * mu - dot);
            }
            ps[q * P + i] = w;
            dss[q * P + i] = ds;
            if (i < C && blockIdx.x == 0) dc_part[((int64_t)b * Q + q) * C + i] = ds;
        }
    }
    __syncthreads();
    // a lane owns 4 columns of every 4th row of its wave: 16 rows per sweep
    const int cchunk = lane & 15, rsub = lane >> 4, c0 = d0 + cchunk * 4;
    f32x4 dmv[QP], av[QP], acc[QP];
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        const int qq = q < Q ? q : 0;
        dmv[q] = *(const f32x4*)(dm + ((int64_t)b * Q + qq) * D + c0);
        av[q] = *(const f32x4*)(a + (int64_t)qq * D + c0);
        acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const uint16_t* xc = X + (int64_t)b * R * D + c0;
    DXT* gx = dX + (int64_t)b * R * D + c0;
    const float* pw = ps + C;
    const float* dsw = dss + C;
    for (int s = wave * 4 + rsub; s < R; s += 16) {
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (s >= row0 && s < row0 + n) {
            const uint2 u = *(const uint2*)(xc + (int64_t)s * D);
            const f32x4 x = {bflo(u.x), bfhi(u.x), bflo(u.y), bfhi(u.y)};
#pragma unroll
            for (int q = 0; q < QP; ++q) {
                if (q < Q) {
                    const float dsv = dsw[q * P + s], w = pw[q * P + s];
                    g += w * dmv[q] + dsv * av[q];
                    acc[q] += dsv * x;
                }
            }
        }
        kw_store4(gx + (int64_t)s * D, g);
    }
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        if (q < Q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[q][e];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (rsub == 0) red[(wave * Q + q) * 64 + cchunk * 4 + e] = v;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < Q * 64; i += 256) {
        const int q = i >> 6, d = i & 63;
        const float v = (red[(0 * Q + q) * 64 + d] + red[(1 * Q + q) * 64 + d]) + (red[(2 * Q + q) * 64 + d] + red[(3 * Q + q) * 64 + d]);
        da_part[((int64_t)b * Q + q) * D + d0 + d] = v;
    }
}

// da[i] = sum_b da_part[b, i] (i < Q D), dc[i] = sum_b dc_part[b, i] (i < Q C): utterances added in index order
__global__ __launch_bounds__(256) void kw_batch_sum_kernel(const float* __restrict__ da_part, const float* __restrict__ dc_part,
                                                           float* __restrict__ da, float* __restrict__ dc, int B, int nA, int nC) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nA + nC) return;
    const bool isA = i < nA;
    const float* src = isA ? da_part + i : dc_part + (i - nA);
    const int pitch = isA ? nA : nC;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += src[(int64_t)b * pitch];
    if (isA) da[i] = s; else dc[i - nA] = s;
}

int kw_scores_launch(const uint16_t* X, const float* vec, int64_t vec_bstride, const int32_t* flen, float* scores, int B, int R, int D,
                     int Q, int row0, hipStream_t s) {
    const dim3 grid((R + 63) / 64, B);
    const int nch = (D / 4 + 63) / 64;
#define SC_KS(NQ, NC) hipLaunchKernelGGL((kw_scores_kernel<NQ, NC>), grid, dim3(256), 0, s, X, vec, vec_bstride, flen, scores, R, D, Q, q0, row0)
#define SC_KS_Q(NQ)                                                                                                        \
    do {                                                                                                                   \
        if (nch <= 1) SC_KS(NQ, 1); else if (nch == 2) SC_KS(NQ, 2); else if (nch == 3) SC_KS(NQ, 3); else SC_KS(NQ, 4);  \
    } while (0)
    // any Q in 1..16 as groups of 8, 4, 2, 1 queries (16 vectors x 4 chunks do not fit the register file)
    for (int q0 = 0; q0 < Q;) {
        const int rem = Q - q0;
        if (rem >= 8) { SC_KS_Q(8); q0 += 8; }
        else if (rem >= 4) { SC_KS_Q(4); q0 += 4; }
        else if (rem >= 2) { SC_KS_Q(2); q0 += 2; }
        else { SC_KS_Q(1); q0 += 1; }
    }
#undef SC_KS_Q
#undef SC_KS
    SC_LAUNCH_CHECK();
    return 0;
}

int kw_check_dims(const char* who, int B, int R, int D, int Q, int C, int row0, size_t lds) {
    SC_CHECK(B > 0 && R > 0 && row0 >= 0 && row0 < R, "%s: bad arguments (B=%d R=%d row0=%d)", who, B, R, row0);
    SC_CHECK(Q >= 1 && Q <= KW_MAXQ && C >= 1 && C <= KW_MAXQ, "%s: Q=%d, C=%d must be in 1..%d", who, Q, C, KW_MAXQ);
    SC_CHECK(D % 64 == 0 && D <= 1024, "%s: D=%d must be a multiple of 64, <= 1024", who, D);
    SC_CHECK(lds <= 64 * 1024, "%s: Q=%d x (C=%d + R=%d) probabilities need %zu bytes of LDS, limit 65536", who, Q, C, R, lds);
    return 0;
}

}  // namespace

extern "C" int sc_kw_pool_max_rows(int32_t Q, int32_t C, int32_t backward) {
    if (Q < 1 || Q > KW_MAXQ || C < 1 || C > KW_MAXQ) return 0;
    const int64_t floats = 64 * 1024 / 4 - 4 * Q * 64;
    const int64_t r = floats / ((backward ? 2 : 1) * Q) - C;
    return r > 0 ? (int32_t)r : 0;
}

extern "C" int sc_kw_pool_fwd(const sc_bf16* X, const float* a, const float* c, const float* crow, const int32_t* flen, float* scores,
                              float* p, float* m, float* psum, const float* mult, int32_t B, int32_t R, int32_t D, int32_t Q, int32_t C,
                              int32_t row0, void* stream) {
    SC_CHECK(X && a && c && crow && flen && scores && p && m, "sc_kw_pool_fwd: null pointer");
    const size_t lds = (size_t)(Q * (C + R) + 4 * Q * 64) * sizeof(float);
    if (kw_check_dims("sc_kw_pool_fwd", B, R, D, Q, C, row0, lds)) return -1;
    SC_CHECK(((uintptr_t)X % 16) == 0 && ((uintptr_t)a % 16) == 0, "sc_kw_pool_fwd: alignment");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = kw_scores_launch(X, a, 0, flen, scores, B, R, D, Q, row0, s)) return rc;
#define SC_KPF(QP) hipLaunchKernelGGL(kw_pool_fwd_kernel<QP>, dim3(D / 64, B), dim3(256), lds, s, X, scores, c, crow, flen, p, m, R, D, Q, C, row0, mult, psum)
    if (Q == 1) SC_KPF(1); else if (Q == 2) SC_KPF(2); else if (Q <= 4) SC_KPF(4); else if (Q <= 8) SC_KPF(8); else SC_KPF(16);
#undef SC_KPF
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_kw_pool_bwd(const sc_bf16* X, const float* a, const float* crow, const int32_t* flen, const float* p, const float* mult,
                              const float* dm, const float* cbias, float* dpw, void* dX, int32_t dx_bf16, float* da_part,
                              float* dc_part, float* da, float* dc, int32_t B, int32_t R, int32_t D, int32_t Q, int32_t C, int32_t row0,
                              void* stream) {
    SC_CHECK(X && a && crow && flen && p && dm && dpw && dX && da_part && dc_part && da && dc, "sc_kw_pool_bwd: null pointer");
    const size_t lds = (size_t)(2 * Q * (C + R) + 4 * Q * 64) * sizeof(float);
    if (kw_check_dims("sc_kw_pool_bwd", B, R, D, Q, C, row0, lds)) return -1;
    SC_CHECK(((uintptr_t)X % 8) == 0 && ((uintptr_t)dX % 16) == 0 && ((uintptr_t)dm % 16) == 0 && ((uintptr_t)a % 16) == 0,
             "sc_kw_pool_bwd: alignment");
    hipStream_t s = (hipStream_t)stream;
    if (int rc = kw_scores_launch(X, dm, (int64_t)Q * D, flen, dpw, B, R, D, Q, row0, s)) return rc;
#define SC_KPB(QP)                                                                                                                        \
    do {                                                                                                                                  \
        if (dx_bf16)                                                                                                                      \
            hipLaunchKernelGGL((kw_pool_bwd_kernel<QP, uint16_t>), dim3(D / 64, B), dim3(256), lds, s, X, p, dpw, dm, a, crow, flen,      \
                               (uint16_t*)dX, da_part, dc_part, R, D, Q, C, row0, mult, cbias);                                           \
        else                                                                                                                              \
            hipLaunchKernelGGL((kw_pool_bwd_kernel<QP, float>), dim3(D / 64, B), dim3(256), lds, s, X, p, dpw, dm, a, crow, flen,         \
                               (float*)dX, da_part, dc_part, R, D, Q, C, row0, mult, cbias);                                              \
    } while (0)
    if (Q == 1) SC_KPB(1); else if (Q == 2) SC_KPB(2); else if (Q <= 4) SC_KPB(4); else if (Q <= 8) SC_KPB(8); else SC_KPB(16);
#undef SC_KPB
    SC_LAUNCH_CHECK();
    const int nA = Q * D, nC = Q * C;
    hipLaunchKernelGGL(kw_batch_sum_kernel, dim3((nA + nC + 255) / 256), dim3(256), 0, s, da_part, dc_part, da, dc, B, nA, nC);
    SC_LAUNCH_CHECK();
    return 0;
}
