// The keyword quantiser's other training modes (include/speechclip_hip_vq.h; my_vector_quantizer.py:124-137):
//   use_gumbel        s = softmax((x + g) / tau), g = -log(-log u) Gumbel noise (F.gumbel_softmax)
//   hard = false      subword_prob = s itself: keywords = s . token_embedding, a dense [Nk, V] x [V, Et] product
//   temp learnable    d tau = -(1 / tau) sum dz z
// x are the MASKED scores sc_vq_rowstats leaves behind (-inf in the special columns): exp -> exactly 0 there, and a zero
// probability never meets its upstream gradient (no 0 * inf).
//
// The noise is stateless: element e = n V + v (V the true vocabulary), w = sc_hash32(e ^ seed), u = ((w >> 9) + 0.5) 2^-23 - exact in
// fp32, in [2^-24, 1 - 2^-24] - and g = -logf(-logf(u)) with the PRECISE logf (1 ulp = 2 U relative, U = 2^-24): the inner logarithm's
// relative error e1 <= 2 U becomes an absolute error e1 of the outer one, whose own rounding adds 2 U |g|: |g - g_exact| <= 2 U + 2 U |g|,
// inside the header's 4 U (1 + |g|).  (The fast __logf is v_log_f32 * ln 2: near u -> 1 its ABSOLUTE error of ~2^-22 in log2 u meets
// -log u = 2^-24, no bound at all; it is not used here.)  Every kernel evaluates g again from (n, v, seed) instead of reading a stored
// [Nk, V] matrix: 78 hashes + 2 logarithms per thread and row pass at V = 19 787, against 4 bytes of HBM each way.
//   sc_vq_gumbel_f32      g materialised (tests' twin, the benchmark's torch yardstick)
//   sc_vq_noisy_rowstats  first argmax (x + g), m = max (x + g), ls = log sum exp((x + g - m) / tau): LSE = m / tau + ls, kept apart
//                         one workgroup per row, sc_vq_rowstats' tie rule; noise 0: the same statistics of x with the precise exp / log
//   sc_vq_soft_prob_f32   dense s
//   sc_vq_soft_split_bf16 s as bf16 hi + lo in the K-blocks [hi | hi | lo] of the soft product (against a table [hi | lo | hi])
//   sc_vq_soft_bwd2       dx = s (t - <s, t>) / tau and the row terms of d tau
// Fixed-order reductions, no atomics.
#include "sc_common.h"
#include "speechclip_hip_vq.h"

namespace {

__device__ __forceinline__ float gumbel_noise(uint32_t e, uint32_t seed) {
    const uint32_t w = sc_hash32(e ^ seed);
    const float u = ((float)(w >> 9) + 0.5f) * 0x1p-23f;          // 23-bit integer + 0.5: 24 significant bits, exact
    return -logf(-logf(u));
}

// y = x + g (noise) or x: the perturbed score of (row n, column v)
__device__ __forceinline__ float noisy_score(float xv, uint32_t n, uint32_t v, uint32_t V, uint32_t seed, int noise) {
    return noise ? xv + gumbel_noise(n * V + v, seed) : xv;        // -inf + finite = -inf
}

__device__ __forceinline__ float block_sum4(float v, float* red) {          // red: 4 floats of LDS; all 256 threads get the total
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void vq_gumbel_kernel(float* __restrict__ g, int64_t ldg, int Nk, int V, uint32_t seed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)Nk * V) return;
    const uint32_t n = (uint32_t)(i / V), v = (uint32_t)(i - (int64_t)n * V);
    g[(int64_t)n * ldg + v] = gumbel_noise((uint32_t)i, seed);
}

__global__ __launch_bounds__(256) void vq_noisy_rowstats_kernel(const float* __restrict__ x, int64_t ldx, int V, float inv_temp, uint32_t seed,
                                                                int noise, int64_t* __restrict__ idx, float* __restrict__ rowmax,
                                                                float* __restrict__ logsum) {
    __shared__ float red[4];
    __shared__ float redm[4];
    __shared__ int redi[4];
    const uint32_t n = blockIdx.x;
    const float* row = x + (int64_t)n * ldx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float m = -INFINITY;
    int mi = 0x7fffffff;
    for (int v = threadIdx.x; v < V; v += 256) {
        const float y = noisy_score(row[v], n, v, V, seed, noise);
        if (y > m || (y == m && v < mi)) { m = y; mi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o);
        const int oi = __shfl_xor(mi, o);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    if (lane == 0) { redm[wave] = m; redi[wave] = mi; }
    __syncthreads();
    m = redm[0];
    mi = redi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (redm[w] > m || (redm[w] == m && redi[w] < mi)) { m = redm[w]; mi = redi[w]; }
    float st = 0.f;
    for (int v = threadIdx.x; v < V; v += 256) {
        const float y = noisy_score(row[v], n, v, V, seed, noise);
        st += expf((y - m) * inv_temp);                      // masked: exp(-inf) = 0
    }
    st = block_sum4(st, red);
    if (threadIdx.x == 0) {
        idx[n] = mi;
        rowmax[n] = m;
        logsum[n] = logf(st);
    }
}

// s = exp((y - m) / tau - ls) with m = max y and ls = log sum exp((y - m) / tau) kept APART: their sum LSE = m / tau + ls would carry an
// absolute rounding error of U |m / tau| into the exponent (6e-5 at tau = 1e-3), while y - m is exact at the maximum and carries only a
// RELATIVE error elsewhere - s stays accurate to a few hundred U at every temperature.
__device__ __forceinline__ float soft_prob_of(float y, float inv_temp, float m, float ls) { return expf(fmaf(y - m, inv_temp, -ls)); }
__device__ __forceinline__ float soft_prob(float xv, uint32_t n, uint32_t v, uint32_t V, uint32_t seed, int noise, float inv_temp, float m,
                                           float ls) {
    return soft_prob_of(noisy_score(xv, n, v, V, seed, noise), inv_temp, m, ls);
}

__global__ __launch_bounds__(256) void vq_soft_prob_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ rowmax,
                                                           const float* __restrict__ logsum, int V,
                                                           float inv_temp, uint32_t seed, int noise, float* __restrict__ s, int64_t lds) {
    const uint32_t n = blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    s[(int64_t)n * lds + v] = soft_prob(x[(int64_t)n * ldx + v], n, v, V, seed, noise, inv_temp, rowmax[n], logsum[n]);
}

// one thread = 4 consecutive columns of a row of the padded [Nkp, Vp] problem; out [Nkp][3 Vp] = [hi | hi | lo]
__global__ __launch_bounds__(256) void vq_soft_split_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ rowmax,
                                                            const float* __restrict__ logsum, int Nk, int V,
                                                            float inv_temp, uint32_t seed, int noise, uint16_t* __restrict__ out, int Nkp,
                                                            int Vp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int q4 = Vp >> 2;
    if (i >= (int64_t)Nkp * q4) return;
    const int n = (int)(i / q4), c = (int)(i - (int64_t)n * q4) * 4;
    float sv[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < Nk) {
        const float m = rowmax[n], ls = logsum[n];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < V) sv[j] = soft_prob(x[(int64_t)n * ldx + c + j], n, c + j, V, seed, noise, inv_temp, m, ls);
    }
    const uint32_t h0 = pack2bf(sv[0], sv[1]), h1 = pack2bf(sv[2], sv[3]);
    // exact: the difference of a value and its rounding
    const uint32_t l0 = pack2bf(sv[0] - bflo(h0), sv[1] - bfhi(h0)), l1 = pack2bf(sv[2] - bflo(h1), sv[3] - bfhi(h1));
    uint16_t* o = out + (int64_t)n * 3 * Vp + c;
    *(uint2*)o = make_uint2(h0, h1);
    *(uint2*)(o + Vp) = make_uint2(h0, h1);
    *(uint2*)(o + 2 * (int64_t)Vp) = make_uint2(l0, l1);
}

template <typename OutT>
__global__ __launch_bounds__(256) void vq_soft_bwd2_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ rowmax,
                                                           const float* __restrict__ logsum, const float* __restrict__ t, int64_t ldt, int V, int Vpad, float inv_temp,
                                                           uint32_t seed, int noise, OutT* __restrict__ dx, int64_t ldd,
                                                           float* __restrict__ dtemp_row) {
    __shared__ float red[4];
    const uint32_t n = blockIdx.x;
    const float* xr = x + (int64_t)n * ldx;
    const float* tr = t + (int64_t)n * ldt;
    OutT* dr = dx + (int64_t)n * ldd;
    const float ym = rowmax[n], ls = logsum[n];
    float m = 0.f;
    for (int v = threadIdx.x; v < V; v += 256) {
        const float s = soft_prob(xr[v], n, v, V, seed, noise, inv_temp, ym, ls);
        if (s > 0.f) m = fmaf(s, tr[v], m);             // masked columns: s = 0 (and t may be anything)
    }
    m = block_sum4(m, red);
    float dt = 0.f;
    for (int v = threadIdx.x; v < Vpad; v += 256) {
        float g = 0.f;
        if (v < V) {
            const float y = noisy_score(xr[v], n, v, V, seed, noise);
            const float s = soft_prob_of(y, inv_temp, ym, ls);
            if (s > 0.f) {
                const float dz = s * (tr[v] - m);
                g = dz * inv_temp;
                dt = fmaf(dz, y * inv_temp, dt);
            }
        }
        if constexpr (sizeof(OutT) == 2) dr[v] = f2bf(g);
        else dr[v] = g;
    }
    if (dtemp_row) {                                    // uniform over the workgroup: the barrier inside block_sum4 is safe
        dt = block_sum4(dt, red);
        if (threadIdx.x == 0) dtemp_row[n] = -dt * inv_temp;
    }
}

}  // namespace

#define VQ_CHECK_ROWS(name)                                                                                               \
    SC_CHECK(Nk > 0 && V > 0, name ": Nk=%d V=%d must be positive", Nk, V);                                            \
    SC_CHECK((int64_t)Nk * V < ((int64_t)1 << 32), name ": Nk * V = %lld does not fit the 32-bit noise index", (long long)Nk * V)

extern "C" int sc_vq_gumbel_f32(float* g, int64_t ldg, int32_t Nk, int32_t V, uint32_t seed, void* stream) {
    SC_CHECK(g, "sc_vq_gumbel_f32: null pointer");
    VQ_CHECK_ROWS("sc_vq_gumbel_f32");
    SC_CHECK(ldg >= V, "sc_vq_gumbel_f32: ldg=%lld < V=%d", (long long)ldg, V);
    const int64_t total = (int64_t)Nk * V;
    hipLaunchKernelGGL(vq_gumbel_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, ldg, Nk, V, seed);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_vq_noisy_rowstats(const float* x, int64_t ldx, int32_t Nk, int32_t V, float temp, uint32_t seed, int32_t noise, int64_t* idx,
                                    float* rowmax, float* logsum, void* stream) {
    SC_CHECK(x && idx && rowmax && logsum, "sc_vq_noisy_rowstats: null pointer");
    VQ_CHECK_ROWS("sc_vq_noisy_rowstats");
    SC_CHECK(ldx >= V && temp > 0.f, "sc_vq_noisy_rowstats: ldx=%lld (>= V=%d) temp=%g (> 0)", (long long)ldx, V, (double)temp);
    hipLaunchKernelGGL(vq_noisy_rowstats_kernel, dim3(Nk), dim3(256), 0, (hipStream_t)stream, x, ldx, V, 1.f / temp, seed, noise != 0, idx, rowmax, logsum);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_vq_soft_prob_f32(const float* x, int64_t ldx, const float* rowmax, const float* logsum, int32_t Nk, int32_t V, float temp, uint32_t seed,
                                   int32_t noise, float* s, int64_t lds, void* stream) {
    SC_CHECK(x && rowmax && logsum && s, "sc_vq_soft_prob_f32: null pointer");
    VQ_CHECK_ROWS("sc_vq_soft_prob_f32");
    SC_CHECK(ldx >= V && lds >= V && temp > 0.f && Nk <= 65535, "sc_vq_soft_prob_f32: ldx=%lld lds=%lld (>= V=%d) temp=%g (> 0) Nk=%d (<= 65535)",
             (long long)ldx, (long long)lds, V, (double)temp, Nk);
    hipLaunchKernelGGL(vq_soft_prob_kernel, dim3((V + 255) / 256, Nk), dim3(256), 0, (hipStream_t)stream, x, ldx, rowmax, logsum, V, 1.f / temp,
                       seed, noise != 0, s, lds);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_vq_soft_split_bf16(const float* x, int64_t ldx, const float* rowmax, const float* logsum, int32_t Nk, int32_t V, float temp, uint32_t seed,
                                     int32_t noise, uint16_t* out, int32_t Nkp, int32_t Vp, void* stream) {
    SC_CHECK(x && rowmax && logsum && out, "sc_vq_soft_split_bf16: null pointer");
    VQ_CHECK_ROWS("sc_vq_soft_split_bf16");
    SC_CHECK(ldx >= V && temp > 0.f && Nkp >= Nk && Vp >= V && Vp % 4 == 0 && ((uintptr_t)out % 8) == 0,
             "sc_vq_soft_split_bf16: ldx=%lld (>= V=%d) temp=%g (> 0) Nkp=%d (>= Nk=%d) Vp=%d (>= V, %% 4 == 0, out 8-byte aligned)",
             (long long)ldx, V, (double)temp, Nkp, Nk, Vp);
    const int64_t total = (int64_t)Nkp * (Vp / 4);
    hipLaunchKernelGGL(vq_soft_split_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, rowmax, logsum,
                       Nk, V, 1.f / temp, seed, noise != 0, out, Nkp, Vp);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_vq_soft_bwd2(const float* x, int64_t ldx, const float* rowmax, const float* logsum, const float* t, int64_t ldt, int32_t Nk, int32_t V, int32_t Vpad,
                               float temp, uint32_t seed, int32_t noise, void* dx, int64_t ldd, int32_t out_bf16, float* dtemp_row,
                               void* stream) {
    SC_CHECK(x && rowmax && logsum && t && dx, "sc_vq_soft_bwd2: null pointer");
    VQ_CHECK_ROWS("sc_vq_soft_bwd2");
    SC_CHECK(ldx >= V && ldt >= V && Vpad >= V && ldd >= Vpad && temp > 0.f, "sc_vq_soft_bwd2: ldx=%lld ldt=%lld (>= V=%d) Vpad=%d (>= V) ldd=%lld (>= Vpad) temp=%g (> 0)",
             (long long)ldx, (long long)ldt, V, Vpad, (long long)ldd, (double)temp);
    if (out_bf16)
        hipLaunchKernelGGL(vq_soft_bwd2_kernel<uint16_t>, dim3(Nk), dim3(256), 0, (hipStream_t)stream, x, ldx, rowmax, logsum, t, ldt, V, Vpad,
                           1.f / temp, seed, noise != 0, (uint16_t*)dx, ldd, dtemp_row);
    else
        hipLaunchKernelGGL(vq_soft_bwd2_kernel<float>, dim3(Nk), dim3(256), 0, (hipStream_t)stream, x, ldx, rowmax, logsum, t, ldt, V, Vpad,
                           1.f / temp, seed, noise != 0, (float*)dx, ldd, dtemp_row);
    SC_LAUNCH_CHECK();
    return 0;
}
