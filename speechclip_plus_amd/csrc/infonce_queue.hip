// A cross-batch negative queue beside the batch: BOTH denominators of the masked contrastive loss (loss_optim.hip) extended by the rows
// of a ring of past embeddings - queue_B (images) for the speech anchors, queue_A (speech) for the image anchors.  The two [Bg, Nq] dot
// products come from the exact-fp32 GEMM (sc_sgemm_mfma_f32, one per enabled side) into buffers that these kernels then own:
//   sc_infonce_queue_fwd   x[i, q] <- inv_temp x[i, q] where the entry is ADMITTED, -inf elsewhere, in place; used[i]; the extended
//                          lse_row[i] = log(e^{lse_row_i} + sum_q e^{xA_iq}), lse_col[j] likewise from xB; the loss from both and the diagonal
//   sc_infonce_queue_grad  x <- w = c inv_temp e^{x - lse_ext} in place (dA += w_A . queue_B, dB += w_B . queue_A on the GEMM afterwards);
//                          dot_i += c sum_q p x / inv_temp over both sides
// Entry (i, q) is admitted iff there are no ids or queue_ids[q] != ids[i] (avssl/module/losses.py:207's rule over more columns): a queued
// item is a false negative only for the anchor that carries its id.  The extras carry no margin; a direction that is off forms none.
//
// Shape of the work.  Both are streaming passes over the scores: 4 bytes read and written per entry, 16 bytes per lane per access; the
// queue's ids (8 bytes per column, the same for every anchor) come out of L2.  Forward: one workgroup per (anchor, chunk of 1024 .. 4096
// columns, side), the chunk in registers, a (max, sum exp, count) partial per chunk; a second small launch merges the chunks in chunk
// order and recomputes the loss in infonce_fwd_kernel's order, so with no entry admitted every output is the plain call's bits.  Backward:
// one workgroup per anchor, waves 0 - 3 on side A and 4 - 7 on side B, columns in a fixed stride order, the eight wave sums added in wave
// order.  No float atomics, no workspace shared between workgroups: two calls give the same bits.  The chunk length depends on (Bg, Nq)
// alone, never on the device, so every rank of a data-parallel step gets the same statistics.
#include "sc_common.h"
#include "speechclip_hip_queue.h"

namespace {

constexpr int64_t QUEUE_MAX_SCORES = (int64_t)1 << 26;    // Bg Nq per side: 256 MiB of fp32 scores (ops.QUEUE_MAX_SCORES)

// columns per workgroup of the forward: 4096, halved down to 1024 (one 16-byte piece per thread) while the grid stays under 512
// workgroups per side.  A function of (Bg, Nq) only.
inline int queue_chunk(int Bg, int Nq) {
    int chunk = 4096;
    while (chunk > 1024 && (int64_t)Bg * ((Nq + chunk - 1) / chunk) < 512) chunk >>= 1;
    return chunk;
}
inline int queue_slabs(int Bg, int Nq) { return (Nq + queue_chunk(Bg, Nq) - 1) / queue_chunk(Bg, Nq); }

// blockIdx.z = 0 works on x0 / part0, 1 on x1 / part1 (the host puts the enabled sides there); the anchors' ids are the batch's on
// either side
__global__ __launch_bounds__(256) void infonce_queue_fwd_kernel(float* __restrict__ x0, float* __restrict__ x1, int64_t ldx,
                                                                const int64_t* __restrict__ ids, const int64_t* __restrict__ queue_ids,
                                                                const float* __restrict__ inv_temp_p, int Nq, int chunk,
                                                                float* __restrict__ part0, float* __restrict__ part1) {
    __shared__ float redm[4], reds[4];
    __shared__ int redc[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    float* xr = (blockIdx.z ? x1 : x0) + (int64_t)i * ldx;
    float* part = blockIdx.z ? part1 : part0;
    const float it = inv_temp_p[0];
    const int64_t idi = ids ? ids[i] : 0;
    const int c0 = s * chunk;
    f32x4 v[4];
    float tm = -INFINITY;
    int cnt = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int col = c0 + (p * 256 + tid) * 4;            // col % 4 == 0 and ldx % 4 == 0: a piece that starts inside Nq ends inside ldx
        const bool in = p * 1024 < chunk && col < Nq;
        v[p] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (in) {
            const f32x4 raw = *(const f32x4*)(xr + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bool adm = col + e < Nq;                     // the pad columns of the last piece are written as -inf
                if (ids && adm) adm = queue_ids[col + e] != idi;
                v[p][e] = adm ? raw[e] * it : -INFINITY;
                cnt += adm ? 1 : 0;
                tm = fmaxf(tm, v[p][e]);
            }
            *(f32x4*)(xr + col) = v[p];
        }
    }
    tm = wave_max(tm);
    if (lane == 0) redm[wave] = tm;
    __syncthreads();
    const float m = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
    float sum = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) sum += v[p][e] == -INFINITY ? 0.f : __expf(v[p][e] - m);
    sum = wave_sum(sum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) { reds[wave] = sum; redc[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
        float* p = part + ((int64_t)i * S + s) * 3;
        p[0] = m;
        p[1] = (reds[0] + reds[1]) + (reds[2] + reds[3]);
        p[2] = (float)((redc[0] + redc[1]) + (redc[2] + redc[3]));      // <= 4096: exact
    }
}

// one anchor's chunks added to its plain statistic in chunk order (infonce_neg_merge_kernel's arithmetic); no entry admitted: lr itself
__device__ __forceinline__ float queue_extend(const float* __restrict__ p, int S, float lr, int* used) {
    float m = lr;
    int cnt = 0;
    for (int s = 0; s < S; ++s) {
        m = fmaxf(m, p[3 * s]);
        cnt += (int)p[3 * s + 2];
    }
    float sum = lr == -INFINITY ? 0.f : __expf(lr - m);
    for (int s = 0; s < S; ++s) {
        const float pm = p[3 * s];
        sum += pm == -INFINITY ? p[3 * s + 1] : p[3 * s + 1] * __expf(pm - m);     // no finite entry: the sum is 0, or the NaN of a NaN entry
    }
    *used = cnt;
    return cnt == 0 ? lr : m + __logf(sum);
}

// the loss in infonce_fwd_kernel's order (thread tid takes rows tid, tid + 256, ..., row term before column term, wave tree,
// (w0 + w1) + (w2 + w3)): with used == 0 everywhere the plain call's bits.  partA / partB NULL: that side has no extras.
__global__ __launch_bounds__(256) void infonce_queue_merge_kernel(const float* __restrict__ partA, const float* __restrict__ partB, int S,
                                                                  const float* __restrict__ lse_row, const float* __restrict__ lse_col,
                                                                  const float* __restrict__ logits, int Bg, int a2b, int b2a,
                                                                  float* __restrict__ lse_row_ext, float* __restrict__ lse_col_ext,
                                                                  int32_t* __restrict__ used_A, int32_t* __restrict__ used_B,
                                                                  float* __restrict__ loss) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float term = 0.f;
    for (int i = tid; i < Bg; i += 256) {
        float lrow = lse_row[i], lcol = lse_col[i];
        int ua = 0, ub = 0;
        if (partA) lrow = queue_extend(partA + (int64_t)i * S * 3, S, lrow, &ua);
        if (partB) lcol = queue_extend(partB + (int64_t)i * S * 3, S, lcol, &ub);
        lse_row_ext[i] = lrow;
        lse_col_ext[i] = lcol;
        used_A[i] = ua;
        used_B[i] = ub;
        const float d = logits[(int64_t)i * Bg + i];
        if (a2b) term += lrow - d;
        if (b2a) term += lcol - d;
    }
    term = wave_sum(term);
    if (lane == 0) red[wave] = term;
    __syncthreads();
    if (tid == 0) loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) / ((float)Bg * (float)((a2b && b2a) ? 2 : 1));
}

// waves 0 - 3: side A (xA, lse_row_ext), waves 4 - 7: side B (xB, lse_col_ext); a NULL side contributes nothing
__global__ __launch_bounds__(512) void infonce_queue_grad_kernel(float* __restrict__ xA, float* __restrict__ xB, int64_t ldx,
                                                                 const float* __restrict__ lse_row_ext, const float* __restrict__ lse_col_ext,
                                                                 const float* __restrict__ gscale, const float* __restrict__ inv_temp_p,
                                                                 int Bg, int Nq, int ndir, float* __restrict__ dot) {
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, t = tid & 255;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = blockIdx.x;
    float* xb = wave < 4 ? xA : xB;
    const float it = inv_temp_p[0];
    const float gs = gscale[0] / ((float)Bg * (float)ndir);
    const float git = gs * it;
    float dsum = 0.f;
    if (xb) {
        float* xr = xb + (int64_t)i * ldx;
        const float lse = wave < 4 ? lse_row_ext[i] : lse_col_ext[i];
        for (int c0 = t * 4; c0 < Nq; c0 += 4096) {                      // four pieces in flight per thread
            f32x4 v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int col = c0 + p * 1024;
                v[p] = col < Nq ? *(const f32x4*)(xr + col) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int col = c0 + p * 1024;
                f32x4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool fin = !(v[p][e] == -INFINITY);             // -inf marks the entries that were not admitted (and the pad columns)
                    const float pr = fin ? __expf(v[p][e] - lse) : 0.f;
                    dsum += fin ? pr * v[p][e] : 0.f;
                    w[e] = fin ? git * pr : 0.f;
                }
                if (col < Nq) *(f32x4*)(xr + col) = w;
            }
        }
    }
    dsum = wave_sum(dsum);
    if (lane == 0) red[wave] = dsum;
    __syncthreads();
    if (tid == 0) dot[i] = dot[i] + gs * (((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]))) / it;
}

}  // namespace

extern "C" int sc_infonce_queue_workspace_floats(int32_t Bg, int32_t Nq) {
    if (Bg <= 0 || Nq <= 0) return 0;
    SC_CHECK((int64_t)Bg * Nq <= QUEUE_MAX_SCORES, "sc_infonce_queue_workspace_floats: Bg Nq = %lld scores per side, at most 2^26 are served",
             (long long)Bg * Nq);
    return 2 * 3 * Bg * queue_slabs(Bg, Nq);                 // Bg slabs <= 2^26 / 1024 + Bg <= 2^26 + 2^16: within int
}

extern "C" int sc_infonce_queue_fwd(float* x_A, float* x_B, int64_t ldx, const int64_t* ids, const int64_t* queue_ids, const float* inv_temp,
                                    const float* lse_row, const float* lse_col, const float* logits, int32_t Bg, int32_t E, int32_t Nq,
                                    int32_t a2b, int32_t b2a, float* lse_row_ext, float* lse_col_ext, int32_t* used_A, int32_t* used_B,
                                    float* loss, float* workspace, void* stream) {
    SC_CHECK(Bg >= 0 && E > 0 && E % 4 == 0, "sc_infonce_queue_fwd: Bg=%d >= 0, E=%d > 0 (E %% 4)", Bg, E);
    SC_CHECK(Nq >= 0 && (int64_t)Bg * Nq <= QUEUE_MAX_SCORES, "sc_infonce_queue_fwd: 0 <= Nq and Bg Nq <= 2^26 scores per side (Bg=%d Nq=%d)", Bg,
             Nq);
    SC_CHECK(ldx >= Nq && ldx % 4 == 0, "sc_infonce_queue_fwd: ldx=%lld >= Nq, 16-byte rows (ldx %% 4)", (long long)ldx);
    SC_CHECK(a2b || b2a, "sc_infonce_queue_fwd: a2b | b2a");
    SC_CHECK((ids == nullptr) == (queue_ids == nullptr), "sc_infonce_queue_fwd: ids and queue_ids come together or not at all");
    if (Bg == 0 || Nq == 0) return 0;
    SC_CHECK((x_A || !a2b) && (x_B || !b2a) && inv_temp && lse_row && lse_col && logits && lse_row_ext && lse_col_ext && used_A && used_B && loss &&
                 workspace,
             "sc_infonce_queue_fwd: null pointer");
    SC_CHECK(((uintptr_t)x_A & 15) == 0 && ((uintptr_t)x_B & 15) == 0, "sc_infonce_queue_fwd: x_A / x_B must be 16-byte aligned");
    const int chunk = queue_chunk(Bg, Nq), S = queue_slabs(Bg, Nq);
    float* partA = a2b ? workspace : nullptr;
    float* partB = b2a ? workspace + (int64_t)3 * Bg * S : nullptr;
    const bool both = a2b && b2a;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(infonce_queue_fwd_kernel, dim3(Bg, S, both ? 2 : 1), dim3(256), 0, st, a2b ? x_A : x_B, x_B, ldx, ids, queue_ids, inv_temp,
                       Nq, chunk, a2b ? partA : partB, partB);
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(infonce_queue_merge_kernel, dim3(1), dim3(256), 0, st, partA, partB, S, lse_row, lse_col, logits, Bg, a2b, b2a, lse_row_ext,
                       lse_col_ext, used_A, used_B, loss);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_infonce_queue_grad(float* x_A, float* x_B, int64_t ldx, const float* lse_row_ext, const float* lse_col_ext, const float* gscale,
                                     const float* inv_temp, int32_t Bg, int32_t Nq, int32_t a2b, int32_t b2a, float* dlogit_dot, void* stream) {
    SC_CHECK(Bg >= 0 && Nq >= 0 && (int64_t)Bg * Nq <= QUEUE_MAX_SCORES, "sc_infonce_queue_grad: 0 <= Nq and Bg Nq <= 2^26 scores per side (Bg=%d Nq=%d)",
             Bg, Nq);
    SC_CHECK(ldx >= Nq && ldx % 4 == 0, "sc_infonce_queue_grad: ldx=%lld >= Nq, 16-byte rows (ldx %% 4)", (long long)ldx);
    SC_CHECK(a2b || b2a, "sc_infonce_queue_grad: a2b | b2a");
    if (Bg == 0 || Nq == 0) return 0;
    SC_CHECK((x_A || !a2b) && (x_B || !b2a) && lse_row_ext && lse_col_ext && gscale && inv_temp && dlogit_dot, "sc_infonce_queue_grad: null pointer");
    SC_CHECK(((uintptr_t)x_A & 15) == 0 && ((uintptr_t)x_B & 15) == 0, "sc_infonce_queue_grad: x_A / x_B must be 16-byte aligned");
    hipLaunchKernelGGL(infonce_queue_grad_kernel, dim3(Bg), dim3(512), 0, (hipStream_t)stream, a2b ? x_A : nullptr, b2a ? x_B : nullptr, ldx,
                       lse_row_ext, lse_col_ext, gscale, inv_temp, Bg, Nq, (a2b && b2a) ? 2 : 1, dlogit_dot);
    SC_LAUNCH_CHECK();
    return 0;
}
