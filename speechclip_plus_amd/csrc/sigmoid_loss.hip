// Pairwise sigmoid loss (SigLIP: Zhai et al. 2023) on the gathered batch A [B, E] (speech), Bm [B, E] (image), ids [B] int64 or none:
//   sc_sigmoid_loss_fwd   raw dots s (exact-fp32 MFMA) + the loss scalar and the three pair counts in ONE launch
//   sc_sigmoid_loss_grad  G = gscale t dloss/dx and the rows' d t / d b terms
//     s_ij = <A_i, Bm_j>,  x_ij = fma(t, s_ij, b),  z_ij = +1 if i == j else -1,  same_ij = ids and i != j and ids[i] == ids[j]
//     same_id 0 "ignore": w_ij = 0 where same_ij;  1 "positive": z_ij = +1 where same_ij;  2 "negative": nothing changes
//     loss = (1 / B) sum_ij w_ij softplus(-z_ij x_ij),   g_ij = -(1 / B) w_ij z_ij sigmoid(-z_ij x_ij)
// There is no denominator: every pair is a decision of its own, so a row whose every negative is ignored is legal.
//
// FORWARD = supcon_fwd_kernel's shape (supcon.hip) on the square: each workgroup owns a 64 x 64 tile of the pairs, the operands staged
// through LDS in K-tiles of 64, the product on the matrix pipe in exact fp32 (v_mfma_f32_32x32x2_f32).  The RAW dots are written out (the
// backward forms x from them again: recovering s from x at b = -10 would lose the digits d t needs).  Each lane weighs its 16 pairs
// straight from the accumulator; the tile's sum and its three integer counts (positives, negatives, ignored) meet through lane shuffles
// and LDS in a fixed order.  The workgroup that takes the last ticket merges the tiles' partials in a fixed order into loss[0] and
// counts[3].  No float atomics: the same operands give the same bits on every call.  A pair with w = 0 is never added, so a tile of such
// pairs contributes exactly 0.  Rows at or behind B are never loaded (the loader zero-fills them and the K tail, E % 4 == 0) and their
// pairs are never weighed; their ids are never read.
#include "sc_common.h"

namespace {

constexpr int LT = 68;       // LDS row pitch of the [k][64 rows] operand images (as loss_optim.hip)
constexpr int KTL = 64;      // K-tile of the product
constexpr int64_t MAX_DOT_BYTES = (int64_t)1 << 30;    // s [B, B] fp32: 1 GiB (B <= 16384)

enum { SAME_IGNORE = 0, SAME_POSITIVE = 1, SAME_NEGATIVE = 2 };

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// softplus(u) = log(1 + e^u) with no overflow: for u = 137 the naive form is inf
__device__ __forceinline__ float softplus(float u) { return fmaxf(u, 0.f) + log1pf(expf(-fabsf(u))); }

// sigmoid(v) = 1 / (1 + e^-v) with no overflow on either side
__device__ __forceinline__ float sigmoid(float v) {
    const float e = expf(-fabsf(v));
    return (v >= 0.f ? 1.f : e) / (1.f + e);
}

__global__ __launch_bounds__(256) void sigmoid_fwd_kernel(const float* __restrict__ A, const float* __restrict__ Bm, int B, int E,
                                                          const int64_t* __restrict__ ids, int same_id,
                                                          const float* __restrict__ scale_p, const float* __restrict__ bias_p,
                                                          float* __restrict__ s, float* part, float* __restrict__ loss,
                                                          int* __restrict__ counts, unsigned int* __restrict__ ticket) {
    __shared__ float As[KTL][LT];
    __shared__ float Bs[KTL][LT];
    __shared__ int64_t idl[2][64];       // the id of the tile's rows / columns (no ids, or behind B: the index itself, which no other pair has)
    __shared__ int last_flag;
    __shared__ float red[4];
    __shared__ int redc[3][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, half = lane >> 5;
    const int ti = blockIdx.y, tj = blockIdx.x;
    const int i0 = ti * 64, j0 = tj * 64;
    const float t = scale_p[0], b = bias_p[0];
    if (tid < 128) {
        const int g = (tid < 64 ? i0 : j0) + (tid & 63);
        idl[tid >> 6][tid & 63] = (ids && g < B) ? ids[g] : (int64_t)g;
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int lr = tid >> 2, kq = (tid & 3) * 4;
    float4 ra[4], rb[4];
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = k0 + c * 16 + kq;
            ra[c] = rb[c] = float4{0.f, 0.f, 0.f, 0.f};
            if (k < E) {                           // E % 4 == 0 (checked on the host)
                if (i0 + lr < B) ra[c] = *(const float4*)(A + (int64_t)(i0 + lr) * E + k);
                if (j0 + lr < B) rb[c] = *(const float4*)(Bm + (int64_t)(j0 + lr) * E + k);
            }
        }
    };
    load_tile(0);
    for (int k0 = 0; k0 < E; k0 += KTL) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int kk = c * 16 + kq;
            As[kk + 0][lr] = ra[c].x; As[kk + 1][lr] = ra[c].y; As[kk + 2][lr] = ra[c].z; As[kk + 3][lr] = ra[c].w;
            Bs[kk + 0][lr] = rb[c].x; Bs[kk + 1][lr] = rb[c].y; Bs[kk + 2][lr] = rb[c].z; Bs[kk + 3][lr] = rb[c].w;
        }
        __syncthreads();
        if (k0 + KTL < E) load_tile(k0 + KTL);
#pragma unroll
        for (int kk = 0; kk < KTL; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + half][wm * 32 + l31], Bs[kk + half][wn * 32 + l31], acc, 0, 0, 0);
    }
    // the lane's 16 pairs: raw dot -> global, the weighed term and the counts in register order
    float sum = 0.f;
    int npos = 0, nneg = 0, nign = 0;
    {
        const int cc = wn * 32 + l31, gj = j0 + cc;
        const int64_t idc = idl[1][cc];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const int gi = i0 + rr;
            if (gi < B && gj < B) {
                s[(int64_t)gi * B + gj] = acc[r];
                const float x = fmaf(t, acc[r], b);
                const bool diag = gi == gj;
                const bool same = !diag && idl[0][rr] == idc;          // 64-bit compare; without ids the indices differ
                if (same && same_id == SAME_IGNORE) {
                    ++nign;
                } else if (diag || (same && same_id == SAME_POSITIVE)) {
                    ++npos;
                    sum += softplus(-x);
                } else {
                    ++nneg;
                    sum += softplus(x);
                }
            }
        }
    }
    sum = wave_sum(sum);
    npos = wave_sum_i(npos); nneg = wave_sum_i(nneg); nign = wave_sum_i(nign);
    if (lane == 0) { red[wave] = sum; redc[0][wave] = npos; redc[1][wave] = nneg; redc[2][wave] = nign; }
    __syncthreads();
    const unsigned total = gridDim.x * gridDim.y;
    float* pl = part;                                    // [total] the tiles' sums
    int* pc = (int*)(part + total);                      // [3][total] the tiles' counts
    if (tid == 0) {
        const float ts = (red[0] + red[1]) + (red[2] + red[3]);
        const int c0 = redc[0][0] + redc[0][1] + redc[0][2] + redc[0][3];
        const int c1 = redc[1][0] + redc[1][1] + redc[1][2] + redc[1][3];
        const int c2 = redc[2][0] + redc[2][1] + redc[2][2] + redc[2][3];
        if (total == 1) {                                // one tile: it is the result, no ticket
            loss[0] = ts / (float)B;
            counts[0] = c0; counts[1] = c1; counts[2] = c2;
        } else {
            const unsigned tile = ti * gridDim.x + tj;
            pl[tile] = ts;
            pc[tile] = c0; pc[total + tile] = c1; pc[2 * total + tile] = c2;
        }
    }
    if (total == 1) return;
    // ---- ticket: the last workgroup to arrive merges (loss_optim.hip's protocol)
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const unsigned tk = atomicAdd(ticket, 1u);
        last_flag = (tk == total - 1);
        if (tk == total - 1) *ticket = 0;               // ready for the next launch on this stream
    }
    __syncthreads();
    if (!last_flag) return;
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // thread tid takes tiles tid, tid + 256, ... in order; then the wave tree and the four waves: a fixed order for a given B
    float ms = 0.f;
    int m0 = 0, m1 = 0, m2 = 0;
    for (unsigned q = tid; q < total; q += 256) {
        ms += pl[q];
        m0 += pc[q]; m1 += pc[total + q]; m2 += pc[2 * total + q];
    }
    ms = wave_sum(ms);
    m0 = wave_sum_i(m0); m1 = wave_sum_i(m1); m2 = wave_sum_i(m2);
    if (lane == 0) { red[wave] = ms; redc[0][wave] = m0; redc[1][wave] = m1; redc[2][wave] = m2; }
    __syncthreads();
    if (tid == 0) {
        loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) / (float)B;
        counts[0] = redc[0][0] + redc[0][1] + redc[0][2] + redc[0][3];
        counts[1] = redc[1][0] + redc[1][1] + redc[1][2] + redc[1][3];
        counts[2] = redc[2][0] + redc[2][1] + redc[2][2] + redc[2][3];
    }
}

// one workgroup per row i:  G[i, j] = gscale t g_ij,  dscale_part[i] = gscale sum_j g_ij s_ij,  dbias_part[i] = gscale sum_j g_ij
__global__ __launch_bounds__(256) void sigmoid_grad_kernel(const float* __restrict__ s, int B, const int64_t* __restrict__ ids,
                                                           int same_id, const float* __restrict__ gscale,
                                                           const float* __restrict__ scale_p, const float* __restrict__ bias_p,
                                                           float* __restrict__ G, float* __restrict__ dscale_part,
                                                           float* __restrict__ dbias_part) {
    __shared__ float red[2][4];
    const int i = blockIdx.x;
    const float t = scale_p[0], b = bias_p[0], gs = gscale[0];
    const float inv_b = 1.f / (float)B;
    const int64_t idi = ids ? ids[i] : 0;
    float ds = 0.f, db = 0.f;
    for (int j = threadIdx.x; j < B; j += 256) {
        const float sv = s[(int64_t)i * B + j];
        const float x = fmaf(t, sv, b);
        const bool diag = j == i;
        const bool same = ids && !diag && ids[j] == idi;
        float g = 0.f;
        if (!(same && same_id == SAME_IGNORE)) {
            const float z = (diag || (same && same_id == SAME_POSITIVE)) ? 1.f : -1.f;
            g = -inv_b * z * sigmoid(-z * x);
            ds += g * sv;
            db += g;
        }
        G[(int64_t)i * B + j] = (g * t) * gs;
    }
    ds = wave_sum(ds);
    db = wave_sum(db);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = ds; red[1][threadIdx.x >> 6] = db; }
    __syncthreads();
    if (threadIdx.x == 0) {
        dscale_part[i] = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) * gs;
        dbias_part[i] = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) * gs;
    }
}

// the checks every entry point shares, before any HIP call
int sigmoid_shape(const char* who, int32_t B) {
    SC_CHECK(B >= 1, "%s: B >= 1 (B=%d)", who, B);
    return 0;
}

int sigmoid_limit(const char* who, int32_t B) {
    SC_CHECK((int64_t)B * B * 4 <= MAX_DOT_BYTES, "%s: the dots [B=%d, B] fp32 take %lld bytes, above the limit of %lld (1 GiB)", who, B,
             (long long)B * B * 4, (long long)MAX_DOT_BYTES);
    return 0;
}

}  // namespace

extern "C" int64_t sc_sigmoid_loss_workspace_floats(int32_t B) {
    if (sigmoid_shape("sc_sigmoid_loss_workspace_floats", B) < 0 || sigmoid_limit("sc_sigmoid_loss_workspace_floats", B) < 0) return -1;
    const int64_t nt = (B + 63) / 64;
    return 4 * nt * nt + 4;             // per tile the sum and three counts; the ticket word (+ padding)
}

extern "C" int sc_sigmoid_loss_fwd(const float* A, const float* Bm, int32_t B, int32_t E, const int64_t* ids, int32_t same_id,
                                   const float* scale, const float* bias, float* s, float* loss, int32_t* counts, float* workspace,
                                   void* stream) {
    if (sigmoid_shape("sc_sigmoid_loss_fwd", B) < 0) return -1;
    SC_CHECK(E > 0 && E % 4 == 0, "sc_sigmoid_loss_fwd: E=%d > 0 (E %% 4)", E);
    SC_CHECK(same_id >= 0 && same_id <= 2, "sc_sigmoid_loss_fwd: same_id=%d is none of 0 (ignore), 1 (positive), 2 (negative)", same_id);
    if (sigmoid_limit("sc_sigmoid_loss_fwd", B) < 0) return -1;
    SC_CHECK(A && Bm && scale && bias && s && loss && counts && workspace, "sc_sigmoid_loss_fwd: null pointer");
    SC_CHECK(((uintptr_t)A & 15) == 0 && ((uintptr_t)Bm & 15) == 0, "sc_sigmoid_loss_fwd: A and Bm must be 16-byte aligned");
    const int nt = (B + 63) / 64;
    unsigned int* ticket = (unsigned int*)(workspace + (int64_t)4 * nt * nt);   // zero before the first launch; every launch leaves it zero
    hipLaunchKernelGGL(sigmoid_fwd_kernel, dim3(nt, nt), dim3(256), 0, (hipStream_t)stream, A, Bm, B, E, ids, same_id, scale, bias, s,
                       workspace, loss, counts, ticket);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_sigmoid_loss_grad(const float* s, int32_t B, const int64_t* ids, int32_t same_id, const float* gscale,
                                    const float* scale, const float* bias, float* G, float* dscale_part, float* dbias_part,
                                    void* stream) {
    if (sigmoid_shape("sc_sigmoid_loss_grad", B) < 0) return -1;
    SC_CHECK(same_id >= 0 && same_id <= 2, "sc_sigmoid_loss_grad: same_id=%d is none of 0 (ignore), 1 (positive), 2 (negative)", same_id);
    if (sigmoid_limit("sc_sigmoid_loss_grad", B) < 0) return -1;
    SC_CHECK(s && gscale && scale && bias && G && dscale_part && dbias_part, "sc_sigmoid_loss_grad: null pointer");
    hipLaunchKernelGGL(sigmoid_grad_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, s, B, ids, same_id, gscale, scale, bias, G,
                       dscale_part, dbias_part);
    SC_LAUNCH_CHECK();
    return 0;
}
