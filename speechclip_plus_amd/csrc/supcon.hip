// Supervised contrastive loss (Khosla et al.; avssl/module/losses.py:8-123) on the contrast rows C [N, E] = cat(unbind(features, 1), 0):
// row r is view r / bsz of sample r % bsz, anchors are rows 0 .. Na - 1.
//   sc_supcon_fwd   logits (exact-fp32 MFMA) + the rows' log-sum-exp over the kept columns, sum w l, sum w + the loss scalar in ONE launch
//   sc_supcon_grad  G = inv_temp gscale dloss/dlogits and the d inv_temp terms
//     l_ij = inv_temp <C_i, C_j>,  keep_ij = [j != i],  w_ij = W[i % bsz, j % bsz] keep_ij,  lse_i = log sum_j keep_ij e^{l_ij},  s_i = sum_j w_ij
//     loss = -(1 / base_temperature) / Na sum_i [ sum_j w_ij l_ij / s_i - lse_i ]
// W is [labels_a == labels_b] (64-bit compare), the caller's float mask [bsz, bsz] (asymmetric, any weights), or the identity.
//
// FORWARD = infonce_fwd_kernel's shape (loss_optim.hip) on a rectangle: each workgroup owns a 64 x 64 tile of the [Na, N] logits, both
// operands rows of C staged through LDS in K-tiles of 64, the product on the matrix pipe in exact fp32 (v_mfma_f32_32x32x2_f32), the scaled
// tile written out (the backward reads it).  Four threads share a tile row: each takes 16 columns, the row's (max, sum exp, sum w l, sum w)
// over the kept columns meet through lane shuffles in a fixed order and go to the tile's partials.  The workgroup that takes the last ticket
// merges the partials of all column tiles in tile order into lse / possum / poscnt and the scalar loss.  No float atomics: the same operands
// give the same bits on every call.  The maximum subtracted before exp is the one over the kept columns (the reference's includes the
// self column; the difference cancels).  s_i = 0 gives 0 / 0: a NaN loss, as the reference's.  Rows of C at or behind N (and behind Na on
// the anchor side) are never loaded; K-tails are zero-filled by the loader (E % 4 == 0).
#include "sc_common.h"

namespace {

constexpr int LT = 68;       // LDS row pitch of the [k][64 rows] operand images (as loss_optim.hip)
constexpr int KTL = 64;      // K-tile of the logits product

__global__ __launch_bounds__(256) void supcon_fwd_kernel(const float* __restrict__ C, int N, int Na, int bsz, int E,
                                                         const int64_t* __restrict__ labels, const float* __restrict__ mask,
                                                         const float* __restrict__ inv_temp_p, float neg_inv_bt,
                                                         float* __restrict__ logits, float* __restrict__ part, float* __restrict__ lse,
                                                         float* __restrict__ possum, float* __restrict__ poscnt, float* __restrict__ loss,
                                                         unsigned int* __restrict__ ticket) {
    __shared__ float As[KTL][LT];
    __shared__ float Bs[KTL][LT];
    __shared__ float Ls[64][65];
    __shared__ int64_t idl[2][64];       // the label of the row's / column's sample (no labels: the sample's index)
    __shared__ int sb[2][64];            // the sample's index r % bsz (the mask's row / column)
    __shared__ int last_flag;
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, half = lane >> 5;
    const int nt = gridDim.x;
    const int ti = blockIdx.y, tj = blockIdx.x;
    const int i0 = ti * 64, j0 = tj * 64;
    const float it = inv_temp_p[0];
    if (tid < 128) {                     // g % bsz < bsz for every g: the label read is in range on tile rows behind Na / N too
        const int b = ((tid < 64 ? i0 : j0) + (tid & 63)) % bsz;
        sb[tid >> 6][tid & 63] = b;
        idl[tid >> 6][tid & 63] = labels ? labels[b] : (int64_t)b;
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
                if (i0 + lr < Na) ra[c] = *(const float4*)(C + (int64_t)(i0 + lr) * E + k);
                if (j0 + lr < N) rb[c] = *(const float4*)(C + (int64_t)(j0 + lr) * E + k);
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
    // scaled tile -> LDS (+ global)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rr = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, cc = wn * 32 + l31;
        const int gi = i0 + rr, gj = j0 + cc;
        const float l = acc[r] * it;
        Ls[rr][cc] = l;
        if (gi < Na && gj < N) logits[(int64_t)gi * N + gj] = l;
    }
    __syncthreads();
    // per-tile row partials over the kept columns: four adjacent lanes per row, 16 columns each (no lane leaves before the shuffles)
    float* prm = part;                                   // [nt][Na] row max     (indexed by column tile)
    float* prs = part + (int64_t)nt * Na;                // sum exp(l - max)
    float* ppl = part + (int64_t)2 * nt * Na;            // sum w l
    float* ppw = part + (int64_t)3 * nt * Na;            // sum w
    {
        const int row = tid >> 2, c0 = (tid & 3) * 16;
        const int gi = i0 + row;
        const bool row_in = gi < Na;
        const int64_t idr = idl[0][row];
        const int64_t mrow = (int64_t)sb[0][row] * bsz;
        float m = -INFINITY;
        for (int c = c0; c < c0 + 16; ++c) {
            const int gj = j0 + c;
            if (row_in && gj < N && gj != gi) m = fmaxf(m, Ls[row][c]);
        }
        m = fmaxf(m, __shfl_xor(m, 1));
        m = fmaxf(m, __shfl_xor(m, 2));
        float sum = 0.f, pl = 0.f, pw = 0.f;
        for (int c = c0; c < c0 + 16; ++c) {
            const int gj = j0 + c;
            if (row_in && gj < N && gj != gi) {
                const float l = Ls[row][c];
                const float w = mask ? mask[mrow + sb[1][c]] : (idl[1][c] == idr ? 1.f : 0.f);
                sum += __expf(l - m);
                pl += w * l;
                pw += w;
            }
        }
        sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2);
        pl += __shfl_xor(pl, 1);   pl += __shfl_xor(pl, 2);
        pw += __shfl_xor(pw, 1);   pw += __shfl_xor(pw, 2);
        if (row_in && (tid & 3) == 0) {
            const int64_t o = (int64_t)tj * Na + gi;
            prm[o] = m; prs[o] = sum; ppl[o] = pl; ppw[o] = pw;
        }
    }
    // ---- ticket: the last workgroup to arrive finalises (loss_optim.hip's protocol).  A single-tile launch is its own last arriver.
    if (gridDim.x * gridDim.y > 1) {
        __threadfence();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            const unsigned total = gridDim.x * gridDim.y;
            const unsigned t = atomicAdd(ticket, 1u);
            last_flag = (t == total - 1);
            if (t == total - 1) *ticket = 0;            // ready for the next launch on this stream
        }
        __syncthreads();
        if (!last_flag) return;
        __threadfence();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    float term = 0.f;
    for (int i = tid; i < Na; i += 256) {
        float mr = -INFINITY;
        for (int t = 0; t < nt; ++t) mr = fmaxf(mr, prm[(int64_t)t * Na + i]);
        float sr = 0.f, pl = 0.f, pw = 0.f;
        for (int t = 0; t < nt; ++t) {
            const float pm = prm[(int64_t)t * Na + i];
            if (pm > -INFINITY) sr += prs[(int64_t)t * Na + i] * __expf(pm - mr);
            pl += ppl[(int64_t)t * Na + i];
            pw += ppw[(int64_t)t * Na + i];
        }
        const float lrow = mr + __logf(sr);             // no kept column (N = 1): log 0 = -inf, as the reference
        lse[i] = lrow;
        possum[i] = pl;
        poscnt[i] = pw;
        term += pl / pw - lrow;                         // no positive: 0 / 0, the reference's NaN
    }
    term = wave_sum(term);
    if (lane == 0) red[wave] = term;
    __syncthreads();
    if (tid == 0) loss[0] = neg_inv_bt * (((red[0] + red[1]) + (red[2] + red[3])) / (float)Na);
}

// G[i,j] = inv_temp gscale g_ij,  g_ij = -(w_ij / s_i - keep_ij e^{l_ij - lse_i}) / (base_temperature Na);
// dlogit_dot[i] = gscale sum_j g_ij l_ij / inv_temp  ->  d loss / d inv_temp = sum_i dlogit_dot[i]
__global__ __launch_bounds__(256) void supcon_grad_kernel(const float* __restrict__ logits, const float* __restrict__ lse,
                                                          const float* __restrict__ poscnt, int N, int Na, int bsz,
                                                          const int64_t* __restrict__ labels, const float* __restrict__ mask,
                                                          const float* __restrict__ gscale, const float* __restrict__ inv_temp_p,
                                                          float inv_bt, float* __restrict__ G, float* __restrict__ dlogit_dot) {
    __shared__ float red[4];
    const int i = blockIdx.x;
    const int ib = i % bsz;
    const int64_t idi = labels ? labels[ib] : (int64_t)ib;
    const float* mrow = mask ? mask + (int64_t)ib * bsz : nullptr;
    const float lr = lse[i];
    const float rs = 1.f / poscnt[i];
    const float it = inv_temp_p[0];
    const float coef = -gscale[0] * inv_bt / (float)Na;
    float dot = 0.f;
    for (int j = threadIdx.x; j < N; j += 256) {
        const float l = logits[(int64_t)i * N + j];
        const int jb = j % bsz;
        float w = 0.f, p = 0.f;
        if (j != i) {
            w = mrow ? mrow[jb] : ((labels ? labels[jb] : (int64_t)jb) == idi ? 1.f : 0.f);
            p = __expf(l - lr);
        }
        const float g = coef * (w * rs - p);
        G[(int64_t)i * N + j] = g * it;
        dot += g * l;
    }
    dot = wave_sum(dot);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0) dlogit_dot[i] = ((red[0] + red[1]) + (red[2] + red[3])) / it;
}

// the checks both entry points share; 1: nothing to launch
int supcon_shape(const char* who, int32_t N, int32_t Na, int32_t bsz) {
    SC_CHECK(N >= 0 && Na >= 0 && Na <= N, "%s: 0 <= Na <= N (Na=%d, N=%d)", who, Na, N);
    SC_CHECK(N == 0 || (bsz > 0 && N % bsz == 0), "%s: N=%d must be a whole number of views of bsz=%d > 0 samples", who, N, bsz);
    SC_CHECK((int64_t)Na * N * 4 <= (int64_t)SC_SUPCON_MAX_LOGIT_BYTES,
             "%s: the logits [Na=%d, N=%d] fp32 take %lld bytes, above the limit of %lld (1 GiB)", who, Na, N, (long long)Na * N * 4,
             (long long)SC_SUPCON_MAX_LOGIT_BYTES);
    return (N == 0 || Na == 0) ? 1 : 0;
}

}  // namespace

extern "C" int64_t sc_supcon_workspace_floats(int32_t Na, int32_t N) {
    const int s = supcon_shape("sc_supcon_workspace_floats", N, Na, 1);
    if (s != 0) return s < 0 ? -1 : 0;
    const int64_t nt = (N + 63) / 64;
    return 4 * nt * Na + 4;             // per-tile row partials, ticket word (+ padding)
}

extern "C" int sc_supcon_fwd(const float* C, int32_t N, int32_t Na, int32_t bsz, int32_t E, const int64_t* labels, const float* mask,
                             const float* inv_temp, float base_temperature, float* logits, float* lse, float* possum, float* poscnt,
                             float* loss, float* workspace, void* stream) {
    const int s = supcon_shape("sc_supcon_fwd", N, Na, bsz);
    if (s < 0) return -1;
    SC_CHECK(E > 0 && E % 4 == 0, "sc_supcon_fwd: E=%d > 0 (E %% 4)", E);
    SC_CHECK(!(labels && mask), "sc_supcon_fwd: labels and mask are both given - one of them or neither");
    SC_CHECK(base_temperature != 0.f, "sc_supcon_fwd: base_temperature is 0");
    if (s == 1) return 0;
    SC_CHECK(C && inv_temp && logits && lse && possum && poscnt && loss && workspace, "sc_supcon_fwd: null pointer");
    SC_CHECK(((uintptr_t)C & 15) == 0, "sc_supcon_fwd: C must be 16-byte aligned");
    const int ntj = (N + 63) / 64, nti = (Na + 63) / 64;
    unsigned int* ticket = (unsigned int*)(workspace + (int64_t)4 * ntj * Na);   // zero before the first launch; every launch leaves it zero
    hipLaunchKernelGGL(supcon_fwd_kernel, dim3(ntj, nti), dim3(256), 0, (hipStream_t)stream, C, N, Na, bsz, E, labels, mask, inv_temp,
                       -1.f / base_temperature, logits, workspace, lse, possum, poscnt, loss, ticket);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_supcon_grad(const float* logits, const float* lse, const float* poscnt, int32_t N, int32_t Na, int32_t bsz,
                              const int64_t* labels, const float* mask, const float* gscale, const float* inv_temp,
                              float base_temperature, float* G, float* dlogit_dot, void* stream) {
    const int s = supcon_shape("sc_supcon_grad", N, Na, bsz);
    if (s < 0) return -1;
    SC_CHECK(!(labels && mask), "sc_supcon_grad: labels and mask are both given - one of them or neither");
    SC_CHECK(base_temperature != 0.f, "sc_supcon_grad: base_temperature is 0");
    if (s == 1) return 0;
    SC_CHECK(logits && lse && poscnt && gscale && inv_temp && G && dlogit_dot, "sc_supcon_grad: null pointer");
    hipLaunchKernelGGL(supcon_grad_kernel, dim3(Na), dim3(256), 0, (hipStream_t)stream, logits, lse, poscnt, N, Na, bsz, labels, mask,
                       gscale, inv_temp, 1.f / base_temperature, G, dlogit_dot);
    SC_LAUNCH_CHECK();
    return 0;
}
