// Mined negatives beside the batch: the speech -> image denominator of the masked contrastive loss (loss_optim.hip) extended by, per
// anchor, a list of rows gathered from a constant bank.
//   sc_infonce_neg_fwd   x[i, n] = inv_temp <A_i, bank[neg_idx[i, n]]> for the slots that take part, -inf elsewhere; used[i]; the
//                        extended lse_row[i] = log(e^{lse_row_i} + sum_n e^{x_in}); the loss scalar from it, lse_col and the diagonal
//   sc_infonce_neg_grad  dA_i += c inv_temp sum_n p_in bank[r_in],  dot_i += c sum_n p_in x_in / inv_temp,  p_in = e^{x_in - lse_row_i}
// Slot (i, n) with r = neg_idx[i, n] TAKES PART iff 0 <= r < N and (ids given) bank_ids[r] equals the id of NO row of the batch: the
// -1 tails of a short list, any other out-of-range value, the false negative (the anchor's own id) and the duplicate (an image that
// already stands in the batch) are empty slots.  A slot that does not take part contributes through a SELECT: its bank row is never
// loaded (no address is formed from an unchecked r), so nothing behind it - a NaN row included - can reach an output.
//
// Shape of the work.  Forward: one wave per gathered row, lanes across E in 16-byte pieces, the anchor row in registers, four rows in
// flight per wave (kwpool.hip's kw_scores_kernel with an index in front).  The slots of an anchor are cut into chunks of 16 .. 64, one
// workgroup per (anchor, chunk) - at Bg = 64 one workgroup per anchor would leave three quarters of the CUs idle - and each leaves a
// (max, sum exp, count) partial; a second small launch merges the chunks in chunk order and recomputes the loss in the plain kernel's
// order, so with no slot taking part lse_row and the loss are the plain call's bits.  Backward: one workgroup per (anchor, 256 columns
// of E); a lane owns four columns and adds its waves' rows in slot order, the four waves merge through LDS in wave order - no
// workspace, no cross-workgroup sum.  No float atomics anywhere: two calls give the same bits.  The chunk length depends on (Bg, M)
// alone, never on the device, so every rank of a data-parallel step gets the same gradient.
#include "sc_common.h"

namespace {

constexpr int NEG_MAX_M = 1024;          // the longest list hard_negatives returns
constexpr int NEG_MAX_IDS = 8192;        // batch ids held in LDS for the admissibility test (64 KiB)

// slots per workgroup of the forward: 64, halved down to 16 (one group of four rows per wave) while the grid stays under 512
// workgroups.  A function of (Bg, M) only.
inline int neg_chunk(int Bg, int M) {
    int chunk = 64;
    while (chunk > 16 && (int64_t)Bg * ((M + chunk - 1) / chunk) < 512) chunk >>= 1;
    return chunk;
}
inline int neg_slabs(int Bg, int M) { return (M + neg_chunk(Bg, M) - 1) / neg_chunk(Bg, M); }

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

// NCH: 16-byte pieces per lane (E <= 256 NCH), whole rows in registers; 0: any E, the four rows streamed piece by piece
template <int NCH>
__global__ __launch_bounds__(256) void infonce_neg_fwd_kernel(const float* __restrict__ A, const float* __restrict__ bank, int64_t ldb,
                                                              const int64_t* __restrict__ neg_idx, const int64_t* __restrict__ ids,
                                                              const int64_t* __restrict__ bank_ids,
                                                              const float* __restrict__ inv_temp_p, int Bg, int E, int64_t N, int M,
                                                              int chunk, float* __restrict__ x, float* __restrict__ part) {
    extern __shared__ int64_t idl[];         // [Bg] the batch's ids (ids given)
    __shared__ float xs[64];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = blockIdx.x, s = blockIdx.y, S = gridDim.y;
    if (ids)
        for (int j = tid; j < Bg; j += 256) idl[j] = ids[j];
    if (tid < 64) xs[tid] = -INFINITY;
    __syncthreads();
    const float it = inv_temp_p[0];
    const int nchunks = E >> 2;                              // E % 4 == 0 (checked on the host)
    const float* ar = A + (int64_t)i * E;
    constexpr int NR = NCH > 0 ? NCH : 1;
    f32x4 av[NR];
    if constexpr (NCH > 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = lane + 64 * c;
            av[c] = ch < nchunks ? *(const f32x4*)(ar + ch * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const int n0 = s * chunk, n1 = min(M, n0 + chunk);
    int cnt = 0;
    for (int g = n0 + wave * 4; g < n1; g += 16) {
        int64_t rr[4];
        bool ok[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t r = g + q < n1 ? neg_idx[(int64_t)i * M + g + q] : (int64_t)-1;
            ok[q] = r >= 0 && r < N;
            rr[q] = ok[q] ? r : 0;                           // the only value an address is formed from
        }
        if (ids) {                                           // bank_ids[r] against every id of the batch: Bg compares per slot
            int64_t bid[4];
            bool hit[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { bid[q] = bank_ids[rr[q]]; hit[q] = false; }
            for (int j = lane; j < Bg; j += 64) {
                const int64_t v = idl[j];
#pragma unroll
                for (int q = 0; q < 4; ++q) hit[q] = hit[q] || v == bid[q];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) ok[q] = ok[q] && __ballot(hit[q]) == 0;
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (NCH > 0) {
            f32x4 u[4][NR];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float* br = bank + rr[q] * ldb;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int ch = lane + 64 * c;
                    u[q][c] = (ok[q] && ch < nchunks) ? *(const f32x4*)(br + ch * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < NCH; ++c) acc[q] += dot4(u[q][c], av[c]);
        } else {
            for (int ch = lane; ch < nchunks; ch += 64) {
                const f32x4 a = *(const f32x4*)(ar + ch * 4);
                f32x4 u[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) u[q] = ok[q] ? *(const f32x4*)(bank + rr[q] * ldb + ch * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] += dot4(u[q], a);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float d = wave_sum(acc[q]);
            const float xv = ok[q] ? d * it : -INFINITY;
            cnt += ok[q] ? 1 : 0;
            if (lane == 0 && g + q < n1) {
                x[(int64_t)i * M + g + q] = xv;
                xs[g + q - n0] = xv;
            }
        }
    }
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    if (wave == 0) {                                         // the chunk's (max, sum exp, count): one slot per lane
        const float v = xs[lane];
        const float m = wave_max(v);
        const float e = v == -INFINITY ? 0.f : __expf(v - m);
        const float sum = wave_sum(e);
        if (lane == 0) {
            float* p = part + ((int64_t)i * S + s) * 3;
            p[0] = m;
            p[1] = sum;
            p[2] = (float)((wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]));
        }
    }
}

// chunks merged in chunk order into the extended lse_row; the loss in infonce_fwd_kernel's order (thread tid takes rows tid, tid +
// 256, ..., wave tree, (w0 + w1) + (w2 + w3)): with used == 0 everywhere the plain call's bits
__global__ __launch_bounds__(256) void infonce_neg_merge_kernel(const float* __restrict__ part, int S, const float* __restrict__ lse_row,
                                                                const float* __restrict__ lse_col, const float* __restrict__ logits,
                                                                int Bg, int b2a, float* __restrict__ lse_ext,
                                                                int32_t* __restrict__ used, float* __restrict__ loss) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float term = 0.f;
    for (int i = tid; i < Bg; i += 256) {
        const float* p = part + (int64_t)i * S * 3;
        const float lr = lse_row[i];
        float m = lr;
        int cnt = 0;
        for (int s = 0; s < S; ++s) {
            m = fmaxf(m, p[3 * s]);
            cnt += (int)p[3 * s + 2];
        }
        float sum = lr == -INFINITY ? 0.f : __expf(lr - m);
        for (int s = 0; s < S; ++s) {
            const float pm = p[3 * s];
            sum += pm == -INFINITY ? p[3 * s + 1] : p[3 * s + 1] * __expf(pm - m);     // no finite slot: the sum is 0, or the NaN of a NaN slot
        }
        const float lext = cnt == 0 ? lr : m + __logf(sum);
        lse_ext[i] = lext;
        used[i] = cnt;
        const float d = logits[(int64_t)i * Bg + i];
        term += lext - d;
        if (b2a) term += lse_col[i] - d;
    }
    term = wave_sum(term);
    if (lane == 0) red[wave] = term;
    __syncthreads();
    if (tid == 0) loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) / ((float)Bg * (float)(b2a ? 2 : 1));
}

__global__ __launch_bounds__(256) void infonce_neg_grad_kernel(const float* __restrict__ bank, int64_t ldb,
                                                               const int64_t* __restrict__ neg_idx, const float* __restrict__ x,
                                                               const float* __restrict__ lse_row, const float* __restrict__ gscale,
                                                               const float* __restrict__ inv_temp_p, int Bg, int E, int64_t N, int M,
                                                               int ndir, float* __restrict__ dA, float* __restrict__ dot) {
    __shared__ f32x4 accs[4][64];
    __shared__ float dots[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = blockIdx.x;
    const int e0 = blockIdx.y * 256 + lane * 4;
    const bool in = e0 < E;                                  // E % 4 == 0: a lane's four columns are inside or outside together
    const float lse = lse_row[i];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float dsum = 0.f;
    for (int g = wave * 4; g < M; g += 16) {
        int64_t rr[4];
        bool ok[4];
        float p[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool valid = g + q < M;
            const int64_t r = valid ? neg_idx[(int64_t)i * M + g + q] : (int64_t)-1;
            const float xv = valid ? x[(int64_t)i * M + g + q] : -INFINITY;
            ok[q] = r >= 0 && r < N && !(xv == -INFINITY);   // x = -inf marks the slots that took no part in the forward
            rr[q] = ok[q] ? r : 0;
            p[q] = ok[q] ? __expf(xv - lse) : 0.f;
            dsum += ok[q] ? p[q] * xv : 0.f;
        }
        f32x4 u[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = (ok[q] && in) ? *(const f32x4*)(bank + rr[q] * ldb + e0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += p[q] * u[q];
    }
    accs[wave][lane] = acc;
    if (lane == 0) dots[wave] = dsum;
    __syncthreads();
    const float it = inv_temp_p[0];
    const float gs = gscale[0] / ((float)Bg * (float)ndir);
    if (wave == 0 && in) {
        const f32x4 t = (accs[0][lane] + accs[1][lane]) + (accs[2][lane] + accs[3][lane]);
        f32x4* out = (f32x4*)(dA + (int64_t)i * E + e0);
        *out = *out + (gs * it) * t;
    }
    if (tid == 0 && blockIdx.y == 0) dot[i] = dot[i] + gs * ((dots[0] + dots[1]) + (dots[2] + dots[3])) / it;
}

}  // namespace

extern "C" int sc_infonce_neg_workspace_floats(int32_t Bg, int32_t M) {
    if (Bg <= 0 || M < 1 || M > NEG_MAX_M) return 0;
    SC_CHECK((int64_t)3 * Bg * neg_slabs(Bg, M) < ((int64_t)1 << 31), "sc_infonce_neg_workspace_floats: Bg=%d", Bg);
    return 3 * Bg * neg_slabs(Bg, M);
}

extern "C" int sc_infonce_neg_fwd(const float* A, const float* bank, int64_t bank_stride, const int64_t* neg_idx, const int64_t* ids,
                                  const int64_t* bank_ids, const float* inv_temp, const float* lse_row, const float* lse_col,
                                  const float* logits, int32_t Bg, int32_t E, int64_t N, int32_t M, int32_t a2b, int32_t b2a, float* x,
                                  int32_t* used, float* lse_row_ext, float* loss, float* workspace, void* stream) {
    SC_CHECK(Bg >= 0 && E > 0 && E % 4 == 0, "sc_infonce_neg_fwd: Bg=%d >= 0, E=%d > 0 (E %% 4)", Bg, E);
    SC_CHECK(M >= 1 && M <= NEG_MAX_M, "sc_infonce_neg_fwd: 1 <= M <= %d (M=%d)", NEG_MAX_M, M);
    SC_CHECK(N >= 0 && N < ((int64_t)1 << 31), "sc_infonce_neg_fwd: 0 <= N < 2^31 (N=%lld)", (long long)N);
    SC_CHECK(bank_stride >= E && bank_stride % 4 == 0, "sc_infonce_neg_fwd: bank_stride=%lld >= E, 16-byte rows (stride %% 4)",
             (long long)bank_stride);
    SC_CHECK(a2b, "sc_infonce_neg_fwd: the extras enter the a2b denominator (a2b = 0)");
    SC_CHECK((ids == nullptr) == (bank_ids == nullptr) || N == 0, "sc_infonce_neg_fwd: ids and bank_ids come together or not at all");
    SC_CHECK(!ids || Bg <= NEG_MAX_IDS, "sc_infonce_neg_fwd: Bg=%d <= %d with ids (the batch's ids are held in LDS)", Bg, NEG_MAX_IDS);
    if (Bg == 0) return 0;
    SC_CHECK(A && neg_idx && inv_temp && lse_row && lse_col && logits && x && used && lse_row_ext && loss && workspace && (bank || N == 0),
             "sc_infonce_neg_fwd: null pointer");
    SC_CHECK(((uintptr_t)A & 15) == 0 && ((uintptr_t)bank & 15) == 0, "sc_infonce_neg_fwd: A / bank must be 16-byte aligned");
    if (N == 0) ids = bank_ids = nullptr;                    // an empty bank: no slot takes part, there is no id to read
    const int chunk = neg_chunk(Bg, M), S = neg_slabs(Bg, M);
    const dim3 grid(Bg, S), block(256);
    const size_t lds = ids ? (size_t)Bg * sizeof(int64_t) : 0;
    const hipStream_t st = (hipStream_t)stream;
#define SC_NEG_FWD(NCH)                                                                                                              \
    hipLaunchKernelGGL(infonce_neg_fwd_kernel<NCH>, grid, block, lds, st, A, bank, bank_stride, neg_idx, ids, bank_ids, inv_temp, Bg, E, N, \
                       M, chunk, x, workspace)
    if (E <= 256) SC_NEG_FWD(1);
    else if (E <= 512) SC_NEG_FWD(2);
    else if (E <= 768) SC_NEG_FWD(3);
    else if (E <= 1024) SC_NEG_FWD(4);
    else SC_NEG_FWD(0);
#undef SC_NEG_FWD
    SC_LAUNCH_CHECK();
    hipLaunchKernelGGL(infonce_neg_merge_kernel, dim3(1), block, 0, st, workspace, S, lse_row, lse_col, logits, Bg, b2a, lse_row_ext, used,
                       loss);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_infonce_neg_grad(const float* bank, int64_t bank_stride, const int64_t* neg_idx, const float* x,
                                   const float* lse_row_ext, const float* gscale, const float* inv_temp, int32_t Bg, int32_t E, int64_t N,
                                   int32_t M, int32_t a2b, int32_t b2a, float* dA, float* dlogit_dot, void* stream) {
    SC_CHECK(Bg >= 0 && E > 0 && E % 4 == 0, "sc_infonce_neg_grad: Bg=%d >= 0, E=%d > 0 (E %% 4)", Bg, E);
    SC_CHECK(M >= 1 && M <= NEG_MAX_M, "sc_infonce_neg_grad: 1 <= M <= %d (M=%d)", NEG_MAX_M, M);
    SC_CHECK(N >= 0 && N < ((int64_t)1 << 31), "sc_infonce_neg_grad: 0 <= N < 2^31 (N=%lld)", (long long)N);
    SC_CHECK(bank_stride >= E && bank_stride % 4 == 0, "sc_infonce_neg_grad: bank_stride=%lld >= E, 16-byte rows (stride %% 4)",
             (long long)bank_stride);
    SC_CHECK(a2b, "sc_infonce_neg_grad: the extras enter the a2b denominator (a2b = 0)");
    if (Bg == 0) return 0;
    SC_CHECK(neg_idx && x && lse_row_ext && gscale && inv_temp && dA && dlogit_dot && (bank || N == 0), "sc_infonce_neg_grad: null pointer");
    SC_CHECK(((uintptr_t)bank & 15) == 0 && ((uintptr_t)dA & 15) == 0, "sc_infonce_neg_grad: bank / dA must be 16-byte aligned");
    hipLaunchKernelGGL(infonce_neg_grad_kernel, dim3(Bg, (E + 255) / 256), dim3(256), 0, (hipStream_t)stream, bank, bank_stride, neg_idx, x,
                       lse_row_ext, gscale, inv_temp, Bg, E, N, M, (a2b && b2a) ? 2 : 1, dA, dlogit_dot);
    SC_LAUNCH_CHECK();
    return 0;
}
