// WavLM's gate of the relative-position bias (microsoft/unilm wavlm/modules.py MultiheadAttention.forward, gru_rel_pos branch;
// transformers WavLMAttention.forward steps 1-3), one launch per layer:
//   p = W_g . x[row, h 64 : h 64 + 64] + b_g      (W_g [8, 64], shared by the heads)
//   a = sigmoid(p[0] + p[1] + p[2] + p[3]),  b = sigmoid(p[4] + .. + p[7]),   gate[h][row] = a (b const[h] - 1) + 2
// x = the bf16 rows the QKV GEMM reads; arithmetic and output fp32.  The attention kernel's BIAS instance multiplies the per-head
// table of bucketed offsets by gate[h][query row] (csrc/attention.hip) - the [B H, T, T] product is never formed.
//
// 8 lanes per (row, head): a lane holds 8 of the head's 64 columns (one 16-byte load; the 8 (row, head) pairs of a wave are 8
// consecutive heads = 1 KiB of one row, or run on into the next) and its 8 x 8 slice of W_g in registers for every pair it visits.
// Memory bound: reads rows x D bf16 once, writes rows x H floats.
#include "sc_common.h"

namespace {

__global__ __launch_bounds__(256) void wavlm_gate_kernel(const uint16_t* __restrict__ x, int64_t ldx, const float* __restrict__ wg,
                                                         const float* __restrict__ bg, const float* __restrict__ cst,
                                                         float* __restrict__ gate, int64_t rows, int H) {
    const int sub = threadIdx.x & 7;
    float w[8][8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) w[k][j] = wg[k * 64 + sub * 8 + j];
    const float ba = (bg[0] + bg[1]) + (bg[2] + bg[3]), bb = (bg[4] + bg[5]) + (bg[6] + bg[7]);
    const int64_t npairs = rows * H, step = (int64_t)gridDim.x * 32;
    // the trip count is uniform over the 8 lanes of a pair and the shuffles below stay inside them
    for (int64_t p = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3); p < npairs; p += step) {
        const int64_t row = p / H;
        const int h = (int)(p - row * H);
        const uint4 v = *(const uint4*)(x + row * ldx + h * 64 + sub * 8);
        const float xv[8] = {bflo(v.x), bfhi(v.x), bflo(v.y), bfhi(v.y), bflo(v.z), bfhi(v.z), bflo(v.w), bfhi(v.w)};
        float pk[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s = fmaf(w[k][j], xv[j], s);
            pk[k] = s;
        }
        float pa = (pk[0] + pk[1]) + (pk[2] + pk[3]), pb = (pk[4] + pk[5]) + (pk[6] + pk[7]);
#pragma unroll
        for (int m = 1; m < 8; m <<= 1) {
            pa += __shfl_xor(pa, m);
            pb += __shfl_xor(pb, m);
        }
        if (sub == 0) {
            const float a = 1.0f / (1.0f + expf(-(pa + ba))), b = 1.0f / (1.0f + expf(-(pb + bb)));
            gate[(int64_t)h * rows + row] = fmaf(a, fmaf(b, cst[h], -1.0f), 2.0f);
        }
    }
}

}  // namespace

extern "C" int sc_wavlm_gate_bf16(const sc_bf16* x, int64_t ldx, const float* wg, const float* bg, const float* cst, float* gate,
                                  int64_t rows, int32_t H, void* stream) {
    SC_CHECK(x && wg && bg && cst && gate, "sc_wavlm_gate_bf16: null pointer");
    SC_CHECK(rows > 0 && H > 0 && ldx >= (int64_t)H * 64 && ldx % 8 == 0, "sc_wavlm_gate_bf16: rows=%lld H=%d ldx=%lld (head_dim 64, ldx %% 8 == 0)",
             (long long)rows, H, (long long)ldx);
    SC_CHECK(((uintptr_t)x % 16) == 0, "sc_wavlm_gate_bf16: x must be 16-byte aligned");
    const int64_t nblk = (rows * H + 31) / 32;
    hipLaunchKernelGGL(wavlm_gate_kernel, dim3((unsigned)(nblk < 2048 ? nblk : 2048)), dim3(256), 0, (hipStream_t)stream, x, ldx, wg, bg, cst,
                       gate, rows, H);
    SC_LAUNCH_CHECK();
    return 0;
}
