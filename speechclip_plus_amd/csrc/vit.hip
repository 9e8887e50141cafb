// Front of the frozen CLIP image tower (openai/CLIP VisionTransformer.forward up to the transformer): conv1 as a GEMM over patch rows,
// class token + positional embedding + ln_pre, in the library's ragged row layout (sc_segments) so that the transformer blocks run
// as sc_hubert_layer_fwd(pre_ln = 1, ffn_act = 2, seg) on the same rows (include/speechclip_hip.h, "Front of the frozen CLIP image
// tower").  Both kernels are memory-bound single passes; the patch GEMM between them is an ordinary sc_gemm_bf16 call (fp32 out).
#include "sc_common.h"

namespace {

// A[r, k] for one row r per block: patch (gy, gx) of image b reads P x P pixels of each channel.  The 8 columns of a 16-byte chunk
// may cross a pixel row (P = 14): the index arithmetic is per element, the store is one uint4.
__global__ __launch_bounds__(128) void vit_patchify_kernel(const float* __restrict__ img, int64_t sb, int64_t sc, int64_t sy,
                                                           uint16_t* __restrict__ A, int Kp, const int32_t* __restrict__ chunk, int P, int g) {
    const int r = blockIdx.x;
    const int4 ent = *(const int4*)(chunk + 4 * (r >> 3));        // (first row, pitch, image, 0) of the image that owns row r
    const int t = r - ent.x, b = ent.z;
    const int K = 3 * P * P;
    uint16_t* a = A + (int64_t)r * Kp;
    const bool patch = t >= 1 && t <= g * g;
    const int gy = patch ? (t - 1) / g : 0, gx = patch ? (t - 1) - gy * g : 0;
    const float* src = img + (int64_t)b * sb + (int64_t)(gy * P) * sy + gx * P;
    for (int c8 = threadIdx.x; c8 < Kp / 8; c8 += 128) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = c8 * 8 + e;
            v[e] = 0.f;
            if (patch && k < K) {
                const int ch = k / (P * P), rem = k - ch * P * P, ky = rem / P, kx = rem - ky * P;
                v[e] = src[(int64_t)ch * sc + (int64_t)ky * sy + kx];
            }
        }
        uint4 o;
        o.x = pack2bf(v[0], v[1]); o.y = pack2bf(v[2], v[3]); o.z = pack2bf(v[4], v[5]); o.w = pack2bf(v[6], v[7]);
        *(uint4*)(a + c8 * 8) = o;
    }
}

// One wave per row (4 rows per block), the row in registers (W <= 1024: at most four f32x4 per lane), LayerNorm in fp32 with the
// centred second moment (two passes over registers, as torch's layer_norm).
__global__ __launch_bounds__(256) void vit_embed_ln_kernel(const float* __restrict__ G, const float* __restrict__ cls, const float* __restrict__ pos,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, uint16_t* __restrict__ X,
                                                           const int32_t* __restrict__ chunk, int rows, int tokens, int W, float eps) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int4 ent = *(const int4*)(chunk + 4 * (r >> 3));
    const int t = r - ent.x;
    uint16_t* x = X + (int64_t)r * W;
    if (t >= tokens) {                               // pad row: zeros (finite; nothing downstream reads it)
        for (int c = lane * 4; c < W; c += 256) *(uint2*)(x + c) = make_uint2(0, 0);
        return;
    }
    const float* e = t == 0 ? cls : G + (int64_t)r * W;
    const float* pp = pos + (int64_t)t * W;
    f32x4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane * 4 + i * 256;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < W) {
            const f32x4 a = *(const f32x4*)(e + c), p = *(const f32x4*)(pp + c);
            v[i] = a + p;
            s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
    }
    const float mean = wave_sum(s) / (float)W;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane * 4 + i * 256;
        if (c < W) {
            const f32x4 d = v[i] - mean;
            q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)W + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane * 4 + i * 256;
        if (c < W) {
            const f32x4 gm = *(const f32x4*)(gamma + c), bt = *(const f32x4*)(beta + c);
            const f32x4 y = (v[i] - mean) * rstd * gm + bt;
            uint2 o;
            o.x = pack2bf(y[0], y[1]);
            o.y = pack2bf(y[2], y[3]);
            *(uint2*)(x + c) = o;
        }
    }
}

}  // namespace

extern "C" int sc_vit_patchify_bf16(const float* img, int64_t sb, int64_t sc, int64_t sy, sc_bf16* A, int32_t Kp, const sc_segments* seg,
                                    int32_t S, int32_t P, void* stream) {
    SC_CHECK(img && A && seg && seg->chunk, "sc_vit_patchify_bf16: null pointer");
    SC_CHECK(P > 0 && S > 0 && S % P == 0, "sc_vit_patchify_bf16: S=%d must be a multiple of P=%d", S, P);
    SC_CHECK(Kp % 64 == 0 && Kp >= 3 * P * P, "sc_vit_patchify_bf16: Kp=%d must be a multiple of 64 and >= 3 P^2 = %d", Kp, 3 * P * P);
    SC_CHECK(seg->B > 0 && seg->rows > 0 && seg->rows % SC_SEG_ROWS == 0, "sc_vit_patchify_bf16: segment table B=%d rows=%d", seg->B, seg->rows);
    SC_CHECK(sb >= 0 && sc >= 0 && sy >= S, "sc_vit_patchify_bf16: strides sb=%lld sc=%lld sy=%lld (rows of S=%d contiguous floats)",
             (long long)sb, (long long)sc, (long long)sy, S);
    SC_CHECK(((uintptr_t)A % 16) == 0 && ((uintptr_t)seg->chunk % 16) == 0, "sc_vit_patchify_bf16: A and the chunk table must be 16-byte aligned");
    hipLaunchKernelGGL(vit_patchify_kernel, dim3(seg->rows), dim3(128), 0, (hipStream_t)stream, img, sb, sc, sy, (uint16_t*)A, Kp, seg->chunk,
                       P, S / P);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_vit_embed_ln_bf16(const float* G, const float* cls, const float* pos, const float* gamma, const float* beta, sc_bf16* X,
                                    const sc_segments* seg, int32_t tokens, int32_t W, float eps, void* stream) {
    SC_CHECK(G && cls && pos && gamma && beta && X && seg && seg->chunk, "sc_vit_embed_ln_bf16: null pointer");
    SC_CHECK(W > 0 && W % 4 == 0 && W <= 1024 && tokens > 0 && eps > 0.f, "sc_vit_embed_ln_bf16: W=%d (%% 4, <= 1024) tokens=%d eps=%g", W,
             tokens, (double)eps);
    SC_CHECK(seg->B > 0 && seg->rows > 0 && seg->rows % SC_SEG_ROWS == 0, "sc_vit_embed_ln_bf16: segment table B=%d rows=%d", seg->B, seg->rows);
    SC_CHECK(((uintptr_t)G % 16) == 0 && ((uintptr_t)cls % 16) == 0 && ((uintptr_t)pos % 16) == 0 && ((uintptr_t)gamma % 16) == 0 &&
                 ((uintptr_t)beta % 16) == 0 && ((uintptr_t)X % 8) == 0 && ((uintptr_t)seg->chunk % 16) == 0,
             "sc_vit_embed_ln_bf16: fp32 operands and the chunk table must be 16-byte aligned, X 8-byte aligned");
    hipLaunchKernelGGL(vit_embed_ln_kernel, dim3((seg->rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, G, cls, pos, gamma, beta, (uint16_t*)X,
                       seg->chunk, seg->rows, tokens, W, eps);
    SC_LAUNCH_CHECK();
    return 0;
}
