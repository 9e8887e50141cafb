// Raw-image input of the frozen CLIP image tower: CLIP's preprocessing (bicubic Resize(224) of a PIL image, CenterCrop(224), ToTensor,
// Normalize; avssl/module/clip_official.py:153-166 prep_image, avssl/data/base_dataset.py:93-106 clip_image_transform) on the device,
// bit for bit what Pillow's 8-bit resampling computes: 22-bit fixed-point coefficients, a horizontal pass, a uint8 intermediate image,
// a vertical pass, int32 accumulation, arithmetic shift, clip to a byte.  Two launches per batch of images of unequal sizes; the
// geometry, the tap bounds and the coefficients are host-built tables (speechclip_plus_amd/image_prep.py: Plan) - the kernels reach the
// source and the intermediate only through them, and every table-derived offset is checked against the buffer's byte count before it is
// used (a corrupt table reads nothing, writes nothing).  Layouts: include/speechclip_hip.h, "Raw-image input".
#include "sc_common.h"

namespace {

constexpr int IP_BITS = 22;             // Pillow's PRECISION_BITS for 8-bit images
constexpr int IP_HROWS = 4;             // intermediate rows per block of the horizontal pass: a coefficient is loaded once for the four
constexpr int IP_VTHREADS = 384;

__device__ __forceinline__ uint32_t ip_clip8(int acc) {
    const int v = (acc + (1 << (IP_BITS - 1))) >> IP_BITS;             // arithmetic shift, as Pillow's clip8
    return (uint32_t)min(max(v, 0), 255);
}

struct ip_desc {                        // one image: 8 x int64 (image_prep.Plan)
    int64_t src_off, src_w, mid_off, mid_rows, src_row0, htab, vtab, ksize;
};

// Horizontal pass.  Block (row group, image): thread x = one of the S crop columns, IP_HROWS consecutive intermediate rows.  The outer loop is
// over the column's taps, so its coefficient sits in a register while the rows' three channels accumulate (12 int32 accumulators).  Source
// reads are byte loads at a stride of (scale x 3) bytes between lanes: neighbouring lanes share cache lines, a row's whole span is read by one
// block and the next rows of the same block follow at once.  The intermediate row [S][3] is written as three byte stores per lane into one
// contiguous 3 S-byte run per row.
__global__ __launch_bounds__(256) void image_resample_h_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ desc,
                                                               const int32_t* __restrict__ tab, uint8_t* __restrict__ mid, int64_t mid_bytes, int S) {
    const ip_desc d = *(const ip_desc*)(desc + 8 * blockIdx.y);
    const int r0 = blockIdx.x * IP_HROWS;
    const int x = threadIdx.x;
    if (r0 >= d.mid_rows || x >= S) return;
    const int ks = (int)(d.ksize & 0xffffffff);
    const int32_t* bounds = tab + d.htab;
    const int32_t* coef = bounds + 2 * S + x * ks;
    const int first = bounds[2 * x], n = min(bounds[2 * x + 1], ks);
    const int nr = min(IP_HROWS, (int)d.mid_rows - r0);
    const int64_t pitch = d.src_w * 3;
    const int64_t base = d.src_off + (d.src_row0 + r0) * pitch + (int64_t)first * 3;
    if (first < 0 || n < 1 || first + n > d.src_w || base < 0 || base + (nr - 1) * pitch + (int64_t)n * 3 > src_bytes) return;
    int acc[IP_HROWS][3];
#pragma unroll
    for (int r = 0; r < IP_HROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0;
    const uint8_t* p = src + base;
    for (int t = 0; t < n; ++t) {
        const int k = coef[t];
#pragma unroll
        for (int r = 0; r < IP_HROWS; ++r) {
            if (r < nr) {
                const uint8_t* q = p + r * pitch + t * 3;
                acc[r][0] += (int)q[0] * k;
                acc[r][1] += (int)q[1] * k;
                acc[r][2] += (int)q[2] * k;
            }
        }
    }
    const int64_t o = d.mid_off + ((int64_t)r0 * S + x) * 3;
    if (o < 0 || d.mid_off + (int64_t)(r0 + nr) * S * 3 > mid_bytes) return;
#pragma unroll
    for (int r = 0; r < IP_HROWS; ++r) {
        if (r < nr) {
            uint8_t* m = mid + o + (int64_t)r * S * 3;
            m[0] = (uint8_t)ip_clip8(acc[r][0]);
            m[1] = (uint8_t)ip_clip8(acc[r][1]);
            m[2] = (uint8_t)ip_clip8(acc[r][2]);
        }
    }
}

// Vertical pass + normalisation.  Block (output row y, image).  Phase 1: thread j = byte j of the 3 S-byte output row [x][c]; tap t reads byte j
// of intermediate row first + t - consecutive lanes, consecutive bytes - and the row's coefficients are the same for the whole block (scalar
// loads).  The byte results go through LDS to change the lane order from [x][c] to [c][x].  Phase 2: thread (c, x pair) looks both bytes up in
// the channel's LUT and stores (a) one float2 of out[b][c][y][:] and / or (b) one packed bf16 pair of the patch GEMM's operand A: row
// row0[b] + 1 + gy g + gx, column c P^2 + ky P + kx (y = gy P + ky, x = gx P + kx) - sc_vit_patchify_bf16's layout and rounding.  The class row,
// the pad rows and the pad columns of A (zeros) are shared out over the image's S blocks, so every element of A is written.
__global__ __launch_bounds__(IP_VTHREADS) void image_resample_v_norm_kernel(const uint8_t* __restrict__ mid, int64_t mid_bytes, const int64_t* __restrict__ desc,
                                                                            const int32_t* __restrict__ tab, const float* __restrict__ lut,
                                                                            float* __restrict__ out, uint16_t* __restrict__ A, int Kp,
                                                                            const int32_t* __restrict__ row0, int S, int P) {
    __shared__ uint8_t row[3 * 256];
    const int b = blockIdx.y, y = blockIdx.x;
    const ip_desc d = *(const ip_desc*)(desc + 8 * b);
    const int ks = (int)(d.ksize >> 32);
    const int32_t* bounds = tab + d.vtab;
    const int32_t* coef = bounds + 2 * S + y * ks;
    const int first = bounds[2 * y], n = min(bounds[2 * y + 1], ks);
    const int rowb = 3 * S;
    const bool ok = first >= 0 && n >= 1 && first + n <= d.mid_rows && d.mid_off >= 0 && d.mid_off + d.mid_rows * rowb <= mid_bytes;
    const uint8_t* m = mid + d.mid_off + (int64_t)first * rowb;
    for (int j = threadIdx.x; j < rowb; j += IP_VTHREADS) {
        int acc = 0;
        if (ok)
            for (int t = 0; t < n; ++t) acc += (int)m[(int64_t)t * rowb + j] * coef[t];
        row[j] = (uint8_t)ip_clip8(acc);
    }
    __syncthreads();
    const int half = S >> 1;
    const int g = A ? S / P : 1, gy = A ? y / P : 0, ky = A ? y - gy * P : 0;
    const int64_t arow = A ? (int64_t)row0[b] : 0;
    for (int i = threadIdx.x; i < 3 * half; i += IP_VTHREADS) {
        const int c = i / half, x = 2 * (i - c * half);
        const float v0 = lut[c * 256 + row[3 * x + c]], v1 = lut[c * 256 + row[3 * x + 3 + c]];
        if (out) *(float2*)(out + (((int64_t)b * 3 + c) * S + y) * S + x) = make_float2(v0, v1);
        if (A) {
            const int gx = x / P, kx = x - gx * P;                                  // P even: the pair stays inside one patch
            *(uint32_t*)(A + (arow + 1 + gy * g + gx) * Kp + c * P * P + ky * P + kx) = pack2bf(v0, v1);
        }
    }
    if (A) {
        const int K = 3 * P * P, tokens = 1 + g * g;
        if (ky == 0 && Kp > K) {                                                    // pad columns of the g patch rows of this gy
            const int padw = (Kp - K) >> 1;                                         // K and Kp are even
            for (int i = threadIdx.x; i < g * padw; i += IP_VTHREADS) {
                const int gx = i / padw, k = K + 2 * (i - gx * padw);
                *(uint32_t*)(A + (arow + 1 + gy * g + gx) * Kp + k) = 0u;
            }
        }
        const int pitch = row0[b + 1] - row0[b];
        const int nz = (pitch - tokens + 1) * (Kp >> 3);                            // 16-byte chunks of the class row and the pad rows
        const int per = (nz + S - 1) / S;
        for (int i = y * per + threadIdx.x; i < min((y + 1) * per, nz); i += IP_VTHREADS) {
            const int zr = i / (Kp >> 3), c8 = i - zr * (Kp >> 3);
            const int r = zr == 0 ? 0 : tokens - 1 + zr;
            *(uint4*)(A + (arow + r) * Kp + c8 * 8) = make_uint4(0, 0, 0, 0);
        }
    }
}

}  // namespace

extern "C" int sc_image_resample_h_u8(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int32_t* tab, uint8_t* mid,
                                      int64_t mid_bytes, int32_t B, int32_t max_rows, int32_t S, void* stream) {
    SC_CHECK(src && desc && tab && mid, "sc_image_resample_h_u8: null pointer");
    SC_CHECK(B > 0 && B < 65536 && max_rows > 0 && src_bytes > 0 && mid_bytes > 0, "sc_image_resample_h_u8: B=%d (1 .. 65535) max_rows=%d src_bytes=%lld "
             "mid_bytes=%lld", B, max_rows, (long long)src_bytes, (long long)mid_bytes);
    SC_CHECK(S > 0 && S <= 256 && S % 2 == 0, "sc_image_resample_h_u8: S=%d must be even and <= 256", S);
    SC_CHECK(((uintptr_t)desc % 8) == 0 && ((uintptr_t)tab % 4) == 0, "sc_image_resample_h_u8: desc must be 8-byte and tab 4-byte aligned");
    hipLaunchKernelGGL(image_resample_h_kernel, dim3((max_rows + IP_HROWS - 1) / IP_HROWS, B), dim3(256), 0, (hipStream_t)stream, src, src_bytes, desc,
                       tab, mid, mid_bytes, S);
    SC_LAUNCH_CHECK();
    return 0;
}

extern "C" int sc_image_resample_v_norm(const uint8_t* mid, int64_t mid_bytes, const int64_t* desc, const int32_t* tab, const float* lut, float* out,
                                        sc_bf16* A, int32_t Kp, const sc_segments* seg, int32_t P, int32_t B, int32_t S, void* stream) {
    SC_CHECK(mid && desc && tab && lut, "sc_image_resample_v_norm: null pointer");
    SC_CHECK(out || A, "sc_image_resample_v_norm: neither output wanted (out and A are both null)");
    SC_CHECK(B > 0 && B < 65536 && mid_bytes > 0, "sc_image_resample_v_norm: B=%d (1 .. 65535) mid_bytes=%lld", B, (long long)mid_bytes);
    SC_CHECK(S > 0 && S <= 256 && S % 2 == 0, "sc_image_resample_v_norm: S=%d must be even and <= 256", S);
    SC_CHECK(((uintptr_t)desc % 8) == 0 && ((uintptr_t)tab % 4) == 0 && ((uintptr_t)lut % 4) == 0 && ((uintptr_t)out % 8) == 0,
             "sc_image_resample_v_norm: desc / out must be 8-byte, tab / lut 4-byte aligned");
    const int32_t* row0 = nullptr;
    if (A) {
        SC_CHECK(seg && seg->row0, "sc_image_resample_v_norm: A needs the segment table");
        SC_CHECK(P > 0 && P % 2 == 0 && S % P == 0, "sc_image_resample_v_norm: P=%d must be even and divide S=%d", P, S);
        SC_CHECK(Kp % 64 == 0 && Kp >= 3 * P * P, "sc_image_resample_v_norm: Kp=%d must be a multiple of 64 and >= 3 P^2 = %d", Kp, 3 * P * P);
        SC_CHECK(seg->B == B && seg->rows > 0 && seg->rows % SC_SEG_ROWS == 0, "sc_image_resample_v_norm: segment table B=%d rows=%d for %d images",
                 seg->B, seg->rows, B);
        SC_CHECK(seg->max_pitch >= 1 + (S / P) * (S / P) && (int64_t)seg->rows >= (int64_t)B * (1 + (S / P) * (S / P)),
                 "sc_image_resample_v_norm: an image needs %d rows, the segment table has max_pitch=%d rows=%d", 1 + (S / P) * (S / P), seg->max_pitch,
                 seg->rows);
        SC_CHECK(((uintptr_t)A % 16) == 0, "sc_image_resample_v_norm: A must be 16-byte aligned");
        row0 = seg->row0;
    }
    hipLaunchKernelGGL(image_resample_v_norm_kernel, dim3(S, B), dim3(IP_VTHREADS), 0, (hipStream_t)stream, mid, mid_bytes, desc, tab, lut, out,
                       (uint16_t*)A, Kp, row0, S, P);
    SC_LAUNCH_CHECK();
    return 0;
}
