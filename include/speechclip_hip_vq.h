/* speechclip_hip_vq.h - the keyword quantiser's other modes (soft, Gumbel, learnable temperature) of libspeechclip_hip.so, beside
 * include/speechclip_hip.h and include/speechclip_hip_supcon.h.
 *
 * A header of its own for the reason the supcon header is one: speechclip_hip.h is a pinned ABI (its function set and
 * sc_abi_version() are asserted by the tests of the binding), and these entry points are additive.  Same conventions:
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - every pointer is a DEVICE pointer; sizes are elements, not bytes; bf16 values are uint16_t words.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - every function returns 0 on success, nonzero on error (see sc_last_error()); arguments are checked before the first HIP call.
 *   - only the C that speechclip_plus_amd/_header.py reads: the ctypes binding is derived from this file as it is from the main header.
 *
 * Training modes of SimpleVectorQuantizer (csrc/vq_modes.hip).
 *   replaces: SimpleVectorQuantizer.forward in training (avssl/module/speechclip_c_modules/my_vector_quantizer.py:124-137) for
 *             use_gumbel true / hard false, and the gradient to a learnable temperature.
 *   x [Nk, ldx >= V] fp32 are the MASKED scores: sc_vq_rowstats has written -inf into the special columns.  tau = temp > 0.
 *     z_nv = (x_nv + g_nv) / tau,  s = softmax(z) per row,  g = 0 without noise.
 *   Noise (noise != 0): stateless, one hash word per element -
 *     e = n V + v as uint32 (n the row, V the TRUE vocabulary, not a pitch; (int64) Nk V < 2^32 is an argument check),
 *     w = sc_hash32(e ^ seed),  u = ((w >> 9) + 0.5) 2^-23 (exact in fp32, in [2^-24, 1 - 2^-24]),
 *     g = -log(-log u) with the precise logf (1 ulp each): finite, in [-2.82, 16.64], |g - g_exact| <= 4 U (1 + |g|), U = 2^-24.
 *   Every kernel that takes (seed, noise) evaluates the same g for the same (n, v): nothing but x and the seed is kept for the backward.
 *   sc_vq_gumbel_f32     : g [Nk, ldg] materialised (columns < V), for host twins and yardsticks.
 *   sc_vq_noisy_rowstats : per row (one workgroup each, sc_vq_rowstats' shape and tie rule: the lowest column among equal maxima)
 *                          idx = first argmax_v (x + g), rowmax = max_v (x + g), logsum = log sum_v exp((x + g - rowmax) / tau).
 *                          LSE((x + g) / tau) = rowmax / tau + logsum; the two stay APART, because their fp32 sum would put an
 *                          absolute error of U |rowmax / tau| into every exponent (6e-5 at tau = 1e-3) where x + g - rowmax is exact at
 *                          the maximum.  noise 0: the same statistics of x itself, with the precise expf / logf.
 *   sc_vq_soft_prob_f32  : s [Nk, lds >= V] = exp((x + g - rowmax) / tau - logsum) dense, exactly 0 in masked columns; rowmax and
 *                          logsum are sc_vq_noisy_rowstats' for the same (temp, seed, noise).
 *   sc_vq_soft_split_bf16: the same s as the bf16 addends hi = bf16(s), lo = bf16(s - hi) in three K-blocks of Vp columns,
 *                          out [Nkp, 3 Vp] = [hi | hi | lo]; against a table laid out [hi | lo | hi] ONE bf16 GEMM sums
 *                          hi hi + hi lo + lo hi, each product exact in fp32.  Rows >= Nk and columns >= V of every block are
 *                          written as zeros.  Vp % 4 == 0, out 8-byte aligned.
 *   sc_vq_soft_bwd2      : with t = d subword_prob:  dz = s (t - <s, t>),  dx [Nk, ldd >= Vpad] = dz / tau (bf16 or fp32; columns
 *                          V .. Vpad - 1 zero-filled; s == 0 gives exactly 0 and never meets t),  and, when dtemp_row [Nk] is given,
 *                          dtemp_row[n] = -(1 / tau) sum_v dz_nv z_nv over s > 0: d tau = sum_n dtemp_row[n] (sc_colsum_f32, index order).
 *                          sc_vq_soft_bwd (main header) is this formula with noise 0, no dtemp_row, on the fused LSE.
 *   Fixed-order reductions, no float atomics: two calls on the same inputs give the same bits.
 */
#ifndef SPEECHCLIP_HIP_VQ_H
#define SPEECHCLIP_HIP_VQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int sc_vq_gumbel_f32(float* g, int64_t ldg, int32_t Nk, int32_t V, uint32_t seed, void* stream);
int sc_vq_noisy_rowstats(const float* x, int64_t ldx, int32_t Nk, int32_t V, float temp, uint32_t seed, int32_t noise, int64_t* idx,
                         float* rowmax, float* logsum, void* stream);
int sc_vq_soft_prob_f32(const float* x, int64_t ldx, const float* rowmax, const float* logsum, int32_t Nk, int32_t V, float temp,
                        uint32_t seed, int32_t noise, float* s, int64_t lds, void* stream);
int sc_vq_soft_split_bf16(const float* x, int64_t ldx, const float* rowmax, const float* logsum, int32_t Nk, int32_t V, float temp,
                          uint32_t seed, int32_t noise, uint16_t* out, int32_t Nkp, int32_t Vp, void* stream);
int sc_vq_soft_bwd2(const float* x, int64_t ldx, const float* rowmax, const float* logsum, const float* t, int64_t ldt, int32_t Nk,
                    int32_t V, int32_t Vpad, float temp, uint32_t seed, int32_t noise, void* dx, int64_t ldd, int32_t out_bf16,
                    float* dtemp_row, void* stream);

#ifdef __cplusplus
}
#endif
#endif
