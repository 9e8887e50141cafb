/* speechclip_hip_supcon.h - the supervised contrastive loss of libspeechclip_hip.so, beside include/speechclip_hip.h.
 *
 * A header of its own: speechclip_hip.h is a pinned ABI (its function set and sc_abi_version() are asserted by the tests of the binding),
 * and these entry points are additive.  Same conventions:
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - every pointer is a DEVICE pointer; sizes are elements, not bytes.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - every function returns 0 on success, nonzero on error (see sc_last_error()); arguments are checked before the first HIP call.
 *   - only the C that speechclip_plus_amd/_header.py reads: the ctypes binding is derived from this file as it is from the main header.
 *
 * Supervised contrastive loss (Khosla et al.; csrc/supcon.hip).
 *   replaces: SupConLoss.forward (avssl/module/losses.py:8-123), on the contrast rows C [N, E] = cat(unbind(features, 1), 0), N = V bsz:
 *             row r is view r / bsz of sample r % bsz.  Anchors are rows 0 .. Na - 1 (Na = N: contrast_mode "all"; Na = bsz: "one").
 *     l_ij   = inv_temp <C_i, C_j>                                   i < Na, j < N
 *     keep_ij = [j != i]                                             an anchor never contrasts with itself
 *     w_ij   = W[i % bsz, j % bsz] keep_ij                           W = [labels_a == labels_b] (all 64 bits) with labels, the float mask
 *                                                                    [bsz, bsz] as given (asymmetric, any weights) with mask, identity with neither
 *     lse_i  = log sum_j keep_ij e^{l_ij},   s_i = sum_j w_ij
 *     loss   = -(1 / base_temperature) / Na sum_i [ sum_j w_ij l_ij / s_i - lse_i ]      (s_i = 0: 0 / 0, a NaN loss as the reference's)
 *   sc_supcon_fwd : ONE launch - 64 x 64 logit tiles on the matrix pipe in exact fp32, per-tile (max, sum exp, sum w l, sum w) row
 *                   partials over the kept columns, the last-arriving workgroup merges them in tile order (deterministic, no float
 *                   atomics) into lse [Na], possum [Na] = sum_j w_ij l_ij, poscnt [Na] = s_i and loss[0]; the scaled logits [Na, N] are
 *                   kept for the backward.  labels and mask: one of them or neither.  inv_temp is a DEVICE scalar, base_temperature a
 *                   host float.  E % 4 == 0, C 16-byte aligned; rows of C at or behind N are never read.  N == 0 launches nothing.
 *                   Na N 4 bytes of logits above 1 GiB (SC_SUPCON_MAX_LOGIT_BYTES) are refused.
 *                   workspace: sc_supcon_workspace_floats(Na, N) floats, whose last word is the ticket - the CALLER zeroes the workspace
 *                   once before its first launch; every launch leaves the ticket zero.  One workspace per stream.
 *   sc_supcon_grad: with p_ij = keep_ij e^{l_ij - lse_i} and g_ij = -(w_ij / s_i - p_ij) / (base_temperature Na):
 *                   G [Na, N] = inv_temp gscale g   (dC = [G . C ; 0] + G^T . C[:Na]: sc_sgemm_mfma_f32, no further scaling) and
 *                   dlogit_dot [Na] = gscale sum_j g_ij l_ij / inv_temp, so that d loss / d inv_temp = sum_i dlogit_dot[i].
 *                   gscale is the incoming gradient of the loss, a DEVICE scalar.  The mask gets no gradient.
 */
#ifndef SPEECHCLIP_HIP_SUPCON_H
#define SPEECHCLIP_HIP_SUPCON_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_SUPCON_MAX_LOGIT_BYTES 1073741824   /* 1 GiB of logits [Na, N] fp32 */

int64_t sc_supcon_workspace_floats(int32_t Na, int32_t N);   /* 0: nothing to launch; -1: refused (see sc_last_error) */
int sc_supcon_fwd(const float* C, int32_t N, int32_t Na, int32_t bsz, int32_t E, const int64_t* labels, const float* mask,
                  const float* inv_temp, float base_temperature, float* logits, float* lse, float* possum, float* poscnt, float* loss,
                  float* workspace, void* stream);
int sc_supcon_grad(const float* logits, const float* lse, const float* poscnt, int32_t N, int32_t Na, int32_t bsz, const int64_t* labels,
                   const float* mask, const float* gscale, const float* inv_temp, float base_temperature, float* G, float* dlogit_dot,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
