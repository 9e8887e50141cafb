/*
 * speechclip_hip_queue.h - the cross-batch negative queue's entry points of libspeechclip_hip.so (csrc/infonce_queue.hip).
 * speechclip_hip.h's conventions hold: extern "C", device pointers, `stream` a hipStream_t as void*, 0 on success and < 0 on error
 * with sc_last_error().
 */
#ifndef SPEECHCLIP_HIP_QUEUE_H
#define SPEECHCLIP_HIP_QUEUE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * A cross-batch negative queue beside the batch (csrc/infonce_queue.hip).  Additive in round 30, in a header of its own beside speechclip_hip.h
 * (which stays as it is: its prototypes are counted); both are bound by _lib.py.  sc_abi_version() stays 7.
 *   extends: MaskedContrastiveLoss.forward (avssl/module/losses.py:185-245), whose negatives are the batch alone, by the rows of two
 *            rings of past embeddings in BOTH directions: queue_B [Nq, E] (images) for the speech anchors A_i, queue_A [Nq, E] (speech)
 *            for the image anchors B_j, queue_ids [Nq] int64 or NULL (with ids, both or neither).
 *     xA_iq = inv_temp <A_i, queue_B[q]>,   xB_jq = inv_temp <B_j, queue_A[q]>
 *     entry (i, q) is ADMITTED iff there are no ids or queue_ids[q] != ids[i]      (losses.py:207's mask rule over more columns)
 *     lse_row_ext[i] = log(e^{lse_row_i} + sum_{q admitted} e^{xA_iq}),   lse_col_ext[j] = log(e^{lse_col_j} + sum_{q admitted} e^{xB_jq})
 *   The logits, the margin (diagonal only; the extras carry none), dcl, the loss formula and its division are sc_infonce_fwd's.  A
 *   direction that is off forms no extras and needs no buffer (x_A with a2b, x_B with b2a; the other may be NULL).
 *   x_A / x_B [Bg, ldx >= Nq] fp32, ldx % 4 == 0, 16-byte aligned: on entry the RAW dot products (sc_sgemm_mfma_f32 of the anchors against
 *   the queue); the kernels own them from then on.
 *   sc_infonce_queue_fwd : x <- inv_temp x where admitted, -inf elsewhere (pad columns Nq .. of the last 16-byte piece included), in place;
 *                          used_A / used_B [Bg] int32 = admitted entries per anchor (0 on a side that is off); lse_row_ext / lse_col_ext
 *                          [Bg] (the plain values on a side that is off); loss[0] recomputed from them and the diagonal of logits in
 *                          sc_infonce_fwd's order - no entry admitted: the plain call's bits.  lse_row / lse_col / logits are
 *                          sc_infonce_fwd's outputs for the same operands.  E is the operands' width (E % 4 == 0, as for the products).
 *                          workspace: sc_infonce_queue_workspace_floats(Bg, Nq) floats, no initial contents needed.  Two launches.
 *   sc_infonce_queue_grad: x <- w = gscale / (Bg n_dir) inv_temp e^{x - lse_ext} in place (an entry of -inf gives exactly 0), so that
 *                          dA += w_A . queue_B and dB += w_B . queue_A (sc_sgemm_mfma_f32, B K-major) need no further scaling, and
 *                          dlogit_dot[i] += gscale / (Bg n_dir) (sum_q pA_iq xA_iq + sum_q pB_iq xB_iq) / inv_temp, p = e^{x - lse_ext}.
 *                          The in-batch gradient is sc_infonce_grad handed lse_row_ext / lse_col_ext.  The queues get no gradient.
 *   Bg Nq <= 2^26 per side (256 MiB of scores).  Bg == 0 or Nq == 0: no launch, nothing written.  Fixed-order reductions, no float
 *   atomics: two calls give the same bits; the chunking depends on (Bg, Nq) alone.
 * ---------------------------------------------------------------------------------------------- */
int sc_infonce_queue_workspace_floats(int32_t Bg, int32_t Nq);   /* the count itself (0: nothing to launch; at most 6 x 2^26), -1: refused */
int sc_infonce_queue_fwd(float* x_A, float* x_B, int64_t ldx, const int64_t* ids, const int64_t* queue_ids,
                         const float* inv_temp /*device scalar*/, const float* lse_row, const float* lse_col, const float* logits,
                         int32_t Bg, int32_t E, int32_t Nq, int32_t a2b, int32_t b2a, float* lse_row_ext, float* lse_col_ext,
                         int32_t* used_A, int32_t* used_B, float* loss, float* workspace, void* stream);
int sc_infonce_queue_grad(float* x_A, float* x_B, int64_t ldx, const float* lse_row_ext, const float* lse_col_ext,
                          const float* gscale /*device scalar*/, const float* inv_temp /*device scalar*/, int32_t Bg, int32_t Nq,
                          int32_t a2b, int32_t b2a, float* dlogit_dot /*[Bg]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif
