/*
 * speechclip_hip_sigmoid.h - the pairwise sigmoid loss's entry points of libspeechclip_hip.so (csrc/sigmoid_loss.hip).
 * speechclip_hip.h's conventions hold: extern "C", device pointers, `stream` a hipStream_t as void*, 0 on success and < 0 on error
 * with sc_last_error().
 */
#ifndef SPEECHCLIP_HIP_SIGMOID_H
#define SPEECHCLIP_HIP_SIGMOID_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * The pairwise sigmoid loss of SigLIP (Zhai et al. 2023, https://arxiv.org/abs/2303.15343) on the gathered batch (csrc/sigmoid_loss.hip).
 * Additive in round 31, in a header of its own beside speechclip_hip.h and speechclip_hip_queue.h (which stay as they are: their
 * prototypes are counted); all three are bound by _lib.py.  sc_abi_version() stays 7.
 *   A [B, E] (speech), Bm [B, E] (image) fp32 unit rows, E % 4 == 0, 16-byte aligned; ids [B] int64 or NULL; scale = t > 0 and bias = b
 *   device scalars; same_id 0 "ignore", 1 "positive", 2 "negative".
 *     s_ij = <A_i, Bm_j>,  x_ij = fma(t, s_ij, b),  z_ij = +1 if i == j else -1
 *     same_ij = ids and i != j and ids[i] == ids[j] (64-bit compare):  ignore w_ij = 0,  positive z_ij = +1,  negative nothing
 *     loss = (1 / B) sum_ij w_ij softplus(-z_ij x_ij),   softplus(u) = max(u, 0) + log1p(exp(-|u|))
 *     g_ij = d loss / d x_ij = -(1 / B) w_ij z_ij sigmoid(-z_ij x_ij)      (sigmoid without overflow on either side)
 *   sc_sigmoid_loss_fwd : one launch.  s [B, B] = the RAW dots (the backward reads them; x is never stored), loss[0], counts[3] int32 =
 *                         (positives, negatives, ignored).  workspace: sc_sigmoid_loss_workspace_floats(B) floats whose LAST four
 *                         (the ticket word and padding) are zero before the first launch; every launch leaves them zero.
 *   sc_sigmoid_loss_grad: one launch.  G [B, B] = gscale t g_ij (exactly 0 where w_ij = 0), so that dA = G . Bm and dB = G^T . A
 *                         (sc_sgemm_mfma_f32) need no further scaling; dscale_part[i] = gscale sum_j g_ij s_ij and dbias_part[i] =
 *                         gscale sum_j g_ij: d loss / d t and d loss / d b are their sums over i.
 *   B >= 1; B B 4 bytes of dots at most 1 GiB (B <= 16384).  Fixed-order reductions, no float atomics: equal operands give equal bits.
 * ---------------------------------------------------------------------------------------------- */
int64_t sc_sigmoid_loss_workspace_floats(int32_t B);   /* the count itself; -1: refused */
int sc_sigmoid_loss_fwd(const float* A, const float* Bm, int32_t B, int32_t E, const int64_t* ids, int32_t same_id,
                        const float* scale /*device scalar*/, const float* bias /*device scalar*/, float* s, float* loss, int32_t* counts,
                        float* workspace, void* stream);
int sc_sigmoid_loss_grad(const float* s, int32_t B, const int64_t* ids, int32_t same_id, const float* gscale /*device scalar*/,
                         const float* scale /*device scalar*/, const float* bias /*device scalar*/, float* G, float* dscale_part /*[B]*/,
                         float* dbias_part /*[B]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif
