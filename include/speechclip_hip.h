/*
 * speechclip_hip.h - C ABI of libspeechclip_hip.so (gfx950 / MI355X).
 *
 * The reference (ShampooWang/SpeechCLIP_plus) is 100 % Python and has no FFI / operator layer of its own
 * (SURVEY.md F1); its seams are nn.Module.forward signatures.  This header is therefore the boundary a
 * maintainer would bind *under* those modules (ctypes stub: INTEGRATION.md).  Every entry point names the
 * reference computation it replaces (file:line under /root/reference).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all buffers
 *     (outputs and workspaces are allocated by the caller and passed in).
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it, never synchronise, keep no
 *     global state.  Re-entrant per stream.
 *   - return 0 on success, <0 on error; sc_last_error() gives a thread-local message.
 *   - bf16 tensors are raw uint16 storage (`sc_bf16`); "rows" of activations live in the padded layout
 *     described in DESIGN.md: utterance b, frame t  ->  row  b*R + t (uniform pitch R), or - round 4, a non-NULL `seg` argument -
 *     row  row0[b] + t  with a pitch per utterance (`sc_segments`): work follows the real lengths of a ragged batch.
 */
#ifndef SPEECHCLIP_HIP_H
#define SPEECHCLIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t sc_bf16;

const char* sc_last_error(void);
int sc_abi_version(void);     /* 7: one encoder entry point per kernel (sc_attn_fwd_bf16 takes seg / work / nwork and gate / table / tmax; sc_posconv_bf16,
                                 sc_posconv_prep, sc_wsum_fwd, sc_wsum_bwd take seg; their _seg and _relbias symbols are gone); 6 (round 13, additive: sc_search_slabs, sc_search_topk_bf16 - gallery search); 6 (round 12, additive: sc_kw_pool_fwd / _bwd / _max_rows, sc_bn_eachkw_fwd / _bwd - the fixed-keyword cascaded branch); 6 (round 10, additive: sc_attn_fwd_relbias_bf16, sc_attn_fwd_seg_relbias_bf16, sc_wavlm_gate_bf16 - WavLM's gated relative-
                                 position bias; nothing else changed); 6 (round 9, additive: sc_gemm_args.a_rep / sc_hubert_layer_args.w_split took the reserved3 / reserved2 slots - split
                                 weights for evaluation; sizes unchanged); 6: one front-end entry point per kernel (sc_wav_prep, sc_conv0_stats, sc_conv0_gn_gelu, sc_conv0_ln_gelu take
                                 seg / wav_off / out_f32; their _seg, _crop, _len and _f32 symbols are gone); 5: sc_adam_f32 takes its betas as doubles; 4 since round 4 (sc_segments; sc_gemm_args / sc_hubert_layer_args grew the segment fields) */
int sc_is_diag_build(void);   /* 1: libspeechclip_hip_diag.so - the same sources built with SC_DIAG_BUILD: also holds the diagnostic kernels
                                 (sc_gemm_args.tile 32 = timing only, RESULTS WRONG; 34 = stamped) and the LayerNorm-folded GEMMs; the
                                 product library refuses both */
int64_t sc_sizeof(int32_t what);   /* sizeof of 0 sc_gemm_args, 1 sc_hubert_layer_args, 2 sc_rt_gemm_args, 3 sc_rt_ln_args, 4 sc_rt_ln_bwd_args, 5 sc_segments */
/* tuning switches for same-process A/B measurements (tools/); results never depend on them.  key 1: the 256-row GEMM uses
 * plain instead of non-temporal stores on tiles with a residual.  key 6: sc_cif_fwd* / sc_cif_bwd* walk the frames in one wave per
 * (utterance, 256 channels) instead of one wave per output slot / per 8 frames (the same bits, 3.7x / 4.5x the time at 64 x 499). */
int sc_set_option(int32_t key, int32_t value);

/* ------------------------------------------------------------------------------------------------
 * Ragged row layout (round 4).  The reference pads every batch to its longest utterance and computes all of it
 * (avssl/module/speech_encoder_plus.py:506-518, 548-552); here utterance b owns rows [row0[b], row0[b + 1]) of every
 * [rows, C] activation buffer - its own pitch, a multiple of SC_SEG_ROWS = 8 rows, sized by its own number of frames - so GEMM rows,
 * attention blocks and row kernels follow the real lengths.  Down the conv stack layer l has the same table scaled by
 * 2^(6-l) (row0 * 64 at conv layer 0), the waveform by `samples_per_row` (320): a strided Conv1d stays ONE flat GEMM.
 *   row0   device [B + 1] int32, multiples of 8, row0[0] = 0, row0[B] = rows
 *   chunk  device [rows / 8][4] int32: for every 8-row chunk (first row of its utterance, pitch of its utterance, utterance, 0)
 *          - the reverse lookup of the flat kernels (one 16-byte load)
 *   max_pitch = max_b (row0[b + 1] - row0[b])   (grid sizing on the host)
 * The struct itself lives in HOST memory (passed by pointer), its two tables in device memory.
 * ---------------------------------------------------------------------------------------------- */
#define SC_SEG_ROWS 8
typedef struct {
    const int32_t* row0;
    const int32_t* chunk;
    int32_t B, rows, max_pitch, reserved;
} sc_segments;

/* ------------------------------------------------------------------------------------------------
 * bf16 MFMA GEMM with fused epilogue:  C = epi(A . W^T)      (every Linear / Conv1d on the path)
 *   replaces: fairseq Linear/Conv1d calls reached from avssl/module/speech_encoder_plus.py:75-105
 *             (conv feature extractor layers 1-6 as strided-row GEMMs, post_extract_proj, q/k/v/out_proj,
 *             fc1, fc2, pos_conv per group).
 *   A   [M, K] bf16, row stride lda (elements; rows may overlap - this is how a channels-last strided
 *       Conv1d becomes a GEMM: lda = stride*C_in, K = k*C_in)
 *   W   [N, K] bf16, row stride ldw   (torch Linear layout [out, in])
 *   C   [M, N] bf16 (or fp32 if out_f32), row stride ldc
 *   epilogue order:  acc -> +bias[n] -> act (0 none, 1 GELU-erf, 2 QuickGELU) -> dropout (train mode) -> +residual[m, n] -> store
 *   dropout (fairseq dropout_input / the layers' residual dropouts, F.dropout semantics: keep with probability 1 - p, scale the
 *       kept values by 1 / (1 - p)): stateless counter-based mask - element (m, n) is kept iff the 16-bit lane of
 *       sc_hash32((m*N + n) / 2 ^ drop_seed) selected by (m*N + n) & 1 is >= round(p * 65536); not applied to Ct columns
 *   columns n >= n_split (if n_split >= 0) are stored TRANSPOSED per head into Ct:
 *       Ct[(((m / R) * H + (n-n_split)/dh) * dh + (n-n_split)%dh) * R + m % R]     (V^T for attention)
 *   batch: grid.z = nb1*nb2 ; operand pointers advance by  (z / nb2) * s?1 + (z % nb2) * s?2  elements.
 *   Requirements: K % 64 == 0, lda/ldw % 8 == 0, ldc % 8 == 0; A, W, C, residual AND bias 16-byte aligned (the epilogue reads the
 *   bias in groups of four floats), sBias1 / sBias2 multiples of 4.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const sc_bf16* A; int64_t lda;
    const sc_bf16* W; int64_t ldw;
    void* C; int64_t ldc;
    int32_t M, N, K;
    const float* bias;            /* [N] fp32 or NULL */
    const sc_bf16* residual; int64_t ldr;   /* [M, N] bf16 or NULL */
    int32_t act;                  /* 0 none, 1 gelu(erf), 2 QuickGELU u * sigmoid(1.702 u) (fused epilogue of every tile family;
                                     act = 2 without dropout, LayerNorm folding or the diagnostic tile ids) */
    int32_t out_f32;              /* 0: C is bf16, 1: C is fp32 */
    sc_bf16* Ct; int32_t n_split; int32_t R; int32_t dh;   /* transposed-store region; n_split < 0 disables */
    int32_t nb1, nb2;             /* batch = nb1*nb2 (>= 1 each) */
    int64_t sA1, sA2, sW1, sW2, sC1, sC2, sBias1, sBias2, sR1, sR2;
    int32_t tile;                 /* 0 auto | 1: 128x128 (4 waves) | 2: 256-row tile, 8 waves, width 256 or 192 by wave quantisation
                                     (7 / 8 force 192 / 256; with n_split >= 0 the forced width must divide n_split, else an
                                     error) | 3: 128x64 (13: four LDS stages) | 14 / 15: 64x64 with two / four stages
                                     (few rows, narrow output, long K).  Every tile family accumulates k in the same order and
                                     shares the epilogue arithmetic: results do not depend on the choice.  (32 / 34: diagnostic
                                     kernels of libspeechclip_hip_diag.so only; the product library returns an error) */
    int32_t reserved;             /* store policy of the bf16 C tile (256-row kernels): 0 auto = non-temporal stores when a residual
                                     is given (the output is the next residual stream, not re-read by this kernel; measured
                                     -3.5 % GEMM time per step), 1 always non-temporal, 2 never */
    float drop_p;                 /* 0 = no dropout */
    uint32_t drop_seed;
    int32_t tap_c;                /* K-tile visiting-order hint for conv-shaped A (rows overlap: lda = 2*tap_c, K = 3*tap_c, i.e. a
                                     channels-last Conv1d with k = 3, stride 2): 0 = ascending k; tap_c = C_in visits, per 64-channel
                                     block, tap 0, tap 2, tap 1 - tap 2 of output row r is tap 0 of row r + 1, so its tile is
                                     re-read while still in the L2 instead of 16 K-tiles later from the fabric. Only the
                                     fp32 summation order over k changes; every tile family uses the same order, so results do not depend on
                                     the dispatcher's choice. */
    /* ---- LayerNorm folded into its neighbour GEMMs (256-row tile family only; see csrc/gemm256_bf16.hip, "LN").  A row-statistics
     * buffer is [M][8][2] fp32: per row 8 strip slots of (sum, sum of squares) - one strip per N-tile of the GEMM that wrote it, at most 4 used (N <= 1024); the
     * strips a producer does not write must be ZERO (allocate the buffer zeroed): consumers add the first four slots of a line.
     *   consumer (no residual, no dropout): A holds RAW (pre-LayerNorm) rows, W = W0 diag(gamma) folded by the caller,
     *       ln_stats / ln_ns = the statistics of A's rows and the number of valid strips, ln_colsum[n] = sum_k W[n,k] (of the bf16
     *       values), bias[n] = sum_k beta[k] W0[n,k] + bias0[n];   C = rstd_m (A W^T - mean_m ln_colsum) + bias  -> act -> store
     *   producer (residual given, act = 0): stats_out receives the statistics of the bf16 rows of C (strip = N-tile index;
     *       sc_gemm_stats_strips() tells how many the dispatcher's tile width gives); res_stats (+ res_ns, res_gamma, res_beta):
     *       the residual operand holds RAW rows too and enters as LayerNorm(residual row) = (r - mean) rstd gamma[n] + beta[n].
     *   ln_eps: the LayerNorm epsilon of both uses. */
    int32_t ln_ns;
    const float* ln_stats;
    const float* ln_colsum;
    const float* res_stats;
    const float* res_gamma;
    const float* res_beta;
    float* stats_out;
    int32_t res_ns;
    float ln_eps;
    /* ---- TN form (256 x 256 tiles only): tn = 1 reads BOTH operands with the reduction index as the row index,
     *       C[m, n] = sum_r A[r, m] W[r, n],   A [K, M] row stride lda, W [K, N] row stride ldw  (K = number of rows r),
     * i.e. a weight gradient dW = dY^T X straight from the row-major dY [rows, M] and X [rows, N] (rows may overlap: the im2col
     * view of a strided conv input), no transposed copies.  Requirements: M % 256 == 0, N % 256 == 0, K % 64 == 0, no bias /
     * activation / residual / dropout / transposed store / LayerNorm folding; split along r through the batch strides
     * (sA1 = rows_per_slice * lda, sW1 = rows_per_slice * ldw) into fp32 partials (out_f32 = 1) or a single bf16 / fp32 result.
     * k_total > 0: the slices are ragged - slice z1 covers rows [z1 K, min((z1 + 1) K, k_total)) (K, k_total multiples of 64). */
    int32_t tn;
    int32_t k_total;
    /* ---- activation fused with a second operand (Ct doubles as the aux pointer [M, N] bf16, row stride ldc; act = 1 erf-GELU - every
     * tile family, the 256-row one without a residual (round 4) - or 2 QuickGELU - 128-row tiles; no transposed store, bf16 output):
     *   aux_mode 1  dual store:  Ct <- u = bf16(acc + bias) (the pre-activation the backward needs),  C <- act(u)   (FFN fc1 of a layer
     *               that is differentiated: one launch instead of GEMM + sc_act_bf16)
     *   aux_mode 2  C <- bf16(acc) * act'(Ct)   (the input-gradient GEMM of fc2 followed by the activation's backward: Ct = the saved u)
     *   aux_mode 3  C <- act(u) as mode 1 computes it, u not stored (Ct NULL; 128-row tiles): the same layer run forward-only gives the
     *               bits of the differentiated run without keeping its pre-activation
     * All reproduce the two-launch sequence bit for bit (the activation reads the ROUNDED values the first kernel would have stored). */
    int32_t aux_mode;
    /* ---- split weights (evaluation mode; docs/rounds/r09_split_weights.md): a_rep = 0 / 1: W is [N, K].  a_rep = 2: W is the [N, 2K]
     * interleave by 64-column K-tile  [hi tile 0 | lo tile 0 | hi tile 1 | lo tile 1 | ...]  of  W_hi = bf16(W), W_lo = bf16(W - W_hi)
     * (ldw >= 2K; K, tap_c, lda still describe A), and the K loop reads every A tile twice: physical K-tile kt multiplies the A tile at
     * koff(kt / 2) with the W tile at 2 koff(kt / 2) + 64 (kt & 1), koff = the visiting order tap_c selects.  One launch, one fp32
     * accumulator over both halves, so every epilogue (bias, activations, residual, transposed store, segment layout, out_f32,
     * aux_mode) is the usual one; every tile family, same order, same bits.  Not with tn, LayerNorm folding (ln_*, res_stats,
     * stats_out), drop_p > 0 or the diagnostic tile ids.  Takes the slot of the former reserved3. */
    int32_t a_rep;
    /* ---- ragged rows (round 4): seg_chunk != NULL replaces the uniform `R` of the transposed store - row m belongs to the
     * utterance of chunk m / 8 = (first row r0, pitch Rb, ...) (sc_segments.chunk) and goes to
     *       Ct[(N - n_split) * r0 + (n - n_split) * Rb + (m - r0)]          (V^T [H, dh, Rb] per utterance, utterances back to back) */
    const int32_t* seg_chunk;
} sc_gemm_args;
int32_t sc_gemm_stats_strips(const sc_gemm_args* args);   /* strips a producer launch with these args writes per row (0: not on the 256-row family) */
int sc_gemm_bf16(const sc_gemm_args* args, void* stream);
uint32_t sc_hash32(uint32_t x);   /* host twin of the kernels' dropout hash (lowbias32): reconstructs a mask exactly */

/* ------------------------------------------------------------------------------------------------
 * Self-attention forward (flash style, key-padding by length), head_dim 64, optionally with WavLM's gated relative-position bias.
 *   replaces: fairseq MultiheadAttention inside TransformerSentenceEncoderLayer, invoked at
 *             avssl/module/speech_encoder_plus.py:52  (softmax((q*dh^-.5) k^T + kpm(-inf)) v); with the bias, microsoft/unilm
 *             wavlm/modules.py MultiheadAttention.forward with position_bias (the s3prl upstreams wavlm_base / wavlm_base_plus /
 *             wavlm_large behind S3prlSpeechEncoderPlus, avssl/module/speech_encoder_plus.py:145,278-281) and transformers
 *             WavLMAttention.forward step 4 + torch_multi_head_self_attention - both materialise gate . position_bias as
 *             [B H, T, T] and hand it to the softmax as an additive mask; here it is never formed
 *   qk   [rows, ldqk] bf16 : columns [0, D) = q (unscaled), [D, 2D) = k ; head h owns 64 columns
 *   vt   bf16 : v transposed per head (written by sc_gemm_bf16's Ct path), see the row layout
 *   valid_len [B] int32 : keys t >= valid_len[b] are masked (-inf)
 *   out  [rows, ldo] bf16, columns h*64..h*64+63
 *   lse2 log2-domain log-sum-exp for the backward (covers the biased values), or NULL
 *   causal (CLIP text tower): 1 = key t visible to query q iff t <= q ; 32 / 64 = causal INSIDE aligned segments of that many
 *       rows (short sequences packed back to back into one 128-row block attend to their own segment only); same for the backward
 *   drop_p, drop_seed: attention-probability dropout (train mode): P' = mask . P / (1 - p), the element index below hashed as in
 *       sc_gemm_args; 0 = off
 * Row layout (seg).  One workgroup = 128 queries of one (utterance, head) in either layout.
 *   NULL: uniform rows.  Utterance b's rows at b R (R a multiple of 8), vt [B, H, 64, R], lse2 [B, H, R], dropout element
 *     ((b*H + h)*R + q)*R + k (B*H*R*R < 2^32).  work must be NULL and nwork 0.  causal: 0, 1, 32 or 64.
 *   ragged rows (sc_segments): q / k rows of utterance b at row0[b] + t, vt = per utterance [H, 64, Rb] at element offset D * row0[b]
 *     (what sc_gemm_bf16 writes with seg_chunk), out rows likewise; lse2 [H][rows]; B < 65536.  B and R are not read.  In a last,
 *     shorter block the waves (32 queries each) past the pitch idle and the rows past it are not stored.  work (optional, device
 *     [nwork][4] int32, 16-byte aligned): the 128-query blocks to run, in launch order, one item = (utterance | q-block << 16, row0 of
 *     the utterance, its pitch, its key count or -1 = read valid_len) - the host sorts them longest first (an utterance's cost grows
 *     with its key count); NULL = every (b, q-block < max_pitch / 128), blocks past an utterance's pitch exit.  Dropout element
 *     ((h * rows + row0[b] + q) * max_pitch + k) (H*rows*max_pitch < 2^32).  causal: 0 or 1.  Bit-identical to the uniform call on
 *     the rows they share.
 * Bias (gate, table: both or neither; both NULL = the plain kernel, tmax is not read):
 *     softmax(scale q k^T + gate[h][i] table[h][j - i] + kpm(-inf)) v
 *   gate  [H][rows] fp32, rows = B R (uniform) or seg->rows: one value per (head, query row) in the row layout of the call
 *         (sc_wavlm_gate_bf16); pad rows may hold any bits ("Reads" below)
 *   table [H][2 tmax - 1] fp32, natural-log units: entry tmax - 1 + (j - i) = the bias of key j seen from query i; tmax >= the
 *         (largest) row pitch, which is limited to 8064 rows (the workgroup's slice of the table sits in LDS)
 *   causal must be 0 (error otherwise).
 * Reads (what the kernel loads but the mathematics excludes; line numbers are csrc/attention.hip's; tested by
 * tests/test_gpu_poison.py, docs/parity.md "What a kernel reads and must ignore").  With n = max(1, min(valid_len[b], pitch)) (:112-113):
 *   rows read as K: whole 64-key tiles (:29, :186-195), i.e. rows 0 .. 64 ceil(n / 64) - 1 of the utterance (:131, :138, :140-141; with
 *       causal a q-block stops at its own last row, :158-159).  Since the pitch is a multiple of 8 that is up to 56 rows past the
 *       pitch: they land in the next utterance or, behind the last one, behind the rows of qk.  They must be READABLE; they may hold
 *       any bits, NaN and Inf included: the scores of keys >= n are overwritten with -inf before anything uses them (:227-233).
 *   elements read as V^T: the same key range of every d row of [H, 64, pitch] (:130, :132, :139, :142-143), running on into the next d
 *       row, the next head, the next utterance or, for the last rows of the last utterance, up to 56 elements behind vt.  They must
 *       be READABLE and FINITE: a masked key's probability is exactly 0 (:260), but its V^T column is still multiplied by it in the
 *       P.V matrix product (:297-308), and 0 x NaN = 0 x Inf = NaN.  A non-finite value there turns the valid outputs of that
 *       (utterance, head) into NaN - and through the next layer's V^T those of the utterance in front of it.
 *   rows read as Q: a wave loads 32 query rows (:110-111, :115-121), so up to row 32 ceil(pitch / 32) - 1 of the utterance, at most 24
 *       rows past the pitch.  READABLE, any bits: a lane's query is one column of every product, and the lanes past the pitch
 *       store nothing (:336).
 *   SC_ATTN_SLACK (64) rows behind the last row of qk and SC_ATTN_SLACK elements behind the last element of vt cover all three;
 *       the caller provides them (zeroed once: nothing writes them).  R % 64 == 0 in the uniform layout needs none.
 *   ignored by value: the q and k of pad rows t >= valid_len[b] (any bits), gate on pad rows (read by the pad row's own lane only, the
 *       index clamped to the last row, :166-167), table offsets outside the head's table (clamped, :168-172), and valid_len itself
 *       outside [1, pitch] (clamped, :112-113).
 *   guarantee: out and lse2 of the query rows t < valid_len[b] do not depend on any of the above by value (bit for bit); rows
 *       t >= valid_len[b] inside the pitch are written (scratch: finite when their q is of ordinary magnitude); nothing is written
 *       past the pitch (:336).
 * ---------------------------------------------------------------------------------------------- */
#define SC_ATTN_SLACK 64
int sc_attn_fwd_bf16(const sc_bf16* qk, int64_t ldqk, const sc_bf16* vt, const int32_t* valid_len, sc_bf16* out, int64_t ldo,
                     const sc_segments* seg, const int32_t* work, int32_t nwork, int32_t B, int32_t R, int32_t H, int32_t D, float scale,
                     const float* gate, const float* table, int32_t tmax, float* lse2, int32_t causal, float drop_p, uint32_t drop_seed,
                     void* stream);

/* The gate of that bias, one launch per layer.
 *   replaces: unilm MultiheadAttention.forward's gru_rel_pos branch (grep_linear / grep_a) = transformers WavLMAttention.forward
 *             steps 1-3 (gru_rel_pos_linear / gru_rel_pos_const)
 *   x [rows, ldx] bf16: the rows the QKV GEMM reads, head h = columns h*64 .. h*64+63; wg [8, 64], bg [8], cst [H] fp32
 *   p = wg . x_h + bg ; a = sigmoid(p[0..3] summed) ; b = sigmoid(p[4..7] summed) ; gate[h][row] = a (b cst[h] - 1) + 2   (fp32) */
int sc_wavlm_gate_bf16(const sc_bf16* x, int64_t ldx, const float* wg, const float* bg, const float* cst, float* gate, int64_t rows,
                       int32_t H, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Self-attention backward, head_dim 64 (fairseq MultiheadAttention / nn.MultiheadAttention / CLIP ResidualAttentionBlock
 * with dh = 64): dq, dk, dv from q, k, v, out, dout and the forward's lse2.  Two kernels (dq ; dk + dv), no atomics.
 *   q, k, v, out, dout : row-major [B*R, ld] bf16, head h at columns h*64..h*64+63 of the given base pointers
 *   qT, kT, doT        : per-head transposed copies [B, H, 64, R] (sc_head_transpose_bf16)
 *   delta              : [B, H, R] fp32 workspace (rowsum(dout . out), written here)
 *   query rows t >= q_rows must carry dout = 0; keys t >= valid_len[b] (and t' > t when causal) get zero gradient
 * Reads (what the kernels load but the mathematics excludes; line numbers are csrc/attention_bwd.hip's; tested by
 * tests/test_gpu_poison_bwd.py, docs/parity.md "What a kernel reads and must ignore", "Backward").  n = max(1, min(valid_len[b], R))
 * (:91, :252), up32 / up64 / up128 = rounded up to a multiple.  Nothing outside the B*R rows of an operand is read: R % 128 == 0
 * (:523) makes every tile whole - the dq kernel loads 64-key tiles of K, V, K^T up to key up64(n) - 1 (:138-159) and its own 128
 * query rows (:89-107), the dk/dv kernel its own 128 keys (:251-275) and 64-row tiles of q, dout, q^T, dout^T, lse2, delta up to row
 * up64(q_rows) - 1 (:288-311), the preparation every row (:416-433, :465-503).
 *   keys n <= t < up32(n) (the last partly valid 32-key block):
 *       K any bits: a masked key is one row of S^T (:170) / one column of S (:335), replaced by a select (:189-190, :375, :390).
 *       V FINITE AND OF ORDINARY MAGNITUDE: dP = V . dO of the masked key is a sum (:171, :336) that is then multiplied by P = 0 (:191,
 *         :392); a NaN, an Inf or an overflowing sum there makes dq of the utterance's valid rows and dk of the masked key NaN.
 *       K^T columns FINITE: multiplied by dS = 0 in dQ^T += K^T dS^T (:201-202).  sc_attn_bwd_fused_bf16 makes K^T from K, so there K
 *         of these keys must be finite as well.
 *   keys up32(n) <= t < up128(n) (later blocks of a partly valid 128-key block): the dq kernel skips them (:164; K, V, K^T of the rest
 *       of a 64-key tile are loaded, never multiplied: any bits).  The dk/dv kernel has no early exit per wave: K any bits (:390), V
 *       FINITE AND OF ORDINARY MAGNITUDE (:336, :392) - otherwise dk of these keys is NaN instead of 0 (valid rows do not notice).
 *   keys t >= up128(n) (wholly padded 128-key blocks): never loaded by the dq kernel; the dk/dv workgroup stores zeros and returns
 *       (:261-265).  K, V, K^T any bits.
 *   query rows n <= t < up32(q_rows) (pad queries of a shorter utterance below q_rows, and the rest of the 32-row block q_rows falls
 *       in): the dk/dv kernel forms P = exp2(s c - lse2) for them (:374, :389) and multiplies it by dout^T = 0 (:404) and dS = P (0 - 0)
 *       by q^T (:406); the dq kernel computes their own dq the same way (:190-207).  So: q FINITE AND OF ORDINARY MAGNITUDE, lse2 THE
 *       FORWARD'S OWN VALUE for that q (then P <= 1), out FINITE (delta = sum 0 x out, :428, :485), dout and the dout^T columns EXACTLY
 *       ZERO, q^T columns FINITE.
 *   query rows t >= up32(q_rows): the dk/dv kernel loads them with the 64-row tile and never multiplies them (:328); the dq kernel uses
 *       a row for that row's own dq only.  No gradient of another row depends on them (any bits, dout included); their own dq is zero
 *       under the conditions of the line above.
 *   delta, and qT / kT / doT of sc_attn_bwd_fused_bf16: written over all B*H*R entries / all rows before they are read; any bits on entry.
 * Guarantee, under these classes: dq of the rows t < valid_len[b] and dk / dv of the keys t < valid_len[b] do not depend on the
 * excluded regions by value (bit for bit); dk / dv of the keys t >= valid_len[b] are exactly zero; dq of every row with dout = 0 is
 * exactly zero.  The row-reducing weight-gradient kernels behind this call sum dq / dk / dv over ALL B*R rows, and rely on it.
 * sc_head_transpose_bf16: xT[b, h, d, t] = x[b*R + t, h*64 + d]
 * ---------------------------------------------------------------------------------------------- */
int sc_attn_bwd_bf16(const sc_bf16* q, int64_t ldq, const sc_bf16* k, int64_t ldk, const sc_bf16* v, int64_t ldv,
                     const sc_bf16* out, int64_t ldo, const sc_bf16* dout, int64_t lddo, const sc_bf16* qT, const sc_bf16* kT,
                     const sc_bf16* doT, const float* lse2, float* delta, const int32_t* valid_len, sc_bf16* dq, int64_t lddq,
                     sc_bf16* dk, int64_t lddk, sc_bf16* dv, int64_t lddv, int32_t B, int32_t R, int32_t H,
                     int32_t q_rows /* query rows t >= q_rows carry dout = 0 (layout padding) */, float scale, int32_t causal,
                     float drop_p, uint32_t drop_seed /* the forward's probability dropout: same mask, regenerated */,
                     void* stream);
/* the same with the operand preparation inside: qT / kT / doT are scratch [B, H, 64, R] the call fills in ONE launch (three head
 * transposes + delta), followed by the dq and dk/dv kernels - 3 launches instead of 6 */
int sc_attn_bwd_fused_bf16(const sc_bf16* q, int64_t ldq, const sc_bf16* k, int64_t ldk, const sc_bf16* v, int64_t ldv,
                           const sc_bf16* out, int64_t ldo, const sc_bf16* dout, int64_t lddo, sc_bf16* qT, sc_bf16* kT,
                           sc_bf16* doT, const float* lse2, float* delta, const int32_t* valid_len, sc_bf16* dq,
                           int64_t lddq, sc_bf16* dk, int64_t lddk, sc_bf16* dv, int64_t lddv, int32_t B, int32_t R,
                           int32_t H, int32_t q_rows, float scale, int32_t causal, float drop_p, uint32_t drop_seed, void* stream);
int sc_head_transpose_bf16(const sc_bf16* x, int64_t ldx, sc_bf16* xT, int32_t B, int32_t R, int32_t H, void* stream);
/* Causal self-attention of 32-row sequences (the frozen CLIP text tower on keyword prompts of <= 32 tokens: clip_official.py:222-279 ->
 * CLIP Transformer / nn.MultiheadAttention, head_dim 64), one wave per (sequence, head), no workspaces:
 *   qkv  [nseq * 32, ld >= 3 heads 64] bf16 rows, Q | K | V side by side, head h at columns h*64.. of each third
 *   forward   out[nseq * 32, heads 64] = softmax(scale Q K^T | key <= query) V
 *   backward  dqkv (laid out like qkv) from qkv and dout alone: the probabilities are recomputed, delta = sum_k P dP in fp32
 * Rows behind a prompt are ordinary causal rows (finite values; zero gradient iff their dout rows are zero).  Backward: with dout = 0
 * there, their q / k / v must be finite and of ordinary magnitude (P of the row is recomputed and multiplied by 0, dP = V . dout is a
 * sum multiplied by P = 0); dqkv of the prompt rows then does not depend on them and dqkv behind the prompt is exactly zero
 * (tests/test_gpu_poison_bwd.py). */
int sc_attn32_fwd_bf16(const sc_bf16* qkv, int64_t ld, sc_bf16* out, int64_t ldo, int32_t nseq, int32_t heads, float scale, void* stream);
int sc_attn32_bwd_bf16(const sc_bf16* qkv, int64_t ld, const sc_bf16* dout, int64_t ldd, sc_bf16* dqkv, int64_t ldg, int32_t nseq,
                       int32_t heads, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row LayerNorm, bf16 in/out, fp32 statistics:  y = (x - mean) * rstd * gamma + beta  [-> GELU]
 *   replaces: fairseq LayerNorm calls (speech_encoder_plus.py:40,78 and inside each encoder layer),
 *             conv-extractor LayerNorm in "layer_norm" mode.
 *   D % 4 == 0, D <= 1024.  act: 0 none, 1 GELU(erf).
 * ---------------------------------------------------------------------------------------------- */
int sc_layernorm_bf16(const sc_bf16* x, int64_t ldx, const float* gamma, const float* beta, sc_bf16* y,
                      int64_t ldy, int64_t rows, int32_t D, float eps, int32_t act, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Waveform front end: one entry point per kernel; the row layout, the crop and the fp32 debug stores are arguments.
 *   sc_wav_prep: speech_encoder_plus.py:506-518 (optional per-utterance layer_norm over the whole waveform, zero padding) of the
 *     caller's [B, ldw_in] batch (padded length L) -> prepared fp32 waveform, samples >= wav_len[b] are 0.
 *   sc_conv0_stats + sc_conv0_finalize: GroupNorm(512,512) statistics of conv layer 0 over the padded time axis T0 (fairseq
 *     Fp32GroupNorm, "default" extractor mode) computed analytically from the 10x10 Gram matrix of the strided waveform (fp64
 *     accumulation) -> scale/shift [B, C] fp32.
 *   sc_conv0_gn_gelu: conv0 (C_in=1, k=10, s=5, no bias) + GroupNorm affine + GELU on the prepared waveform, channels-last.
 *   sc_conv0_ln_gelu: "layer_norm" extractor mode (HuBERT-large): conv0 (+bias; NULL: none) -> LayerNorm over the 512 channels -> GELU.
 * Row layout (seg; sc_wav_prep and the two conv-0 forwards).
 *   NULL: uniform rows.  The prepared waveform is [B, ldw_out] (ldw_out >= L; read as [B, ldw], ldw >= 5 (R0 - 1) + 10) and
 *     utterance b's R0 output rows are out[b*R0 + t, c].  samples_per_row is not read.
 *   ragged rows (round 4; seg = the sc_segments tables): the prepared waveform is ONE flat buffer, utterance b at sample
 *     samples_per_row * row0[b] (320 = 5 * 64: conv layer 0 then reads x[5 r + j] for its flat output row r = 64 * row0[b] + t, like
 *     every later conv layer reads rows 2 r ..), zero from wav_len[b] to the end of its region; it needs samples_per_row * rows + 16
 *     floats.  The conv-0 forwards write out row 64 * row0[b] + t for t < 64 * pitch_b.  B must equal seg->B; ldw_out / ldw / R0 are
 *     not read.
 * Crop (wav_off; the two kernels that read the caller's batch: sc_wav_prep, sc_conv0_stats).  The in-forward training crop (round 5):
 *   avssl/module/speech_encoder_plus.py:548-552 calls random_crop_max_length (avssl/data/audio_transforms.py:5-23) per utterance on
 *   the un-padded list and re-pads (:506-518).  Here the caller's [B, ldw] batch stays where it is: utterance b is
 *   wav[b, wav_off[b] : wav_off[b] + wav_len[b]] (wav_len = the CROPPED lengths, L = their maximum, wav_off[b] + wav_len[b] <= ldw is
 *   the caller's contract), read in place.  NULL: no crop.
 * Padded-length statistics (wav_len of sc_conv0_stats).  The statistics run over the PADDED batch length T0 - fairseq feeds the
 *   zero-padded batch (speech_encoder_plus.py:75) - whatever the row layout.  NULL: wav is the prepared, zero-padded batch
 *   (ldw >= 5 (T0 - 1) + 10; no wav_off).  Otherwise wav is the caller's batch and samples >= wav_len[b] read as 0.
 * out_f32 (the two conv-0 forwards).  0: out is sc_bf16*.  1: the fp32 debug mode - out is float*, the same arithmetic with unrounded
 *   stores; uniform rows only, and sc_conv0_ln_gelu then always runs its two-pass kernel.
 * ---------------------------------------------------------------------------------------------- */
int sc_wav_prep(const float* wav, int64_t ldw_in, const int64_t* wav_len, const int64_t* wav_off, float* out, int64_t ldw_out,
                const sc_segments* seg, int32_t samples_per_row, int32_t B, int32_t L, int32_t normalize, void* stream);
#define SC_CONV0_NSTAT 66   /* 55 Gram entries + 10 sums + pad */
int sc_conv0_stats(const float* wav, int64_t ldw, const int64_t* wav_len, const int64_t* wav_off, int32_t B, int32_t T0, int32_t nchunk,
                   double* partial, void* stream);
int sc_conv0_finalize(const double* partial, int32_t nchunk, const float* w0 /*[C,10]*/, const float* gamma,
                      const float* beta, int32_t B, int32_t C, int32_t T0, float eps, float* scale,
                      float* shift, void* stream);
int sc_conv0_gn_gelu(const float* wav, int64_t ldw, const sc_segments* seg, int32_t samples_per_row, const float* w0, const float* scale,
                     const float* shift, void* out, int32_t out_f32, int32_t B, int32_t R0, int32_t C, void* stream);
int sc_conv0_ln_gelu(const float* wav, int64_t ldw, const sc_segments* seg, int32_t samples_per_row, const float* w0, const float* bias,
                     const float* gamma, const float* beta, float eps, void* out, int32_t out_f32, int32_t B, int32_t R0, int32_t C,
                     void* stream);
/* backward of conv layer 0 + GroupNorm + GELU for the fully trainable encoder (speech_encoder_plus.py:556-562; the input is the
 * waveform: parameter gradients only).  dy [B*R0, 512] bf16 = gradient of the layer's output, scale / shift / stats = the forward's
 * (sc_conv0_finalize, sc_conv0_stats with nchunk chunks).  partial: scratch [B, nwc, 512, 12] fp32 (nwc % 4 == 0 wave chunks);
 * contrib [B, 512, 12] fp32 = per utterance (dW[c][0..9], dgamma[c], dbeta[c]) - sum over B with sc_colsum_f32. */
int sc_conv0_gn_bwd(const float* wav, int64_t ldw, const float* w0, const float* scale, const float* shift, const sc_bf16* dy,
                    const double* stats, int32_t nchunk, const float* gamma, const float* beta, int32_t B, int32_t T0, int32_t R0,
                    int32_t C, float eps, float* partial, int32_t nwc, float* contrib, void* stream);
/* the same for the "layer_norm" extractor (HuBERT-large: conv 0 (+bias) -> LayerNorm over the 512 channels -> GELU): per wave chunk of
 * rows 13 sums per channel - partial [B, nwc, 512, 16] fp32 with (dW[c][0..9], dbias[c], dgamma[c], dbeta[c], 3 unused); sum over
 * B * nwc with sc_colsum_f32 (nwc % 4 == 0). */
int sc_conv0_ln_bwd(const float* wav, int64_t ldw, const float* w0, const float* bias, const float* gamma, const float* beta, float eps,
                    const sc_bf16* dy, int32_t B, int32_t T0, int32_t R0, int32_t C, float* partial, int32_t nwc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pos_conv input: zero padded frames (speech_encoder_plus.py:32-33 index_put(x, padding_mask, 0)) and
 * regroup channels-last rows into the group-major, halo-padded slab layout the grouped conv reads:
 *   xz  [rows, D] : masked copy (residual operand of the pos_conv epilogue)
 *   xg  slabs of D/G channels: the masked frames between zero halos, see the row layout
 * Row layout (seg).
 *   NULL: uniform rows.  xz [B*R, D], xg [G, B, R + 2*halo, D/G] : rows [halo, halo+R) hold the masked frames, everything else 0.
 *   ragged rows: xg [G][rows + 2 * halo * B][D / G], utterance b's slab at row  row0[b] + 2 * halo * b  (its frames at + halo); the
 *     kernel reads seg->chunk (16-byte aligned), rows % 8 == 0, halo > 0.  B and R are not read.
 * ---------------------------------------------------------------------------------------------- */
int sc_posconv_prep(const sc_bf16* x, const int32_t* valid_len, sc_bf16* xz, sc_bf16* xg, const sc_segments* seg, int32_t B, int32_t R,
                    int32_t D, int32_t G, int32_t halo, void* stream);

/* HuBERT positional convolution on the slab layout above + bias + GELU + residual (speech_encoder_plus.py:32-37: grouped Conv1d,
 * kernel Kp = 128, padding 64, SamePad drops the last frame):
 *   out[b*R + t, g*Dg + n] = gelu(bias[g*Dg + n] + sum_j sum_ci w[g][n][j*Dg + ci] * xg[g][b][t + j][ci]) + residual[b*R + t, g*Dg + n]
 * w [G, Dg, Kp*Dg] tap-major per group, Dg = D / G in {48, 64}.  The input slab of a (group, utterance, 512-frame block) stays in LDS
 * for all taps; only the weights stream.  Same arithmetic as the sc_gemm_bf16 formulation (lda = Dg, K = Kp*Dg, act = 1, residual):
 * bit-identical results.
 * Row layout (seg).
 *   NULL: uniform rows.  Rp = rows of an xg slab (>= R + Kp - 1).
 *   ragged rows: the slab layout sc_posconv_prep writes with seg (halo = Kp / 2), out / residual rows row0[b] + t.  B, R and Rp are
 *     not read. */
int sc_posconv_bf16(const sc_bf16* xg, const sc_bf16* w, const float* bias, const sc_bf16* residual, sc_bf16* out, const sc_segments* seg,
                    int32_t B, int32_t R, int32_t D, int32_t G, int32_t Kp, int32_t Rp, void* stream);

/* Weight gradient of that convolution (fully trainable HuBERT; speech_encoder_plus.py:29-40 under trainable: true):
 *   part[z][g][co][tap*Dg + ci] = sum over the z-th slice of slab rows m of  du[g][m][co] * xg[g][m + tap][ci]
 * du, xg [G, rows, Dg] bf16 (rows = B * Rp, the slab row pitch; du must be ZERO on rows whose window straddles two utterances, i.e.
 * laid out like the slab with the frames at row offset 0: pass the du slab advanced by `halo` rows), Dg in {48, 64}, Kp % 16 == 0,
 * rows % (128 * Z) == 0; xg rows past the end of the buffer are never dereferenced (clamped; they meet du = 0).
 * part [Z, G, Dg, Kp*Dg] fp32: reduce over z with sc_colsum_f32. */
int sc_posconv_wgrad_bf16(const sc_bf16* du, const sc_bf16* xg, float* part, int32_t G, int64_t rows, int32_t Dg, int32_t Kp,
                          int32_t Z, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Weighted sum over hidden states (avssl/module/weighted_sum.py:26-45).
 *   h    [NL, B*R, D] bf16 ; w [NL] fp32 = softmax(weights) (host computes the 13-element softmax)
 *   out  [B, R, D] bf16, written at row offset `row_off` inside each utterance (row_off = 1 leaves row 0
 *        for the CLS token of kw_branches.py:266-267), rows t in [0, R - row_off)
 *   bwd: dw[n] = sum_{b,t,d} g[b, t + row_off, d] * (h[n, b, t, d] - h[NL-1, b, t, d])   (g fp32 [B, R, D]).  The gradient of the
 *        13 (25) logits is the softmax projection w_n (dw_n - sum_m w_m dw_m), invariant under a common shift of dw: the last
 *        layer is subtracted element-wise BEFORE the accumulation, so the large common part <g, h> never enters the fp32 sums
 *        (layers of a residual stream differ by 1e-1 .. 1e-2 of their norm; summing first would cost those digits)
 *   normalize != 0: every h[n, row, :] passes through a non-affine LayerNorm(D, eps 1e-5) first
 *        (normalize_features=True, weighted_sum.py:41-42; used by the HuBERT-large recipes), D <= 1024
 * Row layout (seg; both directions).
 *   NULL: uniform rows, as above.
 *   ragged hidden states -> uniform-pitch output (round 4): h [NL, seg->rows, D] in the segment layout; out / g stay [B, R, D] with
 *     utterance b's frame t at out[b, t + row_off] for t + row_off < min(pitch_b + row_off, R), every other row of out is ZEROED (the
 *     consumers - the CLS pooling kernels, the cascaded+/hybrid+ branches - keep a uniform [B, R, D] view and mask by length).  B must
 *     equal seg->B (error otherwise).
 * ---------------------------------------------------------------------------------------------- */
int sc_wsum_fwd(const sc_bf16* h, const float* w, int32_t NL, sc_bf16* out, const sc_segments* seg, int32_t B, int32_t R, int32_t D,
                int32_t row_off, int32_t normalize, void* stream);
/* bwd `flags`: bit 0 = normalize, bit 1 = g is bf16 [B, R, D] instead of fp32 (the attention block of the cascaded+/hybrid+ branches
 * returns its input gradient as the bf16 rows its GEMM wrote; g 16-byte aligned either way) */
int sc_wsum_bwd(const sc_bf16* h, const void* g, int32_t NL, float* dw_partial /*[nblk, NL]*/, int32_t nblk, const sc_segments* seg,
                int32_t B, int32_t R, int32_t D, int32_t row_off, int32_t flags, void* stream);
/* The same sums over RAW hidden states (LayerNorm folded into the encoder GEMMs, see sc_gemm_args): layers n >= first_lazy of h hold
 * the rows in FRONT of the layer's final LayerNorm; stats [NL][B*R][8][2] fp32 their row statistics (ns valid strips), gamma / beta
 * [NL][D] the LayerNorm affines (rows < first_lazy unused): the summed state is (raw - mean) rstd gamma_n + beta_n in fp32. */
int sc_wsum_lazy_fwd(const sc_bf16* h, const float* w, int32_t NL, sc_bf16* out, int32_t B, int32_t R, int32_t D, int32_t row_off,
                     const float* stats, const float* gamma, const float* beta, int32_t first_lazy, int32_t ns, float eps, void* stream);
int sc_wsum_lazy_bwd(const sc_bf16* h, const float* g, int32_t NL, float* dw_partial /*[nblk, NL]*/, int32_t nblk, int32_t B, int32_t R,
                     int32_t D, int32_t row_off, const float* stats, const float* gamma, const float* beta, int32_t first_lazy,
                     int32_t ns, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CLS attention pooling (the query row 0 of the parallel branch's TransformerEncoder layer;
 * avssl/model/kw_branches.py:266-280 -> nn.MultiheadAttention inside TransformerModels.py:48-97).
 * Only the CLS query is consumed by the branch, so K/V are never materialised:
 *   scores[b,h,s] = a[h] . X[b,s]            a[h] = Wk_h^T q_h * dh^-.5  (host side, tiny)
 *   p = softmax_s(scores | s < len[b]) ;  m[b,h,:] = sum_s p[b,h,s] X[b,s,:]
 *   X [B, R, D] bf16 ; a [H, D] fp32 ; len [B] int32 (valid keys incl. CLS) ; H <= 16
 * backward (dm [B,H,D] fp32 given):
 *   dp = dm . X ; ds = p (dp - sum p dp) ; dX = sum_h p dm + ds a ; da_partial[b,h,:] = sum_s ds X
 * train-mode dropout of the attention weights (nn.MultiheadAttention dropout=): mult [B,H,R] fp32 (0 or 1/(1-p_drop),
 *   NULL = none): m = sum_s p*mult X ; psum [B,H] (optional output) = sum_s p*mult, the weight of the value bias.  The backward
 *   takes dp already multiplied by mult, or - cbias [B,H] given - the RAW dp = dm . X and forms (dp + cbias[b,h]) * mult itself
 *   (cbias = the value-bias path, sc_rt_value_bias_bwd); it uses p*mult in the dX term.
 * ---------------------------------------------------------------------------------------------- */
int sc_cls_scores(const sc_bf16* X, const float* vec, int64_t vec_bstride, float* scores, int32_t B, int32_t R,
                  int32_t D, int32_t H, void* stream);
int sc_cls_pool_fwd(const sc_bf16* X, const float* scores, const int32_t* len, float* p, float* m, int32_t B,
                    int32_t R, int32_t D, int32_t H, const float* mult, float* psum, void* stream);
int sc_cls_pool_bwd(const sc_bf16* X, const float* p, const float* dp, const float* dm, const float* a,
                    const int32_t* len, float* dX, float* da_partial, int32_t B, int32_t R, int32_t D, int32_t H,
                    const float* mult, const float* cbias, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Constant-query attention pooling of the fixed-keyword cascaded branch (csrc/kwpool.hip).  Replaces
 * avssl/model/kw_branches.py:365-374 (cat([cls] * bsz) ; self_att ; [:, :keyword_num]) over
 * avssl/module/kw_modules/TransformerModels.py:120-126, for the K keyword rows the branch keeps:
 *   s[b,q,:] = [ c[q, 0..C) ; a[q] . X[b, row0 + t], t < flen[b] ]      a[q] = Wk^T q_q * dh^-.5, c = a . crow^T  (host side, tiny)
 *   p = softmax(s) ; w = p * mult ; m[b,q,:] = sum_j w_j crow[j] + sum_t w_t X[b, row0 + t] ; psum[b,q] = sum w
 *   X [B, R, D] bf16 (frames of utterance b at rows row0 .. row0 + flen[b] - 1; no other row is read) ; a [Q, D], c [Q, C],
 *   crow [C, D] fp32 ; flen [B] int32, 0 allowed ; mult [B, Q, C + R] fp32 or NULL ; Q, C in 1..16 ; D % 64 == 0, D <= 1024.
 *   p [B, Q, C + R]: C constant keys, then one entry per row of X (zero outside the frames) ; m [B, Q, D] ; psum [B, Q] or NULL.
 *   scores / dpw [B, Q, R]: workspace.
 * backward (dm [B,Q,D]; cbias [B,Q] or NULL = the gradient of psum):
 *   dw = dm . key + cbias ; ds = p (dw mult - sum p dw mult) ; dX [B, R, D] fp32 or bf16 (dx_bf16) = sum_q w dm + ds a on the frame rows,
 *   zero elsewhere ; da [Q, D] = sum_b sum_t ds X ; dc [Q, C] = sum_b ds of the constant keys, both summed over b in index order from
 *   da_part [B, Q, D] / dc_part [B, Q, C].  The gradient of crow is sum_{b,q} w[b,q,j] dm[b,q,:] (from p, host side).
 * R is limited by the Q x (C + R) probabilities kept in LDS (twice in the backward): sc_kw_pool_max_rows; past it the entries fail
 * with the numbers.  No atomics: equal inputs give equal bits. */
int sc_kw_pool_max_rows(int32_t Q, int32_t C, int32_t backward);
int sc_kw_pool_fwd(const sc_bf16* X, const float* a, const float* c, const float* crow, const int32_t* flen, float* scores, float* p,
                   float* m, float* psum, const float* mult, int32_t B, int32_t R, int32_t D, int32_t Q, int32_t C, int32_t row0,
                   void* stream);
int sc_kw_pool_bwd(const sc_bf16* X, const float* a, const float* crow, const int32_t* flen, const float* p, const float* mult,
                   const float* dm, const float* cbias, float* dpw, void* dX, int32_t dx_bf16, float* da_part, float* dc_part, float* da,
                   float* dc, int32_t B, int32_t R, int32_t D, int32_t Q, int32_t C, int32_t row0, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row softmax of the GEMM-based attention core (attention block of the cascaded+/hybrid+ branches,
 * avssl/module/kw_modules/TransformerModels.py:101-126 -> nn.MultiheadAttention with head_dim 768 / 128):
 *   forward   P = softmax(scale * scores | key mask)   scores fp32 [rows, n] contiguous (a batched sc_gemm_bf16 output), P bf16;
 *             Pd = keep . P / (1 - p) (train mode, drop_p > 0: the hash mask of sc_gemm_args over element row * n + col)
 *             key_mask uint8 [rows / rows_per_batch, n], non-zero = padded key (probability exactly 0)
 *   backward  dS = scale * P (dP' - sum_k P dP'),  dP' = keep . dP / (1 - p)         dP fp32, dS bf16
 *   n % 4 == 0, n <= 1024.
 * Reads (what the kernels load but the mathematics excludes; line numbers are csrc/softmax.hip's; tested by
 * tests/test_gpu_poison_kw.py, table in docs/parity.md, "Keyword side"):
 *   scores of a masked key       any bits: replaced by -inf as it is loaded (:35-38), P = Pd = exactly 0 there
 *   dP of a key with P = 0       any bits: a key of probability 0 - every masked key - is left out of sum_k P dP' and its dS is
 *                                written as 0 without touching dP (:113-117, :124-126).  dP of such a key is what the GEMM in front
 *                                forms from the V row of a pad frame; 0 x dP' would turn a NaN, an Inf or a finite value that
 *                                dP / (1 - p) overflows into a NaN in every dS of the row.
 *   the columns n .. of a row    never loaded (:32, :96)
 * ---------------------------------------------------------------------------------------------- */
int sc_softmax_fwd(const float* scores, const uint8_t* key_mask, sc_bf16* P, sc_bf16* Pd, int64_t rows, int32_t n,
                   int32_t rows_per_batch, float scale, float drop_p, uint32_t drop_seed, void* stream);
int sc_softmax_bwd(const float* dP, const sc_bf16* P, sc_bf16* dS, int64_t rows, int32_t n, float scale, float drop_p,
                   uint32_t drop_seed, void* stream);
/* fp32 DEBUG mode (SURVEY 8d "fp32 kernel mode (for debugging)"; host side speechclip_plus_amd/debug_fp32.py): the same kernels with
 * unrounded fp32 outputs - softmax probabilities here, the conv layer 0 activations above (out_f32 of sc_conv0_gn_gelu / sc_conv0_ln_gelu);
 * every product of that mode runs on sc_sgemm_mfma_f32 / sc_sgemm_f32_ex, the norms on sc_rowln_f32_fwd, GELU on sc_gelu_f32. */
int sc_softmax_fwd_f32(const float* scores, const uint8_t* key_mask, float* P, int64_t rows, int32_t n, int32_t rows_per_batch,
                       float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Continuous integrate-and-fire accumulation (avssl/module/cif.py:157-240; the downsampler of the cascaded+/hybrid+ branches).
 *   x [B,S,C] fp32, alpha [B,S] fp32 (weights, 0 on padded frames), csum = cumsum(alpha) [B,S] (computed by the caller so
 *   that the slot boundaries floor(csum / thr) are the host framework's), out [B,T+1,C] fp32 (slot T collects the tail;
 *   every slot is written).  Frame s adds lw_s x_s to slot left_s, thr x_s to the slots in between, rw_s x_s to slot right_s.
 *   backward: g [B,T+1,C] -> dx [B,S,C], pa / pb [ceil(C/256), B, S]: per-channel-block partials of
 *   d alpha_s (direct) = x_s . g[left_s]  and  d csum_s = fire_s ? x_s . (g[right_s] - g[left_s]) : 0.        C % 4 == 0.
 * Reads (line numbers are csrc/cif.hip's; tested by tests/test_gpu_poison_kw.py, table in docs/parity.md, "Keyword side").  The
 * kernels take no lengths: alpha = 0 and csum = the running total on the frames behind an utterance's length are OPERANDS
 * (sc_cif_prepare writes them from its pad mask and ignores alpha_raw there, any bits, :366).
 *   x of a frame with alpha = 0  finite: the walk forms lw x = 0 x x into the open slot (:111, :263-266).  pa of such a frame is
 *                                x . g[left] - Inf or NaN for a large finite x; sc_cif_prepare_bwd leaves it out (below)
 *   pa where a_clip = 0          (sc_cif_prepare_bwd) any bits: a frame of weight 0 - every padded frame - is left out of the scaling
 *                                term <g', a> by a select, not multiplied (:466-471); da of a padded frame is written as 0.  pb of a
 *                                padded frame is an operand (the suffix sum): sc_cif_bwd writes an exact 0 there.
 *   g behind slot right_last     any bits, right_last = the slot the last frame lands in (the keyword count): the backward loads
 *                                g[left_s], g[right_s] and the slots between only (:158-182, :308-316).  Slot right_last ITSELF is
 *                                read: the weight left over behind the last fire lands there (1e-5 with the target scaling).
 *   out behind slot right_last   written as zeros (:129-130, :241-243)
 * ---------------------------------------------------------------------------------------------- */
int sc_cif_fwd(const float* x, const float* alpha, const float* csum, float* out, int32_t B, int32_t S, int32_t C, int32_t T,
               float thr, void* stream);
int sc_cif_bwd(const float* x, const float* alpha, const float* csum, const float* g, float* dx, float* pa, float* pb, int32_t B,
               int32_t S, int32_t C, int32_t T, float thr, void* stream);
/* The same kernels on the ROWS of the attention block in front of CIF (round 4): x = frame 0 of utterance 0, fp32 or bf16 (x_bf16), with
 * `xbs` elements between utterances (the block's row pitch x C) - no fp32 copy of the activations.  The gradient leaves in the dtype
 * the frames came in, frame s of utterance b at dx + b dxbs + s C; the zlo rows in front of an utterance's frames and the zhi rows
 * behind them are zero-filled (CLS slot / padding rows of the block's buffer). */
int sc_cif_fwd_rows(const void* x, int32_t x_bf16, int64_t xbs, const float* alpha, const float* csum, float* out, int32_t B, int32_t S,
                    int32_t C, int32_t T, float thr, void* stream);
int sc_cif_bwd_rows(const void* x, int32_t x_bf16, int64_t xbs, const float* alpha, const float* csum, const float* g, void* dx,
                    int32_t dx_bf16, int64_t dxbs, int32_t zlo, int32_t zhi, float* pa, float* pb, int32_t B, int32_t S, int32_t C, int32_t T,
                    float thr, void* stream);
/* buf [lead + B*P + trail, D] bf16: the rows that are not frames <- 0 (the `lead` rows in front, per utterance rows [0, head) and
 * [stop, P), the `trail` rows behind): the zero padding a k-tap conv GEMM reads in place between utterances.  B = 0: lead + trail only. */
int sc_rows_zero_pad_bf16(sc_bf16* buf, int32_t lead, int32_t B, int32_t P, int32_t head, int32_t stop, int32_t trail, int32_t D, void* stream);

/* CIF bookkeeping on the device (avssl/module/cif.py:106-175, 244-297), one workgroup per utterance, no host round trip.
 *   sc_cif_prepare: a = clip(alpha_raw, 0, 1), padded frames (pad != 0) zeroed -> a_clip [B,S] ("orig_alpha") ; quantity = sum a ;
 *     if target && apply_scaling: a *= (thr * target + eps) / quantity (ratio [B] kept for the backward) ; alpha [B,S] ;
 *     csum = inclusive scan [B,S] ; feat_len = clip(floor(sum alpha / thr), 1, max_feat) ; fired [B,S] = slot index advances at the
 *     frame (indices clipped at T) ; flags (8 int32, zeroed once by the caller): [0] += (quantity > 0) ; [1] += (feat_len !=
 *     clip(target, 1, max_feat)) when scaling (the caller sized the output from target) ; [3] += 1 when NO utterance of this call had
 *     a positive quantity (the reference asserts that on every call, cif.py:121) ; [6] += utterances whose zero quantity could not
 *     be rescaled ; [4], [5] scratch of the per-call check (left at 0) ; [2], [7] the caller's.  fp64 sums.
 *   sc_cif_prepare_bwd: pa / pb of sc_cif_bwd + d quantity (gq, may be NULL) -> d alpha_raw [B,S] (suffix sum of d csum, scaling).
 *     PRECONDITION: alpha_raw lies in [0, 1], both ends included (the sigmoid output the product feeds).  No derivative of
 *     clip(alpha_raw, 0, 1) is applied: inside the interval it is 1, and at exactly 0 and 1 torch.clamp passes the gradient too.
 *     For a value outside [0, 1] the forward clips and this gradient is NOT that of the clipped function.  An utterance with
 *     quantity <= 0 (all clipped weights zero; ratio forced to 0 by sc_cif_prepare) gets no gradient through the scaling:
 *     d alpha_raw = gq on its unpadded frames.
 *   sc_cif_tail (inference): tail weight of slot feat_len >= tail_thr -> that row *= thr / weight, feat_len += 1 (clip max_feat),
 *     rows >= feat_len zeroed in out [B,T+1,C]; factor / extend [B] returned for the caller's backward / diagnostics.    S <= 2048. */
int sc_cif_prepare(const float* alpha_raw, int64_t lda, const uint8_t* pad, int64_t ldp, const int64_t* target, int32_t apply_scaling,
                   int32_t B, int32_t S, float thr, float eps, int32_t max_feat, int32_t T, float* a_clip, float* alpha, float* csum,
                   float* quantity, float* ratio, int64_t* feat_len, uint8_t* fired, int32_t* flags, void* stream);
int sc_cif_prepare_bwd(const float* pa, const float* pb, int32_t nblk, int32_t B, int32_t S, const float* a_clip, const uint8_t* pad,
                       int64_t ldp, const float* ratio, const float* quantity, const float* gq, int32_t scaled, float* da, void* stream);
int sc_cif_tail(const float* alpha, const float* csum, int32_t B, int32_t S, int32_t C, int32_t T, float thr, float tail_thr,
                int32_t max_feat, int64_t* feat_len, float* out, float* factor, uint8_t* extend, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Keyword -> CLIP sub-word vector quantiser (cascaded+/hybrid+ tails; csrc/vq.hip).
 *   replaces: GeneralBranch.get_keyword_cosine_score / vq_audio_features (avssl/model/kw_branches.py:158-197) and
 *             SimpleVectorQuantizer.forward (avssl/module/speechclip_c_modules/my_vector_quantizer.py:64-165).
 *   sc_vq_prep_f32     kw [Nk, Et] (row stride ldk) -> kwn_T [Et][ldt] = (kw / max(|kw|, eps))^T (columns >= Nk zero; ldt % 64 == 0),
 *                      rnorm [Nk] = 1 / max(|kw|, eps)                                       (F.normalize, kw_branches.py:170-173)
 *   sc_sgemm_mfma_f32  C [M, N] = A . B^T (+ bias[n]) in exact fp32 on the matrix pipe (v_mfma_f32_32x32x2_f32): the cosine scores
 *                      decide an argmax over the vocabulary and the CIF weights a floor(), so no reduced-precision operand.
 *                      A: [M][K] row-major (a_kmajor 0) or [K][M] (a_kmajor 1); B: [N][K] (the nn.Linear layout) or [K][N].
 *                      any M, N, K (16-byte loads when base and leading dimension allow, element loads otherwise)
 *   sc_sgemm_mfma_f32_split  the same product with the contraction cut into S slices of whole 16-wide K-tiles (partials [S, M, N] fp32:
 *                      the caller's workspace), added in slice order with the bias by a second launch - for products with few output
 *                      tiles and a long K (the keyword projection's 64- and 1600-row products and their weight gradients), which the
 *                      one-slice kernel walks with a handful of workgroups.  sc_sgemm_mfma_slices(M, N, K) = the S to use (1: do not split)
 *   sc_vq_rowstats     x [Nk, ldx] fp32, V columns: columns listed in mask_cols_host (<= 4, host array: the special tokens 0, 2, 3) are
 *                      set to -inf IN PLACE (the reference's x[:, i] += -inf), idx = first argmax, lse_t = LSE(x / temp),
 *                      lse_1 = LSE(x), ent = - sum p log(p + 1e-9) with p = softmax(x)       (my_vector_quantizer.py:80-116)
 *   sc_vq_perplexity   out2[0] = code_perplexity (histogram of idx), out2[1] = prob_perplexity (column means of softmax(x));
 *                      workspaces: partial [nchunk, V] fp32, hist [V + 64] int32 (the last 64 words: per-workgroup entropy partials)
 *   sc_vq_gather_f32   out[n] = table[idx[n]]   (= hard one-hot @ token_embedding)
 *   sc_vq_onehot_f32   dense hard one-hot [Nk, ldo] (module-level subword_prob)
 *   sc_vq_soft_bwd     dx = softmax(x / temp) (t - <softmax, t>) / temp, t = d subword_prob [Nk, ldt]; out bf16 (feeds the bf16
 *                      GEMM dx . normalised table) or fp32; columns V .. Vpad - 1 zero-filled         (straight-through estimator)
 *   sc_vq_norm_bwd_f32 gradient through x / max(|x|, eps)
 * ---------------------------------------------------------------------------------------------- */
int sc_vq_prep_f32(const float* kw, int64_t ldk, int32_t Nk, int32_t Et, float eps, float* kwn_T, int64_t ldt, float* rnorm, void* stream);
/* round 6: x[r, :] * row_scale[r] (row_scale NULL: 1) as three bf16 addends x1 + x2 + x3 (24 significant bits), laid out as the six
 * K-blocks of a product to fp32 accuracy on the bf16 matrix pipe - side 0: [x1 | x1 | x2 | x1 | x3 | x2], side 1: [x1 | x2 | x1 | x3 | x1 | x2];
 * sc_gemm_bf16 (out_f32) over K = 6 Ep on a side-0 and a side-1 operand then sums the products (1,1) (1,2) (2,1) (1,3) (3,1) (2,2), each exact
 * in fp32.  out [Rp][6 Ep] bf16, zero outside [R, E].  Used for the cosine scores the keyword argmax is taken over (was sc_sgemm_mfma_f32). */
int sc_split3_bf16(const float* x, int64_t ldx, const float* row_scale, int32_t R, int32_t E, sc_bf16* out, int32_t Rp, int32_t Ep,
                   int32_t side, void* stream);
int sc_sgemm_mfma_f32(const float* A, int64_t lda, int32_t a_kmajor, const float* B, int64_t ldb, int32_t b_kmajor, float* C, int64_t ldc,
                      int32_t M, int32_t N, int32_t K, const float* bias, void* stream);
int sc_sgemm_mfma_f32_split(const float* A, int64_t lda, int32_t a_kmajor, const float* B, int64_t ldb, int32_t b_kmajor, float* C,
                            int64_t ldc, int32_t M, int32_t N, int32_t K, const float* bias, float* partials, int32_t S, void* stream);
int32_t sc_sgemm_mfma_slices(int32_t M, int32_t N, int32_t K);
int sc_vq_rowstats(float* x, int64_t ldx, int32_t Nk, int32_t V, float temp, const int32_t* mask_cols_host, int32_t n_mask, int64_t* idx,
                   float* lse_t, float* lse_1, float* ent, void* stream);
int sc_vq_perplexity(const float* x, int64_t ldx, int32_t Nk, int32_t V, const int64_t* idx, const float* lse_1, float* partial,
                     int32_t nchunk, int32_t* hist, float* out2, void* stream);
int sc_vq_gather_f32(const float* table, int64_t ldt, const int64_t* idx, float* out, int64_t ldo, int32_t Nk, int32_t Et, void* stream);
int sc_vq_onehot_f32(const int64_t* idx, float* out, int64_t ldo, int32_t Nk, int32_t V, void* stream);
int sc_vq_soft_bwd(const float* x, int64_t ldx, const float* lse_t, const float* t, int64_t ldt, int32_t Nk, int32_t V, int32_t Vpad,
                   float temp, void* dx, int64_t ldd, int32_t out_bf16, void* stream);
int sc_vq_norm_bwd_f32(const float* kw, int64_t ldk, const float* rnorm, const float* dy, int64_t ldy, float eps, float* dx, int64_t ldd,
                       int32_t Nk, int32_t Et, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Keyword detokenisation: per-row top-K over a score matrix (csrc/topk.hip).
 *   replaces: torch.topk(kw_retrevial_score, K) on the CPU in extract_fixed_keyword_neighbors / extract_dynamic_keyword_neighbors
 *             (avssl/util/model_utils.py:101, :230), called once per validation batch by kwClip.py:412-433; the scores it selects
 *             from (F.cosine_similarity, model_utils.py:91-95 / :222-226) come from sc_split3_bf16 + sc_gemm_bf16 above.
 *   sc_topk_rows_f32   scores [rows, ld] fp32 with V valid columns (ld >= V; columns >= V are padding and never candidates) ->
 *                      vals [rows, k] fp32, idx [rows, k] int32, best first.  Order: larger value first, lower column first among
 *                      equal values (a stable descending sort; -0 == +0), NaN above every number (torch.topk), lower column first
 *                      among NaNs.  1 <= k <= 32; V < k: the tail is -inf / -1; rows == 0: no-op.  Deterministic (no atomics).
 *                      16-byte loads when ``scores`` is 16-byte aligned and ld % 4 == 0, element loads otherwise.
 * ---------------------------------------------------------------------------------------------- */
int sc_topk_rows_f32(const float* scores, int64_t ld, int32_t rows, int32_t V, int32_t k, float* vals, int32_t* idx, void* stream);
/* vals[row, r] = cosine of kw[row, :E] and table[idx[row, r], :E] (each norm clamped at eps, F.cosine_similarity) with the three sums
 * accumulated in fp64 and rounded once; idx < 0 (no such neighbour): -inf.  idx must hold indices < V (what sc_topk_rows_f32 wrote).
 * The fp32 score matrix the selection reads carries the accumulation error of 6 E products (up to 3e-6 at a score of 1); the values
 * reported next to the tokens do not. */
int sc_topk_rescore_cos_f32(const float* kw, int64_t ldk, const float* table, int64_t ldt, int32_t V, int32_t E, float eps,
                            const int32_t* idx, int32_t rows, int32_t k, float* vals, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gallery search: the k best gallery rows of every query, the selection fused into the score GEMM (csrc/search.hip).
 *   replaces: torch.argsort(score, descending=True) over the whole score matrix (avssl/module/retrieval.py:45-46) built at
 *             avssl/model/kwClip.py:447-482 - here the [nQ, N] score matrix is never written.
 *   sc_search_slabs      S for (nQ, N, k): the gallery axis is cut into S slabs of whole 128-column tiles, every slab but the last
 *                        full (>= k valid columns), up to two (row tile, slab) workgroups per CU when nQ is small, 1 when the
 *                        row tiles alone do or N fits one tile.
 *   sc_search_topk_bf16  q_split [roundup(nQ, 128), K6] / g_split [roundup(N, 128), K6]: the side-0 / side-1 operands sc_split3_bf16
 *                        writes (K6 = 6 Ep, Ep % 64 == 0, padding rows zero).  Scores = the six K-blocks summed in fp32 on the bf16
 *                        MFMA, K-tiles in increasing order (the arithmetic of sc_gemm_bf16 on the same operands).  Writes, for
 *                        every query and slab, the slab's k best as part_vals / part_idx [nQ, S, k] (fp32 / int32 global gallery
 *                        row), best first, in sc_topk_rows_f32's order: larger value first, lower index first among equal values
 *                        (-0 == +0), NaN above every number, fewer than k columns: -inf / -1 behind them.  Columns >= N never
 *                        enter.  S = 1: the result itself.  S > 1: merge with sc_topk_rows_f32 over [nQ, S k] and gather part_idx
 *                        (lower slab = lower columns, so position order is index order).  1 <= k <= 32; K6 % 384 == 0; S >= 1 and
 *                        S - 1 slabs of ceil(tiles / S) tiles must end before the last tile; nQ == 0: no-op; N == 0: -inf / -1.
 *                        No atomics; results do not depend on S.
 * ---------------------------------------------------------------------------------------------- */
int sc_search_slabs(int32_t nQ, int32_t N, int32_t k);
int sc_search_topk_bf16(const sc_bf16* q_split, const sc_bf16* g_split, int32_t nQ, int32_t N, int32_t K6, int32_t k, int32_t S,
                        float* part_vals, int32_t* part_idx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Retrieval ranks: per query the number of candidates ahead of its best correct candidate, in both directions, computed in the
 * epilogue of the score GEMM (csrc/rank.hip).  Additive in round 14; sc_abi_version() stays 7.
 *   replaces: the sort and rank look-up of avssl/module/retrieval.py:45-121 on the scores of avssl/model/kwClip.py:447-482 - here the
 *             [nA, nB] score matrix is never written and recall at every k, median and mean rank come from two integer vectors.
 *   sc_rank_counts_bf16  a_split [roundup(nA, 128), K6] / b_split [roundup(nB, 128), K6]: sc_search_topk_bf16's operands (side 0 / side 1
 *                        of sc_split3_bf16, K6 = 6 Ep, Ep % 64 == 0, padding rows zero) and its scores, to the bit.  a_ids [nA] /
 *                        b_ids [nB] int64: the pair (i, j) is correct iff a_ids[i] == b_ids[j].  Two launches of one kernel on
 *                        ``stream`` - those of sc_rank_best_bf16 and sc_rank_ahead_bf16 (below) without a mask -: (1) best_a[i] = the largest key over the correct, non-NaN scores of row i, best_b[j] the same of
 *                        column j (atomicMax; key = sc_topk_rows_f32's order as a uint32: float order, -0 == +0; 0 = no such
 *                        candidate); (2) ahead_a[i] = #{j : s_ij > best_i} + #{j not correct : s_ij == best_i or s_ij is NaN} and
 *                        ahead_b[j] its mirror image over rows (int32 atomicAdd).  Rows >= nA / columns >= nB never enter.  All four
 *                        outputs are the caller's and must be ZERO on entry; nothing is allocated.  Integer atomics only: the
 *                        result is bitwise reproducible and does not depend on S.  S: slabs of the nB axis (sc_search_slabs(nA, nB, 1)
 *                        is a good value), S >= 1 (slabs of ceil(tiles / S) column tiles; one past the last tile is empty and adds
 *                        nothing); K6 % 384 == 0; nA == 0 or nB == 0: no-op, returns 0.
 * ---------------------------------------------------------------------------------------------- */
int sc_rank_counts_bf16(const sc_bf16* a_split, const sc_bf16* b_split, const int64_t* a_ids, const int64_t* b_ids, int32_t nA, int32_t nB,
                        int32_t K6, int32_t S, uint32_t* best_a, uint32_t* best_b, int32_t* ahead_a, int32_t* ahead_b, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Compact gallery search: one bf16 copy of the gallery (2 Ep bytes per row), a coarse fused top-D scan, an exact re-rank of the D
 * candidates from the fp32 rows and a per-query certificate (csrc/search_compact.hip).  Additive in round 15; sc_abi_version() stays 7.
 *   replaces: the ranking of avssl/module/retrieval.py:45-46 on the scores of avssl/model/kwClip.py:447-482, as sc_search_topk_bf16 does,
 *             with a sixth of its gallery bytes and matrix work.
 *   sc_rows_bf16           x [R, E] fp32 with row pitch ldx, row_scale [R] or NULL (1) -> out [Rp, Ep] bf16 with
 *                          out[r, i] = bf16_rne(fl32(x[r, i] * row_scale[r])), zero outside [R, E]; Rp % 128 == 0, Ep % 64 == 0.
 *                          norms [3, R] fp32: per row the 2-norm of the scaled row x', of its rounded image x~ and of the residual
 *                          x' - x~ (exact in fp32), each accumulated in fp64 and rounded once.  One pass, memory bound.  R == 0 with
 *                          Rp == 0: no-op.
 *   sc_search_coarse_bf16  sc_search_topk_bf16's contract on plain bf16 operands q_bf16 [roundup(nQ, 128), Ep] / g_bf16
 *                          [roundup(N, 128), Ep] (what sc_rows_bf16 writes; padding rows zero).  scores = sum over Ep of bf16 x bf16
 *                          products on v_mfma_f32_16x16x32_bf16, fp32 accumulation, K-tiles in increasing order.  Writes, per query
 *                          and slab, the slab's D best as part_vals / part_idx [nQ, S, D], best first, in sc_topk_rows_f32's order:
 *                          larger first, lower gallery row first among equals, -0 == +0, NaN on top, -inf / -1 behind the last
 *                          column.  Columns >= N never enter.  1 <= D <= 32; Ep % 64 == 0 (512 works; sc_search_topk_bf16 wants
 *                          K6 % 384 == 0); S as sc_search_slabs(nQ, N, D) rules; merge S > 1 slabs with sc_topk_rows_f32 + a gather.
 *                          nQ == 0: no-op; N == 0: -inf / -1.  No atomics; the result is bit-identical for every S.
 *   sc_search_rerank_f32   q [nQ, E] fp32 (pitch ldq, q_scale [nQ] or NULL), rows [N, E] fp32 (pitch ldr, g_scale [N] or NULL),
 *                          cand_idx / cand_vals [nQ, D] (the merged coarse lists, best first; an index outside [0, N) is a filler and
 *                          is no candidate), eps [nQ] fp32, k <= D <= 32.  Per query: the exact score of every candidate,
 *                          fp32_round(sum_i (double) q'_i * (double) g'_i) with q'_i = fl32(q_i * q_scale), g'_i = fl32(g_i * g_scale)
 *                          and the sum in fp64; the candidates sorted by exact value descending, gallery row ascending, in
 *                          sc_topk_rows_f32's key order (NaN on top, -0 == +0); vals [nQ, k] fp32, idx [nQ, k] int32 (-inf / -1 behind
 *                          the last candidate) and certified [nQ] uint8.  The certificate, evaluated in fp64: 0 if any candidate's
 *                          coarse or exact value, or eps, is not finite; else 1 if N <= D (every row is a candidate); else 1 iff
 *                          e_k - |e_k| 2^-23 > t + eps, e_k the k-th best exact value and t the coarse value of the D-th (last)
 *                          candidate.  A row outside the candidates has a coarse score <= t and an exact score within eps of it, so it
 *                          is strictly below e_k: it cannot enter the list, not even by a tie.  Deterministic, no atomics, nothing
 *                          allocated.  nQ == 0: no-op.
 * ---------------------------------------------------------------------------------------------- */
int sc_rows_bf16(const float* x, int64_t ldx, const float* row_scale, int32_t R, int32_t E, sc_bf16* out, int32_t Rp, int32_t Ep,
                 float* norms, void* stream);
int sc_search_coarse_bf16(const sc_bf16* q_bf16, const sc_bf16* g_bf16, int32_t nQ, int32_t N, int32_t Ep, int32_t D, int32_t S,
                          float* part_vals, int32_t* part_idx, void* stream);
int sc_search_rerank_f32(const float* q, int64_t ldq, const float* q_scale, const float* rows, int64_t ldr, const float* g_scale,
                         const int32_t* cand_idx, const float* cand_vals, const float* eps, int32_t nQ, int32_t N, int32_t E, int32_t D,
                         int32_t k, float* vals, int32_t* idx, uint8_t* certified, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Filtered gallery search: sc_search_topk_bf16 / sc_topk_rows_f32 over the admissible gallery rows only (csrc/search_filter.hip).
 * Additive in round 16; sc_abi_version() stays 7.
 *   replaces: score.masked_fill(mask, -inf) + torch.topk over the whole [nQ, N] matrix of the scores of avssl/model/kwClip.py:447-482
 *             (ranked by avssl/module/retrieval.py:45-46): excluding a query's own item and its sibling captions, mining the k
 *             highest-scoring wrong items of an anchor, dropping removed rows of a built index.
 *   THE RULE (one definition for every layer).  Gallery row j is ADMISSIBLE for query i iff
 *       j < N,  and  live == NULL or live[j] != 0,  and  the ids are NULL or g_ids[j] != q_ids[i].
 *   q_ids [nQ] / g_ids [N] are int64, both or neither, all 64 bits compared, negative values legal; live [N] is uint8.  Neither
 *   g_ids nor live is padded: nothing at or past N is read.  The result is sc_topk_rows_f32's order over the admissible rows only:
 *   larger score first, lower gallery row first among equal scores (-0 == +0), NaN above every number, -inf / -1 behind the last
 *   admissible row.  An inadmissible row never appears, whatever its score (NaN included); an admissible row has the fp32 bits the
 *   unfiltered entry gives it; an admissible row whose score is a real -inf ranks ahead of every filler, in every slab arrangement.
 *   sc_search_topk_filtered_bf16  sc_search_topk_bf16's operands, arithmetic and slabs (S >= 1 slabs of ceil(tiles / S) column
 *                                 tiles; a slab past the last tile is empty).  With a filter any slab may hold fewer than k
 *                                 admissible rows, so the per-slab lists are written as 64-bit words, part [nQ, S, k] uint64, best
 *                                 first: word = key << 32 | ~row (key = sc_topk_rows_f32's order as a uint32: float order,
 *                                 -0 == +0, every NaN 0xffffffff, -inf 0x007fffff), 0 = no entry.  Always merge with
 *                                 sc_search_merge_u64 (S = 1 included: it decodes).  1 <= k <= 32; K6 % 384 == 0; nQ == 0: no-op;
 *                                 N == 0: empty lists.
 *   sc_search_merge_u64           part [nQ, S, k] -> vals [nQ, k] fp32 / idx [nQ, k] int32: per query the k largest words, decoded
 *                                 (a zero comes back as +0, every NaN as the default NaN, no entry as -inf / -1).  Words of
 *                                 distinct rows are distinct, so the order is total and does not depend on S.
 *   sc_topk_rows_filtered_f32     sc_topk_rows_f32's contract (scores [rows, ld], V valid columns, 16-byte loads when the base is
 *                                 16-byte aligned and ld % 4 == 0, vals are the matrix's own bits) with q_ids [rows] / g_ids [V] /
 *                                 live [V].  Inadmissible columns are skipped; the score matrix is not modified.  1 <= k <= 32.
 *   All three: argument checks in front of any launch, no atomics, nothing allocated, bit-identical results for every S and run.
 * ---------------------------------------------------------------------------------------------- */
int sc_search_topk_filtered_bf16(const sc_bf16* q_split, const sc_bf16* g_split, int32_t nQ, int32_t N, int32_t K6, int32_t k, int32_t S,
                                 const int64_t* q_ids, const int64_t* g_ids, const uint8_t* live, uint64_t* part, void* stream);
int sc_search_merge_u64(const uint64_t* part, int32_t nQ, int32_t S, int32_t k, float* vals, int32_t* idx, void* stream);
int sc_topk_rows_filtered_f32(const float* scores, int64_t ld, int32_t rows, int32_t V, int32_t k, const int64_t* q_ids,
                              const int64_t* g_ids, const uint8_t* live, float* vals, int32_t* idx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Filtered compact gallery search: sc_search_coarse_bf16 / sc_search_rerank_f32 over the admissible gallery rows only
 * (csrc/search_compact_filter.hip).  Additive in round 17; sc_abi_version() stays 7.
 *   replaces: what the filtered entries above replace, on the compact index's 2 Ep bytes per gallery row.
 *   THE RULE is the one above, unchanged: gallery row j is ADMISSIBLE for query i iff
 *       j < N,  and  live == NULL or live[j] != 0,  and  the ids are NULL or g_ids[j] != q_ids[i]
 *   (int64, all 64 bits compared, negative values legal).  An inadmissible row never appears, whatever its score (NaN and inf
 *   included), and it spoils nothing.
 *   THE CERTIFICATE OVER ADMISSIBLE ROWS.  The candidates of a query are its D best ADMISSIBLE rows by coarse score (the order
 *   contract is unchanged); t is the coarse value of the last candidate.  Every admissible row outside the candidates has a coarse
 *   score <= t and an exact score within eps of it, so round 15's proof holds verbatim on the admissible set.  Evaluated in fp64:
 *       0 if eps is not finite, or if any candidate's coarse or exact value is not finite;
 *       else 1 if the merged candidate list holds fewer than D entries - every admissible row is then a candidate (this covers fewer
 *            than k admissible rows, where the tail is -inf / -1, and no admissible row at all, where the empty list is the exact
 *            answer; it replaces sc_search_rerank_f32's N <= D clause);
 *       else 1 iff e_k - |e_k| 2^-23 > t + eps.
 *   eps must bound |exact - coarse| over the rows that can be admissible: the caller takes the three gallery norms over the LIVE rows
 *   (a superset of every query's admissible rows is sound, so id exclusions need not enter the bounds).
 *   sc_search_coarse_filtered_bf16  sc_search_coarse_bf16's operands, arithmetic, tile and K-tile order: an admissible row carries the
 *                                   fp32 bits sc_search_coarse_bf16 gives it.  q_ids [nQ] / g_ids [N] int64 (both or neither), live
 *                                   [N] uint8 or NULL, none of them padded: nothing at or past N is read.  S >= 1 slabs of
 *                                   ceil(tiles / S) column tiles, any S (a slab past the last tile is empty).  Writes the per-slab
 *                                   lists as 64-bit words, part [nQ, S, D] uint64, best first: key << 32 | ~row, 0 = no entry
 *                                   (sc_search_topk_filtered_bf16's format).  Always merge and decode with sc_search_merge_u64.
 *                                   1 <= D <= 32; Ep % 64 == 0; nQ == 0: no-op; N == 0: empty lists.
 *   sc_search_rerank_filtered_f32   sc_search_rerank_f32's operands and its fp64 accumulation of the fp32-scaled rows (a candidate
 *                                   index outside [0, N) is a filler), with the certificate above.
 *   Both: argument checks in front of any launch, no atomics, nothing allocated, bit-identical results for every S and run.
 * ---------------------------------------------------------------------------------------------- */
int sc_search_coarse_filtered_bf16(const sc_bf16* q_bf16, const sc_bf16* g_bf16, int32_t nQ, int32_t N, int32_t Ep, int32_t D, int32_t S,
                                   const int64_t* q_ids, const int64_t* g_ids, const uint8_t* live, uint64_t* part, void* stream);
int sc_search_rerank_filtered_f32(const float* q, int64_t ldq, const float* q_scale, const float* rows, int64_t ldr, const float* g_scale,
                                  const int32_t* cand_idx, const float* cand_vals, const float* eps, int32_t nQ, int32_t N, int32_t E,
                                  int32_t D, int32_t k, float* vals, int32_t* idx, uint8_t* certified, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Wide gallery search: per-row top-K for k in the hundreds over a score matrix (csrc/topk_wide.hip).  Additive in round 18;
 * sc_abi_version() stays 7.
 *   replaces: torch.argsort(score, descending=True) over the whole score matrix (avssl/module/retrieval.py:45-46), the ranking that is
 *             computed and dropped - here the first k <= 1024 entries of every row of it, for callers that want the list itself at
 *             @50 / @100, 64 to 256 hard negatives per anchor, or a top-200 shortlist for a slower re-scorer.
 *   sc_topk_rows_wide_f32  scores [rows, ld] fp32 with V valid columns (ld >= V; columns >= V are padding, never candidates and never
 *                          read) -> vals [rows, k] fp32, idx [rows, k] int32, best first.  33 <= k <= 1024 is the range it is meant
 *                          for; 1 <= k <= 1024 is accepted so that it can be compared with sc_topk_rows_f32.  V <= 2^30.
 *                          q_ids [rows] / g_ids [V] int64 (both or both NULL), live [V] uint8 or NULL.
 *                          THE ORDER is sc_topk_rows_f32's, word for word: larger value first; the lower column first among equal
 *                          values (-0 == +0); NaN above every number, the lower column first among NaNs; fewer than k eligible
 *                          columns: -inf / -1 behind them; vals are the matrix's own bits (-0, NaN payloads), re-read at the end;
 *                          rows == 0: no-op; no float atomics, the same input gives the same bits.
 *                          THE FILTER is the rule above: column j is eligible iff j < V, live is NULL or live[j] != 0, and the ids
 *                          are NULL or g_ids[j] != q_ids[row].  An ineligible column behaves as absent, whatever its score (NaN
 *                          included); an eligible real -inf ranks ahead of every filler.  The score matrix is not modified.
 *                          One workgroup per row: an exact radix select of the k-th key over LDS histograms (three passes), one
 *                          admitting pass (a block prefix count in column order decides among the columns equal to the k-th key, so
 *                          a row of V equal scores is no special case), a sort of the k words in LDS.  16-byte loads when ``scores``
 *                          is 16-byte aligned and ld % 4 == 0, element loads otherwise.  Argument checks in front of the launch,
 *                          nothing allocated.
 * ---------------------------------------------------------------------------------------------- */
int sc_topk_rows_wide_f32(const float* scores, int64_t ld, int32_t rows, int32_t V, int32_t k, const int64_t* q_ids,
                          const int64_t* g_ids, const uint8_t* live, float* vals, int32_t* idx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sharded gallery search: the exact merge of per-shard lists of up to 1024 entries (csrc/search_merge_wide.hip).  Additive in round
 * 21; sc_abi_version() stays 7.
 *   replaces: the gather of every rank's embeddings onto one device before the ranking of avssl/module/retrieval.py:45-46 can run, and
 *             the 262 144-row limit of the wide selection: every shard (a row range of the gallery, on this device or on another
 *             rank) is searched on its own and only the k-entry lists meet.
 *   sc_search_merge_lists_f32  part_vals (fp32) / part_idx (int32): entry (s, q, j) lies at s * shard_stride + q * k + j - the natural
 *                              layout is [S, nQ, k]; with shard_stride >= nQ k a slice of query rows of a larger buffer merges
 *                              without a copy.  List (s, q) is what the search entries above return for shard s: best first under
 *                              the order contract, part_idx a row OF THE SHARD, -1 = no entry.  row0 [S] int64 (a device pointer):
 *                              the global row of every shard's row 0; the shards are disjoint row ranges of one gallery and every
 *                              global row must be < 2^31 - 1.  -> vals [nQ, k] fp32, idx [nQ, k] int32 (the GLOBAL row, or -1): per
 *                              query the k best entries over all S lists, best first.
 *                              THE ORDER is sc_topk_rows_f32's over global rows: larger value first; the lower global row first
 *                              among equal values (-0 == +0); NaN above every number, the lower global row first among NaNs;
 *                              -inf / -1 behind the last entry.  An input entry is a filler iff its part_idx < 0, whatever its
 *                              value; a real -inf with part_idx >= 0 ranks ahead of every filler, whichever shard holds it.
 *                              vals carry the INPUT'S OWN 32 bits (-0 stays -0, NaN payloads stay): the 64-bit word key << 32 | ~row
 *                              is only the sort key, the value bits travel beside it.
 *                              1 <= k <= 1024, S >= 1, shard_stride >= 0 (and >= nQ k when S > 1); nQ == 0: no-op; S == 1: a copy
 *                              with the row offset applied.  One workgroup per group of queries, the running list in 12 KiB of LDS,
 *                              log2(roundup_pow2(k)) compare-exchange steps per further shard.  The lists being best first matters
 *                              for the result only, never for memory safety: no address depends on a value or a row.  Argument
 *                              checks in front of the launch, no atomics, nothing allocated, the same input gives the same bits.
 * ---------------------------------------------------------------------------------------------- */
int sc_search_merge_lists_f32(const float* part_vals, const int32_t* part_idx, int64_t shard_stride, const int64_t* row0, int32_t nQ,
                              int32_t S, int32_t k, float* vals, int32_t* idx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Retrieval ranks in parts: sc_rank_counts_bf16's two phases as two accumulating entries, with a removed-row mask on B
 * (csrc/rank.hip: the same kernel, the same argument checks).  Additive in round 22; sc_abi_version() stays 7.
 *   replaces: the gather of every rank's embeddings onto one device before the sort-and-look-up of avssl/module/retrieval.py:45-121
 *             can run: every (A range, B range) pair - a shard of the gallery, on this device or on another rank - is scored on its
 *             own and only keys and counts meet.
 *   Operands are sc_rank_counts_bf16's (a_split / b_split rows padded to 128, K6 % 384 == 0, int64 ids), its scores to the bit, its
 *   keys and its counting rule.  b_live: NULL, or uint8 [nB]; column j takes part iff b_live == NULL or b_live[j] != 0.  A dead column
 *   is neither a candidate of any row nor a query of the column direction, whatever its data (NaN included), and nothing is written
 *   to best_b[j] / ahead_b[j].
 *   THE PROTOCOL.  The caller zeroes best_a [nA], best_b [nB], ahead_a [nA], ahead_b [nB] ONCE, calls sc_rank_best_bf16 for every
 *   (A range, B range) pair with the ranges' slices of the four buffers, then - after every "best" call, and after a MAX-reduction of
 *   the keys where the pairs ran in different places - sc_rank_ahead_bf16 for every pair.  The accumulated result is what
 *   sc_rank_counts_bf16 gives on the whole of A against the live rows of the whole of B, bit for bit.
 *   sc_rank_best_bf16   one launch: atomicMax of the largest key over correct (a_ids[i] == b_ids[j]), non-NaN, live pairs into
 *                       best_a[i] / best_b[j]; key 0 = none.  Calling it twice changes nothing.
 *   sc_rank_ahead_bf16  one launch: READS best_a / best_b; atomicAdd into ahead_a[i] of #{j live : s_ij > best_a[i]} + #{j live, not
 *                       correct : s_ij == best_a[i] or s_ij is NaN}, and the mirror image into ahead_b[j] of the live columns.
 *                       Calling it twice doubles the counts.
 *   Both: only integer atomics, so the result does not depend on S, on the run or on the order of the calls; no address depends on
 *   a score, a key, an id or a mask byte; nothing at or past nA / nB is read of ids, mask, keys or counts; nothing is allocated;
 *   argument checks in front of the launch; S >= 1 as for sc_rank_counts_bf16; nA == 0 or nB == 0: no-op, returns 0.
 * ---------------------------------------------------------------------------------------------- */
int sc_rank_best_bf16(const sc_bf16* a_split, const sc_bf16* b_split, const int64_t* a_ids, const int64_t* b_ids, const uint8_t* b_live,
                      int32_t nA, int32_t nB, int32_t K6, int32_t S, uint32_t* best_a, uint32_t* best_b, void* stream);
int sc_rank_ahead_bf16(const sc_bf16* a_split, const sc_bf16* b_split, const int64_t* a_ids, const int64_t* b_ids, const uint8_t* b_live,
                       int32_t nA, int32_t nB, int32_t K6, int32_t S, const uint32_t* best_a, const uint32_t* best_b, int32_t* ahead_a,
                       int32_t* ahead_b, void* stream);

/* Keyword BatchNorm: nn.BatchNorm1d over the keyword positions (avssl/module/speechclip_c_modules/kw_bn.py:167-228).
 *   x [N, E] fp32 (N = batch x keyword slots), per-channel statistics.  training: batch statistics (biased variance for the
 *   normalisation, unbiased for the running estimate; run_mean / run_var updated in place with `momentum`), save_mean / save_rstd
 *   kept for the backward; inference: the running estimates.  backward (training statistics): dx, dgamma [E], dbeta [E]. */
int sc_bn_rows_fwd(const float* x, int64_t ldx, int32_t N, int32_t E, const float* gamma, const float* beta, float* run_mean,
                   float* run_var, int32_t training, float momentum, float eps, float* y, int64_t ldy, float* save_mean,
                   float* save_rstd, void* stream);
int sc_bn_rows_bwd(const float* x, int64_t ldx, const float* dy, int64_t ldg, int32_t N, int32_t E, const float* gamma,
                   const float* save_mean, const float* save_rstd, float* dx, int64_t ldd, float* dgamma, float* dbeta, void* stream);
/* The fixed-count form (kw_bn.py:47-49,115-123: `eachKw` + `parallel`, nn.BatchNorm1d(Ed * K) over keywords.permute(0, 2, 1).reshape(B, -1)):
 *   x, y, dy, dx [B, K, Ed] fp32 contiguous; one statistic per (keyword slot k, channel d) over the B rows; gamma, beta, run_mean, run_var,
 *   save_mean, save_rstd, dgamma, dbeta hold (k, d) at index d * K + k - the reference checkpoint's layout, read in place. */
int sc_bn_eachkw_fwd(const float* x, int32_t B, int32_t K, int32_t Ed, const float* gamma, const float* beta, float* run_mean, float* run_var,
                     int32_t training, float momentum, float eps, float* y, float* save_mean, float* save_rstd, void* stream);
int sc_bn_eachkw_bwd(const float* x, const float* dy, int32_t B, int32_t K, int32_t Ed, const float* gamma, const float* save_mean,
                     const float* save_rstd, float* dx, float* dgamma, float* dbeta, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp32 strided GEMM  C[i,j] = alpha * sum_k A[i*sai + k*sak] * Bm[j*sbj + k*sbk]  (+ bias[j])
 *   small fp32 products of the loss and of the CLS-row tail (logits = A.B^T / tau, dA = G.B, ...)
 * ---------------------------------------------------------------------------------------------- */
int sc_sgemm_f32(const float* A, int64_t sai, int64_t sak, const float* Bm, int64_t sbj, int64_t sbk, float* C,
                 int64_t ldc, int32_t M, int32_t N, int32_t K, float alpha, const float* bias, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row kernels of the backward pass over bf16 activations (CLIP text tower input gradient, HuBERT layer backward):
 *   sc_layernorm_bwd_bf16 : dx = LayerNorm'(x; gamma)(dy) (+ dres), statistics recomputed from the saved LN input x;
 *                           optional per-workgroup partial sums [n_partial, D] of dgamma = sum dy xhat and dbeta = sum dy
 *                           (n_partial = workgroups launched; reduce with sc_colsum_f32)
 *   sc_act_bf16           : df == NULL: out = act(u) ; else out = df * act'(u) ; act 1 = erf-GELU, 2 = QuickGELU
 * ---------------------------------------------------------------------------------------------- */
int sc_layernorm_bwd_bf16(const sc_bf16* x, int64_t ldx, const sc_bf16* dy, int64_t lddy, const float* gamma, const sc_bf16* dres,
                          int64_t lddres, sc_bf16* dx, int64_t lddx, int64_t rows, int32_t D, float eps, float* dgamma_partial,
                          float* dbeta_partial, int32_t n_partial, void* stream);
/* the same pass with what the NEXT products of a differentiated layer's backward read (round 4): dx_drop (may be NULL) = F.dropout of the
 * stored dx with the stateless mask of element row*D + col (drop_p = 0: a plain copy is not written - pass NULL), dsum_partial
 * [n_partial, D] (may be NULL; needs the parameter partial buffers) = partial column sums of dx_drop's values (of dx when drop_p = 0):
 * the bias gradient of the residual branch behind this LayerNorm - no dropout launch, no column-sum pass */
int sc_layernorm_bwd_drop_bf16(const sc_bf16* x, int64_t ldx, const sc_bf16* dy, int64_t lddy, const float* gamma, const sc_bf16* dres,
                               int64_t lddres, sc_bf16* dx, int64_t lddx, int64_t rows, int32_t D, float eps, float* dgamma_partial,
                               float* dbeta_partial, int32_t n_partial, sc_bf16* dx_drop, int64_t lddd, float drop_p, uint32_t drop_seed,
                               float* dsum_partial, void* stream);
/* out[b*R + t] = (prev ? prev[..] : 0) + bf16(w[0] * dX[b, t + row_off]) for t < T (rows t >= T: prev or 0): the gradient reaching hidden
 * state n of a differentiated encoder = what came down from layer n + 1 + its share of the weighted sum's gradient dX (fp32 [B, R, D]) */
int sc_wsum_share_bf16(const float* dX, const float* w, const sc_bf16* prev, sc_bf16* out, int32_t B, int32_t R, int32_t T, int32_t D,
                       int32_t row_off, void* stream);
int sc_act_bf16(const sc_bf16* u, const sc_bf16* df, sc_bf16* out, int64_t n, int32_t act, void* stream);
/*   sc_transpose_bf16 : y[c, r] = x[r, c]  - operands of the weight-gradient GEMMs (dW = dY^T X: the row index becomes the
 *                       contraction dimension of sc_gemm_bf16, split along K over the batch dimension, partials in fp32)
 *   sc_colsum_bf16    : partial[blk, c] = sum of the block's rows of x[:, c] in fp32 (bias gradients; reduce with sc_colsum_f32) */
/*   sc_transpose_batched_bf16 : nbatch equally shaped [rows, cols] matrices, matrix z starting sx / sy elements after matrix z - 1 */
int sc_transpose_batched_bf16(const sc_bf16* x, int64_t ldx, int64_t sx, sc_bf16* y, int64_t ldy, int64_t sy, int32_t rows, int32_t cols,
                              int32_t nbatch, void* stream);
/*   sc_cast_transpose_f32_bf16 : the bf16 working copies of an fp32 [rows, cols] weight in one pass - y = bf16(x) (same layout) and /
 *   or yT = bf16(x)^T [cols, rows]; either may be NULL.  rows, cols, leading dims multiples of 4. */
int sc_cast_transpose_f32_bf16(const float* x, int64_t ldx, sc_bf16* y, int64_t ldy, sc_bf16* yT, int64_t ldyT, int32_t rows, int32_t cols,
                               void* stream);
/*   sc_dropout_bf16   : out = dropout(x) (F.dropout semantics, the stateless mask of sc_gemm_args over element row*D + col):
 *                       fairseq's encoder dropout after pos_conv + LayerNorm (speech_encoder_plus.py:41), train mode only */
int sc_dropout_bf16(const sc_bf16* x, int64_t ldx, sc_bf16* out, int64_t ldo, int64_t rows, int32_t D, float p, uint32_t seed,
                    void* stream);
/* the multiplier F.dropout applies, as fp32: out[i] = keep(i, seed) ? 1 / (1 - p) : 0, keep = the stateless hash mask above
 * (element index i); n % 8 == 0.  The CLS head's four masks (nn.TransformerEncoderLayer dropout / dropout1 / dropout2 and the
 * attention-weight dropout, avssl/module/kw_modules/TransformerModels.py:61-81) are products with these. */
int sc_dropout_mult_f32(float* out, int64_t n, float p, uint32_t seed, void* stream);
int sc_transpose_bf16(const sc_bf16* x, int64_t ldx, sc_bf16* y, int64_t ldy, int32_t rows, int32_t cols,
                      float* colsum_partial /* NULL, or [ceil(rows / 64), cols] fp32: per-64-row-block column sums of x */, void* stream);
/* input gradient of a channels-last Conv1d(k = 3, stride 2) run as a strided-row GEMM (fully trainable HuBERT, conv layers 1-4):
 * dcols [M, 3C] = dy . W -> dx [2M, C]:  dx[2m] = dcols[m][0:C] + dcols[m-1][2C:3C],  dx[2m+1] = dcols[m][C:2C]   (one pass) */
int sc_conv_overlap_add_bf16(const sc_bf16* dcols, sc_bf16* dx, int64_t M, int32_t C, void* stream);
/* the same followed by the backward of the activation that produced the conv's input (u [2M, C] = its kept pre-activation):
 * dx <- bf16(dx) * act'(u), bit-identical to sc_conv_overlap_add_bf16 + sc_act_bf16(u, dx) in one pass */
int sc_conv_overlap_add_act_bf16(const sc_bf16* dcols, const sc_bf16* u, sc_bf16* dx, int64_t M, int32_t C, int32_t act, void* stream);
int sc_colsum_bf16(const sc_bf16* x, int64_t ldx, int64_t rows, int32_t cols, float* partial, int32_t nblk, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One-row-per-utterance tail of the parallel head in fp32 on the master weights:
 *   nn.TransformerEncoderLayer (post-LN, GELU) row 0 + final LayerNorm + Linear, as instantiated by
 *   avssl/module/kw_modules/TransformerModels.py:48-97 and consumed at avssl/model/kw_branches.py:266-280.
 *   sc_sgemm_f32_ex : C[z][i,j] = alpha sum_k A[z][i*sai + k*sak] B[z][j*sbj + k*sbk] (+ bias[z][j]) + beta C[z][i,j]
 *                     (beta = 1 accumulates weight gradients straight into the flat gradient buffer; with a workspace,
 *                     few-tile products are split along K and the slices reduced in order)
 *   sc_rowln_f32_fwd: y = LayerNorm(x + res) gamma + beta ; res_stride 0 broadcasts one residual row (the CLS token)
 *   sc_rowln_f32_bwd: dx ; dgamma += sum_rows dy xhat ; dbeta += sum_rows dy   (fixed row order, no atomics)
 *   sc_gelu_f32     : df == NULL: out = gelu(u) (erf form) ; else out = df * gelu'(u)
 *   sc_colsum_f32   : out[j] = beta out[j] + alpha sum_i x[i*ld + j]
 *   sc_headmask_f32 : dir 0: Qm[h,j] = q[j] if j / dh == h else 0 ; dir 1: q[j] = Qm[j / dh, j]
 * ---------------------------------------------------------------------------------------------- */
int sc_sgemm_f32_ex(const float* A, int64_t sai, int64_t sak, int64_t saz, const float* Bm, int64_t sbj, int64_t sbk,
                    int64_t sbz, float* C, int64_t ldc, int64_t scz, int32_t M, int32_t N, int32_t K, int32_t nbatch,
                    float alpha, float beta, const float* bias, int64_t sbiasz, float* workspace, int64_t workspace_floats,
                    void* stream);
int sc_rowln_f32_fwd(const float* x, const float* res, int64_t res_stride, const float* gamma, const float* beta, float* y,
                     float* xhat, float* rstd, int32_t rows, int32_t D, float eps, void* stream);
int sc_rowln_f32_bwd(const float* dy, const float* xhat, const float* gamma, const float* rstd, float* dx, float* dgamma_acc,
                     float* dbeta_acc, int32_t rows, int32_t D, void* stream);
int sc_gelu_f32(const float* u, const float* df, float* out, int64_t n, void* stream);
int sc_colsum_f32(const float* x, int64_t ld, int32_t rows, int32_t cols, float* out, float alpha, float beta, void* stream);
int sc_headmask_f32(float* q, float* Qm, int32_t H, int32_t D, int32_t dh, int32_t dir, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Masked contrastive loss: MaskedContrastiveLoss.forward, avssl/module/losses.py:185-245 (ctor options :130-168).
 *   logits[i,j] = inv_temp <A_i, B_j> - margin [i == j]        A, B [Bg, E] fp32 (unit-norm rows), inv_temp: DEVICE scalar
 *   neg[i,j] = (ids ? ids[i] != ids[j] : i != j) || (!dcl && i == j)           (no MAX_EYE = 256 cap, losses.py:126)
 *   loss = 1 / (Bg n_dir) sum_i [ a2b (-l_ii + log sum_j neg_ij e^{l_ij}) + b2a (-l_ii + log sum_j neg_ji e^{l_ji}) ]
 *   sc_infonce_fwd : ONE launch - 64 x 64 logit tiles on the matrix pipe in exact fp32, LDS-tiled operands, per-tile masked
 *                    (max, sum exp) partials, merged by the last-arriving workgroup (ticket) into lse_row / lse_col [Bg] and
 *                    loss[0]; the scaled logits [Bg, Bg] are kept for the backward.  workspace: sc_infonce_workspace_floats(Bg)
 *                    floats, ZEROED once by the caller before the first use (holds the ticket word; each launch leaves it 0),
 *                    one workspace per stream.  E % 4 == 0.
 *   sc_infonce_grad: G = inv_temp gscale dloss/dlogits [Bg, Bg] (dA = G . B, dB = G^T . A: sc_sgemm_mfma_f32), and
 *                    dlogit_dot[i] = sum_j dloss/dlogit_ij <A_i, B_j>  (d loss / d inv_temp = sum_i dlogit_dot[i])
 * ---------------------------------------------------------------------------------------------- */
int64_t sc_infonce_workspace_floats(int32_t Bg);
int sc_infonce_fwd(const float* A, const float* B, int32_t Bg, int32_t E, const int64_t* ids, const float* inv_temp, float margin,
                   int32_t dcl, int32_t a2b, int32_t b2a, float* logits, float* lse_row, float* lse_col, float* loss,
                   float* workspace, void* stream);
int sc_infonce_grad(const float* logits, const int64_t* ids, const float* lse_row, const float* lse_col, int32_t Bg,
                    const float* gscale /*device scalar*/, const float* inv_temp /*device scalar*/, float margin, int32_t dcl,
                    int32_t a2b, int32_t b2a, float* G, float* dlogit_dot /*[Bg]*/, void* stream);

/* Mined negatives beside the batch (csrc/infonce_neg.hip): the a2b denominator of the loss above (avssl/module/losses.py:185-245, whose
 * negatives are the batch alone) extended by, per anchor, a list of rows of a constant bank.  bank [N, E] fp32 with row stride
 * bank_stride (floats, % 4), bank_ids [N] int64 or NULL (with ids, both or neither), neg_idx [Bg, M] int64 in the form hard_negatives
 * returns, 1 <= M <= 1024, N < 2^31.  Slot (i, n), r = neg_idx[i, n], TAKES PART iff 0 <= r < N and (ids given) bank_ids[r] equals the id
 * of no row of the batch (Bg <= 8192 with ids); other slots contribute through selects: their rows are never read.
 *   sc_infonce_neg_fwd : reads the plain call's lse_row / lse_col / logits (the diagonal) and writes x [Bg, M] = inv_temp <A_i, bank[r]>
 *                        (-inf where the slot takes no part), used [Bg] (slots that took part), lse_row_ext[i] = log(e^{lse_row_i} +
 *                        sum_n e^{x_in}) and loss[0] recomputed from lse_row_ext, lse_col and the diagonal in sc_infonce_fwd's order (no
 *                        slot taking part: the plain call's bits).  a2b must be set.  workspace: sc_infonce_neg_workspace_floats(Bg, M)
 *                        floats, no initial contents needed.  Two launches; no atomics.
 *   sc_infonce_neg_grad: dA [Bg, E] (holding G . B) += gscale / (Bg n_dir) inv_temp sum_n p_in bank[r_in], and dlogit_dot[i] += gscale /
 *                        (Bg n_dir) sum_n p_in x_in / inv_temp, p_in = e^{x_in - lse_row_ext_i}; x = -inf marks the empty slots.  The in-batch
 *                        gradient is sc_infonce_grad handed lse_row_ext.  The bank gets no gradient.
 * Bg == 0: no launch.  Deterministic: the same operands give the same bits on every call. */
int sc_infonce_neg_workspace_floats(int32_t Bg, int32_t M);   /* the count itself (0: no anchor or no legal M), -1: too many */
int sc_infonce_neg_fwd(const float* A, const float* bank, int64_t bank_stride, const int64_t* neg_idx, const int64_t* ids,
                       const int64_t* bank_ids, const float* inv_temp /*device scalar*/, const float* lse_row, const float* lse_col,
                       const float* logits, int32_t Bg, int32_t E, int64_t N, int32_t M, int32_t a2b, int32_t b2a, float* x,
                       int32_t* used, float* lse_row_ext, float* loss, float* workspace, void* stream);
int sc_infonce_neg_grad(const float* bank, int64_t bank_stride, const int64_t* neg_idx, const float* x, const float* lse_row_ext,
                        const float* gscale /*device scalar*/, const float* inv_temp /*device scalar*/, int32_t Bg, int32_t E, int64_t N,
                        int32_t M, int32_t a2b, int32_t b2a, float* dA, float* dlogit_dot /*[Bg]*/, void* stream);

/* CIF weight head (avssl/module/cif.py:106-129: ... Conv1d -> Dropout(0.5) -> ReLU -> Dropout(0.5) -> Linear(C, 1) -> Sigmoid): everything
 * behind the conv GEMM in one row kernel, forward and backward.  y [rows, C] fp32 = the conv output (bias included), w [C], bias [1]:
 *   alpha[row] = sigmoid(bias + sum_c w[c] m2 relu(m1 y[row, c]))     m1 / m2: dropout multipliers (p1 / p2, 0 in eval), keep bits =
 *   sc_dropout_mult_f32's for the seed on the index row * C + c.   backward: dy, and per-block partial sums dw_partial [nblk, C],
 *   db_partial [nblk] (reduce with sc_colsum_f32). */
int sc_cif_head_fwd(const float* y, int64_t ldy, const float* w, const float* bias, float* alpha, int32_t rows, int32_t C, float p1,
                    uint32_t seed1, float p2, uint32_t seed2, void* stream);
int sc_cif_head_bwd(const float* y, int64_t ldy, const float* w, const float* alpha, const float* dalpha, float* dy, int64_t lddy,
                    float* dw_partial, float* db_partial, int32_t nblk, int32_t rows, int32_t C, float p1, uint32_t seed1, float p2,
                    uint32_t seed2, void* stream);
/* dy as bf16 rows (dy_bf16 != 0: what the input-gradient GEMM of the weight conv reads) or fp32 */
int sc_cif_head_bwd_rows(const float* y, int64_t ldy, const float* w, const float* alpha, const float* dalpha, void* dy, int32_t dy_bf16,
                         int64_t lddy, float* dw_partial, float* db_partial, int32_t nblk, int32_t rows, int32_t C, float p1, uint32_t seed1,
                         float p2, uint32_t seed2, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row tail of the parallel head, round 3 (csrc/rowtail.hip): the B-row products of nn.TransformerEncoderLayer + final LayerNorm +
 * Linear (avssl/module/kw_modules/TransformerModels.py:48-97, avssl/model/kw_branches.py:266-280) and the L2 normalisation of
 * avssl/model/kwClip.py:857,913-915, fp32 on the master weights.
 *   sc_rt_gemm: C[z] = epi(alpha A[z] . B[z]^T) on the matrix pipe in exact fp32, 64 x 64 tiles.  A [M, K] row-major (then it may be
 *     given as a_ns partial slices that are added on load, plus a_bias[k] * a_rowscale[row][k / a_group]) or contraction-major
 *     [K, M] (a_kmajor); B [N, K] or [K, N] (b_kmajor).  S > 1 splits the contraction: slice s writes its raw partial tile to
 *     C + s * c_slice and the CONSUMER adds the slices (no reduce launch, no epilogue).  S = 1: v = alpha acc + bias[n]; act = 1:
 *     U = v (if given), v = gelu_erf(v); dropout (keep bits = sc_dropout_mult_f32's on the index row * N + col); v += beta C; store.
 *     gb (a_kmajor only): gb[m] += sum_k A[k][m] - the bias gradient as a by-product of a weight-gradient product.
 *   sc_rt_gemm_slices: the S this library would pick for a few-row product (enough workgroups to cover the chip).
 *   sc_rt_ln_fwd: z = (sum_s y_s + bias) * dropout + residual ; out1 = LN1(z) [; out2 = LN2(out1)], xhat / rstd kept.
 *   sc_rt_ln_bwd: d = sum_s dy_s (+ add) ; dx = LayerNorm backward ; dx_masked = dx * dropout multiplier (optional) ; dgamma / dbeta +=.
 *   sc_rt_l2norm_fwd / _bwd: x = sum_s y_s + bias ; e = x / |x| ; backward dx = (g - e <g, e>) / |x|.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float* A; int64_t lda, a_slice, a_z; int32_t a_kmajor, a_ns;
    const float* a_bias; const float* a_rowscale; int32_t a_group, a_nscale;
    const float* B; int64_t ldb, b_z; int32_t b_kmajor, nbatch;
    float* C; int64_t ldc, c_slice, c_z;
    float* U;
    int32_t M, N, K, S;
    float alpha, beta;
    const float* bias; int64_t bias_z;
    int32_t act; float drop_p; uint32_t drop_seed; int32_t pad_;
    float* gb; int64_t gb_z;
} sc_rt_gemm_args;
int sc_rt_gemm(const sc_rt_gemm_args* args, void* stream);
int32_t sc_rt_gemm_slices(int32_t M, int32_t N, int32_t K, int32_t nbatch);
typedef struct {
    const float* y; int64_t y_slice; int32_t ns, rows;
    const float* bias;
    float drop_p; uint32_t drop_seed;
    const float* res; int64_t res_stride;
    const float *g1, *b1; float *out1, *xhat1, *rstd1;
    const float *g2, *b2; float *out2, *xhat2, *rstd2;
    float eps1, eps2; int32_t D, pad_;
} sc_rt_ln_args;
int sc_rt_ln_fwd(const sc_rt_ln_args* args, void* stream);
typedef struct {
    const float* dy; int64_t dy_slice; int32_t ns, rows;
    const float* add;
    const float *xhat, *gamma, *rstd;
    float *dx, *dx_masked;
    float drop_p; uint32_t drop_seed;
    float *dgamma, *dbeta;
    int32_t D, pad_;
} sc_rt_ln_bwd_args;
int sc_rt_ln_bwd(const sc_rt_ln_bwd_args* args, void* stream);
int sc_rt_l2norm_fwd(const float* y, int64_t y_slice, int32_t ns, const float* bias, float* x /*or NULL*/, float* e, float* rnorm,
                     int32_t rows, int32_t D, void* stream);
int sc_rt_l2norm_bwd(const float* g, const float* e, const float* rnorm, float* dx, int32_t rows, int32_t D, void* stream);
/* value-bias terms of the CLS head under attention-weight dropout (ctx_h = Wv_h m_h + bv_h * psum[b,h]):
 *   cbias[b,h] = sum_j dctx[b, h dh + j] bv[h dh + j]   (d psum)      gbv[h dh + j] += sum_b dctx[b, h dh + j] psum[b,h] */
int sc_rt_value_bias_bwd(const float* dctx, const float* bv, const float* psum, float* cbias, float* gbv, int32_t B, int32_t D, int32_t H,
                         void* stream);
/* end of the weighted-sum backward: d_soft[n] = sum_blk part[blk][n] ; out[n] = w[n] (d_soft[n] - sum_m w[m] d_soft[m])  (softmax backward) */
int sc_rt_softmax_bwd_reduce(const float* part, int32_t nblk, int32_t NL, const float* w_soft, float* out, void* stream);
/* elementwise over slices.  mode 0: out = sum_s y_s + bias[j] * rowscale[row][j / group] ; mode 1: u = sum_s y_s + bias, out = gelu_erf(u) *
 * dropout ; mode 2: out = (sum_s y_s) * dropout * gelu_erf'(u)   (dropout keep bits as sc_dropout_mult_f32 on the index row * D + j) */
int sc_rt_elem(const float* y, int64_t y_slice, int32_t ns, const float* bias, const float* rowscale, int32_t group, int32_t nscale, float* out,
               float* u, int32_t rows, int32_t D, int32_t mode, float drop_p, uint32_t drop_seed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused driver: ONE call enqueues a whole frozen HuBERT encoder layer (fairseq TransformerSentenceEncoderLayer as invoked at
 * avssl/module/speech_encoder_plus.py:49-53) on the caller's stream - QKV GEMM (V^T epilogue) -> attention -> out_proj (+bias,
 * dropout, +residual) -> LayerNorm -> FC1 (+bias, GELU) -> FC2 (+bias, dropout, +residual) -> LayerNorm; pre_ln = 1: the
 * HuBERT-large order (LayerNorms in front of the two halves).  x / out: [B*R, D] bf16 in the padded row layout, head_dim 64.
 * Scratch (caller-owned, six pointers): qk [B*R, 2D], vt [B, H, 64, R], ctx / pre / x1 [B*R, D], ffn [B*R, F], all bf16.  p_attn /
 * p_res = 0 in inference; seeds as in sc_gemm_args / sc_attn_fwd_bf16.
 * What lies behind qk and vt (sc_attn_fwd_bf16, "Reads"; the driver hands both to it unchanged, csrc/hubert_layer.cpp:70): SC_ATTN_SLACK
 *   rows of 2D elements behind qk must be readable (any bits); SC_ATTN_SLACK elements behind vt must be readable and FINITE when the
 *   attention launch runs, so they must not be part of ctx / pre / x1 / ffn / out (which this call writes, and which may hold
 *   anything before) - zero them once; no kernel writes them.
 *   sc_workspace_bytes(SC_WS_HUBERT_LAYER, rows = B*R, D, F) is the size of one allocation that carries both:
 *       qk [rows + SC_ATTN_SLACK, 2D] | vt [rows * D + SC_ATTN_SLACK] | ctx [rows, D] | pre [rows, D] | x1 [rows, D] | ffn [rows, F]
 *   = 2 (rows (6D + F) + SC_ATTN_SLACK (2D + 1)) bytes.  (Before this was written down the size was the six buffers back to back: the
 *   elements behind vt were then the first of ctx, uninitialised in a fresh allocation.)
 * Content on entry: apart from the finite elements behind vt, every scratch buffer and `out` may hold any bits (NaN included): each is
 *   written over all rows before it is read (QKV GEMM: qk, vt; attention: every row of ctx inside a pitch; GEMMs / LayerNorms: all rows).
 * Pad rows of x (t >= valid_len[b] inside a pitch) are scratch, not ignored: they pass through the LayerNorms and all four GEMMs, their
 *   k is masked and their V^T columns are multiplied by 0.  They must therefore be FINITE and of ordinary magnitude (zeros, or the
 *   previous layer's output on them): a NaN, an Inf or a value whose V projection overflows bf16 there breaks the valid rows of the
 *   utterance.  With that, out / ffn / qk on the rows t < valid_len[b] do not depend on the pad rows' values (bit for bit).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const sc_bf16* x; sc_bf16* out;
    const int32_t* valid_len;                 /* [B] keys per utterance */
    int32_t B, R, T, D, F, H, pre_ln;
    int32_t ffn_act;                          /* FC1 activation: 0 erf-GELU (HuBERT), 2 QuickGELU (CLIP ResidualAttentionBlock); 2 not with fused_ln */
    const sc_bf16 *qkv_w, *o_w, *fc1_w, *fc2_w;     /* [3D, D], [D, D], [F, D], [D, F] */
    const float *qkv_b, *o_b, *fc1_b, *fc2_b, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    float eps, p_attn, p_res;
    uint32_t seed_attn, seed_o, seed_fc2;
    sc_bf16 *qk, *vt, *ctx, *pre, *x1, *ffn;        /* scratch */
    /* ---- fused_ln = 1 (post-LN order only): no LayerNorm launch - the residual stream stays RAW and the two LayerNorms are folded
     * into their neighbour GEMMs (sc_gemm_args, "LayerNorm folded").  `out` then receives the rows in FRONT of the layer's final
     * LayerNorm and out_stats their row statistics; x may itself be such a raw output (x_stats != NULL, x_ns strips, x_ln_g / x_ln_b =
     * the affine of the LayerNorm that applies to it; qkv_w / qkv_b / qkv_colsum are then the folded forms for THAT LayerNorm).
     * fc1_w / fc1_b / fc1_colsum are always the forms folded with ln1; ln1_g / ln1_b are still read (the residual of fc2).
     * stats1: scratch for the statistics of `pre`.  x1 is not used. */
    int32_t fused_ln, x_ns;
    const float* x_stats;
    const float *x_ln_g, *x_ln_b;
    const float *qkv_colsum, *fc1_colsum;
    float *stats1, *out_stats;
    /* ---- ragged rows (round 4): seg != NULL (host pointer, seg->row0 device) - x / out / scratch hold seg->rows rows in the
     * segment layout (R, T are then ignored; vt = per utterance [H, 64, pitch]); attn_work / n_attn_work = work / nwork of sc_attn_fwd_bf16 */
    const sc_segments* seg;
    const int32_t* attn_work;
    int32_t n_attn_work;
    int32_t w_split;                          /* 1: qkv_w / o_w / fc1_w / fc2_w are the [N, 2K] hi / lo interleaves of sc_gemm_args.a_rep = 2 and the four
                                                 GEMMs run with it (evaluation: p_res must be 0); not with fused_ln.  The former reserved2. */
} sc_hubert_layer_args;
int sc_hubert_layer_fwd(const sc_hubert_layer_args* args, void* stream);
#define SC_WS_INFONCE 0       /* a = Bg */
#define SC_WS_HUBERT_LAYER 1  /* a = B*R rows, b = D, c = F: the six scratch buffers with SC_ATTN_SLACK behind qk and vt (layout above) */
int64_t sc_workspace_bytes(int32_t what, int64_t a, int64_t b, int64_t c);

/* ------------------------------------------------------------------------------------------------
 * Front of the frozen CLIP image tower (openai/CLIP VisionTransformer: conv1 patch embedding, class token, positional embedding,
 * ln_pre), forward only.  Image rows use the ragged row layout (sc_segments): image b owns `pitch` rows at row0[b], pitch = tokens
 * rounded up to SC_SEG_ROWS (tokens = 1 + g^2, g = S / P): row row0[b] is the class token, rows row0[b] + 1 .. + g^2 the patches in
 * row-major (gy, gx) order, the rest pad rows.  The blocks then run as sc_hubert_layer_fwd(pre_ln = 1, ffn_act = 2, seg).
 *   sc_vit_patchify_bf16: A [rows, Kp] bf16 <- the operand of the patch GEMM: patch row (b, gy, gx), column c P^2 + ky P + kx =
 *       bf16(img[b, c, gy P + ky, gx P + kx]) (the flattening of conv1.weight [W, 3, P, P]); columns 3 P^2 .. Kp - 1, class and pad
 *       rows are 0.  img: fp32 [B, 3, S, S], rows of S contiguous floats, strides (elements) sb / sc / sy; Kp = 3 P^2 rounded up to
 *       64.  Every element of A is written.
 *   sc_vit_embed_ln_bf16: X [rows, W] bf16 <- ln_pre(e) in fp32, e = cls + pos[0] on class rows, e = G[r] + pos[t] on patch row t
 *       (G: [rows, W] fp32, the patch GEMM's output), 0 on pad rows.  pos [tokens, W], cls / gamma / beta [W] fp32; W % 4 == 0.
 * ---------------------------------------------------------------------------------------------- */
int sc_vit_patchify_bf16(const float* img, int64_t sb, int64_t sc, int64_t sy, sc_bf16* A, int32_t Kp, const sc_segments* seg, int32_t S,
                         int32_t P, void* stream);
int sc_vit_embed_ln_bf16(const float* G, const float* cls, const float* pos, const float* gamma, const float* beta, sc_bf16* X,
                         const sc_segments* seg, int32_t tokens, int32_t W, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Raw-image input of the CLIP image tower: CLIP's preprocessing on the device - bicubic Resize(S) of a PIL image, CenterCrop(S),
 * ToTensor, Normalize (ClipModel.prep_image, avssl/module/clip_official.py:153-166; the data sets' clip_image_transform,
 * avssl/data/base_dataset.py:93-106), S = 224.  Pillow's 8-bit resampling restated exactly: per pass and output
 *     clip8((2^21 + sum_t pixel[first + t] * k[t]) >> 22)      int32 accumulation, arithmetic shift, clip to 0 .. 255
 * with 22-bit fixed-point coefficients, the horizontal pass first, a uint8 intermediate image, then the vertical pass.  The sources are
 * B images of unequal sizes in one byte buffer (image b: [h_b][w_b][3] uint8 at its offset); geometry, tap bounds and coefficients are
 * host-built (speechclip_plus_amd/image_prep.py).  Tables, in one int32 buffer `tab`:
 *   desc   [B][8] int64: source byte offset, source width (pixels), intermediate byte offset, intermediate rows, first source row of the
 *          intermediate, horizontal table, vertical table (offsets into tab, int32 units), ksize_h | ksize_v << 32
 *   table  bounds [S][2] int32 (first tap, tap count <= ksize) then coef [S][ksize] int32, for the S columns / rows of the crop window;
 *          vertical firsts are relative to the intermediate's first row.  A pass Pillow skips (equal sizes) is the one-tap table k = 2^22.
 * The kernels reach src and mid only through the tables and skip any access the tables would place outside src_bytes / mid_bytes.
 *   sc_image_resample_h_u8:   mid [rows_b][S][3] uint8 per image <- the horizontal pass over the S crop columns of the source rows the
 *       crop window's vertical pass reads.  max_rows = max_b rows_b (grid sizing).
 *   sc_image_resample_v_norm: the vertical pass over mid, then the look-up in lut [3][256] fp32 (channel, byte value).  Two optional
 *       outputs, NULL = not wanted, at least one: out fp32 [B][3][S][S], and A [seg.rows][Kp] bf16, the patch GEMM's operand in the
 *       layout and rounding of sc_vit_patchify_bf16 (pad columns, class and pad rows zero, every element written); A needs seg, P even
 *       dividing S, Kp as there, and every image's pitch >= 1 + (S / P)^2.
 * S even, <= 256.
 * ---------------------------------------------------------------------------------------------- */
int sc_image_resample_h_u8(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int32_t* tab, uint8_t* mid, int64_t mid_bytes,
                           int32_t B, int32_t max_rows, int32_t S, void* stream);
int sc_image_resample_v_norm(const uint8_t* mid, int64_t mid_bytes, const int64_t* desc, const int32_t* tab, const float* lut, float* out,
                             sc_bf16* A, int32_t Kp, const sc_segments* seg, int32_t P, int32_t B, int32_t S, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Raw-audio input of the speech encoder: PCM of any rate to 16 kHz mono fp32 on the device - the work of the reference's
 * librosa.load(path, sr=16_000) behind the decoder (avssl/data/base_dataset.py:81, example.py:21): to float, to mono, resample.  The
 * resampler is the project's own, in closed form.  g = gcd(sr, 16000), P = sr / g, Q = 16000 / g, c = 0.99 min(P, Q), W = 6,
 * x[j] = 0 outside 0 <= j < n_in, u = c (j - m P / Q) / P:
 *     y[m] = sum_j x[j] (c / P) sinc(u) cos^2(pi u / (2 W))   over |u| < W,      n_out = ceil(n_in Q / P)
 * a Hann-windowed sinc, six zero crossings, roll-off 0.99 (the default filter of torchaudio's resample; NOT the reference's soxr_hq -
 * no bit parity with it is claimed).  int16 samples are x / 32768; channels are averaged in fp32, (x0 + x1 + ...) / ch in channel order.
 * Additive in round 25; sc_abi_version() stays 7.
 *   sc_audio_resample: one launch for n_utt utterances of ONE source rate.  src: the packed PCM (interleaved frames), int16 if is_i16
 *       else fp32; desc [n_utt][5] int64: byte offset into src, n_in (frames), ch (1 .. 8), n_out, output row.  table [Q][taps] fp32 and
 *       first [Q] int32 (speechclip_plus_amd/audio_prep.py: resample_table): output m = q Q + i reads x[q P + first[i] + t] with
 *       coefficient table[i][t], t ascending, one fmaf each; P = Q = 1 (16 kHz) converts and down-mixes only, table / first unused.
 *       out [out_rows][ld_out] fp32: row desc.row gets its n_out samples and zeros up to Lout - every element of the rows named is
 *       written.  tile: outputs per workgroup, a multiple of 256 (audio_prep.tile_outputs).  q P is formed in 64 bits.  A sample outside
 *       [0, n_in) of its utterance is never loaded; an utterance that does not fit src_bytes reads nothing and yields zeros.
 * ---------------------------------------------------------------------------------------------- */
int sc_audio_resample(const void* src, int64_t src_bytes, int32_t is_i16, const int64_t* desc, int32_t n_utt, const float* table,
                      const int32_t* first, int32_t P, int32_t Q, int32_t taps, int32_t tile, float* out, int64_t ld_out,
                      int32_t out_rows, int32_t Lout, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimiser step on a flat fp32 parameter buffer: torch.optim.Adam semantics (L2 weight decay added to
 * the gradient), gradient clipping by global norm folded in (avssl/model/kwClip.py:646-674 +
 * trainer.gradient_clip_val).  sumsq: partial sums of squares for the global norm.
 * ---------------------------------------------------------------------------------------------- */
int sc_sumsq_f32(const float* x, int64_t n, float* partial, int32_t nblk, void* stream);
int sc_adam_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2,
                float eps, float weight_decay, int32_t step, const float* gnorm_sq_partial, int32_t nblk,
                float max_norm, void* stream);      /* betas as doubles (ABI 5): 1 - beta and 1 - beta^step are formed in double, rounded once */

/* ------------------------------------------------------------------------------------------------
 * Keyword prompt of the cascaded branches in the text tower's packed rows (round 4; replaces the ~35 element-wise torch launches of
 * ClipModel.encode_keywords, avssl/module/clip_official.py:222-279, and of the padding around the tower).
 *   sc_prompt_assemble: X [Bp*SEG, W] bf16 <- per sample b < B the prefix t < n_pos of
 *       [SOT, kw_1 .. kw_n, EOT, token 0 ...] + positional_embedding  (n = count[b]; keyword t-1 read from keywords[b*ldb + (t-1)*W],
 *       zero past the N keywords given), every other row (t >= n_pos, pad samples b >= B) zero.  tok [3, W] = the embeddings of SOT,
 *       EOT and token 0; pos [>= n_pos, W].  eot_row[b] <- b*SEG + min(count[b] + 1, n_pos - 1): the row the head reads; counts that
 *       pointed behind the prefix are clamped and added to *clamped (device counter, may be NULL).
 *   sc_prompt_assemble_bwd: dkeywords[b, j] <- float(dX[b*SEG + j + 1]) for j + 1 < min(count[b] + 1, n_pos), else 0 (every element
 *       of the [B, N, W] gradient is written).
 *   sc_rows_gather_bf16: out[b] <- float(X[row[b]]);   sc_rows_scatter_bf16: dX [M, W] <- 0 except dX[row[b]] = bf16(d[b]) (the row of
 *       sample b lies in its own segment b*SEG .. b*SEG + SEG - 1; every row of dX is written).
 * ---------------------------------------------------------------------------------------------- */
int sc_prompt_assemble(const float* keywords, int64_t ldb, const int64_t* count, const float* tok, const float* pos, sc_bf16* X,
                       int32_t* eot_row, int64_t* clamped, int32_t B, int32_t Bp, int32_t N, int32_t W, int32_t SEG, int32_t n_pos,
                       void* stream);
/* Caption tokens in the same packed rows (ClipModel.encode_text, avssl/module/clip_official.py:213-220 -> openai/CLIP encode_text), one
 * launch: ids [B, L <= 77] int64 (row stride ld_ids), table [V, W] fp32 (leading dimension ldt), pos [77, W] fp32.
 *   X[b*SEG + t] <- bf16(table[ids[b, t]] + pos[t]) for b < B, t < n_pos (fp32 add, rounded once); every other row of X [Bp*SEG, W] zero,
 *   every row written.  eot_row[b] <- b*SEG + e_b, e_b = the FIRST position of the row's largest id among t < L (text.argmax(dim=-1): the
 *   end-of-text position in the full and in a reduced vocabulary), clamped to n_pos - 1.  An id outside [0, V) reads nothing and
 *   contributes a zero embedding.  *bad (device counter, may be NULL) += clamps + such ids among the rows assembled.
 *   W % 8 == 0, ldt % 4 == 0, n_pos <= min(L, SEG); table, pos and X 16-byte aligned. */
int sc_text_assemble(const int64_t* ids, int64_t ld_ids, const float* table, int64_t ldt, const float* pos, sc_bf16* X, int32_t* eot_row,
                     int64_t* bad, int32_t B, int32_t Bp, int32_t L, int32_t V, int32_t W, int32_t SEG, int32_t n_pos, void* stream);
int sc_prompt_assemble_bwd(const sc_bf16* dX, const int64_t* count, float* dkeywords, int64_t ldb, int32_t B, int32_t N, int32_t W,
                           int32_t SEG, int32_t n_pos, void* stream);
int sc_rows_gather_bf16(const sc_bf16* X, const int32_t* row, float* out, int32_t B, int32_t W, void* stream);
int sc_rows_scatter_bf16(const float* d, const int32_t* row, sc_bf16* dX, int32_t M, int32_t B, int32_t W, int32_t SEG, void* stream);
/* mask[b, k] = (k >= lens[b] + add), k < n, as bytes (1 = padding): get_keypadding_mask (avssl/util/data_utils.py:6-22) and the attention
 * block's padded-pitch key mask from the lengths in one launch. */
int sc_len_mask_u8(const int64_t* lens, int32_t add, uint8_t* mask, int32_t B, int32_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Supervised contrastive loss (Khosla et al.; csrc/supcon.hip).  Additive in round 27; sc_abi_version() stays 7.
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
 * ---------------------------------------------------------------------------------------------- */
#define SC_SUPCON_MAX_LOGIT_BYTES 1073741824   /* 1 GiB of logits [Na, N] fp32 */
int64_t sc_supcon_workspace_floats(int32_t Na, int32_t N);   /* 0: nothing to launch; -1: refused (see sc_last_error) */
int sc_supcon_fwd(const float* C, int32_t N, int32_t Na, int32_t bsz, int32_t E, const int64_t* labels, const float* mask,
                  const float* inv_temp, float base_temperature, float* logits, float* lse, float* possum, float* poscnt, float* loss,
                  float* workspace, void* stream);
int sc_supcon_grad(const float* logits, const float* lse, const float* poscnt, int32_t N, int32_t Na, int32_t bsz, const int64_t* labels,
                   const float* mask, const float* gscale, const float* inv_temp, float base_temperature, float* G, float* dlogit_dot,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training modes of SimpleVectorQuantizer: soft, Gumbel, learnable temperature (csrc/vq.hip, behind sc_vq_rowstats / sc_vq_soft_bwd).
 * Additive in round 28; sc_abi_version() stays 7.
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
 *                          sc_vq_soft_bwd is this formula with noise 0, no dtemp_row, on the fused LSE.
 *   Fixed-order reductions, no float atomics: two calls on the same inputs give the same bits.
 * ---------------------------------------------------------------------------------------------- */
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
