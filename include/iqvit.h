/* iqvit.h -- C ABI of the MI355X-native (gfx950) training path for the ViT / raw-IQ
 * modulation classifiers of aliftffd/ViT-vs-Raw-IQ.
 *
 * The reference has no FFI layer: its boundary is the Python nn.Module surface
 * (SURVEY.md section 8b).  This header is the boundary the MI355X build puts underneath
 * that surface: plain pointers and sizes, no torch types.  Every pointer is DEVICE memory
 * (HBM) unless marked host.  All activations are bf16 (uint16 storage), row-major,
 * tokens-major [B*S, D]; parameters, gradients, statistics, logits and losses are fp32.
 * Every launch goes to the hipStream_t passed as `stream` (iq_stream_t == hipStream_t);
 * no call synchronises, allocates or frees, so a call sequence can be captured in a hipGraph.
 * Return value: 0 ok; IQ_ERR_* otherwise (host mirrors map them to Python exceptions).
 *
 * Citations are to /root/reference/Transformer_Thesis/ (V/ = ViT/, R/ = transformer_rawIQ/).
 */
#ifndef IQVIT_H
#define IQVIT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* iq_stream_t; /* hipStream_t */

enum { IQ_STATUS_OK = 0, IQ_STATUS_ARG = 1, IQ_STATUS_UNSUPPORTED = 2, IQ_STATUS_LAUNCH = 3 };

/* Dropout site: Philox4x32-7 (7 rounds: csrc/common.h) keyed by seed, counter (element_index/8, site, step).
 * p == 0 disables.  Masks are regenerated in backward from the same triple, never stored. */
typedef struct iq_dropout {
  uint64_t seed;
  uint32_t step;
  uint32_t site;
  float p;
  const uint32_t* step_dev; /* optional DEVICE u32 overriding `step` (bumped on device under hipGraph replay) */
} iq_dropout_t;
/* Dropout sites of the model plan are 0 (embedding) and 1 + 3*l, 2 + 3*l, 3 + 3*l of encoder layer l (csrc/model.hip); a
 * caller of a single kernel may pass any other small id.  The top value of the word is RESERVED: it is the `site` counter word
 * of the channel impairments below, so no dropout site may use it (a dropout stream with the same seed and step would repeat
 * the impairment's bits). */
#define IQ_SITE_IMPAIR 0xFFFFFFFFu
/* The value below it is RESERVED too: the `site` counter word of the synthetic frame source (iq_frames_synth). */
#define IQ_SITE_SYNTH 0xFFFFFFFEu
/* And the next: the `site` counter word of the fading channel (iq_frames_fade). */
#define IQ_SITE_FADE 0xFFFFFFFDu

/* ---------------------------------------------------------------------------------------
 * LayerNorm.  Replaces LayerNorm.forward, V/models/layers/layers_norm.py:11-19 (eps 1e-12,
 * biased variance) and its autograd backward; also nn.LayerNorm (eps 1e-5) of the rawIQ head.
 * z,x,dx,dz,dy: bf16 [M,D]; gamma,beta,dgamma,dbeta: fp32 [D]; mean,rstd: fp32 [M].
 * iq_ln_bwd optionally emits dy = dropout(dz) for the site that preceded the residual add
 * (V/models/blocks/encoder_layer.py:24-25,32-33).  ws: iq_ln_bwd_ws_bytes(D) scratch. */
int iq_ln_supported(int D);
int iq_ln_fwd(const void* z, const float* gamma, const float* beta, void* x, float* mean, float* rstd, int M, int D,
              float eps, iq_stream_t stream);
size_t iq_ln_bwd_ws_bytes(int D);
int iq_ln_bwd(const void* dx, const void* z, const float* mean, const float* rstd, const float* gamma, void* dz,
              void* dy, const iq_dropout_t* drop, float* dgamma, float* dbeta, float* ws, int accumulate, int M,
              int D, iq_stream_t stream);
/* iq_ln_bwd with dgamma == dbeta == NULL leaves the per-block partial sums in ws as
 * [iq_ln_bwd_partial_rows(M, D)][2*D] fp32 (dgamma partials | dbeta partials per row) for a later fused, fixed-order
 * reduction: pass them as iq_reduce_seg_t entries to iq_gemm_bf16_wgrad_grouped. */
int iq_ln_bwd_partial_rows(int M, int D);

/* ---------------------------------------------------------------------------------------
 * bf16 MFMA GEMM, C[M,N] = epilogue(A[M,K] * B[N,K]^T), fp32 accumulate.
 * Replaces every nn.Linear on the path: w_q/w_k/w_v/w_concat
 * (V/models/layers/multi_head_attention.py:18,28), linear1/linear2
 * (V/models/layers/position_wise_feed_forward.py:13-16), the non-overlapping Conv2d/Conv1d
 * of the embeddings (V/models/embedding/patch_embedding.py:9-15,
 * R/models/embedding/patch_embedding.py:29-43) and, with B = W^T shadows, their dgrads.
 * Epilogue order: +bias, relu, +pe (row remap), dropout, *gate, +residual.
 *   tok>0 : embedding mode, output row = (m/tok)*seq + m%tok + cls_off and pe[(m%tok+cls_off),:]
 *           is added (V/models/encoder.py:42-47).
 *   gate  : v *= (gate[m,n] > 0) ? gate_scale : 0   (ReLU+dropout backward from the saved hidden).
 * K%8==0, N%8==0, lda/ldb/ldc/ldr/ldg in elements and %8==0 (else IQ_STATUS_UNSUPPORTED).  A, B, C, bias, pe, gate and
 * residual 16-byte aligned (else IQ_STATUS_ARG): every kernel moves 16-byte vectors.
 * The kernel is chosen from the shape; results do not depend on the choice beyond fp32 summation order:
 *   N%256==0, K%64==0, K>=256 and >= 512 tiles of 256x256 (ViT-Base at its batch): persistent 256x256 tiles
 *   (gemm_big.hip, 0.85-1.19 PFLOP/s); otherwise 128x{128,64} tiles (gemm_nt.hip); K%32!=0: register-staged fallback. */
typedef struct iq_epilogue {
  const float* bias;    /* [N] or NULL */
  int relu;
  const float* pe;      /* [seq, N] fp32 or NULL (embedding mode) */
  int tok, seq, cls_off;
  iq_dropout_t drop;    /* indexed by OUTPUT element (row_out*N + n) */
  const void* gate;     /* bf16 [M, ldg] or NULL */
  int ldg;
  float gate_scale;
  const void* residual; /* bf16 [M_out, ldr] or NULL */
  int ldr;
} iq_epilogue_t;
int iq_gemm_bf16_nt(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                    const iq_epilogue_t* epi, iq_stream_t stream);

/* GEMM + the post-norm tail of an encoder sub-layer in ONE launch (whole-row tiles, D in {128,192,256}, K % 32 == 0, K >= 64):
 *   Z = dropout(A[M,K] * W[D,K]^T + bias) + residual        bf16 [M,D]   (kept for backward)
 *   X = gamma * (Z - mean) * rstd + beta                     bf16 [M,D];  mean, rstd fp32 [M] (kept for backward)
 * Replaces `x = norm1(dropout1(attention(x)) + x)` / `x = norm2(dropout2(ffn(x)) + x)`,
 * V/models/blocks/encoder_layer.py:24-25,32-33 with LayerNorm.forward (V/models/layers/layers_norm.py:11-19), i.e. an
 * iq_gemm_bf16_nt (bias, dropout, residual) followed by iq_ln_fwd: same Z bit for bit, same statistics to fp32
 * summation order (taken from the bf16-rounded Z, two-pass).  All pointers 16-byte aligned. */
int iq_gemm_ln_supported(int D, int K);
int iq_gemm_bf16_ln(const void* A, int lda, const void* W, int ldw, const float* bias, const void* residual, int ldr,
                    const iq_dropout_t* drop, const float* gamma, const float* beta, float eps, void* Z, void* X,
                    float* mean, float* rstd, int M, int D, int K, iq_stream_t stream);

/* Data-gradient GEMM + the LayerNorm BACKWARD that consumes its result, in ONE launch (whole-row tiles, D in {128,192},
 * K % 32 == 0, K >= 64):   dX = A[M,K] * Wt[D,K]^T + residual   (fp32, not stored), then exactly iq_ln_bwd on it:
 *   dz = rstd * (g - mean_D(g) - xhat * mean_D(g * xhat)),  g = dX * gamma,  xhat = (z - mean) * rstd      bf16 [M,D]
 *   dy = dropout_mask(dz) * scale (only when drop->p > 0)                                                   bf16 [M,D]
 *   partial: iq_gemm_lnbwd_partial_rows(M) rows of [2*D] fp32 (dgamma | dbeta partial sums), to be reduced like
 *   iq_ln_bwd's (iq_reduce_seg_t).
 * The autograd backward of `x = norm(dropout(f(x)) + x)`, V/models/blocks/encoder_layer.py:24-25,32-33, behind the FFN1 /
 * QKV data-gradient GEMM that feeds it.  All pointers 16-byte aligned. */
int iq_gemm_lnbwd_supported(int D, int K);
int iq_gemm_lnbwd_partial_rows(int M);
int iq_gemm_bf16_lnbwd(const void* A, int lda, const void* Wt, int ldw, const void* residual, int ldr, const void* z,
                       const float* mean, const float* rstd, const float* gamma, const iq_dropout_t* drop, void* dz,
                       void* dy, float* partial, int M, int D, int K, iq_stream_t stream);

/* The feed-forward sub-layer + norm2 in one launch (rows are owned by waves, 32 at a time; M = frames * S rows, D in {128, 192},
 * F % 64 == 0, the LDS weight ring + F floats within 160 KB: iq_ffn_chain_supported):
 *   H = dropout1(relu(X1 * W1^T + b1))            bf16 [M, F]  (written once; the weight gradients read it)
 *   Z = dropout2(H * W2^T + b2) + X1              bf16 [M, D]  (kept for backward)
 *   X = gamma * (Z - mean) * rstd + beta          bf16 [M, D];  mean, rstd fp32 [M]
 * = PositionwiseFeedForward.forward (V/models/layers/position_wise_feed_forward.py:12-17) + `x = norm2(dropout2(ffn(x)) + x)`
 * (V/models/blocks/encoder_layer.py:30-33).  The hidden tile goes from the first product's epilogue into the second product in
 * registers, never re-read from HBM.  H and Z equal iq_gemm_bf16_nt (bias, relu, drop1) followed by iq_gemm_bf16_ln up to fp32
 * summation order inside one MFMA (bf16 rounding ties only); dropout indices as there (output element row*N + n).
 * W1 [F, D], W2 [D, F] bf16 row-major; all pointers 16-byte aligned.
 * iq_attn_out_ffn_chain_fwd: the same launch with the attention output projection + dropout + residual + norm1 in front
 * (`x = norm1(dropout1(attention_out) + x)`, encoder_layer.py:24-28 -- the whole layer after the attention core):
 *   Z1 = dropout0(A * Wo^T + bo) + R              bf16 [M, D]  (kept for backward)
 *   X1 = gamma1 * (Z1 - mean1) * rstd1 + beta1    bf16 [M, D] (written for backward; consumed from registers);  mean1, rstd1 [M]
 * then as above on X1.  A [M, D] attention output, Wo [D, D], R [M, D] the layer input.  Z1 equals iq_gemm_bf16_ln's up to bf16
 * rounding ties (summation order inside one MFMA); the rest equals iq_ffn_chain_fwd on the X1 written, bit for bit.
 * Wq / bq / Yq (all three or none): Yq[M, 3D] = X * Wq[3D, D]^T + bq behind norm2 -- the NEXT layer's packed q,k,v projection
 * (multi_head_attention.py:17-19) of this layer's output, from registers. */
/* iq_ffn_chain_bwd: the data path of the same sub-layer's backward in one launch (replaces the gate data-gradient GEMM and
 * iq_gemm_bf16_lnbwd; autograd of position_wise_feed_forward.py:12-17 and of the norm1 feeding it, encoder_layer.py:24-25):
 *   gH = (H > 0) ? (dO * W2t^T) * gate_scale : 0         bf16 [M,F]   (written once: the W1 / W2 weight gradients read it)
 *        "H > 0" (ReLU and dropout1 of the forward pass at once) comes as ONE BIT per hidden unit in `gate_bits`,
 *        iq_ffn_chain_gate_bytes(M, F) bytes written by iq_ffn_chain_fwd (its `gate_bits` argument, NULL = not wanted) in the
 *        backward kernel's own wave / chunk / lane order (an opaque buffer between the two calls)
 *   dX1 = gH * W1t^T + residual (rounded to bf16), then exactly iq_ln_bwd on it with z1 / mean / rstd / gamma:
 *   dz bf16 [M,D], dy = dropout_mask(dz) * scale (only when drop->p > 0), partial: iq_ffn_chain_bwd_partial_rows(M) rows of
 *   [2*D] fp32 (dgamma | dbeta partial sums, one row per workgroup) for the fused fixed-order reduction (iq_reduce_seg_t).
 * W2t [F, D] and W1t [D, F] are the TRANSPOSED weights (bf16 row-major), M = frames * S.
 * Wot / dA (both or neither): dA[M, D] = dy * Wot[D, D]^T behind it (dz where there is no dropout) -- the data gradient of the
 * attention output projection (Wot = Wo transposed; autograd of multi_head_attention.py:28), i.e. what iq_attn_bwd starts
 * from, in the same launch: equals iq_gemm_bf16_nt(dy, Wot) up to bf16 rounding ties.
 * iq_qkv_dgrad_ffn_chain_bwd: the same launch (Wot / dA required) with the launch that would produce its dO in front -- exactly
 * iq_gemm_bf16_lnbwd(gQKV [M,3D], Wqkv_t [D,3D], residual0, z2, mean2, rstd2, gamma2, drop2) -> dz2, dy2, partial2
 * (iq_ffn_chain_bwd_partial_rows(M) rows): the data gradient of the packed q,k,v projection of the layer ABOVE
 * (multi_head_attention.py:17-19) + the residual path, and this layer's norm2 backward (encoder_layer.py:30-33).  dy2 (dz2 where
 * there is no dropout; same probability at both sites) is the second stage's dO, taken from the CU's LDS instead of HBM;
 * `residual` is normally dz2 itself.  Results equal the two launches up to bf16 rounding ties. */
int iq_ffn_chain_supported(int S, int D, int F);
int iq_ffn_chain_bwd_partial_rows(int M);
size_t iq_ffn_chain_gate_bytes(int M, int F);
int iq_ffn_chain_bwd(const void* dO, const void* W2t, const void* gate_bits, float gate_scale, void* gH, const void* W1t,
                     const void* residual, const void* z1, const float* mean, const float* rstd, const float* gamma,
                     const iq_dropout_t* drop, void* dz, void* dy, float* partial, const void* Wot, void* dA, int frames, int S,
                     int D, int F, iq_stream_t stream);
int iq_qkv_dgrad_ffn_chain_bwd(const void* gQKV, const void* Wqkv_t, const void* residual0, const void* z2, const float* mean2,
                               const float* rstd2, const float* gamma2, const iq_dropout_t* drop2, void* dz2, void* dy2, float* partial2,
                               const void* W2t, const void* gate_bits, float gate_scale, void* gH, const void* W1t, const void* residual,
                               const void* z1, const float* mean, const float* rstd, const float* gamma, const iq_dropout_t* drop, void* dz,
                               void* dy, float* partial, const void* Wot, void* dA, int frames, int S, int D, int F, iq_stream_t stream);
int iq_ffn_chain_fwd(const void* X1, const void* W1, const float* b1, const iq_dropout_t* drop1, void* H, const void* W2,
                     const float* b2, const iq_dropout_t* drop2, const float* gamma, const float* beta, float eps, void* Z,
                     void* X, float* mean, float* rstd, void* gate_bits, int frames, int S, int D, int F, iq_stream_t stream);
int iq_attn_out_ffn_chain_fwd(const void* A, const void* Wo, const float* bo, const iq_dropout_t* drop0, const void* R,
                              const float* gamma1, const float* beta1, void* Z1, void* X1, float* mean1, float* rstd1,
                              const void* W1, const float* b1, const iq_dropout_t* drop1, void* H, const void* W2, const float* b2,
                              const iq_dropout_t* drop2, const float* gamma2, const float* beta2, float eps, void* Z2, void* X,
                              float* mean2, float* rstd2, void* gate_bits, const void* Wq, const float* bq, void* Yq, int frames,
                              int S, int D, int F, iq_stream_t stream);

/* Weight gradient: dW[N,K] (+)= dY[M,N]^T * X[M,K]; dbias[N] (+)= colsum(dY) (NULL to skip).
 * Split over M into slabs in `ws` (iq_wgrad_ws_bytes), reduced deterministically (no atomics). */
size_t iq_wgrad_ws_bytes(int M, int N, int K);
int iq_gemm_bf16_wgrad(const void* dY, int ldy, const void* X, int ldx, float* dW, float* dbias, int M, int N, int K,
                       float* ws, size_t ws_bytes, int accumulate, iq_stream_t stream);

/* Several weight gradients that share M (the four Linear layers of one encoder layer: what torch.autograd runs as
 * separate addmm nodes behind V/models/blocks/encoder_layer.py:16-36) in ONE launch + ONE slab reduce.  At most 4
 * problems are fused; larger groups / large N*K run one at a time through the same workspace.
 * Fast path (gemm_wgrad_big.hip: LDS-shared 256-row tiles, a problem whose N is the model width computed transposed):
 * M%64==0, M>=4096, dY / X 128-byte aligned with ldy%64==0 and ldx%64==0, and one column tile of 128, 192 or 256
 * dividing the shorter side of every problem; anything else runs the wave-private / shared-tile kernels of
 * gemm_wgrad.hip.  Either way the slabs are summed in a fixed order: results are bit-reproducible run to run. */
typedef struct iq_wgrad_problem {
  const void* dY; /* bf16 [M, ldy] */
  int ldy;
  const void* X;  /* bf16 [M, ldx] */
  int ldx;
  float* dW;      /* fp32 [N, K], 16-byte aligned */
  float* dbias;   /* fp32 [N] or NULL */
  int N, K;
} iq_wgrad_problem_t;
/* Extra fixed-order column reductions that ride on the group's slab-reduce launch (the LayerNorm gamma/beta partials
 * of the same encoder layer): out[0..n) (+)= sum over `rows` rows of partials[row * row_stride + 0..n). */
typedef struct iq_reduce_seg {
  const float* partials;
  int rows;
  int64_t row_stride; /* floats */
  float* out;
  int64_t n;
} iq_reduce_seg_t;
/* max_workgroups: 0 = fill the GPU once (768 workgroups); a smaller budget leaves CU slots free for kernels of
 * another stream (the model's backward can overlap a layer's weight gradients with the next layer's dX chain).
 * extra / nextra: up to 4 iq_reduce_seg_t (or NULL / 0). */
size_t iq_wgrad_grouped_ws_bytes(const iq_wgrad_problem_t* probs, int nprob, int M, int max_workgroups);
int iq_gemm_bf16_wgrad_grouped(const iq_wgrad_problem_t* probs, int nprob, int M, float* ws, size_t ws_bytes,
                               int accumulate, int max_workgroups, const iq_reduce_seg_t* extra, int nextra,
                               iq_stream_t stream);

/* The slab reduce of a group as a job that can run later on the same stream: the segments (weights, biases, extra), in
 * the block order of the stand-alone launch.  Filled by iq_gemm_bf16_wgrad_grouped_deferred; callers treat it as opaque.
 * seg[i] owns virtual blocks [blk0, next blk0): 256 threads each, "wide" = 64 float4 columns x 4 row slices, "tall" = 16
 * columns x 16 slices (csrc/wgrad_reduce.h). */
#define IQ_REDUCE_JOB_SEGS 12
typedef struct iq_reduce_job_seg {
  const float* partials; /* [rows][stride] */
  float* out;            /* [n] */
  int64_t n;
  int64_t stride;        /* floats */
  int rows;
  int blk0;
  int tall;
} iq_reduce_job_seg_t;
typedef struct iq_reduce_job {
  iq_reduce_job_seg_t seg[IQ_REDUCE_JOB_SEGS];
  int nseg;
  int nblk;       /* virtual blocks in all; 0 = nothing to do */
  int accumulate;
} iq_reduce_job_t;
/* iq_gemm_bf16_wgrad_grouped without its last launch: the partial-tile kernel runs, the slab reduce (+ the extra
 * segments) comes back in *job.  The job reads `ws`, the extra segments' partials and (accumulate) the outputs, so it must
 * run on the same stream before anything overwrites them: stand-alone with iq_reduce_job_run, or inside a later launch
 * that has room for it (iq_gemm_bf16_lnbwd_ride).  A group that runs one problem at a time through the shared slab area
 * reduces those problems at once, as iq_gemm_bf16_wgrad_grouped does, and only the extra segments are left in the job.
 * iq_gemm_bf16_wgrad_grouped == deferred + run: the same kernels, the same bits. */
int iq_gemm_bf16_wgrad_grouped_deferred(const iq_wgrad_problem_t* probs, int nprob, int M, float* ws, size_t ws_bytes,
                                        int accumulate, int max_workgroups, const iq_reduce_seg_t* extra, int nextra,
                                        iq_reduce_job_t* job, iq_stream_t stream);
int iq_reduce_job_run(const iq_reduce_job_t* job, iq_stream_t stream);
/* iq_gemm_bf16_lnbwd with a reduce job riding in the launch: where the row tiles leave workgroup slots of the GPU free
 * (resident workgroups per CU x CUs - tiles, at least 64), that many extra workgroups behind the tiles sum the job's
 * virtual blocks, with the arithmetic of the stand-alone launch bit for bit, and no launch is spent on the reduce.
 * Otherwise the job runs stand-alone first, then the plain launch.  Nothing the tiles write may be read by the job and
 * vice versa (the model alternates the norm2 partial rows between two buffers for this).  job NULL or empty = iq_gemm_bf16_lnbwd.
 * iq_gemm_lnbwd_ride_workgroups: the reduce workgroups such a call appends for a job of `job_blocks` virtual blocks on the
 * current device (asks the runtime for the kernel's occupancy); 0 = the call falls back to the stand-alone reduce. */
int iq_gemm_lnbwd_ride_workgroups(int M, int D, int K, int job_blocks);
int iq_gemm_bf16_lnbwd_ride(const void* A, int lda, const void* Wt, int ldw, const void* residual, int ldr, const void* z,
                            const float* mean, const float* rstd, const float* gamma, const iq_dropout_t* drop, void* dz,
                            void* dy, float* partial, int M, int D, int K, const iq_reduce_job_t* job, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Scaled-dot-product attention core, softmax(Q K^T / sqrt(dh)) V per (frame, head), no mask,
 * no dropout.  Replaces ScaleDotProductAttention.forward
 * (V/models/layers/scale_dot_product_attention.py:23-39) plus MultiHeadAttention.split/concat
 * (V/models/layers/multi_head_attention.py:34-47): reads the packed projection output
 * qkv[B*S, 3*D] (q | k | v, head h at columns h*dh) and writes out[B*S, D] already "concatenated".
 * The S x S scores never reach HBM; lse[B,H,S] (fp32, natural log) is kept for backward.
 * dh in {16,32,64}; S <= 4096 (backward keeps the staged side in LDS in chunks when one image does not fit:
 * embedding_type='conv1d', S = 1025, R/models/encoder.py:34-41). */
int iq_attn_supported(int S, int dh);
int iq_attn_fwd(const void* qkv, void* out, float* lse, int B, int S, int H, int dh, iq_stream_t stream);
int iq_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int B, int S, int H,
                int dh, iq_stream_t stream);
/* The optional mask branch, V/models/layers/scale_dot_product_attention.py:30-31 (`score.masked_fill(mask == 0, -10000)`
 * after the 1/sqrt(dh) scaling; no reference caller passes a mask).  mask: uint8 (B, 1 | H, S, S), 0 = masked;
 * mask_hstride = S*S when the mask has a head dimension, 0 when it is shared by all heads.  mask NULL = the calls above.
 * Backward passes no gradient through masked positions (masked_fill). */
int iq_attn_fwd_masked(const void* qkv, void* out, float* lse, const uint8_t* mask, long mask_hstride, int B, int S,
                       int H, int dh, iq_stream_t stream);
int iq_attn_bwd_masked(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                       const uint8_t* mask, long mask_hstride, int B, int S, int H, int dh, iq_stream_t stream);
/* The attention matrix the reference forms and drops (V/models/layers/scale_dot_product_attention.py:25-39 returns `score`,
 * V/models/layers/multi_head_attention.py:24 discards it, :30 "5. visualize attention map").
 * P = softmax(q k^T / sqrt(dh)) of the packed qkv [B*S, 3*H*dh] bf16 (layout of iq_attn_fwd), recomputed with the
 * log-sum-exp iq_attn_fwd wrote (fp32 [B, H, S], natural log).  No S x S buffer exists in the forward.
 *   rows  0: every query row      -> out[b*out_bstride + ((h*S + q)*S + key)]
 *         1: query row 0 (CLS)    -> out[b*out_bstride + h*S + key]
 *         2: mean over query rows -> out[b*out_bstride + h*S + key]
 *   heads 0: per head (h < H), 1: mean over heads (h = 0 only)                       fp32 out, no atomics
 * Same (S, dh) set as iq_attn_supported.  Two calls give the same bits. */
int iq_attn_probs(const void* qkv, const float* lse, float* out, long out_bstride, int B, int S, int H, int dh,
                  int rows, int heads, iq_stream_t stream);
/* Gradient-weighted attention (Chefer, Gur & Wolf, "Transformer Interpretability Beyond Attention Visualization", ICCV 2021,
 * arXiv 2103.15679, eqs. 5-6), for the same matrix: the reference's `score` (V/models/layers/scale_dot_product_attention.py:
 * 25-39) times the gradient of a scalar y with respect to it.  dout bf16 [B*S, H*dh] is dy/d(concatenated attention-core
 * output) (head h at columns h*dh, the layout of iq_attn_fwd's out), so dy/dP[q, key] = dout_h[q] . v_h[key].
 * iq_attn_grad_probs writes G = P * dP (positive 1: max(G, 0) per head, before the head mean; 0: signed) with the rows /
 * heads / out layout of iq_attn_probs.  iq_attn_relevance_step writes, fp32 [B, S],
 *   r_out[b,k] = r_in[b,k] + (1/H) sum_h sum_q r_in[b,q] max(P_h[q,k] dP_h[q,k], 0)
 * i.e. one row step r <- r (I + mean_h max(G_h, 0)) of the relevance rollout; r_in and r_out must not overlap.
 * Same (S, dh) set as iq_attn_supported; no atomics, two calls give the same bits. */
int iq_attn_grad_probs(const void* qkv, const float* lse, const void* dout, float* out, long out_bstride, int B, int S,
                       int H, int dh, int rows, int heads, int positive, iq_stream_t stream);
int iq_attn_relevance_step(const void* qkv, const float* lse, const void* dout, const float* r_in, float* r_out, int B,
                           int S, int H, int dh, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Embedding front end.  iq_patchify turns the fp32 input frame batch into the bf16 GEMM
 * operand [B*tok, Kpad] (patch element order = the conv weight's (c, py, px) / (c, j) order,
 * zero padded to Kpad); kind 0: src (B,C,H,W), patch p  (V/models/embedding/patch_embedding.py:11-15)
 *               kind 1: src (B,C,L),   kernel = stride = k (R/models/embedding/patch_embedding.py:47-60).
 * iq_cls_rows writes row 0 of every frame: dropout(cls + pe[0]) (V/models/encoder.py:42-47).
 * iq_embed_bwd_gather compacts d(x0) rows (dropping cls rows, re-applying the dropout mask)
 * into [B*tok, D] for the embedding wgrad and reduces d(cls) = sum_b d(x0)[b,0,:]. */
/* Input pipeline on the device: raw[n_frames, len, 2] fp32 I/Q frames -> per-channel z-score
 * (stats = {i_mean, i_std, q_mean, q_std}) -> out[n_frames, 2, take]: the first `take` I samples then the first `take`
 * Q samples of every frame.  take = len is both reference layouts: viewed as (1, 32, 64) it is the ViT "image" of
 * V/dataloader/dataset.py:210-224, as (2, len) the transpose of R/dataloader/dataset.py:214-222.  Bit-identical to the
 * CPU preprocessing (IEEE subtract and divide). */
int iq_frames_preprocess(const float* raw, float* out, int n_frames, int len, int take, const float* stats,
                         iq_stream_t stream);
/* Channel impairments in front of that pipeline, one launch (csrc/impair.hip): training augmentation (rotation, flip and noise
 * of I/Q frames: Huang et al. 2019, "Data augmentation for deep learning-based radio modulation classification") and the
 * physical axes of a robustness curve.  raw, out, take and stats are those of iq_frames_preprocess.  Per frame, in this order:
 *   circular shift, conjugate, rotate sample n (the OUTPUT index) by theta + k*pi/2 + 2*pi*f*n, gain, add noise, z-score, layout.
 * Noise: P = mean |s|^2 over all `len` samples after the gain; sigma^2 = P / 10^(snr/10) is the total noise power, I and Q
 * get sigma^2 / 2 each (Box-Muller on uniforms in (0,1]).
 * Random numbers: philox4x32 (7 rounds, csrc/common.h), key = seed (high word ^ high word of the frame index), counter =
 * (c, low word of the frame index frame_base + i, IQ_SITE_IMPAIR, step).  c = 0xFFFFFFFF yields the frame's parameters; c = p
 * yields the noise of output samples 2p and 2p+1.  Frame j's result therefore depends on neither n_frames nor how a set of
 * frames is cut into calls.
 * drawn: NULL or fp32 [n_frames, 8] = {theta, f, k, conj, s, g, snr_db, sigma per component}: the values the kernel used
 * (snr_db NaN and sigma 0 without noise).
 * With every range [0,0], rot90 = conj = shift_max = 0, gain 0 dB and SNR NaN the output is bit-identical to
 * iq_frames_preprocess.
 * IQ_STATUS_ARG before any launch: NULL raw / out / stats / imp, lo > hi, a non-finite bound (other than both SNR bounds NaN =
 * no noise), rot90 / conj outside {0,1}, shift_max < 0 or >= len, take > len.  IQ_STATUS_UNSUPPORTED: len * 8 bytes above
 * 64 KB (one workgroup keeps one frame in LDS). */
typedef struct iq_impair {
  float phase_lo, phase_hi;      /* carrier phase theta ~ U[lo,hi] rad */
  float cfo_lo, cfo_hi;          /* frequency offset f ~ U[lo,hi] cycles/sample */
  int   rot90;                   /* 1: add k*pi/2, k uniform in 0..3 */
  int   conj;                    /* 1: Q -> -Q with probability 1/2 (before the rotation) */
  int   shift_max;               /* circular time shift s uniform in 0..shift_max: out[n] = in[(n+s) % len] */
  float gain_db_lo, gain_db_hi;  /* amplitude gain g = 10^(dB/20), dB ~ U[lo,hi] */
  float snr_db_lo, snr_db_hi;    /* complex AWGN at SNR ~ U[lo,hi] dB relative to the power of the frame AS GIVEN (after gain) */
  uint64_t seed; uint32_t step;  /* Philox key / counter word, as in iq_dropout_t */
  uint64_t frame_base;           /* index of frame 0 of this call in the caller's stream of frames */
} iq_impair_t;
int iq_frames_impair(const float* raw, float* out, float* drawn, int n_frames, int len, int take, const float* stats,
                     const iq_impair_t* imp, iq_stream_t stream);
/* Synthetic labelled frames made on the device (csrc/synth.hip): the transmitter in front of the channel above.  Frame j =
 * frame_base + i of stream `stream` is a pure function of (seed, stream, j): it depends on neither n_frames nor how a set of
 * frames is cut into calls.  The recipe is data.make_dataset's, 1 sample per symbol; per frame, in this order:
 *   1. draw the symbols of the frame's class, 2. rotate every sample by one carrier phase theta ~ U[0, 2 pi),
 *   3. divide by sqrt(mean |s|^2 + 1e-12) of that frame, 4. add complex AWGN, sigma = sqrt(0.5 * 10^(-snr/10)) per component.
 * Class and SNR: balanced = 1: class = j % n_classes, SNR index = (j / n_classes) % n_snrs; balanced = 0: both drawn (below).
 * Random numbers: philox4x32 (7 rounds, csrc/common.h), key = (low word of seed, high word of seed ^ high word of j), counter =
 * (c, low word of j, IQ_SITE_SYNTH, stream).  A word w becomes an integer in [0, M) as (uint64(w) * M) >> 32 (no modulo).
 *   c = 0xFFFFFFFF: the frame's parameters.  word 0: theta = fp32(2 pi) * (w >> 8) * 2^-24 (the rotation itself is
 *                   sincospi(2 * (w >> 8) * 2^-24)); balanced = 0 only: word 1 -> class in [0, n_classes), word 2 -> SNR index
 *                   in [0, n_snrs).  Word 3 is not used.
 *   c = p < 0x80000000: words 4p .. 4p+3 of the frame's symbol stream; len + 2 words are used:
 *       kind 0  sample n = points[offset + idx], idx = word n mapped to [0, count);                     symbols[n] = idx
 *       kind 1  GMSK approximation: b_n = 2 * (word n & 1) - 1 for n = 0 .. len+1, m_n = b_n + 2 b_{n+1} + b_{n+2},
 *               M_n = sum_{i <= n} m_i (int32), sample n = exp(j pi (M_n mod 16) / 8);                  symbols[n] = M_n mod 16
 *       kind 2  OQPSK: t_k = word k & 1; I[n] = t_{n/2}, Q[n] = t_{K0 + (n+1)/2}, K0 = len/2 + 1 (integer divisions),
 *               sample n = ((2 I - 1) + j (2 Q - 1)) / sqrt(2);                                         symbols[n] = 2 I + Q
 *   c = 0x80000000 + p: the noise of samples 2p and 2p+1: (I, Q) of sample 2p from words (0, 1), of sample 2p+1 from words
 *       (2, 3), each pair through Box-Muller on uniforms in (0,1] (the transform of iq_frames_impair):
 *       r = sqrt(-2 log(((a >> 8) + 1) 2^-24)), (I, Q) = r * (cos, sin)(2 pi (b >> 8) 2^-24).
 * Outputs: raw[n_frames, len, 2] fp32 (I, Q) pairs, the layout iq_frames_preprocess / iq_frames_impair read; labels[n_frames]
 * the class index; snr[n_frames] the SNR in dB (NaN when n_snrs = 0: no noise); drawn: NULL or fp32 [n_frames, 4] = {class,
 * snr_db, theta, mean |s|^2 before the normalisation}; symbols: NULL or int32 [n_frames, len] as listed above.
 * IQ_STATUS_ARG before any launch: NULL raw / labels / snr / par / classes, n_classes <= 0, n_snrs < 0 or NULL snrs_db with
 * n_snrs > 0, a kind outside 0..2, kind 0 with count <= 0, offset < 0 or NULL points, a non-finite SNR, balanced outside {0,1},
 * len <= 0, a misaligned pointer.  IQ_STATUS_UNSUPPORTED: len * 8 bytes above 64 KB (one workgroup keeps one frame in LDS),
 * more than IQ_SYNTH_MAX_CLASSES classes or IQ_SYNTH_MAX_SNRS SNR values (both tables travel in the kernel arguments). */
#define IQ_SYNTH_MAX_CLASSES 128
#define IQ_SYNTH_MAX_SNRS 64
typedef struct iq_synth_class { int kind; int offset; int count; } iq_synth_class_t;
    /* kind 0: memoryless constellation, points[offset .. offset+count)
       kind 1: GMSK approximation; kind 2: OQPSK (offset / count ignored for 1, 2) */
typedef struct iq_synth {
  const float* points;            /* DEVICE fp32 (re, im) pairs, already scaled to unit mean power */
  const iq_synth_class_t* classes; int n_classes;     /* HOST array, copied into the launch */
  const float* snrs_db; int n_snrs;                    /* HOST array; n_snrs = 0: no noise */
  int balanced;                   /* 1: class = j % K, SNR index = (j / K) % n_snrs (make_dataset's pattern); 0: both drawn */
  uint64_t seed; uint32_t stream; /* Philox key / counter word 3: stream 0 = train, 1 = validation, ... disjoint frames */
  uint64_t frame_base;            /* index j of frame 0 of this call */
} iq_synth_t;
int iq_frames_synth(float* raw /*[n,len,2]*/, int64_t* labels, float* snr /*[n], NaN when no noise*/,
                    float* drawn /*NULL or [n,4] = {class, snr_db, phase, power before normalisation}*/,
                    int32_t* symbols /*NULL or [n,len]*/, int n_frames, int len, const iq_synth_t* par, iq_stream_t stream);
/* Pulse-shaped labelled frames made on the device (csrc/waveform.hip): the transmitter above at `sps` samples per symbol, with a
 * timing phase and a static multipath channel.  Classes, SNRs, balanced, seed, stream, frame_base, raw, labels and snr are those
 * of iq_frames_synth; frame j = frame_base + i is again a pure function of (seed, stream, j).  Per frame, in this order:
 *   1. draw NS symbols, 2. shape them into u[n'], n' = 0 .. len+L-2, 3. pass u through the L-tap channel: v[n], n = 0 .. len-1,
 *   4. rotate by one carrier phase, 5. divide by sqrt(mean |v|^2 + 1e-12), 6. add complex AWGN; 4 to 6 in the arithmetic of
 *   iq_frames_synth.
 * L = n_taps, NS = (len + L - 1 + sps) / sps + span (integer division): the symbol words of a frame; the last few may go unused.
 * Random numbers: the key, the counter layout, the site IQ_SITE_SYNTH and the word-to-integer mapping (uint64(w) * M) >> 32 of
 * iq_frames_synth (the shared site is deliberate: see the identity below).
 *   c = 0xFFFFFFFF: words 0..2 as in iq_frames_synth (theta, class, SNR index); word 3 -> q in [0, n_phase) when timing = 1,
 *                   else q = 0: the frame's timing phase.
 *   c = 0xFFFFFFF0 + t, t = 0..3, only when L > 1: (g_re, g_im) of tap 2t = Box-Muller of words (0, 1), of tap 2t+1 = Box-Muller
 *                   of words (2, 3) (the transform of iq_frames_synth's noise); h_l = ((l == 0 ? los : 0) + tap_sigma[l] g_re,
 *                   tap_sigma[l] g_im).  With L = 1 nothing is drawn and h_0 = (1, 0).
 *   c = p < 0x80000000: words 4p .. 4p+3 of the symbol stream; word k is symbol k, k < NS.
 *   c = 0x80000000 + p: the noise of samples 2p and 2p+1, as in iq_frames_synth.
 * The shaped signal, with m = n' / sps, r = n' % sps, P = pulse[q], F = fpulse[q]:
 *   kind 0  a[k] = points[offset + idx_k], idx_k = word k mapped to [0, count); u[n'] = a[m] P[r][0], then fmaf over i = 1 ..
 *           span-1 ascending with a[m+i] P[r][i], real and imaginary parts separately (the chain starts with a product, not with
 *           zero);                                                                                    symbols[k] = idx_k
 *   kind 1  CPM (GMSK): b_k = 2 (word k & 1) - 1; inc[n'] = sum_i b[m+i] F[r][i] in wrapping int32; PHI[n'] = sum_{j <= n'}
 *           inc[j] mod 2^32; u[n'] = (cos, sin)(pi x), x = (float)(int32)PHI[n'] * 2^-31: the phase is an integer, in units of
 *           2^-32 turn, until that conversion;                                                        symbols[k] = word k & 1
 *   kind 2  OQPSK: I_k = word k & 1, Q_k = (word k >> 1) & 1, rails (2 b - 1) / sqrt 2; Re u[n'] = the I rail shaped at n' as in
 *           kind 0, Im u[n'] = the Q rail shaped at n'' = n' + sps/2 (integer division; m and r of n'');  symbols[k] = 2 I_k + Q_k
 * Channel, only when L > 1: v[n] = sum_{l < L} h_l u[n + L-1 - l], a complex product per tap, l ascending; L = 1: v = u.
 * With sps = span = n_phase = 1, pulse = {1.0}, timing = 0, n_taps = 1 and kind-0 classes only, raw, labels and snr are those
 * of iq_frames_synth for the same seed, stream and frame_base, bit for bit, and symbols[:, :len] are its symbols.
 * Outputs: drawn: NULL or fp32 [n_frames, 8] = {class, snr_db, theta, mean |v|^2 before the normalisation, q, sum_l |h_l|^2, 0,
 * 0}; symbols: NULL or int32 [n_frames, NS]; taps: NULL or fp32 [n_frames, 8, 2] = h_l as (re, im), zeros beyond L.
 * IQ_STATUS_ARG before any launch: what iq_frames_synth refuses; len, sps, span, n_phase or n_taps below 1; timing outside
 * {0,1}; a kind-0 or kind-2 class with NULL pulse, a kind-1 class with NULL fpulse; a non-finite los; a non-finite or negative
 * tap_sigma[l < L]; a misaligned pointer.  IQ_STATUS_UNSUPPORTED: sps > 16, span > 32, n_phase > 64, n_taps > 8; len * 8 bytes
 * above 64 KB; more than IQ_SYNTH_MAX_CLASSES classes or IQ_SYNTH_MAX_SNRS SNR values.  n_frames <= 0: success, no launch. */
typedef struct iq_waveform {
  const float* points; const iq_synth_class_t* classes; int n_classes;   /* as iq_synth_t; kinds 0, 1, 2 */
  const float* snrs_db; int n_snrs; int balanced;
  uint64_t seed; uint32_t stream; uint64_t frame_base;
  int sps;                 /* samples per symbol, 1..16 */
  int span;                /* taps per polyphase branch = pulse length in symbols, 1..32 */
  int n_phase;             /* timing phases in the tables, 1..64 */
  int timing;              /* 1: per-frame phase q drawn in [0, n_phase); 0: q = 0 */
  const float* pulse;      /* DEVICE fp32 [n_phase][sps][span], kinds 0 and 2: plain numbers to the kernel */
  const int32_t* fpulse;   /* DEVICE int32 [n_phase][sps][span], kind 1: phase increment per sample, units of 2^-32 turn */
  int n_taps;              /* channel taps L, 1..8; 1: no channel stage, nothing drawn */
  float los;               /* added to the real part of tap 0 */
  float tap_sigma[8];      /* per-component standard deviation of tap l */
} iq_waveform_t;
int iq_frames_waveform(float* raw /*[n,len,2]*/, int64_t* labels, float* snr, float* drawn /*NULL or [n,8]*/,
                       int32_t* symbols /*NULL or [n,NS]*/, float* taps /*NULL or [n,8,2]*/, int n_frames, int len,
                       const iq_waveform_t* par, iq_stream_t stream);
/* Fading channel (csrc/fading.hip): taps whose gains move with a Doppler spread, read at positions that drift with a sample-clock
 * offset.  It works on any raw frames: x[n_frames, len_in, 2] fp32 -> y[n_frames, len_out, 2] fp32; x[m] = x[m][0] + j x[m][1]
 * is zero outside [0, len_in) (a select supplies the zero, never a read).  L = n_taps, NS = n_sin.
 * Positions are int64 in units of 2^-32 sample; there is no floating-point time anywhere.
 *   P[n] = T0 + n S, n = 0 .. len_out-1; S = 2^32 + d, d the clock drift (int32), T0 the start.
 *   Tap l reads at Q = P[n] - (delay[l] << 16); delay[l] >= 0 is an int32 in units of 2^-16 sample.
 *   m = Q >> 32 (arithmetic: the floor, also of a negative Q); f = ((Q & 0xFFFFFFFF) * n_frac) >> 32, in [0, n_frac).
 * Interpolation: interp is a DEVICE fp32 [n_frac][K] table, plain numbers to the kernel (fading.py fills it with a Kaiser-windowed
 * sinc); c = (K - 1) / 2 (integer division).
 *   r_l[n] = sum_{k < K} x[m + k - c] interp[f][k]: the product of k = 0, then fmaf over k = 1 .. K-1 ascending, real and
 *   imaginary parts separately.
 * Tap gains: tap l is a sum of NS + 1 paths, path 0 the line of sight, paths 1 .. NS the scatterers.  phase and inc are int32 in
 * units of 2^-32 turn (per sample); phase + n inc wraps and is exact until the one conversion iq_frames_waveform and
 * iq_frames_carrier use: e(p) = (cos, sin)(pi x), x = (float)(int32)p * 2^-31 (sincospif).
 *   g_l[n] = sum_s amp[l][s] e(phase[l][s] + n inc[l][s]): from +0, fmaf(amp, cos, re) and fmaf(amp, sin, im), s = 0 .. NS
 *   ascending; a path whose amp is exactly 0 is skipped (an unused slot costs nothing and may hold anything).
 * Output: y[n] = sum_l rot(r_l[n], g_l[n]): from +0, one rounded addition per component and tap, l ascending; rot(v, c, s) = v (c +
 * j s) = (fmaf(v.re, c, -(v.im * s)), fmaf(v.re, s, v.im * c)) as in iq_frames_carrier.  Then the generators' tail: P = mean
 * |y|^2 (thread n % 256 its samples ascending, fmaf(im, im, fmaf(re, re, acc)), the wave's butterfly, the four wave sums in order);
 * normalise = 1: y / sqrt(P + 1e-12) as a product with the rounded reciprocal; snr_db NULL or DEVICE fp32 [n_frames]: where it is
 * given and not NaN, complex AWGN of sigma = sqrt(0.5 * 10^(-snr/10)) per component is added, i.e. at that SNR relative to unit
 * power (with normalise = 0 the caller's frames should have unit power for the figure to be an SNR).
 * Random numbers: key and counter layout of iq_frames_synth with the site IQ_SITE_FADE: key = (low word of seed, high word of
 * seed ^ high word of j), counter = (c, low word of j, IQ_SITE_FADE, stream), j = frame_base + i.  A frame is a pure function of
 * (seed, stream, j) and of its own input.
 *   c = 0x80000000 + p: the noise of samples 2p and 2p+1, as in iq_frames_synth (both modes).
 *   IQ_FADE_DRAWN only:
 *   c = 0xFFFFFFFF: word 0: d = d_lo + umulhi(w, d_hi - d_lo + 1); word 1: T0 = (start << 32) + (timing ? w : 0); word 2: the
 *       frame's maximum Doppler fd = min(fmaf(fd_hi - fd_lo, (w >> 8) 2^-24, fd_lo), fd_hi) cycles per sample in fp32, converted
 *       once: fd_inc = rint(fd * 2^32) (exact in double).  Word 3 is not used.
 *   c = 0xFFFFF000 + 33 l + s, l < L, s <= NS: path s of tap l.  word 0: phase[l][s] for s >= 1 (the raw word); the line of sight
 *       has phase 0 at n = 0 (the frame's carrier phase belongs to the generator, and a channel without Doppler, drift and
 *       scatterers is then the identity).  word 1: u = (w >> 8) 2^-24, inc[l][s] = rint(fd_inc * (double)cos) wrapped to int32,
 *       cos the fp32 cosine of sincospif(2 u): Clarke's model, a random arrival angle per path.
 *   amp[l][0] = los[l]; amp[l][s] = tap_sigma[l] * sqrtf(2.f / NS) (one rounded fp32 product) for 1 <= s <= NS: with tap_sigma the
 *       per-component deviation as in iq_waveform_t, E|g_l|^2 = los^2 + 2 tap_sigma^2.  Every other slot is (0, 0), amp 0.
 * IQ_FADE_GIVEN: paths int32 [n_frames, 8, 33, 2] = (phase, inc), amps fp32 [n_frames, 8, 33] and clock int64 [n_frames, 2] =
 * {T0, S} are the caller's (S as given: the caller keeps T0 + n S inside an int64); only slots l < L, s <= NS are looked at;
 * nothing is drawn but the noise.
 * Outputs: paths_out, amps_out, clock_out: NULL or arrays of those shapes: what the frame used (either mode).
 * With L = 1, NS = 0, los = 1, fd = 0, d = 0, start = 0, timing = 0, K = n_frac = 1, interp = {1.0}, normalise = 0 and no noise,
 * len_out = len_in: y = x bit for bit (but a negative zero may come back positive).
 * One workgroup of 256 threads per frame; both frames, the interpolation table and the path table lie in LDS, the output until
 * its power is known.  Lanes split samples, never paths: every sum is in loop order.  No atomics, no workspace: two runs agree
 * bit for bit, and a frame's output depends on neither n_frames nor its position.  Nothing is allocated, nothing synchronises.
 * IQ_STATUS_ARG before any launch, outputs untouched: NULL x / y / par / interp; mode outside IQ_FADE_*; NULL paths / amps / clock
 * with IQ_FADE_GIVEN; len_out or len_in below 1; n_taps, K or n_frac below 1; n_sin < 0; normalise or timing outside {0,1}; for a
 * tap l < L a negative delay or a non-finite or negative los or tap_sigma; a non-finite or negative fd_lo or fd_hi; fd_hi > 0.5;
 * fd_lo > fd_hi; d_lo > d_hi (or a range of all 2^32 values); x, y, paths, paths_out, clock, clock_out not 8-byte aligned, any
 * other pointer not 4-byte aligned.  IQ_STATUS_UNSUPPORTED: n_taps > 8, n_sin > 32, K > 16, n_frac > 256; len_in * 8 or len_out * 8
 * bytes above 64 KB; frames plus tables above the CU's 160 KB of LDS (with the limits above the largest case takes 147.1 KB, so
 * this one cannot trigger today).  n_frames <= 0: success, nothing is launched. */
enum { IQ_FADE_GIVEN = 0, IQ_FADE_DRAWN = 1 };
typedef struct iq_fading {
  int mode;                /* IQ_FADE_* */
  int len_in;              /* samples of an input frame */
  int n_taps;              /* L, 1..8 */
  int n_sin;               /* NS: scatterers per tap, 0..32 */
  int K;                   /* interpolation taps, 1..16 */
  int n_frac;              /* fractional phases in the table, 1..256 */
  int normalise;           /* 1: unit mean power */
  int timing;              /* DRAWN: 1: a fractional start drawn per frame */
  const float* interp;     /* DEVICE fp32 [n_frac][K] */
  const float* snr_db;     /* NULL or DEVICE fp32 [n_frames]; NaN: no noise for that frame */
  const int32_t* paths;    /* GIVEN: DEVICE int32 [n_frames,8,33,2] = (phase, inc) */
  const float* amps;       /* GIVEN: DEVICE fp32 [n_frames,8,33] */
  const int64_t* clock;    /* GIVEN: DEVICE int64 [n_frames,2] = {T0, S} */
  int32_t delay[8];        /* tap delays, units of 2^-16 sample, >= 0 */
  float los[8];            /* DRAWN: amplitude of the line of sight of tap l */
  float tap_sigma[8];      /* DRAWN: per-component deviation of the scatter of tap l */
  float fd_lo, fd_hi;      /* DRAWN: maximum Doppler ~ U[lo,hi] cycles per sample, 0 <= lo <= hi <= 0.5 */
  int32_t d_lo, d_hi;      /* DRAWN: clock drift d uniform in lo..hi, units of 2^-32 sample per sample */
  int32_t start;           /* DRAWN: integer part of T0, in samples */
  uint32_t stream;         /* Philox counter word 3 */
  uint64_t seed;
  uint64_t frame_base;     /* index j of frame 0 of this call */
} iq_fading_t;
int iq_frames_fade(const float* x /*[n,len_in,2]*/, float* y /*[n,len_out,2]*/, int32_t* paths_out /*NULL or [n,8,33,2]*/,
                   float* amps_out /*NULL or [n,8,33]*/, int64_t* clock_out /*NULL or [n,2]*/, int n_frames, int len_out,
                   const iq_fading_t* par, iq_stream_t stream);
/* Receiver for the frames above (csrc/receiver.hip): matched filter, one timing estimate per frame, one sample per symbol.
 * raw[n_frames, len, 2] fp32, x[n] = raw[n][0] + j raw[n][1], zero outside [0, len).  table G is DEVICE fp32 [n_frac][J+1],
 * J = sps * span, h = J / 2 (integer division): plain numbers to the kernel (receiver.py fills it with G[f][j] =
 * p((f / n_frac + h - j) / sps) / sqrt(sps), p the root-raised cosine, zero where the argument leaves the span).  The
 * interpolating matched filter at time m + f / n_frac (in samples) is
 *   y(m + f / n_frac) = sum_{j = 0 .. J} x[m + j - h] G[f][j].
 * Energies: E[r] = sum_{n = r (mod sps), 0 <= n < len} |y(n)|^2, r = 0 .. sps-1 (f = 0 at every sample of the frame).  y(n) is an
 * fp32-input MFMA product (an fp32 fmaf chain per output), |y|^2 = fmaf(im, im, re * re); the sum over n runs in a fixed order
 * (lane l of a wave adds n = r + sps (l + 64 i), i ascending, then the wave's butterfly): no atomics, two runs agree bit for bit.
 * Timing: u in [0, sps * n_frac) is the sampling instant in units of 1 / n_frac sample, r^ = u / n_frac, f^ = u % n_frac.
 *   IQ_RX_GIVEN        u = par->u[frame] reduced into [0, sps * n_frac) (NULL: 0); est t0 = NaN
 *   IQ_RX_OERDER_MEYR  X = sum_r E[r] exp(-2 pi j r / sps), t0 = (-arg X * sps / 2 pi) mod sps, u = rint(t0 * n_frac) mod
 *                      (sps * n_frac); a non-finite t0 gives u = 0.  Needs sps >= 3.
 *   IQ_RX_ENERGY       u = n_frac * argmax_r E[r], the lowest r on ties (and when no E[r] compares: r = 0); est t0 = r
 * Symbols: v[k] = y(r^ + f^ / n_frac + k sps), k = 0 .. n_out-1, n_out = len / sps (integer division): an fmaf chain over j
 * ascending from 0.  normalise = 1: s = v / sqrt(mean_k |v[k]|^2 + 1e-12); 0: s = v.
 * Outputs: sym[n_frames, n_out, 2] fp32; est: NULL or fp32 [n_frames, 4] = {t0 in samples, u, |X| / sum_r E[r] (0 when the sum
 * is 0), mean |v|^2}; energy: NULL or fp32 [n_frames, sps].  A frame's outputs depend on neither n_frames nor its position.
 * iq_frames_receive_bwd: the adjoint with the timing held fixed: u = par->u as in IQ_RX_GIVEN whatever par->mode says (pass the
 * u of the forward's est).  normalise = 1: dv = (ds - s Re<ds, s> / n_out) / rho, s = the forward's sym, rho = sqrt(est[3] +
 * 1e-12) from the forward's est (required then); 0: dv = ds, sym and est are not read.  Then
 *   dx[n] = sum_k dv[k] G[f^][n - k sps - r^ + h], over the k with an index in [0, J], k ascending: a gather, no atomics, two
 * runs agree bit for bit.  dx[n_frames, len, 2].
 * IQ_STATUS_ARG before any launch, outputs untouched: NULL raw / sym / dsym / dx / par / table, NULL sym or est in the backward
 * with normalise = 1, len, sps, span or n_frac below 1, mode outside 0..2, normalise outside {0,1}, raw / sym / dsym / dx not
 * 8-byte or any other pointer not 4-byte aligned.  IQ_STATUS_UNSUPPORTED: sps > 16, span > 32, n_frac > 64, len * 8 bytes above
 * 64 KB, len < sps, IQ_RX_OERDER_MEYR with sps < 3.  n_frames <= 0: success, nothing is launched. */
enum { IQ_RX_GIVEN = 0, IQ_RX_OERDER_MEYR = 1, IQ_RX_ENERGY = 2 };
typedef struct iq_receiver {
  int sps;                 /* samples per symbol, 1..16 */
  int span;                /* matched-filter length in symbols, 1..32: J = sps * span, J + 1 taps */
  int n_frac;              /* fractional phases in the table, 1..64 */
  int mode;                /* IQ_RX_* */
  int normalise;           /* 1: unit mean power per frame */
  const float* table;      /* DEVICE fp32 [n_frac][J+1] */
  const int32_t* u;        /* DEVICE int32 [n_frames] or NULL: IQ_RX_GIVEN and the backward */
} iq_receiver_t;
int iq_frames_receive(const float* raw /*[n,len,2]*/, float* sym /*[n,len/sps,2]*/, float* est /*NULL or [n,4]*/,
                      float* energy /*NULL or [n,sps]*/, int n_frames, int len, const iq_receiver_t* par, iq_stream_t stream);
int iq_frames_receive_bwd(const float* dsym /*[n,len/sps,2]*/, const float* sym, const float* est, float* dx /*[n,len,2]*/,
                          int n_frames, int len, const iq_receiver_t* par, iq_stream_t stream);
/* Spectrogram front end (csrc/spectrogram.hip): the time-frequency image between the channel above and the ViT, and its adjoint.
 * x[n_frames, 2, len] fp32 is the planar output of iq_frames_preprocess / iq_frames_impair with take = len (I plane, then Q
 * plane).  Column t of a frame's image is the transform of the n_fft samples from j0 = t*hop - pad; with j = j0 + m:
 *   Re[t,k] = sum_m I[j] c[m,k] + Q[j] s[m,k],   Im[t,k] = sum_m Q[j] c[m,k] - I[j] s[m,k],   m = 0 .. n_fft-1,
 * samples with j outside [0, len) count as zero and are never read.  table is DEVICE fp32 [2, n_fft, n_fft], table[0][m][k] =
 * c[m,k], table[1][m][k] = s[m,k]: plain numbers to the kernel (spectrogram.py fills it with w[m] cos / sin(2 pi k m / n_fft),
 * computed in fp64 and rounded).  P = (Re^2 + Im^2) * inv_norm; mode 0: out = P * scale + shift; mode 1: out = log10(P + floor)
 * * scale + shift, the product and the sum rounded separately (no fused multiply-add).  out[n_frames, 1, n_fft, width]: row r
 * holds bin k = (r + n_fft/2) mod n_fft (numpy.fft.fftshift order: row 0 is the most negative frequency), column t is contiguous.
 * Arithmetic: fp32-input MFMA, i.e. per accumulator an fp32 fmaf chain over m in ascending order, for each pair (m, m+1) the
 * two c (Re: I c; Im: Q c) products before the two s products.  A frame's image depends on neither n_frames nor its position.
 * iq_frames_spectrogram_bwd: dx[n_frames, 2, len] = the gradient of sum(out * dout) with respect to x; Re / Im are recomputed
 * from x.  g = dout * scale * inv_norm (mode 1: / (ln 10 * (P + floor))), dRe = 2 Re g, dIm = 2 Im g,
 *   G_I[t,m] = sum_k dRe[t,k] c[m,k] - dIm[t,k] s[m,k],   G_Q[t,m] = sum_k dRe[t,k] s[m,k] + dIm[t,k] c[m,k]   (k in image-row
 * order), dx[0][j] = sum of G_I[t, j + pad - t*hop] over the columns t whose window covers j, dx[1][j] likewise from G_Q: a
 * gather in a fixed order, no atomics, two runs agree bit for bit; samples no window covers get exactly 0.
 * IQ_STATUS_ARG before any launch: NULL x / table / out / dout / dx / par, len < 1, hop < 1, width < 1, pad < 0, mode outside
 * {0,1}, a non-finite inv_norm / floor / scale / shift, floor <= 0 in mode 1, x / out / dout / dx not 4-byte or table not
 * 16-byte aligned.  IQ_STATUS_UNSUPPORTED before any launch: n_fft not a multiple of 32 in [32, 256]; len * 8 bytes above
 * 64 KB (one workgroup keeps one frame in LDS).  n_frames <= 0: success, nothing is launched. */
typedef struct iq_spectrogram {
  int n_fft;      /* window length = number of frequency rows H */
  int hop;        /* column t's window starts at sample t*hop - pad */
  int pad;        /* >= 0; samples outside [0,len) count as zero and are never read */
  int width;      /* number of time columns W */
  int mode;       /* 0: out = P*scale + shift;  1: out = log10(P + floor)*scale + shift */
  float inv_norm, floor, scale, shift;   /* P = (Re^2 + Im^2) * inv_norm */
} iq_spectrogram_t;
int iq_frames_spectrogram(const float* x /*[n,2,len]*/, const float* table /*DEVICE [2,n_fft,n_fft]*/,
                          float* out /*[n,1,n_fft,width]*/, int n_frames, int len, const iq_spectrogram_t* par,
                          iq_stream_t stream);
int iq_frames_spectrogram_bwd(const float* x, const float* table, const float* dout /*[n,1,n_fft,width]*/,
                              float* dx /*[n,2,len]*/, int n_frames, int len, const iq_spectrogram_t* par,
                              iq_stream_t stream);
/* Cyclic-spectrum front end (csrc/cyclic.hip): the spectral correlation function (SCF) of a frame and its conjugate as square
 * (cyclic frequency, frequency) images, by the first stage of the FFT accumulation method.  x and table are the spectrogram's:
 * x[n_frames, 2, len] planar, table DEVICE fp32 [2, Np, Np] = (c, s), Np = n_fft.  rot is DEVICE fp32 [2, Np], rot[0][r] = rc[r],
 * rot[1][r] = rs[r]: plain numbers to the kernel (cyclic.py fills it with cos / sin(2 pi r / Np), computed in fp64 and rounded).
 * Window t = 0 .. columns-1 starts at j0 = t*hop - pad; samples outside [0, len) count as zero and are never read.
 *   X[t,k]  = Re + i Im of the spectrogram entry above
 *   Y[t,k]  = X[t,k] (rc[r] - i rs[r]),  r = (k * (j0 mod Np)) mod Np, both mods non-negative: the phase of window t referred to
 *             sample 0.  Yre = fmaf(Xim, rs, Xre * rc), Yim = fmaf(-Xre, rs, Xim * rc).
 *   S[k,l]  = sum_t Y[t,k] conj(Y[t,l])   (SCF at alpha = f_k - f_l),     Sc[k,l] = sum_t Y[t,k] Y[t,l]   (alpha = f_k + f_l)
 *   D[k]    = sum_t |Y[t,k]|^2
 *   P = |S|^2 * inv2 (Pc from Sc likewise), |S|^2 = fmaf(Sim, Sim, Sre * Sre), inv2 = inv_norm * inv_norm rounded to fp32
 *   mode 0 (power): v = P;  mode 1 (log): v = log10(P + floor);  mode 2 (coherence): v = P / ((D[k] * D[l]) * inv2 + floor), the
 *   two products and the sum rounded separately.  out = v * scale + shift, product and sum rounded separately.
 * out[n_frames, C, Np, Np]: row rho holds cyclic bin a = (rho + Np/2) mod Np, column kappa holds channel k = (kappa + Np/2) mod Np
 * (both in fftshift order); the SCF channel reads l = (k - a) mod Np, the conjugate channel l = (a - k) mod Np.  kind 0: SCF only
 * (C = 1); 1: conjugate only (C = 1); 2: both (C = 2, SCF first).
 * Arithmetic: fp32-input MFMA throughout.  X: per accumulator an fp32 fmaf chain over m ascending, for each pair (m, m+1) the
 * two c products before the two s products, as the spectrogram.  S, Sc: per accumulator an fmaf chain over t ascending from 0,
 * for each pair (t, t+1) the two Re(l) Re(k) products before the two Im(l) Im(k) products (real parts; SCF adds, the conjugate
 * subtracts) resp. the two Re(l) Im(k) before the two Im(l) Re(k) products (imaginary parts; SCF subtracts, the conjugate adds).
 * D[k]: d = fmaf(Yim, Yim, fmaf(Yre, Yre, d)) over t ascending.  No atomics: two runs agree bit for bit, and a frame's image
 * depends on neither n_frames nor its position.  Nothing is allocated, the host is not synchronised.
 * IQ_STATUS_ARG before any launch: NULL x / table / rot / out / par, len < 1, hop < 1, columns < 1, pad < 0, kind or mode outside
 * 0..2, a non-finite inv_norm / floor / scale / shift, floor <= 0 in mode 1 or 2, x / table / rot not 4-byte or out not 16-byte
 * aligned.  IQ_STATUS_UNSUPPORTED before any launch: n_fft not a multiple of 32 in [32, 256]; len * 8 bytes above 64 KB (one
 * workgroup keeps one frame in LDS).  Within these the LDS plan holds every case (frame + rot + D + 32 columns of Y: at most
 * 64 KB + 3 KB + 64.25 KB of 160 KB), so nothing else is refused.  n_frames <= 0: success, nothing is launched.
 * Launch shape (the image is the same bit for bit): with chunks = ceil(columns / 32), when 4 * (2 len rounded up to 4 + 3 Np +
 * chunks * 64 (Np + 1) + 64 Np) bytes <= 144 KB one workgroup per frame keeps all of Y in LDS and takes the bands of 32 channels
 * in turn; otherwise one workgroup per (frame, band) holds 32 columns of Y at a time and recomputes X for its band.
 * iq_frames_cyclic_bwd: dx[n_frames, 2, len] = the gradient of L = sum(out * dout) with respect to x; everything is recomputed
 * from x (no workspace).  For a complex w, G_w = dL/dRe w + i dL/dIm w; rho[t,k] = rc[r] + i rs[r], so Y = X conj(rho).  Per
 * channel an image element is one pair (k, l): SCF row of a = k - l, column of k: g[k,l] = dout there; conjugate row of a =
 * k + l, column of k: gc[k,l].  P, Pc and den = D[k] D[l] inv2 + floor are symmetric in (k, l), so the two elements of a pair
 * fold into one weight:
 *   phi(P, den) = 1 (power),  1 / (ln 10 (P + floor)) (log),  1 / den (coherence)
 *   u[k,l]  = scale (g[k,l] + g[l,k]) phi(P[k,l], den[k,l]),     uc[k,l] = scale (gc[k,l] + gc[l,k]) phi(Pc[k,l], den[k,l])
 *   H[k,l]  = 2 inv2 u[k,l] S[k,l],                              Hc[k,l] = 2 inv2 uc[k,l] Sc[k,l]
 *   gD[k]   = - inv2 sum_l scale [(g[k,l] + g[l,k]) P[k,l] + (gc[k,l] + gc[l,k]) Pc[k,l]] D[l] / den[k,l]^2   (coherence, else 0)
 *   G_Y[t,k] = sum_l H[k,l] Y[t,l] + sum_l Hc[k,l] conj(Y[t,l]) + 2 gD[k] Y[t,k]
 *   G_X[t,k] = rho[t,k] G_Y[t,k]:  dRe = dYre rc - dYim rs,  dIm = dYre rs + dYim rc   (the transpose of the forward's rotation
 *              for ANY table values)
 *   G_z[j]   = sum over the windows t and offsets m with j0(t) + m = j of sum_k (c[m,k] + i s[m,k]) G_X[t,k]
 *   dx[.,0,j] = Re G_z[j],  dx[.,1,j] = Im G_z[j]
 * A kind with one channel drops the other channel's terms; columns at and behind `columns` and samples outside [0, len)
 * contribute nothing; a sample no window covers gets exactly 0.  S, Sc, D and Y are the forward's, bit for bit.  Every element of
 * dx is written exactly once, by one thread, after a gather in a fixed order (per band of 32 channels k, per 32 columns, the
 * columns ascending; the sum over l of G_Y per wave over its l tiles, then (wave 0 + wave 2) + (wave 1 + wave 3)): no atomics,
 * two runs agree bit for bit, a frame's gradient depends on neither n_frames nor its position.  Nothing but dx is written.
 * Refusals as iq_frames_cyclic, in the same order, with dout and dx in the place of out: NULL dout / dx and dout / dx not
 * 4-byte aligned are IQ_STATUS_ARG.  One workgroup holds the frame, its gradient, rot, D, 32 columns of Y and six 32 x 33 tiles
 * in the CU's 160 KB of LDS, so IQ_STATUS_UNSUPPORTED also when
 *   4 * (2 * (2 len rounded up to 4) + 67 Np + 6688) bytes > 160 KB
 * (a function of len and Np alone, not of columns: at Np = 256 every len <= 4280 is taken, at Np = 32 every len <= 8032).
 * n_frames <= 0: success, nothing is launched.  All of Y is kept in LDS when 4 * (2 * (2 len rounded up to 4) + 3 Np + 6624 +
 * chunks * 64 (Np + 1)) bytes <= 160 KB; otherwise every band recomputes X chunk by chunk (the same arithmetic in the same
 * order). */
typedef struct iq_cyclic {
  int n_fft;      /* window length Np = image height = image width */
  int hop;        /* window t starts at sample t*hop - pad */
  int pad;        /* >= 0 */
  int columns;    /* number of windows T summed over */
  int kind;       /* 0: SCF; 1: conjugate SCF; 2: both, SCF first */
  int mode;       /* 0: power; 1: log; 2: coherence */
  float inv_norm, floor, scale, shift;
} iq_cyclic_t;
int iq_frames_cyclic(const float* x /*[n,2,len]*/, const float* table /*DEVICE [2,n_fft,n_fft]*/, const float* rot /*DEVICE [2,n_fft]*/,
                     float* out /*[n,C,n_fft,n_fft]*/, int n_frames, int len, const iq_cyclic_t* par, iq_stream_t stream);
int iq_frames_cyclic_bwd(const float* x, const float* table, const float* rot, const float* dout /*[n,C,n_fft,n_fft]*/,
                         float* dx /*[n,2,len]*/, int n_frames, int len, const iq_cyclic_t* par, iq_stream_t stream);
/* Constellation front end (csrc/constellation.hip): the smoothed 2-D density of the (I, Q) points of a frame as an image, and
 * its adjoint.  x[n_frames, 2, len] planar fp32 as above (for symbols: the transposed output of iq_frames_receive).  table is
 * DEVICE fp32 [radius * n_frac + 1], plain numbers to the kernel: a radial profile sampled every 1 / n_frac pixel of distance;
 * the caller makes table[last] = 0 for continuity.  Column weight of point n for image column c = 0 .. width-1:
 *   u = fmaf(I[n], x_scale, x_off)      pixel units; pixel c covers [c, c+1), its centre is c + 0.5
 *   e = u - (c + 0.5f),  d = |e|,  t = d * (float)n_frac   (one rounding)
 *   not (t < radius * n_frac): b[n,c] = 0 exactly (a NaN or infinite sample fails the compare: it contributes to no pixel)
 *   else i = (int)floorf(t), f = t - i (exact), b[n,c] = fmaf(f, table[i+1] - table[i], table[i]), the difference rounded first.
 * The row weight a[n,r], r = 0 .. height-1, is the same from Q[n] with y_scale / y_off.  D[r,c] = the fp32 fmaf chain over n
 * ascending of a[n,r] * b[n,c], starting from +0 (fp32-input MFMA).  Skipping any n whose a[n,r] or b[n,c] is zero leaves this
 * chain unchanged bit for bit because the table is finite, and the kernel skips the points that cannot reach a 32 x 32 tile;
 * non-finite table entries make the result unspecified.  v = D * inv_norm; mode 0: out = v * scale + shift; mode 1: out =
 * log10f(v + floor) * scale + shift, the product and the sum rounded separately.  out[n_frames, 1, height, width]: row 0 is the
 * most negative Q, column c is contiguous.  No atomics: two runs agree bit for bit, and a frame's image depends on neither
 * n_frames nor its position.  Nothing is allocated, the host is not synchronised.
 * Launch shape (the image is the same bit for bit whatever it is): one workgroup per (frame, 32 image rows); its four waves take
 * the 32-column tiles in turn, each compacting the frame's points within reach of its tile (order preserved) and running the
 * chain over those only.  LDS: the frame, the table and four lists of up to len + 7 16-bit indices, at most 132.1 KB of 160 KB.
 * iq_frames_constellation_bwd: dx[n_frames, 2, len] = the gradient of sum(out * dout) with respect to x; everything is
 * recomputed from x (no workspace), nothing but dx is written.  g[r,c] = (dout * scale) * inv_norm; in mode 1 divided by
 * ln 10 * (v + floor), v the forward's value bit for bit.  b'[n,c] = sgn(e) * (table[i+1] - table[i]) where the compare above
 * passes (the slope of the segment i = floor(t) the weight was taken from, also where the weight itself happens to be 0) and 0
 * elsewhere, sgn(0) = 0; a' likewise for rows.
 *   dx[.,0,n] = (x_scale * n_frac) * sum_{r,c} g[r,c] a[n,r]  b'[n,c]
 *   dx[.,1,n] = (y_scale * n_frac) * sum_{r,c} g[r,c] a'[n,r] b[n,c]
 * Order of the sums: the 32 x 32 tiles in row-major order; per tile the rows r ascending; per row s = the fmaf chain over the
 * tile's columns c ascending of g[r,c] * b'[n,c] (resp. b[n,c]) from +0, then sum = fmaf(a[n,r], s, sum) (resp. a'[n,r]); rows
 * and columns out of the point's reach and rows with a = a' = 0 are skipped; one product by the rounded (x_scale * n_frac) at
 * the end.  Element n of dx is read and written by one thread only (n mod 256 of the frame's workgroup), in program order: no
 * atomics, two runs agree bit for bit, a frame's gradient depends on neither n_frames nor its position.  A dropped sample
 * (NaN, infinite, or out of reach of every pixel) gets exactly 0.  One workgroup per frame; LDS: the frame, the table, four
 * 32 x 33 tiles of g and the four lists, at most 148.6 KB of 160 KB, so the adjoint refuses nothing the forward takes.
 * IQ_STATUS_ARG before any launch, outputs untouched: NULL x / table / out / dout / dx / par, len < 1, mode outside {0,1}, a
 * non-finite x_scale / x_off / y_scale / y_off / inv_norm / floor / scale / shift, floor <= 0 in mode 1, x / table / out /
 * dout / dx not 4-byte aligned (the kernels move single floats; 16-byte aligned frames of even len are staged in 16-byte
 * groups).  IQ_STATUS_UNSUPPORTED before any launch: height or width not a multiple of 32 in [32, 256]; radius outside
 * 1..16; n_frac outside 1..64; len * 8 bytes above 64 KB (one workgroup keeps one frame in LDS).  n_frames <= 0: success,
 * nothing is launched. */
typedef struct iq_constellation {
  int height, width;   /* image rows (Q) and columns (I): multiples of 32 in [32, 256] */
  int radius;          /* pixels, 1 .. 16: a point reaches at most two tiles per axis */
  int n_frac;          /* table samples per pixel, 1 .. 64 */
  int mode;            /* 0: out = v*scale + shift;  1: out = log10(v + floor)*scale + shift */
  float x_scale, x_off, y_scale, y_off;   /* pixel coordinate = sample * scale + off */
  float inv_norm, floor, scale, shift;    /* v = D * inv_norm */
} iq_constellation_t;
int iq_frames_constellation(const float* x /*[n,2,len]*/, const float* table /*DEVICE [radius*n_frac+1]*/,
                            float* out /*[n,1,height,width]*/, int n_frames, int len, const iq_constellation_t* par,
                            iq_stream_t stream);
int iq_frames_constellation_bwd(const float* x, const float* table, const float* dout /*[n,1,height,width]*/,
                                float* dx /*[n,2,len]*/, int n_frames, int len, const iq_constellation_t* par,
                                iq_stream_t stream);
/* Carrier recovery (csrc/carrier.hip): a blind frequency and phase estimate per frame from the spectral line of the M-th power
 * (M-PSK / QAM modulation drops out of z^M and leaves a line at M f), and the derotation.  It sits between the receiver and the
 * constellation.  x and out are fp32 frames of len samples, planar = 0: [n_frames, len, 2]; planar = 1: [n_frames, 2, len];
 * z[n] = I[n] + j Q[n].  t1, t2 and tw are DEVICE tables, plain numbers to the kernel (carrier.py fills them with t[0][m][k] =
 * cos(2 pi m k / n), t[1][m][k] = sin(2 pi m k / n) and tw[0][i] = cos(2 pi i / N), tw[1][i] = sin(2 pi i / N), computed in fp64
 * from integer numerators and rounded; W below is then the N-point DFT of w).  Phases are integers in units of 2^-32 turn, as in
 * iq_frames_waveform: e(p) = (cos, sin)(pi x), x = (float)(int32)p * 2^-31.  rot(v, c, s) = v (c + j s) = (fmaf(v.re, c,
 * -(v.im * s)), fmaf(v.re, s, v.im * c)), the inner products rounded.  Per frame, in this order (IQ_CR_ESTIMATE):
 *   1. w[n] = z[n]^M by log2 M squarings, each v <- rot(v, v.re, v.im); w[n] = 0 for len <= n < N, N = n1 n2.
 *   2. With n = a n2 + b (a < n1, b < n2) and k = k1 + n1 k2 (k1 < n1, k2 < n2):
 *        A[k1,b]  = sum_a w[a n2 + b] (c1 - j s1)[a][k1]
 *        Bm[k1,b] = rot(A[k1,b], twc[b k1], -tws[b k1])          (b k1 < N always)
 *        W[k]     = sum_b Bm[k1,b] (c2 - j s2)[b][k2]
 *      Both sums are fp32-input MFMA products, i.e. per output an fp32 fmaf chain from +0 over the summation index ascending,
 *      for each pair (m, m+1) of it the two c products before the two s products: Re: c Re(v), s Im(v); Im: c Im(v), -s Re(v).
 *   3. P[k] = fmaf(Im W, Im W, Re W * Re W); written to power[frame][k], k = 0 .. N-1 in natural order, when power is not NULL.
 *   4. Peak: s^ = the first maximum of P[s mod N] over the signed bins s = -k_max .. min(k_max, N/2 - 1) ascending (a NaN counts
 *      as +infinity), k^ = s^ mod N, b = P[k^].  If b is 0 or not finite: F = TH = 0, d = 0, est[1] = est[3] = 0, steps 5 to 7
 *      are skipped and out = rot(z, 1, -0).
 *   5. Refinement (refine = 1): a = P[(k^ - 1) mod N], c = P[(k^ + 1) mod N] (neighbours outside the search range count), den =
 *      (a - (b + b)) + c, d = min(max((0.5 (a - c)) / den, -0.5), 0.5) when den < 0 and finite, else 0; every operation
 *      rounded to fp32.  refine = 0: d = 0.
 *   6. F = (int32) rint((s^ + d) / (N M) * 2^32) in double, wrapping: the carrier frequency in units of 2^-32 cycle per sample.
 *   7. G = F M (wrapping); S = sum_{n < len} rot(w[n], cos, -sin of e(G n)), real and imaginary parts added separately: thread
 *      n % 256 its samples n ascending, then the wave's butterfly, then the four wave sums in order; sum |w|^2 likewise with
 *      fmaf(Im, Im, fmaf(Re, Re, acc)).  TH = (int32) rint(atan2(Im S, Re S) / (2 pi M) * 2^32) in double, wrapping.
 *   8. out[n] = rot(z[n], c, -s), (c, s) = e(F n + TH) (wrapping).  The M-th-power line of out is then real and positive at bin
 *      0, up to the resolution of the estimate.
 * What remains: the M-fold ambiguity (the estimate fixes M times the phase: out is the constellation turned by an unknown multiple
 * of 2 pi / M, and F is known modulo 1 / M cycle per sample), and the constellation's own M-th-power angle (sum a^M of a
 * diagonal QPSK is negative: its points come out on the axes, turned by pi / 4).
 * Outputs: est: NULL or fp32 [n_frames, 4] = {F 2^-32 (cycles per sample), TH 2^-32 2 pi (radians), s^ + d (bins of the M-th
 * power), |S|^2 / (len sum |w|^2): a lock quality in [0, 1], 0 when the denominator is 0}; fth_out: NULL or int32 [n_frames, 2]
 * = {F, TH}.  IQ_CR_GIVEN: F and TH are par->fth[frame], only step 8 runs, no table is read (t1, t2, tw may be NULL); fth_out
 * repeats them, est = {F 2^-32, TH 2^-32 2 pi, NaN, NaN}.  No atomics: two runs agree bit for bit, and a frame's outputs depend on
 * neither n_frames nor its position.  Nothing is allocated, the host is not synchronised.
 * iq_frames_carrier_bwd: dx[n] = rot(dout[n], c, s), (c, s) = e(F n + TH), F and TH from par->fth whatever par->mode says: the
 * adjoint with the estimate held fixed (pass the forward's fth_out), as the receiver holds its timing.  dout, dx in x's layout.
 * One workgroup per frame.  LDS: w and Bm, planar, 16 N bytes, and one padding word per row of Bm (8 n2 bytes: the second stage
 * reads Bm transposed relative to how the first writes it), at most 128.3 KB of 160 KB; P takes w's place once stage 1 has
 * consumed it, and z is read from memory again for steps 7 and 8.
 * IQ_STATUS_ARG before any launch, outputs untouched: NULL x / out / dout / dx / par; order outside {1,2,4,8}; refine, planar
 * outside {0,1}; mode outside IQ_CR_*; len < 1; k_max outside [0, N/2]; x / out / dout / dx not 8-byte (planar = 0) or 4-byte
 * (planar = 1) aligned, any other pointer not 4-byte aligned; NULL t1 / t2 / tw with IQ_CR_ESTIMATE; NULL fth with IQ_CR_GIVEN or
 * in the backward; a non-NULL power with IQ_CR_GIVEN.  IQ_STATUS_UNSUPPORTED: n1 or n2 not a multiple of 32 in [32, 256], N < len,
 * N > 8192, len * 8 bytes above 64 KB.  n_frames <= 0: success, nothing is launched. */
enum { IQ_CR_GIVEN = 0, IQ_CR_ESTIMATE = 1 };
typedef struct iq_carrier {
  int order;      /* M in {1,2,4,8} */
  int n1, n2;     /* DFT size N = n1*n2, each a multiple of 32 in [32,256]; N >= len */
  int k_max;      /* search signed bins s in [-k_max, min(k_max, N/2-1)], 0 <= k_max <= N/2 */
  int refine;     /* 1: parabolic interpolation of the peak */
  int planar;     /* 0: x,out [n,len,2]; 1: [n,2,len] */
  int mode;       /* IQ_CR_* */
  const float* t1;     /* DEVICE fp32 [2][n1][n1] = (c,s)[m][k] */
  const float* t2;     /* DEVICE fp32 [2][n2][n2] */
  const float* tw;     /* DEVICE fp32 [2][N] */
  const int32_t* fth;  /* DEVICE int32 [n,2] = {F, TH}: IQ_CR_GIVEN and the backward */
} iq_carrier_t;
int iq_frames_carrier(const float* x, float* out, float* est /*NULL or [n,4]*/, int32_t* fth_out /*NULL or [n,2]*/,
                      float* power /*NULL or [n,N]; must be NULL when GIVEN*/, int n_frames, int len,
                      const iq_carrier_t* par, iq_stream_t stream);
int iq_frames_carrier_bwd(const float* dout, float* dx, int n_frames, int len, const iq_carrier_t* par, iq_stream_t stream);
/* Blind equaliser (csrc/equaliser.hip): an L-tap complex filter per frame, found by block constant-modulus descent (CMA) on the
 * frame itself, and the filter.  It sits behind the receiver and undoes what a static multipath channel (iq_waveform_t.n_taps)
 * leaves between the symbols.  x and out are fp32 frames of len complex points, planar = 0: [n_frames, len, 2], the receiver's
 * output; planar = 1: [n_frames, 2, len], the front ends' input (as iq_carrier_t); z[n] = I[n] + j Q[n], and z[n] = 0 outside
 * [0, len).  L = taps weights w[l], l = 0 .. L-1, centre c = L / 2 (integer division).
 *   Filter:  y[n] = sum_l w[l] z[n + c - l], n = 0 .. len-1: per output one fp32 fmaf chain from +0 over l ascending, the real part
 *            taking + Re z Re w then - Im z Im w, the imaginary part + Re z Im w then + Im z Re w (four fmaf per tap, no
 *            separately rounded product).
 *   IQ_EQ_CMA.  w^0 = par->w0[frame] (DEVICE fp32 [n_frames, L, 2]), or the unit spike at c (w[c] = 1, every other weight 0) when
 *            w0 is NULL.  For t = 0 .. iters-1, with y from w^t:
 *              d[n] = (fmaf(Im y, Im y, Re y * Re y)) - R         R = modulus, the dispersion constant E|a|^4 / E|a|^2 of the
 *              e[n] = (Re y * d, Im y * d)                        constellation: 1 for PSK at unit power
 *              G[l] = sum_n conj(z[n + c - l]) e[n]:  Re += Re z Re e, then Im z Im e;  Im += Re z Im e, then - Im z Re e, all fmaf
 *              w^{t+1}[l] = fmaf(-mu, G[l] / (float)len, w^t[l]), the real and the imaginary word alike (g = G / len)
 *            Every sum over n runs in one order: thread n % 256 its outputs n ascending (a chain of fmaf from +0), then the
 *            wave's butterfly (xor 32, 16, 8, 4, 2, 1), then the four wave sums ((s0 + s1) + s2) + s3.  Then out = y from
 *            w^iters.  The input is expected at unit mean power (iq_receiver_t.normalise = 1): R is in its units.
 *   IQ_EQ_GIVEN.  w = par->w[frame]; only the filter runs.  iters, mu and w0 are checked as below and not read otherwise;
 *            modulus is used: est[1] = J(w) is formed with it.
 * Outputs: out; w_out: NULL or fp32 [n_frames, L, 2] = w^iters (GIVEN: w); est: NULL or fp32 [n_frames, 4] = {J(w^0), J(w^iters),
 * sum_l |w[l]|^2 (l ascending, fmaf(Im, Im, fmaf(Re, Re, acc))), the index of the largest fmaf(Im w, Im w, Re w * Re w), the
 * lowest on ties}, w = w^iters in the last two; J(w) = (sum_n d[n]^2) / (float)len with y from w, the sum as fmaf(d, d, acc) in
 * the order above.  With iters = 0, J(w^0) = J(w^iters); under GIVEN est[0] is NaN.  NaNs are not special-cased: they propagate
 * within their frame only.  No atomics: two runs agree bit for bit, and a frame's outputs depend on neither n_frames nor its
 * position.  Nothing is allocated, the host is not synchronised; the iters steps run inside one launch.
 * iq_frames_equalise_bwd: dx[m] = sum_l conj(w[l]) dout[m - c + l], dout zero outside the frame; per output an fmaf chain over l
 * ascending, Re: + Re d Re w then + Im d Im w, Im: + Im d Re w then - Re d Im w.  w = par->w[frame] whatever par->mode says: the
 * adjoint with the weights held fixed (pass the forward's w_out), as the receiver holds its timing and the carrier its estimate.
 * One workgroup per frame.  LDS: the frame as two planes, each with 32 zeros on either side, w, and the wave sums: at most 65.8 KB.
 * IQ_STATUS_ARG before any launch, outputs untouched: NULL x / out / dout / dx / par; taps < 1; len < 1; iters < 0; mu or modulus
 * not finite, mu < 0; planar outside {0,1}; mode outside IQ_EQ_*; x / out / dout / dx not 8-byte (planar = 0) or 4-byte
 * (planar = 1) aligned, any other pointer not 4-byte aligned; NULL w with IQ_EQ_GIVEN or in the backward.
 * IQ_STATUS_UNSUPPORTED: taps > 32, iters > 4096, len * 8 bytes above 64 KB.  n_frames <= 0: success, nothing is launched. */
enum { IQ_EQ_GIVEN = 0, IQ_EQ_CMA = 1 };
typedef struct iq_equaliser {
  int taps;       /* L in [1,32] */
  int iters;      /* CMA steps in [0,4096] */
  int planar;     /* 0: x,out [n,len,2]; 1: [n,2,len] */
  int mode;       /* IQ_EQ_* */
  float mu;       /* step size, >= 0 */
  float modulus;  /* R */
  const float* w;   /* DEVICE fp32 [n,L,2]: IQ_EQ_GIVEN and the backward */
  const float* w0;  /* DEVICE fp32 [n,L,2] or NULL (the unit spike at c): IQ_EQ_CMA */
} iq_equaliser_t;
int iq_frames_equalise(const float* x, float* out, float* w_out /*NULL or [n,L,2]*/, float* est /*NULL or [n,4]*/, int n_frames,
                       int len, const iq_equaliser_t* par, iq_stream_t stream);
int iq_frames_equalise_bwd(const float* dout, float* dx, int n_frames, int len, const iq_equaliser_t* par, iq_stream_t stream);
/* Tracking equaliser (csrc/equaliser_track.hip): the block CMA of iq_frames_equalise run per overlapping SEGMENT of the frame,
 * every segment from the same start, and a filter whose weights move over the frame, interpolated between the segments' centres.
 * It is for a channel that changes within a frame (iq_fading_t with a Doppler spread), which one filter per frame cannot follow.
 * Frames, layouts (planar 0 / 1), L = taps in [1, 32], c = L / 2, z = 0 outside [0, len) and the four-fmaf-per-tap filter chain
 * are those of iq_frames_equalise.
 *   Segments.  seg in [1, 512] outputs each, hop in [1, seg] apart; len >= seg.  S = (len - seg) / hop + 1 (integer division)
 *            segments, at most 256; segment j covers the outputs n = j hop + k, k = 0 .. seg-1.  (The outputs behind the last
 *            segment, fewer than hop, belong to no segment; they are filtered with the last segment's weights.)
 *   Taper.   h[k] = par->taper[k], DEVICE fp32 [seg], plain numbers shared by all frames and segments: the weight of output k
 *            of a segment in that segment's cost.  The caller normalises it (sum 1: a mean); nothing is divided by seg.
 *   IQ_EQT_CMA.  w_j^0 = par->w0[frame] (DEVICE fp32 [n_frames, L, 2]), or the unit spike at c when w0 is NULL: the same start for
 *            every segment of the frame.  For t = 0 .. iters-1, with y[k] = sum_l w_j^t[l] z[j hop + k + c - l] (the filter chain;
 *            the frame's samples outside the segment are read as they are):
 *              d    = (fmaf(Im y, Im y, Re y * Re y)) - R
 *              e[k] = ((Re y * d) * h[k], (Im y * d) * h[k])                 each product rounded
 *              G[l] = sum_k conj(z[j hop + k + c - l]) e[k]:  Re += Re z Re e, then Im z Im e;  Im += Re z Im e, then - Im z Re e,
 *                     all fmaf, as in iq_frames_equalise
 *              w_j^{t+1}[l] = fmaf(-mu, G[l], w_j^t[l]), the real and the imaginary word alike
 *            Every sum over k runs in one order: lane k % 64 its k ascending (a chain of fmaf from +0; at most 8 terms), then the
 *            wave's butterfly (xor 32, 16, 8, 4, 2, 1).  One wave owns one (frame, segment).
 *   Filter with weights over time.  For output n, t = n - seg / 2 (integer division): the offset from the first segment's centre.
 *            t <= 0: w(n) = w_0.  t >= (S - 1) hop: w(n) = w_{S-1}.  Otherwise j = t / hop, r = t % hop, a = (float)r / (float)hop and
 *            w(n)[l] = fmaf(a, w_{j+1}[l] - w_j[l], w_j[l]), every word alike (the difference rounded).  out[n] = sum_l w(n)[l]
 *            z[n + c - l], the filter chain.  Equal neighbours interpolate to themselves exactly (a * 0 + w), so with iters = 0 out
 *            has the bits of iq_frames_equalise under IQ_EQ_GIVEN with w = w0.
 *   IQ_EQT_GIVEN.  w_j = par->w[frame, j] (DEVICE fp32 [n_frames, S, L, 2]); only the filter runs.  iters, mu, w0 and taper are
 *            checked as below and not read otherwise; modulus is used by est[1].
 * Outputs: out; w_out: fp32 [n_frames, S, L, 2] = the segments' weights (GIVEN: a copy of w).  Under IQ_EQT_CMA w_out is REQUIRED:
 * the descent hands the weights to the filter through it, which is why no workspace is needed; under GIVEN it may be NULL.  est:
 * NULL or fp32 [n_frames, 4] = {J of the frame filtered by w0 alone (NaN when GIVEN), J(out), max_j D_j with D_j = sum_l
 * |w_j[l] - w0[l]|^2 (l ascending from +0, fmaf(dIm, dIm, fmaf(dRe, dRe, acc)), the differences rounded; the maximum walks j
 * ascending and takes D_j where D_j > the best so far, so a NaN is neither larger nor beaten; NaN when GIVEN), (float)S}.
 * J(y) = (sum_n d[n]^2) / (float)len over the whole frame, in the order of iq_frames_equalise (thread n % 256 ascending, fmaf(d, d,
 * acc), the wave's butterfly, ((s0 + s1) + s2) + s3).  NaNs are not special-cased: they propagate within their frame only.  No
 * atomics, no workspace, no allocation, no host synchronisation: two runs agree bit for bit and a frame's outputs depend on
 * neither n_frames nor its position.  Two launches under CMA (the descent: one wave per (frame, segment), four per workgroup, a
 * frame's segments neighbours in the grid, all iters steps inside the launch; then the filter: one workgroup per frame), one
 * under GIVEN.
 * iq_frames_equalise_track_bwd: the adjoint with the weights held fixed at par->w [n_frames, S, L, 2] (pass the forward's w_out)
 * whatever par->mode says, interpolated as in the forward: dx[m] = sum_l conj(w(n)[l]) dout[n], n = m - c + l, dout = 0 outside the
 * frame (w(n) for such an n is the first or the last segment's): a gather, per output one fmaf chain from +0 over l ascending,
 * Re: + Re d Re w then + Im d Im w, Im: + Im d Re w then - Re d Im w.  One workgroup per frame.
 * LDS: descent 4 x (two planes of 544 samples + 512 taper words) = 25.6 KB; filter and adjoint the frame as two planes with 32
 * zeros on either side, the S x L weights, w0 and the sums: at most 133.4 KB.
 * IQ_STATUS_ARG before any launch, outputs untouched: NULL x / out / dout / dx / par; taps < 1; len < 1; iters < 0; seg < 1;
 * hop < 1 or hop > seg; len < seg; mu or modulus not finite, mu < 0; planar outside {0,1}; mode outside IQ_EQT_*; x / out / dout /
 * dx not 8-byte (planar = 0) or 4-byte (planar = 1) aligned, any other pointer not 4-byte aligned; NULL w with IQ_EQT_GIVEN or in
 * the backward; NULL taper or NULL w_out with IQ_EQT_CMA.  IQ_STATUS_UNSUPPORTED: taps > 32, iters > 4096, seg > 512, len * 8 bytes
 * above 64 KB, more than 256 segments.  n_frames <= 0: success, nothing is launched. */
enum { IQ_EQT_GIVEN = 0, IQ_EQT_CMA = 1 };
typedef struct iq_equaliser_track {
  int taps;       /* L in [1,32] */
  int iters;      /* CMA steps per segment in [0,4096] */
  int planar;     /* 0: x,out [n,len,2]; 1: [n,2,len] */
  int mode;       /* IQ_EQT_* */
  int seg;        /* outputs per segment in [1,512] */
  int hop;        /* outputs between segment starts in [1,seg] */
  float mu;       /* step size, >= 0 */
  float modulus;  /* R */
  const float* w;      /* DEVICE fp32 [n,S,L,2]: IQ_EQT_GIVEN and the backward */
  const float* w0;     /* DEVICE fp32 [n,L,2] or NULL (the unit spike at c): IQ_EQT_CMA */
  const float* taper;  /* DEVICE fp32 [seg]: IQ_EQT_CMA */
} iq_equaliser_track_t;
int iq_frames_equalise_track(const float* x, float* out, float* w_out /*[n,S,L,2]; NULL allowed when GIVEN*/,
                             float* est /*NULL or [n,4]*/, int n_frames, int len, const iq_equaliser_track_t* par,
                             iq_stream_t stream);
int iq_frames_equalise_track_bwd(const float* dout, float* dx, int n_frames, int len, const iq_equaliser_track_t* par,
                                 iq_stream_t stream);
/* Likelihood classifier (csrc/likelihood.hip): the classical baseline of modulation classification.  For every frame and every
 * candidate constellation the log-likelihood of the frame's symbols as independent draws from the constellation in complex
 * Gaussian noise of known variance, over a table of carrier rotations (the phase is unknown), and the class of the largest.
 * x: fp32 frames of len symbols at one sample per symbol, planar = 0: [n_frames, len, 2], what the generators, the receiver and
 * the equaliser write; planar = 1: [n_frames, 2, len], what the carrier recovery writes; y[n] = I[n] + j Q[n].  sigma2[b]: the
 * noise variance E|w|^2 of frame b (both components together); gain[b]: the amplitude a of the constellation in the frame.
 * Classes are those of iq_synth_t with kind 0 only: class c has the M_c = count points s_k = points[offset + k].  rot[r] =
 * (c_r, s_r) is taken as two plain numbers (nothing is normalised).  All arithmetic is fp32, every operation rounded once, in
 * this order; fmaf is the fused multiply-add, exp2 / log2 the device's base-2 instructions (v_exp_f32, v_log_f32: 1 ulp).
 *   per frame      q = 1 / sigma2[b] (IEEE division);  q2 = q * LOG2E;  a = gain[b] (1 when gain is NULL);
 *                  p_k = (a * Re s_k, a * Im s_k);  1/M = 1 / (float)M_c (IEEE division)
 *   per rotation   y' = (fmaf(c_r, Re y, s_r * Im y), fmaf(c_r, Im y, -(s_r * Re y)))
 *   per symbol     d_k = fmaf(Im y' - Im p_k, Im y' - Im p_k, (Re y' - Re p_k) * (Re y' - Re p_k)): the difference form, which does
 *                  not cancel at high SNR as |y|^2 + |s|^2 - 2 Re(y conj s) does;  d_min = min_k d_k;
 *                  S = sum_k exp2(q2 * (d_min - d_k)), k ascending from +0;  l_n = fmaf(-q, d_min, LN2 * log2(S * (1/M)))
 *                  (= -q d_min + log((1/M) sum_k exp(-q (d_k - d_min))): with d_min taken out every term is finite and S >= 1,
 *                  so a wrong class at 30 dB does not underflow to log 0)
 *   L[b, c, r]     = sum_n l_n: lane n % 64 of a wave adds its symbols n ascending from +0, then the wave's butterfly
 *                  (xor 32, 16, 8, 4, 2, 1)
 *   loglik[b, c]   IQ_LIK_MAX (GLRT):  max_r L, best_rot the first r that attains it (r ascending; a NaN is never larger nor beaten)
 *                  IQ_LIK_MEAN (ALRT): m + LN2 * log2(T * (1 / (float)R)), m = max_r L, T = sum_r exp2(LOG2E * (L[r] - m)), r
 *                  ascending from +0: the log of the mean over the rotations
 *   pred[b]        the first c with the largest loglik[b, c] (c ascending)
 * The term -len log(pi sigma2), common to all classes, is LEFT OUT: loglik orders the classes of one frame and is not a density.
 * A sigma2[b] that is not a positive finite number is data, not an argument: that frame gets NaN in loglik and rot_ll and -1 in
 * best_rot and pred, and no other frame is touched.  Other NaNs are not special-cased: they stay within their frame.
 * Outputs: loglik fp32 [n_frames, C]; rot_ll: NULL or fp32 [n_frames, C, R] = L; best_rot: NULL or int32 [n_frames, C]; pred:
 * NULL or int32 [n_frames], written by a second small launch.  One workgroup per (frame, class) runs all R rotations: no atomics,
 * no workspace, two runs agree bit for bit and a frame's outputs depend on neither n_frames nor its position.  LDS 17 KB.
 * The backward with respect to x is iq_frames_likelihood_bwd (below); it reads loglik, rot_ll and best_rot as written here.
 * IQ_STATUS_ARG before any HIP call, outputs untouched: NULL x / sigma2 / loglik / par / points / classes / rot; len < 1; n_classes
 * or n_rot < 1; planar outside {0,1}; mode outside IQ_LIK_*; a class with kind != 0, count < 1, offset < 0 or offset + count past
 * the int range; x not 8-byte (planar = 0) or 4-byte (planar = 1) aligned, points not 8-byte, any other pointer not 4-byte aligned.
 * IQ_STATUS_UNSUPPORTED: C > 64, R > 256, a class that ends behind point 2048 of the table (the table's own size is not passed:
 * 2048 points, 16 KB of LDS, is the most a class may reach), len * 8 bytes above 64 KB (the frame kernels' limit), n_frames * C
 * above 2^31 - 1.  n_frames <= 0: success, nothing is launched. */
enum { IQ_LIK_MAX = 0, IQ_LIK_MEAN = 1 };
typedef struct iq_likelihood {
  const float* points;                 /* DEVICE fp32 (re, im) pairs, as iq_synth_t.points */
  const iq_synth_class_t* classes;     /* HOST array, copied into the launch; every kind must be 0 */
  int n_classes;                       /* C in [1, 64] */
  const float* rot;                    /* DEVICE fp32 [R, 2] = (cos, sin): plain numbers to the kernel */
  int n_rot;                           /* R in [1, 256] */
  int planar;                          /* 0: x [n, len, 2]; 1: [n, 2, len] */
  int mode;                            /* IQ_LIK_*: over the rotations, the maximum (GLRT) or the log of the mean (ALRT) */
  const float* gain;                   /* DEVICE fp32 [n] or NULL (= 1): amplitude a of the signal in the frame */
} iq_likelihood_t;
int iq_frames_likelihood(const float* x, const float* sigma2 /*[n]*/, float* loglik /*[n, C]*/,
                         float* rot_ll /*NULL or [n, C, R]*/, int* best_rot /*NULL or [n, C]*/,
                         int* pred /*NULL or [n]*/, int n_frames, int len,
                         const iq_likelihood_t* par, iq_stream_t stream);
/* Hybrid likelihood classifier (csrc/likelihood_em.hip): the likelihood test with nothing known.  For every frame and every
 * candidate constellation the maximum-likelihood complex gain h (amplitude and carrier phase together) and noise variance v, by
 * expectation-maximisation from a table of starts, the log-likelihood at them, and the class of the largest; |h|^2 / v of that
 * class is a blind SNR estimate.  x, planar, points and classes are those of iq_frames_likelihood; y_n = I[n] + j Q[n], s_k the M
 * points of the class.  All arithmetic is fp32, every operation rounded once, in this order; fmaf is the fused multiply-add,
 * exp2 / log2 the device's base-2 instructions (v_exp_f32, v_log_f32: 1 ulp), every '/' and sqrt is IEEE.  "Over the symbols"
 * means: lane n % 64 of ONE wave adds its symbols n ascending from +0, then the wave's butterfly (xor 32, 16, 8, 4, 2, 1).
 *   per class      ss_k = fmaf(Im s_k, Im s_k, Re s_k * Re s_k);  1/M = 1 / (float)M
 *   per frame      M2 = (over the symbols: fmaf(Im y, Im y, Re y * Re y)) / (float)len;  vfloor = floor * M2
 *   start t        IQ_EM_TABLE: v = f0 * M2;  a = sqrt(M2 - v);  h = (a * c_t, a * s_t) with starts[t] = (c_t, s_t), two plain numbers
 *                  IQ_EM_GIVEN: h = h0[b, c], v = v0[b, c], one start (T = 1; starts and n_starts are not looked at)
 *   a pass at (h, v)
 *                  q = 1 / v;  q2 = q * LOG2E;  p_k = (fmaf(Re s_k, Re h, -(Im s_k * Im h)), fmaf(Re s_k, Im h, Im s_k * Re h))
 *                  d_k = fmaf(Im y - Im p_k, Im y - Im p_k, (Re y - Re p_k) * (Re y - Re p_k));  d_min = min_k d_k
 *                  e_k = exp2(q2 * (d_min - d_k));  S = sum_k e_k, k ascending from +0
 *   an update pass (iters of them) also forms, k ascending from +0,
 *                  Wr = fmaf(e_k, Re s_k, Wr), Wi = fmaf(e_k, Im s_k, Wi), Bn = fmaf(e_k, ss_k, Bn), Vn = fmaf(e_k, d_k, Vn);
 *                  r = 1 / S (once per symbol);  gr = Wr * r;  gi = Wi * r;  and over the symbols
 *                  Ar = fmaf(Im y, gi, fmaf(Re y, gr, Ar));  Ai = fmaf(-Re y, gi, fmaf(Im y, gr, Ai));  Bq = fmaf(Bn, r, Bq);
 *                  V = fmaf(Vn, r, V);   then  h' = (Ar / Bq, Ai / Bq);  t = V / (float)len;  v' = t < vfloor ? vfloor : t
 *                  (the variance from the distances of the pass that formed the responsibilities: an ECM step, which never
 *                  lowers the likelihood, costs no second pass and does not cancel at high SNR)
 *   the last pass  l_n = fmaf(-q, d_min, LN2 * log2(S * (1/M)));  L = over the symbols l_n;
 *                  Lambda = fmaf(-(float)len, LN2 * (LOG2PI + log2(v)), L)  (= L - len ln(pi v): v differs between the classes)
 * A start whose state, at the start or after an update, is not (h finite, 2^-126 <= v < inf) is DEAD: its Lambda is NaN and it
 * makes no further pass (a subnormal v counts as no variance: the base-2 logarithm and the division take it for zero).  Over the starts, t ascending, NaNs passed over: the first start with the largest Lambda wins; loglik[b, c] is its
 * Lambda, (h, v)[b, c] its state after the updates, best_start[b, c] = t.  Where every start's Lambda is NaN (a class of the origin
 * alone with iters > 0: Bq = 0; a NaN sample; an all-zero frame: M2 = 0) loglik, h and v are NaN and best_start -1: these are data,
 * never argument errors, and no other (frame, class) is touched.  pred[b] = the first class with the largest loglik[b, c], c
 * ascending, NaN classes PASSED OVER (one impossible class does not cost the frame its decision); -1 where every class is NaN.
 * snr_db[b] = TEN_LOG10_2 * log2(fmaf(Im h, Im h, Re h * Re h) / v) of class pred[b]; NaN where pred is -1.
 * Outputs: loglik fp32 [n_frames, C]; each other NULL or written: h fp32 [n_frames, C, 2], v fp32 [n_frames, C], best_start
 * int32 [n_frames, C], start_ll fp32 [n_frames, C, T] (every start's Lambda), pred int32 [n_frames] and snr_db fp32 [n_frames],
 * the last two by a second small launch; snr_db reads h and v, which must then be given.  One workgroup per (frame, class),
 * classes going out largest first; wave w of four runs the starts t = w, w + 4, ... each through all its passes on its own (no
 * barrier inside the iteration), the frame and the points in LDS: no atomics, no workspace, two runs agree bit for bit and a
 * frame's outputs depend on neither n_frames nor its position.  LDS: 28 KB + len * 8 + 4 * M * 8 bytes.  The backward with
 * respect to x at the estimate held fixed is iq_frames_likelihood_em_bwd (below); it reads h and v as written here.
 * IQ_STATUS_ARG before any HIP call, outputs untouched: NULL x / loglik / par / points / classes; mode outside IQ_EM_*; NULL starts
 * or n_starts < 1 (IQ_EM_TABLE); NULL h0 or v0 (IQ_EM_GIVEN); snr_db without h and v; len < 1; n_classes < 1; iters < 0; planar
 * outside {0,1}; f0 not inside (0, 1) or floor not a finite number >= 0; a class with kind != 0, count < 1, offset < 0 or offset +
 * count past the int range; x not 8-byte (planar = 0) or 4-byte (planar = 1) aligned, points, h0 and h not 8-byte, any other
 * pointer not 4-byte aligned.  IQ_STATUS_UNSUPPORTED: C > 64, T > 256, iters > 4096, a class that ends behind point 2048 of the
 * table, len * 8 bytes above 64 KB, n_frames * C above 2^31 - 1.  n_frames <= 0: success, nothing is launched. */
enum { IQ_EM_TABLE = 0, IQ_EM_GIVEN = 1 };
typedef struct iq_likelihood_em {
  const float* points;                 /* DEVICE fp32 (re, im) pairs, as iq_likelihood_t.points */
  const iq_synth_class_t* classes;     /* HOST array, copied into the launch; every kind must be 0 */
  int n_classes;                       /* C in [1, 64] */
  const float* starts;                 /* DEVICE fp32 [T, 2] = (cos, sin) of the starting phases: plain numbers to the kernel */
  int n_starts;                        /* T in [1, 256] (IQ_EM_TABLE) */
  int iters;                           /* updates per start in [0, 4096]; iters + 1 passes */
  int planar;                          /* 0: x [n, len, 2]; 1: [n, 2, len] */
  int mode;                            /* IQ_EM_* */
  float f0;                            /* share of the frame's power the starting variance takes, in (0, 1) */
  float floor;                         /* the variance never falls below floor * M2; >= 0 */
  const float* h0;                     /* DEVICE fp32 [n, C, 2]: IQ_EM_GIVEN */
  const float* v0;                     /* DEVICE fp32 [n, C]: IQ_EM_GIVEN */
} iq_likelihood_em_t;
int iq_frames_likelihood_em(const float* x, float* loglik /*[n, C]*/, float* h /*NULL or [n, C, 2]*/, float* v /*NULL or [n, C]*/,
                            int* best_start /*NULL or [n, C]*/, float* start_ll /*NULL or [n, C, T]*/, int* pred /*NULL or [n]*/,
                            float* snr_db /*NULL or [n]*/, int n_frames, int len, const iq_likelihood_em_t* par,
                            iq_stream_t stream);
/* Gradients of the two likelihood classifiers with respect to the frame (csrc/likelihood_bwd.hip): given dloglik[b, c], the
 * gradient of a scalar with respect to loglik, dx[b, n] = d(sum_c dloglik[b, c] loglik[b, c]) / d(Re y_n, Im y_n) with everything
 * else held fixed: sigma2, gain, the points and the rotation table, the winning rotation (IQ_LIK_MAX: the true gradient wherever
 * the maximum is unique) and the EM estimate (h, v) (at a converged interior EM point also the total derivative: the estimate
 * maximises the likelihood it is put into).  It is the soft symbol decision: for one hypothesis of one class
 * d l_n / d(Re y, Im y) = -2 q (y - m), m = sum_k e_k p_k / S with e_k and S the forward's.  x, planar, points, classes, rot and
 * gain are the forward's, dx has x's layout.  All arithmetic is fp32, every operation rounded once, in this order; '/' is IEEE.
 *   dx[b, n]       = the sum, from +0, over c ascending and within a class over t ascending, of the terms below; a (class,
 *                  hypothesis) whose weight w is exactly 0 is SKIPPED, and so is a whole class whose dloglik[b, c] is exactly 0
 *                  before anything of it is read: a one-class gradient or the {-1, +1} of a margin loss costs the classes it
 *                  touches, and a NaN in the results of a class nobody asked about stays out of dx
 * iq_frames_likelihood_bwd, with q, q2, a, p_k, 1/M, y', d_k, d_min exactly as iq_frames_likelihood forms them:
 *   hypotheses     IQ_LIK_MAX: t = best_rot[b, c] alone, w = dloglik[b, c] (a best_rot outside [0, R) with a nonzero dloglik:
 *                  NaN in dx[b], nothing is read through it);  IQ_LIK_MEAN: every r,
 *                  w = (dloglik[b, c] * exp2(LOG2E * (rot_ll[b, c, r] - loglik[b, c]))) * (1 / (float)R): the rotation's share
 *                  (no reduction: loglik is the log of the mean already)
 *   per symbol     e_k = exp2(q2 * (d_min - d_k));  S = S + e_k, Wr = fmaf(e_k, Re p_k, Wr), Wi = fmaf(e_k, Im p_k, Wi), k ascending
 *                  from +0;  r = 1 / S;  m = (Wr * r, Wi * r);  wq = w * (-2 * q);  g = (wq * (Re y' - Re m), wq * (Im y' - Im m))
 *   back to y      t = (fmaf(Re g, c_r, -(Im g * s_r)), fmaf(Re g, s_r, Im g * c_r));  dx = (Re dx + Re t, Im dx + Im t)
 * iq_frames_likelihood_em_bwd, one hypothesis (h, v)[b, c] per class, with q, q2, p_k, d_k, d_min, e_k, S as a pass of
 * iq_frames_likelihood_em forms them at that state:
 *   per symbol     Wr, Wi, r and m as above;  wq = dloglik[b, c] * (-2 * q);
 *                  dx = (fmaf(wq, Re y - Re m, Re dx), fmaf(wq, Im y - Im m, Im dx))
 * The term -len log(pi v) does not depend on y.  Data, not arguments: a frame whose sigma2 the forward refuses gets NaN in all of
 * its dx; a (frame, class) with a nonzero dloglik whose state is not (h finite, 2^-126 <= v < inf) -- the forward's NaN -- gets NaN
 * in all of its frame's dx; nothing else is touched, and other NaNs stay within their symbol.  iq_frames_likelihood_em_bwd reads
 * points, classes, n_classes and planar of its struct and IGNORES starts, n_starts, iters, mode, f0, floor, h0 and v0.
 * One workgroup per (frame, 512 symbols), a lane two symbols with their dx in registers over all classes and hypotheses: no
 * cross-lane reduction, no atomics, no workspace; two runs agree bit for bit and a symbol's dx depends on neither n_frames nor
 * the frame's position.  LDS 16 KB.  One launch each.
 * IQ_STATUS_ARG before any HIP call, dx untouched: NULL x / dloglik / dx / par / points / classes, NULL sigma2 / rot (likelihood),
 * NULL h / v (EM); NULL best_rot in IQ_LIK_MAX; NULL loglik or rot_ll in IQ_LIK_MEAN; len < 1; n_classes < 1; n_rot < 1, mode
 * outside IQ_LIK_* (likelihood); planar outside {0,1}; a class with kind != 0, count < 1, offset < 0 or offset + count past the int
 * range; x or dx not 8-byte (planar = 0) or 4-byte (planar = 1) aligned, points and h not 8-byte, any other pointer not 4-byte
 * aligned.  IQ_STATUS_UNSUPPORTED: C > 64, R > 256, a class that ends behind point 2048 of the table, len * 8 bytes above 64 KB,
 * n_frames * ceil(len / 512) above 2^31 - 1.  n_frames <= 0: success, nothing is launched. */
int iq_frames_likelihood_bwd(const float* x, const float* sigma2 /*[n]*/, const float* dloglik /*[n, C]*/,
                             const float* loglik /*[n, C]: IQ_LIK_MEAN*/, const float* rot_ll /*[n, C, R]: IQ_LIK_MEAN*/,
                             const int* best_rot /*[n, C]: IQ_LIK_MAX*/, float* dx /*x's layout*/, int n_frames, int len,
                             const iq_likelihood_t* par, iq_stream_t stream);
int iq_frames_likelihood_em_bwd(const float* x, const float* dloglik /*[n, C]*/, const float* h /*[n, C, 2]*/,
                                const float* v /*[n, C]*/, float* dx /*x's layout*/, int n_frames, int len,
                                const iq_likelihood_em_t* par, iq_stream_t stream);
/* Cumulant classifier (csrc/cumulants.hip): the feature-based baseline of modulation classification beside the likelihood test
 * (higher-order cumulants in the style of Swami & Sadler).  For every frame the mean, the central moments and the cumulants up to
 * order eight, ten features that no carrier rotation changes, and the weighted distance of the features to every class's
 * centroid.  O(len) per frame; Gaussian noise leaves every cumulant above order two in expectation, so sigma2 may be left out.
 * x: fp32 frames of len symbols at one sample per symbol, planar = 0: [n_frames, len, 2]; planar = 1: [n_frames, 2, len];
 * y[n] = I[n] + j Q[n].  With z = y - m and M_pq = mean(z^(p-q) conj(z)^q), all arithmetic fp32, every operation rounded once,
 * in this order (fmaf is the fused multiply-add; (a, b) is a complex number by its parts; nothing else is fused):
 *   sums           the symbols of a lane ascending from +0; then the wave's butterfly (xor 32, 16, 8, 4, 2, 1); then, on the
 *                  workgroup route, the four waves ((w0 + w1) + w2) + w3.  len <= 256 (the wave route): lane l of one wave has
 *                  the symbols l, l + 64, ...; len > 256 (the workgroup route): thread t of 256 has t, t + 256, ...
 *   m              = (sum Re y / (float)len, sum Im y / (float)len)  (IEEE division), the frame read once and kept in LDS
 *   per symbol     z = (a, b) = (Re y - Re m, Im y - Im m);  sq(u) = (fmaf(u.re, u.re, -(u.im * u.im)), (u.re + u.re) * u.im);
 *                  u v = (fmaf(u.re, v.re, -(u.im * v.im)), fmaf(u.re, v.im, u.im * v.re));  |u|^2 = fmaf(u.im, u.im, u.re * u.re);
 *                  z2 = sq(z), z4 = sq(z2), z6 = z4 z2, z8 = sq(z4), r = |z|^2, r2 = r * r, and the 17 terms
 *                  z2 | r | z4 | z2 * r | r2 | z6 | z4 * r | z2 * r2 | r2 * r | z8
 *   moments        each sum / (float)len:  M20 | M21 | M40 | M41 | M42 | M60 | M61 | M62 | M63 | M80  (M21, M42, M63 real)
 *   cumulants      of the pair (z, conj z), by the moment-to-cumulant partition formula; s u + v below is (fmaf(s, u.re, v.re),
 *                  fmaf(s, u.im, v.im)), q = sq(M20), n = |M20|^2, conj(u) v = (fmaf(u.re, v.re, u.im * v.im), fmaf(u.re, v.im, -(u.im * v.re)))
 *                  C20 = M20;  C21 = M21;  C40 = -3 q + M40;  C41 = -(3 * M21) M20 + M41;
 *                  C42 = fmaf(-(M21 + M21), M21, M42 - n)
 *                  C60 = 30 (q M20) + (-15 (M20 M40) + M60)
 *                  C61 = (30 * M21) q + (-10 (M20 M41) + (-(5 * M21) M40 + M61))
 *                  C62 = g M20 + ((-(8 * M21) M41 + (-(6 * M42) M20 + M62)) - conj(M20) M40),  g = fmaf(24 * M21, M21, 6 * n)
 *                  C63 = fmaf(18 * n, M21, fmaf(-6, h, fmaf(12 * (M21 * M21), M21, fmaf(-(9 * M21), M42, M63)))),
 *                        h = fmaf(Re M20, Re M41, Im M20 * Im M41)
 *                  C80 = -630 sq(q) + (420 (q M40) + (-35 sq(M40) + (-28 (M20 M60) + M80)))
 *   P              = C21 - sigma2[b] (sigma2 NULL: - 0): the signal's variance.  P2 = P * P, P3 = P2 * P, P4 = P3 * P
 *   feat[b, 0..9]  |m|^2 / P | |C20| / P | |C40| / P2 | |C41| / P2 | C42 / P2 | |C60| / P3 | |C61| / P3 | |C62| / P3 | C63 / P3 |
 *                  |C80| / P4,  |u| = sqrt(|u|^2) (IEEE square root and division)
 *   score[b, c]    = bias[c] - acc (bias NULL: 0 - acc),  acc from +0, f ascending: d = feat[f] - mu[c, f];
 *                  acc = fmaf(w[c, f] * d, d, acc)
 *   pred[b]        the first c with the largest score[b, c] (c ascending; a NaN is never larger nor ever beaten)
 * mom[b, 0..19] = Re m, Im m, then the moments in the order above (complex ones as re, im), then P.
 * P is data, not an argument: a frame whose P is not a positive finite number (an all-zero frame, len = 1, a sigma2 at or above
 * the frame's variance, a NaN sample) gets NaN in every feature and every score and -1 in pred; mom is written as computed; no
 * other frame is touched.
 * Outputs, each NULL or: feat fp32 [n_frames, 10]; mom fp32 [n_frames, 20]; score fp32 [n_frames, C]; pred int32 [n_frames].  One
 * launch.  No atomics, no workspace, two runs agree bit for bit and a frame's outputs depend on neither n_frames nor its
 * position.  LDS: the frame, len * 8 bytes (four frames on the wave route), and 304 bytes.  The backward with respect to x is
 * iq_frames_cumulants_bwd (below); it reads none of these outputs.
 * IQ_STATUS_ARG before any HIP call, outputs untouched: NULL x / par; all four outputs NULL; len < 1; planar outside {0,1};
 * n_classes < 0; n_classes > 0 with NULL mu or w; score or pred with n_classes == 0; x not 8-byte (planar = 0) or 4-byte
 * (planar = 1) aligned, any other pointer not 4-byte aligned.
 * IQ_STATUS_UNSUPPORTED: C > 64, len * 8 bytes above 64 KB (the frame kernels' limit), n_frames * max(C, 20) above 2^31 - 1.
 * n_frames <= 0: success, nothing is launched. */
typedef struct iq_cumulants {
  int planar;            /* 0: x [n, len, 2]; 1: [n, 2, len] */
  const float* sigma2;   /* DEVICE fp32 [n] or NULL (= 0: blind) */
  const float* mu;       /* DEVICE fp32 [C, 10]; NULL iff n_classes == 0 */
  const float* w;        /* DEVICE fp32 [C, 10] */
  const float* bias;     /* DEVICE fp32 [C] or NULL (= 0) */
  int n_classes;         /* C in [0, 64]; 0: features only */
} iq_cumulants_t;
int iq_frames_cumulants(const float* x, float* feat /*NULL or [n,10]*/, float* mom /*NULL or [n,20]*/,
                        float* score /*NULL or [n,C]*/, int* pred /*NULL or [n]*/,
                        int n_frames, int len, const iq_cumulants_t* par, iq_stream_t stream);
/* Gradient of the cumulant classifier with respect to the frame (csrc/cumulants_bwd.hip): dx[b, n] = dL / d(Re y_n, Im y_n) of
 * L = sum_c dscore[b, c] score[b, c] + sum_f dfeat[b, f] feat[b, f], with sigma2, mu, w and bias held fixed and NOTHING else: the
 * true gradient, through the mean and through P.  x, planar, sigma2, mu, w and n_classes are the forward's (bias is not read), dx
 * has x's layout; dscore NULL: the classes are not looked at; dfeat NULL: 0.  Self-contained: m, the moments, the cumulants, P,
 * P2, P3, P4 and feat are formed again from the frame exactly as iq_frames_cumulants forms them, bit for bit; no forward output is
 * read.  A complex gradient is G = dL/dRe + j dL/dIm.  Beside the forward's notation: s u is (s * u.re, s * u.im),
 * u + v the two sums, u / s the two IEEE divisions, <u, v> = fmaf(u.re, v.re, u.im * v.im) = Re(conj(u) v); all fp32, every
 * operation rounded once, in this order:
 *   gf[0..9]       = dfeat[b, f] (NULL: +0); then for c ascending, a class whose dscore[b, c] is exactly 0 SKIPPED before anything
 *                  of it is read (a NaN row of mu of a class nobody asked about stays out):
 *                  gf[f] = fmaf((-2 * dscore[b, c]) * w[c, f], feat[f] - mu[c, f], gf[f])
 *   gP             = -(acc / P), acc from +0, f ascending: acc = fmaf(k_f * feat[f], gf[f], acc), k = 1 1 2 2 2 3 3 3 3 4
 *   gm             = ((gf[0] + gf[0]) / P) m
 *   mag(g, C, Pk)  = (g / (|C| * Pk)) C, and (0, 0) where |C| is exactly 0 (the subgradient; |C| as the forward rounds it)
 *                  gC20 = mag(gf[1], M20, P); gC40 = mag(gf[2], C40, P2); gC41 = mag(gf[3], C41, P2); gC42 = gf[4] / P2;
 *                  gC60 = mag(gf[5], C60, P3); gC61 = mag(gf[6], C61, P3); gC62 = mag(gf[7], C62, P3); gC63 = gf[8] / P3;
 *                  gC80 = mag(gf[9], C80, P4)
 *   moments        the chain rule on the closed forms above, each line left to right; a term s u + acc is the forward's fused pair
 *                  G60 = -28 (conj(M20) gC80) + gC60
 *                  G42 = fmaf(-(9 * M21), gC63, fmaf(-6, <gC62, M20>, gC42))
 *                  G41 = (-6 * gC63) M20 + (-(8 * M21) gC62 + (-10 (conj(M20) gC61) + gC41))
 *                  G40 = (-1 (M20 gC62) + (-(5 * M21) gC61 + (-15 (conj(M20) gC60) + gC40))) + conj(420 q + (-70 M40)) gC80
 *                  G21 = fmaf(-(4 * M21), gC42, fmaf(-3, <gC41, M20>, gP));  G21 = G21 + <gC61, 30 q + (-5 M40)>;
 *                        G21 = G21 + <gC62, (48 * M21) M20 + (-8 M41)>;
 *                        G21 = fmaf(gC63, fmaf(18, n, fmaf(36 * M21, M21, -9 * M42)), G21)
 *                  G20 = -(gC42 + gC42) M20 + (-(3 * M21) gC41 + (-6 (conj(M20) gC40) + gC20));
 *                        G20 = G20 + conj(90 q + (-15 M40)) gC60;  G20 = G20 + conj((60 * M21) M20 + (-10 M41)) gC61;
 *                        G20 = fmaf(24 * M21, M21, fmaf(12, n, -6 * M42)) gC62 + G20;  G20 = G20 + conj(gC62) (6 q + (-M40));
 *                        G20 = gC63 ((36 * M21) M20 + (-6 M41)) + G20;
 *                        G20 = G20 + conj(-2520 (q M20) + (840 (M20 M40) + (-28 M60))) gC80
 *                  G61 = gC61, G62 = gC62, G63 = gC63, G80 = gC80
 *   coefficients   H = G / (float)len;  A20 = 2 H20, A21 = 2 * H21, A40 = 4 H40, A41 = 3 H41, B41 = conj(H41), A42 = 4 * H42,
 *                  A60 = 6 H60, A61 = 5 H61, B61 = conj(H61), A62 = 4 H62, B62 = conj(2 H62), A63 = 6 * H63, A80 = 8 H80
 *   per symbol     z, z2, z4, r, r2 as the forward; z3 = z2 z, z5 = z4 z, z7 = z4 z3;
 *                  k1 = r2 A62 + (r A41 + A20);  kz = fmaf(r2, A63, fmaf(r, A42, A21));  k3 = r A61 + A40;  k3b = r B62 + B41;
 *                  g = conj(z) k1;  g = kz z + g;  then g = g + t for t = conj(z3) k3 | z3 k3b | conj(z5) A60 | z5 B61 | conj(z7) A80
 *   sum g          in the forward's order of sums (the lane's symbols ascending from +0, the butterfly, the four waves)
 *   dx[b, n]       = g_n + (gm / (float)len - sum g / (float)len), each part
 * Data, not arguments: a frame whose P the forward refuses gets NaN in all of its dx; no other frame is touched.
 * One launch, the forward's two routes by the length alone; a thread touches only the LDS slots it wrote.  No atomics, no
 * workspace; two runs agree bit for bit and a frame's dx depends on neither n_frames nor its position.  LDS: the frame, len * 8
 * bytes (four frames on the wave route), and 336 bytes.
 * IQ_STATUS_ARG before any HIP call, dx untouched: NULL x / dx / par; dscore and dfeat both NULL; len < 1; planar outside {0,1};
 * n_classes < 0; n_classes > 0 with NULL mu or w; dscore with n_classes == 0; x or dx not 8-byte (planar = 0) or 4-byte
 * (planar = 1) aligned, any other pointer not 4-byte aligned.
 * IQ_STATUS_UNSUPPORTED: C > 64, len * 8 bytes above 64 KB, n_frames * max(C, 20) above 2^31 - 1.  n_frames <= 0: success, nothing
 * is launched. */
int iq_frames_cumulants_bwd(const float* x, const float* dscore /*NULL or [n, C]*/, const float* dfeat /*NULL or [n, 10]*/,
                            float* dx /*x's layout*/, int n_frames, int len, const iq_cumulants_t* par, iq_stream_t stream);
int iq_patchify(const float* src, void* patches, int kind, int B, int C, int H, int W, int p, int Kpad,
                iq_stream_t stream);
int iq_cls_rows(const float* cls, const float* pe, void* x0, int B, int S, int D, const iq_dropout_t* drop,
                iq_stream_t stream);
int iq_embed_bwd_gather(const void* dx0, void* demb, float* dcls, int B, int S, int tok, int D, int has_cls,
                        const iq_dropout_t* drop, int accumulate, iq_stream_t stream);
/* Data gradient of the embedding: dsrc = unpatchify(demb . W), the inverse of iq_patchify's layout.  demb bf16 [B*tok, D],
 * w_bf16 bf16 [D, Kpad] (the padded weight, columns >= P ignored; both 16 B aligned), dsrc fp32 in the input's layout
 * (kind 0: (B,C,H,W), p x p patches; kind 1: (B,C,L) with L in H, segments of p).  Every element of dsrc is written: input
 * elements no patch covers (H % p, W % p, L % p) get 0.  Deterministic (no atomics).  IQ_ERR_ARG before any launch for NULL
 * pointers, a bad kind, D % 8, Kpad % 8 or Kpad < P. */
int iq_embed_dgrad(const void* demb, const void* w_bf16, int Kpad, float* dsrc, int kind, int B, int C, int H, int W, int p,
                   int D, iq_stream_t stream);
/* One L-infinity attack step over n fp32 elements: x_adv <- clamp(clamp(x_adv + alpha*sign(grad), x0-eps, x0+eps), lo, hi),
 * sign(0) = 0; lo / hi = NaN means no bound.  alpha, eps >= 0 and finite, lo <= hi. */
int iq_linf_step(float* x_adv, const float* grad, const float* x0, float alpha, float eps, float lo, float hi, size_t n,
                 iq_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Classification head + loss.
 * iq_head_fwd: feat = x[:,0,:] (pool=0) or mean over tokens (pool=1); optional LayerNorm (eps 1e-5,
 * R/models/transformer_rawIQ.py:67-70,88-96); logits = feat*W^T + b (V/models/amc_transformer.py:29-30).
 * featn [B,D] fp32 (the pooled feature, normalised but pre-affine when LN is on) and hstat [B,2]
 * (mean, rstd) are kept for backward.
 * iq_ce_fwd_bwd: CrossEntropyLoss(label_smoothing) mean over `denom` frames (global batch under DDP); a label
 * outside [0, K) makes that frame's loss and gradient NaN (torch asserts on the device),
 * V/training/train.py:405; writes loss_sum (sum over local frames of per-frame loss), n_correct
 * (argmax==label, V/training/train.py:205-207) and dlogits.  Pass dlogits NULL to skip the gradient.
 * iq_head_bwd: gradients of W,b,(ln gamma,beta) and d(x_L) (bf16 [B*S,D], zero outside the pooled rows). */
int iq_head_fwd(const void* x, const float* ln_g, const float* ln_b, const float* W, const float* b, float* featn,
                float* hstat, float* logits, int B, int S, int D, int K, int pool, iq_stream_t stream);
int iq_ce_fwd_bwd(const float* logits, const int64_t* labels, int B, int K, float smoothing, float denom,
                  float* loss_sum, int32_t* n_correct, float* dlogits, iq_stream_t stream);
int iq_head_bwd(const float* dlogits, const float* featn, const float* hstat, const float* ln_g, const float* ln_b,
                const float* W, float* dW, float* db, float* dln_g, float* dln_b, void* dx, int B, int S, int D, int K,
                int pool, int accumulate, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Optimizer on the flat fp32 parameter / gradient buffers.
 * iq_gradnorm_sq: out[0] = sum(g^2)  (clip_grad_norm_, V/training/train.py:199).
 * iq_adamw_step: clip scale min(1, max_norm/(sqrt(gnorm_sq)+1e-6)) folded into AdamW with decoupled
 * weight decay on every element (V/training/train.py:407-412); also writes the bf16 shadow.
 * max_norm <= 0 or gnorm_sq NULL disables clipping.  grad_scale multiplies g first (1/world_size). */
size_t iq_gradnorm_ws_bytes(size_t n);
int iq_gradnorm_sq(const float* g, size_t n, float grad_scale, float* ws, float* out, iq_stream_t stream);
int iq_adamw_step(float* p, const float* g, float* m, float* v, void* shadow_bf16, size_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, const float* gnorm_sq, float max_norm,
                  float grad_scale, const float* dyn, iq_stream_t stream);
/* dyn: optional DEVICE float[2] = {lr, step}; when non-NULL it overrides lr/step (graph replay).
 * iq_counter_add: *ctr_u32 += inc_u32 and/or *ctr_f32 += inc_f32 (either pointer may be NULL). */
int iq_counter_add(uint32_t* ctr_u32, uint32_t inc_u32, float* ctr_f32, float inc_f32, iq_stream_t stream);
int iq_cast_bf16(const float* src, void* dst, size_t n, iq_stream_t stream);
/* dst[c, r] (ld = rows_pad) = bf16(src[r, c]); src fp32 [rows, cols] */
int iq_transpose_cast_bf16(const float* src, void* dst, int rows, int cols, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Whole-model plan: the native runtime underneath AMCTransformer.forward / loss.backward().
 * Mirrors the constructors V/models/amc_transformer.py:9 and R/models/transformer_rawIQ.py:14-26. */
typedef struct iq_model_cfg {
  int kind;            /* 0 = ViT (2-D patches), 1 = raw-IQ (1-D sequence) */
  int in_channels;
  int img_h, img_w, patch;            /* kind 0 */
  int seq_length, conv_k, use_cls;    /* kind 1: conv_k = segment_size, or 1 for embedding_type 'conv1d' */
  int num_classes, d_model, n_head, n_layers, ffn_hidden;
  float drop_prob;
} iq_model_cfg_t;

typedef struct iq_model iq_model_t;

int iq_model_create(const iq_model_cfg_t* cfg, iq_model_t** out);
void iq_model_destroy(iq_model_t* m);
const char* iq_model_last_error(const iq_model_t* m);
int iq_model_tokens(const iq_model_t* m);   /* S, cls included */
/* flat fp32 parameter buffer layout: entries in reference state_dict naming */
size_t iq_model_param_floats(const iq_model_t* m);
int iq_model_param_entries(const iq_model_t* m);
int iq_model_param_entry(const iq_model_t* m, int i, char* name, int name_cap, size_t* offset, int* ndim, int* dims);
size_t iq_model_shadow_bytes(const iq_model_t* m);
size_t iq_model_workspace_bytes(const iq_model_t* m, int batch, int training);
/* bind device buffers (caller-owned, must outlive use): params/grads flat fp32, pe fp32 [S,D], shadow bytes */
int iq_model_bind(iq_model_t* m, float* params, float* grads, const float* pe, void* shadow);
/* Optional: a caller-owned persistent DEVICE u32 that holds the dropout step.  When bound, iq_model_forward with
 * step == 0xFFFFFFFF increments it on the device (hipGraph replays then draw fresh masks), any other step value is
 * written into it; backward regenerates masks from it.  Unbound, a slot of the workspace is used (uninitialised
 * after every workspace reallocation: bind a counter for reproducible masks under graph replay). */
int iq_model_bind_step_counter(iq_model_t* m, uint32_t* counter);
int iq_model_refresh_shadow(iq_model_t* m, iq_stream_t stream);
/* same, minus the flat fp32->bf16 mirror (iq_adamw_step has just written it) */
int iq_model_refresh_transposed(iq_model_t* m, iq_stream_t stream);
/* forward: src fp32 (B,C,H,W)/(B,C,L); enc_out fp32 [B,S,D] or NULL; logits fp32 [B,K] or NULL */
int iq_model_forward(iq_model_t* m, const float* src, int batch, void* workspace, size_t ws_bytes, int training,
                     uint64_t seed, uint32_t step, float* enc_out, float* logits, iq_stream_t stream);
/* backward of the last training forward in `workspace`: dlogits fp32 [B,K] and/or denc fp32 [B,S,D].
 * Gradients are WRITTEN (accumulate=0) or added into the bound flat grad buffer.
 * layer_hi/layer_lo select a slice of the chain for comm overlap: stage ids run
 * n_layers+1 (head) ... 1 (layer 0) ... 0 (embedding); call with (n_layers+1, 0) for everything. */
int iq_model_backward(iq_model_t* m, const float* dlogits, const float* denc, int batch, void* workspace,
                      size_t ws_bytes, int accumulate, int stage_hi, int stage_lo, iq_stream_t stream);
/* Gradient exchange: SURVEY.md 8(b) lists iq_comm_{init, allreduce_bucket, finalize} among the entry points.  They are
 * deliberately NOT part of this library: BASELINE.json's north_star keeps the host in PyTorch-ROCm, whose
 * torch.distributed (backend "nccl" = RCCL over xGMI) already owns communicators, streams and the process group.  The C
 * ABI ends at "this contiguous range of the flat gradient is complete on the stream" (iq_model_backward by stages +
 * iq_model_grad_range below); vit-vs-raw-iq_amd/trainer.py issues one asynchronous all-reduce per range. */
/* flat-gradient range [*off, *off+*len) written by stages [stage_lo, stage_hi] (DDP buckets) */
int iq_model_grad_range(const iq_model_t* m, int stage_hi, int stage_lo, size_t* off, size_t* len);
/* Gradient with respect to the model input of the last forward in `workspace` (same batch; refused otherwise, as
 * iq_model_attention): the whole chain from dlogits [B,K] and/or denc [B,S,D] down to the embedding, then
 * iq_embed_dgrad.  dsrc fp32 in the input's layout is WRITTEN.  Without IQ_BWD_PARAM_GRADS no parameter gradient is formed
 * and the plan may be bound without a gradient buffer; with it the flat gradient is written exactly as
 * iq_model_backward(accumulate=0, n_layers+1, 0) writes it.  dsrc does not depend on the flag. */
#define IQ_BWD_PARAM_GRADS 1
int iq_model_backward_input(iq_model_t* m, const float* dlogits, const float* denc, int batch, void* workspace,
                            size_t ws_bytes, float* dsrc, int flags, iq_stream_t stream);
/* Attention read-back after iq_model_forward(..., batch, workspace): layer `layer`'s attention probabilities from that forward
 * (see iq_attn_probs for rows / heads / out) -- the per-layer `score` of ScaleDotProductAttention.forward
 * (V/models/layers/scale_dot_product_attention.py:25-39) that MultiHeadAttention.forward drops
 * (V/models/layers/multi_head_attention.py:24,30; the raw-IQ tree's layers are the same files).
 * Refused (iq_model_last_error) when no forward has run, when the last forward ran in another workspace or with another
 * batch, for a layer outside [0, n_layers), bad rows / heads, a too-small workspace or out_bstride.  A forward replayed from
 * a captured graph is not seen by the host: run a forward through this call before reading back. */
int iq_model_attention(iq_model_t* m, const void* workspace, size_t ws_bytes, int batch, int layer, int rows,
                       int heads, float* out, long out_bstride, iq_stream_t stream);
/* Attention rollout (Abnar & Zuidema 2020) of that forward, over the same per-layer matrices as above:
 * r <- start; for l = L-1 .. 0: r <- r (alpha * mean_h P_l + (1-alpha) I).  start = e_0 (CLS) when the model has a CLS token
 * (V/models/amc_transformer.py:29 reads x[:, 0]), else uniform 1/S (the mean pooling of R/models/transformer_rawIQ.py:91-93).
 * out fp32 [B, S]; each row sums to 1.  0 <= alpha <= 1; same refusals as iq_model_attention. */
int iq_model_attention_rollout(iq_model_t* m, const void* workspace, size_t ws_bytes, int batch, float alpha,
                               float* out, iq_stream_t stream);
/* Class-specific relevance (Chefer, Gur & Wolf 2021, eqs. 5-6) of that forward, which must have formed logits: the data-only
 * backward chain of iq_model_backward_input from dlogits [B,K] (one-hot of the class asked about: the gradient of that logit),
 * no parameter gradient, stopping at layer 0's attention.  As each layer's attention-output gradient appears (top down):
 *   maps[l] != NULL: iq_attn_grad_probs of layer l into maps[l] (rows / heads / positive / out_bstride as there)
 *   rel != NULL:     r <- r (I + mean_h max(P_l * dP_l, 0)) with r starting as iq_model_attention_rollout's does;
 *                    rel fp32 [B, S] receives the final r (= row 0 of R = prod_l (I + A_l), resp. the mean of R's rows)
 * maps: host array of n_layers device pointers (NULL entries skip the layer) or NULL.  Same refusals as
 * iq_model_attention, and when rel and every map are NULL. */
int iq_model_attention_relevance(iq_model_t* m, const float* dlogits, int batch, void* workspace, size_t ws_bytes,
                                 float* rel, float* const* maps, int rows, int heads, int positive, long out_bstride,
                                 iq_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Measurement aid (bench.py roofline leg): when enabled, every entry point above brackets its
 * launches with a HIP event pair on the launch stream.  iq_prof_collect synchronises and returns, per
 * kernel family, the summed elapsed milliseconds and the number of bracketed calls.
 * Families: 0 gemm_nt, 1 wgrad (+slab reduce), 2 attn_fwd, 3 attn_bwd, 4 ln_fwd, 5 ln_bwd,
 *           6 misc (embedding, head, loss, casts), 7 optimizer (gradnorm, adamw). */
#define IQ_PROF_FAMILIES 8
int iq_prof_enable(int on);
int iq_prof_collect(double* ms, long long* count);
/* Per-KERNEL sums of everything iq_prof_collect has gathered since the last reset: one text line per kernel name (the
 * name rocprofv3 --kernel-trace --stats prints, without its namespace):
 *   name \t family \t launches \t total ms \t total algorithmic bytes \t total flops \n
 * (algorithmic bytes / flops of a launch are computed at its launch site from the problem sizes: operands read once,
 * results written once).  Returns the length of the full text; writes at most cap-1 bytes + a terminating 0. */
size_t iq_prof_kernels(char* out, size_t cap, int reset);

#ifdef __cplusplus
}
#endif
#endif /* IQVIT_H */
