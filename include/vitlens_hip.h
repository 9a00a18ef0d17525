/* vitlens_hip.h — C ABI of libvitlens_hip.so (MI355X / gfx950).
 *
 * The reference (TencentARC/ViT-Lens) has NO native layer: its hot path is stock torch.nn
 * modules.  The drop-in boundary is therefore the Python module surface
 * (open_clip.TriCLIP.encode_*, open_clip.loss.*, mm_vit_lens.ViTLens.encode); this C ABI
 * sits directly under that surface and is what a maintainer's ctypes stub binds (see
 * INTEGRATION.md).  Each entry point names the reference call it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed for the duration of the call; nothing is
 *     retained or freed; workspaces are supplied by the caller.  The few HOST arrays are named as
 *     such at their declaration (stride tables of the attention entries, mean / stdv of the
 *     image resampler) and are read before the call returns
 *   - all matrices are row-major; "bf16" is a 16-bit brain-float bit pattern (uint16_t)
 *   - every function is stream-ordered and non-blocking on `stream` (a hipStream_t)
 *   - return value: 0 on success, non-zero on failure; vl_last_error() gives the message
 *   - no exceptions cross the ABI; no global mutable state except the thread-local last-error string; one-time
 *     initialisation (hipFuncSetAttribute, CU count) is done through C++11 function-local statics (thread-safe);
 *     entry points are re-entrant per stream
 */
#ifndef VITLENS_HIP_H
#define VITLENS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

/* epilogues of vl_gemm_bf16 */
#define VL_EPI_BF16 0     /* out bf16[M,N]   = act(alpha*acc + bias)                     */
#define VL_EPI_F32 1      /* out f32 [M,N]   = alpha*acc + bias                          */
#define VL_EPI_RES_F32 2  /* out f32 [M,N]   = res f32 + alpha*acc + bias (in place ok)  */
#define VL_EPI_RES_BF16 3 /* out bf16[M,N]   = res bf16 + alpha*acc + bias               */
#define VL_EPI_GEGLU 5    /* out bf16[M,N/2] = a*gelu(gate), W rows interleaved (a,gate) */
#define VL_EPI_DGELU 6    /* out bf16[M,N]   = alpha*acc * gelu'(res bf16[M,N])  (dX through GELU); with act =
                           * VL_ACT_GELU_DSAVE or VL_ACT_QGELU_DSAVE res IS the derivative (left by the forward): the epilogue is
                           * one multiplication, the same kernel for both.  The recompute form (act = VL_ACT_NONE, res = the
                           * pre-activation) is exact-erf only: VL_ACT_QGELU is refused */
#define VL_EPI_DGEGLU 7   /* acc = dy[M,N]; res = h bf16[M,2N] interleaved (a,g); out bf16[M,2N] = d h  (dX through GEGLU) */
#define VL_ACT_NONE 0
#define VL_ACT_GELU 1     /* exact-erf GELU (nn.GELU default)                            */
#define VL_ACT_RELU 2
#define VL_ACT_GELU_DSAVE 4 /* forward of a TRAINED MLP: out = gelu(pre), out2 (required) = gelu'(pre), both of the bf16-rounded
                             * pre-activation; pair it with VL_EPI_DGELU + the same act in the backward               */
#define VL_ACT_QGELU 5    /* QuickGELU, u * sigmoid(1.702 u): the OpenAI-pretrained CLIP towers (transformer.py:37).
                           * VL_EPI_BF16 only, without out2 (the store-the-pre-activation form is exact-erf only)          */
#define VL_ACT_QGELU_DSAVE 6 /* VL_ACT_GELU_DSAVE for QuickGELU: out = qgelu(pre), out2 (required) = qgelu'(pre) = s + 1.702 pre s (1 - s),
                             * s = sigmoid(1.702 pre), both of the bf16-rounded pre-activation                              */

/* dtype tags for mixed-dtype entry points */
#define VL_F32 0
#define VL_BF16 1
#define VL_F16 2          /* IEEE half: output of vl_layernorm_fwd (from f32 rows) feeding vl_gemm_f16 */

#define VL_GEMM_AUTO (-1)
#define VL_GEMM_PERSIST 8
#define VL_GEMM_PINGPONG 10

const char* vl_last_error(void);
/* ABI version of THIS header: bumped whenever an exported signature changes (round 5 changed vl_ln_row_stats and added the
 * VL_F16 tag and the fp16 / fp32 entries without bumping it; round 6 starts counting: 600 = round 6, first revision).
 * vl_version() returns the library's value; a client built against this header must find them equal before its first
 * call - the Python binding (vitlens_hip/_lib.py) and tests/native/abi_c_client.c both refuse to run otherwise. */
#define VL_ABI_VERSION 610
int vl_version(void);

/* C[M,N] = A[M,K] · W[N,K]^T with fused epilogue.  A, W bf16.  K % 64 == 0, N % 4 == 0.
 * act: VL_ACT_NONE / GELU / RELU / GELU_DSAVE / QGELU / QGELU_DSAVE with VL_EPI_BF16 (RELU also with VL_EPI_RES_BF16, the _DSAVE
 * codes also with VL_EPI_DGELU).  Checked and refused: a _DSAVE code without out2, and the QuickGELU codes with any other
 * epilogue, with the recompute form of VL_EPI_DGELU or (VL_ACT_QGELU) with out2; an epilogue otherwise ignores an act it does not take.
 * cfg selects the kernel family - the ONE selector of this library: nothing else (no environment variable, no global
 * setter) changes which code runs.  VL_GEMM_AUTO (-1) is what every product path passes; the explicit values exist for the
 * parity tests (every family against fp32 and against each other) and the probes under tools/:
 *   -1 VL_GEMM_AUTO     whole rounds of 256-row tiles on the persistent 256x256 kernel (8; 10 where N % 256 == 128), the
 *                       leftover rows on 64x64 tiles or the split-K tail kernel, small problems on 128x128 tiles
 *    8 VL_GEMM_PERSIST  vl_gemm_park.hip: persistent, 256x256 tiles, LDS-DMA two k-steps ahead, 16x16x32 MFMA, burst of
 *                       non-temporal stores; M % 256 == N % 256 == 0, K >= 512
 *   10 VL_GEMM_PINGPONG vl_gemm_pp.hip: two 4-wave workgroups per CU on 256x128 tiles (widths that are multiples of 128 only)
 *    5 (4 = alias)      round-1 persistent kernel (any shape) | 6: the same on 256x128 tiles
 *    0 / 1              one 256x256 / 128x128 LDS-DMA tile per workgroup | 2 / 3: the same with register staging
 *    9                  split-K tail kernel (32x32 tile per workgroup) | 11 / 12: 64x64 / 128x64 tiles
 * (inside the library every number has a name: enum GemmCfg of csrc/vl_gemm_plan.h, which also holds the row split of -1)
 * Replaces nn.Linear / out_proj / mlp.c_fc(+GELU) / mlp.c_proj(+residual)
 * (open_clip/transformer.py:226-234,268-271), Perceiver to_q/to_kv/to_out/FeedForward
 * (open_clip/perceiver.py:85-123), pooled @ proj (transformer.py:786-787) and
 * logit_scale * x @ y.T (open_clip/loss.py:131-136). */
int vl_gemm_bf16(const void* A, const void* W, const float* bias, void* out, const void* res,
                 int M, int N, int K, int lda, int ldw, int ldo, float alpha, int epi, int act,
                 int cfg, hipStream_t stream);

/* Split-K accumulate for weight-gradient GEMMs (tiny M x N, K = token count): out[M,N] f32 (row stride ldo) +=
 * alpha * A[M,K] . W[N,K]^T.  The K range is cut into `splits` slices computed by separate workgroups into the
 * caller's workspace ws (splits*M*N floats) and summed in a fixed order (deterministic, no atomics).
 * Autograd counterpart of the dW of nn.Linear / 1x1 Conv1d in the trainable Lens. */
int vl_gemm_splitk_accum_f32(const void* A, const void* W, float* out, int M, int N, int K, int lda, int ldw, long ldo,
                             float alpha, int splits, float* ws, hipStream_t stream);
/* The same accumulate on TOKEN-MAJOR operands: out[M,N] f32 += alpha * At[K,M]^T . Bt[K,N], At = dY and Bt = X as the backward
 * holds them (row = token, row strides lda >= M, ldb >= N, multiples of 8) - no transposed copies.  M % 256 == N % 256 == 0,
 * K % 64 == 0; the K/64 steps are cut into slices of ceil(K/64/splits) (the last one may be shorter; every slice >= 4 steps);
 * ws = splits*M*N floats.  Fragments come from gfx950's LDS
 * transpose read (csrc/vl_gemm_tn.hip).  Replaces the dW of nn.Linear / in_proj / out_proj under loss.backward()
 * (open_clip/transformer.py:215,226-234,252-272; training/train.py:212-216). */
int vl_gemm_tn_splitk_accum_f32(const void* At, const void* Bt, float* out, int M, int N, int K, int lda, int ldb, long ldo,
                                float alpha, int splits, float* ws, hipStream_t stream);
/* vl_gemm_bf16 + `out2` (with VL_EPI_BF16/VL_ACT_GELU also stores the pre-activation, bf16, for the
 * backward) + `res_div` (VL_EPI_RES_BF16: residual row = m / res_div, i.e. one row broadcast over a group:
 * the PointNet concat([global, local]) conv of dvae.py:207-210 split into two GEMMs).
 * The packed in-projection of nn.MultiheadAttention (transformer.py:215,252) and the Perceiver's to_q / to_kv
 * (perceiver.py:115-116,124-126) are plain calls of this entry point: the attention kernels read q, k, v out of the
 * [tokens, 3*width] result in place (rounds 1-2a had a head-scatter epilogue and transposed copies instead). */
int vl_gemm_bf16_ex(const void* A, const void* W, const float* bias, void* out, const void* res, void* out2,
                    int M, int N, int K, int lda, int ldw, int ldo, float alpha, int epi, int act,
                    int res_div, int cfg, hipStream_t stream);

/* The FROZEN text tower on IEEE-half operands (round 5).  TriCLIP.encode_text (open_clip/model.py:528-540) is forward-only in
 * every recipe and its cosine-similarity MATRIX amplifies operand rounding (text features share a mutual cosine of ~0.6):
 * bf16 operands leave it 0.8-1.9e-3 from the fp32 CPU path, above BASELINE.json's 1e-3; rounds 4's two-term bf16 weights
 * brought it to 6-8e-4 at twice the products.  fp16 carries three more mantissa bits on EVERY operand (weights, GEMM inputs,
 * q / k / v, attention probabilities) at the bf16 MFMA rate: 1-2e-4 at one product per weight.  The reference itself converts
 * CLIP to fp16 (`convert_weights_to_fp16`, open_clip/model.py:393-419; precision "fp16", factory.py:260-295).  The residual
 * stream stays fp32, 16-bit stores saturate at +-65504.
 *   vl_gemm_f16      C = A . W^T with A [M,K], W [N,K] fp16; epi = VL_EPI_BF16 (here: out fp16 [M,N] = act(alpha*acc + bias),
 *                    act none / GELU / QGELU) or VL_EPI_RES_F32 (out f32 = res f32 + alpha*acc + bias, in place allowed).  The
 *                    persistent 256x256 kernel only: M % 256 == N % 256 == 0, K % 64 == 0, K >= 512, 16-byte aligned
 *                    operands - the caller pads its rows to whole tiles (replaces in_proj / out_proj / c_fc / c_proj of
 *                    the text tower's ResidualAttentionBlocks, transformer.py:226-234,254-272)
 *   vl_attn_fwd_f16  vl_attn_fwd_bf16 on fp16 q, k, v -> fp16 out: head dim 64, <= 288 keys, causal or not
 *                    (F.multi_head_attention_forward with the additive causal mask, transformer.py:241-252,870-876)
 *   vl_layernorm_fwd with y_dtype = VL_F16 writes the GEMM inputs. */
int vl_gemm_f16(const void* A, const void* W, const float* bias, void* out, const void* res, int M, int N, int K,
                int lda, int ldw, int ldo, float alpha, int epi, int act, hipStream_t stream);
int vl_attn_fwd_f16(const void* q, const void* k, const void* v, const long* strides, void* out, float* lse,
                    int B, int H, int Lq, int Lk, int dh, float qscale, int causal, hipStream_t stream);

/* The text tower on the rows UP TO each caption's pooled position only (ABI 608).  The feature is
 * ln_final(x[b, argmax(text[b])]) @ text_projection (open_clip/model.py:528-540) and the tower is causal
 * (transformer.py:870-876): row t depends on rows <= t, so nothing behind the pooled row is ever read.  The captions' needed
 * rows are packed one behind the other; LayerNorm and the GEMMs are row-wise and simply see fewer rows.
 *   vl_text_pack_plan       ids int64 [B, L] -> len[b] = argmax(ids[b]) + 1 (first maximum, as torch.argmax; int [B]),
 *                           start int [B+1] = exclusive sum of len in batch order (start[B] = packed rows), last_row int64 [B]
 *                           = start[b] + len[b] - 1 (vl_layernorm_fwd's row_index with row_mul = 0: the pooling),
 *                           total int [2] = {packed rows, longest caption}.  Integer arithmetic only: deterministic.  Any B.
 *   vl_text_embed_packed    out f32 [>= rows_pad, D]: row start[b] + t = tok_emb[ids[b,t]] + pos[t] for t < len[b]; rows
 *                           [rows, rows_pad) = 0 (the fp16 GEMMs run whole 256-row tiles); rows beyond are not touched.
 *                           rows / rows_pad are the host's copy of the plan's total (B <= rows <= B*L checked; a row index at or
 *                           beyond rows is not written)
 *   vl_attn_fwd_varlen_f16  causal self-attention per caption on fp16 operands: q, k, v = column blocks of the packed
 *                           in-projection output [rows, 3*width], strides = (head, row) element strides of q, k, v (6 values,
 *                           multiples of 8); caption b owns rows start[b] .. start[b] + len[b] - 1 of the operands and of
 *                           out fp16 [rows, H*64]; lse f32 [rows, H] optional (natural log).  Head dim 64, max_len (>= every
 *                           len[b]) <= 288 - the limits of vl_attn_fwd_f16; refused with a status otherwise.  Rows at or beyond
 *                           len[b] are never read: indices are clamped to the caption's own rows.  max_len must be what the
 *                           plan gave: with a len[b] above it (or above the 32 / 96 / 288-key image chosen from it) only the
 *                           first rows of that caption are computed, the others are left unwritten and no status tells. */
int vl_text_pack_plan(const int64_t* ids, int* len, int* start, int64_t* last_row, int* total, int B, int L,
                      hipStream_t stream);
int vl_text_embed_packed(const int64_t* ids, const int* start, const int* len, const float* tok_emb, const float* pos,
                         float* out, int B, int L, int D, int vocab, int rows, int rows_pad, hipStream_t stream);
int vl_attn_fwd_varlen_f16(const void* q, const void* k, const void* v, const long* strides, const int* start,
                           const int* len, void* out, float* lse, int B, int H, int max_len, int dh, float qscale,
                           hipStream_t stream);

/* True fp32 arithmetic for INFERENCE (round 5): `precision="fp32"` of the reference's factory (open_clip/factory.py:260-295,
 * training/precision.py:5-12) means fp32 nn.Linear / attention products; rounds 1-4 ran bf16 operands there and said so in a
 * warning.  gfx950 has fp32-input MFMA at the fp32 vector rate (157 TFLOP/s, 1/16 of bf16), exact fmaf chains:
 *   vl_gemm_f32      out f32 [M,N] = act(alpha * A[M,K] W[N,K]^T + bias) (+ res f32 [M,N], in place allowed); any M, N;
 *                    K, lda, ldw multiples of 4; act none / GELU (erff) / ReLU / QGELU (expf and a true division)
 *                    (csrc/vl_f32.hip, v_mfma_f32_32x32x2_f32)
 *   vl_attn_fwd_f32  softmax(scale * q k^T [+ causal mask]) v on strided f32 [B,H,L,dh] views (strides as vl_attn_fwd_bf16,
 *                    multiples of 4), dh = 32, 64 or a multiple of 8 in (64, 128]; out f32 [B,Lq,H*dh]; lse optional
 *                    (natural log)
 *   vl_im2col_f32    vl_im2col_bf16 with f32 patches
 * LayerNorm, the token assembly and the text embedding already take f32 in and out.  Forward only: training under
 * precision="fp32" keeps bf16 operands with fp32 residual / gradient streams (vitlens_hip/f32.py says what runs). */
int vl_gemm_f32(const float* A, const float* W, const float* bias, float* out, const float* res, int M, int N, int K,
                int lda, int ldw, int ldo, float alpha, int act, hipStream_t stream);
int vl_attn_fwd_f32(const float* q, const float* k, const float* v, const long* strides, float* out, float* lse,
                    int B, int H, int Lq, int Lk, int dh, float scale, int causal, hipStream_t stream);
int vl_im2col_f32(const float* x, float* patches, int N, int C, int H, int W, int kh, int kw, int sh, int sw,
                  int Kp, int transpose_hw, hipStream_t stream);
/* The fp32 Lenses (audio, EEG, point cloud, depth with a Perceiver; vitlens_hip/f32.py):
 *   vl_gemm_f32_ex   vl_gemm_f32 with two more epilogues; with geglu = res_pre = 0 and res_div = 1 it IS vl_gemm_f32 (same
 *                    kernel, bit-identical outputs).
 *                    res_pre = 1: out = act(alpha A W^T + bias + res[m / res_div]) - the residual (row stride ldo) joins BEFORE
 *                    the activation, one row per res_div output rows (PointBERT's second conv, relu(f W3l^T + (max(f) W3g^T +
 *                    b3)[group]), dvae.py:207-210).  res_div > 1 needs res_pre.
 *                    geglu = 1: W rows interleaved (a_j, gate_j), N even, out f32 [M, N/2] = (acc + b)[2j] * gelu((acc + b)[2j+1])
 *                    (erff, as the GELU epilogue; the Perceiver FeedForward, perceiver.py:85-102); no residual, act = none
 *   vl_knn_group_f32 vl_knn_group (same selection code: the same neighbour sets) writing fp32 patches x_j - centre, zero padded
 *                    to Kp (a multiple of 4)
 *   vl_group_max_f32 vl_group_max on f32 input and output (NaN propagates, as torch.max)
 *   vl_pad3_f32      centres [R,3] f32 -> f32 [R,Kp] zero padded (Kp a multiple of 4) */
int vl_gemm_f32_ex(const float* A, const float* W, const float* bias, float* out, const float* res, int M, int N, int K,
                   int lda, int ldw, int ldo, float alpha, int act, int res_div, int res_pre, int geglu, hipStream_t stream);
int vl_knn_group_f32(const float* xyz, const int64_t* center_idx, int* nidx, float* patches, int B, int N, int G,
                     int k, int Kp, hipStream_t stream);
int vl_group_max_f32(const float* x, long ldx, float* out, long ldo, long groups, int M, int C, hipStream_t stream);
int vl_pad3_f32(const float* c, float* out, long R, int Kp, hipStream_t stream);

int vl_device_info(int device, char* arch, int arch_len, int* cus, int* clock_khz, long* hbm_bytes);

/* Fused attention forward: softmax(q k^T [+ causal mask]) v without materialising the scores.
 * q, k, v are STRIDED [B,H,L,dh] views: element (b,h,l,d) of operand i at ptr_i[b*strides[3i] + h*strides[3i+1] +
 * l*strides[3i+2] + d] (strides in elements, multiples of 8; i = 0,1,2 for q,k,v) - normally the three column blocks of
 * the packed in-projection output [tokens, 3*width], read in place.  q is multiplied by qscale (softmax_scale*log2e;
 * pass 1 for a pre-scaled q) as it is loaded; V is transposed while it is staged into LDS.
 * out [B,Lq,H*dh] bf16 (token-major, ready for the out-projection); lse [B,H,Lq] optional (natural-log LSE of the
 * scaled scores, kept for the backward pass).  dh = 32, 64, or a multiple of 8 in (64, 128] (ViT-H/14: 80, ViT-bigG/14:
 * 104): those run zero-padded to 128 inside the kernel, only the real columns are read and written.
 * Replaces F.multi_head_attention_forward (transformer.py:241-252, causal mask :870-876) and
 * the Perceiver einsum attention (perceiver.py:128-145). */
int vl_attn_fwd_bf16(const void* q, const void* k, const void* v, const long* strides, void* out, float* lse,
                     int B, int H, int Lq, int Lk, int dh, float qscale, int causal, hipStream_t stream);

/* LayerNorm folded into the GEMMs either side of it (round 4).  For a FROZEN pre-LN block on a bf16 residual stream
 * (ResidualAttentionBlock, transformer.py:254-272: x + attn(ln_1(x)), x + mlp(ln_2(x)); LayerNorm transformer.py:17-34)
 *     LN(x) W^T + b  =  rstd_m (x (W gamma)^T - mean_m c) + (b + W beta),      c_n = sum_k (W gamma)[n, k]
 * so the consuming GEMM can read the raw residual rows and apply the row statistics in its epilogue, and the GEMM that
 * produced those rows can leave their partial sums behind: the normalised activations are never written or read.
 *   vl_gemm_main_rows          rows of an [M, K] x [N, K]^T problem that vl_gemm_bf16 (cfg -1) gives to the persistent
 *                              256x256-tile kernel; the entries below take exactly such row ranges (0: none)
 *   vl_gemm_rest_cfg           the cfg (1, 11 or 9) vl_gemm_bf16 (cfg -1) runs `rows` rows behind that range on: what a caller
 *                              that splits the rows itself passes for them (a standalone call of that size would get 128x128 tiles)
 *   vl_gemm_lnfold_bf16        out bf16[M,N] = act(rstd_m * (A Wg^T - mean_m * ln_c) + bias_f); A = raw rows bf16 [M,K],
 *                              Wg = bf16(W * gamma) [N,K], bias_f = b + W beta f32 [N], ln_c f32 [N] (sums of the ROUNDED
 *                              Wg rows), ln_mean / ln_rstd f32 [M]; act = VL_ACT_NONE / VL_ACT_GELU / VL_ACT_GELU_DSAVE /
 *                              VL_ACT_QGELU / VL_ACT_QGELU_DSAVE (out2 = the derivative, as vl_gemm_bf16_ex)
 *   vl_gemm_res_rowstats_bf16  out bf16 = res + A W^T + bias (VL_EPI_RES_BF16, in place allowed) and row_part f32
 *                              [M][N/64][2] = (sum, sum of squares) of the STORED bf16 values per row and 64-column slice
 *   vl_ln_row_stats            mean / rstd [rows]: rows < m_main from row_part (P = N/64 slices, summed in slice order),
 *                              rows >= m_main from the bf16 rows themselves (the leftover rows of a row-split GEMM); a row
 *                              whose E[x^2] - mean^2 would cancel (variance below 1e-3 of E[x^2], |mean| > ~30 sigma) is
 *                              also recomputed two-pass from its stored values: x_bf16 is always required.  y_left (optional,
 *                              with ln_w / ln_b): bf16 LayerNorm output of the rows >= y_row0 (>= m_main), row r at
 *                              y_left[(r - y_row0) * y_row_stride] - the rows the consuming GEMM runs as layernorm + small
 *                              tiles get their operand from this launch instead of one more 256-row LayerNorm launch
 * Whole 256x256 tiles, K >= 512, 16-byte aligned operands; anything else is refused (the caller keeps vl_layernorm_fwd +
 * vl_gemm_bf16 for it). */
int vl_gemm_main_rows(int M, int N);
int vl_gemm_rest_cfg(int rows, int N);
int vl_gemm_lnfold_bf16(const void* A, const void* Wg, const float* bias_f, const float* ln_c, const float* ln_mean,
                        const float* ln_rstd, void* out, void* out2, int M, int N, int K, int lda, int ldw, int ldo, int act,
                        hipStream_t stream);
int vl_gemm_res_rowstats_bf16(const void* A, const void* W, const float* bias, void* out, const void* res, float* row_part,
                              int M, int N, int K, int lda, int ldw, int ldo, hipStream_t stream);
int vl_ln_row_stats(const float* row_part, int P, const void* x_bf16, long x_row_stride, int D, int m_main, int rows, float eps,
                    float* mean, float* rstd, const float* ln_w, const float* ln_b, void* y_left, long y_row_stride, int y_row0,
                    hipStream_t stream);

/* LayerNorm over the last dim (eps inside sqrt, biased variance): y = (x-mean)*rstd*w + b.
 * Source row for output row r is  r*row_mul + row_index[r]  when row_index != NULL (EOT gather,
 * model.py:539; cls pooling uses row_index == NULL with x_row_stride = (T+1)*D), else r.
 * Replaces LayerNorm/LayerNormFp32 (transformer.py:17-34) and PreNorm (perceiver.py:67-82).
 * Dtype pairs (x -> y): f32 -> f32 | bf16 | f16, bf16 -> f32 | bf16; any other pair is refused with a status, and so is one of
 * mean / rstd without the other (this holds for vl_assemble_ln_pre and vl_assemble_ln_pre_keep too).  D % 256 == 0 rows whose
 * strides and base addresses (x, y, w, b; cls, pos, pos2, xpre) are multiples of 4 elements are held in registers and moved 8 /
 * 16 bytes at a time; everything else takes the any-D form, one element at a time. */
int vl_layernorm_fwd(const void* x, int x_dtype, long x_row_stride, const int64_t* row_index, long row_mul,
                     const float* w, const float* b, void* y, int y_dtype, long y_row_stride,
                     float* mean, float* rstd, int rows, int D, float eps, hipStream_t stream);

/* [cls ; tokens] + positional_embedding (+ adapter pos on rows 1..T) -> ln_pre, one pass.
 * tokens [B,T,D]; y [B,T+1,D].  Optional (training): xpre f32 [B,T+1,D] = the un-normalised rows,
 * mean/rstd [B*(T+1)].  Replaces transformer.py:756-772 (+ :734-745 for pos2). */
int vl_assemble_ln_pre(const void* tokens, int tok_dtype, const float* cls, const float* pos, const float* pos2,
                       const float* w, const float* b, void* y, int y_dtype, float* xpre, float* mean, float* rstd,
                       int B, int T, int D, float eps, hipStream_t stream);

/* [cls ; tokens] + positional_embedding (+ adapter pos on rows 1..T) with NO LayerNorm behind it: the token assembly of a tower
 * without ln_pre (the BLIP-2 EVA ViT-g adds pos_embed and enters block 0).  vl_assemble_ln_pre's arguments minus w, b, eps,
 * mean, rstd: tokens [B,T,D] f32 | bf16; cls [D], pos [T+1,D], pos2 [T,D] or NULL, f32; y [B,T+1,D] f32 | bf16 (the residual-
 * stream dtype); xpre optional f32 [B,T+1,D] copy of the same rows.  Dense form only.  One wave per row; rows whose operands'
 * base addresses are multiples of 4 elements, with D % 4 == 0, move 8 / 16 bytes at a time, everything else one element at a
 * time (vl_layernorm_fwd's rule).  Refused with a status: an empty problem, a missing operand, any other dtype code.
 *
 * With this entry, vl_layernorm_fwd (row_index == NULL or not) and the three vl_layernorm_bwd* entries hold a D = 1408 row
 * (5 * 256 + 128) in registers too: five 256-element chunks and a half chunk in lanes 0-31, the other lanes entering the wave
 * reductions with zeros - under the same alignment conditions as the D % 256 == 0 forms, the any-D form otherwise.  No other
 * width changes its path.
 * NOTE on the version: like vl_pc_augment, this entry was added under VL_ABI_VERSION 610, which tests/test_linprobe_host.py
 * pins: a library built before it reports the same number and lacks the symbol, and a client must look it up when it loads the
 * library (vitlens_hip/_lib.py does, and names such a library as stale).  No existing entry changes. */
int vl_assemble_tokens(const void* tokens, int tok_dtype, const float* cls, const float* pos, const float* pos2,
                       void* y, int y_dtype, float* xpre, int B, int T, int D, hipStream_t stream);

/* ---- patch dropout (PatchDropout, open_clip/transformer.py:53-90: train mode keeps the class token + K of the T tokens) ----
 * The selection.  keep int32 [B,K]: keep[b,j] = the index of the j-th largest key of sample b, ties to the lower index (with
 * distinct keys: torch.topk(keys, K).indices exactly); inv int32 [B,T]: inv[b,t] = j + 1 if keep[b,j] == t, else 0.
 * keys f32 [B,T], which must be FINITE (a NaN has no place in the order; nothing is read or written out of bounds for one, but
 * the selection is then unspecified) - or NULL: the kernel draws its own.  The key of (b, t) is then word t & 3 of
 * Philox4x32-10 with counter (t >> 2, lo32(sample0 + b), hi32(sample0 + b), 0) and key (lo32(seed), hi32(seed)), compared as
 * unsigned 32-bit integers.  Refused with a status: anything outside 1 <= K <= T <= 4096, B < 1. */
int vl_patch_keep(const float* keys, uint64_t seed, int64_t sample0, int B, int T, int K, int* keep, int* inv,
                  hipStream_t stream);
/* vl_assemble_ln_pre on the kept rows only: y [B,K+1,D]; row 0 of a sample = cls + pos[0], row j >= 1 = tokens[b,t] + pos[1+t]
 * (+ pos2[t]) with t = keep[b,j-1], then ln_pre.  tokens [B,T,D], keep int32 [B,K] with entries in [0, T) (clamped into it).
 * The optional training outputs xpre [B,K+1,D], mean / rstd [B*(K+1)] and the dtype combinations are vl_assemble_ln_pre's; a
 * row is bit-identical to the dense entry's row (b, 1+t) - the same code path computes it. */
int vl_assemble_ln_pre_keep(const void* tokens, int tok_dtype, const int* keep, const float* cls, const float* pos,
                            const float* pos2, const float* w, const float* b, void* y, int y_dtype, float* xpre,
                            float* mean, float* rstd, int B, int T, int K, int D, float eps, hipStream_t stream);
/* The backward of that gather, as a gather through inv: out f32 [B,T,D], row (b,t) = src[b, inv[b,t], :] if inv[b,t] > 0 else
 * zeros; src f32 [B,K+1,D] (the ln_pre input gradient; row 0 = the class token's, never scattered).  Every output row is
 * written once: no fill pass, no atomics, bit-reproducible.  16-byte accesses when D % 4 == 0 and both bases are aligned. */
int vl_scatter_rows_keep(const float* src, const int* inv, float* out, int B, int T, int K, int D, hipStream_t stream);

/* F.normalize(dim=-1, eps): y f32 and/or bf16 copy; norms[rows] optional (model.py:522-540). */
int vl_l2_normalize(const float* x, float* y, void* y_bf16, float* norms, int rows, int D, float eps,
                    hipStream_t stream);
int vl_l2_normalize_bwd(const float* f, const float* df, const float* norms, float* dx, int rows, int D, float eps,
                        hipStream_t stream);

/* Patch extraction for Conv2d(bias=False, padding=0) as a GEMM operand: x [N,C,H,W] f32 ->
 * patches bf16 [N*gh*gw, Kp], column order (c,i,j), zero padded to Kp.  transpose_hw=1 reads the
 * stored tensor as [N,C,W,H] (AST_tokenizer.py:46-47).  Token order is row-major (gh, gw)
 * exactly as conv -> reshape(N,C,-1).permute(0,2,1) (transformer.py:674-676). */
int vl_im2col_bf16(const float* x, void* patches, int N, int C, int H, int W, int kh, int kw, int sh, int sw,
                   int Kp, int transpose_hw, hipStream_t stream);

/* out[b,l,:] = token_embedding[ids[b,l]] + positional_embedding[l]   (model.py:531-533); ids are clamped into [0, vocab).
 * out_dtype VL_F32 | VL_BF16, anything else is refused with a status. */
int vl_text_embed(const int64_t* ids, const float* tok_emb, const float* pos, void* out, int out_dtype,
                  int B, int L, int D, int vocab, hipStream_t stream);

int vl_cast_f32_bf16(const float* x, void* y, long n, hipStream_t stream);
/* y[r,:] = x[r,:] + table[r % T,:]   (x_vada["x"] + x_vada["pos"], transformer.py:743-745).  x_dtype, y_dtype VL_F32 |
 * VL_BF16, anything else is refused with a status. */
int vl_add_rows(const void* x, int x_dtype, const float* table, void* y, int y_dtype, long rows, int T, int D,
                hipStream_t stream);
/* out[c,r] bf16 = in[r,c]; columns r in [R, ldo) zero-filled (operand prep for gradient GEMMs) */
int vl_transpose_to_bf16(const void* in, int in_dtype, long ldi, int R, int C, void* out, long ldo, hipStream_t stream);
/* The same for the weight-gradient path (C % 64 == 0, ldo % 8 == 0, ldi % 8 == 0, 16-byte aligned pointers), optionally
 * fused with the bias gradient: colsum_out[c] += colsum_scale * sum_r in[r, c] (deterministic two-stage sum; ws =
 * ceil(ldo/256)*C floats).  Autograd counterpart of nn.Linear's dW operands and bias gradient. */
int vl_transpose_colsum_bf16(const void* in, int in_dtype, long ldi, int R, int C, void* out, long ldo,
                             float* colsum_out, float colsum_scale, float* ws, hipStream_t stream);

/* InfoNCE pieces over logits f32 [R,C] (row r's positive is column r+label_off):
 *   vl_ce_stats      row_lse[R], col_lse[C], diag[R]; col_ws = 2*ceil(R/64)*C floats of workspace
 *   vl_ce_loss_accum *loss += w_row*mean(row_lse-diag) + w_col*mean(col_lse[r+off]-diag)
 *   vl_ce_grad       G[R,ldg] / GT[C,ldgt] bf16 = dLoss/dlogits (and transpose), *dscale += <G,logits>/scale (two-stage
 *                    fixed-order sum through ws = vl_ce_grad_ws_floats(R, C, ldg, ldgt) floats: deterministic)
 * Replaces F.cross_entropy(logits_per_x)+F.cross_entropy(logits_per_y) and autograd thereof
 * (loss.py:158-163, 300-306, 377-383). */
/* f32 [rows,D] -> bf16 [rows,3D] hi/lo split (pattern 0: hi|lo|hi, 1: hi|hi|lo) for near-fp32 logits */
int vl_split_bf16x3(const float* x, void* out, long rows, int D, int pattern, hipStream_t stream);
int vl_ce_stats(const float* logits, long ld, int R, int C, int label_off, float* row_lse, float* col_lse,
                float* diag, float* col_ws, hipStream_t stream);
int vl_ce_loss_accum(const float* row_lse, const float* col_lse, const float* diag, int R, int C, int label_off,
                     float w_row, float w_col, float* loss_inout, hipStream_t stream);
int vl_ce_grad(const float* logits, long ld, int R, int C, int label_off, const float* row_lse, const float* col_lse,
               float w_row, float w_col, void* G, long ldg, void* GT, long ldgt, float logit_scale,
               float* dscale_inout, float* ws, hipStream_t stream);
long vl_ce_grad_ws_floats(int R, int C, long ldg, long ldgt);
/* The similarity-masked forms (ClipLossSimMask, loss.py:522-598): the same arguments plus sim f32 [R, ld_sim >= C] (teacher
 * similarities of the rows against the columns) and thres.  An element (r, c) with c != r + label_off and
 * sim[r, c] >= thres is read as logit 0.0f (the reference MULTIPLIES the logits by the mask: it stays in the softmax
 * denominators of its row and its column), its entry of G / GT is 0 and it adds nothing to *dscale.  diag is never masked,
 * so vl_ce_loss_accum serves both forms.  sim is read only at r < R, c < C; a NaN similarity is kept. */
int vl_ce_stats_masked(const float* logits, long ld, int R, int C, int label_off, float* row_lse, float* col_lse,
                       float* diag, float* col_ws, const float* sim, long ld_sim, float thres, hipStream_t stream);
int vl_ce_grad_masked(const float* logits, long ld, int R, int C, int label_off, const float* row_lse, const float* col_lse,
                      float w_row, float w_col, void* G, long ldg, void* GT, long ldgt, float logit_scale,
                      float* dscale_inout, float* ws, const float* sim, long ld_sim, float thres, hipStream_t stream);

/* ---- backward / optimizer (trainable towers; autograd of the ops above) ---------------------- */
/* dx = dLN(dy) + dres (optional); outputs f32 `dx` and/or a bf16 copy `dx_bf16` (next GEMM operand). */
int vl_layernorm_bwd(const void* dy, int dy_dtype, long dy_stride, const void* x, int x_dtype, long x_stride,
                     const float* mean, const float* rstd, const float* w, const float* dres, float* dx,
                     void* dx_bf16, long dx_stride, int rows, int D, hipStream_t stream);
/* The same with the residual-gradient stream (dres in, dx out) in dtype g_dtype (VL_F32 | VL_BF16): bf16 is what the
 * reference's amp_bf16 autocast carries for the gradients of its bf16 residual stream.  dy_dtype, x_dtype and g_dtype other
 * than VL_F32 | VL_BF16 are refused with a status (vl_layernorm_bwd_sres too).  D in {256, 512, 768, 1024} with every row
 * stride (the sparse form's dres_stride included) and every base address (dy, x, w, dres, dx, dx_bf16) a multiple of 4
 * elements: one read of the row into registers, 8 / 16-byte accesses; everything else: the any-D form. */
int vl_layernorm_bwd_g(const void* dy, int dy_dtype, long dy_stride, const void* x, int x_dtype, long x_stride,
                       const float* mean, const float* rstd, const float* w, const void* dres, void* dx, int g_dtype,
                       void* dx_bf16, long dx_stride, int rows, int D, hipStream_t stream);
/* vl_layernorm_bwd_g with a SPARSE upstream residual gradient: only the rows i * dres_every have one, row i of dres (row
 * stride dres_stride, dtype g_dtype); every other row adds nothing and reads nothing.  dx is written for all rows, so the
 * caller keeps no zero-filled residual-gradient buffer (the class-token rows behind a block that ran on those rows only).
 * dres must not alias dx. */
int vl_layernorm_bwd_sres(const void* dy, int dy_dtype, long dy_stride, const void* x, int x_dtype, long x_stride,
                          const float* mean, const float* rstd, const float* w, const void* dres, int dres_every,
                          long dres_stride, void* dx, int g_dtype, void* dx_bf16, long dx_stride, int rows, int D,
                          hipStream_t stream);
/* Column reductions are deterministic two-stage sums (row slabs -> fixed-order combine, no atomics) and need a caller
 * workspace of vl_colreduce_ws_floats(rows, cols, planes) floats (planes: 2 for the LayerNorm parameters, 1 for vl_colsum). */
long vl_colreduce_ws_floats(int rows, int cols, int planes);
/* dw[j] += sum_r dy*xhat ; db[j] += sum_r dy   (accumulating; zero the buffers first) */
int vl_layernorm_bwd_params(const void* dy, int dy_dtype, long dy_stride, const void* x, int x_dtype, long x_stride,
                            const float* mean, const float* rstd, float* dw, float* db, int rows, int D,
                            float* ws, hipStream_t stream);
/* out[j] += scale * sum_r a[r,j]  (bias gradients) */
int vl_colsum(const void* a, int a_dtype, long lda, float* out, int rows, int cols, float scale, float* ws, hipStream_t stream);
int vl_gelu_bf16(const void* u, void* y, long n, hipStream_t stream);
/* y[m,j] = h[m,2j] * gelu(h[m,2j+1])  (recompute of the GEGLU output from the saved pre-activation) */
int vl_geglu_bf16(const void* h, void* y, long rows, int n_out, hipStream_t stream);
/* Attention backward (see csrc/vl_attn_bwd.hip).  q, k, v, dO, o are strided [B,H,L,dh] views (strides[15]: sb, sh, sr
 * in elements for q, k, v, dO, o in that order - multiples of 8), read in place: q/k/v out of the packed in-projection
 * output, dO out of the out-projection's input gradient [tokens, width], o = the forward's token-major output.  q is
 * multiplied by qscale (= scale*log2e) as it is loaded, as in the forward.  delta [B,H,Lq] fp32 is a caller workspace:
 * rowsum(dO*o) is produced by the first kernel and consumed by the second.  dq/dk/dv are token-major bf16 destinations
 * with row strides ld_dq / ld_dkv, already offset to their column block; scale = softmax scale. */
int vl_attn_bwd_bf16(const void* q, const void* k, const void* v, const void* dO, const void* o, const long* strides,
                     const float* lse, float* delta, void* dq, void* dk, void* dv, long ld_dq, long ld_dkv,
                     int B, int H, int Lq, int Lk, int dh, float qscale, int causal, float scale, hipStream_t stream);
/* ONE-kernel attention backward for self-attention that fits a workgroup (csrc/vl_attn_bwd_fused.hip, round 4): head dim 64,
 * Lq == Lk == L, no causal mask, L <= 256 or L = 32 m + 1 <= 257.  Same operands and destinations as vl_attn_bwd_bf16
 * (strides[15]); delta is computed while dO is staged (no workspace).  Every score tile is evaluated once: 5 matrix products
 * and 16 exponentials per lane per 32x32 tile instead of 7 and 32.  Replaces the autograd of
 * F.multi_head_attention_forward (open_clip/transformer.py:241-252) and of the Perceiver's latent self-attention
 * (open_clip/perceiver.py:128-145).  vl_attn_bwd_fused_supported returns 1 when the fused entry takes the problem. */
int vl_attn_bwd_fused_supported(int Lq, int Lk, int dh, int causal);
int vl_attn_bwd_fused_bf16(const void* q, const void* k, const void* v, const void* dO, const void* o, const long* strides,
                           const float* lse, void* dq, void* dk, void* dv, long ld_dq, long ld_dkv, int B, int H, int L, int dh,
                           float qscale, float scale, hipStream_t stream);
/* Single-query attention (csrc/vl_attn_pool.hip): ONE query row per (batch, head) - row `qrow` of the q view - against all L
 * keys and values; what the last block of a class-token-pooled tower needs.  q, k, v: bf16 [B,H,L,dh] strided views
 * (strides[9] as vl_attn_fwd_bf16), head dim 64, 1 <= L <= 1024, no mask.  q is multiplied by qscale (softmax scale * log2e)
 * and rounded to bf16 as in vl_attn_fwd_bf16; fp32 math.  out bf16 [B, H*64] (row stride ld_out), lse f32 [B, H] (optional,
 * natural-log domain of the scaled scores). */
int vl_attn_fwd_q1(const void* q, const void* k, const void* v, const long* strides, void* out, long ld_out, float* lse,
                   int B, int H, int L, int dh, int qrow, float qscale, hipStream_t stream);
/* Its backward: dO, o bf16 [B, H*64] (row strides ld_do, ld_o), lse [B, H] as the forward left them.  dq / dk / dv are the
 * token-major [B*L, .] destinations of vl_attn_bwd_bf16 (already offset to their column block, row strides ld_dq / ld_dkv):
 * dk and dv are written for all L rows, dq for row qrow, and the dq rows of every OTHER token are written as zeros, so the
 * buffer is fully defined without a fill pass.  scale = softmax scale, qscale = scale * log2e. */
int vl_attn_bwd_q1(const void* q, const void* k, const void* v, const long* strides, const void* dO, long ld_do,
                   const void* o, long ld_o, const float* lse, void* dq, void* dk, void* dv, long ld_dq, long ld_dkv,
                   int B, int H, int L, int dh, int qrow, float qscale, float scale, hipStream_t stream);
/* ---- Perceiver dropout (csrc/vl_lens_drop.hip; the attention backward in csrc/vl_attn_bwd.hip): the Lens's attn_dropout on
 * the attention probabilities and ff_dropout behind the second Linear of a FeedForward (open_clip/perceiver.py:91-102, 105-154), train mode only.  The mask is a pure function of
 * numbers and is never stored: element e is KEPT iff its Philox4x32-10 word is >= round(p * 2^32) as a uint32, a kept value is
 * multiplied by 1 / (1 - p) computed in fp32.  Key (lo32(seed), hi32(seed)); counter
 *     (group, lo32(sample0 + b), hi32(sample0 + b), sublayer)
 * with b the sample (batch row) and `sublayer` the position of the sub-layer in the Perceiver's forward, counted from 0 over
 * attentions and FeedForwards alike (so an attention and a FeedForward, or two calls of weight-tied modules, never share one).
 * The element group inside the sample and the word of the four:
 *     attention probability (head h, query i, key j):  group = (h * Lq + i) * ceil(Lk / 4) + j / 4,   word j % 4
 *     FeedForward output (latent row i, column c):     group = i * (D / 4) + c / 4,                   word c % 4
 * Refused with a status: p outside [0, 1), a group count beyond 2^32, a shape the kernels do not take - never a run without
 * dropout.  tests/perceiver_drop_ref.py restates the layout in numpy.
 * NOTE on the version: these four entries were added under VL_ABI_VERSION 610, which tests/test_linprobe_host.py pins, so a
 * library built before them reports the same number and does not have them.  A client that calls them must look the
 * symbols up when it loads the library (the Python binding does: vitlens_hip/_lib.py names a library that lacks a symbol of its
 * table as stale).  vl_pc_augment below was added under 610 in the same way; the next change of an EXISTING entry bumps the
 * number and ends the overlap.
 *
 * vl_attn_fwd_drop_bf16: vl_attn_fwd_bf16 (same operands, strides[9], qscale, token-major out, lse) with
 * out = (P * M / (1 - p)) V.  The softmax normaliser is the sum over ALL keys and lse is what vl_attn_fwd_bf16 writes; the
 * mask is applied to the unnormalised fp32 probabilities before they are rounded to bf16 for the P.V product.  Head dims 32,
 * 64, or a multiple of 8 in (64, 128]; any Lq, Lk.
 * vl_attn_bwd_drop_bf16: vl_attn_bwd_bf16 (same operands, strides[15], delta workspace, destinations) for that forward:
 * dV = (P M / (1 - p))^T dO, dP = (dO V^T) M / (1 - p), dS = P (dP - delta), delta = rowsum(dO * O).  Two kernels. */
int vl_attn_fwd_drop_bf16(const void* q, const void* k, const void* v, const long* strides, void* out, float* lse, int B, int H,
                          int Lq, int Lk, int dh, float qscale, int causal, double p, uint64_t seed, int64_t sample0,
                          int sublayer, hipStream_t stream);
int vl_attn_bwd_drop_bf16(const void* q, const void* k, const void* v, const void* dO, const void* o, const long* strides,
                          const float* lse, float* delta, void* dq, void* dk, void* dv, long ld_dq, long ld_dkv, int B, int H,
                          int Lq, int Lk, int dh, float qscale, int causal, float scale, double p, uint64_t seed,
                          int64_t sample0, int sublayer, hipStream_t stream);
/* x1 = x0 + y * M / (1 - p): y f32 [B*n, D] = the down-projection's output with its bias (dropped with it), x0 / x1 f32 [B*n, D]
 * the residual stream (x1 may alias x0 or y), n rows per sample, D % 4 == 0. */
int vl_ff_drop_fwd(const float* y, const float* x0, float* x1, int B, int n, int D, double p, uint64_t seed, int64_t sample0,
                   int sublayer, hipStream_t stream);
/* Its backward on the branch: dy bf16 [B*n, D] = dx1 * M / (1 - p) of the residual gradient dx1 f32 [B*n, D] (the residual
 * branch itself keeps dx1) - the operand of the dW2 and dGEGLU products - and, optionally, the same products unrounded in
 * dy_f32 f32 [B*n, D] (may alias dx1), whose column sum is db2. */
int vl_ff_drop_bwd(const float* dx1, void* dy, float* dy_f32, int B, int n, int D, double p, uint64_t seed, int64_t sample0,
                   int sublayer, hipStream_t stream);
/* ---- audio front end (csrc/vl_audio.hip) ----
 * Kaldi-compatible log-mel filterbank = torchaudio.compliance.kaldi.fbank(htk_compat, 16 kHz, hanning window, 128 bins,
 * no dither, 25 ms / 10 ms frames, snip_edges) + zero-padding / truncation to target_len rows + Normalize(mean, std), i.e.
 * AudioASTProcessorEval.convert2fbank + transform (open_clip/modal_audio/processors/at_processor.py:839-873).
 * wave [batch, n_samples] f32 (row stride wave_stride), window [win] f32, banks [nmel, nfft/2+1] f32 (host-built, device
 * resident), out [batch, target_len, nmel] f32.  Parity unpinned: torchaudio is not available to check against. */
int vl_kaldi_fbank(const float* wave, long wave_stride, int batch, long n_samples, const float* window, const float* banks,
                   float* out, int target_len, int win, int shift, int nfft, int nmel, float preemph, float mean, float std,
                   hipStream_t stream);
/* Windowed-sinc polyphase resampler = torchaudio.functional.resample at its defaults (sinc_interp_hann, width 6, rolloff
 * 0.99; csrc/vl_audio_train.hip; parity unpinned like the filterbank).  o = orig / gcd, n = new / gcd.  in [batch, n_in] f32
 * (row stride in_stride); offsets int32 [n] and taps f32 [n, K], K = 2W + 1: the compact per-phase table of
 * vitlens_hip/audio.py sinc_resample_table - output j = i n + p reads the inputs i o - W + offsets[p] + k, k < K, zeros
 * outside [0, n_in).  out [batch, n_out] f32 (row stride out_stride) receives the output samples out_first ..
 * out_first + n_out - 1 of the ceil(n n_in / o) a whole-row call gives, bit-identical to them.  Refused: a window outside
 * that range, an even K, a ratio whose o is so large that one tile's input span does not fit the staging buffer. */
int vl_resample_sinc(const float* in, long in_stride, int batch, long n_in, const int* offsets, const float* taps, int o, int n,
                     int K, float* out, long out_stride, long out_first, long n_out, hipStream_t stream);
/* The training transform after the filterbank (ASTProcessorTrain, at_processor.py:336-362) in one pass, out of place:
 *   out[b, (t + roll) mod T, f] = ((masked ? 0 : in[b, t, f]) - mean) / std + amp * u(seed_b, t, f)
 * in / out [batch, T, F] f32; params: per sample 32 bytes {int32 f0, fw, t0, tw; float amp; int32 roll; uint64 seed}: masks
 * [f0, f0 + fw) over f and [t0, t0 + tw) over t, roll any integer.  u in [0, 1) = (bits >> 8) 2^-24 of Philox4x32-10 keyed
 * by seed, counter = (t F + f) / 4, word (t F + f) % 4. */
int vl_fbank_augment(const float* in, float* out, int batch, int T, int F, const void* params, float mean, float std,
                     hipStream_t stream);
/* The training clips of a batch, with audio mix-up, in one launch from recordings on the device (csrc/vl_audio_mix.hip):
 * audio_get_clip (at_processor.py:193-224) and `mix = lam * wf + (1 - lam) * sec_wf; mix -= mix.mean()`
 * (open_clip/modal_audio/datasets.py:279-326).  src: packed f32 [src_floats]; source i is C_i rows of L_i samples at float
 * offset off_i, any offset (no alignment is asked for; a row that sits on a 16-byte boundary is read 16 bytes at a time).
 * out [batch, n] f32; means (may be NULL: the same out) [batch, 3] f32 = mA, mB, mM (0 where there is no partner).
 * recs: DEVICE array of one 40-byte record per output row, 10 little-endian 32-bit words:
 *     words 0 .. 3   int32 off_a, ch_a, len_a, start_a     clip A: ch_a rows of len_a samples at src + off_a
 *     words 4 .. 7   int32 off_b, ch_b, len_b, start_b     the partner; ch_b = 0: none
 *     words 8 .. 9   float lam, mu                         float32 roundings of lambda and of the double 1 - lambda
 * Clip A is a[c][t] = src[off_a + c len_a + (start_a + t) mod len_a], t < n (the repeated doubling of a short cut is a
 * periodic extension, the crop a shift), clip B likewise.  Every step below is one float32 operation, nothing contracted:
 *   mA = mean over the ch_a n elements of a,  a' = a - mA;            no partner: out[t] = a'[0][t]
 *   mB, b' likewise;  m[c][t] = (lam a'[ca][t]) + (mu b'[cb][t]) with torch's broadcast over channels (ch_a == ch_b, or
 *   one of them 1);  mM = mean over the max(ch_a, ch_b) n elements of m;  out[t] = m[0][t] - mM     (channel 0 only: the
 *   filterbank reads channel 0).
 * A mean is a sum in the fixed order csrc/vl_audio_mix.hip states (at most ceil(ceil(N / 4) / 256) + 10 additions on any
 * element's way, N the element count), divided by float(N): two calls give the same bits.
 * Refused with a status, nothing launched: a null src / recs / out, batch < 1, n or src_floats outside [1, 2^31 - 1].  The
 * records live in device memory, where the entry cannot look at them: a row whose record has len < 1, ch < 1, start
 * outside [0, len), an offset with [off, off + ch len) outside [0, src_floats), ch n > 2^31 - 1 or channel counts that do
 * not broadcast is refused by the kernel - nothing of that row of out and means is written, and no address outside src is
 * read - and where the records are packed on the host (vitlens_hip.audio.wave_clip_mix: ValueError, no launch).
 * NOTE on the version: like vl_pc_augment, these entries were added under VL_ABI_VERSION 610, which tests/test_linprobe_host.py
 * pins: a library built before them reports the same number and lacks the symbols, and a client must look them up when it
 * loads the library (vitlens_hip/_lib.py does, and names such a library as stale). */
int vl_wave_clip_mix(const float* src, long src_floats, const void* recs, float* out, float* means, int batch, long n,
                     hipStream_t stream);
/* The same mix of two samples' frames (datasets.py:318-321), rows f32 [rows, n]: out[r] = a[r] bit for bit where
 * partner[r] < 0, else out[r][i] = (lam_r a[r][i]) + (mu_r b[partner[r]][i]), three float32 roundings, nothing contracted.
 * partner int32 [rows] (DEVICE; an index >= rows leaves the row of out unwritten - the host wrapper refuses it), lam_mu f32
 * [rows, 2].  out may alias a, not b.  Refused: a null operand, rows or n < 1, n > 65535 * 1024, out == b. */
int vl_mix_rows(const float* a, const float* b, const int* partner, const float* lam_mu, float* out, int rows, long n,
                hipStream_t stream);
/* ---- point-cloud tokenizer (PointBERT grouping) ---- */
/* farthest point sampling: xyz [B,N,3] f32, start [B] (the reference draws it with torch.randint, misc.py:60);
 * idx [B,G] int64 (bit-exact vs misc.fps), centers [B,G,3] optional. */
int vl_fps(const float* xyz, const int64_t* start, int64_t* idx, float* centers, int B, int N, int G, hipStream_t stream);
/* pc_norm after a gather (modal_3d/processors/pc_processor.py:32-38, PCProcessorEval :60-88): out [B,G,C] f32 =
 * (pts[b, idx[b,g], :] - centroid) / max distance from the centroid over the G selected points; idx NULL = all N points. */
int vl_pc_gather_normalize(const float* pts, const int64_t* idx, float* out, int B, int N, int G, int C, hipStream_t stream);
/* The training transform of the 3D recipes after the sampling (csrc/vl_pc_augment.hip), one launch per batch, out of place:
 * ViT-Lens' pc_norm + random_point_dropout + random_scale / shift / rotate_perturbation / rotate_point_cloud
 * (open_clip/modal_3d/datasets.py:97-204, 471-479) and OpenShape's normalize_pc + augment_pc + random_rotate_z + colour drop
 * (VitLens-OpenShape/src/data.py:74-88).  pts [B,N,C] f32, 3 <= C <= 8, xyz first; idx [B,G] int64 (vl_fps' result or a
 * random subset; an index outside [0, N) is clamped into it), NULL = all points (then G == N); out [B,G,C] f32.
 * params: DEVICE array of one 64-byte record per sample, 16 little-endian 32-bit words:
 *     words  0 ..  8   float A[9]       row-major 3x3
 *     words  9 .. 11   float t[3]
 *     word  12         float drop_ratio in [0, 1], or -1: nothing is dropped (0 still drops a point whose u is 0)
 *     word  13         int32 flags      1 = normalise, 2 = normalize_pc's guard, 4 = fill the feature channels
 *     words 14 .. 15   uint64 seed
 * Output point j of sample b, in this order:
 *   1. p = pts[b, idx[b,j], :]
 *   2. flags & 1: xyz = (xyz - mean) / r, mean and r = largest distance from it over the G selected points; with flags & 2
 *      as well r < 1e-6 gives xyz = 0 (normalize_pc), without it the division is done as it comes (pc_norm)
 *   3. u_j = (w >> 8) 2^-24, w = word j % 4 of Philox4x32-10 with key (lo32(seed), hi32(seed)), counter (j / 4, 0, 0, 0);
 *      u_j <= drop_ratio (fp32, the reference's <=): the point takes the xyz of output point 0 after step 2
 *   4. xyz_out[c] = fma(x, A[c], fma(y, A[3 + c], fma(z, A[6 + c], t[c])))      (xyz . A + t)
 *   5. channels 3 .. C-1 are copied, or all set to feat_fill with flags & 4
 * Refused with a status, nothing launched: a bad shape, a null pts / out / params, idx NULL with G != N, pts == out.  The
 * records live in device memory, where the entry cannot look at them without a read-back: a drop_ratio outside [0, 1] (but
 * -1) is refused where the records are packed on the host (vitlens_hip.ops.pc_augment_params); the kernel's comparison is
 * defined for every value.  Stream-ordered, no global state, no host synchronisation.
 * NOTE on the version: like the four Perceiver-dropout entries above, this entry was added under VL_ABI_VERSION 610, which
 * tests/test_linprobe_host.py pins: a library built before it reports the same number and lacks the symbol, and a client must
 * look it up when it loads the library (vitlens_hip/_lib.py does, and names such a library as stale). */
int vl_pc_augment(const float* pts, const int64_t* idx, float* out, int B, int N, int G, int C, const void* params,
                  float feat_fill, hipStream_t stream);
/* The training transform of the depth recipe (csrc/vl_rgbd_augment.hip), one call per batch of n RGB-D samples of any sizes:
 * ToTensor + DepthNorm + RandomResizedCrop(S, bilinear) + RandomHorizontalFlip + ColorJitter3d + RandomErasing + Normalize
 * (modal_depth/processors/vt_processor.py:94-207; RandAugment3d leaves a 4-channel tensor as it is).  out_rgb [n,3,S,S] and
 * out_depth [n,1,S,S] f32.  Every random scalar is drawn by the host and arrives in the sample's record.
 * records: DEVICE array of one 136-byte record per sample, 34 little-endian 32-bit words:
 *     words  0 ..  1   uint64 rgb          device pointer, uint8 [H,W,3]
 *     words  2 ..  3   uint64 depth        device pointer, float32 [H,W]
 *     word   4         int32 rgb_stride    bytes per row of rgb
 *     word   5         int32 depth_stride  floats per row of depth
 *     words  6 ..  7   int32 H, W
 *     words  8 .. 11   int32 top, left, bh, bw     the crop box, inside the image
 *     words 12 .. 13   int32 row0, nrows   the rows of the box, counted from top, that the vertical taps touch
 *     words 14 .. 16   int32 hb, hw, hks   horizontal table (bw -> S): offsets of its bounds [S,2] int32 and weights [S,hks]
 *                                          f32 in `tables`, counted in 32-bit words, and the taps per row
 *     words 17 .. 19   int32 vb, vw, vks   the same for the vertical table (bh -> S)
 *     words 20 .. 21   int64 tmp           offset of the sample's [nrows,S] intermediate in `tmp`, counted in float4
 *     word  22         int32 flags         1 flip, 2 brightness, 4 contrast, 8 saturation, 16 hue (the term is applied),
 *                                          32 erase; bits 8 .. 15: the order of the four terms, two bits per position,
 *                                          first position lowest (0 brightness, 1 contrast, 2 saturation, 3 hue)
 *     words 23 .. 28   float b, 1-b, c, 1-c, s, 1-s        the factors; 1 - f is formed in double on the host
 *     word  29         float hue           the hue shift
 *     words 30 .. 33   int32 ei, ej, eh, ew        the erase rectangle: rows [ei, ei+eh), columns [ej, ej+ew) of the output
 * Taps are relative to the box and clamped into it; tables: the packed per-axis tables of the distinct (size -> S) pairs;
 * tmp: sum of nrows * S float4, 16-byte aligned; max_nrows: the largest nrows; mean / stdv: HOST arrays of 4 floats (RGB,
 * depth); depth is read as min(max(d, depth_lo), depth_hi) / depth_div.  Per sample, in this order: resample (a flipped
 * sample's output column x takes the table row of S-1-x), the enabled jitter terms in the record's order (contrast blends
 * with the mean of 0.2989 R + 0.587 G + 0.114 B over the sample as it is at that point, summed in a fixed order), the erase
 * (all four channels become 0), (x - mean[c]) / stdv[c].  A sample's result does not depend on its place in the batch.
 * Refused with a status, nothing launched: n outside [1, 65535], S outside [1, 4096], max_nrows < 1, a null operand, records
 * not 8-byte or tmp not 16-byte aligned, a zero stdv or depth_div.  The records live in device memory: their contents are
 * checked where they are packed on the host (vitlens_hip.ops.rgbd_augment_pack); in the kernels a row or column outside
 * the image is clamped into it.  Stream-ordered, three launches, no global state, no host synchronisation.
 * NOTE on the version: like vl_pc_augment, this entry was added under VL_ABI_VERSION 610, which tests/test_linprobe_host.py
 * pins: a library built before it reports the same number and lacks the symbol, and a client must look it up when it loads
 * the library (vitlens_hip/_lib.py does, and names such a library as stale). */
int vl_rgbd_augment(const void* records, int n, int S, int max_nrows, const void* tables, float* tmp, const float* mean,
                    const float* stdv, float depth_lo, float depth_hi, float depth_div, float* out_rgb, float* out_depth,
                    hipStream_t stream);
/* The plain-image training transform of the tactile and EEG recipes (csrc/vl_image_augment.hip), one call per batch of n RGB
 * images of any sizes: RandomResizedCrop(S, bilinear) + RandomHorizontalFlip + RandAugment on the 8-bit image, every stage
 * byte for byte the Pillow call it ends in, then ToTensor + ColorJitter + Normalize (modal_eeg/processors/eeg_processor.py:
 * 93-139).  out [n,3,S,S] f32; out_u8 (may be NULL) [n,S,S,3]: the 8-bit image after RandAugment.  Every random scalar is
 * drawn by the host and arrives in the sample's record.
 * records: DEVICE array of one 368-byte record per sample, 92 little-endian 32-bit words:
 *     words  0 ..  1   uint64 src          device pointer, uint8 [H,W,3]
 *     word   2         int32 stride        bytes per row of src
 *     words  3 ..  4   int32 H, W
 *     words  5 ..  8   int32 top, left, bh, bw     the crop box, inside the image
 *     words  9 .. 10   int32 row0, nrows   the rows of the box, counted from top, that the vertical taps touch
 *     words 11 .. 13   int32 hb, hk, hks   horizontal table (bw -> S): offsets of its bounds [S,2] int32 and coefficients
 *                                          [S,hks] int32 (22-bit fixed point) in `tables`, in 32-bit words; taps per row
 *     words 14 .. 16   int32 vb, vk, vks   the same for the vertical table (bh -> S)
 *     word  17         int32 flags         1 flip, 2 brightness, 4 contrast, 8 saturation, 16 hue (the jitter term is applied);
 *                                          bits 8 .. 15: the order of the four terms, two bits per position, first position
 *                                          lowest (0 brightness, 1 contrast, 2 saturation, 3 hue)
 *     words 18 .. 19   int64 tmp           offset of the sample's [nrows,S,3] intermediate in `tmp`, in bytes
 *     words 20 .. 25   float b, 1-b, c, 1-c, s, 1-s        the jitter factors; 1 - f is formed in double on the host
 *     word  26         float hue           the hue shift
 *     word  27         int32 num_ops       RandAugment ops of this sample, 0 .. 4
 *     words 28 .. 91   four 64-byte op slots, applied in order:
 *         word  0      int32 code          0 Identity, 1 ShearX, 2 ShearY, 3 TranslateX, 4 TranslateY, 5 Rotate, 6 Brightness,
 *                                          7 Color, 8 Contrast, 9 Sharpness, 10 Posterize, 11 Solarize, 12 AutoContrast, 13 Equalize
 *         word  1      int32 ipay          Posterize: the mask a byte is and-ed with; Solarize: bytes >= it become 255 - byte
 *         word  2      float fpay          6 .. 9: the factor of ImageEnhance.*.enhance
 *         word  3      unused
 *         words 4 .. 15  double m[6]       1 .. 5: the matrix of Image.transform(AFFINE, BILINEAR), output pixel centre to source
 * tables: the packed per-axis tables of the distinct (edge -> S) pairs; tmp: sum of nrows * S * 3 bytes; max_nrows: the largest
 * nrows; work: 2 * n * S * S * 3 bytes (each sample's two images); max_ops: the largest num_ops of the batch, which the
 * kernels do not read (each sample runs its record's num_ops, clamped to [0, 4]): it is a parameter only so that a batch with
 * more than 4 ops per sample is refused here, on the host, where the records cannot be read; mean / stdv:
 * HOST arrays of 3 floats.  Per sample, in this order: Pillow's two-pass 8-bit resampler over the box (a flipped sample's
 * column x reads column S-1-x), the ops (the affine position and blend in doubles, the enhance blends and the SMOOTH filter in
 * float32, nothing contracted, Pillow's truncation; Contrast blends with int(mean(L) + 0.5); AutoContrast and Equalize build
 * their LUTs from the per-channel histograms), byte / 255, the enabled jitter terms in the record's order (contrast blends
 * with the mean of 0.2989 R + 0.587 G + 0.114 B, summed in a fixed order), (x - mean[c]) / stdv[c].  A sample's result does
 * not depend on its place in the batch.
 * Refused with a status, nothing launched: n outside [1, 65535], S outside [1, 4096], max_nrows < 1, max_ops outside [0, 4], a
 * null operand (out_u8 may be null), records not 8-byte aligned, a zero stdv.  The records live in device memory: their
 * contents (op codes, finite matrices, the box, the order field, the table and intermediate offsets against the sizes of
 * `tables` and `tmp`) are checked where they are packed on the host (vitlens_hip.ops.image_augment_pack); in the kernels an index outside the box or the image is clamped into it and an unknown
 * op code is skipped.  Stream-ordered, three launches, no global state, no host synchronisation.
 * vl_image_crop_resize_u8 is the first two launches alone: out_u8 [n,S,S,3] = img.crop(box).resize((S, S), BILINEAR), flipped
 * where the record says so.
 * NOTE on the version: like vl_pc_augment, these entries were added under VL_ABI_VERSION 610, which tests/test_linprobe_host.py
 * pins: a library built before them reports the same number and lacks the symbols, and a client must look them up when it
 * loads the library (vitlens_hip/_lib.py does, and names such a library as stale). */
int vl_image_crop_resize_u8(const void* records, int n, int S, int max_nrows, const void* tables, uint8_t* tmp, uint8_t* out_u8,
                            hipStream_t stream);
int vl_image_augment(const void* records, int n, int S, int max_nrows, int max_ops, const void* tables, uint8_t* tmp,
                     uint8_t* work, const float* mean, const float* stdv, float* out, uint8_t* out_u8, hipStream_t stream);
/* The training transform of the tactile recipe (csrc/vl_tactile_augment.hip), one call per batch of n RGB images of any sizes:
 * ToTensor + RandomResizedCrop(S, bilinear) + RandomHorizontalFlip + RandomVerticalFlip + RandomRotation(nearest, fill 0) +
 * Normalize, all on the float tensor (modal_tactile/processors/tact_processor.py:189-233).  out [n,3,S,S] f32.  Every random
 * scalar is drawn by the host and arrives in the sample's record.
 * records: DEVICE array of one 96-byte record per sample, 24 little-endian 32-bit words:
 *     words  0 ..  1   uint64 src          device pointer, uint8 [H,W,3]
 *     word   2         int32 stride        bytes per row of src
 *     words  3 ..  4   int32 H, W
 *     words  5 ..  8   int32 top, left, bh, bw     the crop box, inside the image
 *     words  9 .. 10   int32 row0, nrows   the rows of the box, counted from top, that the vertical taps touch
 *     words 11 .. 13   int32 hb, hw, hks   horizontal table (bw -> S): offsets of its bounds [S,2] int32 and weights [S,hks]
 *                                          f32 in `tables`, counted in 32-bit words, and the taps per row
 *     words 14 .. 16   int32 vb, vw, vks   the same for the vertical table (bh -> S)
 *     word  17         int32 flags         bit 0 horizontal flip, bit 1 vertical flip
 *     words 18 .. 19   int64 tmp           offset of the sample's [nrows,S] intermediate in `tmp`, counted in float4
 *     words 20 .. 23   float t00, t01, t10, t11    the rotation: entries 0, 1, 3, 4 of torchvision's inverse affine matrix for
 *                                          -angle about the centre, rounded to float32 and divided in float32 by
 *                                          float32(0.5 S) (its rescaled theta; entries 2 and 5 are 0)
 * Taps are relative to the box and clamped into it; tables: the packed per-axis tables of the distinct (edge -> S) pairs;
 * tmp: sum of nrows * S float4, 16-byte aligned; max_nrows: the largest nrows; mean / stdv: HOST arrays of 3 floats.  Per
 * output pixel (x, y), in float32 with every operation rounded on its own: xb = x - S/2 + 0.5, yb likewise, gx = xb t00 +
 * yb t01, gy = xb t10 + yb t11, ix = ((gx + 1) S - 1) / 2, iy likewise, sx = rint(ix), sy = rint(iy) (half to even).  With sx
 * or sy outside [0, S) the pixel is (0 - mean[c]) / stdv[c].  Otherwise it is pixel (row sy or, vertically flipped, S-1-sy;
 * column sx or, horizontally flipped, S-1-sx) of the box resized to S x S, (v - mean[c]) / stdv[c]; that value has the same
 * bits whichever output pixel takes it.  A sample's result does not depend on its place in the batch.
 * Refused with a status, nothing launched: n outside [1, 65535], S outside [1, 4096], max_nrows < 1, a null operand, records
 * not 8-byte or tmp not 16-byte aligned, a zero stdv.  The records live in device memory: their contents are checked where
 * they are packed on the host (vitlens_hip.ops.tactile_augment_pack); in the kernels a row or column outside the image is
 * clamped into it.  Stream-ordered, two launches, no global state, no host synchronisation.
 * NOTE on the version: like vl_pc_augment, this entry was added under VL_ABI_VERSION 610, which tests/test_linprobe_host.py
 * pins: a library built before it reports the same number and lacks the symbol, and a client must look it up when it loads
 * the library (vitlens_hip/_lib.py does, and names such a library as stale).  No existing entry changes. */
int vl_tactile_augment(const void* records, int n, int S, int max_nrows, const void* tables, float* tmp, const float* mean,
                       const float* stdv, float* out, hipStream_t stream);
/* ---- evaluation-time image / depth preprocessing (csrc/vl_preproc.hip) ----
 * Separable bicubic resampling restricted to a crop window, tables built by the host (vitlens_hip/preproc.py):
 * bounds [n_out,2] int32 = (first tap, tap count) and coefficients [n_out,ksize] per OUTPUT index of the full resized
 * axis; xout0/nxout (yout0/nyout) select the crop.  8-bit path = Pillow's Image.resize(BICUBIC) (22-bit fixed-point
 * int32 taps, 8-bit intermediate; byte-exact), replacing torchvision Resize+CenterCrop+ToTensor+Normalize of
 * open_clip/transform.py:138-155: the vertical pass writes out [C,nyout,W] f32 = (u8/255 - mean[c]) / std[c] (mean/std:
 * HOST arrays of C floats) and/or the resized bytes out_u8 [nyout,W,C]; W = source width of the horizontal pass, and in
 * the vertical pass src is the [nrows, W, C] intermediate whose row 0 is image row row0 (nothing beyond it is read).  Float path = ATen bicubic (antialiased or the
 * 4-tap border-clamped form) with DepthNorm's clamp(lo,hi)/divide_by fused into the read, replacing
 * modal_depth/processors/vt_processor.py:292-337; taps are clamped to the image, so bounds may start at -1. */
int vl_resample_h_u8(const uint8_t* src, long row_stride, int W, int C, int row0, int nrows, const int* bounds,
                     const int* kk, int ksize, int xout0, int nxout, uint8_t* dst, hipStream_t stream);
int vl_resample_v_u8_norm(const uint8_t* src, int W, int C, int row0, int nrows, const int* bounds, const int* kk,
                          int ksize, int yout0, int nyout, const float* mean, const float* stdv, float* out,
                          uint8_t* out_u8, hipStream_t stream);
/* The 8-bit path for a LIST of images of different sizes in two launches (blockIdx.z = image).  desc: device array
 * [n][16] int64 per image = {src pointer, row stride in bytes, source width, row0, nrows, xout0, yout0, horizontal
 * bounds offset, horizontal coefficient offset, horizontal ksize, vertical bounds offset, vertical coefficient offset,
 * vertical ksize, byte offset of the image's [nrows, crop_w, C] intermediate in tmp, 0, 0}; offsets count ints into
 * `tables` (the per-axis bounds / coefficient tables of the distinct sizes, packed).  out [n, C, crop_h, crop_w] f32. */
int vl_resample_batch_u8_norm(const int64_t* desc, int n, int C, int crop_h, int crop_w, int max_nrows, const int* tables,
                              uint8_t* tmp, const float* mean, const float* stdv, float* out, hipStream_t stream);
int vl_resample_h_f32(const float* src, long row_stride, int W, int row0, int nrows, const int* bounds,
                      const float* weights, int ksize, int xout0, int nxout, int clamp_on, float clamp_lo,
                      float clamp_hi, float divide_by, float* dst, hipStream_t stream);
int vl_resample_v_f32_norm(const float* src, int W, int H, int row0, const int* bounds, const float* weights, int ksize,
                           int yout0, int nyout, float mean, float stdv, float* out, hipStream_t stream);
/* k nearest neighbours of each centre (set semantics = topk(sorted=False), dvae.py:107-118) + gather +
 * centre subtraction: nidx [B,G,k] int32 optional, patches bf16 [B*G*k, Kp] optional (xyz in cols 0..2). */
int vl_knn_group(const float* xyz, const int64_t* center_idx, int* nidx, void* patches, int B, int N, int G,
                 int k, int Kp, hipStream_t stream);
/* Ball query + grouping of the `pnsa` tokenizer (query_ball_point + sample_and_group,
 * open_clip/modal_3d/models/pointnet/pointnet_util.py:101-161): for every centre center_idx[b,s] the first `nsample`
 * point indices in ascending order with -2ab+|a|^2+|b|^2 <= radius2 (short groups repeat their first index) -> idx
 * [B,S,nsample] int32 (optional) and patches [B*S*nsample, Kp] bf16 (optional) = (xyz_j - centre, feats[b,j,0:D], 0...):
 * the rows of the first 1x1 convolution.  xyz [B,N,3] f32, feats [B,N,D] f32 or NULL with D = 0. */
int vl_ball_group(const float* xyz, const float* feats, const int64_t* center_idx, int* idx, void* patches, int B, int N,
                  int S, int D, float radius2, int nsample, int Kp, hipStream_t stream);
int vl_group_max(const void* x, long ldx, void* out, int out_dtype, long ldo, long groups, int M, int C, hipStream_t stream);
int vl_pad3_bf16(const float* c, void* out, long R, int Kp, hipStream_t stream);
/* ---- trainable point tokenizer: nn.BatchNorm1d over [R = B*G*M, C] bf16 activations (dvae.py:184-194) ----
 * ws: caller workspace of (nchunk + 1) * 2 * C floats (row-chunk partial sums; deterministic, no atomics).
 * vl_bn_stats: biased batch mean/var per column; running_mean/var (optional) updated as nn.BatchNorm1d does
 * (momentum, unbiased variance).  vl_bn_apply: y = gamma*(x-mean)/sqrt(var+eps)+beta (+ReLU); pass the batch
 * statistics (train) or the running statistics (eval).  vl_bn_bwd: dgamma/dbeta are ACCUMULATED; dx (optional)
 * is the input gradient; train=0 treats mean/var as constants (eval-mode BN). */
int vl_bn_stats(const void* x, long ldx, int R, int C, float* ws, int nchunk, float* mean, float* var,
                float* running_mean, float* running_var, float momentum, hipStream_t stream);
/* SyncBatchNorm (torch.nn.SyncBatchNorm under --use-bn-sync, training/point_cloud/pc_tri_main.py:372-373): the two
 * passes above split where the ranks exchange data.  Forward: vl_bn_stats_local -> local [2C+1] floats = per-column
 * mean, M2 = sum (x-mean)^2, and the row count as int bits; all-gather to [W, 2C+1]; vl_bn_stats_merge -> global
 * mean / biased var (+ running statistics with the global unbiased variance) and *total = global row count.
 * Backward: vl_bn_bwd_reduce accumulates dgamma/dbeta (local, as SyncBatchNorm does) and writes sums [2C] =
 * (sum dy', sum dy'*xhat); all-reduce(sum) them; vl_bn_bwd_apply -> dx with the global sums and count. */
int vl_bn_stats_local(const void* x, long ldx, int R, int C, float* ws, int nchunk, float* local, hipStream_t stream);
int vl_bn_stats_merge(const float* gathered, int W, int C, float* mean, float* var, float* running_mean,
                      float* running_var, float momentum, int* total, hipStream_t stream);
int vl_bn_bwd_reduce(const void* dy, long lddy, const void* x, long ldx, const float* mean, const float* var,
                     const float* gamma, const float* beta, float eps, int relu, float* ws, int nchunk, float* dgamma,
                     float* dbeta, float* sums, int R, int C, hipStream_t stream);
int vl_bn_bwd_apply(const void* dy, long lddy, const void* x, long ldx, const float* mean, const float* var,
                    const float* gamma, const float* beta, float eps, int relu, const float* sums, const int* total,
                    void* dx, long lddx, int R, int C, hipStream_t stream);
int vl_bn_apply(const void* x, long ldx, const float* mean, const float* var, const float* gamma, const float* beta,
                float eps, int relu, void* out, long ldo, long R, int C, hipStream_t stream);
int vl_bn_bwd(const void* dy, long lddy, const void* x, long ldx, const float* mean, const float* var,
              const float* gamma, const float* beta, float eps, int relu, int train, float* ws, int nchunk,
              float* dgamma, float* dbeta, void* dx, long lddx, int R, int C, hipStream_t stream);
/* backward of torch.max over the M rows of each group (gradient to the first arg-max row), added to `base`
 * (optional); and the sum over the M rows of each group (backward of the expand in dvae.py:207-208). bf16. */
int vl_group_max_bwd(const void* f, long ldf, const void* dg, long lddg, const void* base, long ldb, void* out,
                     long ldo, long groups, int M, int C, hipStream_t stream);
int vl_group_sum(const void* x, long ldx, void* out, long ldo, long groups, int M, int C, hipStream_t stream);
/* torch.optim.AdamW step on one tensor (grad is multiplied by grad_scale first); step counts from 1. */
int vl_adamw_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int step, float grad_scale, hipStream_t stream);
/* Squared 2-norm of a contiguous fp32 buffer, written to ONE device float: out[0] = sum_i x[i]^2.  Any n >= 0 (n = 0 writes
 * 0), any 4-byte-aligned x.  Two stages on a grid that depends on n alone, combined in a fixed order: two calls on the same
 * input agree bit for bit (no floating-point atomics).  The squares are accumulated in fp64 and rounded to fp32 once, so the
 * result is the correctly rounded sum up to the fp64 accumulation error; NaN and +-inf propagate as in
 * torch.linalg.vector_norm (a sum beyond FLT_MAX is +inf).  ws: vl_sumsq_ws_floats() floats from the caller, 8-byte aligned.
 * With vl_adamw_multi_step this is torch.nn.utils.clip_grad_norm_(norm_type=2) without a host read of the norm. */
long vl_sumsq_ws_floats(void);
int vl_sumsq_f32(const float* x, long n, float* out, float* ws, hipStream_t stream);
/* One slot of vl_adamw_multi_step's device table: one tensor of the optimizer (48 bytes, no padding besides `reserved`). */
typedef struct vl_adamw_slot {
  float* p; const float* g; float* m; float* v;  /* parameter, gradient, first and second moment: n contiguous floats each */
  long n;
  float weight_decay;                           /* per tensor: the no-decay group passes 0 */
  int reserved;                                 /* 0 */
} vl_adamw_slot;
#define VL_ADAMW_MAX_SLOTS 1024
/* vl_adamw_step on EVERY tensor of a table in ONE launch, with torch.nn.utils.clip_grad_norm_ folded in:
 *   coef = min(1, max_norm / (grad_scale * sqrt(sumsq[0]) + 1e-6))       derived on the device by every thread
 *   update of vl_adamw_step applied to g * grad_scale * coef             (the same __device__ function: with coef == 1 the
 *                                                                         two entries produce the same bits)
 * sumsq: device float, the squared norm of ALL gradients of the table as vl_sumsq_f32 leaves it (so grad_scale * sqrt(sumsq)
 * is the norm of the gradient the optimizer sees - DDP's mean with grad_scale = 1 / world).  A NaN norm gives a NaN
 * coefficient (clip_grad_norm_ with error_if_nonfinite=False).  The host never reads the norm or the coefficient.
 * slots: DEVICE array of nslots <= VL_ADAMW_MAX_SLOTS entries; the work is split by element over the whole table (tiles of
 * 2048 elements dealt to the workgroups), not by tensor.  norm_out: optional device float, receives the UNCLIPPED norm
 * grad_scale * sqrt(sumsq).  max_norm > 0. */
int vl_adamw_multi_step(const vl_adamw_slot* slots, int nslots, float lr, float beta1, float beta2, float eps, int step,
                        float grad_scale, float max_norm, const float* sumsq, float* norm_out, hipStream_t stream);
/* What vl_adamw_multi_step_groups adds to slot s of the table, in an array of its own beside it (8 bytes per tensor). */
typedef struct vl_adamw_group {
  float lr_scale;                               /* the tensor steps with lr * lr_scale (parameter groups with their own lr) */
  int no_clip;                                  /* 1: outside clip_grad_norm_'s parameter list - the tensor sees coef = 1 */
} vl_adamw_group;
/* vl_adamw_multi_step with parameter groups: slot s steps with lr * groups[s].lr_scale (an fp32 product), and a slot with
 * no_clip set is updated with coef = 1.  sumsq is then the squared norm of the gradients of the CLIPPED tensors only (lay them
 * out contiguously and it is one vl_sumsq_f32 call); norm_out receives grad_scale * sqrt(sumsq), the unclipped norm of that set.
 * groups: DEVICE array of nslots entries, read per slot like weight_decay; groups_host: the HOST array the caller uploaded it
 * from, which this entry checks (lr_scale finite and >= 0, no_clip 0 or 1) before anything is launched - the device is never
 * read back.  With every lr_scale == 1.0f and no exempt tensor the results are the bits of vl_adamw_multi_step. */
int vl_adamw_multi_step_groups(const vl_adamw_slot* slots, const vl_adamw_group* groups, const vl_adamw_group* groups_host,
                               int nslots, float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                               float max_norm, const float* sumsq, float* norm_out, hipStream_t stream);
int vl_clamp_scalar(float* p, float lo, float hi, hipStream_t stream);
/* p[i] = value for i < n (fp32; the accumulators of a step start from zero without a framework fill). */
int vl_fill_f32(float* p, float value, long n, hipStream_t stream);
int vl_axpy_f32(float* y, const float* x, float alpha, long n, hipStream_t stream);
/* out[i] = x[i] * exp(log_scale[0]) * mul (in place allowed): `logit_scale.exp()` (open_clip/model.py:619, loss.py:125-127)
 * applied on the device, so that a training step never reads the temperature on the host (hipGraph-capturable). */
int vl_scale_exp_f32(const float* x, float* out, long n, const float* log_scale, float mul, hipStream_t stream);
/* out[t,:] += sum_b x[b*batch_stride_rows + row_offset + t, :]   (positional-embedding gradients) */
int vl_batch_rowsum(const float* x, float* out, int B, int T, int D, long batch_stride_rows, long row_offset,
                    hipStream_t stream);

/* ---- the linear probe (open_clip/linprobe_model.py ViTLensLP; training/optimizer.py LARS; csrc/vl_linprobe.hip) ----
 * A frozen tower's pooled rows -> Dropout(p) -> BatchNorm1d(D, affine=False, eps) -> Linear(D, C), label cross-entropy, LARS.
 * The Linear and its dW are vl_gemm_f32; these entries are the rest.  All fp32 in and out, fp64 accumulators, every reduction
 * in a fixed order: two calls on the same input agree bit for bit.
 *
 * vl_lp_bn_fwd: x f32 [B, ldx >= D] -> xhat f32 [B, ldh >= D], and optionally its transpose xhatT f32 [D, ldt] (ldt % 4 == 0,
 * ldt >= B, columns B .. ldt-1 written as zeros: dW is then one vl_gemm_f32 with K = ldt).  D % 4 == 0, ldx % 4 == ldh % 4 == 0,
 * x and xhat 16-byte aligned; B up to 65536 and beyond.
 *   train = 1: x' = dropout(x): a kept element is x * (1 / (1 - p)), a dropped one 0.  The mask is keep u8 [B, D] (contiguous,
 *     4-byte aligned, non-zero = kept) when given; with keep == NULL and p > 0 element (b, d) is dropped when word d & 3 of
 *     Philox4x32-10 with counter (d >> 2, lo32(sample0 + b), hi32(sample0 + b), 0) and key (lo32(seed), hi32(seed)) is below
 *     (uint32_t)(p * 2^32) - a batch cut into pieces draws the same mask; with p == 0 no mask is read.  Then per column the batch
 *     mean and the BIASED variance (two passes: mean, then squared deviations), xhat = (x' - mean) / sqrt(var + eps), mean[D]
 *     and var[D] (optional outputs), and, when given, running = (1 - momentum) running + momentum {mean, var B / (B - 1)} as
 *     nn.BatchNorm1d.  B < 2 is refused.
 *   train = 0: no dropout; xhat = (x - running_mean) / sqrt(running_var + eps); nothing else is written. */
int vl_lp_bn_fwd(const float* x, long ldx, const uint8_t* keep, float p, uint64_t seed, int64_t sample0, int train,
                 float* running_mean, float* running_var, float momentum, float eps, float* xhat, long ldh, float* xhatT,
                 long ldt, float* mean, float* var, int B, int D, hipStream_t stream);
/* vl_ce_label: torch.nn.CrossEntropyLoss() (mean) over logits f32 [B, ld >= C] and target int64 [B], any C >= 1 (max-subtracted):
 *   loss[0] = mean_b (lse_b - logits[b, target_b]);  optional G f32 [B, ldg >= C] = gscale (softmax - onehot) / B;  optional
 *   GT f32 [C, ldgt] = its transpose (ldgt % 4 == 0, ldgt >= B, zeros behind column B);  optional dbias f32 [C] = sum_b G[b, :].
 * The loss and dbias sums go through ws (vl_ce_label_ws_floats(B, C) floats) in two fixed-order stages.  A target outside
 * [0, C) makes that row's loss term and gradient row NaN (hence the loss and dbias); the index is clamped before any read. */
long vl_ce_label_ws_floats(int B, int C);
int vl_ce_label(const float* logits, long ld, const int64_t* target, int B, int C, float gscale, float* loss, float* G,
                long ldg, float* GT, long ldgt, float* dbias, float* ws, hipStream_t stream);
/* One slot of vl_lars_multi_step's device table (40 bytes): one tensor of the optimizer. */
typedef struct vl_lars_slot {
  float* p; const float* g; float* mu;          /* parameter, gradient, momentum buffer: n contiguous floats each */
  long n;
  float weight_decay;
  int adapt;                                    /* 1: the reference's p.ndim > 1 (weight decay + trust ratio); 0: bias */
} vl_lars_slot;
#define VL_LARS_MAX_SLOTS 1024
/* LARS.step of the reference (training/optimizer.py, from MoCo v3) on every tensor of the table:
 *   g' = g * grad_scale * clip,  clip = min(1, max_norm / (grad_scale * sqrt(sumsq[0]) + 1e-6)) if max_norm > 0 (sumsq as
 *        vl_sumsq_f32 leaves it, as for vl_adamw_multi_step), else 1 (sumsq may be NULL)
 *   adapt = 1:  dp = g' + weight_decay p;  q = trust_coefficient |p| / |dp| if both norms are > 0 else 1;  dp *= q
 *   adapt = 0:  dp = g'                    (no weight decay and no trust ratio: the reference's rule for biases)
 *   mu = momentum mu + dp;  p -= lr mu     (each operation rounded to fp32 on its own: no fused multiply-add)
 * The norms are accumulated in fp64 per 2048-element tile and combined in a fixed order; the host reads neither them nor q.
 * ws: vl_lars_ws_floats(total elements of the table, nslots) floats, 8-byte aligned; ws_floats = its size (tiles beyond it are
 * left alone instead of written out of bounds). */
long vl_lars_ws_floats(long total_elems, int nslots);
int vl_lars_multi_step(const vl_lars_slot* slots, int nslots, float lr, float momentum, float trust_coefficient,
                       float grad_scale, float max_norm, const float* sumsq, float* ws, long ws_floats, hipStream_t stream);
/* Top-k hit counts (training/zero_shot.py test_linprob_single -> accuracy(topk=(1, 5))): rank_b = #{c: logits[b,c] >
 * logits[b,t_b]} + #{c < t_b: logits[b,c] == logits[b,t_b]}; hits[0] += #{b: rank_b < k0}, hits[1] += #{b: rank_b < k1}
 * (integer adds; the caller zeroes hits); optional correct u8 [B, 2].  A NaN logit counts as not greater; a target outside
 * [0, C) is a miss (the index is clamped before the read). */
int vl_topk_hits(const float* logits, long ld, const int64_t* target, int B, int C, int k0, int k1, int* hits,
                 uint8_t* correct, hipStream_t stream);

/* ---- evaluation metrics on the device (training/zero_shot.py's drivers, open_clip/metrics/map.py; csrc/vl_eval.hip) ----
 * vl_eval_hits: vl_topk_hits with a class map, per-class counters and the arg-max.  logits f32 [B, ld >= C], target int64 [B],
 * class_map int32 [C] or NULL (identity).  Per sample b, with t = target[b]:
 *   g = map[t];  m = the best member of group g: the largest logit among {c: map[c] == g}, the lowest index on a tie;
 *   rank_b = #{c: logits[b,c] > logits[b,m]} + #{c < m: logits[b,c] == logits[b,m]}
 * All outputs are int32 and ACCUMULATE (the caller zeroes them once per evaluation; integer atomics, any order gives the same
 * counts): hits[0] += #{b: rank_b < k0}, hits[1] += #{b: rank_b < k1}; optional cls_count[C], cls_hit0[C], cls_hit1[C] indexed
 * by t; optional pred[B] = the row's arg-max, lowest index on ties (written, not accumulated).  The group-best rank is the
 * reference's cond_acc (top-k of the raw logits, predictions and target mapped, a hit if any is equal: the best member of the
 * target's group is within the top k exactly when any member is); with the identity map it is vl_topk_hits, whose conventions
 * hold: a NaN logit counts as not greater (and, where the best member and the arg-max are chosen, orders as -inf); a target
 * outside [0, C) is a miss - the index is clamped before any read and no per-class counter changes.  Any C >= 1, also C < k1.
 *
 * vl_average_precision: scores f32 [N, ld >= C], targets f32 [N, ldt >= C] (positive: > 0) -> ap f64 [C], scikit-learn's
 * average_precision_score(average=None) with tied scores grouped, from its integer form: for class c with P positives
 *   AP_c = (1 / P) sum_{positive i} #{positive j: s_j >= s_i} / #{j: s_j >= s_i}
 * Each ratio is formed in fp64 and the sum runs in a fixed order (no floating-point atomics): two calls agree bit for bit.
 * P = 0 gives AP_c = 0.0, which scikit-learn 1.7 returns with a warning (older releases gave NaN).  The entry takes RAW scores:
 * the sigmoid of open_clip/metrics/map.py is strictly monotone and is never formed; the one difference from that path is that
 * two distinct scores which float32 sigmoid collapses into a tie stay distinct here.  NaN scores are unsupported (scikit-learn
 * raises): nothing faults, the result is unspecified; +-inf order as IEEE numbers.  ws: vl_average_precision_ws_bytes(N, C)
 * bytes, 8-byte aligned (the row tiles' partial sums and counts).  Cost: O(P N) comparisons per class, no sort - O(N^2) for a
 * class where a fixed share of the samples is positive (N = 20 000, every one of 527 classes half positive: 1e11).
 *
 * vl_clip_mean_normalize: x f32 [B * n_clip, ldx >= D], the clips of a sample in consecutive rows -> out f32 [B, D] (contiguous,
 * not x) = F.normalize(x.view(B, n_clip, D).mean(1), dim=-1, eps): the clips are added in order in fp32 and divided by n_clip,
 * then vl_l2_normalize's arithmetic.  n_clip = 1 is vl_l2_normalize.  The audio evaluation's multi-clip mean.
 * NOTE on the version: like vl_pc_augment, these entries were added under VL_ABI_VERSION 610, which tests/test_linprobe_host.py
 * pins: a library built before them reports the same number and lacks the symbols, and a client must look them up when it
 * loads the library (vitlens_hip/_lib.py does, and names such a library as stale). */
int vl_eval_hits(const float* logits, long ld, const int64_t* target, const int* class_map, int B, int C, int k0, int k1,
                 int* hits, int* cls_count, int* cls_hit0, int* cls_hit1, int* pred, hipStream_t stream);
long vl_average_precision_ws_bytes(int N, int C);
int vl_average_precision(const float* scores, long ld, const float* targets, long ldt, int N, int C, double* ap, void* ws,
                         hipStream_t stream);
int vl_clip_mean_normalize(const float* x, long ldx, int B, int n_clip, int D, float eps, float* out, hipStream_t stream);

/* ---- the contrastive exchange over RCCL (csrc/vl_comm.cpp) ----
 * One process per GPU, one communicator per process; RCCL (librccl.so.1) is resolved at run time.  These are the three
 * collectives of a training step of the hot path, for a host that is not Python (the Python host makes the same calls
 * through torch.distributed, or - vitlens_hip.step.AbiComm - through these entries):
 *   vl_allgather_embed     the packed unit features of the step, [b, k*E] f32 per rank -> [W*b, k*E] in rank order
 *                          (replaces gather_features' 2-4 dist.all_gather calls, open_clip/loss.py:20-78); count = floats per rank
 *   vl_reducescatter_grad  backward of that gather under --gather-with-grad: full [W*b, E] f32 -> this rank's [b, E] slice of the
 *                          sum over ranks (loss.py:55-61: torch.distributed.nn.all_gather's autograd)
 *   vl_allreduce_grad      sum of a flat fp32 gradient bucket over the ranks, in place (DistributedDataParallel's all-reduce;
 *                          the 1 / world of its mean is applied by the optimizer step, vl_adamw_step's grad_scale)
 * vl_comm_unique_id fills 128 bytes on ONE rank; the host ships them to the others (its own channel: file, socket, MPI) and
 * every rank calls vl_comm_create (collective).  All calls are asynchronous on `stream`. */
typedef struct vl_comm* vl_comm_t;
int vl_comm_unique_id(void* id128);
int vl_comm_create(vl_comm_t* comm, const void* id128, int rank, int world);
int vl_comm_destroy(vl_comm_t comm);
int vl_allgather_embed(vl_comm_t comm, const float* local, float* gathered, long count, hipStream_t stream);
int vl_reducescatter_grad(vl_comm_t comm, const float* full, float* mine, long count_per_rank, hipStream_t stream);
int vl_allreduce_grad(vl_comm_t comm, float* buf, long count, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VITLENS_HIP_H */
