/* libattnshift_hip.so -- C ABI of the MI355X (gfx950) hot path of AttentionShift.
 *
 * The reference is Python on PyTorch; its only native boundary on this path is
 *   cc_torch.connected_components_labeling(uint8 [H,W]) -> int32 [H,W]
 *   (mmdet/models/roi_heads/stdroi_point_deform_attn_reppoints.py:23,68  -- source absent upstream)
 * Every other entry point below replaces a run of ATen calls inside one reference function
 * (cited per function, paths relative to the reference root, `stdroi` = the file above).
 *
 * Conventions
 *   - return 0 (AS_OK) on success, a negative AS_E_* otherwise; as_last_error() gives the message
 *     (thread-local).  Never throws, never exits.
 *   - all pointers are DEVICE pointers (HBM) unless stated; contiguous row-major layouts only.
 *   - no ownership transfer: inputs, outputs and workspaces are caller-allocated
 *     (sizes through as_*_workspace_bytes); workspaces need no initialisation.
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream); re-entrant;
 *     no global mutable state.  as_sdpa_bwd (bf16) runs one of its kernels on a library-owned helper stream
 *     (per host thread and device, created on first use and freed at thread exit) that is forked from and joined
 *     back to `stream` with events: to the caller everything is ordered on `stream`, but the first call on a thread
 *     creates a stream (not legal inside a stream capture -- warm up before capturing), and a per-stream allocator
 *     must treat the workspace and dqkv as in use until work queued on `stream` after the call has run.
 *   - dtype: AS_F32 = exact fp32 MFMA path (parity), AS_BF16 = bf16 operands with fp32 accumulate.
 *     Biases, log-sum-exp, roll-out matrices and all of Part B are always fp32; indices int32.
 */
#ifndef ATTNSHIFT_H
#define ATTNSHIFT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AS_VERSION 100
#define AS_OK 0
#define AS_E_BADARG (-1)
#define AS_E_UNSUPPORTED (-2)
#define AS_E_LAUNCH (-3)
#define AS_E_WORKSPACE (-4)

#define AS_F32 0
#define AS_BF16 1

#define AS_HEAD_DIM 64 /* every ViT in the reference has D/h = 64 (models/vision_transformer.py:266-288) */

typedef void* as_stream_t;

int as_version(void);
const char* as_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Part A -- backbone attention (models/vision_transformer.py:62-124)
 * ------------------------------------------------------------------------------------------- */

/* padded token count used by the q/k/v workspaces: N rounded up to a multiple of 64 */
int as_npad(int N);

/* out[M,Nout] = act(x[M,K] . W[Nout,K]^T + bias[Nout])           nn.Linear (vision_transformer.py:47-59,
 * 84).  x,W,out in `dtype`; bias fp32 or NULL; act 0 = none, 1 = exact (erf) GELU, 4 = ReLU (the point head's FFN,
 * mmdet/models/backbones/visual_transformer_det.py:26-38).  K % 32 == 0. */
int as_linear_fwd(const void* x, const void* W, const float* bias, void* out, int M, int Nout, int K,
                  int dtype, int act, as_stream_t stream);

/* out[M,Nout] = act(x[M,K] . W[Nout,K]^T + bias) in fp32 for SMALL M (a few hundred rows): the point head of
 * VisionTransformerDet -- class_embed / bbox_embed, two 3-layer FFNs over the B * T = 200 point tokens
 * (mmdet/models/backbones/visual_transformer_det.py:26-38, 145-146, 262-267).  32 x 64 output tiles whose four waves split
 * K, so 200 rows still fill the chip; exact fp32 arithmetic (f32 MFMA chains), deterministic summation order.  Row strides
 * ldx / ldo (elements) let a column slice of a packed activation be read / written in place.  act: 0 none, 1 exact GELU,
 * 4 ReLU, 5 sigmoid (the coordinate head, :267).  K % 16 == 0, K >= 64, ldx % 4 == 0, 16-byte aligned x / W; bias or NULL. */
int as_linear_small_fwd(const float* x, int ldx, const float* W, const float* bias, float* out, int ldo, int M, int Nout, int K,
                        int act, as_stream_t stream);

/* as_linear_fwd with a stream-K schedule for shapes whose tile count leaves the last round of the plain grid mostly empty
 * (ViT-B at 2 x 4197 tokens: fc1 = 396 tiles of 256 x 256 on 256 CUs, fc2 = 198 of 256 x 128): every workgroup contracts
 * the same number of K steps of the flattened (tile, K step) space; a tile cut into pieces is finished by its last-arriving
 * piece from fp32 partials in `ws` (fixed summation order: bitwise reproducible).  as_linear_sk_workspace_bytes returns 0
 * when the plain grid is the better schedule for (M, Nout, K) -- the call then IS as_linear_fwd and ws may be NULL.  bf16.
 * Round-5 measurement: with the fence-based hand-off it is SLOWER than the plain grid on every ViT-B / ViT-L shape (fc1
 * 60 -> 150 us), so the query returns 0 unless AS_GEMM_SK=1 is set in the environment (csrc/gemm.hip sk_plan). */
size_t as_linear_sk_workspace_bytes(int M, int Nout, int K);
int as_linear_sk_fwd(const void* x, const void* W, const float* bias, void* out, int M, int Nout, int K, int dtype, int act,
                     void* ws, size_t ws_bytes, as_stream_t stream);

/* nn.ConvTranspose2d(cin, cout, kernel 2, stride 2) on a channels-last map as one GEMM over its pixels
 * (mmdet/models/backbones/visual_transformer_det.py:107-117, the FPN taps): x [M = B*h*w, cin] (pixel-major, grid w wide),
 * W4 [4*cout, cin] with row (di*2 + dj)*cout + co = weight[ci, co, di, dj], bias4 [4*cout] fp32 or NULL ->
 * out NHWC [B, 2h, 2w, cout]: out[b, 2i+di, 2j+dj, co] = act(sum_ci x[b,i,j,ci] W[ci,co,di,dj] + bias[co]); the epilogue
 * scatters straight to the interleaved pixel (no layout copy).  act as as_linear_fwd (an eval-mode BatchNorm that follows
 * is folded into W4 / bias4 by the caller).  bf16 only; cin % 32 == 0, cout % 8 == 0. */
int as_deconv2x2_fwd(const void* x, const void* W4, const float* bias4, void* out, int M, int w, int cin, int cout,
                     int dtype, int act, as_stream_t stream);

/* nn.Conv2d(Cin, Cout, ksize, stride 1, padding (ksize - 1) / 2), ksize 1 or 3, on a channels-last map as an implicit GEMM
 * over its pixels (no im2col buffer, no padded copy): the FPN's lateral and output convolutions
 * (mmdet/models/necks/fpn.py:170-204) and the RPN trunk (mmdet/models/dense_heads/rpn_head.py forward_single).
 *   x    bf16 [B, H, W, Cin], every image dense, image b at x + b * x_batch_stride elements (a view into a token tensor is
 *        read in place); w bf16 [Cout, ksize, ksize, Cin] (tap-major); bias fp32 [Cout] or NULL;
 *   add  bf16 [B, Ha, Wa, Cout] or NULL: out[b, y, x, :] += add[b, sy(y), sx(x), :] with ATen's nearest source index
 *        sy(y) = min((int)floorf(y * ((float)Ha / H)), Ha - 1) -- F.interpolate(size=, mode='nearest') of the level above
 *        (fpn.py:180-190); Ha <= H, Wa <= W;
 *   out  [B, H, W, Cout] in out_dtype (AS_BF16 / AS_F32) = act(fp32 accumulator + bias + float(add)), one rounding;
 *        act 0 = none, 1 = ReLU.  Taps outside the image contribute exact zeros.  A pure function of its inputs (no
 *        atomics, no split-K): bitwise reproducible.
 * Cin % 32 == 0, Cout % 16 == 0, x_batch_stride % 8 == 0, 16-byte aligned pointers (else AS_E_BADARG); the input must span
 * less than 2^31 bytes (AS_E_UNSUPPORTED).  as_conv2d_tile_n: the output channels per tile of the variant the launcher
 * takes for Cout (128 or 32; a host function). */
int as_conv2d_tile_n(int Cout);
int as_conv2d_fwd(const void* x, long long x_batch_stride, const void* w, const float* bias, const void* add, int Ha, int Wa,
                  int B, int H, int W, int Cin, int Cout, int ksize, int act, int out_dtype, void* out, as_stream_t stream);

/* QKV projection with the head split fused into the epilogue (vision_transformer.py:75-77):
 *   k : [B,h,Npad,64]   vt : [B,h,64,Npad]  (V transposed so the P.V MFMA reads keys contiguously)
 *   q : [B,h,Npad,64] elements, FRAGMENT-MAJOR inside every 32-row x 64-d tile: element (r, d) of a tile sits at
 *       ((d/16)*64 + r + 32*((d%16)/8))*8 + d%8, so the MFMA operand loads of sdpa / roll-out are coalesced.
 *       VALUES are pre-scaled: q holds (x Wq^T + bq) * log2(e) / sqrt(64), rounded once from the fp32 accumulator, so
 *       that q . k is the base-2 logit every consumer (as_sdpa_fwd / _bwd, as_rollout_*, as_attn_mean_rows) feeds to
 *       exp2 without a multiply per score.  A caller that fills q by hand applies the same factor.
 * rows/cols >= N of the padded layouts are never read unmasked, so they need no initialisation. */
int as_qkv_fwd(const void* x /*[B,N,D]*/, const void* Wqkv /*[3D,D]*/, const float* bqkv /*[3D] or NULL*/,
               void* q, void* k, void* vt, int B, int N, int D, int h, int dtype, as_stream_t stream);

/* softmax(q k^T / sqrt(64)) v without materialising [h,N,N] (vision_transformer.py:79-83).
 *   q is the PRE-SCALED fragment-major workspace of as_qkv_fwd (see there): softmax(q' k^T ln 2) = softmax(q k^T / 8).
 *   o   : [B,N,h*64] (heads concatenated, ready for proj)        lse : [B,h,N] fp32, natural log
 *   workspace : optional, as_sdpa_fwd_workspace_bytes(...) bytes (0 for most shapes): lets the launch split the keys
 *               of the last q-tile over extra workgroups when the plain grid would leave a short second round
 *               (ViT-B/1024^2/B=2: 792 workgroups for 768 resident slots); NULL = plain grid.  Same results. */
size_t as_sdpa_fwd_workspace_bytes(int B, int N, int h, int dtype);
int as_sdpa_fwd(const void* q, const void* k, const void* vt, void* o, float* lse, void* workspace,
                size_t workspace_bytes, int B, int N, int h, int dtype, as_stream_t stream);

/* Backward of as_sdpa_fwd (autograd of vision_transformer.py:79-83; the reference trains the backbone, and with
 * use_checkpoint recomputes each block's forward in backward, visual_transformer_det.py:232-236).  Softmax tiles are
 * recomputed from q, k and lse; no [h,N,N] buffer, no atomics, fixed summation order.
 *   q,k,vt,lse : as written by as_qkv_fwd / as_sdpa_fwd           o, d_o : [B,N,h*64] (forward output, its gradient)
 *   dqkv       : [B,N,3,h,64] = gradient of the QKV projection output in the reference's reshape order (:76)
 *   workspace  : as_sdpa_bwd_workspace_bytes(B,N,h,dtype) bytes, caller-owned
 * Rows [N, Npad) of q / k / vt may hold anything (NaN included): nothing outside [0, N) reaches a gradient. */
size_t as_sdpa_bwd_workspace_bytes(int B, int N, int h, int dtype);
int as_sdpa_bwd(const void* q, const void* k, const void* vt, const void* o, const void* d_o, const float* lse,
                void* dqkv, void* workspace, size_t workspace_bytes, int B, int N, int h, int dtype,
                as_stream_t stream);

/* Attention.forward = qkv + sdpa + proj (vision_transformer.py:74-86).  q/k/vt/o are workspaces the
 * caller keeps alive when the roll-out (below) needs this layer; `o` is [B,N,D]. */
int as_attn_fwd(const void* x, const void* Wqkv, const float* bqkv, const void* Wproj, const float* bproj,
                void* out /*[B,N,D]*/, float* lse, void* q, void* k, void* vt, void* o, void* workspace,
                size_t workspace_bytes /* as_sdpa_fwd_workspace_bytes, may be NULL/0 */, int B, int N, int D, int h,
                int dtype, as_stream_t stream);

/* Backward of as_attn_fwd (autograd of Attention.forward, vision_transformer.py:74-86): given dout = dL/d out and the
 * tensors as_attn_fwd saved (q,k,vt,o,lse) returns dL/dx and the parameter gradients.
 *   x, dout, dx : [B,N,D]     dWqkv : [3D,D]   dWproj : [D,D] (element dtype = `dtype`)   dbqkv [3D], dbproj [D] fp32 or NULL
 *   workspace   : as_attn_bwd_workspace_bytes(B,N,D,h,dtype) bytes, caller-owned */
size_t as_attn_bwd_workspace_bytes(int B, int N, int D, int h, int dtype);
int as_attn_bwd(const void* x, const void* Wqkv, const void* Wproj, const void* dout, const void* q, const void* k,
                const void* vt, const void* o, const float* lse, void* dx, void* dWqkv, float* dbqkv, void* dWproj,
                float* dbproj, void* workspace, size_t workspace_bytes, int B, int N, int D, int h, int dtype,
                as_stream_t stream);

/* Swin window attention for one SwinTransformerBlock (models/swin_transformer.py): fuses the pad (:271-276), cyclic
 * shift (:279-280), window_partition (:292-293), the WindowAttention core (:131-153 incl. the relative-position-bias
 * gather :141-144 and the shift mask :233-256), window_reverse (:299-300), reverse shift (:303-304) and un-pad (:308).
 *   qkv      : [B,H,W,3C] = x_normed . Wqkv^T WITHOUT bias, on the original token grid, channel order (3,h,32)
 *   bqkv     : fp32 [3C] or NULL (added here; padded tokens are exactly the bias, as in the reference)
 *   table    : fp32 [(2*ws-1)^2, h] relative_position_bias_table
 *   out      : [B,H,W,C] attention output at the original token positions (input of the proj Linear)
 *   attn_out : fp32 [B*nW, h, ws*ws, ws*ws] softmax (the reference returns it) or NULL
 * ws must be 7 and C == 32*h (all Swin variants of the reference, swin_transformer.py:844-870). */
int as_window_attn_fwd(const void* qkv, const float* bqkv, const float* table, void* out, float* attn_out, int B, int H,
                       int W, int C, int h, int ws, int shift, int dtype, as_stream_t stream);

/* Fused residual add + LayerNorm of the pre-LN block (vision_transformer.py:109-124: x = x + sublayer(norm(x))):
 *   x_out = x_in + delta (fp32 residual stream; delta [M,D] in `dtype`, or NULL),  y_out = LN(x_out)*gamma + beta (`dtype`)
 * x_out may alias x_in; either output may be NULL (x_out NULL: LN only; y_out NULL: add only).  D % 4 == 0, D <= 3072. */
int as_add_layernorm(const float* x_in, const void* delta, const float* gamma, const float* beta, float eps,
                     float* x_out, void* y_out, int M, int D, int dtype, as_stream_t stream);
/* The same with the sub-layer output scaled per SAMPLE: x_out = x_in + delta_scale[row / rows_per_scale] * delta -- the
 * DropPath of the training path (models/vision_transformer.py:21-40, applied at :114-118: x + drop_path(f(norm(x)))),
 * with delta_scale[b] = mask_b / keep_prob drawn by the caller (fp32, one value per image; NULL = 1). */
int as_add_layernorm_scaled(const float* x_in, const void* delta, const float* gamma, const float* beta, float eps,
                            float* x_out, void* y_out, int M, int D, int dtype, const float* delta_scale,
                            int rows_per_scale, as_stream_t stream);

/* out[M,Nout] = x[M,K] . W[Nout,K]^T (no bias, no activation) with the CONTRACTION split over workgroups: fp32 partial
 * products of K ranges, summed in range order (deterministic), written as bf16 (out_f32 = 0) or fp32 (1).  The form of an
 * nn.Linear WEIGHT gradient dW = dy^T . x (models/vision_transformer.py:75-77,84 under autograd): few output tiles, the
 * tokens as K.  bf16 operands, K % 32 == 0, Nout % 4 == 0; workspace: as_linear_splitk_workspace_bytes(M, Nout, K). */
/* The MLP's first linear under autograd (vision_transformer.py:47-59: fc1 -> GELU): pre[M,Nout] = x . W^T + bias rounded
 * to bf16, out = GELU(pre) -- both written by the GEMM's epilogue (no separate activation pass; `pre` is what the
 * backward needs).  bf16 only, K % 32 == 0, Nout % 8 == 0. */
int as_linear_gelu_fwd(const void* x, const void* W, const float* bias, void* out, void* pre, int M, int Nout, int K,
                       int dtype, as_stream_t stream);
/* out[M,Nout] = (x[M,K] . W[Nout,K]^T) * GELU'(pre[M,Nout]): a linear's input gradient times the derivative of the GELU that
 * produced that input, in the epilogue (the GeluBackward pass of autograd).  bf16 only, K % 32 == 0, Nout % 8 == 0. */
int as_linear_dgelu_fwd(const void* x, const void* W, const void* pre, void* out, int M, int Nout, int K, int dtype,
                        as_stream_t stream);

size_t as_linear_splitk_workspace_bytes(int M, int Nout, int K);
int as_linear_splitk_fwd(const void* x, const void* W, void* out, int M, int Nout, int K, int dtype, int out_f32,
                         void* workspace, size_t workspace_bytes, as_stream_t stream);

/* Backward of one nn.Linear y = x W^T + b under autograd (models/vision_transformer.py:47-59 the MLP, :75-77,84 and the
 * MAE-decoder heads' layers, mae_bbox_head_rec.py:148-168), x [M,K], W [Nout,K], dy [M,Nout] bf16:
 *   dx [M,K] bf16   = dy . W           (NULL: skipped)   on the forward kernel against a transposed copy of W
 *   dW [Nout,K]     = dy^T . x         (NULL: skipped)   split-K over the rows (as_linear_splitk_fwd), bf16 or fp32 (dw_f32)
 *   db [Nout] fp32  = column sums of dy (NULL: skipped)  two fixed-order stages, no atomics
 * Nout % 32 == 0, K % 4 == 0; workspace: as_linear_bwd_workspace_bytes(M, Nout, K). */
size_t as_linear_bwd_workspace_bytes(int M, int Nout, int K);
int as_linear_bwd(const void* x, const void* W, const void* dy, void* dx, void* dW, float* db, int M, int Nout, int K,
                  int dtype, int dw_f32, void* workspace, size_t workspace_bytes, as_stream_t stream);
/* as_linear_bwd for the linear that FOLLOWS a GELU (fc2 of the Mlp): x = GELU(pre); dx [M,K] comes out already multiplied
 * by GELU'(pre[M,K]) (as_linear_dgelu_fwd), i.e. it is the gradient of the pre-activation.  pre NULL = as_linear_bwd. */
int as_linear_bwd_dgelu(const void* x, const void* W, const void* dy, const void* pre, void* dx, void* dW, float* db, int M,
                        int Nout, int K, int dtype, int dw_f32, void* workspace, size_t workspace_bytes, as_stream_t stream);

/* k x k / stride-k max pooling of a token-major (NHWC) fp32 map [B,H,W,C] -> [B,H/k,W/k,C] (contiguous): the FPN's
 * coarsest tap, nn.MaxPool2d(k, k) (mmdet/models/backbones/visual_transformer_det.py:120,129,133) on the layout the taps
 * live in here.  x_batch_stride = elements between consecutive images of x (>= H*W*C, multiple of 4): the tap is the
 * patch-token slice of the [B, 1+Np+T, C] token tensor, so its images are not adjacent.  C % 4 == 0, H and W multiples
 * of k; NaNs propagate as in ATen. */
int as_maxpool_nhwc(const float* x, float* out, int B, int H, int W, int C, int k, long long x_batch_stride,
                    as_stream_t stream);

/* Token assembly of prepare_tokens (mmdet/models/backbones/visual_transformer_det.py:192-214: patch embedding + position
 * embedding, class token in front, point tokens + their position embedding behind): out [B,N,D] fp32,
 *   out[b,n] = table[n] + emb[b,n-1]  for 1 <= n <= Np,   out[b,n] = table[n]  otherwise,
 * emb [B,Np,D] (`dtype`), table [N,D] fp32 = [cls + pos_0 ; pos_1..Np ; point_token + point_pos_embed] (the caller's
 * constant).  D % 4 == 0. */
int as_assemble_tokens(const void* emb, const float* table, float* out, int B, int Np, int N, int D, int dtype,
                       as_stream_t stream);

/* Backward of as_add_layernorm for the trainable path.  x [M,D] fp32 = the x_out the forward wrote (x_in + delta); dy
 * [M,D] in `dtype` = gradient of y_out (NULL: the call was add-only); dx_res [M,D] fp32 = gradient of x_out from the
 * residual stream (NULL: none); gamma fp32 [D].  Writes dx_out [M,D] fp32 (gradient of x_in) and / or ddelta_out [M,D]
 * in `dtype` (gradient of delta: the same values), dgamma / dbeta fp32 [D] (either may be NULL).  Column sums go through
 * per-workgroup partials added in workgroup order (deterministic).  D % 4 == 0, D <= 2048. */
size_t as_add_layernorm_bwd_workspace_bytes(int M, int D);
int as_add_layernorm_bwd(const float* x, const void* dy, const float* dx_res, const float* gamma, float eps, float* dx_out,
                         void* ddelta_out, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, int M, int D,
                         int dtype, as_stream_t stream);
/* Backward of as_add_layernorm_scaled: ddelta_out = delta_scale[row / rows_per_scale] * (gradient of x_out). */
int as_add_layernorm_bwd_scaled(const float* x, const void* dy, const float* dx_res, const float* gamma, float eps,
                                float* dx_out, void* ddelta_out, float* dgamma, float* dbeta, void* workspace,
                                size_t workspace_bytes, int M, int D, int dtype, const float* delta_scale,
                                int rows_per_scale, as_stream_t stream);

/* Backward of as_window_attn_fwd (autograd of WindowAttention's core + the index maps around it):
 *   d_out     : [B,H,W,C] gradient of the attention output        dqkv : [B,H,W,3C] gradient w.r.t. the bias-free qkv
 *   dtable    : fp32 [(2*ws-1)^2, h] gradient of relative_position_bias_table
 *   dbqkv_pad : fp32 [3C] bias gradient contributed by PADDED tokens (whose qkv is the bias itself); the full qkv-bias
 *               gradient is the column sum of dqkv over real tokens plus this vector
 * No atomics: window partials are reduced in window order by a second launch. */
size_t as_window_attn_bwd_workspace_bytes(int B, int H, int W, int h, int ws);
int as_window_attn_bwd(const void* qkv, const float* bqkv, const float* table, const void* d_out, void* dqkv,
                       float* dtable, float* dbqkv_pad, void* workspace, size_t workspace_bytes, int B, int H, int W,
                       int C, int h, int ws, int shift, int dtype, as_stream_t stream);

/* Head-mean attention rows, recomputed from q,k,lse (visual_transformer_det.py:236,242 keeps
 * attn.mean(1) of every layer; only row slices are ever consumed, stdroi:2272):
 *   out[b,i,:] = (1/h) sum_h softmax_row(row0 + i)          out : [B,nrows,N] fp32 */
int as_attn_mean_rows(const void* q, const void* k, const float* lse, float* out, int B, int N, int h,
                      int row0, int nrows, int dtype, as_stream_t stream);

/* Row-sliced attention roll-out (stdroi:1257-1272 attns_project_to_feature, rows [-T:] only, T <= 128):
 *   A_hat = (mean_h P + I) / rowsum (rowsum == 2),   R_out = R_in . A_hat        R : [B,T,N] fp32
 * with the tiles of mean_h P recomputed from q,k,lse of that layer.  as_rollout_top gives the top layer's
 * R = rows [N-T, N) of A_hat.  Next to the fp32 row-major R every call also emits a FRAGMENT-MAJOR copy `rf`
 * (as_rollout_rfrag_bytes; element dtype = `dtype`) that the next step reads as its MFMA A operand with fully
 * coalesced loads; rf_out may be NULL on the last step.  as_rollout_step splits the contraction (and, for bf16 with
 * h % 4 == 0, the heads in groups of four: the streamed-operand kernel) over several workgroups when given a workspace
 * of as_rollout_step_workspace_bytes (room for 16 partial products, summed in a fixed order by a second tiny launch:
 * deterministic); with workspace == NULL it runs unsplit. */
size_t as_rollout_rfrag_bytes(int B, int N, int dtype);
/* rf = the fragment-major copy of a row-major R [B,T,N] fp32: lets a caller continue the roll-out from a row SUBSET of a
 * previous result (the RoI head only consumes the rows of the matched point tokens, stdroi:2272 + the pos_inds gather). */
int as_rollout_pack(const float* R, void* rf, int B, int N, int T, int dtype, as_stream_t stream);
size_t as_rollout_step_workspace_bytes(int B, int N, int T);
int as_rollout_top(const void* q, const void* k, const float* lse, float* R_out, void* rf_out, int B, int N, int h,
                   int T, int dtype, as_stream_t stream);
int as_rollout_step(const void* q, const void* k, const float* lse, const float* R_in, const void* rf_in,
                    float* R_out, void* rf_out, void* workspace, size_t workspace_bytes, int B, int N, int h, int T,
                    int dtype, as_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Part B -- attention-shift pseudo-label generator (stdroi:2209-2415), fp32 + int32
 * ------------------------------------------------------------------------------------------- */

/* 8-connectivity connected components of M binary images; label = 1 + min raster index of the
 * component, background 0.  Replaces cc_torch.connected_components_labeling (stdroi:68). */
int as_ccl_2d(const uint8_t* img /*[M,H,W]*/, int32_t* labels /*[M,H,W]*/, int M, int H, int W,
              as_stream_t stream);

/* CAM -> box (stdroi:2272-2294 + get_bbox_from_cam_fast :60-116), batched over M = Lc*G maps:
 * bilinear x`up` upsample (align_corners=False), min-max normalise (clamp 1e-6), binarise at
 * cam_thr, CCL, keep components with area >= area_ratio * max area, tight box, 'expand' about the
 * point, clip to the image.  boxes [M,4] fp32 (x0,y0,x1,y1); status[m] = number of kept pixels
 * (0 = the reference would have raised; -1 = a row held more foreground runs than the workspace
 * provides, result invalid).  cams_up, if not NULL, receives the upsampled maps
 * [M,H,W] fp32 (the reference keeps them as attn_maps_dealed, stdroi:2282); minmax, if not NULL,
 * their per-map (min, max) [M,2] (reused by norm_attns, stdroi:329). */
size_t as_cam_boxes_workspace_bytes(int M, int Hp, int Wp, int up);
int as_cam_boxes(const float* cams /*[M,Hp,Wp]*/, const float* points /*[M,2] (x,y)*/, float cam_thr,
                 float area_ratio, int M, int Hp, int Wp, int up, float* boxes, int32_t* status,
                 float* cams_up, float* minmax, void* ws, size_t ws_bytes, as_stream_t stream);

/* Candidate masks of the seed sampling (stdroi:1003-1007 -> sample_point_grid :343-371 on norm_attns
 * :329-333) for the G selected maps of one image, straight from the low-resolution CAMs:
 *   nm_g = (up(cams[map_idx[g]]) - min) / (max - min)   with (min, max) = minmax[map_idx[g]] of as_cam_boxes
 *   masks [2G+1, H*W] uint8: rows 0..G-1  nm_g < thr_bg,  rows G..2G-1  nm_g >= thr_fg,
 *                            row 2G       mean_g(nm_g) < thr_bg
 *   counts [2G+1] int32: set pixels per row (written by the call); may be NULL (no counting, no fill launch).
 * The upsampled maps are never materialised (same bilinear arithmetic as as_cam_boxes). */
size_t as_cam_sample_masks_workspace_bytes(int G, int Hp, int Wp, int up);     /* 0 for G <= 8 */
int as_cam_sample_masks(const float* cams /*[M,Hp,Wp]*/, const int32_t* map_idx /*[G]*/,
                        const float* minmax /*[M,2]*/, int G, int Hp, int Wp, int up, float thr_bg, float thr_fg,
                        uint8_t* masks, int32_t* counts, void* ws, size_t ws_bytes, as_stream_t stream);

/* The three candidate masks of one image's G objects in one call (stdroi:433-461, :2356-2358); crops [G,4] int32
 * half-open (x0,y0,x1,y1):
 *   pos    [G,H,W] uint8 = erode_k(in_crop && map_fg > max_crop(map_fg) * pos_thr)
 *   neg    [G,H,W] uint8 =          in_crop && map_bg > max_crop(map_bg) * neg_thr
 *   pseudo [G,H,W] uint8 =                     map_fg > max(map_fg)      * mask_thr
 *   counts [3,G] int32 set pixels of pos / neg / pseudo (written by the call). */
size_t as_mask_candidates_workspace_bytes(int G, int H, int W);
int as_mask_candidates(const float* map_fg, const float* map_bg, const int32_t* crops, float pos_thr, float neg_thr,
                       float mask_thr, int k, uint8_t* pos, uint8_t* neg, uint8_t* pseudo, int32_t* counts, void* ws,
                       size_t ws_bytes, int G, int H, int W, as_stream_t stream);

/* Per-part statistics of get_center_coord_with_feat (stdroi:222-262) for M part maps [M, Hp*Wp]; rois [G,4],
 * owner [M] = object of each part: out_c [M,2] = ((x, y) of the peak centroid + 0.5) * stride, out_yx [M,2] = its
 * integer (y, x), out_area [M] = pixels > 0.9, out_inside [M] = centre inside the owner's box. */
int as_part_stats(const float* maps, const float* rois, const int32_t* owner, float stride, float* out_c,
                  int32_t* out_yx, int32_t* out_area, uint8_t* out_inside, int M, int Hp, int Wp, as_stream_t stream);

/* Part selection of get_center_coord_with_feat (stdroi:222-262) for all G objects x P slots on the device: slots
 * p < ngroups[g] visited in stable descending-area order, taken if inside and position <= num_points; taken slots
 * compacted in (object, visiting) order into rows of coords / coords_org [G*P,2], out_labels / labels_org / corres
 * [G*P] int64, feats [G*P,C] = feat_tok[yx.y * Wp + yx.x]; split [G+1] = per-object counts and their total; sel_slot
 * [G*P] scratch.  area / inside / c / yx as as_part_stats writes them.  P <= 256. */
int as_part_select(const int32_t* area, const uint8_t* inside, const int32_t* ngroups, const float* c, const int32_t* yx,
                   const int64_t* labels, const float* feat_tok, int G, int P, int C, int Wp, int num_points, float* coords,
                   float* coords_org, int64_t* out_labels, int64_t* labels_org, int64_t* corres, float* feats,
                   int32_t* sel_slot, int32_t* split, as_stream_t stream);

/* filter_maps (stdroi:263-271) for G*P prototypes: keep[g,p] = share of sim[g,p] > sim_thr lying on fg_inter[g] >= pos_thr. */
int as_filter_parts(const float* sim /*[G,P,Np]*/, const float* fg_inter /*[G,Np]*/, float sim_thr, float pos_thr,
                    uint8_t* keep /*[G,P]*/, int G, int P, int Np, as_stream_t stream);

/* Device-side draw of the mask points (fast-RNG mode; the head of a random permutation, stdroi:447): the first K
 * distinct values of floor(u[g,:] * n_g), n_g = n_pos + n_neg of object g read at counts[g * count_stride_g] and
 * counts[g * count_stride_g + count_stride_k] (so both a [G,2] table and the [3,G] table of as_mask_candidates are read in
 * place), split into ranks among the positive / negative candidates.  *flag (int32, zeroed by the caller) is OR-ed with 1
 * when some object needs the host path (n_g < 4K or too few distinct draws). */
int as_draw_distinct(const int32_t* counts, int count_stride_g, int count_stride_k, const float* u /*[G,M]*/,
                     int32_t* rank_pos /*[G,K]*/, int32_t* rank_neg, uint8_t* is_pos, int32_t* flag, int G, int M, int K,
                     as_stream_t stream);

/* The reference-RNG mode's draws made on the device (csrc/mt19937.hip): `state` = torch's CPU mt19937 engine as int32[626]
 * (624 state words, left, next: attentionshift_amd/mt19937.py), advanced in place exactly as the reference's host calls
 * advance the global generator.  as_mt_sample_ranks: for S candidate sets with counts[s] members,
 * ranks[s, 0:K] = (torch.randint(n, (len(range(0, n, n // K)),)) % n)[:K]  (sample_point_grid, stdroi:343-371).
 * as_mt_perm_ranks: for G objects with n = counts2[g,0] + counts2[g,1] candidates, ranks[g, 0:K] = torch.randperm(n)[:K]
 * (get_mask_points_single_instance, stdroi:447).  flag (int32, written) != 0: a set the host path must handle (fewer
 * than K candidates -- the reference's refill / fill-in / empty branches -- or a range beyond the one-word draws). */
int as_mt_sample_ranks(int32_t* state /*[626]*/, const int32_t* counts /*[S]*/, int32_t* ranks /*[S,K]*/, int32_t* flag,
                       int S, int K, as_stream_t stream);
int as_mt_perm_ranks(int32_t* state /*[626]*/, const int32_t* counts2 /*[G,2]*/, int32_t* ranks /*[G,K]*/, int32_t* flag,
                     int G, int K, as_stream_t stream);

/* Greedy grouping of merge_maps (stdroi:278-294) for G objects: keep [G,P] uint8, link [G,P,P] uint8 (cos >= thr)
 * -> groups [G,P] int32 bit sets over the prototype ids, in the reference's emission order (0 = unused), ngroups [G]. */
int as_merge_plan(const uint8_t* keep, const uint8_t* link, int32_t* groups, int32_t* ngroups, int G, int P,
                  as_stream_t stream);

/* Patch-grid foreground of get_semantic_centers (stdroi:2011-2012, 2020), one launch:
 *   fg_inter [G,Hp*Wp] = bilinear x(1/up) of erode_k(map_fg > thr)   (map_fg [G, Hp*up, Wp*up])
 *   mask     [G,Hp*Wp] uint8 = fg_inter > thr,  counts [G] = set entries per object (the grid-seed candidates, :1784);
 *   counts may be NULL (no counting, no fill launch) */
int as_semantic_prestage(const float* map_fg, float thr, int k, int G, int Hp, int Wp, int up, float* fg_inter,
                         uint8_t* mask, int32_t* counts, as_stream_t stream);

/* Mean-shift token clustering (stdroi:830-854 cosine_shift_batch + :882-908 update_density_batch,
 * with the box masking of :1819-1824 folded in):
 *   feat      [B,Np,C]  token-major ViT features (Np = Hp*Wp)
 *   box_patch [G,4]     inclusive patch-grid box (x0,y0,x1,y1) of each object = rois // 16
 *   obj_img   [G]       image index of each object
 *   prot_in   [G,P,C]   seed prototypes;  prot_out [G,P,C] shifted prototypes (unnormalised, as the reference); the
 *                       two may be the same buffer
 *   sim_out   [G,P,Np]  cos(prot, UNMASKED feat) (not clamped)
 *   assign_out[S,G,Np]  (optional) argmax prototype per patch per iteration, ties -> lowest index
 *   tau_out   [S,G,P]   (optional) per-prototype density after each iteration
 *   tau0, temp          doubles: the first iteration divides by the python float temp*tau0 rounded once to fp32, exactly
 *                       as `sim_map/(temp*tau)` with scalar arguments does (stdroi:834) */
size_t as_cosine_shift_workspace_bytes(int B, int C, int Hp, int Wp, int G, int P);
int as_cosine_shift(const float* feat, const int32_t* box_patch, const int32_t* obj_img, const float* prot_in,
                    float* prot_out, double tau0, double temp, int n_shift, float* sim_out, int32_t* assign_out,
                    float* tau_out, void* ws, size_t ws_bytes, int B, int C, int Hp, int Wp, int G, int P,
                    as_stream_t stream);
/* The same call on a feature tensor whose images are `feat_batch_stride` floats apart (>= Np*C, a multiple of 4): the
 * reference's caller passes vit_feat as a VIEW of last_feat [B, 1 + Np, C] without its cls row
 * (mmdet/models/detectors/two_stage_point_align.py:77), whose per-image token blocks are contiguous but not adjacent. */
int as_cosine_shift_strided(const float* feat, long long feat_batch_stride, const int32_t* box_patch, const int32_t* obj_img,
                            const float* prot_in, float* prot_out, double tau0, double temp, int n_shift, float* sim_out,
                            int32_t* assign_out, float* tau_out, void* ws, size_t ws_bytes, int B, int C, int Hp, int Wp, int G,
                            int P, as_stream_t stream);

/* Cosine-affinity refinement on the patch grid (stdroi:668-707 get_refined_similarity):
 *   feat   [Np,C] one image, seeds [Gp,C] (mean feature of the sampled points, :335-338)
 *   boxes  [G,4] inclusive patch boxes of the first G maps (selection group only)
 *   n_select  the first n_select maps form the selection group of `is_select=True` (box masking of its first G maps,
 *             keep-the-winner among the group, :676-683 / :697-703); 0 = none (`is_select=False`), Gp = all, a value in
 *             between refines the foreground and the background seed sets of an image in ONE call (group first)
 *   maps   [R+1,Gp,Np] ;  seeds_out [Gp,C] = refined seed features of the last round (with refine_times = 0 a copy of
 *   `seeds`, skipped when seeds_out == seeds) */
size_t as_refine_similarity_workspace_bytes(int C, int Np, int Gp);
int as_refine_similarity(const float* feat, const float* seeds, const int32_t* boxes, int G, int Gp,
                         int refine_times, float tau, int n_select, float* maps, float* seeds_out, void* ws,
                         size_t ws_bytes, int C, int Hp, int Wp, as_stream_t stream);

/* Full-resolution instance maps from the patch-grid refinement (stdroi:1010-1019):
 * bilinear x`up` of fg/bg levels, (1-bg)*fg, per-map max normalisation, decouple_instance.
 *   sim_fg [L,Gp,Np] (first G maps used), sim_bg [L,G,Np] -> map_fg, map_bg [L,G,H,W] */
size_t as_instance_maps_workspace_bytes(int L, int G);
int as_instance_maps(const float* sim_fg, const float* sim_bg, int L, int G, int Gp, int Hp, int Wp, int up,
                     float* map_fg, float* map_bg, void* ws, size_t ws_bytes, as_stream_t stream);

/* Thresholded + eroded candidate masks inside per-map crops: the fg candidates of
 * get_mask_points_single_box_cos_map_fg_bg (stdroi:442, erode(map > max*thr, 21) on the box crop), its bg
 * candidates (:443, k = 1) and the full-map erosion of get_semantic_centers (:2011, crops = NULL, absolute thr):
 *   mask[m][y][x] = 1 iff (y,x) in crop_m and min over the k x k window (restricted to the crop) of [map > t_m]
 *   t_m = relative ? thr * max(map over crop_m) : thr;  crops [M,4] int32 (x0,y0,x1,y1), half-open like the
 *   reference's slicing [y0:y1, x0:x1];  counts[m] = number of set pixels. */
size_t as_crop_threshold_erode_workspace_bytes(int M, int H, int W);
int as_crop_threshold_erode(const float* maps /*[M,H,W]*/, const int32_t* crops, float thr, int relative, int k,
                            uint8_t* mask /*[M,H,W]*/, int32_t* counts /*[M]*/, void* ws, size_t ws_bytes, int M, int H,
                            int W, as_stream_t stream);

/* Rank select: out[m][k] = flat index of the ranks[m][k]-th (0-based) set byte of mask[m] in raster order, i.e.
 * `mask[m].nonzero()[ranks[m][k]]` without the compaction (the reference indexes a .nonzero() list with random
 * indices, stdroi:368-369 and :456); -1 when the rank is outside the population.  HW % 16 == 0. */
/* counts[m] = number of non-zero bytes of row m of a [M,HW] byte mask (the candidate counts of stdroi:346-366 that the
 * reference gets from .nonzero().shape); HW % 16 == 0. */
int as_mask_count(const uint8_t* mask, int32_t* counts, int M, int HW, as_stream_t stream);

size_t as_rank_select_workspace_bytes(int M, int HW);
int as_rank_select(const uint8_t* mask /*[M,HW] 0/1*/, const int32_t* ranks /*[M,K]*/, int32_t* out /*[M,K]*/, void* ws,
                   size_t ws_bytes, int M, int HW, int K, as_stream_t stream);
/* The same selection returning grid coordinates: out_xy [M,K,2] int64 = (flat % W, flat / W), or (flat / W, flat % W)
 * with yx_order, of the selected pixel on a W-wide grid; an out-of-range rank gives pixel 0 (the `clamp(min=0)` of the
 * callers, which flag that case separately). */
int as_rank_select_xy(const uint8_t* mask /*[M,HW] 0/1*/, const int32_t* ranks /*[M,K]*/, int64_t* out_xy /*[M,K,2]*/, void* ws,
                      size_t ws_bytes, int M, int HW, int K, int W, int yx_order, as_stream_t stream);

/* merge_maps (stdroi:278-294) of every object in one launch: cosine links between the kept prototypes (>= thr), the greedy
 * upper-triangular grouping of as_merge_plan, and the merged prototypes matmul(weight, prot) / (weight.sum(-1) + 1e-8) of
 * the first `slots` groups per object (unused slots are zero rows).  ngroups [G] = min(groups, slots); *flag (may be NULL)
 * is OR-ed with 1 when an object has more than `slots` groups.  prot [G,P,C] fp32, keep [G,P] 0/1, P <= 32. */
int as_merge_parts(const float* prot, const uint8_t* keep, float thr, float* merged /*[G,slots,C]*/, int32_t* ngroups /*[G]*/,
                   int32_t* flag, int G, int P, int C, int slots, as_stream_t stream);

/* The default layer selector and its index arithmetic in one launch (roi_head.median_area_selector standing in for the MIL
 * head's choice, stdroi:2953-2972; the patch box of stdroi:1812): per object o with meta[o] = (first row of its image in
 * `boxes`, objects in that image, index in the image) and the image's boxes layer-major ([Lc, cnt, 4] from as_cam_boxes),
 *   pick[o]      the layer whose box area max(x1-x0,0)*max(y1-y0,0) has stable ascending rank (Lc-1)/2 -- or, with
 *                `pick_in` [n] (may be NULL), the layer another selector chose (the trained MIL head), clamped to [0, Lc)
 *   chosen[o]    that box;  map_idx[o] its row in `boxes` (= the row of the CAM stack);  box_patch[o] = floor(box / stride);
 *   box_int[o]   (may be NULL) the box truncated to integers, the crop of stdroi:1981
 * `status` (may be NULL) [rows] int32, the per-box status of as_cam_boxes: *bad (zeroed by the caller) is OR-ed with 1 when any
 * row of any listed object has status <= 0 (a CAM without a foreground component -- where stdroi:80 raises). */
int as_select_median_boxes(const float* boxes /*[rows,4]*/, const int32_t* meta /*[n,3]*/, int Lc, int stride,
                           const int64_t* pick_in, int64_t* pick /*[n]*/, float* chosen /*[n,4]*/, int32_t* map_idx /*[n]*/, int32_t* box_patch /*[n,4]*/,
                           int32_t* box_int /*[n,4]*/, const int32_t* status, int32_t* bad, int n, as_stream_t stream);

/* Rank selection whose ranks are derived on the device from each row's population n (known from the same counting pass), so
 * that the sampling chains need no tensor-op glue and no readback (fast-RNG mode of the seed sampling, stdroi:346-369, and the
 * grid seeds of mean_shift_grid_prototype, stdroi:1790-1792):
 *   mode 1  rank[m][k] = min(int(u[m][k] * float(n_m)), max(n_m - 1, 0))     u [M,K] uniform in [0, 1)
 *   mode 2  rank[m][k] = k * max(n_m / K, 1)                                 every (n / K)-th positive
 * out_xy as as_rank_select_xy (may be NULL if patch_out is given); *flag (int32, may be NULL) is OR-ed with 1 when some
 * n_m < K (the reference's refill branches: the caller repeats that image on the host path).
 * patch_out (may be NULL) [M,K] int64: patch_base + (y / patch_div) * patch_w + x / patch_div of the selected pixel (x, y),
 * i.e. its token index on a patch_w-wide grid of patch_div-pixel patches (`point // 16` of seed_features stdroi:335-338, or
 * with patch_div = 1 the flat seed index of stdroi:1793), row m written to row (m + M - row_rot) % M. */
int as_rank_draw_xy(const uint8_t* mask /*[M,HW] 0/1*/, int mode, const float* u /*[M,K] or NULL*/, int32_t* flag,
                    int64_t* out_xy /*[M,K,2]*/, int64_t* patch_out /*[M,K]*/, int patch_div, int patch_w, int64_t patch_base,
                    int row_rot, void* ws, size_t ws_bytes, int M, int HW, int K, int W, int yx_order, as_stream_t stream);

/* Small-N batched multi-head self-attention (the MAE-decoder box / mask heads: thousands of 50- / 197-token problems of
 * head dim 32 per step; models/vision_transformer.py:62-86 as used by mae_bbox_head_rec.py:148-168):
 *   qkv  [Bp, N, 3, h, d]  the packed output of the reference's qkv Linear (fp32 or bf16), d = 32
 *   out  [Bp, N, h*d]      softmax(q k^T d^-0.5) v, same dtype;   lse [Bp, h, N] fp32 (kept for the backward)
 *   dqkv [Bp, N, 3, h, d]  gradient of qkv given d_out (recomputes the probabilities from q, k, lse; no atomics). */
int as_small_attn_fwd(const void* qkv, void* out, float* lse, int Bp, int N, int h, int d, int dtype, as_stream_t stream);
size_t as_small_attn_bwd_workspace_bytes(int Bp, int N, int h);
int as_small_attn_bwd(const void* qkv, const void* out, const void* d_out, const float* lse, void* dqkv, void* workspace,
                      size_t workspace_bytes, int Bp, int N, int h, int d, int dtype, as_stream_t stream);

/* RoIAlign on the stride-16 feature map (mmcv.ops.RoIAlign as configured at
 * configs/mae/attnshift_voc12aug.py:64-68, 123-127; call sites stdroi:2958 and the RoI head's bbox / mask forward):
 * adaptive sampling (sampling_ratio = 0 -> ceil(roi size / out) samples per bin and axis), aligned half-pixel shift,
 * average pooling.  Token-major layouts:
 *   feat [B,H,W,C] fp32, rois [R,5] = (batch index, x1, y1, x2, y2) in image coordinates, out [R, out*out, C] fp32
 *   backward: dfeat [B,H,W,C] is written completely by a deterministic gather (no atomics; C a multiple of 8, maps of up
 *   to 8192 pixels) */
int as_roi_align_fwd(const float* feat, const float* rois, float* out, int B, int H, int W, int C, int R, int out_size,
                     float spatial_scale, int sampling_ratio, int aligned, as_stream_t stream);
int as_roi_align_bwd(const float* dout, const float* rois, float* dfeat, int B, int H, int W, int C, int R, int out_size,
                     float spatial_scale, int sampling_ratio, int aligned, as_stream_t stream);

/* 2-D chamfer distance, the reference's second native op (mmdet/ops/chamfer_2d/src/chamfer_2d.cu:12-161 behind
 * mmdet/ops/chamfer_2d/dist_chamfer_2d.py:11-58; off the hot path): xyz1 [B,n,2], xyz2 [B,m,2] fp32 ->
 * dist1 [B,n] / dist2 [B,m] = squared distance to the nearest point of the other set, idx1 / idx2 int32 its index
 * (lowest on ties); backward: gxyz += 2 * gdist * (p - q) on the point, -= on its neighbour (both outputs written). */
int as_chamfer_2d_fwd(const float* xyz1, const float* xyz2, float* dist1, float* dist2, int32_t* idx1, int32_t* idx2,
                      int B, int n, int m, as_stream_t stream);
int as_chamfer_2d_bwd(const float* xyz1, const float* xyz2, const float* gdist1, const float* gdist2, const int32_t* idx1,
                      const int32_t* idx2, float* gxyz1, float* gxyz2, int B, int n, int m, as_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Part C -- test-time post-processing of the RoI head (csrc/detect_post.hip, csrc/rle.hip, csrc/rpn.hip, csrc/det.hip)
 * ------------------------------------------------------------------------------------------- */

/* Greedy NMS, the mmcv.ops.nms behind mmdet/core/post_processing/bbox_nms.py:84 (batched_nms; IoU without the +1 offset):
 * boxes_sorted [n,4] fp32 (x1,y1,x2,y2) ALREADY in decreasing-score order -> keep_idx [n] int64, the kept positions of
 * that order, compacted and ascending; count [1] int32, how many.  Box j is dropped iff a kept box i < j has
 * IoU(i, j) > iou_thr, with IoU = inter / max(area_i + area_j - inter, 1e-12) evaluated in fp32 exactly as the ATen ops of
 * the host route round it (no contraction, correctly rounded divide, NaN propagating).  max_keep > 0 stops after that many
 * kept boxes (the result is the prefix of the full one); <= 0 keeps all.  Workspace: the pair bit mask,
 * as_nms_workspace_bytes(n) = n * ceil(n / 64) * 8 bytes (0 for n <= 0), 8-byte aligned; boxes 16-byte aligned.
 * n == 0 writes count = 0 (only `count` is touched).  n > 65535 is AS_E_UNSUPPORTED: the mask would pass 512 MB. */
size_t as_nms_workspace_bytes(int n);
int as_nms(const float* boxes_sorted, int n, float iou_thr, int max_keep, long long* keep_idx, int* count, void* workspace,
           size_t workspace_bytes, as_stream_t stream);

/* The mask paste of mae_mask_head_pointSup.py:277-375 (get_seg_masks) and :411-480 (_do_paste_mask) in one pass:
 *   src [n,K,h,w] fp32, labels [n] int64 = the channel of each detection (NULL: channel 0, the class-agnostic head),
 *   boxes [n,4] fp32 (x0,y0,x1,y1) in output-image pixels, out [n,H,W].
 * Output pixel (x, y) of detection i samples its channel bilinearly (grid_sample, align_corners = False, zero padding) at
 *   gx = (x + 0.5 - x0) / (x1 - x0) * 2 - 1,  ix = ((gx + 1) * w - 1) / 2      (the same in y)
 * after the sigmoid when apply_sigmoid (applied to the source values, as the reference takes the sigmoid first).
 * out_mode 0: fp32 values; 1: bytes v >= thr ? 1 : 0; 2: bytes (uint8)(v * 255).  A sample outside (-1, w) x (-1, h)
 * gives v = 0; so does a box of non-positive (or NaN) width or height -- where the reference's inf - inf samples are NaN,
 * i.e. all-zero masks in mode 1 and undefined values in modes 0 / 2 -- and a label outside [0, K).
 * h * w <= 16384 (the channel is staged in LDS), H * W < 2^31, n <= 65535; out 4-byte, boxes 16-byte aligned. */
int as_paste_masks(const float* src, const long long* labels, const float* boxes, void* out, int n, int K, int h, int w,
                   int H, int W, int apply_sigmoid, int out_mode, float thr, as_stream_t stream);

/* COCO run-length encoding of test-time masks on the device (csrc/rle.hip): what mmdet/core/mask/utils.py:36-63
 * (encode_mask_results, pycocotools.mask.encode of every mask in Fortran order) does on the host to every simple_test
 * result (mmdet/apis/test.py:60,100), so that only the encoded strings leave the device.
 *   masks [n,H,W] bytes, row-major, any alignment (as_paste_masks' mode 1 output); ANY NONZERO BYTE COUNTS AS 1.
 * Pixels run column by column (p = x * H + y); the counts alternate between runs of 0 and 1 starting with a run of 0
 * (T value changes -> T + 1 counts); count i is written as x = cnt[i] - cnt[i-2] for i > 2, else cnt[i], in 5-bit groups
 * low first: c = x & 31, x >>= 5, continuation bit 0x20 unless the rest is the sign extension of bit 0x10, byte c + 48
 * (rleEncode + rleToString; at most 7 bytes per count).
 *
 * as_rle_count: totals [n] uint32 = T of every mask (the output size is data dependent: the caller reads the totals back,
 *   as it does as_nms' count), and the scanned cell offsets as_rle_encode needs, left in the workspace.
 * as_rle_encode: the same masks, totals and workspace again.  pos: room for pos_capacity >= sum(T) uint32 (the change
 *   positions, scratch; NULL allowed when pos_capacity = 0).  Mask d's string is written at str + 7 * (sum(T[0..d)) + d)
 *   -- the room of its T + 1 counts -- and lens[d] (uint64) is its length; str_capacity >= 7 * (sum(T) + n) bytes.  Stores
 *   past either capacity are dropped.  Deterministic: every position's place follows from the scan, no atomics.
 * Workspace: as_rle_workspace_bytes(n, H, W) = 8 * (n + 1) + 5 * n * ceil(H / rows) * W bytes (0 when n, H or W <= 0),
 *   8-byte aligned; totals 4-byte, lens 8-byte aligned.  as_rle_tile reports the tiling: rows per row segment (one wave)
 *   and columns per workgroup.
 * n == 0 or H * W == 0 returns 0 without a launch; H * W > 2^31 - 1 or n > 65535 is AS_E_UNSUPPORTED. */
int as_rle_tile(int* rows_per_segment, int* cols_per_workgroup);
size_t as_rle_workspace_bytes(int n, int H, int W);
int as_rle_count(const void* masks, int n, int H, int W, uint32_t* totals, void* workspace, size_t workspace_bytes,
                 as_stream_t stream);
int as_rle_encode(const void* masks, int n, int H, int W, const uint32_t* totals, void* workspace, size_t workspace_bytes,
                  uint32_t* pos, size_t pos_capacity, void* str, size_t str_capacity, unsigned long long* lens,
                  as_stream_t stream);

/* RPN proposal candidates (csrc/rpn.hip): everything mmdet/models/dense_heads/rpn_head.py:82-236 (RPNHead._get_bboxes) does
 * before its batched_nms -- per-level top-k (:162-169), the anchors of mmdet/core/anchor/anchor_generator.py:142-270, the
 * decode of mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:134-237, the minimum-size filter (:221-231) -- and the class
 * offset of mmcv.ops.batched_nms with the level as the class, in three launches for all B images and L levels.
 *   levels [L]: a HOST array of level descriptors, L <= 8: cls = cls_scores[l] [B,A,H,W] fp32, reg = bbox_preds[l]
 *     [B,4A,H,W] fp32 (device pointers), the anchor strides in pixels.
 *   base_anchors [L,A,4] fp32 and img_shapes [B,2] fp32 = (h, w) of every image are device arrays; means_stds is a HOST
 *     array of 8 floats (the 4 means, then the 4 stds); max_ratio = |log(wh_ratio_clip)|.
 * Candidate i = (y * W + x) * A + a of level l has the logit cls[b,a,y,x], the deltas reg[b,4a..4a+3,y,x] and the anchor
 * base_anchors[l][a] + (x * stride_x, y * stride_y, x * stride_x, y * stride_y); no anchor tensor is written.  The total
 * order is (logit descending, level ascending, i ascending), -0.0 == +0.0, any NaN above +inf.  Every (image, level) keeps
 * its first min(nms_pre, n_l) candidates of that order (nms_pre <= 0: all n_l = A * H * W); C = the sum of these over the
 * levels, passed in and checked.  The survivors of an image are decoded (score = 1 / (1 + exp(-logit)); every step but exp
 * rounds as the ATen ops do), those with w or h below min_bbox_size (when > 0) are dropped, and the rest are written in
 * the total order:
 *   cand_box [B,C,4] fp32, cand_nms_box [B,C,4] fp32 = box + level * (M + 1) with M the largest coordinate of the image's
 *   remaining boxes (as_nms' input), cand_score [B,C], cand_level [B,C] and cand_index [B,C] int32 (l and i),
 *   cand_count [B] int32 (= C when min_bbox_size <= 0); rows past the count are not written.
 * Limits: L <= 8, at most 2048 survivors per (image, level) (so nms_pre <= 2048 whenever a level is larger, C <= 16384),
 *   n_l < 2^28, B <= 65535, stride * extent < 2^24; beyond them AS_E_UNSUPPORTED.  Selection reads every logit twice (a
 *   histogram of the keys' first 11 bits, then one collecting pass; four times when more than 4096 keys share the first 11
 *   bits of the k-th one: the radix select then goes on over the other bits), never sorts a level.
 * Workspace: as_rpn_candidates_workspace_bytes(B, C) = 36 * B * C bytes (0 when B or C <= 0), 16-byte aligned like
 *   cand_box and cand_nms_box.  B == 0 returns 0 without a launch. */
typedef struct {
  const float* cls;
  const float* reg;
  int H, W, stride_x, stride_y;
} as_rpn_level;
size_t as_rpn_candidates_workspace_bytes(int B, int C);
int as_rpn_candidates(const as_rpn_level* levels, int L, int B, int A, const float* base_anchors, const float* img_shapes,
                      int nms_pre, float min_bbox_size, const float* means_stds, float max_ratio, int C, float* cand_box,
                      float* cand_nms_box, float* cand_score, int32_t* cand_level, int32_t* cand_index, int32_t* cand_count,
                      void* workspace, size_t workspace_bytes, as_stream_t stream);

/* The box head's detection candidates (csrc/det.hip): everything between the box head's outputs and the NMS of ONE image --
 * BBoxHead.get_bboxes (mmdet/models/roi_heads/bbox_heads/bbox_head.py: softmax, decode, rescale), the decode of
 * mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:134-237, the threshold, gathers and ordering of multiclass_nms
 * (mmdet/core/post_processing/bbox_nms.py:34-93) and the class offset of mmcv.ops.batched_nms -- in five launches without
 * a host sync, decoding only the boxes that pass the threshold.
 *   scores [n,K+1] fp32, the last column the background class (never a candidate); deltas [n,4*Kb] fp32 with Kb = 1 (one
 *   shared / class-agnostic box per RoI) or K, and then rois_or_boxes = the RoIs [n,4]; deltas == NULL: rois_or_boxes
 *   [n,4*Kb] are final boxes, taken as they are (no decode, no clip; the scale still applies).  img_shape (h, w), scale
 *   (4 divisors) and means_stds (the 4 means, then the 4 stds) are HOST arrays; img_shape NULL: no clip, scale NULL: no
 *   rescale, means_stds may be NULL without deltas.  max_ratio = |log(wh_ratio_clip)|.
 * Scores: p = scores, or with apply_softmax p[r,c] = exp(x[r,c] - max_c' x[r,c']) / sum_c' exp(x[r,c'] - max) over the K + 1
 *   columns in fp32 (a correctly rounded divide; the sum in no fixed association).  A row that holds a NaN or +inf has NaN
 *   probabilities, as torch.softmax gives, and so no candidate.  prob_out [n,K+1], when not NULL, receives p.
 * Candidates: all (r, c), c < K, with p[r,c] > score_thr, compared in fp32 (the caller's threshold rounded to fp32, as the
 *   tensor op compares); a NaN never qualifies.  m = their number.
 * Order: score descending, then the flat index r * K + c ascending; -0.0 == +0.0 (a stable descending argsort).
 * Box of (r, c): delta2bbox of RoI r with the deltas of column block c (block 0 when Kb == 1): d = delta * std + mean, dw / dh
 *   clamped to +-max_ratio, (gx, gy) = centre + size * (dx, dy), (gw, gh) = size * exp(dw, dh), corners gx -+ gw / 2, clipped
 *   to [0, w] x [0, h]; every step but exp rounds as the ATen ops of the tensor-op route do (no contraction).  Then each
 *   coordinate j is divided by scale[j], correctly rounded.
 * Outputs, rows 0 .. m-1 in that order (rows past m are not written), cap = min(n * K, 65535) rows each:
 *   cand_box [cap,4] fp32, cand_score [cap] fp32 (the bits of p), cand_roi [cap] int32 (r), cand_label [cap] int32 (c),
 *   cand_nms_box [cap,4] fp32 = cand_box + (float)label * (M + 1), M the largest coordinate of all candidate boxes (NaN
 *   propagating, as Tensor.max()), the fp32 operations in that order: as_nms' input.  cand_count [1] int32 = m.
 *   When m > 65535 (as_nms' limit) only cand_count is meaningful.
 * Limits: n <= 65535, K <= 255, n * K <= 2^20; beyond them AS_E_UNSUPPORTED.  n < 0, K < 1 and Kb outside {1, K} are
 *   AS_E_BADARG.  n == 0 writes cand_count = 0 (when not NULL) and launches nothing else.
 * Workspace: as_det_candidates_workspace_bytes(n, K) = 16 * ceil(cap / 2) + 16 * ceil((n + 1) / 4) + 16 * ceil(n * (K + 1) / 4)
 *   bytes (the keys, the rows' offsets, the probabilities; 0 when n or K <= 0), 16-byte aligned like rois_or_boxes, cand_box
 *   and cand_nms_box. */
size_t as_det_candidates_workspace_bytes(int n, int K);
int as_det_candidates(const float* rois_or_boxes, const float* deltas, int Kb, const float* scores, int apply_softmax, int n,
                      int K, float score_thr, const float* img_shape, const float* scale, const float* means_stds,
                      float max_ratio, float* prob_out, float* cand_box, float* cand_nms_box, float* cand_score,
                      int32_t* cand_roi, int32_t* cand_label, int32_t* cand_count, void* workspace, size_t workspace_bytes,
                      as_stream_t stream);

/* RPN training targets (csrc/rpn_train.hip): what AnchorHead._get_targets_single (mmdet/models/dense_heads/anchor_head.py:
 * 175-271) does per image before the losses, for all B images and L levels, without an anchor tensor or an IoU matrix.
 * Anchor t of an image is level l, i = (y * W_l + x) * A + a, t = offset_l + i, T = the sum of the levels' A * H * W (the
 * order of as_rpn_candidates); its coordinates are base_anchors[l][a] + the grid shift.
 *   levels [L]: a HOST array; only H, W and the strides are read (cls / reg may be NULL).  base_anchors [L,A,4] fp32,
 *   gt_boxes [sum_g,4] fp32 (the boxes of image b are rows gt_offsets[b] .. gt_offsets[b+1]), gt_offsets [B+1] int32 and
 *   shapes [B,4] int32 = (pad_h, pad_w, img_h, img_w) are DEVICE arrays; sum_g and max_g (the largest number of boxes of
 *   one image) are what the host knows of the offsets.
 *
 * as_rpn_assign replaces AnchorGenerator.valid_flags (mmdet/core/anchor/anchor_generator.py:272-328), anchor_inside_flags
 * (mmdet/core/anchor/utils.py:20-46), BboxOverlaps2D and MaxIoUAssigner.assign / assign_wrt_overlaps
 * (mmdet/core/bbox/assigners/max_iou_assigner.py:93-212; gt_max_assign_all = True, no ignore boxes, a float neg_iou_thr):
 *   an anchor is inside when x < min(ceil(pad_w / sx), W_l), y < min(ceil(pad_h / sy), H_l) and, with allowed_border >= 0,
 *   x1, y1 >= -allowed_border, x2 < img_w + allowed_border, y2 < img_h + allowed_border.
 *   assigned [B,T] int32: -2 outside; inside: -1, 0 where 0 <= max_iou < neg_iou_thr, argmax + 1 where max_iou >=
 *     pos_iou_thr (ties to the lowest box), then with match_low_quality for g ascending g + 1 on every anchor whose IoU with
 *     box g equals the box's maximum over the inside anchors when that maximum is >= min_pos_iou; an image without boxes: 0.
 *   max_iou [B,T] fp32 (0 outside and without boxes), counts [B,2] int32 = (positives, negatives).
 *   The IoU is inter / max((area_gt + area_anchor) - inter, 1e-6) with every step one correctly rounded fp32 operation; the
 *   per-box maxima are combined by integer atomic max on the bits (IoUs are >= 0): all outputs are bitwise reproducible.
 *   NaN coordinates do not fault; a NaN IoU compares false everywhere (it is never a maximum), which torch.max would propagate.
 * Workspace: as_rpn_assign_workspace_bytes(B, T, sum_g) = 16 * ceil(sum_g / 4) + 8 * B * ceil(T / 256) bytes (0 when B or
 *   T <= 0 or sum_g < 0), 16-byte aligned: the per-box maxima, then per 256 anchors the scanned (positive, negative) counts
 *   that as_rpn_sample reads -- pass the SAME workspace there.
 *
 * as_rpn_sample replaces the index side of RandomSampler (mmdet/core/bbox/samplers/base_sampler.py:82-100, random_sampler.py:
 * 61-79: gallery[perm] and .unique()): plan [B,4] int32 = (n_pos, all_pos, n_neg, all_neg) and ranks [B,2,num] int32
 *   (positives, then negatives) are device arrays; set s of image b takes n anchors: the ranks[b,s,j]-th positive (assigned
 *   > 0) / negative (assigned == 0) in anchor order, or with `all` the ranks 0 .. n-1.  inds [B,2,num] int32: the anchor
 *   indices t ascending, -1 past n and for ranks outside the set.
 *
 * as_rpn_targets replaces pos_assigned_gt_inds and DeltaXYWHBBoxCoder.encode (mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:
 * 88-130, bbox2delta) of anchor_head.py:237-243: pos_inds rows of inds_stride int32 whose first num entries are anchor
 *   indices or -1; pos_gt [B,num] int32 = assigned - 1 (-1 for no anchor), pos_delta [B,num,4] fp32 =
 *   (((gx - px) / pw, (gy - py) / ph, log(gw / pw), log(gh / ph)) - means) / stds in that operation order (zeros for no
 *   anchor); only logf may round differently from ATen.  means_stds is a HOST array of 8 floats.
 *
 * Limits: L <= 8, a level below 2^28 anchors, stride * extent < 2^24, at most 1024 boxes per image, num <= 2048,
 *   B <= 65535; beyond them AS_E_UNSUPPORTED.  Boxes are assumed finite.  B == 0 returns 0 without a launch. */
size_t as_rpn_assign_workspace_bytes(int B, int T, int sum_g);
int as_rpn_assign(const as_rpn_level* levels, int L, int B, int A, const float* base_anchors, const float* gt_boxes,
                  const int32_t* gt_offsets, int sum_g, int max_g, const int32_t* shapes, float pos_iou_thr, float neg_iou_thr,
                  float min_pos_iou, int match_low_quality, int allowed_border, int32_t* assigned, float* max_iou,
                  int32_t* counts, void* workspace, size_t workspace_bytes, as_stream_t stream);
int as_rpn_sample(int B, int T, int sum_g, int num, const int32_t* assigned, const int32_t* plan, const int32_t* ranks,
                  const void* workspace, size_t workspace_bytes, int32_t* inds, as_stream_t stream);
int as_rpn_targets(const as_rpn_level* levels, int L, int B, int A, const float* base_anchors, const float* gt_boxes,
                   const int32_t* gt_offsets, int sum_g, const int32_t* assigned, const int32_t* pos_inds, int inds_stride,
                   int num, const float* means_stds, int32_t* pos_gt, float* pos_delta, as_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ATTNSHIFT_H */
