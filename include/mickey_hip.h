/* mickey_hip.h -- C ABI of libmickey_hip.so: the MI355X (gfx950) kernels behind the MicKey
 * inference hot path.
 *
 * The reference (nianticlabs/mickey) has no native code and no FFI: every GPU op is an ATen call
 * made from Python.  Each entry point below therefore cites the reference
 * PYTHON call site(s) (file:line under /root/reference) whose arithmetic it replaces; the Python
 * binding a maintainer adds on the reference side is shown in INTEGRATION.md (ctypes).
 *
 * Conventions
 *   - plain C: raw DEVICE pointers (tensor.data_ptr()), explicit sizes/strides, a stream handle
 *     (hipStream_t passed as void*); no torch types.
 *   - every function returns MK_OK (0) or an MK_ERR_* code; mk_last_error() gives the text.
 *   - functions only enqueue work on `stream`: no allocation, no synchronisation, no host<->device
 *     copies.  Scratch memory is passed in by the caller (sizes documented per function).
 *   - re-entrant: no mutable globals besides the thread-local error string (the process-wide schedule
 *     selectors for benchmarks / tests live in mickey_hip_dev.h, not in this ABI); state a kernel reports
 *     (e.g. the saturation word of the split-operand planes) is a per-call argument.
 *   - "lp" (low precision) buffers hold bf16 or fp16 according to `dtype` (MK_BF16 / MK_F16);
 *     accumulation is always fp32.  dtype MK_F32 is the exact parity mode: "lp" buffers hold fp32 and
 *     every contraction runs on the fp32-input MFMA (the reference's FLOAT16: False path and its
 *     always-fp32 heads, mickey_extractor.py:31-35,49-56); about 16x slower, same entry points.
 */
#ifndef MICKEY_HIP_H
#define MICKEY_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mk_stream_t; /* hipStream_t */

enum { MK_OK = 0, MK_ERR_INVALID_ARGUMENT = 1, MK_ERR_LAUNCH = 2 };
enum { MK_BF16 = 0, MK_F16 = 1, MK_F32 = 2 };
enum { MK_ACT_NONE = 0, MK_ACT_RELU = 1, MK_ACT_GELU = 2 };
/* internal epilogue selectors of the GEMM kernel (exposed for tests/tools only) */
enum { MK_EPI_STORE = 0, MK_EPI_LS_RESIDUAL = 1, MK_EPI_QKV = 2, MK_EPI_PATCH = 3 };

int mk_version(void);
const char* mk_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Input pipeline (the caller in FRONT of the hot path)
 * ---------------------------------------------------------------------------------------------- */

/* Decoded frames -> model input: replaces cv2.resize + float + permute(2,0,1) + /255 of read_color_image
 * (lib/datasets/utils.py:61-78; same in demo_inference.py:12-29) for n frames at once.
 *   src  uint8 [n, Hs, Ws, 3] RGB on the device, frame stride stride_img bytes (>= Hs*Ws*3)
 *   dst  fp32  [n, 3, H, W] in [0, 1]
 * cv2.resize(uint8, INTER_LINEAR) exactly as OpenCV 4.8.0 computes it: half-pixel centres, edge clamp, 11-bit fixed-point
 * weights (INTER_RESIZE_COEF_BITS) and its rounding of the two passes, the area-fast path for exact 2x decimation; byte-equal to
 * oracle/input_oracle.py.  Hs == H and Ws == W is the identity resize and gives exactly float(v) / 255. */
int mk_preprocess_u8(const unsigned char* src, long long stride_img, int n, int Hs, int Ws, float* dst, int H, int W,
                     mk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Encoder: DINOv2 ViT/14 (reference lib/models/MicKey/modules/DINO_modules/)
 * ---------------------------------------------------------------------------------------------- */

/* out[M,N] = act(A[M,K] . W[N,K]^T + bias).  A, W lp with K contiguous; out lp or fp32.
 * Replaces nn.Linear call sites: mlp.fc1+GELU (layers/mlp.py:36-37) and the heads' small linears
 * (att_layers/transformer_utils.py:55-57,60,64).  K % 64 == 0, N % 4 == 0, lda/ldw % 8 == 0. */
int mk_gemm(const void* A, int lda, const void* W, int ldw, const float* bias, void* out, int ldc, int M, int N, int K,
            int act, int out_is_f32, int dtype, mk_stream_t stream);

/* `groups` independent GEMMs of identical shape in one launch (element strides per group; a stride
 * of 0 shares the operand).  Used to run the four heads side by side. */
int mk_gemm_grouped(const void* A, int lda, long long strideA, const void* W, int ldw, long long strideW, const float* bias,
                    long long strideBias, void* out, int ldc, long long strideOut, int groups, int M, int N, int K, int act,
                    int out_is_f32, int dtype, mk_stream_t stream);

/* x[M,N] (fp32, in place) += gamma[N] * (A . W^T + bias): attn.proj+ls1+residual and mlp.fc2+ls2+
 * residual (layers/attention.py:60, mlp.py:39, layer_scale.py:27-28, block.py:105-106). */
int mk_gemm_ls_residual(const void* A, int lda, const void* W, int ldw, const float* bias, const float* gamma, float* x,
                        int ldx, int M, int N, int K, int dtype, mk_stream_t stream);

/* attn.qkv (layers/attention.py:51-53): [nimg*ntok, D] x [3D, D]^T + bias, split per head into
 *   q  [nimg, heads, ntok_pad, 64]  (multiplied by qscale = 64^-0.5 * log2(e): the attention kernel
 *                                    exponentiates with exp2)
 *   k  [nimg, heads, ntok_pad, 64]
 *   vt [nimg, heads, 64, ntok_pad]  V transposed, token index stored with bits 2 and 3 swapped
 * Pad rows (token >= ntok) are never written: the caller zero-fills q/k/vt once.  head_dim is 64
 * for every DINOv2 size (S/B/L/g). */
int mk_gemm_qkv(const void* A, int lda, const void* W, int ldw, const float* bias, void* q, void* k, void* vt, int nimg,
                int ntok, int ntok_pad, int heads, float qscale, int dtype, mk_stream_t stream);

/* Patch embedding (layers/patch_embed.py:76-78) + pos-embed add (dinov2.py:198): A = im2col rows
 * [nimg*npatch, K], W = conv weight [D, K]; x[img, 1+p, :] = A.W^T + bias + pos[1+p, :] (fp32). */
int mk_gemm_patch_embed(const void* A, int lda, const void* W, int ldw, const float* bias, const float* pos, float* x,
                        int nimg, int npatch, int D, int K, int dtype, mk_stream_t stream);

/* im2col for the 14x14/stride-14 patch conv.  img fp32 NCHW (3 channels) with explicit element
 * strides (so the /14 crop of mickey_extractor.py:46 is just a smaller gh/gw); out lp
 * [nimg*gh*gw, ldo], column ch*196 + dy*14 + dx, columns 588..ldo-1 zero. */
int mk_im2col_patch14(const float* img, long long stride_img, long long stride_ch, int stride_row, int nimg, int gh,
                      int gw, void* out, int ldo, int dtype, mk_stream_t stream);

/* x[img, 0, :] = cls + pos[0, :]  (dinov2.py:197-198) */
int mk_cls_token(const float* cls, const float* pos, float* x, int nimg, int ntok, int D, mk_stream_t stream);

/* ---- LayerNorm folded into the GEMMs around it (the encoder's pre-norm blocks, block.py:84-88,105-106) ----
 * y = LN(x) . W^T + b  ==  rstd_m * (x . (W diag(w_ln))^T) - rstd_m * mean_m * colsum + (b + W . b_ln).
 * The residual stream x is kept in HBM as TWO 16-bit planes, x = hi + lo with hi = rn16(x), lo = rn16(x - hi): the 4
 * bytes per element of an fp32 stream, 17 (bf16) / 22 (fp16) mantissa bits -- and hi is, as it stands, the raw A operand
 * of the next GEMM.  The GEMM that PRODUCES rows of x (patch embedding, cls row, proj / fc2 + LayerScale + residual)
 * writes hi / lo and the partial row statistics of the fp32 values it rounded; the GEMM that CONSUMES norm1(x) /
 * norm2(x) (qkv, fc1) reads hi and applies mean / rstd per row in its epilogue.  No stand-alone LayerNorm pass and no
 * extra copy of the token matrix remain in a block (ViT-L: 48 passes of fp32 read + 16-bit write each); mk_layernorm
 * stays for the final norm and for the exact-fp32 mode, where x is a plain fp32 matrix.  16-bit dtypes only.
 *   xh, xl  [rows, ldxs] 16 bit;   stats fp32 [rows][N / 64][2]: (sum, sum of squares) of the row over each 64-column
 *           slot (deterministic: one writer per slot, fixed summation order);   N % 64 == 0.
 *   x_f32_out (mk_gemm_ls_residual_ln): if not NULL the updated rows go there as fp32 [M, ldx] and hi / lo / stats are
 *           left alone -- the last block, whose output feeds the final norm.
 *   colsum fp32 [N]: sum_k W'[n][k] over the 16-bit-ROUNDED folded weights (so that the mean term cancels exactly what
 *           the MFMA accumulates);  bias = b + W . b_ln (fp32, folded on the host);  eps as nn.LayerNorm (1e-6).
 *   Row centring (shift_out / shift_in, fp32 [M], each may be NULL = off): LayerNorm is blind to a constant added to all
 *           channels of a row and nothing but LayerNorm reads the residual stream, so the stream may carry a per-row offset.
 *           A consumer publishes every row's current mean in shift_out; the next producer subtracts shift_in while it adds the
 *           branch output.  Rows then stay centred to within one residual update and the 16-bit hi plane rounds x - mean
 *           instead of x: the folded form's operand rounding becomes that of a LayerNorm OUTPUT at any common-mode level. */
int mk_gemm_ls_residual_ln(const void* A, int lda, const void* W, int ldw, const float* bias, const float* gamma, void* xh,
                           void* xl, int ldxs, float* stats, const float* shift_in, float* x_f32_out, int ldx, int M, int N,
                           int K, int dtype, mk_stream_t stream);
int mk_gemm_patch_embed_ln(const void* A, int lda, const void* W, int ldw, const float* bias, const float* pos, void* xh,
                           void* xl, float* stats, int nimg, int npatch, int D, int K, int dtype, mk_stream_t stream);
int mk_cls_token_ln(const float* cls, const float* pos, void* xh, void* xl, float* stats, int nimg, int ntok, int D, int dtype,
                    mk_stream_t stream);
/* Row centring of a freshly produced stream (after mk_gemm_patch_embed_ln + mk_cls_token_ln): every row of hi + lo gets its
 * own mean subtracted in place and its statistics rewritten, so that the first consumer also meets centred rows. */
int mk_recentre_split(void* xh, void* xl, float* stats, long long rows, int D, int dtype, mk_stream_t stream);
/* consumers: mk_gemm (bias, optional GELU, 16-bit output) and mk_gemm_qkv with A = the hi plane [M, K] (lda == K) */
int mk_gemm_ln(const void* A, int lda, const void* W, int ldw, const float* bias, const float* colsum, const float* stats,
               float eps, float* shift_out, void* out, int ldc, int M, int N, int K, int act, int dtype, mk_stream_t stream);
int mk_gemm_qkv_ln(const void* A, int lda, const void* W, int ldw, const float* bias, const float* colsum, const float* stats,
                   float eps, float* shift_out, void* q, void* k, void* vt, int nimg, int ntok, int ntok_pad, int heads,
                   float qscale, int dtype, mk_stream_t stream);

/* LayerNorm over the last dim (dinov2.py:87,230; block.py:84,87; transformer_utils.py:37-38).
 * x fp32 [*, ldx]; output row r reads input row (r / (rows_per_img - skip)) * rows_per_img + skip +
 * r % (rows_per_img - skip)  (skip = 1 drops the CLS token, dinov2.py:233).  out lp or fp32.
 * If resid != NULL (fp32 [rows_out, ldr]): resid += LN(x) and `out` receives the updated resid
 * (transformer_utils.py:64-66).  wgroup_rows > 0: output rows [g*wgroup_rows, (g+1)*wgroup_rows) use
 * w + g*D, b + g*D (the four heads normalised in one launch).
 * bord_h > 0: `out` is a stack of BORDERED feature maps (below, mk_bordered_rows) of bord_m = nimg * bord_h * bord_w pixels
 * each: output row r goes to row (r / bord_m) * mk_bordered_rows(nimg, bord_h, bord_w) + bordered(r % bord_m).  The
 * border rows are not written.  bord_h = 0: dense rows.  ldx, ldo, ldr: multiples of 4 and >= D (ldo / ldr of a null out /
 * resid are not looked at beyond the multiple). */
int mk_layernorm(const float* x, int ldx, const float* w, const float* b, float eps, void* out, int ldo, int out_is_f32,
                 float* resid, int ldr, int rows_out, int D, int rows_per_img, int skip, int wgroup_rows, int bord_h,
                 int bord_w, int bord_m, int dtype, mk_stream_t stream);

/* The encoder's final LayerNorm written CHANNEL-major with the CLS row dropped: what a torch Conv2d stack reads (the
 * reference's heads in a training step: dinov2.py:230-233 x_norm_patchtokens, then mickey_extractor.py:49-52
 * .permute(0, 2, 1).reshape(B, C, h, w).float()).  x fp32 [*, ldx], out fp32 [nimg, D, npix]:
 *   out[(img * D + c) * npix + p] = LN_D(x[(img * rows_per_img + skip + p) * ldx + 0..D-1])[c] * w[c] + b[c]
 * Every value is bit-identical to mk_layernorm's fp32 output of the same rows (same statistics in the same summation order,
 * same normalisation expression; the D <= 128 and D > 128 forms as mk_layernorm dispatches them).  round_fp16 != 0: each value
 * is additionally rounded to the nearest fp16 (ties to even, overflow to inf, NaN kept) and widened back -- what the
 * reference's fp16 encoder hands its heads through .float().  D % 4 == 0, D <= 2048, ldx % 4 == 0, rows_per_img >= skip + npix;
 * x, w and b 16-byte aligned (read as float4, as in mk_layernorm; not checked), out 4-byte aligned; npix is arbitrary.  Deterministic, one writer per element, nothing outside out[0 .. nimg * D * npix) is written. */
int mk_layernorm_nchw(const float* x, int ldx, const float* w, const float* b, float eps, float* out, int nimg, int npix, int D,
                      int rows_per_img, int skip, int round_fp16, mk_stream_t stream);

/* A 128-wide linear and the LayerNorm behind it in one pass (the linear-attention layers of the heads: merge -> norm1 and
 * mlp[2] -> norm2 + the layer's residual, att_layers/transformer_utils.py:58-66): per group g and row r
 *   y = LayerNorm_128(A[g][r, :K] . W[g]^T) * ln_w[g] + ln_b[g];   resid != NULL: resid[g*M + r] += y, out = the updated resid
 * A lp [groups][M, lda], W lp [groups][128, ldw] (no bias), ln_w / ln_b fp32 [groups, 128], resid fp32 [groups * M, ldr], out lp
 * [groups * M, ldo] dense, or (bord_h > 0) a stack of bordered feature maps as in mk_layernorm.  K a multiple of 32, <= 256.  The
 * fp32 GEMM output never reaches memory; K steps are summed in order (the accumulators are mk_gemm_grouped's, bit for bit). */
int mk_gemm_ln128(const void* A, int lda, long long strideA, const void* W, int ldw, long long strideW, const float* ln_w,
                  const float* ln_b, float eps, float* resid, int ldr, void* out, int ldo, int groups, int M, int K, int bord_h,
                  int bord_w, int dtype, mk_stream_t stream);

/* The same LayerNorm writing its rows as the (hi, lo) fp16 operand planes of the split-operand head kernels (mk_conv3x3_split,
 * mk_gemm_grouped_split; AMD.HEADS_DTYPE: split): LN(x) * plane_scale = hi + lo, both [.., ldo] fp16, dense or bordered as above
 * (no fp32 copy, no separate mk_split_planes pass).  out_lo == NULL: only the hi plane is written -- the rows ROUNDED to fp16,
 * what the reference's fp16 encoder hands its heads (mickey_extractor.py:49-52: forward_features(x.to(amp_dtype)) ... .float());
 * a zero-initialised lo plane then stays zero.  sat_flag: see mk_split_planes. */
int mk_layernorm_planes(const float* x, int ldx, const float* w, const float* b, float eps, void* out_hi, void* out_lo, int ldo,
                        float plane_scale, float* resid, int ldr, int rows_out, int D, int rows_per_img, int skip, int wgroup_rows,
                        int bord_h, int bord_w, int bord_m, int* sat_flag, mk_stream_t stream);

/* Non-causal multi-head attention, softmax(q k^T) v with head_dim 64 (layers/attention.py:53-59),
 * flash style (the ntok x ntok matrix is never materialised).  q/k/vt as written by mk_gemm_qkv;
 * out lp [nimg*ntok, ldo] with column head*64 + d.  No output bit depends on what the pad rows (token >= ntok) of q and k hold:
 * pad queries take no part in any wave-wide decision and masked scores are overwritten before use; the pad columns of vt MUST be zero (a masked key
 * has P = 0 exactly and is still multiplied into them). */
int mk_flash_attn_fwd(const void* q, const void* k, const void* vt, void* out, int ldo, int nimg, int heads, int ntok,
                      int ntok_pad, int dtype, mk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Heads (reference lib/models/MicKey/modules/mickey_extractor.py:67-251)
 * ---------------------------------------------------------------------------------------------- */

/* BORDERED feature map: the layout of every activation a 3x3 convolution reads.  Pixel (b, y, x) of a [nimg, H, Wd]
 * grid is row ((b (H+1) + y + 1)(Wd+1) + x + 1) of a [mk_bordered_rows(nimg, H, Wd), C] matrix; all other rows are the
 * zero padding of nn.Conv2d(padding=1) (one shared column between grid rows, one shared grid row between images) and
 * must be zero -- allocate the buffer zeroed once; no kernel of this library ever writes them.  Every 3x3 tap of every
 * pixel is then the same row shift dy (Wd+1) + dx: the implicit GEMM addresses its A operand like a dense matrix (one
 * scalar-addressed LDS-DMA instruction per 8 rows; per-lane tap / border arithmetic cost the round-2 kernel 8 %). */
long long mk_bordered_rows(int nimg, int H, int Wd);

/* 3x3 conv, pad 1, as implicit GEMM over bordered NHWC lp activations, BatchNorm folded into W/bias by the
 * caller (utils/extractor_utils.py:28-35):
 *   out[g][pix, co] = act( sum_{tap,ci} W[g][co, tap*C1+ci] * in1[g][pix+tap, ci]
 *                        + sum_{ci} W[g][co, 9*C1+ci] * in2[g][pix, ci]      (1x1 shortcut, optional)
 *                        + bias[g][co] + resid[g][pix, co] (identity shortcut, optional) )
 * tap = ky*3+kx.  in1, in2, resid: bordered feature maps (resid [.., Cout]).  out_kind: MK_CONV_OUT_DENSE = lp rows
 * [nimg*H*Wd, Cout]; MK_CONV_OUT_BORDERED = lp, bordered (the next conv's input); MK_CONV_OUT_F32 = fp32 dense rows.
 * C1, C2 % 64 == 0; Cout % 4 == 0.  Strides are element strides per group (0 = shared input). */
enum { MK_CONV_OUT_DENSE = 0, MK_CONV_OUT_BORDERED = 1, MK_CONV_OUT_F32 = 2 };
int mk_conv3x3(const void* in1, long long stride_in1, int C1, const void* in2, long long stride_in2, int C2, const void* W,
               int ldw, long long strideW, const float* bias, long long strideBias, const void* resid, long long strideResid,
               void* out, int Cout, long long strideOut, int groups, int nimg, int H, int Wd, int act, int out_kind, int dtype,
               mk_stream_t stream);

/* The same convolution with SPLIT operands -- fp32-grade products on the 16-bit matrix cores (the reference runs its heads in
 * fp32, mickey_extractor.py:53-56; the fp32-input MFMA is 1/16 of the 16-bit rate).  Activations and weights are each held as
 * two fp16 planes, x * s = hi + lo (22 mantissa bits; s a power of two that keeps lo out of fp16's subnormals), and every
 * product is evaluated as hi.hi + lo.hi + hi.lo with fp32 accumulation.  SHARED operands (round 6): a K step of 32 stages the
 * four planes a_hi, a_lo, w_hi, w_lo ONCE in LDS (one 128-byte row = 32 hi | 32 lo elements) and issues the three MFMA sets from
 * those fragments -- L2 -> LDS bytes and LDS fragment reads per product are 2/3 of three plain sweeps'.
 *   in1_hi / in1_lo, in2_hi / in2_lo: bordered fp16 feature maps (mk_split_planes of the fp32 maps, scale s_a); the two planes
 *      of a source must lie within 2 GiB of each other (one allocation); in1_lo == NULL (then without in2): the source IS its
 *      hi plane -- fp16 features of an fp16 encoder -- and hi_w . lo_a is not computed: two MFMA sets per K step instead of three;
 *   W: fp16 [Cout, 2 K], K = 9 C1 + C2: the BatchNorm-folded weights times s_w as INTERLEAVED planes -- for every block of 32
 *      K columns, 32 hi values then 32 lo values (weights.split_conv_weight); an identity shortcut is passed as in2 = the
 *      block input with identity columns in W;
 *   out: out_lo == NULL: fp32 [.., Cout], dense rows or (out_bordered) a bordered feature map; out_lo != NULL: the result
 *      goes out as the NEXT split conv's operand planes instead, fp16 out = hi, out_lo = lo of result * plane_scale (same
 *      layout; saturating at fp16's largest finite value, NaN kept); acc_scale = 1 / (s_a s_w), applied to the accumulators
 *      before bias / activation;
 *   sat_flag: NULL, or a zero-initialised int in device memory that gets bit 0 set when a plane value had to be clamped
 *      (|result * plane_scale| > 65504) or was NaN -- per call, so that two models / streams never share a word.
 *   C1, C2 % 32 == 0. */
int mk_conv3x3_split(const void* in1_hi, const void* in1_lo, long long stride_in1, int C1, const void* in2_hi, const void* in2_lo,
                     long long stride_in2, int C2, const void* W, int ldw, long long strideW, const float* bias,
                     long long strideBias, void* out, void* out_lo, int Cout, long long strideOut, int groups, int nimg, int H,
                     int Wd, int act, int out_bordered, float acc_scale, float plane_scale, int* sat_flag, mk_stream_t stream);

/* fp32 [rows, cols] (row stride ld_src) -> fp16 planes hi = rn16(x scale), lo = rn16(x scale - hi) (saturating at +-65504, NaN
 * kept), each [rows, cols] with row stride ld_dst.  cols, ld_src, ld_dst % 4 == 0.  sat_flag: NULL, or a zero-initialised
 * device int that gets bit 0 set when a value was clamped or NaN (activations are held as x * 64: |x| > 1023 saturates). */
int mk_split_planes(const float* src, long long rows, int cols, long long ld_src, float scale, void* hi, void* lo,
                    long long ld_dst, int* sat_flag, mk_stream_t stream);

/* Grouped GEMM with SPLIT operands (the small linears of the heads' attention layers in AMD.HEADS_DTYPE: split; reference
 * att_layers/transformer_utils.py:51-66 runs them in fp32): out[g] = act(A[g] W[g]^T + bias[g]) with A = (A_hi + A_lo) / s_a
 * as fp16 planes [M, lda] (within 2 GiB of each other) and W fp16 [N, 2 K] = the interleaved (32 hi | 32 lo) planes of the
 * weights times s_w -- hi.hi + lo.hi + hi.lo on the 16-bit matrix cores from operands staged once, fp32 accumulation (as
 * mk_conv3x3_split).  out: fp32 [M, ldc], or with out_lo != NULL the (hi, lo) planes of result * plane_scale.  K % 32 == 0. */
int mk_gemm_grouped_split(const void* A_hi, const void* A_lo, int lda, long long strideA, const void* W, int ldw, long long strideW,
                          const float* bias, long long strideBias, void* out, void* out_lo, int ldc, long long strideOut, int groups,
                          int M, int N, int K, int act, float acc_scale, float plane_scale, int* sat_flag, mk_stream_t stream);

/* ---- Training: the heads' trainable 3x3 convolutions (utils/extractor_utils.py:18-31: nn.Conv2d(k=3, stride=1, padding=1,
 * bias=False), fp32 forward and backward through autograd).  Forward and input gradient are the split convolution above on operand
 * planes made on the device every step; the weight gradient is its own GEMM.  Plane scales follow each tensor's abs-max and live
 * in DEVICE memory: nothing here synchronises with the host.  No atomics: every result is bit-identical from run to run. */

/* mk_conv3x3_split (one source, one group, no bias, no activation, fp32 dense rows out) with the accumulator scale read from
 * DEVICE memory when the kernels run (utils/extractor_utils.py:18-31 in a training step, where the scale follows a tensor's
 * abs-max and the host never learns it): out[pix, co] = acc_scale[0] * sum_{tap, ci} W[co, tap * C1 + ci] * in[pix + tap, ci].
 * The split conv's kernels run with scale 1 and one in-place pass multiplies the rows by acc_scale[0] (a power of two: the same
 * bits as scaling in the epilogue; a NaN scale makes every output NaN).  in_hi / in_lo: bordered fp16 planes within 2 GiB of each
 * other; W: fp16 [Cout, ldw] interleaved planes, ldw >= 18 C1; C1 % 32 == 0, Cout % 4 == 0; out 16-byte aligned. */
int mk_conv3x3_split_dscale(const void* in_hi, const void* in_lo, int C1, const void* W, int ldw, float* out, int Cout, int nimg, int H,
                            int Wd, const float* acc_scale, mk_stream_t stream);

/* Power-of-two plane scale of an fp32 tensor [d0, d1, d2, d3] with element strides s0..s3 (utils/extractor_utils.py:18-31: the
 * operands of the conv and of its backward): scale[0] = s with max|x| * s in [2^14, 2^15) (exponent clamped to +-100), scale[1] =
 * 1 / s.  An all-zero tensor gives s = 1; a tensor with an Inf or NaN gives s = 1 and scale[1] = NaN, so that whatever is computed
 * with its planes comes out non-finite.  Two launches, deterministic.  work: mk_absmax_scale_work_floats() floats; scale: 2. */
long long mk_absmax_scale_work_floats(void);
int mk_absmax_scale(const float* x, int d0, int d1, int d2, int d3, long long s0, long long s1, long long s2, long long s3,
                    float* work, float* scale, mk_stream_t stream);

/* Operand planes of a training conv (utils/extractor_utils.py:18-31).  A plane buffer is a zero-initialised fp16 matrix of
 * mk_conv_train_plane_rows(nimg, H, Wd) rows whose row mk_conv_train_lead_rows(Wd) is row 0 of the bordered feature map: the
 * weight-gradient kernel sweeps whole K steps of 32 rows with one row shift per tap and no bounds test, so Wd + 2 rows in front
 * of the map and the rows behind it up to the buffer's end must exist.  What they must hold depends on the operand: in gY's
 * buffers the rows behind the map must be zero, like its border rows (they are summed; the rows in front are never read); in X's
 * buffers the rows in front of and behind the map only ever meet zero rows of gY and need to be FINITE, no more (an Inf or NaN
 * times zero would reach dw), and likewise gY's columns Cout .. ldg - 1, whose results are dropped.  A zero-initialised buffer
 * (ops.conv_train_plane_buffer) satisfies all of it; tests/test_conv_edges_gpu.py holds dw bit-identical between zero and finite
 * non-zero fillings.  hi / lo point at bordered row 0.
 * mk_conv_train_planes: fp32 [nimg, C, H, Wd] with element strides (contiguous, channels_last, sliced ...) -> x * scale[0] = hi +
 * lo, [.., ld] fp16 (no clamping: an Inf gives Inf / NaN planes); C % 4 == 0, ld % 4 == 0, ld >= C; columns C .. ld - 1 and all
 * border rows are left alone. */
long long mk_conv_train_lead_rows(int Wd);
long long mk_conv_train_plane_rows(int nimg, int H, int Wd);
int mk_conv_train_planes(const float* src, long long stride_b, long long stride_c, long long stride_h, long long stride_w, int nimg,
                         int C, int H, int Wd, const float* scale, void* hi, void* lo, int ld, mk_stream_t stream);

/* fp32 weight [Cout, Cin, 3, 3] (contiguous; utils/extractor_utils.py:18-31) -> the interleaved (32 hi | 32 lo) planes of
 * w * w_scale[0] that mk_conv3x3_split reads (weights.split_conv_weight):
 *   transposed == 0: fp16 [Cout, 2 * 9 Cin], column tap * Cin + ci -- the forward;
 *   transposed != 0: fp16 [Cin, 2 * 9 Cp], column tap * Cp + co of w[co, ci, 2 - ky, 2 - kx], Cp = Cout rounded up to 32, zero for
 *     co >= Cout -- the conv that turns gY's planes [.., Cp] into the input gradient.
 * acc_scale[0] = w_scale[1] * act_scale[1]: the accumulator scale of that conv (act_scale: the scale of its activation planes).
 * Cin % 32 == 0, Cout % 4 == 0. */
int mk_conv_train_weight_planes(const float* w, int Cout, int Cin, int transposed, const float* w_scale, const float* act_scale,
                                void* planes, float* acc_scale, mk_stream_t stream);

/* Weight gradient of the 3x3 conv (utils/extractor_utils.py:18-31 under autograd):
 *   dw[co, ci, ky, kx] = sum over bordered rows r of gY[r, co] * X[r + (ky - 1)(Wd + 1) + kx - 1, ci]
 * gy_hi / gy_lo [.., ldg] and x_hi / x_lo [.., Cin]: plane buffers as above (scales gy_scale, x_scale); ldg % 32 == 0, ldg >= Cout.
 * Split-fp16 A^T . B on the matrix cores (gY_hi.X_hi + gY_lo.X_hi + gY_hi.X_lo, fp32 accumulation), rows cut into fixed chunks
 * whose partial sums (work: mk_conv_wgrad_work_floats floats) are added in chunk order.  dw: fp32 [Cout, Cin, 3, 3].
 * Cin % 32 == 0, Cout % 4 == 0; planes, work and dw 16-byte aligned. */
long long mk_conv_wgrad_work_floats(int Cout, int Cin, int nimg, int H, int Wd);
int mk_conv_wgrad(const void* gy_hi, const void* gy_lo, int ldg, const void* x_hi, const void* x_lo, int Cout, int Cin, int nimg, int H,
                  int Wd, const float* gy_scale, const float* x_scale, float* work, float* dw, mk_stream_t stream);

/* Start of Transformer_self_att (att_layers/transformer.py:92-95): xs = x + pe (fp32 stream) and an
 * lp copy into columns [0,C) of a [rows, ld_cat] buffer.  x lp [G][rows, C]; pe fp32 [npix, C] or NULL. */
int mk_posenc_add(const void* x, const float* pe, float* xs, void* cat, int ld_cat, int groups, int nimg, int npix, int C,
                  int dtype, mk_stream_t stream);

/* Linear attention (att_layers/attention.py:46-64), heads of 16 channels.
 * qkv fp32 [G][nimg*L, 3C] (q | k | v).  Step 1 computes per (g, img, head)
 *   KV[16][16] = sum_s (elu(k_s)+1) (x) v_s / L   and   Ksum[16] = sum_s (elu(k_s)+1)
 * into kv fp32 [G*nimg*(C/16)][272], deterministically (per-chunk partials in `work`, then a fixed-
 * order reduction).  work: mk_linattn_work_floats(G, nimg, L, C) fp32 elements. */
long long mk_linattn_work_floats(int groups, int nimg, int L, int C);
int mk_linattn_kv(const float* qkv, float* kv, float* work, int groups, int nimg, int L, int C, mk_stream_t stream);
/* Step 2: msg[s, h*16+v] = (phi(q_s) . KV[:, v]) * L / (phi(q_s) . Ksum + 1e-6), written lp to
 * out [G][nimg*L, ldo].  C % 16 == 0, C <= 128 (what mk_linattn_kv can produce kv for), ldo % 8 == 0, ldo >= C. */
int mk_linattn_apply(const float* qkv, const float* kv, void* out, int ldo, int groups, int nimg, int L, int C, int dtype,
                     mk_stream_t stream);

/* Steps 1 and 2 with the projections inside (C = 128, 16-bit operands: the heads' default path).  x lp [G][nimg*L, lda] holds the
 * layer's input rows (columns [0, C)), qkv_w lp [G][3C, ldw] the rows of q | k | v.  Nothing of q, k, v reaches memory.
 * mk_linattn_kv_fused: kv and work exactly as mk_gemm_grouped (fp32 out) -> mk_linattn_kv leave them, bit for bit (the same
 * accumulators, the same order of every sum).
 * mk_linattn_apply_fused: with merge_w lp [G][C, ldwm] and ln_w / ln_b fp32 [G, C] the rows
 *   LayerNorm_C(msg . merge_w^T) * ln_w + ln_b   (mk_gemm_grouped -> mk_linattn_apply -> mk_gemm_ln128, bit for bit)
 * are written lp to out [G][nimg*L, ldo]; merge_w == NULL: out receives msg itself (mk_linattn_apply's rows).  out may be other
 * columns of the rows x is read from.  x, qkv_w, merge_w, kv 16-byte aligned, out 8-byte aligned, strides in elements. */
int mk_linattn_kv_fused(const void* x, int lda, long long strideX, const void* qkv_w, int ldw, long long strideW, float* kv,
                        float* work, int groups, int nimg, int L, int C, int dtype, mk_stream_t stream);
int mk_linattn_apply_fused(const void* x, int lda, long long strideX, const void* qkv_w, int ldw, long long strideW, const float* kv,
                           const void* merge_w, int ldwm, long long strideWm, const float* ln_w, const float* ln_b, float eps,
                           void* out, int ldo, long long strideOut, int groups, int nimg, int L, int C, int dtype,
                           mk_stream_t stream);

/* The same linear attention for TRAINING (att_layers/attention.py:46-64 under autograd), forward and backward, all fp32.
 * Per image n and head h (16 channels), phi(x) = elu(x) + 1, phi'(x) = 1 for x > 0, else phi(x):
 *   forward   M[d, v] = sum_s phi(k)[s, d] (v[s, v] / S),  ks[d] = sum_s phi(k)[s, d]
 *             den[l] = phi(q)[l] . ks + eps,  out[l, v] = (phi(q)[l] . M[:, v]) / den[l] * S
 *   backward  gnum[l, v] = go[l, v] S / den[l],  gden[l] = -(go[l] . out[l]) / den[l]      (out and den recomputed from q, M, ks)
 *             gq[l, d] = (sum_v gnum[l, v] M[d, v] + gden[l] ks[d]) phi'(q[l, d])
 *             gM[d, v] = sum_l phi(q)[l, d] gnum[l, v],  gks[d] = sum_l phi(q)[l, d] gden[l]
 *             gk[s, d] = (sum_v (v[s, v] / S) gM[d, v] + gks[d]) phi'(k[s, d]),  gv[s, v] = (sum_d phi(k)[s, d] gM[d, v]) / S
 * q [nimg][L rows], k, v [nimg][S rows]: three separate fp32 operands of C = 16 H channels per row, each with its own row stride
 * (ld*, elements, >= C) and image stride (s*, elements); pointers 16-byte aligned, strides multiples of 4.  L and S may differ.
 *   out  fp32 [nimg * L, C] dense
 *   kv   fp32 [nimg * (C / 16)][272]: M (16 x 16, d-major) | ks per (image, head), the layout of mk_linattn_kv; written by the
 *        forward, read by the backward (what a caller keeps between the two, besides q, k and v)
 *   go   fp32 [nimg * L, C] dense;  gq [nimg * L, C], gk, gv [nimg * S, C] dense, each may be NULL (not wanted: not computed)
 *   gkv  fp32 [nimg * (C / 16)][272] scratch (gM | gks), work: mk_linattn_train_work_floats(nimg, L, S, C) fp32 elements; both
 *        may be NULL when gk and gv are
 * Both token sums are deterministic: per-chunk partials in `work`, added in chunk order, no atomics; an image's results do not
 * depend on the other images of the call.  3 launches forward; backward 3, or 1 when neither gk nor gv is wanted.
 * eps is a per-call argument.  C % 16 == 0, C <= 128, nimg <= 65535. */
long long mk_linattn_train_work_floats(int nimg, int L, int S, int C);
int mk_linattn_train_fwd(const float* q, long long ldq, long long sq, const float* k, long long ldk, long long sk, const float* v,
                         long long ldv, long long sv, float eps, float* out, float* kv, float* work, int nimg, int L, int S, int C,
                         mk_stream_t stream);
int mk_linattn_train_bwd(const float* q, long long ldq, long long sq, const float* k, long long ldk, long long sk, const float* v,
                         long long ldv, long long sv, const float* kv, const float* go, float eps, float* work, float* gkv, float* gq,
                         float* gk, float* gv, int nimg, int L, int S, int C, mk_stream_t stream);

/* The rest of the heads' EncoderLayer for TRAINING (att_layers/transformer_utils.py:40-66 under autograd): its bias-free
 * nn.Linears and its two LayerNorm(128), forward and backward, all fp32.  Contractions on the fp32-input MFMA (an exact fp32 fma
 * chain) in an order fixed by the shape: bit-identical from run to run, a row of a forward / input-gradient result does not depend
 * on the other rows, gradients are bit-linear in the incoming gradient under a power-of-two scale; no atomics, no host sync.
 * All pointers 16-byte aligned, all row strides (elements) multiples of 4 and >= the row's width.
 *
 * mk_train_linear_fwd (transformer_utils.py:55-57,59,63: q_proj / k_proj / v_proj, merge, mlp[0] + ReLU on the concat, mlp[2]):
 *   out[M, N] = act([A1 | A2] . W^T),  A1 [M, K1], A2 [M, K2] (K2 == 0: one source), W [N, K1 + K2] dense in nn.Linear's layout;
 *   relu != 0: act = max(., 0) (a NaN stays a NaN).  wsplit != 0: W is three dense matrices w | w2 | w3 of wsplit rows each
 *   (N == 3 wsplit; wq | wk | wv read where they lie).  K1, K2 multiples of 16, N of 4.
 * mk_train_linear_ln128_fwd (transformer_utils.py:59-60 and 63-66: merge + norm1, mlp[2] + norm2 + the residual, one pass):
 *   out[M, 128] = LayerNorm_128([A1 | A2] . W^T) gamma + beta (+ resid), the row statistics taken in the accumulators; xhat [M, 128]
 *   and rstd [M] (either may be NULL) as mk_train_ln128_fwd leaves them (another summation order: not the same bits).
 * mk_train_linear_dgrad (the input gradient of the same Linears):
 *   [o1 | o2][M, K1 + K2] (+)= (G[M, N] . W[N, K1 + K2]) with an exact zero wherever mask[m, j] <= 0 (mask NULL: none; mlp[1]'s ReLU
 *   backward behind mlp[2]'s input gradient).  Columns [0, K1) go to o1, [K1, K1 + K2) to o2 (mlp[0]'s gradient lands as gx and gm
 *   without a split); accumulate bit 0 / bit 1 adds to what o1 / o2 holds (one writer per element).  N a multiple of 16, K1, K2 of 4.
 *   gsplit != 0: G lies as N / gsplit planes of gsplit columns, gplane elements apart, rows ldg apart (gq | gk | gv as
 *   mk_linattn_train_bwd leaves them; gsplit a multiple of 16); the same for mk_train_linear_wgrad.
 * mk_train_linear_wgrad (the weight gradient):
 *   part[c * chunk_stride + n (K1 + K2) + k] = sum over the rows m of chunk c of G[m, n] [A1 | A2][m, k],  c < chunks; chunk c is
 *   rows [c rows_per_chunk, (c + 1) rows_per_chunk) (a chunk past M gets zeros).  mk_train_rows_per_chunk(M) / mk_train_chunks(M)
 *   give the chunking of an M-row call: whole steps of 128 rows, at most 32 chunks, a function of M alone.
 * mk_train_tail (one launch for every partial sum of a backward pass):
 *   out[j] = sum_c wpart[c wstride + j], j < nw, and out[nw + j] = sum_s lpart[s lstride + j], j < nl, both in index order.
 * mk_train_ln128_fwd (transformer_utils.py:60,64,66: norm1, norm2 and the residual):
 *   xhat = (u - mean) rstd, out = xhat gamma + beta (+ resid), rows of 128; xhat [M, 128] and rstd [M] (either may be NULL) are what
 *   the backward needs.
 * mk_train_ln128_bwd:
 *   gu = rstd (gamma g - mean(gamma g) - xhat mean(gamma g xhat)) (gu NULL: not wanted), and per step s of 128 rows
 *   part[s part_stride + 0..127] = sum_m g xhat (gamma's gradient), part[s part_stride + 128..255] = sum_m g (beta's); part NULL:
 *   not wanted.  mk_train_ln_steps(M) steps. */
int mk_train_rows_per_chunk(int M);
int mk_train_chunks(int M);
int mk_train_ln_steps(int M);
int mk_train_linear_fwd(const float* a1, long long lda1, int K1, const float* a2, long long lda2, int K2, const float* w,
                        const float* w2, const float* w3, int wsplit, float* out, long long ldo, int M, int N, int relu,
                        mk_stream_t stream);
int mk_train_linear_ln128_fwd(const float* a1, long long lda1, int K1, const float* a2, long long lda2, int K2, const float* w,
                              const float* gamma, const float* beta, float eps, const float* resid, long long ldr, float* out,
                              float* xhat, float* rstd, int M, mk_stream_t stream);
int mk_train_linear_dgrad(const float* g, long long ldg, long long gplane, int gsplit, const float* w, const float* w2, const float* w3, int wsplit,
                          const float* mask, long long ldmask, float* o1, long long ldo1, int K1, float* o2, long long ldo2, int K2,
                          int accumulate, int M, int N, mk_stream_t stream);
int mk_train_linear_wgrad(const float* g, long long ldg, long long gplane, int gsplit, const float* a1, long long lda1, int K1, const float* a2, long long lda2,
                          int K2, float* part, long long chunk_stride, int rows_per_chunk, int chunks, int M, int N,
                          mk_stream_t stream);
int mk_train_tail(const float* wpart, long long wstride, int wchunks, long long nw, const float* lpart, long long lstride,
                  int lsteps, long long nl, float* out, mk_stream_t stream);
int mk_train_ln128_fwd(const float* u, const float* gamma, const float* beta, float eps, const float* resid, long long ldr,
                       float* out, float* xhat, float* rstd, int M, mk_stream_t stream);
int mk_train_ln128_bwd(const float* g, const float* xhat, const float* rstd, const float* gamma, float* gu, float* part,
                       long long part_stride, int M, mk_stream_t stream);

/* The head tails for TRAINING (mickey_extractor.py:98-124 remove_borders / remove_brd_and_softmax, 134-140 the detector's score conv,
 * 172-176 xy_offset + sigmoid, 211-216 depth (+ max_depth sigmoid), 248-249 with utils/extractor_utils.py:6-10 desc_l2norm, all
 * under autograd; mk_head_tails below is their inference form).  fp32, vector ALU only; every sum in an order fixed by the shape
 * (no atomics, no host sync): bit-identical from run to run, an image's forward and input-gradient rows do not depend on the other
 * images, gradients are bit-linear in the incoming gradient under a power-of-two scale.  feat / gfeat / x / gx are dense rows
 * [nimg n, C] (channels_last memory), n = h wd pixels per image, C a multiple of 4 in [4, 256], 16-byte aligned.
 *
 * mk_train_headtail_fwd: z[o, p] = sum_c feat[p, c] w[o, c], o < Cout in {1, 2}, w [Cout, C] dense; out [nimg, Cout, n] =
 *   MK_TAIL_IDENTITY        z                                                              (depth)
 *   MK_TAIL_SIGMOID         scale sigmoid(z)                    (offset: scale 1; depth with use_depth_sigmoid: scale max_depth)
 *   MK_TAIL_MASKED_SIGMOID  in_p sigmoid(z),  in_p = 1 on pixels at least `border` from every edge, else 0       (Cout == 1)
 *   MK_TAIL_SOFTMAX         per image: mean = sum_p z_p / n + eps over ALL pixels (a constant of the backward: the reference detaches
 *                           it), e_p = in_p exp((z_p - mean) / temperature), y_p = e_p / (sum_p e_p + eps)       (Cout == 1;
 *                           a second launch, one workgroup per image)
 * mk_train_headtail_bwd: g, y [nimg, Cout, n] (y = the forward's output; unused for MK_TAIL_IDENTITY).
 *   gz = g (identity),  g y (1 - y / scale) (both sigmoids; the masked one with scale 1: y == 0 outside the border),
 *   gz_p = (y_p / temperature) (g_p - dot_img) with dot_img = sum_q g_q y_q over the image's pixels (softmax: exact including eps,
 *   dy_i/dz_k = (delta_ik y_i - y_i y_k) / temperature; dot [nimg] is work memory, written by a launch of its own).
 *   gfeat[p, c] = sum_o gz[o, p] w[o, c]  (gfeat NULL: not wanted, no pass over it);
 *   gw[o, c] = sum_p gz[o, p] feat[p, c]  (gw NULL: not wanted, feat is not read): chunk k of mk_train_headtail_chunk_rows() rows
 *   leaves its sum in part[k Cout C ..], mk_train_headtail_chunks(rows) chunks (a function of the row count alone), which a last
 *   launch adds in chunk order (sixteen consecutive runs of chunks, then the sixteen sums in order).  At most 3 launches; none
 *   when neither output is wanted.
 * mk_train_desc_l2norm_fwd: y[img, c, p] = x[p, c] rnorm_p, rnorm_p = 1 / sqrt(sum_c x[p, c]^2 + eps); y [nimg, C, n] (transposed,
 *   the layout the matcher reads), rnorm [nimg n] (NULL: not kept).  The bits of mk_head_tails' dsc.
 * mk_train_desc_l2norm_bwd: gx[p, c] = rnorm_p (g[img, c, p] - y[img, c, p] sum_c g[img, c, p] y[img, c, p]), g and y [nimg, C, n]. */
enum { MK_TAIL_IDENTITY = 0, MK_TAIL_SIGMOID = 1, MK_TAIL_MASKED_SIGMOID = 2, MK_TAIL_SOFTMAX = 3 };
int mk_train_headtail_chunk_rows(void);
int mk_train_headtail_chunks(long long rows);
int mk_train_headtail_fwd(const float* feat, const float* w, float* out, int nimg, int h, int wd, int C, int Cout, int act,
                          float scale, int border, float temperature, float eps, mk_stream_t stream);
int mk_train_headtail_bwd(const float* g, const float* y, const float* feat, const float* w, float* dot, float* gfeat, float* part,
                          float* gw, int nimg, int n, int C, int Cout, int act, float scale, float temperature,
                          mk_stream_t stream);
int mk_train_desc_l2norm_fwd(const float* x, float* y, float* rnorm, int nimg, int n, int C, float eps, mk_stream_t stream);
int mk_train_desc_l2norm_bwd(const float* g, const float* y, const float* rnorm, float* gx, int nimg, int n, int C,
                             mk_stream_t stream);

/* The glue of the heads' BasicBlock for TRAINING (utils/extractor_utils.py:12-35 under autograd; 16 blocks per model,
 * mickey_extractor.py:76-79,155-158,194-197,232-235): nn.BatchNorm2d (extractor_utils.py:19,21) with the residual add (:32) and
 * F.relu (:30,33-34) in the same pass, forward and backward.  The bias-free 1x1 shortcut (:23-26,29) is mk_train_linear_* above.
 * fp32 data, vector ALU only; the forward computes in fp32, the backward's per-channel sums and x - mean terms in fp64 (below).
 * Rows are [M, C], channels innermost (channels_last memory, M = B H W), C a multiple of 4 in [4, 1024], row
 * strides (elements) multiples of 4 and >= C, every pointer 16-byte aligned.  Every per-channel sum runs over chunks of
 * mk_train_bn_chunk_rows() rows (mk_train_bn_chunks(M) of them, a function of M alone): 16 row slots in slot order, then the chunks
 * in chunk order (four consecutive runs, then the four sums in order).  No atomics, no host sync, bit-identical from run to run; a
 * launch writes the chunk partials into work (mk_train_bn_work_floats(M, C) floats: the backward's four rows of C doubles per chunk, of which the forward uses two rows of floats) and the next launch combines them in its
 * prologue, every workgroup for its own 64 channels.
 *
 * mk_train_bn_fwd: y = act(xhat gamma + beta (+ resid)), xhat = (x - mean) rstd, rstd = 1 / sqrt(var + eps), act = max(., 0) with
 *   relu != 0 (a NaN stays a NaN), resid NULL: none.
 *   training != 0 (2 launches; M > 1): mean and the biased var of the batch.  Launch 1 leaves per chunk its mean (taken as K + sum(x - K)
 *   / n, K the chunk's first row) and its sum of squares about that mean; launch 2 combines them as centred moments,
 *   mean = m_0 + sum_k n_k (m_k - m_0) / M, var = sum_k (M2_k + n_k (m_k - mean)^2) / M: a channel mean 1000 times its spread costs no
 *   digits.  The workgroups of chunk 0 then write running_mean = (1 - momentum) running_mean + momentum mean, running_var likewise
 *   with var M / (M - 1), and num_batches_tracked += 1 (the module's int64 buffer where it lies in device memory).
 *   training == 0 (1 launch): mean = running_mean, var = running_var; nothing is updated, work may be NULL.
 *   mean [C], rstd [C]: what the backward needs (either may be NULL: not kept).  mask [M, C] bytes, dense: 1 where y > 0 (relu only;
 *   NULL: not kept).  A NaN or Inf in x reaches every output of its channel in training, its own element in eval.
 * mk_train_bn_bwd (2 launches): g' = g where mask != 0, else 0 (mask NULL: g' = g; no ReLU).  xhat is recomputed from x, mean, rstd.
 *   Launch 1 leaves per chunk sum g', sum g' (x - mean), sum (x - mean)^2 and sum (x - mean), taken in double.  In training the
 *   variance is retaken from them about mean + delta, delta = mean(x - mean) being the rounding the fp32 mean carries, and launch 2
 *   forms x - mean - delta in double too, so that g' (1 - xhat^2), all that is left of gx when a channel has a handful of rows, keeps
 *   its digits (eps: the forward's).  Launch 2 combines the partials and writes
 *   gx = gamma rstd (g' - mean(g') - xhat mean(g' xhat))   (training == 0: gamma rstd g'),   gresid = g',
 *   and from the workgroups of chunk 0 dgamma = sum g' xhat, dbeta = sum g'.  gx, gresid, dgamma, dbeta: NULL = not wanted (without
 *   gx and gresid launch 2 is one chunk tall; with none of the four nothing is launched).  Gradients are bit-linear in g under a
 *   power-of-two scale; a NaN in g reaches every gradient of its channel in training. */
int mk_train_bn_chunk_rows(void);
int mk_train_bn_chunks(long long M);
long long mk_train_bn_work_floats(long long M, int C);
int mk_train_bn_fwd(const float* x, long long ldx, const float* gamma, const float* beta, const float* resid, long long ldr,
                    float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps, float* work,
                    float* y, long long ldy, float* mean, float* rstd, unsigned char* mask, int M, int C, int relu, int training,
                    mk_stream_t stream);
int mk_train_bn_bwd(const float* g, long long ldg, const float* x, long long ldx, const float* gamma, const float* mean,
                    const float* rstd, const unsigned char* mask, float* work, float* gx, long long ldgx, float* gresid,
                    long long ldgr, float* dgamma, float* dbeta, float eps, int M, int C, int training, mk_stream_t stream);

/* The tail of a training step (lib/models/MicKey/model.py:104-145): the isnan / isinf checks of :104-108 and :140 (six host
 * synchronisations there), torch.nn.utils.clip_grad_norm_ (:137) and torch.optim.Adam.step (:145; created at :284 with eps = 1e-6), as three
 * launches without a host synchronisation.  fp32 tensors, vector ALU only; the sums of squares and the bias corrections in fp64.
 *
 * The kernels follow a TABLE in device memory, one mk_optim_row per tensor, and a CHUNK MAP next to it: the tensors are cut into
 * chunks of mk_optim_chunk_elems() elements (mk_optim_chunks(numel) per tensor, a function of numel alone; a chunk never spans two
 * tensors), and entry c of the map is two ints, the row of chunk c and its index inside that tensor.  One workgroup runs one chunk.
 * The library cannot look into the table: the caller vouches that every pointer of a row addresses numel fp32 elements (any memory
 * order: the ops are element-wise, the four tensors of a row share one order) and that the map's entries lie inside the table.  An
 * entry that names no row, or a chunk past its tensor's end, is skipped.  A tensor is read and written with 16-byte accesses when
 * every pointer the kernel follows for it is 16-byte aligned, with dword accesses otherwise; results do not depend on which.
 *   p, m, v   parameter, exp_avg, exp_avg_sq (MK_OPTIM_PARAM rows; NULL on a row that is only checked)
 *   g         the gradient, or a tensor that is only checked for NaN / Inf
 *   step      mk_optim_chunks(numel) fp32 cells that all hold the tensor's step count: the workgroup of chunk i reads and writes
 *             cell i alone, so that no workgroup reads a cell that another one writes in the same launch
 *   flags     MK_OPTIM_NORM: g counts towards the norm; MK_OPTIM_PARAM: the row takes the Adam update
 *
 * mk_optim_grad_stats: partials[c] (2 chunks doubles, 16-byte aligned) = { s, s on a MK_OPTIM_NORM row else 0 }, s = the sum of g^2
 *   over chunk c in double, lanes in a fixed order.  An fp32 square cannot overflow a double: s is non-finite exactly when the
 *   chunk holds a NaN or an Inf.
 * mk_optim_reduce (one workgroup): adds both columns in chunk order and writes state[4] = { ok, total_norm, clip_coef, 0 }:
 *   ok = 1 when every partial is finite, else 0; total_norm = sqrt(sum over the MK_OPTIM_NORM rows), rounded once to fp32;
 *   clip_coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 as clip_grad_norm_ computes it, 1 with max_norm < 0 (no clipping).
 * mk_optim_adam: over the first `chunks` entries of the map (the caller puts the MK_OPTIM_PARAM rows first).  state[0] == 0: returns
 *   without touching anything.  Else g' = g clip_coef (stored back to g only when clip_coef < 1), g' += weight_decay p when
 *   weight_decay != 0, and with t = step + 1:  m = beta1 m + (1 - beta1) g',  v = beta2 v + (1 - beta2) g'^2,
 *   p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps);  step = t.  The scalars in double once per workgroup, the
 *   element math in fp32.  Plain Adam is this launch alone with state = { 1, -, 1, - }.
 * No atomics; bit-identical from run to run. */
typedef struct mk_optim_row {
  float *p, *g, *m, *v, *step;
  long long numel;
  double lr, beta1, beta2, eps, weight_decay;
  long long flags;
} mk_optim_row; /* 96 bytes */
#define MK_OPTIM_NORM 1
#define MK_OPTIM_PARAM 2
int mk_optim_chunk_elems(void);
long long mk_optim_chunks(long long numel);
int mk_optim_grad_stats(const mk_optim_row* table, int rows, const int* chunk_map, int chunks, double* partials, mk_stream_t stream);
int mk_optim_reduce(const double* partials, int chunks, float max_norm, float* state, mk_stream_t stream);
int mk_optim_adam(const mk_optim_row* table, int rows, const int* chunk_map, int chunks, const float* state, mk_stream_t stream);

/* Head tails (mickey_extractor.py:134-138,173-176,213-216,246-249 and
 * compute_correspondences.py:20-31).  feat* fp32 [nimg*h*w, C] (resblock4 outputs).
 *   scr   [nimg, h*w]      border-masked temperature-100 softmax (or sigmoid) of w_score . feat_det
 *   kps   [nimg, 2, h*w]   (sigmoid(w_xy . feat_off) + cell) * down   (x row, then y row)
 *   depth [nimg, h*w]      w_depth . feat_depth  (max_depth * sigmoid(.) if use_depth_sigmoid)
 *   dsc   [nimg, Cd, h*w]  feat_dsc / sqrt(sum_c feat_dsc^2 + 1e-10) if norm_dsc, transposed
 * h * w + 32 floats and Cd * 65 floats of LDS, each up to 160 KiB (reserved on the first call). */
int mk_head_tails(const float* feat_det, const float* w_score, const float* feat_off, const float* w_xy,
                  const float* feat_depth, const float* w_depth, const float* feat_dsc, float* scr, float* kps, float* depth,
                  float* dsc, int nimg, int h, int w, int C, int Cd, int border, int use_softmax, int use_depth_sigmoid,
                  float max_depth, int norm_dsc, float down, mk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Matcher (reference lib/models/MicKey/modules/utils/feature_matcher.py)
 * ---------------------------------------------------------------------------------------------- */

/* dualSoftmax.forward (feature_matcher.py:64-83) + kp_matrix_scores (compute_correspondences.py:46-50)
 * + final_scores (compute_pose.py:23), exact-fp32 MFMA correlation.
 *   dsc0 [B, C, n0], dsc1 [B, C, n1] fp32;  scr0 [B, n0], scr1 [B, n1] fp32 (may be NULL with kp/final NULL)
 *   scores / kp_scores / final_scores [B, n0, n1] fp32, each may be NULL (lean mode).
 *   use_dustbin: append the scalar `dustbin` as extra row/column/corner before both softmaxes.
 *   work: fp32 scratch, mk_dual_softmax_work_floats(B, n0, n1, own_copy) elements, 16-byte aligned: the softmax partials,
 *          plus -- with own_copy != 0 -- one [B, n0, n1] copy of the scaled correlation.  The copy lives in `scores` /
 *          `final_scores` when one of them is requested: pass own_copy = 1 only for a call with scores == final_scores ==
 *          NULL (kp_scores alone). */
long long mk_dual_softmax_work_floats(int B, int n0, int n1, int own_copy);
int mk_dual_softmax(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float inv_temperature,
                    int use_dustbin, float dustbin, float* scores, float* kp_scores, float* final_scores, float* work, int B,
                    int C, int n0, int n1, mk_stream_t stream);

/* dualSoftmax.forward with the descriptor correlation on the 16-bit matrix cores (BASELINE.json configs[4]: "fp16 MFMA
 * descriptor correlation"; reference feature_matcher.py:65 is an fp32 matmul): every descriptor entry is split into fp16 hi + lo
 * parts (x 2^10 = hi + lo, 22 mantissa bits) and x0.x1 evaluated as lo.hi + hi.lo + hi.hi on v_mfma_f32_32x32x16_f16 with fp32
 * accumulation -- fp32-grade values (<= 1e-5 rel vs the fp32 reference, same row / column arg-max), a sixth of the matrix
 * time of the exact fp32 MFMA; the correlation is evaluated twice (statistics, then outputs) instead of being stored.
 * PRECONDITIONS (else use mk_dual_softmax): C == 128; |dsc| <= 1 everywhere (L2-normalised descriptors,
 * MICKEY.DSC_HEAD.NORM_DSC: True, extractor_utils.py:6-10); inv_temperature * log2(e) <= 100 (the row / column sums are
 * taken without a running maximum).  Arguments as mk_dual_softmax; work: mk_dual_softmax_split_work_floats fp32 elements. */
long long mk_dual_softmax_split_work_floats(int B, int n0, int n1);
int mk_dual_softmax_split(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float inv_temperature,
                          int use_dustbin, float dustbin, float* scores, float* kp_scores, float* final_scores, float* work,
                          int B, int C, int n0, int n1, mk_stream_t stream);

/* sinkhorn.forward (feature_matcher.py:93-137): 10 log-domain iterations on u, v only.
 *   scr0/scr1/kp_scores/final_scores as in mk_dual_softmax (optional).
 *   work: mk_sinkhorn_work_floats(B, n0, n1) fp32 elements (holds the (n0+1)x(n1+1) coupling matrix). */
long long mk_sinkhorn_work_floats(int B, int n0, int n1);
int mk_sinkhorn(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float alpha, int iters,
                float* scores, float* kp_scores, float* final_scores, float* work, int B, int C, int n0, int n1,
                mk_stream_t stream);

/* Keyframe mode of the three matchers: B pairs that share K <= B image-0 frames (Map-free val / test: every pair of a scene is
 * its keyframe seq0/frame_00000 against one query frame, reference lib/datasets/mapfree.py:83-99).  Arguments as the entry
 * point without _kf, except that dsc0 [K, C, n0] and scr0 [K, n0] hold the K keyframes and pair b reads row kf_index[b]:
 *   kf_index  int32 [B] device map pair -> keyframe, or NULL = the identity (then K must equal B: the call IS the one without _kf).
 *   PRECONDITION: 0 <= kf_index[b] < K for every b; the caller validates the map on the host (mickey_amd.ops.check_keyframe_index).
 *             A kernel never dereferences an entry outside [0, K): the workgroups of such a pair return without reading, and its
 *             outputs are left unwritten.
 * Work sizes: the same *_work_floats(B, n0, n1) as the call without _kf (K <= B: operand 0 only gets smaller).
 * mk_dual_softmax_split_kf makes the split planes of each keyframe ONCE (K, not B, plane sets). */
int mk_dual_softmax_kf(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float inv_temperature,
                       int use_dustbin, float dustbin, float* scores, float* kp_scores, float* final_scores, float* work, int B,
                       int C, int n0, int n1, const int* kf_index, int K, mk_stream_t stream);
int mk_dual_softmax_split_kf(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float inv_temperature,
                             int use_dustbin, float dustbin, float* scores, float* kp_scores, float* final_scores, float* work,
                             int B, int C, int n0, int n1, const int* kf_index, int K, mk_stream_t stream);
int mk_sinkhorn_kf(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float alpha, int iters,
                   float* scores, float* kp_scores, float* final_scores, float* work, int B, int C, int n0, int n1,
                   const int* kf_index, int K, mk_stream_t stream);

/* Pair-list mode of the three matchers: B pairs drawn from image sets that are encoded once -- a map on EACH operand (a sequence:
 * pairs (i, i+1) of N frames; Q queries against K keyframes; all pairs of a small collection).  No counterpart in the reference,
 * whose matcher takes one image-0 and one image-1 row per pair (compute_correspondences.py:52-92 builds both per pair,
 * feature_matcher.py:64-83 / :93-137 consume them; lib/datasets/mapfree.py:83-99 lists a frame once per pair it appears in): the
 * results are those of the entry point without a suffix on the materialised operands dsc0[idx0], dsc1[idx1], ..., bit for bit.
 * Arguments as that entry point, plus, in front of the stream:
 *   idx0, idx1  int32 [B] device maps: pair b reads row idx0[b] of operand 0 (dsc0 [N0, C, n0], scr0 [N0, n0]) and row idx1[b] of
 *               operand 1 (dsc1 [N1, C, n1], scr1 [N1, n1]).  NULL = the identity on that side; its row count must then equal B.
 *               Both NULL: the call IS the plain one.  idx1 == NULL: the call IS the _kf one (which is implemented on top of this).
 *   N0, N1      rows of operand 0 / 1; NOT limited by B (the K <= B of keyframe mode is a rule of that mode's callers only).
 *   dsc0 == dsc1 (with scr0 == scr1) is the usual case: one image set, both maps into it.
 *   PRECONDITION: 0 <= idx0[b] < N0 and 0 <= idx1[b] < N1; the caller validates on the host (mickey_amd.ops.check_pair_index).  A
 *               kernel never dereferences an entry outside its operand's rows: the workgroups of such a pair return before their
 *               first load and its outputs are left unwritten.
 * Everything that belongs to a pair (outputs, partials, log-sums) is indexed by the pair.
 * Work sizes: mk_dual_softmax_pairs: mk_dual_softmax_work_floats(B, n0, n1, own_copy); mk_sinkhorn_pairs:
 * mk_sinkhorn_work_floats(B, n0, n1) -- both hold per-pair data only.  mk_dual_softmax_split_pairs:
 * mk_dual_softmax_split_pairs_work_floats(B, n0, n1, N0, N1, shared) = the split planes of N0 + N1 images (shared != 0: of the N0
 * images of ONE set, which is what the call makes when dsc0 == dsc1, n0 == n1 and N0 == N1) + the per-pair part. */
int mk_dual_softmax_pairs(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float inv_temperature,
                          int use_dustbin, float dustbin, float* scores, float* kp_scores, float* final_scores, float* work, int B,
                          int C, int n0, int n1, const int* idx0, const int* idx1, int N0, int N1, mk_stream_t stream);
long long mk_dual_softmax_split_pairs_work_floats(int B, int n0, int n1, int N0, int N1, int shared);
int mk_dual_softmax_split_pairs(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float inv_temperature,
                                int use_dustbin, float dustbin, float* scores, float* kp_scores, float* final_scores, float* work,
                                int B, int C, int n0, int n1, const int* idx0, const int* idx1, int N0, int N1, mk_stream_t stream);
int mk_sinkhorn_pairs(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float alpha, int iters,
                      float* scores, float* kp_scores, float* final_scores, float* work, int B, int C, int n0, int n1,
                      const int* idx0, const int* idx1, int N0, int N1, mk_stream_t stream);

/* The two halves of mk_dual_softmax_split_pairs for a caller that walks a long pair list in chunks (same reference lines): the
 * split planes of an image set are made ONCE, then every chunk of pairs runs the two correlation passes on them.
 * mk_dsc_split_planes: dsc fp32 [N, C = 128, n] -> planes, mk_dsc_split_planes_floats(N, n) fp32 elements, 16-byte aligned (the
 *   plane layout is the same for both sides: one set serves as operand 0 and as operand 1).
 * mk_dual_softmax_split_planes: mk_dual_softmax_split_pairs with planes0 / planes1 (of N0 / N1 images, may be the same buffer) in
 *   place of dsc0 / dsc1 and C; work: mk_dual_softmax_split_planes_work_floats(B, n0, n1) fp32 elements (per-pair data only),
 *   16-byte aligned.  Same bits as mk_dual_softmax_split_pairs. */
long long mk_dsc_split_planes_floats(int N, int n);
int mk_dsc_split_planes(const float* dsc, float* planes, int N, int C, int n, mk_stream_t stream);
long long mk_dual_softmax_split_planes_work_floats(int B, int n0, int n1);
int mk_dual_softmax_split_planes(const float* planes0, const float* planes1, const float* scr0, const float* scr1,
                                 float inv_temperature, int use_dustbin, float dustbin, float* scores, float* kp_scores,
                                 float* final_scores, float* work, int B, int n0, int n1, const int* idx0, const int* idx1, int N0,
                                 int N1, mk_stream_t stream);

/* Training: the dual softmax with its backward (reference lib/models/MicKey/model.py:124-134 back-propagates d loss / d final_scores
 * through final_scores = dualSoftmax(dsc0, dsc1) * kp_matrix_scores: feature_matcher.py:64-83, compute_correspondences.py:46-50,
 * model.py:201).  C == 128; split != 0 selects the split-fp16 correlation (preconditions of mk_dual_softmax_split), else exact fp32.
 *
 * mk_dual_softmax_train: the forward.  scores / kp_scores / final_scores are those of mk_dual_softmax (split = 0) /
 *   mk_dual_softmax_split (split = 1) on the same inputs, bit for bit (at least one of scores, final_scores non-NULL).
 *   dustbin: DEVICE pointer to the fp32 dustbin scalar (feature_matcher.py:60: a trainable Parameter; no host synchronisation),
 *            NULL = no dustbin.
 *   lse [B, 2, max(n0, n1)] fp32, written: the merged log-sums of the augmented matrix in the LOG2 domain, lse[b][0][i] =
 *            log2 sum_j 2^(S_ij log2 e) over row i (dustbin column included), lse[b][1][j] the same over column j; S = dsc0^T dsc1 / T.
 *   work: mk_dual_softmax_train_work_floats(B, n0, n1, split) fp32 elements, 16-byte aligned. */
long long mk_dual_softmax_train_work_floats(int B, int n0, int n1, int split);
int mk_dual_softmax_train(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float inv_temperature,
                          const float* dustbin, float* scores, float* kp_scores, float* final_scores, float* lse, float* work, int B,
                          int C, int n0, int n1, int split, mk_stream_t stream);
/* mk_dual_softmax_bwd: the backward of final_scores (scr0 / scr1 given) or of scores (both NULL).
 *   Inputs as given to mk_dual_softmax_train (same split), its lse, and G [B, n0, n1] fp32 = d loss / d final_scores (or / d scores).
 *   Outputs, each may be NULL (not computed): g_dsc0 [B, C, n0], g_dsc1 [B, C, n1], g_scr0 [B, n0], g_scr1 [B, n1] (need scores),
 *   g_dustbin [B] (needs the dustbin): one value per pair, the caller sums them.  Outputs are overwritten, not accumulated.
 *   Deterministic and batch-invariant: no atomics, every reduction in a fixed order, pair b's values do not depend on B.
 *   work: mk_dual_softmax_bwd_work_floats(B, n0, n1, split) fp32 elements, 16-byte aligned. */
long long mk_dual_softmax_bwd_work_floats(int B, int n0, int n1, int split);
int mk_dual_softmax_bwd(const float* dsc0, const float* dsc1, const float* scr0, const float* scr1, float inv_temperature,
                        const float* dustbin, const float* lse, const float* G, float* g_dsc0, float* g_dsc1, float* g_scr0,
                        float* g_scr1, float* g_dustbin, float* work, int B, int C, int n0, int n1, int split, mk_stream_t stream);

/* featureMatcher.get_matches_list (feature_matcher.py:19-46), batched: mutual nearest neighbours on
 * scores[b, :n0-1, :n1-1], sorted by score descending.  matches int32 [B, n0, 2] (row i, col j),
 * count int32 [B].  work: 2*B*(n0+n1) ints. */
int mk_mutual_nn(const float* scores, int* matches, int* count, int* work, int B, int n0, int n1, mk_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Probabilistic Procrustes solver (reference .../utils/probabilisticProcrustes.py:183-348)
 * ---------------------------------------------------------------------------------------------- */

/* Weighted sampling without replacement == top-k of p / Exp(1) ("exponential race"); what
 * torch.multinomial(p, k) computes (probabilisticProcrustes.py:230-231).  For every pair b and every
 * r in [0, rows_per_pair): idx[b*rows_per_pair + r, 0..k) = indices of the k largest p[b, c] / e[b, r, c],
 * in descending key order (the order torch.topk returns).
 *   p      [B, ncell] fp32, >= 0
 *   noise  NULL: the race is drawn on device from Philox4x32-10(seed, offset) -- not cell by cell: with the threshold T of the
 *          keys known from the histogram of p, the candidates {p / e > T} of a row are generated directly as a thinned
 *          Bernoulli process (geometric skipping under a per-16-cell bound of p, acceptance s / S, e drawn from Exp(1)
 *          conditioned on e < p / T; mk_sampler.hip), the same law as drawing every e; else fp32 [B*rows_per_pair, ncell]
 *          injected Exp(1) draws (tests: bit-comparable with torch)
 *   idx    int32 [B*rows_per_pair, k];  cnt int32 [B*rows_per_pair] = number of non-zero-key entries
 *          actually available (< k only if fewer than k cells have p > 0; the tail is then filled
 *          with zero-probability cells in ascending index order)
 *   invalid int32 [1] or NULL: OR-ed with 1 when torch.multinomial would have raised (a NaN / inf /
 *          negative probability, or a row without any positive cell) -- the reference then returns
 *          the zero pose for the whole batch (probabilisticProcrustes.py:331-336)
 *   work   bytes: mk_exprace_topk_work_bytes(B, rows_per_pair, k, ncell), 16-byte aligned.  Its first
 *          mk_exprace_topk_state_bytes(B, rows_per_pair) bytes are SELF-CLEANING state (per-row candidate counts, per-pair
 *          flags and histograms, arrival counters): they must be ZERO when a call starts and every call leaves them zero, so
 *          the chain carries no zero-fill launch -- zero the buffer once when it is allocated and reuse it; a buffer must not
 *          be shared by calls that may run concurrently (two streams).  After a call that returns an error the state is
 *          undefined (the chain may have stopped between its launches): zero those bytes again before the buffer's next use.
 *          The chain is four launches: histogram of p (+ the threshold as its tail), the collect pass, the exact fallback
 *          (+ the shortfall check as its head; idle unless a pair came up short), the select kernel.
 *   pair_base  GLOBAL index of pair 0 of this call.  The Philox streams are keyed by (seed, offset, global pair index,
 *          draw, cell), so a batch may be split arbitrarily -- over calls or over the GPUs of a node -- without changing
 *          any pair's draws: pair i of a B = 32 call and the same pair alone with pair_base = i sample identically. */
long long mk_exprace_topk_work_bytes(int B, int rows_per_pair, int k, long long ncell);
long long mk_exprace_topk_state_bytes(int B, int rows_per_pair);
int mk_exprace_topk(const float* p, const float* noise, unsigned long long seed, unsigned long long offset,
                    const unsigned long long* offset_dev, int* idx, int* cnt, int* invalid, void* work, int B, int rows_per_pair,
                    long long ncell, int k, int pair_base, mk_stream_t stream);

/* *counter += inc on the stream.  `offset_dev` of mk_exprace_topk / mk_ransac_hypotheses (may be NULL) is such a
 * counter: the Philox stream offset used is offset + *offset_dev, read on the device when the kernel runs, so a
 * captured hipGraph of the forward draws fresh samples at every replay (the reference advances torch's generator). */
int mk_counter_add(unsigned long long* counter, unsigned long long inc, mk_stream_t stream);

/* Index decode + gathers + back-projection (probabilisticProcrustes.py:233-244, training_utils.py:7-22):
 * for every sampled cell c = idx[r, s]: i = c / n1 (image-0 keypoint), j = c % n1;
 *   X[r, s, :] = depth0[b, i] * K0[b]^-1 [kps0[b, :, i], 1],  Y likewise from image 1,
 *   wts[r, s] = final_scores[b, c],  corr[r, s, :] = (u0, v0, u1, v1, d0, d1)   (for the inlier list)
 * kps [B, 2, n], depth [B, n], K [B, 3, 3] fp32.  r = b*rows_per_pair + o. */
int mk_gather_backproject(const int* idx, const float* final_scores, const float* kps0, const float* depth0,
                          const float* kps1, const float* depth1, const float* K0, const float* K1, float* X, float* Y,
                          float* wts, float* corr, int B, int rows_per_pair, int k, int n0, int n1, mk_stream_t stream);

/* Keyframe mode of mk_gather_backproject (the pairs of a Map-free scene share its keyframe, reference
 * lib/datasets/mapfree.py:83-99): kps0 [K, 2, n0] and depth0 [K, n0] hold the K <= B keyframes, pair b reads row kf_index[b];
 * K0 stays per pair [B, 3, 3].  kf_index: int32 [B] device map, NULL = the identity (K == B).  PRECONDITION and
 * out-of-range behaviour as mk_dual_softmax_kf. */
int mk_gather_backproject_kf(const int* idx, const float* final_scores, const float* kps0, const float* depth0,
                             const float* kps1, const float* depth1, const float* K0, const float* K1, float* X, float* Y,
                             float* wts, float* corr, int B, int rows_per_pair, int k, int n0, int n1, const int* kf_index,
                             int K, mk_stream_t stream);

/* Pair-list mode of mk_gather_backproject (probabilisticProcrustes.py:233-244 gathers kps0[b] / kps1[b] of per-pair tensors; here
 * both come from image sets): kps0 [N0, 2, n0], depth0 [N0, n0] read through idx0 and kps1 [N1, 2, n1], depth1 [N1, n1] through
 * idx1; K0 / K1 [B, 3, 3], idx, final_scores and the outputs stay per pair.  idx0, idx1, N0, N1, PRECONDITION and out-of-range
 * behaviour as mk_dual_softmax_pairs. */
int mk_gather_backproject_pairs(const int* idx, const float* final_scores, const float* kps0, const float* depth0,
                                const float* kps1, const float* depth1, const float* K0, const float* K1, float* X, float* Y,
                                float* wts, float* corr, int B, int rows_per_pair, int k, int n0, int n1, const int* idx0,
                                const int* idx1, int N0, int N1, mk_stream_t stream);

/* Backward of mk_gather_backproject w.r.t. keypoints and depths (training: loss_class.py:139-146 + training_utils.py:7-22 under
 * autograd; intrinsics and scores get no gradient).  gX, gY [B*rows_per_pair, k, 3] = dL/dX, dL/dY; corr as written by the forward;
 * gkps [B, 2, n], gdepth [B, n] must be ZEROED by the caller: contributions are accumulated with fp32 atomic adds (a keypoint is
 * drawn by many cells; the order of the additions is not fixed, as in torch's index backward). */
int mk_gather_backproject_bwd(const int* idx, const float* corr, const float* gX, const float* gY, const float* K0, const float* K1,
                              float* gkps0, float* gdepth0, float* gkps1, float* gdepth1, int B, int rows_per_pair, int k, int n0,
                              int n1, mk_stream_t stream);

/* Hypothesis generation and scoring (probabilisticProcrustes.py:247-268; loss/solvers.py:31-52;
 * training_utils.py:55-61).  For every correspondence set r (k points) and every h in [0, it_ransac):
 * draw 3 of k without replacement weighted by wts (exponential race; noise3 = NULL: Philox, else fp32
 * [R*it_ransac, k] injected; idx3_in != NULL injects the 3 indices directly), fit R,t by Kabsch on the
 * 3 point pairs, score = sum_j sigmoid(5/th * (th - sqrt(|R X_j + t - Y_j|^2 + 1e-6))).
 *   Rh [R*it_ransac, 9], th [R*it_ransac, 3], score [R*it_ransac], idx3 int32 [R*it_ransac, 3] (out)
 *   set_base  GLOBAL index of correspondence set 0 of this call (= pair_base * rows_per_pair): keys the Philox streams of
 *          the 3-samples the same way as pair_base in mk_exprace_topk */
int mk_ransac_hypotheses(const float* X, const float* Y, const float* wts, const float* noise3, const int* idx3_in,
                         unsigned long long seed, unsigned long long offset, const unsigned long long* offset_dev,
                         float th_soft, float* Rh, float* th, float* score, int* idx3, int nsets, int it_ransac, int k,
                         long long set_base, mk_stream_t stream);

/* Arg-max over a pair's hypotheses, <= num_ref rounds of {hard-inlier recount, masked weighted Kabsch},
 * final confidence (probabilisticProcrustes.py:275-303, loss/solvers.py:13-26, training_utils.py:71-75).
 * One workgroup per pair.  hyp_per_pair = it_matches*it_ransac; the winning set is best / it_ransac.
 *   R [B, 9], t [B, 3], conf [B], best int32 [B], inl_mask uint8 [B, k] (hard inliers of the final pose),
 *   rounds int32 [B] (refits done), invalid int32 [1]: set to 1 if any hypothesis of the BATCH is
 *   non-finite (the reference then zeroes the whole batch, :261-262,329-342; applied by mk_pose_finalize). */
int mk_refine_pose(const float* X, const float* Y, const float* Rh, const float* th, const float* score, float th_inlier,
                   int num_ref, int min_inliers, float* R, float* t, float* conf, int* best, unsigned char* inl_mask,
                   int* rounds, int* invalid, int B, int it_matches, int it_ransac, int k, mk_stream_t stream);

/* If *invalid != 0: zero R, t, conf for the whole batch (reference :338-342). */
int mk_pose_finalize(float* R, float* t, float* conf, const int* invalid, int B, mk_stream_t stream);

/* ---- training-time RANSAC -----------------------------------------------------------------------
 * The no-grad core of MetricPoseLoss.single_iteration_RANSAC (reference lib/models/MicKey/modules/loss/loss_class.py:141-184):
 * for every sampled match set r in [0, nsets) (S matches: X, Y [nsets, S, 3], wts [nsets, S]) and every hypothesis
 * h in [0, it_ransac): draw num_corr matches without replacement ~ wts (:148; exponential race; noise = NULL: Philox
 * keyed by (seed, offset, set_base * it_ransac + r * it_ransac + h); noise != NULL: fp32 Exp(1) [nsets*it_ransac, S]
 * injected; idx_in != NULL: int32 [nsets*it_ransac, num_corr] indices injected), then <= num_ref refinement rounds
 * {masked weighted Procrustes over the current set (loss/solvers.py:13-26,45-52) -> matches within th_ref
 * (training_utils.py:71-75) -> accept iff their number grew} exactly as the reference's masked tensor updates do (:152-184).
 *   final_mask float32 [nsets*it_ransac, S]  `inliers_final`: 0/1, the set that produced the last accepted pose -- the
 *                                            weights of the differentiable Procrustes the caller runs next (:187)
 *   idx_out    int32 [nsets*it_ransac, num_corr]  the drawn matches, in draw order (descending race key)
 *   rounds     int32 [nsets*it_ransac]       accepted refinement rounds
 * S <= 1024, 3 <= num_corr <= S. */
int mk_train_ransac_masks(const float* X, const float* Y, const float* wts, const float* noise, const int* idx_in,
                          unsigned long long seed, unsigned long long offset, const unsigned long long* offset_dev,
                          float th_ref, int num_ref, int num_corr, float* final_mask, int* idx_out, int* rounds, int nsets,
                          int it_ransac, int S, long long set_base, mk_stream_t stream);

/* The DIFFERENTIABLE tail of the same function (loss_class.py:187-246), forward and backward: for every hypothesis
 * hyp = r * it_ransac + h of every match set r (pair b = r / it_matches)
 *   forward   weighted_procrustes(X_r, Y_r, mask_hyp) (loss/solvers.py:13-26,45-52: centroids with w / (sum|w| + 1e-16),
 *             H = A_c^T (w B_c), H = U S V^T, R = V diag(1, 1, det(U V^T)) U^T, t = b_mean - a_mean R^T), the soft inlier score
 *             sum_j sigmoid(5 / th (th - |R x_j + t - y_j|)) over all S matches (training_utils.py:55-61) and the loss:
 *             loss_type 0 = compute_vcre_loss (loss_utils.py:41-69 with metrics.py:56-80: the 7 x 4 x 7 eye grid projected with
 *             K0 / K1, clipped to [0, img_h], tanh(. / 80) with soft_clip), 1 = compute_pose_loss (:27-39);
 *               out   float32 [nhyp, 4]  (loss_value, rot_angle_loss, trans_l1_loss, score)
 *               Rt    float32 [nhyp, 12] (R row-major, t)
 *               saved float32 [nhyp, 32] (U, V, S, det sign, centroids, sum of weights: for the backward pass)
 *   backward  grad_out float32 [nhyp, 2] = dL/d(loss_value, score)  ->  gX, gY float32 [nsets, S, 3] = dL/dX, dL/dY, summed over
 *             the it_ransac hypotheses of a set in hypothesis order (no atomics); the SVD is differentiated in closed form
 *             (the adjoint of H -> R; finite for equal singular values, where torch.svd's backward is not);
 *             work float32 [nhyp, 16] scratch.  mask, the poses and the intrinsics receive no gradient (the reference detaches
 *             them: the mask comes out of torch.no_grad, :152-184).
 * X, Y [nsets, S, 3], mask [nsets * it_ransac, S], Rgt [B, 9], tgt [B, 3], K0, K1 [B, 9] (VCRE only), S <= 1024. */
int mk_train_tail_fwd(const float* X, const float* Y, const float* mask, const float* Rgt, const float* tgt, const float* K0,
                      const float* K1, int nsets, int it_ransac, int S, int it_matches, float th_soft, int loss_type,
                      int soft_clip, float img_h, float* out, float* Rt, float* saved, mk_stream_t stream);
int mk_train_tail_bwd(const float* X, const float* Y, const float* mask, const float* Rgt, const float* tgt, const float* K0,
                      const float* K1, int nsets, int it_ransac, int S, int it_matches, float th_soft, int loss_type,
                      int soft_clip, float img_h, const float* Rt, const float* saved, const float* grad_out, float* work,
                      float* gX, float* gY, mk_stream_t stream);

/* The reductions between the tail and the loss (loss_class.py:229-246, :263-268), forward and backward:
 *   forward   per set (row = b*it_matches + o) of it_ransac hypotheses, from out [nhyp, 4] of mk_train_tail_fwd:
 *               sm      = softmax over [score_k / temperature (, null_score / temperature if add_null)]
 *               loss_value[row] = sum_k sm_k loss_k (+ sm_null * null_loss)                                   (:240-246)
 *               rot / trans     = sum_k softmax(score / temperature)_k (rot_k | trans_k), WITHOUT the null column     (:229-238)
 *               coef [nhyp, 2]  = d loss_value[row] / d (loss_k, score_k) = (sm_k, sm_k (loss_k - loss_value[row]) / temperature)
 *             per pair: per_pair [B, 3] = sums over its it_matches rows of (loss_value, rot, trans), in row order        (:263-268)
 *             flags int32 [2] (caller zeroes): [0] |= 1 if any R / t of Rt [nhyp, 12] is not finite (:225-227), [1] += number of
 *             hypotheses whose cross-covariance has rank one (singular values saved[:, 18:21]; torch.linalg.matrix_rank, :190).
 *   backward  grad_out [nhyp, 2] = g_pair[b] * coef  (g_pair [B] = dL/d per_pair[:, 0]; what mk_train_tail_bwd takes)
 * it_matches <= 64. */
int mk_train_aggregate_fwd(const float* out, const float* Rt, const float* saved, int B, int it_matches, int it_ransac,
                           float temperature, int add_null, float null_loss, float null_score, float* loss_value, float* per_pair,
                           float* coef, int* flags, mk_stream_t stream);
int mk_train_aggregate_bwd(const float* coef, const float* g_pair, int B, int it_matches, int it_ransac, float* grad_out,
                           mk_stream_t stream);

/* REINFORCE bookkeeping of the same function (loss_class.py:251-261, a python loop over B*it_matches rows in the
 * reference): for row = b*it_matches + r, r ascending, and every sampled cell c = idx[row, s]:
 *   gradients[b, c] += loss_value[row];  gradients_b[b, c] += 1
 * fp32, rows applied in the reference's order (bit-identical sums).  Cells of one row must be distinct (they come from
 * sampling without replacement).  idx int32 [B*it_matches, S]; gradients, gradients_b float32 [B, ncell], zeroed by the
 * caller. */
int mk_reinforce_scatter(const int* idx, const float* loss_value, float* gradients, float* gradients_b, int B,
                         int it_matches, int S, long long ncell, mk_stream_t stream);

/* ---- validation on the device (mk_metrics.hip) ---------------------------------------------------------------------------
 * The per-pair metrics of a validation step (reference lib/utils/metrics.py:12-53 pose_error_torch and :83-125 vcre_torch, as
 * lib/models/MicKey/model.py:76-85 calls them): one launch, one wave per pair, fp64 arithmetic from the fp32 inputs, every
 * result rounded once to fp32.  For pair b of R [B, 9], t [B, 3], T_gt [B, 16] (the 4 x 4 T_0to1, row-major: Rgt, tgt),
 * K [B, 9] (Kori_color0), conf [B] (the solver's soft inlier count; NULL: 0) the record
 *   records[(row0 + b) * 8 ..] = (t_err_ang, t_err_scale, t_err_scale_sym, t_err_euc, R_err, vcre, conf, 0)
 *   t_err_ang        a = deg acos(clip(<t, tgt> / (|t| |tgt| + 1e-9), -1, 1)),  min(a, 180 - a)
 *   t_err_scale      |t| / |tgt|;   t_err_scale_sym  max(|t| / |tgt|, |tgt| / |t|);   t_err_euc  |t - tgt|
 *   R_err            deg acos(clip((trace(R^T Rgt) - 1) / 2, -1, 1))
 *   vcre             mean over the 196 eye-grid points e of sqrt(du^2 + dv^2 + 1e-6), (du, dv) = clip(proj(K, e)) -
 *                    clip(proj(K, Rgt^T (R e + t - tgt))), proj divides by z + 1e-16, u clipped to [0, W], v to [0, H]
 *                    (the residual is inv(cam2w_gt) cam2w_est, the direction of vcre_torch, in closed form)
 * A NaN input comes out as NaN (torch.clip / minimum / maximum semantics), in its pair's record only.  records float32
 * [capacity, 8], 16-byte aligned; rows outside [row0, row0 + B) are not written.  B >= 1, row0 >= 0, row0 + B <= capacity. */
int mk_pose_metrics(const float* R, const float* t, const float* T_gt, const float* K, const float* conf, float W, float H,
                    float* records, long long row0, int B, long long capacity, mk_stream_t stream);

/* The summary of a validation epoch (reference lib/models/MicKey/model.py:205-280 on_validation_epoch_end with
 * lib/benchmarks/utils.py:138-188 precision_recall, three times on the host there): two launches, no atomics, no sort, sums
 * in a fixed order (bit-identical from run to run).  records float32 [N, 8] as mk_pose_metrics writes them; three acceptance
 * tests (strict, as the trainer): t_err_euc < th_t and R_err < th_R | t_err_euc < th_t2 and R_err < th_R2 | vcre < th_px.
 * Average precision without a sort:  AP = 1 / (N + failures) * sum_i cumTP_i / cumN_i  with  cumN_i = #{j : c_j >= c_i},
 * cumTP_i = #{j : c_j >= c_i and tp_j} (integers; the quotient and the sums fp64): every group of tied confidences contributes
 * count * precision / (N + failures), which is precision_recall's sum of recall steps times precisions.  A confidence that is
 * not finite ranks as -inf and is counted in out[1]; a NaN metric makes its mean NaN and its acceptance false.
 *   out float32 [16] = (N, records with a non-finite confidence, mean t_err_ang, mean t_err_euc, mean R_err, mean vcre,
 *                       prec_pose, auc_pose, prec_pose_10, auc_pose_10, prec_vcre, auc_vcre,
 *                       mean loss, mean loss_R, mean loss_t, 0),   precisions = accepted / (N + failures)
 *   losses float32 [S, 3] (loss, loss_R, loss_t of the S validation steps) or NULL with S = 0 (the three means are then 0)
 *   work   double [mk_pose_summary_work_doubles(N)]: row k < ceil(N / tile) the partial sums of workgroup k, the last row the
 *          16 values of `out` before their rounding to fp32.
 * The ranking is quadratic: every record is compared with every record, in LDS tiles of mk_pose_summary_tile() records.
 * 1 <= N <= 2^18 (6.9e10 compares), failures >= 0. */
int mk_pose_summary_tile(void);
long long mk_pose_summary_work_doubles(int N);
int mk_pose_summary(const float* records, int N, int failures, float th_t, float th_R, float th_t2, float th_R2, float th_px,
                    const float* losses, int S, float* out, double* work, mk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MICKEY_HIP_H */
