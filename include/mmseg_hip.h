/*
 * mmseg_hip.h -- C ABI of libmmseg_hip.so, the gfx950 (MI355X / CDNA4) kernel library behind the
 * DAFNet / MMSDNet training step.
 *
 * The reference (agis85/multimodal_segmentation) has no FFI of its own: its arithmetic lives in Keras 2.1.6 /
 * TensorFlow 1.4 ops reached through the Python layer API.  Each entry point below replaces the TF op(s) that
 * the cited reference line instantiates; the Python host code in multimodal_segmentation_amd/ binds them with
 * ctypes (multimodal_segmentation_amd/_native.py) -- the binding a maintainer of the reference would add is
 * shown in INTEGRATION.md.
 *
 * Conventions
 *   - all tensors are dense fp32, NHWC, in device (HBM) memory; the caller owns every buffer (outputs and
 *     workspaces are allocated by the caller; *_workspace_floats() tell how much); no allocation, no
 *     synchronisation and no host<->device copy happens inside any entry point, so all of them may be
 *     captured into a hipGraph;
 *   - `stream` is a hipStream_t passed as void*; every launch goes to that stream;
 *   - the return value is a hipError_t as int (0 = hipSuccess); invalid geometry returns hipErrorInvalidValue
 *     without launching anything;
 *   - reductions are two-stage and run in a fixed order: results are bitwise reproducible run to run
  *     (the one scatter, mmseg_tps_warp_bwd's d_vol, accumulates in 64-bit fixed point with integer atomics, which is
 *     order-independent as well).
 */
#ifndef MMSEG_HIP_H
#define MMSEG_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* activation codes */
#define MMSEG_ACT_NONE 0
#define MMSEG_ACT_RELU 1
#define MMSEG_ACT_LEAKY 2
#define MMSEG_ACT_TANH 3

/* ---- convolution family (csrc/conv.hip): keras Conv2D [+UpSampling2D] [+Concatenate] -----------------------
 * reference: models/unet.py:94-101, utils/model_utils.py:15-22, model_components/segmentor.py:16-24,
 * modality_encoder.py:36-45, decoder.py:28,45-48, layers/spade.py:9-33, layers/stn_spline.py:106-114,
 * models/discriminator.py:24,39.
 * Implicit GEMM on v_mfma_f32_32x32x2_f32.  Logical input [B,H,W,C1+C2] = concat(x1 (optionally stored at
 * H/2 x W/2 and nearest-upsampled: ups=1), x2); kernel w [KH,KW,C1+C2,Cout] (keras HWIO); output [B,Ho,Wo,Cout].
 * transposed=1 selects the fractionally-strided gather used for the data gradient of a strided convolution
 * (tap valid iff (ho + kh - pad) % stride == 0).  y2/nsplit1: optional channel-split of the output
 * (channels [0,nsplit1) -> y, the rest -> y2), used for the data gradient of a two-input convolution. */
int mmseg_conv2d_fwd(const float* x1, const float* x2, const float* w, const float* wt, const float* bias, float* y, float* y2,
                     int B, int H, int W, int C1, int C2, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                     int pad_h, int pad_w, int ups, int transposed, int act, float alpha, int nsplit1, void* stream);
/* precision of the fast-path convolutions -- forward, data gradient, weight gradient (process-wide): 0 = fp32 MFMA (default),
 * 1 = operands rounded to bf16 (RNE) + v_mfma_f32_32x32x16_bf16, 2 = fp16 + v_mfma_f32_32x32x16_f16, both with fp32 accumulation; HBM tensors, weight gradients and everything else stay fp32
 * (BASELINE configs #3 / #5: reduced-precision compute with fp32 master weights and fp32 gradient all-reduce).
 * mmseg_set_conv_precision returns the previous mode. */
int mmseg_set_conv_precision(int mode);
/* Which kernel multiplies 16-bit tensors with channel counts that are multiples of 64 (the UNet / SPADE 3x3 layers of
 * models/unet.py:94-101, layers/spade.py:26-33 in the reduced-precision configurations): 0 = always the 128-wide register-staged
 * kernel, 1 (default) = the 256-pixel direct-to-LDS kernel where the launch has enough tiles, 2 = wherever it applies.  Same
 * 16-bit products and fp32 accumulation, K tiles of another depth: results agree to fp32 rounding.  Returns the previous mode; other
 * values only query. */
int mmseg_conv16_mode(int mode);
int mmseg_get_conv_precision(void);
/* y = act(conv(x) * oscale[c] + bias[c]): convolution + inference-mode BatchNormalization (+ReLU) in one launch (`predict` of the
 * conv blocks of models/unet.py:94-101 and model_components/segmentor.py:16-22); oscale / bias from mmseg_bn_infer_fold */
int mmseg_conv2d_fwd_scaled(const float* x1, const float* x2, const float* w, const float* wt, const float* bias, const float* oscale,
                            float* y, int B, int H, int W, int C1, int C2, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                            int pad_h, int pad_w, int ups, int act, float alpha, void* stream);
/* mmseg_conv2d_fwd / _fwd_scaled with 16-bit tensors in HBM (build-defined reduced-precision storage; mmseg_set_conv_precision(1 | 2)
 * selects bf16 | fp16): io bit 0 = x1, bit 1 = x2 hold 16-bit elements (MFMA fast path only), bit 2 = y / y2 are written 16-bit. */
int mmseg_conv2d_fwd_t(const void* x1, const void* x2, const float* w, const float* wt, const float* bias, void* y, void* y2,
                       int B, int H, int W, int C1, int C2, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                       int pad_h, int pad_w, int ups, int transposed, int act, float alpha, int nsplit1, int io, void* stream);
int mmseg_conv2d_fwd_scaled_t(const void* x1, const void* x2, const float* w, const float* wt, const float* bias, const float* oscale,
                              void* y, int B, int H, int W, int C1, int C2, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                              int pad_h, int pad_w, int ups, int act, float alpha, int io, void* stream);
/* which kernel template the last convolution entry point launched: family * 1000000 + 500000 * flag + (M | K tile) * 1000 + N tile (flag:
 * 16-byte gather of the generic kernels / two inputs of conv_wgrad_tr_kernel); families
 * 1 conv_fast_kernel, 2 conv_fwd_kernel, 3 conv_direct_kernel, 4 conv_fast_batched_kernel, 5 conv_dgrad_s2k4_smallc_kernel,
 * 6 conv_wgrad_tr_kernel, 7 conv_wgrad_fast_kernel, 8 conv_wgrad_kernel, 9 conv_wgrad_c8_kernel, 25 conv_fast_planes_kernel (the
 * products of mmseg_conv2d_fwd_wino), 26 winof_kernel (mmseg_conv2d_fwd_winof) (profiling aid, no launch) */
int mmseg_conv2d_last_kernel(void);
/* fast path (Cin % 32 == 0, not transposed, at most 32 taps -- the reference's largest kernel is 5 x 5; more taps fall back to the
 * generic kernel, which reads `w`): K tiles lie inside one tap, gather by buffer loads, weights read from
 * `wt` = the kernel re-laid out as [Cout][K] by mmseg_conv2d_wprep (mode 0 forward, mode 1 data gradient incl. the
 * spatial flip, mode 2 the kernel as it is, in the image's element type); pass wt = NULL to force the generic kernel.  In the reduced-precision modes (mmseg_set_conv_precision 1 | 2) the
 * image holds elements of the 16-bit MFMA operand type (rounded once by the prep launch; it occupies the first half of the same
 * fp32-sized buffer) -- prepare it in the mode the convolution runs in. */
int mmseg_conv2d_fast_path(int C1, int C2, int Cout, int transposed);
int mmseg_conv2d_wprep(const float* w, float* out, int KH, int KW, int Cin, int Cout, int mode, void* stream);
/* the mode 0 / 1 images of n weights in ONE launch (all images of a model after its optimiser step); table: device int64 [n + 1][8] rows
 * {src, dst, KH*KW, Cin, Cout, mode, first block, 0}, row n carries the total block count; blocks per row = taps * ceil(Cin/32) * ceil(Cout/32) */
int mmseg_conv2d_wprep_batch(const long long* table, int n, long total_blocks, void* stream);
/* data gradient of a STRIDED convolution, one launch per parity class (ph, pw) of the input pixels: only the taps
 * kh = ph + s*a, kw = pw + s*b contribute, so each class is a stride-1 convolution over dy with a small sub-kernel and a
 * strided store -- no multiplications by the zeros of a dilated gradient.  wt from mmseg_conv2d_wprep_parity. */
int mmseg_conv2d_parity_taps(int K, int stride, int p);
int mmseg_conv2d_wprep_parity(const float* w, float* out, int KH, int KW, int Cin, int Cout, int stride, int ph, int pw, void* stream);
/* all stride x stride classes in one launch: out = the class images back to back in (ph, pw) raster order (what mmseg_conv2d_dgrad_parity_all reads) */
int mmseg_conv2d_wprep_parity_all(const float* w, float* out, int KH, int KW, int Cin, int Cout, int stride, void* stream);
int mmseg_conv2d_dgrad_parity(const float* dy, const float* wt, float* dx, int B, int Ho, int Wo, int Cout, int H, int W, int Cin,
                              int TH, int TW, int stride, int ph, int pw, void* stream);
/* data gradient of the discriminators' first layer (models/discriminator.py:24: 4x4, stride 2, valid; Cin = 1 or 4, Cout = 64):
 * direct kernel, w in the Keras layout */
int mmseg_conv2d_dgrad_s2k4_smallc(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Ho, int Wo, int Cout,
                                   void* stream);
/* all stride x stride parity classes of the data gradient in one batched launch; wt_all = the classes' sub-kernels from
 * mmseg_conv2d_wprep_parity back to back in (ph, pw) raster order */
int mmseg_conv2d_dgrad_parity_all(const float* dy, const float* wt_all, float* dx, int B, int Ho, int Wo, int Cout, int H, int W,
                                  int Cin, int KH, int KW, int stride, void* stream);
/* ---- UpSampling2D(2) -> Conv2D(3, 'same') of the UNet up path (models/unet.py:67-82) with the up-sampling folded into the weights:
 * output pixels of parity class (py, px) see 2 x 2 distinct pixels of x, so 4 of the 9 multiplications remain.
 * Process-wide switch, modelled on mmseg_conv16_mode: 0 = never, 1 (default) = the inference forward only, where the channel conditions
 * hold and the class grid fills the chip, 2 = every direction wherever the channel conditions hold.  (The folded sums round differently
 * from the nine-tap ones; the default keeps the training directions' results bit for bit, while the inference passes end in the anatomy
 * encoder's Rounding layer.)  Returns the previous mode; other values only query. */
int mmseg_conv2d_ups_fold_mode(int mode);
/* 1 when the layer x [B,H1,W1,C1] -> y [B,2H1,2W1,Cout] (models/unet.py:67-82) takes the folded route in direction dir (0 training
 * forward, 1 data gradient, 2 weight gradient, 3 folded-BN inference forward): fp32 precision mode, C1 % 32 == 0, Cout % 32 == 0,
 * Cout > 32, every tensor below 2^31 bytes; in mode 1 also dir == 3 and 4 * ceil(B*H1*W1 / 128) * ceil(Cout / 64) >= 384.  No launch. */
int mmseg_conv2d_ups_fold_ok(int B, int H1, int W1, int C1, int Cout, int dir);
/* weight images of such a layer (models/unet.py:67-82), w [3,3,C1,Cout], each element a sum of 1, 2 or 4 weights in a fixed order:
 * which 0 = the four forward class images back to back in (py, px) raster order, each [Cout][2*2][C1] in the fast layout, tap (a, b) of
 *           class (py, px) summing kernel rows R[py][a] and columns R[px][b], R[0] = [{0},{1,2}], R[1] = [{0,1},{2}];
 * which 1 = the data-gradient image [C1][4*4][Cout], tap (u, v) summing rows U[u] and columns U[v], U = [{2},{1,2},{0,1},{0}]. */
int mmseg_conv2d_wprep_ups(const float* w, float* out, int C1, int Cout, int which, void* stream);
/* forward of such a layer (models/unet.py:67-82) as ONE batched launch of its four parity classes: class (py, px) is the 2 x 2 stride-1
 * convolution of x with pad (1-py, 1-px) stored at y[:, 2i+py, 2j+px]; y = act(conv * oscale[c] + bias[c]) (oscale / bias may be NULL).
 * wt_classes from mmseg_conv2d_wprep_ups(which 0).  fp32 mode only; C1 % 32 == 0, Cout % 4 == 0, 16-byte aligned x / wt_classes,
 * tensors below 2^31 bytes -- otherwise refused.  The data gradient is mmseg_conv2d_fwd over dy with KH = KW = 4, stride 2, pad 1 and
 * wt = mmseg_conv2d_wprep_ups(which 1); the weight gradient is mmseg_conv2d_wgrad of that convolution (x1 := dy, dy := x) followed by
 * mmseg_conv2d_ups_wgrad_fold. */
int mmseg_conv2d_fwd_ups_parity(const float* x, const float* wt_classes, const float* bias, const float* oscale, float* y, int B, int H1,
                                int W1, int C1, int Cout, int act, float alpha, void* stream);
/* weight gradient of such a layer (models/unet.py:67-82), second half: dW [3,3,C1,Cout] += sum_{u in KU[kh], v in KU[kw]} dWe[u][v][co][ci]
 * with KU = [{2,3},{1,2},{0,1}] and dWe [4,4,Cout,C1] the weight gradient of the 4x4 stride-2 pad-1 convolution that maps dy to dx. */
int mmseg_conv2d_ups_wgrad_fold(const float* dWe, float* dW, int C1, int Cout, void* stream);
/* ---- Winograd F(2x2, 3x3) for the inference forward of the deep 3x3 'same' layers (`predict` of the conv blocks of models/unet.py:94-101):
 * weight image, input transform, sixteen products in one launch of the fast-path body, output transform with the folded BatchNorm.
 * Process-wide switch like mmseg_conv2d_ups_fold_mode: 0 = never, 1 (default) = the shapes measured faster than the direct launch,
 * 2 = wherever the structural conditions hold.  Returns the previous mode; other values only query. */
int mmseg_conv2d_wino_mode(int mode);
/* 1 when the inference forward of a 3x3, stride 1, 'same' layer without up-sampling x1 [B,H,W,C1] (+ x2 [B,H,W,C2]) -> y [B,H,W,Cout]
 * takes the route: fp32 precision mode, H and W even, C1 / C2 / Cout multiples of 32 (C1, Cout >= 32), every tensor and every plane of
 * the workspace below 2^31 - 64 bytes; in mode 1 also H, W <= 64, B * H/2 * W/2 >= 512, C1 + C2 >= 256 and Cout >= 256
 * (the region measured faster, profiles/wino_ab.txt).  No launch. */
int mmseg_conv2d_wino_ok(int B, int H, int W, int C1, int C2, int Cout);
/* floats of workspace of mmseg_conv2d_fwd_wino: 16 * B * H/2 * W/2 * (C1 + C2 + Cout) */
long mmseg_conv2d_wino_workspace(int B, int H, int W, int C1, int C2, int Cout);
/* weight image out [16][Cout][Cin] = G w G^T per (ci, co) of w [3,3,Cin,Cout], plane p = i * 4 + j, G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]];
 * fixed summation order.  fp32 mode only. */
int mmseg_conv2d_wprep_wino(const float* w, float* out, int Cin, int Cout, void* stream);
/* y = act(conv3x3_same(concat(x1, x2)) * oscale[c] + bias[c]) (oscale / bias may be NULL; scale before bias, the expression of
 * mmseg_conv2d_fwd_scaled) in four launches; U from mmseg_conv2d_wprep_wino; ws = caller's scratch of at least
 * mmseg_conv2d_wino_workspace floats (checked, with the structural conditions and 16-byte alignment, before anything is queued). */
int mmseg_conv2d_fwd_wino(const float* x1, const float* x2, const float* U, const float* bias, const float* oscale, float* y, int B, int H,
                          int W, int C1, int C2, int Cout, int act, float alpha, float* ws, long ws_floats, void* stream);
/* Fused Winograd F(2x2,3x3) of the same operation in ONE launch (family 26 winof_kernel, no workspace): a block builds the transformed
 * input of 8 image rows x 32 columns in LDS, keeps the sixteen plane accumulators of 64 tiles x 64 output channels in registers and applies
 * the output transform, scale, bias and activation in its epilogue.  Asked only by callers that opt in (ops.conv2d_bn_infer(rounded=True):
 * the output is seen through a Rounding layer only), before mmseg_conv2d_wino_ok.  1 when the route is taken: mmseg_conv2d_wino_mode 1 or 2,
 * fp32 precision mode, H % 8 == 0, W % 32 == 0, C1 % 32 == C2 % 32 == 0 (C1 >= 32), Cout % 64 == 0, every tensor and the weight image below
 * 2^31 - 64 bytes; in mode 1 also one of the shapes measured faster than the other routes (profiles/winof_ab.txt).  No launch. */
int mmseg_conv2d_winof_ok(int B, int H, int W, int C1, int C2, int Cout);
/* y = act(conv3x3_same(concat(x1, x2)) * oscale[c] + bias[c]) (oscale / bias may be NULL); U from mmseg_conv2d_wprep_wino.  The structural
 * conditions above and 16-byte alignment of every pointer are checked before the launch is queued (hipErrorInvalidValue otherwise). */
int mmseg_conv2d_fwd_winof(const float* x1, const float* x2, const float* U, const float* bias, const float* oscale, float* y, int B, int H,
                           int W, int C1, int C2, int Cout, int act, float alpha, void* stream);
/* Data gradient of a stride-1 convolution with few input channels (segmentor c0 8 -> 64, the SPADE shared convolutions 8 -> 128:
 * model_components/segmentor.py:16, layers/spade.py:29), second half: dx = sum over the taps of the shifted planes of
 * T [B,Ho,Wo,KH*KW*Cin], which the caller computes with ONE 1x1 mmseg_conv2d_fwd over dy (wt = the Keras kernel itself read as
 * [KH*KW*Cin][Cout]). */
int mmseg_conv2d_dgrad_tapsum(const float* T, float* dx, int B, int H, int W, int Ho, int Wo, int Cin, int KH, int KW, int ph, int pw,
                              void* stream);
long mmseg_conv2d_wgrad_workspace(int B, int Ho, int Wo, int Cin, int Cout, int KH, int KW);
/* mmseg_conv2d_wgrad with 16-bit operands in HBM (reduced-precision modes; stride 1 and Wo % 4 == 0 only): io bit 0 = x1 (and x2),
 * bit 2 = dy hold 16-bit elements; dw and the workspace stay fp32 */
int mmseg_conv2d_wgrad_t_supported(int Ho, int Wo, int stride, int C1, int C2, int Cout);
int mmseg_conv2d_wgrad_t(const void* x1, const void* x2, const void* dy, float* dw, float* ws, long ws_floats,
                         int B, int H, int W, int C1, int C2, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                         int pad_h, int pad_w, int ups, int accumulate, int io, void* stream);
/* dW[KH,KW,Cin,Cout] (+)= sum over output pixels of im2col(x)^T * dy (accumulate != 0 adds to dW: gradient arenas);
 * ws: mmseg_conv2d_wgrad_workspace floats */
int mmseg_conv2d_wgrad(const float* x1, const float* x2, const float* dy, float* dw, float* ws, long ws_floats,
                       int B, int H, int W, int C1, int C2, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                       int pad_h, int pad_w, int ups, int accumulate, void* stream);
/* wt[kh][kw][co][ci] = w[KH-1-kh][KW-1-kw][ci][co]: the kernel of the data-gradient convolution */
int mmseg_conv2d_wflip(const float* w, float* wt, int KH, int KW, int Cin, int Cout, void* stream);

/* ---- element-wise and small reductions (csrc/pointwise.hip) --------------------------------------------- */
int mmseg_act_fwd(const float* x, float* y, long n, int act, float alpha, void* stream);
/* dx = dy * act'(.) evaluated from the activation OUTPUT y */
int mmseg_act_bwd(const float* dy, const float* y, float* dx, long n, int act, float alpha, void* stream);
int mmseg_axpby(const float* a, const float* b, float* out, long n, float sa, float sb, void* stream);
int mmseg_fill(float* x, long n, float v, void* stream);
int mmseg_colsum_blocks(long M);
long mmseg_colsum_workspace_floats(long M, int C);
/* out[c] (+)= scale * sum_m x[m][c]; ws: mmseg_colsum_workspace_floats(M, C) floats.  (bias gradients) */
int mmseg_colsum(const float* x, float* out, float* ws, long M, int C, float scale, int accumulate, void* stream);
/* keras MaxPooling2D(2) (models/unet.py:39-51, layers/stn_spline.py:108,111) */
int mmseg_maxpool2_fwd(const float* x, float* y, int B, int H, int W, int C, void* stream);
int mmseg_maxpool2_bwd(const float* x, const float* y, const float* dy, float* dx, int B, int H, int W, int C, void* stream);
/* gradient of keras UpSampling2D(2): dx[B,H,W,C] = 2x2 block sums of dy[B,2H,2W,C] */
int mmseg_upsample2_bwd(const float* dy, float* dx, int B, int H, int W, int C, void* stream);
/* keras UpSampling2D(2) standalone (decoder.py:70-80): y[B,2H,2W,C] */
int mmseg_upsample2_fwd(const float* x, float* y, int B, int H, int W, int C, void* stream);
/* tf.image.resize_nearest_neighbor for an integer down-sampling factor f (layers/spade.py:36-38): y[B,Ho,Wo,C] */
int mmseg_subsample_fwd(const float* x, float* y, int B, int Ho, int Wo, int C, int f, void* stream);
int mmseg_subsample_bwd(const float* dy, float* dx, int B, int Ho, int Wo, int C, int f, void* stream);
/* channel softmax; s (optional) = round-half-even(p): conv_anatomy softmax + layers/rounding.py:23-42 */
int mmseg_softmax_fwd(const float* x, float* p, float* s, long npix, int C, void* stream);
int mmseg_softmax_bwd(const float* dy, const float* p, float* dx, long npix, int C, void* stream);
/* layers/film.py:26-36 fused with the LeakyReLU and residual Add of decoder.py:50-53: y = leaky(x*g+b) [+ res] */
int mmseg_film_fwd(const float* x, const float* gamma, const float* beta, const float* res, float* y, int B, long HW, int C,
                   float alpha, void* stream);
int mmseg_film_bwd_workspace(int B, int C);
int mmseg_film_bwd(const float* du, const float* x, const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta,
                   float* ws, int B, long HW, int C, float alpha, void* stream);
/* keras Maximum (model_components/anatomy_fuser.py:33); gradient ties go to the first argument (tf.maximum) */
int mmseg_maximum_fwd(const float* a, const float* b, float* y, long n, void* stream);
int mmseg_maximum_bwd(const float* a, const float* b, const float* dy, float* da, float* db, long n, void* stream);
/* Lambda x[..., c0:c0+Cs] (models/dafnet.py:187) */
int mmseg_slice_fwd(const float* x, float* y, long M, int C, int c0, int Cs, void* stream);
int mmseg_slice_bwd(const float* dy, float* dx, long M, int C, int c0, int Cs, void* stream);
/* utils/sdnet_utils.py:9-21 (eps explicit) + costs.py:186-189 */
int mmseg_sampling_kl_fwd(const float* mu, const float* lv, const float* eps, float* z, float* kl, int B, int Z, void* stream);
int mmseg_sampling_kl_bwd(const float* mu, const float* lv, const float* eps, const float* dz, const float* dkl, float* dmu,
                          float* dlv, int B, int Z, void* stream);

/* ---- normalisation (csrc/norm.hip) ------------------------------------------------------------------- */
int mmseg_norm_workspace_floats(int C);
/* keras BatchNormalization, training: batch statistics; updates moving stats in place when non-null */
int mmseg_bn_stats(const float* x, const float* gamma, const float* beta, float* mean, float* invstd, float* scale, float* shift,
                   float* mov_mean, float* mov_var, float* ws, long M, int C, float eps, float momentum, void* stream);
int mmseg_bn_infer_prep(const float* gamma, const float* beta, const float* mov_mean, const float* mov_var, float* scale, float* shift,
                        int C, float eps, void* stream);
/* the same folded behind a convolution with bias conv_bias (may be NULL): scale = gamma / sqrt(var + eps),
 * shift = beta - mean * scale + conv_bias * scale  ->  bn(conv + conv_bias) = conv * scale + shift */
int mmseg_bn_infer_fold(const float* gamma, const float* beta, const float* mov_mean, const float* mov_var, const float* conv_bias,
                        float* scale, float* shift, int C, float eps, void* stream);
int mmseg_bn_apply(const float* x, const float* scale, const float* shift, float* y, long M, int C, int relu, void* stream);
int mmseg_bn_bwd(const float* dy, const float* y, const float* x, const float* gamma, const float* mean, const float* invstd,
                 float* dx, float* dgamma, float* dbeta, float* coef, float* ws, long M, int C, int relu, int accumulate, void* stream);
/* the same without the saved output y: the ReLU mask is recomputed from x with the forward pass's scale / shift (mmseg_bn_stats),
 * bit-identical to the mask of mmseg_bn_apply's output -- 5 tensor passes over HBM instead of 7 */
int mmseg_bn_bwd_x(const float* dy, const float* x, const float* scale, const float* shift, const float* gamma, const float* mean,
                   const float* invstd, float* dx, float* dgamma, float* dbeta, float* coef, float* ws, long M, int C, int relu,
                   int accumulate, void* stream);
/* Synchronised BatchNorm over data-parallel ranks (build-defined option conf.sync_bn; the reference is single device, SURVEY 8e iii):
 * the two halves of mmseg_bn_stats / mmseg_bn_bwd, the caller exchanging [2][C] floats in between (all-gather of (mean, biased
 * variance) in rank order; all-reduce(sum) of (sum g, sum g*xhat)).  stat2 / sums: [2][C]; gathered: [R][2][C]; coef: [3][C]. */
int mmseg_bn_stats_local(const float* x, float* stat2, float* ws, long M, int C, void* stream);
int mmseg_bn_stats_combine(const float* gathered, int R, const float* gamma, const float* beta, float* mean, float* invstd, float* scale,
                           float* shift, float* mov_mean, float* mov_var, long M_total, int C, float eps, float momentum, void* stream);
int mmseg_bn_bwd_sums(const float* dy, const float* y, const float* x, const float* mean, const float* invstd, float* sums, float* ws,
                      long M, int C, int relu, void* stream);
int mmseg_bn_bwd_finish(const float* sums_local, const float* sums_global, const float* gamma, const float* mean, const float* invstd,
                        float* dgamma, float* dbeta, float* coef, int C, long M_total, int accumulate, void* stream);
int mmseg_bn_bwd_apply(const float* dy, const float* y, const float* x, const float* coef, float* dx, long M, int C, int relu, void* stream);
/* ---- reduced-precision STORAGE of the convolutional trunk (csrc/act16.hip; build-defined, BASELINE configs #3 / #5): BatchNorm, 2x2
 *      max pooling and the gradient of nearest x2 up-sampling on tensors stored as fp32 or a 16-bit type, per tensor: element code
 *      h = 0 fp32, 1 bf16, 2 fp16.  Arithmetic, statistics and reductions are fp32 as in the fp32 entry points.  C % 64 == 0 for
 *      the statistics / backward passes.  mmseg_bn_bwd_t: dy, y carry hy; x, dx carry hx; dgamma / dbeta may be NULL. ---- */
int mmseg_bn_stats_t(const void* x, const float* gamma, const float* beta, float* mean, float* invstd, float* scale, float* shift,
                     float* mov_mean, float* mov_var, float* ws, long M, int C, float eps, float momentum, int hx, void* stream);
int mmseg_bn_apply_t(const void* x, const float* scale, const float* shift, void* y, long M, int C, int relu, int hx, int hy, void* stream);
int mmseg_bn_bwd_t(const void* dy, const void* y, const void* x, const float* gamma, const float* mean, const float* invstd, void* dx,
                   float* dgamma, float* dbeta, float* coef, float* ws, long M, int C, int relu, int accumulate, int hx, int hy, void* stream);
int mmseg_maxpool2_fwd_t(const void* x, void* y, int B, int H, int W, int C, int h, void* stream);
int mmseg_maxpool2_bwd_t(const void* x, const void* y, const void* dy, void* dx, int B, int H, int W, int C, int h, void* stream);
int mmseg_upsample2_bwd_t(const void* dy, void* dx, int B, int H, int W, int C, int h, void* stream);
/* dx = gradient of MaxPooling2D(2) + add (add may be NULL): the down-path activation of models/unet.py:39-51 feeds the pooling AND the
 * skip Concatenate (models/unet.py:69-84); both gradients in one pass instead of the autograd engine's separate addition */
int mmseg_maxpool2_bwd_add_t(const void* x, const void* y, const void* dy, const void* add, void* dx, int B, int H, int W, int C, int h,
                             void* stream);
/* out = p0 + ... + p(n-1), 1 <= n <= 8, tensors of `numel` elements with element code h: the sum of the gradients of a tensor with
 * several consumers (keras / TF add them inside the backward graph, e.g. the anatomy s feeding 7 layers in models/dafnet.py:163-222) */
int mmseg_sum_n_t(const void* p0, const void* p1, const void* p2, const void* p3, const void* p4, const void* p5, const void* p6,
                  const void* p7, int n, void* out, long numel, int h, void* stream);
/* out = concatenation of n <= 8 equally sized contiguous parts of `words` 4-byte words along the leading axis; NULL part = zeros
 * (batched calls of per-sample components: the 6 decodings / 4 D_Mask passes of models/dafnet.py:187-215, the pools of
 * model_executors/dafnet_executor.py:524-570) */
int mmseg_cat_words(const void* p0, const void* p1, const void* p2, const void* p3, const void* p4, const void* p5, const void* p6,
                    const void* p7, int n, void* out, long words, void* stream);
/* out[r] = src[idx[r]], rows of `words` 4-byte words (utils/data_utils.py sample(): np.random.choice rows of a fake pool) */
int mmseg_gather_rows(const void* src, const long long* idx, void* out, int rows, long words, int src_rows, void* stream);
/* base_executor.py:83-87 add_residual on the device: out[M][C+1] = masks + background channel */
int mmseg_add_residual(const float* msk, float* out, long M, int C, void* stream);
/* dx = dy * act'(y) of a convolution's fused activation (y = its output), tensors stored with element code h (0 fp32, 1 bf16, 2 fp16);
 * with bias_grad != NULL also the bias gradient bias_grad[c] (+)= sum_m dx[m][c] in the same pass (C % 64 == 0, ws =
 * mmseg_colsum_workspace_floats(M, C) floats) -- one pass instead of mmseg_act_bwd + mmseg_colsum */
int mmseg_act_bwd_bias_t(const void* dy, const void* y, void* dx, float* bias_grad, float* ws, long M, int C, int act, float alpha,
                         int accumulate, int h, void* stream);
/* out[B*H*W][96] (16-bit, code hy) = im2col of x[B,H,W,8] (code hx) for a 3x3 stride-1 'same' convolution: K index = tap * 8 + channel,
 * columns 72..95 zero.  A 1x1 fast-path convolution over it (Cin = 96, weights = the Keras kernel read as [72][Cout] + 24 zero rows)
 * is the reduced-precision form of the SPADE units' 8 -> 128 convolution (layers/spade.py:28) */
int mmseg_im2col8_t(const void* x, void* out, int B, int H, int W, int hx, int hy, void* stream);
/* Conv2D(Cout, 3, padding='same') of an 8-channel tensor in the 16-bit modes in ONE launch: the shared convolution of a SPADE unit (layers/spade.py:27:
 * anatomy -> 128 hidden channels + ReLU) and the segmentor's first layer (model_components/segmentor.py:16).  x fp32 (hx 0) or the mode's 16-bit type, w the
 * Keras kernel [3,3,8,Cout], y fp32 (hy 0) or 16-bit; W % 32 == 0, Cout % 4 == 0 (% 8 for a 16-bit y); act 0 none, 1 ReLU, 2 LeakyReLU(alpha).  Replaces mmseg_im2col8_t + a 1x1 mmseg_conv2d_fwd_t. */
int mmseg_conv8h_fwd_t(const void* x, const float* w, const float* bias, void* y, int B, int H, int W, int Cout, int act, float alpha,
                       int hx, int hy, void* stream);
/* keras_contrib InstanceNormalization(axis=None) fused with SPADE_COND and LeakyReLU (layers/spade.py:7-33,51-54) */
int mmseg_in_workspace_floats(int B);
int mmseg_instnorm_spade_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stat, float* ws, int B,
                             long per_sample, float eps, float act_alpha, void* stream);
int mmseg_instnorm_spade_bwd(const float* dy, const float* x, const float* stat, const float* gamma, const float* beta, float* dx,
                             float* dgamma, float* dbeta, float* dxn, float* ws, int B, long per_sample, float eps, float act_alpha,
                             void* stream);
/* The same with gamma and beta as the two halves of ONE tensor gb [B*H*W][2C] (gamma = channels [0, C), beta = [C, 2C)) -- the
 * output of a SPADE unit's gamma and beta convolutions run as one convolution (layers/spade.py:30-33 of the reference computes
 * Conv2D(f)(a) twice on the same 128-channel tensor); dgb has the layout of gb.  per_sample = H*W*C, C % 4 == 0. */
int mmseg_instnorm_spade_fwd_gb(const float* x, const float* gb, float* y, float* stat, float* ws, int B, long per_sample, int C, float eps,
                                float act_alpha, void* stream);
int mmseg_instnorm_spade_bwd_gb(const float* dy, const float* x, const float* stat, const float* gb, float* dx, float* dgb, float* dxn,
                                float* ws, int B, long per_sample, int C, float eps, float act_alpha, void* stream);
/* the same with gb / dgb stored with element code h and the output y / its gradient dy with element code hy (0 fp32, 1 bf16, 2 fp16):
 * with 16-bit activation storage the fused gamma / beta tensor, the modulated output that feeds the next convolution and their
 * gradients live in HBM in the 16-bit type (x and dx stay fp32) */
int mmseg_instnorm_spade_fwd_gb_t(const float* x, const void* gb, void* y, float* stat, float* ws, int B, long per_sample, int C, float eps,
                                  float act_alpha, int h, int hy, void* stream);
int mmseg_instnorm_spade_bwd_gb_t(const void* dy, const float* x, const float* stat, const void* gb, float* dx, void* dgb, float* dxn,
                                  float* ws, int B, long per_sample, int C, float eps, float act_alpha, int h, int hy, void* stream);
/* out[c] (+)= column sums of a tensor stored with element code h (C % 64 == 0; ws: mmseg_colsum_workspace_floats(M, C) floats) */
int mmseg_colsum_t(const void* x, float* out, float* ws, long M, int C, int accumulate, int h, void* stream);
/* out[m] = (a[m] | b[m]) for M rows of Ca and Cb floats; da[m] += src[m][0:Ca], db[m] += src[m][Ca:]: the fused operand of two
 * convolutions that share their input, and its gradient back into the two parameters */
int mmseg_concat_cols(const float* a, const float* b, float* out, long M, int Ca, int Cb, void* stream);
int mmseg_split_cols_acc(const float* src, float* da, float* db, long M, int Ca, int Cb, void* stream);


/* ---- keras Dense for rows <= 32 (csrc/dense.hip) ----------------------------------------------------- */
long mmseg_dense_workspace_floats(int R, int K, int N);
int mmseg_dense_fwd(const float* x, const float* w, const float* bias, float* y, float* ws, int R, int K, int N, int act,
                    float alpha, void* stream);
int mmseg_dense_dgrad(const float* dy, const float* w, float* dx, int R, int K, int N, void* stream);
int mmseg_dense_wgrad(const float* x, const float* dy, float* dw, int R, int K, int N, int accumulate, void* stream);

/* ---- thin-plate-spline warp (csrc/tps.hip): layers/stn_spline.py:36-67 + interpolate_spline.py + resampler --- */
int mmseg_tps_workspace_floats(int B);
int mmseg_tps_warp_fwd(const float* vol, const float* theta, const float* Mb, float* out, float* loc, int B, int H, int W, int C,
                       void* stream);
long mmseg_tps_scatter_workspace_floats(int B, int H, int W, int C);
/* acc: mmseg_tps_scatter_workspace_floats floats (8-byte aligned) -- 64-bit fixed-point accumulators of the d_vol scatter, which
 * make it independent of the order of the atomics (bitwise reproducible).  Each of the four contributions of an output pixel to
 * d_vol is rounded to a multiple of 2^-36 (error <= 2^-37) and the sum of an element is exact while it stays below 2^27 (1.34e8) in
 * magnitude; beyond that it wraps, unchecked.  dvol or dtheta may be NULL to skip that gradient (dloc is written only when dtheta
 * is requested); C must be 8 and H, W >= 2, as in the forward, else hipErrorInvalidValue. */
int mmseg_tps_warp_bwd(const float* vol, const float* loc, const float* Mb, const float* dout, float* dvol, float* dtheta, float* dloc,
                       float* ws, float* acc, int B, int H, int W, int C, void* stream);

/* ---- batch gather + affine (rotation) augmentation (csrc/augment.hip): keras ImageDataGenerator(rotation_range=20)
 *      .flow of model_executors/base_executor.py:37-78,103-110 = scipy affine_transform(order=1, mode='nearest') ---- */
int mmseg_affine_gather(const float* data, const int* rows, const float* mat, float* out, int B, int H, int W, int C, int order,
                        void* stream);
/* the whole ImageDataGenerator pixel surface of get_datagen_params() (model_executors/base_executor.py:37-78,103-110; keras 2.1.6
 * random_transform): per-sample 2x3 fp64 matrix mat [B,6] (rotation, shift, shear, zoom about the centre, flips folded in),
 * fill_mode 0 nearest / 1 constant (cval) / 2 reflect / 3 wrap with scipy.ndimage's boundary rules, order 0 or 1; shift [B,C]
 * or NULL: random_channel_shift, out = clip(x_c + shift[b][c], min, max of the transformed sample).  rows NULL = identity;
 * data holds N slices.  ws: mmseg_augment_workspace_floats(B, H, W, C) floats (only read with a shift). */
long mmseg_augment_workspace_floats(int B, int H, int W, int C);
int mmseg_augment_gather(const float* data, const int* rows, const double* mat, const float* shift, float* out, float* ws, int N,
                         int B, int H, int W, int C, int order, int fill_mode, float cval, void* stream);

/* ---- elastic deformation of training batches (csrc/augment.hip; build-defined: Simard 2003 / albumentations' ElasticTransform) ----
 * A random smooth displacement field that depends on (seed, batch, sample, pixel) only:
 *   noise  P = Philox4x32-10(counter (r*W + c, b, 0, 0), key (seed, batch)), multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments
 *          0x9E3779B9 / 0xBB67AE85;  u_a = (P[a] >> 8) * 2^-23 - 1, a = 0 (row), 1 (column): exact in fp32, in [-1, 1 - 2^-23]
 *   blur   g_a = scipy.ndimage.gaussian_filter(u_a[b], sigma, mode='reflect', truncate=4.0): separable, radius R = int(4 sigma + 0.5),
 *          half-sample symmetric reflection of period 2n (right when R exceeds the extent); both passes multiply and add in fp64
 *   field  disp[b][r][c][a] = (float)(scale[b] * g_a); a sample with scale[b] == 0 gets +0.0 everywhere and is not blurred
 * scale [B] fp64 and weights [R+1] fp64 (w_0 .. w_R of the normalised kernel, w_-k = w_k) on the device, disp [B,H,W,2] fp32, ws:
 * mmseg_elastic_workspace_doubles(B, H, W) doubles, 16-byte aligned (the query launches nothing and returns 0 for a refused shape).  seed and batch are read
 * as 32-bit patterns.  1 <= R <= 128, B, H <= 65535, H*W < 2^30; anything else or a null pointer is refused (hipErrorInvalidValue, nothing
 * is launched); B == 0 does nothing.  Two launches in a fixed summation order: two runs are bitwise equal.  No host synchronisation,
 * allocation or copy. */
long mmseg_elastic_workspace_doubles(int B, int H, int W);
int mmseg_elastic_field(const double* scale, const double* weights, float* disp, double* ws, int seed, int batch, int B, int H, int W,
                        int R, void* stream);
/* mmseg_augment_gather with the field added to the output pixel before the matrix, in fp64:
 *   sr = m0*(r + disp_r) + m1*(c + disp_c) + m2,  sc = m3*(r + disp_r) + m4*(c + disp_c) + m5
 * i.e. z(p) = x(M (p + d(p))): an elastic warp of the affinely transformed sample with one interpolation and the boundary rule applied
 * once.  Everything after the coordinates (fill modes, orders, zero-weight taps, NaN rows, channel shift) is mmseg_augment_gather's;
 * an all-zero field gives its bits.  disp [B,H,W,2] fp32, not NULL. */
int mmseg_elastic_gather(const float* data, const int* rows, const double* mat, const float* disp, const float* shift, float* out,
                         float* ws, int N, int B, int H, int W, int C, int order, int fill_mode, float cval, void* stream);

/* ---- MR intensity augmentation of a gathered batch (csrc/intensity.hip; build-defined, after nnU-Net's gamma / contrast / noise / blur
 *      transforms and TorchIO's RandomBiasField) ----
 * x [B,H,W,C] fp32 is an image array of one training batch as the gathers above wrote it.  lo, hi, mean are the minimum, maximum and mean
 * of a sample measured ONCE, before any intensity operation.  In this order, in fp64, rounded to fp32 once at the end:
 *   blur      v = scipy.ndimage.gaussian_filter(x, sigma, mode='reflect', truncate=4.0) over H and W per channel, rounded to fp32
 *             (mmseg_intensity_blur; the steps below are mmseg_intensity_apply)
 *   bias      v = lo + (v - lo) * exp(f[r][c]), f = component 0 of field [B,H,W,2] (an mmseg_elastic_field), one value for all channels
 *   contrast  v = mean + (v - mean) * c
 *   clip      v = min(max(v, lo), hi), only after bias or contrast
 *   gamma     if hi > lo: t = clamp((v - lo) / (hi - lo), 0, 1); t = invert ? 1 - pow(1 - t, g) : pow(t, g); v = lo + t * (hi - lo)
 *   noise     v += std * sqrt(-2 ln u1) * cos(2 pi u2), u1 = ((P[0] >> 8) + 1) * 2^-24 in (0, 1], u2 = (P[1] >> 8) * 2^-24,
 *             P = Philox4x32-10(counter (e, b, array, 3), key (seed, batch)), e = (r*W + c)*C + ch; no clip afterwards
 * Shapes: 1 <= B <= 65535, H*W*C <= 2^31 - 1 - 65536 (32-bit element indices; below the 2^32 of the noise counter); the blur also needs
 * H <= 65535, B*C <= 65535 and H*W < 2^30.  Anything else or a null pointer is refused (hipErrorInvalidValue, nothing is launched); B == 0
 * does nothing.  Every sum runs in a fixed order: two runs are bitwise equal.  No host synchronisation, allocation or copy.
 *
 * ws: mmseg_intensity_workspace_doubles(B, H, W, C) doubles serve either mmseg_intensity_stats or mmseg_intensity_blur (launches of one
 * stream run in order); the query launches nothing and returns 0 for a refused shape. */
long mmseg_intensity_workspace_doubles(int B, int H, int W, int C);
/* stats [B,3] fp64 = (min, max, sum) of every sample: per-block partials (wave64 shuffles + LDS) in ws, then one block per sample folds
 * them.  The table stays on the device for mmseg_intensity_apply. */
int mmseg_intensity_stats(const float* x, double* stats, double* ws, int B, int H, int W, int C, void* stream);
/* separable blur with a per-sample radius: radius [B] int32 (0: the sample is copied bit for bit; above 32 is read as 32), weights [B,33]
 * fp64 (row b holds w_0 .. w_radius[b] of the normalised kernel, w_-k = w_k), half-sample symmetric reflection of period 2n (right when
 * the radius exceeds the extent), fp64 sums along W into ws, then along H; out [B,H,W,C] fp32, not x. */
int mmseg_intensity_blur(const float* x, const int* radius, const double* weights, float* out, double* ws, int B, int H, int W, int C,
                         void* stream);
/* in place on x.  params [B,5] fp64 per sample: flags (1 bias + 2 contrast + 4 gamma + 8 noise), c, g, invert (non-zero: the curve is
 * applied to the inverted sample), std.  stats: the table of mmseg_intensity_stats taken BEFORE the blur.  field NULL: no sample is
 * biased.  A sample whose flags are 0 is neither read nor written; the noise is drawn only where its flag is set.  seed, batch and array
 * are read as 32-bit patterns. */
int mmseg_intensity_apply(float* x, const double* params, const double* stats, const float* field, int seed, int batch, int array,
                          int B, int H, int W, int C, void* stream);

/* ---- MR k-space artefact augmentation of a gathered batch (csrc/kspace.hip; build-defined, after TorchIO's RandomMotion / RandomGhosting /
 *      RandomSpike and MONAI's GibbsNoise / KSpaceSpikeNoise / RicianNoise) ----
 * x [B,H,W,C] fp32 as above.  lo_b = column 0 of the [B,3] table of mmseg_intensity_stats taken on x as gathered, y = x - lo_b >= 0,
 * X = fft2(y) per channel in complex fp64, numpy's convention (unshifted; the inverse scaled by 1 / (H W)).  Signed frequencies
 * ky = u < ceil(H/2) ? u : u - H, kx likewise (numpy.fft.fftfreq(H) * H); p the phase-encode axis (0 rows, 1 columns), k_p the signed
 * frequency along it, P its extent.  table [B,48] fp64, one row per sample:
 *   [0] flags = 1 motion + 2 ghosting + 4 Gibbs + 8 spikes + 16 Rician     [1] p     [2] number of breaks (<= 7)     [3..9] sorted breaks
 *   [10..25] (dy, dx) in pixels of segments 0 .. 7; the host puts (0, 0) into the segment that holds k_p = 0
 *   [26] n, [27] 1 - a of the ghosts     [28] T = f f H H W W of the Gibbs cut     [29] K <= 4 spikes
 *   [30..45] per spike (ky mod H, kx mod W, s cos phi, s sin phi)     [46] std of the Rician draw     [47] unused
 * In this order, each only where its flag is set:
 *   motion  X *= exp(-2 pi i (ky dy / H + kx dx / W)) with the shift of segment seg(k_p + floor(P/2)), seg(l) = number of breaks <= l
 *   ghost   X *= 1 - a where k_p != 0 and k_p mod n == 0
 *   gibbs   X = 0 where 4 (ky^2 W^2 + kx^2 H^2) > T (the left side is an exact integer in fp64)
 *   spikes  X[ky mod H][kx mod W] += A (s cos phi + i s sin phi), then X[-ky mod H][-kx mod W] += A (s cos phi - i s sin phi), spike after
 *           spike, both adds also where the two places coincide; A = (sum - H W C lo) / C from the stats table: for C = 1 the DC term
 *           sum(y), the spectrum's maximum; every element looks its spikes up, nothing is scattered
 *   rician  z = ifft2(X) + std sqrt(-2 ln u1) (cos 2 pi u2 + i sin 2 pi u2), u1 = ((P[0] >> 8) + 1) * 2^-24, u2 = (P[1] >> 8) * 2^-24,
 *           P = Philox4x32-10(counter (e, b, array, 5), key (seed, batch)), e = (r*W + c)*C + ch
 *   output  x = (float)(lo_b + |z|), no clip: an undershoot of the Gibbs ringing folds up, as in a magnitude image
 * A sample whose flags are 0 is neither read nor written and its slot of spec is left alone; a flagged sample whose spectrum stays as it
 * was comes back within one fp32 rounding of lo + (x - lo), not bit for bit.
 *
 * The transform: 2 <= H, W <= 1024 with no prime factor but 2, 3, 5; Stockham autosort in LDS with radix 4 / 2 / 3 / 5 passes over the
 * roots of twiddles [H + W] complex fp64: (cos, sin)(2 pi k / H), k < H, then the same for W, made by the host in fp64.  Also needed:
 * 1 <= B, B*C <= 65535, H*W*C < 2^31, spec and twiddles 16-byte aligned.  Anything else or a null pointer is refused
 * (hipErrorInvalidValue, nothing is launched); B == 0 does nothing.  No atomics and a fixed order of operations: two runs are bitwise
 * equal.  No host synchronisation, allocation or copy.
 *
 * mmseg_kspace_workspace_doubles: the doubles of spec [B,C,H,W] complex fp64, 2 B C H W; launches nothing, 0 for a refused shape. */
long mmseg_kspace_workspace_doubles(int B, int H, int W, int C);
/* spec = fft2(x - lo_b) of the flagged samples: one launch along W (a block per row), one along H (a block per tile of 16 / 8 / 4 / 2
 * adjacent columns for H <= 128 / 256 / 512 / 1024) */
int mmseg_kspace_forward(const float* x, const double* table, const double* stats, const double* twiddles, double* spec, int B, int H,
                         int W, int C, void* stream);
/* motion, ghosting, Gibbs and spikes on spec, in place: one launch */
int mmseg_kspace_apply(double* spec, const double* table, const double* stats, int B, int H, int W, int C, void* stream);
/* x = (float)(lo_b + |ifft2(spec) + the Rician draw|) of the flagged samples: one launch along H, in place on spec (which is left holding
 * that half-transformed image), one along W.  seed, batch and array are read as 32-bit patterns. */
int mmseg_kspace_inverse(double* spec, const double* table, const double* stats, const double* twiddles, float* x, int seed, int batch,
                         int array, int B, int H, int W, int C, void* stream);

/* ---- losses (csrc/loss.hip): costs.py:43-85,129-136, keras mae/mse, costs.ypred ---------------------------- */
int mmseg_segloss_workspace_floats(int B);
int mmseg_segloss_stats_floats(int B);
int mmseg_segloss_coef_floats(int B, int C);
int mmseg_segloss_class_offset(int B);
int mmseg_segloss_stats(const float* pred, const float* target, float* stats, float* ws, int B, long HW, int C, int nm, void* stream);
/* n_pix_global normalises the loss value (pixels of the whole data-parallel batch); n_pix_grad normalises the gradient
 * coefficients (the LOCAL pixel count: the gradient all-reduce takes the mean over ranks).  Equal on one device. */
int mmseg_segloss_finalize(const float* stats, float* loss, float* coef, int B, int C, float n_pix_global, float n_pix_grad,
                           float lambda_bce, void* stream);
int mmseg_segloss_grad(const float* pred, const float* target, const float* coef, float* dpred, int B, long HW, int C, int nm,
                       float scale, int use_bce, void* stream);
/* build-defined (dynamic loss scale, see mmseg_unscale_check8): the same gradient with the factor scale * scale_dev[0] */
int mmseg_segloss_grad_s(const float* pred, const float* target, const float* coef, float* dpred, int B, long HW, int C, int nm,
                         float scale, const float* scale_dev, int use_bce, void* stream);
/* ---- in-graph per-sample loss terms of the automated-pairing trainers (csrc/pairloss.hip): model_components/balancer.py:33-38
 *      (pair dice), costs.py:24-26 (mae_single_input), costs.py:43-49,88-108,138-143 (combined dice + swapped-argument
 *      per-batch cross-entropy), keras Multiply/Add of models/dafnet.py:290-312 (row dot) ------------------------------ */
int mmseg_pairloss_workspace_floats(int B);
int mmseg_pair_dice_fwd(const float* a, const float* b, float* stats, float* out, int ldo, float* ws, int B, long per_sample,
                        void* stream);
int mmseg_pair_dice_bwd(const float* a, const float* b, const float* stats, const float* g, int ldg, float* da, float* db,
                        int accumulate_a, int B, long per_sample, void* stream);
int mmseg_row_mae_fwd(const float* x, const float* y, float* out, float* ws, int B, long per_sample, void* stream);
int mmseg_row_mae_bwd(const float* x, const float* y, const float* g, float* dy, int B, long per_sample, void* stream);
int mmseg_segpb_stats_floats(int B);
int mmseg_segpb_class_offset(int B);
int mmseg_segpb_stats(const float* pred, const float* target, float* stats, float* ws, int B, long HW, int C, int nm, void* stream);
int mmseg_segpb_loss(const float* stats, float* loss, int B, long HW, int C, float lambda_bce, void* stream);
int mmseg_segpb_classgrad(const float* stats, const float* g, float* A, int B, void* stream);
int mmseg_segpb_grad(const float* target, const float* stats, const float* g, const float* A, float* dpred, int B, long HW, int C,
                     int nm, float lambda_bce, void* stream);
int mmseg_rowdot_fwd(const float* w, const float* l, float* out, int B, int J, void* stream);
int mmseg_rowdot_bwd(const float* w, const float* l, const float* g, float* dw, float* dl, int B, int J, void* stream);

int mmseg_diffloss_workspace_floats(void);
/* mode 0: mean|p-t|, 1: mean (p-t)^2, 2: mean p ; t == NULL -> constant target tconst */
int mmseg_diffloss(const float* p, const float* t, float tconst, long n, int mode, float* loss, float* ws, void* stream);
int mmseg_diffloss_grad(const float* p, const float* t, float tconst, long n, int mode, float scale, float* dp, void* stream);
/* build-defined (dynamic loss scale): the same gradient with the factor scale * scale_dev[0] */
int mmseg_diffloss_grad_s(const float* p, const float* t, float tconst, long n, int mode, float scale, const float* scale_dev, float* dp,
                          void* stream);

/* ---- boundary loss of the segmentor (csrc/boundary.hip; BUILD-DEFINED, conf.w_boundary: the reference's losses hold no distance.
 *      Kervadec et al., "Boundary loss for highly unbalanced segmentation", MIDL 2019) ----
 * mmseg_boundary_map: target [B,H,W,C] fp32 NHWC (the tensor mmseg_segloss_* reads), foreground of channel k < nm is target > 0.5;
 * phi [B,H,W,nm] fp32, every element written.  Per sample and channel, with d_fg(q) / d_bg(q) the Euclidean distance in pixels from
 * q to the nearest foreground / background pixel (the image edge is not background):
 *     phi(q) = d_fg(q) where q is background,  phi(q) = -(d_bg(q) - 1) where q is foreground,
 *     phi = 0 everywhere for a mask that is empty or full
 * (one_hot2dist of the paper's code over scipy.ndimage.distance_transform_edt; the full mask is defined here).  Exact: int32 squared
 * distances from a two-pass separable minimum, one correctly rounded sqrtf, then the "- 1" in fp32.  1 <= nm <= C <= 8,
 * 1 <= H, W <= 2048 (H^2 + W^2 < 2^24), 1 <= B <= 65535; anything else, or a null pointer, returns hipErrorInvalidValue and launches
 * nothing.  ws: mmseg_boundary_workspace_bytes(B, H, W, nm) bytes (0 for arguments that would be refused).  No host synchronisation,
 * no allocation, no atomics: two runs are bitwise equal, and the launches may be recorded into a hipGraph.
 * mmseg_boundary_loss: loss_b[0] = sum over b, px, k < nm of pred[b,px,k] * phi[b,px,k], divided by B * HW * nm; pred [B,HW,C], phi
 * [B,HW,nm].  Two stages in a fixed order; ws: mmseg_boundary_loss_workspace_floats(B) floats.
 * mmseg_boundary_grad_add: for k < nm, dpred[b,px,k] += s * phi[b,px,k] with s = ((scale_host * scale_dev[0]) * weight_dev[0]) /
 * (float)(B * HW * nm), every step rounded to fp32 (scale_dev == NULL: the factor is left out); channels >= nm are not touched.  It adds
 * to what mmseg_segloss_grad[_s] wrote.  weight_dev [1] lives on the device so that a recorded step follows a weight the host changes
 * between replays.
 * mmseg_boundary_combine: loss[0] += weight_dev[0] * loss_b[0] (one thread; loss_b stays as it was). */
long mmseg_boundary_workspace_bytes(int B, int H, int W, int nm);
int mmseg_boundary_map(const float* target, float* phi, int* ws, int B, int H, int W, int C, int nm, void* stream);
int mmseg_boundary_loss_workspace_floats(int B);
int mmseg_boundary_loss(const float* pred, const float* phi, float* loss_b, float* ws, int B, long HW, int C, int nm, void* stream);
int mmseg_boundary_grad_add(const float* phi, float* dpred, int B, long HW, int C, int nm, float scale_host, const float* scale_dev,
                            const float* weight_dev, void* stream);
int mmseg_boundary_combine(float* loss, const float* loss_b, const float* weight_dev, void* stream);

/* ---- Lovasz-Softmax loss of the segmentor (csrc/lovasz.hip; BUILD-DEFINED, conf.w_lovasz: the reference's losses hold no sort.
 *      Berman et al., "The Lovasz-Softmax loss", CVPR 2018; here per image and over the organ channels k < nm only) ----
 * Per sample b and channel k < nm, over the P = HW pixels:
 *     y_i = target > 0.5 ? 1 : 0,   e_i = fabsf(y_i - p_i) in fp32 (one subtraction)
 *     order: e descending, equal e by pixel index ascending (numpy.argsort(-e, kind='stable'))
 *     G = sum y;  c / n = the positives / negatives strictly before a sorted position
 *     g = 1 / (G + n)                                   y = 1
 *     g = (G - c) / ((G + n) (G + n + 1))               y = 0, G > 0
 *     g = 1 at the first position, 0 elsewhere          G = 0            (lovasz_grad, J_k - J_{k-1}, without cancellation)
 *     m[b,i,k] = s_i g_i q_b,  s = +1 for y = 0, -1 for y = 1;  m = 0 where e_i == 0;  q_b = 1 / (B |K_b|), K_b the classes with G > 0
 *     (classes_all = 0, 'present') or all nm classes (classes_all != 0); m = 0 for a class outside K_b (so for a sample with empty K_b)
 *     L = sum over b, i, k of m (p - y)  in [0, 1];   dL/dp = m (the order is constant almost everywhere).
 * mmseg_lovasz_map: pred, target [B,HW,C] fp32 NHWC; m [B,HW,nm] fp32, every element written.  A stable least-significant-digit radix
 * sort (four 8-bit passes over the bit pattern of e) of 64-bit records per (b, k), a scan of the label bit along the sorted order, g in
 * fp64 from the integers, times q_b, rounded to fp32 once.  1 <= nm <= C <= 8, 1 <= HW <= 2^22, 1 <= B <= 65535; anything else, or a null
 * pointer, returns hipErrorInvalidValue and launches nothing.  ws: mmseg_lovasz_workspace_bytes(B, HW, nm) bytes, 8-byte aligned (0 for
 * arguments that would be refused).  No host synchronisation, no allocation, integer atomics only: two runs are bitwise equal; every
 * grid is a function of (B, HW, nm), so the launches may be recorded into a hipGraph.  Non-finite pred: the kernels terminate, stay in
 * bounds and write every element; the values are unspecified.
 * mmseg_lovasz_loss: loss_l[0] = sum m * (p - y), fp64 in two stages of a fixed order, rounded once; ws:
 * mmseg_lovasz_loss_workspace_floats(B) floats, 8-byte aligned.
 * mmseg_lovasz_grad_add: for k < nm, dpred[b,px,k] += ((scale_host * scale_dev[0]) * weight_dev[0]) * m[b,px,k], every step rounded to
 * fp32 (scale_dev == NULL: the factor is left out); channels >= nm are not touched.  It adds to what mmseg_segloss_grad[_s] and
 * mmseg_boundary_grad_add wrote.  The weighted term enters the loss through mmseg_boundary_combine. */
long mmseg_lovasz_workspace_bytes(int B, long HW, int nm);
int mmseg_lovasz_map(const float* pred, const float* target, float* m, int* ws, int B, long HW, int C, int nm, int classes_all, void* stream);
int mmseg_lovasz_loss_workspace_floats(int B);
int mmseg_lovasz_loss(const float* pred, const float* target, const float* m, float* loss_l, float* ws, int B, long HW, int C, int nm, void* stream);
int mmseg_lovasz_grad_add(const float* m, float* dpred, int B, long HW, int C, int nm, float scale_host, const float* scale_dev,
                          const float* weight_dev, void* stream);

/* ---- optimiser / regulariser (csrc/optim.hip)---------------------------------------------------------- */
/* Keras 2.1.6 Adam step over a flat arena (models/dafnet.py:93,114,155,161) */
int mmseg_adam(float* p, const float* g, float* m, float* v, long n, float lr_t, float b1, float b2, float eps, void* stream);
/* the same update with lr_t read from device memory (one float) -- the form recorded when a training step is captured into a hipGraph */
int mmseg_adam_p(float* p, const float* g, float* m, float* v, long n, const float* lr_t, float b1, float b2, float eps, void* stream);
/* layers/spectralnorm.py:199-239 */
long mmseg_spectral_workspace_floats(int K, int N);
int mmseg_spectral_fwd(const float* w, const float* u0, float* loss, float* sgn, float* ws, int K, int N, float alpha, void* stream);
int mmseg_spectral_grad(const float* w, const float* sgn, float scale, long n, float* dw, void* stream);
/* the penalties of up to 4 matrices (the 4 down-sample blocks of one discriminator, models/discriminator.py:24-41) in one batch
 * of launches: loss[i], sgn[i]; ws = the per-matrix workspaces back to back; and their gradients accumulated into dw_i */
int mmseg_spectral_fwd4(const float* w0, const float* w1, const float* w2, const float* w3, const float* u0, const float* u1,
                        const float* u2, const float* u3, float* loss, float* sgn, float* ws, int n, int K0, int N0, int K1, int N1,
                        int K2, int N2, int K3, int N3, float alpha, void* stream);
int mmseg_spectral_grad4(const float* w0, const float* w1, const float* w2, const float* w3, const float* sgn, float* dw0, float* dw1,
                         float* dw2, float* dw3, int n, long n0, long n1, long n2, long n3, float scale, void* stream);
/* build-defined (dynamic loss scale): the same accumulation with the factor scale * scale_dev[0] */
int mmseg_spectral_grad4_s(const float* w0, const float* w1, const float* w2, const float* w3, const float* sgn, float* dw0, float* dw1,
                           float* dw2, float* dw3, int n, long n0, long n1, long n2, long n3, float scale, const float* scale_dev,
                           void* stream);

/* ---- dynamic loss scaling (csrc/optim.hip): build-defined, the reference trains in fp32 and has none ------------------------------
 * torch.cuda.amp.GradScaler semantics with power-of-two factors, all state in device memory (no host read during a step, so a step
 * may be captured into a hipGraph): scale[1] (fp32, a power of two) and st[4] (int32) = {found_inf, growth counter, skipped steps,
 * Adam iterations}.  One step: the seed gradients use the _s entry points above with scale_dev = scale; mmseg_unscale_check8 over
 * the trainer's gradient arenas; mmseg_adam_guarded per arena; mmseg_loss_scale_update. */
/* g_i *= 1 / scale[0] for the first `count` (1..8) arenas (16-byte aligned, any length); st[0] = 1 if any element was +-inf or NaN
 * (exponent bits all ones).  st[0] is only ever set here, never cleared. */
int mmseg_unscale_check8(float* g0, float* g1, float* g2, float* g3, float* g4, float* g5, float* g6, float* g7, long n0, long n1,
                         long n2, long n3, long n4, long n5, long n6, long n7, int count, const float* scale, int* st, void* stream);
/* mmseg_adam_p's update (models/dafnet.py:93,114,155,161) with lr_t = lr_table[min(st[3] + 1, table_len) - 1] (the host writes
 * lr_table[j] = lr_t(j + 1) in fp64-then-fp32, its last entry equal to lr); p, m, v untouched when st[0] is set */
int mmseg_adam_guarded(float* p, const float* g, float* m, float* v, long n, const float* lr_table, int table_len, const int* st,
                       float b1, float b2, float eps, void* stream);
/* end of a step (one thread): st[0] set -> scale = max(scale / 2, 1), st[1] = 0, st[2] += 1; else st[3] += 1, st[1] += 1 and at
 * growth_interval scale *= 2 (at most 2^127), st[1] = 0.  Clears st[0]. */
int mmseg_loss_scale_update(float* scale, int* st, int growth_interval, void* stream);

/* ---- volume preprocessing (csrc/preprocess.hip): loaders/chaos.py:324-343 (resample = skimage.transform.rescale, order 1 for
 * images / order 0 for labels, mode='constant', no anti-aliasing), 303-319 (grey label value -> one binary channel per organ),
 * 242-246 (every slice to [-1, 1] by the min / max of the whole resampled slice), 248-264 (utils/data_utils.crop_same, mode 'equal',
 * pad_mode 'edge').  One call handles the S raw slices [S,H,W] of one (volume, modality) and writes its channels of the NHWC
 * containers the gather kernels read; the resampled RH x RW frame (RH = round(H * old_res / target_res), decided by the caller) is
 * never stored.  Source coordinate of resampled pixel d: (d + 0.5) * (in / out) - 0.5 in fp64; outside [0, in-1] -> 0.
 * Per axis the final index o reads resampled index lo + clamp(o - before, 0, kept - 1): crop (lo), the odd-surplus quirk of
 * data_utils._crop (kept = size - 1) and edge padding (before) in one map; 0 <= lo, kept >= 1, lo + kept <= R, 0 <= before < O.
 * The label entry point is the one place where a tensor is not fp32: lab holds the uint8 grey values as read from disk. */
long mmseg_preprocess_workspace_floats(int S, int RH, int RW);
/* ws[S][blocks][2] = (min, max) partials of the bilinearly resampled slices; read by mmseg_preprocess_image with the same S, RH, RW */
int mmseg_preprocess_minmax(const float* img, float* ws, int S, int H, int W, int RH, int RW, void* stream);
/* out [S,OH,OW,C], channel ch = 2 * (v - min) / (max - min) - 1 (a constant slice: -1) */
int mmseg_preprocess_image(const float* img, const float* ws, float* out, int S, int H, int W, int RH, int RW, int OH, int OW, int lo_r,
                           int kept_r, int before_r, int lo_c, int kept_c, int before_c, int C, int ch, void* stream);
/* out [S,OH,OW,C], channel ch0 + k = (nearest label (tap floor(c + 0.5)) == values[k]) as 0 / 1, k < K <= 16; values [K] int32 on
 * the device */
int mmseg_preprocess_label(const unsigned char* lab, const int* values, float* out, int S, int H, int W, int RH, int RW, int OH, int OW,
                           int lo_r, int kept_r, int before_r, int lo_c, int kept_c, int before_c, int C, int ch0, int K, void* stream);

/* ---- percentile-window and landmark intensity normalisation (csrc/preprocess.hip; build-defined, the reference rescales by min / max) --
 * Population of a (volume, modality): the values the bilinear resampling above produces over the WHOLE RH x RW frame of every
 * slice, the zeros of the strict border rule included -- what mmseg_preprocess_minmax visits.  A segment is one slice (per_volume
 * = 0: G = S segments of N = RH * RW values) or the volume (per_volume = 1: G = 1, N = S * RH * RW); N >= 2^31 is refused.
 * Knots: for percentiles q_0 < ... < q_{K-1} in [0, 100], 2 <= K <= 16, knot x_k of a segment is its order statistic of rank
 * r_k = floor((N - 1) * (q_k / 100)), computed by the CALLER in fp64 in that order (numpy's method='lower'); the device is given
 * ranks, 0 <= r_k <= N - 1, never percentiles.  The selected value is an element of the population bit for bit (the order is IEEE
 * totalOrder: -0 below +0); nothing is interpolated between ranks.
 * Map of a resampled value v through its segment's knots x and the targets y [K] (non-decreasing, y_0 < y_{K-1}), in fp32 without
 * contraction: v <= x_0 -> y_0 exactly; v >= x_{K-1} -> y_{K-1} exactly; otherwise, with k the largest index that has x_k < v (so
 * x_k < v <= x_{k+1} and the denominator is positive), fminf(y_k + (v - x_k) * ((y_{k+1} - y_k) / (x_{k+1} - x_k)), y_{k+1}).
 * Equal knots need no special case; a constant segment gives y_0 everywhere.
 * Bytes of the workspace of one mmseg_preprocess_quantiles call (per segment K prefixes and K ranks, and four histograms
 * [G][K][256] of uint32); 0 for S < 1 or K outside 2..16 */
long mmseg_preprocess_quantiles_workspace_bytes(int S, int K, int per_volume);
/* x [G,K] fp32 = the knots of every segment of img [S,H,W]; ranks [K] int32 on the device, the same for every segment.  Radix select
 * on the order-preserving key of an fp32 value, four passes of 8-bit digits, each recomputing the resampling; integer atomics only,
 * so two runs are bitwise equal.  ws is zeroed here, on the stream. */
int mmseg_preprocess_quantiles(const float* img, const int* ranks, int* ws, float* x, int S, int H, int W, int RH, int RW, int K,
                               int per_volume, void* stream);
/* mmseg_preprocess_image with the map above in place of the min / max rescale: out [S,OH,OW,C], channel ch; slice s uses row
 * (per_volume ? 0 : s) of x [G,K]; y [K] fp32 on the device */
int mmseg_preprocess_image_map(const float* img, const float* x, const float* y, float* out, int S, int H, int W, int RH, int RW, int OH,
                               int OW, int lo_r, int kept_r, int before_r, int lo_c, int kept_c, int before_c, int C, int ch, int K,
                               int per_volume, void* stream);

/* ---- predicted label volumes on a volume's own grid (csrc/postprocess.hip; build-defined, the reference writes no segmentation) ----
 * mmseg_restore_label inverts the geometry of mmseg_preprocess_label and binarises in the same pass: prob [S,OH,OW,C] (the
 * segmentor's output, the K <= 16 organ channels first, K <= C) -> out [S,H,W] uint8 grey values, every byte written.  Per axis the
 * raw index d has the resampled coordinate (d + 0.5) * (R / n) - 0.5 in fp64, clamped into [0, R - 1]; outside [lo, lo + kept - 1]
 * the pixel was cropped away on the way in and gets 0; inside, the container coordinate is coord - lo + before.  order 1 samples
 * every organ channel bilinearly (fp32, the expression order of the image resampling), order 0 takes the tap floor(coord + 0.5)
 * limited to the window.  The pixel gets values[k] of the lowest k whose sampled probability is > 0.5, else 0.  (lo, kept, before)
 * and (RH, RW) are the ones given to mmseg_preprocess_*; additionally before + kept <= O, since this direction reads the window. */
int mmseg_restore_label(const float* prob, const int* values, unsigned char* out, int S, int H, int W, int RH, int RW, int OH, int OW,
                        int lo_r, int kept_r, int before_r, int lo_c, int kept_c, int before_c, int C, int K, int order, void* stream);
/* pred, truth [S,n] uint8 (n = H * W pixels per slice) -> counts [S,K,3] int32 = |pred == values[k]|, |truth == values[k]|, |both| per
 * slice and organ.  The launcher zeroes counts on the stream; integer sums, so two runs are bitwise equal. */
int mmseg_label_overlap(const unsigned char* pred, const unsigned char* truth, const int* values, int* counts, int S, int n, int K,
                        void* stream);

/* ---- scores in mm on a volume's own grid (csrc/postprocess.hip; build-defined, the reference scores Dice only) ----------------------
 * K + 1 binary problems per label volume [S,H,W]: problem k < K has foreground "== values[k]", problem K "equals any of values".
 * S * H * W < 2^31, 1 <= K <= 16, spacings (mm between slices, rows, columns) finite and > 0; anything else is refused.  S == 0 does
 * nothing.  A surface voxel is a foreground voxel with a face neighbour that is background or outside the volume.  Distances are
 * exact: three per-axis passes out[i] = min over all j of in[j] + (spacing * (i - j))^2 in fp64, then one square root.
 * surf [K+1,S,H,W] uint8 0 / 1, every byte written; counts [K+1][2] int32 = (|foreground|, |surface|), zeroed on the stream, or null */
int mmseg_label_surface(const unsigned char* label, const int* values, unsigned char* surf, int* counts, int S, int H, int W, int K,
                        void* stream);
/* out [S,H,W] fp64 = mm to the nearest non-zero voxel of sites [S,H,W] (+inf when there is none); tmp: S * H * W doubles of scratch */
int mmseg_distance_to_sites(const unsigned char* sites, double* out, double* tmp, int S, int H, int W, double dz, double dy, double dx,
                            void* stream);
long mmseg_surface_metrics_workspace_doubles(int S, int H, int W, int K);
/* table [K+1,6] fp64 = nP, nT, |surface(P)|, |surface(T)|, sum and max over both surfaces of the distance to the other one (nan when
 * either surface is empty).  The sum is reduced in a fixed order (per-block partials in ws, one final block): two runs are bitwise
 * equal.  ws: mmseg_surface_metrics_workspace_doubles(S, H, W, K) doubles. */
int mmseg_surface_metrics(const unsigned char* pred, const unsigned char* truth, const int* values, double* table, double* ws, int S,
                          int H, int W, int K, double dz, double dy, double dx, void* stream);

/* ---- order statistics of the surface distances (csrc/postprocess.hip; build-defined: HD(q) and NSD(tau) of INTEGRATION.md section 5) ----
 * The multiset D = {a[e] : ma[e] != 0} + {b[e] : mb[e] != 0} over a, b [n] fp64 and ma, mb [n] uint8, N = |D|.  By contract every selected
 * value is finite and >= 0 (such a value orders as its bit pattern, which is what the selection works on); unselected values may be
 * anything.  The percentile follows numpy's linear rule: h = (N - 1) * (percentile / 100) in fp64 (numpy's order of evaluation), lo = floor(h),
 * hi = min(lo + 1, N - 1), value = D_(lo) + (h - lo) * (D_(hi) - D_(lo)) over the sorted D.  0 <= n < 2^31, 0 <= percentile <= 100, 0 <= tolerance, both
 * finite; anything else or a null pointer is refused (hipErrorInvalidValue, nothing is launched).  The selection is an exact radix
 * selection on the device: no host synchronisation, allocation or copy; integer atomics only, so two runs are bitwise equal. */
/* doubles of ws for mmseg_masked_select: 2 n for the list of selected values, and the selection's state; 0 for an n it would refuse */
long mmseg_masked_select_workspace_doubles(long n);
/* out [5] fp64 = N, |{x in D : x <= tolerance}|, the percentile, D_(lo), D_(hi); the last three nan when N == 0 (n == 0 included) */
int mmseg_masked_select(const double* a, const unsigned char* ma, const double* b, const unsigned char* mb, long n, double percentile,
                        double tolerance, double* out, double* ws, void* stream);
/* doubles of ws for mmseg_surface_scores: mmseg_surface_metrics' 2 S H W (two distance maps) and surfaces, plus 2 S H W for the list of
 * surface distances: about 420 MB more for a 100 x 512 x 512 CT volume.  0 for arguments that it would refuse. */
long mmseg_surface_scores_workspace_doubles(int S, int H, int W, int K);
/* mmseg_surface_metrics with two more columns: table [K+1,8] fp64 = nP, nT, |surface(P)|, |surface(T)|, sum, max (the same kernels, the
 * same bits), then |{x in D : x <= tolerance}| and the percentile of D = the distances of surface(P) to surface(T) and of surface(T) to
 * surface(P) together, tolerance in mm; columns 5 to 8 are nan when either surface is empty.  Every distance transform runs once. */
int mmseg_surface_scores(const unsigned char* pred, const unsigned char* truth, const int* values, double* table, double* ws, int S,
                         int H, int W, int K, double dz, double dy, double dx, double percentile, double tolerance, void* stream);

/* ---- the largest connected component of every organ (csrc/postprocess.hip; build-defined: these replace nothing in the reference,
 * which writes no segmentation) -------------------------------------------------------------------------------------------------------
 * Two voxels of label [S,H,W] uint8 are joined when they hold the same grey value, that value is one of values [K] (int32, device)
 * and they are neighbours: connectivity 6 (faces) or 26 (faces, edges, corners).  S * H * W < 2^31 - 1, 1 <= H, W, 1 <= K <= 16;
 * anything else, a null pointer or another connectivity is refused (hipErrorInvalidValue, nothing is launched).  S == 0 does nothing.
 * comp [S,H,W] int32, every element written: 0 where the grey value is none of `values`, else 1 + the smallest linear index
 * (s * H * W + y * W + x) in the voxel's component.  Canonical: independent of the order of blocks and atomics, so two runs are
 * bitwise equal.  All K organs are labelled in one pass (a union-find in comp itself; parents only decrease). */
int mmseg_label_components(const unsigned char* label, const int* values, int* comp, int S, int H, int W, int K, int connectivity,
                           void* stream);
/* bytes of ws for mmseg_keep_largest_components; 0 for arguments that it would refuse */
long mmseg_keep_largest_workspace_bytes(int S, int H, int W, int K);
/* out [S,H,W] uint8 = label, except that a voxel of values[k] outside the largest component of values[k] becomes 0 (of equally large
 * components the one with the smallest linear index stays); other grey values are copied.  stats [K,3] int32 = (number of
 * components, voxels of values[k] before, voxels kept), (0, 0, 0) for an organ without voxels.  Every byte of out and stats is
 * written.  ws (8-byte aligned) is the only scratch; integer atomics only, so two runs are bitwise equal. */
int mmseg_keep_largest_components(const unsigned char* label, const int* values, unsigned char* out, int* stats, int* ws, int S, int H,
                                  int W, int K, int connectivity, void* stream);

/* ---- enclosed holes of every organ (csrc/postprocess.hip; build-defined, the rule is in INTEGRATION.md section 5) -----------------------
 * A hole of organ k is a connected component of the complement of (label == values[k]) that holds no border voxel; the complement
 * is joined through faces only.  per_slice 0: six neighbours, the border is the six faces of the volume; per_slice 1: every slice
 * on its own, four neighbours, the border is the four edges of the slice (scipy.ndimage.binary_fill_holes with its default
 * structure, on the volume or slice by slice).  S * H * W < 2^31 - 1, 1 <= H, W, 1 <= K <= 16; anything else, another per_slice or a
 * null pointer is refused (hipErrorInvalidValue, nothing is launched).  S == 0 does nothing. */
/* bytes of ws for mmseg_fill_label_holes (about 5 per voxel); 0 for arguments that it would refuse */
long mmseg_fill_label_holes_workspace_bytes(int S, int H, int W, int K);
/* out [S,H,W] uint8 = label, except that a voxel which is 0 in label and lies in a hole of organ k becomes values[k]; holes are those
 * of label itself, and where several organs enclose a voxel the lowest k wins.  Other grey values inside a hole are copied.  stats
 * [K,3] int32 = (number of holes, voxels of values[k] before, voxels added), (0, 0, 0) for an organ without voxels.  Every byte of
 * out and stats is written; out must not alias label.  ws (4-byte aligned) is the only scratch; integer atomics only and a canonical
 * labelling, so two runs are bitwise equal.  No kernel waits for another block; no host synchronisation, allocation or copy. */
int mmseg_fill_label_holes(const unsigned char* label, const int* values, unsigned char* out, int* stats, void* ws, int S, int H, int W,
                           int K, int per_slice, void* stream);

/* ---- opening, closing and smoothing of every organ by a ball in mm (csrc/postprocess.hip; build-defined, the rule is in INTEGRATION.md
 * section 5) ------------------------------------------------------------------------------------------------------------------------------
 * The ball.  For an integer offset o = (oz, oy, ox), t(o) in fp64 without contraction other than the fmas named: a = dx * ox, t = a * a;
 * b = dy * oy, t = fma(b, b, t); c = dz * oz, t = fma(c, c, t): the order of the W, H and S passes of mmseg_distance_to_sites.
 * B = { o : t(o) <= radius * radius }, the rounded fp64 product.  per_slice 1: only oz == 0 belongs to B and dz is not read.
 * For a set X of voxels of the volume: erode(X) keeps p in X iff no voxel q OF THE VOLUME outside X has q - p in B (what lies outside the
 * volume is no background: scipy.ndimage.binary_erosion(X, B, border_value=1)); dilate(X) holds p iff some q in X has q - p in B
 * (scipy.ndimage.binary_dilation(X, B)); open(X) = dilate(erode(X)), a subset of X; close(X) = erode(dilate(X)), a superset of X.
 * With X_k = (label == values[k]):
 *   op 0, open    a voxel of values[k] outside open(X_k) becomes 0
 *   op 1, close   a voxel that is 0 in label and lies in close(X_k) becomes values[k]; where several organs claim it the lowest k wins;
 *                 other organs and foreign grey values are never overwritten, and do not stop a dilation from passing
 *   op 2, smooth  op 0 on label gives L1, then op 1 with L1 as its input
 * radius and the spacings in use finite and > 0; the reach floor(radius / spacing) per axis in use at most 32; S * H * W < 2^31 - 1,
 * 1 <= H, W, 1 <= K <= 16; anything else, another op or per_slice or a null pointer is refused (hipErrorInvalidValue, nothing is
 * launched).  S == 0 does nothing.  A radius below every spacing in use gives B = {0}: out = label. */
/* bytes of ws for mmseg_smooth_label (about 3 per voxel); 0 for arguments that it would refuse */
long mmseg_smooth_label_workspace_bytes(int S, int H, int W, int K);
/* out [S,H,W] uint8 as above; stats [K,3] int32 = (voxels of values[k] in label, voxels removed, voxels added), (0, 0, 0) for an organ
 * without voxels.  Every byte of out and stats is written; out must not alias label.  ws is the only scratch.  Work per voxel follows
 * the window of the ball (2 * reach + 1 per axis), an axis of reach 0 costs no pass.  Integer atomics only, so two runs are bitwise
 * equal.  No kernel waits for another block; no host synchronisation, allocation or copy. */
int mmseg_smooth_label(const unsigned char* label, const int* values, unsigned char* out, int* stats, void* ws, int S, int H, int W, int K,
                       double dz, double dy, double dx, double radius, int op, int per_slice, void* stream);

/* ---- tiles of a frame larger than the network's input (csrc/postprocess.hip; build-defined, the rule is in INTEGRATION.md section 5) ----
 * prob [TR*TC,S,OH,OW,C] fp32: the segmentor's output for every tile of a TR x TC plan (tile tr * TC + tc), the K organ channels
 * first.  rows [TR,3] and cols [TC,3] int32 = (lo, kept, before) per tile and axis, wr [TR,OH] and wc [TC,OW] fp32 weights, all on the
 * device.  out [S,RH,RW,K] fp32, every element written: the blended map on the resampled frame.  Tile row tr covers frame row y when
 * lo <= y < lo + kept (and the container row iy = y - lo + before lies inside [0, OH)); columns alike; a container's padding is never
 * read.  Over the covering tiles in ascending (tr, tc) order, W = wr[tr][iy] * wc[tc][ix]: num_k = sum of W * p_k, den = sum of W, in
 * fp32 in that order without contraction, out_k = num_k / den.  A pixel that exactly one tile covers takes that tile's value
 * unchanged (no multiply, no divide); a pixel that no tile covers gets 0.  A gather without atomics: two runs are bitwise equal.
 * 1 <= TR, TC <= 8, 1 <= K <= min(C, 16), extents >= 1, prob and out below 2^31 bytes each; anything else or a null pointer is refused
 * (hipErrorInvalidValue, nothing is launched); out must not alias prob.  S == 0 does nothing.  No host synchronisation, allocation or
 * copy. */
int mmseg_blend_tiles(const float* prob, const int* rows, const int* cols, const float* wr, const float* wc, float* out, int S, int TR,
                      int TC, int OH, int OW, int C, int K, int RH, int RW, void* stream);

/* ---- views of a slice, merged: test-time augmentation (csrc/postprocess.hip; build-defined, the rule is in INTEGRATION.md section 5) ----
 * prob [V*N,OH,OW,C] fp32: the segmentor's output for V views of N slices, view-major (view v holds slices v * N ..), the K organ channels
 * first.  back [V,6] fp64 on the device: per view the matrix that takes an image pixel (r, c) to the view pixel that shows it, in
 * mmseg_augment_gather's convention.  out [N,OH,OW,K] fp32, every element written.  Per output pixel and view, in ascending v:
 * sr = (b0 * r + b1 * c) + b2, sc = (b3 * r + b4 * c) + b5 in fp64 without contraction; the view covers the pixel iff 0 <= sr <= OH - 1
 * and 0 <= sc <= OW - 1 (a NaN covers nothing); its sample is bilinear on the taps floor and floor + 1 (limited to the container), the
 * fractions cast to fp32, v = (1-fy)*((1-fx)*a00 + fx*a01) + fy*((1-fx)*a10 + fx*a11) in fp32 in that order, a zero fraction skipping
 * its taps: an integer coordinate returns the tap bit for bit.  num = the sum of the covering views' samples from 0 in that order,
 * in fp32 without contraction; out = num / (float)cnt; cnt == 1 copies the sample unchanged, cnt == 0 gives 0.  A gather without
 * atomics: two runs are bitwise equal.  1 <= V <= 16, 1 <= K <= min(C, 16), extents >= 1, N * OH * OW < 2^29; anything else or a null
 * pointer is refused (hipErrorInvalidValue, nothing is launched); out must not alias prob.  N == 0 does nothing.  No host
 * synchronisation, allocation or copy. */
int mmseg_merge_views(const float* prob, const double* back, float* out, int V, int N, int OH, int OW, int C, int K, void* stream);

/* ---- several models and views, their mean, its uncertainty and its calibration (csrc/postprocess.hip; build-defined, the rule is in
 * INTEGRATION.md section 5).  Common to the five entry points: a bad argument or a null pointer is refused (hipErrorInvalidValue, nothing is
 * launched); no host synchronisation, allocation or copy; two runs are bitwise equal; no kernel waits for another block; N == 0, S == 0
 * or n == 0 does nothing.
 * mmseg_members_accumulate: prob [V*N,OH,OW,C] fp32, the output of ONE model for V views of N slices, view-major, the K organ channels
 * first; back [V,6] fp64 on the device as for mmseg_merge_views (a plain model: V = 1 and the identity 1 0 0 0 1 0).  sum [N,OH,OW,K] and
 * aux [N,OH,OW,2] = (sum of h, cnt) fp32 are the accumulators: with first != 0 they count as 0 and are never read, otherwise the call
 * continues from them, so that several models stream through one pair of buffers.  Per pixel and covering view, in ascending v, with the
 * coverage test and the sample q_k of mmseg_merge_views: sum_k += q_k; rest = max(0, 1 - (((q_0 + q_1) + ..) + q_(K-1)));
 * h = t(q_0) + .. + t(q_(K-1)) + t(rest) added from 0 in that order, t(x) = x > 0 ? -x * logf(x) : 0; aux_0 += h; aux_1 += 1.  fp32
 * without contraction.  1 <= V <= 16, 1 <= K <= min(C, 16), extents >= 1, N * OH * OW < 2^29, prob below 2^31 bytes; the three buffers
 * must not alias. */
int mmseg_members_accumulate(const float* prob, const double* back, float* sum, float* aux, int first, int V, int N, int OH, int OW, int C,
                             int K, void* stream);
/* In place.  cnt = aux_1.  sum becomes the mean map: p_k = cnt == 1 ? sum_k : cnt == 0 ? 0 : sum_k / cnt (so one model's mean is
 * mmseg_merge_views's map bit for bit).  rest and Hraw = sum of t over the mean's K + 1 probabilities by the expressions above;
 * E = cnt == 1 ? aux_0 : aux_0 / cnt; inv = (float)(1 / ln(K + 1)).  aux becomes (H, I): H = min(1, Hraw * inv), the predictive entropy,
 * and I = max(0, Hraw - E) * inv, the mutual information between the label and the member (the part of H that is disagreement between
 * members), both as shares of ln(K + 1).  cnt == 0: mean 0, H = 0, I = 0.  One member gives I == 0 bit for bit. */
int mmseg_members_finish(float* sum, float* aux, int N, int OH, int OW, int K, void* stream);
/* planes [S,OH,OW,U] fp32, 1 <= U <= 4: plane 0 <= u < U goes to out [S,H,W] uint8, every byte written.  Geometry, taps and the bilinear
 * expression are those of mmseg_restore_label.  A pixel that was cropped away gets 0; inside the window the sample v becomes
 * level = (unsigned char)(min(max(v, 0), 1) * 255 + 0.5f) in fp32 without contraction. */
int mmseg_restore_map(const float* planes, unsigned char* out, int S, int H, int W, int RH, int RW, int OH, int OW, int lo_r, int kept_r,
                      int before_r, int lo_c, int kept_c, int before_c, int U, int u, int order, void* stream);
/* The reliability table of a map against a label volume.  prob [S,OH,OW,C] fp32, truth [S,H,W] uint8, values [K] int32 on the device,
 * 2 <= B <= 64, S * H * W < 2^31 - 1.  For every raw pixel inside the window (the others are skipped) and every organ k: p is sampled as
 * mmseg_restore_label samples it, y = truth == values[k], b = min(B - 1, (int)(p * (float)B)) in fp32 (and at least 0).
 * bins [K,B,2] int32 = (n, positives) per organ and bin: zeroed on the stream, integer atomics.  sums [K,B+2] fp64, every element written:
 * per organ the sum of p in each bin, then the sum of (p - y)^2 (fp64 from the fp32 p), then the sum of -logf(max(y ? p : 1 - p, 1e-6))
 * (fp32 terms).  Every sum is taken in one fixed order (per block over its pixels in ascending order, then over the blocks): no
 * floating-point atomics.  ws: the bytes the query returns (0 for arguments that the call would refuse). */
long mmseg_calibration_table_workspace_bytes(int S, int H, int W, int K, int B);
int mmseg_calibration_table(const float* prob, const unsigned char* truth, const int* values, int* bins, double* sums, double* ws, int S,
                            int H, int W, int RH, int RW, int OH, int OW, int lo_r, int kept_r, int before_r, int lo_c, int kept_c,
                            int before_c, int C, int K, int B, int order, void* stream);
/* pred, truth [n] uint8, levels [U,n] uint8 (1 <= U <= 4, n < 2^31 - 1) -> out [2,1+U] int64, zeroed on the stream: row 0 covers the
 * pixels with pred == truth, row 1 the others; a row holds their number and, per plane, the sum of their levels.  Integers only. */
int mmseg_uncertainty_by_error(const unsigned char* pred, const unsigned char* truth, const unsigned char* levels, long long* out, long n,
                               int U, void* stream);

/* ---- maps refined against the image: a windowed mean-field CRF (csrc/crf.hip; build-defined, the rule is in INTEGRATION.md section 5) ----
 * prob [N,H,W,C] fp32: a segmentor's output on the network grid, the K organ channels first.  image [N,H,W,1] fp32: the slices the network
 * saw, in [-1, 1] (finite).  out [N,H,W,K] fp32, every element written: the organ channels of Q^T.  L = K + 1 labels: the K organs and
 * "rest" = max(0, 1 - sum of the K organ channels), whatever C is.  u_l(p) = log(max(P_l(p), 1e-6)), Q^0 = softmax_l(u).  Iteration
 * t = 1 .. iterations, every pixel reading Q^(t-1) only, over the neighbours q = p + (dy, dx), |dy|, |dx| <= radius, q != p, q inside the
 * slice (pixels beyond it are skipped, not padded; slices never see each other):
 *   a(p,q) = exp(-|p-q|^2 / (2 theta_alpha^2) - (I_p - I_q)^2 / (2 theta_beta^2)),  s(p,q) = exp(-|p-q|^2 / (2 theta_gamma^2))
 *   m_l(p) = w_a * sum_q a Q_l(q) / sum_q a + w_s * sum_q s Q_l(q) / sum_q s,        Q^t(p) = softmax_l(u_l(p) + m_l(p))
 * Each kernel is normalised by its own sum over the neighbours that exist; a pixel without neighbours (a 1 x 1 slice) gets m = 0, and so
 * does the appearance term of a pixel whose fp32 appearance sum underflows to 0.  fp32 throughout, the window walked in ascending
 * (dy, dx); the appearance weight through the hardware exp2, the unary and the soft-max through logf / expf; the spatial factors from a
 * table built once per call.  A gather without atomics: two runs are bitwise equal, and the result of a slice does not depend on the
 * other slices of the call.  prob and image are only read.
 * 1 <= radius <= 8, 1 <= iterations <= 20, the three theta finite and > 0, w_a and w_s finite and >= 0 and not both 0, 1 <= K <= min(C, 16),
 * extents >= 1, prob, image and out below 2^31 bytes each; anything else, a null pointer, or out or ws overlapping another operand is
 * refused (hipErrorInvalidValue, nothing is launched).  N == 0 does nothing. */
/* bytes of ws for mmseg_crf_refine: the two tables and two planar Q buffers [N,K+1,H,W]; 0 for sizes that it would refuse */
long mmseg_crf_refine_workspace_bytes(int N, int H, int W, int K);
/* ws is the only scratch.  2 + iterations launches on the stream; no host synchronisation, allocation or copy. */
int mmseg_crf_refine(const float* prob, const float* image, float* out, void* ws, int N, int H, int W, int C, int K, int radius,
                     int iterations, float w_a, float theta_alpha, float theta_beta, float w_s, float theta_gamma, void* stream);

/* ---- bias-field (coil shading) correction of one MR volume (csrc/biasfield.hip; build-defined: the reference loads CHAOS as exported) ----
 * An N3 / N4-family rule: Sled's log-domain histogram sharpening in the form of N4's SharpenImage.  One deliberate departure: the
 * residual is smoothed by a masked, normalised Gaussian convolution in mm, not by a B-spline fit; the levels halve the Gaussian's width
 * where N4 doubles the spline mesh; nothing is shrunk.  Nearest-bin integer counts replace N4's two-bin split, so that integer atomics
 * give the same counts every run.  Iteration counts are fixed: no convergence test, nothing comes back to the host, two runs are bitwise
 * equal.  x [S,H,W] fp32 (finite), n = S * H * W < 2^31 - 1, S, H, W <= 65535.  B = 200 bins, P = 512, offset = (P - B) / 2, fwhm 0.15,
 * noise 0.01.  All arithmetic fp64, one rounding to fp32 at the end.
 *   mask       lo, hi = min, max of x.  256-bin histogram, bin min(floor((x - lo) * (256 / (hi - lo))), 255), integer counts n_j.  Over the
 *              cuts after bin t = 0 .. 254: w0 = sum_{j<=t} n_j, w1 = N - w0, s0 = sum_{j<=t} j n_j, s1 = sum_j j n_j - s0 (integers);
 *              var = (w0 * w1) * (d * d), d = s0 / w0 - s1 / w1, 0 when w0 or w1 is 0; the first maximum wins.  threshold =
 *              max(lo + ((t + 1) * (hi - lo)) / 256, 0); m = x > threshold; v0 = log(x) on the mask.  f = 0.
 *   level l    sigma_axis = sigma_mm / 2^l / d_axis voxels, radius R = int(4 sigma + 0.5), weights w_k = exp(-0.5 k^2 / sigma^2) / sum
 *              (scipy.ndimage's normalised kernel, made by the host).  G * y = the separable convolution along W, then H, then S (not S
 *              when the extent is 2d: Rs = 0), zero outside the volume, each pass w_0 y_0 + sum_k w_k (y_-k + y_+k), k ascending.
 *              den = G * m once per level.
 *   iteration  v = v0 - f on the mask; vmin, vmax over the mask; slope = (vmax - vmin) / (B - 1); c = (v - vmin) / slope;
 *              Hh[floor(c + 0.5)] += 1.  V = Hh at offset in a zero array of P; F[n] = (2 sqrt(ln 2 / pi) / w) exp(-(n'^2 4 ln 2) / w^2),
 *              w = fwhm / slope, n' = min(n, P - n); G = conj(F^) / (|F^|^2 + noise); U = max(Re ifft(V^ Re G), 0); b_j = vmin +
 *              (j - offset) slope; E = Re ifft(fft(U b) F^) / Re ifft(fft(U) F^), 0 where the denominator is 0, entries offset ..
 *              offset + B - 1 kept.  e = E[i] + (c - i) (E[i+1] - E[i]), i = min(floor(c), B - 2); r = v - e on the mask, 0 elsewhere;
 *              f += (G * r) / den where den > 0.  vmax == vmin (or an empty mask): this iteration and all later ones change nothing.
 *   output     x = fp32(fp64(x) * exp(-f)) at every voxel, in place.  A volume that is constant, whose mask is empty or whose masked
 *              values are all equal keeps its bits: no kernel writes it.
 * The sharpen runs in one block: five 512-point radix-2 Stockham transforms (U b + i U share one) over roots [512,2] fp64 = (cos, sin)
 * (2 pi q / 512) made by the host.  weights [3,129] fp64: rows for S, H, W, w_0 .. w_R each.  1 <= R <= 128 per smoothed axis (R may exceed
 * the extent of the axis; taps outside contribute nothing), Rs = 0 skips the pass along S; anything else, a null pointer or a shape outside
 * the limits is refused (hipErrorInvalidValue, nothing is launched).  Buffers are the caller's; no host synchronisation, allocation or
 * copy; integer atomics only. */
/* doubles of ws for the entry points below (the state, six fp64 volumes, the mask); 0 for a shape they refuse */
long mmseg_bias_workspace_doubles(int S, int H, int W);
/* the stages on their own.  otsu: out [4] fp64 = lo, hi, threshold, 1 when the volume is constant (ws: 512 doubles suffice) */
int mmseg_bias_otsu(const float* x, double* ws, double* out, int S, int H, int W, void* stream);
/* v [n] fp64, mask [n] uint8 -> hist [200] int32, range [2] fp64 = vmin, vmax over the mask (NaN when it is empty; ws: 512 doubles) */
int mmseg_bias_histogram(const double* v, const unsigned char* mask, double* ws, int* hist, double* range, long n, void* stream);
/* hist [200] int32, range [2] fp64 -> E [200] fp64 (zeros when range[1] <= range[0]; ws: 512 doubles) */
int mmseg_bias_sharpen(const int* hist, const double* range, const double* roots, double* ws, double* E, void* stream);
/* out [S,H,W] fp64 = G * in; tmp: 2 n doubles; out may be in, tmp may be neither */
int mmseg_bias_smooth(const double* in, double* out, double* tmp, const double* weights, int S, int H, int W, int Rs, int Rr, int Rc,
                      void* stream);
/* f [n] += num / den where den > 0 */
int mmseg_bias_update(double* f, const double* num, const double* den, long n, void* stream);
/* the correction: begin (mask, v0, f = 0), one call of level per level (den, then `iterations` iterations; 1 + 3 + 8 * iterations launches,
 * one pass fewer each time when Rs = 0), finish (x in place) -- all on one stream with the same ws. */
int mmseg_bias_begin(const float* x, double* ws, int S, int H, int W, void* stream);
int mmseg_bias_level(double* ws, const double* roots, const double* weights, int S, int H, int W, int Rs, int Rr, int Rc, int iterations,
                     void* stream);
int mmseg_bias_finish(float* x, const double* ws, int S, int H, int W, void* stream);
/* field [S,H,W] fp64 = f (zeros for a volume that keeps its bits); info [2] int32 = (frozen, iterations that updated f), or null */
int mmseg_bias_field(const double* ws, double* field, int* info, int S, int H, int W, void* stream);

/* ---- non-local means denoising of one MR volume (csrc/denoise.hip; build-defined: the reference loads CHAOS as exported) ----
 * The step that precedes bias correction in an MR chain (ANTs: DenoiseImage, then N4; dipy: nlmeans).  Buades' voxel-wise non-local means
 * with Manjon's / Wiest-Daessle's Rician correction.  Departures from the literature: patches are always in-plane (CHAOS slices lie 5 to
 * 9 mm apart against 1.4 to 1.9 mm in plane: a patch across slices compares different anatomy); voxel-wise, not block-wise; sigma = auto is
 * Immerkaer's estimate; 2 sigma^2 is subtracted from the patch distance inside the weight.
 * x [S,H,W] fp32 (finite) -> out [S,H,W] fp32, every element written; out must not overlap x; n = S * H * W < 2^31 - 1.
 * Parameters: search_radius Rs in 1..10, patch_radius Rp in 1..3, search_radius_z Rz in 0..4 (0: every slice on its own, "2d"; > 0: the
 * search, never the patch, also reaches the same in-plane window of the Rz slices before and after, "3d" / 2.5-D), h finite > 0 (the
 * smoothing strength in units of sigma), rician 1 | 0 (0: Gaussian noise), sigma in the volume's grey values.
 *   per voxel p   walk the offsets t = (dz, dy, dx), |dz| <= Rz, |dy| <= Rs, |dx| <= Rs, t != 0, in ascending (dz, dy, dx) order.  A
 *                 neighbour q = p + t outside the volume is skipped, not padded.  With T = (2 Rp + 1)^2:
 *                     d2(p, q) = (1 / T) sum_{|a|, |b| <= Rp} (u(p + (0, a, b)) - u(q + (0, a, b)))^2,    a, then b, ascending,
 *                 the patch coordinates clamped to the slice (edge replicate) on both sides;
 *                     w(p, q) = exp2(max(d2 - 2 sigma^2, 0) * c),    c = -log2(e) / (h sigma)^2    (the hardware exp2),
 *                 and 0 where the argument of exp2 is below -126: no weight is a denormal number.
 *                 sw = sum w, sv = sum w v(q), with v = u (Gaussian) or u^2 (Rician), added in the walk order.  The centre comes last with
 *                 w(p, p) = the largest of the other weights (Buades' and dipy's convention; 0 without a neighbour).
 *   output        sw = 0 (no neighbour, or every weight underflowed): out = u(p).  Else m = sv / sw; Gaussian: out = m; Rician
 *                 (Wiest-Daessle 2008): out = sqrt(max(m - 2 sigma^2, 0)).
 *   arithmetic    all fp32 (sigma is rounded to fp32 once); a gather without atomics: two runs are bitwise equal, and with Rz = 0 a slice's
 *                 result does not depend on the other slices of the call.
 *   sigma         Immerkaer's estimator, always in-plane: sigma = sqrt(pi / 2) / (6 S (H - 2) (W - 2)) sum |L * x| over the interior
 *                 pixels of every slice, L = [[1, -2, 1], [-2, 4, -2], [1, -2, 1]], each term and the sum in fp64 in an order fixed by the
 *                 shape (two runs are bitwise equal); H < 3 or W < 3 gives 0.  The estimator reads anatomy edges as noise: it runs high on
 *                 small or busy slices, and a sigma measured in a background region is better where the user has one.
 *   keeps its bits  a volume whose sigma, given or estimated, is <= 0 or not finite (a constant volume under `auto` is one), or so small or
 *                 large that 2 sigma^2, (h sigma)^2 or c leaves the positive finite fp32 numbers: out is a copy of x.
 * Anything outside the limits, a null pointer, out overlapping x or n >= 2^31 - 1 is refused (hipErrorInvalidValue, nothing is launched);
 * S = 0 does nothing.  No host synchronisation, allocation or copy; sigma never returns to the host.  Launches: mmseg_nlm_sigma 2 (partial
 * sums per block, then one block that adds them; no block waits for another), mmseg_nlm_denoise 1.  A block owns a tile of 8 rows x 32
 * columns of one slice. */
/* bytes of ws for mmseg_nlm_sigma (the partial sums; 8-byte aligned); 0 for a shape it refuses */
long mmseg_nlm_workspace_bytes(int S, int H, int W);
/* sigma_out [1] fp64 on the device */
int mmseg_nlm_sigma(const float* x, double* ws, double* sigma_out, int S, int H, int W, void* stream);
/* sigma_dev: one fp64 on the device (what mmseg_nlm_sigma wrote), or null: then `sigma` is used.  Both ways give the same bits for the
 * same number. */
int mmseg_nlm_denoise(const float* x, float* out, const double* sigma_dev, double sigma, int S, int H, int W, int search_radius,
                      int patch_radius, int search_radius_z, float h, int rician, void* stream);

/* ---- alignment of a volume's modalities by mutual information (csrc/align.hip; build-defined: the reference pairs CHAOS slices by hand) ----
 * Translation only: an integer slice shift dz and an integer in-plane shift (dy, dx) in pixels of the resampled frames, of a moving
 * volume B against a reference volume A.  Scale is the loader's resampling; rotation and deformation stay with the model.
 * O = (OH, OW) is the network's input extent, R_x = (RH_x, RW_x) the resampled extent of volume x, c(R) = centre_start(R, O) per axis:
 * (R - O + 1) / 2 (floor) for R > O, else -((O - R) / 2) (floor).
 *   1 quantise   q_x [S,RH,RW] uint8 on the resampled grid: v = the bilinear value of mmseg_preprocess_image (same coordinates, same fp32
 *                expression order, outside -> 0); lo, hi = two order statistics of the volume (mmseg_preprocess_quantiles, per volume;
 *                knots [2] fp32 on the device).  q = 0 for v <= lo; bins - 1 for v >= hi; else min(bins - 1, (int)floorf((v - lo) *
 *                ((float)bins / (hi - lo)))) in fp32 without contraction.  hi == lo: all 0.  2 <= bins <= 64.
 *   2 pairing    candidate (dz, dy, dx): reference slice i pairs with moving slice i + dz; window coordinate (oy, ox) reads A at
 *                (oy + c_a, ox + c_a) and B at (oy + c_b + dy, ox + c_b + dx) (per axis), so the zero shift is the loader's centre
 *                pairing.  Only pairs with both indices inside their frames count: nothing is padded, o is not limited to [0, O), the
 *                whole overlap of the frames is used.  At stride t only o with o mod t == 0 on both axes is sampled (floor-mod: o may be
 *                negative).  A byte >= bins counts as bins - 1.
 *   3 score      h [bins,bins] uint32 = the joint histogram of the sampled pairs (row: A's bin), N = sum h.  With p = count / N in fp64 and
 *                H = sum of -(p * log(p)) over the non-empty bins (natural log) of h, of its row sums and of its column sums: score =
 *                (H(A) + H(B)) / H(A,B), Studholme's normalised mutual information, in fp64.  Summation order: thread k of 256 adds
 *                the terms k, k + 256, ... in ascending order, the 256 sums are halved pairwise (k += k + 128, k + 64, ... 1).  Score =
 *                -1 where N == 0 or H(A,B) == 0, and where the candidate is not admissible: n_full(c) >= min_overlap * n_full(0) in
 *                fp64, n_full = the stride-1 pair count = the product of the three overlap lengths (closed form), 0 <= min_overlap <= 1.
 *   4 search     a stage scores C candidates at stride t.  mode 0: cand [C,3] int32 on the device (a test's list; no probe).  mode 1, the
 *                lattice: dz in [-Z, Z], dy in t * [-floor(Py / t), floor(Py / t)], dx likewise, index ((dz + Z) * ny + iy) * nx + ix.
 *                mode 2, refinement: centre + (jz - 1, (jy - 1) t, (jx - 1) t), index (jz * 3 + jy) * 3 + jx, centre = state[0..2]; a
 *                candidate outside [-Z, Z] x [-Py, Py] x [-Px, Px] is skipped (score -1, never selected).  In modes 1 and 2 the last
 *                candidate, C - 1, is the zero-shift PROBE (0, 0, 0): scored like any other, never selected; its score is reported.
 *                Best = the highest score; ties go to the smaller dz^2, then the smaller dy^2 + dx^2, then the lexicographically smaller
 *                (dz, dy, dx).  If the best score is < 0 (nothing admissible) the shift is (0, 0, 0).
 *   5 state      state [8] fp64 on the device, zeroed by the caller before the first stage: [0..2] (dz, dy, dx) of the stage's best, the
 *                centre the next refinement stage reads; [3] its score; [4] the probe's score (mode 0: unchanged); [5] its N (the probe's
 *                where nothing was admissible); [6] 1 where a candidate was admissible; [7] the stages run.  A search of L levels is the
 *                lattice at t = 2^(L-1), then refinement at t = 2^(L-2) .. 1, each stage three launches (histograms, scores, select); the
 *                host reads `state` once, after the last.  Integer atomics and fixed-order fp64 only: two runs are bitwise equal.
 * Limits: S * RH * RW < 2^31 - 1 per volume, 1 <= C <= 65535, 1 <= t <= 65536, |shift| <= 2^20.  Outside them, or with a null pointer, a call
 * is refused (hipErrorInvalidValue, nothing is launched).  No host synchronisation, allocation or copy.
 * The candidates of a stage in mode 1 or 2, the probe included; 0 where the kernels refuse the stage */
long mmseg_align_stage_candidates(int mode, int stride, int Z, int Py, int Px);
/* bytes of h [C,bins,bins] uint32 followed (8-byte aligned) by scores [C,2] fp64 of one stage; 0 outside the limits */
long mmseg_align_workspace_bytes(int C, int bins);
/* img [S,H,W] fp32 raw slices, knots [2] fp32 (lo, hi) on the device -> q [S,RH,RW] uint8 */
int mmseg_align_quantise(const float* img, const float* knots, unsigned char* q, int S, int H, int W, int RH, int RW, int bins,
                         void* stream);
/* h [C,bins,bins] (uint32 counts in int32 storage), zeroed here on the stream.  A block counts in LDS (LDS atomics) and merges its
 * non-empty bins with integer atomics.  aggregate 1: the lanes of a wave that meet the bin of its first active lane are added by one
 * atomic (the air of an MR frame); 0: one LDS atomic per pair.  The counts are the same.  cand: mode 0 only; state: mode 2 only. */
int mmseg_align_histograms(const unsigned char* qa, const unsigned char* qb, const int* cand, const double* state, int* h, int Sa,
                           int RHa, int RWa, int Sb, int RHb, int RWb, int OH, int OW, int mode, int stride, int Z, int Py, int Px, int C,
                           int bins, int aggregate, void* stream);
/* scores [C,2] fp64 = (score, N) of every candidate's table in h */
int mmseg_align_scores(const int* h, const int* cand, const double* state, double* scores, int Sa, int RHa, int RWa, int Sb, int RHb,
                       int RWb, int OH, int OW, int mode, int stride, int Z, int Py, int Px, int C, int bins, double min_overlap,
                       void* stream);
/* the stage's best under the tie rule -> state (item 5) */
int mmseg_align_select(const double* scores, const int* cand, double* state, int mode, int stride, int Z, int Py, int Px, int C,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMSEG_HIP_H */
