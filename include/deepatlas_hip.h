/*
 * deepatlas_hip.h -- C ABI of libdeepatlas_hip.so, the MI355X (gfx950) native hot path for
 * uncbiag/DeepAtlas' 3D volumetric training step.
 *
 * The reference has no FFI layer: its hot path is Python (L2) calling PyTorch ATen ops (L1)
 * (SURVEY.md §1, §8b).  This header is the seam a maintainer would bind instead of those ATen
 * calls; each entry cites the reference call site(s) it replaces (file:line in uncbiag/DeepAtlas).
 *
 * Conventions
 *   - every activation tensor is fp32, channels-last 3D ("NDHWC"): [N][D][H][W][C], dense.
 *     (torch side: a N x C x D x H x W tensor with torch.channels_last_3d strides.)
 *   - raw device pointers, explicit dims, no hidden allocation: scratch memory is passed in as
 *     (ws, ws_bytes); da_*_ws_bytes() returns the size a call needs.  A call only checks ws_bytes
 *     against that size (DA_ERR_WS_SMALL): where it places things inside ws depends on the shape
 *     alone, never on how much more the caller passed.
 *   - `stream` is a hipStream_t (NULL = default stream).  Calls only enqueue work.
 *   - return value: 0 on success, otherwise a hipError_t, or DA_ERR_* (negative) for bad arguments.
 *   - 3x3x3 conv weights use the "TIO" layout [27 taps (kd,kh,kw)][Cin][Cout]; 2x2x2 transposed-conv
 *     weights [8 taps][Cin][Cout]; 1x1x1 weights [Cin][Cout].  da_w_* convert from/to the PyTorch
 *     state_dict layouts ([Cout][Cin][k][k][k], ConvTranspose [Cin][Cout][k][k][k]).
 */
#ifndef DEEPATLAS_HIP_H
#define DEEPATLAS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DA_ERR_BADARG   (-1)
#define DA_ERR_WS_SMALL (-2)
#define DA_ERR_UNSUPPORTED (-3)

/* library / device info */
int  da_version(void);
int  da_device_info(int* cu_count, int* wave_size, size_t* hbm_bytes, char* arch, int arch_len);

/* ---- weight layout transforms (tiny) -------------------------------------------------------- */
/* [Cout][Cin][k^3] (nn.Conv3d, unets.py:30,36,250; modules.py:48; voxel_morph.py:57) <-> [k^3][Cin][Cout] */
int da_w_oik_to_tio(const float* w_oik, float* w_tio, int Cout, int Cin, int K3, void* stream);
int da_w_tio_to_oik(const float* w_tio, float* w_oik, int Cout, int Cin, int K3, void* stream);
/* [Cin][Cout][k^3] (nn.ConvTranspose3d, unets.py:49,55) <-> [k^3][Cin][Cout] */
int da_w_iok_to_tio(const float* w_iok, float* w_tio, int Cin, int Cout, int K3, void* stream);
int da_w_tio_to_iok(const float* w_tio, float* w_iok, int Cin, int Cout, int K3, void* stream);
/* ConvTranspose3d(k=3, s=1, p=1) weights [Cin][Cout][27] (unets.py:88-96 `UNet.decoder`): the same op as a 3x3x3 convolution with
 * flipped taps, so it runs on the da_conv3d_k3_* entries after this re-layout. */
int da_w_iok_flip_to_tio(const float* w_iok, float* w_tio, int Cin, int Cout, int K3, void* stream);
int da_w_tio_to_iok_flip(const float* w_tio, float* w_iok, int Cin, int Cout, int K3, void* stream);
/* the three gradient conversions, accumulating: dst += layout(w_tio) (dst: the parameter's .grad inside the optimiser's flat bucket) */
int da_w_tio_to_oik_acc(const float* w_tio, float* w_oik, int Cout, int Cin, int K3, void* stream);
int da_w_tio_to_iok_acc(const float* w_tio, float* w_iok, int Cin, int Cout, int K3, void* stream);
int da_w_tio_to_iok_flip_acc(const float* w_tio, float* w_iok, int Cin, int Cout, int K3, void* stream);

/* ---- 3x3x3 convolution, padding 1, stride 1|2 (rows a1, a7, a9) ----------------------------- */
/* replaces nn.Conv3d(k=3,p=1) forward: unets.py:30,36; modules.py:48,56; voxel_morph.py:57,82.
 * Input = channel-concat(in1[C1], in2[C2]) without materialising it (torch.cat at unets.py:275,
 * voxel_morph.py:65,74,76,78,82); in2 may be NULL with C2 = 0.
 * out[N][Do][Ho][Wo][Cout], Do = (D-1)/stride+1.  bias may be NULL.
 * act_slope < 0: no activation; == 0: ReLU (modules.py:58); > 0: LeakyReLU(slope) fused in the epilogue.
 * stats (optional, may be NULL): per-channel double [2][Cout] (sum, sum of squares) of the PRE-activation
 * output, ACCUMULATED into by the kernel's epilogue is not done here; see da_bn_stats. */
size_t da_conv3d_k3_ws_bytes(int N, int D, int H, int W, int Cin, int Cout, int stride);
int da_conv3d_k3_fwd(const float* in1, int C1, const float* in2, int C2,
                     const float* w_tio, const float* bias, float* out,
                     int N, int D, int H, int W, int Cout, int stride, float act_slope,
                     void* ws, size_t ws_bytes, void* stream);
/* Forward of a conv that feeds a train-mode BatchNorm: same as da_conv3d_k3_fwd (no activation) and, when the MFMA path
 * serves the layer, the epilogue also writes per-workgroup partial sums stats_partial[nparts][2][Cout] (double: sum, sum of
 * squares of the output) so the BN statistics need no extra pass over the tensor.  *stats_nparts = 0 means "not fused":
 * run da_bn_train_stats.  stats_capacity = number of [2][Cout] slots available (>= 512). */
int da_conv3d_k3_fwd_bnstats(const float* in1, int C1, const float* in2, int C2,
                             const float* w_tio, const float* bias, float* out,
                             int N, int D, int H, int W, int Cout, int stride,
                             double* stats_partial, int stats_capacity, int* stats_nparts,
                             void* ws, size_t ws_bytes, void* stream);
/* data gradient (autograd of the above): dx = concat(dx1[C1], dx2[C2]); D,H,W are the INPUT dims. */
int da_conv3d_k3_dgrad(const float* dy, const float* w_tio, float* dx1, int C1, float* dx2, int C2,
                       int N, int D, int H, int W, int Cout, int stride,
                       void* ws, size_t ws_bytes, void* stream);
/* weight / bias gradient: dw_tio[27][C1+C2][Cout], dbias[Cout] (may be NULL). */
int da_conv3d_k3_wgrad(const float* in1, int C1, const float* in2, int C2, const float* dy,
                       float* dw_tio, float* dbias,
                       int N, int D, int H, int W, int Cout, int stride,
                       void* ws, size_t ws_bytes, void* stream);

/* Forward / weight gradient of the same convolution with an INPUT PROLOGUE (the reference's Conv3d -> BatchNorm3d -> LeakyReLU
 * -> Conv3d chains, unets.py:24-39, 259-278): in1 / in2 may be the RAW output of the producing convolution; its BatchNorm
 * scale[C] / shift[C] (da_bn_train_stats* / da_bn_eval_affine) and activation slope are applied while the tile is staged, with
 * the arithmetic of da_bn_act_fwd (bit-identical to materialising the activated tensor).  proN_scale == NULL: input N is an
 * ordinary tensor.  stats_* as in da_conv3d_k3_fwd_bnstats (NULL / capacity < 512: no statistics, act_slope is applied).
 * Stride 1 on the matrix cores only: DA_ERR_UNSUPPORTED tells the caller to apply da_bn_act_fwd and use the plain entries. */
int da_conv3d_k3_fwd_pro(const float* in1, int C1, const float* pro1_scale, const float* pro1_shift, float pro1_slope,
                         const float* in2, int C2, const float* pro2_scale, const float* pro2_shift, float pro2_slope,
                         const float* w_tio, const float* bias, float* out,
                         int N, int D, int H, int W, int Cout, float act_slope,
                         double* stats_partial, int stats_capacity, int* stats_nparts,
                         void* ws, size_t ws_bytes, void* stream);
int da_conv3d_k3_wgrad_pro(const float* in1, int C1, const float* pro1_scale, const float* pro1_shift, float pro1_slope,
                           const float* in2, int C2, const float* pro2_scale, const float* pro2_shift, float pro2_slope,
                           const float* dy, float* dw_tio,
                           int N, int D, int H, int W, int Cout,
                           void* ws, size_t ws_bytes, void* stream);

/* ---- nearest x2 up-sampling folded into the 3x3x3 convolution that consumes it (row a8 + a7; voxel_morph.py:72-80: `F.interpolate(x,
 * size=skip.shape)` -- default mode 'nearest' -- then modules.convBlock, modules.py:48,56-58).  s1 / s2: the one or two COARSE source
 * tensors [N][Dc][Hc][Wc][C1|C2] (s2 / C2 = NULL / 0 for a single input; the reference concatenates, voxel_morph.py:73,75); out and dy
 * live on the fine grid [N][2Dc][2Hc][2Wc][Cout]; w_tio / dw_tio [27][C1+C2][Cout] as for da_conv3d_k3_*.  Exact x2 only (callers use
 * da_upsample_nearest_* + da_conv3d_k3_* otherwise), split matrix mode only (da_upconv3d_k3_supported returns 0 otherwise; the entry
 * points then return DA_ERR_UNSUPPORTED).  Per output parity the layer is a 2x2x2-tap convolution on the coarse grid with summed weights
 * (conv3d_up2.hip): neither the up-sampled tensor nor its gradient is materialised. */
int da_upconv3d_k3_supported(int C1, int C2, int Cout);
size_t da_upconv3d_k3_ws_bytes(int N, int Dc, int Hc, int Wc, int Cin, int Cout);
int da_upconv3d_k3_fwd(const float* s1, int C1, const float* s2, int C2, const float* w_tio, const float* bias, float* out,
                       int N, int Dc, int Hc, int Wc, int Cout, float act_slope, void* ws, size_t ws_bytes, void* stream);
int da_upconv3d_k3_dgrad(const float* dy, const float* w_tio, float* dx1, int C1, float* dx2, int C2,
                         int N, int Dc, int Hc, int Wc, int Cout, void* ws, size_t ws_bytes, void* stream);
int da_upconv3d_k3_wgrad(const float* s1, int C1, const float* s2, int C2, const float* dy, float* dw_tio,
                         int N, int Dc, int Hc, int Wc, int Cout, void* ws, size_t ws_bytes, void* stream);

/* test/diagnostic knob: force the direct (VALU) kernels instead of the MFMA implicit-GEMM path; returns the previous setting.
 * Used by the GPU tests to A/B the two implementations. */
int da_set_conv_direct(int on);

/* bf16 matrix mode (BASELINE config 5; the reference itself is fp32-only, train_seg.py has no autocast): when on, the 3x3x3
 * convolutions (forward, data gradient, weight gradient) round their operands to bf16 while staging them and run on
 * v_mfma_f32_16x16x16_bf16 with fp32 accumulation; tensors in HBM, BatchNorm, losses and the optimiser stay fp32.
 * Off by default (exact fp32 v_mfma_f32_16x16x4_f32); returns the previous setting. */
int da_set_matrix_bf16(int on);
/* Matrix mode of the 3x3x3 convolutions (forward, data gradient, weight gradient); returns the previous mode, -1 for an unknown one.
 *   0  fp32 operands on v_mfma_f32_16x16x4_f32 -- one fmaf per product, the arithmetic of the reference's nn.Conv3d on the CPU
 *      (lib/network_factory/modules.py:48);
 *   1  = da_set_matrix_bf16(1): operands ROUNDED to bf16 (not fp32-accurate);
 *   2  "split": every staged tile is scaled by a power of two (its largest magnitude into [2^14, 2^15)) and every fp32 operand split into
 *      two fp16 terms (x s = h + l to 2^-22 |x s|); a product is formed from three of the four partial products (h l', l h', h h') on
 *      v_mfma_f32_16x16x32_f16 with fp32 accumulation, the accumulators rescaled by exact powers of two between tiles.  Per product the
 *      error bound is 2^-21 + 2^-22 |x y| (typically one fp32 rounding); over the sums of a convolution the result is closer to double
 *      than mode 0's fmaf chain (tests/test_gpu_split.py), at 3/16 of the matrix-pipe time.  Tensors in HBM stay fp32
 *      (deepatlas_amd/csrc/split_f16.h). */
int da_set_matrix_mode(int mode);

/* ---- 1x1x1 convolution (segmentation head, row a5; unets.py:249-250) ------------------------- */
/* scratch for the packed weights of the 1x1 / transposed-conv forward and data-gradient launchers */
size_t da_pointwise_ws_bytes(int ntaps, int Cin, int Cout);
int da_conv1x1_fwd(const float* in, const float* w_io, const float* bias, float* out,
                   long long M, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
/* Head with an INPUT PROLOGUE (see da_conv3d_k3_fwd_pro): `in` is the raw output of the last decoder convolution and
 * act(in * pro_scale + pro_shift) is what the 1x1x1 convolution consumes; same arithmetic as da_bn_act_fwd followed by the plain
 * entries.  Channel counts in multiples of 16 (matrix-core kernels), else DA_ERR_UNSUPPORTED. */
int da_conv1x1_fwd_pro(const float* in, const float* pro_scale, const float* pro_shift, float pro_slope,
                       const float* w_io, const float* bias, float* out,
                       long long M, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int da_conv1x1_wgrad_pro(const float* in, const float* pro_scale, const float* pro_shift, float pro_slope,
                         const float* dy, float* dw_io, float* dbias,
                         long long M, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int da_conv1x1_dgrad(const float* dy, const float* w_io, float* dx, long long M, int Cin, int Cout,
                     void* ws, size_t ws_bytes, void* stream);
/* dW [Cin][Cout] (+ optional dbias).  Channel counts in multiples of 16 run on the matrix cores at any width; every other shape on the direct kernel, which
 * covers Cin * Cout <= 4096 -- beyond that DA_ERR_UNSUPPORTED (never a partly written dW). */
size_t da_conv1x1_wgrad_ws_bytes(long long M, int Cin, int Cout);
int da_conv1x1_wgrad(const float* in, const float* dy, float* dw_io, float* dbias,
                     long long M, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);

/* ---- 2x2x2 stride-2 transposed convolution (row a3; unets.py:49,55,240-241) ------------------ */
/* out[N][2D][2H][2W][Cout] = bias + sum_ci in[N][D][H][W][ci] * w_tio[tap(i,j,k)][ci][co] */
int da_deconv_k2s2_fwd(const float* in, const float* w_tio, const float* bias, float* out,
                       int N, int D, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
/* Same, with the BatchNorm3d partial sums of the output accumulated in the epilogue (unets.py:49-51: ConvTranspose3d ->
 * BatchNorm3d): stats_partial[stats_nparts][2][Cout] doubles for da_bn_train_stats_from_partials; needs
 * stats_capacity >= ceil(N*D*H*W / 256).  *stats_nparts == 0 on return: no statistics were produced (shape / capacity), run
 * da_bn_train_stats over the output instead. */
int da_deconv_k2s2_fwd_bnstats(const float* in, const float* w_tio, const float* bias, float* out,
                               int N, int D, int H, int W, int Cin, int Cout,
                               double* stats_partial, int stats_capacity, int* stats_nparts,
                               void* ws, size_t ws_bytes, void* stream);
int da_deconv_k2s2_dgrad(const float* dy, const float* w_tio, float* dx,
                         int N, int D, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
/* Fused backward of the up-sampler block ConvTranspose3d(k2, s2) -> BatchNorm3d(train) -> LeakyReLU/ReLU (autograd of unets.py:49-52).  gout = gradient
 * with respect to the ACTIVATED output, y = the raw transposed-conv output, both [N][2D][2H][2W][Cout]; mean / rstd / scale / shift = the block's statistics
 * rows; in = the block's input [N][D][H][W][Cin].  One pass over (gout, y) after the sums (one reduction pass, or `pre`[pre_n][2][Cout] = sums accumulated by
 * the producer of gout as for da_bn_act_bwd_dbias_pre): dx [N][D][H][W][Cin], dw_tio [8][Cin][Cout], dbias[Cout] (may be NULL), dgamma[Cout], dbeta[Cout].
 * The tensor dy = d loss / d y is never written.  DA_ERR_UNSUPPORTED unless Cin = Cout = 32 (callers fall back to da_bn_act_bwd_dbias +
 * da_deconv_k2s2_dgrad + da_deconv_k2s2_wgrad). */
size_t da_deconv_k2s2_bn_bwd_ws_bytes(int N, int D, int H, int W, int Cin, int Cout);
int da_deconv_k2s2_bn_bwd(const float* gout, const float* y, const float* mean, const float* rstd, const float* scale, const float* shift, float act_slope,
                          const float* in, const float* w_tio, float* dx, float* dw_tio, float* dbias, float* dgamma, float* dbeta,
                          int N, int D, int H, int W, int Cin, int Cout, const double* pre, int pre_n,
                          void* ws, size_t ws_bytes, void* stream);
size_t da_deconv_k2s2_wgrad_ws_bytes(int N, int D, int H, int W, int Cin, int Cout);
int da_deconv_k2s2_wgrad(const float* in, const float* dy, float* dw_tio, float* dbias,
                         int N, int D, int H, int W, int Cin, int Cout,
                         void* ws, size_t ws_bytes, void* stream);

/* ---- BatchNorm3d + LeakyReLU (rows a1, a3; unets.py:31,51 + :5-6) ---------------------------- */
/* Train-mode statistics over M = N*D*H*W rows of x[M][C]: writes mean[C], rstd[C] (1/sqrt(biased var+eps)),
 * scale[C] = gamma*rstd, shift[C] = beta - mean*scale, and updates running_mean/var in place with
 * `momentum` and the UNBIASED variance (nn.BatchNorm3d semantics).  running_* may be NULL. */
size_t da_bn_ws_bytes(long long M, int C);
int da_bn_train_stats(const float* x, long long M, int C, const float* gamma, const float* beta,
                      float eps, float momentum, float* running_mean, float* running_var,
                      float* mean, float* rstd, float* scale, float* shift,
                      void* ws, size_t ws_bytes, void* stream);
/* Same result from partial sums produced by da_conv3d_k3_fwd_bnstats. */
int da_bn_train_stats_from_partials(const double* partial, int nparts, long long M, int C,
                                    const float* gamma, const float* beta, float eps, float momentum,
                                    float* running_mean, float* running_var,
                                    float* mean, float* rstd, float* scale, float* shift, void* stream);
/* Eval-mode affine from running statistics. */
int da_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                      float eps, int C, float* mean, float* rstd, float* scale, float* shift, void* stream);
/* y = act(x*scale + shift); act_slope as in da_conv3d_k3_fwd. */
int da_bn_act_fwd(const float* x, const float* scale, const float* shift, float act_slope, float* y,
                  long long M, int C, void* stream);
/* Backward of act(BN_train(x)): given dy (grad wrt y) and the saved x, mean, rstd, gamma, scale, shift:
 * dx[M][C], dgamma[C], dbeta[C].  train != 0: full batch-statistics backward; train == 0: dx = dz*scale. */
int da_bn_act_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                  const float* scale, const float* shift, float act_slope, int train,
                  float* dx, float* dgamma, float* dbeta, long long M, int C,
                  void* ws, size_t ws_bytes, void* stream);
/* Same, additionally writing dxsum[C] = per-channel column sums of dx: the bias gradient of the convolution (or transposed
 * convolution) that produced x, fused into the apply pass so the conv weight-gradient call can skip its own pass over dy. */
int da_bn_act_bwd_dbias(const float* dy, const float* x, const float* mean, const float* rstd,
                        const float* scale, const float* shift, float act_slope, int train,
                        float* dx, float* dgamma, float* dbeta, float* dxsum, long long M, int C,
                        void* ws, size_t ws_bytes, void* stream);
/* da_bn_act_bwd_dbias without its reduction pass over (dy, x): the two sums come from the kernel that PRODUCED dy, which accumulated them in its
 * epilogue -- pre[pre_n][2][C] doubles = (sum dz, sum dz (x - mean)) per workgroup, dz = dy act'(x scale + shift) (da_head_dice_bwd_bst).
 * train only.  autograd of nn.BatchNorm3d + nn.LeakyReLU (unets.py:31-32). */
int da_bn_act_bwd_dbias_pre(const float* dy, const float* x, const float* mean, const float* rstd,
                            const float* scale, const float* shift, float act_slope, int train,
                            float* dx, float* dgamma, float* dbeta, float* dxsum, long long M, int C,
                            const double* pre, int pre_n, void* ws, size_t ws_bytes, void* stream);
/* Backward of a bare activation from its OUTPUT y (ReLU / LeakyReLU): dx = dy * (y > 0 ? 1 : slope). */
int da_act_bwd(const float* dy, const float* y, float act_slope, float* dx, long long numel, void* stream);
/* Per-channel column sum of x[M][C] -> out[C] (bias gradients). */
/* backward of a conv block without BatchNorm (modules.py:56-58 conv -> act): dx = (g1 [+ g2]) * act'(y) and dbias = column sums of dx
 * in ONE pass.  g2 (may be NULL): second incoming gradient of a block whose output has two consumers (skip connection); y: the
 * block's ACTIVATED output (unused when act_slope < 0); dbias may be NULL; ws as da_bn_ws_bytes(M, C). */
int da_act_bwd_add_dbias(const float* g1, const float* g2, const float* y, float act_slope, float* dx, float* dbias,
                         long long M, int C, void* ws, size_t ws_bytes, void* stream);
int da_colsum(const float* x, long long M, int C, float* out, void* ws, size_t ws_bytes, void* stream);
/* da_act_bwd_add_dbias in two halves (same call site, modules.py:56-58): the big pass leaves its per-block double partial sums in the
 * caller-owned `partial` (da_bn_ws_bytes(M, C) bytes; *nparts = number of partial sets written), and da_colsum_finish reduces them to
 * out[C] (accumulate != 0: out[c] += sum) -- possibly on another stream, once the first call has completed there. */
int da_act_bwd_add_partial(const float* g1, const float* g2, const float* y, float act_slope, float* dx,
                           long long M, int C, void* partial, size_t partial_bytes, int* nparts, void* stream);
int da_colsum_finish(const void* partial, int nparts, int C, float* out, int accumulate, void* stream);

/* ---- MaxPool3d(2) (row a2; unets.py:230,267) ------------------------------------------------- */
int da_maxpool2_fwd(const float* x, float* y, int N, int D, int H, int W, int C, void* stream);
/* MaxPool3d(2) of a tensor whose BatchNorm + activation is still pending (see da_conv3d_k3_fwd_pro): one pass writes the activated
 * tensor `act` (the skip connection of unets.py:266-267) and its pooled version `y`; arithmetic of da_bn_act_fwd + da_maxpool2_fwd.
 * Even D, H, W and C % 4 == 0, else DA_ERR_UNSUPPORTED. */
int da_maxpool2_fwd_pro(const float* x, const float* pro_scale, const float* pro_shift, float pro_slope, float* act, float* y,
                        int N, int D, int H, int W, int C, void* stream);
/* dx (input-sized) from dy and the saved input x; gradient goes to the first maximum in (d,h,w) scan order. */
int da_maxpool2_bwd(const float* dy, const float* x, float* dx, int N, int D, int H, int W, int C, void* stream);
/* dx = gskip + maxpool_bwd(dy): the pooled tensor also feeds a skip connection (unets.py:266-267,275) */
int da_maxpool2_bwd_add(const float* dy, const float* x, const float* gskip, float* dx, int N, int D, int H, int W, int C, void* stream);
/* The same (gskip may be NULL) on the RAW tensor da_maxpool2_fwd_pro pooled, whose BatchNorm + activation was applied on the fly: x_raw = the producer's raw
 * conv output, stats4 = its statistics rows [mean | rstd | scale | shift][C], slope its activation.  The arg-max is that of the activated values (formed again
 * with the forward's expression); besides dx the kernel accumulates the PRODUCER's BatchNorm-backward sums, bst[*bst_n][2][C] doubles =
 * (sum dz, sum dz (x - mean)), dz = dx act'(x scale + shift), for da_bn_act_bwd_dbias_pre.  Even D, H, W, C / 4 a power of two, bst_cap >= 1024; else
 * DA_ERR_UNSUPPORTED.  autograd of nn.MaxPool3d(2) + the skip connection behind conv -> BatchNorm -> LeakyReLU (unets.py:30-37, 266-267). */
int da_maxpool2_bwd_bst(const float* dy, const float* x_raw, const float* gskip, float* dx, int N, int D, int H, int W, int C,
                        const float* stats4, float slope, double* bst, int bst_cap, int* bst_n, void* stream);

/* ---- nearest-neighbour up-sampling to a given size (row a8; voxel_morph.py:72,74,76,80) ------ */
int da_upsample_nearest_fwd(const float* x, float* y, int N, int D, int H, int W, int C,
                            int Do, int Ho, int Wo, void* stream);
int da_upsample_nearest_bwd(const float* dy, float* dx, int N, int D, int H, int W, int C,
                            int Do, int Ho, int Wo, void* stream);

/* ---- deformation-field trilinear warp (rows a9-a10; voxel_morph.py:85-91, lib/utils.py:89-102) */
/* deform = disp + identity (identity generated in-kernel, channel order (x,y,z) = (W,H,D) axis, normalised
 * to [-1,1]); out = grid_sample(src, deform, bilinear, zeros, align_corners=True).
 * src[N][D][H][W][C], disp[N][D][H][W][3], deform (may be NULL) [N][D][H][W][3], out[N][D][H][W][C]. */
int da_warp_fwd(const float* src, const float* disp, float* deform, float* out,
                int N, int D, int H, int W, int C, void* stream);
/* gradients: d_disp[N][D][H][W][3] (may be NULL) and d_src (may be NULL; must be ZERO-FILLED by the caller,
 * accumulated with float atomics). */
int da_warp_bwd(const float* dout, const float* src, const float* disp, float* d_disp, float* d_src,
                int N, int D, int H, int W, int C, void* stream);
/* lib/utils.py:78-102 get_identity_transform(_batch): out[3][D][H][W] (reference layout, channel-first) */
/* warp of one-hot(labels) without materialising the one-hot tensor (joint step): out [N][D][H][W][C];
 * labels uint8 (1) / int64 (8) [N][D][H][W]; backward w.r.t. the displacement only (labels carry no gradient). */
int da_warp_labels_fwd(const void* labels, int label_bytes, const float* disp, float* out,
                       int N, int D, int H, int W, int C, void* stream);
int da_warp_labels_bwd(const float* dout, const void* labels, int label_bytes, const float* disp, float* d_disp,
                       int N, int D, int H, int W, int C, void* stream);
int da_identity_grid(float* out, int D, int H, int W, int normalize, void* stream);
/* ---- fused anatomy losses of the joint step (parts: lib/loss.py:410-476 Dice, voxel_morph.py:90-91 warp) ------
 * Dice's input gradient is g[v][c] = coef[0][n][c] [St[v] == c] + coef[1][n][c] (coef as written by da_dice_fwd), which lets both
 * anatomy terms skip their 32-channel intermediate tensors:
 *  registration phase: loss = Dice(warp(onehot(lab_m), id + disp), onehot(lab_t)) straight from the two label maps (no warped
 *    one-hot, no gradient tensor); bwd writes d loss / d disp.
 *  segmentation phase: the adjoint warp of g is coef[1][c] A[u] + coef[0][c] B[u][c] with A = W^T 1 ([N][V]) and
 *    B = W^T onehot(lab_t), stored CLASS-MAJOR ([N][C][V]: the atomics of a wave then fall into consecutive floats of one plane) --
 *    da_warp_adjoint_labels zero-fills and scatters B (8 float atomics per voxel instead of 8 C);
 *    A[u] = sum_c B[u][c] is formed on the fly, the optional array A only collects the weights of voxels whose target label is outside
 *    [0, C) (pass NULL when the labels are known to be valid) -- and da_seg_anat_dlogits forms dlogits ([N][V][C]) = d(loss_sup + loss_anat) / d logits from prob and B through the softmax Jacobian
 *    (prob = softmax(logits); coef_sup / lab_m / dloss_sup NULL when there is no supervised Dice term). */
size_t da_label_warp_dice_ws_bytes(int N, int C);
int da_label_warp_dice_fwd(const void* lab_m, int lab_m_bytes, const void* lab_t, int lab_t_bytes, const float* disp,
                           int N, int D, int H, int W, int C, int weight_type, int no_bg, float eps,
                           float* loss, float* coef /*[2][N][C]*/, void* ws, size_t ws_bytes, void* stream);
int da_label_warp_dice_bwd(const void* lab_m, int lab_m_bytes, const void* lab_t, int lab_t_bytes, const float* disp,
                           const float* coef, const float* dloss, float* d_disp, int N, int D, int H, int W, int C, void* stream);
/* segmentation phase, forward: (a) Dice(softmax(src), labels) as da_dice_fwd(softmax = 1) AND prob = softmax(src) written in the same pass
 * (the warp below needs the probabilities: one pass over the logits instead of da_dice_fwd + da_softmax_fwd); (b) Dice(warp(prob, id + disp),
 * onehot(lab_t)) without writing the warped tensor (da_warp_fwd + da_dice_fwd minus one write and one read of N V C floats).  Both return
 * DA_ERR_UNSUPPORTED for class counts whose 4-channel groups are not a power of two; callers then run the separate entries. */
int da_softmax_dice_fwd(const float* src, const void* labels, int label_bytes, float* prob,
                        int N, long long V, int C, int weight_type, int no_bg, float eps,
                        float* loss, float* coef /*[2][N][C]*/, void* ws /* da_dice_ws_bytes */, size_t ws_bytes, void* stream);
size_t da_warp_dice_ws_bytes(int N, int C);
int da_warp_dice_fwd(const float* src, const float* disp, const void* lab_t, int lab_t_bytes,
                     int N, int D, int H, int W, int C, int weight_type, int no_bg, float eps,
                     float* loss, float* coef /*[2][N][C]*/, void* ws, size_t ws_bytes, void* stream);
int da_warp_adjoint_labels(const void* lab_t, int lab_t_bytes, const float* disp, float* A, float* B,
                           int N, int D, int H, int W, int C, void* stream);
int da_seg_anat_dlogits(const float* prob, const void* lab_m, int lab_m_bytes, const float* A, const float* B, float* dlogits,
                        const float* coef_sup, const float* coef_anat, const float* dloss_sup, const float* dloss_anat,
                        int N, long long V, int C, void* stream);
/* ---- Dice between a WARPED LABEL MAP and a DENSE tensor (joint step on a pair whose fixed image has no manual segmentation; parts:
 * lib/loss.py:410-476 Dice, voxel_morph.py:85-91 warp).  W = warp(onehot(lab_m), id + disp) (trilinear, zeros padding, align_corners=True; a corner
 * label outside [0, C) counts for no class, a non-finite or >= 1e9 coordinate gives no taps) is never written.  dense [N][D][H][W][C] fp32:
 *   role 0 (registration phase): dense = probabilities, loss = Dice(source = W, target = dense)
 *   role 1 (segmentation phase): dense = logits, loss = Dice(source = softmax(dense), target = W), the softmax formed per voxel in the kernel
 * weight_type / no_bg / eps, loss[1] and coef[2][N][C] as da_dice_fwd (weights from the TARGET's volume; d loss / d source_c(v) =
 * coef[0][n][c] target_c(v) + coef[1][n][c]).  Double partials per workgroup in ws, summed in a fixed order: no atomics, run-to-run bit-identical.
 * C in {4, 8, 16, 32, 64}, else DA_ERR_UNSUPPORTED (callers compose da_warp_labels_fwd + da_dice_fwd); N <= 64. */
size_t da_softwarp_dice_ws_bytes(int N, int C);
int da_softwarp_dice_fwd(const void* lab_m, int lab_m_bytes, const float* disp, const float* dense, int role,
                         int N, int D, int H, int W, int C, int weight_type, int no_bg, float eps,
                         float* loss, float* coef /*[2][N][C]*/, void* ws, size_t ws_bytes, void* stream);
/* role 0 backward (lib/loss.py:410-476 through voxel_morph.py:85-91): d_disp [N][D][H][W][3] = dloss * d loss / d disp, da_label_warp_dice_bwd with the
 * indicator [corner label == target label] replaced by prob[v][corner label]. */
int da_softwarp_dice_bwd_disp(const void* lab_m, int lab_m_bytes, const float* disp, const float* prob, const float* coef, const float* dloss,
                              float* d_disp, int N, int D, int H, int W, int C, void* stream);
/* role 1 backward (lib/loss.py:410-476, 427 softmax; voxel_morph.py:85-91 on the constant side): dlogits [N][D][H][W][C] = dloss p (g - sum_k p_k g_k),
 * g_c = coef[0][c] W_c + coef[1][c], p = softmax(logits) recomputed: one read of the logits, one write, no scatter. */
int da_softwarp_dice_bwd_logits(const void* lab_m, int lab_m_bytes, const float* disp, const float* logits, const float* coef, const float* dloss,
                                float* dlogits, int N, int D, int H, int W, int C, void* stream);
/* deterministic d_src (parity runs): the same scatter as da_warp_bwd's d_src, accumulated in 64-bit fixed point with integer atomics
 * (order-independent, hence run-to-run bit-identical), scale = power of two from max|dout|.  d_src is OVERWRITTEN (no pre-zeroing). */
size_t da_warp_bwd_dsrc_det_ws_bytes(int N, int D, int H, int W, int C);
int da_warp_bwd_dsrc_det(const float* dout, const float* disp, float* d_src, int N, int D, int H, int W, int C,
                         void* ws, size_t ws_bytes, void* stream);

/* ---- fused softmax + Dice loss (row a11; lib/loss.py:410-476, lib/transforms.py:675-689) ------ */
/* src[N][V][C] logits (softmax != 0) or probabilities; target: labels (label_bytes = 1 uint8 | 8 int64,
 * [N][V]) or, when soft_target != NULL, a soft target [N][V][C] (loss.py:435-436).
 * weight_type: 0 Uniform, 1 Simple, 2 Volume.  Writes loss[1] and coef[2][N][C] for the backward. */
size_t da_dice_ws_bytes(int N, long long V, int C);
int da_dice_fwd(const float* src, const void* labels, int label_bytes, const float* soft_target,
                int N, long long V, int C, int softmax, int weight_type, int no_bg, float eps,
                float* loss, float* coef, void* ws, size_t ws_bytes, void* stream);
/* d_src[N][V][C] = dloss * dL/dsrc; d_soft (may be NULL) = dloss * dL/dsoft_target is not provided. */
int da_dice_bwd(const float* src, const void* labels, int label_bytes, const float* soft_target,
                const float* coef, const float* dloss, float* d_src,
                int N, long long V, int C, int softmax, void* stream);
/* softmax over the channel axis of x[M][C] (joint step: probabilities to warp), and its backward. */
int da_softmax_fwd(const float* x, float* y, long long M, int C, void* stream);
int da_softmax_bwd(const float* dy, const float* y, float* dx, long long M, int C, void* stream);
/* lib/transforms.py:675-689 mask_to_one_hot: labels[N][V] -> out[N][V][C] float */
int da_one_hot(const void* labels, int label_bytes, float* out, long long M, int C, void* stream);

/* ---- fused segmentation head + softmax + Dice (rows a5 + a11: unets.py:249-250 followed by lib/loss.py:410-476 with softmax=True and
 *      an index target).  loss = Dice(softmax(x W + b), labels) WITHOUT writing the logits: the 16 -> 32 head is recomputed in the
 *      backward pass, which turns Dice's gradient straight into dx, dW and db.  x [N][V][Cin] channels-last; w_io [Cin][C];
 *      pro_scale / pro_shift (may be NULL) + pro_slope: BatchNorm + activation of the producer still to be applied to x (as in
 *      da_conv1x1_fwd_pro); coef [2][N][C] as da_dice_fwd.  Shapes: Cin in {16, 64}, C in {16, 32}; others -> DA_ERR_UNSUPPORTED
 *      (callers then run da_conv1x1_* + da_dice_*).  dx is the gradient with respect to the ACTIVATED input. */
size_t da_head_dice_ws_bytes(int N, long long V, int Cin, int C);
int da_head_dice_fwd(const float* x, const float* pro_scale, const float* pro_shift, float pro_slope,
                     const float* w_io, const float* bias, const void* labels, int label_bytes,
                     int N, long long V, int Cin, int C, int weight_type, int no_bg, float eps,
                     float* loss, float* coef, void* ws, size_t ws_bytes, void* stream);
int da_head_dice_bwd(const float* x, const float* pro_scale, const float* pro_shift, float pro_slope,
                     const float* w_io, const float* bias, const void* labels, int label_bytes,
                     const float* coef, const float* dloss, float* dx, float* dw_io, float* dbias,
                     int N, long long V, int Cin, int C, void* ws, size_t ws_bytes, void* stream);
/* da_head_dice_bwd that also accumulates the BatchNorm-backward sums of the layer that produced x (x = its raw conv output; pro_scale / pro_shift /
 * pro_mean = rows of its batch statistics): bst[*bst_n][2][Cin] doubles for da_bn_act_bwd_dbias_pre.  *bst_n = 0: shape without that epilogue
 * (Cin != 16, bst_cap < 1024) -- run da_bn_act_bwd_dbias as usual. */
int da_head_dice_bwd_bst(const float* x, const float* pro_scale, const float* pro_shift, float pro_slope, const float* pro_mean,
                         const float* w_io, const float* bias, const void* labels, int label_bytes,
                         const float* coef, const float* dloss, float* dx, float* dw_io, float* dbias,
                         int N, long long V, int Cin, int C, double* bst, int bst_cap, int* bst_n, void* ws, size_t ws_bytes, void* stream);

/* da_conv3d_k3_dgrad of a layer whose FIRST input was act(BN(y)) applied on the fly: y = the producer's raw conv output, stats4 = its statistics rows
 * [mean | rstd | scale | shift][C1], slope its activation.  dx1 / dx2 as always (gradients with respect to the ACTIVATED tensors); the epilogue also accumulates
 * the PRODUCER's BatchNorm-backward sums, bst[*bst_n][2][C1] doubles = (sum dz, sum dz (y - mean)), dz = dx1 act'(y scale + shift), for
 * da_bn_act_bwd_dbias_pre -- no reduction pass over (dx1, y).  Shapes: one input of <= 16 channels (dx2 NULL, C2 0), or the decoder's concat layer (C1 = 32
 * up-sampled channels, C2 = 16 skip channels; unets.py:275).  Split matrix mode only; DA_ERR_UNSUPPORTED: run da_conv3d_k3_dgrad and the usual backward.
 * autograd of nn.Conv3d / nn.ConvTranspose3d -> nn.BatchNorm3d -> nn.LeakyReLU chains (unets.py:30-37, 50-53). */
int da_conv3d_k3_dgrad_bst(const float* dy, const float* w_tio, float* dx1, int C1, float* dx2, int C2, int N, int D, int H, int W, int Cout,
                           const float* y, const float* stats4, float slope, double* bst, int bst_cap, int* bst_n,
                           void* ws, size_t ws_bytes, void* stream);

/* ---- packed convolution operands kept across calls (split matrix mode; conv3d_mfma.hip) ----------------------------------------------
 * A 3x3x3 convolution call first packs its weights for the matrix cores and writes its tile table (a 10-us launch in front of every matrix kernel).  Both
 * only change when the weights do (torch.optim.Adam.step in the reference's loop, models/segmentation.py:157): the caller may keep them.
 *   da_conv3d_k3_pack_bytes      bytes of one region for a C1 + C2 = Cin -> Cout layer on an N x D x H x W grid (0: no such kernel for the shape)
 *   da_conv3d_k3_prepack         fill b0 (and b1: the data gradient of a 32 + 16 concat layer runs two launches) for the forward (dgrad = 0) or the data
 *                                gradient (dgrad = 1); *used = regions filled, 0 = this shape / matrix mode keeps nothing.  Only enqueues on `stream`.
 *   da_conv3d_k3_use_prepacked   the NEXT da_conv3d_k3_{fwd,fwd_bnstats,fwd_pro,dgrad} call of this thread on `w_tio` skips its pack launch and reads b0 / b1
 *                                (one call; dropped when the next call is on other weights).  The caller orders the fill before the use (stream / event). */
size_t da_conv3d_k3_pack_bytes(int N, int D, int H, int W, int Cin, int Cout);
int da_conv3d_k3_prepack(const float* w_tio, int C1, int C2, int Cout, int dgrad, int N, int D, int H, int W,
                         void* b0, size_t n0, void* b1, size_t n1, int* used, void* stream);
void da_conv3d_k3_use_prepacked(const float* w_tio, const void* b0, size_t n0, const void* b1, size_t n1);
/* da_conv3d_k3_prepack for n layers (arrays of length n) in ceil(regions / 48) launches: the whole network behind one optimiser step. */
int da_conv3d_k3_prepack_many(int n, const float* const* w_tio, const int* C1, const int* C2, const int* Cout, const int* dgrad,
                              const int* N, const int* D, const int* H, const int* W,
                              void* const* b0, const size_t* n0, void* const* b1, const size_t* n1, int* used, void* stream);

/* ---- NCC loss (row a12; lib/loss.py:493-501) -------------------------------------------------- */
/* x, y: [N][V] fp32, any N <= 64 and any V >= 1; the bases need only float alignment (16-byte aligned samples take the float4-from-0 form,
 * every other layout a scalar head up to the next 16-byte boundary, the float4 body and a scalar tail). */
size_t da_ncc_ws_bytes(int N, long long V);
int da_ncc_fwd(const float* x, const float* y, int N, long long V, float* loss, double* stats /*[N][8]*/,
               void* ws, size_t ws_bytes, void* stream);
int da_ncc_bwd(const float* x, const float* y, const double* stats, const float* dloss,
               float* dx, float* dy, int N, long long V, void* stream);

/* ---- bending-energy loss (row a13; lib/loss.py:687-730) --------------------------------------- */
size_t da_bending_ws_bytes(int N, int D, int H, int W);
/* norm: 2 = 'L2' (the weighted squared differences, :721-727); 1 = any other value of the reference's `norm`: the block at :721-727
 * is skipped and the loss is the plain mean of the |differences| (:729). */
int da_bending_fwd(const float* disp, int N, int D, int H, int W, const float* spacing3, int normalize, int norm,
                   float* loss, void* ws, size_t ws_bytes, void* stream);
int da_bending_bwd(const float* disp, const float* dloss, float* d_disp, int N, int D, int H, int W,
                   const float* spacing3, int normalize, int norm, void* stream);

/* ---- cross-entropy family of the loss registry (lib/loss.py:739-761) ------------------------------------------------------
 * logits [M][C] (channels-last voxels), C <= 64.  mode 0: 'cross_entropy' = torch.nn.CrossEntropyLoss(ignore_index, reduction);
 * mode 1: 'focal' = FocalLoss.forward (lib/loss.py:181-213): -alpha[t] (1 + P[t])^gamma log_softmax(x)[t] with P = softmax(x) when
 * `softmax` else x -- the reference's `1 - F.nll_loss(P, t)` is 1 PLUS p_t, kept; mode 2: 'soft_cross_entropy' = SoftCrossEntropy.forward
 * (:115-154) with a class-probability target [M][C]: mean over voxels of sum_c -t_c log_softmax(x)_c (softmax) or -t_c log(max(x_c, 1e-8)).
 * reduction: 0 mean (cross_entropy: over the non-ignored voxels), 1 sum.  denom (1 float, device) is written by fwd and read by bwd. */
size_t da_xent_ws_bytes(void);
int da_xent_fwd(const float* logits, const void* labels, int label_bytes, const float* soft_target, const float* alpha,
                long long M, int C, int mode, int softmax, float gamma, long long ignore_index, int reduction,
                float* loss, float* denom, void* ws, size_t ws_bytes, void* stream);
int da_xent_bwd(const float* logits, const void* labels, int label_bytes, const float* soft_target, const float* alpha,
                const float* dloss, const float* denom, float* dlogits, long long M, int C, int mode, int softmax, float gamma,
                long long ignore_index, void* stream);

/* ---- UNet_generator options (unets.py:230-237) ---------------------------------------------------------------
 * maxpool=False: nn.Conv3d(k2, s2, p0) down-sampler = the adjoint of the k2/s2 transposed conv (same pointwise MFMA kernels).
 * D, H, W are the COARSE (output) dims, the input is 2D x 2H x 2W; w_tio [8][Cin][Cout]; dw_toi [8][Cout][Cin]. */
int da_conv_k2s2_fwd(const float* x, const float* w_tio, const float* bias, float* y,
                     int N, int D, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int da_conv_k2s2_dgrad(const float* dy, const float* w_tio, float* dx,
                       int N, int D, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
size_t da_conv_k2s2_wgrad_ws_bytes(int N, int D, int H, int W, int Cin, int Cout);
int da_conv_k2s2_wgrad(const float* x, const float* dy, float* dw_toi, float* dbias,
                       int N, int D, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
/* upsample=True: nn.Upsample(scale_factor=2, mode='trilinear') (align_corners=False); x [N][D][H][W][C] -> y [N][2D][2H][2W][C] */
int da_upsample_trilinear2_fwd(const float* x, float* y, int N, int D, int H, int W, int C, void* stream);
int da_upsample_trilinear2_bwd(const float* dy, float* dx, int N, int D, int H, int W, int C, void* stream);

/* ---- device data path (lib/transforms.py:71-92 SitkToTensor, :124-158 CropTensor, :508-649 Partition) ------
 * src_dtype: 0 f32, 1 f64, 2 i16, 3 u8, 4 i32.  Volumes are [D][H][W] (numpy order z, y, x), tile3 / overlap3 likewise. */
int da_clamp01_to_f32(const void* src, int src_dtype, float* dst, long long n, void* stream);
int da_crop3d(const void* src, void* dst, int elem_bytes, long long C, int D, int H, int W,
              int d0, int h0, int w0, int Do, int Ho, int Wo, void* stream);
/* overlap tiling with numpy 'reflect' padding; tiles [ceil(D/ez)*ceil(H/ey)*ceil(W/ex)][tz][ty][tx], e = tile - 2*overlap */
int da_partition_tiles(const void* vol, void* tiles, int elem_bytes, int D, int H, int W, const int* tile3, const int* overlap3, void* stream);
/* vote == 0: copy the effective core of each tile; vote != 0 (uint8 labels): per-voxel majority over the covering tiles */
int da_assemble_tiles(const void* tiles, void* vol, int elem_bytes, int D, int H, int W, const int* tile3, const int* overlap3, int vote, void* stream);

/* ---- blended sliding-window inference (csrc/blend.hip; the project's own, after nnU-Net / MONAI sliding_window_inference) --------------
 * The tiling is da_partition_tiles': per axis e = t - 2 o, g = ceil(S / e), tile i holds the volume coordinates i e - o + l, l in [0, t);
 * coordinates outside [0, S) are the reflect padding and take no part.
 * da_blend_accumulate: logits [n_tiles][tz][ty][tx][K] fp32 channels-last = tiles tile0 ... tile0 + n_tiles - 1 of the raster tile order;
 * acc [D][H][W][K] fp32 channels-last, read and written; wz / wy / wx [tz] / [ty] / [tx] fp32 on the device, the window of local position
 * (lz, ly, lx) is (wz[lz] * wy[ly]) * wx[lx] in fp32.  flip: bit 0 / 1 / 2 = the tile was mirrored along z / y / x before the net saw it, its
 * logits are read at t - 1 - l on that axis (the window always at l).  For every voxel and every tile j of the call that covers it, in ascending
 * j: acc[x][c] = acc[x][c] + w * p_c (product and sum rounded separately), p = exp(v_c - max v) / sum_c exp(v_c - max v) in fp32.  Every add
 * starts from the stored value, so acc is a function of the logits and the order of the calls' flip passes alone: bit-identical from run to
 * run and for every split of the tiles into calls.  No atomics: the lanes of the call's lowest covering tile own a voxel.
 * K = 2 ... DA_BLEND_MAX_CLASSES.  DA_ERR_BADARG: null pointers, a geometry da_partition_tiles refuses, tile0 < 0, n_tiles < 1,
 * tile0 + n_tiles beyond the grid, flip outside 0 ... 7, K out of range.
 * da_blend_finalize: labels [V] uint8 = the first-maximum argmax over c of acc[x][.] (da_argmax_dice_counts' tie rule); conf [V] fp32 (may be
 * NULL) = acc[x][label] / sum_c acc[x][c], summed in class order in double, rounded once: NaN where a NaN logit reached the voxel. */
#define DA_BLEND_MAX_CLASSES 256
int da_blend_accumulate(const float* logits, float* acc, int D, int H, int W, int K, const int* tile3, const int* overlap3, int tile0, int n_tiles,
                        const float* wz, const float* wy, const float* wx, int flip, void* stream);
int da_blend_finalize(const float* acc, long long V, int K, unsigned char* labels, float* conf, void* stream);

/* ---- applying a registration on the files' own grids (csrc/regapply.hip; the project's own: one interpolation of the native moving data,
 * cubic B-spline as the reference's resample() defaults to, lib/transforms.py:287) -------------------------------------------------------
 * Volumes are [C][D][H][W], src_dtype as in the preprocessing section (0 f32, 1 f64, 2 i16, 3 u8, 4 i32).  No workspace, no atomics, every
 * output element written by one lane from its own inputs: results are bit-identical from run to run.  No autograd.
 *
 * da_bspline3_prefilter: dst [C][D][H][W] fp32 = the cubic B-spline coefficients of src, scipy.ndimage.spline_filter(x, 3, mode='mirror'):
 * per axis the recursive filter with pole z = sqrt(3) - 2 and gain 6 under whole-sample mirror boundaries (x[-k] = x[k], x[n - 1 + k] =
 * x[n - 1 - k]), c+[k] = 6 x[k] + z c+[k - 1], c[n - 1] = z / (z^2 - 1) (c+[n - 1] + z c+[n - 2]), c[k] = z (c[k + 1] - c+[k]), computed in
 * fp32.  axes: bit 0 / 1 / 2 = filter along W / H / D (7: the full prefilter; the first launch always converts src to fp32 into dst, so a
 * mask is the prefilter of the chosen axes alone); an axis of extent 1 is left as it is.  Three launches, W first: along W the combined
 * causal + anticausal response h_k = sqrt(3) z^|k| is summed directly over mirrored indices from an LDS row segment (lanes along W, Horner
 * from the outermost tap inwards); along H and D one lane owns one line, neighbouring lanes neighbouring W, and runs the recursion in place
 * on dst.  Horizon: the direct sum along W takes DA_BSPLINE_HORIZON taps per side and the causal start of the H and D lines
 * c+[0] = 6 sum_k z^k x[mirror(k)] the same number of terms; |z|^(DA_BSPLINE_HORIZON + 1) = 5e-15, below fp32 rounding of any tap, and no
 * other truncation is made (a line shorter than the horizon is walked through its mirror images).  src and dst must not be the same buffer
 * (the W pass reads its neighbours' inputs): DA_ERR_BADARG, as are null pointers, an extent < 1, a src_dtype or axes out of range; 2^31 or more elements: DA_ERR_UNSUPPORTED.
 *
 * da_warp_frames: out [C][Do][Ho][Wo] on the fixed scan's native grid, one launch.  For output voxel x = (d, h, w):
 *   p = (x - b_f) / a_f          continuous index on the prepared fixed grid (double; the reciprocal of a_f is formed once on the host)
 *   u(p) = s B[u](g(p))          disp [Dp][Hp][Wp][3] fp32, normalised units, channel 0 = x (W axis), sampled trilinearly under border padding
 *                                at the fp32 normalised coordinate g = p / (size - 1) * 2 - 1 (da_field_sample_border, fieldinv.hip's B[u]),
 *                                s = (size - 1) / 2 voxels
 *   q = p + u(p),  y = a_m q + b_m      index on the prepared moving grid, then on the moving scan's native grid (double)
 *   inside iff -0.5 <= y < n - 0.5 on every axis (ops.resample_axis_table's rule); a voxel outside gets default_value
 *   order 0: moving[clamp(floor(y + 0.5))], the source dtype copied bit for bit
 *   order 1: taps f = floor(y), lower clamp(f, 0, n - 1), upper min(lower + 1, n - 1), fraction fp32(y - f), 0 for y < 0; fp32,
 *            fmaf(t, b - a, a) along W, then H, then D (da_resample_axes' arithmetic)
 *   order 3: moving = fp32 coefficients of da_bspline3_prefilter (src_dtype 0); sum of 64 taps floor(y) - 1 ... floor(y) + 2 per axis under
 *            whole-sample mirror indexing (period 2 n - 2; index 0 when n = 1), weights ((1-t)^3, 3t^3 - 6t^2 + 4, -3t^3 + 3t^2 + 3t + 1,
 *            t^3) / 6 at t = fp32(y - floor(y)); fp32, summed along W, then H, then D; not clamped to the input's range.
 * frames: 12 host doubles (a, b) per axis in (D, H, W) order, the fixed frame then the moving frame: native index = a * prepared index + b.
 * A sample position (p, or y after the field) that is NaN, infinite or >= 1e9 in magnitude reads no memory: its voxel gets NaN in a
 * floating-point output and default_value in an integer one; no other voxel is affected.  No address is formed from a data value.
 * world (may be NULL) [3][Do][Ho][Wo] fp32 = A_m (y, 1) - A_f (x, 1) in millimetres, for every voxel (inside or not; NaN for a refused
 * position): affines = 24 host doubles, the 3 x 4 index-to-world matrices A_f then A_m acting on (i, j, k) = (w, h, d); evaluated in
 * double as M_m y - M_f x + (t_m - t_f) and rounded once.
 * DA_ERR_BADARG: null pointers, an extent < 1, a prepared extent < 2, order not 0 / 1 / 3, order 3 with src_dtype != 0, an a that is 0 or
 * not finite, a b that is not finite, world without affines.  DA_ERR_UNSUPPORTED: 2^31 or more elements in moving or out, 2^29 or more
 * voxels in disp. */
#define DA_BSPLINE_HORIZON 24
int da_bspline3_prefilter(const void* src, int src_dtype, float* dst, int C, int D, int H, int W, int axes, void* stream);
int da_warp_frames(const void* moving, int src_dtype, const float* disp, void* out, float* world, int C, int Dm, int Hm, int Wm,
                   int Dp, int Hp, int Wp, int Do, int Ho, int Wo, const double* frames, const double* affines, int order,
                   double default_value, void* stream);

/* synthetic volumes generated on the device (row f4; the structure of the BASELINE configs' synthetic data, the reference's sample
 * convention lib/datasets.py:150-166: image [N][D][H][W] fp32 in [0,1], segmentation uint8).  Counter-based hash: element = f(seed,
 * sample0 + n, voxel), restated bit-exactly in oracle/datapath.py.  mode 0: iid image ~ U[0,1), labels ~ U{0..C-1};
 * mode 1: blocky coordinate-function labels, image = clamp(label / (C-1) + noise U, 0, 1).  img or labels may be NULL. */
int da_synth_volume(float* img, unsigned char* labels, int N, int D, int H, int W, int n_classes, int mode, float noise,
                    unsigned int seed, int sample0, void* stream);

/* ---- volume preprocessing (preprocess.hip; lib/transforms.py:9-57 Resample, :59-68 Normalization, :269-284 LeftToRight, :692-706
 * SegmentationLabelFilter; the percentile rescale is the project's own) on the raw array of a NIfTI file (lib/nifti.py).
 * Volumes are [C][D][H][W]; src_dtype as above (0 f32, 1 f64, 2 i16, 3 u8, 4 i32).  Every entry checks its arguments before any launch
 * (DA_ERR_BADARG), refuses volumes of 2^31 or more elements (DA_ERR_UNSUPPORTED) and has no autograd.  Launch shape of every kernel:
 * 256-thread workgroups, lanes consecutive along W, no workgroup waits for another, what one launch reads from another goes through
 * stream order; reductions accumulate in double in a fixed order (thread -> workgroup -> one finishing launch), the only atomics are
 * integer adds: results are bit-identical from run to run.
 *
 * da_resample_axes: axis-aligned resample onto a grid [C][Do][Ho][Wo], a gather through one table per output axis.  `tables` (device):
 * int32 [Do + Ho + Wo][3], the D entries, then H, then W: {lower tap, upper tap, bits of the float32 fraction}; lower tap -1 marks an entry
 * outside the input.  The table rule (ops.resample_axis_table builds it on the host in float64): output index o reads the continuous input
 * index q = scale * o + offset (one multiply, one add); inside iff -0.5 <= q < n_in - 0.5 (ITK ResampleImageFilter's buffer test on the
 * continuous index).  Nearest: tap clamp(floor(q + 0.5), 0, n_in - 1) (ties round up).  Linear: f = floor(q), lower tap clamp(f, 0, n_in - 1),
 * upper tap min(lower + 1, n_in - 1), fraction float32(q - f); for q < 0 the lower tap is 0 and the fraction 0 (edge-clamped taps).  A negative
 * scale with offset n - 1 is a flip; scale 1 with offset 0 a bit-exact copy.  interpolator 1 (nearest) writes the source dtype bit for bit;
 * interpolator 0 (linear) writes float32, computed in float32 as fmaf(t, b - a, a) along W, then H, then D.  A voxel outside on any axis gets
 * default_value (converted to the output dtype).  Agreement with ITK itself is not tested. */
int da_resample_axes(const void* src, int src_dtype, void* dst, int interpolator, int C, int D, int H, int W, int Do, int Ho, int Wo,
                     const int* tables, double default_value, void* stream);
/* da_volume_moments: out3 (device doubles) = {number of finite voxels, their mean, their unbiased variance}; two passes over the volume, the
 * second accumulating (x - mean)^2 (a sigma of 0.01 on a mean of 1000 survives).  No finite voxel: mean 0; fewer than two: variance 0. */
size_t da_volume_moments_ws_bytes(long long n);
int da_volume_moments(const void* src, int src_dtype, long long n, double* out3, void* ws, size_t ws_bytes, void* stream);
/* da_volume_percentiles: exact order statistics of the float32 values of a volume for one or two percentiles in [0, 100] (host array).
 * Every value maps to a monotone uint32 key (sign bit flipped for non-negatives, all bits for negatives); NaNs are left out and counted.
 * Three-digit radix select (11 + 11 + 10 bits): per digit one launch builds LDS histograms of the keys matching each wanted rank's prefix
 * and adds them into a global histogram, one single-workgroup launch picks the digit of each rank.  numpy's 'linear' rule:
 * rank = p / 100 (n - 1), the two neighbouring order statistics interpolated in double.  out8 (device doubles): {percentile 0, percentile 1,
 * the order statistics (lower, upper) of percentile 0 and of percentile 1, number of non-NaN values, number of NaNs}; NaN where undefined. */
size_t da_volume_percentiles_ws_bytes(long long n);
int da_volume_percentiles(const void* src, int src_dtype, long long n, const double* percentiles, int n_percentiles, double* out8,
                          void* ws, size_t ws_bytes, void* stream);
/* y = (x - a) / b in float32 (x converted to float32 first), optionally clamped to [0, 1]; b == 0 writes zeros. */
int da_affine_intensity_to_f32(const void* src, int src_dtype, float* dst, long long n, float a, float b, int clamp01, void* stream);
/* dst = lut[label] for u8 (3) / i32 (4) labels, dst of the source dtype; lut: device int32 [n_lut], n_lut <= 65536; labels outside it -> 0. */
int da_label_lut(const void* src, int src_dtype, void* dst, long long n, const int* lut, int n_lut, void* stream);

/* ---- random spatial augmentation (lib/transforms.py:161-290: RandomBSplineTransform, RandomRigidTransform, resample) --------
 * sitk.Resample with the image as its own reference grid, for a batch of N samples in one launch.  img / img_out [N][C][D][H][W] fp32,
 * labels / labels_out [N][D][H][W] of label_bytes (1, 4 or 8) bytes; either pair may be NULL (not both).  Output voxel i = (x, y, z) =
 * (w, h, d) reads the input at the continuous index q = A[n][:, :3] (i - o) + A[n][:, 3] (+ the B-spline displacement), with
 * o = (W/2, H/2, D/2) (integer division) and affine A [N][3][4] fp32 on the device.  Inside (-0.5 <= q < size - 0.5 on every axis):
 * image trilinear with neighbours clamped to the volume (interp 0) or nearest (interp 1), labels nearest floor(q + 0.5); outside:
 * 0.1 for the image, 0 for labels.  order 0: no displacement (coef unused).  order 1..3: coef [N][3][gz][gy][gx] fp32 on the device,
 * the (x, y, z) displacement components in INDEX units over a control grid of g = M + order points per axis, M mesh cells spanning
 * the voxel centres [0, size - 1] (ITK BSplineTransformInitializer); every axis needs >= 2 voxels and g >= order + 1.
 * DA_ERR_UNSUPPORTED for gx gy gz > DA_AUG_MAX_GRID_POINTS (the coefficients are staged in LDS) or volumes of >= 2^31 voxels. */
#define DA_AUG_MAX_GRID_POINTS 2048
int da_spatial_resample(const float* img, float* img_out, int C, int interp,
                        const void* labels, void* labels_out, int label_bytes,
                        const float* affine, const float* coef, int order, int gx, int gy, int gz,
                        int N, int D, int H, int W, void* stream);

/* ---- intensity augmentation (lib/transforms.py:293-320: GaussianBlur, BilateralFilter; the fused pointwise pass is the project's own) ----
 * img / out [N][C][D][H][W] fp32, planar, distinct buffers.  `apply` [N] int32 on the device: a sample whose flag is 0 is copied through
 * bit for bit in the same launch.  No atomics; bit-identical from run to run.  DA_ERR_UNSUPPORTED for volumes of >= 2^31 voxels per
 * sample and for N C > 65535.
 *
 * da_gauss_blur3d (lib/transforms.py:293-306, sitk.DiscreteGaussian with useImageSpacing off): separable, taps [3][2 radius + 1] fp32 on the
 * device, axis order (x, y, z) = (W, H, D), computed on the host in fp64 (ITK's GaussianOperator) and rounded once.  Boundary
 * ZeroFluxNeumann: out[i] = sum_k taps[k] in[clamp(i + k - radius)], k ascending, per axis W then H then D.  `tmp`: scratch of the size
 * of img.  radius <= DA_BLUR_MAX_RADIUS; extents below the radius (down to 1) are fine.
 *
 * da_bilateral3d (lib/transforms.py:308-320, sitk.Bilateral = ITK's BilateralImageFilter): domain_w [2 rz + 1][2 ry + 1][2 rx + 1] fp32 =
 * exp(-sum_k (o_k spacing_k)^2 / (2 sigma_d^2)), table [n_samples] fp32 = exp(-0.5 (i cutoff / n_samples)^2 / sigma_r^2), both computed on
 * the host in fp64; cutoff = 4 sigma_r, scale = n_samples / cutoff (fp64 on the host, one fp32).  For centre a and neighbour b (indices
 * clamped to the volume), delta = |b - a|: the tap takes part only if delta < cutoff, with range weight table[floorf(delta * scale)];
 * out = sum w_d w_r b / sum w_d w_r (evaluated as a + sum w (b - a) / sum w).  A NaN neighbour fails the comparison and is skipped; a NaN
 * centre skips every tap and yields NaN for that voxel only.  Radii <= DA_BILATERAL_MAX_RADIUS and n_samples <= DA_BILATERAL_MAX_SAMPLES,
 * else DA_ERR_UNSUPPORTED.  One workgroup per DA_BILATERAL_TILE_D x _H x _W output tile, tile + halo staged in LDS.
 *
 * da_intensity_augment: one pointwise pass.  params [N][DA_INTENSITY_PARAM_STRIDE] 32-bit words on the device: [0] flag word (uint32),
 * [1] gamma, [2] gain, [3] offset, [4] sigma (fp32), [5] seed (uint32).  Stages in this order, each only if its bit is set (all off: an
 * exact copy): BIAS x *= exp(b(i)), b a scalar B-spline of `order` 1..3 over bias_coef [N][gz][gy][gx] (the support rule of
 * da_spatial_resample; staged in LDS, gx gy gz <= DA_AUG_MAX_GRID_POINTS; order 0: no field, the bit is ignored); GAMMA x =
 * clamp01(x)^gamma, with INVERT 1 - (1 - clamp01(x))^gamma; LINEAR x = gain x + offset; NOISE x += sigma n, n = sqrt(-2 ln u1) cos(2 pi u2),
 * u = ((bits >> 8) + 0.5) 2^-24 from the counter hash keyed by (seed, (sample0 + n) C D H W + element index within the sample, stream
 * DA_INTENSITY_STREAM_U1 / _U2), accurate logf / cosf; CLAMP to [0, 1]. */
#define DA_BLUR_MAX_RADIUS 16
#define DA_BILATERAL_MAX_RADIUS 4
#define DA_BILATERAL_MAX_SAMPLES 1024
#define DA_BILATERAL_TILE_D 8
#define DA_BILATERAL_TILE_H 8
#define DA_BILATERAL_TILE_W 32
#define DA_INTENSITY_PARAM_STRIDE 8
#define DA_INTENSITY_BIAS 1
#define DA_INTENSITY_GAMMA 2
#define DA_INTENSITY_INVERT 4
#define DA_INTENSITY_LINEAR 8
#define DA_INTENSITY_NOISE 16
#define DA_INTENSITY_CLAMP 32
#define DA_INTENSITY_STREAM_U1 2u
#define DA_INTENSITY_STREAM_U2 3u
int da_gauss_blur3d(const float* img, float* out, float* tmp, const float* taps, int radius, const int* apply,
                    int N, int C, int D, int H, int W, void* stream);
int da_bilateral3d(const float* img, float* out, const float* domain_w, const float* table, int rx, int ry, int rz, int n_samples,
                   float cutoff, float scale, const int* apply, int N, int C, int D, int H, int W, void* stream);
int da_intensity_augment(const float* img, float* out, const float* params, const float* bias_coef, int order, int gx, int gy, int gz,
                         int sample0, int N, int C, int D, int H, int W, void* stream);

/* ---- random crops (crop.hip; lib/transforms.py:322-505 RandomCrop, BalancedRandomCrop, random_3d_coordinates) ----------------------
 * labels [N][D][H][W], label_dtype 3 u8, 4 i32, 5 i64; window3 (host) = {wd, wh, ww}, 1 <= w <= extent.  Every entry checks its arguments
 * before any launch: DA_ERR_BADARG also for D H W >= 2^31, DA_ERR_UNSUPPORTED for W > 32768 (a row's bits are staged in LDS).  No autograd.
 * Separate launches in stream order, no workgroup waits for another; the only atomic is an integer maximum: bit-identical results.
 *
 * da_window_label_counts (replaces the count of :381, :455 and :473, np.sum(seg_crop == c), for every window at once):
 * counts int32 [N][D - wd + 1][H - wh + 1][W - ww + 1], entry [n][z][y][x] = #{labels[n][z .. z + wd)[y .. y + wh)[x .. x + ww) == cls}.
 * Three separable passes: along W per row (wave ballots, a prefix sum over the words' popcounts, uint16), then running sums along H and D
 * with lanes along x (int32).  Workspace: the two intermediate tensors.
 *
 * da_crop_sample_starts (replaces the rejection loops :437-475 and random_3d_coordinates :497-505): P draws per sample.  Domain per axis:
 * max(S - w, 1) starts (randint's exclusive upper end: the last start is never used), or S - w + 1 with include_last.  conds (host)
 * int32 [n_conds][2] = {class, min_count >= 0}, equal classes adjacent (they share the row and H passes); draw_cond (device) int32 [P]: the
 * condition of each draw, or -1 for an unconditioned draw.  A = the starts of the domain, in raster order, whose count of the class is
 * >= min_count (the whole domain for an unconditioned draw); bits = the counter hash (csrc/counter_hash.h) of seed, counter (sample0 + n) * 65536 + p and stream DA_CROP_STREAM;
 * k = (bits * |A|) >> 32; the result is the k-th element of A.  If A is empty: the start with the largest count, the first in raster order.
 * starts int32 [N][P][3] (z, y, x); info int32 [N][P][2] = {|A|, count at the chosen start (-1 for an unconditioned draw)}.  Workspace: the
 * uint16 row sums and int32 H sums over the domain, one bit per start, one count per z plane; the count tensor itself is never built.
 *
 * da_crop_gather (replaces RegionOfInterestImageFilter, :350-351, :366-368, :384, :429-430, :480-483): img [N][C][D][H][W] fp32 ->
 * img_out [N P][C][wd][wh][ww], labels -> labels_out [N P][wd][wh][ww] of label_bytes (1, 4, 8), sample-major, one launch; img or labels
 * may be NULL.  starts (device) as above; a start outside [0, S - w] is clamped into it in the kernel. */
size_t da_window_label_counts_ws_bytes(int N, int D, int H, int W, const int* window3);
int da_window_label_counts(const void* labels, int label_dtype, int N, int D, int H, int W, const int* window3, long long cls,
                           int* counts, void* ws, size_t ws_bytes, void* stream);
size_t da_crop_sample_starts_ws_bytes(int N, int D, int H, int W, const int* window3, int include_last);
int da_crop_sample_starts(const void* labels, int label_dtype, int N, int D, int H, int W, const int* window3, int include_last,
                          int P, const int* conds, int n_conds, const int* draw_cond, unsigned int seed, int sample0,
                          int* starts, int* info, void* ws, size_t ws_bytes, void* stream);
int da_crop_gather(const float* img, float* img_out, int C, const void* labels, void* labels_out, int label_bytes, const int* starts,
                   int N, int P, int D, int H, int W, const int* window3, void* stream);

/* ---- LNCC similarity (lib/loss.py:589-617 VoxelMorphLNCC = registry 'lncc', and :512-586 LNCCLoss) -----
 * I, J: [N][D][H][W] fp32 (single channel); all-ones F^3 window with dilation `dil` and stride `stride` (1, 1 for VoxelMorphLNCC),
 * valid padding; loss = 1 - mean(cross^2 / (Ivar Jvar + eps)).  Output extent per axis: (L - dil (F-1) - 1) / stride + 1.
 * sums: [5][N][Do][Ho][Wo] floats written by fwd and consumed by bwd of the SAME geometry, opaque to the caller: the five window
 * sums (I, J, I^2, J^2, IJ) in the separable form; in the z-marching form (dil = stride = 1, F = 5 or 9: one fused kernel per
 * direction, reglosses.hip) the five per-window backward terms A', B', C', E1', E2'. */
size_t da_lncc_ws_bytes(int N, int D, int H, int W, int F, int dil, int stride);
int da_lncc_fwd(const float* I, const float* J, int N, int D, int H, int W, int F, int dil, int stride, float eps,
                float* loss, float* sums, void* ws, size_t ws_bytes, void* stream);
int da_lncc_bwd(const float* I, const float* J, const float* sums, const float* dloss, float* dI, float* dJ,
                int N, int D, int H, int W, int F, int dil, int stride, float eps, void* ws, size_t ws_bytes, void* stream);

/* ---- mutual information (VoxelMorph's global MutualInformation; Gaussian Parzen windows) -------------------------------
 * x, y: [N][V] fp32 (float alignment only).  centres c_i = linspace(vmin, vmax, bins), sigma = (vmax - vmin) / (bins - 1) * sigma_ratio,
 * values clamped to [vmin, vmax]; w_i(x) = exp(-(x - c_i)^2 / (2 sigma^2)) / sum_k (same); P = mean_v w(x_v) w(y_v)^T, a / b its marginals;
 * MI = sum_ij P_ij log(P_ij / (a_i b_j + 1e-6) + 1e-6); loss[1] = -mean_n MI.  The V x bins weight matrices are never written: both
 * directions generate them as operands of the fp32 matrix instructions (mi.hip).  stats [N][DA_MI_STATS_FLOATS] is written by fwd and read
 * by bwd (per sample G = dMI/dP [32][32], ga[32], gb[32], MI, padding).  d loss / dx is zero where x lies outside (vmin, vmax); a NaN voxel
 * makes its sample's MI, hence the loss, NaN; +-inf is clamped.  dx or dy may be NULL.  Double partials per workgroup in ws, summed in a fixed
 * order: no atomics, run-to-run bit-identical.  2 <= bins <= 32, finite vmin < vmax, sigma_ratio > 0, N <= 65535; anything else returns
 * DA_ERR_BADARG before any launch. */
#define DA_MI_STATS_FLOATS 1096
size_t da_mi_ws_bytes(int N, long long V, int bins);
int da_mi_fwd(const float* x, const float* y, int N, long long V, int bins, float vmin, float vmax, float sigma_ratio,
              float* loss, float* stats, void* ws, size_t ws_bytes, void* stream);
int da_mi_bwd(const float* x, const float* y, const float* stats, const float* dloss, float* dx, float* dy,
              int N, long long V, int bins, float vmin, float vmax, float sigma_ratio, void* stream);

/* ---- displacement gradient regulariser (row f2; lib/loss.py:625-671 gradientLoss, registry 'gradient') ------------------
 * disp [N][D][H][W][3]; norm = 2 ('L2') or 1; keeps the reference's +/- quirk along H and W (loss.py:661,663). */
size_t da_gradloss_ws_bytes(int N, int D, int H, int W);
int da_gradloss_fwd(const float* disp, int N, int D, int H, int W, const float* spacing3, int normalize, int norm,
                    float* loss, void* ws, size_t ws_bytes, void* stream);
int da_gradloss_bwd(const float* disp, const float* dloss, float* d_disp, int N, int D, int H, int W,
                    const float* spacing3, int normalize, int norm, void* stream);

/* ---- eval: argmax + per-class overlap counts (row a15; models/segmentation.py:188-194) -------- */
/* counts[N][C][3] uint64 = (|pred==c|, |truth==c|, |pred==c & truth==c|), must be zero-filled; pred (may be NULL) uint8 [N][V]. */
int da_argmax_dice_counts(const float* logits, const void* truth, int label_bytes, int N, long long V, int C,
                          unsigned long long* counts, unsigned char* pred, void* stream);

/* ---- eval on label maps (lib/evalMetrics.py:103-217 get_multi_metric / cal_metric / get_multiclass_dice,
 *      lib/loss.py:348-391 DiceLossOnLabel): every one of those metrics is a function of these integer counts ---------- */
/* pred / truth: uint8 (1) or int64 (8) label maps [N][V]; labels outside [0, C) are ignored; counts as above, zero-filled. */
int da_label_overlap_counts(const void* pred, int pred_bytes, const void* truth, int truth_bytes, int N, long long V, int C,
                            unsigned long long* counts, void* stream);

/* ---- registration evaluation (regeval.hip).  The reference lists registration / joint training as TODO (README.md:15-19) and has no
 *      registration metric; these serve the deformation its registration net builds -- deform = disp + identity (voxel_morph.py:85-88,
 *      lib/utils.py:89-102) sampled by F.grid_sample(..., align_corners=True) (voxel_morph.py:90-91) -- and the pairwise datasets it
 *      left as hooks (lib/datasets.py:331-451).  disp [N][D][H][W][3] fp32, channels (x, y, z) = (W, H, D) axis, normalised units. ---- */
/* Nearest-neighbour warp of a label map fused with the overlap counts of the registration Dice: warped = F.grid_sample(lab_m, deform,
 * mode='nearest', padding_mode='zeros', align_corners=True).  The sampling coordinate is computed with the fp32 expressions of da_warp_fwd's
 * kernel, each axis rounded half-to-even; the moving label is read where all three indices are in range, else 0; a non-finite coordinate
 * gives 0.  lab_m / lab_t: uint8 (1) or int64 (8) maps [N][D][H][W].  warped (may be NULL) uint8 [N][D][H][W]: moving labels are stored
 * as uint8 (an int64 label outside [0, 255] wraps) and counted as stored.  counts (may be NULL; not both) [N][C][3] uint64 =
 * (|warped==c|, |lab_t==c|, |both|), zero-filled by the caller, labels outside [0, C) ignored, C <= 1024; lab_t is only read with counts.
 * Exact integers, independent of the order.  DA_ERR_UNSUPPORTED for volumes of >= 2^29 voxels. */
int da_warp_labels_nearest_counts(const void* lab_m, int m_bytes, const void* lab_t, int t_bytes, const float* disp,
                                  int N, int D, int H, int W, int C, unsigned long long* counts, unsigned char* warped, void* stream);
/* Jacobian determinant of x -> x + u(x) with u_c = disp_c (size_c - 1) / 2 voxels, size = (W, H, D): J[c][a] = delta_ca + d u_c / d a,
 * numpy.gradient's differences at unit spacing (central inside, one-sided on the faces), determinant by cofactor expansion in fp32.
 * Every extent >= 2.  stats [N][8] doubles = (sum det, sum det^2, min, max, number of voxels with det <= 0, mean, population variance, 0),
 * accumulated in double from per-workgroup partials added in index order (no atomics: two runs are bit-identical); mean and variance come
 * from the sums of det - 1, which do not cancel for a nearly rigid field.  det_out (may be NULL) [N][D][H][W] fp32. */
size_t da_jacobian_det_ws_bytes(int N, int D, int H, int W);
int da_jacobian_det(const float* disp, int N, int D, int H, int W, double* stats /*[N][8]*/, float* det_out,
                    void* ws, size_t ws_bytes, void* stream);
/* Jacobian folding penalty (jacpen.hip), the differentiable companion of da_jacobian_det's folding count:
 * loss[1] = 1 / (N V) sum_n sum_x max(0, eps - det J_n(x))^power with det J exactly as above (same units, differences and fp32 cofactor
 * expansion; here an extent of 1 is accepted and gives a zero derivative along its axis).  power 1 or 2, 0 <= eps <= 1, N <= 65535; anything
 * else returns DA_ERR_BADARG before any launch, DA_ERR_UNSUPPORTED for volumes of >= 2^29 voxels.  A voxel is active iff det < eps; the
 * identity field has loss 0 and a gradient of exact zeros.  A voxel whose det is not finite makes the loss NaN (and its gradient terms NaN):
 * a non-finite displacement never passes as fold-free, and nothing is indexed by a data value.  fwd writes det [N][D][H][W] fp32, which bwd
 * reads, and, when stats is not NULL, stats[2] doubles = (sum of the penalties, number of active voxels).  The sum is accumulated in double
 * from per-workgroup partials added in index order.  bwd: d_disp [N][D][H][W][3] = dloss[0] x d loss / d disp, a gather through
 * d det / d J_ca = cofactor_ca and the difference stencil (one-sided face rows and the scale (size_c - 1) / 2 included); the Jacobian of a
 * neighbour is formed again only where that neighbour is active.  No atomics in either direction: two runs are bit-identical. */
size_t da_jacdet_penalty_ws_bytes(int N, int D, int H, int W);
int da_jacdet_penalty_fwd(const float* disp, int N, int D, int H, int W, float eps, int power, float* loss, double* stats /*[2]*/,
                          float* det, void* ws, size_t ws_bytes, void* stream);
int da_jacdet_penalty_bwd(const float* disp, const float* det, const float* dloss, float* d_disp, int N, int D, int H, int W,
                          float eps, int power, void* stream);
/* Inverse-consistency penalty of two displacement fields (invcons.hip): the composition residual r(x) = u_a(x) + T[u_b](x + u_a(x)), where T is
 * da_warp_fwd's trilinear sample (zeros outside, align_corners=True) at da_warp_fwd's own fp32 coordinate, and
 * loss[1] = 1 / (N V) sum_n sum_x sum_c (s_c r_c(x))^2 in voxels^2, s_c = (size_c - 1) / 2.  disp_a, disp_b [N][D][H][W][3], units and
 * channel order as above.  A NULL input, N <= 0 or N > 65535, or an extent < 2 returns DA_ERR_BADARG before any launch, a short workspace
 * DA_ERR_WS_SMALL, a volume of >= 2^29 voxels DA_ERR_UNSUPPORTED.  A voxel whose sample coordinate is NaN, infinite or >= 1e9 samples
 * nothing, as in the warp; it makes the loss and both sums NaN and the maximum infinite, and bwd writes NaN into its three d_disp_a components
 * (it adds nothing to d_disp_b), so a bad field never passes as consistent in either direction.
 * fwd writes, when not NULL, resid [N][D][H][W][3] = r (normalised units; bwd reads it) and stats [N][4] doubles per sample = (sum |s r|^2,
 * sum |s r|, max |s r|, number of voxels whose sample point leaves [0, size - 1] on some axis or is not finite), |.| the Euclidean norm in
 * voxels.  The sums are accumulated in double from per-workgroup partials added in index order: two runs are bit-identical.
 * bwd, with g_c(x) = dloss[0] 2 s_c^2 r_c(x) / (N V): d_disp_a (written; may be NULL) = g_k(x) + s_k sum_c g_c(x) dT[u_b,c] / d(voxel
 * coordinate k), a gather; d_disp_b (ADDED into: the caller zero-fills it; may be NULL) = the adjoint of the gather, sum_x w(x -> y) g_c(x),
 * by fp32 atomic adds, one lane per element, in a kernel of its own (arrival order: the last bits vary from run to run).  deterministic != 0: d_disp_b is written (no zero-fill needed)
 * through da_warp_bwd_dsrc_det's fixed-point accumulation, bit-identical from run to run, and ws must hold
 * da_warp_bwd_dsrc_det_ws_bytes(N, D, H, W, 3) bytes; otherwise bwd uses no workspace and ws may be NULL. */
size_t da_invcons_ws_bytes(int N, int D, int H, int W);
int da_invcons_fwd(const float* disp_a, const float* disp_b, int N, int D, int H, int W, float* loss, double* stats /*[N][4] or NULL*/,
                   float* resid /*[N][V][3] or NULL*/, void* ws, size_t ws_bytes, void* stream);
int da_invcons_bwd(const float* disp_a, const float* disp_b, const float* resid, const float* dloss, float* d_disp_a, float* d_disp_b,
                   int N, int D, int H, int W, int deterministic, void* ws, size_t ws_bytes, void* stream);
/* Affine pre-alignment (affine.hip).  theta [N][3][4] fp32 on the device, in exactly the convention of
 *     grid = torch.nn.functional.affine_grid(theta, (N, C, D, H, W), align_corners=True)
 *     out  = torch.nn.functional.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
 * which these entries restate without the V x 3 grid: normalised coordinates, rows and columns in (x, y, z) = (W, H, D) order, the frame of
 * da_warp_fwd's deform; resolution-independent, so one theta serves every pyramid level.  src / out / g [N][D][H][W][C], any C >= 1.
 * The arithmetic runs in centred index space: with s_k = (size_k - 1) / 2 the sample point of output voxel i is
 * q_k = sum_j theta_kj (s_k / s_j) (i_j - s_j) + theta_k3 s_k + s_k, the twelve coefficients, q, the tap weights and the eight-tap sums in double: an output is rounded once.
 * The identity theta returns src bit for bit; a translation by a whole number of voxels whose theta entry 2 t / (size - 1) is exact in fp32
 * returns the shifted volume bit for bit, zeros where it leaves.  A sample coordinate that is NaN, infinite or >= 1e9 in magnitude samples
 * nothing, as in the warp; nothing is indexed by a data value.  A NULL pointer, N <= 0 or N > 65535, C < 1 or an extent < 2 returns
 * DA_ERR_BADARG before any launch, a short workspace DA_ERR_WS_SMALL, a volume of >= 2^29 voxels DA_ERR_UNSUPPORTED.
 * bwd_theta: d_theta [N][3][4] (written) = the gradient of sum_x sum_c g_c(x) out_c(x) with respect to theta,
 * d theta_kj = sum_x sum_c g_c(x) d out_c / d q_k (x) (i_j - s_j) s_k / s_j and d theta_k3 = sum ... s_k: one pass over g, eight taps of src
 * per voxel, accumulated in double from per-workgroup partial rows added in index order (no atomics: two runs are bit-identical).  A sample
 * with a refused coordinate gets a d_theta of NaN, so a broken transform never passes as converged; the other samples are untouched.
 * compose_disp: out(x) = theta (x_n + disp(x), 1) - x_n in the warp's normalised units, x_n the identity coordinate of voxel x: the single
 * displacement field of "affine, then the field predicted on the pre-aligned image"; disp NULL gives the affine's own field. */
int da_affine_warp_fwd(const float* src, const float* theta, float* out, int N, int D, int H, int W, int C, void* stream);
size_t da_affine_warp_ws_bytes(int N, int D, int H, int W);
int da_affine_warp_bwd_theta(const float* g, const float* src, const float* theta, float* d_theta /*[N][3][4]*/, int N, int D, int H, int W,
                             int C, void* ws, size_t ws_bytes, void* stream);
int da_affine_compose_disp(const float* theta, const float* disp /*[N][D][H][W][3] or NULL*/, float* out /*[N][D][H][W][3]*/,
                           int N, int D, int H, int W, void* stream);
/* Instance refinement of a displacement field (refine.hip): descend on 1 - mean_n NCC(moving_n o (identity + disp_n), fixed_n) for this pair,
 * the warped image never written.  moving / fixed [N][D][H][W] fp32 (one channel), disp [N][D][H][W][3]; everything else is da_warp_fwd's
 * convention (normalised units, channels (x, y, z) = (W, H, D), trilinear, zeros outside, align_corners=True; at an integer coordinate the
 * derivative is da_warp_bwd's).  1 <= N <= 64; an extent of 1 is legal (that axis samples index 0 and has gradient 0); < 2^29 voxels per sample
 * (DA_ERR_UNSUPPORTED otherwise).  A sample coordinate that is NaN, infinite or >= 1e9 in magnitude makes the sums of its sample NaN (moments) and
 * its own three gradient / disp / m / v elements NaN (step); nothing is indexed by a data value.
 * moments: stats [N][8] doubles in da_ncc_fwd's layout {mean_w, mean_f, cov, var_w, var_f, ncc, V, 0} of w = the warped moving image, what
 * da_ncc_fwd(warp, fixed) returns up to rounding.  Per-workgroup partial sums in double added in workgroup order: two runs are bit-identical.
 * step: one voxel per lane.  g = lambda_sim d(1 - mean_n NCC_n)/d disp (from stats) + g_extra (the caller's regulariser gradient, already
 * weighted; NULL: none).  grad_out (or NULL) receives g.  update != 0: Adam on disp, m, v in place (a lane touches them at its own voxel only)
 * with the scalars of `state`, DA_REFINE_STATE_FLOATS floats in DEVICE memory = {1 / bc1, beta1, beta2, eps, 1 / sqrt(bc2), grad_scale,
 * lambda_sim, lr_x / bc1, lr_y / bc1, lr_z / bc1, iter, 0}: da_adam_step_dev's state6 for lr = 1, the similarity weight, the per-channel step
 * sizes (lr_c in normalised units; da_adam_step's own lr / bc1, so a channel updates exactly as da_adam_step with lr = lr_c would) and the slot
 * of hist this launch fills.  da_refine_host_state fills a HOST array with them for Adam step `step` (>= 1).  update == 0 needs grad_out, update != 0
 * needs m and v (DA_ERR_BADARG otherwise).  hist (or NULL; hist_len floats): hist[iter] = 1 - mean_n stats[n][5], written by one lane when
 * 0 <= iter < hist_len.  The launch arguments do not depend on the iteration, so the sequence can be captured in a HIP graph and replayed. */
#define DA_REFINE_STATE_FLOATS 12
size_t da_refine_moments_ws_bytes(int N, int D, int H, int W);
int da_refine_moments(const float* moving, const float* fixed, const float* disp, int N, int D, int H, int W, double* stats /*[N][8]*/,
                      void* ws, size_t ws_bytes, void* stream);
int da_refine_host_state(const float* lr3, float beta1, float beta2, float eps, int step, float grad_scale, float lambda_sim, int iter,
                         float* state_host /*[DA_REFINE_STATE_FLOATS]*/);
int da_refine_step(const float* moving, const float* fixed, float* disp, const float* g_extra /*[N][D][H][W][3] or NULL*/, const double* stats,
                   const float* state, float* m, float* v, float* grad_out /*or NULL*/, float* hist /*or NULL*/, int hist_len,
                   int N, int D, int H, int W, int update, void* stream);
/* Inverse of a displacement field and transport of points through it (fieldinv.hip).  disp [N][D][H][W][3], units and channel order as above,
 * is the pull-back map x -> x + u(x).  B[u](p) = F.grid_sample(u, p, 'bilinear', padding_mode='border', align_corners=True): the unnormalised
 * coordinate is clamped to [0, size - 1] before the taps are formed, a tap of index `size` has weight 0 and is not read.  With g the
 * normalised coordinate of an element (da_identity_grid's value at a grid node; index / (size - 1) * 2 - 1 for a point), v_0 = 0 and
 * v_{k+1} = -B[u](g + v_k); the update d_k = |s (v_{k+1} - v_k)| is the Euclidean norm in voxels, s_c = (size_c - 1) / 2.  An element stops
 * after the first update with d_k <= tol_vox or after max_iters updates, all of them inside one launch (tol_vox = 0 runs max_iters updates
 * except where an update is exactly 0).
 * da_field_invert: out [N][D][H][W][3] = v at every voxel, the field with (id + u)(id + v) = id wherever the map stays inside the volume;
 * iters (may be NULL) [N][D][H][W] uint8 = updates performed.
 * da_field_transport_points: points / out [N][P][3] fp32 in voxel index coordinates (x, y, z).  inverse == 0: out = p + s B[u](p), the
 * fixed-frame point p carried into the moving frame (one sample; max_iters and tol_vox are checked but not used).  inverse != 0: out = q + s v,
 * the solution x of x + s B[u](x) = q.  At the grid nodes this is da_field_invert's v bit for bit: both run one device function, and the
 * output's product and sum are rounded separately.
 * An element whose coordinate g + v_k is NaN, infinite or >= 1e9 in magnitude at any update reads no memory, yields NaN in all three
 * components and counts as not converged; so does one whose last update is not finite.  No other element is affected.
 * stats (may be NULL; then ws may be NULL too) [N][4] doubles per sample = (largest final update in voxels, infinite if any element is
 * non-finite; number of elements not converged: final update > tol_vox, or non-finite; number of updates performed; number of elements whose
 * last sample point leaves [0, size - 1] on some axis, where the result is an extrapolation, or is non-finite).  For inverse == 0 the first is
 * the largest displacement and only non-finite points count as not converged.  Reduced per thread, wave, workgroup and then over the
 * per-workgroup rows in index order: no atomics, two runs are bit-identical.
 * A NULL disp / points / out, N <= 0 or N > 65535, an extent < 2, P < 1, max_iters < 1 or > 255, a tol_vox that is negative or NaN return
 * DA_ERR_BADARG before any launch, a short workspace DA_ERR_WS_SMALL, a volume of >= 2^29 voxels DA_ERR_UNSUPPORTED. */
size_t da_field_invert_ws_bytes(int N, int D, int H, int W);
int da_field_invert(const float* disp, float* out, unsigned char* iters /*[N][V] or NULL*/, int N, int D, int H, int W, int max_iters,
                    float tol_vox, double* stats /*[N][4] or NULL*/, void* ws, size_t ws_bytes, void* stream);
size_t da_field_points_ws_bytes(int N, int P);
int da_field_transport_points(const float* disp, const float* points, float* out, int N, int D, int H, int W, int P, int inverse,
                              int max_iters, float tol_vox, double* stats /*[N][4] or NULL*/, void* ws, size_t ws_bytes, void* stream);
/* Multi-atlas label fusion: K atlas label maps warped to each of N target grids and voted per voxel, in one pass.  disp [N][K][D][H][W][3]
 * (units and channel order as above; field (n, k) maps target n's grid into atlas k), addressed with 64-bit offsets.  labels: uint8 (1) or
 * int64 (8) maps [K][D][H][W] shared by all targets (label_sample_stride 0) or one block per target (label_sample_stride = elements between
 * the blocks of consecutive targets, >= K D H W).  The label of atlas k at a target voxel is exactly what da_warp_labels_nearest_counts stores
 * (same fp32 coordinate, half-to-even rounding, 0 outside the volume or for a non-finite coordinate, stored as uint8).  Weights (>= 0; at
 * most one form, both NULL = majority vote): w_atlas [N][K] or w_voxel [N][K][D][H][W] fp32.  score(c) = sum_k w_k [label_k = c], added in
 * atlas order in fp32 (integer counts without weights); fused [N][D][H][W] uint8 = the class of the largest score, ties to the smallest
 * label; conf (may be NULL) [N][D][H][W] fp32 = winning score / sum_k w_k; a zero total gives fused 0, conf 0.  No atomics: two runs are
 * bit-identical.  1 <= K <= 32; DA_ERR_UNSUPPORTED for K > 32 or volumes of >= 2^29 voxels. */
int da_label_fusion_vote(const void* labels, int label_bytes, long long label_sample_stride, const float* disp,
                         const float* w_atlas, const float* w_voxel, int N, int K, int D, int H, int W,
                         unsigned char* fused, float* conf, void* stream);
/* Weights of locally weighted voting: weights[n][k][x] = exp(-beta m), m = (2 radius + 1)^-3 x the sum over the (2 radius + 1)^3 window
 * around x of (warped[n][k] - target[n])^2; voxels outside the volume contribute 0, the divisor is constant.  warped [N][K][D][H][W],
 * target [N][D][H][W], weights [N][K][D][H][W] fp32; radius 1..4, beta >= 0.  Separable direct window sums (no sliding sum) in fp32, expf.
 * ws: one field of the size of `weights` (da_local_msd_weights_ws_bytes). */
size_t da_local_msd_weights_ws_bytes(int N, int K, int D, int H, int W);
int da_local_msd_weights(const float* warped, const float* target, int N, int K, int D, int H, int W, int radius, float beta,
                         float* weights, void* ws, size_t ws_bytes, void* stream);

/* ---- connected components of a label map and the largest-component / minimum-size clean-up (cc.hip).  No reference call site: the
 *      reference scores the raw argmax; these replace what its users run before scoring or using a prediction, scipy.ndimage.label on a
 *      host copy, once per class and volume. ---------- */
/* labels: uint8 (1), int32 (4) or int64 (8) maps [N][D][H][W].  Labels <= 0 are background, and so are labels >= n_class where n_class > 0
 * (da_cc_label: n_class 0 = every positive label is a class).  Two voxels are connected when they hold the same class and are neighbours
 * under `connectivity`: 6 (faces), 18 (faces, edges) or 26 (faces, edges, corners); samples, rows and planes never wrap into each other.
 * da_cc_label: roots [N][D][H][W] int32 = 0 on background, elsewhere 1 + the smallest raster index (d H + h) W + w of the voxel's component;
 * sizes [N][D][H][W] int32 = the component's voxel count at its root's position, 0 elsewhere.  Both are functions of the input alone: two runs
 * are bit-identical.  Union-find over the grid: tiles of DA_CC_TILE_D x _H x _W labelled in LDS, the tile seams joined with lock-free
 * min-linking on agent-scope atomics (no workgroup waits for another), roots and sizes written by a launch of its own.
 * ws: one int32 per voxel (da_cc_ws_bytes).
 * da_cc_select (after da_cc_label with the same labels and n_class): best [N][n_class] uint64, zero-filled by the caller =
 * max over the components of the class of (size << 32) | (0xFFFFFFFF - root index): the largest component, ties to the smallest root;
 * 0 for a class without voxels.  stats [N][n_class][3] int64, zero-filled by the caller = (number of components, size of the largest,
 * voxels of the class); row 0 (background) stays 0.
 * da_cc_filter: out [N][D][H][W] in the labels' dtype = the label where the voxel is kept, else 0.  mode 0 keeps the voxels of their class's
 * largest component (needs best), mode 1 those of components with at least min_size >= 1 voxels (needs sizes).
 * A NULL pointer, N <= 0 or N > 65535, an extent < 1, label_bytes not 1 / 4 / 8, another connectivity or mode, n_class < 0 (label) or < 1
 * (select, filter), min_size < 1 return DA_ERR_BADARG before any launch, a short workspace DA_ERR_WS_SMALL, a volume of >= 2^31 voxels or
 * n_class > DA_CC_MAX_CLASSES DA_ERR_UNSUPPORTED. */
#define DA_CC_TILE_D 4
#define DA_CC_TILE_H 8
#define DA_CC_TILE_W 32
#define DA_CC_MAX_CLASSES 1024
size_t da_cc_ws_bytes(int N, int D, int H, int W);
int da_cc_label(const void* labels, int label_bytes, int N, int D, int H, int W, int n_class, int connectivity,
                int* roots, int* sizes, void* ws, size_t ws_bytes, void* stream);
int da_cc_select(const void* labels, int label_bytes, const int* sizes, int N, long long V, int n_class,
                 unsigned long long* best /*[N][n_class]*/, unsigned long long* stats /*[N][n_class][3]*/, void* stream);
int da_cc_filter(const void* labels, int label_bytes, const int* roots, const int* sizes, const unsigned long long* best,
                 int N, long long V, int n_class, int mode, int min_size, void* out, void* stream);

/* ---- exact Euclidean distance transform, signed distance maps of a label map and the boundary loss on them (edt.hip).  No reference call
 *      site: these replace a host copy and scipy.ndimage.distance_transform_edt once per class and volume; the loss is Kervadec et al.,
 *      "Boundary loss for highly unbalanced segmentation". ---------- */
/* A site set is the set of voxels a distance is measured to; the transform of a volume [D][H][W] with the spacing (sD, sH, sW) is
 * out(x) = min over sites y of (sD (xd - yd))^2 + (sH (xh - yh))^2 + (sW (xw - yw))^2, +inf where the sample has no site.  Exact and separable:
 * a pass along W with wave ballots, then the exhaustive pruned minimum along H and along D on lines staged in LDS, DA_EDT_LINE_CHUNK entries at a
 * time.  float32 throughout; with unit spacing every value is an exact integer, which is why extents with D^2 + H^2 + W^2 >= 2^24 are refused.
 * No atomics; results are functions of the input alone, bit-identical from run to run.
 * Maps (masks, labels) are uint8 (1), int32 (4) or int64 (8), [N][D][H][W]; samples never interact.
 * da_edt_ws_bytes: the workspace of both entries below for Kp site sets per sample (da_edt_sq: Kp = 1).
 * da_edt_sq: out [N][D][H][W] = the squared distance (take_sqrt != 0: the distance, one correctly rounded square root) of every voxel to the
 * nearest ZERO voxel of the mask -- scipy's convention: 0 on the zero voxels.
 * da_signed_distance_maps: classes [Kp] int32 on the device.  phi is PLANAR, [N][Kp][D][H][W] float32 (not channels-last like the logits: the
 * last pass stores whole rows of a plane, and the loss kernel reads the planes directly): for class c = classes[j],
 * phi = + the distance to the nearest voxel of class c outside the class, - the distance to the nearest voxel not of class c inside it, and 0
 * everywhere in a sample where class c is absent or fills the sample.  The plain signed distance: Kervadec's one_hot2dist shifts the inside by
 * one voxel ((d_in - 1)), this does not.  Labels that are in no class list are simply "not of class c".
 * da_boundary_loss_fwd: logits [N][D][H][W][K] channels-last (V = D H W), slots [K] int32 on the device = the plane of class k in phi or -1
 * (entries outside [0, Kp) count as -1);  loss[0] = 1 / (N Kp V) sum_n sum_k with slot sum_x softmax(logits)_k(x) phi_slot(k)(x).  The softmax
 * runs over all K logits in registers (K % 4 == 0 and K / 4 a power of two <= 16: K / 4 lanes per voxel; otherwise a thread per voxel), nothing of
 * size K x V is written, the sum has a fixed order (per-workgroup doubles, one finalising workgroup; ws: da_boundary_loss_ws_bytes).
 * da_boundary_loss_bwd: dlogits [N][V][K] = dloss[0] p_k (m_k phi_k - sum_c m_c p_c phi_c) / (N Kp V), one pass, the softmax recomputed.
 * A NULL pointer, N < 1 or N > 65535, an extent < 1, bytes not 1 / 4 / 8, a spacing that is not positive and finite, Kp < 1, K < 1 or Kp > K
 * return DA_ERR_BADARG before any launch, a short workspace DA_ERR_WS_SMALL; D^2 + H^2 + W^2 >= 2^24, a volume of >= 2^31 voxels or K > 64
 * DA_ERR_UNSUPPORTED. */
#define DA_EDT_LINE_CHUNK 256
size_t da_edt_ws_bytes(int N, int Kp, int D, int H, int W);
int da_edt_sq(const void* mask, int mask_bytes, int N, int D, int H, int W, float sD, float sH, float sW, int take_sqrt,
              float* out, void* ws, size_t ws_bytes, void* stream);
int da_signed_distance_maps(const void* labels, int label_bytes, const int* classes /*[Kp]*/, int Kp, int N, int D, int H, int W,
                            float sD, float sH, float sW, float* phi /*[N][Kp][D][H][W]*/, void* ws, size_t ws_bytes, void* stream);
size_t da_boundary_loss_ws_bytes(int N);
int da_boundary_loss_fwd(const float* logits, const float* phi, const int* slots /*[K]*/, int N, long long V, int K, int Kp,
                         float* loss, void* ws, size_t ws_bytes, void* stream);
int da_boundary_loss_bwd(const float* logits, const float* phi, const int* slots /*[K]*/, const float* dloss, int N, long long V, int K, int Kp,
                         float* dlogits, void* stream);

/* ---- surface-distance metrics of two label maps (edt.hip): Hausdorff distance, its percentile (HD95) and the average symmetric surface
 *      distance, medpy's conventions.  No reference call site: these replace a host copy, scipy.ndimage.binary_erosion and two
 *      distance_transform_edt per class and volume. ---------- */
/* A surface voxel of class c is a voxel with label c that has a neighbour under the connectivity (6, 18 or 26: scipy's
 * generate_binary_structure(3, 1 | 2 | 3)) with another label or outside the volume.  For c = classes[j] and sample n, d_PT are the Euclidean
 * distances, under the spacing, of the surface voxels of pred's class c to the nearest surface voxel of truth's class c, d_TP the other way.
 * stats [N][Kp][7] double = n_pred, n_truth (the surface voxel counts), hd = max(max d_PT, max d_TP), hd_pct = numpy's linear percentile of
 * the pooled d_PT and d_TP, assd = (mean d_PT + mean d_TP) / 2, mean d_PT, mean d_TP; the last five are NaN where the class is absent from
 * either map of the sample.  The distances come from the transform above with the surfaces as site sets, in class groups as the signed
 * maps; the order statistics from a radix select on the float32 bit patterns of the squared distances, the sums from a fixed order in
 * double: integer atomics only, bit-identical from run to run.  pred and truth are [N][D][H][W], uint8 (1), int32 (4) or int64 (8) each;
 * a label that is in no entry of `classes` belongs to no class.
 * da_label_surface: mask [N][D][H][W] uint8 = the voxel is a surface voxel of its own label.
 * A NULL pointer, bytes not 1 / 4 / 8, a connectivity other than 6 / 18 / 26, a percentile outside (0, 100], a bad spacing, extent or Kp
 * return DA_ERR_BADARG before any launch, a short workspace DA_ERR_WS_SMALL; extents the transform refuses or Kp > 65535 DA_ERR_UNSUPPORTED. */
int da_label_surface(const void* labels, int label_bytes, int N, int D, int H, int W, int connectivity, unsigned char* mask, void* stream);
size_t da_surface_dist_ws_bytes(int N, int Kp, int D, int H, int W);
int da_surface_dist_stats(const void* pred, int pred_bytes, const void* truth, int truth_bytes, const int* classes /*[Kp]*/, int Kp,
                          int N, int D, int H, int W, float sD, float sH, float sW, int connectivity, double percentile,
                          double* stats /*[N][Kp][7]*/, void* ws, size_t ws_bytes, void* stream);

/* ---- optimiser (models/segmentation.py:91 torch.optim.Adam defaults) -------------------------- */
int da_adam_step(float* p, const float* g, float* m, float* v, long long n,
                 float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* stream);

/* the same update with its per-step scalars in DEVICE memory -- state6 = {lr / bc1, beta1, beta2, eps, 1 / sqrt(bc2), grad_scale} -- so
 * that the launch can be captured in a HIP graph and replayed (deepatlas_amd/graphs.py); da_adam_host_state fills a HOST array with
 * those six values for step `step`, using da_adam_step's own expressions (the two paths update bit-identically). */
int da_adam_host_state(float lr, float beta1, float beta2, float eps, int step, float grad_scale, float* state6_host);
int da_adam_step_dev(float* p, const float* g, float* m, float* v, long long n, float* state6, void* stream);

/* =====================================================================================================================
 * bf16 ACTIVATION STORAGE (BASELINE.json configs[4]: "bf16 mixed precision"; SURVEY.md 8(d) config 5: "bf16 activations / MFMA, fp32
 * master weights, fp32 reductions").  The reference has no such mode (train_seg.py is fp32-only); these are the `_bf16` twins of the
 * entries above for a network whose INTERNAL activation and gradient tensors are stored as bf16 (same NDHWC layout, 2 bytes per element).
 * `void*` arguments are those bf16 tensors; every `float*` keeps its meaning (weights, biases, statistics, scale / shift, weight and bias
 * gradients, logits and their gradient, losses).  Arithmetic is fp32 (double in the reductions); a value is rounded to nearest-even once,
 * when it is stored.  BatchNorm statistics fused into a producer's epilogue are those of the fp32 values before that rounding.
 * The convolution twins need the bf16 matrix mode (da_set_matrix_mode(1)) and the matrix-core shapes; DA_ERR_UNSUPPORTED otherwise -- the
 * caller then converts with da_cast_* around the fp32 entry (deepatlas_amd/ops.py: call_act).
 * ===================================================================================================================== */
int da_cast_f32_to_bf16(const float* x, void* y, long long numel, void* stream);
int da_cast_bf16_to_f32(const void* x, float* y, long long numel, void* stream);
/* norm_act.hip */
int da_bn_train_stats_bf16(const void* x, long long M, int C, const float* gamma, const float* beta,
                           float eps, float momentum, float* running_mean, float* running_var,
                           float* mean, float* rstd, float* scale, float* shift, void* ws, size_t ws_bytes, void* stream);
int da_bn_act_fwd_bf16(const void* x, const float* scale, const float* shift, float act_slope, void* y, long long M, int C, void* stream);
int da_bn_act_bwd_dbias_bf16(const void* dy, const void* x, const float* mean, const float* rstd,
                             const float* scale, const float* shift, float act_slope, int train,
                             void* dx, float* dgamma, float* dbeta, float* dxsum, long long M, int C,
                             void* ws, size_t ws_bytes, void* stream);
int da_act_bwd_bf16(const void* dy, const void* y, float act_slope, void* dx, long long numel, void* stream);
int da_act_bwd_add_dbias_bf16(const void* g1, const void* g2, const void* y, float act_slope, void* dx, float* dbias,
                              long long M, int C, void* ws, size_t ws_bytes, void* stream);
int da_act_bwd_add_partial_bf16(const void* g1, const void* g2, const void* y, float act_slope, void* dx,
                                long long M, int C, void* partial, size_t partial_bytes, int* nparts, void* stream);
int da_colsum_bf16(const void* x, long long M, int C, float* out, void* ws, size_t ws_bytes, void* stream);
/* pool.hip */
int da_maxpool2_fwd_bf16(const void* x, void* y, int N, int D, int H, int W, int C, void* stream);
int da_maxpool2_fwd_pro_bf16(const void* x, const float* pro_scale, const float* pro_shift, float pro_slope, void* act, void* y,
                             int N, int D, int H, int W, int C, void* stream);      /* the maximum is taken over the ROUNDED activations */
int da_maxpool2_bwd_bf16(const void* dy, const void* x, void* dx, int N, int D, int H, int W, int C, void* stream);
int da_maxpool2_bwd_add_bf16(const void* dy, const void* x, const void* gskip, void* dx, int N, int D, int H, int W, int C, void* stream);
int da_upsample_nearest_fwd_bf16(const void* x, void* y, int N, int D, int H, int W, int C, int Do, int Ho, int Wo, void* stream);
int da_upsample_nearest_bwd_bf16(const void* dy, void* dx, int N, int D, int H, int W, int C, int Do, int Ho, int Wo, void* stream);
/* conv3d.hip / conv3d_mfma.hip: `bf16_mask` = one bit per activation argument in signature order (set = bf16).  Native: all set. */
int da_conv3d_k3_fwd_bf16(const void* in1, int C1, const void* in2, int C2, const float* w_tio, const float* bias, void* out,
                          int N, int D, int H, int W, int Cout, int stride, float act_slope,
                          void* ws, size_t ws_bytes, void* stream, unsigned bf16_mask);
int da_conv3d_k3_fwd_bnstats_bf16(const void* in1, int C1, const void* in2, int C2, const float* w_tio, const float* bias, void* out,
                                  int N, int D, int H, int W, int Cout, int stride,
                                  double* stats_partial, int stats_capacity, int* stats_nparts,
                                  void* ws, size_t ws_bytes, void* stream, unsigned bf16_mask);
int da_conv3d_k3_fwd_pro_bf16(const void* in1, int C1, const float* pro1_scale, const float* pro1_shift, float pro1_slope,
                              const void* in2, int C2, const float* pro2_scale, const float* pro2_shift, float pro2_slope,
                              const float* w_tio, const float* bias, void* out,
                              int N, int D, int H, int W, int Cout, float act_slope,
                              double* stats_partial, int stats_capacity, int* stats_nparts,
                              void* ws, size_t ws_bytes, void* stream, unsigned bf16_mask);
int da_conv3d_k3_wgrad_pro_bf16(const void* in1, int C1, const float* pro1_scale, const float* pro1_shift, float pro1_slope,
                                const void* in2, int C2, const float* pro2_scale, const float* pro2_shift, float pro2_slope,
                                const void* dy, float* dw_tio, int N, int D, int H, int W, int Cout,
                                void* ws, size_t ws_bytes, void* stream, unsigned bf16_mask);
int da_conv3d_k3_dgrad_bf16(const void* dy, const float* w_tio, void* dx1, int C1, void* dx2, int C2,
                            int N, int D, int H, int W, int Cout, int stride, void* ws, size_t ws_bytes, void* stream, unsigned bf16_mask);
int da_conv3d_k3_wgrad_bf16(const void* in1, int C1, const void* in2, int C2, const void* dy, float* dw_tio, float* dbias,
                            int N, int D, int H, int W, int Cout, int stride, void* ws, size_t ws_bytes, void* stream, unsigned bf16_mask);
/* deconv.hip / pointwise_mfma.hip: transposed conv k2 s2 (input, output, their gradients bf16); 1x1x1 head (input and its gradient
 * bf16; logits and their gradient fp32).  An entry whose OUTPUT is bf16 returns DA_ERR_UNSUPPORTED when its reduction runs over more than 64 channels (forward:
 * Cin > 64; data gradients: Cout > 64): the 64-channel slices accumulate through the output tensor, which would round a bf16 output once per slice. */
int da_deconv_k2s2_fwd_bf16(const void* in, const float* w_tio, const float* bias, void* out,
                            int N, int D, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int da_deconv_k2s2_fwd_bnstats_bf16(const void* in, const float* w_tio, const float* bias, void* out,
                                    int N, int D, int H, int W, int Cin, int Cout,
                                    double* stats_partial, int stats_capacity, int* stats_nparts, void* ws, size_t ws_bytes, void* stream);
int da_deconv_k2s2_dgrad_bf16(const void* dy, const float* w_tio, void* dx,
                              int N, int D, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int da_deconv_k2s2_wgrad_bf16(const void* in, const void* dy, float* dw_tio, float* dbias,
                              int N, int D, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int da_conv1x1_fwd_bf16(const void* in, const float* w_io, const float* bias, float* out,
                        long long M, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int da_conv1x1_fwd_pro_bf16(const void* in, const float* pro_scale, const float* pro_shift, float pro_slope,
                            const float* w_io, const float* bias, float* out, long long M, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int da_conv1x1_dgrad_bf16(const float* dy, const float* w_io, void* dx, long long M, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int da_conv1x1_wgrad_bf16(const void* in, const float* dy, float* dw_io, float* dbias,
                          long long M, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int da_conv1x1_wgrad_pro_bf16(const void* in, const float* pro_scale, const float* pro_shift, float pro_slope,
                              const float* dy, float* dw_io, float* dbias, long long M, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
/* headdice.hip: fused head + softmax + Dice with a bf16 input x and a bf16 gradient dx */
int da_head_dice_fwd_bf16(const void* x, const float* pro_scale, const float* pro_shift, float pro_slope,
                          const float* w_io, const float* bias, const void* labels, int label_bytes,
                          int N, long long V, int Cin, int C, int weight_type, int no_bg, float eps,
                          float* loss, float* coef, void* ws, size_t ws_bytes, void* stream);
int da_head_dice_bwd_bf16(const void* x, const float* pro_scale, const float* pro_shift, float pro_slope,
                          const float* w_io, const float* bias, const void* labels, int label_bytes,
                          const float* coef, const float* dloss, void* dx, float* dw_io, float* dbias,
                          int N, long long V, int Cin, int C, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPATLAS_HIP_H */
