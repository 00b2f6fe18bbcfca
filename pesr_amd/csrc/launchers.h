// Internal C++ launchers (one per kernel family); wrapped by api.hip into the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <type_traits>

// Kernels templated on the channel count: calls f(std::integral_constant<int, c>) for the listed c equal to C, as in
// pesr_dispatch_c<64, 128, 256>(C, [&](auto c) { hipLaunchKernelGGL(kernel<c()>, ...); }).  false: C is not in the list, f was not called.
template <int... Cs, class F>
static inline bool pesr_dispatch_c(int C, F&& f) {
    return ((C == Cs && (f(std::integral_constant<int, Cs>{}), true)) || ...);
}

int pesr_pack_conv3x3_launch(const float* w, float* out, int O, int I, int mode, int ps, hipStream_t stream);
int pesr_pack_conv3x3_batched_launch(const long long* desc, int count, hipStream_t stream);
int pesr_pack_bias_ps_launch(const float* b, float* out, int O, hipStream_t stream);

// BatchNorm sums out of a conv kernel's epilogue (round 6; include/pesr_hip.h PesrBnFuse + the launcher's own in / out fields)
struct PesrBnFuseArgs {
    int mode;                 // 1: sum / sum of squares of the stored output; 2: the kernel writes g' = v * lrelu'(bn(z)) and sums g', g' * xhat
    int rows;                 // capacity of `part` in rows of [2][C]
    float* part;
    const float* z;           // mode 2
    const float* mean_invstd; // mode 2: [2][C]
    const float* gamma;
    const float* beta;
    float slope;
    int dry;                  // plan only: report rows_out, launch nothing
    long rows_out;            // rows the launch writes (0: this shape is not covered - split-K, packed-shuffle stores, odd channel counts)
};

int pesr_conv3x3_launch(const float* x, const float* wp, const float* bias, const float* skip, const float* mask, float* y,
                        int N, int H, int W, int Cin, int Cout, int stride, float alpha, int act, float slope, int ps,
                        int ps_in, int flip, int cin_real, int cout_store, void* ws, size_t ws_bytes, hipStream_t stream,
                        PesrBnFuseArgs* fuse = nullptr);
int pesr_conv3x3_s2_dgrad_launch(const float* dy, const float* wp, const float* mask, float* dx, int N, int H, int W,
                                 int Cout_fwd, int Cin_fwd, float alpha, hipStream_t stream, PesrBnFuseArgs* fuse = nullptr);

size_t pesr_conv3x3_wgrad_ws_bytes(int N, int H, int W, int Cin, int Cout, int stride, int algo);
// The kernel a weight gradient runs on (include/pesr_hip.h PESR_WGRAD_KERNEL_*): the answer of pesr_conv3x3_wgrad_kernel_impl, the rule
// pesr_conv3x3_wgrad_launch dispatches by, and (the two F(4,3) values) the `variant` of pesr_conv3x3_wgrad_wino4_launch.
enum PesrWgradKernel {
    PESR_WGK_DIRECT = 0,          // conv3x3_wgrad_kernel
    PESR_WGK_WINO23 = 1,          // conv3x3_wgrad_wino_kernel
    // 2, 3: retired (the 16x16x4-MFMA kernel, the 1-D transform on the 12-wave kernel); never answered any more
    PESR_WGK_WINO4_12W = 4,       // conv3x3_wgrad_wino4x_kernel: F(2,3)y x F(4,3)x on 32x32x2 MFMA, 12 waves that stage and multiply
    PESR_WGK_WINO4_PRODUCER = 5   // conv3x3_wgrad_wino4p_kernel: the same transform, staging on four producer waves (the product)
};
// Host only.  A PesrWgradKernel, or the error the launch returns (PESR_EINVAL, PESR_EWORKSPACE).  ws_bytes: the caller's workspace (a Winograd form that
// needs more than it is passed over, as the launch always did); a query passes SIZE_MAX.
int pesr_conv3x3_wgrad_kernel_impl(int N, int H, int W, int Cin, int Cout, int stride, int ps_in, int algo, int accumulate, size_t ws_bytes);
int pesr_conv3x3_wgrad_launch(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                              int stride, float alpha, int ps_in, int algo, int accumulate, void* ws, size_t ws_bytes, hipStream_t stream);
int pesr_bias_grad_launch(const float* dy, float* db, long pixels, int Cout, int OW, float alpha, int ps_in, float* part,
                          size_t part_bytes, hipStream_t stream);

size_t pesr_conv3x3_wgrad_rgb_ws_bytes(int N, int H, int W, int C);
int pesr_conv3x3_wgrad_rgb_launch(const float* A, const float* b3, float* dw, float* db, int N, int H, int W, int C, int mode,
                                  float alpha, int accumulate, void* ws, size_t ws_bytes, hipStream_t stream);

int pesr_meanshift_fwd_launch(const float* x, const float* w, const float* b, float* y, int N, int H, int W, long xsn, long xsc,
                              long xsp, long ysn, long ysc, long ysp, hipStream_t stream);
int pesr_meanshift_bwd_launch(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, int N, int H,
                              int W, long xsn, long xsc, long xsp, void* ws, size_t ws_bytes, hipStream_t stream);
int pesr_pixel_shuffle_launch(const float* in, float* out, int N, int H, int W, int C, int inverse, hipStream_t stream);
int pesr_pixel_shuffle_r_launch(const float* in, float* out, int N, int H, int W, int C, int r, int inverse, hipStream_t stream);
int pesr_relu_mask_launch(const float* g, const float* ref, const float* add, float* out, long n, float alpha, float slope, hipStream_t stream);
int pesr_maxpool2x2_fwd_launch(const float* x, float* y, int N, int H, int W, int C, hipStream_t stream);
int pesr_maxpool2x2_bwd_launch(const float* x, const float* dy, float* dx, int N, int H, int W, int C, int relu_in, hipStream_t stream);

size_t pesr_bn_ws_bytes(long M, int C);
size_t pesr_conv_rgb_bn_ws_bytes(int N, int H, int W, int C);
int pesr_conv_rgb_bn_lrelu_fwd_launch(const float* x, const float* w, float* z, const float* gamma, const float* beta, float* y,
                                      float* mean_invstd, float* running_mean, float* running_var, long long* num_batches, int N, int H,
                                      int W, int C, float eps, float momentum, float slope, int y_nchw, void* ws, size_t ws_bytes,
                                      hipStream_t stream);
int pesr_bn_lrelu_fwd_launch(const float* x, const float* gamma, const float* beta, float* y, float* mean_invstd,
                             float* running_mean, float* running_var, long long* num_batches, long M, int C, long HW, float eps,
                             float momentum, float slope, int y_nchw, void* ws, size_t ws_bytes, hipStream_t stream);
int pesr_bn_lrelu_bwd_launch(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean_invstd,
                             float* dx, float* dgamma, float* dbeta, long M, int C, long HW, float slope, int dy_nchw, int accumulate,
                             void* ws, size_t ws_bytes, hipStream_t stream);

int pesr_bn_finalize_launch(const float* part, int rows, int C, long M, float eps, float momentum, float* mean_invstd, float* running_mean,
                            float* running_var, long long* num_batches, hipStream_t stream);
int pesr_bn_lrelu_bwd_fused_launch(const float* z, const float* gmasked, const float* part, int rows, const float* gamma, const float* beta,
                                   const float* mean_invstd, float* dz, float* dgamma, float* dbeta, long M, int C, long HW, int accumulate,
                                   void* ws, size_t ws_bytes, hipStream_t stream);
int pesr_bn_lrelu_apply_launch(const float* x, const float* gamma, const float* beta, const float* mean_invstd, float* y, long M,
                               int C, long HW, float slope, int y_nchw, hipStream_t stream);
int pesr_bn_lrelu_bwd_eval_launch(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean_invstd,
                                  float* dx, float* dgamma, float* dbeta, long M, int C, long HW, float slope, int dy_nchw, void* ws,
                                  size_t ws_bytes, hipStream_t stream);

size_t pesr_bn_bwd_bwd_ws_bytes(long M, int C);
int pesr_bn_bwd_bwd_launch(const float* z, const float* du, const float* g, const float* gamma, const float* mean_invstd, float* l_du,
                           float* l_z, float* l_gamma, long M, int C, void* ws, size_t ws_bytes, hipStream_t stream);

size_t pesr_linear_ws_bytes(int M, int N, long K);
int pesr_linear_fwd_launch(const float* x, const float* W, const float* b, float* y, int M, int N, long K, int act, float slope,
                           void* ws, size_t ws_bytes, hipStream_t stream);
int pesr_linear_dgrad_launch(const float* dy, const float* W, float* dx, int M, int N, long K, void* ws, size_t ws_bytes,
                             hipStream_t stream);
int pesr_linear_wgrad_launch(const float* dy, const float* x, float* dW, float* db, int M, int N, long K, int accumulate,
                             hipStream_t stream);

int pesr_loss_l1_tv_launch(const float* sr, const float* hr, float* grad, float* out2, int N, int H, int W, float g_l1, float g_tv,
                           void* ws, size_t ws_bytes, hipStream_t stream);
int pesr_loss_mse_launch(const float* a, const float* b, float* grad, float* out1, long n, float gscale, void* ws, size_t ws_bytes,
                         hipStream_t stream);
int pesr_gan_loss_launch(const float* pred_real, const float* pred_fake, int B, int gan, int side, int focal, float gamma, float scale,
                         float* out, float* d_real, float* d_fake, hipStream_t stream);
int pesr_adam_ema_launch(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float b1, float b2, float eps, int step,
                         float gscale, float decay, hipStream_t stream);
int pesr_adam_ema_dev_launch(float* p, const float* g, float* m, float* v, float* ema, long n, float* state, float b1, float b2, float eps,
                             float gscale, float decay, hipStream_t stream);
int pesr_adam_dev_launch(float* p, const float* g, float* m, float* v, long n, float* state, float b1, float b2, float eps, float gscale,
                         hipStream_t stream);
int pesr_adam_launch(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps, int step,
                     float gscale, hipStream_t stream);

// dsum[col] = sum_k part[k*ncols + col] in double, fixed order (reduce.hip)
int pesr_reduce_rows_launch(const float* part, double* dsum, int nb, int ncols, hipStream_t stream);
// out[n] = (sum of part[n*per .. n*per + per - 1]) / count for n < N, float64, fixed order (reduce.hip): the second stage of the SSIM
// score, the SSIM loss, the LPIPS head and the Gram distance
int pesr_mean_partials_launch(const double* part, double* out, int N, long per, double count, hipStream_t stream);

// fixed-order split-K reduce of the direct wgrad kernel: slab [split][9][Cout][Cin] -> dw OIHW (+ bias partials -> db)
int pesr_wgrad_reduce_launch(const float* slab, float* dw, int split, int Cout, int Cin, float alpha, int ps, const float* bias_part,
                             int bias_rows, float* db, int accumulate, hipStream_t stream);
// transposed Winograd F(4,3) weight gradient (conv3x3_wgrad_wino4.hip); PESR_EINVAL for shapes it does not cover.  _side: images per
// 12-x-tile strip of its plan (1; 2 .. 6 for rows shorter than a strip), 0 where the plan does not cover the shape.  variant: a
// PESR_WGK_WINO4_* value.
size_t pesr_conv3x3_wgrad_wino4_ws_bytes(int N, int H, int W, int Cin, int Cout);
int pesr_conv3x3_wgrad_wino4_side_impl(int N, int H, int W, int Cin, int Cout);
int pesr_conv3x3_wgrad_wino4_launch(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                                    float alpha, int ps_in, int accumulate, int variant, void* ws, size_t ws_bytes, hipStream_t stream);
// transposed Winograd weight gradient (conv3x3_wgrad_wino.hip); the launch returns PESR_EINVAL for shapes it does not cover
size_t pesr_conv3x3_wgrad_wino_ws_bytes(int N, int H, int W, int Cin, int Cout);
int pesr_conv3x3_wgrad_wino_launch(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                                   float alpha, int ps_in, void* ws, size_t ws_bytes, hipStream_t stream);
// 1-D Winograd F(2,3) variant of the stride-1 conv (conv3x3_wino.hip)
int pesr_conv3x3_wino_supported_impl(int N, int H, int W, int Cin, int Cout);
int pesr_pack_conv3x3_wino_launch(const float* w, float* out, int O, int I, int mode, int ps, hipStream_t stream);
int pesr_conv3x3_wino_launch(const float* x, const float* wp, const float* bias, const float* skip, const float* mask, float* y,
                             int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps, int ps_in,
                             void* ws, size_t ws_bytes, hipStream_t stream);
// bf16-operand mode (conv3x3_bf16.hip, conv3x3_wgrad_bf16.hip): operands rounded to bf16, fp32 accumulation
int pesr_conv3x3_bf16_score_impl(int N, int H, int W, int Cin, int Cout, int min_wgs);
int pesr_pack_conv3x3_bf16_launch(const float* w, void* out, int O, int I, int mode, int ps, hipStream_t stream);
int pesr_conv3x3_bf16_launch(const float* x, const void* wp, const float* bias, const float* skip, const float* mask, float* y,
                             int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps, int ps_in,
                             hipStream_t stream);
// split-bf16 mode (conv3x3_bf16x3.hip): every operand as hi + lo bf16 terms, three products, fp32 accumulation
int pesr_conv3x3_bf16x3_score_impl(int N, int H, int W, int Cin, int Cout, int min_wgs);
int pesr_pack_conv3x3_bf16x3_launch(const float* w, void* out, int O, int I, int mode, int ps, hipStream_t stream);
int pesr_conv3x3_bf16x3_launch(const float* x, const void* wp, const float* bias, const float* skip, const float* mask, float* y,
                               int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps, int ps_in,
                               hipStream_t stream);
int pesr_conv3x3_bf16_s2_score_impl(int N, int H, int W, int Cin, int Cout, int min_wgs);
int pesr_conv3x3_bf16_s2_launch(const float* x, const void* wp, const float* bias, const float* skip, const float* mask, float* y,
                                int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, hipStream_t stream);
int pesr_conv3x3_bf16_s2_dgrad_score_impl(int N, int H, int W, int Cout_fwd, int Cin_fwd, int min_wgs);
int pesr_conv3x3_bf16_s2_dgrad_launch(const float* dy, const void* wp, const float* mask, const float* skip, float* dx, int N, int H, int W,
                                      int Cout_fwd, int Cin_fwd, float alpha, hipStream_t stream);
size_t pesr_conv3x3_wgrad_bf16_ws_bytes(int N, int H, int W, int Cin, int Cout);
int pesr_conv3x3_wgrad_bf16_launch(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                                   float alpha, int ps_in, int accumulate, void* ws, size_t ws_bytes, hipStream_t stream);

// 1-D Winograd F(4,3) variant (conv3x3_wino4.hip): half of the direct conv's multiplies
int pesr_conv3x3_wino4_score_impl(int N, int H, int W, int Cin, int Cout, int allow_split);
int pesr_pack_conv3x3_wino4_launch(const float* w, float* out, int O, int I, int mode, int ps, hipStream_t stream);
int pesr_conv3x3_wino4_launch(const float* x, const float* wp, const float* bias, const float* skip, const float* mask, float* y,
                              int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps, int ps_in,
                              void* ws, size_t ws_bytes, hipStream_t stream, PesrBnFuseArgs* fuse = nullptr);
struct BnEpi;
long pesr_conv_splitk_finish_bn_rows(int C, int ksplit);
int pesr_conv_splitk_finish_bn_launch(const float* slab, const float* bias, float* y, long total, int C, int ksplit, float alpha, const BnEpi& bn,
                                      hipStream_t stream);
int pesr_conv_splitk_finish_launch(const float* slab, const float* bias, const float* skip, const float* mask, float* y, long total,
                                   int C, int ksplit, float alpha, int act, float slope, hipStream_t stream);
int pesr_conv_rgb_in_launch(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, int act,
                            float slope, hipStream_t stream);
int pesr_conv_rgb_out_fwd_launch(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, int act,
                                 float slope, hipStream_t stream);
int pesr_conv_rgb_in_dgrad_launch(const float* dy, const float* w, float* dx, int N, int H, int W, int C, hipStream_t stream);
// the same conv (no bias) leaving BatchNorm partial sums per workgroup: part[rows][2][C] (conv_rgb_in.hip)
int pesr_conv_rgb_in_stats_rows(int N, int H, int W, int C);
int pesr_conv_rgb_in_stats_launch(const float* x, const float* w, float* y, float* part, int N, int H, int W, int C, hipStream_t stream);
int pesr_conv_rgb_out_dgrad_launch(const float* dy, const float* w, float* dx, int N, int H, int W, int C, hipStream_t stream);

int pesr_conv_kxk_fwd_launch(const float* x, const float* w, const float* b, float* y, int N, int H, int W, int Cin, int Cout, int k, int s,
                             hipStream_t stream);
int pesr_conv_kxk_dgrad_launch(const float* dy, const float* w, float* dx, int N, int H, int W, int Cin, int Cout, int k, int s,
                               hipStream_t stream);
int pesr_conv_kxk_wgrad_launch(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout, int k, int s,
                               hipStream_t stream);

size_t pesr_spectral_norm_ws_bytes(int O, int K);
int pesr_spectral_norm_fwd_launch(const float* W, float* u, float* v, float* w_hat, float* sigma, int O, int K, int update, float eps,
                                  void* ws, size_t ws_bytes, hipStream_t stream);
int pesr_spectral_norm_bwd_launch(const float* G, const float* w_hat, const float* u, const float* v, const float* sigma, float* dW, int O,
                                  int K, int accumulate, void* ws, size_t ws_bytes, hipStream_t stream);

int pesr_crop_augment_launch(const unsigned char* pool, const long long* desc, float* out, int B, int P, int nhwc, hipStream_t stream);

// bicubic resize of a pool of uint8 HWC images, one pass along one axis (resize.hip)
int pesr_imresize_u8_pass_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev,
                                 int n_images, int axis, int s, int up, const double* weights_host, hipStream_t stream);

// classical degradation (blur, subsample, noise) of windows of a pool of uint8 HWC images (degrade.hip)
int pesr_degrade_u8_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n,
                           int s, int K, const double* bank_dev, int n_kernels, hipStream_t stream);

// JPEG round trip (colour, chroma subsampling, 8 x 8 DCT, quantisation and back) of windows of a pool of uint8 HWC images (jpeg.hip)
size_t pesr_jpeg_workspace_bytes_host(const long long* desc_host, int n, int chroma);
int pesr_jpeg_u8_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n,
                        int chroma, const double* dct_dev, const double* quant_dev, void* ws, size_t ws_bytes, hipStream_t stream);

// resize of windows of a pool of uint8 HWC images from any size to any size, one pass (axis 0: height, 1: width) (resize_to.hip)
int pesr_resize_to_u8_pass_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev,
                                  int n, int axis, const void* tables_dev, long table_words, hipStream_t stream);

int pesr_psnr_y_launch(const float* a, const float* b, double* out2, int H, int W, int a_nhwc, int b_nhwc, void* ws, size_t ws_bytes,
                       hipStream_t stream);

// SSIM on the Y channel with a border shave (ssim.hip, docs/modes.md section 4g)
int pesr_ssim_y_launch(const float* a, const float* b, double* out, int N, int H, int W, int a_nhwc, int b_nhwc, int shave,
                       double* map, void* ws, size_t ws_bytes, hipStream_t stream);

// SSIM-Y on the unquantised luma as a training loss, and its gradient with respect to a (ssim.hip, docs/modes.md section 4p)
int pesr_ssim_loss_fwd_launch(const float* a, const float* b, double* score, int N, int H, int W, int a_nhwc, int b_nhwc, double* coef,
                              void* ws, size_t ws_bytes, hipStream_t stream);
int pesr_ssim_loss_bwd_launch(const float* a, const float* b, const double* coef, const double* g, float* ga, int N, int H, int W,
                              int a_nhwc, int b_nhwc, hipStream_t stream);

// Texture loss: patch-wise Gram matrices of NHWC features, their squared distance, the gradient (gram.hip, docs/modes.md section 4q)
int pesr_gram_splits_host(int N, int H, int W, int C, int ph, int pw);
size_t pesr_gram_workspace_bytes_host(int N, int H, int W, int C, int ph, int pw);
size_t pesr_gram_loss_workspace_bytes_host(int N, int P, int C);
int pesr_gram_fwd_launch(const float* f, float* G, int N, int H, int W, int C, int ph, int pw, void* ws, size_t ws_bytes,
                         hipStream_t stream);
int pesr_gram_loss_launch(const float* ga, const float* gb, double* t, float* dg, int N, int P, int C, void* ws, size_t ws_bytes,
                          hipStream_t stream);
int pesr_gram_bwd_launch(const float* f, const float* dg, const double* g, float* gf, int N, int H, int W, int C, int ph, int pw,
                         hipStream_t stream);

// Contextual loss: normalised points, their distances with row minima, CX and -log CX, the gradient (cx.hip, docs/modes.md section 4r)
int pesr_cx_row_blocks_host(int N, int P, int C);
int pesr_cx_col_pieces_host(int N, int P, int C);
size_t pesr_cx_workspace_bytes_host(int N, int P, int C);
size_t pesr_cx_saved_bytes_host(int N, int P, int C);
int pesr_cx_normalize_launch(const float* fa, const float* fb, float* mu, float* xh, float* yh, float* inv, int N, int P, int C,
                             hipStream_t stream);
int pesr_cx_dist_launch(const float* xh, const float* yh, float* D, float* m, int* b, int N, int P, int C, hipStream_t stream);
int pesr_cx_fwd_launch(const float* D, const float* m, double h, float* S, int* a, float* M, double* CX, double* L, int N, int P, int C,
                       void* ws, size_t ws_bytes, hipStream_t stream);
int pesr_cx_bwd_launch(const float* D, const float* m, const int* b, const float* S, const int* a, const float* M, const double* CX,
                       const double* gL, const float* xh, const float* yh, const float* inv, double h, float* gf, float* e_out,
                       float* gxh_out, int N, int P, int C, void* ws, size_t ws_bytes, hipStream_t stream);

// NIQE block statistics: luma, crop, two scales, MSCN maps, 26 sums per block and scale (niqe.hip)
int pesr_niqe_stats_launch(const float* img, int N, int H, int W, int nhwc, int shave, int B, int luma, double* stats, double* mscn1,
                           double* mscn2, void* ws, size_t ws_bytes, hipStream_t stream);

// LPIPS head of one tapped layer: unit-normalise two feature maps, weighted squared difference, mean per image pair (lpips.hip)
int pesr_lpips_layer_launch(const float* feat, const float* w, double* out, int N, int H, int W, int C, double* map, void* ws,
                            size_t ws_bytes, hipStream_t stream);
// ... with fa and fb as two base pointers, and its gradient with respect to fa (docs/modes.md section 4o)
int pesr_lpips_layer2_launch(const float* fa, const float* fb, const float* w, double* out, int N, int H, int W, int C, double* map,
                             void* ws, size_t ws_bytes, hipStream_t stream);
int pesr_lpips_layer_bwd_launch(const float* fa, const float* fb, const float* w, const double* g, float* ga, int N, int H, int W, int C,
                                hipStream_t stream);

// DISTS (dists.hip): the L2 pooling of the trunk, and the head of one stage (per-channel statistics of two feature maps -> S1, S2)
long pesr_l2pool_blocks_of(int N, int H, int W, int C);
int pesr_l2pool_fwd_launch(const float* x, float* y, int N, int H, int W, int C, hipStream_t stream);
long pesr_dists_pixel_blocks_of(int N, long P, int C);
size_t pesr_dists_ws_bytes(int N, long P, int C);
int pesr_dists_layer_launch(const float* feat, const double* alpha, const double* beta, double* out, int N, int H, int W, int C,
                            double* stats, void* ws, size_t ws_bytes, hipStream_t stream);

// channel attention of a residual block (channel_attention.hip): the two pixel sums (gy null: of t; else of gy * t) with their fixed-order
// second stage, the two apply passes (x: forward, dm: backward - exactly one of them), the gate forward and backward
int pesr_ca_pool_partials_of(int N, long HW, int C);
size_t pesr_ca_ws_bytes(int N, long HW, int C, int R);
int pesr_ca_sum_launch(const float* t, const float* gy, float* out, int N, long HW, int C, double scale, void* ws, size_t ws_bytes,
                       hipStream_t stream);
int pesr_ca_apply_launch(const float* in, const float* x, const float* s, const float* dm, float* out, int N, long HW, int C, float a,
                         hipStream_t stream);
int pesr_ca_gate_fwd_launch(const float* m, const float* W1, const float* B1, const float* W2, const float* B2, float* h, float* s, int N,
                            int C, int R, hipStream_t stream);
int pesr_ca_gate_bwd_launch(const float* ds, const float* s, const float* h, const float* m, const float* W1, const float* W2, float* dm,
                            float* dW1, float* dB1, float* dW2, float* dB2, int N, int C, int R, void* ws, size_t ws_bytes,
                            hipStream_t stream);

// the U-Net discriminator's kernels: bilinear x2 and its adjoint (upsample2x.hip), the GAN loss of a logit map (loss.hip), the 3 x 3 conv
// from C channels to one (conv_c1.hip)
int pesr_bilinear_up2_fwd_launch(const float* a, const float* b, float* y, int N, int H, int W, int C, hipStream_t stream);
int pesr_bilinear_up2_bwd_launch(const float* gy, float* gx, int N, int H, int W, int C, hipStream_t stream);
size_t pesr_gan_loss_map_ws_bytes(long n);
int pesr_gan_loss_map_launch(const float* pred_real, const float* pred_fake, long n, int gan, int side, int focal, float gamma, float scale,
                             float* out, float* d_real, float* d_fake, void* ws, size_t ws_bytes, hipStream_t stream);
size_t pesr_conv3x3_c1_wgrad_ws_bytes(int N, int H, int W, int C);
int pesr_conv3x3_c1_fwd_launch(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, hipStream_t stream);
int pesr_conv3x3_c1_dgrad_launch(const float* dy, const float* w, float* dx, int N, int H, int W, int C, hipStream_t stream);
int pesr_conv3x3_c1_wgrad_launch(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int C, float alpha, void* ws,
                                 size_t ws_bytes, hipStream_t stream);

// window self-attention of the Generator's attention blocks (window_attention.hip): 8 x 8 windows, heads of 32 channels
int pesr_window_attention_fwd_launch(const float* qkv, float* out, int N, int H, int W, int D, int shift, hipStream_t stream);
int pesr_window_attention_bwd_launch(const float* qkv, const float* dout, float* dqkv, int N, int H, int W, int D, int shift,
                                     hipStream_t stream);

// LayerNorm over the channels of each pixel (layernorm.hip), x [P][C], stats [P][2] = (mean, rstd); _partials_of: the workgroups of a
// launch = the rows of the backward's [rows][2 C] workspace (0: a shape the kernels do not take)
int pesr_layernorm_partials_of(long P, int C);
size_t pesr_layernorm_ws_bytes(long P, int C);
int pesr_layernorm_fwd_launch(const float* x, const float* gamma, const float* beta, float* y, float* stats, long P, int C, float eps,
                              hipStream_t stream);
int pesr_layernorm_bwd_launch(const float* x, const float* gamma, const float* stats, const float* dy, float* dx, float* dgamma,
                              float* dbeta, void* ws, long P, int C, hipStream_t stream);

// backward of the upsampler's tail (conv C -> 4C, PixelShuffle(2), conv C -> 3) as one virtual C -> 64 conv (upsample_tail.hip)
int pesr_upsample_tail_gather_launch(const float* g, float* gw, int N, int H, int W, hipStream_t stream);
int pesr_upsample_tail_compose_launch(const float* w2, const float* w4, float* weff, int C, hipStream_t stream);
int pesr_upsample_tail_chain_launch(const float* w2, const float* b2, const float* w4, const float* S, const float* T, float* dw2,
                                    float* db2, float* dw4, float* db4, int C, int accumulate, hipStream_t stream);

// tiled inference: tiles of one image -> a batch, and a batch's outputs -> the owned pixels of the image (tile.hip)
int pesr_tile_gather_launch(const void* src, int src_u8, int H, int W, float* dst, const int* desc_host, const int* desc_dev, int n,
                            int oh, int ow, hipStream_t stream);
int pesr_tile_scatter_launch(const float* t_lo, const float* t_hi, int t_nhwc, const float* p, int p_nhwc, float wa, float wb,
                             const int* desc_host, const int* desc_dev, int n, int E, int th, int tw, int s, int H, int W,
                             float* out_f32, unsigned char* out_u8, hipStream_t stream);
