// extern "C" surface of libpesr_hip.so (declared in include/pesr_hip.h).  Thin, exception-free
// wrappers over the per-family launchers; no torch types cross this boundary.
#include "common.h"
#include "launchers.h"
#include "../../include/pesr_hip.h"

static inline int pad16(int c) { return (c + 15) / 16 * 16; }
// "n" channel padding of the packed weights: <= 16 channels (the C -> 3 layers) pad to 16, everything else to a multiple of 64
static inline int pad64(int c) { return c <= 16 ? 16 : (c + 63) / 64 * 64; }

PESR_API int pesr_abi_version(void) { return 20; }

PESR_API int pesr_pack_conv3x3(const float* w, float* out, int O, int I, int mode, int ps, void* stream) {
    return pesr_pack_conv3x3_launch(w, out, O, I, mode, ps, (hipStream_t)stream);
}
PESR_API int pesr_pack_conv3x3_batched(const long long* desc, int count, void* stream) {
    return pesr_pack_conv3x3_batched_launch(desc, count, (hipStream_t)stream);
}
PESR_API int pesr_pack_bias_ps(const float* b, float* out, int O, void* stream) {
    return pesr_pack_bias_ps_launch(b, out, O, (hipStream_t)stream);
}

PESR_API int pesr_conv3x3_fwd(const float* x, const float* w_packed, const float* bias, const float* skip, const float* mask,
                              float* y, int N, int H, int W, int Cin, int Cout, int stride, float alpha, int act,
                              float slope, int ps_out, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_conv3x3_launch(x, w_packed, bias, skip, mask, y, N, H, W, pad16(Cin), pad64(Cout), stride, alpha, act, slope,
                               ps_out, 0, 0, Cin, Cout, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_conv3x3_dgrad(const float* dy, const float* w_packed_dgrad, const float* mask, const float* skip, float* dx,
                                int N, int H, int W, int Cin, int Cout, int stride, float alpha, int ps_in, void* workspace,
                                size_t ws_bytes, void* stream) {
    if (stride == 1)  // a stride-1 conv over dy with Cin/Cout swapped and the taps flipped
        return pesr_conv3x3_launch(dy, w_packed_dgrad, nullptr, skip, mask, dx, N, H, W, pad16(Cout), pad64(Cin), 1, alpha,
                                   PESR_ACT_NONE, 0.f, 0, ps_in, 1, Cout, Cin, workspace, ws_bytes, (hipStream_t)stream);
    if (stride == 2 && !ps_in && !skip)
        return pesr_conv3x3_s2_dgrad_launch(dy, w_packed_dgrad, mask, dx, N, H, W, Cout, Cin, alpha, (hipStream_t)stream);
    return PESR_EINVAL;
}

// split-K scratch for layers whose tiles cannot fill the chip: up to 8 partial copies of a (small) output
PESR_API size_t pesr_conv3x3_workspace_bytes(int N, int OH, int OW, int Cout) {
    const long tiles = ((long)N * OH * OW + 143) / 144 * ((Cout + 63) / 64);
    return tiles < 640 ? (size_t)8 * N * OH * OW * Cout * sizeof(float) : 0;
}

// ---- convs whose epilogue leaves BatchNorm sums (round 6, ABI 18; common.h BnEpi) ------------------------------------------------
static PesrBnFuseArgs fuse_args(const PesrBnFuse* f, int dry) {
    PesrBnFuseArgs a{};
    a.dry = dry;
    if (f) { a.mode = f->mode; a.rows = f->rows; a.part = f->part; a.z = f->z; a.mean_invstd = f->mean_invstd; a.gamma = f->gamma; a.beta = f->beta; a.slope = f->slope; }
    return a;
}
PESR_API long pesr_conv3x3_bn_rows(int which, int N, int H, int W, int Cin, int Cout, int stride) {
    PesrBnFuseArgs a = fuse_args(nullptr, 1);
    int rc = PESR_EINVAL;
    // the planners decide split-K from the workspace the caller would pass: the same sizes as ops.py / pesr_conv3x3_workspace_bytes
    if (which == 0) {
        const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
        const size_t wsb = pesr_conv3x3_workspace_bytes(N, OH, OW, Cout);
        rc = pesr_conv3x3_launch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N, H, W, pad16(Cin), pad64(Cout), stride, 1.f, PESR_ACT_NONE, 0.f,
                                 0, 0, 0, Cin, Cout, wsb ? (void*)8 : nullptr, wsb, nullptr, &a);
    } else if (which == 1) {
        if (stride == 1) {
            const size_t wsb = pesr_conv3x3_workspace_bytes(N, H, W, Cin);
            rc = pesr_conv3x3_launch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N, H, W, pad16(Cout), pad64(Cin), 1, 1.f, PESR_ACT_NONE, 0.f, 0, 0,
                                     1, Cout, Cin, wsb ? (void*)8 : nullptr, wsb, nullptr, &a);
        } else if (stride == 2) {
            rc = pesr_conv3x3_s2_dgrad_launch(nullptr, nullptr, nullptr, nullptr, N, H, W, Cout, Cin, 1.f, nullptr, &a);
        }
    } else if (which == 2) {
        const size_t wsb = pesr_conv3x3_workspace_bytes(N, H, W, Cout);
        rc = pesr_conv3x3_wino4_launch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N, H, W, Cin, Cout, 1.f, PESR_ACT_NONE, 0.f, 0, 0,
                                       wsb ? (void*)8 : nullptr, wsb, nullptr, &a);
    }
    return rc ? 0 : a.rows_out;
}
PESR_API int pesr_conv3x3_fwd_bn(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                                 int stride, void* workspace, size_t ws_bytes, const PesrBnFuse* fuse, void* stream) {
    if (!fuse) return PESR_EINVAL;
    PesrBnFuseArgs a = fuse_args(fuse, 0);
    return pesr_conv3x3_launch(x, w_packed, bias, nullptr, nullptr, y, N, H, W, pad16(Cin), pad64(Cout), stride, 1.f, PESR_ACT_NONE, 0.f, 0, 0, 0, Cin,
                               Cout, workspace, ws_bytes, (hipStream_t)stream, &a);
}
PESR_API int pesr_conv3x3_dgrad_bn(const float* dy, const float* w_packed_dgrad, float* dx, int N, int H, int W, int Cin, int Cout, int stride,
                                   void* workspace, size_t ws_bytes, const PesrBnFuse* fuse, void* stream) {
    if (!fuse) return PESR_EINVAL;
    PesrBnFuseArgs a = fuse_args(fuse, 0);
    if (stride == 1)
        return pesr_conv3x3_launch(dy, w_packed_dgrad, nullptr, nullptr, nullptr, dx, N, H, W, pad16(Cout), pad64(Cin), 1, 1.f, PESR_ACT_NONE, 0.f, 0, 0,
                                   1, Cout, Cin, workspace, ws_bytes, (hipStream_t)stream, &a);
    if (stride == 2) return pesr_conv3x3_s2_dgrad_launch(dy, w_packed_dgrad, nullptr, dx, N, H, W, Cout, Cin, 1.f, (hipStream_t)stream, &a);
    return PESR_EINVAL;
}
PESR_API int pesr_conv3x3_wino4_bn(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                                   void* workspace, size_t ws_bytes, const PesrBnFuse* fuse, void* stream) {
    if (!fuse) return PESR_EINVAL;
    PesrBnFuseArgs a = fuse_args(fuse, 0);
    return pesr_conv3x3_wino4_launch(x, w_packed, bias, nullptr, nullptr, y, N, H, W, Cin, Cout, 1.f, PESR_ACT_NONE, 0.f, 0, 0, workspace, ws_bytes,
                                     (hipStream_t)stream, &a);
}
PESR_API int pesr_bn_finalize(const float* part, int rows, int C, long M, float eps, float momentum, float* mean_invstd, float* running_mean,
                              float* running_var, long long* num_batches, void* stream) {
    return pesr_bn_finalize_launch(part, rows, C, M, eps, momentum, mean_invstd, running_mean, running_var, num_batches, (hipStream_t)stream);
}
PESR_API int pesr_bn_lrelu_bwd_fused(const float* z, const float* g_masked, const float* part, int rows, const float* gamma, const float* beta,
                                     const float* mean_invstd, float* dz, float* dgamma, float* dbeta, int N, int H, int W, int C, int accumulate,
                                     void* workspace, size_t ws_bytes, void* stream) {
    return pesr_bn_lrelu_bwd_fused_launch(z, g_masked, part, rows, gamma, beta, mean_invstd, dz, dgamma, dbeta, (long)N * H * W, C, (long)H * W,
                                          accumulate, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API size_t pesr_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int stride, int algo) {
    return pesr_conv3x3_wgrad_ws_bytes(N, H, W, Cin, Cout, stride, algo);
}
PESR_API int pesr_conv3x3_wgrad_kernel(int N, int H, int W, int Cin, int Cout, int stride, int ps_in, int algo, int accumulate) {
    return pesr_conv3x3_wgrad_kernel_impl(N, H, W, Cin, Cout, stride, ps_in, algo, accumulate, (size_t)-1);
}
PESR_API int pesr_conv3x3_wgrad_wino4_side(int N, int H, int W, int Cin, int Cout) { return pesr_conv3x3_wgrad_wino4_side_impl(N, H, W, Cin, Cout); }
PESR_API int pesr_conv3x3_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                                int stride, float alpha, int ps_in, int algo, int accumulate, void* workspace, size_t ws_bytes,
                                void* stream) {
    return pesr_conv3x3_wgrad_launch(x, dy, dw, db, N, H, W, Cin, Cout, stride, alpha, ps_in, algo, accumulate, workspace, ws_bytes,
                                     (hipStream_t)stream);
}

PESR_API size_t pesr_conv3x3_wgrad_rgb_workspace_bytes(int N, int H, int W, int C) {
    return pesr_conv3x3_wgrad_rgb_ws_bytes(N, H, W, C);
}
PESR_API int pesr_conv3x3_wgrad_rgb(const float* a, const float* b3, float* dw, float* db, int N, int H, int W, int C, int mode,
                                    float alpha, int accumulate, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_conv3x3_wgrad_rgb_launch(a, b3, dw, db, N, H, W, C, mode, alpha, accumulate, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_meanshift_fwd(const float* x, const float* w, const float* b, float* y, int N, int H, int W, int x_nchw,
                                int y_nchw, void* stream) {
    const long HW = (long)H * W;
    const long xsn = 3 * HW, xsc = x_nchw ? HW : 1, xsp = x_nchw ? 1 : 3;
    const long ysn = 3 * HW, ysc = y_nchw ? HW : 1, ysp = y_nchw ? 1 : 3;
    return pesr_meanshift_fwd_launch(x, w, b, y, N, H, W, xsn, xsc, xsp, ysn, ysc, ysp, (hipStream_t)stream);
}
PESR_API int pesr_meanshift_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, int N, int H,
                                int W, int x_nchw, void* workspace, size_t ws_bytes, void* stream) {
    const long HW = (long)H * W;
    const long xsn = 3 * HW, xsc = x_nchw ? HW : 1, xsp = x_nchw ? 1 : 3;
    return pesr_meanshift_bwd_launch(dy, x, w, dx, dw, db, N, H, W, xsn, xsc, xsp, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_pixel_shuffle_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream) {
    return pesr_pixel_shuffle_launch(x, y, N, H, W, C, 0, (hipStream_t)stream);
}
PESR_API int pesr_pixel_shuffle_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream) {
    return pesr_pixel_shuffle_launch(dy, dx, N, H, W, C, 1, (hipStream_t)stream);
}
PESR_API int pesr_pixel_shuffle_r_fwd(const float* x, float* y, int N, int H, int W, int C, int r, void* stream) {
    return pesr_pixel_shuffle_r_launch(x, y, N, H, W, C, r, 0, (hipStream_t)stream);
}
PESR_API int pesr_pixel_shuffle_r_bwd(const float* dy, float* dx, int N, int H, int W, int C, int r, void* stream) {
    return pesr_pixel_shuffle_r_launch(dy, dx, N, H, W, C, r, 1, (hipStream_t)stream);
}
PESR_API int pesr_relu_mask(const float* g, const float* ref, const float* add, float* out, long n, float alpha, float slope,
                            void* stream) {
    return pesr_relu_mask_launch(g, ref, add, out, n, alpha, slope, (hipStream_t)stream);
}
PESR_API int pesr_maxpool2x2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream) {
    return pesr_maxpool2x2_fwd_launch(x, y, N, H, W, C, (hipStream_t)stream);
}
PESR_API int pesr_maxpool2x2_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C, int relu_in, void* stream) {
    return pesr_maxpool2x2_bwd_launch(x, dy, dx, N, H, W, C, relu_in, (hipStream_t)stream);
}

PESR_API size_t pesr_bn_workspace_bytes(long M, int C) { return pesr_bn_ws_bytes(M, C); }
PESR_API int pesr_bn_lrelu_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean_invstd,
                               float* running_mean, float* running_var, long long* num_batches, int N, int H, int W, int C,
                               float eps, float momentum, float slope, int y_nchw, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_bn_lrelu_fwd_launch(x, gamma, beta, y, mean_invstd, running_mean, running_var, num_batches, (long)N * H * W, C,
                                    (long)H * W, eps, momentum, slope, y_nchw, workspace, ws_bytes, (hipStream_t)stream);
}
PESR_API size_t pesr_conv3x3_rgb_bn_workspace_bytes(int N, int H, int W, int C) { return pesr_conv_rgb_bn_ws_bytes(N, H, W, C); }
PESR_API int pesr_conv3x3_rgb_bn_lrelu_fwd(const float* x, const float* w, float* z, const float* gamma, const float* beta, float* y,
                                           float* mean_invstd, float* running_mean, float* running_var, long long* num_batches, int N,
                                           int H, int W, int C, float eps, float momentum, float slope, int y_nchw, void* workspace,
                                           size_t ws_bytes, void* stream) {
    return pesr_conv_rgb_bn_lrelu_fwd_launch(x, w, z, gamma, beta, y, mean_invstd, running_mean, running_var, num_batches, N, H, W, C, eps,
                                             momentum, slope, y_nchw, workspace, ws_bytes, (hipStream_t)stream);
}
PESR_API int pesr_bn_lrelu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean_invstd,
                               float* dx, float* dgamma, float* dbeta, int N, int H, int W, int C, float slope, int dy_nchw,
                               int accumulate, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_bn_lrelu_bwd_launch(x, dy, gamma, beta, mean_invstd, dx, dgamma, dbeta, (long)N * H * W, C, (long)H * W, slope,
                                    dy_nchw, accumulate, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_bn_lrelu_eval_fwd(const float* x, const float* gamma, const float* beta, const float* mean_invstd, float* y, int N,
                                    int H, int W, int C, float slope, int y_nchw, void* stream) {
    return pesr_bn_lrelu_apply_launch(x, gamma, beta, mean_invstd, y, (long)N * H * W, C, (long)H * W, slope, y_nchw, (hipStream_t)stream);
}
PESR_API int pesr_bn_lrelu_eval_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean_invstd,
                                    float* dx, float* dgamma, float* dbeta, int N, int H, int W, int C, float slope, int dy_nchw,
                                    void* workspace, size_t ws_bytes, void* stream) {
    return pesr_bn_lrelu_bwd_eval_launch(x, dy, gamma, beta, mean_invstd, dx, dgamma, dbeta, (long)N * H * W, C, (long)H * W, slope,
                                         dy_nchw, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API size_t pesr_bn_bwd_bwd_workspace_bytes(long M, int C) { return pesr_bn_bwd_bwd_ws_bytes(M, C); }
PESR_API int pesr_bn_bwd_bwd(const float* z, const float* du, const float* g, const float* gamma, const float* mean_invstd, float* l_du,
                             float* l_z, float* l_gamma, int N, int H, int W, int C, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_bn_bwd_bwd_launch(z, du, g, gamma, mean_invstd, l_du, l_z, l_gamma, (long)N * H * W, C, workspace, ws_bytes,
                                  (hipStream_t)stream);
}

PESR_API size_t pesr_linear_workspace_bytes(int M, int N, long K) { return pesr_linear_ws_bytes(M, N, K); }
PESR_API int pesr_linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int N, long K, int act, float slope,
                             void* workspace, size_t ws_bytes, void* stream) {
    return pesr_linear_fwd_launch(x, w, b, y, M, N, K, act, slope, workspace, ws_bytes, (hipStream_t)stream);
}
PESR_API int pesr_linear_dgrad(const float* dy, const float* w, float* dx, int M, int N, long K, void* workspace, size_t ws_bytes,
                               void* stream) {
    return pesr_linear_dgrad_launch(dy, w, dx, M, N, K, workspace, ws_bytes, (hipStream_t)stream);
}
PESR_API int pesr_linear_wgrad(const float* dy, const float* x, float* dw, float* db, int M, int N, long K, int accumulate,
                               void* stream) {
    return pesr_linear_wgrad_launch(dy, x, dw, db, M, N, K, accumulate, (hipStream_t)stream);
}

PESR_API int pesr_loss_l1_tv_fwd_bwd(const float* sr, const float* hr, float* grad, float* out2, int N, int H, int W, float g_l1,
                                     float g_tv, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_loss_l1_tv_launch(sr, hr, grad, out2, N, H, W, g_l1, g_tv, workspace, ws_bytes, (hipStream_t)stream);
}
PESR_API int pesr_mse_fwd_bwd(const float* a, const float* b, float* grad, float* out1, long n, float gscale, void* workspace,
                              size_t ws_bytes, void* stream) {
    return pesr_loss_mse_launch(a, b, grad, out1, n, gscale, workspace, ws_bytes, (hipStream_t)stream);
}
PESR_API int pesr_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                            int step, float grad_scale, void* stream) {
    return pesr_adam_launch(p, g, m, v, n, lr, beta1, beta2, eps, step, grad_scale, (hipStream_t)stream);
}

PESR_API int pesr_adam_step_dev(float* p, const float* g, float* m, float* v, long n, float* state, float beta1, float beta2, float eps,
                                float grad_scale, void* stream) {
    return pesr_adam_dev_launch(p, g, m, v, n, state, beta1, beta2, eps, grad_scale, (hipStream_t)stream);
}

PESR_API int pesr_adam_ema_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                                int step, float grad_scale, float* ema, float ema_decay, void* stream) {
    return pesr_adam_ema_launch(p, g, m, v, ema, n, lr, beta1, beta2, eps, step, grad_scale, ema_decay, (hipStream_t)stream);
}

PESR_API int pesr_adam_ema_step_dev(float* p, const float* g, float* m, float* v, long n, float* state, float beta1, float beta2,
                                    float eps, float grad_scale, float* ema, float ema_decay, void* stream) {
    return pesr_adam_ema_dev_launch(p, g, m, v, ema, n, state, beta1, beta2, eps, grad_scale, ema_decay, (hipStream_t)stream);
}

PESR_API int pesr_conv3x3_rgb_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cout,
                                  int act, float slope, void* stream) {
    return pesr_conv_rgb_in_launch(x, w, bias, y, N, H, W, Cout, act, slope, (hipStream_t)stream);
}

PESR_API int pesr_conv3x3_rgb_out_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, int act,
                                      float slope, void* stream) {
    return pesr_conv_rgb_out_fwd_launch(x, w, bias, y, N, H, W, C, act, slope, (hipStream_t)stream);
}

PESR_API int pesr_conv3x3_rgb_in_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, void* stream) {
    return pesr_conv_rgb_in_dgrad_launch(dy, w, dx, N, H, W, C, (hipStream_t)stream);
}

PESR_API int pesr_conv3x3_rgb_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, void* stream) {
    return pesr_conv_rgb_out_dgrad_launch(dy, w, dx, N, H, W, C, (hipStream_t)stream);
}

PESR_API int pesr_conv3x3_wino_supported(int N, int H, int W, int Cin, int Cout) {
    return pesr_conv3x3_wino_supported_impl(N, H, W, Cin, Cout);
}
PESR_API int pesr_pack_conv3x3_wino(const float* w, float* w_packed, int Cout, int Cin, int mode, int ps, void* stream) {
    return pesr_pack_conv3x3_wino_launch(w, w_packed, Cout, Cin, mode, ps, (hipStream_t)stream);
}
PESR_API int pesr_conv3x3_wino(const float* x, const float* w_packed, const float* bias, const float* skip, const float* mask,
                               float* y, int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps_out,
                               int ps_in, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_conv3x3_wino_launch(x, w_packed, bias, skip, mask, y, N, H, W, Cin, Cout, alpha, act, slope, ps_out, ps_in,
                                    workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_conv3x3_wino4_score(int N, int H, int W, int Cin, int Cout, int allow_split) {
    return pesr_conv3x3_wino4_score_impl(N, H, W, Cin, Cout, allow_split);
}
PESR_API int pesr_pack_conv3x3_wino4(const float* w, float* w_packed, int Cout, int Cin, int mode, int ps, void* stream) {
    return pesr_pack_conv3x3_wino4_launch(w, w_packed, Cout, Cin, mode, ps, (hipStream_t)stream);
}
PESR_API int pesr_conv3x3_wino4(const float* x, const float* w_packed, const float* bias, const float* skip, const float* mask,
                                float* y, int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps_out,
                                int ps_in, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_conv3x3_wino4_launch(x, w_packed, bias, skip, mask, y, N, H, W, Cin, Cout, alpha, act, slope, ps_out, ps_in,
                                     workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_conv3x3_bf16_score(int N, int H, int W, int Cin, int Cout, int min_wgs) {
    return pesr_conv3x3_bf16_score_impl(N, H, W, Cin, Cout, min_wgs);
}
PESR_API int pesr_pack_conv3x3_bf16(const float* w, void* w_packed, int Cout, int Cin, int mode, int ps, void* stream) {
    return pesr_pack_conv3x3_bf16_launch(w, w_packed, Cout, Cin, mode, ps, (hipStream_t)stream);
}
PESR_API int pesr_conv3x3_bf16(const float* x, const void* w_packed, const float* bias, const float* skip, const float* mask,
                               float* y, int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps_out,
                               int ps_in, void* stream) {
    return pesr_conv3x3_bf16_launch(x, w_packed, bias, skip, mask, y, N, H, W, Cin, Cout, alpha, act, slope, ps_out, ps_in,
                                    (hipStream_t)stream);
}
PESR_API int pesr_conv3x3_bf16x3_score(int N, int H, int W, int Cin, int Cout, int min_wgs) {
    return pesr_conv3x3_bf16x3_score_impl(N, H, W, Cin, Cout, min_wgs);
}
PESR_API int pesr_pack_conv3x3_bf16x3(const float* w, void* w_packed, int Cout, int Cin, int mode, int ps, void* stream) {
    return pesr_pack_conv3x3_bf16x3_launch(w, w_packed, Cout, Cin, mode, ps, (hipStream_t)stream);
}
PESR_API int pesr_conv3x3_bf16x3(const float* x, const void* w_packed, const float* bias, const float* skip, const float* mask,
                                 float* y, int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps_out,
                                 int ps_in, void* stream) {
    return pesr_conv3x3_bf16x3_launch(x, w_packed, bias, skip, mask, y, N, H, W, Cin, Cout, alpha, act, slope, ps_out, ps_in,
                                      (hipStream_t)stream);
}
PESR_API int pesr_conv3x3_bf16_s2_score(int N, int H, int W, int Cin, int Cout, int min_wgs) {
    return pesr_conv3x3_bf16_s2_score_impl(N, H, W, Cin, Cout, min_wgs);
}
PESR_API int pesr_conv3x3_bf16_s2(const float* x, const void* w_packed, const float* bias, const float* skip, const float* mask,
                                  float* y, int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, void* stream) {
    return pesr_conv3x3_bf16_s2_launch(x, w_packed, bias, skip, mask, y, N, H, W, Cin, Cout, alpha, act, slope, (hipStream_t)stream);
}
PESR_API int pesr_conv3x3_bf16_s2_dgrad_score(int N, int H, int W, int Cout_fwd, int Cin_fwd, int min_wgs) {
    return pesr_conv3x3_bf16_s2_dgrad_score_impl(N, H, W, Cout_fwd, Cin_fwd, min_wgs);
}
PESR_API int pesr_conv3x3_bf16_s2_dgrad(const float* dy, const void* w_packed, const float* mask, const float* skip, float* dx, int N,
                                        int H, int W, int Cout_fwd, int Cin_fwd, float alpha, void* stream) {
    return pesr_conv3x3_bf16_s2_dgrad_launch(dy, w_packed, mask, skip, dx, N, H, W, Cout_fwd, Cin_fwd, alpha, (hipStream_t)stream);
}
PESR_API size_t pesr_conv3x3_wgrad_bf16_workspace_bytes(int N, int H, int W, int Cin, int Cout) {
    return pesr_conv3x3_wgrad_bf16_ws_bytes(N, H, W, Cin, Cout);
}
PESR_API int pesr_conv3x3_wgrad_bf16(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                                     float alpha, int ps_in, int accumulate, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_conv3x3_wgrad_bf16_launch(x, dy, dw, db, N, H, W, Cin, Cout, alpha, ps_in, accumulate, workspace, ws_bytes,
                                          (hipStream_t)stream);
}

PESR_API int pesr_crop_augment(const unsigned char* pool, const long long* desc, float* out, int B, int P, int nhwc, void* stream) {
    return pesr_crop_augment_launch(pool, desc, out, B, P, nhwc, (hipStream_t)stream);
}

PESR_API int pesr_imresize_u8_pass(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev,
                                   int n_images, int axis, int s, int up, const double* weights_host, void* stream) {
    return pesr_imresize_u8_pass_launch(src, dst, desc_host, desc_dev, n_images, axis, s, up, weights_host, (hipStream_t)stream);
}

PESR_API int pesr_degrade_u8(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n,
                             int s, int K, const double* bank_dev, int n_kernels, void* stream) {
    return pesr_degrade_u8_launch(src, dst, desc_host, desc_dev, n, s, K, bank_dev, n_kernels, (hipStream_t)stream);
}

PESR_API size_t pesr_jpeg_workspace_bytes(const long long* desc_host, int n, int chroma) {
    return pesr_jpeg_workspace_bytes_host(desc_host, n, chroma);
}

PESR_API int pesr_jpeg_u8(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n,
                          int chroma, const double* dct_dev, const double* quant_dev, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_jpeg_u8_launch(src, dst, desc_host, desc_dev, n, chroma, dct_dev, quant_dev, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_resize_to_u8_pass(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev,
                                    int n, int axis, const void* tables_dev, long table_words, void* stream) {
    return pesr_resize_to_u8_pass_launch(src, dst, desc_host, desc_dev, n, axis, tables_dev, table_words, (hipStream_t)stream);
}

PESR_API int pesr_psnr_y(const float* a, const float* b, double* out2, int H, int W, int a_nhwc, int b_nhwc, void* workspace,
                         size_t ws_bytes, void* stream) {
    return pesr_psnr_y_launch(a, b, out2, H, W, a_nhwc, b_nhwc, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_ssim_y(const float* a, const float* b, double* out, int N, int H, int W, int a_nhwc, int b_nhwc, int shave,
                         double* map_or_null, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_ssim_y_launch(a, b, out, N, H, W, a_nhwc, b_nhwc, shave, map_or_null, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_ssim_loss_fwd(const float* a, const float* b, double* score, int N, int H, int W, int a_nhwc, int b_nhwc,
                                double* coef_or_null, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_ssim_loss_fwd_launch(a, b, score, N, H, W, a_nhwc, b_nhwc, coef_or_null, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_ssim_loss_bwd(const float* a, const float* b, const double* coef, const double* g, float* ga, int N, int H, int W,
                                int a_nhwc, int b_nhwc, void* stream) {
    return pesr_ssim_loss_bwd_launch(a, b, coef, g, ga, N, H, W, a_nhwc, b_nhwc, (hipStream_t)stream);
}

PESR_API int pesr_gram_splits(int N, int H, int W, int C, int ph, int pw) { return pesr_gram_splits_host(N, H, W, C, ph, pw); }

PESR_API size_t pesr_gram_workspace_bytes(int N, int H, int W, int C, int ph, int pw) {
    return pesr_gram_workspace_bytes_host(N, H, W, C, ph, pw);
}

PESR_API size_t pesr_gram_loss_workspace_bytes(int N, int P, int C) { return pesr_gram_loss_workspace_bytes_host(N, P, C); }

PESR_API int pesr_gram_fwd(const float* f, float* G, int N, int H, int W, int C, int ph, int pw, void* workspace, size_t ws_bytes,
                           void* stream) {
    return pesr_gram_fwd_launch(f, G, N, H, W, C, ph, pw, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_gram_loss(const float* ga, const float* gb, double* t, float* dg_or_null, int N, int P, int C, void* workspace,
                            size_t ws_bytes, void* stream) {
    return pesr_gram_loss_launch(ga, gb, t, dg_or_null, N, P, C, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_gram_bwd(const float* f, const float* dg, const double* g, float* gf, int N, int H, int W, int C, int ph, int pw,
                           void* stream) {
    return pesr_gram_bwd_launch(f, dg, g, gf, N, H, W, C, ph, pw, (hipStream_t)stream);
}

PESR_API int pesr_cx_row_blocks(int N, int P, int C) { return pesr_cx_row_blocks_host(N, P, C); }

PESR_API int pesr_cx_col_pieces(int N, int P, int C) { return pesr_cx_col_pieces_host(N, P, C); }

PESR_API size_t pesr_cx_workspace_bytes(int N, int P, int C) { return pesr_cx_workspace_bytes_host(N, P, C); }

PESR_API size_t pesr_cx_saved_bytes(int N, int P, int C) { return pesr_cx_saved_bytes_host(N, P, C); }

PESR_API int pesr_cx_normalize(const float* fa, const float* fb, float* mu, float* xh, float* yh, float* inv, int N, int P, int C,
                               void* stream) {
    return pesr_cx_normalize_launch(fa, fb, mu, xh, yh, inv, N, P, C, (hipStream_t)stream);
}

PESR_API int pesr_cx_dist(const float* xh, const float* yh, float* D, float* m, int* b, int N, int P, int C, void* stream) {
    return pesr_cx_dist_launch(xh, yh, D, m, b, N, P, C, (hipStream_t)stream);
}

PESR_API int pesr_cx_fwd(const float* D, const float* m, double h, float* S, int* a, float* cmax, double* CX, double* L, int N, int P,
                         int C, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_cx_fwd_launch(D, m, h, S, a, cmax, CX, L, N, P, C, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_cx_bwd(const float* D, const float* m, const int* b, const float* S, const int* a, const float* cmax, const double* CX,
                         const double* gL, const float* xh, const float* yh, const float* inv, double h, float* gf, float* e_or_null,
                         float* gxh_or_null, int N, int P, int C, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_cx_bwd_launch(D, m, b, S, a, cmax, CX, gL, xh, yh, inv, h, gf, e_or_null, gxh_or_null, N, P, C, workspace, ws_bytes,
                              (hipStream_t)stream);
}

PESR_API int pesr_niqe_stats(const float* img, int N, int H, int W, int nhwc, int shave, int B, int luma, double* stats,
                             double* mscn1_or_null, double* mscn2_or_null, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_niqe_stats_launch(img, N, H, W, nhwc, shave, B, luma, stats, mscn1_or_null, mscn2_or_null, workspace, ws_bytes,
                                  (hipStream_t)stream);
}

PESR_API int pesr_lpips_layer(const float* feat, const float* w, double* out, int N, int H, int W, int C, double* map_or_null,
                              void* workspace, size_t ws_bytes, void* stream) {
    return pesr_lpips_layer_launch(feat, w, out, N, H, W, C, map_or_null, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_lpips_layer2(const float* fa, const float* fb, const float* w, double* out, int N, int H, int W, int C,
                               double* map_or_null, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_lpips_layer2_launch(fa, fb, w, out, N, H, W, C, map_or_null, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_lpips_layer_bwd(const float* fa, const float* fb, const float* w, const double* g, float* ga, int N, int H, int W,
                                  int C, void* stream) {
    return pesr_lpips_layer_bwd_launch(fa, fb, w, g, ga, N, H, W, C, (hipStream_t)stream);
}

PESR_API long pesr_l2pool_blocks(int N, int H, int W, int C) { return pesr_l2pool_blocks_of(N, H, W, C); }
PESR_API int pesr_l2pool_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream) {
    return pesr_l2pool_fwd_launch(x, y, N, H, W, C, (hipStream_t)stream);
}
PESR_API long pesr_dists_pixel_blocks(int N, long P, int C) { return pesr_dists_pixel_blocks_of(N, P, C); }
PESR_API size_t pesr_dists_workspace_bytes(int N, long P, int C) { return pesr_dists_ws_bytes(N, P, C); }
PESR_API int pesr_dists_layer(const float* feat, const double* alpha, const double* beta, double* out, int N, int H, int W, int C,
                              double* stats_or_null, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_dists_layer_launch(feat, alpha, beta, out, N, H, W, C, stats_or_null, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_ca_pool_partials(int N, long HW, int C) { return pesr_ca_pool_partials_of(N, HW, C); }
PESR_API size_t pesr_ca_workspace_bytes(int N, long HW, int C, int R) { return pesr_ca_ws_bytes(N, HW, C, R); }
PESR_API int pesr_ca_pool(const float* t, float* m, int N, long HW, int C, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_ca_sum_launch(t, nullptr, m, N, HW, C, HW > 0 ? 1.0 / (double)HW : 0.0, workspace, ws_bytes, (hipStream_t)stream);
}
PESR_API int pesr_ca_ds(const float* gy, const float* t, float* ds, int N, long HW, int C, float res_scale, void* workspace,
                        size_t ws_bytes, void* stream) {
    if (!gy) return PESR_EINVAL;
    return pesr_ca_sum_launch(t, gy, ds, N, HW, C, (double)res_scale, workspace, ws_bytes, (hipStream_t)stream);
}
PESR_API int pesr_ca_gate_fwd(const float* m, const float* w1, const float* b1, const float* w2, const float* b2, float* h, float* s,
                              int N, int C, int R, void* stream) {
    return pesr_ca_gate_fwd_launch(m, w1, b1, w2, b2, h, s, N, C, R, (hipStream_t)stream);
}
PESR_API int pesr_ca_apply_fwd(const float* x, const float* t, const float* s, float* y, int N, long HW, int C, float res_scale,
                               void* stream) {
    if (!x) return PESR_EINVAL;
    return pesr_ca_apply_launch(t, x, s, nullptr, y, N, HW, C, res_scale, (hipStream_t)stream);
}
PESR_API int pesr_ca_gate_bwd(const float* ds, const float* s, const float* h, const float* m, const float* w1, const float* w2,
                              float* dm, float* dw1, float* db1, float* dw2, float* db2, int N, int C, int R, void* workspace,
                              size_t ws_bytes, void* stream) {
    return pesr_ca_gate_bwd_launch(ds, s, h, m, w1, w2, dm, dw1, db1, dw2, db2, N, C, R, workspace, ws_bytes, (hipStream_t)stream);
}
PESR_API int pesr_ca_apply_bwd(const float* gy, const float* s, const float* dm, float* gt, int N, long HW, int C, float res_scale,
                               void* stream) {
    if (!dm) return PESR_EINVAL;
    return pesr_ca_apply_launch(gy, nullptr, s, dm, gt, N, HW, C, res_scale, (hipStream_t)stream);
}

PESR_API int pesr_bilinear_up2_fwd(const float* a, const float* b_or_null, float* y, int N, int H, int W, int C, void* stream) {
    return pesr_bilinear_up2_fwd_launch(a, b_or_null, y, N, H, W, C, (hipStream_t)stream);
}
PESR_API int pesr_bilinear_up2_bwd(const float* gy, float* gx, int N, int H, int W, int C, void* stream) {
    return pesr_bilinear_up2_bwd_launch(gy, gx, N, H, W, C, (hipStream_t)stream);
}
PESR_API size_t pesr_gan_loss_map_workspace_bytes(long n) { return pesr_gan_loss_map_ws_bytes(n); }
PESR_API int pesr_gan_loss_map(const float* pred_real, const float* pred_fake, long n, int gan_type, int side, int focal, float gamma,
                               float scale, float* out, float* d_real, float* d_fake, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_gan_loss_map_launch(pred_real, pred_fake, n, gan_type, side, focal, gamma, scale, out, d_real, d_fake, workspace, ws_bytes,
                                    (hipStream_t)stream);
}
PESR_API size_t pesr_conv3x3_c1_wgrad_workspace_bytes(int N, int H, int W, int C) { return pesr_conv3x3_c1_wgrad_ws_bytes(N, H, W, C); }
PESR_API int pesr_conv3x3_c1_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, void* stream) {
    return pesr_conv3x3_c1_fwd_launch(x, w, bias, y, N, H, W, C, (hipStream_t)stream);
}
PESR_API int pesr_conv3x3_c1_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, void* stream) {
    return pesr_conv3x3_c1_dgrad_launch(dy, w, dx, N, H, W, C, (hipStream_t)stream);
}
PESR_API int pesr_conv3x3_c1_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int C, float alpha,
                                   void* workspace, size_t ws_bytes, void* stream) {
    return pesr_conv3x3_c1_wgrad_launch(x, dy, dw, db, N, H, W, C, alpha, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_window_attention_fwd(const float* qkv, float* out, int N, int H, int W, int D, int shift, void* stream) {
    return pesr_window_attention_fwd_launch(qkv, out, N, H, W, D, shift, (hipStream_t)stream);
}
PESR_API int pesr_window_attention_bwd(const float* qkv, const float* dout, float* dqkv, int N, int H, int W, int D, int shift,
                                       void* stream) {
    return pesr_window_attention_bwd_launch(qkv, dout, dqkv, N, H, W, D, shift, (hipStream_t)stream);
}

PESR_API int pesr_layernorm_partials(long P, int C) { return pesr_layernorm_partials_of(P, C); }
PESR_API size_t pesr_layernorm_workspace_bytes(long P, int C) { return pesr_layernorm_ws_bytes(P, C); }
PESR_API int pesr_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stats, long P, int C, float eps,
                                void* stream) {
    return pesr_layernorm_fwd_launch(x, gamma, beta, y, stats, P, C, eps, (hipStream_t)stream);
}
PESR_API int pesr_layernorm_bwd(const float* x, const float* gamma, const float* stats, const float* dy, float* dx, float* dgamma,
                                float* dbeta, void* workspace, long P, int C, void* stream) {
    return pesr_layernorm_bwd_launch(x, gamma, stats, dy, dx, dgamma, dbeta, workspace, P, C, (hipStream_t)stream);
}

PESR_API int pesr_upsample_tail_gather(const float* g, float* gw, int N, int H, int W, void* stream) {
    return pesr_upsample_tail_gather_launch(g, gw, N, H, W, (hipStream_t)stream);
}
PESR_API int pesr_upsample_tail_compose(const float* w2, const float* w4, float* weff, int C, void* stream) {
    return pesr_upsample_tail_compose_launch(w2, w4, weff, C, (hipStream_t)stream);
}
PESR_API int pesr_upsample_tail_chain(const float* w2, const float* b2_or_null, const float* w4, const float* S, const float* T,
                                      float* dw2_or_null, float* db2_or_null, float* dw4_or_null, float* db4_or_null, int C,
                                      int accumulate, void* stream) {
    return pesr_upsample_tail_chain_launch(w2, b2_or_null, w4, S, T, dw2_or_null, db2_or_null, dw4_or_null, db4_or_null, C, accumulate,
                                           (hipStream_t)stream);
}

PESR_API int pesr_tile_gather(const void* src, int src_u8, int H, int W, float* dst, const int* desc_host, const int* desc_dev, int n,
                             int oh, int ow, void* stream) {
    return pesr_tile_gather_launch(src, src_u8, H, W, dst, desc_host, desc_dev, n, oh, ow, (hipStream_t)stream);
}

PESR_API int pesr_tile_scatter(const float* t_lo, const float* t_hi, int t_nhwc, const float* p_or_null, int p_nhwc, float wa, float wb,
                              const int* desc_host, const int* desc_dev, int n, int E, int th, int tw, int s, int H, int W,
                              float* out_f32_or_null, unsigned char* out_u8_or_null, void* stream) {
    return pesr_tile_scatter_launch(t_lo, t_hi, t_nhwc, p_or_null, p_nhwc, wa, wb, desc_host, desc_dev, n, E, th, tw, s, H, W,
                                    out_f32_or_null, out_u8_or_null, (hipStream_t)stream);
}

PESR_API size_t pesr_spectral_norm_workspace_bytes(int O, int K) { return pesr_spectral_norm_ws_bytes(O, K); }
PESR_API int pesr_spectral_norm_fwd(const float* w, float* u, float* v, float* w_hat, float* sigma, int O, int K, int update, float eps,
                                    void* workspace, size_t ws_bytes, void* stream) {
    return pesr_spectral_norm_fwd_launch(w, u, v, w_hat, sigma, O, K, update, eps, workspace, ws_bytes, (hipStream_t)stream);
}
PESR_API int pesr_spectral_norm_bwd(const float* g, const float* w_hat, const float* u, const float* v, const float* sigma, float* dw,
                                    int O, int K, int accumulate, void* workspace, size_t ws_bytes, void* stream) {
    return pesr_spectral_norm_bwd_launch(g, w_hat, u, v, sigma, dw, O, K, accumulate, workspace, ws_bytes, (hipStream_t)stream);
}

PESR_API int pesr_conv_kxk_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                               int k, int stride, void* stream) {
    return pesr_conv_kxk_fwd_launch(x, w, bias, y, N, H, W, Cin, Cout, k, stride, (hipStream_t)stream);
}
PESR_API int pesr_conv_kxk_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int Cin, int Cout, int k, int stride,
                                 void* stream) {
    return pesr_conv_kxk_dgrad_launch(dy, w, dx, N, H, W, Cin, Cout, k, stride, (hipStream_t)stream);
}
PESR_API int pesr_conv_kxk_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout, int k,
                                 int stride, void* stream) {
    return pesr_conv_kxk_wgrad_launch(x, dy, dw, db, N, H, W, Cin, Cout, k, stride, (hipStream_t)stream);
}

PESR_API int pesr_gan_loss_fwd_bwd(const float* pred_real, const float* pred_fake, int B, int gan_type, int side, int focal, float gamma,
                                   float scale, float* out, float* d_real, float* d_fake, void* stream) {
    return pesr_gan_loss_launch(pred_real, pred_fake, B, gan_type, side, focal, gamma, scale, out, d_real, d_fake, (hipStream_t)stream);
}
