/*
 * pesr_hip.h - C ABI of libpesr_hip.so: the MI355X (gfx950) kernels behind PESR's x4 SR GAN train step.
 *
 * The reference (thangvubk/PESR) has no FFI of its own: every kernel it runs is a PyTorch built-in
 * reached from model/basic.py, model/pesr.py, model/vgg.py, model/focal_loss.py and train.py.  Each
 * entry point below therefore names the ATen op / reference line it stands in for.  The Python side
 * (pesr_amd/_lib.py) binds these with ctypes; see INTEGRATION.md for the stub.
 *
 * Conventions
 *   - all tensors are fp32 device pointers owned by the caller (torch's caching allocator);
 *   - activations are NHWC ("channels_last" physical layout of a logical NCHW tensor);
 *   - 3x3 conv weights are passed PRE-PACKED (pesr_pack_conv3x3) - the nn.Module keeps OIHW;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant, and
 *     returns 0 on success, a positive hipError_t, or a negative PESR_E* code; nothing throws;
 *   - workspaces are caller-allocated; their byte sizes come from the *_workspace_bytes helpers.
 */
#ifndef PESR_HIP_H
#define PESR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PESR_OK 0
#define PESR_EINVAL (-1)
#define PESR_EWORKSPACE (-2)

#define PESR_ACT_NONE 0
#define PESR_ACT_RELU 1
#define PESR_ACT_LRELU 2

int pesr_abi_version(void);

/* ---- weight packing (build-owned layout transform; no reference counterpart) --------------- */
/* mode 0: forward packing [9][I/16][O][16]; mode 1: dgrad packing [9][O/16][I][16].
 * ps=1: output channels ordered sub-pixel-major for a conv feeding nn.PixelShuffle(2)
 * (reference model/basic.py:56-59). w is OIHW [O][I][3][3]. */
int pesr_pack_conv3x3(const float* w, float* out, int O, int I, int mode, int ps, void* stream);
/* many packs in one launch: desc is a DEVICE array of `count` rows of 8 int64 {w ptr, out ptr, O, I, mode, ps, R, Nn}
 * with R = ceil16(reduction channels), Nn = 16 if n-channels <= 16 else ceil64 (the sizes pesr_pack_conv3x3 derives itself);
 * modes 2 / 3: the F(2,3) Winograd packing of mode 0 / 1 (pesr_pack_conv3x3_wino), modes 4 / 5: the F(4,3) one */
int pesr_pack_conv3x3_batched(const long long* desc, int count, void* stream);
int pesr_pack_bias_ps(const float* b, float* out, int O, void* stream);

/* ---- 3x3 conv, pad 1 (reference model/basic.py:4-7 `Conv`; ATen conv2d / convolution_backward) */
/* y = act( alpha * (conv(x, w) + bias) [masked by mask > 0] + skip ).
 * x [N][H][W][Cin], y [N][OH][OW][Cout] with OH = (H-1)/stride+1.  bias/skip/mask may be NULL.
 * ps_out=1 writes y pixel-shuffled: [N][2*OH][2*OW][Cout/4] (fuses nn.PixelShuffle(2)).
 * Fused epilogues stand in for relu_ (model/basic.py:43), .mul(res_scale) and `res += x`
 * (model/basic.py:49-50, model/pesr.py:33). */
/* workspace (may be NULL / 0): scratch for split-K on layers too small to fill 256 CUs; size from
 * pesr_conv3x3_workspace_bytes(N, OH, OW, Cout) (0 for large layers). */
size_t pesr_conv3x3_workspace_bytes(int N, int OH, int OW, int Cout);
int pesr_conv3x3_fwd(const float* x, const float* w_packed, const float* bias, const float* skip, const float* mask,
                     float* y, int N, int H, int W, int Cin, int Cout, int stride, float alpha, int act, float slope,
                     int ps_out, void* workspace, size_t ws_bytes, void* stream);

/* dx = alpha * conv_transpose(dy, w) [masked by mask > 0] + skip.  dx [N][H][W][Cin], dy [N][OH][OW][Cout].
 * w_packed_dgrad from pesr_pack_conv3x3(mode 1).  mask fuses ReLU's threshold_backward (the conv's
 * own input was a ReLU output); skip fuses the residual fan-in add.  ps_in=1: dy is the gradient of
 * the pixel-shuffled output, [N][2*OH][2*OW][Cout/4] (fuses pixel_unshuffle; stride 1 only). */
int pesr_conv3x3_dgrad(const float* dy, const float* w_packed_dgrad, const float* mask, const float* skip, float* dx,
                       int N, int H, int W, int Cin, int Cout, int stride, float alpha, int ps_in, void* workspace,
                       size_t ws_bytes, void* stream);

/* dw[O][I][3][3] (OIHW, the parameter's own layout) = alpha * sum_pixels dy (x) x ;  db[O] = alpha * sum dy.
 * db may be NULL.  ps_in as above.  Workspace: pesr_conv3x3_wgrad_workspace_bytes (same algo).
 * algo: PESR_WGRAD_AUTO = the transposed Winograd kernel (on v_mfma_f32_32x32x2_f32; F(4,3) along x nested with F(2,3) along y: a third of
 * the multiplies) where it applies (stride 1, 64-multiple channels, width % 4 == 0 and >= 48 - or a width of 24 / 16 / 12 / 8 pixels, whose images are
 * laid side by side in the kernel's 48-pixel strips), else the F(2,3) one (even width >= 48; 2/3), else the direct kernel;
 * PESR_WGRAD_DIRECT = the direct kernel everywhere; PESR_WGRAD_WINO23 = F(2,3) where it applies, else direct.  All produce
 * the same gradient up to fp32 rounding (measured vs fp64: <= 2e-6 of the gradient's maximum); the choice is an argument,
 * never process state.
 * accumulate = 1: dw (and db) are ADDED TO instead of overwritten - the second contribution of a layer that is used twice in one
 * backward pass (the Discriminator sees hr and sr in one graph, reference train.py:205-214), written straight into the
 * gradient buffer the first use filled; stands in for autograd's fan-in add_.  (The F(2,3) form has no such mode: an
 * accumulating call runs on the F(4,3) or the direct kernel.) */
#define PESR_WGRAD_AUTO 0
#define PESR_WGRAD_DIRECT 1
#define PESR_WGRAD_WINO23 2
/* algo 3: retired with ABI 20 (was the F(4,3) kernel in its v_mfma_f32_16x16x4_f32 form, 8 waves); the calls return PESR_EINVAL, the workspace query 0 */
/* algo 4: retired with ABI 20 (was the 1-D F(4,3) transform on the 12-wave 32x32x2 kernel); the calls return PESR_EINVAL, the workspace query 0 */
#define PESR_WGRAD_WINO4_12W 5   /* (ABI 16) as AUTO, but on round 4's 12-wave kernel (every wave stages and multiplies) instead of the 16-wave one with
                                  * four producer waves AUTO uses since round 5: same transform, same order of additions, bit-identical results */
size_t pesr_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int stride, int algo);
int pesr_conv3x3_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                       int stride, float alpha, int ps_in, int algo, int accumulate, void* workspace, size_t ws_bytes, void* stream);
/* (ABI 19) Host only: the kernel pesr_conv3x3_wgrad runs for these arguments when its workspace has pesr_conv3x3_wgrad_workspace_bytes
 * - the rule the call itself dispatches by - as a PESR_WGRAD_KERNEL_* value, or PESR_EINVAL for arguments the call refuses.
 * pesr_conv3x3_wgrad_wino4_side: images the F(4,3) plan lays side by side in one 48-pixel strip (1; 2 .. 6 for widths below 48), 0 where
 * that plan does not cover the shape (whatever ps_in, algo and accumulate then decide). */
#define PESR_WGRAD_KERNEL_DIRECT 0         /* conv3x3_wgrad_kernel */
#define PESR_WGRAD_KERNEL_WINO23 1         /* conv3x3_wgrad_wino_kernel: F(2,3) along x */
/* kernel 2: retired with ABI 20, never answered any more (was conv3x3_wgrad_wino4_kernel: F(4,3) along x, 16x16x4 MFMA, 8 waves) */
/* kernel 3: retired with ABI 20, never answered any more (was the 1-D transform on conv3x3_wgrad_wino4x_kernel) */
#define PESR_WGRAD_KERNEL_WINO4_12W 4      /* conv3x3_wgrad_wino4x_kernel: F(4,3) along x with F(2,3) along y nested on top, 32x32x2 MFMA, 12 waves */
#define PESR_WGRAD_KERNEL_WINO4_PRODUCER 5 /* conv3x3_wgrad_wino4p_kernel: the nested transform, 12 MFMA waves + 4 staging waves (what AUTO runs) */
int pesr_conv3x3_wgrad_kernel(int N, int H, int W, int Cin, int Cout, int stride, int ps_in, int algo, int accumulate);
int pesr_conv3x3_wgrad_wino4_side(int N, int H, int W, int Cin, int Cout);

/* Stride-1 3x3 conv (pad 1) with a 1-D Winograd F(2,3) transform along x: 2/3 of the multiplies of pesr_conv3x3_fwd, same
 * tensors and fused epilogue (y = act(alpha * (conv + bias) [masked] + skip)), for even W, Cin % 16 == 0, Cout % 128 == 0
 * (pesr_conv3x3_wino_supported).  Stands in for the same ATen conv2d / convolution_backward(input) calls of the reference
 * `Conv` (model/basic.py:4-7).  w_packed: 12 * Cin * Cout floats from pesr_pack_conv3x3_wino (mode 0: forward weights from
 * OIHW [Cout][Cin][3][3]; mode 1: the input-gradient weights - then call with Cin/Cout of the gradient problem swapped).
 * ps / ps_out / ps_in: as for pesr_pack_conv3x3 / pesr_conv3x3_fwd / pesr_conv3x3_dgrad (fused PixelShuffle store, fused
 * pixel-unshuffle load).  workspace (optional, pesr_conv3x3_workspace_bytes): lets layers with few tiles split K. */
int pesr_conv3x3_wino_supported(int N, int H, int W, int Cin, int Cout);
int pesr_pack_conv3x3_wino(const float* w, float* w_packed, int Cout, int Cin, int mode, int ps, void* stream);
int pesr_conv3x3_wino(const float* x, const float* w_packed, const float* bias, const float* skip, const float* mask, float* y,
                      int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps_out, int ps_in,
                      void* workspace, size_t ws_bytes, void* stream);

/* Stride-1 3x3 conv (pad 1) with a 1-D Winograd F(4,3) transform along x (interpolation points 0, +-1, +-2, inf): HALF of
 * the multiplies of pesr_conv3x3_fwd, same tensors and fused epilogue as pesr_conv3x3_wino, for W % 4 == 0, Cin % 16 == 0,
 * Cout % 64 == 0 (Cout % 256 == 0 with ps_out).  Same ATen calls of the reference `Conv` (model/basic.py:4-7).
 * Measured relative error vs fp64: 1.2e-6 .. 1.7e-6 of the output maximum at 256 input channels (direct kernel: 3e-7).
 * w_packed: 18 * Cin * Cout floats from pesr_pack_conv3x3_wino4 (mode 0 forward / mode 1 input gradient, as above).
 * pesr_conv3x3_wino4_score: per-mille of the kernel's 576-pixel tiles that lies inside the image, or 0 if the shape is not
 * supported or gives fewer than 192 workgroups; allow_split = 1 when the split-K workspace (pesr_conv3x3_workspace_bytes) is passed. */
int pesr_conv3x3_wino4_score(int N, int H, int W, int Cin, int Cout, int allow_split);
int pesr_pack_conv3x3_wino4(const float* w, float* w_packed, int Cout, int Cin, int mode, int ps, void* stream);
int pesr_conv3x3_wino4(const float* x, const float* w_packed, const float* bias, const float* skip, const float* mask, float* y,
                       int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps_out, int ps_in,
                       void* workspace, size_t ws_bytes, void* stream);
/* ---- OPTIONAL bf16-operand mode (never the default) ---------------------------------------------------------------
 * Stride-1 3x3 conv (pad 1) on v_mfma_f32_16x16x32_bf16: same tensors (fp32 NHWC in HBM), same fused epilogue and PixelShuffle
 * options as pesr_conv3x3_wino4, but BOTH operands of every product are rounded to bf16 (round to nearest even) and summed in
 * fp32.  Not the reference's arithmetic (model/basic.py:4-7 runs nn.Conv2d in fp32): checked against its own oracle
 * (oracle/ops.py conv3x3_bf16: the same rounding, float64 sums) with its own tolerance.  Cin % 32 == 0, Cout % 64 == 0
 * (with ps_out: Cout a multiple of four workgroup widths - 256 / 128 / 64 channels for Cout % 256 / 128 / 64 == 0; Cin % 128 == 0 with ps_in).
 * w_packed: 9 * Cin * Cout bf16 (2 bytes each) from pesr_pack_conv3x3_bf16 (mode 0 forward / mode 1 input gradient - then call
 * with Cin / Cout of the gradient problem swapped).  pesr_conv3x3_bf16_score: per-mille of the kernel's 144-pixel tiles inside
 * the image, 0 for unsupported shapes or fewer than min_wgs workgroups (the host-side dispatch passes 64). */
int pesr_conv3x3_bf16_score(int N, int H, int W, int Cin, int Cout, int min_wgs);
int pesr_pack_conv3x3_bf16(const float* w, void* w_packed, int Cout, int Cin, int mode, int ps, void* stream);
int pesr_conv3x3_bf16(const float* x, const void* w_packed, const float* bias, const float* skip, const float* mask, float* y,
                      int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps_out, int ps_in,
                      void* stream);
/* ---- OPTIONAL split-bf16 mode (SURVEY 8 f4 "bf16/split-bf16 MFMA"; never the default, never the headline row; ABI 12) --------
 * The same stride-1 3x3 conv with every fp32 operand written as hi + lo (hi = bf16(v), lo = bf16(v - hi)) and every product
 * replaced by a_hi*b_lo + a_lo*b_hi + a_hi*b_hi on v_mfma_f32_16x16x32_bf16, summed in fp32: 3.6 .. 4.7e-6 of the output maximum
 * against an fp64 conv (profiles/r04_split_bf16_numerics.txt) - inside the tolerances the fp32 kernels are held to, so its oracle
 * is the reference's fp32 arithmetic itself (model/basic.py:4-7), not a restatement of the mode.  Cin % 32 == 0, Cout % 128 == 0
 * (ps_out: Cout a multiple of four workgroup widths, 256 or 128 channels; ps_in: Cin % 128 == 0).  w_packed: 2 * 9 * Cin * Cout
 * bf16 from pesr_pack_conv3x3_bf16x3 (hi plane, then lo plane; mode 0 forward / mode 1 input gradient).  Weight gradients stay on
 * the fp32 kernels.  _score: per-mille of the 144-pixel tiles inside the image, 0 if unsupported or fewer than min_wgs workgroups. */
int pesr_conv3x3_bf16x3_score(int N, int H, int W, int Cin, int Cout, int min_wgs);
int pesr_pack_conv3x3_bf16x3(const float* w, void* w_packed, int Cout, int Cin, int mode, int ps, void* stream);
int pesr_conv3x3_bf16x3(const float* x, const void* w_packed, const float* bias, const float* skip, const float* mask, float* y,
                        int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps_out, int ps_in, void* stream);

/* Stride-2 forward in the bf16 mode (the Discriminator's down-sampling convs, reference model/pesr.py:56-64: Conv(k=3, stride=2,
 * padding=1)): x [N][H][W][Cin] -> y [N][(H-1)/2+1][(W-1)/2+1][Cout], skip / mask shaped like y; weights packed by
 * pesr_pack_conv3x3_bf16 mode 0 (the stride-1 forward's packing).  Its weight gradient stays on the fp32 kernels.
 * pesr_conv3x3_bf16_s2_score: as above, but half of min_wgs workgroups already qualify (these layers are small). */
int pesr_conv3x3_bf16_s2_score(int N, int H, int W, int Cin, int Cout, int min_wgs);
int pesr_conv3x3_bf16_s2(const float* x, const void* w_packed, const float* bias, const float* skip, const float* mask, float* y,
                         int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, void* stream);
/* Input gradient of the same stride-2 conv in the bf16 mode: dy [N][(H-1)/2+1][(W-1)/2+1][Cout_fwd] -> dx [N][H][W][Cin_fwd] =
 * alpha * grad [zeroed where mask <= 0] + skip (mask / skip shaped like dx, may be null); the four output parity classes are
 * four small stride-1 problems with 1 / 2 / 2 / 4 taps inside ONE launch.  w_packed: pesr_pack_conv3x3_bf16 mode 1 of the forward
 * weights (the stride-1 input gradient's packing).  Cout_fwd % 32 == 0, Cin_fwd % 64 == 0. */
int pesr_conv3x3_bf16_s2_dgrad_score(int N, int H, int W, int Cout_fwd, int Cin_fwd, int min_wgs);
int pesr_conv3x3_bf16_s2_dgrad(const float* dy, const void* w_packed, const float* mask, const float* skip, float* dx, int N, int H,
                               int W, int Cout_fwd, int Cin_fwd, float alpha, void* stream);
/* Weight / bias gradient of the same conv in the bf16 mode: dw = alpha * sum bf16(dy) * bf16(x) (fp32 sums; fixed-order split-K
 * reduce, bit-reproducible), db = alpha * sum dy (fp32, un-rounded).  Same tensors and ps_in / accumulate meaning as
 * pesr_conv3x3_wgrad.  Stride 1, W % 48 == 0, Cin % 64 == 0, Cout % 128 == 0 (Cout % 512 == 0 with ps_in); workspace_bytes
 * returns 0 for shapes it does not cover. */
size_t pesr_conv3x3_wgrad_bf16_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int pesr_conv3x3_wgrad_bf16(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                            float alpha, int ps_in, int accumulate, void* workspace, size_t ws_bytes, void* stream);

/* Forward 3x3 conv from a 3-channel input, stride 1 (reference `embed` model/pesr.py:23, Discriminator features.0
 * model/pesr.py:53, vgg19 features.0): x [N][H][W][3], w OIHW [Cout][3][3][3] (NOT packed), y [N][H][W][Cout]. */
int pesr_conv3x3_rgb_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cout, int act,
                         float slope, void* stream);

/* Forward 3x3 conv to 3 output channels, stride 1 (the Generator's last conv, reference model/pesr.py:38 `Conv(num_channels, 3)`
 * via model/basic.py:4-7): x [N][H][W][C] (C a multiple of 64, <= 512), w OIHW [3][C][3][3] (NOT packed), bias [3] or null,
 * y [N][H][W][3].  HBM-bound: every input row is read once per band of 12 output rows. */
int pesr_conv3x3_rgb_out_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, int act,
                             float slope, void* stream);

/* Input gradient of a C -> 3 conv (stride 1): reference Upsampler's last conv (model/basic.py:60), i.e. ATen
 * convolution_backward(input) for it.  dy [N][H][W][3], w OIHW [3][C][3][3] (NOT packed), dx [N][H][W][C]. */
int pesr_conv3x3_rgb_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, void* stream);

/* Input gradient of a 3 -> C conv (stride 1): Discriminator features.0 (reference model/pesr.py:53) and vgg19 features.0
 * (model/vgg.py:8-10) on the Generator's backward path, i.e. ATen convolution_backward(input) for them.  dy [N][H][W][C]
 * (C a multiple of 64, <= 512), w = the forward conv's OIHW [C][3][3][3] (NOT packed), dx [N][H][W][3].  HBM-bound (reads dy
 * once): the kernel of pesr_conv3x3_rgb_out_fwd with a transposing weight index.  (ABI 12) */
int pesr_conv3x3_rgb_in_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, void* stream);

/* Weight gradient of the RGB-boundary convs (one operand has 3 channels): reference `embed`
 * (model/pesr.py:23), Discriminator features.0 (model/pesr.py:53), Upsampler's last conv (model/basic.py:60).
 * a: the C-channel tensor [N][H][W][C], b3: the 3-channel tensor [N][H][W][3].
 * mode 0 (3 -> C): a = dy, b3 = x, dw [C][3][3][3], db [C].  mode 1 (C -> 3): a = x, b3 = dy, dw [3][C][3][3], db [3].
 * accumulate = 1: dw is added to (db must then be NULL), as for pesr_conv3x3_wgrad. */
size_t pesr_conv3x3_wgrad_rgb_workspace_bytes(int N, int H, int W, int C);
int pesr_conv3x3_wgrad_rgb(const float* a, const float* b3, float* dw, float* db, int N, int H, int W, int C, int mode,
                           float alpha, int accumulate, void* workspace, size_t ws_bytes, void* stream);

/* ---- MeanShift: trainable 1x1 conv 3->3 (reference model/basic.py:9-17) ----------- */
/* x_nchw / y_nchw: the 3-channel tensor is stored NCHW-contiguous instead of NHWC (folds the layout
 * change of the network's RGB input/output into this kernel). */
int pesr_meanshift_fwd(const float* x, const float* w, const float* b, float* y, int N, int H, int W, int x_nchw, int y_nchw,
                       void* stream);
/* dy, dx NHWC; dx may be NULL.  dw [3][3], db [3].  workspace >= 1024*12*4 + 128 bytes. */
int pesr_meanshift_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, int N, int H, int W,
                       int x_nchw, void* workspace, size_t ws_bytes, void* stream);

/* ---- nn.PixelShuffle(2) standalone (reference model/basic.py:57,59), bit-exact indexing ------- */
/* x [N][H][W][4C] -> y [N][2H][2W][C]:  y[n][2h+i][2w+j][c] = x[n][h][w][4c+2i+j];  bwd is the inverse. */
int pesr_pixel_shuffle_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int pesr_pixel_shuffle_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream);

/* ---- nn.PixelShuffle(r) standalone for r = 2 or 3 (the x2 / x3 Upsampler), bit-exact indexing --- */
/* x [N][H][W][r*r*C] -> y [N][r*H][r*W][C]:  y[n][r*h+i][r*w+j][c] = x[n][h][w][c*r*r + i*r + j];  bwd is the inverse
 * (dy [N][r*H][r*W][C] -> dx [N][H][W][r*r*C]).  Any C >= 1; r outside {2, 3} -> PESR_EINVAL.  r = 2 gives the bits of
 * pesr_pixel_shuffle_fwd / _bwd.  64-bit offsets; no workspace. */
int pesr_pixel_shuffle_r_fwd(const float* x, float* y, int N, int H, int W, int C, int r, void* stream);
int pesr_pixel_shuffle_r_bwd(const float* dy, float* dx, int N, int H, int W, int C, int r, void* stream);

/* out = (ref > 0 ? alpha*g : slope*alpha*g) + add : ReLU (slope 0) / LeakyReLU backward (+ residual fan-in);
 * ref/add may be NULL */
int pesr_relu_mask(const float* g, const float* ref, const float* add, float* out, long n, float alpha, float slope,
                   void* stream);

/* ---- 2x2/2 max-pool (torchvision vgg19 features, reference model/vgg.py:8-10) ------------------ */
/* forward: floor mode, y is [N][H/2][W/2][C] (an odd side's last row / column is dropped); H, W >= 2, C % 4 == 0.  The backward
 * takes even sides only. */
int pesr_maxpool2x2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* relu_in=1 also applies the mask of the ReLU that produced x (gradient only where x > 0) */
int pesr_maxpool2x2_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C, int relu_in, void* stream);

/* ---- BatchNorm2d(train) + LeakyReLU (reference model/basic.py:29-30, model/pesr.py:47) --------- */
size_t pesr_bn_workspace_bytes(long M, int C);
/* mean_invstd [2][C] is saved for backward; running stats / num_batches (int64) updated as nn.BatchNorm2d
 * does, may be NULL.  y_nchw=1 writes y NCHW-contiguous (the flatten of reference model/pesr.py:79). */
int pesr_bn_lrelu_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean_invstd,
                      float* running_mean, float* running_var, long long* num_batches, int N, int H, int W, int C, float eps,
                      float momentum, float slope, int y_nchw, void* workspace, size_t ws_bytes, void* stream);
/* (ABI 14) conv 3 -> C (pad 1, stride 1, NO bias) -> BatchNorm2d(train) -> LeakyReLU in one call, for the layer where the statistics
 * pass costs most (the Discriminator's features.0, reference model/pesr.py:53 + model/basic.py:26-30: 16 x 192 x 192 x 64): the conv
 * kernel (that of pesr_conv3x3_rgb_fwd, OIHW weights [C][3][3][3]) leaves per-workgroup sums / sums of squares of its result, the
 * finalize step reduces them in a fixed order in double - no pass over z for the statistics (SURVEY K10's first half).  Writes z
 * (the conv output, saved for backward) AND y; everything else as pesr_bn_lrelu_fwd.  C % 4 == 0 and 256 % (C / 4) == 0. */
size_t pesr_conv3x3_rgb_bn_workspace_bytes(int N, int H, int W, int C);
int pesr_conv3x3_rgb_bn_lrelu_fwd(const float* x, const float* w, float* z, const float* gamma, const float* beta, float* y,
                                  float* mean_invstd, float* running_mean, float* running_var, long long* num_batches, int N, int H,
                                  int W, int C, float eps, float momentum, float slope, int y_nchw, void* workspace, size_t ws_bytes,
                                  void* stream);
/* accumulate = 1: dgamma / dbeta are added to instead of overwritten (second use of the layer in one backward pass). */
int pesr_bn_lrelu_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean_invstd,
                      float* dx, float* dgamma, float* dbeta, int N, int H, int W, int C, float slope, int dy_nchw,
                      int accumulate, void* workspace, size_t ws_bytes, void* stream);

/* Eval-mode BatchNorm2d (+ activation): the statistics are GIVEN - mean_invstd [2][C] = {running_mean, 1/sqrt(running_var + eps)}
 * (nn.BatchNorm2d in .eval(), a constructor branch of reference model/basic.py:29 the reference's own scripts never take).
 * slope: 0.2 LeakyReLU, 0 ReLU, 1 no activation (also accepted by the training-mode entry points above).
 * bwd: dx = gamma * invstd * dz, dgamma = sum dz * xhat, dbeta = sum dz with dz = dy * act'(z); workspace as pesr_bn_workspace_bytes. */
int pesr_bn_lrelu_eval_fwd(const float* x, const float* gamma, const float* beta, const float* mean_invstd, float* y, int N, int H,
                           int W, int C, float slope, int y_nchw, void* stream);
int pesr_bn_lrelu_eval_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean_invstd, float* dx,
                           float* dgamma, float* dbeta, int N, int H, int W, int C, float slope, int dy_nchw, void* workspace,
                           size_t ws_bytes, void* stream);

/* Backward OF the training-mode BatchNorm backward - what the gradient penalty (reference train.py:216-226, autograd.grad(...,
 * create_graph=True) through D's eight BatchNorm2d layers) needs: for dz = gamma * invstd * (du - mean(du) - xhat * mean(du * xhat))
 * and g = dL/d(dz) it returns l_du = dL/d(du), l_z = dL/dz (through xhat and invstd) and l_gamma = dL/dgamma; any of the three
 * outputs may be NULL.  All tensors [N][H][W][C]; mean_invstd as saved by pesr_bn_lrelu_fwd. */
size_t pesr_bn_bwd_bwd_workspace_bytes(long M, int C);
int pesr_bn_bwd_bwd(const float* z, const float* du, const float* g, const float* gamma, const float* mean_invstd, float* l_du,
                    float* l_z, float* l_gamma, int N, int H, int W, int C, void* workspace, size_t ws_bytes, void* stream);

/* ---- skinny-batch Linear (reference model/pesr.py:69-74; ATen addmm/mm), M <= 32 per call ------- */
/* (the Python binding walks larger batches in chunks of 32 rows: pesr_amd/ops.py linear_*).
 * pesr_linear_wgrad: accumulate = 1 adds to dw / db instead of overwriting them (the second use of a layer inside one
 * backward pass - the Discriminator sees hr and sr in the same graph, reference train.py:205-214 - and batch chunks). */
size_t pesr_linear_workspace_bytes(int M, int N, long K);
int pesr_linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int N, long K, int act, float slope,
                    void* workspace, size_t ws_bytes, void* stream);
int pesr_linear_dgrad(const float* dy, const float* w, float* dx, int M, int N, long K, void* workspace, size_t ws_bytes,
                      void* stream);
int pesr_linear_wgrad(const float* dy, const float* x, float* dw, float* db, int M, int N, long K, int accumulate, void* stream);

/* ---- losses, fused forward + gradient (reference train.py:131-140) --------------------------------- */
/* sr, hr, grad: [N][H][W][3].  out2[0] = mean|sr-hr|, out2[1] = TV sum.  grad = g_l1*sign(sr-hr) + g_tv*dTV/dsr
 * (caller folds alpha_l1/numel and alpha_tv into g_l1, g_tv); grad may be NULL.  workspace >= 8 KiB + 64 B. */
int pesr_loss_l1_tv_fwd_bwd(const float* sr, const float* hr, float* grad, float* out2, int N, int H, int W, float g_l1,
                            float g_tv, void* workspace, size_t ws_bytes, void* stream);
/* out1[0] = mean (a-b)^2 ; grad = gscale*(a-b) (caller passes 2*alpha/numel); grad may be NULL */
int pesr_mse_fwd_bwd(const float* a, const float* b, float* grad, float* out1, long n, float gscale, void* workspace,
                     size_t ws_bytes, void* stream);

/* ---- training-sample assembly on the GPU (reference data.py:79-126: _crop, _aug_data, _to_tensor) ---- */
/* pool: device uint8 HWC images back to back.  desc: B rows of 3 int64 {byte offset of the image, stride_w | y0 << 32,
 * x0 | aug << 32} (stride_w = image width in pixels; (y0, x0) crop origin; aug bit 0 hflip, bit 1 vflip, bit 2
 * transpose, applied transpose -> vflip -> hflip as the reference).  out: [B][3][P][P] fp32 (nhwc = 0) or [B][P][P][3]. */
int pesr_crop_augment(const unsigned char* pool, const long long* desc, float* out, int B, int P, int nhwc, void* stream);

/* ---- bicubic resize of uint8 HWC images by s in {2, 3, 4}: MATLAB's imresize for uint8 input (docs/modes.md section 4f) ------- */
/* One pass along one axis (0 = height, 1 = width) over n_images images of a device-resident pool.  Descriptor: n_images rows of
 * 4 int64 {source byte offset in src, destination byte offset in dst, H, W}, H and W being the size of the pass's INPUT image; the
 * output is H/s (up = 0) or s*H (up = 1) rows of W pixels for axis 0, H rows of W/s or s*W pixels for axis 1.  desc_host and
 * desc_dev hold the same rows: the host copy is checked and sizes the grid, the kernel reads the device copy.  weights_host: 16
 * doubles on the host, copied by value - up = 0: the 8 / 11 / 16 tap weights in ascending tap order; up = 1: [s][4], one row per
 * output phase (pesr_amd/resize.py resize_weights); the rest ignored.  float64 accumulation in ascending tap order without fused
 * multiply-add, clamp, round half up: bit-identical to the float64 host restatement.  A full resize is axis 0 into an
 * intermediate pool, then axis 1.  PESR_EINVAL (nothing launched): s outside {2, 3, 4}, H or W < 1, the pass's axis length not a
 * multiple of s when up = 0, a negative offset.  64-bit offsets; no workspace. */
int pesr_imresize_u8_pass(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev,
                          int n_images, int axis, int s, int up, const double* weights_host, void* stream);

/* ---- classical degradation LR = (HR (*) k) subsampled by s, plus noise (docs/modes.md section 4j) ------- */
/* n entries in one launch.  Descriptor: n rows of 11 int64 {source byte offset in src, destination byte offset in dst (both at any
 * alignment), H, W of the uint8 HWC source image (multiples of s), y0, x0, h, w of the window of its H/s x W/s LR grid that the
 * entry produces, index of its blur kernel in the bank, sigma_n as float64 bits, noise stream number q}.  Entry i writes h*w*3 bytes,
 * HWC, at its destination offset.  bank_dev: device doubles [n_kernels][K][K], row-major.  LR pixel (oy, ox) of the image reads HR
 * rows s*oy + (s-K)/2 + i, i = 0 .. K-1 (columns likewise), an index outside the image clamped to the edge; float64 accumulation
 * over i, then j, ascending, without fused multiply-add; sigma_n != 0 adds sigma_n * g(q, element of the window); clamp, round half
 * up: bit-identical to the float64 host restatement.  desc_host and desc_dev hold the same rows: the host copy is checked and sizes
 * the grid, the kernel reads the device copy.  PESR_EINVAL (nothing launched): s outside {2, 3, 4}, K outside 1..24 or K - s odd,
 * H % s or W % s nonzero, an empty window or one outside the LR grid, a kernel index outside the bank, a negative or non-finite
 * sigma_n, a negative offset, n < 1.  No workspace. */
int pesr_degrade_u8(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n, int s,
                    int K, const double* bank_dev, int n_kernels, void* stream);

/* ---- JPEG round trip of uint8 HWC RGB windows: encoder at quality q, then decoder (docs/modes.md section 4l) ------- */
/* n entries in one call (two launches).  Descriptor: n rows of 8 int64 {source byte offset in src, source row stride in pixels,
 * destination byte offset in dst, destination row stride in pixels (offsets at any alignment), h, w of the window, quality q in
 * 1 .. 100, byte offset of the entry's planes in the workspace = the workspace bytes of the entries before it}.  Entry i reads the
 * h x w pixels at its source offset and writes h x w pixels at its destination offset; the entries' windows must not overlap, but
 * dst may be src (in place).  chroma: 420 (chroma planes of ceil(h/2) x ceil(w/2): 2 x 2 mean, back up with the 9/3/3/1 triangle
 * filter) or 444.  dct_dev: 64 device doubles, T[u][x] = 0.5 c(u) cos((2x+1) u pi / 16); quant_dev: device doubles [100][2][64], the
 * luminance and chrominance tables of q = 1 .. 100 in row-major (vertical frequency first) order (pesr_amd/jpeg.py makes both).
 * The 8 x 8 block grid starts at the window's origin; planes are extended by replication.  float64 without fused multiply-add, sums
 * in ascending order: bit-identical to the float64 host restatement.  Workspace: an entry needs h*w + 2*ceil(h/2)*ceil(w/2) bytes
 * at 420, 3*h*w at 444; pesr_jpeg_workspace_bytes adds them up (0 if the descriptors are not valid).  desc_host and desc_dev hold
 * the same rows: the host copy is checked and sizes the grid, the kernels read the device copy.  PESR_EINVAL (nothing launched): q
 * outside 1 .. 100, h or w < 1, a stride below w, a negative offset, a workspace offset that is not the running sum, n < 1, chroma
 * not 420 or 444, a workspace smaller than pesr_jpeg_workspace_bytes.  No atomics: the same bits on every run. */
size_t pesr_jpeg_workspace_bytes(const long long* desc_host, int n, int chroma);
int pesr_jpeg_u8(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n,
                 int chroma, const double* dct_dev, const double* quant_dev, void* workspace, size_t ws_bytes, void* stream);

/* ---- resize of uint8 HWC RGB windows from any size to any size, one pass (docs/modes.md section 4m) ------- */
/* n entries in one launch; axis 0 resizes the height (w_out must equal w_in), axis 1 the width (h_out must equal h_in); a resize is
 * the height pass into an intermediate uint8 image, then the width pass.  Descriptor: n rows of 12 int64 {source byte offset in
 * src, source row stride in pixels, destination byte offset in dst, destination row stride in pixels (offsets at any alignment),
 * h_in, w_in, h_out, w_out, offset of the entry's table in tables_dev in 8-byte words, taps T, the float64 bits of the noise level
 * sigma_n (grey levels; 0 = none; width pass only), noise stream}.  An entry may be a window of a larger image: the symmetric
 * reflection is at the window's own border.  Table of an axis with n_out outputs (pesr_amd/resize.py makes it): (T + 1) * n_out
 * words, tap-major - word [o] the unreflected first tap of output o as an int64, word [(1 + k) * n_out + o] the float64 weight k of
 * output o, rows with fewer than T taps ending in 0.0; entries may share a table.  out[o] = sum over k ascending of w[k][o] *
 * in[reflect(first[o] + k)] in float64 without fused multiply-add, then section 4j's noise, clamp, round half up: bit-identical to
 * the float64 host restatement.  desc_host and desc_dev hold the same rows: the host copy is checked and sizes the grid, the kernel
 * reads the device copy.  PESR_EINVAL (nothing launched): n < 1, a side < 1, the pass's axis beyond 8:1 or 1:8, the other axis
 * changed, a stride below the width, a negative offset, T outside 1 .. 32, a table that does not lie inside table_words, a negative,
 * NaN or infinite sigma_n, a nonzero sigma_n on the height pass, an axis other than 0 or 1.  No workspace, no atomics. */
int pesr_resize_to_u8_pass(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n,
                           int axis, const void* tables_dev, long table_words, void* stream);

/* ---- validation PSNR on the Y channel (reference utils.py:32-41 compute_PSNR), one image pair [1][3][H][W] ------- */
/* a_nhwc / b_nhwc: the tensor is stored [H][W][3] instead of [3][H][W].  out2 (device doubles): {mse, psnr dB}; all
 * arithmetic in double on integer-valued terms -> bit-identical to the reference's numpy path.  workspace >= 2 KiB. */
int pesr_psnr_y(const float* a, const float* b, double* out2, int H, int W, int a_nhwc, int b_nhwc, void* workspace,
                size_t ws_bytes, void* stream);

/* ---- SSIM on the Y channel with a border shave (docs/modes.md section 4g), N image pairs [N][3][H][W] ------- */
/* The SSIM of Wang et al.'s ssim_index.m on the Y image of the PSNR-Y above: rows and columns [shave, H-shave) x [shave, W-shave),
 * 11 x 11 Gaussian window of sigma 1.5 applied separably (height, then width) over the "valid" region, K1 = 0.01, K2 = 0.03,
 * L = 255; float64 without fused multiply-add, bit-identical to the float64 host restatement.  a_nhwc / b_nhwc: that tensor is
 * stored [N][H][W][3].  out: N device doubles, the mean of each pair's map.  map_or_null: when non-null the
 * [N][H-2*shave-10][W-2*shave-10] double map is written too.  The workspace holds one double per workgroup:
 * 8 * N * ceil((H-2*shave-10)/16) * ceil((W-2*shave-10)/16) bytes are enough for every tile size the library may be built with,
 * less -> PESR_EWORKSPACE.  PESR_EINVAL (nothing launched): N < 1, shave < 0, H-2*shave or W-2*shave below 11 (no smaller window is
 * substituted), N > 65535.  No atomics: the result is the same bits on every run.  64-bit offsets. */
int pesr_ssim_y(const float* a, const float* b, double* out, int N, int H, int W, int a_nhwc, int b_nhwc, int shave,
                double* map_or_null, void* workspace, size_t ws_bytes, void* stream);

/* ---- SSIM-Y as a training loss (docs/modes.md section 4p), N image pairs [N][3][H][W] ------- */
/* The score of pesr_ssim_y on the UNQUANTISED luma: Y = ((r*(65.738/256) + g*(129.057/256)) + b*(25.064/256)) + 16 in double from the
 * fp32 values, nothing clipped or rounded (so not the metric's bits, even on integer images); window, "valid" region, separable
 * filtering and the map's expression order as there; no shave.  score: N device doubles, the mean of each pair's
 * [H-10][W-10] map.  coef_or_null: when non-null, double [N][3][H-10][W-10], the derivatives of each window's value with respect
 * to its moments mean(x), mean(x*x), mean(x*y) (the raw moments held fixed) - what pesr_ssim_loss_bwd reads.  The workspace holds one
 * double per workgroup: 8 * N * ceil((H-10)/16) * ceil((W-10)/16) bytes are enough, less -> PESR_EWORKSPACE.  PESR_EINVAL (nothing
 * launched): a null a, b or score, N < 1 or N > 65535, a side below 11, score, coef or the workspace not on an 8-byte boundary.
 * Float64 without fused multiply-add, no atomics: bit-identical to the ordered float64 host restatement and on every call. */
int pesr_ssim_loss_fwd(const float* a, const float* b, double* score, int N, int H, int W, int a_nhwc, int b_nhwc,
                       double* coef_or_null, void* workspace, size_t ws_bytes, void* stream);
/* Its gradient with respect to a.  coef: what the forward wrote for the same a and b; g: N device doubles, dL/dscore of each pair;
 * ga: fp32 in a's layout ([N][H][W][3] when a_nhwc).  With T[m] the transpose of the valid filter applied to map m, x and y the lumas:
 *     dY = (g[n] / ((H-10) (W-10))) * ((T[ca] + (2 x) T[cb]) + y T[cc]),  ga_c = (float)(dY * k_c),  k = the three luma weights.
 * Every input element is read once, every gradient element written once; no workspace, no atomics; b gets no gradient.  PESR_EINVAL
 * (nothing launched): a null pointer, N < 1 or N > 65535, a side below 11, coef or g not on an 8-byte boundary, ga not on 4. */
int pesr_ssim_loss_bwd(const float* a, const float* b, const double* coef, const double* g, float* ga, int N, int H, int W,
                       int a_nhwc, int b_nhwc, void* stream);

/* ---- Texture loss: patch-wise Gram matrices (docs/modes.md section 4q), features f [N][H][W][C] fp32 ------- */
/* Patches of ph x pw pixels tile the map (H % ph == 0, W % pw == 0; ph = H, pw = W is the whole-map Gram of Gatys / Johnson):
 * P = (H / ph) (W / pw) per image, row-major; K = ph pw pixels each.  G [N][P][C][C] fp32,
 *     G[n][p][c][c'] = s * sum_k f[n][k][c] f[n][k][c'],   s = 1 / (C K),
 * on the fp32 MFMA (a k-ordered fmaf chain per element), scaled once at the end; bit-for-bit symmetric, and the same bits on every
 * call (no atomics).  Long patches are cut into pesr_gram_splits(...) slices of K whose sums go through the workspace
 * ([S][N P][C][C] floats = pesr_gram_workspace_bytes(...), 0 when S == 1) and are added in ascending order.  Both planners are pure
 * host functions of the shape; pesr_gram_splits returns 0 for a shape the kernels do not take.  PESR_EINVAL (nothing launched): a
 * null f or G, N < 1, a side < 1, C not 64, 128 or 256, a patch that does not divide the map, f, G or the workspace not on a
 * 16-byte boundary; PESR_EWORKSPACE: S > 1 and a missing or smaller workspace.  64-bit offsets. */
int pesr_gram_splits(int N, int H, int W, int C, int ph, int pw);
size_t pesr_gram_workspace_bytes(int N, int H, int W, int C, int ph, int pw);
int pesr_gram_fwd(const float* f, float* G, int N, int H, int W, int C, int ph, int pw, void* workspace, size_t ws_bytes, void* stream);
/* The squared distance of two such tensors ga, gb [N][P][C][C]: d = (double)ga - (double)gb (exact), t[n] = (sum_p sum_cc' d^2) / P as
 * N device doubles (fixed summation tree, no fused multiply-add, no atomics); dg_or_null: when non-null, fp32 [N][P][C][C], (float)d -
 * what pesr_gram_bwd reads.  The workspace holds one double per workgroup: pesr_gram_loss_workspace_bytes(N, P, C), less ->
 * PESR_EWORKSPACE.  PESR_EINVAL: a null ga, gb or t, N < 1 or N > 65535, P < 1, C as above, ga, gb or dg not on a 16-byte boundary,
 * t or the workspace not on 8. */
size_t pesr_gram_loss_workspace_bytes(int N, int P, int C);
int pesr_gram_loss(const float* ga, const float* gb, double* t, float* dg_or_null, int N, int P, int C, void* workspace,
                   size_t ws_bytes, void* stream);
/* The gradient of sum_n g[n] t[n] with respect to the f that ga was made from: dg a SYMMETRIC [N][P][C][C] (pesr_gram_loss's), g N
 * device doubles, gf fp32 [N][H][W][C],
 *     gf[n][k][c] = (float)(g[n] * 4 s / P) * sum_c' f[n][k][c'] dg[n][p(k)][c'][c]
 * on the fp32 MFMA; every element written once, no workspace, no atomics; not masked by f > 0.  Shape errors as pesr_gram_fwd;
 * f, dg and gf on 16-byte boundaries, g on 8. */
int pesr_gram_bwd(const float* f, const float* dg, const double* g, float* gf, int N, int H, int W, int C, int ph, int pw, void* stream);

/* ---- Contextual loss (docs/modes.md section 4r), features as P points of C channels per image: [N][P][C] fp32 ------- */
/* N in 1 .. 65535, P in 1 .. 4096, C in {64, 128, 256}: anything else -> PESR_EINVAL with nothing launched, as do a null pointer and a
 * misaligned one (feature-sized arrays on 16-byte boundaries, doubles on 8, the rest on 4).  fp32 MFMA for the two GEMMs, doubles for
 * the sums, no atomics, fixed summation orders: the same call gives the same bits.  64-bit offsets (D is [N][P][P]).
 * The four planners are pure host functions of the shape and return 0 for a shape the kernels do not take: the row blocks (of 64 rows)
 * of the distance and the row kernels, the column pieces (of 64 columns) that the distance kernel stages, the workspace that
 * pesr_cx_fwd and pesr_cx_bwd want (less -> PESR_EWORKSPACE), and the bytes that a forward keeps for its backward. */
int pesr_cx_row_blocks(int N, int P, int C);
int pesr_cx_col_pieces(int N, int P, int C);
size_t pesr_cx_workspace_bytes(int N, int P, int C);
size_t pesr_cx_saved_bytes(int N, int P, int C);
/* mu [N][C] = the mean of fb's points (double sum, one rounding); xh = (fa - mu) r, yh = (fb - mu) r with
 * r = (float)(1 / sqrt(sum_c (f - mu)^2 + 1e-12)), the sum in double; inv [N][P] = r of fa's points. */
int pesr_cx_normalize(const float* fa, const float* fb, float* mu, float* xh, float* yh, float* inv, int N, int P, int C, void* stream);
/* D [N][P][P] = fma(-0.5, xh_i . yh_j, 0.5) with the dot product on the MFMA (a channel-ordered fmaf chain); m [N][P] = min_k D_ik and
 * b [N][P] (int32) its lowest index, bit for bit from the stored D. */
int pesr_cx_dist(const float* xh, const float* yh, float* D, float* m, int* b, int N, int P, int C, void* stream);
/* w_ik = expf(fma(-D_ik, 1 / (m_i + 1e-5), 1) (float)(1 / h)); S [N][P] = sum_k w_ik (double, rounded once); c_ik = w_ik (1 / S_i);
 * cmax [N][P] = max_i c_ij and a [N][P] (int32) its lowest index; CX [N] = (sum_j cmax_j) / P and L [N] = -log CX as doubles.  h > 0. */
int pesr_cx_fwd(const float* D, const float* m, double h, float* S, int* a, float* cmax, double* CX, double* L, int N, int P, int C,
                void* workspace, size_t ws_bytes, void* stream);
/* The gradient of sum_n gL[n] L[n] with respect to fa, with a and b held fixed: gf [N][P][C] fp32.  E = dL/dD is formed from D on the fly
 * (section 4r), g_xh = -E yh / 2 on the MFMA, gf = (g_xh - xh (xh . g_xh)) inv.  gL[n] == 0 -> image n all zero.  e_or_null [N][P][P] and
 * gxh_or_null [N][P][C]: when non-null they receive E and g_xh (for tests; nothing else reads them).  Not masked by fa > 0. */
int pesr_cx_bwd(const float* D, const float* m, const int* b, const float* S, const int* a, const float* cmax, const double* CX,
                const double* gL, const float* xh, const float* yh, const float* inv, double h, float* gf, float* e_or_null,
                float* gxh_or_null, int N, int P, int C, void* workspace, size_t ws_bytes, void* stream);

/* ---- NIQE block statistics (docs/modes.md section 4k), N images [N][3][H][W] (nhwc: [N][H][W][3]) ------- */
/* The device half of the no-reference score of Mittal et al. as section 4k restates it.  RGB clipped to 0..255 and rounded; luma
 * 0 = MATLAB's rgb2gray, floor(((r*0.298936021293775 + g*0.587043074451121) + b*0.114020904255103) + 0.5), luma 1 = the Y of the
 * PSNR-Y above; `shave` pixels dropped on each side, then a top-left crop to Hc = B*floor((H-2*shave)/B), Wc likewise: nby x nbx
 * blocks.  Scale 1 is that luma, scale 2 its x0.5 antialiased bicubic resize (pesr_imresize_u8_pass's x2-down weights and border
 * rule, height then width, never rounded or clamped), with blocks of B/2.  Per scale the MSCN map (I - mu) / (sigma + 1), mu and
 * sigma from the 7-tap Gaussian window of sigma 7/6 applied separably with replicated edges.  stats: double [N][2][nby*nbx][26], per
 * block and scale: for the map m and for m * circshift(m, d), d = (0,1), (1,0), (1,1), (1,-1), the shift wrapping inside the block,
 * {sum of x*x over x < 0, count of x < 0, sum of x*x over x > 0, count of x > 0, sum of |x|}; the 26th value is the sum of sigma.
 * mscn1_or_null / mscn2_or_null: when non-null the maps [N][Hc][Wc] and [N][Hc/2][Wc/2] are written there.  float64 without fused
 * multiply-add: both maps are bit-identical to the float64 host restatement; the sums are taken in a fixed order without atomics,
 * the same bits on every run.  Workspace: 30 * N * Hc * Wc bytes (luma, sigma and MSCN map of both scales, 8-byte aligned), whether
 * or not the maps are asked for; less -> PESR_EWORKSPACE.  PESR_EINVAL (nothing launched): B odd or outside 8..96, shave < 0,
 * fewer than 2 blocks, N < 1 or N > 65535, luma not 0 or 1.  64-bit offsets. */
int pesr_niqe_stats(const float* img, int N, int H, int W, int nhwc, int shave, int B, int luma, double* stats,
                    double* mscn1_or_null, double* mscn2_or_null, void* workspace, size_t ws_bytes, void* stream);

/* ---- LPIPS head of one tapped layer (docs/modes.md section 4n), N pairs of NHWC feature maps ------- */
/* feat: fp32 [2N][H][W][C], entries 0 .. N-1 the features of image a, N .. 2N-1 those of image b (the trunk runs [a; b] as one
 * batch); w: C floats, the layer's 1 x 1 "lin" weights.  Per pixel p: na = sqrt(sum_c a_c^2), nb likewise, d(p) = sum_c w_c *
 * (a_c / (na + 1e-10) - b_c / (nb + 1e-10))^2; out: N device doubles, the mean of d over the H * W pixels of each pair.
 * map_or_null: when non-null the [N][H][W] double map d is written too; the score is the same bits either way.  Every feature
 * element is read once; float64 after the load, no fused multiply-add, every sum in an order that depends on (H, W, C) alone, no
 * atomics: bit-identical to the ordered float64 host restatement and on every call.  The workspace holds one double per 64 pixels
 * of an image: 8 * N * ceil(H * W / 64) bytes, less -> PESR_EWORKSPACE.  PESR_EINVAL (nothing launched): C not 64, 128, 256 or
 * 512, N < 1 or N > 65535, a side < 1, feat not on a 16-byte boundary.  64-bit offsets. */
int pesr_lpips_layer(const float* feat, const float* w, double* out, int N, int H, int W, int C, double* map_or_null,
                     void* workspace, size_t ws_bytes, void* stream);

/* The same head with the two feature tensors as separate base pointers fa, fb: fp32 [N][H][W][C] each (the training path,
 * docs/modes.md section 4o, runs the trunk on sr and on hr apart).  One kernel with pesr_lpips_layer, which is this call with
 * fb = feat + N * H * W * C: the same bits.  Arguments, workspace and errors as there; fa and fb each on a 16-byte boundary. */
int pesr_lpips_layer2(const float* fa, const float* fb, const float* w, double* out, int N, int H, int W, int C, double* map_or_null,
                      void* workspace, size_t ws_bytes, void* stream);

/* The head's gradient with respect to fa (docs/modes.md section 4o).  g: N device doubles, dL/dscore of each pair; ga: fp32
 * [N][H][W][C].  With ah = a / (na + 1e-10), bh likewise, t = ah - bh and q = sum_c w_c t_c ah_c per pixel:
 *     ga_j = (2 g[n] / (H W)) * (w_j t_j - (a_j / na) q) / (na + 1e-10),  rounded once to fp32;  ga_j = 0 where na == 0
 * (a definition: the formula's own value there is 2 w_j t_j / 1e-10).  Float64 after the load, no fused multiply-add, na and nb with
 * the forward's bits, one fixed order of operations per pixel (the header of csrc/lpips.hip): bit-identical to the ordered float64
 * host restatement and on every call.  Every feature element is read once, every gradient element written once; no workspace, no
 * atomics.  fb gets no gradient.  PESR_EINVAL (nothing launched): C not 64, 128, 256 or 512, N < 1 or N > 65535, a side < 1, fa, fb
 * or ga not on a 16-byte boundary, g not on 8.  64-bit offsets. */
int pesr_lpips_layer_bwd(const float* fa, const float* fb, const float* w, const double* g, float* ga, int N, int H, int W, int C,
                         void* stream);

/* ---- DISTS (docs/modes.md section 4t): the L2 pooling of its VGG16 trunk and the head of one stage ------- */
/* x: fp32 NHWC [N][H][W][C] -> y [N][ceil(H/2)][ceil(W/2)][C] = sqrt(conv(x * x, g, stride 2, zero padding 1, depthwise) + 1e-12),
 * g = [1,2,1] (x) [1,2,1] / 16.  Forward only.  fp32, nothing fused, one fixed order inside a window (the header of csrc/dists.hip):
 * nine squares, eight additions, the + 1e-12 and the square root round (the weights are powers of two).  PESR_EINVAL (nothing
 * launched): C not a multiple of 64, N, H or W < 1, x or y not on a 16-byte boundary.  64-bit offsets.  pesr_l2pool_blocks: the
 * workgroups a shape takes (each 256 lanes of four channels of one output pixel), 0 for a shape the kernel does not take; host only. */
long pesr_l2pool_blocks(int N, int H, int W, int C);
int pesr_l2pool_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);

/* The head of one stage.  feat: fp32 NHWC [2N][H][W][C], entries 0 .. N-1 the features of image a, N .. 2N-1 those of image b; C in
 * {3, 64, 128, 256, 512} (3: stage 0, the image itself as NHWC).  alpha, beta: C device doubles each, the stage's slices of
 * alpha / w and beta / w.  Per pair and channel over the P = H * W pixels, in float64: mu_a, mu_b = sum / P, var_a = sum((a - mu_a)^2)
 * / P, var_b likewise, cov = sum((a - mu_a)(b - mu_b)) / P (the centred two-pass form: the features are read twice);
 * S1 = (2 mu_a mu_b + 1e-6) / (mu_a^2 + mu_b^2 + 1e-6), S2 = (2 cov + 1e-6) / (var_a + var_b + 1e-6);
 * out: N device doubles, sum_c alpha_c S1_c + beta_c S2_c.  stats_or_null: when non-null [N][C][5] doubles {mu_a, mu_b, var_a, var_b,
 * cov} are written too; out is the same bits either way.  No fused multiply-add, no atomics, every sum in an order that depends on
 * (P, C) alone (partials per block of 256 pixels, combined in ascending block order): bit-identical to the ordered float64 host
 * restatement and on every call.  pesr_dists_pixel_blocks and pesr_dists_workspace_bytes are pure host functions of the shape (P
 * pixels per image) and return 0 for a shape the kernels do not take; a smaller workspace -> PESR_EWORKSPACE.  PESR_EINVAL (nothing
 * launched): another C, N < 1 or N > 32767, a side < 1.  64-bit offsets. */
long pesr_dists_pixel_blocks(int N, long P, int C);
size_t pesr_dists_workspace_bytes(int N, long P, int C);
int pesr_dists_layer(const float* feat, const double* alpha, const double* beta, double* out, int N, int H, int W, int C,
                     double* stats_or_null, void* workspace, size_t ws_bytes, void* stream);

/* ---- channel attention of a residual block (docs/modes.md section 4u; RCAN's RCAB): squeeze, excite, scale ------- */
/* With t = the block's second conv output, fp32 NHWC [N][HW][C], R = C / reduction hidden units and a = res_scale:
 *     m[n][c] = (1/HW) sum_p t[n][p][c];  h[n][j] = relu(sum_c w1[j][c] m[n][c] + b1[j]);  s[n][c] = sigmoid(sum_j w2[c][j] h[n][j] + b2[c]);
 *     y = x + a * t * s[n][c]
 * backward: ds[n][c] = a sum_p gy * t -> (gate backward) -> dm, dw1, db1, dw2, db2;  gt = a * gy * s + dm / HW;  gx = gy.
 * w1 [R][C], b1 [R], w2 [C][R], b2 [C], m, s, ds, dm [N][C], h [N][R], all fp32.  Shapes: C % 4 == 0, 4 <= C <= 2048, 1 <= R <= C,
 * N >= 1, 1 <= HW <= 2^30; anything else, a NULL tensor or an activation tensor off a 16-byte boundary is PESR_EINVAL with nothing
 * launched, a workspace below pesr_ca_workspace_bytes PESR_EWORKSPACE.  Vector loads and stores only, no atomics, every sum in an
 * order that depends on the shape alone: the same bits on every call.  64-bit element offsets.
 * The pixel sums (pesr_ca_pool, pesr_ca_ds) run in two stages: one workgroup per (image, chunk of pixels) adds its pixels in fp32 (for
 * ds with one fused multiply-add per pixel) and leaves a row in the workspace; the rows are added in double in the fixed order of
 * the library's second stage, scaled (by 1 / HW, by a) and rounded once.  pesr_ca_pool_partials: the chunks per image of that rule, a
 * pure host function of the shape (0: a shape the kernels do not take) - at least eight pixels per lane, about 2048 workgroups in all.
 * In the gate backward the batch sums of the parameter gradients run in increasing n. */
int pesr_ca_pool_partials(int N, long HW, int C);
size_t pesr_ca_workspace_bytes(int N, long HW, int C, int R);
int pesr_ca_pool(const float* t, float* m, int N, long HW, int C, void* workspace, size_t ws_bytes, void* stream);
int pesr_ca_ds(const float* gy, const float* t, float* ds, int N, long HW, int C, float res_scale, void* workspace, size_t ws_bytes,
               void* stream);
int pesr_ca_gate_fwd(const float* m, const float* w1, const float* b1, const float* w2, const float* b2, float* h, float* s, int N,
                     int C, int R, void* stream);
int pesr_ca_apply_fwd(const float* x, const float* t, const float* s, float* y, int N, long HW, int C, float res_scale, void* stream);
int pesr_ca_gate_bwd(const float* ds, const float* s, const float* h, const float* m, const float* w1, const float* w2, float* dm,
                     float* dw1, float* db1, float* dw2, float* db2, int N, int C, int R, void* workspace, size_t ws_bytes,
                     void* stream);
int pesr_ca_apply_bwd(const float* gy, const float* s, const float* dm, float* gt, int N, long HW, int C, float res_scale, void* stream);

/* ---- the U-Net discriminator's own kernels (docs/modes.md section 4v): bilinear x2, the GAN loss of a logit map, conv C -> 1 -------- */
/* All fp32, no atomics, every sum in an order that depends on the shape alone (the same bits on every call), size_t element offsets;
 * a bad argument is PESR_EINVAL with nothing launched, a workspace below the stated size PESR_EWORKSPACE.
 * pesr_bilinear_up2_fwd: NHWC a (and b, or NULL) [N][H][W][C] -> y [N][2H][2W][C] = up2(a + b), up2 = F.interpolate(scale_factor=2,
 *   mode='bilinear', align_corners=False): per axis out[2i] = 0.25 in[max(i-1,0)] + 0.75 in[i], out[2i+1] = 0.75 in[i] + 0.25 in[min(i+1,n-1)].
 *   Any N, H, W, C >= 1 (H, W <= 2^29); 16-byte accesses where C % 4 == 0 and the tensors are 16-byte aligned, scalar ones otherwise.
 * pesr_bilinear_up2_bwd: gy [N][2H][2W][C] -> gx [N][H][W][C], the exact adjoint in gather form: each gx pixel adds its 16 weighted gy
 *   pixels (rows clamp(2i-1), 2i, 2i+1, clamp(2i+2) with 0.25, 0.75, 0.75, 0.25, the same along x) in a fixed order; the clamp folds
 *   the border taps onto the edge pixel.  gx is the gradient of both addends.
 * pesr_gan_loss_map: pesr_gan_loss_fwd_bwd's definitions (gan_type 0 SGAN, 1 RSGAN, 2 RaSGAN; side 0 discriminator, 1 generator; focal
 *   on side 1 only) on n >= 1 logits: out[0] = scale * mean over the n elements, d_real / d_fake [n] = scale * d/dlogit (either may be
 *   NULL).  RSGAN pairs the logits of one index; RaSGAN's means run over all n logits.  workspace >= pesr_gan_loss_map_workspace_bytes(n).
 * pesr_conv3x3_c1_*: the 3 x 3 conv (pad 1, stride 1) from C channels to ONE on the OIHW weights w [1][C][3][3]: x, dx [N][H][W][C],
 *   y, dy [N][H][W]; C % 4 == 0, 4 <= C <= 1024, N H W < 2^31, x / dx 16-byte aligned.  fwd: bias [1] or NULL.  wgrad: dw [1][C][3][3]
 *   and db [1] (or NULL), both times alpha; workspace >= pesr_conv3x3_c1_wgrad_workspace_bytes (0: a shape the kernels do not take). */
int pesr_bilinear_up2_fwd(const float* a, const float* b_or_null, float* y, int N, int H, int W, int C, void* stream);
int pesr_bilinear_up2_bwd(const float* gy, float* gx, int N, int H, int W, int C, void* stream);
size_t pesr_gan_loss_map_workspace_bytes(long n);
int pesr_gan_loss_map(const float* pred_real, const float* pred_fake, long n, int gan_type, int side, int focal, float gamma, float scale,
                      float* out, float* d_real, float* d_fake, void* workspace, size_t ws_bytes, void* stream);
size_t pesr_conv3x3_c1_wgrad_workspace_bytes(int N, int H, int W, int C);
int pesr_conv3x3_c1_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, void* stream);
int pesr_conv3x3_c1_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, void* stream);
int pesr_conv3x3_c1_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int C, float alpha, void* workspace,
                          size_t ws_bytes, void* stream);

/* ---- window self-attention of the Generator's attention blocks (docs/modes.md section 4w) ---------------------------------------- */
/* qkv fp32 NHWC [N][H][W][3 D]: channels 0..D-1 q, D..2D-1 k, 2D..3D-1 v, head h the channels 32h..32h+31 of each.  Windows of 8 x 8
 * pixels on a grid with its origin at (-shift, -shift); positions outside the image are no tokens.  Per window and head, over its
 * tokens: S = q k^T / sqrt(32), A = softmax over the keys (row maximum subtracted), o = A v -> out [N][H][W][D].
 * backward: dout [N][H][W][D] -> dqkv [N][H][W][3 D] (dv = A^T do, dA = do v^T, dS = A (dA - rowsum(dA A)), dq = dS k / sqrt(32),
 * dk = dS^T q / sqrt(32)), every element written once, no zero-fill needed; S and A are recomputed from qkv, nothing else is kept.
 * fp32 MFMA products, no atomics, fixed summation orders: the same bits on every call.  64-bit element offsets.
 * PESR_EINVAL with nothing launched (checked before any device call): D < 32, D % 32, D > 1024, shift outside 0..7, N, H or W < 1,
 * more than 2^31 - 1 windows, a NULL tensor or one off a 16-byte boundary. */
int pesr_window_attention_fwd(const float* qkv, float* out, int N, int H, int W, int D, int shift, void* stream);
int pesr_window_attention_bwd(const float* qkv, const float* dout, float* dqkv, int N, int H, int W, int D, int shift, void* stream);

/* ---- LayerNorm over the channels of each pixel, in front of the window attention (docs/modes.md section 4x) ------------------------- */
/* x fp32 [P][C] (the P = N H W pixels of an NHWC tensor), gamma, beta [C].  Per pixel: mean = (1/C) sum_c x, var = (1/C) sum_c
 * (x - mean)^2 (centred, from the values held in registers), rstd = 1 / sqrt(var + eps), xh = (x - mean) rstd, y = xh gamma + beta;
 * stats [P][2] = (mean, rstd) is what the backward keeps.
 * backward: g = dy gamma, dx = rstd (g - mean_c(g) - xh mean_c(g xh)), dgamma_c = sum_p dy xh, dbeta_c = sum_p dy.  The channel sums
 * leave one row per workgroup in workspace [pesr_layernorm_partials(P, C)][2 C] (pesr_layernorm_workspace_bytes), added in double in
 * row order by a second launch of the same call.  dx, dgamma and dbeta are written exactly once, no zero-fill needed; no atomics,
 * fixed summation orders: the same bits on every call.  The number of workgroups and rows depends on (P, C) alone; 64-bit element
 * offsets.  pesr_layernorm_partials / _workspace_bytes are host-only and return 0 for a shape the kernels do not take.
 * PESR_EINVAL with nothing launched (checked before any device call): C no multiple of 4 from 4 to 1024, P < 1, eps not positive and
 * finite, a NULL pointer or one off a 16-byte boundary (stats and workspace included). */
int pesr_layernorm_partials(long P, int C);
size_t pesr_layernorm_workspace_bytes(long P, int C);
int pesr_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stats, long P, int C, float eps,
                       void* stream);
int pesr_layernorm_bwd(const float* x, const float* gamma, const float* stats, const float* dy, float* dx, float* dgamma, float* dbeta,
                       void* workspace, long P, int C, void* stream);

/* ---- backward of the upsampler's tail: conv C -> 4C, PixelShuffle(2), conv C -> 3 (reference model/basic.py:56-60), as the backward
 * of one virtual 3 x 3 conv V from C to 64 channels (48 used) at the resolution of the tail's input h [N][H][W][C]
 * (docs/experiments/upsample_tail.md has the algebra).  w2 OIHW [4C][C][3][3], b2 [4C], w4 OIHW [3][C][3][3], all fp32; C % 16 == 0,
 * 16 <= C <= 4096, else PESR_EINVAL with nothing launched.  No workspace, no atomics, no host synchronisation; the compose and chain
 * sums run in double in one fixed order and are rounded once: the same bits on every call. */
/* g: dL/d(output) NHWC [N][2H][2W][3] -> gw NHWC [N][H][W][64] (on a 16-byte boundary), channel z = (k*4+p)*4+q (k < 3; p, q < 4) =
 * g[n][2y-1+p][2x-1+q][k], zero outside the image; channels 48..63 zero.  Values are copied exactly.  64-bit offsets. */
int pesr_upsample_tail_gather(const float* g, float* gw, int N, int H, int W, void* stream);
/* weff OIHW [64][C][3][3] = V's weight: weff[z] = sum over m = 4c+2i+j of w4[k][c][i+2-p][j+2-q] * w2[m] where both taps lie in 0..2;
 * rows 48..63 zero. */
int pesr_upsample_tail_compose(const float* w2, const float* w4, float* weff, int C, void* stream);
/* S [64][C][3][3], T [64]: V's weight and bias gradient from (h, gw) (pesr_conv3x3_wgrad) -> dw2 [4C][C][3][3], db2 [4C],
 * dw4 [3][C][3][3], db4 [3]; each may be NULL (not wanted; b2 NULL: no bias).  accumulate = 1 adds to them. */
int pesr_upsample_tail_chain(const float* w2, const float* b2_or_null, const float* w4, const float* S, const float* T,
                             float* dw2_or_null, float* db2_or_null, float* dw4_or_null, float* db4_or_null, int C, int accumulate,
                             void* stream);

/* ---- tiled inference (docs/modes.md section 4h): tiles of one LR image -> a batch, a batch's outputs -> the image ------- */
/* Gather.  src: the LR image, fp32 [3][H][W] (src_u8 = 0) or uint8 [H][W][3] (src_u8 = 1).  desc: n rows of 3 int32 {y0, x0, m}:
 * tile origin and ensemble member m in 0..7 = entry m of test.py:x8_forward's inputs (bit 0 reverses the W axis, then bit 1 the H
 * axis, then bit 2 transposes).  dst: fp32 [n][3][oh][ow]; the tile read for an entry is oh x ow (m < 4) or ow x oh (m >= 4).
 * Values are copied exactly.  desc_host is checked here, desc_dev (the same rows on the device) is what the kernel reads.
 * PESR_EINVAL (nothing launched): a tile outside the image, m outside 0..7, n < 1 or n > 65535. */
int pesr_tile_gather(const void* src, int src_u8, int H, int W, float* dst, const int* desc_host, const int* desc_dev, int n,
                     int oh, int ow, void* stream);
/* Scatter.  n entries, E = 1 or 8 consecutive ones per tile, each the Generator's fp32 output [3][s*th][s*tw] of a th x tw tile
 * (members 4-7: [3][s*tw][s*th]), stored channel-first (t_nhwc = 0) or channel-last (1).  t_hi = NULL: t_lo holds every entry
 * (E = 8 needs th == tw then); else t_lo holds members 0-3 and t_hi members 4-7 of every tile, four entries per tile each.
 * desc: n / E rows of 6 int32 {y0, x0, oy, ox, oh, ow}: the tile's origin and the rectangle of LR pixels it owns (origin, rows,
 * columns; image coordinates).  For every owned output pixel: undo each member's transform (transpose, then H, then W),
 * v = t0 or (((((((t0+t1)+t2)+t3)+t4)+t5)+t6)+t7)/8, out = v or wa*p + wb*v (p_or_null: [n/E][3][s*th][s*tw], layout p_nhwc), fp32,
 * no fused multiply-add.  out_f32: [3][s*H][s*W]; out_u8: [s*H][s*W][3], clamped to 0..255 and rounded half to even; either may be
 * NULL.  The owned rectangles must not overlap (not checked): each pixel is then written once, no atomics, same bits every run.
 * PESR_EINVAL (nothing launched): E not 1 or 8, n not a multiple of E, s outside 2..4, a tile outside the image, an owned rectangle
 * outside its tile or empty, both outputs NULL, more than 65535 tiles. */
int pesr_tile_scatter(const float* t_lo, const float* t_hi, int t_nhwc, const float* p_or_null, int p_nhwc, float wa, float wb,
                      const int* desc_host, const int* desc_dev, int n, int E, int th, int tw, int s, int H, int W,
                      float* out_f32_or_null, unsigned char* out_u8_or_null, void* stream);

/* ---- GAN losses on the [B][1] logits (reference train.py:132-133,210-213,244-253; model/focal_loss.py:9-13), value and both
 * gradients in one launch.  gan_type 0 SGAN, 1 RSGAN, 2 RaSGAN (an extension: batch means over the B samples given);
 * side 0 = discriminator loss (BCE), 1 = generator loss (BCE, or the reference's FocalLoss when focal = 1, with the torch-0.4
 * gradient through its weight AND the BCE term).  out[0] = scale * loss; d_real / d_fake [B] = scale * dloss/dlogit, may be NULL.
 * B <= 1024. */
int pesr_gan_loss_fwd_bwd(const float* pred_real, const float* pred_fake, int B, int gan_type, int side, int focal, float gamma,
                          float scale, float* out, float* d_real, float* d_fake, void* stream);

/* ---- fused Adam on one flat buffer (reference train.py:124-125; torch.optim.Adam) ---------------- */
/* g is multiplied by grad_scale first (1/world_size after a sum all-reduce). step is 1-based. */
int pesr_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                   int step, float grad_scale, void* stream);

/* The same Adam step with its step-dependent scalars in DEVICE memory, for hipGraph replay (a captured launch replays its kernel
 * arguments): state = 6 floats {lr, unused, lr/bc1, sqrt(bc2), step count low 32 bits, high 32 bits (bit patterns)}.  The call
 * first advances the step count and recomputes state[2..3] in double (reference train.py:124-125 / torch.optim.Adam's
 * bias_correction1/2), then applies the update.  The host writes state[0] (StepLR, reference train.py:127-128) between replays. */
int pesr_adam_step_dev(float* p, const float* g, float* m, float* v, long n, float* state, float beta1, float beta2, float eps,
                       float grad_scale, void* stream);

/* Both forms of the step with an exponential moving average of the parameters kept in the same launch (an extension: the
 * ema_decay of ESRGAN-style trainers): after p' is formed, ema' = ema + (p' - ema) * (1 - ema_decay), in fp32, with (1 - ema_decay)
 * formed once on the host.  p, m, v come out bit-identical to pesr_adam_step / pesr_adam_step_dev on the same inputs.  ema has n
 * floats.  PESR_EINVAL, with nothing launched, for n % 4 != 0, ema == NULL, ema_decay outside (0, 1), and as for the plain forms
 * step < 1 / state == NULL. */
int pesr_adam_ema_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                       int step, float grad_scale, float* ema, float ema_decay, void* stream);
int pesr_adam_ema_step_dev(float* p, const float* g, float* m, float* v, long n, float* state, float beta1, float beta2, float eps,
                           float grad_scale, float* ema, float ema_decay, void* stream);

/* ---- convs whose epilogue leaves the BatchNorm sums (round 6, ABI 18): SURVEY K10 for the Discriminator's BasicBlocks (reference
 * model/basic.py:26-30: conv -> BatchNorm2d(train) -> LeakyReLU).  Replaces aten::native_batch_norm's statistics pass and
 * aten::native_batch_norm_backward's reduction pass: the conv kernel that WRITES a tensor also leaves, per pixel tile, the per-channel sums the
 * BatchNorm needs of it - no pass of its own over the tensor, no atomics (one row of [2][C] floats per pixel tile, added up in a fixed order
 * by pesr_bn_finalize / pesr_bn_lrelu_bwd_fused).
 *   mode PESR_BN_FWD_STATS      rows hold sum(y), sum(y^2) of the stored output y (a conv in front of a BatchNorm);
 *   mode PESR_BN_BWD_MASK_SUMS  the kernel is the input gradient that produces the gradient g of a BatchNorm + LeakyReLU OUTPUT; it stores
 *                               g' = g * lrelu'(gamma * xhat(z) + beta) instead of g and the rows hold sum(g'), sum(g' * xhat).
 * pesr_conv3x3_bn_rows(which, ...): rows the call will write - 0 when the fused form does not cover the shape (split-K layers, odd channel
 * counts): the caller then uses the un-fused calls.  which: 0 = pesr_conv3x3_fwd_bn, 1 = pesr_conv3x3_dgrad_bn, 2 = pesr_conv3x3_wino4_bn
 * (arguments as that call takes them).  Workspace sizes: as for the un-fused calls. */
#define PESR_BN_FWD_STATS 1
#define PESR_BN_BWD_MASK_SUMS 2
typedef struct PesrBnFuse {
    int mode;
    int rows;                     /* capacity of `part` in rows of 2 * C floats */
    float* part;                  /* [rows][2][C], written by the conv kernel */
    const float* z;               /* PESR_BN_BWD_MASK_SUMS: the BatchNorm's input, shape of the conv's output */
    const float* mean_invstd;     /* PESR_BN_BWD_MASK_SUMS: [2][C] saved by the forward */
    const float* gamma;
    const float* beta;
    float slope;                  /* negative slope of the activation behind the BatchNorm */
} PesrBnFuse;
long pesr_conv3x3_bn_rows(int which, int N, int H, int W, int Cin, int Cout, int stride);
int pesr_conv3x3_fwd_bn(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int stride,
                        void* workspace, size_t ws_bytes, const PesrBnFuse* fuse, void* stream);
int pesr_conv3x3_dgrad_bn(const float* dy, const float* w_packed_dgrad, float* dx, int N, int H, int W, int Cin, int Cout, int stride,
                          void* workspace, size_t ws_bytes, const PesrBnFuse* fuse, void* stream);
int pesr_conv3x3_wino4_bn(const float* x, const float* w_packed, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                          void* workspace, size_t ws_bytes, const PesrBnFuse* fuse, void* stream);
/* rows of sums -> mean / invstd [2][C] (+ running statistics, num_batches_tracked as nn.BatchNorm2d updates them); M = N * H * W */
int pesr_bn_finalize(const float* part, int rows, int C, long M, float eps, float momentum, float* mean_invstd, float* running_mean,
                     float* running_var, long long* num_batches, void* stream);
/* rows of (sum g', sum g' xhat) + the masked gradient g' -> dz = gamma invstd (g' - mean g' - xhat mean(g' xhat)), dgamma, dbeta (NULL: not
 * wanted; accumulate: added to).  workspace: 2 * C floats. */
int pesr_bn_lrelu_bwd_fused(const float* z, const float* g_masked, const float* part, int rows, const float* gamma, const float* beta,
                            const float* mean_invstd, float* dz, float* dgamma, float* dbeta, int N, int H, int W, int C, int accumulate,
                            void* workspace, size_t ws_bytes, void* stream);

/* ---- gradient exchange over peer memory (round 5, ABI 15): the replacement of nn.DataParallel's reduce_add (reference
 * train.py:114-118) as a reduce-scatter + all-gather that keeps no workgroup resident - stream wait / write-value operations and
 * peer copies on one stream, ONE small kernel over 1/N of the bytes (pesr_amd/csrc/peer_exchange.hip).
 * pesr_peer_alloc: hipMalloc + zero + the allocation's IPC handle (64 bytes).  pesr_peer_export: IPC handle of the allocation that
 * CONTAINS ptr, ptr's byte offset in it and the allocation's size.  pesr_peer_open / _close: map / unmap another process's
 * allocation.  pesr_peer_allreduce: SUM over the ranks, in place, of args->mine (numel % 4 == 0), enqueued on `stream`; all ranks
 * must call it in the same order with the same numel and the next `epoch` (1, 2, 3, ...). */
typedef struct PesrPeerArgs {
    int rank, world;
    unsigned epoch, pad_;
    float* mine;
    float* peer[16];              /* the same tensor in every rank's buffer as mapped in THIS process (peer[rank] == mine) */
    unsigned* my_flags;           /* [3][16] zero-initialised words of this rank (pesr_peer_alloc), written by the peers */
    unsigned* peer_flags[16];     /* every rank's flag block as mapped in this process */
    float* scratch;               /* (world - 1) * ((numel / world rounded up to a multiple of 4)) floats of this rank */
    size_t numel;
    void* ctx;                    /* pesr_peer_ctx_create(world): one side stream + event per peer, so that a phase's copies use all links at once */
} PesrPeerArgs;
int pesr_peer_ctx_create(int world, void** ctx);
int pesr_peer_ctx_destroy(void* ctx);
int pesr_peer_alloc(size_t bytes, void** ptr, unsigned char* handle64);
int pesr_peer_free(void* ptr);
int pesr_peer_release(void* my_flags, size_t bytes);   /* (ABI 17) abandon a stuck exchange: fill this rank's own flag block with 0xffffffff so that every wait of its streams runs out; the transport is unusable afterwards */
int pesr_peer_export(const void* ptr, unsigned char* handle64, size_t* offset, size_t* alloc_bytes);
int pesr_peer_open(const unsigned char* handle64, void** base);
int pesr_peer_close(void* base);
int pesr_peer_allreduce(const void* args, void* stream);
/* (ABI 18) measurement helper: which engine moves a copy out of a peer mapping?  Times hipMemcpyAsync(dst <- src, bytes) alone, then started
 * while a kernel holds every wave slot of this GPU for hog_us microseconds (100 .. 50000), and that kernel: out_ms[3] = {alone, under the
 * hog, hog}.  A blit kernel waits for the hog, a copy engine does not.  Synchronises its own two streams. */
int pesr_peer_copy_probe(const void* src, void* dst, size_t bytes, int hog_us, float* out_ms);

/* ---- generic k x k conv, odd k != 3 (reference `Conv(in, out, kernel_size, stride, bias)`, model/basic.py:4-7, accepts any
 * kernel size; its networks only use 3): padding k/2, NHWC activations, w OIHW [Cout][Cin][k][k] (not packed).  Plain VALU
 * kernels for completeness - untuned, deterministic.  fwd: y = conv(x, w) + bias (bias may be NULL); dgrad: dx [N][H][W][Cin] from
 * dy [N][OH][OW][Cout]; wgrad: dw OIHW and db (may be NULL). */
int pesr_conv_kxk_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Cout, int k,
                      int stride, void* stream);
int pesr_conv_kxk_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int Cin, int Cout, int k, int stride,
                        void* stream);
int pesr_conv_kxk_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Cout, int k, int stride,
                        void* stream);

/* ---- spectral normalisation of a conv weight (reference model/basic.py:25 `spectral_norm(Conv(...))`: an undefined name there;
 * the evident intent is torch.nn.utils.spectral_norm, whose algorithm - one power iteration per training forward - this is) ---- */
/* w [O][K] (the OIHW tensor as it lies in memory, K = Cin * 9).  update = 1 (training): v <- normalize(W^T u), u <- normalize(W v)
 * in place (x / max(||x||, eps)); always: sigma[0] = u^T W v, w_hat = w / sigma.  workspace: pesr_spectral_norm_workspace_bytes. */
size_t pesr_spectral_norm_workspace_bytes(int O, int K);
int pesr_spectral_norm_fwd(const float* w, float* u, float* v, float* w_hat, float* sigma, int O, int K, int update, float eps,
                           void* workspace, size_t ws_bytes, void* stream);
/* dw = (g - <g, w_hat> u v^T) / sigma for g = dL/d(w_hat), with the u, v, sigma of that forward (constants, as in torch);
 * accumulate = 1 adds to dw. */
int pesr_spectral_norm_bwd(const float* g, const float* w_hat, const float* u, const float* v, const float* sigma, float* dw, int O,
                           int K, int accumulate, void* workspace, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PESR_HIP_H */
