// Image-space and feature-space losses of the GAN step, fused forward + gradient (gfx950, HBM-bound).
//   l1_tv : reference train.py:131,137-140,240-242 on sr/hr [N][H][W][3] (NHWC):
//             l1 = mean |sr - hr| ; tv = SUM |sr[..,x]-sr[..,x+1]| + SUM |sr[y]-sr[y+1]|   (a sum)
//             grad = a_l1 * sign(sr-hr)/numel + a_tv * d(tv)/d(sr)
//   mse   : reference train.py:134-136 F.mse_loss(vgg_sr, vgg_hr): mean (a-b)^2, grad_a = g * 2 (a-b)/numel
// Sums go through per-block fp32 partials and a fixed-order double finalize (deterministic).
#include "common.h"
#include "launchers.h"
#include "reduce_rows.h"

__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(256) void l1_tv_kernel(const float* __restrict__ sr, const float* __restrict__ hr, float* __restrict__ grad,
                                                    float* __restrict__ part, int N, int H, int W, float g_l1, float g_tv) {
    // one thread per pixel (3 channels); g_l1 = upstream * alpha_l1 / numel, g_tv = upstream * alpha_tv
    const long total = (long)N * H * W;
    float s_l1 = 0.f, s_tv = 0.f;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int x = (int)(e % W);
        const int y = (int)((e / W) % H);
        const float* p = sr + e * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = p[c];
            const float d = v - hr[e * 3 + c];
            s_l1 += fabsf(d);
            float g = g_l1 * sgn(d);
            float t = 0.f;
            if (x + 1 < W) { const float q = v - p[3 + c]; s_tv += fabsf(q); t += sgn(q); }
            if (x > 0) { t -= sgn(p[c - 3] - v); }
            if (y + 1 < H) { const float q = v - p[(long)W * 3 + c]; s_tv += fabsf(q); t += sgn(q); }
            if (y > 0) { t -= sgn(p[c - (long)W * 3] - v); }
            if (grad) grad[e * 3 + c] = g + g_tv * t;
        }
    }
    __shared__ float red[4][2];
    const float a = wave_sum(s_l1), b = wave_sum(s_tv);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x < 2) part[blockIdx.x * 2 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}
// second stage (fixed-order row reduce, reduce_rows.h) and the scalar finish in one launch
__global__ __launch_bounds__(1024) void l1_tv_final_kernel(const float* __restrict__ part, int nb, float* __restrict__ out, double inv_numel) {
    __shared__ double red[16][64];
    const double t = reduce_rows_block(part, nb, 2, threadIdx.x & 63, (threadIdx.x & 63) < 2, red);
    if (threadIdx.x < 2) out[threadIdx.x] = (float)(threadIdx.x == 0 ? t * inv_numel : t);   // L1 mean, TV sum
}

__global__ __launch_bounds__(256) void mse_kernel(const f32x4* __restrict__ a, const f32x4* __restrict__ b, f32x4* __restrict__ grad,
                                                  float* __restrict__ part, long n4, float gscale) {
    float s = 0.f;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (long)gridDim.x * blockDim.x) {
        const f32x4 d = a[e] - b[e];
        s += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
        if (grad) grad[e] = d * gscale;
    }
    __shared__ float red[4];
    const float w = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(1024) void mse_final_kernel(const float* __restrict__ part, int nb, float* __restrict__ out, double inv_numel) {
    __shared__ double red[16][64];
    const double t = reduce_rows_block(part, nb, 1, 0, (threadIdx.x & 63) == 0, red);
    if (threadIdx.x == 0) out[0] = (float)(t * inv_numel);
}

int pesr_loss_l1_tv_launch(const float* sr, const float* hr, float* grad, float* out2, int N, int H, int W, float g_l1, float g_tv,
                           void* ws, size_t ws_bytes, hipStream_t stream) {
    const int nb = 1024;
    if (!ws || ws_bytes < 64 + (size_t)nb * 2 * sizeof(float)) return PESR_EWORKSPACE;
    double* dsum = (double*)ws;
    float* part = (float*)((char*)ws + 64);
    hipLaunchKernelGGL(l1_tv_kernel, dim3(nb), dim3(256), 0, stream, sr, hr, grad, part, N, H, W, g_l1, g_tv);
    hipLaunchKernelGGL(l1_tv_final_kernel, dim3(1), dim3(1024), 0, stream, (const float*)part, nb, out2, 1.0 / ((double)N * H * W * 3));
    return pesr_launch_status();
}
int pesr_loss_mse_launch(const float* a, const float* b, float* grad, float* out1, long n, float gscale, void* ws, size_t ws_bytes,
                         hipStream_t stream) {
    if (n % 4) return PESR_EINVAL;
    const int nb = 512;
    if (!ws || ws_bytes < 64 + (size_t)nb * sizeof(float)) return PESR_EWORKSPACE;
    double* dsum = (double*)ws;
    float* part = (float*)((char*)ws + 64);
    hipLaunchKernelGGL(mse_kernel, dim3(nb), dim3(256), 0, stream, (const f32x4*)a, (const f32x4*)b, (f32x4*)grad, part, n / 4, gscale);
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(1024), 0, stream, (const float*)part, nb, out1, 1.0 / (double)n);
    return pesr_launch_status();
}

// ------------------------------------------------------------------------------------------------
// Validation PSNR on the device (reference utils.py:10-18,32-41): both images are clipped to 0..255 and rounded to
// uint8 values, converted to the BT.601 luma y = (65.738 r + 129.057 g + 25.064 b)/256 + 16 in DOUBLE (as numpy does),
// clipped and rounded again, and the squared differences are summed.  Every term is an integer-valued double, so the sum
// is exact whatever its order: the result is bit-identical to the host computation.
// Element (n = 0, c, y, x) of a logical NCHW tensor lives at c*sc + (y*W + x)*sp.
// luma_u8 is exact_u8.h's exact_luma601_u8 step for step, compiled under this file's default contraction (that header switches
// contraction off for whatever includes it, which would change psnr_y_kernel's code): it stays a copy.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double luma_u8(const float* p, long sc) {
    const double r = rint(fmin(fmax((double)p[0], 0.0), 255.0));
    const double g = rint(fmin(fmax((double)p[sc], 0.0), 255.0));
    const double b = rint(fmin(fmax((double)p[2 * sc], 0.0), 255.0));
    const double y = ((r * (65.738 / 256) + g * (129.057 / 256)) + b * (25.064 / 256)) + 16.0;
    return rint(fmin(fmax(y, 0.0), 255.0));
}
__global__ __launch_bounds__(256) void psnr_y_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ part,
                                                     long P, long asc, long asp, long bsc, long bsp) {
    double s = 0.0;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long)gridDim.x * blockDim.x) {
        const double d = luma_u8(a + p * asp, asc) - luma_u8(b + p * bsp, bsc);
        s += d * d;
    }
    __shared__ double red[4];
    const double t = block_sum_d(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}
__global__ void psnr_final_kernel(const double* __restrict__ part, double* __restrict__ out, int nb, double inv_n) {
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < nb; ++k) s += part[k];
        const double mse = s * inv_n;
        out[0] = mse;
        out[1] = 20.0 * log10(255.0 / sqrt(mse));
    }
}
int pesr_psnr_y_launch(const float* a, const float* b, double* out2, int H, int W, int a_nhwc, int b_nhwc, void* ws, size_t ws_bytes,
                       hipStream_t stream) {
    const int nb = 256;
    if (!ws || ws_bytes < (size_t)nb * sizeof(double)) return PESR_EWORKSPACE;
    const long P = (long)H * W;
    hipLaunchKernelGGL(psnr_y_kernel, dim3(nb), dim3(256), 0, stream, a, b, (double*)ws, P, a_nhwc ? 1L : P, a_nhwc ? 3L : 1L,
                       b_nhwc ? 1L : P, b_nhwc ? 3L : 1L);
    hipLaunchKernelGGL(psnr_final_kernel, dim3(1), dim3(64), 0, stream, (const double*)ws, out2, nb, 1.0 / (double)P);
    return pesr_launch_status();
}

// ------------------------------------------------------------------------------------------------
// GAN losses on the [B, 1] logits (reference train.py:132-133,210-213,244-253 and model/focal_loss.py:9-13): value and the
// gradients w.r.t. both logit vectors in ONE launch instead of ~25 scalar-sized ATen kernels per loss (sigmoid, log_sigmoid, sub,
// mul, mean, their backward ...).  B <= 1024, one block.
//   side 0 (discriminator): SGAN  BCE(r, 1) + BCE(f, 0)            RSGAN  BCE(r - f, 1)      RaSGAN [BCE(r - mean f, 1) + BCE(f - mean r, 0)] / 2
//   side 1 (generator):     SGAN  L(f, 1)                          RSGAN  L(f - r, 1)        RaSGAN [L(r - mean f, 0) + L(f - mean r, 1)] / 2
//   L = BCE-with-logits, or (focal = 1) the reference's FocalLoss with the torch-0.4 gradient through w = (1 - pt)^gamma AND the
//   BCE term: dL/dx = [dw/dx * bce + w * (p - t)] / B,  dw/dx = -gamma (1 - pt)^(gamma - 1) (2t - 1) p (1 - p).
// All means are over the B samples given (the data-parallel RaSGAN, whose batch means span the ranks, stays on the torch path).
// out[0] = scale * loss;  d_real / d_fake [B] = scale * dloss/dlogit (either may be NULL).
// ------------------------------------------------------------------------------------------------
namespace {
__device__ __forceinline__ float bce_logits(float x, float t) {              // as ATen: (1 - t) x + max(-x, 0) + log(exp(-m) + exp(-x - m))
    const float m = fmaxf(-x, 0.f);
    return (1.f - t) * x + m + logf(expf(-m) + expf(-x - m));
}
__device__ __forceinline__ void loss_term(float x, float t, int focal, float gamma, float* val, float* dx) {
    const float p = 1.f / (1.f + expf(-x));
    const float bce = bce_logits(x, t);
    if (!focal) { *val = bce; *dx = p - t; return; }
    const float pt = p * t + (1.f - p) * (1.f - t);
    const float w = powf(1.f - pt, gamma);
    const float dw = gamma == 0.f ? 0.f : -gamma * powf(1.f - pt, gamma - 1.f) * (2.f * t - 1.f) * p * (1.f - p);
    *val = w * bce;
    *dx = dw * bce + w * (p - t);
}
__device__ __forceinline__ double block_sum1024(double v, double* red) {     // fixed order over the 16 waves
    const double w = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < 16; ++k) s += red[k];
    return s;
}
}  // namespace

__global__ __launch_bounds__(1024) void gan_loss_kernel(const float* __restrict__ pr, const float* __restrict__ pf, int B, int gan, int side,
                                                        int focal, float gamma, float scale, float* __restrict__ out,
                                                        float* __restrict__ d_real, float* __restrict__ d_fake) {
    __shared__ double red[16];
    const int i = threadIdx.x;
    const bool on = i < B;
    const float r = on ? pr[i] : 0.f, f = on ? pf[i] : 0.f;
    const float invB = 1.0f / (float)B;
    float val = 0.f, gr = 0.f, gf = 0.f;                   // per-sample loss term(s) and d(sum of terms)/d(r_i), d/d(f_i) before the 1/B
    const int fo = side == 1 ? focal : 0;                  // the discriminator side is plain BCE in the reference
    if (gan == 0) {                                        // SGAN
        if (side == 0) {
            float v1, g1, v2, g2;
            loss_term(r, 1.f, 0, 0.f, &v1, &g1); loss_term(f, 0.f, 0, 0.f, &v2, &g2);
            val = v1 + v2; gr = g1; gf = g2;
        } else { loss_term(f, 1.f, fo, gamma, &val, &gf); }
    } else if (gan == 1) {                                 // RSGAN
        float g;
        if (side == 0) { loss_term(r - f, 1.f, 0, 0.f, &val, &g); gr = g; gf = -g; }
        else { loss_term(f - r, 1.f, fo, gamma, &val, &g); gf = g; gr = -g; }
    }
    if (gan == 2) {                                        // RaSGAN: two passes (the means first)
        const float mr = (float)(block_sum1024(on ? (double)r : 0.0, red)) * invB;
        const float mf = (float)(block_sum1024(on ? (double)f : 0.0, red)) * invB;
        float va, ga, vb, gb;
        loss_term(r - mf, side == 0 ? 1.f : 0.f, fo, gamma, &va, &ga);
        loss_term(f - mr, side == 0 ? 0.f : 1.f, fo, gamma, &vb, &gb);
        if (!on) { va = vb = ga = gb = 0.f; }
        const float sa = (float)block_sum1024((double)ga, red), sb = (float)block_sum1024((double)gb, red);
        val = 0.5f * (va + vb);
        gr = 0.5f * (ga - sb * invB);                      // r_i also moves every b_j through mean r
        gf = 0.5f * (gb - sa * invB);
    }
    if (!on) val = 0.f;
    const double tot = block_sum1024((double)val, red);
    if (i == 0) out[0] = scale * (float)(tot * (double)invB);
    if (on) {
        if (d_real) d_real[i] = scale * gr * invB;
        if (d_fake) d_fake[i] = scale * gf * invB;
    }
}

int pesr_gan_loss_launch(const float* pred_real, const float* pred_fake, int B, int gan, int side, int focal, float gamma, float scale,
                         float* out, float* d_real, float* d_fake, hipStream_t stream) {
    if (B < 1 || B > 1024 || gan < 0 || gan > 2 || side < 0 || side > 1) return PESR_EINVAL;
    hipLaunchKernelGGL(gan_loss_kernel, dim3(1), dim3(1024), 0, stream, pred_real, pred_fake, B, gan, side, focal, gamma, scale, out, d_real,
                       d_fake);
    return pesr_launch_status();
}

// ------------------------------------------------------------------------------------------------
// The same losses on a logit MAP (docs/modes.md section 4v: the U-Net discriminator's [B, 1, H, W] output, or any patch-wise D):
// n = B * H * W logits of any n >= 1, the real and the fake logit of one (b, y, x) paired by their index.  bce_logits / loss_term above
// are the definitions; every mean runs over all n elements.  No atomics: a 256-lane workgroup owns MAP_PER_BLOCK consecutive logits
// (past MAP_MAX_BLOCKS workgroups: every MAP_MAX_BLOCKS-th such chunk), a lane adds its elements in increasing order in fp32, the
// lanes meet in wave_sum's tree and the four waves in order; the workgroups' rows are added in double by reduce_rows.h's second
// stage - an order that depends on n alone.
//   RaSGAN:  sums (r, f per workgroup) -> means (mean r, mean f)  -> terms (value, ga, gb per workgroup) -> final (the value; sa, sb)
//            -> grads (d_real, d_fake, the terms computed again: they are cheaper than a round trip of two more maps)
//   others:  terms (which also writes the gradients) -> final
// Workspace: [0, 64) four floats (mean r, mean f, sa, sb), then the [blocks][2] and [blocks][3] rows.
// ------------------------------------------------------------------------------------------------
#define MAP_LANES 256
#define MAP_PER_BLOCK 1024
#define MAP_MAX_BLOCKS 4096

static int map_blocks(long n) {
    const long nb = (n + MAP_PER_BLOCK - 1) / MAP_PER_BLOCK;
    return (int)(nb < MAP_MAX_BLOCKS ? nb : MAP_MAX_BLOCKS);
}
size_t pesr_gan_loss_map_ws_bytes(long n) { return n < 1 ? 0 : 64 + (size_t)map_blocks(n) * 5 * sizeof(float); }

namespace {
// the fixed-order sum of one value per lane over a 256-lane workgroup, to lane 0 (red: [4] floats of LDS)
__device__ __forceinline__ float map_block_sum(float v, float* red) {
    const float w = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
// the per-element terms: val, and d(sum of terms)/d(r_i), d/d(f_i) before the 1/n.  RaSGAN: ga, gb (the caller adds the mean's part)
__device__ __forceinline__ void map_terms(float r, float f, int gan, int side, int fo, float gamma, float mr, float mf, float* val,
                                          float* gr, float* gf) {
    *gr = 0.f; *gf = 0.f;
    if (gan == 0) {
        if (side == 0) {
            float v1, v2;
            loss_term(r, 1.f, 0, 0.f, &v1, gr); loss_term(f, 0.f, 0, 0.f, &v2, gf);
            *val = v1 + v2;
        } else { loss_term(f, 1.f, fo, gamma, val, gf); }
    } else if (gan == 1) {
        float g;
        if (side == 0) { loss_term(r - f, 1.f, 0, 0.f, val, &g); *gr = g; *gf = -g; }
        else { loss_term(f - r, 1.f, fo, gamma, val, &g); *gf = g; *gr = -g; }
    } else {
        float va, vb;
        loss_term(r - mf, side == 0 ? 1.f : 0.f, fo, gamma, &va, gr);      // ga
        loss_term(f - mr, side == 0 ? 0.f : 1.f, fo, gamma, &vb, gf);      // gb
        *val = 0.5f * (va + vb);
    }
}
}  // namespace

__global__ __launch_bounds__(MAP_LANES) void gan_map_sums_kernel(const float* __restrict__ pr, const float* __restrict__ pf, long n,
                                                                 float* __restrict__ part) {
    __shared__ float red[4];
    float sr = 0.f, sf = 0.f;
    for (long base = (long)blockIdx.x * MAP_PER_BLOCK; base < n; base += (long)gridDim.x * MAP_PER_BLOCK)
        for (long e = base + threadIdx.x; e < base + MAP_PER_BLOCK && e < n; e += MAP_LANES) { sr += pr[e]; sf += pf[e]; }
    const float a = map_block_sum(sr, red), b = map_block_sum(sf, red);
    if (threadIdx.x == 0) { part[blockIdx.x * 2] = a; part[blockIdx.x * 2 + 1] = b; }
}
__global__ __launch_bounds__(1024) void gan_map_means_kernel(const float* __restrict__ part, int nb, double inv_n, float* __restrict__ head) {
    __shared__ double red[16][64];
    const int cl = threadIdx.x & 63;
    const double t = reduce_rows_block(part, nb, 2, cl, cl < 2, red);
    if (threadIdx.x < 2) head[threadIdx.x] = (float)(t * inv_n);
}
// GRADS: the RaSGAN gradient pass (head holds the means and sa, sb); else the terms pass, which writes the gradients of SGAN / RSGAN
template <bool GRADS>
__global__ __launch_bounds__(MAP_LANES) void gan_map_terms_kernel(const float* __restrict__ pr, const float* __restrict__ pf, long n, int gan,
                                                                  int side, int focal, float gamma, float gscale,
                                                                  const float* __restrict__ head, float* __restrict__ part,
                                                                  float* __restrict__ d_real, float* __restrict__ d_fake, float inv_n) {
    __shared__ float red[4];
    const int fo = side == 1 ? focal : 0;
    float mr = 0.f, mf = 0.f, sa = 0.f, sb = 0.f;
    if (gan == 2) { mr = head[0]; mf = head[1]; }
    if (GRADS) { sa = head[2]; sb = head[3]; }
    float sv = 0.f, sga = 0.f, sgb = 0.f;
    for (long base = (long)blockIdx.x * MAP_PER_BLOCK; base < n; base += (long)gridDim.x * MAP_PER_BLOCK)
        for (long e = base + threadIdx.x; e < base + MAP_PER_BLOCK && e < n; e += MAP_LANES) {
            float val, gr, gf;
            map_terms(pr[e], pf[e], gan, side, fo, gamma, mr, mf, &val, &gr, &gf);
            if (GRADS) {                      // r_i also moves every b_j through mean r (and f_i every a_j)
                if (d_real) d_real[e] = gscale * (0.5f * (gr - sb * inv_n));
                if (d_fake) d_fake[e] = gscale * (0.5f * (gf - sa * inv_n));
            } else {
                sv += val; sga += gr; sgb += gf;
                if (gan != 2) {
                    if (d_real) d_real[e] = gscale * gr;
                    if (d_fake) d_fake[e] = gscale * gf;
                }
            }
        }
    if (!GRADS) {
        const float a = map_block_sum(sv, red), b = map_block_sum(sga, red), c = map_block_sum(sgb, red);
        if (threadIdx.x == 0) { part[blockIdx.x * 3] = a; part[blockIdx.x * 3 + 1] = b; part[blockIdx.x * 3 + 2] = c; }
    }
}
__global__ __launch_bounds__(1024) void gan_map_final_kernel(const float* __restrict__ part, int nb, double inv_n, float scale,
                                                             float* __restrict__ out, float* __restrict__ head) {
    __shared__ double red[16][64];
    const int cl = threadIdx.x & 63;
    const double t = reduce_rows_block(part, nb, 3, cl, cl < 3, red);
    if (threadIdx.x == 0) out[0] = scale * (float)(t * inv_n);
    if (threadIdx.x == 1 || threadIdx.x == 2) head[1 + threadIdx.x] = (float)t;       // sa, sb
}

int pesr_gan_loss_map_launch(const float* pred_real, const float* pred_fake, long n, int gan, int side, int focal, float gamma, float scale,
                             float* out, float* d_real, float* d_fake, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (n < 1 || gan < 0 || gan > 2 || side < 0 || side > 1 || !pred_real || !pred_fake || !out) return PESR_EINVAL;
    if (!ws || ws_bytes < pesr_gan_loss_map_ws_bytes(n)) return PESR_EWORKSPACE;
    const int nb = map_blocks(n);
    float* head = (float*)ws;
    float* part1 = (float*)((char*)ws + 64);
    float* part2 = part1 + (size_t)nb * 2;
    const double inv_n = 1.0 / (double)n;
    const float gscale = (float)((double)scale * inv_n);
    if (gan == 2) {
        hipLaunchKernelGGL(gan_map_sums_kernel, dim3(nb), dim3(MAP_LANES), 0, stream, pred_real, pred_fake, n, part1);
        hipLaunchKernelGGL(gan_map_means_kernel, dim3(1), dim3(1024), 0, stream, (const float*)part1, nb, inv_n, head);
    }
    hipLaunchKernelGGL(gan_map_terms_kernel<false>, dim3(nb), dim3(MAP_LANES), 0, stream, pred_real, pred_fake, n, gan, side, focal, gamma,
                       gscale, (const float*)head, part2, d_real, d_fake, (float)inv_n);
    hipLaunchKernelGGL(gan_map_final_kernel, dim3(1), dim3(1024), 0, stream, (const float*)part2, nb, inv_n, scale, out, head);
    if (gan == 2 && (d_real || d_fake))
        hipLaunchKernelGGL(gan_map_terms_kernel<true>, dim3(nb), dim3(MAP_LANES), 0, stream, pred_real, pred_fake, n, gan, side, focal, gamma,
                           gscale, (const float*)head, (float*)nullptr, d_real, d_fake, (float)inv_n);
    return pesr_launch_status();
}
