// SSIM on the Y channel, twice: the score with a border shave that test.py and validation report (docs/modes.md section 4g), and the
// same score as a training loss with its gradient with respect to the first image (section 4p).
//
// What both share.  Five maps (x, y, x*x, y*y, x*y) of the luma of rows and columns [shave, H-shave) x [shave, W-shave) are filtered
// with the 11 x 11 Gaussian window of sigma 1.5, separably - height pass, then width pass, "valid" region - each pass
// acc = 0; for k ascending: acc = acc + g[k] * v  in float64 with the product and the sum rounded separately; the map value S and its
// coefficients are ssim_point's expressions in ssim_point's order.  No fused multiply-add anywhere in the filter and the map
// arithmetic: the float64 host restatements (tests/ssim_oracle.py, tests/ssim_loss_oracle.py) reproduce every bit of map, score,
// coefficients and gradient.  Hence `fp contract(off)` and exact_u8.h's plain * and + (the __dmul_rn / __dadd_rn of the HIP headers
// are fused once inlined).  The only v_fma_f64 / v_div_fmas_f64 left in this file's code are those of the IEEE double division's own
// expansion (v_div_scale, v_rcp, the Newton steps, v_div_fmas, v_div_fixup), which is correctly rounded.  No atomics: a lane adds its
// CB values in ascending x, block_sum_d gives one partial per workgroup, and reduce.hip's mean_partials_kernel adds an image's
// partials in a fixed order and divides by Ho*Wo once: the same bits on every run.
//
// Forward, ssim_fwd_kernel: one workgroup of 256 lanes per TH x TW tile of the map of one image.  Every load of the
// (TH+10) x (TW+10) halo of both images is issued before the first luma is formed (one round trip to memory per tile); every pixel is
// converted to luma once and Y stays in LDS.  Height pass: a lane owns one column and RB output rows, walks RB+10 rows of Y down the
// column (lanes read consecutive words: conflict-free) and forms the three products once per input pixel; the five height-filtered
// maps go to LDS as doubles with an odd row stride.  Width pass: a lane owns CB consecutive outputs of one row (one item per lane) and
// reads CB+10 values per map.  Nothing intermediate goes to HBM.
//
// Where the two differ.
//   score  Both images are clipped to 0..255, rounded, converted to the BT.601 luma in double, clipped and rounded again
//          (exact_luma601_u8, the Y image of the PSNR-Y).  Y is an integer in 0..255 and lies in LDS as floats: exact, and half the LDS
//          of doubles.  16 x 48 tile with RB = 4, CB = 3: 232 and 256 of the 256 lanes busy in the two passes, 49 KB of LDS and 150
//          VGPRs (3 workgroups per CU); the tiles it was measured against are in section 4g.  Stores S as [N][Ho][Wo] when `out` is given.
//   loss   Nothing is clipped or rounded: Y = ((r*(65.738/256) + g*(129.057/256)) + b*(25.064/256)) + 16 in double from the fp32
//          values, doubles in LDS; no shave.  16 x 32 tile with RB = 4, CB = 2: 45.0 KB of LDS (2 x 26 x 42 + 5 x 16 x 43 doubles),
//          three workgroups per CU; the score's tile with double Y would need 61.9 KB, two per CU.  Stores the three coefficients
//              ca = dS/dmx, cb = dS/dxx, cc = dS/dxy     (raw moments held fixed)
//          as [N][3][Ho][Wo] doubles when `out` is given.
//
// Backward of the loss, one workgroup per 16 x 32 tile of INPUT pixels.  The transpose of the valid filter is the full correlation
// with the same window; the window is symmetric (g[k] == g[10-k], the same literals), so it is the valid filter of the map padded
// with 10 zeros on every side, and that is what runs: the three coefficient maps of the tile plus a halo of 10 towards the top and the
// left are staged in LDS (zeros outside the map), then the forward's height and width passes give T[ca], T[cb], T[cc] at the tile's
// pixels.  x(q), y(q) are recomputed from a and b (loaded once, before the passes), and
//     u = (T[ca] + (2 x) T[cb]) + y T[cc];   dY = (g[n] / ((double)Ho * (double)Wo)) * u;   da_c = (float)(dY * k_c)
// is stored in a's layout.  Every input element is read once, every gradient element written once; 42.7 KB of LDS, no atomics.
#pragma clang fp contract(off)
#include <type_traits>
#include "common.h"
#include "launchers.h"
#include "exact_u8.h"

// The score's tile and per-lane blocks.  Overridable for experiment builds only (scripts/build_variant.sh, PESR_HIP_LIB).
#ifndef PESR_SSIM_TH
#define PESR_SSIM_TH 16
#define PESR_SSIM_TW 48
#define PESR_SSIM_RB 4
#define PESR_SSIM_CB 3
#endif

constexpr int SSIM_TAPS = 11;
constexpr int SSIM_HALO = SSIM_TAPS - 1;
constexpr int SSIM_THREADS = 256;
constexpr double SSIM_C1 = (0.01 * 255) * (0.01 * 255);
constexpr double SSIM_C2 = (0.03 * 255) * (0.03 * 255);

// g[k] = exp(-(k-5)^2 / 4.5) / sum (ascending k), the doubles that pesr_amd/ops.py SSIM_WINDOW and tests/ssim_oracle.py hold.
// A function of a constant argument after unrolling: the weights are literals in the code.
__device__ __forceinline__ constexpr double ssim_g(int k) {
    const int d = k < 5 ? 5 - k : k - 5;
    return d == 0 ? 0.26601172486179436
         : d == 1 ? 0.2130055377112537
         : d == 2 ? 0.10936068950970002
         : d == 3 ? 0.03600077212843083
         : d == 4 ? 0.007598758135239185
                  : 0.00102838008447911;
}

// A TH x TW tile: RB rows per lane in the height pass, CB columns per lane in the width pass
template <int TH_, int TW_, int RB_, int CB_>
struct SsimTile {
    static constexpr int TH = TH_, TW = TW_, RB = RB_, CB = CB_;
    static constexpr int YH = TH + SSIM_HALO, YW = TW + SSIM_HALO;    // the staged region
    static constexpr int SW = YW | 1;                                 // odd row stride of the height-filtered maps
    static_assert(TH % RB == 0 && TW % CB == 0 && TH * (TW / CB) == SSIM_THREADS, "the width pass has one item per lane");
};
using SsimScoreTile = SsimTile<PESR_SSIM_TH, PESR_SSIM_TW, PESR_SSIM_RB, PESR_SSIM_CB>;
using SsimLossTile = SsimTile<16, 32, 4, 2>;                          // of the loss's forward and backward

// element (c, y, x) of image n of a and b lives at n*3*H*W + c*sc + (y*W + x)*sp
struct SsimStrides {
    long asc, asp, bsc, bsp;
};

// the luma of section 4g without its two clip-and-round steps
__device__ __forceinline__ double ssim_raw_luma(const float (&p)[3]) {
    return (((double)p[0] * (65.738 / 256) + (double)p[1] * (129.057 / 256)) + (double)p[2] * (25.064 / 256)) + 16.0;
}

// Height pass of M maps over the staged T::YH x T::YW region: fetch(i, v) gives the M values at staged element i; the filtered maps go
// to st[m][row * T::SW + column].  A lane owns one column and T::RB output rows.
template <class T, int M, class Fetch>
__device__ __forceinline__ void ssim_height_pass(double* __restrict__ st, int tid, Fetch fetch) {
    for (int item = tid; item < (T::TH / T::RB) * T::YW; item += SSIM_THREADS) {
        const int r0 = (item / T::YW) * T::RB, c = item % T::YW;
        double acc[M][T::RB];
#pragma unroll
        for (int r = 0; r < T::RB; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) acc[m][r] = 0.0;
#pragma unroll
        for (int i = 0; i < T::RB + SSIM_HALO; ++i) {
            double v[M];
            fetch((r0 + i) * T::YW + c, v);
#pragma unroll
            for (int r = 0; r < T::RB; ++r) {
                const int k = i - r;                               // ascending in i for every output row r
                if (k >= 0 && k < SSIM_TAPS) {
#pragma unroll
                    for (int m = 0; m < M; ++m) acc[m][r] = exact_mac(acc[m][r], ssim_g(k), v[m]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < T::RB; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) st[m * (T::TH * T::SW) + (r0 + r) * T::SW + c] = acc[m][r];
    }
}

// Width pass: the T::CB outputs of row r that start at column c0
template <class T, int M>
__device__ __forceinline__ void ssim_width_pass(const double* __restrict__ st, int r, int c0, double (&acc)[M][T::CB]) {
#pragma unroll
    for (int q = 0; q < T::CB; ++q)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m][q] = 0.0;
#pragma unroll
    for (int j = 0; j < T::CB + SSIM_HALO; ++j) {
        double v[M];
#pragma unroll
        for (int m = 0; m < M; ++m) v[m] = st[m * (T::TH * T::SW) + r * T::SW + c0 + j];
#pragma unroll
        for (int q = 0; q < T::CB; ++q) {
            const int k = j - q;
            if (k >= 0 && k < SSIM_TAPS) {
#pragma unroll
                for (int m = 0; m < M; ++m) acc[m][q] = exact_mac(acc[m][q], ssim_g(k), v[m]);
            }
        }
    }
}

// One window: the map value S and the three coefficients of section 4p (a caller that stores only S leaves them to the compiler)
__device__ __forceinline__ double ssim_point(double mx, double my, double xx, double yy, double xy, double (&co)[3]) {
    const double mxmx = mx * mx, mymy = my * my, mxmy = mx * my;
    const double sx = xx - mxmx, sy = yy - mymy, sxy = xy - mxmy;
    const double a1 = 2.0 * mxmy + SSIM_C1, a2 = 2.0 * sxy + SSIM_C2;
    const double b1 = (mxmx + mymy) + SSIM_C1, b2 = (sx + sy) + SSIM_C2;
    const double den = b1 * b2;
    const double s = (a1 * a2) / den;
    co[0] = ((2.0 * my) * (a2 - a1)) / den - ((2.0 * mx) * s) * (1.0 / b1 - 1.0 / b2);
    co[1] = -(s / b2);
    co[2] = (2.0 * a1) / den;
    return s;
}

// grid (tiles_x, tiles_y, N) over the Ho x Wo map; (Ho+10) x (Wo+10) is the shaved image.  QUANT: the score (8-bit luma, floats in LDS,
// out = the map or null); otherwise the loss (raw luma, doubles in LDS, out = the coefficients or null).
template <bool QUANT, class T>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                double* __restrict__ part, double* __restrict__ out, int H, int W,
                                                                int shave, int Ho, int Wo, SsimStrides L) {
    using Y = std::conditional_t<QUANT, float, double>;
    __shared__ Y ya[T::YH * T::YW], yb[T::YH * T::YW];
    __shared__ double st[5 * T::TH * T::SW];
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int oy0 = blockIdx.y * T::TH, ox0 = blockIdx.x * T::TW;
    const int Hs = Ho + SSIM_HALO, Ws = Wo + SSIM_HALO;
    const long img = (long)n * 3 * H * W;

    // halo of both images -> luma, once per pixel; zero outside the shaved image (such values only reach outputs that are dropped).
    // All of a lane's loads are issued before the first luma is formed: one round trip to memory per tile, not one per pixel.
    constexpr int NL = (T::YH * T::YW + SSIM_THREADS - 1) / SSIM_THREADS;
    float pa[NL][3], pb[NL][3];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int idx = tid + l * SSIM_THREADS;
        const int iy = oy0 + idx / T::YW, ix = ox0 + idx % T::YW;
#pragma unroll
        for (int c = 0; c < 3; ++c) pa[l][c] = pb[l][c] = 0.0f;
        if (idx < T::YH * T::YW && iy < Hs && ix < Ws) {
            const long p = (long)(iy + shave) * W + (ix + shave);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pa[l][c] = a[img + p * L.asp + c * L.asc];
                pb[l][c] = b[img + p * L.bsp + c * L.bsc];
            }
        }
    }
    auto luma = [](const float (&p)[3]) {
        if constexpr (QUANT) return exact_luma601_u8(p[0], p[1], p[2]);
        else return ssim_raw_luma(p);
    };
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int idx = tid + l * SSIM_THREADS;
        const int iy = oy0 + idx / T::YW, ix = ox0 + idx % T::YW;
        if (idx < T::YH * T::YW) {
            const bool in = iy < Hs && ix < Ws;
            ya[idx] = in ? (Y)luma(pa[l]) : (Y)0;
            yb[idx] = in ? (Y)luma(pb[l]) : (Y)0;
        }
    }
    __syncthreads();

    ssim_height_pass<T, 5>(st, tid, [&](int i, double (&v)[5]) {
        const double x = (double)ya[i], y = (double)yb[i];
        v[0] = x, v[1] = y, v[2] = x * x, v[3] = y * y, v[4] = x * y;
    });
    __syncthreads();

    const int r = tid / (T::TW / T::CB), c0 = (tid % (T::TW / T::CB)) * T::CB;
    double acc[5][T::CB];
    ssim_width_pass<T, 5>(st, r, c0, acc);
    const int oy = oy0 + r;
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < T::CB; ++q) {
        const int ox = ox0 + c0 + q;
        if (oy < Ho && ox < Wo) {
            double co[3];
            const double s = ssim_point(acc[0][q], acc[1][q], acc[2][q], acc[3][q], acc[4][q], co);
            sum += s;
            if (out) {
                const long o = (((long)n * (QUANT ? 1 : 3)) * Ho + oy) * Wo + ox;
                if constexpr (QUANT) {
                    out[o] = s;
                } else {
#pragma unroll
                    for (int m = 0; m < 3; ++m) out[o + (long)m * Ho * Wo] = co[m];
                }
            }
        }
    }
    __shared__ double red[SSIM_THREADS / 64];
    const double t = block_sum_d(sum, red);
    if (tid == 0) part[((long)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
}

// grid (tiles_x, tiles_y, N) over the H x W image; ga has a's layout
__global__ __launch_bounds__(SSIM_THREADS) void ssim_loss_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                     const double* __restrict__ coef, const double* __restrict__ g,
                                                                     float* __restrict__ ga, int H, int W, int Ho, int Wo,
                                                                     SsimStrides L) {
    using T = SsimLossTile;
    __shared__ double cf[3 * T::YH * T::YW];
    __shared__ double st[3 * T::TH * T::SW];
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int qy0 = blockIdx.y * T::TH, qx0 = blockIdx.x * T::TW;
    const long img = (long)n * 3 * H * W;

    // this lane's T::CB pixels of both images: loaded now, used after the two passes
    const int r = tid / (T::TW / T::CB), c0 = (tid % (T::TW / T::CB)) * T::CB;
    const int qy = qy0 + r;
    float pa[T::CB][3], pb[T::CB][3];
#pragma unroll
    for (int q = 0; q < T::CB; ++q) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pa[q][c] = pb[q][c] = 0.0f;
        if (qy < H && qx0 + c0 + q < W) {
            const long p = (long)qy * W + (qx0 + c0 + q);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pa[q][c] = a[img + p * L.asp + c * L.asc];
                pb[q][c] = b[img + p * L.bsp + c * L.bsc];
            }
        }
    }

    // the three coefficient maps at rows qy0-10 .. qy0+15 and columns qx0-10 .. qx0+31 of the map, zero outside it
    const long cimg = (long)n * 3 * Ho * Wo;
#pragma unroll 4
    for (int idx = tid; idx < 3 * T::YH * T::YW; idx += SSIM_THREADS) {
        const int m = idx / (T::YH * T::YW), rem = idx % (T::YH * T::YW);
        const int oy = qy0 - SSIM_HALO + rem / T::YW, ox = qx0 - SSIM_HALO + rem % T::YW;
        const bool in = oy >= 0 && oy < Ho && ox >= 0 && ox < Wo;
        cf[idx] = in ? coef[cimg + ((long)m * Ho + oy) * Wo + ox] : 0.0;
    }
    __syncthreads();

    ssim_height_pass<T, 3>(st, tid, [&](int i, double (&v)[3]) {
#pragma unroll
        for (int m = 0; m < 3; ++m) v[m] = cf[m * (T::YH * T::YW) + i];
    });
    __syncthreads();

    double t[3][T::CB];
    ssim_width_pass<T, 3>(st, r, c0, t);
    const double scale = g[n] / ((double)Ho * (double)Wo);
#pragma unroll
    for (int q = 0; q < T::CB; ++q) {
        if (qy < H && qx0 + c0 + q < W) {
            const double x = ssim_raw_luma(pa[q]), y = ssim_raw_luma(pb[q]);
            const double u = (t[0][q] + (2.0 * x) * t[1][q]) + y * t[2][q];
            const double dy = scale * u;
            const long p = (long)qy * W + (qx0 + c0 + q);
            ga[img + p * L.asp + 0 * L.asc] = (float)(dy * (65.738 / 256));
            ga[img + p * L.asp + 1 * L.asc] = (float)(dy * (129.057 / 256));
            ga[img + p * L.asp + 2 * L.asc] = (float)(dy * (25.064 / 256));
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// What a launch needs: the size Ho x Wo of the map, the grid of tiles and the strides of both images
struct SsimPlan {
    int Ho, Wo;
    dim3 grid;
    SsimStrides L;
};

// The checks and the arithmetic all three entry points share.  The grid covers the map, or (the backward) the image.
template <class T>
static int ssim_plan(const float* a, const float* b, int N, int H, int W, int a_nhwc, int b_nhwc, int shave, bool over_image,
                     SsimPlan* p) {
    if (!a || !b || N < 1 || N > 65535 || H < 1 || W < 1 || shave < 0) return PESR_EINVAL;
    const long Hs = (long)H - 2L * shave, Ws = (long)W - 2L * shave;
    if (Hs < SSIM_TAPS || Ws < SSIM_TAPS) return PESR_EINVAL;       // no silent smaller window
    p->Ho = (int)Hs - SSIM_HALO, p->Wo = (int)Ws - SSIM_HALO;
    const int gh = over_image ? H : p->Ho, gw = over_image ? W : p->Wo;
    const int tx = (gw + T::TW - 1) / T::TW, ty = (gh + T::TH - 1) / T::TH;
    if (ty > 65535) return PESR_EINVAL;
    p->grid = dim3(tx, ty, N);
    const long P = (long)H * W;
    p->L = SsimStrides{a_nhwc ? 1L : P, a_nhwc ? 3L : 1L, b_nhwc ? 1L : P, b_nhwc ? 3L : 1L};
    return PESR_OK;
}

// forward of either kind: one partial per tile in the workspace, then the mean of an image's partials
template <bool QUANT, class T>
static int ssim_fwd_launch(const float* a, const float* b, double* score, int N, int H, int W, int a_nhwc, int b_nhwc, int shave,
                           double* out, void* ws, size_t ws_bytes, hipStream_t stream) {
    SsimPlan p;
    if (ssim_plan<T>(a, b, N, H, W, a_nhwc, b_nhwc, shave, false, &p) != PESR_OK || !score) return PESR_EINVAL;
    const long tiles = (long)p.grid.x * p.grid.y;
    if (!ws || ws_bytes < (size_t)N * tiles * sizeof(double)) return PESR_EWORKSPACE;
    hipLaunchKernelGGL((ssim_fwd_kernel<QUANT, T>), p.grid, dim3(SSIM_THREADS), 0, stream, a, b, (double*)ws, out, H, W, shave, p.Ho,
                       p.Wo, p.L);
    return pesr_mean_partials_launch((const double*)ws, score, N, tiles, (double)p.Ho * (double)p.Wo, stream);
}

int pesr_ssim_y_launch(const float* a, const float* b, double* out, int N, int H, int W, int a_nhwc, int b_nhwc, int shave,
                       double* map, void* ws, size_t ws_bytes, hipStream_t stream) {
    return ssim_fwd_launch<true, SsimScoreTile>(a, b, out, N, H, W, a_nhwc, b_nhwc, shave, map, ws, ws_bytes, stream);
}

int pesr_ssim_loss_fwd_launch(const float* a, const float* b, double* score, int N, int H, int W, int a_nhwc, int b_nhwc, double* coef,
                              void* ws, size_t ws_bytes, hipStream_t stream) {
    if (((uintptr_t)score | (uintptr_t)coef | (uintptr_t)ws) & 7) return PESR_EINVAL;
    return ssim_fwd_launch<false, SsimLossTile>(a, b, score, N, H, W, a_nhwc, b_nhwc, 0, coef, ws, ws_bytes, stream);
}

int pesr_ssim_loss_bwd_launch(const float* a, const float* b, const double* coef, const double* g, float* ga, int N, int H, int W,
                              int a_nhwc, int b_nhwc, hipStream_t stream) {
    SsimPlan p;
    if (ssim_plan<SsimLossTile>(a, b, N, H, W, a_nhwc, b_nhwc, 0, true, &p) != PESR_OK || !coef || !g || !ga) return PESR_EINVAL;
    if ((((uintptr_t)coef | (uintptr_t)g) & 7) || ((uintptr_t)ga & 3)) return PESR_EINVAL;
    hipLaunchKernelGGL(ssim_loss_bwd_kernel, p.grid, dim3(SSIM_THREADS), 0, stream, a, b, coef, g, ga, H, W, p.Ho, p.Wo, p.L);
    return pesr_launch_status();
}
