// SSIM-Y as a training loss (docs/modes.md section 4p): the score of section 4g on the UNQUANTISED luma, and its gradient with respect
// to the first image.  Nothing is clipped or rounded: Y = ((r*(65.738/256) + g*(129.057/256)) + b*(25.064/256)) + 16 in double from the
// fp32 values.  Window, "valid" region, separable filtering (height pass, then width pass, acc = acc + g[k]*v for k ascending, product
// and sum rounded separately), the five maps and the expression order of the map are ssim.hip's; no fused multiply-add outside the
// IEEE double divisions' own expansion (`fp contract(off)`, exact_u8.h's plain operators), so the float64 host restatement
// (tests/ssim_loss_oracle.py) reproduces every bit of score, coefficients and gradient.
//
// Forward, one workgroup of 256 lanes per 16 x 32 tile of the map: the 26 x 42 halo of both images is loaded (every load issued before
// the first luma is formed), Y goes to LDS as doubles, height pass (a lane owns one column and 4 output rows), width pass (a lane owns
// 2 consecutive outputs of one row: 256 items, one per lane), then the map value S and, when `coef` is given, the three coefficients
//     ca = dS/dmx, cb = dS/dxx, cc = dS/dxy     (raw moments held fixed; the order of operations is ssim_loss_point's)
// as [N][3][Ho][Wo] doubles.  Nothing else goes to HBM.  45.0 KB of LDS (2 x 26 x 42 + 5 x 16 x 43 doubles): three workgroups per CU;
// ssim.hip's 16 x 48 tile with double Y would need 61.9 KB, two per CU.  Reduction without atomics, as in ssim.hip: a lane adds its two
// values in ascending x, wave_sum_d's fixed tree, the four waves in ascending order, one partial per workgroup; ssim_loss_final_kernel
// adds an image's partials (lane t: t, t + 256, ... ascending; the same tree) and divides by Ho*Wo once.
//
// Backward, one workgroup per 16 x 32 tile of INPUT pixels.  The transpose of the valid filter is the full correlation with the same
// window; the window is symmetric (g[k] == g[10-k], the same literals), so it is the valid filter of the map padded with 10 zeros on
// every side, and that is what runs: the three coefficient maps of the tile plus a halo of 10 towards the top and the left are staged in
// LDS (zeros outside the map), then the SAME height and width passes as the forward's (sl_height_pass / sl_width_pass) give
// T[ca], T[cb], T[cc] at the tile's pixels.  x(q), y(q) are recomputed from a and b (loaded once, before the passes), and
//     u = (T[ca] + (2 x) T[cb]) + y T[cc];   dY = (g[n] / ((double)Ho * (double)Wo)) * u;   da_c = (float)(dY * k_c)
// is stored in a's layout.  Every input element is read once, every gradient element written once; 42.7 KB of LDS, no atomics.
#pragma clang fp contract(off)
#include "common.h"
#include "launchers.h"
#include "exact_u8.h"

constexpr int SL_TAPS = 11;
constexpr int SL_HALO = SL_TAPS - 1;
constexpr int SL_THREADS = 256;
constexpr int SL_TH = 16, SL_TW = 32;                              // the tile of both kernels
constexpr int SL_RB = 4, SL_CB = 2;                                // rows per lane in the height pass, columns per lane in the width pass
constexpr int SL_YH = SL_TH + SL_HALO, SL_YW = SL_TW + SL_HALO;    // the staged region
constexpr int SL_SW = SL_YW | 1;                                   // odd row stride of the height-filtered maps
constexpr double SL_C1 = (0.01 * 255) * (0.01 * 255);
constexpr double SL_C2 = (0.03 * 255) * (0.03 * 255);
static_assert(SL_TH % SL_RB == 0 && SL_TH * (SL_TW / SL_CB) == SL_THREADS, "the width pass has one item per lane");

// ssim.hip's ssim_g: g[k] = exp(-(k-5)^2 / 4.5) / sum, the doubles of pesr_amd/ops.py SSIM_WINDOW (tests/test_ssim_loss_cpu.py compares)
__device__ __forceinline__ constexpr double ssim_loss_g(int k) {
    const int d = k < 5 ? 5 - k : k - 5;
    return d == 0 ? 0.26601172486179436
         : d == 1 ? 0.2130055377112537
         : d == 2 ? 0.10936068950970002
         : d == 3 ? 0.03600077212843083
         : d == 4 ? 0.007598758135239185
                  : 0.00102838008447911;
}

// the luma of section 4g without its two clip-and-round steps
__device__ __forceinline__ double ssim_loss_luma(const float (&p)[3]) {
    return (((double)p[0] * (65.738 / 256) + (double)p[1] * (129.057 / 256)) + (double)p[2] * (25.064 / 256)) + 16.0;
}

// Height pass of M maps over the staged SL_YH x SL_YW region: fetch(i, v) gives the M values at staged element i; the filtered maps go
// to st[m][row * SL_SW + column].  A lane owns one column and SL_RB output rows.
template <int M, class Fetch>
__device__ __forceinline__ void sl_height_pass(double* __restrict__ st, int tid, Fetch fetch) {
    for (int item = tid; item < (SL_TH / SL_RB) * SL_YW; item += SL_THREADS) {
        const int r0 = (item / SL_YW) * SL_RB, c = item % SL_YW;
        double acc[M][SL_RB];
#pragma unroll
        for (int r = 0; r < SL_RB; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) acc[m][r] = 0.0;
#pragma unroll
        for (int i = 0; i < SL_RB + SL_HALO; ++i) {
            double v[M];
            fetch((r0 + i) * SL_YW + c, v);
#pragma unroll
            for (int r = 0; r < SL_RB; ++r) {
                const int k = i - r;                               // ascending in i for every output row r
                if (k >= 0 && k < SL_TAPS) {
#pragma unroll
                    for (int m = 0; m < M; ++m) acc[m][r] = exact_mac(acc[m][r], ssim_loss_g(k), v[m]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < SL_RB; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) st[m * (SL_TH * SL_SW) + (r0 + r) * SL_SW + c] = acc[m][r];
    }
}

// Width pass: the SL_CB outputs of row r that start at column c0
template <int M>
__device__ __forceinline__ void sl_width_pass(const double* __restrict__ st, int r, int c0, double (&acc)[M][SL_CB]) {
#pragma unroll
    for (int q = 0; q < SL_CB; ++q)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m][q] = 0.0;
#pragma unroll
    for (int j = 0; j < SL_CB + SL_HALO; ++j) {
        double v[M];
#pragma unroll
        for (int m = 0; m < M; ++m) v[m] = st[m * (SL_TH * SL_SW) + r * SL_SW + c0 + j];
#pragma unroll
        for (int q = 0; q < SL_CB; ++q) {
            const int k = j - q;
            if (k >= 0 && k < SL_TAPS) {
#pragma unroll
                for (int m = 0; m < M; ++m) acc[m][q] = exact_mac(acc[m][q], ssim_loss_g(k), v[m]);
            }
        }
    }
}

// One window: S with ssim.hip's ssim_value order, and the three coefficients (docs/modes.md section 4p)
__device__ __forceinline__ double ssim_loss_point(double mx, double my, double xx, double yy, double xy, double (&co)[3]) {
    const double mxmx = mx * mx, mymy = my * my, mxmy = mx * my;
    const double sx = xx - mxmx, sy = yy - mymy, sxy = xy - mxmy;
    const double a1 = 2.0 * mxmy + SL_C1, a2 = 2.0 * sxy + SL_C2;
    const double b1 = (mxmx + mymy) + SL_C1, b2 = (sx + sy) + SL_C2;
    const double den = b1 * b2;
    const double s = (a1 * a2) / den;
    co[0] = ((2.0 * my) * (a2 - a1)) / den - ((2.0 * mx) * s) * (1.0 / b1 - 1.0 / b2);
    co[1] = -(s / b2);
    co[2] = (2.0 * a1) / den;
    return s;
}

// grid (tiles_x, tiles_y, N) over the Ho x Wo map
__global__ __launch_bounds__(SL_THREADS) void ssim_loss_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                   double* __restrict__ part, double* __restrict__ coef, int H, int W,
                                                                   int Ho, int Wo, long asc, long asp, long bsc, long bsp) {
    __shared__ double ya[SL_YH * SL_YW], yb[SL_YH * SL_YW];
    __shared__ double st[5 * SL_TH * SL_SW];
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int oy0 = blockIdx.y * SL_TH, ox0 = blockIdx.x * SL_TW;
    const long img = (long)n * 3 * H * W;                          // element (c, y, x) of the image lives at img + c*sc + (y*W + x)*sp

    // halo of both images -> luma, once per pixel; zero outside the image (such values only reach outputs that are dropped)
    constexpr int NL = (SL_YH * SL_YW + SL_THREADS - 1) / SL_THREADS;
    float pa[NL][3], pb[NL][3];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int idx = tid + l * SL_THREADS;
        const int iy = oy0 + idx / SL_YW, ix = ox0 + idx % SL_YW;
#pragma unroll
        for (int c = 0; c < 3; ++c) pa[l][c] = pb[l][c] = 0.0f;
        if (idx < SL_YH * SL_YW && iy < H && ix < W) {
            const long p = (long)iy * W + ix;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pa[l][c] = a[img + p * asp + c * asc];
                pb[l][c] = b[img + p * bsp + c * bsc];
            }
        }
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int idx = tid + l * SL_THREADS;
        const int iy = oy0 + idx / SL_YW, ix = ox0 + idx % SL_YW;
        if (idx < SL_YH * SL_YW) {
            const bool in = iy < H && ix < W;
            ya[idx] = in ? ssim_loss_luma(pa[l]) : 0.0;
            yb[idx] = in ? ssim_loss_luma(pb[l]) : 0.0;
        }
    }
    __syncthreads();

    sl_height_pass<5>(st, tid, [&](int i, double (&v)[5]) {
        const double x = ya[i], y = yb[i];
        v[0] = x, v[1] = y, v[2] = x * x, v[3] = y * y, v[4] = x * y;
    });
    __syncthreads();

    const int r = tid / (SL_TW / SL_CB), c0 = (tid % (SL_TW / SL_CB)) * SL_CB;
    double acc[5][SL_CB];
    sl_width_pass<5>(st, r, c0, acc);
    const int oy = oy0 + r;
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < SL_CB; ++q) {
        const int ox = ox0 + c0 + q;
        if (oy < Ho && ox < Wo) {
            double co[3];
            sum += ssim_loss_point(acc[0][q], acc[1][q], acc[2][q], acc[3][q], acc[4][q], co);
            if (coef) {
                const long o = (((long)n * 3) * Ho + oy) * Wo + ox;
#pragma unroll
                for (int m = 0; m < 3; ++m) coef[o + (long)m * Ho * Wo] = co[m];
            }
        }
    }
    __shared__ double red[SL_THREADS / 64];
    const double w = wave_sum_d(sum);
    if ((tid & 63) == 0) red[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) part[((long)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup per image: lane t adds partials t, t + 256, ... in ascending order, then the fixed tree of wave_sum_d
__global__ __launch_bounds__(SL_THREADS) void ssim_loss_final_kernel(const double* __restrict__ part, double* __restrict__ out,
                                                                     long tiles, double count) {
    const double* p = part + blockIdx.x * tiles;
    double s = 0.0;
    for (long k = threadIdx.x; k < tiles; k += SL_THREADS) s += p[k];
    __shared__ double red[SL_THREADS / 64];
    const double w = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (((red[0] + red[1]) + red[2]) + red[3]) / count;
}

// grid (tiles_x, tiles_y, N) over the H x W image; ga has a's layout
__global__ __launch_bounds__(SL_THREADS) void ssim_loss_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                   const double* __restrict__ coef, const double* __restrict__ g,
                                                                   float* __restrict__ ga, int H, int W, int Ho, int Wo, long asc,
                                                                   long asp, long bsc, long bsp) {
    __shared__ double cf[3 * SL_YH * SL_YW];
    __shared__ double st[3 * SL_TH * SL_SW];
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int qy0 = blockIdx.y * SL_TH, qx0 = blockIdx.x * SL_TW;
    const long img = (long)n * 3 * H * W;

    // this lane's SL_CB pixels of both images: loaded now, used after the two passes
    const int r = tid / (SL_TW / SL_CB), c0 = (tid % (SL_TW / SL_CB)) * SL_CB;
    const int qy = qy0 + r;
    float pa[SL_CB][3], pb[SL_CB][3];
#pragma unroll
    for (int q = 0; q < SL_CB; ++q) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pa[q][c] = pb[q][c] = 0.0f;
        if (qy < H && qx0 + c0 + q < W) {
            const long p = (long)qy * W + (qx0 + c0 + q);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pa[q][c] = a[img + p * asp + c * asc];
                pb[q][c] = b[img + p * bsp + c * bsc];
            }
        }
    }

    // the three coefficient maps at rows qy0-10 .. qy0+15 and columns qx0-10 .. qx0+31 of the map, zero outside it
    const long cimg = (long)n * 3 * Ho * Wo;
#pragma unroll 4
    for (int idx = tid; idx < 3 * SL_YH * SL_YW; idx += SL_THREADS) {
        const int m = idx / (SL_YH * SL_YW), rem = idx % (SL_YH * SL_YW);
        const int oy = qy0 - SL_HALO + rem / SL_YW, ox = qx0 - SL_HALO + rem % SL_YW;
        const bool in = oy >= 0 && oy < Ho && ox >= 0 && ox < Wo;
        cf[idx] = in ? coef[cimg + ((long)m * Ho + oy) * Wo + ox] : 0.0;
    }
    __syncthreads();

    sl_height_pass<3>(st, tid, [&](int i, double (&v)[3]) {
#pragma unroll
        for (int m = 0; m < 3; ++m) v[m] = cf[m * (SL_YH * SL_YW) + i];
    });
    __syncthreads();

    double t[3][SL_CB];
    sl_width_pass<3>(st, r, c0, t);
    const double scale = g[n] / ((double)Ho * (double)Wo);
#pragma unroll
    for (int q = 0; q < SL_CB; ++q) {
        if (qy < H && qx0 + c0 + q < W) {
            const double x = ssim_loss_luma(pa[q]), y = ssim_loss_luma(pb[q]);
            const double u = (t[0][q] + (2.0 * x) * t[1][q]) + y * t[2][q];
            const double dy = scale * u;
            const long p = (long)qy * W + (qx0 + c0 + q);
            ga[img + p * asp + 0 * asc] = (float)(dy * (65.738 / 256));
            ga[img + p * asp + 1 * asc] = (float)(dy * (129.057 / 256));
            ga[img + p * asp + 2 * asc] = (float)(dy * (25.064 / 256));
        }
    }
}

// the checks both entry points share; Ho x Wo is the size of the map
static int ssim_loss_shape(const float* a, const float* b, int N, int H, int W, int* Ho, int* Wo) {
    if (!a || !b || N < 1 || N > 65535 || H < SL_TAPS || W < SL_TAPS) return PESR_EINVAL;      // no silent smaller window
    *Ho = H - SL_HALO, *Wo = W - SL_HALO;
    return PESR_OK;
}

int pesr_ssim_loss_fwd_launch(const float* a, const float* b, double* score, int N, int H, int W, int a_nhwc, int b_nhwc, double* coef,
                              void* ws, size_t ws_bytes, hipStream_t stream) {
    int Ho, Wo;
    if (ssim_loss_shape(a, b, N, H, W, &Ho, &Wo) != PESR_OK || !score) return PESR_EINVAL;
    if (((uintptr_t)score | (uintptr_t)coef | (uintptr_t)ws) & 7) return PESR_EINVAL;
    const int tx = (Wo + SL_TW - 1) / SL_TW, ty = (Ho + SL_TH - 1) / SL_TH;
    if (ty > 65535) return PESR_EINVAL;
    const long tiles = (long)tx * ty;
    if (!ws || ws_bytes < (size_t)N * tiles * sizeof(double)) return PESR_EWORKSPACE;
    const long P = (long)H * W;
    hipLaunchKernelGGL(ssim_loss_fwd_kernel, dim3(tx, ty, N), dim3(SL_THREADS), 0, stream, a, b, (double*)ws, coef, H, W, Ho, Wo,
                       a_nhwc ? 1L : P, a_nhwc ? 3L : 1L, b_nhwc ? 1L : P, b_nhwc ? 3L : 1L);
    hipLaunchKernelGGL(ssim_loss_final_kernel, dim3(N), dim3(SL_THREADS), 0, stream, (const double*)ws, score, tiles,
                       (double)Ho * (double)Wo);
    return pesr_launch_status();
}

int pesr_ssim_loss_bwd_launch(const float* a, const float* b, const double* coef, const double* g, float* ga, int N, int H, int W,
                              int a_nhwc, int b_nhwc, hipStream_t stream) {
    int Ho, Wo;
    if (ssim_loss_shape(a, b, N, H, W, &Ho, &Wo) != PESR_OK || !coef || !g || !ga) return PESR_EINVAL;
    if ((((uintptr_t)coef | (uintptr_t)g) & 7) || ((uintptr_t)ga & 3)) return PESR_EINVAL;
    const int tx = (W + SL_TW - 1) / SL_TW, ty = (H + SL_TH - 1) / SL_TH;
    if (ty > 65535) return PESR_EINVAL;
    const long P = (long)H * W;
    hipLaunchKernelGGL(ssim_loss_bwd_kernel, dim3(tx, ty, N), dim3(SL_THREADS), 0, stream, a, b, coef, g, ga, H, W, Ho, Wo,
                       a_nhwc ? 1L : P, a_nhwc ? 3L : 1L, b_nhwc ? 1L : P, b_nhwc ? 3L : 1L);
    return pesr_launch_status();
}
