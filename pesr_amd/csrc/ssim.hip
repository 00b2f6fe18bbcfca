// SSIM on the Y channel with a border shave (docs/modes.md section 4g): the SSIM of Wang et al.'s ssim_index.m as the
// super-resolution literature reports it, beside psnr_y_kernel.  Both images are clipped to 0..255, rounded, converted to the BT.601
// luma in double, clipped and rounded again (the Y image of the PSNR-Y); rows and columns [shave, H-shave) x [shave, W-shave) are used.
// Five maps (x, y, x*x, y*y, x*y) are filtered with the 11 x 11 Gaussian window of sigma 1.5, separably - height pass, then width
// pass, "valid" region - each pass  acc = 0; for k ascending: acc = acc + g[k] * v  in float64 with the product and the sum rounded
// separately.  No fused multiply-add anywhere in the filter and the map arithmetic: the float64 host restatement
// (tests/ssim_oracle.py) reproduces every bit of the map.  Hence `fp contract(off)` and exact_u8.h's plain * and + (the
// __dmul_rn / __dadd_rn of the HIP headers are fused once inlined).  The only v_fma_f64 / v_div_fmas_f64 left in this file's code are
// those of the IEEE double division's own expansion (v_div_scale, v_rcp, the Newton steps, v_div_fmas, v_div_fixup), which is
// correctly rounded.
//
// One workgroup of 256 lanes per TH x TW output tile of one image (16 x 48).  Every load of the (TH+10) x (TW+10) halo of both images
// is issued before the first luma is formed (one round trip to memory per tile); every pixel is converted to luma once and Y stays
// in LDS as floats (an integer in 0..255: exact, and half the LDS of doubles).  Height pass: a lane owns one column and RB output
// rows, walks RB+10 rows of Y down the column (lanes read consecutive words: conflict-free) and forms the three products once per
// input pixel; the five height-filtered maps go to LDS as doubles with an odd row stride.  Width pass: a lane owns CB consecutive
// outputs of one row and reads CB+10 values per map.  Nothing intermediate goes to HBM.  16 x 48 with RB = 4, CB = 3 keeps 232 and
// 256 of the 256 lanes busy in the two passes, at 49 KB of LDS and 150 VGPRs (3 workgroups per CU); the tiles it was measured
// against are in docs/modes.md section 4g.  Reduction without atomics: one partial sum per workgroup, summed in a fixed order, then
// ssim_final_kernel adds an image's partials in a fixed order too: the result is the same bits on every run.
#pragma clang fp contract(off)
#include "common.h"
#include "launchers.h"
#include "exact_u8.h"

// Tile and per-lane blocks.  Overridable for experiment builds only (scripts/build_variant.sh, PESR_HIP_LIB).
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

// psnr_y_kernel's luma of one RGB pixel, here without contraction.
__device__ __forceinline__ double ssim_luma(const float (&p)[3]) {
    const double r = rint(fmin(fmax((double)p[0], 0.0), 255.0));
    const double g = rint(fmin(fmax((double)p[1], 0.0), 255.0));
    const double b = rint(fmin(fmax((double)p[2], 0.0), 255.0));
    const double y = ((r * (65.738 / 256) + g * (129.057 / 256)) + b * (25.064 / 256)) + 16.0;
    return rint(fmin(fmax(y, 0.0), 255.0));
}

__device__ __forceinline__ double ssim_value(double mx, double my, double xx, double yy, double xy) {
    const double mxmx = mx * mx, mymy = my * my, mxmy = mx * my;
    const double sx = xx - mxmx, sy = yy - mymy, sxy = xy - mxmy;
    const double num = (2.0 * mxmy + SSIM_C1) * (2.0 * sxy + SSIM_C2);
    const double den = ((mxmx + mymy) + SSIM_C1) * ((sx + sy) + SSIM_C2);
    return num / den;
}

// grid (tiles_x, tiles_y, N).  Ho x Wo is the size of the map, (Ho+10) x (Wo+10) the shaved image.
template <int TH, int TW, int RB, int CB>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_y_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              double* __restrict__ part, double* __restrict__ map, int H, int W,
                                                              int shave, int Ho, int Wo, long asc, long asp, long bsc, long bsp) {
    static_assert(TH % RB == 0 && TW % CB == 0, "row / column blocks must divide the tile");
    constexpr int YH = TH + SSIM_HALO, YW = TW + SSIM_HALO;
    constexpr int SW = YW | 1;                                     // odd row stride of the height-filtered maps
    __shared__ float ya[YH * YW], yb[YH * YW];                     // Y is an integer in 0..255: exact as a float, half the LDS
    __shared__ double st[5][TH * SW];
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;
    const int Hs = Ho + SSIM_HALO, Ws = Wo + SSIM_HALO;
    const long img = (long)n * 3 * H * W;                          // element (c, y, x) of the image lives at img + c*sc + (y*W + x)*sp

    // halo of both images -> luma, once per pixel; zero outside the shaved image (such values only reach outputs that are dropped).
    // All of a lane's loads are issued before the first luma is formed: one round trip to memory per tile, not one per pixel.
    constexpr int NL = (YH * YW + SSIM_THREADS - 1) / SSIM_THREADS;
    float pa[NL][3], pb[NL][3];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int idx = tid + l * SSIM_THREADS;
        const int iy = oy0 + idx / YW, ix = ox0 + idx % YW;
#pragma unroll
        for (int c = 0; c < 3; ++c) pa[l][c] = pb[l][c] = 0.0f;
        if (idx < YH * YW && iy < Hs && ix < Ws) {
            const long p = (long)(iy + shave) * W + (ix + shave);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pa[l][c] = a[img + p * asp + c * asc];
                pb[l][c] = b[img + p * bsp + c * bsc];
            }
        }
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int idx = tid + l * SSIM_THREADS;
        const int iy = oy0 + idx / YW, ix = ox0 + idx % YW;
        if (idx < YH * YW) {
            const bool in = iy < Hs && ix < Ws;
            ya[idx] = in ? (float)ssim_luma(pa[l]) : 0.0f;
            yb[idx] = in ? (float)ssim_luma(pb[l]) : 0.0f;
        }
    }
    __syncthreads();

    // height pass: RB output rows of one column per lane
    for (int item = tid; item < (TH / RB) * YW; item += SSIM_THREADS) {
        const int r0 = (item / YW) * RB, c = item % YW;
        double acc[5][RB];
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[m][r] = 0.0;
#pragma unroll
        for (int i = 0; i < RB + SSIM_HALO; ++i) {
            const double x = (double)ya[(r0 + i) * YW + c], y = (double)yb[(r0 + i) * YW + c];
            const double xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int k = i - r;                               // ascending in i for every output row r
                if (k >= 0 && k < SSIM_TAPS) {
                    acc[0][r] = exact_mac(acc[0][r], ssim_g(k), x);
                    acc[1][r] = exact_mac(acc[1][r], ssim_g(k), y);
                    acc[2][r] = exact_mac(acc[2][r], ssim_g(k), xx);
                    acc[3][r] = exact_mac(acc[3][r], ssim_g(k), yy);
                    acc[4][r] = exact_mac(acc[4][r], ssim_g(k), xy);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int m = 0; m < 5; ++m) st[m][(r0 + r) * SW + c] = acc[m][r];
    }
    __syncthreads();

    // width pass and the map: CB consecutive outputs of one row per lane
    double sum = 0.0;
    for (int item = tid; item < TH * (TW / CB); item += SSIM_THREADS) {
        const int r = item / (TW / CB), c0 = (item % (TW / CB)) * CB;
        double acc[5][CB];
#pragma unroll
        for (int q = 0; q < CB; ++q)
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[m][q] = 0.0;
#pragma unroll
        for (int j = 0; j < CB + SSIM_HALO; ++j) {
            double v[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) v[m] = st[m][r * SW + c0 + j];
#pragma unroll
            for (int q = 0; q < CB; ++q) {
                const int k = j - q;
                if (k >= 0 && k < SSIM_TAPS) {
#pragma unroll
                    for (int m = 0; m < 5; ++m) acc[m][q] = exact_mac(acc[m][q], ssim_g(k), v[m]);
                }
            }
        }
        const int oy = oy0 + r;
#pragma unroll
        for (int q = 0; q < CB; ++q) {
            const int ox = ox0 + c0 + q;
            if (oy < Ho && ox < Wo) {
                const double s = ssim_value(acc[0][q], acc[1][q], acc[2][q], acc[3][q], acc[4][q]);
                sum += s;
                if (map) map[((long)n * Ho + oy) * Wo + ox] = s;
            }
        }
    }
    __shared__ double red[SSIM_THREADS / 64];
    const double w = wave_sum_d(sum);
    if ((tid & 63) == 0) red[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) part[((long)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup per image: lane t adds partials t, t + 256, ... in ascending order, then the fixed tree of wave_sum_d
__global__ __launch_bounds__(SSIM_THREADS) void ssim_final_kernel(const double* __restrict__ part, double* __restrict__ out, long tiles,
                                                                  double count) {
    const double* p = part + blockIdx.x * tiles;
    double s = 0.0;
    for (long k = threadIdx.x; k < tiles; k += SSIM_THREADS) s += p[k];
    __shared__ double red[SSIM_THREADS / 64];
    const double w = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (((red[0] + red[1]) + red[2]) + red[3]) / count;
}

int pesr_ssim_y_launch(const float* a, const float* b, double* out, int N, int H, int W, int a_nhwc, int b_nhwc, int shave,
                       double* map, void* ws, size_t ws_bytes, hipStream_t stream) {
    constexpr int TH = PESR_SSIM_TH, TW = PESR_SSIM_TW;
    if (!a || !b || !out || N < 1 || H < 1 || W < 1 || shave < 0) return PESR_EINVAL;
    const long Hs = (long)H - 2L * shave, Ws = (long)W - 2L * shave;
    if (Hs < SSIM_TAPS || Ws < SSIM_TAPS) return PESR_EINVAL;       // no silent smaller window
    const int Ho = (int)Hs - SSIM_HALO, Wo = (int)Ws - SSIM_HALO;
    const int tx = (Wo + TW - 1) / TW, ty = (Ho + TH - 1) / TH;
    if (ty > 65535 || N > 65535) return PESR_EINVAL;
    const long tiles = (long)tx * ty;
    if (!ws || ws_bytes < (size_t)N * tiles * sizeof(double)) return PESR_EWORKSPACE;
    const long P = (long)H * W;
    hipLaunchKernelGGL((ssim_y_kernel<TH, TW, PESR_SSIM_RB, PESR_SSIM_CB>), dim3(tx, ty, N), dim3(SSIM_THREADS), 0, stream, a, b,
                       (double*)ws, map, H, W, shave, Ho, Wo, a_nhwc ? 1L : P, a_nhwc ? 3L : 1L, b_nhwc ? 1L : P, b_nhwc ? 3L : 1L);
    hipLaunchKernelGGL(ssim_final_kernel, dim3(N), dim3(SSIM_THREADS), 0, stream, (const double*)ws, out, tiles,
                       (double)Ho * (double)Wo);
    return pesr_launch_status();
}
