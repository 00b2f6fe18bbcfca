// NIQE block statistics (docs/modes.md section 4k): the device half of the no-reference score of Mittal et al. as this project
// restates it in float64 (tests/niqe_oracle.py).  Per image: luma (MATLAB's rgb2gray, or the Y of the PSNR-Y) of the clipped and
// rounded RGB, a border shave and a top-left crop to multiples of the block side B; scale 2 is the x0.5 antialiased bicubic resize of
// that luma (section 4f's x2-down taps and reflect rule, height pass then width pass, no rounding and no clamp); per scale the MSCN
// map  (I - mu) / (sigma + 1)  with mu = filt(I), sigma = sqrt(|filt(I*I) - mu*mu|) and filt the 7-tap Gaussian window of sigma 7/6
// applied separably (height, then width) with replicated edges; per B x B (scale 2: B/2 x B/2) block 26 doubles: for the map and its
// four products with a copy of itself shifted circularly INSIDE the block {sum x*x over x < 0, count x < 0, sum x*x over x > 0,
// count x > 0, sum |x|}, then the sum of sigma.  The AGGD fits, the features and the score are host work (pesr_amd/niqe.py).
//
// float64 throughout, every filter pass  acc = 0; for k ascending: acc = acc + g[k] * v  with the product and the sum rounded
// separately: `fp contract(off)` and plain * + - as in exact_u8.h, so that the restatement reproduces every bit of both
// MSCN maps (the division and the square root are the IEEE ones).  Four kernels, none fused (nobody has measured a fusion yet):
//   niqe_luma_kernel   one lane per cropped pixel, RGB floats -> the luma as a double image;
//   niqe_down2_kernel  one lane per scale-2 pixel: the 8 x 8 window straight from the luma image (it sits in L2), the height pass
//                      of each of the 8 columns, then the width pass over them - the same operations in the same order as two
//                      whole-image passes, without their intermediate image;
//   niqe_mscn_kernel   one workgroup per 16 x 64 tile of a double image, for both scales: the 22 x 70 halo goes to LDS with clamped
//                      indices, the height pass leaves filt_h(I) and filt_h(I*I) in LDS (rows of 70 doubles: lanes read consecutive
//                      words), the width pass forms mu, sigma and the map;
//   niqe_stats_kernel  one workgroup per (image, scale, block): the block of the map in LDS (96 x 96 doubles = 72 KB, dynamic), the
//                      four wrapped products from there, every lane sums its elements in ascending order, then the fixed tree of
//                      wave_sum_d and ((w0 + w1) + w2) + w3.  No atomics: two calls return the same bits.
// 64-bit offsets everywhere.
#pragma clang fp contract(off)
#include "common.h"
#include "launchers.h"
#include "exact_u8.h"

constexpr int NIQE_TAPS = 7;
constexpr int NIQE_HALO = NIQE_TAPS - 1;
constexpr int NIQE_THREADS = 256;
constexpr int NIQE_TH = 16, NIQE_TW = 64;
constexpr int NIQE_NSTAT = 26;

// g[k] = exp(-(k-3)^2 / (2 (7/6)^2)) / sum (ascending k), the doubles that pesr_amd/niqe.py NIQE_WINDOW and tests/niqe_oracle.py hold
__device__ __forceinline__ constexpr double niqe_g(int k) {
    const int d = k < 3 ? 3 - k : k - 3;
    return d == 0 ? 0.34263151546524945 : d == 1 ? 0.2372960771171706 : d == 2 ? 0.07882796468173002 : 0.012560200468474614;
}

// section 4f's x2-down weights, exact in binary
__device__ __forceinline__ constexpr double niqe_w2(int t) {
    const int d = t < 4 ? 3 - t : t - 4;
    return d == 0 ? 111.0 / 256 : d == 1 ? 29.0 / 256 : d == 2 ? -9.0 / 256 : -3.0 / 256;
}

// mode 0: floor(((r*0.2989.. + g*0.5870..) + b*0.1140..) + 0.5), MATLAB's rgb2gray; mode 1: exact_u8.h's Y.  Integers in 0..255.
__device__ __forceinline__ double niqe_luma(float pr, float pg, float pb, int mode) {
    if (mode == 0) {
        const double r = exact_clip8(pr), g = exact_clip8(pg), b = exact_clip8(pb);
        return floor(((r * 0.298936021293775 + g * 0.587043074451121) + b * 0.114020904255103) + 0.5);
    }
    return exact_luma601_u8(pr, pg, pb);
}

// grid (ceil(Hc*Wc / 256), 1, N).  Element (c, y, x) of image n lives at n*3*H*W + c*sc + (y*W + x)*sp.
__global__ __launch_bounds__(NIQE_THREADS) void niqe_luma_kernel(const float* __restrict__ img, double* __restrict__ lum, int H, int W,
                                                                 int shave, int Hc, int Wc, long sc, long sp, int mode) {
    const long P = (long)Hc * Wc;
    const long i = (long)blockIdx.x * NIQE_THREADS + threadIdx.x;
    if (i >= P) return;
    const long n = blockIdx.z;
    const int y = (int)(i / Wc), x = (int)(i % Wc);
    const float* base = img + n * 3 * H * W + ((long)(y + shave) * W + (x + shave)) * sp;
    lum[n * P + i] = niqe_luma(base[0], base[sc], base[2 * sc], mode);
}

// grid (ceil(Ho*Wo / 256), 1, N), Ho = Hc/2, Wo = Wc/2
__global__ __launch_bounds__(NIQE_THREADS) void niqe_down2_kernel(const double* __restrict__ lum, double* __restrict__ out, int Hc,
                                                                  int Wc) {
    const int Ho = Hc / 2, Wo = Wc / 2;
    const long P = (long)Ho * Wo;
    const long i = (long)blockIdx.x * NIQE_THREADS + threadIdx.x;
    if (i >= P) return;
    const long n = blockIdx.z;
    const int oy = (int)(i / Wo), ox = (int)(i % Wo);
    const double* src = lum + n * Hc * (long)Wc;
    long row[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = (long)exact_reflect(2 * oy - 3 + k, Hc) * Wc;
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int c = exact_reflect(2 * ox - 3 + t, Wc);
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = src[row[k] + c];
        double h = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) h = exact_mac(h, niqe_w2(k), v[k]);
        acc = exact_mac(acc, niqe_w2(t), h);
    }
    out[n * P + i] = acc;
}

// grid (tiles_x, tiles_y, N) over a double image [N][Hs][Ws]
__global__ __launch_bounds__(NIQE_THREADS) void niqe_mscn_kernel(const double* __restrict__ src, double* __restrict__ mscn,
                                                                 double* __restrict__ sigma, int Hs, int Ws) {
    constexpr int TH = NIQE_TH, TW = NIQE_TW, YH = TH + NIQE_HALO, YW = TW + NIQE_HALO;
    __shared__ double in[YH * YW];
    __shared__ double hm[TH * YW], hq[TH * YW];
    const int tid = threadIdx.x;
    const long base = (long)blockIdx.z * Hs * Ws;
    const int oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;
    for (int idx = tid; idx < YH * YW; idx += NIQE_THREADS) {
        const int iy = min(max(oy0 - 3 + idx / YW, 0), Hs - 1), ix = min(max(ox0 - 3 + idx % YW, 0), Ws - 1);   // replicate
        in[idx] = src[base + (long)iy * Ws + ix];
    }
    __syncthreads();
    for (int item = tid; item < TH * YW; item += NIQE_THREADS) {
        const int r = item / YW, c = item % YW;
        double am = 0.0, aq = 0.0;
#pragma unroll
        for (int k = 0; k < NIQE_TAPS; ++k) {
            const double v = in[(r + k) * YW + c];
            const double vv = v * v;
            am = exact_mac(am, niqe_g(k), v);
            aq = exact_mac(aq, niqe_g(k), vv);
        }
        hm[item] = am;
        hq[item] = aq;
    }
    __syncthreads();
    for (int item = tid; item < TH * TW; item += NIQE_THREADS) {
        const int r = item / TW, c = item % TW;
        double mu = 0.0, q = 0.0;
#pragma unroll
        for (int k = 0; k < NIQE_TAPS; ++k) {
            mu = exact_mac(mu, niqe_g(k), hm[r * YW + c + k]);
            q = exact_mac(q, niqe_g(k), hq[r * YW + c + k]);
        }
        const int oy = oy0 + r, ox = ox0 + c;
        if (oy < Hs && ox < Ws) {
            const double mumu = mu * mu;
            const double sg = sqrt(fabs(q - mumu));
            const double v = in[(r + 3) * YW + c + 3];
            const long o = base + (long)oy * Ws + ox;
            mscn[o] = (v - mu) / (sg + 1.0);
            sigma[o] = sg;
        }
    }
}

// grid (nby*nbx, 2, N); dynamic LDS: B*B + 4*26 doubles (scale 2 uses a quarter of the block area)
__global__ __launch_bounds__(NIQE_THREADS) void niqe_stats_kernel(const double* __restrict__ m1, const double* __restrict__ m2,
                                                                  const double* __restrict__ s1, const double* __restrict__ s2,
                                                                  double* __restrict__ stats, int Hc, int Wc, int B, int nbx) {
    extern __shared__ __attribute__((aligned(16))) char niqe_smem[];
    double* m = (double*)niqe_smem;                                // B*B doubles (a multiple of 16 bytes: B is even), then
    double (*red)[NIQE_NSTAT] = (double (*)[NIQE_NSTAT])(m + B * B);   // one row of partial sums per wave
    const int tid = threadIdx.x;
    const int s = blockIdx.y;
    const int Bs = B >> s, Hs = Hc >> s, Ws = Wc >> s;
    const double* __restrict__ map = s ? m2 : m1;
    const double* __restrict__ sig = s ? s2 : s1;
    const int by = blockIdx.x / nbx, bx = blockIdx.x % nbx;
    const long org = (long)blockIdx.z * Hs * Ws + (long)by * Bs * Ws + (long)bx * Bs;
    double acc[NIQE_NSTAT];
#pragma unroll
    for (int j = 0; j < NIQE_NSTAT; ++j) acc[j] = 0.0;
    for (int e = tid; e < Bs * Bs; e += NIQE_THREADS) {
        const long o = org + (long)(e / Bs) * Ws + e % Bs;
        m[e] = map[o];
        acc[25] += sig[o];
    }
    __syncthreads();
    for (int e = tid; e < Bs * Bs; e += NIQE_THREADS) {
        const int y = e / Bs, x = e % Bs;
        const int ym = y ? y - 1 : Bs - 1, xm = x ? x - 1 : Bs - 1, xp = x + 1 < Bs ? x + 1 : 0;
        const double v = m[e];
        // circshift(m, d)[y][x] = m[y - d0][x - d1], wrapped: d = (0,1), (1,0), (1,1), (1,-1)
        const double val[5] = {v, v * m[y * Bs + xm], v * m[ym * Bs + x], v * m[ym * Bs + xm], v * m[ym * Bs + xp]};
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const double t = val[q];
            const double tt = t * t;
            if (t < 0.0) {
                acc[5 * q] += tt;
                acc[5 * q + 1] += 1.0;
            } else if (t > 0.0) {
                acc[5 * q + 2] += tt;
                acc[5 * q + 3] += 1.0;
            }
            acc[5 * q + 4] += fabs(t);
        }
    }
#pragma unroll
    for (int j = 0; j < NIQE_NSTAT; ++j) {
        const double w = wave_sum_d(acc[j]);
        if ((tid & 63) == 0) red[tid >> 6][j] = w;
    }
    __syncthreads();
    if (tid < NIQE_NSTAT) {
        const long o = (((long)blockIdx.z * 2 + s) * gridDim.x + blockIdx.x) * NIQE_NSTAT + tid;
        stats[o] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

int pesr_niqe_stats_launch(const float* img, int N, int H, int W, int nhwc, int shave, int B, int luma, double* stats, double* mscn1,
                           double* mscn2, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!img || !stats || N < 1 || N > 65535 || H < 1 || W < 1 || shave < 0) return PESR_EINVAL;
    if (B < 8 || B > 96 || (B & 1) || (luma != 0 && luma != 1)) return PESR_EINVAL;
    const long Hs = (long)H - 2L * shave, Ws = (long)W - 2L * shave;
    if (Hs < B || Ws < B) return PESR_EINVAL;
    const long nby = Hs / B, nbx = Ws / B;
    if (nby * nbx < 2 || nby * nbx > 0x7fffffffL) return PESR_EINVAL;          // a covariance needs two rows
    const int Hc = (int)(nby * B), Wc = (int)(nbx * B);
    const int ty = (Hc + NIQE_TH - 1) / NIQE_TH;
    if (ty > 65535) return PESR_EINVAL;
    const long P1 = (long)Hc * Wc, P2 = P1 / 4;
    if (!ws || ws_bytes < (size_t)N * 3 * (P1 + P2) * sizeof(double)) return PESR_EWORKSPACE;
    double* lum1 = (double*)ws;
    double* lum2 = lum1 + N * P1;
    double* sig1 = lum2 + N * P2;
    double* sig2 = sig1 + N * P1;
    double* map1 = mscn1 ? mscn1 : sig2 + N * P2;
    double* map2 = mscn2 ? mscn2 : sig2 + N * P2 + N * P1;
    const long P = (long)H * W;
    hipLaunchKernelGGL(niqe_luma_kernel, dim3((unsigned)((P1 + NIQE_THREADS - 1) / NIQE_THREADS), 1, N), dim3(NIQE_THREADS), 0, stream,
                       img, lum1, H, W, shave, Hc, Wc, nhwc ? 1L : P, nhwc ? 3L : 1L, luma);
    hipLaunchKernelGGL(niqe_down2_kernel, dim3((unsigned)((P2 + NIQE_THREADS - 1) / NIQE_THREADS), 1, N), dim3(NIQE_THREADS), 0, stream,
                       (const double*)lum1, lum2, Hc, Wc);
    hipLaunchKernelGGL(niqe_mscn_kernel, dim3((Wc + NIQE_TW - 1) / NIQE_TW, ty, N), dim3(NIQE_THREADS), 0, stream,
                       (const double*)lum1, map1, sig1, Hc, Wc);
    hipLaunchKernelGGL(niqe_mscn_kernel, dim3((Wc / 2 + NIQE_TW - 1) / NIQE_TW, (Hc / 2 + NIQE_TH - 1) / NIQE_TH, N), dim3(NIQE_THREADS),
                       0, stream, (const double*)lum2, map2, sig2, Hc / 2, Wc / 2);
    static PesrDeviceOnce attr_once;
    attr_once([&] { (void)hipFuncSetAttribute((const void*)niqe_stats_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (96 * 96 + (NIQE_THREADS / 64) * NIQE_NSTAT) * 8); });
    hipLaunchKernelGGL(niqe_stats_kernel, dim3((unsigned)(nby * nbx), 2, N), dim3(NIQE_THREADS),
                       ((size_t)B * B + (NIQE_THREADS / 64) * NIQE_NSTAT) * sizeof(double), stream,
                       (const double*)map1, (const double*)map2, (const double*)sig1, (const double*)sig2, stats, Hc, Wc, B, (int)nbx);
    return pesr_launch_status();
}
