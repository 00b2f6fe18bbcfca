// Classical degradation of uint8 HWC images, LR = (HR (*) k) subsampled by s, plus noise, as pinned in docs/modes.md section 4j:
// a K x K float64 blur kernel (1 <= K <= 24, K of the parity of s) centred on the s x s block of every LR pixel, replicate clamp at
// the IMAGE border, Gaussian-like noise made from integers, clamp to [0, 255], round half up.  One launch serves n entries through
// a descriptor array; an entry is a window (y0, x0, h, w) of the LR grid of one image of the pool, so a training crop reads the real
// image around it and only the image border is special.
//   acc = 0; for i ascending, for j ascending: acc = acc + k[i][j] * hr[clamp(s*oy + (s-K)/2 + i)][clamp(s*ox + (s-K)/2 + j)]
//   if sigma_n != 0: acc = acc + sigma_n * g(q, e),  e = (y*w + x)*3 + c in the window
// float64 with the product and the sum rounded separately (no fused multiply-add: the host restatement reproduces every bit).
// One workgroup of 256 lanes per 16 x 16 LR tile of one entry: the clamped HR window of the tile (side 16s + K - s at most, one
// dword per pixel) and the entry's K*K weights are staged in LDS, each lane carries the three channel sums of one LR pixel and
// walks the taps in the fixed order with one LDS read per tap.
#pragma clang fp contract(off)
#include "common.h"
#include "launchers.h"
#include "exact_u8.h"

constexpr int DEGRADE_THREADS = 256;
constexpr int DEGRADE_TILE = 16;                           // LR pixels per workgroup and axis
constexpr int DEGRADE_MAX_K = 24;
constexpr int DEGRADE_DESC = 11;                           // int64 words per entry (include/pesr_hip.h)

template <int S>
__global__ __launch_bounds__(DEGRADE_THREADS) void degrade_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                  const long long* __restrict__ desc, int n, int K,
                                                                  const double* __restrict__ bank) {
    constexpr int MAX_SIDE = DEGRADE_TILE * S + DEGRADE_MAX_K - S;
    __shared__ unsigned spx[MAX_SIDE * MAX_SIDE];          // r | g << 8 | b << 16 of the clamped HR window
    __shared__ double sw[DEGRADE_MAX_K * DEGRADE_MAX_K];
    const int tap0 = (S - K) / 2;                          // S - K is even
    for (int ent = blockIdx.y; ent < n; ent += gridDim.y) {
        const long long* d = desc + (long long)ent * DEGRADE_DESC;
        const long long so = d[0], dof = d[1];
        const int H = (int)d[2], W = (int)d[3], y0 = (int)d[4], x0 = (int)d[5], h = (int)d[6], w = (int)d[7];
        const double* kern = bank + d[8] * (long long)(K * K);
        const double sigma = __longlong_as_double(d[9]);
        const unsigned long long key = exact_splitmix64((unsigned long long)d[10]);
        const long long xtiles = (w + DEGRADE_TILE - 1) / DEGRADE_TILE;
        const long long tiles = ((h + DEGRADE_TILE - 1) / DEGRADE_TILE) * xtiles;
        for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int ty = (int)(t / xtiles) * DEGRADE_TILE, tx = (int)(t % xtiles) * DEGRADE_TILE;      // tile origin in the window
            const int th = min(DEGRADE_TILE, h - ty), tw = min(DEGRADE_TILE, w - tx);
            const int sy = th * S + K - S, sx = tw * S + K - S;                                  // staged HR rows / columns
            const int row0 = S * (y0 + ty) + tap0, col0 = S * (x0 + tx) + tap0;
            __syncthreads();                                // the previous tile's readers are done
            for (int p = threadIdx.x; p < K * K; p += DEGRADE_THREADS) sw[p] = kern[p];
            for (int p = threadIdx.x; p < sy * sx; p += DEGRADE_THREADS) {
                const int r = exact_replicate(row0 + p / sx, H), c = exact_replicate(col0 + p % sx, W);
                const unsigned char* px = src + so + ((long long)r * W + c) * 3;
                spx[p] = exact_load_px(px);
            }
            __syncthreads();
            const int ly = threadIdx.x / DEGRADE_TILE, lx = threadIdx.x % DEGRADE_TILE;
            if (ly < th && lx < tw) {
                double a0 = 0.0, a1 = 0.0, a2 = 0.0;
                const unsigned* base = spx + (ly * S) * sx + lx * S;
                for (int i = 0; i < K; ++i) {
                    for (int j = 0; j < K; ++j) {
                        const double wt = sw[i * K + j];
                        const unsigned v = base[i * sx + j];
                        a0 = exact_mac_u(a0, wt, v & 0xff);
                        a1 = exact_mac_u(a1, wt, (v >> 8) & 0xff);
                        a2 = exact_mac_u(a2, wt, v >> 16);
                    }
                }
                const long long pix = (long long)(ty + ly) * w + (tx + lx);
                if (sigma != 0.0) {
                    const unsigned long long e = 3ULL * (unsigned long long)pix;
                    a0 = exact_noise(a0, sigma, exact_gauss(key, e));
                    a1 = exact_noise(a1, sigma, exact_gauss(key, e + 1));
                    a2 = exact_noise(a2, sigma, exact_gauss(key, e + 2));
                }
                unsigned char* o = dst + dof + pix * 3;
                o[0] = (unsigned char)exact_round8(a0);
                o[1] = (unsigned char)exact_round8(a1);
                o[2] = (unsigned char)exact_round8(a2);
            }
        }
    }
}

int pesr_degrade_u8_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n,
                           int s, int K, const double* bank_dev, int n_kernels, hipStream_t stream) {
    if (!src || !dst || !desc_host || !desc_dev || !bank_dev || n < 1 || n_kernels < 1) return PESR_EINVAL;
    if (s < 2 || s > 4 || K < 1 || K > DEGRADE_MAX_K || (K - s) % 2) return PESR_EINVAL;
    constexpr long long MAX_SIDE = 1LL << 26;              // 3 * W and s * (LR index) stay inside an int
    long long max_tiles = 1;
    for (int i = 0; i < n; ++i) {
        const long long* d = desc_host + (long long)i * DEGRADE_DESC;
        const long long H = d[2], W = d[3], y0 = d[4], x0 = d[5], h = d[6], w = d[7];
        if (d[0] < 0 || d[1] < 0 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || H % s || W % s) return PESR_EINVAL;
        if (h < 1 || w < 1 || y0 < 0 || x0 < 0 || y0 + h > H / s || x0 + w > W / s) return PESR_EINVAL;
        if (d[8] < 0 || d[8] >= n_kernels) return PESR_EINVAL;
        double sigma;
        __builtin_memcpy(&sigma, &d[9], 8);
        if (!exact_sigma_ok(sigma)) return PESR_EINVAL;
        const long long tiles = ((h + DEGRADE_TILE - 1) / DEGRADE_TILE) * ((w + DEGRADE_TILE - 1) / DEGRADE_TILE);
        if (tiles > max_tiles) max_tiles = tiles;
    }
    const dim3 grid = exact_pool_grid(n, max_tiles);
    if (s == 2) hipLaunchKernelGGL(degrade_kernel<2>, grid, dim3(DEGRADE_THREADS), 0, stream, src, dst, desc_dev, n, K, bank_dev);
    else if (s == 3) hipLaunchKernelGGL(degrade_kernel<3>, grid, dim3(DEGRADE_THREADS), 0, stream, src, dst, desc_dev, n, K, bank_dev);
    else hipLaunchKernelGGL(degrade_kernel<4>, grid, dim3(DEGRADE_THREADS), 0, stream, src, dst, desc_dev, n, K, bank_dev);
    return pesr_launch_status();
}
