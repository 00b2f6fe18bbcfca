// Resize of uint8 HWC images from any size to any size (each axis within 8:1 either way) with a bicubic, bilinear or box filter, as
// pinned in docs/modes.md section 4m: section 4f's arithmetic (float64, acc = acc + w * v in ascending tap order with the product and
// the sum rounded separately, symmetric reflection at the border, clamp, round half up, height pass then width pass with a uint8
// intermediate) with taps and weights that come from a table the HOST makes - the device evaluates no polynomial and no division.
// One launch per pass serves n entries through a descriptor array of RT_DESC int64 words per entry:
//   {source byte offset, source row stride in pixels, destination byte offset, destination row stride in pixels, h_in, w_in, h_out,
//    w_out, offset of the entry's table in the table buffer (8-byte words), taps T, float64 bits of sigma_n, noise stream}
// so an entry may be a window of a larger image (the reflection is at the window's own border), at any byte alignment.
// Table of an axis (n_out outputs, T taps), tap-major: word [o] = the unreflected first tap of output o (int64), word
// [(1 + k) * n_out + o] = weight k of output o (float64; rows with fewer taps end in 0.0, and acc + 0.0 * v == acc).  Tap-major so that
// in the width pass, where neighbouring lanes own neighbouring outputs, every weight read of a wave is one run of consecutive doubles;
// in the height pass the weight and the source row are uniform over the workgroup.
//   out[o] = round(sum_k w[k][o] * in[reflect(first[o] + k)]),  k = 0 .. T-1
//   width pass, if sigma_n != 0: acc = acc + sigma_n * g(splitmix64(stream), e),  e = (y * w_out + x) * 3 + c  (degrade.hip's noise)
// Height pass: a lane owns 4 consecutive bytes of an output row and walks the taps down the rows with dword loads (resize.hip's
// scheme).  Width pass: a workgroup owns RT_W_PIX neighbouring output pixels of one row, one pixel (three sums) per lane; the source
// pixels between the first tap of its first output and the last tap of its last one - at 8:1 eight times the tile plus a kernel width -
// are staged in LDS, reflected, one dword per pixel, so a tap costs one LDS read and one weight read for three multiply-adds.  A lane
// whose taps are not all inside the staged run (never with a table the host made; the table is device memory the library cannot
// check) reads them from global memory instead: no table content can take an access outside the entry's window.
#pragma clang fp contract(off)
#include "common.h"
#include "launchers.h"
#include "exact_u8.h"

constexpr int RT_THREADS = 256;
constexpr int RT_DESC = 12;                            // int64 words per entry (include/pesr_hip.h)
constexpr int RT_MAX_TAPS = 32;
constexpr int RT_MAX_RATIO = 8;
constexpr int RT_H_TILE = RT_THREADS * 4;              // bytes of one output row per workgroup (height pass)
constexpr int RT_W_PIX = RT_THREADS;                   // output pixels of one row per workgroup (width pass)
constexpr int RT_W_SPAN = RT_W_PIX * RT_MAX_RATIO + RT_MAX_TAPS;   // source pixels a tile can need at the 8:1 limit (8 KiB + 128 B of LDS)

// a first tap as the table holds it, kept where first + k cannot overflow whatever the table says
__device__ __forceinline__ long long rt_first(const long long* __restrict__ tab, int o) {
    const long long lim = 1LL << 40;
    const long long f = tab[o];
    return f < -lim ? -lim : (f > lim ? lim : f);
}

__global__ __launch_bounds__(RT_THREADS) void resize_to_h_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                 const long long* __restrict__ desc, int n,
                                                                 const long long* __restrict__ tables) {
    for (int ent = blockIdx.y; ent < n; ent += gridDim.y) {
        const long long* d = desc + (long long)ent * RT_DESC;
        const long long so = d[0], sstride = 3 * d[1], dof = d[2], dstride = 3 * d[3];
        const int H = (int)d[4], Ho = (int)d[6], T = (int)d[9];
        const long long R = 3 * d[5];                                   // bytes per row of the window, input and output alike
        const long long* tab = tables + d[8];
        const double* wt = (const double*)tab + Ho;
        const long long ctiles = (R + RT_H_TILE - 1) / RT_H_TILE;
        const long long tiles = Ho * ctiles;
        for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int yo = (int)(t / ctiles);
            const long long col = (t % ctiles) * RT_H_TILE + threadIdx.x * 4;
            if (col >= R) continue;
            const int nb = R - col < 4 ? (int)(R - col) : 4;
            const long long j0 = rt_first(tab, yo);
            const unsigned char* base = src + so + col;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            for (int k = 0; k < T; ++k) {
                const double w = wt[(long long)k * Ho + yo];
                const unsigned v = exact_load4(base + exact_reflect(j0 + k, H) * sstride, nb);
                a0 = exact_mac_u(a0, w, v & 0xff);
                a1 = exact_mac_u(a1, w, (v >> 8) & 0xff);
                a2 = exact_mac_u(a2, w, (v >> 16) & 0xff);
                a3 = exact_mac_u(a3, w, v >> 24);
            }
            const unsigned o = exact_round8x4(a0, a1, a2, a3);
            exact_store4(dst + dof + yo * dstride + col, o, nb);
        }
    }
}

__global__ __launch_bounds__(RT_THREADS) void resize_to_w_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                 const long long* __restrict__ desc, int n,
                                                                 const long long* __restrict__ tables) {
    __shared__ unsigned spx[RT_W_SPAN];                                 // r | g << 8 | b << 16 of the reflected source run
    for (int ent = blockIdx.y; ent < n; ent += gridDim.y) {
        const long long* d = desc + (long long)ent * RT_DESC;
        const long long so = d[0], sstride = 3 * d[1], dof = d[2], dstride = 3 * d[3];
        const int H = (int)d[4], Wi = (int)d[5], Wo = (int)d[7], T = (int)d[9];
        const long long* tab = tables + d[8];
        const double* wt = (const double*)tab + Wo;
        double sigma;
        __builtin_memcpy(&sigma, &d[10], 8);
        const unsigned long long key = exact_splitmix64((unsigned long long)d[11]);
        const long long ctiles = (Wo + RT_W_PIX - 1) / RT_W_PIX;
        const long long tiles = H * ctiles;
        for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int y = (int)(t / ctiles);
            const int xo_lo = (int)(t % ctiles) * RT_W_PIX;
            const int xo_hi = min(xo_lo + RT_W_PIX, Wo) - 1;
            const long long in_lo = rt_first(tab, xo_lo);
            long long span = rt_first(tab, xo_hi) + T - in_lo;         // first tap of the first output .. last tap of the last one
            span = span < 0 ? 0 : (span > RT_W_SPAN ? RT_W_SPAN : span);
            const unsigned char* rowp = src + so + y * sstride;
            __syncthreads();                                            // the previous tile's readers are done
            for (int p = threadIdx.x; p < (int)span; p += RT_THREADS) spx[p] = exact_load_px(rowp + 3LL * exact_reflect(in_lo + p, Wi));
            __syncthreads();
            const int xo = xo_lo + threadIdx.x;
            if (xo <= xo_hi) {
                const long long j0 = rt_first(tab, xo);
                const long long rel = j0 - in_lo;
                const double* w = wt + xo;
                double a0 = 0.0, a1 = 0.0, a2 = 0.0;
                if (rel >= 0 && rel + T <= span) {
                    const unsigned* px = spx + rel;
                    for (int k = 0; k < T; ++k) {
                        const double wk = w[(long long)k * Wo];
                        const unsigned v = px[k];
                        a0 = exact_mac_u(a0, wk, v & 0xff);
                        a1 = exact_mac_u(a1, wk, (v >> 8) & 0xff);
                        a2 = exact_mac_u(a2, wk, v >> 16);
                    }
                } else {
                    for (int k = 0; k < T; ++k) {
                        const double wk = w[(long long)k * Wo];
                        const unsigned v = exact_load_px(rowp + 3LL * exact_reflect(j0 + k, Wi));
                        a0 = exact_mac_u(a0, wk, v & 0xff);
                        a1 = exact_mac_u(a1, wk, (v >> 8) & 0xff);
                        a2 = exact_mac_u(a2, wk, v >> 16);
                    }
                }
                if (sigma != 0.0) {
                    const unsigned long long e = 3ULL * ((unsigned long long)y * (unsigned long long)Wo + (unsigned long long)xo);
                    a0 = exact_noise(a0, sigma, exact_gauss(key, e));
                    a1 = exact_noise(a1, sigma, exact_gauss(key, e + 1));
                    a2 = exact_noise(a2, sigma, exact_gauss(key, e + 2));
                }
                unsigned char* o = dst + dof + y * dstride + 3LL * xo;
                o[0] = (unsigned char)(unsigned)exact_round8(a0);        // (through unsigned, as exact_round8x4 converts)
                o[1] = (unsigned char)(unsigned)exact_round8(a1);
                o[2] = (unsigned char)(unsigned)exact_round8(a2);
            }
        }
    }
}

int pesr_resize_to_u8_pass_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev,
                                  int n, int axis, const void* tables_dev, long table_words, hipStream_t stream) {
    if (!src || !dst || !desc_host || !desc_dev || !tables_dev || n < 1 || table_words < 1) return PESR_EINVAL;
    if (axis != 0 && axis != 1) return PESR_EINVAL;
    constexpr long long MAX_SIDE = 1LL << 24;              // 3 * W and the table's integers stay far inside an int / a float64
    long long max_tiles = 1;
    for (int i = 0; i < n; ++i) {
        const long long* d = desc_host + (long long)i * RT_DESC;
        const long long sstride = d[1], dstride = d[3], hi = d[4], wi = d[5], ho = d[6], wo = d[7], toff = d[8], T = d[9];
        if (d[0] < 0 || d[2] < 0) return PESR_EINVAL;
        if (hi < 1 || wi < 1 || ho < 1 || wo < 1 || hi > MAX_SIDE || wi > MAX_SIDE || ho > MAX_SIDE || wo > MAX_SIDE) return PESR_EINVAL;
        // the pass resizes its own axis and leaves the other one as it is
        const long long n_in = axis == 0 ? hi : wi, n_out = axis == 0 ? ho : wo;
        if ((axis == 0 ? wo != wi : ho != hi)) return PESR_EINVAL;
        if (n_in > RT_MAX_RATIO * n_out || n_out > RT_MAX_RATIO * n_in) return PESR_EINVAL;
        if (sstride < wi || dstride < wo || sstride > MAX_SIDE || dstride > MAX_SIDE) return PESR_EINVAL;
        if (T < 1 || T > RT_MAX_TAPS) return PESR_EINVAL;
        if (toff < 0 || toff > table_words || (T + 1) * n_out > table_words - toff) return PESR_EINVAL;
        double sigma;
        __builtin_memcpy(&sigma, &d[10], 8);
        if (!exact_sigma_ok(sigma)) return PESR_EINVAL;
        if (axis == 0 && sigma != 0.0) return PESR_EINVAL;                                     // the noise belongs to the width pass
        const long long tiles = axis == 0 ? ho * ((3 * wi + RT_H_TILE - 1) / RT_H_TILE) : hi * ((wo + RT_W_PIX - 1) / RT_W_PIX);
        if (tiles > max_tiles) max_tiles = tiles;
    }
    const dim3 grid = exact_pool_grid(n, max_tiles);
    const long long* tables = (const long long*)tables_dev;
    if (axis == 0)
        hipLaunchKernelGGL(resize_to_h_kernel, grid, dim3(RT_THREADS), 0, stream, src, dst, desc_dev, n, tables);
    else
        hipLaunchKernelGGL(resize_to_w_kernel, grid, dim3(RT_THREADS), 0, stream, src, dst, desc_dev, n, tables);
    return pesr_launch_status();
}
