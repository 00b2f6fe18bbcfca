// Bicubic resize of uint8 HWC images by an integer factor s in {2, 3, 4}, down (antialiased) and up: MATLAB's imresize for uint8
// input as pinned in docs/modes.md section 4f.  One launch per pass (height, then width, uint8 in between) serves a whole pool of
// images through a descriptor array, as crop_augment_kernel does: per image {source byte offset, destination byte offset, H, W} with
// H, W the size of the pass's INPUT image.
//   down: out[o] = round(sum_t w[t] * in[reflect(s*o + T0 + t)]),  t = 0 .. NT-1          (NT = 8 / 11 / 16, T0 = -3 / -4 / -6)
//   up:   out[s*q + p] = round(sum_i w[p][i] * in[reflect(q + d_p + i)]),  i = 0 .. 3     (d_p = -2 if 2p + 1 < s, else -1)
// float64, acc = acc + w * v in ascending tap order with the product and the sum rounded separately (no fused multiply-add: the
// host restatement must reproduce every bit), clamp to [0, 255], round half up (exact_u8.h).  The weights come from the host by value.
// Height pass: all taps of an output byte sit at the same byte column of other rows, so a lane owns 4 consecutive bytes of an output
// row and walks the taps down the rows with dword loads (coalesced; rows of 3W bytes start at any alignment - gfx950 global memory
// takes unaligned dwords).  Width pass: neighbouring outputs read overlapping windows 3 bytes apart: a workgroup stages the row
// segment it needs, reflected halo included, in LDS and reads the taps from there.
#pragma clang fp contract(off)
#include "common.h"
#include "launchers.h"
#include "exact_u8.h"

struct ResizeWeights { double w[16]; };

template <int S> struct DownTaps {
    static constexpr int N = S == 2 ? 8 : (S == 3 ? 11 : 16);
    static constexpr int T0 = S == 2 ? -3 : (S == 3 ? -4 : -6);
};

constexpr int RESIZE_THREADS = 256;
constexpr int RESIZE_H_TILE = RESIZE_THREADS * 4;      // bytes of one output row per workgroup
constexpr int RESIZE_W_PIX = 340;                      // output pixels of one row per workgroup: 1020 bytes, 4 per lane on 255 lanes

template <int S, bool UP>
__global__ __launch_bounds__(RESIZE_THREADS) void resize_h_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                  const long long* __restrict__ desc, int n_images, ResizeWeights W) {
    constexpr int NT = UP ? 4 : DownTaps<S>::N;
    __shared__ double sw[16];
    if (UP) {
#pragma unroll
        for (int i = 0; i < 4 * S; ++i)
            if (threadIdx.x == i) sw[i] = W.w[i];
        __syncthreads();
    }
    for (int img = blockIdx.y; img < n_images; img += gridDim.y) {
        const long long so = desc[img * 4], dof = desc[img * 4 + 1];
        const int H = (int)desc[img * 4 + 2];
        const long long R = 3 * desc[img * 4 + 3];                      // bytes per row, input and output alike
        const int Ho = UP ? H * S : H / S;
        const long long ctiles = (R + RESIZE_H_TILE - 1) / RESIZE_H_TILE;
        const long long tiles = Ho * ctiles;
        for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int yo = (int)(t / ctiles);
            const long long col = (t % ctiles) * RESIZE_H_TILE + threadIdx.x * 4;
            if (col >= R) continue;
            const int nb = R - col < 4 ? (int)(R - col) : 4;
            int j0, wbase = 0;
            if (UP) {
                const int q = yo / S, p = yo % S;
                j0 = q + (2 * p + 1 < S ? -2 : -1);
                wbase = p * 4;
            } else {
                j0 = S * yo + DownTaps<S>::T0;
            }
            const unsigned char* base = src + so + col;
            unsigned v[NT];
#pragma unroll
            for (int i = 0; i < NT; ++i) v[i] = exact_load4(base + (long long)exact_reflect(j0 + i, H) * R, nb);
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const double w = UP ? sw[wbase + i] : W.w[i];
                a0 = exact_mac_u(a0, w, v[i] & 0xff);
                a1 = exact_mac_u(a1, w, (v[i] >> 8) & 0xff);
                a2 = exact_mac_u(a2, w, (v[i] >> 16) & 0xff);
                a3 = exact_mac_u(a3, w, v[i] >> 24);
            }
            const unsigned o = exact_round8x4(a0, a1, a2, a3);
            exact_store4(dst + dof + (long long)yo * R + col, o, nb);
        }
    }
}

template <int S, bool UP>
__global__ __launch_bounds__(RESIZE_THREADS) void resize_w_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                  const long long* __restrict__ desc, int n_images, ResizeWeights W) {
    constexpr int NT = UP ? 4 : DownTaps<S>::N;
    constexpr int IN_PIX = UP ? RESIZE_W_PIX / S + 6 : RESIZE_W_PIX * S + NT;       // input pixels one tile can need (rounded up)
    constexpr int SM_BYTES = (IN_PIX * 3 + 3) / 4 * 4;
    __shared__ __attribute__((aligned(16))) unsigned char sm[SM_BYTES];
    __shared__ double sw[16];
    if (UP) {
#pragma unroll
        for (int i = 0; i < 4 * S; ++i)
            if (threadIdx.x == i) sw[i] = W.w[i];
    }
    for (int img = blockIdx.y; img < n_images; img += gridDim.y) {
        const long long so = desc[img * 4], dof = desc[img * 4 + 1];
        const int H = (int)desc[img * 4 + 2], Wi = (int)desc[img * 4 + 3];
        const int Wo = UP ? Wi * S : Wi / S;
        const long long ctiles = (Wo + RESIZE_W_PIX - 1) / RESIZE_W_PIX;
        const long long tiles = H * ctiles;
        for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int y = (int)(t / ctiles);
            const int xo_lo = (int)(t % ctiles) * RESIZE_W_PIX;
            const int xo_hi = min(xo_lo + RESIZE_W_PIX, Wo) - 1;
            const int in_lo = UP ? xo_lo / S - 2 : S * xo_lo + DownTaps<S>::T0;
            const int in_hi = UP ? xo_hi / S + 2 : S * xo_hi + DownTaps<S>::T0 + NT - 1;
            const int nbytes = (in_hi - in_lo + 1) * 3;                 // <= SM_BYTES by construction
            const unsigned char* rowp = src + so + (long long)y * (3LL * Wi);
            __syncthreads();                                            // the previous tile's readers are done (and sw is written)
            for (int k = threadIdx.x * 4; k < nbytes; k += RESIZE_THREADS * 4) {
                const int px0 = in_lo + k / 3, px3 = in_lo + (k + 3) / 3;
                if (k + 3 < nbytes && px0 >= 0 && px3 < Wi) {
                    unsigned v;
                    __builtin_memcpy(&v, rowp + (3LL * in_lo + k), 4);
                    *(unsigned*)(sm + k) = v;
                } else {
                    for (int b = 0; b < 4 && k + b < nbytes; ++b) {
                        const int kk = k + b;
                        sm[kk] = rowp[3LL * exact_reflect(in_lo + kk / 3, Wi) + kk % 3];
                    }
                }
            }
            __syncthreads();
            const int tile_bytes = (xo_hi - xo_lo + 1) * 3;
            const int ob0 = threadIdx.x * 4;
            if (ob0 < tile_bytes) {
                const int nb = min(4, tile_bytes - ob0);
                unsigned o = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    if (b < nb) {
                        const int rel = (ob0 + b) / 3, c = (ob0 + b) % 3;
                        int idx, wbase = 0;
                        if (UP) {
                            const int xo = xo_lo + rel, q = xo / S, p = xo % S;
                            idx = 3 * (q + (2 * p + 1 < S ? -2 : -1) - in_lo) + c;
                            wbase = p * 4;
                        } else {
                            idx = 3 * S * rel + c;                      // in_lo is the first tap of the tile's first pixel
                        }
                        double acc = 0.0;
#pragma unroll
                        for (int i = 0; i < NT; ++i) acc = exact_mac_u(acc, UP ? sw[wbase + i] : W.w[i], sm[idx + 3 * i]);
                        o |= (unsigned)exact_round8(acc) << (8 * b);
                    }
                }
                exact_store4(dst + dof + (long long)y * (3LL * Wo) + 3LL * xo_lo + ob0, o, nb);
            }
        }
    }
}

template <int S, bool UP>
static void resize_launch(int axis, dim3 grid, hipStream_t stream, const unsigned char* src, unsigned char* dst, const long long* desc,
                          int n_images, const ResizeWeights& W) {
    if (axis == 0)
        hipLaunchKernelGGL((resize_h_kernel<S, UP>), grid, dim3(RESIZE_THREADS), 0, stream, src, dst, desc, n_images, W);
    else
        hipLaunchKernelGGL((resize_w_kernel<S, UP>), grid, dim3(RESIZE_THREADS), 0, stream, src, dst, desc, n_images, W);
}

int pesr_imresize_u8_pass_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev,
                                 int n_images, int axis, int s, int up, const double* weights_host, hipStream_t stream) {
    if (!src || !dst || !desc_host || !desc_dev || !weights_host || n_images < 1) return PESR_EINVAL;
    if (s < 2 || s > 4 || (axis != 0 && axis != 1) || (up != 0 && up != 1)) return PESR_EINVAL;
    constexpr long long MAX_SIDE = 1LL << 26;              // 3 * W * s and H * s stay inside an int
    long long max_tiles = 1;
    for (int i = 0; i < n_images; ++i) {
        const long long so = desc_host[i * 4], dof = desc_host[i * 4 + 1], H = desc_host[i * 4 + 2], W = desc_host[i * 4 + 3];
        if (so < 0 || dof < 0 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) return PESR_EINVAL;
        const long long n = axis == 0 ? H : W;
        if (!up && n % s) return PESR_EINVAL;
        long long tiles;
        if (axis == 0) {
            tiles = (up ? H * s : H / s) * ((3 * W + RESIZE_H_TILE - 1) / RESIZE_H_TILE);
        } else {
            tiles = H * (((up ? W * s : W / s) + RESIZE_W_PIX - 1) / RESIZE_W_PIX);
        }
        if (tiles > max_tiles) max_tiles = tiles;
    }
    const dim3 grid = exact_pool_grid(n_images, max_tiles);
    ResizeWeights W;
    for (int i = 0; i < 16; ++i) W.w[i] = weights_host[i];
    if (up) {
        if (s == 2) resize_launch<2, true>(axis, grid, stream, src, dst, desc_dev, n_images, W);
        else if (s == 3) resize_launch<3, true>(axis, grid, stream, src, dst, desc_dev, n_images, W);
        else resize_launch<4, true>(axis, grid, stream, src, dst, desc_dev, n_images, W);
    } else {
        if (s == 2) resize_launch<2, false>(axis, grid, stream, src, dst, desc_dev, n_images, W);
        else if (s == 3) resize_launch<3, false>(axis, grid, stream, src, dst, desc_dev, n_images, W);
        else resize_launch<4, false>(axis, grid, stream, src, dst, desc_dev, n_images, W);
    }
    return pesr_launch_status();
}
