// Tiled inference (docs/modes.md section 4h): the two data-movement kernels around the Generator of a tiled run, siblings of
// crop_augment_kernel (input_pipeline.hip).
//
// tile_gather_kernel cuts fixed-size tiles out of one LR image (fp32 [3][H][W] or uint8 [H][W][3]) and writes them as an
// NCHW-contiguous fp32 batch, each entry under one of the eight flips / transposes of test.py:x8_forward: member m = entry m of its
// `inputs` list - bit 0 reverses the W axis, then bit 1 reverses the H axis, then bit 2 transposes.  Values are copied exactly.
//
// tile_scatter_kernel takes the Generator's outputs of those entries, undoes each member's transform (transpose, then H, then W),
// forms
//     v = t0                                                        (E = 1)
//     v = (((((((t0 + t1) + t2) + t3) + t4) + t5) + t6) + t7) / 8   (E = 8)
//     out = v            or            out = wa * p + wb * v        (blend with the E = 1 result p of a second set of tiles)
// in fp32 with every operation rounded on its own (hence `fp contract(off)`: no fused multiply-add in this arithmetic), and writes the
// pixels each tile OWNS into the fp32 [3][s*H][s*W] and / or the uint8 [s*H][s*W][3] image (clamp to 0..255, round half to even).
// Every output pixel belongs to one tile: no atomics, the same bits on every run.
//
// Both kernels work on 32 x 32 pixel blocks with 32 x 8 lanes.  Members 0-3 read and write rows that are contiguous on both sides.
// Members 4-7 go through an LDS block with a row stride of 33 words: the global side is walked along its own rows (coalesced), the
// transposition happens between the LDS write and the LDS read (both conflict-free).  Offsets into the images are 64-bit.
#pragma clang fp contract(off)
#include "common.h"
#include "launchers.h"

constexpr int TILE_B = 32;              // block side in pixels
constexpr int TILE_TY = 8;              // lane rows: each lane handles TILE_B / TILE_TY rows of its column
constexpr int TILE_R = TILE_B / TILE_TY;
constexpr int TILE_LS = TILE_B + 1;     // LDS row stride

template <bool U8>
__device__ __forceinline__ float tile_src(const void* __restrict__ src, long P, int W, int c, int y, int x) {
    const long p = (long)y * W + x;
    if (U8) return (float)((const unsigned char*)src)[p * 3 + c];
    return ((const float*)src)[(long)c * P + p];
}

// grid (ceil(ow / 32), ceil(oh / 32), n).  desc: n rows {y0, x0, m}.  dst [n][3][oh][ow].
template <bool U8>
__global__ __launch_bounds__(TILE_B * TILE_TY) void tile_gather_kernel(const void* __restrict__ src, float* __restrict__ dst,
                                                                      const int* __restrict__ desc, int H, int W, int oh, int ow) {
    __shared__ float lds[3][TILE_B * TILE_LS];
    const int e = blockIdx.z;
    const int y0 = desc[e * 3], x0 = desc[e * 3 + 1], m = desc[e * 3 + 2];
    const bool tr = (m & 4) != 0, fw = (m & 1) != 0, fh = (m & 2) != 0;
    const int th = tr ? ow : oh, tw = tr ? oh : ow;          // the tile in the source image
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int i0 = blockIdx.y * TILE_B, j0 = blockIdx.x * TILE_B;   // block origin in the output entry
    const long P = (long)H * W;
    float* o = dst + (long)e * 3 * oh * ow;
    if (!tr) {
        const int j = j0 + tx;
#pragma unroll
        for (int r = 0; r < TILE_R; ++r) {
            const int i = i0 + ty + r * TILE_TY;
            if (i < oh && j < ow) {
                const int y = y0 + (fh ? th - 1 - i : i), x = x0 + (fw ? tw - 1 - j : j);
#pragma unroll
                for (int c = 0; c < 3; ++c) o[((long)c * oh + i) * ow + j] = tile_src<U8>(src, P, W, c, y, x);
            }
        }
        return;
    }
    // transposed: output (i, j) is flipped-tile (a, b) = (j, i).  Read with the lane index along b (the source row), write with it
    // along j.
    const int b = i0 + tx;
#pragma unroll
    for (int r = 0; r < TILE_R; ++r) {
        const int la = ty + r * TILE_TY, a = j0 + la;
        if (a < th && b < tw) {
            const int y = y0 + (fh ? th - 1 - a : a), x = x0 + (fw ? tw - 1 - b : b);
#pragma unroll
            for (int c = 0; c < 3; ++c) lds[c][la * TILE_LS + tx] = tile_src<U8>(src, P, W, c, y, x);
        }
    }
    __syncthreads();
    const int j = j0 + tx;
#pragma unroll
    for (int r = 0; r < TILE_R; ++r) {
        const int li = ty + r * TILE_TY, i = i0 + li;
        if (i < oh && j < ow) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[((long)c * oh + i) * ow + j] = lds[c][tx * TILE_LS + li];
        }
    }
}

int pesr_tile_gather_launch(const void* src, int src_u8, int H, int W, float* dst, const int* desc_host, const int* desc_dev, int n,
                            int oh, int ow, hipStream_t stream) {
    if (!src || !dst || !desc_host || !desc_dev || n < 1 || n > 65535 || H < 1 || W < 1 || oh < 1 || ow < 1) return PESR_EINVAL;
    if (src_u8 != 0 && src_u8 != 1) return PESR_EINVAL;
    if ((long)oh * ow > (1L << 28)) return PESR_EINVAL;
    for (int e = 0; e < n; ++e) {
        const int y0 = desc_host[e * 3], x0 = desc_host[e * 3 + 1], m = desc_host[e * 3 + 2];
        if (m < 0 || m > 7) return PESR_EINVAL;
        const long th = (m & 4) ? ow : oh, tw = (m & 4) ? oh : ow;
        if (y0 < 0 || x0 < 0 || y0 + th > H || x0 + tw > W) return PESR_EINVAL;
    }
    const dim3 grid((ow + TILE_B - 1) / TILE_B, (oh + TILE_B - 1) / TILE_B, n), block(TILE_B, TILE_TY);
    if (grid.y > 65535) return PESR_EINVAL;
    if (src_u8) hipLaunchKernelGGL(tile_gather_kernel<true>, grid, block, 0, stream, src, dst, desc_dev, H, W, oh, ow);
    else hipLaunchKernelGGL(tile_gather_kernel<false>, grid, block, 0, stream, src, dst, desc_dev, H, W, oh, ow);
    return pesr_launch_status();
}

struct TileScatterArgs {
    const float* t_lo;      // E = 1: the entries; E = 8: members 0-3 (and 4-7 behind them when t_hi == t_lo + 4 entries)
    const float* t_hi;      // members 4-7 of tile 0 (E = 8)
    const float* p;         // blend partner or null
    float* out_f;
    unsigned char* out_u;
    const int* desc;        // rows {y0, x0, oy, ox, oh, ow} in LR pixels
    long lo_stride, hi_stride;   // floats between one tile's first entry and the next tile's, in t_lo / t_hi
    long tsc, tsp, psc, psp;     // element (c, pixel q) of an entry at c * sc + q * sp
    int H, W, th, tw, s;
    float wa, wb;
};

__device__ __forceinline__ unsigned char tile_u8(float v) {
    return (unsigned char)rintf(fminf(fmaxf(v, 0.0f), 255.0f));
}

// grid (ceil(s * max ow / 32), ceil(s * max oh / 32), tiles)
template <int E>
__global__ __launch_bounds__(TILE_B * TILE_TY) void tile_scatter_kernel(const TileScatterArgs A) {
    __shared__ float lds[3][TILE_B * TILE_LS];
    const int k = blockIdx.z;
    const int* d = A.desc + k * 6;
    const int s = A.s;
    const int Ht = s * A.th, Wt = s * A.tw;                        // a tile's output
    const int a_lo = s * (d[2] - d[0]), b_lo = s * (d[3] - d[1]);  // the owned rectangle in that output
    const int a_hi = a_lo + s * d[4], b_hi = b_lo + s * d[5];
    const int A0 = a_lo + blockIdx.y * TILE_B, B0 = b_lo + blockIdx.x * TILE_B;
    if (A0 >= a_hi || B0 >= b_hi) return;                          // uniform over the workgroup
    const int tx = threadIdx.x, ty = threadIdx.y;
    const long ent = 3L * Ht * Wt;
    const int b = B0 + tx;

    float v[TILE_R][3];
    // members 0-3 (E = 1: member 0 alone): rows of the entry are rows of the output
#pragma unroll
    for (int m = 0; m < (E == 8 ? 4 : 1); ++m) {
        const float* t = A.t_lo + k * A.lo_stride + m * ent;
#pragma unroll
        for (int r = 0; r < TILE_R; ++r) {
            const int a = A0 + ty + r * TILE_TY;
            if (a < a_hi && b < b_hi) {
                const int a1 = (m & 2) ? Ht - 1 - a : a, b1 = (m & 1) ? Wt - 1 - b : b;
                const long q = (long)a1 * Wt + b1;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float x = t[c * A.tsc + q * A.tsp];
                    v[r][c] = m == 0 ? x : v[r][c] + x;
                }
            }
        }
    }
    if (E == 8) {
        // members 4-7: the entry is [Wt][Ht]; output (a, b) is its element (b1, a1).  Read with the lane index along a1 (the entry's
        // row), use with it along b.
#pragma unroll
        for (int m = 4; m < 8; ++m) {
            const float* t = A.t_hi + k * A.hi_stride + (m - 4) * ent;
            const int a = A0 + tx;
            __syncthreads();
#pragma unroll
            for (int r = 0; r < TILE_R; ++r) {
                const int lb = ty + r * TILE_TY, bb = B0 + lb;
                if (a < a_hi && bb < b_hi) {
                    const int a1 = (m & 2) ? Ht - 1 - a : a, b1 = (m & 1) ? Wt - 1 - bb : bb;
                    const long q = (long)b1 * Ht + a1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) lds[c][lb * TILE_LS + tx] = t[c * A.tsc + q * A.tsp];
                }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < TILE_R; ++r) {
                const int la = ty + r * TILE_TY;
                if (A0 + la < a_hi && b < b_hi) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[r][c] = v[r][c] + lds[c][tx * TILE_LS + la];
                }
            }
        }
    }
    const long sW = (long)s * A.W, sP = (long)s * A.H * sW;
#pragma unroll
    for (int r = 0; r < TILE_R; ++r) {
        const int a = A0 + ty + r * TILE_TY;
        if (a < a_hi && b < b_hi) {
            const long q = (long)a * Wt + b;
            const long o = ((long)s * d[0] + a) * sW + ((long)s * d[1] + b);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float x = E == 8 ? v[r][c] / 8.0f : v[r][c];
                if (A.p) {
                    const float pa = A.wa * A.p[k * ent + c * A.psc + q * A.psp];
                    const float vb = A.wb * x;
                    x = pa + vb;
                }
                if (A.out_f) A.out_f[c * sP + o] = x;
                if (A.out_u) A.out_u[o * 3 + c] = tile_u8(x);
            }
        }
    }
}

int pesr_tile_scatter_launch(const float* t_lo, const float* t_hi, int t_nhwc, const float* p, int p_nhwc, float wa, float wb,
                             const int* desc_host, const int* desc_dev, int n, int E, int th, int tw, int s, int H, int W,
                             float* out_f32, unsigned char* out_u8, hipStream_t stream) {
    if (!t_lo || !desc_host || !desc_dev || (!out_f32 && !out_u8)) return PESR_EINVAL;
    if ((E != 1 && E != 8) || s < 2 || s > 4 || n < 1 || n % E) return PESR_EINVAL;
    if ((t_nhwc != 0 && t_nhwc != 1) || (p_nhwc != 0 && p_nhwc != 1)) return PESR_EINVAL;
    if (H < 1 || W < 1 || th < 1 || tw < 1 || th > H || tw > W) return PESR_EINVAL;
    if ((long)s * s * th * tw > (1L << 28) || (long)s * H > (1L << 30) || (long)s * W > (1L << 30)) return PESR_EINVAL;
    if (E == 1 && t_hi) return PESR_EINVAL;
    if (E == 8 && !t_hi && th != tw) return PESR_EINVAL;            // one tensor holds all eight members of square tiles only
    const int tiles = n / E;
    if (tiles > 65535) return PESR_EINVAL;
    int max_oh = 0, max_ow = 0;
    for (int k = 0; k < tiles; ++k) {
        const int* d = desc_host + k * 6;
        const long y0 = d[0], x0 = d[1], oy = d[2], ox = d[3], oh = d[4], ow = d[5];
        if (y0 < 0 || x0 < 0 || y0 + th > H || x0 + tw > W) return PESR_EINVAL;
        if (oh < 1 || ow < 1 || oy < y0 || ox < x0 || oy + oh > y0 + th || ox + ow > x0 + tw) return PESR_EINVAL;
        if (oh > max_oh) max_oh = (int)oh;
        if (ow > max_ow) max_ow = (int)ow;
    }
    const long Q = (long)s * s * th * tw, ent = 3 * Q;
    TileScatterArgs A;
    A.t_lo = t_lo;
    A.t_hi = E == 8 ? (t_hi ? t_hi : t_lo + 4 * ent) : nullptr;
    A.lo_stride = E == 1 ? ent : (t_hi ? 4 * ent : 8 * ent);
    A.hi_stride = A.lo_stride;
    A.p = p;
    A.out_f = out_f32;
    A.out_u = out_u8;
    A.desc = desc_dev;
    A.tsc = t_nhwc ? 1 : Q;
    A.tsp = t_nhwc ? 3 : 1;
    A.psc = p_nhwc ? 1 : Q;
    A.psp = p_nhwc ? 3 : 1;
    A.H = H;
    A.W = W;
    A.th = th;
    A.tw = tw;
    A.s = s;
    A.wa = wa;
    A.wb = wb;
    const dim3 grid((s * max_ow + TILE_B - 1) / TILE_B, (s * max_oh + TILE_B - 1) / TILE_B, tiles), block(TILE_B, TILE_TY);
    if (grid.y > 65535) return PESR_EINVAL;
    if (E == 8) hipLaunchKernelGGL(tile_scatter_kernel<8>, grid, block, 0, stream, A);
    else hipLaunchKernelGGL(tile_scatter_kernel<1>, grid, block, 0, stream, A);
    return pesr_launch_status();
}
