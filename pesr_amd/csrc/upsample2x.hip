// Bilinear x2 upsampling (F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)) of an NHWC fp32 map, with an optional
// second addend, and its exact adjoint (docs/modes.md section 4v: the decoder of the U-Net discriminator).
//   forward   y [N][2H][2W][C] = up2(a + b)      per axis  out[2i]   = 0.25 in[max(i-1, 0)] + 0.75 in[i]
//                                                          out[2i+1] = 0.75 in[i] + 0.25 in[min(i+1, n-1)]
//   backward  gx [N][H][W][C]  = up2^T(gy)       per axis  in[i] gathers rows clamp(2i-1), 2i, 2i+1, clamp(2i+2) with 0.25, 0.75, 0.75,
//                                                          0.25: the clamp folds the border taps onto the edge pixel
// Both are streaming kernels: a 256-lane workgroup takes a tile of 8 x 8 input pixels (backward: gx pixels) and a block of channel
// units, reads the tile and its halo from global memory ONCE into LDS (forward: already summed, a + b rounded once) and every lane then
// works from LDS.  A unit is four channels (one 16-byte access) where C % 4 == 0 and the tensors sit on 16-byte boundaries, else one
// float.  No atomics; every output is a fixed expression of its inputs (forward: the row pass, then the column pass; backward: the
// four rows in increasing order, each row's four taps in increasing order), so every call gives the same bits.  size_t element offsets.
#include "common.h"
#include "launchers.h"

#define UP_LANES 256
#define UP_TH 8
#define UP_TW 8
#define UP_FWD_CB 16      // units per workgroup, forward:  10 x 10 x 16 units = 25.6 KB of LDS as f32x4
#define UP_BWD_CB 8       // ... backward: 18 x 18 x 8 units = 41.5 KB

namespace {

struct UpGeom {
    int H, W;             // of the low-resolution map (a, gx)
    int U;                // units per pixel
    int tiles_x, tiles_y, ublocks;
};

__device__ __forceinline__ int up_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <typename T, bool ADD>
__global__ __launch_bounds__(UP_LANES) void up2_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y, UpGeom g) {
    constexpr int HH = UP_TH + 2, HW = UP_TW + 2, CB = UP_FWD_CB;
    __shared__ T s[HH * HW * CB];
    int bid = blockIdx.x;
    const int ub = bid % g.ublocks; bid /= g.ublocks;
    const int tx = bid % g.tiles_x; bid /= g.tiles_x;
    const int ty = bid % g.tiles_y;
    const int n = bid / g.tiles_y;
    const int i0 = ty * UP_TH, j0 = tx * UP_TW, u0 = ub * CB;
    const int cb = g.U - u0 < CB ? g.U - u0 : CB;
    const size_t img = (size_t)n * g.H * g.W * g.U;
    for (int e = threadIdx.x; e < HH * HW * CB; e += UP_LANES) {
        const int uu = e % CB, p = e / CB;
        if (uu >= cb) continue;
        const int gi = up_clamp(i0 + p / HW - 1, g.H - 1), gj = up_clamp(j0 + p % HW - 1, g.W - 1);
        const size_t off = img + ((size_t)gi * g.W + gj) * g.U + u0 + uu;
        T v = a[off];
        if (ADD) v = v + b[off];
        s[e] = v;
    }
    __syncthreads();
    const size_t W2U = (size_t)2 * g.W * g.U;
    for (int e = threadIdx.x; e < UP_TH * UP_TW * CB; e += UP_LANES) {
        const int uu = e % CB, p = e / CB;
        const int pi = p / UP_TW, pj = p % UP_TW;
        const int i = i0 + pi, j = j0 + pj;
        if (uu >= cb || i >= g.H || j >= g.W) continue;
        T hl[3], hr[3];                       // the row pass at output columns 2j and 2j + 1, input rows i - 1, i, i + 1
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const T* row = s + ((pi + r) * HW + pj) * CB + uu;
            const T l = row[0], c = row[CB], q = row[2 * CB];
            hl[r] = l * 0.25f + c * 0.75f;
            hr[r] = c * 0.75f + q * 0.25f;
        }
        const size_t o = (size_t)n * 4 * g.H * g.W * g.U + (size_t)(2 * i) * W2U + (size_t)(2 * j) * g.U + u0 + uu;
        y[o] = hl[0] * 0.25f + hl[1] * 0.75f;
        y[o + g.U] = hr[0] * 0.25f + hr[1] * 0.75f;
        y[o + W2U] = hl[1] * 0.75f + hl[2] * 0.25f;
        y[o + W2U + g.U] = hr[1] * 0.75f + hr[2] * 0.25f;
    }
}

template <typename T>
__global__ __launch_bounds__(UP_LANES) void up2_bwd_kernel(const T* __restrict__ gy, T* __restrict__ gx, UpGeom g) {
    constexpr int HH = 2 * UP_TH + 2, HW = 2 * UP_TW + 2, CB = UP_BWD_CB;
    __shared__ T s[HH * HW * CB];
    int bid = blockIdx.x;
    const int ub = bid % g.ublocks; bid /= g.ublocks;
    const int tx = bid % g.tiles_x; bid /= g.tiles_x;
    const int ty = bid % g.tiles_y;
    const int n = bid / g.tiles_y;
    const int i0 = ty * UP_TH, j0 = tx * UP_TW, u0 = ub * CB;
    const int cb = g.U - u0 < CB ? g.U - u0 : CB;
    const size_t img = (size_t)n * 4 * g.H * g.W * g.U;
    for (int e = threadIdx.x; e < HH * HW * CB; e += UP_LANES) {
        const int uu = e % CB, p = e / CB;
        if (uu >= cb) continue;
        // gy rows 2 i0 - 1 .. 2 i0 + 2 TH: clamped into the map, which is what folds the border taps (and keeps a ragged tile in bounds)
        const int gi = up_clamp(2 * i0 - 1 + p / HW, 2 * g.H - 1), gj = up_clamp(2 * j0 - 1 + p % HW, 2 * g.W - 1);
        s[e] = gy[img + ((size_t)gi * (2 * g.W) + gj) * g.U + u0 + uu];
    }
    __syncthreads();
    const float wt[4] = {0.25f, 0.75f, 0.75f, 0.25f};
    for (int e = threadIdx.x; e < UP_TH * UP_TW * CB; e += UP_LANES) {
        const int uu = e % CB, p = e / CB;
        const int pi = p / UP_TW, pj = p % UP_TW;
        const int i = i0 + pi, j = j0 + pj;
        if (uu >= cb || i >= g.H || j >= g.W) continue;
        T acc = {};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const T* row = s + ((2 * pi + r) * HW + 2 * pj) * CB + uu;
            T h = row[0] * wt[0];
#pragma unroll
            for (int c = 1; c < 4; ++c) h = h + row[c * CB] * wt[c];
            acc = r == 0 ? h * wt[0] : acc + h * wt[r];
        }
        gx[(size_t)n * g.H * g.W * g.U + ((size_t)i * g.W + j) * g.U + u0 + uu] = acc;
    }
}

bool up_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// -> false for a shape whose grid or whose 2H x 2W map does not fit the kernels' ints
bool up_geom(int N, int H, int W, int C, bool vec, int cb, UpGeom* g) {
    if (N < 1 || H < 1 || W < 1 || C < 1 || H > (1 << 29) || W > (1 << 29)) return false;
    g->H = H; g->W = W; g->U = vec ? C / 4 : C;
    g->tiles_x = (W + UP_TW - 1) / UP_TW; g->tiles_y = (H + UP_TH - 1) / UP_TH;
    g->ublocks = (g->U + cb - 1) / cb;
    const long long wgs = (long long)N * g->tiles_x * g->tiles_y * g->ublocks;
    return wgs <= 0x7fffffffLL;
}

}  // namespace

int pesr_bilinear_up2_fwd_launch(const float* a, const float* b, float* y, int N, int H, int W, int C, hipStream_t stream) {
    if (!a || !y) return PESR_EINVAL;
    const bool vec = C % 4 == 0 && up_aligned16(a) && up_aligned16(b) && up_aligned16(y);
    UpGeom g;
    if (!up_geom(N, H, W, C, vec, UP_FWD_CB, &g)) return PESR_EINVAL;
    const dim3 grid((unsigned)((long long)N * g.tiles_x * g.tiles_y * g.ublocks)), block(UP_LANES);
    if (vec) {
        if (b) hipLaunchKernelGGL((up2_fwd_kernel<f32x4, true>), grid, block, 0, stream, (const f32x4*)a, (const f32x4*)b, (f32x4*)y, g);
        else hipLaunchKernelGGL((up2_fwd_kernel<f32x4, false>), grid, block, 0, stream, (const f32x4*)a, (const f32x4*)nullptr, (f32x4*)y, g);
    } else {
        if (b) hipLaunchKernelGGL((up2_fwd_kernel<float, true>), grid, block, 0, stream, a, b, y, g);
        else hipLaunchKernelGGL((up2_fwd_kernel<float, false>), grid, block, 0, stream, a, (const float*)nullptr, y, g);
    }
    return pesr_launch_status();
}

int pesr_bilinear_up2_bwd_launch(const float* gy, float* gx, int N, int H, int W, int C, hipStream_t stream) {
    if (!gy || !gx) return PESR_EINVAL;
    const bool vec = C % 4 == 0 && up_aligned16(gy) && up_aligned16(gx);
    UpGeom g;
    if (!up_geom(N, H, W, C, vec, UP_BWD_CB, &g)) return PESR_EINVAL;
    const dim3 grid((unsigned)((long long)N * g.tiles_x * g.tiles_y * g.ublocks)), block(UP_LANES);
    if (vec) hipLaunchKernelGGL((up2_bwd_kernel<f32x4>), grid, block, 0, stream, (const f32x4*)gy, (f32x4*)gx, g);
    else hipLaunchKernelGGL((up2_bwd_kernel<float>), grid, block, 0, stream, gy, gx, g);
    return pesr_launch_status();
}
