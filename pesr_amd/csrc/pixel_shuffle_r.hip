// nn.PixelShuffle(r) / nn.PixelUnshuffle(r) standalone for r = 2 and 3, NHWC fp32 (the x2 / x3 Upsampler of
// pesr_amd/model/basic.py; the conv kernels fuse r = 2 and do not know r = 3):
//   y[n][r*h+i][r*w+j][c] = x[n][h][w][c*r*r + i*r + j]      (torch.nn.functional.pixel_shuffle's order)
// Pure data movement, so the only goal is the HBM rate.  An input pixel's r*r*C floats are contiguous, and so are the
// r*C*TW floats that a run of TW input pixels becomes in each of its r output rows.  A workgroup therefore owns one such
// run ("tile"): it stages the run's input floats in LDS with 16-byte coalesced loads, reads the stride-r*r columns out of
// LDS and writes the r output row segments with 16-byte coalesced stores.  The backward (pixel unshuffle) is the mirror
// image: 16-byte row loads, stride-r*r scatter into LDS, 16-byte stores of the contiguous input-gradient run.
//
// LDS banking (ds_read_b32 / ds_write_b32: bank (a/4) % 32 per 32-lane half): a lane moves four consecutive channels c..c+3
// of one output pixel, i.e. four dwords at stride r*r, and neighbouring lanes are 4*r*r dwords apart.  For r = 3 that is 36
// = 4 (mod 32), so lanes l and l+8 would meet on a bank; each group of eight lanes therefore visits the four channels in
// an order rotated by (lane / 8) % 4, which makes every ds_read_b32 / ds_write_b32 of a 32-lane half hit 32 distinct banks
// when C % 32 == 0.  (r = 2: 16 dwords apart, the rotation leaves a 4-way conflict; r = 2 runs on the conv-fused path.)
//
// C % 4 != 0, or a single pixel too wide for the LDS budget: a plain gather per element (coalesced on the written side).
// All offsets are 64-bit (the x3 upsampler of a [4,3,512,512] batch has 2.4e9 elements); no allocation, no host sync.
#include "common.h"
#include "launchers.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsBudget = 40 * 1024;     // bytes per workgroup: four workgroups per CU (160 KiB)

template <int R>
__device__ __forceinline__ int rot_group(int tid) { return R == 3 ? (tid >> 3) & 3 : (tid >> 1) & 3; }

// r*r*C floats per input pixel, tiles of TW input pixels along W; one workgroup per tile (grid-stride over tiles)
template <int R, bool INVERSE>
__global__ __launch_bounds__(kThreads) void pixel_shuffle_r_tiled_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                         int H, int W, int C, int TW, int ntw, long tiles) {
    extern __shared__ float lds[];
    constexpr int RR = R * R;
    const long pix = (long)RR * C;                 // floats per input pixel
    const int tid = threadIdx.x;
    const int q = rot_group<R>(tid);
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tw_i = (int)(t % ntw);
        const long nh = t / ntw;                   // n * H + h
        const int h = (int)(nh % H);
        const long n = nh / H;
        const int w0 = tw_i * TW;
        const int tw = min(TW, W - w0);
        const long xbase = (nh * W + w0) * pix;                      // the tile's contiguous input run
        const long n4x = (long)tw * pix / 4;                         // its float4 count
        const int seg4 = tw * R * C / 4;                             // float4 per output row segment
        __syncthreads();                                             // the previous tile's LDS reads are done
        if (!INVERSE) {
            const f32x4* x4 = reinterpret_cast<const f32x4*>(src + xbase);
            f32x4* l4 = reinterpret_cast<f32x4*>(lds);
            for (long e = tid; e < n4x; e += kThreads) l4[e] = x4[e];
            __syncthreads();
        }
        for (int i = 0; i < R; ++i) {
            const long ybase = ((n * H * R + (long)h * R + i) * W * R + (long)w0 * R) * C;
            for (int e = tid; e < seg4; e += kThreads) {
                const int o = 4 * e;
                const int X = o / C, c = o - X * C;
                const int wl = X / R, j = X - wl * R;
                const int base = wl * (int)pix + c * RR + i * R + j;   // < TW * r*r*C <= kLdsBudget / 4
                if (!INVERSE) {
                    float a[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) a[s] = lds[base + ((s + q) & 3) * RR];
                    f32x4 v;                                           // un-rotate: a[s] holds channel (s + q) & 3
                    v.x = q == 0 ? a[0] : q == 1 ? a[3] : q == 2 ? a[2] : a[1];
                    v.y = q == 0 ? a[1] : q == 1 ? a[0] : q == 2 ? a[3] : a[2];
                    v.z = q == 0 ? a[2] : q == 1 ? a[1] : q == 2 ? a[0] : a[3];
                    v.w = q == 0 ? a[3] : q == 1 ? a[2] : q == 2 ? a[1] : a[0];
                    reinterpret_cast<f32x4*>(dst + ybase)[e] = v;
                } else {
                    const f32x4 v = reinterpret_cast<const f32x4*>(src + ybase)[e];
                    const float b[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int m = (s + q) & 3;
                        lds[base + m * RR] = m == 0 ? b[0] : m == 1 ? b[1] : m == 2 ? b[2] : b[3];
                    }
                }
            }
        }
        if (INVERSE) {
            __syncthreads();
            f32x4* d4 = reinterpret_cast<f32x4*>(dst + xbase);
            const f32x4* l4 = reinterpret_cast<const f32x4*>(lds);
            for (long e = tid; e < n4x; e += kThreads) d4[e] = l4[e];
        }
    }
}

// any C: one thread per element of the written tensor, gathering from the other one
template <bool INVERSE>
__global__ __launch_bounds__(kThreads) void pixel_shuffle_r_gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                          int H, int W, int C, int R, long total) {
    const int RR = R * R;
    for (long e = (long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long)gridDim.x * kThreads) {
        long small, big;                 // offsets in the [N][H][W][r*r*C] and the [N][rH][rW][C] tensors
        if (!INVERSE) {                  // e walks y
            big = e;
            const int c = (int)(e % C);
            long rest = e / C;
            const int X = (int)(rest % ((long)R * W)); rest /= (long)R * W;
            const int Y = (int)(rest % ((long)R * H));
            const long n = rest / ((long)R * H);
            small = ((n * H + Y / R) * W + X / R) * RR * C + (long)c * RR + (Y % R) * R + (X % R);
            dst[big] = src[small];
        } else {                         // e walks dx
            small = e;
            const int k = (int)(e % ((long)RR * C));
            long rest = e / ((long)RR * C);
            const int w = (int)(rest % W); rest /= W;
            const int h = (int)(rest % H);
            const long n = rest / H;
            const int c = k / RR, ij = k - c * RR, i = ij / R, j = ij - i * R;
            big = ((n * H * R + (long)h * R + i) * W * R + (long)w * R + j) * C + c;
            dst[small] = src[big];
        }
    }
}

template <int R, bool INVERSE>
int launch_tiled(const float* src, float* dst, int N, int H, int W, int C, int TW, hipStream_t stream) {
    const int ntw = (W + TW - 1) / TW;
    const long tiles = (long)N * H * ntw;
    const int grid = (int)(tiles < (1L << 30) ? tiles : (1L << 30));
    const size_t lds = (size_t)TW * R * R * C * sizeof(float);
    hipLaunchKernelGGL((pixel_shuffle_r_tiled_kernel<R, INVERSE>), dim3(grid), dim3(kThreads), lds, stream, src, dst, H, W, C, TW,
                       ntw, tiles);
    return pesr_launch_status();
}

}  // namespace

int pesr_pixel_shuffle_r_launch(const float* in, float* out, int N, int H, int W, int C, int r, int inverse, hipStream_t stream) {
    if (!in || !out || N < 1 || H < 1 || W < 1 || C < 1 || (r != 2 && r != 3)) return PESR_EINVAL;
    const long pix_bytes = (long)r * r * C * (long)sizeof(float);
    const uintptr_t align = (uintptr_t)in | (uintptr_t)out;
    if (C % 4 == 0 && pix_bytes <= kLdsBudget && (align & 15) == 0) {
        // tile width: as many input pixels as the LDS budget holds, spread evenly over the row
        const int tw_max = (int)(kLdsBudget / pix_bytes) < W ? (int)(kLdsBudget / pix_bytes) : W;
        const int ntw = (W + tw_max - 1) / tw_max;
        const int TW = (W + ntw - 1) / ntw;
        if (r == 2) return inverse ? launch_tiled<2, true>(in, out, N, H, W, C, TW, stream)
                                   : launch_tiled<2, false>(in, out, N, H, W, C, TW, stream);
        return inverse ? launch_tiled<3, true>(in, out, N, H, W, C, TW, stream)
                       : launch_tiled<3, false>(in, out, N, H, W, C, TW, stream);
    }
    const long total = (long)N * H * W * r * r * C;
    const long blocks = (total + kThreads - 1) / kThreads;
    const int grid = (int)(blocks < (1L << 30) ? blocks : (1L << 30));
    if (inverse)
        hipLaunchKernelGGL(pixel_shuffle_r_gather_kernel<true>, dim3(grid), dim3(kThreads), 0, stream, in, out, H, W, C, r, total);
    else
        hipLaunchKernelGGL(pixel_shuffle_r_gather_kernel<false>, dim3(grid), dim3(kThreads), 0, stream, in, out, H, W, C, r, total);
    return pesr_launch_status();
}
