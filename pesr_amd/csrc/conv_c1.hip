// 3 x 3 conv (pad 1, stride 1) from C channels to ONE: the logit layer of the U-Net discriminator (docs/modes.md section 4v).  The
// implicit-GEMM kernels pad the "n" side to sixteen channels and refuse a one-channel tensor on their input-gradient and
// weight-gradient sides, and the layer is HBM-bound anyway (at [16, 192, 192, 64] it reads 151 MB to write 2.4 MB), so it has three
// small streaming kernels of its own on the un-packed OIHW weights w [1][C][3][3], in the manner of conv_rgb_out.hip / rgb_wgrad.hip.
// x, dx: NHWC [N][H][W][C], C % 4 == 0, 4 <= C <= 1024, 16-byte aligned;  y, dy: [N][H][W] (one channel).
//   forward   p[i][t] = sum_c x[i][c] w[c][t] for every pixel i of a 16 x 16 tile and its halo (sixteen lanes per pixel, a lane's
//             channels in increasing order, then a fixed xor tree), kept in LDS;  y[o] = bias + sum_t p[o + d_t][t], t increasing.
//             Each input pixel is read once per tile.
//   dgrad     dx[i][c] = sum_t dy[i - d_t] w[c][t], t increasing: one 16-byte store per lane.
//   wgrad     dw[c][t] = alpha sum_i x[i][c] dy[i - d_t], db = alpha sum_i dy[i]: one workgroup per chunk of pixels leaves a row
//             [9][C] + db in the workspace (a lane owns four channels and every rows-th pixel, in increasing order; the row lanes meet
//             in LDS in increasing order), reduce_rows.h's second stage adds the rows in double.
// No atomics, every sum in an order that depends on the shape alone; size_t element offsets.
#include "common.h"
#include "launchers.h"
#include "reduce_rows.h"

#define C1_LANES 256
#define C1_MAX_C 1024
#define C1_T 16                    // forward tile: 16 x 16 output pixels
#define C1_HALO (C1_T + 2)

namespace {

bool c1_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool c1_shape_ok(int N, int H, int W, int C) {
    return N >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && C <= C1_MAX_C && (long long)N * H * W <= 0x7fffffffLL;
}

__global__ __launch_bounds__(C1_LANES) void conv_c1_fwd_kernel(const f32x4* __restrict__ x, const float* __restrict__ w,
                                                               const float* __restrict__ bias, float* __restrict__ y, int H, int W, int C4,
                                                               int tiles_x, int tiles_y) {
    extern __shared__ f32x4 sw[];                        // [t][c4]: 9 * C4 vectors, sized by the launch
    __shared__ float sp[C1_HALO * C1_HALO * 9];          // [halo pixel][t]
    int bid = blockIdx.x;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int n = bid / tiles_y;
    const int y0 = ty * C1_T - 1, x0 = tx * C1_T - 1;    // image coordinates of halo pixel (0, 0)
    for (int e = threadIdx.x; e < 9 * C4; e += C1_LANES) {
        const int t = e / C4, c4 = e - t * C4;
        const float* wc = w + (size_t)c4 * 36 + t;       // w[c][t] at c * 9 + t
        const f32x4 v = {wc[0], wc[9], wc[18], wc[27]};
        sw[e] = v;
    }
    __syncthreads();
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;          // sixteen lanes per pixel, sixteen pixels at a time
    const size_t img = (size_t)n * H * W * C4;
    for (int p = grp; p < C1_HALO * C1_HALO; p += C1_LANES / 16) {
        const int iy = y0 + p / C1_HALO, ix = x0 + p % C1_HALO;
        float acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            const f32x4* px = x + img + ((size_t)iy * W + ix) * C4;
            for (int c4 = sub; c4 < C4; c4 += 16) {
                const f32x4 v = px[c4];
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const f32x4 k = sw[t * C4 + c4];
                    acc[t] = fmaf(v.w, k.w, fmaf(v.z, k.z, fmaf(v.y, k.y, fmaf(v.x, k.x, acc[t]))));
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) acc[t] += __shfl_xor(acc[t], off, 16);
        }
        if (sub < 9) {
            float v = acc[0];
#pragma unroll
            for (int t = 1; t < 9; ++t) v = sub == t ? acc[t] : v;
            sp[p * 9 + sub] = v;
        }
    }
    __syncthreads();
    const int oy = threadIdx.x / C1_T, ox = threadIdx.x % C1_T;
    const int gy = ty * C1_T + oy, gx = tx * C1_T + ox;
    if (gy < H && gx < W) {
        float s = bias ? bias[0] : 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) s += sp[((oy + t / 3) * C1_HALO + ox + t % 3) * 9 + t];
        y[((size_t)n * H + gy) * W + gx] = s;
    }
}

__global__ __launch_bounds__(C1_LANES) void conv_c1_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                 f32x4* __restrict__ dx, int H, int W, int C4, long pixels) {
    extern __shared__ f32x4 sw[];                        // [t][c4]: 9 * C4 vectors, sized by the launch
    for (int e = threadIdx.x; e < 9 * C4; e += C1_LANES) {
        const int t = e / C4, c4 = e - t * C4;
        const float* wc = w + (size_t)c4 * 36 + t;
        const f32x4 v = {wc[0], wc[9], wc[18], wc[27]};
        sw[e] = v;
    }
    __syncthreads();
    const int cols = C4 < C1_LANES ? C4 : C1_LANES, rows = C1_LANES / cols;
    const int r = threadIdx.x / cols, cl = threadIdx.x - r * cols;
    if (r >= rows) return;
    for (long p = (long)blockIdx.x * rows + r; p < pixels; p += (long)gridDim.x * rows) {
        const int ix = (int)(p % W), iy = (int)((p / W) % H);
        float g[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {                    // dx[i] takes dy[i - d_t], d_t = (t / 3 - 1, t % 3 - 1)
            const int qy = iy - (t / 3 - 1), qx = ix - (t % 3 - 1);
            g[t] = (qy >= 0 && qy < H && qx >= 0 && qx < W) ? dy[p - (long)(t / 3 - 1) * W - (t % 3 - 1)] : 0.f;
        }
        for (int c4 = cl; c4 < C4; c4 += cols) {
            f32x4 acc = sw[c4] * g[0];
#pragma unroll
            for (int t = 1; t < 9; ++t) acc += sw[t * C4 + c4] * g[t];
            dx[(size_t)p * C4 + c4] = acc;
        }
    }
}

// Pixels per chunk of the weight gradient: about 1024 workgroups, at least 32 pixels per row lane.
struct C1Wg { int cols, rows, chunks; long P; };
C1Wg c1_wg(long pixels, int C) {
    C1Wg g;
    g.cols = C / 4 < C1_LANES ? C / 4 : C1_LANES;
    g.rows = C1_LANES / g.cols;
    const long even = (pixels + 1023) / 1024, floor_ = 32L * g.rows;
    g.P = even > floor_ ? even : floor_;
    g.chunks = (int)((pixels + g.P - 1) / g.P);
    return g;
}

__global__ __launch_bounds__(C1_LANES) void conv_c1_wgrad_kernel(const f32x4* __restrict__ x, const float* __restrict__ dy,
                                                                 float* __restrict__ part, int H, int W, int C4, long pixels, long P,
                                                                 int cols, int rows, int ncols) {
    __shared__ f32x4 red[C1_LANES];
    __shared__ float redb[C1_LANES];
    const int r = threadIdx.x / cols, cl = threadIdx.x - r * cols;
    const long p0 = (long)blockIdx.x * P, p1 = p0 + P < pixels ? p0 + P : pixels;
    float* row = part + (size_t)blockIdx.x * ncols;
    for (int c0 = 0; c0 < C4; c0 += cols) {
        const int c4 = c0 + cl;
        const bool live = r < rows && c4 < C4;
        f32x4 acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        float gsum = 0.f;
        if (live) {
            for (long p = p0 + r; p < p1; p += rows) {
                const int ix = (int)(p % W), iy = (int)((p / W) % H);
                const f32x4 v = x[(size_t)p * C4 + c4];
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int qy = iy - (t / 3 - 1), qx = ix - (t % 3 - 1);
                    const float g = (qy >= 0 && qy < H && qx >= 0 && qx < W) ? dy[p - (long)(t / 3 - 1) * W - (t % 3 - 1)] : 0.f;
                    acc[t] += v * g;
                }
                gsum += dy[p];
            }
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            __syncthreads();                             // (red may still be read for the previous tap)
            red[threadIdx.x] = acc[t];
            __syncthreads();
            if (live && r == 0) {
                f32x4 s = red[cl];
                for (int k = 1; k < rows; ++k) s += red[k * cols + cl];
                *(f32x4*)(row + (size_t)t * C4 * 4 + c4 * 4) = s;
            }
        }
        if (c0 == 0) {                                   // db: the lanes of column 0, one per row lane
            __syncthreads();
            redb[threadIdx.x] = gsum;
            __syncthreads();
            if (threadIdx.x == 0) {
                float s = redb[0];
                for (int k = 1; k < rows; ++k) s += redb[k * cols];
                row[9 * C4 * 4] = s;
            }
        }
    }
}

// second stage: column t * C + c of the rows -> dw[c * 9 + t]; column 9 C -> db (a row is 9 C + 4 floats: 16-byte rows)
__global__ __launch_bounds__(1024) void conv_c1_wgrad_final_kernel(const float* __restrict__ part, int nb, int ncols, int C, float alpha,
                                                                   float* __restrict__ dw, float* __restrict__ db) {
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + cl;
    __shared__ double red[16][64];
    const double s = reduce_rows_block(part, nb, ncols, col, col <= 9 * C, red);
    if (rl == 0 && col <= 9 * C) {
        const float v = (float)(s * (double)alpha);
        if (col < 9 * C) dw[(col % C) * 9 + col / C] = v;
        else if (db) db[0] = v;
    }
}

}  // namespace

size_t pesr_conv3x3_c1_wgrad_ws_bytes(int N, int H, int W, int C) {
    if (!c1_shape_ok(N, H, W, C)) return 0;
    return (size_t)c1_wg((long)N * H * W, C).chunks * (9 * C + 4) * sizeof(float);
}

int pesr_conv3x3_c1_fwd_launch(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int C, hipStream_t stream) {
    if (!c1_shape_ok(N, H, W, C) || !x || !w || !y || !c1_aligned16(x)) return PESR_EINVAL;
    const int tiles_x = (W + C1_T - 1) / C1_T, tiles_y = (H + C1_T - 1) / C1_T;
    if ((long long)N * tiles_x * tiles_y > 0x7fffffffLL) return PESR_EINVAL;
    hipLaunchKernelGGL(conv_c1_fwd_kernel, dim3((unsigned)(N * tiles_x * tiles_y)), dim3(C1_LANES), (size_t)9 * C * sizeof(float), stream, (const f32x4*)x, w, bias, y, H,
                       W, C / 4, tiles_x, tiles_y);
    return pesr_launch_status();
}

int pesr_conv3x3_c1_dgrad_launch(const float* dy, const float* w, float* dx, int N, int H, int W, int C, hipStream_t stream) {
    if (!c1_shape_ok(N, H, W, C) || !dy || !w || !dx || !c1_aligned16(dx)) return PESR_EINVAL;
    const long pixels = (long)N * H * W;
    const int rows = C1_LANES / (C / 4 < C1_LANES ? C / 4 : C1_LANES);
    const long want = (pixels + rows - 1) / rows;
    hipLaunchKernelGGL(conv_c1_dgrad_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(C1_LANES), (size_t)9 * C * sizeof(float), stream, dy, w, (f32x4*)dx, H, W,
                       C / 4, pixels);
    return pesr_launch_status();
}

int pesr_conv3x3_c1_wgrad_launch(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int C, float alpha, void* ws,
                                 size_t ws_bytes, hipStream_t stream) {
    if (!c1_shape_ok(N, H, W, C) || !x || !dy || !dw || !c1_aligned16(x) || !c1_aligned16(ws)) return PESR_EINVAL;
    if (!ws || ws_bytes < pesr_conv3x3_c1_wgrad_ws_bytes(N, H, W, C)) return PESR_EWORKSPACE;
    const long pixels = (long)N * H * W;
    const C1Wg g = c1_wg(pixels, C);
    const int ncols = 9 * C + 4;
    hipLaunchKernelGGL(conv_c1_wgrad_kernel, dim3(g.chunks), dim3(C1_LANES), 0, stream, (const f32x4*)x, dy, (float*)ws, H, W, C / 4, pixels,
                       g.P, g.cols, g.rows, ncols);
    hipLaunchKernelGGL(conv_c1_wgrad_final_kernel, dim3((ncols + 63) / 64), dim3(1024), 0, stream, (const float*)ws, g.chunks, ncols, C, alpha,
                       dw, db);
    return pesr_launch_status();
}
