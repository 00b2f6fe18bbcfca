// The backward of the upsampler's tail - conv C -> 4C, PixelShuffle(2), conv C -> 3 (reference model/basic.py:56-60), nothing
// non-linear in between - as the backward of ONE virtual 3x3 conv V from C to 48 (padded to 64) channels at the resolution of the
// tail's input h [N][H][W][C].  With g = dL/d(output) [N][2H][2W][3], W2 [4C][C][3][3], b2 [4C], W4 [3][C][3][3]:
//   gather    Gw[n][y][x][z = (k*4+p)*4+q] = g[n][2y-1+p][2x-1+q][k]   (k < 3, p, q < 4; 0 outside the image; channels 48..63 zero):
//             the 4 x 4 window of the HR gradient that one pixel of h reaches through the pair;
//   compose   Weff[z][ci][e][f] = sum_m A[m][z] W2[m][ci][e][f],  A[m = 4c+2i+j][z] = W4[k][c][i+2-p][j+2-q] where both taps lie in 0..2;
//   (the two heavy launches - dh = input gradient of V on Gw, S [64][C][3][3] / T [64] = its weight / bias gradient from (h, Gw) -
//   run on the library's 3x3 conv kernels)
//   chain     dW2[m] = sum_z A[m][z] S[z],  db2 = A T,
//             dW4[k][c][a][b] = sum_{i,j} ( <W2[m], S[z]> + b2[m] T[z] ),  m = 4c+2i+j, z = (k*4 + i+2-a)*4 + j+2-b,
//             db4[k] = T[k,1,1] + T[k,1,2] + T[k,2,1] + T[k,2,2]        (the four window positions that tile the HR image).
// V's zero padding over H x W is exactly "g exists only inside the image", so the borders need no special case.
// The compose and chain sums run in double, in one fixed order (no atomics), and are rounded once.
#include "common.h"
#include "launchers.h"

// One thread per (pixel, 4 window columns): 12 threads of a pixel read a row of 4 HR gradients of one colour (the loads of a thread are
// independent of each other), 4 write the zero channels; every thread stores 16 bytes.
__global__ void upsample_tail_gather_kernel(const float* __restrict__ g, float* __restrict__ gw, int N, int H, int W) {
    const long total = (long)N * H * W * 16;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int t = (int)(e & 15);
        const long pix = e >> 4;
        const int x = (int)(pix % W);
        const long rest = pix / W;
        const int y = (int)(rest % H);
        const long n = rest / H;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int k = t >> 2, gy = 2 * y - 1 + (t & 3);
        if (t < 12 && gy >= 0 && gy < 2 * H) {
            const float* row = g + ((n * 2 * H + gy) * (2L * W)) * 3 + k;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gx = 2 * x - 1 + q;
                v[q] = (gx >= 0 && gx < 2 * W) ? row[(long)gx * 3] : 0.f;
            }
        }
        *(f32x4*)(gw + e * 4) = v;
    }
}

// 64 outputs per workgroup, the sum over c of each split over the 4 waves (a quarter of the channels each, 4 channels = 16 loads of W2 in
// flight per lane); the four partial sums are added in wave order.  Of the four sub-pixels (i, j) of a channel c only those whose taps lie
// inside W4's 3 x 3 kernel count; the others are loaded like them (a regular, batched loop) and take the coefficient 0.
__global__ __launch_bounds__(256) void upsample_tail_compose_kernel(const float* __restrict__ w2, const float* __restrict__ w4,
                                                                    float* __restrict__ weff, int C) {
    __shared__ double part[3][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const long K = 9L * C;                                  // elements of one output channel's row [C][3][3]
    const long o = (long)blockIdx.x * 64 + lane;            // < 64 K: the grid is K workgroups
    const bool live = o < 48 * K;                           // rows 48..63 are zero
    double acc = 0.0;
    if (live) {
        const int z = (int)(o / K);
        const long r = o - z * K;
        const int k = z >> 4, p = (z >> 2) & 3, q = z & 3;
        int off[4];
        bool ok[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int a = (s >> 1) + 2 - p, b = (s & 1) + 2 - q;
            ok[s] = a >= 0 && a <= 2 && b >= 0 && b <= 2;
            off[s] = ok[s] ? a * 3 + b : 0;
        }
        const float* w4k = w4 + (long)k * K;
        const int c0 = slice * (C >> 2), c1 = c0 + (C >> 2);      // C % 16 == 0: a multiple of 4 channels per wave
        for (int c = c0; c < c1; c += 4) {
            float cf[4][4], wv[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    cf[u][s] = w4k[(c + u) * 9 + off[s]];
                    wv[u][s] = w2[(4L * (c + u) + s) * K + r];
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = fma((double)(ok[s] ? cf[u][s] : 0.f), (double)wv[u][s], acc);
        }
    }
    if (slice) part[slice - 1][lane] = acc;
    __syncthreads();
    if (slice == 0) weff[o] = live ? (float)(((acc + part[0][lane]) + part[1][lane]) + part[2][lane]) : 0.f;
}

// dW2 and db2: one thread per element, 27 terms in the order (k, a, b).  Column K of a row m is the bias: the same sum over T.
__global__ void upsample_tail_dw2_kernel(const float* __restrict__ w4, const float* __restrict__ S, const float* __restrict__ T,
                                         float* __restrict__ dw2, float* __restrict__ db2, int C, int accumulate) {
    const long K = 9L * C, total = 4L * C * (K + 1);
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long m = e / (K + 1), r = e - m * (K + 1);
        const bool bias = r == K;
        float* const dst = bias ? (db2 ? db2 + m : nullptr) : (dw2 ? dw2 + m * K + r : nullptr);
        if (!dst) continue;
        const int c = (int)(m >> 2), i = (int)(m >> 1) & 1, j = (int)m & 1;
        const float* src = bias ? T : S + r;
        const long zs = bias ? 1 : K;
        float cf[27], sv[27];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    cf[(k * 3 + a) * 3 + b] = w4[((long)k * C + c) * 9 + a * 3 + b];
                    sv[(k * 3 + a) * 3 + b] = src[((k * 4 + i + 2 - a) * 4 + j + 2 - b) * zs];
                }
        double acc = accumulate ? (double)*dst : 0.0;
#pragma unroll
        for (int t = 0; t < 27; ++t) acc = fma((double)cf[t], (double)sv[t], acc);
        *dst = (float)acc;
    }
}

// dW4: one wave per element (four dot products of length K, 8 loads in flight per lane, the wave's sum by a fixed butterfly); the three
// elements behind them are db4.
__global__ __launch_bounds__(256) void upsample_tail_dw4_kernel(const float* __restrict__ w2, const float* __restrict__ b2,
                                                                const float* __restrict__ S, const float* __restrict__ T,
                                                                float* __restrict__ dw4, float* __restrict__ db4, int C, int accumulate) {
    const int lane = threadIdx.x & 63;
    const long K = 9L * C, n4 = 27L * C;
    const long out = (long)blockIdx.x * 4 + (threadIdx.x >> 6);        // the same in every lane of a wave
    if (out >= n4) {
        const int k = (int)(out - n4);
        if (k < 3 && db4 && lane == 0) {
            const double s = (((double)T[(k * 4 + 1) * 4 + 1] + (double)T[(k * 4 + 1) * 4 + 2]) + (double)T[(k * 4 + 2) * 4 + 1]) +
                             (double)T[(k * 4 + 2) * 4 + 2];
            db4[k] = (float)(accumulate ? (double)db4[k] + s : s);
        }
        return;
    }
    if (!dw4) return;
    const int b = (int)(out % 3), a = (int)(out / 3 % 3), c = (int)(out / 9 % C), k = (int)(out / K);
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const long m = 4L * c + s;
        const int z = (k * 4 + (s >> 1) + 2 - a) * 4 + (s & 1) + 2 - b;
        const float* wr = w2 + m * K;
        const float* sr = S + z * K;
        for (long r = lane; r < K; r += 256) {
            float wv[4], sv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long rr = r + 64 * u;
                wv[u] = rr < K ? wr[rr] : 0.f;
                sv[u] = rr < K ? sr[rr] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = fma((double)wv[u], (double)sv[u], acc);
        }
    }
    acc = wave_sum_d(acc);
    if (lane == 0) {
        if (b2)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc = fma((double)b2[4L * c + s], (double)T[(k * 4 + (s >> 1) + 2 - a) * 4 + (s & 1) + 2 - b], acc);
        dw4[out] = (float)(accumulate ? (double)dw4[out] + acc : acc);
    }
}

static inline int tail_grid(long threads) {
    const long g = (threads + 255) / 256;
    return (int)(g < 8192 ? g : 8192);
}

int pesr_upsample_tail_gather_launch(const float* g, float* gw, int N, int H, int W, hipStream_t stream) {
    if (!g || !gw || N < 1 || H < 1 || W < 1 || ((uintptr_t)gw & 15)) return PESR_EINVAL;
    hipLaunchKernelGGL(upsample_tail_gather_kernel, dim3(tail_grid((long)N * H * W * 16)), dim3(256), 0, stream, g, gw, N, H, W);
    return pesr_launch_status();
}

int pesr_upsample_tail_compose_launch(const float* w2, const float* w4, float* weff, int C, hipStream_t stream) {
    if (!w2 || !w4 || !weff || C < 16 || C % 16 || C > 4096) return PESR_EINVAL;
    hipLaunchKernelGGL(upsample_tail_compose_kernel, dim3(9 * C), dim3(256), 0, stream, w2, w4, weff, C);
    return pesr_launch_status();
}

int pesr_upsample_tail_chain_launch(const float* w2, const float* b2, const float* w4, const float* S, const float* T, float* dw2,
                                    float* db2, float* dw4, float* db4, int C, int accumulate, hipStream_t stream) {
    if (!w2 || !w4 || !S || !T || C < 16 || C % 16 || C > 4096) return PESR_EINVAL;
    if (dw2 || db2) {
        hipLaunchKernelGGL(upsample_tail_dw2_kernel, dim3(tail_grid(4L * C * (9L * C + 1))), dim3(256), 0, stream, w4, S, T, dw2, db2, C,
                           accumulate);
        const int rc = pesr_launch_status();
        if (rc) return rc;
    }
    if (dw4 || db4)
        hipLaunchKernelGGL(upsample_tail_dw4_kernel, dim3((27 * C + 3 + 3) / 4), dim3(256), 0, stream, w2, b2, S, T, dw4, db4, C, accumulate);
    return pesr_launch_status();
}
