// Channel attention of a residual block (RCAN's RCAB, Zhang et al. ECCV 2018; docs/modes.md section 4u), NHWC fp32:
//   m[n][c] = (1/HW) sum_p t[n][p][c]                    squeeze (global average pool)
//   h[n][j] = relu(sum_c W1[j][c] m[n][c] + B1[j])       j < R
//   s[n][c] = sigmoid(sum_j W2[c][j] h[n][j] + B2[c])    excite
//   y       = x + a * t * s[n][c]
// and its backward (gx = gy is the caller's):
//   ds[n][c] = a sum_p gy * t  ->  through the sigmoid, W2, the ReLU and W1  ->  dm, dW1, dB1, dW2, dB2;   gt = a * gy * s + dm / HW
//
// Four streaming kernels (the two pixel sums, the two apply passes) and three small ones (the gate, forward and backward).  The
// streaming kernels share one geometry: an image's HW pixels are cut into chunks of ca_chunk_pixels() pixels, one 256-lane workgroup
// per (image, chunk); a lane owns four channels (one 16-byte access per pixel) and every (256 / (C/4))-th pixel of the chunk, so what
// it needs per channel (s, dm) sits in registers.  The sums leave one fp32 row per chunk in the caller's workspace, which
// reduce_rows.h's fixed-order second stage adds in double: no atomics, the same bits on every call.  Element offsets are size_t
// (config 5's [4][512][512][256] tensor is 2^28 elements, 2^30 bytes).
#include "common.h"
#include "launchers.h"
#include "reduce_rows.h"

#define CA_LANES 256
#define CA_GATE_LANES 1024   // the gate kernels: sixteen waves, so that the hidden units' reductions (latency chains) run side by side
#define CA_MAX_C 2048

// Host: the chunk rule.  cols: 16-byte columns a workgroup covers at once; rows: pixels it reads at once.
static inline int ca_cols(int C) { return C / 4 < CA_LANES ? C / 4 : CA_LANES; }
static inline int ca_rows(int C) { return CA_LANES / ca_cols(C); }
static bool ca_shape_ok(int N, long HW, int C) { return N >= 1 && HW >= 1 && C >= 4 && C % 4 == 0 && C <= CA_MAX_C && HW <= (1L << 30); }
// Pixels per chunk: at least eight per lane (eight independent 16-byte loads), and no more than about 2048 workgroups in all - eight
// per CU - whether these are sixteen training patches of 2304 pixels (72 chunks each) or one 512 x 512 image (2048 chunks).
static long ca_chunk_pixels(int N, long HW, int C) {
    const long per_image = 2048 / N > 1 ? 2048 / N : 1;
    const long even = (HW + per_image - 1) / per_image, floor_ = 8L * ca_rows(C);
    return even > floor_ ? even : floor_;
}
int pesr_ca_pool_partials_of(int N, long HW, int C) {
    if (!ca_shape_ok(N, HW, C)) return 0;
    const long P = ca_chunk_pixels(N, HW, C);
    const long chunks = (HW + P - 1) / P;
    return chunks * N > 0x7fffffffL ? 0 : (int)chunks;
}
// The larger of: the partial rows of a pixel sum [chunks][N * C]; the gate backward's two pre-activation gradients [N][C] + [N][R].
size_t pesr_ca_ws_bytes(int N, long HW, int C, int R) {
    const int chunks = pesr_ca_pool_partials_of(N, HW, C);
    if (chunks < 1 || R < 1 || R > C) return 0;
    const size_t a = (size_t)chunks * N * C * sizeof(float), b = (size_t)N * ((size_t)C + R) * sizeof(float);
    return a > b ? a : b;
}

struct CaGeom {
    int cols, rows;      // of a workgroup: 16-byte columns x pixels
    int C4;              // C / 4
    int chunks;          // per image
    long P, HW;          // pixels per chunk, per image
};

// ---- pixel sums, first stage: part[chunk][n * C + c] = sum over the chunk's pixels of t (PROD: of gy * t) ---------------------------
// A lane adds its pixels in increasing order in fp32 (PROD: one fused multiply-add per pixel, the product is not rounded on its own),
// the row lanes meet through LDS and are added in increasing order.
template <bool PROD>
__global__ __launch_bounds__(CA_LANES) void ca_sum_kernel(const f32x4* __restrict__ t, const f32x4* __restrict__ gy,
                                                          f32x4* __restrict__ part, CaGeom g, int N) {
    __shared__ f32x4 red[CA_LANES];
    const int n = blockIdx.x / g.chunks, chunk = blockIdx.x - n * g.chunks;
    const int r = threadIdx.x / g.cols, cl = threadIdx.x - r * g.cols;
    const long p0 = (long)chunk * g.P, p1 = p0 + g.P < g.HW ? p0 + g.P : g.HW;
    const size_t image = (size_t)n * (size_t)g.HW * g.C4;
    for (int c0 = 0; c0 < g.C4; c0 += g.cols) {
        const int c = c0 + cl;
        const bool live = r < g.rows && c < g.C4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            const f32x4* tp = t + image + c;
            const f32x4* gp = PROD ? gy + image + c : nullptr;
            long p = p0 + r;
            for (; p + 3L * g.rows < p1; p += 4L * g.rows) {     // four (PROD: eight) independent loads in flight
                f32x4 v[4], w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    v[u] = tp[(size_t)(p + (long)u * g.rows) * g.C4];
                    if (PROD) w[u] = gp[(size_t)(p + (long)u * g.rows) * g.C4];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (PROD) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[k] = fmaf(w[u][k], v[u][k], acc[k]);
                    } else {
                        acc += v[u];
                    }
                }
            }
            for (; p < p1; p += g.rows) {
                const f32x4 v = tp[(size_t)p * g.C4];
                if (PROD) {
                    const f32x4 w = gp[(size_t)p * g.C4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = fmaf(w[k], v[k], acc[k]);
                } else {
                    acc += v;
                }
            }
        }
        __syncthreads();                                         // (red may still be read for the previous column tile)
        red[threadIdx.x] = acc;
        __syncthreads();
        if (live && r == 0) {
            f32x4 s = red[cl];
            for (int k = 1; k < g.rows; ++k) s += red[k * g.cols + cl];
            part[((size_t)chunk * N + n) * g.C4 + c] = s;
        }
    }
}

// ---- pixel sums, second stage: out[col] = (float)(scale * sum_k part[k][col]), reduce_rows.h's order, in double ---------------------
__global__ __launch_bounds__(1024) void ca_sum_final_kernel(const float* __restrict__ part, float* __restrict__ out, int nb, int ncols,
                                                            double scale) {
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + cl;
    __shared__ double red[16][64];
    const double s = reduce_rows_block(part, nb, ncols, col, col < ncols, red);
    if (rl == 0 && col < ncols) out[col] = (float)(s * scale);
}

// ---- apply: out = in * (a * s[n][c]) + add,  add = x (forward: y = x + a t s) or dm[n][c] / HW (backward: gt = a gy s + dm / HW) ----
template <bool BWD>
__global__ __launch_bounds__(CA_LANES) void ca_apply_kernel(const f32x4* __restrict__ in, const f32x4* __restrict__ x,
                                                            const f32x4* __restrict__ s, const f32x4* __restrict__ dm,
                                                            f32x4* __restrict__ out, CaGeom g, float a, float inv_hw) {
    const int n = blockIdx.x / g.chunks, chunk = blockIdx.x - n * g.chunks;
    const int r = threadIdx.x / g.cols, cl = threadIdx.x - r * g.cols;
    if (r >= g.rows) return;
    const long p0 = (long)chunk * g.P, p1 = p0 + g.P < g.HW ? p0 + g.P : g.HW;
    const size_t image = (size_t)n * (size_t)g.HW * g.C4;
    for (int c = cl; c < g.C4; c += g.cols) {
        const f32x4 k = s[(size_t)n * g.C4 + c] * a;
        f32x4 add = {0.f, 0.f, 0.f, 0.f};
        if (BWD) add = dm[(size_t)n * g.C4 + c] * inv_hw;
        const size_t base = image + c;
        long p = p0 + r;
        for (; p + 3L * g.rows < p1; p += 4L * g.rows) {
            f32x4 v[4], w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t e = base + (size_t)(p + (long)u * g.rows) * g.C4;
                v[u] = in[e];
                w[u] = BWD ? add : x[e];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                f32x4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = fmaf(v[u][q], k[q], w[u][q]);
                out[base + (size_t)(p + (long)u * g.rows) * g.C4] = o;
            }
        }
        for (; p < p1; p += g.rows) {
            const size_t e = base + (size_t)p * g.C4;
            const f32x4 v = in[e], w = BWD ? add : x[e];
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = fmaf(v[q], k[q], w[q]);
            out[e] = o;
        }
    }
}

// ---- gate forward: one workgroup per image.  m -> h (a wave per j, its lanes stride over c, wave_sum's fixed tree) -> s (a lane
// per c, j increasing).  The work is a few thousand multiply-adds: what it costs is the chain of memory round trips, so every wave's
// loads are issued before they are used and sixteen waves take sixteen hidden units at once. --------------------------------------------
__global__ __launch_bounds__(CA_GATE_LANES) void ca_gate_fwd_kernel(const float* __restrict__ m, const float* __restrict__ W1,
                                                               const float* __restrict__ B1, const float* __restrict__ W2,
                                                               const float* __restrict__ B2, float* __restrict__ h,
                                                               float* __restrict__ s, int C, int R) {
    __shared__ float sm[CA_MAX_C], sh[CA_MAX_C];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < C; c += CA_GATE_LANES) sm[c] = m[(size_t)n * C + c];
    __syncthreads();
    for (int j = wave; j < R; j += CA_GATE_LANES / 64) {
        const float bj = B1[j];
        float acc = 0.f;
#pragma unroll 4
        for (int c = lane; c < C; c += 64) acc = fmaf(W1[(size_t)j * C + c], sm[c], acc);
        acc = wave_sum(acc) + bj;
        acc = acc > 0.f ? acc : 0.f;
        if (lane == 0) { sh[j] = acc; h[(size_t)n * R + j] = acc; }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += CA_GATE_LANES) {
        const float bc = B2[c];
        float acc = 0.f;
#pragma unroll 8
        for (int j = 0; j < R; ++j) acc = fmaf(W2[(size_t)c * R + j], sh[j], acc);
        acc += bc;
        s[(size_t)n * C + c] = 1.f / (1.f + expf(-acc));
    }
}

// ---- gate backward, per image: dz2 = ds * s (1 - s);  dz1[j] = (h[j] > 0) sum_c W2[c][j] dz2[c];  dm[c] = sum_j W1[j][c] dz1[j] ------
__global__ __launch_bounds__(CA_GATE_LANES) void ca_gate_bwd_image_kernel(const float* __restrict__ ds, const float* __restrict__ s,
                                                                     const float* __restrict__ h, const float* __restrict__ W1,
                                                                     const float* __restrict__ W2, float* __restrict__ dz2,
                                                                     float* __restrict__ dz1, float* __restrict__ dm, int C, int R) {
    __shared__ float s2[CA_MAX_C], s1[CA_MAX_C];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < C; c += CA_GATE_LANES) {
        const float sv = s[(size_t)n * C + c];
        const float v = ds[(size_t)n * C + c] * (sv * (1.f - sv));
        s2[c] = v;
        dz2[(size_t)n * C + c] = v;
    }
    __syncthreads();
    for (int j = wave; j < R; j += CA_GATE_LANES / 64) {
        const float hj = h[(size_t)n * R + j];
        float acc = 0.f;
#pragma unroll 4
        for (int c = lane; c < C; c += 64) acc = fmaf(W2[(size_t)c * R + j], s2[c], acc);
        acc = wave_sum(acc);
        acc = hj > 0.f ? acc : 0.f;
        if (lane == 0) { s1[j] = acc; dz1[(size_t)n * R + j] = acc; }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += CA_GATE_LANES) {
        float acc = 0.f;
#pragma unroll 8
        for (int j = 0; j < R; ++j) acc = fmaf(W1[(size_t)j * C + c], s1[j], acc);
        dm[(size_t)n * C + c] = acc;
    }
}

// ---- gate backward, the parameters: a lane per element of (dW1 [R][C], dW2 [C][R], dB1 [R], dB2 [C]), the batch sum in increasing n --
__global__ __launch_bounds__(CA_LANES) void ca_gate_bwd_param_kernel(const float* __restrict__ dz2, const float* __restrict__ dz1,
                                                                     const float* __restrict__ h, const float* __restrict__ m,
                                                                     float* __restrict__ dW1, float* __restrict__ dB1,
                                                                     float* __restrict__ dW2, float* __restrict__ dB2, int N, int C,
                                                                     int R) {
    const int RC = R * C;
    const int e = blockIdx.x * CA_LANES + threadIdx.x;
    if (e >= 2 * RC + R + C) return;
    const float *pa, *pb = nullptr;            // sum_n pa[n * sa + ia] * pb[n * sb + ib]   (pb null: * 1)
    int sa, ia, sb = 0, ib = 0;
    float* o;
    if (e < RC) {                               // dW1[j][c] = sum_n dz1[n][j] m[n][c]
        pa = dz1; sa = R; ia = e / C; pb = m; sb = C; ib = e - ia * C; o = dW1 + e;
    } else if (e < 2 * RC) {                    // dW2[c][j] = sum_n dz2[n][c] h[n][j]
        const int f = e - RC;
        pa = dz2; sa = C; ia = f / R; pb = h; sb = R; ib = f - ia * R; o = dW2 + f;
    } else if (e < 2 * RC + R) {
        pa = dz1; sa = R; ia = e - 2 * RC; o = dB1 + ia;
    } else {
        pa = dz2; sa = C; ia = e - 2 * RC - R; o = dB2 + ia;
    }
    float acc = 0.f;
    int n = 0;
    for (; n + 8 <= N; n += 8) {                 // sixteen loads in flight; the additions stay in increasing n
        float a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            a[u] = pa[(size_t)(n + u) * sa + ia];
            b[u] = pb ? pb[(size_t)(n + u) * sb + ib] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = pb ? fmaf(a[u], b[u], acc) : acc + a[u];
    }
    for (; n < N; ++n) {
        const float a = pa[(size_t)n * sa + ia];
        acc = pb ? fmaf(a, pb[(size_t)n * sb + ib], acc) : acc + a;
    }
    *o = acc;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
static bool ca_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static CaGeom ca_geom(int N, long HW, int C) {
    CaGeom g;
    g.cols = ca_cols(C); g.rows = ca_rows(C); g.C4 = C / 4;
    g.P = ca_chunk_pixels(N, HW, C); g.HW = HW;
    g.chunks = (int)((HW + g.P - 1) / g.P);
    return g;
}

int pesr_ca_sum_launch(const float* t, const float* gy, float* out, int N, long HW, int C, double scale, void* ws, size_t ws_bytes,
                       hipStream_t stream) {
    const int chunks = pesr_ca_pool_partials_of(N, HW, C);
    if (chunks < 1 || !t || !out || !ca_aligned16(t) || !ca_aligned16(gy) || !ca_aligned16(ws)) return PESR_EINVAL;
    if (!ws || ws_bytes < (size_t)chunks * N * C * sizeof(float)) return PESR_EWORKSPACE;
    const CaGeom g = ca_geom(N, HW, C);
    if (gy)
        hipLaunchKernelGGL(ca_sum_kernel<true>, dim3(chunks * N), dim3(CA_LANES), 0, stream, (const f32x4*)t, (const f32x4*)gy, (f32x4*)ws, g, N);
    else
        hipLaunchKernelGGL(ca_sum_kernel<false>, dim3(chunks * N), dim3(CA_LANES), 0, stream, (const f32x4*)t, (const f32x4*)nullptr, (f32x4*)ws, g, N);
    const long ncols = (long)N * C;
    if (ncols > 0x7fffffffL) return PESR_EINVAL;
    hipLaunchKernelGGL(ca_sum_final_kernel, dim3((unsigned)((ncols + 63) / 64)), dim3(1024), 0, stream, (const float*)ws, out, chunks, (int)ncols, scale);
    return pesr_launch_status();
}

int pesr_ca_apply_launch(const float* in, const float* x, const float* s, const float* dm, float* out, int N, long HW, int C, float a,
                         hipStream_t stream) {
    const int chunks = pesr_ca_pool_partials_of(N, HW, C);
    if (chunks < 1 || !in || !s || !out || (!x) == (!dm)) return PESR_EINVAL;
    if (!ca_aligned16(in) || !ca_aligned16(x) || !ca_aligned16(s) || !ca_aligned16(dm) || !ca_aligned16(out)) return PESR_EINVAL;
    const CaGeom g = ca_geom(N, HW, C);
    if (dm)
        hipLaunchKernelGGL(ca_apply_kernel<true>, dim3(chunks * N), dim3(CA_LANES), 0, stream, (const f32x4*)in, (const f32x4*)nullptr, (const f32x4*)s,
                           (const f32x4*)dm, (f32x4*)out, g, a, (float)(1.0 / (double)HW));
    else
        hipLaunchKernelGGL(ca_apply_kernel<false>, dim3(chunks * N), dim3(CA_LANES), 0, stream, (const f32x4*)in, (const f32x4*)x, (const f32x4*)s,
                           (const f32x4*)nullptr, (f32x4*)out, g, a, 0.f);
    return pesr_launch_status();
}

static bool ca_gate_ok(int N, int C, int R) { return N >= 1 && C >= 4 && C % 4 == 0 && C <= CA_MAX_C && R >= 1 && R <= C; }

int pesr_ca_gate_fwd_launch(const float* m, const float* W1, const float* B1, const float* W2, const float* B2, float* h, float* s, int N,
                            int C, int R, hipStream_t stream) {
    if (!ca_gate_ok(N, C, R) || !m || !W1 || !B1 || !W2 || !B2 || !h || !s) return PESR_EINVAL;
    hipLaunchKernelGGL(ca_gate_fwd_kernel, dim3(N), dim3(CA_GATE_LANES), 0, stream, m, W1, B1, W2, B2, h, s, C, R);
    return pesr_launch_status();
}

int pesr_ca_gate_bwd_launch(const float* ds, const float* s, const float* h, const float* m, const float* W1, const float* W2, float* dm,
                            float* dW1, float* dB1, float* dW2, float* dB2, int N, int C, int R, void* ws, size_t ws_bytes,
                            hipStream_t stream) {
    if (!ca_gate_ok(N, C, R) || !ds || !s || !h || !m || !W1 || !W2 || !dm || !dW1 || !dB1 || !dW2 || !dB2) return PESR_EINVAL;
    if (!ws || ws_bytes < (size_t)N * ((size_t)C + R) * sizeof(float)) return PESR_EWORKSPACE;
    float* dz2 = (float*)ws;
    float* dz1 = dz2 + (size_t)N * C;
    hipLaunchKernelGGL(ca_gate_bwd_image_kernel, dim3(N), dim3(CA_GATE_LANES), 0, stream, ds, s, h, W1, W2, dz2, dz1, dm, C, R);
    const int elems = 2 * R * C + R + C;
    hipLaunchKernelGGL(ca_gate_bwd_param_kernel, dim3((elems + CA_LANES - 1) / CA_LANES), dim3(CA_LANES), 0, stream, (const float*)dz2,
                       (const float*)dz1, h, m, dW1, dB1, dW2, dB2, N, C, R);
    return pesr_launch_status();
}
