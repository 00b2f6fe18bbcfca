// LayerNorm over the channels of each pixel (docs/modes.md section 4x), x [P][C] fp32 (the P = N H W pixels of an NHWC tensor):
//   mean = (1/C) sum_c x      var = (1/C) sum_c (x - mean)^2      rstd = 1 / sqrt(var + eps)      xh = (x - mean) rstd
//   y = xh gamma + beta                                            stats[p] = (mean, rstd)
// and its backward:
//   g = dy gamma      dx = rstd (g - mean_c(g) - xh mean_c(g xh))      dgamma_c = sum_p dy xh      dbeta_c = sum_p dy
//
// Two streaming kernels with one geometry.  A pixel's channels sit in the registers of a GROUP of G lanes, G the power of two that
// covers C / 4 (at most 64); a lane holds K = ceil(C / 4 / 64) float4 pieces, piece k of lane l the channels 4 (l + k G) .. + 3, so
// that every access is 16 bytes and a wave reads whole contiguous rows.  The variance is the centred form, from the values in the
// registers: x is read once.  Both reductions of a pixel run across its group's lanes by xor shuffles (a butterfly: every lane of the
// group ends with the same bits), no LDS.  A 256-lane workgroup takes 256 / G pixels at once and walks on by the grid's width, U
// pixels (U K <= 4 pieces per tensor in flight) per step; the grid is capped at LN_MAX_ROWS workgroups and depends on the shape alone.
// In the backward a lane owns the same channels for every pixel it meets and keeps their dgamma / dbeta in registers; the lanes of
// a wave with the same channels meet by shuffles, the four waves through LDS in wave order, and the workgroup leaves one row of a
// [rows][2 C] workspace (dgamma | dbeta), which reduce_rows.h's fixed-order second stage adds in double.  No atomics, every output
// element is written exactly once, the same bits on every call.  Element offsets are size_t.
#include "common.h"
#include "launchers.h"
#include "reduce_rows.h"

#include <math.h>

#define LN_LANES 256
#define LN_MAX_C 1024
#define LN_MAX_ROWS 1024     // workgroups of a launch = partial rows of the backward: four per CU

// Host: the geometry.
static inline int ln_group(int C) {
    int g = 1;
    while (g < C / 4 && g < 64) g <<= 1;
    return g;
}
static inline int ln_pieces(int C) { return (C / 4 + 63) / 64; }
static bool ln_shape_ok(long P, int C) { return P >= 1 && C >= 4 && C % 4 == 0 && C <= LN_MAX_C; }

int pesr_layernorm_partials_of(long P, int C) {
    if (!ln_shape_ok(P, C)) return 0;
    const long at_once = LN_LANES / ln_group(C);
    const long rows = (P + at_once - 1) / at_once;
    return (int)(rows < LN_MAX_ROWS ? rows : LN_MAX_ROWS);
}
size_t pesr_layernorm_ws_bytes(long P, int C) { return (size_t)pesr_layernorm_partials_of(P, C) * 2 * (size_t)C * sizeof(float); }

template <int G> __device__ __forceinline__ float ln_group_sum(float v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// the lanes of a wave that hold the same channels: one per group
template <int G> __device__ __forceinline__ float ln_across_groups(float v) {
#pragma unroll
    for (int off = G; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float ln_sum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

template <int K> struct LnUnroll { static constexpr int U = K == 1 ? 4 : K == 2 ? 2 : 1; };

// ---- forward -------------------------------------------------------------------------------------------------------------------------
template <int G, int K>
__global__ __launch_bounds__(LN_LANES) void ln_fwd_kernel(const f32x4* __restrict__ x, const f32x4* __restrict__ gamma,
                                                          const f32x4* __restrict__ beta, f32x4* __restrict__ y,
                                                          f32x2* __restrict__ stats, long P, int C4, float c, float eps) {
    constexpr int U = LnUnroll<K>::U, AT_ONCE = LN_LANES / G;
    const int l = threadIdx.x & (G - 1), sub = threadIdx.x / G;
    const long Q = (long)gridDim.x * AT_ONCE;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 gm[K], bt[K];
    bool act[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        act[k] = l + k * G < C4;
        gm[k] = act[k] ? gamma[l + k * G] : zero;
        bt[k] = act[k] ? beta[l + k * G] : zero;
    }
    // (`first` is the same in every lane of the workgroup: all of them take every step, so every shuffle finds its partner)
    for (long first = (long)blockIdx.x * AT_ONCE; first < P; first += Q * U) {
        f32x4 v[U][K];
        long p[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            p[u] = first + sub + (long)u * Q;
#pragma unroll
            for (int k = 0; k < K; ++k) v[u][k] = (p[u] < P && act[k]) ? x[(size_t)p[u] * C4 + (l + k * G)] : zero;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) s += ln_sum4(v[u][k]);
            const float mean = ln_group_sum<G>(s) / c;      // (a division: 1 / C is not a float for every C, and the mean may be large)
            f32x4 d[K];
            float q = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                d[k] = act[k] ? v[u][k] - mean : zero;
                q += ln_sum4(d[k] * d[k]);
            }
            const float rstd = 1.f / sqrtf(ln_group_sum<G>(q) / c + eps);
            if (p[u] < P) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (!act[k]) continue;
                    const f32x4 xh = d[k] * rstd;
                    f32x4 o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = fmaf(xh[j], gm[k][j], bt[k][j]);
                    y[(size_t)p[u] * C4 + (l + k * G)] = o;
                }
                if (l == 0) {
                    const f32x2 st = {mean, rstd};
                    stats[p[u]] = st;
                }
            }
        }
    }
}

// ---- backward, first stage: dx, and part[workgroup][0 .. C-1] = sum dy xh, part[workgroup][C .. 2C-1] = sum dy over its pixels --------
template <int G, int K>
__global__ __launch_bounds__(LN_LANES) void ln_bwd_kernel(const f32x4* __restrict__ x, const f32x4* __restrict__ gamma,
                                                          const f32x2* __restrict__ stats, const f32x4* __restrict__ dy,
                                                          f32x4* __restrict__ dx, f32x4* __restrict__ part, long P, int C4,
                                                          float inv_c) {
    constexpr int U = LnUnroll<K>::U, AT_ONCE = LN_LANES / G;
    __shared__ f32x4 red[LN_LANES / 64][2][64];
    const int l = threadIdx.x & (G - 1), sub = threadIdx.x / G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long Q = (long)gridDim.x * AT_ONCE;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 gm[K], dg[K], db[K];
    bool act[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        act[k] = l + k * G < C4;
        gm[k] = act[k] ? gamma[l + k * G] : zero;
        dg[k] = zero;
        db[k] = zero;
    }
    for (long first = (long)blockIdx.x * AT_ONCE; first < P; first += Q * U) {
        f32x4 v[U][K], w[U][K];
        f32x2 st[U];
        long p[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            p[u] = first + sub + (long)u * Q;
            const bool in = p[u] < P;
            const f32x2 none = {0.f, 0.f};
            st[u] = in ? stats[p[u]] : none;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const bool take = in && act[k];
                v[u][k] = take ? x[(size_t)p[u] * C4 + (l + k * G)] : zero;
                w[u][k] = take ? dy[(size_t)p[u] * C4 + (l + k * G)] : zero;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float mean = st[u][0], rstd = st[u][1];
            f32x4 xh[K], g[K];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                xh[k] = (v[u][k] - mean) * rstd;
                g[k] = w[u][k] * gm[k];                 // (zero in a piece past C and in a pixel past P: dy is)
                s1 += ln_sum4(g[k]);
                s2 += ln_sum4(g[k] * xh[k]);
            }
            s1 = ln_group_sum<G>(s1) * inv_c;
            s2 = ln_group_sum<G>(s2) * inv_c;
#pragma unroll
            for (int k = 0; k < K; ++k) {
#pragma unroll
                for (int j = 0; j < 4; ++j) dg[k][j] = fmaf(w[u][k][j], xh[k][j], dg[k][j]);
                db[k] += w[u][k];
                if (p[u] < P && act[k]) dx[(size_t)p[u] * C4 + (l + k * G)] = (g[k] - s1 - xh[k] * s2) * rstd;
            }
        }
    }
    // the wave's groups by shuffles, the waves through LDS in wave order
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dg[k][j] = ln_across_groups<G>(dg[k][j]);
            db[k][j] = ln_across_groups<G>(db[k][j]);
        }
        if (k) __syncthreads();                          // (red is still read for the previous piece)
        if (lane < G) {
            red[wave][0][lane] = dg[k];
            red[wave][1][lane] = db[k];
        }
        __syncthreads();
        if (threadIdx.x < G && act[k]) {                 // (wave 0's first group: l == threadIdx.x)
            f32x4* row = part + (size_t)blockIdx.x * 2 * C4;
            row[l + k * G] = ((red[0][0][l] + red[1][0][l]) + red[2][0][l]) + red[3][0][l];
            row[C4 + l + k * G] = ((red[0][1][l] + red[1][1][l]) + red[2][1][l]) + red[3][1][l];
        }
    }
}

// ---- backward, second stage: the rows in increasing order, in double (reduce_rows.h) ------------------------------------------------
__global__ __launch_bounds__(1024) void ln_bwd_final_kernel(const float* __restrict__ part, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, int rows, int C) {
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + cl;
    __shared__ double red[16][64];
    const double s = reduce_rows_block(part, rows, 2 * C, col, col < 2 * C, red);
    if (rl == 0 && col < 2 * C) {
        if (col < C) dgamma[col] = (float)s;
        else dbeta[col - C] = (float)s;
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
static bool ln_ptr_ok(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

// One case per (G, K) the geometry can give: K = 1 with every G, G = 64 with K = 2 .. 4.
#define LN_DISPATCH(LAUNCH)                                                                                                  \
    switch (ln_pieces(C) * 128 + ln_group(C)) {                                                                              \
        case 128 + 1: LAUNCH(1, 1); break;                                                                                   \
        case 128 + 2: LAUNCH(2, 1); break;                                                                                   \
        case 128 + 4: LAUNCH(4, 1); break;                                                                                   \
        case 128 + 8: LAUNCH(8, 1); break;                                                                                   \
        case 128 + 16: LAUNCH(16, 1); break;                                                                                 \
        case 128 + 32: LAUNCH(32, 1); break;                                                                                 \
        case 128 + 64: LAUNCH(64, 1); break;                                                                                 \
        case 256 + 64: LAUNCH(64, 2); break;                                                                                 \
        case 384 + 64: LAUNCH(64, 3); break;                                                                                 \
        case 512 + 64: LAUNCH(64, 4); break;                                                                                 \
        default: return PESR_EINVAL;                                                                                         \
    }

int pesr_layernorm_fwd_launch(const float* x, const float* gamma, const float* beta, float* y, float* stats, long P, int C, float eps,
                              hipStream_t stream) {
    if (!ln_shape_ok(P, C) || !(eps > 0.f) || !isfinite(eps)) return PESR_EINVAL;
    if (!ln_ptr_ok(x) || !ln_ptr_ok(gamma) || !ln_ptr_ok(beta) || !ln_ptr_ok(y) || !ln_ptr_ok(stats)) return PESR_EINVAL;
    const int rows = pesr_layernorm_partials_of(P, C);
#define LN_FWD(G_, K_)                                                                                                            \
    hipLaunchKernelGGL((ln_fwd_kernel<G_, K_>), dim3(rows), dim3(LN_LANES), 0, stream, (const f32x4*)x, (const f32x4*)gamma,          \
                       (const f32x4*)beta, (f32x4*)y, (f32x2*)stats, P, C / 4, (float)C, eps)
    LN_DISPATCH(LN_FWD)
#undef LN_FWD
    return pesr_launch_status();
}

int pesr_layernorm_bwd_launch(const float* x, const float* gamma, const float* stats, const float* dy, float* dx, float* dgamma,
                              float* dbeta, void* ws, long P, int C, hipStream_t stream) {
    if (!ln_shape_ok(P, C)) return PESR_EINVAL;
    if (!ln_ptr_ok(x) || !ln_ptr_ok(gamma) || !ln_ptr_ok(stats) || !ln_ptr_ok(dy) || !ln_ptr_ok(dx) || !ln_ptr_ok(dgamma) ||
        !ln_ptr_ok(dbeta) || !ln_ptr_ok(ws))
        return PESR_EINVAL;
    const int rows = pesr_layernorm_partials_of(P, C);
    const float inv_c = 1.f / (float)C;
#define LN_BWD(G_, K_)                                                                                                            \
    hipLaunchKernelGGL((ln_bwd_kernel<G_, K_>), dim3(rows), dim3(LN_LANES), 0, stream, (const f32x4*)x, (const f32x4*)gamma,          \
                       (const f32x2*)stats, (const f32x4*)dy, (f32x4*)dx, (f32x4*)ws, P, C / 4, inv_c)
    LN_DISPATCH(LN_BWD)
#undef LN_BWD
    hipLaunchKernelGGL(ln_bwd_final_kernel, dim3((2 * C + 63) / 64), dim3(1024), 0, stream, (const float*)ws, dgamma, dbeta, rows, C);
    return pesr_launch_status();
}
