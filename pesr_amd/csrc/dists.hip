// DISTS (Ding et al., "Image Quality Assessment: Unifying Structure and Texture Similarity"; docs/modes.md section 4t): the two pieces
// of device arithmetic the VGG16 trunk of lpips.py lacks.
//
// L2 pooling, fp32, NHWC [N][H][W][C] -> [N][ceil(H/2)][ceil(W/2)][C]:
//     y = sqrt(sum_{ky,kx < 3} g[ky] g[kx] x[2 oy - 1 + ky][2 ox - 1 + kx]^2 + 1e-12),   g = [1, 2, 1] / 4,  zero outside the image.
// One lane owns four consecutive channels of one output pixel (one 16-byte load per tap, a wave reads 1 KiB runs).  Per channel, in this
// order, in fp32 with nothing fused (`fp contract(off)`): t_k = x_k * x_k for the nine taps k = 3 ky + kx (a tap outside the image is
// 0); s = w_0 t_0; s = s + w_k t_k for k = 1 .. 8 ascending; s = s + 1e-12f; y = sqrtf(s).  The weights 1/16, 1/8, 1/4 are powers of
// two, so the nine squares, the eight additions, the + 1e-12 and the square root are all that round.
//
// The head of one stage: per image pair and channel c over the P = H W pixels of an NHWC feature batch [2N][H][W][C] (a's features, then
// b's), in float64 from the fp32 features, the centred two-pass statistics
//     mu_a = sum(a) / P,  var_a = sum((a - mu_a)^2) / P,  cov = sum((a - mu_a)(b - mu_b)) / P      (mu_b, var_b likewise)
//     S1 = (2 mu_a mu_b + c1) / (mu_a^2 + mu_b^2 + c1),  S2 = (2 cov + c2) / (var_a + var_b + c2),  c1 = c2 = 1e-6
// and per pair sum_c alpha_c S1_c + beta_c S2_c with the stage's slices of alpha / w and beta / w.  The features are read twice.  Lanes
// run along channels (lane l of channel group g owns channel 64 g + l), so a wave's load of a pixel is one run of 256 bytes.  Every sum
// has one fixed order, which tests/dists_oracle.py layer_ordered restates operation by operation; all of it float64 with plain operators:
//   block partial  a workgroup of 4 waves owns 256 consecutive pixels of one image and 64 channels; wave v adds pixels v, v + 4, v + 8,
//                  ... of the block in ascending order from 0.0 (pixels past the image are skipped); then ((s0 + s1) + s2) + s3
//   first pass     s = s + a;  s = s + b                                                   -> partials [N][2][C][blocks]
//   means          mean_partials_kernel (reduce.hip) over a channel's partials in ascending block order, / P -> mu [N][2][C]
//   second pass    da = a - mu_a; db = b - mu_b; va = va + da * da; vb = vb + db * db; cv = cv + da * db
//                                                                                         -> partials [N][3][C][blocks]
//   moments        mean_partials_kernel again, / P                                         -> var_a, var_b, cov [N][3][C]
//   score          one workgroup of 256 lanes per pair; lane t takes channels t, t + 256, ... ascending:
//                  m = mu_a * mu_b;  n1 = 2 m + c1;  d1 = (mu_a * mu_a + mu_b * mu_b) + c1;  S1 = n1 / d1
//                  n2 = 2 cov + c2;  d2 = (var_a + var_b) + c2;  S2 = n2 / d2
//                  acc = acc + (alpha_c * S1 + beta_c * S2);  then block_sum_d (common.h)
// No atomics; the order is a function of (P, C) alone, so the result has the same bits on every call, with or without the statistics.
#pragma clang fp contract(off)
#include "common.h"
#include "launchers.h"

constexpr int L2POOL_THREADS = 256;
constexpr float L2POOL_EPS = 1e-12f;

// grid ceil(N Ho Wo (C / 4) / 256)
__global__ __launch_bounds__(L2POOL_THREADS) void l2pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long total, int H,
                                                                     int W, int Ho, int Wo, int C4) {
    const long i = (long)blockIdx.x * L2POOL_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    long pix = i / C4;
    const int ox = (int)(pix % Wo);
    pix /= Wo;
    const int oy = (int)(pix % Ho);
    const long n = pix / Ho;
    const float* xn = x + n * H * W * C4 * 4 + c4 * 4;
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const f32x4*)(xn + ((long)iy * W + ix) * C4 * 4);
            const float wt = (ky == 1 ? 0.5f : 0.25f) * (kx == 1 ? 0.5f : 0.25f);
            const float in[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = in[e] * in[e];
                const float wtt = wt * t;                               // a power of two: exact
                s[e] = (ky == 0 && kx == 0) ? wtt : s[e] + wtt;
            }
        }
    }
    f32x4 o;
    o.x = sqrtf(s[0] + L2POOL_EPS), o.y = sqrtf(s[1] + L2POOL_EPS), o.z = sqrtf(s[2] + L2POOL_EPS), o.w = sqrtf(s[3] + L2POOL_EPS);
    *(f32x4*)(y + i * 4) = o;
}

static bool l2pool_shape_ok(int N, int H, int W, int C) { return N >= 1 && H >= 1 && W >= 1 && C >= 64 && C % 64 == 0; }

long pesr_l2pool_blocks_of(int N, int H, int W, int C) {
    if (!l2pool_shape_ok(N, H, W, C)) return 0;
    const long total = (long)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4);
    return (total + L2POOL_THREADS - 1) / L2POOL_THREADS;
}

int pesr_l2pool_fwd_launch(const float* x, float* y, int N, int H, int W, int C, hipStream_t stream) {
    if (!x || !y || !l2pool_shape_ok(N, H, W, C)) return PESR_EINVAL;
    if (((uintptr_t)x & 15) || ((uintptr_t)y & 15)) return PESR_EINVAL;   // the vector loads and stores need 16-byte bases
    const long blocks = pesr_l2pool_blocks_of(N, H, W, C);
    if (blocks > 2147483647L) return PESR_EINVAL;
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    hipLaunchKernelGGL(l2pool_fwd_kernel, dim3((unsigned)blocks), dim3(L2POOL_THREADS), 0, stream, x, y, (long)N * Ho * Wo * (C / 4), H, W,
                       Ho, Wo, C / 4);
    return pesr_launch_status();
}

// ---- the head ----------------------------------------------------------------------------------------------------------------------
constexpr int DISTS_THREADS = 256;
constexpr int DISTS_BLOCK_PIX = 256;                                // pixels per workgroup: 64 per wave
constexpr int DISTS_UNROLL = 4;                                     // pixels whose loads are in flight together in a lane
constexpr double DISTS_C1 = 1e-6, DISTS_C2 = 1e-6;

// ((s0 + s1) + s2) + s3 of the four waves' values of one lane, per quantity q < Q; the sum goes to part[q][c][block]
template <int Q>
__device__ __forceinline__ void dists_store_partials(const double* s, double (*red)[DISTS_THREADS], double* __restrict__ part, long n, int c,
                                                     int C, bool on) {
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int q = 0; q < Q; ++q) red[q][tid] = s[q];
    __syncthreads();
    if (tid < 64 && on) {
        const long nb = gridDim.x;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const double t = ((red[q][lane] + red[q][64 + lane]) + red[q][128 + lane]) + red[q][192 + lane];
            part[((n * Q + q) * C + c) * nb + blockIdx.x] = t;
        }
    }
}

// grid (blocks, ceil(C / 64), N).  MODE 0: the sums of a and of b; MODE 1: the centred second moments, mu [N][2][C] from the first pass.
template <int MODE>
__global__ __launch_bounds__(DISTS_THREADS) void dists_pass_kernel(const float* __restrict__ feat, const double* __restrict__ mu,
                                                                   double* __restrict__ part, long P, int C, int N) {
    constexpr int Q = MODE == 0 ? 2 : 3;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long n = blockIdx.z;
    const int c = blockIdx.y * 64 + lane;
    const bool on = c < C;
    const float* fa = feat + n * P * C + c;
    const float* fb = feat + (n + N) * P * C + c;
    double ma = 0.0, mb = 0.0;
    if (MODE == 1 && on) ma = mu[(n * 2 + 0) * C + c], mb = mu[(n * 2 + 1) * C + c];
    const long p0 = (long)blockIdx.x * DISTS_BLOCK_PIX + wv;
    const long bend = ((long)blockIdx.x + 1) * DISTS_BLOCK_PIX;
    const long pend = bend < P ? bend : P;
    double s[3] = {0.0, 0.0, 0.0};
    if (on) {
        for (long pb = p0; pb < pend; pb += 4 * DISTS_UNROLL) {
            float xa[DISTS_UNROLL], xb[DISTS_UNROLL];
#pragma unroll
            for (int u = 0; u < DISTS_UNROLL; ++u) {
                const long p = pb + 4 * u;
                xa[u] = p < pend ? fa[p * C] : 0.0f;
                xb[u] = p < pend ? fb[p * C] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < DISTS_UNROLL; ++u) {
                if (pb + 4 * u < pend) {
                    const double a = (double)xa[u], b = (double)xb[u];
                    if (MODE == 0) {
                        s[0] = s[0] + a;
                        s[1] = s[1] + b;
                    } else {
                        const double da = a - ma, db = b - mb;
                        const double aa = da * da, bb = db * db, ab = da * db;
                        s[0] = s[0] + aa;
                        s[1] = s[1] + bb;
                        s[2] = s[2] + ab;
                    }
                }
            }
        }
    }
    __shared__ double red[Q][DISTS_THREADS];
    dists_store_partials<Q>(s, red, part, n, c, C, on);
}

// grid N.  mu [N][2][C], mom [N][3][C] -> out[n], and the five statistics [N][C][5] when asked for.
__global__ __launch_bounds__(DISTS_THREADS) void dists_score_kernel(const double* __restrict__ mu, const double* __restrict__ mom,
                                                                    const double* __restrict__ alpha, const double* __restrict__ beta,
                                                                    double* __restrict__ out, double* __restrict__ stats, int C) {
    const long n = blockIdx.x;
    double acc = 0.0;
    for (int c = threadIdx.x; c < C; c += DISTS_THREADS) {
        const double ma = mu[(n * 2 + 0) * C + c], mb = mu[(n * 2 + 1) * C + c];
        const double va = mom[(n * 3 + 0) * C + c], vb = mom[(n * 3 + 1) * C + c], cv = mom[(n * 3 + 2) * C + c];
        const double m = ma * mb;
        const double n1 = 2.0 * m + DISTS_C1;
        const double qa = ma * ma, qb = mb * mb;
        const double d1 = (qa + qb) + DISTS_C1;
        const double s1 = n1 / d1;
        const double n2 = 2.0 * cv + DISTS_C2;
        const double d2 = (va + vb) + DISTS_C2;
        const double s2 = n2 / d2;
        const double t1 = alpha[c] * s1, t2 = beta[c] * s2;
        const double term = t1 + t2;
        acc = acc + term;
        if (stats) {
            double* st = stats + (n * C + c) * 5;
            st[0] = ma, st[1] = mb, st[2] = va, st[3] = vb, st[4] = cv;
        }
    }
    __shared__ double red[4];
    const double t = block_sum_d(acc, red);
    if (threadIdx.x == 0) out[n] = t;
}

static bool dists_shape_ok(int N, long P, int C) {
    return N >= 1 && N <= 32767 && P >= 1 && (C == 3 || C == 64 || C == 128 || C == 256 || C == 512);
}

long pesr_dists_pixel_blocks_of(int N, long P, int C) {
    if (!dists_shape_ok(N, P, C)) return 0;
    return (P + DISTS_BLOCK_PIX - 1) / DISTS_BLOCK_PIX;
}

// partials [N][2][C][blocks] and [N][3][C][blocks], mu [N][2][C], moments [N][3][C]: doubles
size_t pesr_dists_ws_bytes(int N, long P, int C) {
    const long nb = pesr_dists_pixel_blocks_of(N, P, C);
    if (nb < 1) return 0;
    return (size_t)N * C * 5 * ((size_t)nb + 1) * sizeof(double);
}

int pesr_dists_layer_launch(const float* feat, const double* alpha, const double* beta, double* out, int N, int H, int W, int C,
                            double* stats, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!feat || !alpha || !beta || !out || H < 1 || W < 1) return PESR_EINVAL;
    const long P = (long)H * W;
    if (!dists_shape_ok(N, P, C)) return PESR_EINVAL;
    if (((uintptr_t)feat & 3) || ((uintptr_t)alpha & 7) || ((uintptr_t)beta & 7) || ((uintptr_t)out & 7) || ((uintptr_t)stats & 7) ||
        ((uintptr_t)ws & 7))
        return PESR_EINVAL;
    const long nb = pesr_dists_pixel_blocks_of(N, P, C);
    if (nb > 2147483647L) return PESR_EINVAL;
    if (!ws || ws_bytes < pesr_dists_ws_bytes(N, P, C)) return PESR_EWORKSPACE;
    double* part1 = (double*)ws;                                    // [N][2][C][nb]
    double* part2 = part1 + (size_t)N * 2 * C * nb;                 // [N][3][C][nb]
    double* mu = part2 + (size_t)N * 3 * C * nb;                    // [N][2][C]
    double* mom = mu + (size_t)N * 2 * C;                           // [N][3][C]
    const dim3 grid((unsigned)nb, (unsigned)((C + 63) / 64), (unsigned)N), block(DISTS_THREADS);
    hipLaunchKernelGGL(dists_pass_kernel<0>, grid, block, 0, stream, feat, (const double*)nullptr, part1, P, C, N);
    int rc = pesr_mean_partials_launch(part1, mu, N * 2 * C, nb, (double)P, stream);
    if (rc != PESR_OK) return rc;
    hipLaunchKernelGGL(dists_pass_kernel<1>, grid, block, 0, stream, feat, (const double*)mu, part2, P, C, N);
    rc = pesr_mean_partials_launch(part2, mom, N * 3 * C, nb, (double)P, stream);
    if (rc != PESR_OK) return rc;
    hipLaunchKernelGGL(dists_score_kernel, dim3(N), block, 0, stream, (const double*)mu, (const double*)mom, alpha, beta, out, stats, C);
    return pesr_launch_status();
}
