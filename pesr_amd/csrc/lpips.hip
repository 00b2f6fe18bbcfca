// The LPIPS head of one tapped layer (docs/modes.md section 4n): for every pixel p of an NHWC feature tensor [2N][H][W][C] whose first N
// entries are the features of image a and whose last N those of image b,
//     na = sqrt(sum_c a_c^2),  nb likewise,  d(p) = sum_c w_c * (a_c / (na + 1e-10) - b_c / (nb + 1e-10))^2,
// and per image pair the mean of d(p) over the H * W pixels.  Zhang et al.'s "lin" layer on the squared difference of the
// unit-normalised features, the two-pass form: the one-pass expansion into sum a^2, sum b^2, sum w a^2, sum w b^2, sum w a b cancels
// when a ~ b, the regime a good result is in.
//
// Every feature element is read once.  One wave per pixel: lane l holds K = C / 64 channels of a and of b in registers, loaded as the
// widest vector C allows (C = 64: one float, channel l; 128: two, 2l + e; 256: four, 4l + e; 512: two vectors of four, 256 j + 4l + e),
// so a wave's load of a pixel is one contiguous run.  All arithmetic after the load is float64 with plain operators and no fused
// multiply-add (`fp contract(off)`, as ssim.hip), and every sum has one fixed order, which tests/lpips_oracle.py restates operation
// by operation:
//   lane partial   s = 0; for k = 0 .. K-1 ascending: s = s + x_k * x_k             (a and b: two independent chains)
//   across lanes   lpips_wave_sum: v = v + v[lane ^ off], off = 1, 2, 4, 8, 16, 32    (every lane ends with the same bits)
//   per channel    t = a_k / (na + 1e-10) - b_k / (nb + 1e-10);  acc = acc + w_k * (t * t), k ascending, then across lanes
//   workgroup      256 lanes = 4 waves own 64 consecutive pixels of one image, wave v pixels 16 v .. 16 v + 15 in ascending order:
//                  s = s + d(p); then ((s0 + s1) + s2) + s3 -> one partial per workgroup in the workspace
//   image          mean_partials_kernel (reduce.hip): lane t adds partials t, t + 256, ... ascending, wave_sum_d (off = 32 .. 1),
//                  ((r0 + r1) + r2) + r3, / (H * W).
// No atomics; the order is a function of (H, W, C) alone, so the score has the same bits on every call, with or without the map.
// The IEEE double division and square root are correctly rounded (their expansions are the only fused operations in this file's code).
//
// lpips_layer2 is the same forward with the two feature tensors as separate base pointers (the training path has no [a; b] batch);
// pesr_lpips_layer is a call of it with fb = feat + N * H * W * C: one kernel, the same bits.
//
// The head's gradient (docs/modes.md section 4o): with g[n] = dL/dscore of pair n (float64), ga = dL/dfa, fp32, for fa only.  The same
// wave per pixel, the same lane-to-channel layout, loads and stores of the same width, every feature element read once and every
// gradient element written once; no LDS, no atomics, no cross-pixel sum.  Per pixel, in this order, which tests/lpips_grad_oracle.py
// restates operation by operation:
//   per image      scale = (2 * g[n]) / (double)(H * W)
//   norms          na = sqrt(lpips_wave_sum(sa)), nb likewise, sa and sb the forward's lane chains;  da = na + 1e-10, db = nb + 1e-10
//                  (the forward's bits)
//   per channel    ah = a_k / da;  bh = b_k / db;  t = ah - bh;  wt_k = w_k * t;  acc = acc + wt_k * ah, k ascending;
//                  q = lpips_wave_sum(acc)
//   per pixel      r = q / na;  c = scale / da                       (two divisions per pixel, none per element beyond ah and bh)
//   per channel    ga_k = (float)(c * (wt_k - a_k * r)): one rounding to fp32;  ga_k = 0 for every k where na == 0
// na == 0 is a definition, not the formula's value: every channel of such a pixel left its ReLU at zero, so the conv behind the tap
// masks the gradient anyway; the formula would give 2 w t / 1e-10 there and autograd NaN, and neither may reach the trunk.
#pragma clang fp contract(off)
#include "common.h"
#include "launchers.h"

constexpr int LPIPS_THREADS = 256;
constexpr int LPIPS_WAVE_PIX = 16;                                  // consecutive pixels per wave
constexpr int LPIPS_WG_PIX = LPIPS_WAVE_PIX * (LPIPS_THREADS / 64);  // 64 per workgroup
constexpr double LPIPS_EPS = 1e-10;

// v = v + v[lane ^ off], off = 1, 2, 4, 8, 16, 32, all 64 lanes active: three such sums per pixel.
#ifdef PESR_LPIPS_SHFL_ONLY
// The plain form, for the A/B measurement of docs/modes.md section 4n only (an experiment build through PESR_HIP_LIB): every step a
// __shfl_xor, two ds_bpermute per step of a double.  The same bits as the form below.
__device__ __forceinline__ double lpips_wave_sum(double v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}
#else
// The four steps inside a row of 16 lanes are DPP moves, which cost no LDS traffic (measured against the plain form in section 4n).
template <int CTRL> __device__ __forceinline__ double lpips_dpp(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// After the first two steps the four lanes of a quad hold the same bits, so the lane that row_half_mirror reads (7 - i of its eight)
// holds what lane ^ 4 holds; likewise row_mirror and lane ^ 8.
__device__ __forceinline__ double lpips_wave_sum(double v) {
    v = v + lpips_dpp<0xB1>(v);                                      // quad_perm [1, 0, 3, 2]
    v = v + lpips_dpp<0x4E>(v);                                      // quad_perm [2, 3, 0, 1]
    v = v + lpips_dpp<0x141>(v);                                     // row_half_mirror
    v = v + lpips_dpp<0x140>(v);                                     // row_mirror
    v = v + __shfl_xor(v, 16, 64);
    v = v + __shfl_xor(v, 32, 64);
    return v;
}
#endif

template <int V> __device__ __forceinline__ void lpips_load(const float* __restrict__ p, float* o) {
    if constexpr (V == 1) {
        o[0] = __builtin_nontemporal_load(p);
    } else if constexpr (V == 2) {
        const f32x2 t = __builtin_nontemporal_load((const f32x2*)p);
        o[0] = t.x, o[1] = t.y;
    } else {
        const f32x4 t = __builtin_nontemporal_load((const f32x4*)p);
        o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = t.w;
    }
}

// grid (ceil(HW / 64), N)
template <int C>
__global__ __launch_bounds__(LPIPS_THREADS) void lpips_layer_kernel(const float* __restrict__ fa0, const float* __restrict__ fb0,
                                                                     const float* __restrict__ w, double* __restrict__ part,
                                                                     double* __restrict__ map, long HW) {
    constexpr int K = C / 64, V = K < 4 ? K : 4, J = K / V;
    constexpr int UNROLL = K < 8 ? 4 : 2;                           // pixels whose loads are in flight together in a wave
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = blockIdx.y;
    const float* fa = fa0 + (long)n * HW * C;
    const float* fb = fb0 + (long)n * HW * C;
    double wd[K];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < V; ++e) wd[j * V + e] = (double)w[j * 64 * V + lane * V + e];

    const long p0 = (long)blockIdx.x * LPIPS_WG_PIX + wv * LPIPS_WAVE_PIX;
    double s = 0.0;
    for (int i0 = 0; i0 < LPIPS_WAVE_PIX; i0 += UNROLL) {
        float xa[UNROLL][K], xb[UNROLL][K];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const long p = p0 + i0 + u;                             // the same for a whole wave: no divergence
            if (p < HW) {
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    lpips_load<V>(fa + p * C + j * 64 * V + lane * V, &xa[u][j * V]);
                    lpips_load<V>(fb + p * C + j * 64 * V + lane * V, &xb[u][j * V]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k) xa[u][k] = xb[u][k] = 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const long p = p0 + i0 + u;
            if (p < HW) {
                double sa = 0.0, sb = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double a = (double)xa[u][k], b = (double)xb[u][k];
                    const double aa = a * a, bb = b * b;
                    sa = sa + aa;
                    sb = sb + bb;
                }
                const double da = sqrt(lpips_wave_sum(sa)) + LPIPS_EPS;
                const double db = sqrt(lpips_wave_sum(sb)) + LPIPS_EPS;
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double ah = (double)xa[u][k] / da, bh = (double)xb[u][k] / db;
                    const double t = ah - bh;
                    const double tt = t * t;
                    const double wt = wd[k] * tt;
                    acc = acc + wt;
                }
                const double d = lpips_wave_sum(acc);
                s = s + d;
                if (map && lane == 0) map[(long)n * HW + p] = d;
            }
        }
    }
    __shared__ double red[LPIPS_THREADS / 64];                      // block_sum_d without its wave_sum_d: s is the wave's sum already
    if (lane == 0) red[wv] = s;
    __syncthreads();
    if (tid == 0) part[(long)n * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// grid (ceil(HW / 64), N): the forward's loads and norms, then the gradient of fa (the order is in this file's header)
template <int V> __device__ __forceinline__ void lpips_store(float* __restrict__ p, const float* o) {
    if constexpr (V == 1) {
        __builtin_nontemporal_store(o[0], p);
    } else if constexpr (V == 2) {
        f32x2 t;
        t.x = o[0], t.y = o[1];
        __builtin_nontemporal_store(t, (f32x2*)p);
    } else {
        f32x4 t;
        t.x = o[0], t.y = o[1], t.z = o[2], t.w = o[3];
        __builtin_nontemporal_store(t, (f32x4*)p);
    }
}

template <int C>
__global__ __launch_bounds__(LPIPS_THREADS) void lpips_layer_bwd_kernel(const float* __restrict__ fa0, const float* __restrict__ fb0,
                                                                         const float* __restrict__ w, const double* __restrict__ g,
                                                                         float* __restrict__ ga0, long HW) {
    constexpr int K = C / 64, V = K < 4 ? K : 4, J = K / V;
    constexpr int UNROLL = K < 8 ? 4 : 2;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = blockIdx.y;
    const float* fa = fa0 + (long)n * HW * C;
    const float* fb = fb0 + (long)n * HW * C;
    float* ga = ga0 + (long)n * HW * C;
    double wd[K];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < V; ++e) wd[j * V + e] = (double)w[j * 64 * V + lane * V + e];
    const double two_g = 2.0 * g[n];
    const double scale = two_g / (double)HW;

    const long p0 = (long)blockIdx.x * LPIPS_WG_PIX + wv * LPIPS_WAVE_PIX;
    for (int i0 = 0; i0 < LPIPS_WAVE_PIX; i0 += UNROLL) {
        float xa[UNROLL][K], xb[UNROLL][K];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const long p = p0 + i0 + u;                             // the same for a whole wave: no divergence
            if (p < HW) {
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    lpips_load<V>(fa + p * C + j * 64 * V + lane * V, &xa[u][j * V]);
                    lpips_load<V>(fb + p * C + j * 64 * V + lane * V, &xb[u][j * V]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k) xa[u][k] = xb[u][k] = 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const long p = p0 + i0 + u;
            if (p < HW) {                                           // nothing is written for a pixel past the image
                double sa = 0.0, sb = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double a = (double)xa[u][k], b = (double)xb[u][k];
                    const double aa = a * a, bb = b * b;
                    sa = sa + aa;
                    sb = sb + bb;
                }
                const double na = sqrt(lpips_wave_sum(sa));
                const double nb = sqrt(lpips_wave_sum(sb));
                const double da = na + LPIPS_EPS, db = nb + LPIPS_EPS;
                double wt[K];
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double ah = (double)xa[u][k] / da, bh = (double)xb[u][k] / db;
                    const double t = ah - bh;
                    wt[k] = wd[k] * t;
                    const double qa = wt[k] * ah;
                    acc = acc + qa;
                }
                const double q = lpips_wave_sum(acc);
                const double r = q / na;                            // (non-finite where na == 0: not used there)
                const double c = scale / da;
                float o[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double m = (double)xa[u][k] * r;
                    const double v = wt[k] - m;
                    const double cv = c * v;
                    o[k] = na == 0.0 ? 0.0f : (float)cv;
                }
#pragma unroll
                for (int j = 0; j < J; ++j) lpips_store<V>(ga + p * C + j * 64 * V + lane * V, &o[j * V]);
            }
        }
    }
}

// the channel counts of the five taps
template <class F>
static bool lpips_dispatch_c(int C, F&& f) { return pesr_dispatch_c<64, 128, 256, 512>(C, f); }

static bool lpips_shape_ok(int N, int H, int W, int C) {
    return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && lpips_dispatch_c(C, [](auto) {});
}

int pesr_lpips_layer2_launch(const float* fa, const float* fb, const float* w, double* out, int N, int H, int W, int C, double* map,
                             void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!fa || !fb || !w || !out || !lpips_shape_ok(N, H, W, C)) return PESR_EINVAL;
    if (((uintptr_t)fa & 15) || ((uintptr_t)fb & 15) || ((uintptr_t)w & 3) || ((uintptr_t)out & 7) || ((uintptr_t)map & 7) ||
        ((uintptr_t)ws & 7))
        return PESR_EINVAL;                                         // the vector loads need each tensor's base on 16 bytes
    const long HW = (long)H * W;
    const long groups = (HW + LPIPS_WG_PIX - 1) / LPIPS_WG_PIX;
    if (groups > 2147483647L) return PESR_EINVAL;
    if (!ws || ws_bytes < (size_t)N * (size_t)groups * sizeof(double)) return PESR_EWORKSPACE;
    const dim3 grid((unsigned)groups, (unsigned)N), block(LPIPS_THREADS);
    double* part = (double*)ws;
    lpips_dispatch_c(C, [&](auto c) { hipLaunchKernelGGL(lpips_layer_kernel<c()>, grid, block, 0, stream, fa, fb, w, part, map, HW); });
    return pesr_mean_partials_launch(part, out, N, groups, (double)HW, stream);
}

// [a; b] in one tensor: b's features start N * H * W * C floats behind a's, a multiple of 256 bytes
int pesr_lpips_layer_launch(const float* feat, const float* w, double* out, int N, int H, int W, int C, double* map, void* ws,
                            size_t ws_bytes, hipStream_t stream) {
    if (!feat || !lpips_shape_ok(N, H, W, C)) return PESR_EINVAL;
    return pesr_lpips_layer2_launch(feat, feat + (size_t)N * H * W * C, w, out, N, H, W, C, map, ws, ws_bytes, stream);
}

int pesr_lpips_layer_bwd_launch(const float* fa, const float* fb, const float* w, const double* g, float* ga, int N, int H, int W, int C,
                                hipStream_t stream) {
    if (!fa || !fb || !w || !g || !ga || !lpips_shape_ok(N, H, W, C)) return PESR_EINVAL;
    if (((uintptr_t)fa & 15) || ((uintptr_t)fb & 15) || ((uintptr_t)ga & 15) || ((uintptr_t)w & 3) || ((uintptr_t)g & 7))
        return PESR_EINVAL;                                         // the vector loads and stores need each tensor's base on 16 bytes
    const long HW = (long)H * W;
    const long groups = (HW + LPIPS_WG_PIX - 1) / LPIPS_WG_PIX;
    if (groups > 2147483647L) return PESR_EINVAL;
    const dim3 grid((unsigned)groups, (unsigned)N), block(LPIPS_THREADS);
    lpips_dispatch_c(C, [&](auto c) { hipLaunchKernelGGL(lpips_layer_bwd_kernel<c()>, grid, block, 0, stream, fa, fb, w, g, ga, HW); });
    return pesr_launch_status();
}
