// Texture loss (docs/modes.md section 4q): patch-wise Gram matrices of NHWC feature maps, the squared distance of two of them, and
// the gradient with respect to the features.  fp32 in, fp32 MFMA (mfma_f32.h: its layout, the padded staging, the backward's tiles),
// fp32 out; the distance in double.  No atomics anywhere: the same call gives the same bits every time.
//
// F [N][H][W][C], patches of ph x pw pixels (ph | H, pw | W), P = (H / ph) (W / pw) of them per image, K = ph pw pixels each; pixel k
// of a patch is row k / pw, column k % pw of it.  s = 1 / (C K).
//
// Forward, G[n][p][c][c'] = s sum_k F[k][c] F[k][c']: one workgroup of 4 waves per (image, patch, K slice).  The slice's rows are
// staged 32 KB at a time ([8192 / C pixels][C], 16-byte loads, channels contiguous, rows past the slice zero - so any K works, odd
// ones too); both MFMA operands of a 32 x 32 output tile are one ds_read_b32 per lane from that image (lane l: row 2 step + l / 32,
// channel 32 tile + l % 32: the two half-waves read two rows, 32 consecutive banks each, no padding needed).  Only the
// T (T + 1) / 2 tiles with ti <= tj are computed (T = C / 32: 3, 10, 36 tiles, dealt round-robin to the waves: 1, 3, 3 accumulators, the
// 36 tiles of C = 256 as three workgroups of 12);
// the epilogue stores element (r, c), r <= c, and the same register to (c, r), so G is symmetric by construction.
// Split-K: a whole-map Gram is few, long GEMMs (N of them), so `gram_splits` cuts K into up to 64 slices of at least 256 pixels while
// that helps to reach 1024 workgroups; slice j writes its unscaled sums to slab j of the workspace ([S][N P][C][C]) and
// gram_finish_kernel adds the slabs in ascending j and scales once.  Without a split the kernel scales and writes G itself.
//
// Distance: d = (double)Gsr - (double)Ghr (exact), dG = (float)d (one rounding; written only when asked for), t[n] = (sum d^2) / P
// in double: a lane adds its elements in ascending address order, wave_sum_d's tree, the four waves in order, one partial per
// workgroup (block_sum_d); reduce.hip's mean_partials_kernel adds an image's partials in its fixed order and divides by P.
//
// Backward, gF[k][c] = (float)(g[n] 4 s / P) * sum_c' F[k][c'] dG[c'][c]: one workgroup per (image, patch, run of 64 pixels; 32 at
// C = 256: Mfma32Bwd).  The operand indexed [pixel][c'] has its pixel on the lane, which memory does not give contiguously: the run's
// rows go through the padded staging of mfma_f32.h.  The other operand is dG[c'][c] with c on the lane, read coalesced from global
// (L2: a patch's dG is read by all its pixel runs).  Not masked by F > 0: the tap's own conv does that.
#include "mfma_f32.h"

constexpr int GR_THREADS = 256;
constexpr int GR_CHUNK = 8192;            // floats of one staged piece of the forward: 32 KB
constexpr int GR_MIN_SLICE = 256;         // split-K: no slice shorter than this many pixels
constexpr int GR_MAX_SPLITS = 64;
constexpr long GR_TARGET_WGS = 1024;      // split-K: stop splitting once the launch has this many workgroups

// (ti, tj) of the id-th tile of the upper triangle, rows in order
__device__ __forceinline__ void gram_tile(int id, int T, int& ti, int& tj) {
    int i = 0;
    while (id >= T - i) { id -= T - i; ++i; }
    ti = i, tj = i + id;
}

// grid.x = N * P * S: block b is slice b % S of patch b / S; grid.y = TG: the upper triangle's tiles in TG equal groups, one workgroup
// each (C = 256: 3 groups of 12 tiles, 3 per wave - one group of 36 needs 234 VGPRs and leaves a patch-of-16 launch at the training
// shape with 144 workgroups for 256 CUs).  out: G (S == 1, scale = s) or the workspace (scale = 1)
template <int C, int TG>
__global__ __launch_bounds__(GR_THREADS) void gram_fwd_kernel(const float* __restrict__ F, float* __restrict__ out, int H, int W, int ph,
                                                              int pw, int npx, int P, int K, int Ks, int S, long NP, float scale) {
    constexpr int T = C / 32, U = T * (T + 1) / 2 / TG, TPW = (U + 3) / 4, KC = GR_CHUNK / C;
    static_assert(T * (T + 1) / 2 % TG == 0, "equal groups");
    __shared__ float lds[GR_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int split = (int)(blockIdx.x % (unsigned)S);
    const long np = blockIdx.x / (unsigned)S;
    const int n = (int)(np / P), p = (int)(np % P);
    const int py = p / npx, px = p % npx;
    const int k0 = split * Ks, k1 = min(K, k0 + Ks);
    const float* base = F + (((long)n * H + (long)py * ph) * W + (long)px * pw) * C;

    int ti[TPW], tj[TPW];
    f32x16 acc[TPW];
    mfma32_zero(acc);
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        ti[u] = tj[u] = 0;
        if (wave + 4 * u < U) gram_tile(blockIdx.y * U + wave + 4 * u, T, ti[u], tj[u]);
    }

    for (int kc = k0; kc < k1; kc += KC) {
        f32x4 v[GR_CHUNK / (GR_THREADS * 4)];
#pragma unroll
        for (int it = 0; it < GR_CHUNK / (GR_THREADS * 4); ++it) {
            const int e = (it * GR_THREADS + tid) * 4;
            const int k = kc + e / C, c = e % C;
            v[it] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (k < k1) {
                const int r = k / pw, q = k - r * pw;
                v[it] = *(const f32x4*)(base + ((long)r * W + q) * C + c);
            }
        }
#pragma unroll
        for (int it = 0; it < GR_CHUNK / (GR_THREADS * 4); ++it) *(f32x4*)(lds + (it * GR_THREADS + tid) * 4) = v[it];
        __syncthreads();
        const int steps = (min(KC, k1 - kc) + 1) / 2;                  // (an odd count ends on a zero row)
        const float* row = lds + (lane >> 5) * C + (lane & 31);
        for (int s = 0; s < steps; ++s, row += 2 * C) {
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                if (wave + 4 * u < U) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(row[ti[u] * 32], row[tj[u] * 32], acc[u], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    float* o = out + ((S == 1 ? 0 : (long)split * NP) + np) * ((long)C * C);
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        if (wave + 4 * u < U) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gr = mfma32_row(r, lane, ti[u] * 32), gc = tj[u] * 32 + (lane & 31);
                const float val = acc[u][r] * scale;
                if (gr <= gc) {
                    o[gr * C + gc] = val;
                    if (gr < gc) o[gc * C + gr] = val;
                }
            }
        }
    }
}

// G = s * (slab 0 + slab 1 + ... in this order); total = N P C C elements, a multiple of 4
__global__ __launch_bounds__(GR_THREADS) void gram_finish_kernel(const float* __restrict__ ws, float* __restrict__ G, long total, int S,
                                                                 float scale) {
    const long e = ((long)blockIdx.x * GR_THREADS + threadIdx.x) * 4;
    if (e >= total) return;
    f32x4 s = *(const f32x4*)(ws + e);
    for (int j = 1; j < S; ++j) s += *(const f32x4*)(ws + (long)j * total + e);
    *(f32x4*)(G + e) = s * scale;
}

// grid (nb, N): block b of image n takes the float4 groups b * 256 + t, + nb * 256, ... of the image's `per` elements
__global__ __launch_bounds__(GR_THREADS) void gram_loss_kernel(const float* __restrict__ ga, const float* __restrict__ gb,
                                                               float* __restrict__ dg, double* __restrict__ part, long per) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const long img = (long)blockIdx.y * per;
    double s = 0.0;
    for (long e = ((long)blockIdx.x * GR_THREADS + tid) * 4; e < per; e += (long)gridDim.x * GR_THREADS * 4) {
        const f32x4 a = *(const f32x4*)(ga + img + e), b = *(const f32x4*)(gb + img + e);
        f32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double d = (double)a[i] - (double)b[i];
            s += d * d;
            o[i] = (float)d;
        }
        if (dg) *(f32x4*)(dg + img + e) = o;
    }
    __shared__ double red[GR_THREADS / 64];
    const double t = block_sum_d(s, red);
    if (tid == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// grid.x = N * P * runs: block b is pixel run b % runs of patch b / runs
template <int C>
__global__ __launch_bounds__(GR_THREADS) void gram_bwd_kernel(const float* __restrict__ F, const float* __restrict__ dG,
                                                              const double* __restrict__ g, float* __restrict__ gF, int H, int W, int ph,
                                                              int pw, int npx, int P, int K, int runs, double coef) {
    using Tl = Mfma32Bwd<C>;
    constexpr int PIX = Tl::PIX, LD = C + 1;
    __shared__ float lds[PIX * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int run = (int)(blockIdx.x % (unsigned)runs);
    const long np = blockIdx.x / (unsigned)runs;
    const int n = (int)(np / P), p = (int)(np % P);
    const int py = p / npx, px = p % npx;
    const int k0 = run * PIX;
    const long origin = (((long)n * H + (long)py * ph) * W + (long)px * pw) * C;

    f32x4 v[PIX * C / (GR_THREADS * 4)];
    mfma32_stage_load<C, GR_THREADS>(v, tid, [&](int row, const float*& src) {
        const int k = k0 + row, r = k / pw, q = k - r * pw;
        return src = F + origin + ((long)r * W + q) * C, k < K;
    });
    mfma32_stage_store<C, GR_THREADS>(lds, v, tid);
    __syncthreads();

    const int half = Tl::half(wave);
    f32x16 acc[Tl::TPW];
    mfma32_zero(acc);
    const float* a = lds + (half * 32 + (lane & 31)) * LD + (lane >> 5);
    const float* b = dG + np * ((long)C * C) + (long)(lane >> 5) * C + (lane & 31);
#pragma unroll 8
    for (int kk = 0; kk < C; kk += 2) {
        const float av = a[kk];
#pragma unroll
        for (int u = 0; u < Tl::TPW; ++u)
            acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[(long)kk * C + Tl::band(wave, u) * 32], acc[u], 0, 0, 0);
    }

    const float cf = (float)(g[n] * coef);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int k = mfma32_row(r, lane, k0 + half * 32);
        if (k < K) {
            const int rr = k / pw, q = k - rr * pw;
            float* o = gF + origin + ((long)rr * W + q) * C + (lane & 31);
#pragma unroll
            for (int u = 0; u < Tl::TPW; ++u) o[Tl::band(wave, u) * 32] = acc[u][r] * cf;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct GramPlan {
    int P, npx, K, S, Ks;
    long NP;
};

// the shape checks all entry points share; fills the plan
static int gram_plan(int N, int H, int W, int C, int ph, int pw, GramPlan* pl) {
    if (N < 1 || H < 1 || W < 1 || ph < 1 || pw < 1 || ph > H || pw > W || H % ph || W % pw) return PESR_EINVAL;
    if (!mfma32_c_ok(C)) return PESR_EINVAL;
    const long hw = (long)H * W;
    if (hw > (1L << 30)) return PESR_EINVAL;
    pl->npx = W / pw;
    pl->P = (int)(hw / ((long)ph * pw));
    pl->K = ph * pw;
    pl->NP = (long)N * pl->P;
    long s = pl->K / GR_MIN_SLICE;
    if (s > GR_TARGET_WGS / pl->NP) s = GR_TARGET_WGS / pl->NP;
    if (s > GR_MAX_SPLITS) s = GR_MAX_SPLITS;
    if (s < 1) s = 1;
    pl->Ks = (int)(((pl->K + s - 1) / s + 3) / 4 * 4);
    pl->S = (pl->K + pl->Ks - 1) / pl->Ks;                             // (no empty slice)
    if (pl->NP * pl->S > 0x7fffffffL || pl->NP * ((pl->K + 31) / 32) > 0x7fffffffL) return PESR_EINVAL;
    return PESR_OK;
}

int pesr_gram_splits_host(int N, int H, int W, int C, int ph, int pw) {
    GramPlan pl;
    return gram_plan(N, H, W, C, ph, pw, &pl) == PESR_OK ? pl.S : 0;
}

size_t pesr_gram_workspace_bytes_host(int N, int H, int W, int C, int ph, int pw) {
    GramPlan pl;
    if (gram_plan(N, H, W, C, ph, pw, &pl) != PESR_OK || pl.S == 1) return 0;
    return (size_t)pl.S * (size_t)pl.NP * C * C * sizeof(float);
}

int pesr_gram_fwd_launch(const float* f, float* G, int N, int H, int W, int C, int ph, int pw, void* ws, size_t ws_bytes,
                         hipStream_t stream) {
    GramPlan pl;
    if (!f || !G || gram_plan(N, H, W, C, ph, pw, &pl) != PESR_OK) return PESR_EINVAL;
    if (((uintptr_t)f | (uintptr_t)G | (uintptr_t)ws) & 15) return PESR_EINVAL;
    const long total = pl.NP * C * C;
    if (pl.S > 1 && (!ws || ws_bytes < (size_t)pl.S * total * sizeof(float))) return PESR_EWORKSPACE;
    const float s = (float)(1.0 / ((double)C * pl.K));
    float* out = pl.S > 1 ? (float*)ws : G;
    const float scale = pl.S > 1 ? 1.0f : s;
    const dim3 block(GR_THREADS);
    mfma32_dispatch_c(C, [&](auto c) {
        constexpr int TG = c() == 256 ? 3 : 1;                         // (gram_fwd_kernel's comment)
        hipLaunchKernelGGL((gram_fwd_kernel<c(), TG>), dim3((unsigned)(pl.NP * pl.S), TG), block, 0, stream, f, out, H, W, ph, pw, pl.npx,
                           pl.P, pl.K, pl.Ks, pl.S, pl.NP, scale);
    });
    if (pl.S > 1)
        hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)((total / 4 + GR_THREADS - 1) / GR_THREADS)), block, 0, stream,
                           (const float*)ws, G, total, pl.S, s);
    return pesr_launch_status();
}

// workgroups per image of the distance kernel: 16 float4 groups per lane, at most 1024
static int gram_loss_blocks(long per) {
    const long nb = (per + 16 * GR_THREADS * 4 - 1) / (16 * GR_THREADS * 4);
    return (int)(nb < 1 ? 1 : nb > 1024 ? 1024 : nb);
}

size_t pesr_gram_loss_workspace_bytes_host(int N, int P, int C) {
    if (N < 1 || P < 1 || !mfma32_c_ok(C)) return 0;
    return sizeof(double) * (size_t)N * gram_loss_blocks((long)P * C * C);
}

int pesr_gram_loss_launch(const float* ga, const float* gb, double* t, float* dg, int N, int P, int C, void* ws, size_t ws_bytes,
                          hipStream_t stream) {
    if (!ga || !gb || !t || N < 1 || N > 65535 || P < 1 || !mfma32_c_ok(C)) return PESR_EINVAL;
    if ((long)P * C * C > (1L << 40)) return PESR_EINVAL;
    if ((((uintptr_t)ga | (uintptr_t)gb | (uintptr_t)dg) & 15) || (((uintptr_t)t | (uintptr_t)ws) & 7)) return PESR_EINVAL;
    const long per = (long)P * C * C;
    const int nb = gram_loss_blocks(per);
    if (!ws || ws_bytes < sizeof(double) * (size_t)N * nb) return PESR_EWORKSPACE;
    hipLaunchKernelGGL(gram_loss_kernel, dim3(nb, N), dim3(GR_THREADS), 0, stream, ga, gb, dg, (double*)ws, per);
    return pesr_mean_partials_launch((const double*)ws, t, N, nb, (double)P, stream);
}

int pesr_gram_bwd_launch(const float* f, const float* dg, const double* g, float* gf, int N, int H, int W, int C, int ph, int pw,
                         hipStream_t stream) {
    GramPlan pl;
    if (!f || !dg || !g || !gf || gram_plan(N, H, W, C, ph, pw, &pl) != PESR_OK) return PESR_EINVAL;
    if ((((uintptr_t)f | (uintptr_t)dg | (uintptr_t)gf) & 15) || ((uintptr_t)g & 7)) return PESR_EINVAL;
    const double coef = 4.0 * (1.0 / ((double)C * pl.K)) / pl.P;
    mfma32_dispatch_c(C, [&](auto c) {
        constexpr int pix = Mfma32Bwd<c()>::PIX;
        const int runs = (pl.K + pix - 1) / pix;
        hipLaunchKernelGGL(gram_bwd_kernel<c()>, dim3((unsigned)(pl.NP * runs)), dim3(GR_THREADS), 0, stream, f, dg, g, gf, H, W, ph, pw,
                           pl.npx, pl.P, pl.K, runs, coef);
    });
    return pesr_launch_status();
}
