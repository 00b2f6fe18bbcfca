// Contextual loss (docs/modes.md section 4r): CX of two NHWC feature maps, as P = H W points of C channels per image.  fp32 in, fp32
// MFMA for the two GEMMs (mfma_f32.h: its layout, the padded staging, the backward's tiles), double for the sums that decide the value.
// No atomics anywhere, every reduction in a fixed order: the same call gives the same bits every time.  All offsets are 64-bit: D is [N][P][P].
//
//   normalise   mu[n][c] = the mean of the hr points (double sum: rows s, s + 16, ... per wave s, the 16 waves in order; one rounding),
//               xb = x - mu, r = (float)(1 / sqrt(sum_c xb^2 + 1e-12)) with the sum in double (wave_sum_d's tree), xh = xb r; one wave
//               per point.  r of the sr points is kept for the backward.
//   distance    one workgroup of 4 waves per 64 rows i of one image.  Its xh rows stay in LDS ([64][C + 1], the padded staging: the MFMA
//               operand has the point on the lane), yh is staged in pieces of 64 columns the same way (the next
//               piece's global loads are issued before this piece's MFMAs); wave w owns the 32 x 32 tile (w & 1, w >> 1) of the piece,
//               C / 2 MFMAs.  D = fma(-0.5, s, 0.5) (one rounding) is stored, and every lane keeps the least value and its column of
//               its 16 rows as it goes (strict <, columns ascending: the lowest column wins among equals); at the end 32 lanes and
//               the two column halves are merged with the same rule.
//   rows        per 64 rows: S_i = sum_k w_ik (double: a lane adds columns lane, lane + 64, ... then wave_sum_d's tree), then per
//               column the largest c_ij = w_ij (1 / S_i) over the block's rows in ascending i (strict >) -> workspace [row blocks][P].
//   reduce      per image: the blocks' maxima in ascending block order (strict >) -> max_i c_ij, a(j); CX = (sum_j max) / P in double
//               (a lane adds columns tid, tid + 256, ...; block_sum_d), L = -log CX.
//   backward    two per-row scalars (one wave per row): T_i = sum of max_j over the columns j with a(j) = i, and
//               U_i = sum_k c_ik ([a(k) = i] - T_i) d_ik / (h (m_i + eps)^2), both double in the order of S_i.  Then per 64 rows (32 at
//               C = 256) E = dL/dD is formed from D while it is staged as the MFMA operand ([rows][64 + 1] in LDS),
//               E_ik = q (-c_ik ([a(k) = i] - T_i) / (h (m_i + eps)) + [k = b(i)] U_i), q = -gL / (P CX); the other operand is yh with
//               the channel on the lane, read coalesced from global (L2).  g_xh = -E yh / 2 goes through LDS once for the per-point
//               projection (g_xh - xh (xh . g_xh)) r.  Not masked by x > 0: the tap's own conv does that.
#include "mfma_f32.h"

constexpr int CX_THREADS = 256;
constexpr int CX_MEAN_THREADS = 1024;
constexpr int CX_ROWS = 64;               // rows of one workgroup of the distance and the row kernels
constexpr int CX_COLS = 64;               // columns of one staged piece
constexpr int CX_MAX_P = 4096;
constexpr float CX_EPS = 1e-5f;

// w_ik from d_ik: the same operations wherever it is needed, so the same bits
__device__ __forceinline__ float cx_weight(float d, float rinv, float hinv) { return expf(fmaf(-d, rinv, 1.0f) * hinv); }

// grid (C / 64, N), 16 waves: wave s adds the rows s, s + 16, ... of its 64 channels, then the 16 partial sums are added in order
__global__ __launch_bounds__(CX_MEAN_THREADS) void cx_mean_kernel(const float* __restrict__ fb, float* __restrict__ mu, int P, int C) {
    constexpr int W = CX_MEAN_THREADS / 64;
    __shared__ double part[W][64];
    const int tid = threadIdx.x, l = tid & 63, s = tid >> 6, c = blockIdx.x * 64 + l;
    const float* f = fb + (long)blockIdx.y * P * C + c;
    double acc = 0.0;
#pragma unroll 8
    for (int j = s; j < P; j += W) acc += (double)f[(long)j * C];
    part[s][l] = acc;
    __syncthreads();
    if (s == 0) {
        double t = part[0][l];
#pragma unroll
        for (int w = 1; w < W; ++w) t += part[w][l];
        mu[(long)blockIdx.y * C + c] = (float)(t / (double)P);
    }
}

// one wave per point; points 0 .. NP - 1 are fa's, NP .. 2 NP - 1 are fb's
template <int C>
__global__ __launch_bounds__(CX_THREADS) void cx_normalize_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                                  const float* __restrict__ mu, float* __restrict__ xh,
                                                                  float* __restrict__ yh, float* __restrict__ inv, int P, long NP) {
    constexpr int V = C / 64;
    const int lane = threadIdx.x & 63;
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= 2 * NP) return;
    const bool hr = q >= NP;
    const long pt = hr ? q - NP : q;
    const float* src = (hr ? fb : fa) + pt * C;
    float* dst = (hr ? yh : xh) + pt * C;
    const float* m = mu + (pt / P) * C;
    float v[V];
    double ss = 0.0;
#pragma unroll
    for (int u = 0; u < V; ++u) {
        v[u] = src[u * 64 + lane] - m[u * 64 + lane];
        ss += (double)v[u] * (double)v[u];
    }
    ss = wave_sum_d(ss);
    const float r = (float)(1.0 / sqrt(ss + 1e-12));
#pragma unroll
    for (int u = 0; u < V; ++u) dst[u * 64 + lane] = v[u] * r;
    if (!hr && lane == 0) inv[pt] = r;
}

// grid (row blocks, N); dynamic LDS 2 * 64 * (C + 1) floats
template <int C>
__global__ __launch_bounds__(CX_THREADS) void cx_dist_kernel(const float* __restrict__ xh, const float* __restrict__ yh,
                                                             float* __restrict__ D, float* __restrict__ m, int* __restrict__ b, int P) {
    constexpr int LD = C + 1, LOADS = CX_ROWS * C / (CX_THREADS * 4);
    extern __shared__ __attribute__((aligned(16))) float cx_lds[];
    float* xs = cx_lds;
    float* ys = cx_lds + CX_ROWS * LD;
    __shared__ float cand_v[2][CX_ROWS];
    __shared__ int cand_i[2][CX_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rh = wave & 1, ch = wave >> 1;
    const int i0 = blockIdx.x * CX_ROWS;
    const long img = (long)blockIdx.y * P;
    const float* xn = xh + img * C;
    const float* yn = yh + img * C;
    float* Dn = D + img * P;

    // rows r0 .. r0 + 63 of an image's points, zeros past P
    const auto rows = [=](const float* pts, int r0) {
        return [=](int r, const float*& src) { return src = pts + (long)(r0 + r) * C, r0 + r < P; };
    };
    f32x4 v[LOADS];
    mfma32_stage_load<C, CX_THREADS>(v, tid, rows(xn, i0));
    mfma32_stage_store<C, CX_THREADS>(xs, v, tid);
    mfma32_stage_load<C, CX_THREADS>(v, tid, rows(yn, 0));

    float best[16];
    int bidx[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) best[r] = __builtin_inff(), bidx[r] = 0;
    const float* a = xs + (rh * 32 + (lane & 31)) * LD + (lane >> 5);
    const float* bb = ys + (ch * 32 + (lane & 31)) * LD + (lane >> 5);

    for (int j0 = 0; j0 < P; j0 += CX_COLS) {
        mfma32_stage_store<C, CX_THREADS>(ys, v, tid);
        __syncthreads();
        if (j0 + CX_COLS < P) mfma32_stage_load<C, CX_THREADS>(v, tid, rows(yn, j0 + CX_COLS));
        f32x16 acc;
        mfma32_zero(acc);
#pragma unroll 8
        for (int kk = 0; kk < C; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], bb[kk], acc, 0, 0, 0);
        const int j = j0 + ch * 32 + (lane & 31);
        if (j < P) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = mfma32_row(r, lane, i0 + rh * 32);
                const float d = fmaf(-0.5f, acc[r], 0.5f);
                if (i < P) {
                    Dn[(long)i * P + j] = d;
                    if (d < best[r]) best[r] = d, bidx[r] = j;
                }
            }
        }
        __syncthreads();
    }

    // the 32 lanes of a half-wave hold 32 columns' candidates of the same 16 rows
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) {
            const float ov = __shfl_xor(best[r], off, 64);
            const int oi = __shfl_xor(bidx[r], off, 64);
            if (ov < best[r] || (ov == best[r] && oi < bidx[r])) best[r] = ov, bidx[r] = oi;
        }
        if ((lane & 31) == 0) {
            const int rr = mfma32_row(r, lane, rh * 32);
            cand_v[ch][rr] = best[r];
            cand_i[ch][rr] = bidx[r];
        }
    }
    __syncthreads();
    if (tid < CX_ROWS && i0 + tid < P) {
        float bv = cand_v[0][tid];
        int bi = cand_i[0][tid];
        if (cand_v[1][tid] < bv || (cand_v[1][tid] == bv && cand_i[1][tid] < bi)) bv = cand_v[1][tid], bi = cand_i[1][tid];
        m[img + i0 + tid] = bv;
        b[img + i0 + tid] = bi;
    }
}

// grid (row blocks, N)
__global__ __launch_bounds__(CX_THREADS) void cx_rows_kernel(const float* __restrict__ D, const float* __restrict__ m,
                                                             float* __restrict__ S, float* __restrict__ wv, int* __restrict__ wi, int P,
                                                             float hinv) {
    __shared__ float s_rinv[CX_ROWS], s_sinv[CX_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * CX_ROWS, rows = min(CX_ROWS, P - i0);
    const long img = (long)blockIdx.y * P;
    const float* Dn = D + img * P;
    for (int rr = wave; rr < rows; rr += 4) {
        const float* row = Dn + (long)(i0 + rr) * P;
        const float rinv = 1.0f / (m[img + i0 + rr] + CX_EPS);
        double acc = 0.0;
#pragma unroll 8
        for (int k = lane; k < P; k += 64) acc += (double)cx_weight(row[k], rinv, hinv);
        const float s = (float)wave_sum_d(acc);
        if (lane == 0) {
            S[img + i0 + rr] = s;
            s_rinv[rr] = rinv;
            s_sinv[rr] = 1.0f / s;
        }
    }
    __syncthreads();
    const long o = ((long)blockIdx.y * gridDim.x + blockIdx.x) * P;
    for (int j = tid; j < P; j += CX_THREADS) {
        float bv = -1.0f;
        int bi = i0;
#pragma unroll 8
        for (int rr = 0; rr < rows; ++rr) {
            const float c = cx_weight(Dn[(long)(i0 + rr) * P + j], s_rinv[rr], hinv) * s_sinv[rr];
            if (c > bv) bv = c, bi = i0 + rr;
        }
        wv[o + j] = bv;
        wi[o + j] = bi;
    }
}

// grid N
__global__ __launch_bounds__(CX_THREADS) void cx_reduce_kernel(const float* __restrict__ wv, const int* __restrict__ wi,
                                                               float* __restrict__ M, int* __restrict__ a, double* __restrict__ CX,
                                                               double* __restrict__ L, int P, int RB) {
    __shared__ double red[CX_THREADS / 64];
    const int tid = threadIdx.x;
    const long img = (long)blockIdx.x * P, w0 = (long)blockIdx.x * RB * P;
    double acc = 0.0;
    for (int j = tid; j < P; j += CX_THREADS) {
        float bv = wv[w0 + j];
        int bi = wi[w0 + j];
        for (int rb = 1; rb < RB; ++rb) {
            const float c = wv[w0 + (long)rb * P + j];
            if (c > bv) bv = c, bi = wi[w0 + (long)rb * P + j];
        }
        M[img + j] = bv;
        a[img + j] = bi;
        acc += (double)bv;
    }
    const double tot = block_sum_d(acc, red);
    if (tid == 0) {
        const double cx = tot / (double)P;
        CX[blockIdx.x] = cx;
        L[blockIdx.x] = -log(cx);
    }
}

// grid (ceil(P / 4), N): one wave per row -> rows[n][i] = {T_i, U_i}
__global__ __launch_bounds__(CX_THREADS) void cx_bwd_rows_kernel(const float* __restrict__ D, const float* __restrict__ m,
                                                                 const float* __restrict__ S, const int* __restrict__ a,
                                                                 const float* __restrict__ M, float* __restrict__ rows, int P, float hinv) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= P) return;
    const long img = (long)blockIdx.y * P;
    const int* an = a + img;
    double t = 0.0;
#pragma unroll 8
    for (int k = lane; k < P; k += 64)
        if (an[k] == i) t += (double)M[img + k];
    const float T = (float)wave_sum_d(t);
    const float rinv = 1.0f / (m[img + i] + CX_EPS), sinv = 1.0f / S[img + i];
    const float* row = D + (img + i) * P;
    double u = 0.0;
#pragma unroll 8
    for (int k = lane; k < P; k += 64) {
        const float d = row[k];
        const float g = cx_weight(d, rinv, hinv) * sinv * ((an[k] == i ? 1.0f : 0.0f) - T);
        u += (double)g * (double)d;
    }
    u = wave_sum_d(u);
    if (lane == 0) {
        rows[(img + i) * 2] = T;
        rows[(img + i) * 2 + 1] = (float)u * (hinv * rinv * rinv);
    }
}

// grid (ceil(P / PIX), N)
template <int C>
__global__ __launch_bounds__(CX_THREADS) void cx_bwd_kernel(const float* __restrict__ D, const float* __restrict__ m,
                                                            const int* __restrict__ b, const float* __restrict__ S,
                                                            const int* __restrict__ a, const double* __restrict__ CX,
                                                            const double* __restrict__ gL, const float* __restrict__ xh,
                                                            const float* __restrict__ yh, const float* __restrict__ inv,
                                                            const float* __restrict__ rows, float* __restrict__ gf,
                                                            float* __restrict__ e_out, float* __restrict__ gxh_out, int P, float hinv) {
    using Tl = Mfma32Bwd<C>;
    constexpr int PIX = Tl::PIX, LE = CX_COLS + 1, LG = C + 1, V = C / 64;
    __shared__ float es[PIX * LE];
    __shared__ float gs[PIX * LG];
    __shared__ float p_k[PIX], p_sinv[PIX], p_T[PIX], p_U[PIX];
    __shared__ int p_b[PIX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * PIX, n = blockIdx.y, nrows = min(PIX, P - i0);
    const long img = (long)n * P;
    const float q = (float)(-gL[n] / ((double)P * CX[n]));
    if (q == 0.0f) {                                                   // gL[n] = 0: an all-zero image, whatever the rest holds
        for (int e = tid; e < nrows * C; e += CX_THREADS) gf[(img + i0) * C + e] = 0.0f;
        if (gxh_out)
            for (int e = tid; e < nrows * C; e += CX_THREADS) gxh_out[(img + i0) * C + e] = 0.0f;
        if (e_out)
            for (long e = tid; e < (long)nrows * P; e += CX_THREADS) e_out[(img + i0) * P + e] = 0.0f;
        return;
    }
    if (tid < PIX) {
        const bool ok = tid < nrows;
        const long r = img + i0 + (ok ? tid : 0);
        const float rinv = 1.0f / (m[r] + CX_EPS);
        p_k[tid] = rinv;
        p_sinv[tid] = 1.0f / S[r];
        p_T[tid] = rows[r * 2];
        p_U[tid] = rows[r * 2 + 1];
        p_b[tid] = b[r];
    }
    __syncthreads();

    const int half = Tl::half(wave);
    f32x16 acc[Tl::TPW];
    mfma32_zero(acc);
    const float* ap = es + (half * 32 + (lane & 31)) * LE + (lane >> 5);
    const float* yn = yh + img * C + (lane & 31);

    for (int j0 = 0; j0 < P; j0 += CX_COLS) {
#pragma unroll
        for (int it = 0; it < PIX * CX_COLS / CX_THREADS; ++it) {
            const int e = it * CX_THREADS + tid, rr = e / CX_COLS, kk = e % CX_COLS, k = j0 + kk;
            float val = 0.0f;
            if (rr < nrows && k < P) {
                const int i = i0 + rr;
                const float c = cx_weight(D[(img + i) * P + k], p_k[rr], hinv) * p_sinv[rr];
                const float dense = -(hinv * p_k[rr]) * (c * ((a[img + k] == i ? 1.0f : 0.0f) - p_T[rr]));
                val = q * (k == p_b[rr] ? dense + p_U[rr] : dense);
                if (e_out) e_out[(img + i) * P + k] = val;
            }
            es[rr * LE + kk] = val;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < CX_COLS; kk += 2) {
            const float av = ap[kk];
            const int jj = min(j0 + kk + (lane >> 5), P - 1);          // (past P the other operand is 0)
            const float* bp = yn + (long)jj * C;
#pragma unroll
            for (int u = 0; u < Tl::TPW; ++u)
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[Tl::band(wave, u) * 32], acc[u], 0, 0, 0);
        }
        __syncthreads();
    }

#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rr = half * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);      // mfma32_row, written out: see mfma_f32.h
#pragma unroll
        for (int u = 0; u < Tl::TPW; ++u) gs[rr * LG + Tl::band(wave, u) * 32 + (lane & 31)] = -0.5f * acc[u][r];
    }
    __syncthreads();
    for (int rr = wave; rr < nrows; rr += 4) {
        const long pt = img + i0 + rr;
        float x[V], g[V], dot = 0.0f;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            x[u] = xh[pt * C + u * 64 + lane];
            g[u] = gs[rr * LG + u * 64 + lane];
            dot = fmaf(x[u], g[u], dot);
        }
        dot = wave_sum(dot);
        const float r = inv[pt];
#pragma unroll
        for (int u = 0; u < V; ++u) {
            gf[pt * C + u * 64 + lane] = fmaf(-x[u], dot, g[u]) * r;
            if (gxh_out) gxh_out[pt * C + u * 64 + lane] = g[u];
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static bool cx_shape_ok(int N, int P, int C) {
    return N >= 1 && N <= 65535 && P >= 1 && P <= CX_MAX_P && mfma32_c_ok(C);
}

int pesr_cx_row_blocks_host(int N, int P, int C) { return cx_shape_ok(N, P, C) ? (P + CX_ROWS - 1) / CX_ROWS : 0; }

int pesr_cx_col_pieces_host(int N, int P, int C) { return cx_shape_ok(N, P, C) ? (P + CX_COLS - 1) / CX_COLS : 0; }

// the row blocks' column maxima (a float and an int per column); the backward's two floats per row fit in it
size_t pesr_cx_workspace_bytes_host(int N, int P, int C) {
    if (!cx_shape_ok(N, P, C)) return 0;
    return (size_t)N * ((P + CX_ROWS - 1) / CX_ROWS) * P * (sizeof(float) + sizeof(int));
}

// what a forward keeps for its backward: xh, yh, D, six values per point (r, m, b, S, a, max) and CX
size_t pesr_cx_saved_bytes_host(int N, int P, int C) {
    if (!cx_shape_ok(N, P, C)) return 0;
    return (size_t)N * P * ((size_t)2 * C + P + 6) * sizeof(float) + (size_t)N * sizeof(double);
}

int pesr_cx_normalize_launch(const float* fa, const float* fb, float* mu, float* xh, float* yh, float* inv, int N, int P, int C,
                             hipStream_t stream) {
    if (!cx_shape_ok(N, P, C) || !fa || !fb || !mu || !xh || !yh || !inv) return PESR_EINVAL;
    if ((((uintptr_t)fa | (uintptr_t)fb | (uintptr_t)xh | (uintptr_t)yh) & 15) || (((uintptr_t)mu | (uintptr_t)inv) & 3)) return PESR_EINVAL;
    const long NP = (long)N * P;
    hipLaunchKernelGGL(cx_mean_kernel, dim3(C / 64, N), dim3(CX_MEAN_THREADS), 0, stream, fb, mu, P, C);
    const dim3 grid((unsigned)((2 * NP + 3) / 4)), block(CX_THREADS);
    mfma32_dispatch_c(C, [&](auto c) {
        hipLaunchKernelGGL(cx_normalize_kernel<c()>, grid, block, 0, stream, fa, fb, (const float*)mu, xh, yh, inv, P, NP);
    });
    return pesr_launch_status();
}

int pesr_cx_dist_launch(const float* xh, const float* yh, float* D, float* m, int* b, int N, int P, int C, hipStream_t stream) {
    if (!cx_shape_ok(N, P, C) || !xh || !yh || !D || !m || !b) return PESR_EINVAL;
    if ((((uintptr_t)xh | (uintptr_t)yh) & 15) || (((uintptr_t)D | (uintptr_t)m | (uintptr_t)b) & 3)) return PESR_EINVAL;
    // the dynamic part only: the kernel has 1 KB of static LDS besides, and the two together must fit in the 160 KB
    static PesrDeviceOnce once;
    hipError_t attr = hipSuccess;
    once([&] {
        for (int ci : {64, 128, 256})
            mfma32_dispatch_c(ci, [&](auto c) {
                if (attr == hipSuccess)
                    attr = hipFuncSetAttribute((const void*)cx_dist_kernel<c()>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               2 * CX_ROWS * (c() + 1) * 4);
            });
    });
    if (attr != hipSuccess) return (int)attr;
    const dim3 grid((P + CX_ROWS - 1) / CX_ROWS, N), block(CX_THREADS);
    const size_t lds = (size_t)2 * CX_ROWS * (C + 1) * sizeof(float);
    mfma32_dispatch_c(C, [&](auto c) { hipLaunchKernelGGL(cx_dist_kernel<c()>, grid, block, lds, stream, xh, yh, D, m, b, P); });
    return pesr_launch_status();
}

int pesr_cx_fwd_launch(const float* D, const float* m, double h, float* S, int* a, float* M, double* CX, double* L, int N, int P, int C,
                       void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!cx_shape_ok(N, P, C) || !D || !m || !S || !a || !M || !CX || !L || !(h > 0.0)) return PESR_EINVAL;
    if ((((uintptr_t)D | (uintptr_t)m | (uintptr_t)S | (uintptr_t)a | (uintptr_t)M | (uintptr_t)ws) & 3) || (((uintptr_t)CX | (uintptr_t)L) & 7))
        return PESR_EINVAL;
    if (!ws || ws_bytes < pesr_cx_workspace_bytes_host(N, P, C)) return PESR_EWORKSPACE;
    const int RB = (P + CX_ROWS - 1) / CX_ROWS;
    float* wv = (float*)ws;
    int* wi = (int*)(wv + (size_t)N * RB * P);
    const float hinv = (float)(1.0 / h);
    hipLaunchKernelGGL(cx_rows_kernel, dim3(RB, N), dim3(CX_THREADS), 0, stream, D, m, S, wv, wi, P, hinv);
    hipLaunchKernelGGL(cx_reduce_kernel, dim3(N), dim3(CX_THREADS), 0, stream, (const float*)wv, (const int*)wi, M, a, CX, L, P, RB);
    return pesr_launch_status();
}

int pesr_cx_bwd_launch(const float* D, const float* m, const int* b, const float* S, const int* a, const float* M, const double* CX,
                       const double* gL, const float* xh, const float* yh, const float* inv, double h, float* gf, float* e_out,
                       float* gxh_out, int N, int P, int C, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!cx_shape_ok(N, P, C) || !D || !m || !b || !S || !a || !M || !CX || !gL || !xh || !yh || !inv || !gf || !(h > 0.0)) return PESR_EINVAL;
    if ((((uintptr_t)xh | (uintptr_t)yh | (uintptr_t)gf) & 15) || (((uintptr_t)CX | (uintptr_t)gL) & 7)) return PESR_EINVAL;
    if (((uintptr_t)D | (uintptr_t)m | (uintptr_t)b | (uintptr_t)S | (uintptr_t)a | (uintptr_t)M | (uintptr_t)inv | (uintptr_t)e_out |
         (uintptr_t)gxh_out | (uintptr_t)ws) & 3)
        return PESR_EINVAL;
    if (!ws || ws_bytes < pesr_cx_workspace_bytes_host(N, P, C)) return PESR_EWORKSPACE;
    float* rows = (float*)ws;                                          // [N][P][2] <= the forward's workspace
    const float hinv = (float)(1.0 / h);
    hipLaunchKernelGGL(cx_bwd_rows_kernel, dim3((P + 3) / 4, N), dim3(CX_THREADS), 0, stream, D, m, S, a, M, rows, P, hinv);
    mfma32_dispatch_c(C, [&](auto c) {
        constexpr int pix = Mfma32Bwd<c()>::PIX;
        hipLaunchKernelGGL(cx_bwd_kernel<c()>, dim3((P + pix - 1) / pix, N), dim3(CX_THREADS), 0, stream, D, m, b, S, a, CX, gL, xh, yh, inv,
                           (const float*)rows, gf, e_out, gxh_out, P, hinv);
    });
    return pesr_launch_status();
}
