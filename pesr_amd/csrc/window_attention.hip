// Window self-attention of the Generator's attention blocks (docs/modes.md section 4w), NHWC fp32:
//   qkv [N][H][W][3 D]: channels 0..D-1 q, D..2D-1 k, 2D..3D-1 v; head h owns channels 32h..32h+31 of each.
//   Windows of 8 x 8 pixels on a grid whose origin is (-shift, -shift); positions outside the image are no tokens.
//   Per window and head, over its valid tokens:  S = tau q k^T,  A = softmax_rows(S),  o = A v          -> out [N][H][W][D]
//   backward:  dv = A^T do,  dA = do v^T,  dS = A * (dA - rowsum(dA * A)),  dq = tau dS k,  dk = tau dS^T q   -> dqkv [N][H][W][3 D]
//
// One workgroup of four waves per window, one wave per head (a loop when there are more than four heads).  A wave stages its head's
// 64 x 32 operands into LDS rows of 33 floats (mfma_f32.h's padded staging, tokens outside the image as zeros) and runs every product
// on v_mfma_f32_32x32x2_f32.  S is computed TRANSPOSED, keys on the accumulator's rows and queries on its lanes: a query's softmax
// is then a sum over a lane's own registers and one exchange with lane ^ 32, and the accumulator is as it stands the B operand of
// the next product whenever that sums over keys (o, dq).  The products that sum over queries (dv, dk) take S the other way round,
// recomputed by the same MFMAs with the operands exchanged - the same fmaf chains, so the same bits - with each query's maximum, sum
// and rowsum(dA * A) passed through 3 x 64 floats of LDS.  Neither S nor A ever leaves the registers, the forward leaves no
// statistics and the backward does not read out: with S recomputed in registers they are a few VALU operations, against 9 - 19 MB
// more traffic per call.  (The second orientation is what costs MFMA work: two of the backward's seven products.)
// An accumulator's registers 4g..4g+3 are four consecutive channels of one token: every global access is 16 bytes along the channels.
// No atomics, every element of dqkv written once, summation orders fixed by the shape: the same bits on every run.
#include "mfma_f32.h"

#define WA_WIN 8                  // window side
#define WA_TOK (WA_WIN * WA_WIN)  // tokens per window
#define WA_HD 32                  // head width
#define WA_LDR (WA_HD + 1)        // LDS row stride of a staged operand
#define WA_WAVES 4
#define WA_MAX_D 1024
#define WA_OPER (WA_TOK * WA_LDR) // floats of one staged operand
static constexpr float WA_TAU = 0.17677669529663687f;   // 1 / sqrt(32)

struct WaGeom {
    int H, W, D, shift;
    int wh, ww;           // windows per image along y and x
};

// the window of this workgroup: image, first row and column (may be negative), and the 64-bit mask of its tokens inside the image
struct WaWindow {
    int n, y0, x0;
    unsigned long long valid;
};
__device__ __forceinline__ WaWindow wa_window(const WaGeom& g) {
    const int per = g.wh * g.ww, b = blockIdx.x;
    WaWindow w;
    w.n = b / per;
    const int r = b - w.n * per;
    w.y0 = (r / g.ww) * WA_WIN - g.shift;
    w.x0 = (r % g.ww) * WA_WIN - g.shift;
    unsigned cols = 0;
    for (int i = 0; i < WA_WIN; ++i) cols |= (unsigned)(w.x0 + i >= 0 && w.x0 + i < g.W) << i;
    w.valid = 0;
    for (int i = 0; i < WA_WIN; ++i)
        if (w.y0 + i >= 0 && w.y0 + i < g.H) w.valid |= (unsigned long long)cols << (WA_WIN * i);
    return w;
}
// element offset of token t's pixel, in pixels (64-bit: [4][512][512] pixels x 3 D channels pass 2^31 elements)
__device__ __forceinline__ size_t wa_pixel(const WaGeom& g, const WaWindow& w, int t) {
    return ((size_t)w.n * g.H + (w.y0 + t / WA_WIN)) * g.W + (w.x0 + t % WA_WIN);
}
__device__ __forceinline__ bool wa_is(const WaWindow& w, int t) { return (w.valid >> t) & 1; }

// ---- staging: one head's 64 x 32 block of channels [c0, c0 + 32) of a [pixels][stride] tensor -> LDS [64][33] ----------------------------
typedef f32x4 WaStage[WA_TOK * WA_HD / (64 * 4)];
__device__ __forceinline__ void wa_load(WaStage& v, const float* __restrict__ base, int stride, int c0, const WaGeom& g, const WaWindow& w,
                                        int lane) {
    mfma32_stage_load<WA_HD, 64, WA_TOK * WA_HD / (64 * 4)>(v, lane, [&](int t, const float*& src) {
        if (!wa_is(w, t)) return false;
        src = base + wa_pixel(g, w, t) * stride + c0;
        return true;
    });
}
__device__ __forceinline__ void wa_store(float* lds, const WaStage& v, int lane) {
    mfma32_stage_store<WA_HD, 64, WA_TOK * WA_HD / (64 * 4)>(lds, v, lane);
}

// ---- the three MFMA forms ---------------------------------------------------------------------------------------------------------------
// acc[mi][ni] (rows 32 mi.., lanes 32 ni..) = rowop[row][:] . colop[lane][:], both operands with their token on the lane
__device__ __forceinline__ void wa_outer(f32x16 (&acc)[2][2], const float* rowop, const float* colop, int lane) {
    mfma32_zero(acc[0]);
    mfma32_zero(acc[1]);
    const int o = (lane & 31) * WA_LDR + (lane >> 5);
#pragma unroll
    for (int k = 0; k < WA_HD; k += 2) {
        const float a0 = rowop[o + k], a1 = rowop[o + 32 * WA_LDR + k];
        const float b0 = colop[o + k], b1 = colop[o + 32 * WA_LDR + k];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}
// out[ni] (rows: 32 channels, lanes 32 ni..) = sum over the rows t of x (the accumulator as the B operand) of op[t][channel] x[t][lane]:
// register r of x[mi][ni] holds rows mfma32_row(r, .) of the two lane halves, which is one k-step of 2
__device__ __forceinline__ void wa_contract(f32x16 (&out)[2], const f32x16 (&x)[2][2], const float* op, int lane) {
    mfma32_zero(out);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float a = op[mfma32_row(r, lane, 32 * mi) * WA_LDR + (lane & 31)];
            out[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x[mi][0][r], out[0], 0, 0, 0);
            out[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x[mi][1][r], out[1], 0, 0, 0);
        }
}
// an accumulator of wa_contract -> global: token 32 ni + (lane & 31), channels c0 + 8 g + 4 (lane >> 5) .. + 3, times scale[ni]
__device__ __forceinline__ void wa_write(float* __restrict__ dst, int stride, int c0, const f32x16 (&acc)[2], const float (&scale)[2],
                                         const WaGeom& g, const WaWindow& w, int lane) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int t = 32 * ni + (lane & 31);
        if (!wa_is(w, t)) continue;
        float* p = dst + wa_pixel(g, w, t) * stride + c0 + 4 * (lane >> 5);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *(f32x4*)(p + 8 * q) = f32x4{acc[ni][4 * q] * scale[ni], acc[ni][4 * q + 1] * scale[ni], acc[ni][4 * q + 2] * scale[ni],
                                         acc[ni][4 * q + 3] * scale[ni]};
    }
}

// st = K Q^T (keys on the rows, queries on the lanes) -> p = exp(tau st - max) over the valid keys, 0 elsewhere, in place; mx, sum: of the
// lane's two queries (both lane halves end with the same bits: a + b and b + a)
__device__ __forceinline__ void wa_softmax_t(f32x16 (&st)[2][2], float (&mx)[2], float (&sum)[2], const WaWindow& w, int lane) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        float m = -INFINITY;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                st[mi][ni][r] = __fmul_rn(st[mi][ni][r], WA_TAU);      // (never fused into the subtraction below)
                if (wa_is(w, mfma32_row(r, lane, 32 * mi))) m = fmaxf(m, st[mi][ni][r]);
            }
        m = fmaxf(m, __shfl_xor(m, 32, 64));      // (a window has a token inside the image: m is finite)
        float s = 0.0f;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = wa_is(w, mfma32_row(r, lane, 32 * mi)) ? expf(st[mi][ni][r] - m) : 0.0f;
                st[mi][ni][r] = p;
                s += p;
            }
        s += __shfl_xor(s, 32, 64);
        mx[ni] = m;
        sum[ni] = s;
    }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * WA_WAVES) void window_attention_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                            WaGeom g) {
    extern __shared__ float wa_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* qs = wa_lds + wave * 3 * WA_OPER;
    float *ks = qs + WA_OPER, *vs = ks + WA_OPER;
    const WaWindow w = wa_window(g);
    const int heads = g.D / WA_HD;
    for (int h0 = 0; h0 < heads; h0 += WA_WAVES) {
        const int h = h0 + wave;
        const bool active = h < heads;
        if (active) {
            WaStage a, b, c;
            wa_load(a, qkv, 3 * g.D, h * WA_HD, g, w, lane);
            wa_load(b, qkv, 3 * g.D, g.D + h * WA_HD, g, w, lane);
            wa_load(c, qkv, 3 * g.D, 2 * g.D + h * WA_HD, g, w, lane);
            wa_store(qs, a, lane);
            wa_store(ks, b, lane);
            wa_store(vs, c, lane);
        }
        __syncthreads();
        if (active) {
            f32x16 st[2][2], o[2];
            float mx[2], sum[2];
            wa_outer(st, ks, qs, lane);
            wa_softmax_t(st, mx, sum, w, lane);
            wa_contract(o, st, vs, lane);
            const float inv[2] = {1.0f / sum[0], 1.0f / sum[1]};
            wa_write(out, g.D, h * WA_HD, o, inv, g, w, lane);
        }
        __syncthreads();      // (the next head's staging overwrites what this one read)
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * WA_WAVES) void window_attention_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                            float* __restrict__ dqkv, WaGeom g) {
    extern __shared__ float wa_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* qs = wa_lds + wave * (4 * WA_OPER + 3 * WA_TOK);
    float *ks = qs + WA_OPER, *vs = ks + WA_OPER, *gs = vs + WA_OPER, *stat = gs + WA_OPER;      // stat: [max | sum | delta][64 queries]
    const WaWindow w = wa_window(g);
    const int heads = g.D / WA_HD;
    const float tau2[2] = {WA_TAU, WA_TAU};
    for (int h0 = 0; h0 < heads; h0 += WA_WAVES) {
        const int h = h0 + wave;
        const bool active = h < heads;
        if (active) {
            WaStage a, b, c, d;
            wa_load(a, qkv, 3 * g.D, h * WA_HD, g, w, lane);
            wa_load(b, qkv, 3 * g.D, g.D + h * WA_HD, g, w, lane);
            wa_load(c, qkv, 3 * g.D, 2 * g.D + h * WA_HD, g, w, lane);
            wa_load(d, dout, g.D, h * WA_HD, g, w, lane);
            wa_store(qs, a, lane);
            wa_store(ks, b, lane);
            wa_store(vs, c, lane);
            wa_store(gs, d, lane);
        }
        __syncthreads();
        if (active) {
            // keys on the rows, queries on the lanes: A^T, dA^T, the three per-query numbers, dS^T and from it dq
            f32x16 st[2][2], da[2][2], acc[2];
            float mx[2], sum[2], delta[2];
            wa_outer(st, ks, qs, lane);
            wa_softmax_t(st, mx, sum, w, lane);
            wa_outer(da, vs, gs, lane);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const float inv = 1.0f / sum[ni];
                float dl = 0.0f;
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        st[mi][ni][r] *= inv;
                        dl += da[mi][ni][r] * st[mi][ni][r];
                    }
                dl += __shfl_xor(dl, 32, 64);
                delta[ni] = dl;
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int r = 0; r < 16; ++r) st[mi][ni][r] *= da[mi][ni][r] - dl;
                if (lane < 32) {
                    stat[32 * ni + lane] = mx[ni];
                    stat[WA_TOK + 32 * ni + lane] = inv;
                    stat[2 * WA_TOK + 32 * ni + lane] = dl;
                }
            }
            wa_contract(acc, st, ks, lane);
            wa_write(dqkv, 3 * g.D, h * WA_HD, acc, tau2, g, w, lane);
        }
        __syncthreads();
        if (active) {
            // queries on the rows, keys on the lanes: A again (the same fmaf chains, so the same bits), dv, dA, dS and from it dk
            f32x16 s2[2][2], da[2][2], acc[2];
            const float one[2] = {1.0f, 1.0f};
            wa_outer(s2, qs, ks, lane);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int q = mfma32_row(r, lane, 32 * mi);
                    const float m = stat[q], inv = stat[WA_TOK + q];
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        s2[mi][ni][r] = wa_is(w, 32 * ni + (lane & 31)) ? expf(__fmul_rn(s2[mi][ni][r], WA_TAU) - m) * inv : 0.0f;
                }
            wa_contract(acc, s2, gs, lane);
            wa_write(dqkv, 3 * g.D, 2 * g.D + h * WA_HD, acc, one, g, w, lane);
            wa_outer(da, gs, vs, lane);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float dl = stat[2 * WA_TOK + mfma32_row(r, lane, 32 * mi)];
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) s2[mi][ni][r] *= da[mi][ni][r] - dl;
                }
            wa_contract(acc, s2, qs, lane);
            wa_write(dqkv, 3 * g.D, g.D + h * WA_HD, acc, tau2, g, w, lane);
        }
        __syncthreads();
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
static constexpr size_t WA_FWD_LDS = (size_t)WA_WAVES * 3 * WA_OPER * sizeof(float);                        // 101376 bytes
static constexpr size_t WA_BWD_LDS = (size_t)WA_WAVES * (4 * WA_OPER + 3 * WA_TOK) * sizeof(float);         // 138240 bytes
static_assert(WA_BWD_LDS <= 160 * 1024, "a workgroup's LDS");

// Everything the entry points refuse, before any device call: PESR_EINVAL with nothing launched.
static bool wa_geom(WaGeom& g, long& blocks, int N, int H, int W, int D, int shift) {
    if (N < 1 || H < 1 || W < 1 || D < WA_HD || D % WA_HD || D > WA_MAX_D || shift < 0 || shift >= WA_WIN) return false;
    g = WaGeom{H, W, D, shift, (H + shift + WA_WIN - 1) / WA_WIN, (W + shift + WA_WIN - 1) / WA_WIN};
    blocks = (long)N * g.wh * g.ww;
    return blocks <= 0x7fffffffL;
}
static bool wa_aligned(const void* p) { return p && ((uintptr_t)p & 15) == 0; }
// More than 64 KB of dynamic LDS has to be allowed per kernel and device.  Asked for at every call (a host-side setting of the function
// object, no stream operation, so it is legal inside a capture as well) and its error returned: a flag set once would hide a refusal
// behind the generic launch error of every later call.
template <class K> static int wa_allow_lds(K kernel, size_t bytes) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e == hipSuccess ? PESR_OK : (int)e;
}

int pesr_window_attention_fwd_launch(const float* qkv, float* out, int N, int H, int W, int D, int shift, hipStream_t stream) {
    WaGeom g;
    long blocks;
    if (!wa_aligned(qkv) || !wa_aligned(out) || !wa_geom(g, blocks, N, H, W, D, shift)) return PESR_EINVAL;
    if (const int rc = wa_allow_lds(window_attention_fwd_kernel, WA_FWD_LDS)) return rc;
    window_attention_fwd_kernel<<<dim3((unsigned)blocks), dim3(64 * WA_WAVES), WA_FWD_LDS, stream>>>(qkv, out, g);
    return pesr_launch_status();
}

int pesr_window_attention_bwd_launch(const float* qkv, const float* dout, float* dqkv, int N, int H, int W, int D, int shift,
                                     hipStream_t stream) {
    WaGeom g;
    long blocks;
    if (!wa_aligned(qkv) || !wa_aligned(dout) || !wa_aligned(dqkv) || !wa_geom(g, blocks, N, H, W, D, shift)) return PESR_EINVAL;
    if (const int rc = wa_allow_lds(window_attention_bwd_kernel, WA_BWD_LDS)) return rc;
    window_attention_bwd_kernel<<<dim3((unsigned)blocks), dim3(64 * WA_WAVES), WA_BWD_LDS, stream>>>(qkv, dout, dqkv, g);
    return pesr_launch_status();
}
