// The fused epilogue of the 3x3 conv kernels (conv3x3_mfma.hip, conv3x3_wino.hip, conv3x3_wino4.hip, conv3x3_bf16.hip,
// conv3x3_bf16x3.hip and the split-K finish kernels): ONE statement of the contract every family has to keep, since dispatch
// moves a layer between them by shape, precision mode and environment switch:
//     y = act(alpha * (conv + bias) [zeroed where mask <= 0] + skip),   stored plain or pixel-shuffled (r = 2).
// Device only.  pesr_epi4 takes values that are ALREADY LOADED: where and when a kernel issues its mask / skip / z loads (batches
// of three in the bf16 kernels, of six in F(4,3), all z loads behind the exchange barrier) is that kernel's measured choice.
#pragma once
#include "common.h"

__device__ __forceinline__ float pesr_act1(float v, int act, float slope) {
    if (act == PESR_ACT_RELU) v = v > 0.f ? v : 0.f;
    else if (act == PESR_ACT_LRELU) v = v > 0.f ? v : v * slope;
    return v;
}
__device__ __forceinline__ f32x4 pesr_act4(f32x4 v, int act, float slope) {
    if (act == PESR_ACT_RELU) {
        v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f; v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
    } else if (act == PESR_ACT_LRELU) {
        v.x = v.x > 0.f ? v.x : v.x * slope; v.y = v.y > 0.f ? v.y : v.y * slope;
        v.z = v.z > 0.f ? v.z : v.z * slope; v.w = v.w > 0.f ? v.w : v.w * slope;
    }
    return v;
}

__device__ __forceinline__ f32x4 pesr_mask4(f32x4 v, f32x4 mk) {
    v.x = mk.x > 0.f ? v.x : 0.f; v.y = mk.y > 0.f ? v.y : 0.f; v.z = mk.z > 0.f ? v.z : 0.f; v.w = mk.w > 0.f ? v.w : 0.f;
    return v;
}

// act(alpha * (v + bias) [masked by mk] + sk) on values that are already loaded; bias4 / mk / sk are read only where their flag is set
__device__ __forceinline__ f32x4 pesr_epi4(f32x4 v, bool has_bias, f32x4 bias4, float alpha, bool has_mask, f32x4 mk, bool has_skip, f32x4 sk,
                                           int act, float slope) {
    if (has_bias) v += bias4;
    v *= alpha;
    if (has_mask) v = pesr_mask4(v, mk);
    if (has_skip) v += sk;
    return pesr_act4(v, act, slope);
}
// The same with the loads AT the point of use, for the kernels that store one element per loop trip and have nothing to put between
// a load and its use: bias[bi ..], mask[idx ..], skip[idx ..]; a null pointer = absent.  (Handing these kernels' values to pesr_epi4
// costs a v_cndmask per register: the value is then defined on both sides of its `if`.)
__device__ __forceinline__ f32x4 pesr_epi4_at(f32x4 v, const float* bias, size_t bi, float alpha, const float* mask, const float* skip, size_t idx,
                                              int act, float slope) {
    if (bias) v += *(const f32x4*)(bias + bi);
    v *= alpha;
    if (mask) v = pesr_mask4(v, *(const f32x4*)(mask + idx));
    if (skip) v += *(const f32x4*)(skip + idx);
    return pesr_act4(v, act, slope);
}
__device__ __forceinline__ float pesr_epi1_at(float v, const float* bias, size_t bi, float alpha, const float* mask, const float* skip, size_t idx,
                                              int act, float slope) {
    if (bias) v += bias[bi];
    v *= alpha;
    if (mask) v = mask[idx] > 0.f ? v : 0.f;
    if (skip) v += skip[idx];
    return pesr_act1(v, act, slope);
}

// The conv feeds nn.PixelShuffle(2) and stores shuffled: packed channel co = (2*si+sj)*C + c of conv output pixel (oy, ox) goes to
// out[img][2*oy+si][2*ox+sj][c], C = Cout/4, OH x OW the conv's output size: -> that element's offset.  (Only this arm of a kernel's
// `if (a.ps) .. else (img_out + oy * OW + ox) * Cout + co` is a function: with both arms in one, the kernel arguments of both are
// read in front of the branch, and the scalar-register-bound kernels - the direct conv, F(4,3) with BatchNorm sums - came out in a
// different instruction order; docs/experiments/conv_epilogue_share.md.)
__device__ __forceinline__ size_t pesr_ps_out_index(int img, int oy, int ox, int co, int OH, int OW, int Cout) {
    const int C = Cout >> 2;
    const int sub = co / C, cc = co - sub * C;
    return (((size_t)img * (2 * OH) + 2 * oy + (sub >> 1)) * (2 * OW) + 2 * ox + (sub & 1)) * C + cc;
}

// ps_in: x is a pixel-shuffled tensor [N][2H][2W][Cq] (Cq = Cin/4) read as its un-shuffled, sub-pixel-major [N][H][W][Cin] view (the
// input gradient of a PixelShuffle conv).  A chunk that starts at packed channel coff = sub*Cq + cc0 is part of ONE pixel of the
// shuffled tensor: -> its element offset relative to the pixel (2*iy, 2*ix).
__device__ __forceinline__ int pesr_ps_in_chunk_off(int coff, int Cq, int W) {
    const int sub = coff / Cq, cc0 = coff - sub * Cq;
    return ((sub >> 1) * (2 * W) + (sub & 1)) * Cq + cc0;
}

// ---- BatchNorm sums out of the epilogue (common.h BnEpi) ------------------------------------------------------------------------
// the four per-channel coefficient vectors of mode 2, for channels c .. c + 3 of a C-channel BatchNorm
struct PesrBnCoef4 { f32x4 mu, istd, gamma, beta; };
__device__ __forceinline__ PesrBnCoef4 pesr_bn_coef4_zero() {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    return PesrBnCoef4{z, z, z, z};
}
__device__ __forceinline__ PesrBnCoef4 pesr_bn_coef4_load(const BnEpi* bn, int C, int c) {
    PesrBnCoef4 k;
    k.mu = *(const f32x4*)(bn->mi + c); k.istd = *(const f32x4*)(bn->mi + C + c);
    k.gamma = *(const f32x4*)(bn->gamma + c); k.beta = *(const f32x4*)(bn->beta + c);
    return k;
}
// mode 2: o is the gradient of y = lrelu(gamma * xhat(z) + beta); -> g' = o * lrelu'(..), and the sums of g' and g' * xhat
__device__ __forceinline__ f32x4 pesr_bn_lrelu_grad4(f32x4 o, f32x4 z, PesrBnCoef4 k, float slope, f32x4& st1, f32x4& st2) {
    const f32x4 xh = (z - k.mu) * k.istd;
    const f32x4 zz = k.gamma * xh + k.beta;
    o.x = zz.x > 0.f ? o.x : o.x * slope; o.y = zz.y > 0.f ? o.y : o.y * slope;
    o.z = zz.z > 0.f ? o.z : o.z * slope; o.w = zz.w > 0.f ? o.w : o.w * slope;
    st1 += o; st2 += o * xh;
    return o;
}
