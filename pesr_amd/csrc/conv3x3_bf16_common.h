// What conv3x3_bf16.hip (one bf16 product) and conv3x3_bf16x3.hip (split operands, three products) have in common: the tile plan
// and its search, the packed-weight index, and the kernels' set-up (workgroup decode, fragment offsets, staging items, the channel
// offset of a chunk).  The two main loops - staging store, weight-ring depth, MFMA count - are each kernel's own.
#pragma once
#include "common.h"
#include "conv_epilogue.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int B16_MG = 9;      // m-tiles of 16 pixels per workgroup
constexpr int B16_PX = 96;     // LDS bytes per halo pixel (and plane): 64 of data + 32 of padding

// ---------------------------------------------------------------------------------------------------------------------------------
// host: the tile plan
struct Bf16Plan { int TR, TW, HT, WT, tiles_x, tiles_y, n_tiles, ntw, bn; long tiles; size_t lds; int score; };

// halo of a TR x TW tile: (mul * TR + add) x (mul * TW + add) input pixels
struct Bf16Halo { int mul, add; };
constexpr Bf16Halo B16_HALO_S1 = {1, 2};     // stride 1: TR + 2 x TW + 2
constexpr Bf16Halo B16_HALO_S2 = {2, 1};     // stride-2 forward: 2 TR + 1 x 2 TW + 1
constexpr Bf16Halo B16_HALO_S2D = {1, 1};    // a parity class of the stride-2 input gradient: TR + 1 x TW + 1, origin AT the tile

// Tile shape TR x TW == 144 positions over an ext_h x ext_w domain: least out-of-image area first; then m-tiles that stay inside one
// row (conflict-free fragment reads); then the smallest halo - among the shapes whose halo fits item_cap staging items (8 per pixel:
// NU * NT of the kernel).  Fills TR, TW, HT, WT, tiles_y, tiles_x.
static inline bool b16_pick_tile(int ext_h, int ext_w, Bf16Halo halo, int item_cap, Bf16Plan* p) {
    long best = -1;
    for (int TW = 1; TW <= 144; ++TW) {
        if (144 % TW) continue;
        const int TR = 144 / TW, HT = halo.mul * TR + halo.add, WT = halo.mul * TW + halo.add;
        if (HT * WT * 8 > item_cap) continue;
        const long cover = (long)pesr_cdiv(ext_h, TR) * TR * pesr_cdiv(ext_w, TW) * TW;
        const long score = cover * 8192 + (TW % 16 ? 4096 : 0) + (long)HT * WT;
        if (best < 0 || score < best) { best = score; p->TR = TR; p->TW = TW; }
    }
    if (best < 0) return false;
    p->HT = halo.mul * p->TR + halo.add; p->WT = halo.mul * p->TW + halo.add;
    p->tiles_y = pesr_cdiv(ext_h, p->TR); p->tiles_x = pesr_cdiv(ext_w, p->TW);
    return true;
}
// per-mille of the tiles' area that lies inside the ext_h x ext_w domain
static inline int b16_cover_permille(int ext_h, int ext_w, const Bf16Plan* p) {
    const double cover_eff = (double)ext_h * ext_w / ((double)p->tiles_y * p->TR * p->tiles_x * p->TW);
    return (int)(1000.0 * cover_eff);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// weight packing: OIHW fp32 -> [9][R/32][Nn][32] (R = the reduction channels, Nn = the n channels).  -> the OIHW source index of packed
// element e:
//   mode 0 (forward): out[t][c][n][k] = w[o = unperm(n)][i = 32c + k][t]
//   mode 1 (dgrad)  : out[t][c][n][k] = w[o = unperm(32c + k)][i = n][8 - t]   (the input gradient is the conv with the flipped kernel)
// ps = 1: the conv feeds nn.PixelShuffle(2); its output channels are ordered sub-pixel-major like pack.hip does.
__device__ __forceinline__ long pesr_bf16_pack_src(long e, int O, int I, int mode, int ps) {
    const int R = mode == 0 ? I : O, Nn = mode == 0 ? O : I;
    const int k = (int)(e & 31);
    long rest = e >> 5;
    const int n = (int)(rest % Nn); rest /= Nn;
    const int c = (int)(rest % (R >> 5));
    const int t = (int)(rest / (R >> 5));
    const int red = c * 32 + k;
    int o = mode == 0 ? n : red;
    const int i = mode == 0 ? red : n;
    if (ps) { const int C = O >> 2; const int sub = o / C, cc = o - sub * C; o = 4 * cc + sub; }
    return ((long)o * I + i) * 9 + (mode == 0 ? t : 8 - t);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// device: the kernels' set-up.  A = the kernel's argument struct (Bf16Args / B3Args: the same fields under the same names).
// S = 2: the stride-2 forward; CLS = 0..3: a parity class of the stride-2 input gradient, -1: a plain conv (conv3x3_bf16.hip's header).

// blockIdx -> (pixel tile, n-tile).  Workgroups b and b + 8 share an XCD: give every XCD a contiguous range of logical tiles,
// n-tile fastest, so the workgroups that read the same pixels share an L2.
struct Bf16Wg { int nt, tx, ty, img; };
template <class A>
__device__ __forceinline__ Bf16Wg b16_decode_wg(const A& a) {
    int b = blockIdx.x;
    if ((gridDim.x & 7) == 0) b = (b & 7) * (gridDim.x >> 3) + (b >> 3);
    int bid = b;
    Bf16Wg w;
    w.nt = bid % a.n_tiles;  bid /= a.n_tiles;
    w.tx = bid % a.tiles_x;  bid /= a.tiles_x;
    w.ty = bid % a.tiles_y;
    w.img = bid / a.tiles_y;
    return w;
}

// pixel-operand fragment offsets: lane (r, g) reads k-group g of pixel 16 i + r (the tap's shift is added per read)
template <int S>
__device__ __forceinline__ void b16_frag_offsets(int (&a_off)[B16_MG], int TW, int WT, int r, int g) {
#pragma unroll
    for (int i = 0; i < B16_MG; ++i) {
        const int m = i * 16 + r;
        const int trow = m / TW, tcol = m - trow * TW;
        a_off[i] = (S * trow * WT + tcol) * B16_PX + g * 16;
    }
}

// staging items: (halo pixel, 4-channel group q of 8), NU per thread of an NT-thread workgroup: -> the byte offset inside the image
// (out-of-image pixels are fetched beyond the buffer descriptor's range: the load returns zeros; images are < 2 GB) and the byte
// offset inside an LDS plane (items past the halo land in a dump pixel behind it).  S = 2: a halo row is stored de-interleaved.
template <int S, int CLS, int NU, int NT, class A>
__device__ __forceinline__ void b16_stage_items(const A& a, int WT, int tid, int gy0, int gx0, unsigned (&st_off)[NU], int (&st_dst)[NU]) {
    const int WE = (WT + 1) >> 1;                                       // even columns of a halo row (S = 2)
    const int n_items = a.HT * WT * 8;
    const int Cq = a.Cin >> 2;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int it = tid + u * NT;
        const int q = it & 7, px = it >> 3;
        const int hrow = px / WT, slot = px - hrow * WT;
        const int hcol = S == 2 ? (slot < WE ? 2 * slot : 2 * (slot - WE) + 1) : slot;      // LDS slot `slot` of the row holds halo column hcol
        const int iy = S * gy0 - (CLS < 0 ? 1 : 0) + hrow, ix = S * gx0 - (CLS < 0 ? 1 : 0) + hcol;
        const bool ok = it < n_items && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const int pix = a.ps_in ? ((2 * iy) * (2 * a.W) + 2 * ix) * Cq : (iy * a.W + ix) * a.Cin;
        st_off[u] = ok ? (unsigned)((pix + q * 4) * 4) : 0x80000000u;
        st_dst[u] = (it < n_items ? px : a.HT * WT) * B16_PX + q * 8;
    }
}
// buffer descriptor of image img of the input
template <class A>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t b16_x_rsrc(const A& a, int img) {
    const float* const x_img = a.x + (size_t)img * a.H * a.W * a.Cin;
    return __builtin_amdgcn_make_buffer_rsrc((void*)x_img, 0, (unsigned)((size_t)a.H * a.W * a.Cin * 4), 0x00020000);
}
// channel part of an input address (bytes) for the 32-channel chunk cc
template <class A>
__device__ __forceinline__ int b16_chunk_off(const A& a, int cc) {
    int coff = cc * 32;
    if (a.ps_in) coff = pesr_ps_in_chunk_off(coff, a.Cin >> 2, a.W);   // one pixel of the shuffled tensor
    return coff * 4;
}
