// 3x3 convolution (stride 1; stride 2 forward) on the bf16 MFMA (v_mfma_f32_16x16x32_bf16), gfx950: the OPTIONAL reduced-precision mode.
//
// The contract and fused epilogue of conv_epilogue.h (reference nn.Conv2d(k=3, padding=1), model/basic.py:4-7, forward and -
// with mode-1 packed weights - input gradient): y = act(alpha * (conv + bias) [masked] + skip), fused PixelShuffle store / fused
// pixel-unshuffle load.  Activations stay fp32 in HBM; BOTH operands of every product are rounded to bf16 (round to nearest
// even) on their way into the matrix pipe and the products are accumulated in fp32.  That is a different arithmetic from the
// reference's fp32 conv (relative error of a product 2^-8 instead of 2^-24): it has its own oracle (oracle/ops.py
// conv3x3_bf16: the same rounding, float64 accumulation) and its own tolerance, and is never selected by default.
//
// One workgroup = 144 output pixels (TR rows x TW columns) x BN = 128 * NTW output channels, 8 waves (64-channel layers: 64 channels,
// 4 waves); wave w owns the 16 * NTW channels (w * NTW + j) * 16 .. for all nine 16-pixel m-tiles: 9 * NTW accumulator tiles.  Per 32-channel chunk:
//   * B operand (pixels): the tile's (TR + 2) x (TW + 2) input halo as bf16, [pixel][32 ch] = 64 B per pixel, double buffered in
//     LDS.  Global fp32 -> registers (issued at the top of the previous chunk) -> v_cvt_pk_bf16_f32 -> ds_write_b64 two thirds
//     into the previous chunk's MFMA stream; ONE barrier per chunk.  All nine taps read the same image at shifted pixel offsets
//     (a wave-uniform byte offset per tap); a pixel takes 96 bytes of LDS (64 of data, 32 of padding), the stride at which the
//     ds_read_b128 of 16 consecutive pixels is bank-conflict free at EVERY start offset with plain linear addressing (lane groups
//     of MI355X_MICROARCH.md, LDS table; 64 / 80 / 112 / 144 bytes are 2-way).
//   * A operand (weights): the wave's [16 ch][32 k] bf16 slabs straight from global memory into registers (1 KiB per wave and
//     slab, nothing to share through LDS), a whole chunk (9 taps) ahead.
// The weights are the MFMA's A operand, so a lane ends up with FOUR CONSECUTIVE output channels of one pixel: 16-byte stores,
// 16-byte skip / mask loads.
#include <mutex>
#include "common.h"
#include "launchers.h"
#include "conv_epilogue.h"
#include "conv3x3_bf16_common.h"

struct Bf16Args {
    const float* x;            // [N][H][W][Cin]
    const char* wp;            // packed bf16 weights [9][Cin/32][Cout][32]
    const float* bias;         // [Cout] or null
    const float* skip;         // [N][H][W][Cout] or null
    const float* mask;         // [N][H][W][Cout] or null : result zeroed where mask <= 0
    float* y;                  // [N][H][W][Cout]
    int N, H, W, Cin, Cout;    // H, W: the INPUT's size
    int OH, OW;                // the output's size (== H, W for stride 1)
    int TR, TW;                // tile: TR rows x TW OUTPUT pixels (TR * TW == 144)
    int tiles_x, tiles_y, n_tiles;
    int HT, WT;                // halo rows / columns
    float alpha, slope;
    int act;
    int ps;                    // 1: output stored pixel-shuffled (r = 2): packed channel (2*si+sj)*C + c -> y[n][2oy+si][2ox+sj][c], C = Cout/4
    int ps_in;                 // 1: x is a pixel-shuffled tensor [N][2H][2W][Cin/4] read as its sub-pixel-major [N][H][W][Cin] view
};

constexpr int B16_STAGE_T = 6; // the staged halo is converted and stored after this tap (4 / 6 / 8 measured the same)
constexpr int B16_FXD = 3;     // register sets of the pixel-fragment ring (2 measured the same)

// WTC: the halo width TW + 2 as a compile-time constant (the tile shapes of the networks' layers), or 0 = a.WT at run time.  With it
// a tap's LDS offset is an immediate of the ds_read, and the fragment reads need no address arithmetic inside the loop: with two
// waves per SIMD on 16-cycle MFMAs every other vector instruction competes with the matrix pipe for issue slots.
// NW: waves per workgroup.  8 (x NTW = 2 / 1: 256 / 128 output channels per workgroup), or 4 with NTW = 1 for the 64-channel layers
// (vgg19 conv1_2, the input gradients of the 64 -> 128 convs): 144 pixels x 64 channels, 256 threads, several workgroups per CU.
// S = 2: the stride-2 forward (the Discriminator's down-sampling convs, reference model/pesr.py:56-64).  The halo is (2 TR + 1) x
// (2 TW + 1) input pixels (up to 640: ten staging items per thread instead of four); a halo row is stored DE-INTERLEAVED - its even
// columns first, then the odd ones - so that the 16 pixels of a fragment read are again 16 consecutive LDS entries and a tap is
// again one uniform offset: kx = 0 / 1 / 2 -> even plane / odd plane / even plane + 1.
//
// CLS = 0..3: one output parity class (py, px) = (CLS >> 1, CLS & 1) of the STRIDE-2 INPUT GRADIENT: dx[2u + py][2v + px] =
// sum over the taps with ky = 1 (py = 0) or ky in {0, 2} (py = 1), likewise kx, of dy[u + (ky == 0)][v + (kx == 0)] * w[ky][kx]
// - a stride-1 problem over dy with 1 / 2 / 2 / 4 taps, no multiply-by-zero work (conv3x3_mfma.hip does the same in fp32).  x = dy,
// H, W = dy's size, OH, OW = dx's size; the halo is (TR + 1) x (TW + 1) with its origin AT the tile; the weights are the mode-1
// packing (its slab t holds forward tap 8 - t).
__host__ __device__ constexpr bool b16_tap_used(int cls, int t) {
    return cls < 0 || ((((cls >> 1) != 0) == (t / 3 != 1)) && (((cls & 1) != 0) == (t % 3 != 1)));
}
__host__ __device__ constexpr int b16_ntaps(int cls) { return cls < 0 ? 9 : (1 + (cls >> 1)) * (1 + (cls & 1)); }
// the k-th used tap of a class (forward tap index ky * 3 + kx), in increasing order
__host__ __device__ constexpr int b16_tap(int cls, int k) {
    int n = 0;
    for (int t = 0; t < 9; ++t)
        if (b16_tap_used(cls, t)) { if (n == k) return t; ++n; }
    return 0;
}

template <int NTW, int WTC, int NW, int S, int CLS>
__device__ __forceinline__ void conv3x3_bf16_body(const Bf16Args& a) {
    constexpr int NTAP = b16_ntaps(CLS);
    constexpr int PY = CLS < 0 ? 0 : (CLS >> 1), PX = CLS < 0 ? 0 : (CLS & 1);
    constexpr int NT = NW * 64, NU = (S == 2 ? 5120 : 2048) / NT, BN = NW * 16 * NTW;
    const int WT = WTC ? WTC : a.WT;
    const int WE = (WT + 1) >> 1;                                       // even columns of a halo row (S = 2)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int v_bytes = (a.HT * WT + 1) * B16_PX;                       // + the dump pixel

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;

    const Bf16Wg wg = b16_decode_wg(a);                                 // blockIdx -> (pixel tile, n-tile), n-tiles of a pixel tile on one XCD
    const int img = wg.img;
    const int gy0 = wg.ty * a.TR, gx0 = wg.tx * a.TW;
    const int n0 = wg.nt * BN;
    const int C32 = a.Cin >> 5;

    // ---- pixel-operand fragment offsets: lane (r, g) reads k-group g of pixel 16 i + r, shifted by the tap's column kx ---------
    int a_off[B16_MG];
    b16_frag_offsets<S>(a_off, a.TW, WT, r, g);

    // ---- weight operand: this lane's 16 bytes of slab (tap, chunk), n-tile j.  A buffer load: the slab's offset is a SCALAR offset
    // and j a 1-KiB immediate, so a weight fetch costs the vector unit nothing but its issue slot (the packed weights are < 4 GB).
    const int slab_bytes = a.Cout * 64;
    const unsigned b_lane = (unsigned)(((n0 + wave * NTW * 16 + r) * 32 + g * 8) * 2);
    const __amdgpu_buffer_rsrc_t w_rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.wp, 0, (unsigned)((size_t)9 * a.Cin * a.Cout * 2), 0x00020000);
    auto ldw = [&](int t, int j, int cc) -> bf16x8 {
        const int so = ((CLS < 0 ? t : 8 - t) * C32 + cc) * slab_bytes;
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, b_lane + j * 1024, so, 0));
    };

    // ---- staging items: (halo pixel, 4-channel group q of 8) ---------------------------------------------------------------------
    unsigned st_off[NU];
    int st_dst[NU];
    b16_stage_items<S, CLS, NU, NT>(a, WT, tid, gy0, gx0, st_off, st_dst);
    const __amdgpu_buffer_rsrc_t x_rsrc = b16_x_rsrc(a, img);
    u32x4 sx[NU];
    auto stage_load = [&](int cc) {
        const int so = __builtin_amdgcn_readfirstlane(b16_chunk_off(a, cc));
#pragma unroll
        for (int u = 0; u < NU; ++u) sx[u] = __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, st_off[u], so, 0);
    };
    auto stage_store = [&](char* vdst) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            // (volatile: left to itself hipcc converts right behind the loads, i.e. waits for them at the top of the chunk)
            unsigned lo, hi;
            asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(lo) : "v"(sx[u].x), "v"(sx[u].y));
            asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(hi) : "v"(sx[u].z), "v"(sx[u].w));
            *(u32x2*)(vdst + st_dst[u]) = (u32x2){lo, hi};
        }
    };

    f32x4 acc[NTW][B16_MG];
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int i = 0; i < B16_MG; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    bf16x8 fw[9][NTW];         // the wave's weight fragments, one chunk ahead
    bf16x8 fx[B16_FXD][3];     // pixel fragments: groups of three m-tiles in a ring of B16_FXD register sets

#define B16_READ_X(FX, VB, T, GRP)                                                                       \
    {                                                                                                    \
        const int tt_ = b16_tap(CLS, (T));      /* (folds to a constant once the tap loop is unrolled) */ \
        const int to_ = CLS >= 0 ? ((tt_ / 3 == 0 ? WT : 0) + (tt_ % 3 == 0 ? 1 : 0)) * B16_PX                \
                                 : ((tt_ / 3) * WT + (S == 2 ? (tt_ % 3 == 1 ? WE : (tt_ % 3) >> 1) : tt_ % 3)) * B16_PX; \
        _Pragma("unroll") for (int i = 0; i < 3; ++i)                                                    \
            FX[i] = *(const bf16x8*)((VB) + a_cur[(GRP) * 3 + i] + to_);                                 \
    }
#define B16_MFMA(FX, T, GRP)                                                                             \
    _Pragma("unroll") for (int i = 0; i < 3; ++i)                                                        \
        _Pragma("unroll") for (int j = 0; j < NTW; ++j)                                                  \
            acc[j][(GRP) * 3 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[T][j], FX[i], acc[j][(GRP) * 3 + i], 0, 0, 0);

    // ---- prologue: chunk 0 staged synchronously, its nine weight slabs -----------------------------------------------------------
    // (the loads are pinned in the loop's issue order: the waits the compiler counts for the loop's first uses cover both ways in)
    stage_load(0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < NTAP; ++t) {
#pragma unroll
        for (int j = 0; j < NTW; ++j) fw[t][j] = ldw(b16_tap(CLS, t), j, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    stage_store(smem);
    __syncthreads();

#pragma unroll 1
    for (int c = 0; c < C32; ++c) {
        const int cur_off = (c & 1) * v_bytes;
        int a_cur[B16_MG];                                 // this chunk's image folded into the per-lane offsets: 9 adds per chunk, not 81
#pragma unroll
        for (int i = 0; i < B16_MG; ++i) a_cur[i] = a_off[i] + cur_off;
        char* const vnext = smem + ((c & 1) ^ 1) * v_bytes;
        // The last chunk "prefetches" itself again (loads and LDS stores nobody consumes): with no branch in the loop the
        // compiler counts the outstanding loads exactly instead of draining the queue (vmcnt(0)) at every use.
        const int cn = c + 1 < C32 ? c + 1 : c;
        stage_load(cn);                                    // lands while this chunk computes
        // fragment groups G = 3 t + grp (27 per chunk) go through a ring of B16_FXD register sets: the reads of group G + B16_FXD - 1
        // are issued in front of the MFMAs of group G, i.e. B16_FXD - 1 groups (6 MFMAs each) ahead of their use
#pragma unroll
        for (int G0 = 0; G0 < B16_FXD - 1; ++G0) B16_READ_X(fx[G0], smem, G0 / 3, G0 % 3)
#pragma unroll
        for (int t = 0; t < NTAP; ++t) {
#pragma unroll
            for (int grp = 0; grp < 3; ++grp) {
                const int G = t * 3 + grp, Gn = G + B16_FXD - 1;
                if (Gn < 3 * NTAP) B16_READ_X(fx[Gn % B16_FXD], smem, Gn / 3, Gn % 3)
                __builtin_amdgcn_sched_barrier(0);         // keep the prefetch ahead of the MFMA group
                B16_MFMA(fx[G % B16_FXD], t, grp)
                __builtin_amdgcn_sched_barrier(0);
            }
            // this tap's weights are consumed: fetch the same tap of the next chunk into their registers
#pragma unroll
            for (int j = 0; j < NTW; ++j) fw[t][j] = ldw(b16_tap(CLS, t), j, cn);
            if (t == (NTAP == 9 ? B16_STAGE_T : NTAP - 1)) { stage_store(vnext); __builtin_amdgcn_sched_barrier(0); }
        }
        __syncthreads();                                   // the next image is complete and visible; everyone is done with this one
    }
#undef B16_READ_X
#undef B16_MFMA

    // ---- epilogue: lane (r, g) holds channels co .. co + 3 of pixel 16 i + r -----------------------------------------------------
    const size_t img_out = (size_t)img * a.OH * a.OW;
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
        const int co = n0 + (wave * NTW + j) * 16 + g * 4;
        f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
        if (a.bias) bias4 = *(const f32x4*)(a.bias + co);
#pragma unroll
        for (int ib = 0; ib < B16_MG; ib += 3) {
            f32x4 mkv[3], skv[3];
            size_t idx[3];
            bool ok[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int m = (ib + e) * 16 + r;
                const int trow = m / a.TW, tcol = m - trow * a.TW;
                const int oy = CLS < 0 ? gy0 + trow : 2 * (gy0 + trow) + PY, ox = CLS < 0 ? gx0 + tcol : 2 * (gx0 + tcol) + PX;
                ok[e] = oy < a.OH && ox < a.OW;
                if (a.ps) idx[e] = pesr_ps_out_index(img, oy, ox, co, a.OH, a.OW, a.Cout);
                else idx[e] = (img_out + (size_t)oy * a.OW + ox) * a.Cout + co;
                if (!ok[e]) idx[e] = 0;
                if (a.mask) mkv[e] = *(const f32x4*)(a.mask + idx[e]);
                if (a.skip) skv[e] = *(const f32x4*)(a.skip + idx[e]);
            }
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                if (!ok[e]) continue;
                *(f32x4*)(a.y + idx[e]) = pesr_epi4(acc[j][ib + e], a.bias != nullptr, bias4, a.alpha, a.mask != nullptr, mkv[e],
                                                    a.skip != nullptr, skv[e], a.act, a.slope);
            }
        }
    }
}

template <int NTW, int WTC, int NW, int S = 1>
__global__ __launch_bounds__(NW * 64) void conv3x3_bf16_kernel(const Bf16Args a) {
    conv3x3_bf16_body<NTW, WTC, NW, S, -1>(a);
}

// stride-2 input gradient: blockIdx.y = parity class, so that the four small problems fill the chip together
template <int NTW, int WTC, int NW>
__global__ __launch_bounds__(NW * 64) void conv3x3_bf16_s2_dgrad_kernel(const Bf16Args a) {
    switch (blockIdx.y) {           // the four-tap class is dispatched first
        case 0: conv3x3_bf16_body<NTW, WTC, NW, 1, 3>(a); break;
        case 1: conv3x3_bf16_body<NTW, WTC, NW, 1, 2>(a); break;
        case 2: conv3x3_bf16_body<NTW, WTC, NW, 1, 1>(a); break;
        default: conv3x3_bf16_body<NTW, WTC, NW, 1, 0>(a); break;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// weight packing: OIHW fp32 -> [9][R/32][Nn][32] bf16 (round to nearest even), in the order of pesr_bf16_pack_src (conv3x3_bf16_common.h)
__global__ void pack_bf16_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int O, int I, int mode, int ps) {
    const long total = 9L * O * I;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
        out[e] = (__bf16)w[pesr_bf16_pack_src(e, O, I, mode, ps)];
}

int pesr_pack_conv3x3_bf16_launch(const float* w, void* out, int O, int I, int mode, int ps, hipStream_t stream) {
    if (O % 32 || I % 32 || (mode != 0 && mode != 1) || (ps && O % 128)) return PESR_EINVAL;
    const long total = 9L * O * I;
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_bf16_kernel, dim3(grid), dim3(256), 0, stream, w, (__bf16*)out, O, I, mode, ps);
    return pesr_launch_status();
}

namespace {
// Tile shape TR x TW == 144 pixels with the least out-of-image area whose halo fits the four staging items per thread.
static bool b16_plan(int N, int H, int W, int Cin, int Cout, Bf16Plan* p, int min_wgs = 128) {
    if (N < 1 || H < 1 || W < 1 || Cin % 32 || Cin < 32 || Cout % 64) return false;
    if ((size_t)H * W * Cin * 4 >= ((size_t)1 << 31)) return false;   // one image per buffer descriptor, offsets below 2^31
    if (!b16_pick_tile(H, W, B16_HALO_S1, 2048, p)) return false;
    // 256 output channels per workgroup unless that leaves fewer than 128 workgroups (the 12^2 / 24^2 layers): then 128 each
    p->ntw = (Cout % 256 == 0 && (long)N * p->tiles_y * p->tiles_x * (Cout / 256) >= 128) ? 2 : 1;
    p->bn = Cout % 128 == 0 ? 128 * p->ntw : 64;              // 64: the four-wave workgroups
    p->n_tiles = Cout / p->bn;
    p->tiles = (long)N * p->tiles_y * p->tiles_x * p->n_tiles;
    p->lds = (size_t)2 * (p->HT * p->WT + 1) * B16_PX;
    p->score = p->tiles >= min_wgs ? b16_cover_permille(H, W, p) : 0;
    return true;
}
// Stride 2 (forward only): TR x TW == 144 OUTPUT pixels whose (2 TR + 1) x (2 TW + 1) halo fits the ten staging items per thread;
// 128 output channels per eight-wave workgroup (64: four waves).  These layers are small (the Discriminator's 24^2 / 12^2 outputs
// give 128 / 64 workgroups) and the fp32 alternative is the small-tile direct kernel: half of min_wgs is already worth the switch.
static bool b16_plan_s2(int N, int H, int W, int Cin, int Cout, Bf16Plan* p, int min_wgs = 128) {
    if (N < 1 || H < 2 || W < 2 || Cin % 32 || Cin < 32 || Cout % 64) return false;
    if ((size_t)H * W * Cin * 4 >= ((size_t)1 << 31)) return false;
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    if (!b16_pick_tile(OH, OW, B16_HALO_S2, 5120, p)) return false;
    p->ntw = 1;
    p->bn = Cout % 128 == 0 ? 128 : 64;
    p->n_tiles = Cout / p->bn;
    p->tiles = (long)N * p->tiles_y * p->tiles_x * p->n_tiles;
    p->lds = (size_t)2 * (p->HT * p->WT + 1) * B16_PX;
    p->score = p->tiles >= (min_wgs + 1) / 2 ? b16_cover_permille(OH, OW, p) : 0;
    return true;
}
// Stride-2 input gradient (four parity classes over dy [N][DH][DW][Cin]; Cout = the forward conv's input channels): TR x TW == 144
// dy positions per tile, (TR + 1) x (TW + 1) halo; blockIdx.y = class.
static bool b16_plan_s2d(int N, int DH, int DW, int Cin, int Cout, Bf16Plan* p, int min_wgs = 128) {
    if (N < 1 || DH < 1 || DW < 1 || Cin % 32 || Cin < 32 || Cout % 64) return false;
    if ((size_t)DH * DW * Cin * 4 >= ((size_t)1 << 31)) return false;
    if (!b16_pick_tile(DH, DW, B16_HALO_S2D, 2048, p)) return false;
    p->ntw = (Cout % 256 == 0 && (long)N * p->tiles_y * p->tiles_x * (Cout / 256) * 4 >= 128) ? 2 : 1;
    p->bn = Cout % 128 == 0 ? 128 * p->ntw : 64;
    p->n_tiles = Cout / p->bn;
    p->tiles = (long)N * p->tiles_y * p->tiles_x * p->n_tiles;       // per class
    p->lds = (size_t)2 * (p->HT * p->WT + 1) * B16_PX;
    p->score = 4 * p->tiles >= min_wgs ? b16_cover_permille(DH, DW, p) : 0;
    return true;
}
}  // namespace

// per-mille of tile area inside the image (0: unsupported shape, or fewer than min_wgs workgroups: not worth leaving the fp32 kernels)
int pesr_conv3x3_bf16_score_impl(int N, int H, int W, int Cin, int Cout, int min_wgs) {
    Bf16Plan p;
    if (!b16_plan(N, H, W, Cin, Cout, &p, min_wgs)) return 0;
    return p.score;
}

int pesr_conv3x3_bf16_launch(const float* x, const void* wp, const float* bias, const float* skip, const float* mask, float* y,
                             int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, int ps, int ps_in,
                             hipStream_t stream) {
    Bf16Plan p;
    if (!b16_plan(N, H, W, Cin, Cout, &p)) return PESR_EINVAL;
    if (ps && (Cout % (4 * p.bn) || skip || mask)) return PESR_EINVAL;          // an n-tile must stay inside one sub-pixel plane
    if (ps_in && Cin % 128) return PESR_EINVAL;                                 // a 32-channel chunk must stay inside one sub-pixel
    Bf16Args a{};
    a.x = x; a.wp = (const char*)wp; a.bias = bias; a.skip = skip; a.mask = mask; a.y = y;
    a.N = N; a.H = H; a.W = W; a.OH = H; a.OW = W; a.Cin = Cin; a.Cout = Cout;
    a.alpha = alpha; a.slope = slope; a.act = act; a.ps = ps; a.ps_in = ps_in;
    a.TR = p.TR; a.TW = p.TW; a.HT = p.HT; a.WT = p.WT;
    a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.n_tiles = p.n_tiles;
#define B16_LAUNCH(NTW_, WT_, NW_) \
    hipLaunchKernelGGL((conv3x3_bf16_kernel<NTW_, WT_, NW_>), dim3((unsigned)p.tiles), dim3(NW_ * 64), p.lds, stream, a)
#define B16_BY_WT(NTW_, NW_)                                 \
    switch (p.WT) {                                          \
        case 50: B16_LAUNCH(NTW_, 50, NW_); break;           \
        case 26: B16_LAUNCH(NTW_, 26, NW_); break;           \
        case 14: B16_LAUNCH(NTW_, 14, NW_); break;           \
        default: B16_LAUNCH(NTW_, 0, NW_); break;            \
    }
    if (p.bn == 64) { B16_BY_WT(1, 4) } else if (p.ntw == 2) { B16_BY_WT(2, 8) } else { B16_BY_WT(1, 8) }
#undef B16_BY_WT
#undef B16_LAUNCH
    return pesr_launch_status();
}

// Stride-2 forward (input [N][H][W][Cin] -> output [N][(H-1)/2+1][(W-1)/2+1][Cout]); same packed weights as the stride-1 forward.
int pesr_conv3x3_bf16_s2_score_impl(int N, int H, int W, int Cin, int Cout, int min_wgs) {
    Bf16Plan p;
    if (!b16_plan_s2(N, H, W, Cin, Cout, &p, min_wgs)) return 0;
    return p.score;
}

int pesr_conv3x3_bf16_s2_launch(const float* x, const void* wp, const float* bias, const float* skip, const float* mask, float* y,
                                int N, int H, int W, int Cin, int Cout, float alpha, int act, float slope, hipStream_t stream) {
    Bf16Plan p;
    if (!b16_plan_s2(N, H, W, Cin, Cout, &p)) return PESR_EINVAL;
    Bf16Args a{};
    a.x = x; a.wp = (const char*)wp; a.bias = bias; a.skip = skip; a.mask = mask; a.y = y;
    a.N = N; a.H = H; a.W = W; a.OH = (H - 1) / 2 + 1; a.OW = (W - 1) / 2 + 1; a.Cin = Cin; a.Cout = Cout;
    a.alpha = alpha; a.slope = slope; a.act = act; a.ps = 0; a.ps_in = 0;
    a.TR = p.TR; a.TW = p.TW; a.HT = p.HT; a.WT = p.WT;
    a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.n_tiles = p.n_tiles;
#define B16_LAUNCH_S2(WT_, NW_)                                                                                        \
    {                                                                                                                  \
        auto kern = conv3x3_bf16_kernel<1, WT_, NW_, 2>;                                                               \
        static PesrDeviceOnce once;                                                                                    \
        once([&] { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }); \
        hipLaunchKernelGGL(kern, dim3((unsigned)p.tiles), dim3(NW_ * 64), p.lds, stream, a);                           \
    }
    if (p.bn == 64) { if (p.WT == 25) B16_LAUNCH_S2(25, 4) else B16_LAUNCH_S2(0, 4) }
    else { if (p.WT == 25) B16_LAUNCH_S2(25, 8) else B16_LAUNCH_S2(0, 8) }
#undef B16_LAUNCH_S2
    return pesr_launch_status();
}

// Stride-2 input gradient: dy [N][DH][DW][Cout_fwd] (DH = (H-1)/2+1 ...) -> dx [N][H][W][Cin_fwd]; weights: mode-1 packing of the
// forward weights [Cout_fwd][Cin_fwd][3][3] (the stride-1 input gradient's packing).  dx = alpha * grad [masked] + skip.
int pesr_conv3x3_bf16_s2_dgrad_score_impl(int N, int H, int W, int Cout_fwd, int Cin_fwd, int min_wgs) {
    Bf16Plan p;
    if (H < 1 || W < 1 || !b16_plan_s2d(N, (H - 1) / 2 + 1, (W - 1) / 2 + 1, Cout_fwd, Cin_fwd, &p, min_wgs)) return 0;
    return p.score;
}

int pesr_conv3x3_bf16_s2_dgrad_launch(const float* dy, const void* wp, const float* mask, const float* skip, float* dx, int N, int H, int W,
                                      int Cout_fwd, int Cin_fwd, float alpha, hipStream_t stream) {
    Bf16Plan p;
    if (H < 1 || W < 1) return PESR_EINVAL;
    const int DH = (H - 1) / 2 + 1, DW = (W - 1) / 2 + 1;
    if (!b16_plan_s2d(N, DH, DW, Cout_fwd, Cin_fwd, &p)) return PESR_EINVAL;
    Bf16Args a{};
    a.x = dy; a.wp = (const char*)wp; a.bias = nullptr; a.skip = skip; a.mask = mask; a.y = dx;
    a.N = N; a.H = DH; a.W = DW; a.OH = H; a.OW = W; a.Cin = Cout_fwd; a.Cout = Cin_fwd;
    a.alpha = alpha; a.slope = 0.f; a.act = PESR_ACT_NONE; a.ps = 0; a.ps_in = 0;
    a.TR = p.TR; a.TW = p.TW; a.HT = p.HT; a.WT = p.WT;
    a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.n_tiles = p.n_tiles;
    const dim3 grid((unsigned)p.tiles, 4);
    if (p.bn == 64) hipLaunchKernelGGL((conv3x3_bf16_s2_dgrad_kernel<1, 0, 4>), grid, dim3(256), p.lds, stream, a);
    else if (p.ntw == 2) hipLaunchKernelGGL((conv3x3_bf16_s2_dgrad_kernel<2, 0, 8>), grid, dim3(512), p.lds, stream, a);
    else hipLaunchKernelGGL((conv3x3_bf16_s2_dgrad_kernel<1, 0, 8>), grid, dim3(512), p.lds, stream, a);
    return pesr_launch_status();
}
