// fp32 MFMA tile code shared by the small fp32 GEMMs (gram.hip, cx.hip; conv3x3_wgrad_wino4.hip takes the type and the row function).
// v_mfma_f32_32x32x2_f32 is bit for bit a k-ordered fmaf chain.  Operands, one float per lane: lane l gives A[row l & 31][k = l >> 5]
// and B[k = l >> 5][column l & 31].  Accumulator, 16 floats per lane: lane l holds column l & 31, and register r holds the row that
// mfma32_row(r, l) spells out (base: the tile's first row, added in front so that the sum associates as it did when written out).
#pragma once
#include "common.h"
#include "launchers.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int mfma32_row(int r, int lane, int base = 0) { return base + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ void mfma32_zero(f32x16& acc) { acc = (f32x16)0.0f; }
template <int N>
__device__ __forceinline__ void mfma32_zero(f32x16 (&acc)[N]) {
#pragma unroll
    for (int u = 0; u < N; ++u) acc[u] = (f32x16)0.0f;
}

// ---- padded staging: ROWS x C floats -> LDS [ROWS][C + 1] ------------------------------------------------------------------------------
// The operand with its row on the lane: 32 lanes with the odd stride C + 1 hit 32 banks.  Two calls, so that a kernel can issue the
// loads of the next block before the MFMAs of this one and store them behind the barrier.  row(r, src) sets src to where row r of the
// block starts in global memory and says whether there is such a row; the others are zeros.  LOADS = ROWS * C / (THREADS * 4).
template <int C, int THREADS, int LOADS, class Row>
__device__ __forceinline__ void mfma32_stage_load(f32x4 (&v)[LOADS], int tid, Row&& row) {
#pragma unroll
    for (int it = 0; it < LOADS; ++it) {
        const int e = (it * THREADS + tid) * 4;
        const float* src;
        v[it] = row(e / C, src) ? *(const f32x4*)(src + e % C) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
}
// staged a float4 per lane (the odd row stride makes the LDS writes scalar, four lanes to a bank; one float per lane - coalesced
// loads, conflict-free writes - measured slower: 1057 us against 768 at the contextual loss's training shape)
template <int C, int THREADS, int LOADS>
__device__ __forceinline__ void mfma32_stage_store(float* lds, const f32x4 (&v)[LOADS], int tid) {
#pragma unroll
    for (int it = 0; it < LOADS; ++it) {
        const int e = (it * THREADS + tid) * 4;
        float* d = lds + (e / C) * (C + 1) + e % C;
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = v[it][i];
    }
}

// ---- the two backward kernels: [PIX rows][C channels] of output per workgroup of 4 waves -------------------------------------------------
// 32 x 32 tile t = wave + 4 u: row half t % NPH (the same for all of a wave's tiles: 4 % NPH == 0), channel band t / NPH
template <int C>
struct Mfma32Bwd {
    static constexpr int PIX = C == 256 ? 32 : 64;
    static constexpr int NPH = PIX / 32, TILES = (C / 32) * NPH, TPW = TILES / 4;
    static_assert(TILES % 4 == 0, "every wave owns the same number of tiles");
    static __host__ __device__ constexpr int half(int wave) { return wave % NPH; }
    static __host__ __device__ constexpr int band(int wave, int u) { return (wave + 4 * u) / NPH; }
};
// (The two inner loops - one LDS operand, one global operand, TPW MFMAs per k-step - stay written out in gram.hip and cx.hip, and so
// does the row decode of cx_bwd_kernel's epilogue: with either shared, hipcc moves a load of that kernel's loop and it runs 0.4 %
// slower, docs/experiments/mfma_tile_share.md.)

// ---- host: the channel counts these kernels are instantiated for -----------------------------------------------------------------------
template <class F> static inline bool mfma32_dispatch_c(int C, F&& f) { return pesr_dispatch_c<64, 128, 256>(C, f); }
static inline bool mfma32_c_ok(int C) { return mfma32_dispatch_c(C, [](auto) {}); }
