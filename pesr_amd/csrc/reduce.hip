// Fixed-order second-stage reduction shared by every "per-block partials -> final" pattern in this library
// (bias gradients, BatchNorm statistics, loss sums, RGB weight gradients):
//   dsum[col] = sum_{k < nb} part[k * ncols + col]      accumulated in double
// One 1024-thread block owns 64 columns x 16 row lanes; each thread adds its rows in increasing order, the
// 16 lanes are combined through LDS in lane order - the result does not depend on scheduling (bitwise
// reproducible), and no atomics are used.
#include "common.h"
#include "launchers.h"
#include "reduce_rows.h"

__global__ __launch_bounds__(1024) void reduce_rows_kernel(const float* __restrict__ part, double* __restrict__ dsum, int nb,
                                                           int ncols) {
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + cl;
    __shared__ double red[16][64];
    const double t = reduce_rows_block(part, nb, ncols, col, col < ncols, red);
    if (rl == 0 && col < ncols) dsum[col] = t;
}

int pesr_reduce_rows_launch(const float* part, double* dsum, int nb, int ncols, hipStream_t stream) {
    hipLaunchKernelGGL(reduce_rows_kernel, dim3((ncols + 63) / 64), dim3(1024), 0, stream, part, dsum, nb, ncols);
    return pesr_launch_status();
}

// The float64 one, for the exact kernels (ssim.hip, lpips.hip, gram.hip): out[n] = (sum of image n's `per` partials) / count.  One
// workgroup of 256 lanes per image: lane t adds partials t, t + 256, ... in ascending order, then block_sum_d's fixed tree, then one
// division.  Additions and one IEEE division only: there is nothing to contract, so this file needs no `fp contract(off)`.
__global__ __launch_bounds__(256) void mean_partials_kernel(const double* __restrict__ part, double* __restrict__ out, long per,
                                                            double count) {
    const double* p = part + blockIdx.x * per;
    double s = 0.0;
    for (long k = threadIdx.x; k < per; k += 256) s += p[k];
    __shared__ double red[4];
    const double t = block_sum_d(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = t / count;
}

int pesr_mean_partials_launch(const double* part, double* out, int N, long per, double count, hipStream_t stream) {
    hipLaunchKernelGGL(mean_partials_kernel, dim3(N), dim3(256), 0, stream, part, out, per, count);
    return pesr_launch_status();
}
