// Stands in for pesr_amd/csrc/common.h when a byte-image kernel file (csrc/jpeg.hip, resize_to.hip, resize.hip, degrade.hip) is
// compiled as plain C++ for the host (tests/host_build.py, used by the tests/test_*_host_cpu.py modules): the lanes of a workgroup
// run as std::threads with a std::barrier for __syncthreads, `__shared__` arrays are statics, workgroups run one after the other.
// The kernels' own code - indexing, order of operations, barriers - is what runs; no GPU is involved.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <barrier>
#include <thread>
#include <vector>
#include <functional>
using std::min; using std::max;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
typedef void* hipStream_t;
#define PESR_OK 0
#define PESR_EINVAL (-1)
#define PESR_EWORKSPACE (-2)
#define __global__
#define __device__
#define __host__
#define __shared__ static
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
inline thread_local dim3 threadIdx;
inline dim3 blockIdx, gridDim;
inline std::barrier<>* emu_barrier;
inline void __syncthreads() { emu_barrier->arrive_and_wait(); }
static inline int pesr_launch_status() { return 0; }
inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
inline void emu_launch(dim3 grid, dim3 block, std::function<void()> fn) {
    gridDim = grid;
    for (unsigned by = 0; by < grid.y; ++by) for (unsigned bx = 0; bx < grid.x; ++bx) {
        blockIdx = dim3(bx, by);
        std::barrier<> bar(block.x);
        emu_barrier = &bar;
        std::vector<std::thread> ts;
        for (unsigned t = 0; t < block.x; ++t) ts.emplace_back([&, t] { threadIdx = dim3(t); fn(); });
        for (auto& t : ts) t.join();
    }
}
#define hipLaunchKernelGGL(k, grid, block, shm, stream, ...) emu_launch(grid, block, [&] { k(__VA_ARGS__); })
