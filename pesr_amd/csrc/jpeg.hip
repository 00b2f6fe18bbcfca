// The JPEG round trip of uint8 HWC RGB windows as pinned in docs/modes.md section 4l: what a baseline encoder at quality q followed
// by a decoder returns, without the (lossless) entropy coding.  JFIF colour conversion with 8-bit samples between the stages, 4:2:0
// (2 x 2 mean, rounded half up) or 4:4:4 chroma, 8 x 8 blocks anchored at the window's origin with the planes extended by
// replication, the orthonormal float64 DCT-II from a host-made table (rows, then columns, sums ascending), k = sign(F) floor(|F| / Q
// + 0.5), the inverse (columns, then rows), the 9/3/3/1 triangle filter back up, conversion back to RGB.  float64 with every product
// and sum rounded separately (no fused multiply-add: the host restatement reproduces every bit).  One call serves n entries through
// a descriptor array, in two launches:
//   A  one workgroup of 256 lanes per 16 x 16 pixel MCU of one entry (4 Y + 1 Cb + 1 Cr blocks at 4:2:0, 4 + 4 + 4 at 4:4:4): the
//      clamped source pixels are converted and staged in LDS, the chroma downsampled, then four passes over the blocks, each lane one
//      output value of a block per pass, ping-pong between two LDS buffers; the decoded 8-bit Y, Cb, Cr planes go to the workspace.
//   B  one lane per pixel: chroma upsampling (its neighbours lie in other blocks, hence the second launch) and the RGB conversion.
// Launch B reads nothing of the source, so source and destination may be the same bytes.
#pragma clang fp contract(off)
#include "common.h"
#include "launchers.h"
#include "exact_u8.h"

constexpr int JPEG_THREADS = 256;
constexpr int JPEG_MCU = 16;                               // pixels per workgroup and axis
constexpr int JPEG_DESC = 8;                               // int64 words per entry (include/pesr_hip.h)
constexpr long long JPEG_MAX_SIDE = 1LL << 26;             // 3 * stride stays inside an int

__host__ __device__ __forceinline__ long long jpeg_entry_bytes(long long h, long long w, bool c420) {
    return c420 ? h * w + 2 * ((h + 1) / 2) * ((w + 1) / 2) : 3 * h * w;
}

template <bool C420>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_code_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ ws,
                                                                 const long long* __restrict__ desc, int n,
                                                                 const double* __restrict__ dct, const double* __restrict__ quant) {
    constexpr int NBLK = C420 ? 6 : 12;                    // blocks 0..3: Y (block row * 2 + block column); then Cb, then Cr
    __shared__ double bufa[NBLK * 64];
    __shared__ double bufb[NBLK * 64];
    __shared__ double st[64];                              // T[u][x]
    __shared__ double sq[2 * 64];                          // the entry's luminance and chrominance tables, [v][u]
    __shared__ unsigned char sc[2][JPEG_MCU * JPEG_MCU];   // 4:2:0: the MCU's full-resolution Cb and Cr samples
    const int tid = threadIdx.x;
    if (tid < 64) st[tid] = dct[tid];
    for (int ent = blockIdx.y; ent < n; ent += gridDim.y) {
        const long long* d = desc + (long long)ent * JPEG_DESC;
        const long long so = d[0], sstride = d[1], wo = d[7];
        const int h = (int)d[4], w = (int)d[5], q = (int)d[6];
        const int ch = C420 ? (h + 1) / 2 : h, cw = C420 ? (w + 1) / 2 : w;
        unsigned char* py = ws + wo;
        unsigned char* pcb = py + (long long)h * w;
        unsigned char* pcr = pcb + (long long)ch * cw;
        const long long xm = (w + JPEG_MCU - 1) / JPEG_MCU;
        const long long mcus = ((h + JPEG_MCU - 1) / JPEG_MCU) * xm;
        __syncthreads();                                    // the previous entry's readers of sq are done
        if (tid < 128) sq[tid] = quant[(long long)(q - 1) * 128 + tid];
        for (long long t = blockIdx.x; t < mcus; t += gridDim.x) {
            const int my = (int)(t / xm) * JPEG_MCU, mx = (int)(t % xm) * JPEG_MCU;              // MCU origin in the window
            __syncthreads();                                // the previous MCU's readers are done
            {
                const int ly = tid / JPEG_MCU, lx = tid % JPEG_MCU;
                const int y = min(my + ly, h - 1), x = min(mx + lx, w - 1);
                const unsigned char* px = src + so + ((long long)y * sstride + x) * 3;
                const double R = (double)px[0], G = (double)px[1], B = (double)px[2];
                double Y = 0.299 * R;
                Y = exact_mac(Y, 0.587, G);
                Y = exact_mac(Y, 0.114, B);
                double Cb = 128.0 - 0.168736 * R;
                Cb = Cb - 0.331264 * G;
                Cb = exact_mac(Cb, 0.5, B);
                double Cr = exact_mac(128.0, 0.5, R);
                Cr = Cr - 0.418688 * G;
                Cr = Cr - 0.081312 * B;
                const int at = ((ly >> 3) * 2 + (lx >> 3)) * 64 + (ly & 7) * 8 + (lx & 7);
                bufa[at] = exact_round8(Y) - 128.0;
                if (C420) {
                    sc[0][tid] = (unsigned char)exact_round8(Cb);
                    sc[1][tid] = (unsigned char)exact_round8(Cr);
                } else {
                    bufa[4 * 64 + at] = exact_round8(Cb) - 128.0;
                    bufa[8 * 64 + at] = exact_round8(Cr) - 128.0;
                }
            }
            if (C420) {
                __syncthreads();
                if (tid < 128) {
                    // chroma sample (j, i) of the MCU; one past the plane's end replicates the plane's last sample
                    const int c = tid >> 6, j = (tid >> 3) & 7, i = tid & 7;
                    const int lj = min(my / 2 + j, ch - 1) - my / 2, li = min(mx / 2 + i, cw - 1) - mx / 2;
                    const unsigned char* p = sc[c] + (2 * lj) * JPEG_MCU + 2 * li;             // (the staging clamped rows / columns past the window)
                    const int sum = (int)p[0] + (int)p[1] + (int)p[JPEG_MCU] + (int)p[JPEG_MCU + 1];
                    bufa[(4 + c) * 64 + j * 8 + i] = (double)((sum + 2) >> 2) - 128.0;
                }
            }
            __syncthreads();
            // a block whose origin lies outside its plane produces nothing that is kept
            auto live = [&](int blk) -> bool {
                if (C420 && blk >= 4) return true;
                const int by = my + ((blk & 3) >> 1) * 8, bx = mx + (blk & 1) * 8;
                return by < h && bx < w;
            };
            // forward rows: G[y][u] = sum_x T[u][x] p[y][x]
            for (int idx = tid; idx < NBLK * 64; idx += JPEG_THREADS) {
                const int blk = idx >> 6, y = (idx >> 3) & 7, u = idx & 7;
                if (!live(blk)) continue;
                const double* p = bufa + blk * 64 + y * 8;
                double acc = 0.0;
#pragma unroll
                for (int x = 0; x < 8; ++x) acc = exact_mac(acc, st[u * 8 + x], p[x]);
                bufb[idx] = acc;
            }
            __syncthreads();
            // forward columns, quantise, dequantise: F[v][u] = sum_y T[v][y] G[y][u]
            for (int idx = tid; idx < NBLK * 64; idx += JPEG_THREADS) {
                const int blk = idx >> 6, v = (idx >> 3) & 7, u = idx & 7;
                if (!live(blk)) continue;
                const double* g = bufb + blk * 64 + u;
                double acc = 0.0;
#pragma unroll
                for (int y = 0; y < 8; ++y) acc = exact_mac(acc, st[v * 8 + y], g[y * 8]);
                const double Q = sq[(blk >= 4 ? 64 : 0) + v * 8 + u];
                const double kq = floor(fabs(acc) / Q + 0.5) * Q;
                bufa[idx] = acc < 0.0 ? -kq : kq;
            }
            __syncthreads();
            // inverse columns: H[y][u] = sum_v T[v][y] F'[v][u]
            for (int idx = tid; idx < NBLK * 64; idx += JPEG_THREADS) {
                const int blk = idx >> 6, y = (idx >> 3) & 7, u = idx & 7;
                if (!live(blk)) continue;
                const double* f = bufa + blk * 64 + u;
                double acc = 0.0;
#pragma unroll
                for (int v = 0; v < 8; ++v) acc = exact_mac(acc, st[v * 8 + y], f[v * 8]);
                bufb[idx] = acc;
            }
            __syncthreads();
            // inverse rows: p'[y][x] = sum_u T[u][x] H[y][u]; level shift, 8 bits, to the workspace plane
            for (int idx = tid; idx < NBLK * 64; idx += JPEG_THREADS) {
                const int blk = idx >> 6, y = (idx >> 3) & 7, x = idx & 7;
                if (!live(blk)) continue;
                const double* hm = bufb + blk * 64 + y * 8;
                double acc = 0.0;
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = exact_mac(acc, st[u * 8 + x], hm[u]);
                const unsigned char out = (unsigned char)exact_round8(acc + 128.0);
                if (C420 && blk >= 4) {
                    const int gy = my / 2 + y, gx = mx / 2 + x;
                    if (gy < ch && gx < cw) (blk == 4 ? pcb : pcr)[(long long)gy * cw + gx] = out;
                } else {
                    const int gy = my + ((blk & 3) >> 1) * 8 + y, gx = mx + (blk & 1) * 8 + x;
                    if (gy < h && gx < w) (blk < 4 ? py : (blk < 8 ? pcb : pcr))[(long long)gy * w + gx] = out;
                }
            }
        }
    }
}

template <bool C420>
__global__ __launch_bounds__(JPEG_THREADS) void jpeg_rgb_kernel(const unsigned char* __restrict__ ws, unsigned char* __restrict__ dst,
                                                                const long long* __restrict__ desc, int n) {
    for (int ent = blockIdx.y; ent < n; ent += gridDim.y) {
        const long long* d = desc + (long long)ent * JPEG_DESC;
        const long long dof = d[2], dstride = d[3], wo = d[7];
        const int h = (int)d[4], w = (int)d[5];
        const int ch = C420 ? (h + 1) / 2 : h, cw = C420 ? (w + 1) / 2 : w;
        const unsigned char* py = ws + wo;
        const unsigned char* pcb = py + (long long)h * w;
        const unsigned char* pcr = pcb + (long long)ch * cw;
        const long long xm = (w + JPEG_MCU - 1) / JPEG_MCU;
        const long long mcus = ((h + JPEG_MCU - 1) / JPEG_MCU) * xm;
        for (long long t = blockIdx.x; t < mcus; t += gridDim.x) {
            const int y = (int)(t / xm) * JPEG_MCU + threadIdx.x / JPEG_MCU, x = (int)(t % xm) * JPEG_MCU + threadIdx.x % JPEG_MCU;
            if (y >= h || x >= w) continue;
            const double Y = (double)py[(long long)y * w + x];
            int icb, icr;
            if (C420) {
                const int cy = y >> 1, cx = x >> 1;
                const int ny = min(max((y & 1) ? cy + 1 : cy - 1, 0), ch - 1), nx = min(max((x & 1) ? cx + 1 : cx - 1, 0), cw - 1);
                const long long a = (long long)cy * cw + cx, b = (long long)cy * cw + nx, c = (long long)ny * cw + cx, e = (long long)ny * cw + nx;
                icb = (9 * (int)pcb[a] + 3 * (int)pcb[b] + 3 * (int)pcb[c] + (int)pcb[e] + 8) >> 4;
                icr = (9 * (int)pcr[a] + 3 * (int)pcr[b] + 3 * (int)pcr[c] + (int)pcr[e] + 8) >> 4;
            } else {
                icb = pcb[(long long)y * w + x];
                icr = pcr[(long long)y * w + x];
            }
            const double cb = (double)(icb - 128), cr = (double)(icr - 128);
            const double R = exact_mac(Y, 1.402, cr);
            double G = Y - 0.344136 * cb;
            G = G - 0.714136 * cr;
            const double B = exact_mac(Y, 1.772, cb);
            unsigned char* o = dst + dof + ((long long)y * dstride + x) * 3;
            o[0] = (unsigned char)exact_round8(R);
            o[1] = (unsigned char)exact_round8(G);
            o[2] = (unsigned char)exact_round8(B);
        }
    }
}

// 0 unless every entry is valid and its workspace offset is the sum of the entries before it; else the bytes all n entries need
static long long jpeg_checked_bytes(const long long* desc_host, int n, int chroma, long long* max_mcus) {
    if (!desc_host || n < 1 || (chroma != 420 && chroma != 444)) return 0;
    long long total = 0, most = 1;
    for (int i = 0; i < n; ++i) {
        const long long* d = desc_host + (long long)i * JPEG_DESC;
        const long long h = d[4], w = d[5], q = d[6];
        if (d[0] < 0 || d[2] < 0 || h < 1 || w < 1 || h > JPEG_MAX_SIDE || w > JPEG_MAX_SIDE) return 0;
        if (d[1] < w || d[3] < w || d[1] > JPEG_MAX_SIDE || d[3] > JPEG_MAX_SIDE || q < 1 || q > 100) return 0;
        if (d[7] != total) return 0;
        total += jpeg_entry_bytes(h, w, chroma == 420);
        const long long mcus = ((h + JPEG_MCU - 1) / JPEG_MCU) * ((w + JPEG_MCU - 1) / JPEG_MCU);
        if (mcus > most) most = mcus;
    }
    if (max_mcus) *max_mcus = most;
    return total;
}

size_t pesr_jpeg_workspace_bytes_host(const long long* desc_host, int n, int chroma) {
    return (size_t)jpeg_checked_bytes(desc_host, n, chroma, nullptr);
}

int pesr_jpeg_u8_launch(const unsigned char* src, unsigned char* dst, const long long* desc_host, const long long* desc_dev, int n,
                        int chroma, const double* dct_dev, const double* quant_dev, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!src || !dst || !desc_dev || !dct_dev || !quant_dev || !ws) return PESR_EINVAL;
    long long max_mcus = 1;
    const long long need = jpeg_checked_bytes(desc_host, n, chroma, &max_mcus);
    if (need < 1 || (unsigned long long)need > (unsigned long long)ws_bytes) return PESR_EINVAL;
    const dim3 grid = exact_pool_grid(n, max_mcus);
    unsigned char* wsp = (unsigned char*)ws;
    if (chroma == 420) {
        hipLaunchKernelGGL(jpeg_code_kernel<true>, grid, dim3(JPEG_THREADS), 0, stream, src, wsp, desc_dev, n, dct_dev, quant_dev);
        hipLaunchKernelGGL(jpeg_rgb_kernel<true>, grid, dim3(JPEG_THREADS), 0, stream, (const unsigned char*)wsp, dst, desc_dev, n);
    } else {
        hipLaunchKernelGGL(jpeg_code_kernel<false>, grid, dim3(JPEG_THREADS), 0, stream, src, wsp, desc_dev, n, dct_dev, quant_dev);
        hipLaunchKernelGGL(jpeg_rgb_kernel<false>, grid, dim3(JPEG_THREADS), 0, stream, (const unsigned char*)wsp, dst, desc_dev, n);
    }
    return pesr_launch_status();
}
