// The pinned float64 arithmetic and byte-image access that the exact kernels share (resize.hip, resize_to.hip, degrade.hip, jpeg.hip,
// niqe.hip, ssim.hip with the SSIM-Y score and loss): each of them promises bit equality with a float64 restatement on the host, and
// every operation that promise rests on is here once.  Include it after common.h, under the including file's own
// `#pragma clang fp contract(off)`.
#pragma once
#pragma clang fp contract(off)

// acc + w * v with the product and the sum rounded separately.  Plain operators under `fp contract(off)`: the multiply and the add
// carry no contraction flag, so the backend cannot fuse them.  (__dmul_rn / __dadd_rn are defined in the HIP headers, ahead of the
// pragma and under hipcc's default fast contraction: inlined here, they DO come out as v_fma_f64.)
__device__ __forceinline__ double exact_mac(double acc, double w, double v) {
    const double prod = w * v;
    return acc + prod;
}

__device__ __forceinline__ double exact_mac_u(double acc, double w, unsigned v) {
    const double prod = w * (double)v;
    return acc + prod;
}

__device__ __forceinline__ double exact_noise(double acc, double sigma, double g) {
    const double prod = sigma * g;
    return acc + prod;
}

// Clamp to [0, 255] and round half up.  The integer 0 .. 255 comes back as a double: the caller's own cast decides the conversion.
__device__ __forceinline__ double exact_round8(double v) {
    v = fmin(fmax(v, 0.0), 255.0);
    return floor(v + 0.5);
}

// four of them as the bytes of a dword, lowest first
__device__ __forceinline__ unsigned exact_round8x4(double a0, double a1, double a2, double a3) {
    return (unsigned)exact_round8(a0) | ((unsigned)exact_round8(a1) << 8) | ((unsigned)exact_round8(a2) << 16) | ((unsigned)exact_round8(a3) << 24);
}

// The 8-bit BT.601 luma of one RGB pixel, the Y of the PSNR-Y, SSIM-Y and NIQE's mode 1: each channel clipped to 0..255 and rounded
// (to even), weighed in double, + 16, clipped and rounded again.  An integer in 0..255.  loss.hip's luma_u8 is the same steps under
// that file's default contraction (psnr_y_kernel predates this header) and stays there.
__device__ __forceinline__ double exact_clip8(float v) { return rint(fmin(fmax((double)v, 0.0), 255.0)); }
__device__ __forceinline__ double exact_luma601_u8(float pr, float pg, float pb) {
    const double r = exact_clip8(pr), g = exact_clip8(pg), b = exact_clip8(pb);
    const double y = ((r * (65.738 / 256) + g * (129.057 / 256)) + b * (25.064 / 256)) + 16.0;
    return rint(fmin(fmax(y, 0.0), 255.0));
}

// symmetric reflection ... 1 0 | 0 1 ... n-1 | n-1 n-2 ... (period 2n), for any j
__device__ __forceinline__ int exact_reflect(int j, int n) {
    if ((unsigned)j < (unsigned)n) return j;
    int m = j % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

__device__ __forceinline__ int exact_reflect(long long j, int n) {
    if ((unsigned long long)j < (unsigned long long)n) return (int)j;
    long long m = j % (2LL * n);
    if (m < 0) m += 2LL * n;
    return (int)(m < n ? m : 2LL * n - 1 - m);
}

// replicate: ... 0 0 | 0 1 ... n-1 | n-1 n-1 ...
__device__ __forceinline__ int exact_replicate(int j, int n) { return j < 0 ? 0 : (j >= n ? n - 1 : j); }

// 4 bytes (nb of them inside the row) from any alignment
__device__ __forceinline__ unsigned exact_load4(const unsigned char* __restrict__ p, int nb) {
    unsigned v = 0;
    if (nb == 4) {
        __builtin_memcpy(&v, p, 4);
    } else {
        for (int b = 0; b < nb; ++b) v |= (unsigned)p[b] << (8 * b);
    }
    return v;
}

__device__ __forceinline__ void exact_store4(unsigned char* __restrict__ p, unsigned v, int nb) {
    if (nb == 4) {
        __builtin_memcpy(p, &v, 4);
    } else {
        for (int b = 0; b < nb; ++b) p[b] = (unsigned char)(v >> (8 * b));
    }
}

// one RGB pixel as r | g << 8 | b << 16
__device__ __forceinline__ unsigned exact_load_px(const unsigned char* __restrict__ p) {
    return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

// oracle/detrand.py's mixer, restated
__device__ __forceinline__ unsigned long long exact_splitmix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// docs/modes.md section 4j's twelve-term Irwin-Hall variate from the twelve 16-bit fields of three hashed counters: exact in float64
__device__ __forceinline__ double exact_gauss(unsigned long long key, unsigned long long e) {
    int sum = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const unsigned long long z = exact_splitmix64(key + 3ULL * e + (unsigned long long)j);
        sum += (int)(z & 0xffff) + (int)((z >> 16) & 0xffff) + (int)((z >> 32) & 0xffff) + (int)(z >> 48);
    }
    return (double)(2 * sum - 786420) / 131072.0;
}

// ---- host side of a pooled launch -----------------------------------------------------------------------------------------------
// About 32 K workgroups in all: each walks its entry's tiles with a stride (at most max_tiles of them: the most any entry has), and
// gridDim.y walks the n entries.
static inline dim3 exact_pool_grid(int n, long long max_tiles) {
    const int gy = n < 65535 ? n : 65535;
    long long gx = 32768 / gy;
    if (gx < 1) gx = 1;
    if (gx > max_tiles) gx = max_tiles;
    return dim3((unsigned)gx, (unsigned)gy);
}

// a noise level: not negative, not NaN, not infinite
static inline bool exact_sigma_ok(double sigma) { return sigma >= 0.0 && sigma <= 1.7976931348623157e308; }
