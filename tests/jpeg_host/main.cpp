// Runs pesr_jpeg_u8_launch of csrc/jpeg.hip, compiled for the host, on one call read from a file (tests/test_jpeg_host_cpu.py).
#include "common.h"
#include "launchers.h"
// in.bin: int64 n, chroma, pool_bytes, inplace; desc n*8 int64; 64 doubles T; 12800 doubles quant; pool bytes.  out.bin: dst bytes
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    long long hd[4]; fread(hd, 8, 4, f);
    long long n = hd[0], chroma = hd[1], pool_bytes = hd[2], inplace = hd[3];
    long long* desc = (long long*)malloc(n * 64); fread(desc, 8, n * 8, f);
    double* T = (double*)malloc(64 * 8); fread(T, 8, 64, f);
    double* Q = (double*)malloc(12800 * 8); fread(Q, 8, 12800, f);
    unsigned char* pool = (unsigned char*)malloc(pool_bytes); fread(pool, 1, pool_bytes, f); fclose(f);
    size_t need = pesr_jpeg_workspace_bytes_host(desc, (int)n, (int)chroma);
    long long out_bytes = pool_bytes;
    if (!inplace) { out_bytes = 0; for (long long i = 0; i < n; ++i) out_bytes += 3 * desc[i * 8 + 4] * desc[i * 8 + 5]; }
    unsigned char* dst = inplace ? pool : (unsigned char*)malloc(out_bytes);
    if (!inplace) memset(dst, 9, out_bytes);
    unsigned char* ws = (unsigned char*)malloc(need ? need : 1);
    int rc = pesr_jpeg_u8_launch(pool, dst, desc, desc, (int)n, (int)chroma, T, Q, ws, need, nullptr);
    printf("rc %d need %zu\n", rc, need);
    f = fopen(argv[2], "wb"); fwrite(dst, 1, out_bytes, f); fclose(f);
    return rc;
}
