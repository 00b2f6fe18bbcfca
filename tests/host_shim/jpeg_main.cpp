// Runs pesr_jpeg_u8_launch of csrc/jpeg.hip, compiled for the host, on one call read from a file (tests/test_jpeg_host_cpu.py).
#include "common.h"
#include "launchers.h"
// in.bin: int64 n, chroma, pool_bytes, inplace; desc n*8 int64; 64 doubles T; 12800 doubles quant; pool bytes.  out.bin: dst bytes,
// which start out as 9s unless the call is in place
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long hd[4];
    if (fread(hd, 8, 4, f) != 4) return 2;
    const long long n = hd[0], chroma = hd[1], pool_bytes = hd[2], inplace = hd[3];
    std::vector<long long> desc((n > 0 ? n : 1) * 8);
    std::vector<double> T(64), Q(12800);
    std::vector<unsigned char> pool(pool_bytes);
    if (n > 0 && fread(desc.data(), 8, n * 8, f) != (size_t)(n * 8)) return 2;
    if (fread(T.data(), 8, 64, f) != 64 || fread(Q.data(), 8, 12800, f) != 12800) return 2;
    if (fread(pool.data(), 1, pool_bytes, f) != (size_t)pool_bytes) return 2;
    fclose(f);
    const size_t need = pesr_jpeg_workspace_bytes_host(desc.data(), (int)n, (int)chroma);
    long long out_bytes = 0;
    for (long long i = 0; i < n; ++i) out_bytes += 3 * desc[i * 8 + 4] * desc[i * 8 + 5];
    std::vector<unsigned char> fresh(inplace ? 0 : out_bytes, 9), ws(need ? need : 1);
    std::vector<unsigned char>& dst = inplace ? pool : fresh;
    const int rc = pesr_jpeg_u8_launch(pool.data(), dst.data(), desc.data(), desc.data(), (int)n, (int)chroma, T.data(), Q.data(), ws.data(),
                                       need, nullptr);
    printf("rc %d need %zu\n", rc, need);
    f = fopen(argv[2], "wb");
    fwrite(dst.data(), 1, dst.size(), f);
    fclose(f);
    return rc;
}
