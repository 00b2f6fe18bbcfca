// Runs pesr_imresize_u8_pass_launch of csrc/resize.hip, compiled for the host, on one call read from a file
// (tests/test_resize_host_cpu.py).
#include "common.h"
#include "launchers.h"
// in.bin: int64 n, axis, s, up, pool_bytes, dst_bytes; desc n*4 int64; 16 doubles of weights; pool bytes.  out.bin: dst bytes, which
// start out as 9s
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long hd[6];
    if (fread(hd, 8, 6, f) != 6) return 2;
    const long long n = hd[0], axis = hd[1], s = hd[2], up = hd[3], pool_bytes = hd[4], dst_bytes = hd[5];
    std::vector<long long> desc((n > 0 ? n : 1) * 4);
    std::vector<double> wts(16);
    std::vector<unsigned char> pool(pool_bytes), dst(dst_bytes, 9);
    if (n > 0 && fread(desc.data(), 8, n * 4, f) != (size_t)(n * 4)) return 2;
    if (fread(wts.data(), 8, 16, f) != 16) return 2;
    if (fread(pool.data(), 1, pool_bytes, f) != (size_t)pool_bytes) return 2;
    fclose(f);
    const int rc = pesr_imresize_u8_pass_launch(pool.data(), dst.data(), desc.data(), desc.data(), (int)n, (int)axis, (int)s, (int)up,
                                                wts.data(), nullptr);
    printf("rc %d\n", rc);
    f = fopen(argv[2], "wb");
    fwrite(dst.data(), 1, dst_bytes, f);
    fclose(f);
    return rc;
}
