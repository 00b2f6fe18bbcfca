// Runs pesr_degrade_u8_launch of csrc/degrade.hip, compiled for the host, on one call read from a file
// (tests/test_degrade_host_cpu.py).
#include "common.h"
#include "launchers.h"
// in.bin: int64 n, s, K, n_kernels, bank_words, pool_bytes, dst_bytes; desc n*11 int64; the bank's doubles; pool bytes.  out.bin: dst
// bytes, which start out as 9s
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long hd[7];
    if (fread(hd, 8, 7, f) != 7) return 2;
    const long long n = hd[0], s = hd[1], K = hd[2], n_kernels = hd[3], bank_words = hd[4], pool_bytes = hd[5], dst_bytes = hd[6];
    std::vector<long long> desc((n > 0 ? n : 1) * 11);
    std::vector<double> bank(bank_words > 0 ? bank_words : 1);
    std::vector<unsigned char> pool(pool_bytes), dst(dst_bytes, 9);
    if (n > 0 && fread(desc.data(), 8, n * 11, f) != (size_t)(n * 11)) return 2;
    if (bank_words > 0 && fread(bank.data(), 8, bank_words, f) != (size_t)bank_words) return 2;
    if (fread(pool.data(), 1, pool_bytes, f) != (size_t)pool_bytes) return 2;
    fclose(f);
    const int rc = pesr_degrade_u8_launch(pool.data(), dst.data(), desc.data(), desc.data(), (int)n, (int)s, (int)K, bank.data(),
                                          (int)n_kernels, nullptr);
    printf("rc %d\n", rc);
    f = fopen(argv[2], "wb");
    fwrite(dst.data(), 1, dst_bytes, f);
    fclose(f);
    return rc;
}
