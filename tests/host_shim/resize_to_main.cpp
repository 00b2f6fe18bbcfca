// Runs pesr_resize_to_u8_pass_launch of csrc/resize_to.hip, compiled for the host, on one call read from a file
// (tests/test_resize_to_host_cpu.py).
#include "common.h"
#include "launchers.h"
// in.bin: int64 n, axis, pool_bytes, table_words, dst_bytes; desc n*12 int64; the table words; pool bytes.  out.bin: dst bytes, which
// start out as 9s
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long hd[5];
    if (fread(hd, 8, 5, f) != 5) return 2;
    const long long n = hd[0], axis = hd[1], pool_bytes = hd[2], table_words = hd[3], dst_bytes = hd[4];
    const long long nd = n > 0 ? n : 1;
    std::vector<long long> desc(nd * 12), table(table_words > 0 ? table_words : 1);
    std::vector<unsigned char> pool(pool_bytes), dst(dst_bytes, 9);
    if (n > 0 && fread(desc.data(), 8, n * 12, f) != (size_t)(n * 12)) return 2;
    if (table_words > 0 && fread(table.data(), 8, table_words, f) != (size_t)table_words) return 2;
    if (fread(pool.data(), 1, pool_bytes, f) != (size_t)pool_bytes) return 2;
    fclose(f);
    const int rc = pesr_resize_to_u8_pass_launch(pool.data(), dst.data(), desc.data(), desc.data(), (int)n, (int)axis, table.data(),
                                                 (long)table_words, nullptr);
    printf("rc %d\n", rc);
    f = fopen(argv[2], "wb");
    fwrite(dst.data(), 1, dst_bytes, f);
    fclose(f);
    return rc;
}
