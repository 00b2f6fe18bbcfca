// Host-only check of bn.hip's workspace layout (bn_ws_layout): for the Discriminator's eight BatchNorm layers at batch 16, patch 192, and
// for (M, C) = (1, 4), the regions part / sums / dyt lie inside the size pesr_bn_ws_bytes reports, do not overlap, part and dyt start on
// 256 bytes and sums on 16 (it is read as float4); every byte of every region is then written, which is the sanitizer's part.  No GPU
// call is made.  Build and run from the repository root:
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -Ipesr_amd/csrc scripts/bn_ws_check.cpp -o /tmp/bn_ws_check && /tmp/bn_ws_check
#include "../pesr_amd/csrc/bn.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>

// what bn.hip's launchers call in other files of the library; never reached here
int pesr_conv_rgb_in_stats_rows(int, int, int, int) { return 0; }
int pesr_conv_rgb_in_stats_launch(const float*, const float*, float*, float*, int, int, int, int, hipStream_t) { return PESR_EINVAL; }
int pesr_reduce_rows_launch(const float*, double*, int, int, hipStream_t) { return PESR_EINVAL; }

static int check(long M, int C) {
    const size_t bytes = pesr_bn_ws_bytes(M, C);
    char* ws = (char*)aligned_alloc(256, (bytes + 255) / 256 * 256);
    if (!ws) return 1;
    BnWs w;
    int bad = 0;
    if (!bn_ws_layout(M, C, ws, bytes, &w) || !w.dyt || w.bytes != bytes) bad = 1;
    if (!bad) {
        const size_t part_b = (size_t)w.nb * 2 * C * sizeof(double), sums_b = 2 * (size_t)C * sizeof(float), dyt_b = (size_t)M * C * sizeof(float);
        const size_t part_o = (char*)w.part - ws, sums_o = (char*)w.sums - ws, dyt_o = (char*)w.dyt - ws;
        bad |= part_o % 256 || dyt_o % 256 || sums_o % 16;
        bad |= !(part_o + part_b <= sums_o && sums_o + sums_b <= dyt_o && dyt_o + dyt_b <= bytes);
        bad |= w.nb < 1 || w.nb > 512 || w.nb * w.rpb < M || (w.nb - 1) * w.rpb >= M;      // every row in exactly one non-empty block
        if (!bad) { memset(w.part, 1, part_b); memset(w.sums, 2, sums_b); memset(w.dyt, 3, dyt_b); }
        // one byte less than reported: no room for the copy; less than part + sums: refused
        BnWs s;
        bad |= !bn_ws_layout(M, C, ws, bytes - 1, &s) || s.dyt != nullptr;
        bad |= bn_ws_layout(M, C, ws, part_b + sums_b - 1, &s) || bn_ws_layout(M, C, nullptr, bytes, &s);
        printf("M %8ld C %4d: nb %3ld rpb %5ld part@%zu sums@%zu dyt@%zu bytes %zu %s\n", M, C, w.nb, w.rpb, part_o, sums_o, dyt_o, bytes,
               bad ? "BAD" : "ok");
    }
    free(ws);
    return bad;
}

int main() {
    const long hw[8] = {192 * 192, 96 * 96, 96 * 96, 48 * 48, 48 * 48, 24 * 24, 24 * 24, 12 * 12};
    const int ch[8] = {64, 64, 128, 128, 256, 256, 512, 512};
    int bad = check(1, 4);
    for (int i = 0; i < 8; ++i) bad |= check(16 * hw[i], ch[i]);
    puts(bad ? "FAILED" : "all layouts ok");
    return bad;
}
