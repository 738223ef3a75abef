// select_check.cpp -- the selection rule of preemptive matching (csrc/sift_select.h) on the host:
// includes only that header, so that g++ builds it without HIP, under AddressSanitizer and UBSan
// (tests/test_select.py).
//
//   select_check                 self-test: select_host against a stable sort of the order keys on
//                                small random sets with many ties; prints "select ok"
//   select_check <in> <out>      file mode: runs select_host on the cases of <in> and writes the
//                                selections to <out>
// <in>:  int32 cases, then per case int32 n, stride, top and n * stride float32 (row r's scale at
//        r * stride).   <out>: per case int32 m, then m int32 row indices.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "sift_select.h"

namespace {

bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int file_mode(const char* in_path, const char* out_path) {
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) return fprintf(stderr, "cannot open the case files\n"), 2;
    int32_t cases = 0;
    if (!read_all(in, &cases, sizeof(cases)) || cases < 0) return fprintf(stderr, "bad header\n"), 2;
    for (int c = 0; c < cases; c++) {
        int32_t hdr[3];
        if (!read_all(in, hdr, sizeof(hdr)) || hdr[0] < 0 || hdr[1] < 1)
            return fprintf(stderr, "bad case %d\n", c), 2;
        const int n = hdr[0], stride = hdr[1], top = hdr[2];
        std::vector<float> scale((size_t)n * stride);
        if (!read_all(in, scale.data(), scale.size() * sizeof(float)))
            return fprintf(stderr, "short case %d\n", c), 2;
        // exactly the capacity the rule promises to stay within
        std::vector<int> sel((size_t)std::max(0, std::min(n, top)));
        const int32_t m = sgsel::select_host(scale.data(), stride, n, top, sel.data());
        if (m != (int32_t)sel.size()) return fprintf(stderr, "case %d: m = %d\n", c, m), 1;
        fwrite(&m, sizeof(m), 1, out);
        if (m > 0) fwrite(sel.data(), sizeof(int), sel.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}

uint32_t rng_state = 12345u;
uint32_t rnd() {   // xorshift32
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

int self_test() {
    // order_key is monotone over the floats and total over the bit patterns
    const float ordered[] = {-1e30f, -2.0f, -1e-40f, -0.0f, 0.0f, 1e-40f, 1.0f, 2.0f, 1e30f};
    for (size_t i = 0; i + 1 < sizeof(ordered) / sizeof(ordered[0]); i++) {
        uint32_t a, b;
        memcpy(&a, &ordered[i], 4);
        memcpy(&b, &ordered[i + 1], 4);
        if (!(sgsel::order_key(a) < sgsel::order_key(b))) return printf("order_key not monotone at %zu\n", i), 1;
    }
    if (sgsel::order_key(0x7f800000u) <= sgsel::order_key(0x7f7fffffu)) return printf("+inf\n"), 1;
    if (sgsel::order_key(0xff800000u) >= sgsel::order_key(0xff7fffffu)) return printf("-inf\n"), 1;
    for (int iter = 0; iter < 3000; iter++) {
        const int n = (int)(rnd() % 300), stride = 1 + (int)(rnd() % 3), top = 1 + (int)(rnd() % 320);
        const int values = 1 + (int)(rnd() % 6);   // few distinct values: ties at most cuts
        std::vector<float> scale((size_t)n * stride, -7.0f);
        for (int i = 0; i < n; i++) {
            const uint32_t bits = iter % 3 == 0 ? rnd() : 0x3f800000u + (rnd() % values) * 0x01010101u;
            memcpy(&scale[(size_t)i * stride], &bits, 4);
        }
        std::vector<int> order(n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            return sgsel::scale_key(scale.data(), stride, a) > sgsel::scale_key(scale.data(), stride, b);
        });
        const int m = std::min(n, top);
        std::vector<int> want(order.begin(), order.begin() + m);
        std::sort(want.begin(), want.end());
        std::vector<int> got((size_t)m);
        if (sgsel::select_host(scale.data(), stride, n, top, got.data()) != m || got != want)
            return printf("select_host differs: iter %d n %d top %d\n", iter, n, top), 1;
    }
    int none = -1;
    if (sgsel::select_host(nullptr, 1, 0, 5, &none) != 0 || none != -1) return printf("empty set\n"), 1;
    std::vector<int64_t> sub;
    const int64_t off[] = {0, 0, 3, 103, 203};
    sgsel::subset_offsets(off, 4, 100, sub);
    if (sub != std::vector<int64_t>{0, 0, 3, 103, 203}) return printf("subset_offsets\n"), 1;
    sgsel::subset_offsets(off, 4, 2, sub);
    if (sub != std::vector<int64_t>{0, 0, 2, 4, 6}) return printf("subset_offsets (cut)\n"), 1;
    printf("select ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3) return file_mode(argv[1], argv[2]);
    if (argc == 1) return self_test();
    fprintf(stderr, "usage: select_check [<cases in> <selections out>]\n");
    return 2;
}
