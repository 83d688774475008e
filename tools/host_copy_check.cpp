// host_copy_check.cpp -- csrc/host_copy.hpp on the host, for the sanitizers: copy_rows against a plain row loop over the band
// edge cases (fewer rows than threads, one-row spans split by bytes, a source stride wider than the row), guard bytes around
// the destination, and two caller threads that use the pool at once.  tests/test_host_copy_host.py builds and runs it.
//
//   c++ -std=c++17 -pthread -fsanitize=address,undefined tools/host_copy_check.cpp -o host_copy_check && ./host_copy_check
#include <stdio.h>
#include <stdint.h>
#include <vector>

#include "../shinestacker_amd/csrc/host_copy.hpp"

namespace {

constexpr size_t GUARD = 64;
constexpr unsigned char GUARD_BYTE = 0xA5, STALE_BYTE = 0x5A;

unsigned char source_byte(size_t i, unsigned seed) { return (unsigned char)((i * 131u + seed * 29u + (i >> 8)) & 0xFF); }

// one copy; 0 when the destination equals the row loop's and the guards are untouched
int one_case(size_t rows, size_t row_bytes, size_t stride, int nthr, unsigned seed) {
    // the source ends with its last row: a read past it is the address sanitizer's
    std::vector<unsigned char> src((rows - 1) * stride + row_bytes);
    for (size_t i = 0; i < src.size(); ++i) src[i] = source_byte(i, seed);
    const size_t n = rows * row_bytes;
    std::vector<unsigned char> want(n), buf(GUARD + n + GUARD, GUARD_BYTE);
    for (size_t y = 0; y < rows; ++y)
        for (size_t x = 0; x < row_bytes; ++x) want[y * row_bytes + x] = src[y * stride + x];
    memset(buf.data() + GUARD, STALE_BYTE, n);
    mi::copy_rows(buf.data() + GUARD, src.data(), stride, row_bytes, rows, nthr);
    int bad = memcmp(buf.data() + GUARD, want.data(), n) != 0;
    for (size_t i = 0; i < GUARD; ++i) bad |= buf[i] != GUARD_BYTE || buf[GUARD + n + i] != GUARD_BYTE;
    if (bad) fprintf(stderr, "copy_rows differs: rows %zu, row bytes %zu, stride %zu, %d threads\n", rows, row_bytes, stride, nthr);
    return bad;
}

}  // namespace

int main() {
    int bad = 0, cases = 0;
    if (mi::copy_threads(((size_t)32 << 20) - 1) != 1 || mi::copy_threads((size_t)32 << 20) != 4) {
        fprintf(stderr, "copy_threads: 4 threads from 32 MiB, else 1\n");
        bad = 1;
    }
    unsigned seed = 0;
    for (size_t rows : {1, 3, 4, 5, 7})
        for (size_t row_bytes : {1, 13, 4096})
            for (size_t extra : {0, 5})
                for (int nthr : {1, 4}) { bad |= one_case(rows, row_bytes, row_bytes + extra, nthr, ++seed); ++cases; }
    // a packed span: one row, split by bytes
    for (size_t bytes : {1, 3, 1000})
        for (int nthr : {1, 4}) { bad |= one_case(1, bytes, bytes, nthr, ++seed); ++cases; }
    // two callers at once: the pool takes one copy at a time
    int bad_thread[2] = {0, 0};
    std::thread callers[2];
    for (int c = 0; c < 2; ++c)
        callers[c] = std::thread([c, &bad_thread] {
            for (unsigned k = 0; k < 50; ++k) {
                bad_thread[c] |= one_case(7, 4096, 4096 + 5 * (size_t)c, 4, 1000u * (c + 1) + k);
                bad_thread[c] |= one_case(1, 1000, 1000, 4, 3000u * (c + 1) + k);
            }
        });
    for (auto& t : callers) t.join();
    cases += 200;
    bad |= bad_thread[0] | bad_thread[1];
    if (!bad) printf("ok %d\n", cases);
    return bad;
}
