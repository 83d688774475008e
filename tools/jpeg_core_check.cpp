// jpeg_core_check.cpp -- csrc/jpeg_core.hpp on the CPU: the tables and the block walk that meet untrusted bytes, compiled for
// the host (with -fsanitize=address,undefined by tests/test_jpeg_core_host.py) and run over a file of dumped scans, one
// after the other, serially, interval by interval as jpeg_entropy walks them.
//
//   jpeg_core_check DUMP
//
// DUMP, text: per scan one line "W H NCOMP HMAX VMAX DRI NINT NBYTES HEX" (HEX: the scan's bytes, "-" when empty), one line
// of NINT + 1 offsets, one line of NCOMP pairs "TD TA", and four lines (DC 0, DC 1, AC 0, AC 1) of 16 counts and 256 values.
// Output, per scan: one line of the NINT status words followed by every coefficient, component after component, its blocks
// in grid order, 64 values each.  The bytes are copied into an allocation of exactly NBYTES bytes, so that a read beyond
// them is an error the sanitizer sees.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../shinestacker_amd/csrc/jpeg_core.hpp"

using namespace mi::jpeg;
using mi::ljpeg::BitReader;
using mi::ljpeg::SpanBytes;

static int hexval(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s DUMP\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    int W, H, nc, hmax, vmax, dri, nint;
    unsigned nbytes;
    while (fscanf(f, "%d %d %d %d %d %d %d %u", &W, &H, &nc, &hmax, &vmax, &dri, &nint, &nbytes) == 8) {
        std::string hex(2 * (size_t)nbytes + 2, '\0');
        if (fscanf(f, "%s", &hex[0]) != 1 || nc < 1 || nc > 3 || dri < 1 || nint < 1) return 3;
        uint8_t* data = (uint8_t*)malloc(nbytes ? nbytes : 1);     // exactly as long as the scan
        for (unsigned i = 0; i < nbytes; ++i) data[i] = (uint8_t)(hexval(hex[2 * i]) << 4 | hexval(hex[2 * i + 1]));
        std::vector<uint32_t> off(nint + 1);
        for (int i = 0; i <= nint; ++i)
            if (fscanf(f, "%u", &off[i]) != 1) return 3;
        int td[3], ta[3];
        for (int c = 0; c < nc; ++c)
            if (fscanf(f, "%d %d", &td[c], &ta[c]) != 2) return 3;
        std::vector<Huff256> tabs(4);
        for (int t = 0; t < 4; ++t) {
            uint8_t counts[16], values[256];
            int v;
            for (int i = 0; i < 16; ++i) { if (fscanf(f, "%d", &v) != 1) return 3; counts[i] = (uint8_t)v; }
            for (int i = 0; i < 256; ++i) { if (fscanf(f, "%d", &v) != 1) return 3; values[i] = (uint8_t)v; }
            huff_build(tabs[t], counts, values);
        }
        const int mcus_x = (W + 8 * hmax - 1) / (8 * hmax), mcus_y = (H + 8 * vmax - 1) / (8 * vmax), n_mcus = mcus_x * mcus_y;
        int h[3], v[3], bw[3];
        std::vector<std::vector<int16_t>> coef(nc);
        for (int c = 0; c < nc; ++c) {
            h[c] = c == 0 ? hmax : 1;
            v[c] = c == 0 ? vmax : 1;
            bw[c] = mcus_x * h[c];
            coef[c].assign((size_t)bw[c] * mcus_y * v[c] * 64, (int16_t)0);
        }
        std::string line;
        for (int i = 0; i < nint; ++i) {
            const uint32_t o0 = std::min(off[i], nbytes), o1 = std::min(off[i + 1], nbytes);
            const uint32_t len = o1 > o0 ? o1 - o0 : 0u;
            BitReader<SpanBytes> rd(SpanBytes{data + o0, len, len});
            rd.fill<8>();
            uint32_t status = 0, pred[3] = {0, 0, 0};
            const int first = i * dri, n = first < n_mcus ? std::min(dri, n_mcus - first) : 0;
            for (int m = first; m < first + n; ++m) {
                const int my = m / mcus_x, mx = m % mcus_x;
                for (int c = 0; c < nc; ++c)
                    for (int by = 0; by < v[c]; ++by)
                        for (int bx = 0; bx < h[c]; ++bx) {
                            const size_t b = (size_t)(my * v[c] + by) * bw[c] + (size_t)(mx * h[c] + bx);
                            decode_block(rd, tabs[td[c] & 1], tabs[2 + (ta[c] & 1)], pred[c], &coef[c][b * 64], status);
                        }
            }
            if (rd.overrun()) status |= ST_OVERRUN;
            line += std::to_string(status);
            line += ' ';
        }
        for (int c = 0; c < nc; ++c)
            for (int16_t q : coef[c]) {
                line += std::to_string((int)q);
                line += ' ';
            }
        printf("%s\n", line.c_str());
        free(data);
    }
    fclose(f);
    return 0;
}
