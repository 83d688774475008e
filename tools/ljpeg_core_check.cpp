// ljpeg_core_check.cpp -- csrc/ljpeg_core.hpp on the CPU: the bit reader and the one-symbol decode that meet untrusted bytes,
// compiled for the host (with -fsanitize=address,undefined by tests/test_ljpeg_core_host.py) and run over a file of dumped
// streams, one segment after the other, serially.
//
//   ljpeg_core_check DUMP
//
// DUMP, text: per segment one line "P Y X Nf Ss NBYTES HEX" (HEX: the entropy-coded data, "-" when empty) and Nf lines of 16
// counts and 17 values.  Output, per segment: one line "STATUS v v v ..." with the Y * X * Nf samples in stream order.
// The data is copied into an allocation of exactly NBYTES bytes, so that a read beyond it is an error the sanitizer sees.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../shinestacker_amd/csrc/ljpeg_core.hpp"

using namespace mi::ljpeg;

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
    int P, Y, X, Nf, Ss;
    unsigned nbytes;
    while (fscanf(f, "%d %d %d %d %d %u", &P, &Y, &X, &Nf, &Ss, &nbytes) == 6) {
        std::string hex(2 * (size_t)nbytes + 2, '\0');
        if (fscanf(f, "%s", &hex[0]) != 1 || Nf < 1 || Nf > 2) return 3;
        uint8_t* data = (uint8_t*)malloc(nbytes ? nbytes : 1);     // exactly as long as the data
        for (unsigned i = 0; i < nbytes; ++i) data[i] = (uint8_t)(hexval(hex[2 * i]) << 4 | hexval(hex[2 * i + 1]));
        Huff h[2];
        for (int c = 0; c < Nf; ++c) {
            uint8_t counts[16], values[17];
            int v;
            for (int i = 0; i < 16; ++i) { if (fscanf(f, "%d", &v) != 1) return 3; counts[i] = (uint8_t)v; }
            for (int i = 0; i < 17; ++i) { if (fscanf(f, "%d", &v) != 1) return 3; values[i] = (uint8_t)v; }
            huff_build(h[c], counts, values);
        }
        const int W = X * Nf;
        std::vector<uint32_t> prev(W, 0), cur(W, 0);
        std::string line;
        uint32_t status = 0;
        BitReader<SpanBytes> rd(SpanBytes{data, nbytes, nbytes});
        rd.fill<8>();
        for (int r = 0; r < Y; ++r) {
            for (int col = 0; col < W; ++col) {
                rd.fill<4>();
                const uint32_t d = decode_difference(rd, h[col % Nf], status);
                int px;
                if (r == 0 && col < Nf) px = 1 << (P - 1);
                else if (r == 0) px = (int)cur[col - Nf];
                else if (col < Nf) px = (int)prev[col];
                else {
                    const int Ra = (int)cur[col - Nf], Rb = (int)prev[col], Rc = (int)prev[col - Nf];
                    switch (Ss) {
                        case 1: px = Ra; break;
                        case 2: px = Rb; break;
                        case 3: px = Rc; break;
                        case 4: px = Ra + Rb - Rc; break;
                        case 5: px = Ra + ((Rb - Rc) >> 1); break;
                        case 6: px = Rb + ((Ra - Rc) >> 1); break;
                        default: px = (Ra + Rb) >> 1; break;
                    }
                }
                cur[col] = ((uint32_t)px + d) & 0xffffu;
                line += ' ';
                line += std::to_string(cur[col]);
            }
            prev.swap(cur);
        }
        if (rd.overrun()) status |= ST_OVERRUN;
        printf("%u%s\n", status, line.c_str());
        free(data);
    }
    fclose(f);
    return 0;
}
