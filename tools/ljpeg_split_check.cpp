// ljpeg_split_check.cpp -- csrc/ljpeg_sync_core.hpp on the CPU: the symbol transition and the subsequence walk of the split
// lossless-JPEG decoder, compiled for the host (with -fsanitize=address,undefined by tests/test_ljpeg_split_core_host.py) and
// run over a file of dumped segments the way kernels_ljpeg_split.hpp runs them, the lanes one after the other: the tables and
// their lookup, every subsequence from its cold state, sweeps in which a lane walks again when its predecessor's exit changed
// until none changes, the scan of the sample counts, the writing walk.
//
//   ljpeg_split_check DUMP SUB_BYTES
//
// DUMP, per segment: NCOMP ROWS COLUMNS NBYTES HEX (NBYTES bytes of entropy-coded data as hex digits, "-"
// for none), then per component 16 counts and 17 values.  Output, per segment, two lines: the status word followed by the
// ROWS x COLUMNS differences; then per subsequence four words, its exit from the cold state and its exit from the true state,
// each as the byte and the packed rest (sync_pack).  The bytes are copied into an allocation of exactly NBYTES bytes, so that a
// read beyond them is an error the sanitizer sees.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../shinestacker_amd/csrc/ljpeg_sync_core.hpp"

using namespace mi::ljpeg;

static int hexval(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

struct Bytes {
    const uint8_t* p;
    uint32_t byte(uint32_t i) const { return p[i]; }
};
struct Exit {
    uint32_t p, w;
    bool operator==(const Exit& o) const { return p == o.p && w == o.w; }
};

struct Writer {
    std::vector<uint16_t>& plane;
    uint32_t at, quota, status;
    void symbol(const SyncSym& y) {
        if (at >= quota) return;
        status |= y.status;
        plane.at(at) = (uint16_t)y.val;
        ++at;
    }
    void end() {
        if (at < quota) status |= ST_OVERRUN;
    }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s DUMP SUB_BYTES\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    const uint32_t sub = (uint32_t)atoi(argv[2]);
    if (sub < 8 || sub > 128) return 2;
    int nc, rows, cols;
    unsigned nbytes;
    while (fscanf(f, "%d %d %d %u", &nc, &rows, &cols, &nbytes) == 4) {
        std::string hex(2 * (size_t)nbytes + 2, '\0');
        if (fscanf(f, "%s", &hex[0]) != 1 || nc < 1 || nc > 2 || rows < 0 || cols < 0) return 3;
        uint8_t* data = (uint8_t*)malloc(nbytes ? nbytes : 1);     // exactly as long as the data
        for (unsigned i = 0; i < nbytes; ++i) data[i] = (uint8_t)(hexval(hex[2 * i]) << 4 | hexval(hex[2 * i + 1]));
        Huff tabs[2];
        memset(tabs, 0, sizeof(tabs));
        for (int c = 0; c < nc; ++c) {
            uint8_t counts[16], values[17];
            int v;
            for (int i = 0; i < 16; ++i) { if (fscanf(f, "%d", &v) != 1) return 3; counts[i] = (uint8_t)v; }
            for (int i = 0; i < 17; ++i) { if (fscanf(f, "%d", &v) != 1) return 3; values[i] = (uint8_t)v; }
            huff_build(tabs[c], counts, values);
        }
        std::vector<uint16_t> lut((size_t)nc << SYNC_LUT_BITS);     // ljpeg_split_prep's
        for (size_t j = 0; j < lut.size(); ++j) {
            int len;
            const int s = huff_decode(tabs[j >> SYNC_LUT_BITS], (uint32_t)(j & ((1u << SYNC_LUT_BITS) - 1)) << (16 - SYNC_LUT_BITS), len);
            lut[j] = s >= 0 && s <= 16 && len <= SYNC_LUT_BITS ? (uint16_t)(len << 8 | s) : (uint16_t)0;
        }
        const SyncTabs T{tabs, lut.data(), (uint32_t)nc};
        const uint32_t len = sync_data_len(0, nbytes, nbytes);
        const Bytes src{data};
        const uint32_t nsub = sync_nsub(len, sub);
        SyncNoEmit none;
        auto walk = [&](uint32_t j, Exit e) {
            SyncState s = j == 0 ? sync_start(0) : sync_unpack(e.p, e.w);
            uint32_t n = 0;
            sync_lane(src, len, std::min((j + 1) * sub, len), j == nsub - 1, 8 * sub, T, s, n, none);
            return Exit{s.end ? 0u : s.p, sync_pack(s, n)};
        };
        std::vector<Exit> cold(nsub), ex(nsub);
        std::vector<char> need(nsub), chg(nsub);
        for (uint32_t j = 0; j < nsub; ++j) {
            const SyncState c = sync_cold(src, len, j * sub);
            cold[j] = ex[j] = walk(j, Exit{c.p, sync_pack(c, 0)});
            need[j] = j > 0;
        }
        for (uint32_t sweep = 0; sweep < nsub; ++sweep) {      // the kernel's iteration, all groups as one
            std::vector<Exit> nw(ex);
            bool any = false;
            for (uint32_t j = 1; j < nsub; ++j) {
                chg[j] = 0;
                if (!need[j]) continue;
                nw[j] = walk(j, Exit{ex[j - 1].p, ex[j - 1].w & 0xffffu});
                chg[j] = !(nw[j] == ex[j]);
            }
            ex = nw;
            for (uint32_t j = nsub - 1; j >= 1; --j) {
                need[j] = j > 1 ? chg[j - 1] : 0;
                any = any || need[j];
            }
            if (!any) break;
        }
        const uint32_t quota = (uint32_t)rows * (uint32_t)cols;
        std::vector<uint16_t> plane(quota, (uint16_t)0);
        uint32_t before = 0, status = 0;
        std::string lanes;
        for (uint32_t j = 0; j < nsub; ++j) {
            SyncState s = j == 0 ? sync_start(0) : sync_unpack(ex[j - 1].p, ex[j - 1].w);
            Writer wr{plane, before, quota, 0u};
            uint32_t n = 0;
            sync_lane(src, len, std::min((j + 1) * sub, len), j == nsub - 1, 8 * sub, T, s, n, wr);
            if (!(Exit{s.end ? 0u : s.p, sync_pack(s, n)} == ex[j])) wr.status |= ST_UNSYNCED;
            status |= wr.status;
            before += ex[j].w >> 16;
            lanes += std::to_string(cold[j].p) + ' ' + std::to_string(cold[j].w) + ' ' + std::to_string(ex[j].p) + ' ' +
                     std::to_string(ex[j].w) + ' ';
        }
        std::string line = std::to_string((status & ST_UNSYNCED) ? ST_UNSYNCED : status);
        for (uint16_t d : plane) {
            line += ' ';
            line += std::to_string((unsigned)d);
        }
        printf("%s\n%s\n", line.c_str(), lanes.c_str());
        free(data);
    }
    fclose(f);
    return 0;
}
