// jpeg_split_check.cpp -- csrc/jpeg_sync_core.hpp on the CPU: the symbol transition and the subsequence walk of the split
// JPEG decoder, compiled for the host (with -fsanitize=address,undefined by tests/test_jpeg_split_core_host.py) and run over
// a file of dumped scans the way kernels_jpeg_split.hpp runs them, the lanes one after the other: every subsequence from its
// cold state, sweeps in which a lane walks again when its predecessor's exit changed until none changes, the scan of the
// block counts, the writing walk, the DC sums.
//
//   jpeg_split_check DUMP SUB_BYTES
//
// DUMP: the format of jpeg_core_check.cpp.  Output, per scan, two lines: the NINT status words followed by every
// coefficient, component after component, its blocks in grid order, 64 values each; then per subsequence four words, its
// exit from the cold state and its exit from the true state, each as the byte and the packed rest (sync_pack).  The bytes
// are copied into an allocation of exactly NBYTES bytes, so that a read beyond them is an error the sanitizer sees.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../shinestacker_amd/csrc/jpeg_sync_core.hpp"

using namespace mi::jpeg;

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
    std::vector<std::vector<int16_t>>& coef;
    const int *h, *v, *bw;
    int mcus_x;
    long long first_mcu;
    uint32_t B, quota, nbm, status;
    void symbol(const SyncSym& y) {
        if (B >= quota) return;
        status |= y.status;
        if (y.at >= 0 && (y.val != 0 || y.at == 0)) {
            const long long mcu = first_mcu + B / nbm;
            const uint32_t bb = B % nbm, hv = (uint32_t)(h[0] * v[0]);
            const int c = bb < hv ? 0 : (int)(bb - hv) + 1;
            const int by = c == 0 ? (int)bb / h[0] : 0, bx = c == 0 ? (int)bb % h[0] : 0;
            const int my = (int)(mcu / mcus_x), mx = (int)(mcu % mcus_x);
            const size_t b = (size_t)(my * v[c] + by) * bw[c] + (size_t)(mx * h[c] + bx);
            coef[c].at(b * 64 + zigzag(y.at)) = (int16_t)(uint16_t)y.val;
        }
        B += y.done ? 1u : 0u;
    }
    void end() {
        if (B < quota) status |= ST_OVERRUN;
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
        SyncTabs T{};
        T.tabs = tabs.data();
        for (int c = 0; c < nc; ++c) {
            h[c] = c == 0 ? hmax : 1;
            v[c] = c == 0 ? vmax : 1;
            bw[c] = mcus_x * h[c];
            coef[c].assign((size_t)bw[c] * mcus_y * v[c] * 64, (int16_t)0);
            for (int k = 0; k < h[c] * v[c]; ++k) {
                T.dc[T.nbm] = (uint8_t)td[c];
                T.ac[T.nbm] = (uint8_t)ta[c];
                ++T.nbm;
            }
        }
        std::string line, lanes;
        for (int i = 0; i < nint; ++i) {
            const uint32_t o0 = std::min(off[i], nbytes), o1 = std::min(off[i + 1], nbytes);
            const uint32_t len = o1 > o0 ? o1 - o0 : 0u;
            const Bytes src{data + o0};
            const uint32_t nsub = std::max(1u, (len + sub - 1) / sub);
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
            const long long first = (long long)i * dri;
            const long long mcus = first < n_mcus ? std::min((long long)dri, n_mcus - first) : 0;
            uint32_t before = 0, status = 0;
            for (uint32_t j = 0; j < nsub; ++j) {
                SyncState s = j == 0 ? sync_start(0) : sync_unpack(ex[j - 1].p, ex[j - 1].w);
                Writer wr{coef, h, v, bw, mcus_x, first, before, (uint32_t)mcus * T.nbm, T.nbm, 0u};
                uint32_t n = 0;
                sync_lane(src, len, std::min((j + 1) * sub, len), j == nsub - 1, 8 * sub, T, s, n, wr);
                if (!(Exit{s.end ? 0u : s.p, sync_pack(s, n)} == ex[j])) wr.status |= ST_UNSYNCED;
                status |= wr.status;
                before += ex[j].w >> 16;
                lanes += std::to_string(cold[j].p) + ' ' + std::to_string(cold[j].w) + ' ' + std::to_string(ex[j].p) + ' ' +
                         std::to_string(ex[j].w) + ' ';
            }
            line += std::to_string((status & ST_UNSYNCED) ? ST_UNSYNCED : status);
            line += ' ';
        }
        // the DC sums: per component in scan order, from 0 at every interval
        for (int c = 0; c < nc; ++c) {
            uint32_t pred = 0;
            for (int m = 0; m < n_mcus; ++m) {
                if (m % dri == 0) pred = 0;
                const int my = m / mcus_x, mx = m % mcus_x;
                for (int by = 0; by < v[c]; ++by)
                    for (int bx = 0; bx < h[c]; ++bx) {
                        int16_t& d = coef[c][((size_t)(my * v[c] + by) * bw[c] + (size_t)(mx * h[c] + bx)) * 64];
                        pred = (pred + (uint32_t)(uint16_t)d) & 0xffffu;
                        d = (int16_t)(uint16_t)pred;
                    }
            }
        }
        for (int c = 0; c < nc; ++c)
            for (int16_t q : coef[c]) {
                line += std::to_string((int)q);
                line += ' ';
            }
        printf("%s\n%s\n", line.c_str(), lanes.c_str());
        free(data);
    }
    fclose(f);
    return 0;
}
