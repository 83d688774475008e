// jpeg_core.hpp -- the part of the baseline-JPEG decoder (ITU-T T.81, process SOF0, Huffman coded) that meets untrusted bytes:
// the canonical code tables of up to 256 values and the walk over the symbols of one 8 x 8 block.  Plain C++ over
// ljpeg_core.hpp's bit reader, with no intrinsic and no LDS, so that it compiles for the host as well:
// tools/jpeg_core_check.cpp runs it on the CPU under the address and undefined-behaviour sanitizers against
// tests/jpeg_restatement.py, and kernels_jpeg.hpp runs the same lines on the device.
//
//   bits     as ljpeg_core.hpp: most significant bit first, FF 00 is the byte FF, FF before anything else (a restart marker)
//            ends the interval, and every bit at or beyond the end counts as 0
//   DC       the category s from the component's DC table (a value above 15 counts as no code), the difference behind it
//            extended as in T.81 F.2.2.1; the coefficient is the running sum of the differences mod 2^16, as int16
//   AC       up to 63 symbols rs = (r << 4) | s from the AC table, k = 1 at the start:
//              s == 0, r == 15   k += 16 (a k past 63 ends the block with status bit 2)
//              s == 0 otherwise  end of block
//              else              k += r; the s bits behind the code are taken; k <= 63: coef[zigzag[k]] = extend(bits, s),
//                                k += 1; k > 63: the value is dropped, status bit 2, the block ends
//            the block also ends once k passes 63
//   status   bit 0: a 16-bit prefix matched no code (it counts as symbol 0 behind 16 bits); bit 1: bits were taken from
//            beyond the interval's end (set by the caller from BitReader::overrun); bit 2: a run carried k past 63
//
// Every loop here has a constant trip count: nothing waits for the stream to say when to stop.
#pragma once
#include "ljpeg_core.hpp"

namespace mi {
namespace jpeg {

constexpr uint32_t ST_NOCODE = 1u;
constexpr uint32_t ST_OVERRUN = 2u;
constexpr uint32_t ST_RUN = 4u;

// A Huffman table in canonical form (T.81 Annex C), as ljpeg::Huff with room for the 256 values an AC table may hold.
struct Huff256 {
    uint32_t first[17];
    uint16_t count[17];
    uint16_t base[17];
    uint8_t values[256];
};

LJ_HD void huff_build(Huff256& h, const uint8_t counts[16], const uint8_t values[256]) {
    uint32_t code = 0, k = 0;
    h.first[0] = 0; h.count[0] = 0; h.base[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        h.first[l] = code;
        h.count[l] = counts[l - 1];
        h.base[l] = (uint16_t)k;
        k += counts[l - 1];
        code = (code + counts[l - 1]) << 1;
    }
    for (int i = 0; i < 256; ++i) h.values[i] = values[i];
}

// the symbol whose code leads the 16 bits `peek` (bit 15 first), and the code's length; -1 when none does (length 16)
LJ_HD int huff_decode(const Huff256& h, uint32_t peek, int& len) {
    for (int l = 1; l <= 16; ++l) {
        const uint32_t d = (peek >> (16 - l)) - h.first[l];     // (wraps to a huge value below first[l])
        if (d < h.count[l]) {
            len = l;
            return h.values[(h.base[l] + d) & 255u];            // (a table the host forms refuse may count past 256)
        }
    }
    len = 16;
    return -1;
}

// T.81 F.2.2.1 EXTEND of the s-bit value v, mod 2^16 (1 <= s <= 15)
LJ_HD uint32_t extend(uint32_t v, int s) { return (v >> (s - 1)) ? v : (v - ((1u << s) - 1u)) & 0xffffu; }

// natural index of the k-th coefficient in zigzag order
LJ_HD int zigzag(int k) {
    const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return zz[k & 63];
}

// One block: 64 coefficients in natural order into `out` (every one written), `pred` the component's DC predictor.  The
// reader holds 32 bits or more before every symbol: a code of up to 16 bits and up to 15 bits behind it.
template <class Src>
LJ_HD void decode_block(ljpeg::BitReader<Src>& r, const Huff256& dc, const Huff256& ac, uint32_t& pred, int16_t* out,
                        uint32_t& status) {
    for (int j = 0; j < 64; ++j) out[j] = 0;
    int len;
    r.template fill<4>();
    int s = huff_decode(dc, r.peek16(), len);
    r.skip(len);
    if (s < 0 || s > 15) { status |= ST_NOCODE; s = 0; }
    if (s) pred = (pred + extend(r.take(s), s)) & 0xffffu;
    out[0] = (int16_t)(uint16_t)pred;
    int k = 1;
    bool done = false;
    for (int i = 0; i < 63; ++i) {
        if (done) continue;
        r.template fill<4>();
        int rs = huff_decode(ac, r.peek16(), len);
        r.skip(len);
        if (rs < 0) { status |= ST_NOCODE; rs = 0; }
        const int run = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            if (run == 15) {
                k += 16;
                if (k > 63) status |= ST_RUN;
            } else {
                done = true;
            }
        } else {
            k += run;
            const uint32_t v = extend(r.take(sz), sz);
            if (k <= 63) out[zigzag(k)] = (int16_t)(uint16_t)v;
            else status |= ST_RUN;
            k += 1;
        }
        if (k > 63) done = true;
    }
}

}  // namespace jpeg
}  // namespace mi
