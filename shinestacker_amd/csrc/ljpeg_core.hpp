// ljpeg_core.hpp -- the part of the lossless-JPEG decoder (ITU-T T.81, process SOF3, Huffman coded) that meets untrusted bytes:
// the canonical code tables, the bit reader and the decode of one difference.  Plain C++ over a byte source, with no
// intrinsic and no LDS, so that it compiles for the host as well: tools/ljpeg_core_check.cpp runs it on the CPU under the
// address and undefined-behaviour sanitizers against tests/ljpeg_restatement.py, and kernels_ljpeg.hpp runs the same lines on
// the device.
//
//   bits     the data bytes most significant bit first; FF 00 yields the byte FF; FF before anything else is a marker: it ends
//            the data, and every bit at or beyond it counts as 0, as does every bit beyond the data's length or the span's end
//   sample   the category s from the component's table; s = 0: difference 0; s = 16: 32768, no further bits; else s bits v,
//            the difference v when v >= 2^(s-1) and v - (2^s - 1) otherwise
//   status   bit 0: a 16-bit prefix matched no code (the sample counts as category 0 behind 16 bits); bit 1: bits were taken
//            from beyond the end of the data
//
// Every loop here has a constant trip count: nothing waits for the stream to say when to stop.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LJ_HD __host__ __device__ inline
#else
#define LJ_HD inline
#endif

namespace mi {
namespace ljpeg {

constexpr uint32_t ST_NOCODE = 1u;    // a 16-bit prefix matched no code
constexpr uint32_t ST_OVERRUN = 2u;   // the last sample needed bits from beyond the end of the data

// A component's Huffman table in canonical form (T.81 Annex C): the codes of length l are first[l] .. first[l] + count[l] - 1,
// their categories values[base[l]] onwards.
struct Huff {
    uint32_t first[17];
    uint16_t count[17];
    uint16_t base[17];
    uint8_t values[17];
};

LJ_HD void huff_build(Huff& h, const uint8_t counts[16], const uint8_t values[17]) {
    uint32_t code = 0, k = 0;
    h.first[0] = 0; h.count[0] = 0; h.base[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        h.first[l] = code;
        h.count[l] = counts[l - 1];
        h.base[l] = (uint16_t)k;
        k += counts[l - 1];
        code = (code + counts[l - 1]) << 1;
    }
    for (int i = 0; i < 17; ++i) h.values[i] = values[i];
}

// the category whose code leads the 16 bits `peek` (bit 15 first), and the code's length; -1 when none does (length 16)
LJ_HD int huff_decode(const Huff& h, uint32_t peek, int& len) {
    for (int l = 1; l <= 16; ++l) {
        const uint32_t d = (peek >> (16 - l)) - h.first[l];     // (wraps to a huge value below first[l])
        if (d < h.count[l]) {
            const uint32_t i = h.base[l] + d;
            len = l;
            return h.values[i < 16 ? i : 16];
        }
    }
    len = 16;
    return -1;
}

// A byte source over a pointer and two lengths: byte i of the entropy-coded data, 0 at or beyond `data_bytes` (the segment's
// data) and at or beyond `span_left` (what the span holds from the data's first byte on).
struct SpanBytes {
    const uint8_t* p;
    uint32_t data_bytes, span_left;
    LJ_HD uint32_t limit() const { return data_bytes < span_left ? data_bytes : span_left; }
    LJ_HD uint32_t byte(uint32_t i) const { return i < limit() ? (uint32_t)p[i] : 0u; }
};

// The bit reader.  `acc` holds `nbits` unread bits from bit 63 down.  `fill<N>` takes up to N source bytes (constant trip
// count) while eight more bits fit; a sample reads at most 31 bits, so fill<8> at the start and fill<4> before every sample
// keep 32 bits or more in hand.
template <class Src>
struct BitReader {
    Src src;
    uint64_t acc = 0;
    int nbits = 0;
    uint32_t pos = 0;          // the next source byte
    uint32_t loaded = 0;       // bytes put into acc, the zeros behind the end included
    uint32_t real = 0;         // ... of which lay in front of the end
    bool ended = false;        // a marker or the end of the data was met

    LJ_HD explicit BitReader(const Src& s) : src(s) {}

    // Written as selects over the byte and the one behind it, not as nested branches.  Observed with the branchy form
    // (`b = byte(pos++); if (b == 0xff) { if (byte(pos) == 0) ++pos; else { ended = true; return 0; } } ++real; return b;`)
    // built by hipcc of ROCm 7.2.0 with -O3 for gfx950, inlined into fill<N> inside raw_ljpeg: every stream with a stuffed FF
    // decoded wrongly on the device while the same source passed on the host under ASan and UBSan --
    // tests/test_gpu_ljpeg.py::test_ljpeg_equals_the_restatement[12bit-ones], whose data is FF 00 FF 00 FF 00 ..., came back
    // with every difference 0, and [12bit-5x17-nf1] went wrong from the sample that holds its first FF 00.  In the kernel's
    // assembly the b == 0xff path ended in `v_mov_b64 v[2:3], 0` for the stuffed and the marker case alike, and 0xff was never
    // ORed into the window.  Not reduced to a stand-alone case.  To re-check after a compiler update: restore the branchy form
    // and run those two cases.
    LJ_HD uint32_t next_byte() {
        const uint32_t lim = src.limit();
        const bool live = !ended && pos < lim;
        const uint32_t b = live ? src.byte(pos) : 0u;
        const uint32_t n = live ? src.byte(pos + 1) : 0u;          // (0 beyond the data: an FF as the very last byte reads as FF)
        const bool marker = b == 0xffu && n != 0u;                  // FF before anything but 00 ends the data
        const bool stuffed = b == 0xffu && n == 0u && pos + 1 < lim;   // FF 00 is the byte FF
        ended = !live || marker;
        pos += live && !marker ? (stuffed ? 2u : 1u) : 0u;
        real += live && !marker ? 1u : 0u;
        return marker ? 0u : b;
    }
    template <int N>
    LJ_HD void fill() {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (nbits <= 56) {
                acc |= (uint64_t)next_byte() << (56 - nbits);
                nbits += 8;
                ++loaded;
            }
    }
    LJ_HD uint32_t peek16() const { return (uint32_t)(acc >> 48); }
    LJ_HD void skip(int n) { acc <<= n; nbits -= n; }
    LJ_HD uint32_t take(int n) {        // 1 <= n <= 16
        const uint32_t v = (uint32_t)(acc >> (64 - n));
        skip(n);
        return v;
    }
    // bits taken so far beyond the last bit of the data
    LJ_HD bool overrun() const { return (uint64_t)loaded * 8 - (uint64_t)nbits > (uint64_t)real * 8; }
};

// the difference behind category s (mod 2^16), s bits taken from the reader
template <class Src>
LJ_HD uint32_t take_difference(BitReader<Src>& r, int s) {
    if (s == 0) return 0u;
    if (s >= 16) return 32768u;
    const uint32_t v = r.take(s);
    return (v >> (s - 1)) ? v : (v - ((1u << s) - 1u)) & 0xffffu;
}

// one difference (mod 2^16) with the table `h`; the caller has filled the reader
template <class Src>
LJ_HD uint32_t decode_difference(BitReader<Src>& r, const Huff& h, uint32_t& status) {
    int len;
    int s = huff_decode(h, r.peek16(), len);
    r.skip(len);
    if (s < 0 || s > 16) { status |= ST_NOCODE; s = 0; }
    return take_difference(r, s);
}

}  // namespace ljpeg
}  // namespace mi
