// ljpeg_sync_core.hpp -- the transition of the split lossless-JPEG decoder (kernels_ljpeg_split.hpp): one Huffman symbol of a
// SOF3 scan taken from a decoder STATE, and the walk of one subsequence of a segment from an entry state to its exit.  The
// counterpart of jpeg_sync_core.hpp, whose head has the scheme and the reasoning; here the state is smaller -- a symbol is a
// sample, so only the bit position and the component are carried -- and what comes out are differences mod 2^16, which
// prefix sums turn into samples afterwards.  Plain C++ over ljpeg_core.hpp's Huff, huff_decode and difference rule, with no
// intrinsic and no LDS, so that it compiles for the host as well: tools/ljpeg_split_check.cpp runs it on the CPU under the
// address and undefined-behaviour sanitizers against tests/ljpeg_split_restatement.py, and kernels_ljpeg_split.hpp runs the
// same lines on the device.
//
//   data         `len` = min(scan_bytes, span_bytes - scan_off) bytes behind a byte source (`src.byte(i)`, asked only for
//                i < len).  They end at the first FF followed by anything but 00 (an FF that is the very last byte reads as
//                FF), else at `len`; bits beyond the end are 0.  BitReader::next_byte's rule, restated.
//   state        (p, q, c) at a symbol boundary: p the byte that holds the next unread bit -- never the 00 of an FF 00 pair
//                --, q the bits of it already read, c the component of the next sample; or `end`, once a symbol would start
//                at or beyond the data's end.
//   symbol       exactly ljpeg_core.hpp's decode_difference: the category from component c's table, a 16-bit prefix that
//                leads no code or a category above 16 counts as category 0 behind 16 bits and sets ST_NOCODE; category 16 is
//                32768 with no further bits, else s bits follow.  At most 7 + 16 + 15 = 38 bits from p on: five data bytes,
//                ten source bytes when every one is stuffed.  A symbol that takes bits from beyond the end sets ST_OVERRUN
//                and leaves p at the end: the next one is `end`.
//   ownership    a subsequence [lo, hi) owns the symbols whose first bit lies in it, the segment's last one everything
//                behind it too; a lane whose entry lies at or beyond hi walks nothing and passes the state through.  The cold
//                state of a subsequence is (lo, 0, 0), one byte later where lo is a stuffed 00.
//
// The byte reader is written as selects, not branches: the compiler note in ljpeg_core.hpp (BitReader::next_byte) applies.
// Every loop has a trip count fixed by the geometry: five bytes a symbol, 8 * sub_bytes + 1 symbols a subsequence.
#pragma once
#include "ljpeg_core.hpp"

namespace mi {
namespace ljpeg {

constexpr uint32_t ST_UNSYNCED = 8u;    // a lane's entry was not its predecessor's exit: the rounds enqueued were too few
constexpr int SYNC_LUT_BITS = 10;       // the optional lookup: 2^10 entries a component, length << 8 | category, 0: search

struct SyncState {
    uint32_t p;
    uint32_t q, c;
    bool end;
};
LJ_HD SyncState sync_start(uint32_t p) { return SyncState{p, 0u, 0u, false}; }
// two words: p, and q | c << 3 | end << 4 | n << 16 (n: the samples of the lane, at most 8 * 128)
LJ_HD uint32_t sync_pack(const SyncState& s, uint32_t n) { return s.end ? (1u << 4) | (n << 16) : s.q | (s.c << 3) | (n << 16); }
LJ_HD SyncState sync_unpack(uint32_t p, uint32_t w) {
    const bool end = (w >> 4) & 1u;
    return SyncState{end ? 0u : p, end ? 0u : w & 7u, end ? 0u : (w >> 3) & 1u, end};
}

// the tables of a segment's components; `lut` may be null
struct SyncTabs {
    const Huff* tabs;
    const uint16_t* lut;    // ncomp << SYNC_LUT_BITS entries
    uint32_t ncomp;         // 1 or 2
};

// what a symbol did: status bits and the difference mod 2^16
struct SyncSym {
    uint32_t status;
    uint32_t val;
};

// One symbol from `s`.  False, with s.end set, when it would start at or beyond the data's end.
template <class Src>
LJ_HD bool sync_symbol(const Src& src, uint32_t len, const SyncTabs& T, SyncState& s, SyncSym& y) {
    uint32_t pos = s.p, rp[6];
    uint64_t w = 0;
    uint32_t nlive = 0;
    bool ended = false;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        rp[i] = pos;
        const bool live = !ended && pos < len;
        const uint32_t b = live ? src.byte(pos) : 0u;
        const uint32_t n = live && pos + 1 < len ? src.byte(pos + 1) : 0u;
        const bool marker = b == 0xffu && n != 0u;
        const bool stuffed = b == 0xffu && n == 0u && pos + 1 < len;
        const bool take = live && !marker;
        ended = !take;
        pos += take ? (stuffed ? 2u : 1u) : 0u;
        nlive += take ? 1u : 0u;
        w |= (uint64_t)(take ? b : 0u) << (32 - 8 * i);
    }
    rp[5] = pos;
    if (nlive == 0) {
        s.end = true;
        return false;
    }
    const uint32_t c = s.c < T.ncomp ? s.c : 0u;
    const uint32_t peek = (uint32_t)(w >> (24 - s.q)) & 0xffffu;
    const uint32_t e = T.lut ? (uint32_t)T.lut[(c << SYNC_LUT_BITS) + (peek >> (16 - SYNC_LUT_BITS))] : 0u;
    int len_code = (int)(e >> 8), sz = (int)(e & 0xffu);
    y.status = 0;
    if (!e) {
        sz = huff_decode(T.tabs[c], peek, len_code);
        if (sz < 0 || sz > 16) { y.status |= ST_NOCODE; sz = 0; }
    }
    const int extra = sz < 16 ? sz : 0;
    uint32_t val = sz >= 16 ? 32768u : 0u;
    if (extra) {
        const uint32_t v = (uint32_t)(w >> (40 - (int)s.q - len_code - extra)) & ((1u << extra) - 1u);
        val = (v >> (extra - 1)) ? v : (v - ((1u << extra) - 1u)) & 0xffffu;
    }
    y.val = val;
    const uint32_t t = s.q + (uint32_t)len_code + (uint32_t)extra;     // at most 7 + 16 + 15
    const bool over = t > 8u * nlive;
    const uint32_t a = over ? nlive : t >> 3;
    uint32_t np = rp[0];
#pragma unroll
    for (uint32_t i = 1; i < 6; ++i) np = a == i ? rp[i] : np;
    if (over) y.status |= ST_OVERRUN;
    s.p = np;
    s.q = over ? 0u : t & 7u;
    s.c = c + 1 < T.ncomp ? c + 1 : 0u;
    return true;
}

// the cold state of the subsequence that starts at byte `lo`
template <class Src>
LJ_HD SyncState sync_cold(const Src& src, uint32_t len, uint32_t lo) {
    const bool stuffed = lo > 0 && lo < len && src.byte(lo - 1) == 0xffu && src.byte(lo) == 0u;
    return sync_start(stuffed ? lo + 1 : lo);
}

// The walk of the subsequence that ends at `hi` (`last`: the segment's last, which owns everything behind it) from the entry
// state `s`, which becomes the exit; the samples decoded are added to `n`.  `emit.symbol(y)` sees every symbol in turn,
// `emit.end()` the moment the walk meets the data's end.  max_symbols: 8 * sub_bytes, what the subsequence can hold.
template <class Src, class Emit>
LJ_HD void sync_lane(const Src& src, uint32_t len, uint32_t hi, bool last, uint32_t max_symbols, const SyncTabs& T, SyncState& s,
                     uint32_t& n, Emit& emit) {
    for (uint32_t it = 0; it <= max_symbols; ++it) {
        if (s.end || (!last && s.p >= hi)) break;
        SyncSym y;
        if (!sync_symbol(src, len, T, s, y)) {
            emit.end();
            break;
        }
        emit.symbol(y);
        n += 1u;
    }
}

struct SyncNoEmit {
    LJ_HD void symbol(const SyncSym&) {}
    LJ_HD void end() {}
};

// the geometry the host and the kernels share: a segment's data and its subsequences
LJ_HD uint32_t sync_data_len(uint32_t scan_off, uint32_t scan_bytes, uint32_t span_bytes) {
    return scan_off < span_bytes ? (scan_bytes < span_bytes - scan_off ? scan_bytes : span_bytes - scan_off) : 0u;
}
LJ_HD uint32_t sync_nsub(uint32_t len, uint32_t sub) {
    const uint32_t n = len / sub + (len % sub ? 1u : 0u);
    return n ? n : 1u;
}

}  // namespace ljpeg
}  // namespace mi
