// jpeg_sync_core.hpp -- the transition of the split entropy decoder (kernels_jpeg_split.hpp): one Huffman symbol of a baseline
// scan taken from a decoder STATE, and the walk of one subsequence of a restart interval from an entry state to its exit.
// Huffman streams re-synchronise: a decoder started at an arbitrary byte soon falls into step with the true one, so an
// interval of any length is cut into subsequences, every one is walked from a guess, and the guesses are repaired until each
// lane's entry is its predecessor's exit (Weissenberger and Schmidt's self-synchronising scheme).  Plain C++ over
// jpeg_core.hpp's tables, with no intrinsic and no LDS, so that it compiles for the host as well:
// tools/jpeg_split_check.cpp runs it on the CPU under the address and undefined-behaviour sanitizers against
// tests/jpeg_split_restatement.py, and kernels_jpeg_split.hpp runs the same lines on the device.
//
//   interval     `len` bytes behind a byte source (`src.byte(i)`, asked only for i < len).  Its data end at the first FF
//                followed by anything but 00 (an FF that is the very last byte reads as FF), else at `len`.
//   state        (p, q, b, k) at a symbol boundary: p the byte that holds the next unread bit -- never the 00 of an FF 00
//                pair --, q the bits of it already read, b the block within the MCU (it selects the tables), k the zigzag
//                index, 0 where a DC symbol is expected; or `end`, once a symbol would start at or beyond the data's end.
//   symbol       exactly jpeg_core.hpp's decode_block: a prefix with no code counts as symbol 0 behind 16 bits, a DC symbol
//                above 15 as no code, ZRL and runs past 63 end the block with ST_RUN, bits beyond the end are 0.  A symbol
//                that takes bits from beyond the end sets ST_OVERRUN and leaves p at the end: the next one is `end`.
//   ownership    a subsequence [lo, hi) owns the symbols whose first bit lies in it, the interval's last one everything
//                behind it too; a lane whose entry lies at or beyond hi walks nothing and passes the state through.  The cold
//                state of a subsequence is (lo, 0, 0, 0), one byte later where lo is a stuffed 00.
//
// The byte reader is written as selects, not branches: the compiler note in ljpeg_core.hpp (BitReader::next_byte) applies.
// Every loop has a trip count fixed by the geometry: five bytes a symbol, 8 * sub_bytes + 1 symbols a subsequence.
#pragma once
#include "jpeg_core.hpp"

namespace mi {
namespace jpeg {

constexpr uint32_t ST_UNSYNCED = 8u;    // a lane's entry was not its predecessor's exit: the rounds enqueued were too few

struct SyncState {
    uint32_t p;
    uint32_t q, b, k;
    bool end;
};
LJ_HD SyncState sync_start(uint32_t p) { return SyncState{p, 0u, 0u, 0u, false}; }
LJ_HD bool sync_same(const SyncState& x, const SyncState& y) {
    return x.end == y.end && (x.end || (x.p == y.p && x.q == y.q && x.b == y.b && x.k == y.k));
}
// two words: p, and q | b << 3 | k << 6 | end << 12 | n << 16 (n: the blocks that ended in the lane, at most 8 * 128)
LJ_HD uint32_t sync_pack(const SyncState& s, uint32_t n) {
    return s.end ? (1u << 12) | (n << 16) : s.q | (s.b << 3) | (s.k << 6) | (n << 16);
}
LJ_HD SyncState sync_unpack(uint32_t p, uint32_t w) {
    const bool end = (w >> 12) & 1u;
    return SyncState{end ? 0u : p, end ? 0u : w & 7u, end ? 0u : (w >> 3) & 7u, end ? 0u : (w >> 6) & 63u, end};
}

// the tables of every block of the MCU
struct SyncTabs {
    const Huff256* tabs;    // DC 0, DC 1, AC 0, AC 1
    uint8_t dc[8], ac[8];   // per block of the MCU: its tables among the four
    uint32_t nbm;           // blocks per MCU, 1 .. 6
};

// what a symbol did: status bits, whether its block ended, the zigzag index it sets (-1: none; 0: the DC difference) and the
// value mod 2^16
struct SyncSym {
    uint32_t status;
    bool done;
    int at;
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
    const uint32_t b = s.b < T.nbm ? s.b : 0u;
    const uint32_t peek = (uint32_t)(w >> (24 - s.q)) & 0xffffu;
    int len_code, sz;
    uint32_t k = s.k;
    y.status = 0;
    y.done = false;
    y.at = -1;
    y.val = 0;
    if (k == 0) {
        sz = huff_decode(T.tabs[T.dc[b] & 1], peek, len_code);
        if (sz < 0 || sz > 15) { y.status |= ST_NOCODE; sz = 0; }
        y.at = 0;
        k = 1;
    } else {
        int rs = huff_decode(T.tabs[2 + (T.ac[b] & 1)], peek, len_code);
        if (rs < 0) { y.status |= ST_NOCODE; rs = 0; }
        const uint32_t run = (uint32_t)rs >> 4;
        sz = rs & 15;
        if (sz == 0) {
            if (run == 15) {
                k += 16;
                if (k > 63) y.status |= ST_RUN;
            } else {
                y.done = true;
            }
        } else {
            k += run;
            if (k <= 63) y.at = (int)k;
            else y.status |= ST_RUN;
            k += 1;
        }
        if (k > 63) y.done = true;
    }
    if (sz) y.val = extend((uint32_t)(w >> (40 - (int)s.q - len_code - sz)) & ((1u << sz) - 1u), sz);
    const uint32_t t = s.q + (uint32_t)len_code + (uint32_t)sz;     // at most 7 + 16 + 15
    const bool over = t > 8u * nlive;
    const uint32_t a = over ? nlive : t >> 3;
    uint32_t np = rp[0];
#pragma unroll
    for (uint32_t i = 1; i < 6; ++i) np = a == i ? rp[i] : np;
    if (over) y.status |= ST_OVERRUN;
    s.p = np;
    s.q = over ? 0u : t & 7u;
    s.b = y.done ? (b + 1 < T.nbm ? b + 1 : 0u) : b;
    s.k = y.done ? 0u : k;
    return true;
}

// the cold state of the subsequence that starts at byte `lo`
template <class Src>
LJ_HD SyncState sync_cold(const Src& src, uint32_t len, uint32_t lo) {
    const bool stuffed = lo > 0 && lo < len && src.byte(lo - 1) == 0xffu && src.byte(lo) == 0u;
    return sync_start(stuffed ? lo + 1 : lo);
}

// The walk of the subsequence that ends at `hi` (`last`: the interval's last, which owns everything behind it) from the
// entry state `s`, which becomes the exit; the blocks that ended are added to `n`.  `emit.symbol(y)` sees every symbol in
// turn, `emit.end()` the moment the walk meets the data's end.  max_symbols: 8 * sub_bytes, what the subsequence can hold.
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
        n += y.done ? 1u : 0u;
    }
}

struct SyncNoEmit {
    LJ_HD void symbol(const SyncSym&) {}
    LJ_HD void end() {}
};

}  // namespace jpeg
}  // namespace mi
