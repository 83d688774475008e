// sync_walk_core.hpp -- what the transitions of the two split entropy decoders share (jpeg_sync_core.hpp, ljpeg_sync_core.hpp):
// the byte window a symbol is taken from, the advance behind it, the cold position of a subsequence and the walk of one
// subsequence from an entry state to its exit.  Huffman streams re-synchronise: a decoder started at an arbitrary byte soon
// falls into step with the true one, so data of any length are cut into subsequences, every one is walked from a guess, and
// the guesses are repaired until each lane's entry is its predecessor's exit (Weissenberger and Schmidt's self-synchronising
// scheme).  Plain C++ with no intrinsic and no LDS, so that it compiles for the host as well: the two check programs under
// tools/ run these lines on the CPU under the address and undefined-behaviour sanitizers, the kernels on the device.
//
//   data         `len` bytes behind a byte source (`src.byte(i)`, asked only for i < len).  They end at the first FF followed
//                by anything but 00 (an FF that is the very last byte reads as FF), else at `len`; bits beyond the end are 0.
//                BitReader::next_byte's rule, restated.
//   position     (p, q) at a symbol boundary: p the byte that holds the next unread bit -- never the 00 of an FF 00 pair --,
//                q the bits of it already read.  A decoder's state adds what selects its tables, and `end`, once a symbol
//                would start at or beyond the data's end.
//   symbol       at most 7 + 16 + 15 = 38 bits from p on: five data bytes, ten source bytes when every one is stuffed.  One
//                that takes bits from beyond the end is an overrun and leaves p at the end: the next one is `end`.
//   ownership    a subsequence [lo, hi) owns the symbols whose first bit lies in it, the data's last one everything behind it
//                too; a lane whose entry lies at or beyond hi walks nothing and passes the state through.  The cold position
//                of a subsequence is lo, one byte later where lo is a stuffed 00.
//
// The byte reader is written as selects, not branches: the compiler note in ljpeg_core.hpp (BitReader::next_byte) applies.
// Every loop has a trip count fixed by the geometry: five bytes a symbol, 8 * sub_bytes + 1 symbols a subsequence.
#pragma once
#include "ljpeg_core.hpp"

namespace mi {
namespace sync {

constexpr uint32_t ST_UNSYNCED = 8u;    // a lane's entry was not its predecessor's exit: the rounds enqueued were too few

// The five data bytes from byte p on, the first in bits 39 .. 32 of `w`; nlive: how many lie before the data's end; rp[i]:
// where a reader that has used up i of them stands.  (Handed on by value: behind a reference the compiler turns sync_advance's
// selects into an indexed load, and rp[] then lives in scratch memory, not in registers.)
struct SyncWindow {
    uint64_t w;
    uint32_t nlive, rp[6];
};
template <class Src>
LJ_HD SyncWindow sync_window(const Src& src, uint32_t len, uint32_t p) {
    SyncWindow W;
    uint32_t pos = p;
    W.w = 0;
    W.nlive = 0;
    bool ended = false;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        W.rp[i] = pos;
        const bool live = !ended && pos < len;
        const uint32_t b = live ? src.byte(pos) : 0u;
        const uint32_t n = live && pos + 1 < len ? src.byte(pos + 1) : 0u;
        const bool marker = b == 0xffu && n != 0u;
        const bool stuffed = b == 0xffu && n == 0u && pos + 1 < len;
        const bool take = live && !marker;
        ended = !take;
        pos += take ? (stuffed ? 2u : 1u) : 0u;
        W.nlive += take ? 1u : 0u;
        W.w |= (uint64_t)(take ? b : 0u) << (32 - 8 * i);
    }
    W.rp[5] = pos;
    return W;
}

// The position behind a symbol that began q bits into the window and took `bits` more (q + bits: at most 7 + 16 + 15).  True
// when it took bits from beyond the data's end: p is then the end.
LJ_HD bool sync_advance(const SyncWindow W, uint32_t bits, uint32_t& p, uint32_t& q) {
    const uint32_t t = q + bits;
    const bool over = t > 8u * W.nlive;
    const uint32_t a = over ? W.nlive : t >> 3;
    uint32_t np = W.rp[0];
#pragma unroll
    for (uint32_t i = 1; i < 6; ++i) np = a == i ? W.rp[i] : np;
    p = np;
    q = over ? 0u : t & 7u;
    return over;
}

// the cold position of the subsequence that starts at byte `lo`
template <class Src>
LJ_HD uint32_t sync_cold_at(const Src& src, uint32_t len, uint32_t lo) {
    const bool stuffed = lo > 0 && lo < len && src.byte(lo - 1) == 0xffu && src.byte(lo) == 0u;
    return stuffed ? lo + 1 : lo;
}

// The walk of the subsequence that ends at `hi` (`last`: the data's last, which owns everything behind it) from the entry
// state `s`, which becomes the exit.  The decoder's sync_symbol(src, len, T, s, y, n) takes one symbol from `s` and adds what it
// completes to `n` (JPEG: a block that ended; lossless: a sample), or returns false, with s.end set, when the symbol would
// start at or beyond the data's end.  `emit.symbol(y)` sees every symbol in turn, `emit.end()` the moment the walk meets the
// data's end.  max_symbols: 8 * sub_bytes, what the subsequence can hold.
template <class Src, class Tabs, class State, class Sym, class Emit>
LJ_HD void sync_lane(const Src& src, uint32_t len, uint32_t hi, bool last, uint32_t max_symbols, const Tabs& T, State& s, uint32_t& n,
                     Emit& emit) {
    for (uint32_t it = 0; it <= max_symbols; ++it) {
        if (s.end || (!last && s.p >= hi)) break;
        Sym y;
        if (!sync_symbol(src, len, T, s, y, n)) {
            emit.end();
            break;
        }
        emit.symbol(y);
    }
}

struct SyncNoEmit {
    template <class Sym>
    LJ_HD void symbol(const Sym&) {}
    LJ_HD void end() {}
};

// the subsequences of `len` bytes: at least one
LJ_HD uint32_t sync_nsub(uint32_t len, uint32_t sub) {
    const uint32_t n = len / sub + (len % sub ? 1u : 0u);
    return n ? n : 1u;
}

}  // namespace sync
}  // namespace mi
