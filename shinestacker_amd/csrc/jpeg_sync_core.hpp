// jpeg_sync_core.hpp -- the transition of the split entropy decoder (kernels_jpeg_split.hpp): one Huffman symbol of a baseline
// scan taken from a decoder STATE.  sync_walk_core.hpp has the scheme, the byte window, the advance and the walk of a
// subsequence, shared with ljpeg_sync_core.hpp; here is what a restart interval's state and symbol are.  Plain C++ over
// jpeg_core.hpp's tables, with no intrinsic and no LDS, so that it compiles for the host as well:
// tools/jpeg_split_check.cpp runs it on the CPU under the address and undefined-behaviour sanitizers against
// tests/jpeg_split_restatement.py, and kernels_jpeg_split.hpp runs the same lines on the device.
//
//   state        (p, q, b, k) at a symbol boundary: the position (p, q), b the block within the MCU (it selects the tables), k
//                the zigzag index, 0 where a DC symbol is expected; or `end`.  The cold state of a subsequence is its cold
//                position with b = k = 0.
//   symbol       exactly jpeg_core.hpp's decode_block: a prefix with no code counts as symbol 0 behind 16 bits, a DC symbol
//                above 15 as no code, ZRL and runs past 63 end the block with ST_RUN, bits beyond the end are 0.  A symbol
//                that takes bits from beyond the end sets ST_OVERRUN.
#pragma once
#include "jpeg_core.hpp"
#include "sync_walk_core.hpp"

namespace mi {
namespace jpeg {

using sync::ST_UNSYNCED;
using sync::SyncNoEmit;

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

// One symbol from `s`; a block that ended is added to `n`.  False, with s.end set, when it would start at or beyond the
// data's end.
template <class Src>
LJ_HD bool sync_symbol(const Src& src, uint32_t len, const SyncTabs& T, SyncState& s, SyncSym& y, uint32_t& n) {
    const sync::SyncWindow W = sync::sync_window(src, len, s.p);
    if (W.nlive == 0) {
        s.end = true;
        return false;
    }
    const uint64_t w = W.w;
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
    if (sync::sync_advance(W, (uint32_t)len_code + (uint32_t)sz, s.p, s.q)) y.status |= ST_OVERRUN;
    s.b = y.done ? (b + 1 < T.nbm ? b + 1 : 0u) : b;
    s.k = y.done ? 0u : k;
    n += y.done ? 1u : 0u;
    return true;
}

// the cold state of the subsequence that starts at byte `lo`
template <class Src>
LJ_HD SyncState sync_cold(const Src& src, uint32_t len, uint32_t lo) {
    return sync_start(sync::sync_cold_at(src, len, lo));
}

// sync_walk_core.hpp's walk over this transition; the blocks that ended are added to `n`
template <class Src, class Emit>
LJ_HD void sync_lane(const Src& src, uint32_t len, uint32_t hi, bool last, uint32_t max_symbols, const SyncTabs& T, SyncState& s,
                     uint32_t& n, Emit& emit) {
    sync::sync_lane<Src, SyncTabs, SyncState, SyncSym, Emit>(src, len, hi, last, max_symbols, T, s, n, emit);
}

}  // namespace jpeg
}  // namespace mi
