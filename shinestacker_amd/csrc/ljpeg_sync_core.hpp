// ljpeg_sync_core.hpp -- the transition of the split lossless-JPEG decoder (kernels_ljpeg_split.hpp): one Huffman symbol of a
// SOF3 scan taken from a decoder STATE.  sync_walk_core.hpp has the scheme, the byte window, the advance and the walk of a
// subsequence, shared with jpeg_sync_core.hpp; here the state is small -- a symbol is a sample, so only the position and the
// component are carried -- and what comes out are differences mod 2^16, which prefix sums turn into samples afterwards.
// Plain C++ over ljpeg_core.hpp's Huff, huff_decode and difference rule, with no intrinsic and no LDS, so that it compiles for
// the host as well: tools/ljpeg_split_check.cpp runs it on the CPU under the address and undefined-behaviour sanitizers
// against tests/ljpeg_split_restatement.py, and kernels_ljpeg_split.hpp runs the same lines on the device.
//
//   data         `len` = min(scan_bytes, span_bytes - scan_off) bytes (sync_data_len).
//   state        (p, q, c) at a symbol boundary: the position (p, q), c the component of the next sample; or `end`.  The cold
//                state of a subsequence is its cold position with c = 0.
//   symbol       exactly ljpeg_core.hpp's decode_difference: the category from component c's table, a 16-bit prefix that
//                leads no code or a category above 16 counts as category 0 behind 16 bits and sets ST_NOCODE; category 16 is
//                32768 with no further bits, else s bits follow.  A symbol that takes bits from beyond the end sets
//                ST_OVERRUN.
#pragma once
#include "ljpeg_core.hpp"
#include "sync_walk_core.hpp"

namespace mi {
namespace ljpeg {

using sync::ST_UNSYNCED;
using sync::SyncNoEmit;
using sync::sync_nsub;
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

// One symbol from `s`; it is one sample more in `n`.  False, with s.end set, when it would start at or beyond the data's end.
template <class Src>
LJ_HD bool sync_symbol(const Src& src, uint32_t len, const SyncTabs& T, SyncState& s, SyncSym& y, uint32_t& n) {
    const sync::SyncWindow W = sync::sync_window(src, len, s.p);
    if (W.nlive == 0) {
        s.end = true;
        return false;
    }
    const uint64_t w = W.w;
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
    if (sync::sync_advance(W, (uint32_t)len_code + (uint32_t)extra, s.p, s.q)) y.status |= ST_OVERRUN;
    s.c = c + 1 < T.ncomp ? c + 1 : 0u;
    n += 1u;
    return true;
}

// the cold state of the subsequence that starts at byte `lo`
template <class Src>
LJ_HD SyncState sync_cold(const Src& src, uint32_t len, uint32_t lo) {
    return sync_start(sync::sync_cold_at(src, len, lo));
}

// sync_walk_core.hpp's walk over this transition; the samples decoded are added to `n`
template <class Src, class Emit>
LJ_HD void sync_lane(const Src& src, uint32_t len, uint32_t hi, bool last, uint32_t max_symbols, const SyncTabs& T, SyncState& s,
                     uint32_t& n, Emit& emit) {
    sync::sync_lane<Src, SyncTabs, SyncState, SyncSym, Emit>(src, len, hi, last, max_symbols, T, s, n, emit);
}

// a segment's data, as the host and the kernels see them
LJ_HD uint32_t sync_data_len(uint32_t scan_off, uint32_t scan_bytes, uint32_t span_bytes) {
    return scan_off < span_bytes ? (scan_bytes < span_bytes - scan_off ? scan_bytes : span_bytes - scan_off) : 0u;
}

}  // namespace ljpeg
}  // namespace mi
