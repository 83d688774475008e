// kernels_split_common.hpp -- the device scaffold of the two split entropy decoders (kernels_jpeg_split.hpp: baseline JPEG;
// kernels_ljpeg_split.hpp: lossless JPEG inside a DNG segment).  sync_walk_core.hpp has the scheme and the reasoning.  A decoder
// brings its units (restart intervals; segments), its transition and what it does with a symbol; lanes, staging, the repair
// rounds and the frame of the write pass are here, once.
//
// The units' subsequences -- sub_bytes bytes each, counted unit after unit, at least one per unit -- are the lanes, 256
// consecutive ones a workgroup ("group"); a unit may cover many groups and a group many units.  A segmented scan of the
// units' subsequence counts (`incl`) gives every unit its first lane; a lane finds its unit by bisection.
//
//   round_body   round 0: every lane walks its subsequence from its cold state, then the group iterates in LDS -- a lane takes
//                a new exit when its predecessor's changed -- until no lane changes, at most 256 times.  Round r > 0: the
//                group's first lane takes the exit its predecessor group left in round r - 1 (two boundary arrays, written in
//                alternation, so no group reads what another writes in the same launch) and the group converges again; a
//                group whose entry did not change returns before it stages a byte.  A round returns at once when the round
//                before it changed no boundary (a flag word per round).  After r rounds the first r + 1 groups of a unit are
//                exact, so groups - 1 rounds always suffice; photographs need none or one.
//   write_body   every lane walks once more from its predecessor's stored exit, its first symbol's place given by the
//                segmented scan of the lanes' counts, and hands every symbol to the decoder's writer.  Status bits come from
//                this pass alone.  A lane whose walk does not reproduce its stored exit sets ST_UNSYNCED: the rounds were
//                too few.
//
// Bytes: a group's 256 * sub_bytes bytes and 24 more, from its first lane's first byte on, are staged into LDS with coalesced
// dword loads and every walk reads LDS; the stage is padded by 4 bytes every 128, which puts the 32 lanes of a half-wave,
// sub_bytes apart, on 32 different banks for every sub_bytes from 8 to 128 (byte reads bank by (a / 4) % 32).  A byte outside
// the stage (units out of file order, gaps, headers between small tiles, offsets the host forms refuse) is read from the span.
// No workgroup ever waits for another: the rounds are separate launches.  Bounded by construction: every byte index is checked
// against the unit, every unit against the span, every lane against the arrays' lengths; what a writer stores it bounds itself.
#pragma once
#include "common.hpp"
#include "kernels_segscan.hpp"
#include "sync_walk_core.hpp"

namespace mi {
namespace split {

constexpr int GROUP = 256;                  // lanes a workgroup
constexpr uint32_t SUB_DEFAULT = 128, ROUNDS_DEFAULT = 8;
constexpr uint32_t OVERSHOOT = 24;          // bytes staged behind the group's last subsequence: a symbol reads at most 11

__host__ __device__ inline uint32_t stage_index(uint32_t a) { return a + ((a >> 7) << 2); }
inline uint32_t stage_bytes(uint32_t sub) { return stage_index(GROUP * sub + OVERSHOOT + 4) + 8; }
__device__ inline bool same2(uint2 a, uint2 b) { return a.x == b.x && a.y == b.y; }

// ---- the scratch both decoders begin with, in words; a decoder's own arrays follow through the same `take`
struct Take {
    size_t at = 0;
    size_t operator()(size_t words) {
        const size_t o = at;
        at += (words + 63) & ~(size_t)63;
        return o;
    }
};
struct Layout {
    size_t lanes, groups, rounds;
    size_t incl, exits, alts, counts, gentry, bnd, flags;
};
// lanes: span_bytes / sub_bytes rounded up, and one per unit.  `two`: the decoder keeps a second exit per lane.
inline Layout layout(Take& take, size_t span_bytes, uint32_t sub, uint32_t max_rounds, size_t units, bool two) {
    Layout L{};
    L.lanes = (span_bytes + sub - 1) / sub + units;
    L.groups = (L.lanes + GROUP - 1) / GROUP;
    L.rounds = L.groups > 1 ? (max_rounds < L.groups - 1 ? max_rounds : L.groups - 1) : 0;
    L.incl = take(units);
    L.exits = take(2 * L.lanes);
    L.alts = take(two ? 2 * L.lanes : 0);
    L.counts = take(L.lanes);
    L.gentry = take(2 * L.groups);
    L.bnd = take(4 * L.groups);
    L.flags = take(L.rounds + 2);
    return L;
}

struct Args {
    const uint8_t* span;
    uint32_t* incl;         // per unit: lanes of it and of every unit before it (seg_scan of the counts)
    uint2* exits;           // per lane: its exit state and count (the decoder's sync_pack)
    uint2* alts;            // per lane: its second exit (decoders with TWO; else unused)
    uint32_t* counts;       // per lane: its count, bit 31 on a unit's first lane; scanned before the write pass
    uint2* gentry;          // per group: the entry its first lane last walked from
    uint2* bnd;             // two arrays of one exit per group
    uint32_t* flags;        // per round: a boundary changed
    uint32_t span_bytes, sub, lanes, groups;
};
inline Args bind(const Layout& L, uint32_t* words, const void* span, size_t span_bytes, uint32_t sub) {
    Args S{};
    S.span = (const uint8_t*)span;
    S.incl = words + L.incl; S.exits = (uint2*)(words + L.exits); S.alts = (uint2*)(words + L.alts); S.counts = words + L.counts;
    S.gentry = (uint2*)(words + L.gentry); S.bnd = (uint2*)(words + L.bnd); S.flags = words + L.flags;
    S.span_bytes = (uint32_t)span_bytes; S.sub = sub; S.lanes = (uint32_t)L.lanes; S.groups = (uint32_t)L.groups;
    return S;
}

// ---- a lane's place: its unit and the bytes of its subsequence
struct Lane {
    bool active, first, last;
    uint32_t k, o0, len, lo, hi;
};
// unit(k, o0, len): unit k's first byte in the span and its length, clamped to the span; false where the unit is not decoded
template <class Unit>
__device__ inline Lane place_lane(const uint32_t* incl, uint32_t n_units, uint32_t g, uint32_t lanes, uint32_t sub, Unit unit) {
    Lane P{};
    const uint32_t total = incl[n_units - 1] & segscan::MASK;
    uint32_t lo = 0, hi = n_units - 1;  // the first unit whose inclusive count exceeds g (bisection: trip count log2 n)
    for (int it = 0; it < 32; ++it) {
        if (lo >= hi) break;
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((incl[mid] & segscan::MASK) > g) hi = mid;
        else lo = mid + 1;
    }
    P.k = lo;
    const uint32_t before = lo ? incl[lo - 1] & segscan::MASK : 0u;
    const bool ok = unit(lo, P.o0, P.len);
    const uint32_t nsub = sync::sync_nsub(P.len, sub);
    const uint32_t j = g - before;
    P.active = ok && g < total && g < lanes && g >= before && j < nsub;
    P.first = j == 0;
    P.last = j == nsub - 1;
    P.lo = P.active ? j * sub : 0u;
    P.hi = min(P.lo + sub, P.len);
    return P;
}

// the unit's bytes: from the group's stage in LDS where they lie in it, else from the span (i < len: inside the span)
struct StagedBytes {
    const uint8_t* stage;
    const uint8_t* span;
    uint32_t o0, base, staged;      // the unit's first byte, the stage's first byte (both in the span), bytes staged
    __device__ uint32_t byte(uint32_t i) const {
        const uint32_t a = o0 + i, d = a - base;
        return d < staged ? stage[stage_index(d)] : span[a];
    }
};

// The group's bytes into LDS, from its first lane's first byte (4-byte aligned down); two barriers.  The base is guarded for
// descriptors that lie outside the span.  Where a decoder clamps its units to the span beforehand (JPEG: o0 <= span_bytes and
// o0 + len <= span_bytes, and lo is 0 or below len), the guard changes nothing: o0 == span_bytes gives span_bytes either way,
// and below it lo <= span_bytes - o0, so the base is o0 + lo.
__device__ inline StagedBytes stage_group(const Args& S, const Lane& P, uint8_t* stage) {
    __shared__ uint32_t shared_base;
    const int t = (int)threadIdx.x;
    if (t == 0) shared_base = min(P.o0 < S.span_bytes ? P.o0 + min(P.lo, S.span_bytes - P.o0) : S.span_bytes, S.span_bytes) & ~3u;
    __syncthreads();
    const uint32_t base = shared_base;
    const uint32_t want = GROUP * S.sub + OVERSHOOT + 4;
    const uint32_t staged = min(want, S.span_bytes - base);
    for (uint32_t d = 4u * t; d < staged; d += 4u * GROUP) {
        uint32_t w;
        if (d + 4 <= staged) {
            w = *(const uint32_t*)(S.span + base + d);
        } else {
            w = 0;
            for (uint32_t k = 0; k < 3; ++k)
                if (d + k < staged) w |= (uint32_t)S.span[base + d + k] << (8 * k);
        }
        *(uint32_t*)(stage + stage_index(d)) = w;
    }
    __syncthreads();
    return StagedBytes{stage, S.span, P.o0, base, staged};
}

// What a decoder D gives the two bodies below:
//   D::Lane              split::Lane, or a type derived from it
//   D::ENDED             the second word of the packed state `end` (sync_pack)
//   D::TWO               whether a lane keeps a second exit (below); then D::ALT_VALID, a bit of the second word sync_pack
//                        leaves free, W.two() and W.other(e), the packed entry `e` with the other table selection
//   dec.lane(g)          lane g's place
//   dec.prepare()        the group's own LDS (tables), written before the stage's first barrier
//   dec.tabs_of(P)       T, the lane's tables
//   D::Walker            W{P, src, T, max_symbols}, with W.cold(), the lane's packed cold entry, and W.walk(e, emit), the walk
//                        from the packed entry `e` (a unit's first lane: from the unit's start), which returns the packed
//                        exit and count
//
// The second exit (TWO): where a state selects between two tables, a cold lane falls into step with the true BIT position
// quickly and has the SELECTION right half of the time -- with two similar tables the wrong one decodes just as well --, so a
// lane walks from its entry and from the entry with the other selection, keeps both exits (the second in `alts`, across
// rounds too), and a predecessor that flips its selection costs a swap, not a walk: the repair of a whole group is then 256
// cheap iterations at worst, not 256 walks.  This changes no result -- a memo of the same function.
template <class D>
__device__ inline void round_body(const D& dec, const Args& S, uint32_t round, uint8_t* stage) {
    __shared__ uint2 ex[GROUP];
    __shared__ uint32_t chg[GROUP];
    if (round > 0 && S.flags[round - 1] == 0) return;      // the round before changed no boundary: nothing can change
    const int t = (int)threadIdx.x;
    const uint32_t grp = blockIdx.x, g = grp * GROUP + t;
    const typename D::Lane P = dec.lane(g);
    const uint2 ended = make_uint2(0u, D::ENDED);
    const auto is_end = [](uint2 e) { return (e.y & D::ENDED) != 0; };
    const auto bnd_at = [&](uint32_t r) { return S.bnd + (size_t)(r & 1) * S.groups; };    // round r's boundary array
    uint2 e0 = make_uint2(0, 0);        // lane 0: the entry from outside the group
    [[maybe_unused]] uint2 en = ended;  // TWO: the entry this lane last walked from; `ax`: its exit from en with the other selection
    bool need = false;
    if (round > 0) {
        if (t == 0) {
            e0 = grp ? bnd_at(round - 1)[grp - 1] : ended;
            e0.y &= 0xffffu;
            en = S.gentry[grp];
            need = P.active && !P.first && grp > 0 && !same2(e0, en);
        }
        // This group's entry is what it was: its exits stand.  Nothing stored differs from walking on: such a group's lanes
        // all find `need` false, so it would write back the exits and counts it read, raise no flag -- its last exit is the
        // one it left in round r - 1's boundary array -- and store that exit in this round's.  (Every group of round r - 1
        // wrote its boundary word, on this path or below: this round runs only where that one passed its flag.)
        if (!__syncthreads_or(need ? 1 : 0)) {
            if (t == GROUP - 1) bnd_at(round)[grp] = bnd_at(round - 1)[grp];
            return;
        }
    }
    dec.prepare();
    const StagedBytes src = stage_group(S, P, stage);
    const auto T = dec.tabs_of(P);
    const typename D::Walker W{P, src, T, 8 * S.sub};
    sync::SyncNoEmit none;
    uint2 cur;
    [[maybe_unused]] uint2 ax = ended;
    [[maybe_unused]] bool axv = false;
    if (round == 0) {
        const uint2 cold = W.cold();
        cur = P.active ? W.walk(cold, none) : ended;
        if (t == 0) {
            e0 = cold;
            S.gentry[grp] = cold;
            if (grp == 0) S.flags[0] = 1;
        }
        if constexpr (D::TWO) {
            ax = cur;
            en = cold;
            if (t == 0 && P.active && !P.first && W.two()) {
                ax = W.walk(W.other(cold), none);
                axv = true;
            }
        }
        need = P.active && !P.first && t > 0;
    } else {
        cur = g < S.lanes ? S.exits[g] : ended;
        if constexpr (D::TWO) {
            ax = g < S.lanes ? S.alts[g] : ended;
            axv = (ax.y & D::ALT_VALID) != 0;
            ax.y &= ~D::ALT_VALID;
        }
        if (t == 0 && need) S.gentry[grp] = e0;
    }
    ex[t] = cur;
    chg[t] = 0;
    __syncthreads();
    if constexpr (D::TWO) {
        if (round > 0 && t > 0) {
            en = ex[t - 1];
            en.y &= 0xffffu;
        }
    }
    for (int it = 0; it < GROUP; ++it) {        // (a change moves on by one lane or more an iteration)
        bool c = false;
        uint2 nw = cur;
        if (need) {
            uint2 e = e0;
            if (t > 0) {
                e = ex[t - 1];
                e.y &= 0xffffu;
            }
            if constexpr (D::TWO) {
                if (same2(e, en)) {
                    nw = cur;
                } else if (W.two() && axv && !is_end(e) && !is_end(en) && same2(e, W.other(en))) {
                    nw = ax;
                    ax = cur;
                } else {
                    nw = W.walk(e, none);
                    axv = W.two() && !is_end(e);
                    ax = axv ? W.walk(W.other(e), none) : nw;
                }
                en = e;
            } else {
                nw = W.walk(e, none);
            }
            c = !same2(nw, cur);
        }
        __syncthreads();
        if (c) {
            ex[t] = nw;
            cur = nw;
        }
        chg[t] = c ? 1u : 0u;
        __syncthreads();
        need = P.active && !P.first && t > 0 && chg[t - 1] != 0;
        if (!__syncthreads_or(need ? 1 : 0)) break;
    }
    if (g < S.lanes) {
        S.exits[g] = cur;
        if constexpr (D::TWO) S.alts[g] = axv ? make_uint2(ax.x, ax.y | D::ALT_VALID) : cur;
        S.counts[g] = (P.active ? cur.y >> 16 : 0u) | (P.first || !P.active ? segscan::HEAD : 0u);
    }
    if (t == GROUP - 1) {
        if (round > 0 && !same2(bnd_at(round - 1)[grp], cur)) atomicOr(S.flags + round, 1u);
        bnd_at(round)[grp] = cur;
    }
}

// The write pass up to the decoder's writer and behind it.  make(W, first): the lane's writer (`symbol`, `end`, `status`),
// `first` the place of the lane's first symbol within its unit, from the scanned counts.  `status`: one word per unit.
template <class D, class Make>
__device__ inline void write_body(const D& dec, const Args& S, uint8_t* stage, uint32_t* status, Make make) {
    dec.prepare();          // (first: the table build needs the most registers of the pass, and nothing else is live yet)
    const uint32_t g = blockIdx.x * GROUP + threadIdx.x;
    const typename D::Lane P = dec.lane(g);
    const StagedBytes src = stage_group(S, P, stage);
    if (!P.active) return;
    const auto T = dec.tabs_of(P);
    const typename D::Walker W{P, src, T, 8 * S.sub};
    const uint2 stored = S.exits[g];
    const uint2 entry = P.first ? make_uint2(0, 0) : S.exits[g - 1];
    auto wr = make(W, ((S.counts[g] & segscan::MASK) - (stored.y >> 16)) & segscan::MASK);
    const uint2 now = W.walk(entry, wr);
    if (!same2(now, stored)) wr.status |= sync::ST_UNSYNCED;
    if (wr.status) atomicOr(status + P.k, wr.status);
}

}  // namespace split
}  // namespace mi
