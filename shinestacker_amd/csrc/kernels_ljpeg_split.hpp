// kernels_ljpeg_split.hpp -- the second entropy path of the lossless-JPEG decoder: a segment (mi_ljpeg_seg_t: one or two
// components, every predictor, every precision) of ANY length, a file written as one strip included, decoded on many lanes at
// once and exactly.  ljpeg_sync_core.hpp has the transition, jpeg_sync_core.hpp the scheme's reasoning; the definition is
// tests/ljpeg_split_restatement.py, held bit for bit.  Tables, descriptors, layout, crop, linearisation table, shift and
// output are exactly raw_ljpeg's (kernels_ljpeg.hpp), and so is the result.  No reference counterpart.
//
// Deliberately left for later: three-component streams (mi_ljpeg_seg3_t, raw_ljpeg3) stay on the serial kernel.
//
// The segments' subsequences -- sub_bytes bytes each, counted segment after segment, at least one per segment -- are the
// lanes, 256 consecutive ones a workgroup ("group"); a segment may cover many groups and a group many segments.
//
//   ljpeg_split_prep      per segment (one workgroup): its subsequence count (from the descriptor, clamped to the span), its
//                         status word, its tables in canonical form and their lookup over the next 10 bits in scratch --
//                         converters write different tables in every tile, so a lane reads its own segment's.  A descriptor
//                         the host forms refuse (ncomp outside 1 and 2, a bad predictor or precision, a width that is no
//                         multiple of ncomp, predictors 2 to 7 wider than MI_LJPEG_MAX_LINE) sets MI_LJPEG_UNDECODED: the
//                         segment keeps one lane that walks nothing, and NOTHING of it is written (as raw_ljpeg3 does).
//                         seg_scan then gives every segment its first lane; a lane finds its segment by bisection.
//   ljpeg_split_round     round 0: every lane walks its subsequence from its cold state, then the group iterates in LDS -- a
//                         lane takes a new exit when its predecessor's changed -- until no lane changes, at most 256 times.
//                         Round r > 0: the group's first lane takes the exit its predecessor group left in round r - 1 (two
//                         boundary arrays, written in alternation, so no group reads what another writes in the same launch)
//                         and the group converges again; a group whose entry did not change returns before it stages a byte.
//                         A round returns at once when the round before it changed no boundary.  After r rounds the first
//                         r + 1 groups of a segment are exact, so groups - 1 rounds always suffice.
//                         Two components: a cold lane falls into step with the true BIT position quickly and has the
//                         COMPONENT right half of the time -- with two similar tables the wrong one decodes just as well --,
//                         so a lane walks from its entry and from the entry with the other component, keeps both exits (the
//                         second in `alts`, across rounds too), and a predecessor that flips its component costs a swap, not
//                         a walk: the repair of a whole group is then 256 cheap iterations at worst, not 256 walks.  This
//                         changes no result -- a memo of the same function.
//   ljpeg_split_write     every lane walks once more from its predecessor's stored exit, its first sample given by the
//                         segmented scan of the sample counts, and writes the differences mod 2^16 of the samples below its
//                         segment's quota (rows x columns) into the difference plane, seg_h x seg_w uint16 per segment,
//                         zeroed beforehand.  Status bits come from this pass alone.  A lane whose walk does not reproduce its
//                         stored exit sets MI_LJPEG_UNSYNCED: the rounds were too few.
//   ljpeg_split_columns   predictor 1: a scan down each segment's first ncomp columns from 2^(P-1), in place (one wave per
//   ljpeg_split_rows      segment); then one wave per segment ROW, in chunks of ROW_CHUNK = 512 samples with a carry: a
//                         per-component inclusive scan mod 2^16 -- after the column pass a row is a plain scan with carry 0 --
//                         straight into ljpeg_store.  A one-strip file spreads over the device; any width, no line kept.
//   ljpeg_split_segments  predictors 2 to 7: one wave per segment, raw_ljpeg's own predict half reading the difference plane
//                         where the walker stood (first line: the wave's scan; 2: an add against the line above; 3 to 7: one
//                         lane against the line in LDS).  The MI_LJPEG_MAX_LINE rule is unchanged.
//   ljpeg_split_status    an unsynced segment reports MI_LJPEG_UNSYNCED and nothing else: its other bits came from wrong
//                         states.  A segment whose lanes were cut off (descriptors that overlap: more subsequences than the
//                         span has bytes for) reports MI_LJPEG_UNDECODED.
//
// Bytes: as kernels_jpeg_split.hpp -- a group's 256 * sub_bytes bytes and 24 more, from its first lane's first byte on, are
// staged into LDS with coalesced dword loads, padded by 4 bytes every 128; a byte outside the stage (segments out of file
// order, gaps, headers between small tiles) is read from the span.  No workgroup ever waits for another.  Bounded by
// construction: every byte index is checked against the segment, every segment against the span, every lane against the
// arrays' lengths, every sample index against the quota and every store against the crop (ljpeg_store, the one write path).
// A corrupt stream costs status bits and nothing else.
#pragma once
#include "common.hpp"
#include "kernels_jpeg_split.hpp"
#include "kernels_ljpeg.hpp"
#include "ljpeg_sync_core.hpp"

namespace mi {

namespace ljpeg {
constexpr int SPLIT_GROUP = 256;            // lanes a workgroup
constexpr uint32_t SPLIT_SUB_DEFAULT = 128, SPLIT_ROUNDS_DEFAULT = 8;
constexpr uint32_t SPLIT_OVERSHOOT = 24;    // bytes staged behind the group's last subsequence: a symbol reads at most 11
constexpr int ROW_PER_LANE = 8, ROW_CHUNK = LANES * ROW_PER_LANE, ROWS_PER_BLOCK = 4;
constexpr int SPLIT_LUT = 2 << SYNC_LUT_BITS;   // lookup entries a segment
static_assert(SYNC_LUT_BITS == LUT_BITS, "one lookup width");

inline size_t split_lanes(size_t span_bytes, uint32_t sub, size_t nseg) { return (span_bytes + sub - 1) / sub + nseg; }

// the scratch, in words
struct SplitLayout {
    size_t nseg, lanes, groups, rounds, samples;
    size_t incl, exits, alts, counts, gentry, bnd, flags, stat, tmp, huff, lut, plane, words;
};
inline SplitLayout split_layout(const mi_raw_layout_t& R, size_t span_bytes, uint32_t sub, uint32_t max_rounds) {
    SplitLayout L{};
    L.nseg = (size_t)unpack_nsegs(R);
    L.lanes = split_lanes(span_bytes, sub, L.nseg);
    L.groups = (L.lanes + SPLIT_GROUP - 1) / SPLIT_GROUP;
    L.rounds = L.groups > 1 ? (max_rounds < L.groups - 1 ? max_rounds : L.groups - 1) : 0;
    L.samples = L.nseg * (size_t)R.seg_height * (size_t)R.seg_width;
    size_t at = 0;
    auto take = [&](size_t words) { const size_t o = at; at += (words + 63) & ~(size_t)63; return o; };
    L.incl = take(L.nseg);
    L.exits = take(2 * L.lanes);
    L.alts = take(2 * L.lanes);
    L.counts = take(L.lanes);
    L.gentry = take(2 * L.groups);
    L.bnd = take(4 * L.groups);
    L.flags = take(L.rounds + 2);
    L.stat = take(L.nseg);
    L.tmp = take(segscan::tmp_words(L.lanes > L.nseg ? L.lanes : L.nseg));
    L.huff = take((2 * L.nseg * sizeof(Huff) + 3) / 4);
    L.lut = take(L.nseg * SPLIT_LUT / 2);
    L.plane = take((L.samples + 1) / 2);
    L.words = at;
    return L;
}

// descriptors in host memory: the largest number of groups any one segment's lanes touch, minus 1 -- after r rounds the first
// r + 1 groups of a segment are exact, so this many rounds never leave a segment unsynced
inline uint32_t split_exact_rounds(const mi_ljpeg_seg_t* segs, size_t nseg, size_t span_bytes, uint32_t sub) {
    uint64_t at = 0, most = 1;
    for (size_t k = 0; k < nseg; ++k) {
        const uint64_t n = sync_nsub(sync_data_len(segs[k].scan_off, segs[k].scan_bytes, (uint32_t)span_bytes), sub);
        const uint64_t groups = (at + n - 1) / SPLIT_GROUP - at / SPLIT_GROUP + 1;
        most = groups > most ? groups : most;
        at += n;
    }
    return (uint32_t)(most - 1);
}

struct SplitArgs {
    LjpegArgs L;            // the span, the descriptors, the table, the output, the geometry: raw_ljpeg's
    uint32_t* incl;         // per segment: lanes of it and of every segment before it (seg_scan of the counts)
    uint2* exits;           // per lane: its exit state and sample count (sync_pack)
    uint2* alts;            // per lane: its exit from the entry with the other component
    uint32_t* counts;       // per lane: its sample count, bit 31 on a segment's first lane; scanned before the write pass
    uint2* gentry;          // per group: the entry its first lane last walked from
    uint2* bnd;             // two arrays of one exit per group
    uint32_t* flags;        // per round: a boundary changed
    uint32_t* stat;
    Huff* huff;             // per segment: two tables
    uint16_t* lut;          // per segment: SPLIT_LUT entries
    uint16_t* plane;        // the differences: seg_h * seg_w per segment
    uint32_t nseg, sub, lanes, groups;
};

// what a descriptor says, checked: `ok` false where the host forms refuse it
struct SplitSeg {
    bool ok;
    int nc, pred, prec, rows;
    uint32_t o0, len;
};
__device__ inline SplitSeg split_seg(const SplitArgs& A, uint32_t k) {
    const mi_ljpeg_seg_t& S = A.L.segs[k];
    SplitSeg G;
    const int sy = (int)k / A.L.nsx, W = A.L.seg_w;
    G.rows = A.L.tiled ? A.L.seg_h : max(0, min(A.L.seg_h, A.L.image_h - sy * A.L.seg_h));
    G.nc = S.ncomp; G.pred = S.predictor; G.prec = S.precision;
    G.ok = !((G.nc != 1 && G.nc != 2) || W % G.nc || G.pred < 1 || G.pred > 7 || G.prec < 2 || G.prec > 16 || (G.pred != 1 && W > MAX_LINE));
    G.o0 = S.scan_off;
    G.len = sync_data_len(S.scan_off, S.scan_bytes, A.L.span_bytes);
    if (!G.ok) { G.nc = 1; G.len = 0; }
    return G;
}

// a lane's place: its segment and the bytes of its subsequence
struct SplitLane {
    bool active, first, last;
    uint32_t k, o0, len, lo, hi, nc;
};
__device__ inline SplitLane split_lane(const SplitArgs& A, uint32_t g) {
    SplitLane P{};
    const uint32_t n = A.nseg;
    const uint32_t total = A.incl[n - 1] & segscan::MASK;
    uint32_t lo = 0, hi = n - 1;        // the first segment whose inclusive count exceeds g (bisection: trip count log2 n)
    for (int it = 0; it < 32; ++it) {
        if (lo >= hi) break;
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((A.incl[mid] & segscan::MASK) > g) hi = mid;
        else lo = mid + 1;
    }
    P.k = lo;
    const uint32_t before = lo ? A.incl[lo - 1] & segscan::MASK : 0u;
    const SplitSeg G = split_seg(A, lo);
    P.o0 = G.o0; P.len = G.len; P.nc = (uint32_t)G.nc;
    const uint32_t nsub = sync_nsub(G.len, A.sub);
    const uint32_t j = g - before;
    P.active = G.ok && g < total && g < A.lanes && g >= before && j < nsub;
    P.first = j == 0;
    P.last = j == nsub - 1;
    P.lo = P.active ? j * A.sub : 0u;
    P.hi = min(P.lo + A.sub, P.len);
    return P;
}

// the segment's bytes: from the group's stage in LDS where they lie in it, else from the span (i < len: inside the span)
struct SplitBytes {
    const uint8_t* stage;
    const uint8_t* span;
    uint32_t o0, base, staged;      // the segment's first byte, the stage's first byte (both in the span), bytes staged
    __device__ uint32_t byte(uint32_t i) const {
        const uint32_t a = o0 + i, d = a - base;
        return d < staged ? stage[jpeg::split_stage_index(d)] : span[a];
    }
};

// the group's bytes into LDS, from its first lane's first byte (4-byte aligned down)
__device__ inline void split_stage(const SplitArgs& A, const SplitLane& P, uint8_t* stage, uint32_t* shared_base, uint32_t& base, uint32_t& staged) {
    const int t = (int)threadIdx.x;
    if (t == 0) *shared_base = min(P.o0 < A.L.span_bytes ? P.o0 + min(P.lo, A.L.span_bytes - P.o0) : A.L.span_bytes, A.L.span_bytes) & ~3u;
    __syncthreads();
    base = *shared_base;
    const uint32_t want = SPLIT_GROUP * A.sub + SPLIT_OVERSHOOT + 4;
    staged = min(want, A.L.span_bytes - base);
    for (uint32_t d = 4u * t; d < staged; d += 4u * SPLIT_GROUP) {
        uint32_t w;
        if (d + 4 <= staged) {
            w = *(const uint32_t*)(A.L.span + base + d);
        } else {
            w = 0;
            for (uint32_t k = 0; k < 3; ++k)
                if (d + k < staged) w |= (uint32_t)A.L.span[base + d + k] << (8 * k);
        }
        *(uint32_t*)(stage + jpeg::split_stage_index(d)) = w;
    }
    __syncthreads();
}

__device__ inline SyncTabs split_tabs(const SplitArgs& A, const SplitLane& P) {
    return SyncTabs{A.huff + 2 * (size_t)P.k, A.lut + (size_t)P.k * SPLIT_LUT, P.nc};
}
__device__ inline bool same2(uint2 a, uint2 b) { return a.x == b.x && a.y == b.y; }
__device__ inline bool is_end(uint2 e) { return (e.y >> 4) & 1u; }
}  // namespace ljpeg

// one workgroup per segment
__global__ __launch_bounds__(256) void ljpeg_split_prep(ljpeg::SplitArgs A, uint32_t n_flags) {
    using namespace ljpeg;
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    if (k == 0)
        for (uint32_t i = t; i < n_flags; i += 256) A.flags[i] = 0;
    const SplitSeg G = split_seg(A, k);
    const mi_ljpeg_seg_t& S = A.L.segs[k];
    Huff* h = A.huff + 2 * (size_t)k;
    if (t < 2) huff_build(h[t], S.counts[t], S.values[t]);
    if (t == 0) {
        A.incl[k] = sync_nsub(G.len, A.sub) | (k == 0 ? segscan::HEAD : 0u);
        A.stat[k] = G.ok ? 0u : MI_LJPEG_UNDECODED;
    }
    __syncthreads();
    uint16_t* lut = A.lut + (size_t)k * SPLIT_LUT;
    for (int j = (int)t; j < SPLIT_LUT; j += 256) {
        int len;
        const int s = huff_decode(h[j >> SYNC_LUT_BITS], (uint32_t)(j & ((1 << SYNC_LUT_BITS) - 1)) << (16 - SYNC_LUT_BITS), len);
        lut[j] = s >= 0 && s <= 16 && len <= SYNC_LUT_BITS ? (uint16_t)(len << 8 | s) : (uint16_t)0;
    }
}

__global__ __launch_bounds__(256) void ljpeg_split_round(ljpeg::SplitArgs A, uint32_t round) {
    using namespace ljpeg;
    extern __shared__ __align__(16) uint8_t stage[];
    __shared__ uint2 ex[SPLIT_GROUP];
    __shared__ uint32_t chg[SPLIT_GROUP];
    __shared__ uint32_t shared_base, go;
    if (round > 0 && A.flags[round - 1] == 0) return;      // the round before changed no boundary: nothing can change
    const int t = (int)threadIdx.x;
    const uint32_t grp = blockIdx.x, g = grp * SPLIT_GROUP + t;
    const SplitLane P = split_lane(A, g);
    const uint2 ended = make_uint2(0u, 1u << 4);
    uint2 e0 = make_uint2(0, 0);        // lane 0: the entry from outside the group
    uint2 en = ended;                   // the entry this lane last walked from; `ax`: its exit from en with the other component
    bool need = false;
    if (round > 0) {
        if (t == 0) {
            e0 = grp ? A.bnd[(size_t)((round - 1) & 1) * A.groups + grp - 1] : ended;
            e0.y &= 0xffffu;
            en = A.gentry[grp];
            need = P.active && !P.first && grp > 0 && !same2(e0, en);
            go = need ? 1u : 0u;
        }
        __syncthreads();
        if (!go) {          // this group's entry is what it was: its exits stand
            if (t == SPLIT_GROUP - 1) A.bnd[(size_t)(round & 1) * A.groups + grp] = A.bnd[(size_t)((round - 1) & 1) * A.groups + grp];
            return;
        }
    }
    uint32_t base, staged;
    split_stage(A, P, stage, &shared_base, base, staged);
    const SyncTabs T = split_tabs(A, P);
    const SplitBytes src{stage, A.L.span, P.o0, base, staged};
    const uint32_t max_symbols = 8 * A.sub;
    const bool two = P.nc == 2;
    SyncNoEmit none;

    // a walk from `e`, packed
    auto walk = [&](uint2 e) {
        SyncState s = P.first ? sync_start(0) : sync_unpack(e.x, e.y);
        uint32_t n = 0;
        sync_lane(src, P.len, P.hi, P.last, max_symbols, T, s, n, none);
        return make_uint2(s.end ? 0u : s.p, sync_pack(s, n));
    };
    const auto other = [](uint2 e) { return make_uint2(e.x, e.y ^ 8u); };     // the same place, the other component
    uint2 cur, ax;
    bool axv = false;
    if (round == 0) {
        const SyncState c = sync_cold(src, P.len, P.lo);
        const uint2 cold = make_uint2(c.p, sync_pack(c, 0));
        cur = P.active ? walk(cold) : ended;
        ax = cur;
        en = cold;
        if (t == 0) {
            e0 = cold;
            A.gentry[grp] = cold;
            if (grp == 0) A.flags[0] = 1;
            if (P.active && !P.first && two) {
                ax = walk(other(cold));
                axv = true;
            }
        }
        need = P.active && !P.first && t > 0;
        ex[t] = cur;
    } else {
        cur = g < A.lanes ? A.exits[g] : ended;
        ax = g < A.lanes ? A.alts[g] : ended;
        axv = (ax.y & 32u) != 0;        // (bit 5: the second exit is there)
        ax.y &= ~32u;
        ex[t] = cur;
        if (t == 0 && need) A.gentry[grp] = e0;
    }
    chg[t] = 0;
    __syncthreads();
    if (round > 0 && t > 0) {
        en = ex[t - 1];
        en.y &= 0xffffu;
    }
    for (int it = 0; it < SPLIT_GROUP; ++it) {      // (a change moves on by one lane or more an iteration)
        bool c = false;
        uint2 nw = cur;
        if (need) {
            uint2 e = e0;
            if (t > 0) {
                e = ex[t - 1];
                e.y &= 0xffffu;
            }
            if (same2(e, en)) {
                nw = cur;
            } else if (two && axv && !is_end(e) && !is_end(en) && same2(e, other(en))) {
                nw = ax;
                ax = cur;
            } else {
                nw = walk(e);
                axv = two && !is_end(e);
                ax = axv ? walk(other(e)) : nw;
            }
            en = e;
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
    if (g < A.lanes) {
        A.exits[g] = cur;
        A.alts[g] = axv ? make_uint2(ax.x, ax.y | 32u) : cur;
        A.counts[g] = (P.active ? cur.y >> 16 : 0u) | (P.first || !P.active ? segscan::HEAD : 0u);
    }
    if (t == SPLIT_GROUP - 1) {
        if (round > 0) {
            const uint2 was = A.bnd[(size_t)((round - 1) & 1) * A.groups + grp];
            if (!same2(was, cur)) atomicOr(A.flags + round, 1u);
        }
        A.bnd[(size_t)(round & 1) * A.groups + grp] = cur;
    }
}

// what the write pass does with a symbol
struct LjpegSplitWriter {
    uint16_t* plane;        // the segment's
    uint32_t at, quota, status;
    __device__ void symbol(const ljpeg::SyncSym& y) {
        if (at >= quota) return;
        status |= y.status;
        plane[at] = (uint16_t)y.val;
        ++at;
    }
    __device__ void end() {
        if (at < quota) status |= ljpeg::ST_OVERRUN;
    }
};

__global__ __launch_bounds__(256) void ljpeg_split_write(ljpeg::SplitArgs A) {
    using namespace ljpeg;
    extern __shared__ __align__(16) uint8_t stage[];
    __shared__ uint32_t shared_base;
    const int t = (int)threadIdx.x;
    const uint32_t g = blockIdx.x * SPLIT_GROUP + t;
    const SplitLane P = split_lane(A, g);
    uint32_t base, staged;
    split_stage(A, P, stage, &shared_base, base, staged);
    if (!P.active) return;
    const SyncTabs T = split_tabs(A, P);
    const SplitBytes src{stage, A.L.span, P.o0, base, staged};
    const uint2 stored = A.exits[g];
    SyncState s = sync_start(0);
    if (!P.first) {
        const uint2 e = A.exits[g - 1];
        s = sync_unpack(e.x, e.y);
    }
    const SplitSeg G = split_seg(A, P.k);
    const uint32_t quota = (uint32_t)G.rows * (uint32_t)A.L.seg_w;      // (rows <= seg_h: inside the segment's part of the plane)
    LjpegSplitWriter wr{A.plane + (size_t)P.k * A.L.seg_h * A.L.seg_w, ((A.counts[g] & segscan::MASK) - (stored.y >> 16)) & segscan::MASK,
                        quota, 0u};
    uint32_t n = 0;
    sync_lane(src, P.len, P.hi, P.last, 8 * A.sub, T, s, n, wr);
    const uint2 now = make_uint2(s.end ? 0u : s.p, sync_pack(s, n));
    if (!same2(now, stored)) wr.status |= ST_UNSYNCED;
    if (wr.status) atomicOr(A.stat + P.k, wr.status);
}

// predictor 1, first pass: one wave per segment scans down the first ncomp columns from the seed, in place
__global__ __launch_bounds__(64) void ljpeg_split_columns(ljpeg::SplitArgs A) {
    using namespace ljpeg;
    const uint32_t k = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const SplitSeg G = split_seg(A, k);
    if (!G.ok || G.pred != 1) return;
    const int W = A.L.seg_w;
    uint16_t* plane = A.plane + (size_t)k * A.L.seg_h * W;
    for (int c = 0; c < G.nc; ++c) {
        uint32_t carry = 1u << (G.prec - 1);
        for (int r0 = 0; r0 < G.rows; r0 += LANES) {
            const int r = r0 + lane;
            uint32_t x = r < G.rows ? (uint32_t)plane[(size_t)r * W + c] : 0u;
#pragma unroll
            for (int o = 1; o < LANES; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)x, o);
                if (lane >= o) x += y;
            }
            x = (x + carry) & 0xffffu;
            if (r < G.rows) plane[(size_t)r * W + c] = (uint16_t)x;
            carry = (uint32_t)__shfl((int)x, LANES - 1);
        }
    }
}

// predictor 1, second pass: one wave per segment row; table, shift, crop and store through ljpeg_store
template <typename T>
__global__ __launch_bounds__(256) void ljpeg_split_rows(ljpeg::SplitArgs A) {
    using namespace ljpeg;
    const int lane = (int)threadIdx.x & (LANES - 1);
    const size_t row = (size_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    const uint32_t k = (uint32_t)(row / (size_t)A.L.seg_h);
    const int r = (int)(row - (size_t)k * A.L.seg_h);
    if (k >= A.nseg) return;
    const SplitSeg G = split_seg(A, k);
    if (!G.ok || G.pred != 1 || r >= G.rows) return;        // (uniform over the wave)
    const int W = A.L.seg_w;
    const uint16_t* d = A.plane + ((size_t)k * A.L.seg_h + r) * W;
    const int sy = (int)k / A.L.nsx, sx = (int)k - sy * A.L.nsx;
    const int ys = sy * A.L.seg_h + r, xs0 = sx * W;
    uint32_t carry0 = 0, carry1 = 0;
    for (int c0 = 0; c0 < W; c0 += ROW_CHUNK) {
        const int i0 = c0 + lane * ROW_PER_LANE;
        uint32_t p[ROW_PER_LANE];
#pragma unroll
        for (int j = 0; j < ROW_PER_LANE; ++j) p[j] = i0 + j < W ? (uint32_t)d[i0 + j] : 0u;
        uint32_t t0, t1;
        if (G.nc == 1) {
#pragma unroll
            for (int j = 1; j < ROW_PER_LANE; ++j) p[j] += p[j - 1];
            t0 = p[ROW_PER_LANE - 1];
            t1 = 0;
        } else {
#pragma unroll
            for (int j = 2; j < ROW_PER_LANE; ++j) p[j] += p[j - 2];
            t0 = p[ROW_PER_LANE - 2];
            t1 = p[ROW_PER_LANE - 1];
        }
        uint32_t x0 = t0, x1 = t1;             // inclusive scan of the lanes' totals
#pragma unroll
        for (int o = 1; o < LANES; o <<= 1) {
            const uint32_t y0 = (uint32_t)__shfl_up((int)x0, o), y1 = (uint32_t)__shfl_up((int)x1, o);
            if (lane >= o) { x0 += y0; x1 += y1; }
        }
        const uint32_t a0 = x0 - t0 + carry0, a1 = x1 - t1 + carry1;      // exclusive, plus the carry
        carry0 += (uint32_t)__shfl((int)x0, LANES - 1);
        carry1 += (uint32_t)__shfl((int)x1, LANES - 1);
#pragma unroll
        for (int j = 0; j < ROW_PER_LANE; ++j)
            if (i0 + j < W) ljpeg_store<T>(A.L, ys, xs0 + i0 + j, (p[j] + (G.nc == 2 && (j & 1) ? a1 : a0)) & 0xffffu);
    }
}

// predictors 2 to 7: one wave per segment, raw_ljpeg's predict half over the difference plane
template <typename T>
__global__ __launch_bounds__(64) void ljpeg_split_segments(ljpeg::SplitArgs A) {
    using namespace ljpeg;
    extern __shared__ __attribute__((aligned(16))) unsigned char ljpeg_split_smem[];
    uint16_t* d = (uint16_t*)ljpeg_split_smem;      // a batch: differences, then values
    uint16_t* line = d + BATCH;                     // the line above (seg_w <= MAX_LINE)
    const int lane = (int)threadIdx.x;
    const uint32_t k = blockIdx.x;
    const SplitSeg G = split_seg(A, k);
    if (!G.ok || G.pred == 1) return;               // (pred != 1 and ok: seg_w <= MAX_LINE, the line is there)
    const int W = A.L.seg_w, nc = G.nc, pred = G.pred;
    const uint16_t* plane = A.plane + (size_t)k * A.L.seg_h * W;
    const int sy = (int)k / A.L.nsx, sx = (int)k - sy * A.L.nsx;
    uint32_t carry[2] = {0, 0};
    uint32_t ra[2] = {0, 0}, rc[2] = {0, 0};
    const int nb = (W + BATCH - 1) / BATCH;
    for (int r = 0; r < G.rows; ++r) {
        for (int b = 0; b < nb; ++b) {
            const int c0 = b * BATCH, n = min(BATCH, W - c0);
            __syncthreads();
            for (int i = lane; i < n; i += LANES) d[i] = plane[(size_t)r * W + c0 + i];
            __syncthreads();
            if (r == 0) {
                if (b == 0) { carry[0] = 1u << (G.prec - 1); carry[1] = carry[0]; }
                const int i0 = lane * PER_LANE;
                uint32_t p[PER_LANE];
#pragma unroll
                for (int j = 0; j < PER_LANE; ++j) p[j] = i0 + j < n ? (uint32_t)d[i0 + j] : 0u;
                uint32_t t0, t1;
                if (nc == 1) { p[1] += p[0]; p[2] += p[1]; p[3] += p[2]; t0 = p[3]; t1 = 0; }
                else { p[2] += p[0]; p[3] += p[1]; t0 = p[2]; t1 = p[3]; }
                uint32_t x0 = t0, x1 = t1;
#pragma unroll
                for (int o = 1; o < LANES; o <<= 1) {
                    const uint32_t y0 = (uint32_t)__shfl_up((int)x0, o), y1 = (uint32_t)__shfl_up((int)x1, o);
                    if (lane >= o) { x0 += y0; x1 += y1; }
                }
                x0 += carry[0] - t0;
                x1 += carry[1] - t1;
                __syncthreads();
#pragma unroll
                for (int j = 0; j < PER_LANE; ++j)
                    if (i0 + j < n) {
                        const uint32_t v = (p[j] + (nc == 2 && (j & 1) ? x1 : x0)) & 0xffffu;
                        d[i0 + j] = (uint16_t)v;
                        line[c0 + i0 + j] = (uint16_t)v;
                    }
                __syncthreads();
                carry[0] = d[n - nc];
                carry[1] = d[n - 1];
            } else if (pred == 2) {
                for (int i = lane; i < n; i += LANES) {
                    const uint32_t v = ((uint32_t)line[c0 + i] + d[i]) & 0xffffu;
                    d[i] = (uint16_t)v;
                    line[c0 + i] = (uint16_t)v;
                }
                __syncthreads();
            } else {
                if (lane == 0) {
                    for (int i = 0; i < n; ++i) {
                        const int c = nc == 2 ? i & 1 : 0;
                        const int col = c0 + i;
                        const int Rb = line[col], Ra = (int)(c ? ra[1] : ra[0]), Rc = (int)(c ? rc[1] : rc[0]);
                        int px;
                        if (col < nc) px = Rb;
                        else if (pred == 3) px = Rc;
                        else if (pred == 4) px = Ra + Rb - Rc;
                        else if (pred == 5) px = Ra + ((Rb - Rc) >> 1);
                        else if (pred == 6) px = Rb + ((Ra - Rc) >> 1);
                        else px = (Ra + Rb) >> 1;
                        const uint32_t v = ((uint32_t)px + d[i]) & 0xffffu;
                        line[col] = (uint16_t)v;
                        if (c) { ra[1] = v; rc[1] = (uint32_t)Rb; } else { ra[0] = v; rc[0] = (uint32_t)Rb; }
                        d[i] = (uint16_t)v;
                    }
                }
                __syncthreads();
            }
            const int ys = sy * A.L.seg_h + r, xs0 = sx * W + c0;
            for (int i = lane; i < n; i += LANES) ljpeg_store<T>(A.L, ys, xs0 + i, d[i]);
        }
    }
}

__global__ __launch_bounds__(256) void ljpeg_split_status(ljpeg::SplitArgs A) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= A.nseg) return;
    uint32_t st = A.stat[k];
    if ((A.incl[k] & segscan::MASK) > A.lanes) st |= MI_LJPEG_UNDECODED;      // (descriptors that overlap: lanes were cut off)
    if (st & ljpeg::ST_UNSYNCED) st = ljpeg::ST_UNSYNCED;
    if (A.L.status) A.L.status[k] = st;
    if (A.L.status_or && st) atomicOr(A.L.status_or, st);
}

// arguments checked by the caller (capi.hip); `words` is the scratch split_layout describes.  `plane_out`: null, or where
// the differences go in place of the scratch's plane -- then nothing is predicted and `out` is not written (the tap for tests).
inline void ljpeg_split_launch(hipStream_t st, const void* span, size_t span_bytes, const mi_ljpeg_seg_t* segs, const mi_raw_layout_t& R,
                               const uint16_t* table, uint32_t sub, uint32_t max_rounds, uint32_t* words, void* out, uint16_t* plane_out,
                               uint32_t* status, uint32_t* status_or) {
    using namespace ljpeg;
    const SplitLayout L = split_layout(R, span_bytes, sub, max_rounds);
    SplitArgs A{};
    A.L.span = (const uint8_t*)span; A.L.segs = segs; A.L.table = R.table_len > 0 ? table : nullptr; A.L.out = out;
    A.L.status = status; A.L.status_or = status_or;
    A.L.span_bytes = (uint32_t)span_bytes;
    A.L.h = R.height; A.L.w = R.width; A.L.crop_y = R.crop_y; A.L.crop_x = R.crop_x; A.L.image_h = R.image_height;
    A.L.seg_h = R.seg_height; A.L.seg_w = R.seg_width; A.L.nsx = unpack_nsx(R); A.L.tiled = R.tiled;
    A.L.shift = R.shift; A.L.table_len = R.table_len;
    A.incl = words + L.incl; A.exits = (uint2*)(words + L.exits); A.alts = (uint2*)(words + L.alts); A.counts = words + L.counts;
    A.gentry = (uint2*)(words + L.gentry); A.bnd = (uint2*)(words + L.bnd); A.flags = words + L.flags; A.stat = words + L.stat;
    A.huff = (Huff*)(words + L.huff); A.lut = (uint16_t*)(words + L.lut);
    A.plane = plane_out ? plane_out : (uint16_t*)(words + L.plane);
    A.nseg = (uint32_t)L.nseg; A.sub = sub; A.lanes = (uint32_t)L.lanes; A.groups = (uint32_t)L.groups;
    uint32_t* tmp = words + L.tmp;
    const unsigned ns = (unsigned)L.nseg, nflags = (unsigned)L.rounds + 2;
    const size_t lds = jpeg::split_stage_bytes(sub);
    (void)hipMemsetAsync(A.plane, 0, L.samples * sizeof(uint16_t), st);
    hipLaunchKernelGGL(ljpeg_split_prep, dim3(ns), dim3(256), 0, st, A, nflags);
    segscan::launch(st, A.incl, ns, tmp);
    for (uint32_t r = 0; r <= (uint32_t)L.rounds; ++r)
        hipLaunchKernelGGL(ljpeg_split_round, dim3((unsigned)L.groups), dim3(SPLIT_GROUP), lds, st, A, r);
    segscan::launch(st, A.counts, L.lanes, tmp);
    hipLaunchKernelGGL(ljpeg_split_write, dim3((unsigned)L.groups), dim3(SPLIT_GROUP), lds, st, A);
    if (!plane_out) {
        const size_t rows = L.nseg * (size_t)R.seg_height;
        const dim3 rgrid((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK));
        const size_t slds = BATCH * 2 + (R.seg_width <= MAX_LINE ? 2 * (size_t)((R.seg_width + 7) & ~7) : 0);
        hipLaunchKernelGGL(ljpeg_split_columns, dim3(ns), dim3(LANES), 0, st, A);
        if (R.dtype == MI_U8) {
            hipLaunchKernelGGL(ljpeg_split_rows<uint8_t>, rgrid, dim3(256), 0, st, A);
            hipLaunchKernelGGL(ljpeg_split_segments<uint8_t>, dim3(ns), dim3(LANES), slds, st, A);
        } else {
            hipLaunchKernelGGL(ljpeg_split_rows<uint16_t>, rgrid, dim3(256), 0, st, A);
            hipLaunchKernelGGL(ljpeg_split_segments<uint16_t>, dim3(ns), dim3(LANES), slds, st, A);
        }
    }
    hipLaunchKernelGGL(ljpeg_split_status, dim3((ns + 255) / 256), dim3(256), 0, st, A);
}

}  // namespace mi
