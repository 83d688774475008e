// kernels_jpeg_split.hpp -- the second entropy path of the JPEG decoder: a restart interval of ANY length, a scan in one piece
// included, decoded on many lanes at once and exactly (jpeg_sync_core.hpp has the transition and the reasoning; the definition
// is tests/jpeg_split_restatement.py, held bit for bit).  It fills the coefficient planes jpeg_entropy fills, for jpeg_idct and
// jpeg_colour as they are.  No reference counterpart.
//
// The scan's subsequences -- sub_bytes bytes each, counted interval after interval, at least one per interval -- are the
// lanes, 256 consecutive ones a workgroup ("group"); an interval may cover many groups and a group many intervals.
//
//   jpeg_split_prep     per interval: its subsequence count (from the offsets, clamped to the span), its status word zeroed.
//                       seg_scan then gives every interval its first lane; a lane finds its interval by bisection.
//   jpeg_split_round    round 0 (passes 1 and 2 of the scheme): every lane walks its subsequence from its cold state, then the
//                       group iterates in LDS -- a lane walks again when its predecessor's exit changed -- until no lane
//                       changes, at most 256 times.  Round r > 0: the group's first lane takes the exit its predecessor
//                       group left in round r - 1 (two boundary arrays, written in alternation, so no group reads what
//                       another writes in the same launch) and the group converges again.  A round returns at once when the
//                       round before it changed no boundary (a flag word per round).  After r rounds the first r + 1 groups
//                       of an interval are exact, so groups - 1 rounds always suffice; photographs need none or one.
//   jpeg_split_write    pass 3: every lane walks once more from its predecessor's stored exit, its first block given by the
//                       segmented scan of the block counts, and writes the non-zero coefficients and the DC differences of
//                       the blocks of its interval's quota into planes zeroed beforehand.  Status bits come from this pass
//                       alone.  A lane whose walk does not reproduce its stored exit sets ST_UNSYNCED: the rounds were too few.
//   jpeg_split_dc_*     pass 4: the DC differences gathered in scan order per component, summed mod 2^16 by seg_scan with a
//                       restart at every interval, scattered back.
//   jpeg_split_status   an unsynced interval reports ST_UNSYNCED and nothing else: its other bits came from wrong states.
//
// Bytes: a group's 256 * sub_bytes bytes and 24 more are staged into LDS with coalesced dword loads and every walk reads
// LDS; the stage is padded by 4 bytes every 128, which puts the 32 lanes of a half-wave, sub_bytes apart, on 32 different
// banks for every sub_bytes from 8 to 128 (byte reads bank by (a / 4) % 32).  A byte outside the stage -- which only offsets
// that the host forms refuse can ask for -- is read from the span.  No workgroup ever waits for another: the rounds are
// separate launches.  Bounded by construction: every byte index is checked against the interval, every interval against the
// span, every lane against the arrays' lengths, and a lane writes only blocks below its interval's quota.
#pragma once
#include "common.hpp"
#include "jpeg_sync_core.hpp"
#include "kernels_jpeg.hpp"

namespace mi {

// ---- a segmented inclusive sum over uint32 words: bits 0 .. 30 the value (sums mod 2^31), bit 31 set where a segment starts.
// Three kernels a level: the blocks of 1024 scan themselves, their totals are scanned the same way (recursively), and every
// block takes its predecessors' total in.  Integer addition is associative, so the result does not depend on the grouping.
namespace segscan {
constexpr uint32_t HEAD = 0x80000000u, MASK = 0x7fffffffu;
constexpr int THREADS = 256, ITEMS = 4, BLOCK = THREADS * ITEMS;
__host__ __device__ inline uint32_t op(uint32_t a, uint32_t b) { return (b & HEAD) ? b : ((a & HEAD) | ((a + b) & MASK)); }

__global__ __launch_bounds__(THREADS) void seg_scan_block(uint32_t* v, size_t n, uint32_t* totals) {
    __shared__ uint32_t part[THREADS];
    const int t = (int)threadIdx.x;
    const size_t at = ((size_t)blockIdx.x * THREADS + t) * ITEMS;
    uint32_t x[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) x[i] = at + i < n ? v[at + i] : 0u;
#pragma unroll
    for (int i = 1; i < ITEMS; ++i) x[i] = op(x[i - 1], x[i]);
    part[t] = x[ITEMS - 1];
    __syncthreads();
#pragma unroll
    for (int d = 1; d < THREADS; d <<= 1) {
        const uint32_t mine = part[t], left = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] = op(left, mine);
        __syncthreads();
    }
    const uint32_t before = t ? part[t - 1] : 0u;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i)
        if (at + i < n) v[at + i] = op(before, x[i]);
    if (t == THREADS - 1) totals[blockIdx.x] = part[t];
}

__global__ __launch_bounds__(THREADS) void seg_scan_carry(uint32_t* v, size_t n, const uint32_t* totals) {
    if (blockIdx.x == 0) return;
    const uint32_t carry = totals[blockIdx.x - 1];
    const size_t at = ((size_t)blockIdx.x * THREADS + threadIdx.x) * ITEMS;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i)
        if (at + i < n) v[at + i] = op(carry, v[at + i]);
}

inline size_t blocks(size_t n) { return (n + BLOCK - 1) / BLOCK; }
// the words of scratch a scan of n words needs
inline size_t tmp_words(size_t n) {
    size_t w = 0;
    while (n > 1) {
        n = blocks(n);
        w += (n + 63) & ~(size_t)63;
    }
    return w + 64;
}
inline void launch(hipStream_t st, uint32_t* v, size_t n, uint32_t* tmp) {
    if (n == 0) return;
    const size_t nb = blocks(n);
    hipLaunchKernelGGL(seg_scan_block, dim3((unsigned)nb), dim3(THREADS), 0, st, v, n, tmp);
    if (nb > 1) {
        launch(st, tmp, nb, tmp + ((nb + 63) & ~(size_t)63));
        hipLaunchKernelGGL(seg_scan_carry, dim3((unsigned)nb), dim3(THREADS), 0, st, v, n, (const uint32_t*)tmp);
    }
}
}  // namespace segscan

namespace jpeg {
constexpr int SPLIT_GROUP = 256;            // lanes a workgroup
constexpr uint32_t SPLIT_SUB_DEFAULT = 128, SPLIT_ROUNDS_DEFAULT = 8;
constexpr uint32_t SPLIT_OVERSHOOT = 24;    // bytes staged behind the group's last subsequence: a symbol reads at most 11

inline size_t split_lanes(size_t span_bytes, uint32_t sub, const mi_jpeg_t& J) { return (span_bytes + sub - 1) / sub + (size_t)J.n_intervals; }
inline size_t split_groups(size_t lanes) { return (lanes + SPLIT_GROUP - 1) / SPLIT_GROUP; }
__host__ __device__ inline uint32_t split_stage_index(uint32_t a) { return a + ((a >> 7) << 2); }
inline uint32_t split_stage_bytes(uint32_t sub) { return split_stage_index(SPLIT_GROUP * sub + SPLIT_OVERSHOOT + 4) + 8; }

// the scratch behind the coefficient and sample planes, in words
struct SplitLayout {
    size_t lanes, groups, rounds;
    size_t incl, exits, counts, gentry, bnd, flags, status, dc, tmp, words;
};
inline SplitLayout split_layout(size_t span_bytes, uint32_t sub, uint32_t max_rounds, const mi_jpeg_t& J, size_t nblocks) {
    SplitLayout L{};
    L.lanes = split_lanes(span_bytes, sub, J);
    L.groups = split_groups(L.lanes);
    L.rounds = L.groups > 1 ? (max_rounds < L.groups - 1 ? max_rounds : L.groups - 1) : 0;
    size_t at = 0;
    auto take = [&](size_t words) { const size_t o = at; at += (words + 63) & ~(size_t)63; return o; };
    L.incl = take((size_t)J.n_intervals);
    L.exits = take(2 * L.lanes);
    L.counts = take(L.lanes);
    L.gentry = take(2 * L.groups);
    L.bnd = take(4 * L.groups);
    L.flags = take(L.rounds + 2);
    L.status = take((size_t)J.n_intervals);
    L.dc = take(nblocks);
    const size_t longest = L.lanes > nblocks ? L.lanes : nblocks;
    L.tmp = take(segscan::tmp_words(longest > (size_t)J.n_intervals ? longest : (size_t)J.n_intervals));
    L.words = at;
    return L;
}

struct SplitArgs {
    const uint8_t* span;
    const uint32_t* offsets;
    uint32_t* incl;         // per interval: lanes of it and of every interval before it (seg_scan of the counts)
    uint2* exits;           // per lane: its exit state and block count (sync_pack)
    uint32_t* counts;       // per lane: its block count, bit 31 on an interval's first lane; scanned before pass 3
    uint2* gentry;          // per group: the entry its first lane last walked from
    uint2* bnd;             // two arrays of one exit per group
    uint32_t* flags;        // per round: a boundary changed
    uint32_t* status;
    int16_t* coef;
    uint32_t* dc;
    uint32_t span_bytes, sub, lanes;
    Geom G;
    mi_jpeg_t J;
};

// a lane's place: its interval and the bytes of its subsequence
struct SplitLane {
    bool active;
    uint32_t i, o0, len, lo, hi;
    bool first, last;
};
__device__ inline SplitLane split_lane(const SplitArgs& A, uint32_t g) {
    SplitLane P{};
    const uint32_t n = (uint32_t)A.J.n_intervals;
    const uint32_t total = A.incl[n - 1] & segscan::MASK;
    uint32_t lo = 0, hi = n - 1;        // the first interval whose inclusive count exceeds g (bisection: trip count log2 n)
    for (int it = 0; it < 32; ++it) {
        if (lo >= hi) break;
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((A.incl[mid] & segscan::MASK) > g) hi = mid;
        else lo = mid + 1;
    }
    P.i = lo;
    const uint32_t before = lo ? A.incl[lo - 1] & segscan::MASK : 0u;
    const uint32_t o0 = min(A.offsets[lo], A.span_bytes), o1 = min(A.offsets[lo + 1], A.span_bytes);
    P.o0 = o0;
    P.len = o1 > o0 ? o1 - o0 : 0u;
    const uint32_t nsub = max(1u, (P.len + A.sub - 1) / A.sub);
    const uint32_t j = g - before;
    P.active = g < total && g < A.lanes && g >= before && j < nsub;
    P.first = j == 0;
    P.last = j == nsub - 1;
    P.lo = P.active ? j * A.sub : 0u;
    P.hi = min(P.lo + A.sub, P.len);
    return P;
}

// the interval's bytes: from the group's stage in LDS where they lie in it, else from the span
struct StagedBytes {
    const uint8_t* stage;
    const uint8_t* span;
    uint32_t o0, base, staged;      // the interval's first byte, the stage's first byte (both in the span), bytes staged
    __device__ uint32_t byte(uint32_t i) const {
        const uint32_t a = o0 + i, d = a - base;
        return d < staged ? stage[split_stage_index(d)] : span[a];
    }
};

// the group's tables and bytes into LDS; returns the stage's first byte in the span (4-byte aligned) through `base`
__device__ inline void split_stage(const SplitArgs& A, const SplitLane& P, Huff256* tabs, uint8_t* stage, uint32_t* shared_base,
                                   uint32_t& base, uint32_t& staged) {
    const int t = (int)threadIdx.x;
    if (t < 4) huff_build(tabs[t], A.J.counts[t], A.J.values[t]);
    if (t == 0) *shared_base = min(P.o0 + P.lo, A.span_bytes) & ~3u;
    __syncthreads();
    base = *shared_base;
    const uint32_t want = SPLIT_GROUP * A.sub + SPLIT_OVERSHOOT + 4;
    staged = min(want, A.span_bytes - base);
    for (uint32_t d = 4u * t; d < staged; d += 4u * SPLIT_GROUP) {
        uint32_t w;
        if (d + 4 <= staged) {
            w = *(const uint32_t*)(A.span + base + d);
        } else {
            w = 0;
            for (uint32_t k = 0; k < 3; ++k)
                if (d + k < staged) w |= (uint32_t)A.span[base + d + k] << (8 * k);
        }
        *(uint32_t*)(stage + split_stage_index(d)) = w;
    }
    __syncthreads();
}

__device__ inline SyncTabs split_tabs(const SplitArgs& A, const Huff256* tabs) {
    SyncTabs T{};
    T.tabs = tabs;
    uint32_t n = 0;
    for (int c = 0; c < A.J.ncomp; ++c)
        for (int k = 0; k < A.G.h[c] * A.G.v[c]; ++k) {
            T.dc[n & 7] = A.J.td[c];
            T.ac[n & 7] = A.J.ta[c];
            ++n;
        }
    T.nbm = n;
    return T;
}

__device__ inline bool same2(uint2 a, uint2 b) { return a.x == b.x && a.y == b.y; }
}  // namespace jpeg

__global__ __launch_bounds__(256) void jpeg_split_prep(jpeg::SplitArgs A, uint32_t n_flags) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_flags) A.flags[i] = 0;
    if (i >= (uint32_t)A.J.n_intervals) return;
    const uint32_t o0 = min(A.offsets[i], A.span_bytes), o1 = min(A.offsets[i + 1], A.span_bytes);
    const uint32_t len = o1 > o0 ? o1 - o0 : 0u;
    A.incl[i] = max(1u, (len + A.sub - 1) / A.sub) | (i == 0 ? segscan::HEAD : 0u);
    A.status[i] = 0;
}

__global__ __launch_bounds__(256) void jpeg_split_round(jpeg::SplitArgs A, uint32_t round) {
    using namespace jpeg;
    extern __shared__ __align__(16) uint8_t stage[];
    __shared__ Huff256 tabs[4];
    __shared__ uint2 ex[SPLIT_GROUP];
    __shared__ uint32_t chg[SPLIT_GROUP];
    __shared__ uint32_t shared_base;
    if (round > 0 && A.flags[round - 1] == 0) return;      // the round before changed no boundary: nothing can change
    const int t = (int)threadIdx.x;
    const uint32_t grp = blockIdx.x, g = grp * SPLIT_GROUP + t;
    const SplitLane P = split_lane(A, g);
    uint32_t base, staged;
    split_stage(A, P, tabs, stage, &shared_base, base, staged);
    const SyncTabs T = split_tabs(A, tabs);
    const StagedBytes src{stage, A.span, P.o0, base, staged};
    const uint32_t max_symbols = 8 * A.sub;
    SyncNoEmit none;
    const uint2 ended = make_uint2(0u, 1u << 12);

    // a walk from `e`, packed
    auto walk = [&](uint2 e) {
        SyncState s = P.first ? sync_start(0) : sync_unpack(e.x, e.y);
        uint32_t n = 0;
        sync_lane(src, P.len, P.hi, P.last, max_symbols, T, s, n, none);
        return make_uint2(s.end ? 0u : s.p, sync_pack(s, n));
    };
    uint2 e0 = make_uint2(0, 0);        // lane 0: the entry from outside the group
    bool need = false;
    if (round == 0) {
        const SyncState c = sync_cold(src, P.len, P.lo);
        const uint2 cold = make_uint2(c.p, sync_pack(c, 0));
        ex[t] = P.active ? walk(cold) : ended;
        if (t == 0) {
            e0 = cold;
            A.gentry[grp] = cold;
            if (grp == 0) A.flags[0] = 1;
        }
        need = P.active && !P.first && t > 0;
    } else {
        ex[t] = g < A.lanes ? A.exits[g] : ended;
        if (t == 0) {
            e0 = grp ? A.bnd[(size_t)((round - 1) & 1) * gridDim.x + grp - 1] : ended;
            e0.y &= 0xffffu;
            need = P.active && !P.first && grp > 0 && !same2(e0, A.gentry[grp]);
            if (need) A.gentry[grp] = e0;
        }
    }
    chg[t] = 0;
    __syncthreads();
    for (int it = 0; it < SPLIT_GROUP; ++it) {      // (a change moves on by one lane or more an iteration)
        bool c = false;
        uint2 nw = make_uint2(0, 0);
        if (need) {
            uint2 e = e0;
            if (t > 0) {
                e = ex[t - 1];
                e.y &= 0xffffu;
            }
            nw = walk(e);
            c = !same2(nw, ex[t]);
        }
        __syncthreads();
        if (c) ex[t] = nw;
        chg[t] = c ? 1u : 0u;
        __syncthreads();
        need = P.active && !P.first && t > 0 && chg[t - 1] != 0;
        if (!__syncthreads_or(need ? 1 : 0)) break;
    }
    if (g < A.lanes) {
        A.exits[g] = ex[t];
        A.counts[g] = (P.active ? ex[t].y >> 16 : 0u) | (P.first || !P.active ? segscan::HEAD : 0u);
    }
    if (t == SPLIT_GROUP - 1) {
        uint2* mine = A.bnd + (size_t)(round & 1) * gridDim.x + grp;
        if (round > 0) {
            const uint2 was = A.bnd[(size_t)((round - 1) & 1) * gridDim.x + grp];
            if (!same2(was, ex[t])) atomicOr(A.flags + round, 1u);
        }
        *mine = ex[t];
    }
}

// what pass 3 does with a symbol
struct SplitWriter {
    const jpeg::SplitArgs& A;
    uint32_t i, B, quota, nbm, status;
    __device__ void symbol(const jpeg::SyncSym& y) {
        if (B >= quota) return;
        status |= y.status;
        if (y.at >= 0 && (y.val != 0 || y.at == 0)) {
            const long long mcu = (long long)i * A.J.dri + B / nbm;
            const uint32_t bb = B % nbm, hv = (uint32_t)(A.G.h[0] * A.G.v[0]);
            const int c = bb < hv ? 0 : (int)(bb - hv) + 1;
            const int by = c == 0 ? (int)bb / A.G.h[0] : 0, bx = c == 0 ? (int)bb % A.G.h[0] : 0;
            const int my = (int)(mcu / A.G.mcus_x), mx = (int)(mcu - (long long)my * A.G.mcus_x);
            const size_t b = A.G.boff[c] + (size_t)(my * A.G.v[c] + by) * A.G.bw[c] + (size_t)(mx * A.G.h[c] + bx);
            if (b < A.G.nblocks) A.coef[b * 64 + jpeg::zigzag(y.at)] = (int16_t)(uint16_t)y.val;
        }
        B += y.done ? 1u : 0u;
    }
    __device__ void end() {
        if (B < quota) status |= jpeg::ST_OVERRUN;
    }
};

__global__ __launch_bounds__(256) void jpeg_split_write(jpeg::SplitArgs A) {
    using namespace jpeg;
    extern __shared__ __align__(16) uint8_t stage[];
    __shared__ Huff256 tabs[4];
    __shared__ uint32_t shared_base;
    const int t = (int)threadIdx.x;
    const uint32_t g = blockIdx.x * SPLIT_GROUP + t;
    const SplitLane P = split_lane(A, g);
    uint32_t base, staged;
    split_stage(A, P, tabs, stage, &shared_base, base, staged);
    if (!P.active) return;
    const SyncTabs T = split_tabs(A, tabs);
    const StagedBytes src{stage, A.span, P.o0, base, staged};
    const uint2 stored = A.exits[g];
    SyncState s = sync_start(0);
    if (!P.first) {
        const uint2 e = A.exits[g - 1];
        s = sync_unpack(e.x, e.y);
    }
    const long long first = (long long)P.i * A.J.dri;
    const long long mcus = first < A.G.n_mcus ? min((long long)A.J.dri, A.G.n_mcus - first) : 0;
    SplitWriter wr{A, P.i, ((A.counts[g] & segscan::MASK) - (stored.y >> 16)) & segscan::MASK, (uint32_t)mcus * T.nbm, T.nbm, 0u};
    uint32_t n = 0;
    sync_lane(src, P.len, P.hi, P.last, 8 * A.sub, T, s, n, wr);
    const uint2 now = make_uint2(s.end ? 0u : s.p, sync_pack(s, n));
    if (!same2(now, stored)) wr.status |= ST_UNSYNCED;
    if (wr.status) atomicOr(A.status + P.i, wr.status);
}

namespace jpeg {
// block e of the scan-order list (component after component, MCU after MCU, the component's blocks of the MCU in T.81 order):
// its place among the planes' blocks, and whether a restart interval begins with it
__device__ inline size_t split_dc_block(const SplitArgs& A, size_t e, bool& head) {
    int c = 0;
    size_t at = e;
    for (int k = 0; k < 2; ++k) {
        const size_t nc = (size_t)A.G.n_mcus * (A.G.h[c] * A.G.v[c]);
        if (c + 1 < A.J.ncomp && at >= nc) {
            at -= nc;
            ++c;
        }
    }
    const int per = A.G.h[c] * A.G.v[c];
    const long long mcu = (long long)(at / per);
    const int bb = (int)(at - (size_t)mcu * per);
    head = bb == 0 && mcu % A.J.dri == 0;
    const int my = (int)(mcu / A.G.mcus_x), mx = (int)(mcu - (long long)my * A.G.mcus_x);
    const int by = bb / A.G.h[c], bx = bb % A.G.h[c];
    return A.G.boff[c] + (size_t)(my * A.G.v[c] + by) * A.G.bw[c] + (size_t)(mx * A.G.h[c] + bx);
}
}  // namespace jpeg

__global__ __launch_bounds__(256) void jpeg_split_dc_gather(jpeg::SplitArgs A) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= A.G.nblocks) return;
    bool head;
    const size_t b = jpeg::split_dc_block(A, e, head);
    A.dc[e] = (b < A.G.nblocks ? (uint32_t)(uint16_t)A.coef[b * 64] : 0u) | (head ? segscan::HEAD : 0u);
}

__global__ __launch_bounds__(256) void jpeg_split_dc_scatter(jpeg::SplitArgs A) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= A.G.nblocks) return;
    bool head;
    const size_t b = jpeg::split_dc_block(A, e, head);
    if (b < A.G.nblocks) A.coef[b * 64] = (int16_t)(uint16_t)(A.dc[e] & 0xffffu);
}

// `out` may be the array the passes wrote into
__global__ __launch_bounds__(256) void jpeg_split_status(jpeg::SplitArgs A, uint32_t* out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint32_t)A.J.n_intervals) return;
    uint32_t st = A.status[i];
    if ((A.incl[i] & segscan::MASK) > A.lanes) st |= jpeg::ST_OVERRUN;      // (offsets the host forms refuse: lanes were cut off)
    if (out) out[i] = (st & jpeg::ST_UNSYNCED) ? jpeg::ST_UNSYNCED : st;
}

// arguments checked by the caller (capi.hip); `words` is the scratch split_layout describes
inline void jpeg_split_launch(hipStream_t st, const void* span, size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t& J, uint32_t sub,
                              uint32_t max_rounds, uint32_t* words, int16_t* coef, uint32_t* status) {
    using namespace jpeg;
    SplitArgs A{};
    A.G = geom(J);
    A.J = J;
    const SplitLayout L = split_layout(span_bytes, sub, max_rounds, J, A.G.nblocks);
    A.span = (const uint8_t*)span; A.offsets = offsets; A.coef = coef;
    A.incl = words + L.incl; A.exits = (uint2*)(words + L.exits); A.counts = words + L.counts;
    A.gentry = (uint2*)(words + L.gentry); A.bnd = (uint2*)(words + L.bnd); A.flags = words + L.flags;
    A.status = words + L.status; A.dc = words + L.dc;
    A.span_bytes = (uint32_t)span_bytes; A.sub = sub; A.lanes = (uint32_t)L.lanes;
    uint32_t* tmp = words + L.tmp;
    const unsigned ni = (unsigned)J.n_intervals, nflags = (unsigned)L.rounds + 2;
    const size_t lds = split_stage_bytes(sub);
    (void)hipMemsetAsync(coef, 0, A.G.nblocks * 128, st);
    hipLaunchKernelGGL(jpeg_split_prep, dim3(((ni > nflags ? ni : nflags) + 255) / 256), dim3(256), 0, st, A, nflags);
    segscan::launch(st, A.incl, ni, tmp);
    for (uint32_t r = 0; r <= (uint32_t)L.rounds; ++r)
        hipLaunchKernelGGL(jpeg_split_round, dim3((unsigned)L.groups), dim3(SPLIT_GROUP), lds, st, A, r);
    segscan::launch(st, A.counts, L.lanes, tmp);
    hipLaunchKernelGGL(jpeg_split_write, dim3((unsigned)L.groups), dim3(SPLIT_GROUP), lds, st, A);
    const unsigned nb = (unsigned)((A.G.nblocks + 255) / 256);
    hipLaunchKernelGGL(jpeg_split_dc_gather, dim3(nb), dim3(256), 0, st, A);
    segscan::launch(st, A.dc, A.G.nblocks, tmp);
    hipLaunchKernelGGL(jpeg_split_dc_scatter, dim3(nb), dim3(256), 0, st, A);
    hipLaunchKernelGGL(jpeg_split_status, dim3((ni + 255) / 256), dim3(256), 0, st, A, status);
}

}  // namespace mi
