// kernels_jpeg_split.hpp -- the second entropy path of the JPEG decoder: a restart interval of ANY length, a scan in one piece
// included, decoded on many lanes at once and exactly (jpeg_sync_core.hpp has the transition, kernels_split_common.hpp the
// lanes, the bytes, the rounds and the frame of the write pass; the definition is tests/jpeg_split_restatement.py, held bit
// for bit).  It fills the coefficient planes jpeg_entropy fills, for jpeg_idct and jpeg_colour as they are.  No reference
// counterpart.  The scaffold's units are the scan's restart intervals.
//
//   jpeg_split_prep     per interval: its subsequence count (from the offsets, clamped to the span), its status word zeroed.
//                       seg_scan then gives every interval its first lane.
//   jpeg_split_round    the scaffold's rounds (passes 1 and 2 of the scheme), one exit a lane; the four tables in LDS.
//   jpeg_split_write    pass 3, the scaffold's write pass: a lane's first block is given by the segmented scan of the block
//                       counts, and it writes the non-zero coefficients and the DC differences of the blocks of its
//                       interval's quota into planes zeroed beforehand.
//   jpeg_split_dc_*     pass 4: the DC differences gathered in scan order per component, summed mod 2^16 by seg_scan with a
//                       restart at every interval, scattered back.
//   jpeg_split_status   an unsynced interval reports ST_UNSYNCED and nothing else: its other bits came from wrong states.
//
// Only offsets that the host forms refuse can ask for a byte outside a group's stage.  A lane writes only blocks below its
// interval's quota and inside the planes.
#pragma once
#include "common.hpp"
#include "jpeg_sync_core.hpp"
#include "kernels_jpeg.hpp"
#include "kernels_split_common.hpp"

namespace mi {

namespace jpeg {
// the scratch behind the coefficient and sample planes, in words
struct SplitLayout {
    split::Layout S;
    size_t status, dc, tmp, words;
};
inline SplitLayout split_layout(size_t span_bytes, uint32_t sub, uint32_t max_rounds, const mi_jpeg_t& J, size_t nblocks) {
    SplitLayout L{};
    split::Take take;
    L.S = split::layout(take, span_bytes, sub, max_rounds, (size_t)J.n_intervals, false);
    L.status = take((size_t)J.n_intervals);
    L.dc = take(nblocks);
    const size_t longest = L.S.lanes > nblocks ? L.S.lanes : nblocks;
    L.tmp = take(segscan::tmp_words(longest > (size_t)J.n_intervals ? longest : (size_t)J.n_intervals));
    L.words = take.at;
    return L;
}

struct SplitArgs {
    split::Args S;          // the span and the scaffold's arrays; counts are blocks that ended
    const uint32_t* offsets;
    uint32_t* status;
    int16_t* coef;
    uint32_t* dc;
    Geom G;
    mi_jpeg_t J;
};

// interval i's bytes, clamped to the span
__device__ inline void split_interval(const SplitArgs& A, uint32_t i, uint32_t& o0, uint32_t& len) {
    o0 = min(A.offsets[i], A.S.span_bytes);
    const uint32_t o1 = min(A.offsets[i + 1], A.S.span_bytes);
    len = o1 > o0 ? o1 - o0 : 0u;
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

// what the scaffold's bodies ask of a decoder (kernels_split_common.hpp)
struct SplitDecoder {
    static constexpr bool TWO = false;
    static constexpr uint32_t ENDED = 1u << 12;
    using Lane = split::Lane;
    const SplitArgs& A;
    Huff256* tabs;          // four, in LDS
    struct Walker {
        const Lane& P;
        const split::StagedBytes& src;
        const SyncTabs& T;
        uint32_t max_symbols;
        __device__ uint2 cold() const {
            const SyncState c = sync_cold(src, P.len, P.lo);
            return make_uint2(c.p, sync_pack(c, 0));
        }
        template <class Emit>
        __device__ uint2 walk(uint2 e, Emit& emit) const {
            SyncState s = P.first ? sync_start(0) : sync_unpack(e.x, e.y);
            uint32_t n = 0;
            sync_lane(src, P.len, P.hi, P.last, max_symbols, T, s, n, emit);
            return make_uint2(s.end ? 0u : s.p, sync_pack(s, n));
        }
    };
    __device__ Lane lane(uint32_t g) const {
        return split::place_lane(A.S.incl, (uint32_t)A.J.n_intervals, g, A.S.lanes, A.S.sub, [&](uint32_t i, uint32_t& o0, uint32_t& len) {
            split_interval(A, i, o0, len);
            return true;
        });
    }
    __device__ void prepare() const {
        if (threadIdx.x < 4) huff_build(tabs[threadIdx.x], A.J.counts[threadIdx.x], A.J.values[threadIdx.x]);
    }
    __device__ SyncTabs tabs_of(const Lane&) const { return split_tabs(A, tabs); }
};
}  // namespace jpeg

// (sync_nsub: max(1, (len + sub - 1) / sub) wherever that sum does not wrap, len < 2^32 - sub; a span is far shorter)
__global__ __launch_bounds__(256) void jpeg_split_prep(jpeg::SplitArgs A, uint32_t n_flags) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_flags) A.S.flags[i] = 0;
    if (i >= (uint32_t)A.J.n_intervals) return;
    uint32_t o0, len;
    jpeg::split_interval(A, i, o0, len);
    A.S.incl[i] = sync::sync_nsub(len, A.S.sub) | (i == 0 ? segscan::HEAD : 0u);
    A.status[i] = 0;
}

__global__ __launch_bounds__(256) void jpeg_split_round(jpeg::SplitArgs A, uint32_t round) {
    extern __shared__ __align__(16) uint8_t stage[];
    __shared__ jpeg::Huff256 tabs[4];
    split::round_body(jpeg::SplitDecoder{A, tabs}, A.S, round, stage);
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
    extern __shared__ __align__(16) uint8_t stage[];
    __shared__ jpeg::Huff256 tabs[4];
    split::write_body(jpeg::SplitDecoder{A, tabs}, A.S, stage, A.status, [&](const jpeg::SplitDecoder::Walker& W, uint32_t first_block) {
        const long long first = (long long)W.P.k * A.J.dri;
        const long long mcus = first < A.G.n_mcus ? min((long long)A.J.dri, A.G.n_mcus - first) : 0;
        return SplitWriter{A, W.P.k, first_block, (uint32_t)mcus * W.T.nbm, W.T.nbm, 0u};
    });
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
    if ((A.S.incl[i] & segscan::MASK) > A.S.lanes) st |= jpeg::ST_OVERRUN;  // (offsets the host forms refuse: lanes were cut off)
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
    A.S = split::bind(L.S, words, span, span_bytes, sub);
    A.offsets = offsets; A.coef = coef; A.status = words + L.status; A.dc = words + L.dc;
    uint32_t* tmp = words + L.tmp;
    const unsigned ni = (unsigned)J.n_intervals, nflags = (unsigned)L.S.rounds + 2;
    const size_t lds = split::stage_bytes(sub);
    (void)hipMemsetAsync(coef, 0, A.G.nblocks * 128, st);
    hipLaunchKernelGGL(jpeg_split_prep, dim3(((ni > nflags ? ni : nflags) + 255) / 256), dim3(256), 0, st, A, nflags);
    segscan::launch(st, A.S.incl, ni, tmp);
    for (uint32_t r = 0; r <= (uint32_t)L.S.rounds; ++r)
        hipLaunchKernelGGL(jpeg_split_round, dim3((unsigned)L.S.groups), dim3(split::GROUP), lds, st, A, r);
    segscan::launch(st, A.S.counts, L.S.lanes, tmp);
    hipLaunchKernelGGL(jpeg_split_write, dim3((unsigned)L.S.groups), dim3(split::GROUP), lds, st, A);
    const unsigned nb = (unsigned)((A.G.nblocks + 255) / 256);
    hipLaunchKernelGGL(jpeg_split_dc_gather, dim3(nb), dim3(256), 0, st, A);
    segscan::launch(st, A.dc, A.G.nblocks, tmp);
    hipLaunchKernelGGL(jpeg_split_dc_scatter, dim3(nb), dim3(256), 0, st, A);
    hipLaunchKernelGGL(jpeg_split_status, dim3((ni + 255) / 256), dim3(256), 0, st, A, status);
}

}  // namespace mi
