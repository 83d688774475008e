// kernels_ljpeg_split.hpp -- the second entropy path of the lossless-JPEG decoder: a segment (mi_ljpeg_seg_t: one or two
// components, every predictor, every precision) of ANY length, a file written as one strip included, decoded on many lanes at
// once and exactly.  ljpeg_sync_core.hpp has the transition, kernels_split_common.hpp the lanes, the bytes, the rounds and the
// frame of the write pass; the definition is tests/ljpeg_split_restatement.py, held bit for bit.  Tables, descriptors, layout,
// crop, linearisation table, shift and output are exactly raw_ljpeg's (kernels_ljpeg.hpp), and so is the result.  No reference
// counterpart.  The scaffold's units are the segments.
//
// Deliberately left for later: three-component streams (mi_ljpeg_seg3_t, raw_ljpeg3) stay on the serial kernel.
//
//   ljpeg_split_prep      per segment (one workgroup): its subsequence count (from the descriptor, clamped to the span), its
//                         status word, its tables in canonical form and their lookup over the next 10 bits in scratch --
//                         converters write different tables in every tile, so a lane reads its own segment's.  A descriptor
//                         the host forms refuse (ncomp outside 1 and 2, a bad predictor or precision, a width that is no
//                         multiple of ncomp, predictors 2 to 7 wider than MI_LJPEG_MAX_LINE) sets MI_LJPEG_UNDECODED: the
//                         segment keeps one lane that walks nothing, and NOTHING of it is written (as raw_ljpeg3 does).
//                         seg_scan then gives every segment its first lane.
//   ljpeg_split_round     the scaffold's rounds.  Two components: the state's table selection is the COMPONENT, and a lane
//                         keeps the scaffold's second exit, from the entry with the other component.
//   ljpeg_split_write     the scaffold's write pass: a lane's first sample is given by the segmented scan of the sample
//                         counts, and it writes the differences mod 2^16 of the samples below its segment's quota (rows x
//                         columns) into the difference plane, seg_h x seg_w uint16 per segment, zeroed beforehand.  A lane
//                         whose walk does not reproduce its stored exit sets MI_LJPEG_UNSYNCED.
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
// Segments out of file order, gaps and headers between small tiles put bytes outside a group's stage.  Every sample index is
// checked against the quota and every store against the crop (ljpeg_store, the one write path).  A corrupt stream costs status
// bits and nothing else.
#pragma once
#include "common.hpp"
#include "kernels_ljpeg.hpp"
#include "kernels_split_common.hpp"
#include "ljpeg_sync_core.hpp"

namespace mi {

namespace ljpeg {
constexpr int ROW_PER_LANE = 8, ROW_CHUNK = LANES * ROW_PER_LANE, ROWS_PER_BLOCK = 4;
constexpr int SPLIT_LUT = 2 << SYNC_LUT_BITS;   // lookup entries a segment
static_assert(SYNC_LUT_BITS == LUT_BITS, "one lookup width");

// the scratch, in words
struct SplitLayout {
    split::Layout S;
    size_t nseg, samples;
    size_t stat, tmp, huff, lut, plane, words;
};
inline SplitLayout split_layout(const mi_raw_layout_t& R, size_t span_bytes, uint32_t sub, uint32_t max_rounds) {
    SplitLayout L{};
    L.nseg = (size_t)unpack_nsegs(R);
    L.samples = L.nseg * (size_t)R.seg_height * (size_t)R.seg_width;
    split::Take take;
    L.S = split::layout(take, span_bytes, sub, max_rounds, L.nseg, true);
    L.stat = take(L.nseg);
    L.tmp = take(segscan::tmp_words(L.S.lanes > L.nseg ? L.S.lanes : L.nseg));
    L.huff = take((2 * L.nseg * sizeof(Huff) + 3) / 4);
    L.lut = take(L.nseg * SPLIT_LUT / 2);
    L.plane = take((L.samples + 1) / 2);
    L.words = take.at;
    return L;
}

// descriptors in host memory: the largest number of groups any one segment's lanes touch, minus 1 -- after r rounds the first
// r + 1 groups of a segment are exact, so this many rounds never leave a segment unsynced
inline uint32_t split_exact_rounds(const mi_ljpeg_seg_t* segs, size_t nseg, size_t span_bytes, uint32_t sub) {
    uint64_t at = 0, most = 1;
    for (size_t k = 0; k < nseg; ++k) {
        const uint64_t n = sync_nsub(sync_data_len(segs[k].scan_off, segs[k].scan_bytes, (uint32_t)span_bytes), sub);
        const uint64_t groups = (at + n - 1) / split::GROUP - at / split::GROUP + 1;
        most = groups > most ? groups : most;
        at += n;
    }
    return (uint32_t)(most - 1);
}

struct SplitArgs {
    LjpegArgs L;            // the span, the descriptors, the table, the output, the geometry: raw_ljpeg's
    split::Args S;          // the span again and the scaffold's arrays; counts are samples, `alts` the other component's exits
    uint32_t* stat;
    Huff* huff;             // per segment: two tables
    uint16_t* lut;          // per segment: SPLIT_LUT entries
    uint16_t* plane;        // the differences: seg_h * seg_w per segment
    uint32_t nseg;
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

// a lane's place and its segment's components
struct SplitLane : split::Lane {
    uint32_t nc;
};

// what the scaffold's bodies ask of a decoder (kernels_split_common.hpp)
struct SplitDecoder {
    static constexpr bool TWO = true;
    static constexpr uint32_t ENDED = 1u << 4, ALT_VALID = 1u << 5;
    using Lane = SplitLane;
    const SplitArgs& A;
    struct Walker {
        const Lane& P;
        const split::StagedBytes& src;
        const SyncTabs& T;
        uint32_t max_symbols;
        __device__ bool two() const { return P.nc == 2; }
        __device__ static uint2 other(uint2 e) { return make_uint2(e.x, e.y ^ 8u); }     // the same place, the other component
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
        Lane P{};
        SplitSeg G{};
        static_cast<split::Lane&>(P) = split::place_lane(A.S.incl, A.nseg, g, A.S.lanes, A.S.sub, [&](uint32_t k, uint32_t& o0, uint32_t& len) {
            G = split_seg(A, k);
            o0 = G.o0;
            len = G.len;
            return G.ok;
        });
        P.nc = (uint32_t)G.nc;
        return P;
    }
    __device__ void prepare() const {}      // (the tables are in scratch: ljpeg_split_prep)
    __device__ SyncTabs tabs_of(const Lane& P) const { return SyncTabs{A.huff + 2 * (size_t)P.k, A.lut + (size_t)P.k * SPLIT_LUT, P.nc}; }
};
}  // namespace ljpeg

// one workgroup per segment
__global__ __launch_bounds__(256) void ljpeg_split_prep(ljpeg::SplitArgs A, uint32_t n_flags) {
    using namespace ljpeg;
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    if (k == 0)
        for (uint32_t i = t; i < n_flags; i += 256) A.S.flags[i] = 0;
    const SplitSeg G = split_seg(A, k);
    const mi_ljpeg_seg_t& S = A.L.segs[k];
    Huff* h = A.huff + 2 * (size_t)k;
    if (t < 2) huff_build(h[t], S.counts[t], S.values[t]);
    if (t == 0) {
        A.S.incl[k] = sync_nsub(G.len, A.S.sub) | (k == 0 ? segscan::HEAD : 0u);
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
    extern __shared__ __align__(16) uint8_t stage[];
    split::round_body(ljpeg::SplitDecoder{A}, A.S, round, stage);
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
    extern __shared__ __align__(16) uint8_t stage[];
    split::write_body(ljpeg::SplitDecoder{A}, A.S, stage, A.stat, [&](const ljpeg::SplitDecoder::Walker& W, uint32_t first_sample) {
        // (rows <= seg_h: inside the segment's part of the plane)
        const uint32_t quota = (uint32_t)ljpeg::split_seg(A, W.P.k).rows * (uint32_t)A.L.seg_w;
        return LjpegSplitWriter{A.plane + (size_t)W.P.k * A.L.seg_h * A.L.seg_w, first_sample, quota, 0u};
    });
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
    if ((A.S.incl[k] & segscan::MASK) > A.S.lanes) st |= MI_LJPEG_UNDECODED;      // (descriptors that overlap: lanes were cut off)
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
    A.S = split::bind(L.S, words, span, span_bytes, sub);
    A.stat = words + L.stat; A.huff = (Huff*)(words + L.huff); A.lut = (uint16_t*)(words + L.lut);
    A.plane = plane_out ? plane_out : (uint16_t*)(words + L.plane);
    A.nseg = (uint32_t)L.nseg;
    uint32_t* tmp = words + L.tmp;
    const unsigned ns = (unsigned)L.nseg, nflags = (unsigned)L.S.rounds + 2;
    const size_t lds = split::stage_bytes(sub);
    (void)hipMemsetAsync(A.plane, 0, L.samples * sizeof(uint16_t), st);
    hipLaunchKernelGGL(ljpeg_split_prep, dim3(ns), dim3(256), 0, st, A, nflags);
    segscan::launch(st, A.S.incl, ns, tmp);
    for (uint32_t r = 0; r <= (uint32_t)L.S.rounds; ++r)
        hipLaunchKernelGGL(ljpeg_split_round, dim3((unsigned)L.S.groups), dim3(split::GROUP), lds, st, A, r);
    segscan::launch(st, A.S.counts, L.S.lanes, tmp);
    hipLaunchKernelGGL(ljpeg_split_write, dim3((unsigned)L.S.groups), dim3(split::GROUP), lds, st, A);
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
