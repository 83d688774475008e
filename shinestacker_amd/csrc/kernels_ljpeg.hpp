// kernels_ljpeg.hpp -- raw_ljpeg: the strips or tiles of a DNG with Compression 7, each one lossless-JPEG stream (ITU-T T.81,
// Huffman coded, SOF3), uploaded as they lie in the file, become the cropped H x W mosaic the rest of the raw path takes --
// what raw_unpack (kernels_unpack.hpp) does for uncompressed samples.  No reference counterpart; tests/ljpeg_restatement.py is
// the definition, held bit for bit.
//
//   per segment (mi_ljpeg_seg_t, read from the stream's headers on the host): lines top to bottom, x = 0 .. X-1 within a line,
//   components c = 0 .. Nf-1 within x; the sample lands at segment row r, column x * Nf + c.  Its category s comes from the
//   component's Huffman table, the difference from the s bits behind it (ljpeg_core.hpp); prediction is per component with Ra
//   the sample Nf columns to the left, Rb the one above and Rc above-left: 2^(P-1) for the first sample, Ra on the rest of the
//   first line, Rb for the first sample of every other line, the scan's predictor (1 Ra, 2 Rb, 3 Rc, 4 Ra + Rb - Rc,
//   5 Ra + ((Rb - Rc) >> 1), 6 Rb + ((Ra - Rc) >> 1), 7 (Ra + Rb) >> 1) everywhere else; value = (prediction + difference)
//   mod 2^16.  Then as raw_unpack: v = table[min(v, len - 1)] with a table, out = (v << shift) truncated to the dtype, written
//   at (ys - crop_y, xs - crop_x) when the stored site lies inside the crop.  Samples of an edge tile outside the image are
//   decoded -- later ones depend on them -- and not written.
//
// Why on the device: the compressed bytes are the smallest form of the frame that can cross the host link, the link the raw
// path is bound by, and a host decoder would put a serial bit loop of several hundred milliseconds per 50 MP frame in front of
// a device pipeline that spends about 12 ms on it.
//
// Mapping: one segment per wavefront (a workgroup of 64).  The symbol walk of a segment is serial -- where a code ends is only
// known once it is decoded -- and the wave around it is not:
//   tables    lanes 0 and 1 put the components' tables into canonical form in LDS, then the 64 lanes expand them into a
//             lookup over the next ljpeg::LUT_BITS = 10 bits (length and category; longer codes take the canonical search of
//             ljpeg_core.hpp).  Per segment: converters write different tables in every tile.
//   staging   the segment's bytes go from HBM into a ring of ljpeg::RING bytes of LDS in chunks of 256 (64 aligned dwords, one
//             coalesced load per lane).  Before every batch the wave tops the ring up: a constant ljpeg::RING / ljpeg::CHUNK
//             predicated steps, after which more than RING - CHUNK bytes lie in front of the walker, or the data's end does.
//   walk      lane 0 decodes a batch of up to ljpeg::BATCH = 256 differences of one line out of the ring into LDS.  A sample
//             takes at most 4 bytes of bits, 8 ring bytes when every one is a stuffed FF 00: a batch cannot outrun the ring.
//             The walker removes the stuffing itself as it refills its 64-bit window (one compare per byte, no trip that the
//             stream decides): a ballot-and-prefix-count pass by the wave was weighed and left out -- what a chunk yields
//             would then depend on its content, and the ring's guarantee with it.  What that costs the walk was not
//             measured (see Measured below).
//   predict   predictor 1 and the first line are a per-component prefix sum mod 2^16 by the wave (four samples per lane, a
//             shuffle scan of the lanes' totals, the carry from batch to batch); predictor 2 is one add per sample against the
//             line above, kept in LDS; predictors 3 to 7 depend on the sample to the left AND the line above and stay with the
//             walking lane, against the same line in LDS.
//   write     the wave applies table, shift and crop and writes the batch, consecutive lanes to consecutive samples.
// The line above takes 2 bytes a column of LDS: predictors 2 to 7 are decoded on segments of up to ljpeg::MAX_LINE = 24576
// columns (58 KB of LDS at that width); a wider segment is decoded with predictor 1 alone, which keeps no line, and refused
// by dng.read and the C boundary otherwise (status bit 2 where the descriptors are only on the device).  This is LESS than
// was asked for: the plain fallback for segments wider than the LDS budget exists for predictor 1 only.  A serial path that
// keeps the line above in a scratch buffer in HBM would serve predictors 2 to 7 there and is not built; no sensor is 24 576
// samples wide, so the refusal costs no file known today.
//
// Bounded by construction: every loop's trip count comes from the launch (rows, columns, the batch, the ring) and none from
// the stream.  Every read of the span goes through ljpeg_dword / ljpeg_byte, which return 0 at or beyond span_bytes; the
// walker's byte source returns 0 at or beyond the segment's data; every write goes through ljpeg_store, which checks the site
// against the crop.  A corrupt stream costs a status bit and nothing else.
//
// Measured (docs/studies.md, DNG files; tools/ljpeg_time.py, a smooth scene with sensor-like noise, beside raw_unpack and a
// device copy of the output in the same run): 50.3 MP of 12-bit samples in 256 x 256 tiles of two components, predictor 1, in
// 33.1 ms (14 bits: 37.0 ms), 24 MP in 27.9 ms; in strips of 64 rows 212 ms and 147 ms.  raw_unpack of the same samples takes
// 0.039 ms, the copy 0.026 ms, the upload of the compressed span (0.49 of the uint16 mosaic) 0.86 ms.  The walk is the bound,
// and by a wide margin: the time is that of ONE segment's walk -- 782 tiles at 50 MP or 376 at 24 MP are all resident at once
// and take nearly the same time -- at about 0.45 us a sample on the one walking lane (65 536 samples a tile, 556 032 a strip),
// some 1000 cycles a sample.  Where inside the walk those cycles go was NOT measured (no counters, no variant was run): the
// candidates are the dependent LDS byte reads of the refill (two per source byte, the second for the stuffing test), the
// lookup and the difference arithmetic, all under a one-lane mask.  That the wave's part -- staging, prediction, stores -- is
// small is arithmetic, not measurement: a few thousand wave instructions a tile against 65 536 serial walks.  The decode is 38
// times the span's upload: a stack of compressed frames is bound by the decode, not by the link.  Decode INSIDE a segment
// (self-synchronising sub-sequences: many lanes start at guessed bit positions and converge on the true symbol boundaries) is
// kernels_ljpeg_split.hpp, an option beside this kernel for segments of one and two components: measured there, 50 MP in
// tiles 33.2 -> 16.1 ms, in strips of 64 rows 212 -> 54.0 ms, as one strip 18.9 s -> 0.26 s (docs/studies.md).  Three-component
// streams (raw_ljpeg3 below) stay on this walker: the step deliberately left for later.  A leaner walker (dword reads of the
// ring, the stuffing removed by the wave after all, a wider lookup that also yields short differences) is still not built;
// whether it pays is for a counter run to say.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "kernels_unpack.hpp"
#include "ljpeg_core.hpp"

namespace mi {

namespace ljpeg {
constexpr int LANES = 64;
constexpr int RING = 4096;                 // bytes of the staging ring (a power of two)
constexpr int CHUNK = LANES * 4;           // bytes staged per step
constexpr int BATCH = 256;                 // samples the walker decodes between two top-ups (even; at most 8 * BATCH + 16 < RING - CHUNK ring bytes)
constexpr int PER_LANE = BATCH / LANES;    // samples of a batch per lane
constexpr int LUT_BITS = 10;
constexpr int LUT_BYTES = 2 * (1 << LUT_BITS) * 2;
constexpr int HUFF_STRIDE = 160;           // >= sizeof(Huff), a multiple of 16
constexpr int MAX_LINE = MI_LJPEG_MAX_LINE;
constexpr int LDS_FIXED = RING + LUT_BYTES + 2 * HUFF_STRIDE + BATCH * 2;
static_assert(sizeof(Huff) <= HUFF_STRIDE && LDS_FIXED % 16 == 0 && PER_LANE == 4, "LDS carve");
static_assert(8 * BATCH + 16 < RING - CHUNK, "a batch must not outrun the ring");
static_assert(LDS_FIXED + 2 * MAX_LINE <= 65536, "LDS budget");

// the walker's byte source: the ring in LDS, addressed by the byte's offset in the span
struct RingBytes {
    const uint8_t* ring;
    uint32_t scan_off, lim;
    __host__ __device__ uint32_t limit() const { return lim; }
    __host__ __device__ uint32_t byte(uint32_t i) const { return i < lim ? (uint32_t)ring[(scan_off + i) & (RING - 1)] : 0u; }
};
}  // namespace ljpeg

struct LjpegArgs {
    const uint8_t* span;
    const mi_ljpeg_seg_t* segs;
    const uint16_t* table;      // or null
    void* out;                  // h x w
    uint32_t* status;           // one word per segment, or null
    uint32_t* status_or;        // one word all segments OR their flags into, or null
    uint32_t span_bytes;
    int h, w;                   // the output
    int crop_y, crop_x;
    int image_h;
    int seg_h, seg_w, nsx, tiled;
    int shift, table_len;
};

// the byte at `off`, 0 beyond the span
__device__ __forceinline__ uint32_t ljpeg_byte(const LjpegArgs& A, uint64_t off) {
    return off < A.span_bytes ? (uint32_t)A.span[off] : 0u;
}
// the aligned dword at `off` (off % 4 == 0) in memory order
__device__ __forceinline__ uint32_t ljpeg_dword(const LjpegArgs& A, uint64_t off) {
    if (off + 4 <= A.span_bytes) return *(const uint32_t*)(A.span + off);
    return ljpeg_byte(A, off) | ljpeg_byte(A, off + 1) << 8 | ljpeg_byte(A, off + 2) << 16 | ljpeg_byte(A, off + 3) << 24;
}
// the one write path: the sample of the stored site (ys, xs), when it lies inside the crop
template <typename T>
__device__ __forceinline__ void ljpeg_store(const LjpegArgs& A, int ys, int xs, uint32_t v) {
    const int y = ys - A.crop_y, x = xs - A.crop_x;
    if ((unsigned)y >= (unsigned)A.h || (unsigned)x >= (unsigned)A.w) return;
    if (A.table) v = A.table[min(v, (uint32_t)(A.table_len - 1))];
    ((T*)A.out)[(size_t)y * A.w + x] = (T)(v << A.shift);
}

template <typename T>
__global__ __launch_bounds__(64) void raw_ljpeg(LjpegArgs A) {
    using namespace ljpeg;
    extern __shared__ __attribute__((aligned(16))) unsigned char ljpeg_smem[];
    uint32_t* ring = (uint32_t*)ljpeg_smem;
    uint16_t* lut = (uint16_t*)(ljpeg_smem + RING);
    unsigned char* const huffs = ljpeg_smem + RING + LUT_BYTES;                  // two Huff, HUFF_STRIDE apart
    const auto huff = [huffs](int c) -> Huff& { return *(Huff*)(huffs + c * HUFF_STRIDE); };
    uint16_t* d = (uint16_t*)(ljpeg_smem + RING + LUT_BYTES + 2 * HUFF_STRIDE);       // a batch: differences, then values
    uint16_t* line = d + BATCH;                                                 // the line above (seg_w <= MAX_LINE)
    const int lane = (int)threadIdx.x, k = (int)blockIdx.x;
    const int sy = k / A.nsx, sx = k - sy * A.nsx;
    const int rows = A.tiled ? A.seg_h : min(A.seg_h, A.image_h - sy * A.seg_h);
    const int W = A.seg_w;
    const mi_ljpeg_seg_t& S = A.segs[k];
    uint32_t status = 0;
    int nc = S.ncomp, pred = S.predictor, prec = S.precision;
    if ((nc != 1 && nc != 2) || W % nc || pred < 1 || pred > 7 || prec < 2 || prec > 16 || (pred != 1 && W > MAX_LINE)) {
        status = MI_LJPEG_UNDECODED;   // (the host forms refuse it: decode something bounded, write it inside the output)
        nc = 1; pred = 1; prec = 16;
    }
    // tables
    if (lane < nc) huff_build(huff(lane), S.counts[lane], S.values[lane]);
    __syncthreads();
    for (int j = lane; j < nc << LUT_BITS; j += LANES) {
        int len;
        const int s = huff_decode(huff(j >> LUT_BITS), (uint32_t)(j & ((1 << LUT_BITS) - 1)) << (16 - LUT_BITS), len);
        lut[j] = s >= 0 && s <= 16 && len <= LUT_BITS ? (uint16_t)(len << 8 | s) : (uint16_t)0;
    }
    // the data: [scan_off, data_end) of the span
    const uint32_t scan_off = S.scan_off;
    const uint32_t lim = scan_off < A.span_bytes ? min(S.scan_bytes, A.span_bytes - scan_off) : 0u;
    const uint32_t data_end = scan_off + lim;
    uint32_t staged = scan_off & ~3u;          // the ring holds [.., staged) of the span
    BitReader<RingBytes> rd(RingBytes{(const uint8_t*)ring, scan_off, lim});
    uint32_t seed[2] = {1u << (prec - 1), 1u << (prec - 1)};    // what predicts a line's first sample, per component
    uint32_t carry[2] = {0, 0};                                  // Ra at the start of a batch (the prefix sum's)
    uint32_t ra[2] = {0, 0}, rc[2] = {0, 0};                     // the walker's, predictors 3 to 7
    const int nb = (W + BATCH - 1) / BATCH;
    for (int r = 0; r < rows; ++r) {
        const bool scan = pred == 1 || r == 0, serial = !scan && pred >= 3;
        for (int b = 0; b < nb; ++b) {
            const int c0 = b * BATCH, n = min(BATCH, W - c0);
            // top the ring up
            const uint32_t rpos = (scan_off + (uint32_t)__shfl((int)rd.pos, 0)) & ~3u;
            for (int t = 0; t < RING / CHUNK; ++t)
                if (staged < data_end && staged - rpos <= (uint32_t)(RING - CHUNK)) {
                    ring[((staged >> 2) + lane) & (RING / 4 - 1)] = ljpeg_dword(A, (uint64_t)staged + 4 * lane);
                    staged += CHUNK;
                }
            __syncthreads();
            // the walk
            if (lane == 0) {
                if (r == 0 && b == 0) rd.template fill<8>();
                for (int i = 0; i < n; ++i) {
                    const int c = nc == 2 ? i & 1 : 0;
                    rd.template fill<4>();
                    const uint32_t e = lut[(c << LUT_BITS) + (rd.peek16() >> (16 - LUT_BITS))];
                    uint32_t v;
                    if (e) {
                        rd.skip((int)(e >> 8));
                        v = take_difference(rd, (int)(e & 0xff));
                    } else {
                        v = decode_difference(rd, huff(c), status);
                    }
                    if (serial) {
                        const int col = c0 + i;
                        const int Rb = line[col], Ra = (int)(c ? ra[1] : ra[0]), Rc = (int)(c ? rc[1] : rc[0]);
                        int px;
                        if (col < nc) px = Rb;
                        else if (pred == 3) px = Rc;
                        else if (pred == 4) px = Ra + Rb - Rc;
                        else if (pred == 5) px = Ra + ((Rb - Rc) >> 1);
                        else if (pred == 6) px = Rb + ((Ra - Rc) >> 1);
                        else px = (Ra + Rb) >> 1;
                        v = ((uint32_t)px + v) & 0xffffu;
                        line[col] = (uint16_t)v;
                        if (c) { ra[1] = v; rc[1] = (uint32_t)Rb; } else { ra[0] = v; rc[0] = (uint32_t)Rb; }
                    }
                    d[i] = (uint16_t)v;
                }
            }
            __syncthreads();
            // differences -> values
            if (scan) {
                if (b == 0) { carry[0] = seed[0]; carry[1] = seed[1]; }
                const int i0 = lane * PER_LANE;
                uint32_t p[PER_LANE];
#pragma unroll
                for (int j = 0; j < PER_LANE; ++j) p[j] = i0 + j < n ? (uint32_t)d[i0 + j] : 0u;
                uint32_t t0, t1;
                if (nc == 1) { p[1] += p[0]; p[2] += p[1]; p[3] += p[2]; t0 = p[3]; t1 = 0; }
                else { p[2] += p[0]; p[3] += p[1]; t0 = p[2]; t1 = p[3]; }
                uint32_t x0 = t0, x1 = t1;             // inclusive scan of the lanes' totals
#pragma unroll
                for (int o = 1; o < LANES; o <<= 1) {
                    const uint32_t y0 = (uint32_t)__shfl_up((int)x0, o), y1 = (uint32_t)__shfl_up((int)x1, o);
                    if (lane >= o) { x0 += y0; x1 += y1; }
                }
                x0 += carry[0] - t0;                    // exclusive, plus the carry
                x1 += carry[1] - t1;
#pragma unroll
                for (int j = 0; j < PER_LANE; ++j)
                    if (i0 + j < n) {
                        const uint32_t v = (p[j] + (nc == 2 && (j & 1) ? x1 : x0)) & 0xffffu;
                        d[i0 + j] = (uint16_t)v;
                        if (pred != 1) line[c0 + i0 + j] = (uint16_t)v;
                    }
                __syncthreads();
                carry[0] = d[n - nc];
                carry[1] = d[n - 1];
                if (b == 0) { seed[0] = d[0]; seed[1] = d[nc - 1]; }
            } else if (pred == 2) {
                for (int i = lane; i < n; i += LANES) {
                    const uint32_t v = ((uint32_t)line[c0 + i] + d[i]) & 0xffffu;
                    d[i] = (uint16_t)v;
                    line[c0 + i] = (uint16_t)v;
                }
                __syncthreads();
            }
            // table, shift, crop, store
            const int ys = sy * A.seg_h + r, xs0 = sx * W + c0;
            for (int i = lane; i < n; i += LANES) ljpeg_store<T>(A, ys, xs0 + i, d[i]);
        }
    }
    if (lane == 0) {
        if (rd.overrun()) status |= ST_OVERRUN;
        if (A.status) A.status[k] = status;
        if (A.status_or && status) atomicOr(A.status_or, status);
    }
}

// arguments checked by the caller (capi.hip: raw_layout_check, ljpeg_segs_check)
inline void ljpeg_launch(hipStream_t st, const void* span, size_t span_bytes, const mi_ljpeg_seg_t* segs, const mi_raw_layout_t& L,
                         const uint16_t* table, void* out, uint32_t* status, uint32_t* status_or) {
    using namespace ljpeg;
    LjpegArgs A{};
    A.span = (const uint8_t*)span; A.segs = segs; A.table = L.table_len > 0 ? table : nullptr; A.out = out;
    A.status = status; A.status_or = status_or;
    A.span_bytes = (uint32_t)span_bytes;
    A.h = L.height; A.w = L.width; A.crop_y = L.crop_y; A.crop_x = L.crop_x; A.image_h = L.image_height;
    A.seg_h = L.seg_height; A.seg_w = L.seg_width; A.nsx = unpack_nsx(L); A.tiled = L.tiled;
    A.shift = L.shift; A.table_len = L.table_len;
    const size_t lds = LDS_FIXED + (L.seg_width <= MAX_LINE ? 2 * (size_t)((L.seg_width + 7) & ~7) : 0);
    const dim3 grid((unsigned)unpack_nsegs(L)), blk(LANES);
    if (L.dtype == MI_U8) hipLaunchKernelGGL(raw_ljpeg<uint8_t>, grid, blk, lds, st, A);
    else hipLaunchKernelGGL(raw_ljpeg<uint16_t>, grid, blk, lds, st, A);
}

// ---------------------------------------------------------------- three components: the tiles of a LinearRaw frame
// raw_ljpeg3 is raw_ljpeg's sibling for streams of Nf = 3 (mi_ljpeg_seg3_t: R, G, B interleaved along the line; the layout
// counts samples, seg_w = 3 X).  Everything above holds -- one segment per wavefront, the tables and the walker of
// ljpeg_core.hpp unchanged, the same ring, top-up and guarantee, the same status bits, every loop bound from the launch -- and
// one thing differs: the batch is ljpeg::BATCH3 = 192 samples, 64 whole pixels, one pixel per lane, so the per-component prefix
// scan keeps its phase from batch to batch (a batch of 256 would start every third batch on another component).  A
// descriptor the host forms refuse (ncomp other than 3, a width that is no multiple of 3, ...) sets MI_LJPEG_UNDECODED and
// the segment is left unwritten: nothing is decoded from it.
namespace ljpeg {
constexpr int NC3 = 3;
constexpr int BATCH3 = NC3 * LANES;        // one pixel per lane
constexpr int LUT3_BYTES = NC3 * (1 << LUT_BITS) * 2;
constexpr int LDS3_FIXED = RING + LUT3_BYTES + NC3 * HUFF_STRIDE + BATCH3 * 2;
static_assert(LDS3_FIXED % 16 == 0, "LDS carve");
static_assert(8 * BATCH3 + 16 < RING - CHUNK, "a batch must not outrun the ring");
static_assert(LDS3_FIXED + 2 * MAX_LINE <= 65536, "LDS budget");
}  // namespace ljpeg

struct Ljpeg3Args : LjpegArgs {
    const mi_ljpeg_seg3_t* segs3;   // (`segs` of the base is not read)
};

template <typename T>
__global__ __launch_bounds__(64) void raw_ljpeg3(Ljpeg3Args A) {
    using namespace ljpeg;
    extern __shared__ __attribute__((aligned(16))) unsigned char ljpeg_smem[];
    uint32_t* ring = (uint32_t*)ljpeg_smem;
    uint16_t* lut = (uint16_t*)(ljpeg_smem + RING);
    unsigned char* const huffs = ljpeg_smem + RING + LUT3_BYTES;                  // three Huff, HUFF_STRIDE apart
    const auto huff = [huffs](int c) -> Huff& { return *(Huff*)(huffs + c * HUFF_STRIDE); };
    uint16_t* d = (uint16_t*)(ljpeg_smem + RING + LUT3_BYTES + NC3 * HUFF_STRIDE);      // a batch: differences, then values
    uint16_t* line = d + BATCH3;                                                  // the line above (seg_w <= MAX_LINE)
    const int lane = (int)threadIdx.x, k = (int)blockIdx.x;
    const int sy = k / A.nsx, sx = k - sy * A.nsx;
    const int rows = A.tiled ? A.seg_h : min(A.seg_h, A.image_h - sy * A.seg_h);
    const int W = A.seg_w;
    const mi_ljpeg_seg3_t& S = A.segs3[k];
    uint32_t status = 0;
    const int pred = S.predictor, prec = S.precision;
    if (S.ncomp != NC3 || W % NC3 || pred < 1 || pred > 7 || prec < 2 || prec > 16 || (pred != 1 && W > MAX_LINE)) {
        if (lane == 0) {            // (the host forms refuse it; uniform over the wave: no barrier is skipped by a part of it)
            if (A.status) A.status[k] = MI_LJPEG_UNDECODED;
            if (A.status_or) atomicOr(A.status_or, MI_LJPEG_UNDECODED);
        }
        return;
    }
    // tables
    if (lane < NC3) huff_build(huff(lane), S.counts[lane], S.values[lane]);
    __syncthreads();
    for (int j = lane; j < NC3 << LUT_BITS; j += LANES) {
        int len;
        const int s = huff_decode(huff(j >> LUT_BITS), (uint32_t)(j & ((1 << LUT_BITS) - 1)) << (16 - LUT_BITS), len);
        lut[j] = s >= 0 && s <= 16 && len <= LUT_BITS ? (uint16_t)(len << 8 | s) : (uint16_t)0;
    }
    // the data: [scan_off, data_end) of the span
    const uint32_t scan_off = S.scan_off;
    const uint32_t lim = scan_off < A.span_bytes ? min(S.scan_bytes, A.span_bytes - scan_off) : 0u;
    const uint32_t data_end = scan_off + lim;
    uint32_t staged = scan_off & ~3u;          // the ring holds [.., staged) of the span
    BitReader<RingBytes> rd(RingBytes{(const uint8_t*)ring, scan_off, lim});
    const uint32_t half = 1u << (prec - 1);
    uint32_t seed[NC3] = {half, half, half};    // what predicts a line's first pixel, per component
    uint32_t carry[NC3] = {0, 0, 0};            // Ra at the start of a batch (the prefix sum's)
    uint32_t ra[NC3] = {0, 0, 0}, rc[NC3] = {0, 0, 0};     // the walker's, predictors 3 to 7
    const int nb = (W + BATCH3 - 1) / BATCH3;
    for (int r = 0; r < rows; ++r) {
        const bool scan = pred == 1 || r == 0, serial = !scan && pred >= 3;
        for (int b = 0; b < nb; ++b) {
            const int c0 = b * BATCH3, n = min(BATCH3, W - c0);      // (W % 3 == 0: n is a whole number of pixels)
            // top the ring up
            const uint32_t rpos = (scan_off + (uint32_t)__shfl((int)rd.pos, 0)) & ~3u;
            for (int t = 0; t < RING / CHUNK; ++t)
                if (staged < data_end && staged - rpos <= (uint32_t)(RING - CHUNK)) {
                    ring[((staged >> 2) + lane) & (RING / 4 - 1)] = ljpeg_dword(A, (uint64_t)staged + 4 * lane);
                    staged += CHUNK;
                }
            __syncthreads();
            // the walk
            if (lane == 0) {
                if (r == 0 && b == 0) rd.template fill<8>();
                int c = 0;
                for (int i = 0; i < n; ++i) {
                    rd.template fill<4>();
                    const uint32_t e = lut[(c << LUT_BITS) + (rd.peek16() >> (16 - LUT_BITS))];
                    uint32_t v;
                    if (e) {
                        rd.skip((int)(e >> 8));
                        v = take_difference(rd, (int)(e & 0xff));
                    } else {
                        v = decode_difference(rd, huff(c), status);
                    }
                    if (serial) {
                        const int col = c0 + i;
                        const int Rb = line[col], Ra = (int)ra[c], Rc = (int)rc[c];
                        int px;
                        if (col < NC3) px = Rb;
                        else if (pred == 3) px = Rc;
                        else if (pred == 4) px = Ra + Rb - Rc;
                        else if (pred == 5) px = Ra + ((Rb - Rc) >> 1);
                        else if (pred == 6) px = Rb + ((Ra - Rc) >> 1);
                        else px = (Ra + Rb) >> 1;
                        v = ((uint32_t)px + v) & 0xffffu;
                        line[col] = (uint16_t)v;
                        ra[c] = v;
                        rc[c] = (uint32_t)Rb;
                    }
                    d[i] = (uint16_t)v;
                    c = c == NC3 - 1 ? 0 : c + 1;
                }
            }
            __syncthreads();
            // differences -> values
            if (scan) {
                if (b == 0) { carry[0] = seed[0]; carry[1] = seed[1]; carry[2] = seed[2]; }
                const int i0 = lane * NC3;
                const bool on = i0 < n;                 // this lane's pixel lies in the batch
                uint32_t x[NC3];
#pragma unroll
                for (int c = 0; c < NC3; ++c) x[c] = on ? (uint32_t)d[i0 + c] : 0u;
#pragma unroll
                for (int o = 1; o < LANES; o <<= 1) {   // inclusive scan over the lanes, per component
#pragma unroll
                    for (int c = 0; c < NC3; ++c) {
                        const uint32_t y = (uint32_t)__shfl_up((int)x[c], o);
                        if (lane >= o) x[c] += y;
                    }
                }
                if (on) {
#pragma unroll
                    for (int c = 0; c < NC3; ++c) {
                        const uint32_t v = (x[c] + carry[c]) & 0xffffu;
                        d[i0 + c] = (uint16_t)v;
                        if (pred != 1) line[c0 + i0 + c] = (uint16_t)v;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int c = 0; c < NC3; ++c) {
                    carry[c] = d[n - NC3 + c];
                    if (b == 0) seed[c] = d[c];
                }
            } else if (pred == 2) {
                for (int i = lane; i < n; i += LANES) {
                    const uint32_t v = ((uint32_t)line[c0 + i] + d[i]) & 0xffffu;
                    d[i] = (uint16_t)v;
                    line[c0 + i] = (uint16_t)v;
                }
                __syncthreads();
            }
            // table, shift, crop, store
            const int ys = sy * A.seg_h + r, xs0 = sx * W + c0;
            for (int i = lane; i < n; i += LANES) ljpeg_store<T>(A, ys, xs0 + i, d[i]);
        }
    }
    if (lane == 0) {
        if (rd.overrun()) status |= ST_OVERRUN;
        if (A.status) A.status[k] = status;
        if (A.status_or && status) atomicOr(A.status_or, status);
    }
}

// arguments checked by the caller (capi.hip: raw_layout_check, ljpeg3_segs_check)
inline void ljpeg3_launch(hipStream_t st, const void* span, size_t span_bytes, const mi_ljpeg_seg3_t* segs, const mi_raw_layout_t& L,
                          const uint16_t* table, void* out, uint32_t* status, uint32_t* status_or) {
    using namespace ljpeg;
    Ljpeg3Args A{};
    A.span = (const uint8_t*)span; A.segs = nullptr; A.segs3 = segs; A.table = L.table_len > 0 ? table : nullptr; A.out = out;
    A.status = status; A.status_or = status_or;
    A.span_bytes = (uint32_t)span_bytes;
    A.h = L.height; A.w = L.width; A.crop_y = L.crop_y; A.crop_x = L.crop_x; A.image_h = L.image_height;
    A.seg_h = L.seg_height; A.seg_w = L.seg_width; A.nsx = unpack_nsx(L); A.tiled = L.tiled;
    A.shift = L.shift; A.table_len = L.table_len;
    const size_t lds = LDS3_FIXED + (L.seg_width <= MAX_LINE ? 2 * (size_t)((L.seg_width + 7) & ~7) : 0);
    const dim3 grid((unsigned)unpack_nsegs(L)), blk(LANES);
    if (L.dtype == MI_U8) hipLaunchKernelGGL(raw_ljpeg3<uint8_t>, grid, blk, lds, st, A);
    else hipLaunchKernelGGL(raw_ljpeg3<uint16_t>, grid, blk, lds, st, A);
}

}  // namespace mi
