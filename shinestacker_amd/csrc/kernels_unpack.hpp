// kernels_unpack.hpp -- raw_unpack: the sample bytes of a raw file (DNG: strips or tiles of 8, 10, 12, 14 or 16-bit samples),
// uploaded as they lie in the file, become the cropped H x W mosaic the rest of the raw path takes.  No reference counterpart;
// tests/unpack_restatement.py is the definition, held bit for bit.
//
//   stored site (ys, xs) = (y + crop_y, x + crop_x);  segment k = (ys / seg_h) * nsx + xs / seg_w, nsx = ceil(image_w / seg_w);
//   inside it row ry = ys % seg_h, column xt = xs % seg_w;  a row takes row_bytes = ceil(seg_w * bits / 8) bytes and starts on a
//   byte boundary; the sample is the `bits` bits from bit xt * bits of the row, most significant first (16 bits: two bytes in
//   the file's order, 8 bits: the byte).  v = table[min(v, len - 1)] with a table; out = (v << shift) truncated to the dtype.
//
// Why on the device: a 12-bit mosaic is 1.5 bytes per site in the file and 2 once unpacked, so uploading the file's bytes
// takes a quarter off what crosses the host link -- the link the mosaic push is bound by -- and the host never shuffles bits.
//
// Mapping.  A workgroup of 256 is unpack::TILE_H = 4 rows of 64 lanes; a lane owns one 16-byte window of its OUTPUT row (8
// uint16 or 16 uint8 samples) and writes it with one 16-byte store.  As in mosaic_calibrate the windows are aligned in memory,
// not in x: a row that does not start on a 16-byte boundary has a partial first window and every row may have a partial last
// one.  The window's samples are V * bits contiguous bits of one segment row -- 10 to 16 bytes -- that start at ANY byte (file
// offsets are arbitrary) and, with a crop origin that is no multiple of 8, at any bit.  One unaligned 16-byte load would not
// do: behind a bit offset the window takes 17 bytes, and a load must not reach past the span's end; 17 byte loads per lane
// would be 17 requests.  The lane reads the four or five ALIGNED dwords that cover its bits (neighbouring lanes share the edge
// dwords, which the cache serves), byte-swaps them into stream order and funnel-shifts
// them by its bit offset (0 .. 31) into four dwords, from which every sample comes out at a compile-time position.  A dword
// that would reach past the end of the span is put together from the bytes that exist.  Partial windows, and windows that
// cross a tile's right edge, go sample by sample (three byte loads each).  No byte at or beyond span_bytes is ever read.
// Measured (docs/studies.md, DNG files; beside a device copy of the output's bytes in the same run): 50 MP in 0.039 to 0.044 ms
// for 10 to 16 bits, strips and tiles alike, 1.55 to 1.8 times the copy's 0.025 ms; from a crop origin of (13, 7) strips take
// 0.044 to 0.049 ms and 256 x 256 tiles 0.081 to 0.100 ms -- every wave then holds windows that cross a tile's edge and waits
// for their byte loads.  A two-segment fast path for those windows is not built.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace mi {

namespace unpack {
constexpr int VEC_BYTES = 16;              // one lane's window of an output row
constexpr int NT = 256;
constexpr int LANES = 64;                  // windows of one row per workgroup
constexpr int TILE_H = NT / LANES;         // rows per workgroup
constexpr int MAX_TABLE = 65536;
}  // namespace unpack

struct UnpackArgs {
    const uint8_t* span;
    const uint32_t* seg;        // segment offsets into span
    const uint16_t* table;      // or null
    void* out;                  // h x w
    uint32_t span_bytes;
    int h, w;                   // the output
    int crop_y, crop_x;
    int seg_h, seg_w, nsx;
    uint32_t row_bytes;         // of a segment row
    int shift, table_len;
    int swap16;                 // 16 bits: the file is little-endian (the stream below is read big-endian)
    int nbx;                    // workgroups along a row
};

// the byte at `off`, 0 beyond the span
__device__ __forceinline__ uint32_t unpack_byte(const UnpackArgs& A, uint64_t off) {
    return off < A.span_bytes ? (uint32_t)A.span[off] : 0u;
}

// the aligned dword at `off` (off % 4 == 0) in STREAM order: its first byte in the top bits
__device__ __forceinline__ uint32_t unpack_dword(const UnpackArgs& A, uint64_t off) {
    if (off + 4 <= A.span_bytes) return __builtin_bswap32(*(const uint32_t*)(A.span + off));
    return unpack_byte(A, off) << 24 | unpack_byte(A, off + 1) << 16 | unpack_byte(A, off + 2) << 8 | unpack_byte(A, off + 3);
}

template <int BITS>
__device__ __forceinline__ uint32_t unpack_finish(const UnpackArgs& A, uint32_t v) {
    if constexpr (BITS == 16) {
        if (A.swap16) v = (v >> 8 | v << 8) & 0xffffu;
    }
    if (A.table) v = A.table[min(v, (uint32_t)(A.table_len - 1))];
    v <<= A.shift;
    return BITS == 8 ? v & 0xffu : v & 0xffffu;
}

// the byte offset in the span of row `ry` of the segment in segment row `sy`, segment column `sx`
__device__ __forceinline__ uint64_t unpack_row(const UnpackArgs& A, int sy, int ry, int sx) {
    return (uint64_t)A.seg[sy * A.nsx + sx] + (uint64_t)ry * A.row_bytes;
}

// one sample, byte by byte: column xt of the segment row that starts at byte `row`
template <int BITS>
__device__ __forceinline__ uint32_t unpack_one(const UnpackArgs& A, uint64_t row, int xt) {
    const uint64_t bit = (uint64_t)xt * BITS;
    const uint64_t b = row + (bit >> 3);
    const int sh = (int)(bit & 7);
    const uint32_t w = unpack_byte(A, b) << 16 | unpack_byte(A, b + 1) << 8 | unpack_byte(A, b + 2);   // 24 bits >= 7 + 16
    return unpack_finish<BITS>(A, (w >> (24 - sh - BITS)) & ((1u << BITS) - 1u));
}

template <int BITS>
__global__ __launch_bounds__(256) void raw_unpack(UnpackArgs A) {
    using namespace unpack;
    using T = std::conditional_t<BITS == 8, uint8_t, uint16_t>;
    constexpr int V = VEC_BYTES / (int)sizeof(T);       // samples of a window
    const int by = (int)blockIdx.x / A.nbx, bx = (int)blockIdx.x - by * A.nbx;
    const int y = by * TILE_H + (int)threadIdx.x / LANES;
    if (y >= A.h) return;
    T* row = (T*)A.out + (size_t)y * A.w;
    const int off = (int)(((uintptr_t)row & (VEC_BYTES - 1)) / sizeof(T));   // the row starts `off` samples into its first window
    const int x0 = (bx * LANES + ((int)threadIdx.x & (LANES - 1))) * V - off;
    if (x0 >= A.w) return;
    const int ys = y + A.crop_y;
    const int sy = ys / A.seg_h, ry = ys - sy * A.seg_h;
    const int i0 = x0 < 0 ? -x0 : 0, i1 = min(V, A.w - x0);      // the window's samples inside the row: [i0, i1)
    const int xs0 = x0 + i0 + A.crop_x;
    int sx = xs0 / A.seg_w, xt = xs0 - sx * A.seg_w;
    if (i0 > 0 || i1 < V || xt + V > A.seg_w) {         // a partial window, or one that crosses a tile's right edge
        uint64_t srow = unpack_row(A, sy, ry, sx);
        for (int i = i0; i < i1; ++i) {
            row[x0 + i] = (T)unpack_one<BITS>(A, srow, xt);
            if (++xt == A.seg_w && i + 1 < i1) {        // on into the next tile
                xt = 0;
                srow = unpack_row(A, sy, ry, ++sx);
            }
        }
        return;
    }
    const uint64_t bit = (uint64_t)xt * BITS;
    const uint64_t b = unpack_row(A, sy, ry, sx) + (bit >> 3);
    const uint64_t b4 = b & ~(uint64_t)3;
    const int sh = (int)(b - b4) * 8 + (int)(bit & 7);  // 0 .. 31: where the window's first bit lies in w[0]
    // sh + V * BITS <= 31 + 128 bits: five dwords.  The fifth is only fetched when a bit of it is wanted.
    uint32_t w[5];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = unpack_dword(A, b4 + 4 * j);
    w[4] = sh + V * BITS > 128 ? unpack_dword(A, b4 + 16) : 0u;
    uint32_t s[4];                                      // the window's bits from bit 0 of s[0]
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = (uint32_t)((((uint64_t)w[j] << 32 | w[j + 1]) << sh) >> 32);
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < V; ++i) {
        constexpr uint32_t MASK = (1u << BITS) - 1u;
        const int p = i * BITS, k = p >> 5, r = p & 31;     // compile-time after unrolling
        uint32_t v;
        if (r + BITS <= 32) v = (s[k] >> (32 - r - BITS)) & MASK;
        else v = (uint32_t)(((uint64_t)s[k] << 32 | s[k + 1 < 4 ? k + 1 : 3]) >> (64 - r - BITS)) & MASK;
        v = unpack_finish<BITS>(A, v);
        o[i * (int)sizeof(T) / 4] |= v << (8 * (int)sizeof(T) * (i % (4 / (int)sizeof(T))));
    }
    *(uint4*)(row + x0) = make_uint4(o[0], o[1], o[2], o[3]);
}

// arguments checked by the caller (capi.hip, raw_layout_check)
inline uint32_t unpack_row_bytes(const mi_raw_layout_t& L) { return (uint32_t)(((uint64_t)L.seg_width * L.bits + 7) / 8); }
inline int unpack_nsx(const mi_raw_layout_t& L) { return cdiv(L.image_width, L.seg_width); }
inline int unpack_nsegs(const mi_raw_layout_t& L) { return unpack_nsx(L) * cdiv(L.image_height, L.seg_height); }

inline void unpack_launch(hipStream_t st, const void* span, size_t span_bytes, const uint32_t* seg, const mi_raw_layout_t& L,
                          const uint16_t* table, void* out) {
    using namespace unpack;
    UnpackArgs A{};
    A.span = (const uint8_t*)span; A.seg = seg; A.table = L.table_len > 0 ? table : nullptr; A.out = out;
    A.span_bytes = (uint32_t)span_bytes;
    A.h = L.height; A.w = L.width; A.crop_y = L.crop_y; A.crop_x = L.crop_x;
    A.seg_h = L.seg_height; A.seg_w = L.seg_width; A.nsx = unpack_nsx(L);
    A.row_bytes = unpack_row_bytes(L);
    A.shift = L.shift; A.table_len = L.table_len;
    A.swap16 = L.bits == 16 && !L.big_endian;
    const int V = VEC_BYTES / (L.bits == 8 ? 1 : 2);
    A.nbx = cdiv(cdiv(L.width + V - 1, V), LANES);      // (a row may start V - 1 samples into its first window)
    const dim3 grid((unsigned)A.nbx * (unsigned)cdiv(L.height, TILE_H)), blk(NT);
    switch (L.bits) {
        case 8: hipLaunchKernelGGL(raw_unpack<8>, grid, blk, 0, st, A); break;
        case 10: hipLaunchKernelGGL(raw_unpack<10>, grid, blk, 0, st, A); break;
        case 12: hipLaunchKernelGGL(raw_unpack<12>, grid, blk, 0, st, A); break;
        case 14: hipLaunchKernelGGL(raw_unpack<14>, grid, blk, 0, st, A); break;
        default: hipLaunchKernelGGL(raw_unpack<16>, grid, blk, 0, st, A); break;
    }
}

}  // namespace mi
