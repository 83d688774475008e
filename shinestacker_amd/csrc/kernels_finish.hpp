// kernels_finish.hpp -- what a raw file says about the finished picture and the reader had only reported (DNG:
// FixVignetteRadial of OpcodeList3, DefaultCropOrigin / DefaultCropSize, Orientation).  No reference counterpart -- the
// reference never opens a raw file; tests/finish_restatement.py is the definition, held bit for bit.  The kernels see integers
// only: the polynomial, the warp's inverse and the file's geometry are resolved on the host (dng.RadialGain, dng.Finish).
//
//   radial gain (mosaic_radial_gain, in place on the H x W mosaic, uint8 / uint16, behind the site corrections and ahead of
//                the calibration: the gain belongs on linear samples, as the GainMap's does)
//                  the centre in half pixels (cx2, cy2);  d2 = (2x - cx2)^2 + (2y - cy2)^2 in 64 bits; D = the largest d2 of
//                  the four corner sites (1 <= D < 2^40: radial_check);  shift = the largest s with (2^(18+s) / D) < 2^24,
//                  mul = floor(2^(18+s) / D) (radial_map: one division per LAUNCH, none per site)
//                  q = min((d2 * mul) >> shift, 2^18): u = d2 / D in [0, 1] as node (q >> 8, of 1024 intervals) and weight
//                  (q & 255); d2 * mul < 2^40 * 2^24: no overflow, and q <= 2^18 by construction (the min is a guard)
//                  g = (t[node] (256 - weight) + t[min(node + 1, 1024)] weight + 128) >> 8     t: 1025 Q12 uint16 nodes
//                  e = max(v - black[pos], 0);  e' = (e g + 2048) >> 12 (< 2^32);  out = min(maxv, e' + black[pos])
//   frame finish (frame_finish, out of place: H x W x 3 -> the cropped, oriented H' x W' x 3; B, G, R stay in place inside a
//                pixel).  With a the crop a[y, x] = src[cy + y, cx + x] (ch x cw) and the TIFF orientations:
//                  1: a   2: a[:, ::-1]   3: a[::-1, ::-1]   4: a[::-1]                   (H' x W' = ch x cw)
//                  5: a.T   6: rot90(a, -1)   7: a[::-1, ::-1].T   8: rot90(a, 1)         (H' x W' = cw x ch)
//                as two flips and a transposition: out[i, j] = a[fy ? ch-1-i : i, fx ? cw-1-j : j] for 1..4 (fx: 2, 3; fy: 3,
//                4), out[i, j] = a[fy ? ch-1-j : j, fx ? cw-1-i : i] for 5..8 (fy: 6, 7; fx: 7, 8).
//
// mosaic_radial_gain has the shape of mosaic_site_correct: a workgroup of 256 is 4 rows of 64 lanes, a lane owns one 16-byte
// window of its row, aligned in MEMORY; partial windows go site by site.  The table is staged in LDS as 1025 dwords
// (t[i] | t[min(i + 1, 1024)] << 16: 4.1 KB, every site reads one dword, ds_read_b32): it is read by every site at an address
// that depends on the site's radius, and a wave's 64 sites of a row span few nodes, so most lanes of a group read the same
// or neighbouring dwords (equal addresses broadcast).  Per site: two 32-bit multiplies for the squares' sum (dy^2 is per
// row), one 64 x 24-bit multiply, one LDS read, the blend and the gain.
//
// frame_finish<T, false> (orientations 1..4): a row copy.  A lane owns one 16-byte window of a DESTINATION row, aligned in
// memory (rows of cw x 3 samples start anywhere on the 16-byte grid); whole windows are one 16-byte store.  Without the
// column flip the window's source is 16 contiguous bytes at whatever alignment the crop's origin leaves (a byte offset of
// (cy W + cx) 3 sizeof(T)): one 16-byte load at the samples' own alignment.  With the flip the pixels reverse and the three
// samples inside one do not: the window's samples come from 18 (uint8) or 9 to 12 (uint16) contiguous source samples, read
// with two 16-byte loads and put in place in registers (finish_flip_window), then stored as one window.
//
// frame_finish<T, true> (orientations 5..8): through an LDS tile of 32 x 32 pixels, one DWORD PER SAMPLE: 32 rows of 96
// dwords, row stride 99.  Load phase: the 256 threads walk the tile's source rows, sample k of a row from lane k (reads
// along source rows: consecutive lanes, consecutive samples) into dword r * 99 + k.  Store phase: they walk the
// destination rows; a destination row holds the tile's column xc, its samples k = 3 jj + c in destination order come from
// the tile's row r = jj (fy: R - 1 - jj), dword r * 99 + 3 xc + c, and go out to consecutive samples of the destination row
// (writes along destination rows).  96 = 3 * 32: every 32-lane group lies inside one row in both phases.
// Conflict arithmetic, by the bank rule (64 banks of 4 bytes; ds_write_b32 and ds_read_b32 bank on (a / 4) % 32, conflicts
// are counted inside each 32-lane half): the load phase writes 32 consecutive dwords per group: 32 banks, no conflict.  The
// store phase reads dword 99 r + 3 xc + c; 99 = 3 (mod 32), so the bank is 3 jj + c + const = k + const: the 32 consecutive k
// of a group hit 32 different banks -- no conflict (a stride of 96 would put all rows on one bank: 32 / 3 = 11-way; 97 puts
// r + c on a bank: 3-way).  With fy the bank is c - 3 jj + const: inside whole triples still a run of consecutive integers;
// a group that starts inside a triple covers 33 or 34 consecutive integers with one or two holes: at most one or two
// 2-way conflicts per group.  This is arithmetic from the rule, NOT a counter reading.
// The global accesses of this kernel are one sample per lane (64 or 128 bytes per wave-instruction): coalesced, not wide.
//
// Measured (docs/studies.md, DNG files; tools/finish_time.py, resident frames, each beside a device-to-device copy of the same
// bytes in the same run): 50 MP uint16: the gain 0.053 ms (copy of the mosaic 0.029, mosaic_site_correct's deltas 0.034);
// frame_finish 0.112 (orientations 1, 4), 0.153 (2, 3), 0.259 (5 to 8) against a copy of the frame at 0.112.  24 MP uint8: the
// gain 0.025 (copy 0.008, deltas 0.011); frame_finish 0.024, 0.025, 0.091 against 0.021.  The plain row copy runs at the rate
// of the copy, odd crop origin or not; the column flip, which took 0.062 at uint8 while it gathered sample by sample, is 1.2
// copies at uint8 and 1.4 at uint16 with its two wide loads; the transposition pays for one sample per lane on both sides
// (4.3 copies at uint8, 2.3 at uint16).  Packing the tile's samples into dwords before they leave is the step not built: the
// pass runs once per frame, at most a seventh of the frame's upload over the host link.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace mi {

namespace finish {
constexpr int VEC_BYTES = 16;              // one lane's window of a row
constexpr int NT = 256;
constexpr int LANES = 64;                  // windows of one row per workgroup
constexpr int TILE_H = NT / LANES;         // rows per workgroup (row kernels)
constexpr int NODES = 1025;                // the radial table: 1024 intervals over u in [0, 1]
constexpr int Q_ONE = 1 << 18;             // u = 1 as node << 8 | weight
constexpr int TILE = 32;                   // the transposition's tile, pixels each way
constexpr int TROW = 3 * TILE;             // dwords of a tile row in use
constexpr int TSTRIDE = TROW + 3;          // 99 = 3 (mod 32)
constexpr long long D2_MAX = 1ll << 40;    // D below it: d2 * mul < 2^64
constexpr int CENTRE_MAX = 1 << 24;        // |cx2|, |cy2| up to it: the corner distances are computed in 64 bits without care
}  // namespace finish

struct RadialArgs {
    void* mosaic;               // H x W, in place
    const uint16_t* table;      // finish::NODES Q12 entries
    int h, w;
    int nbx;                    // workgroups along a row
    int cx2, cy2;
    unsigned long long mul;
    int shift;
    int32_t black[4];
};

// the largest d2 of the four corner sites
inline long long radial_d2max(int h, int w, int cx2, int cy2) {
    long long best = 0;
    for (int yy = 0; yy < 2; ++yy)
        for (int xx = 0; xx < 2; ++xx) {
            const long long dx = 2ll * (xx ? w - 1 : 0) - cx2, dy = 2ll * (yy ? h - 1 : 0) - cy2;
            best = dx * dx + dy * dy > best ? dx * dx + dy * dy : best;
        }
    return best;
}

// d2 -> q: the largest shift whose multiplier stays below 2^24 (1 <= D < 2^40: 5 <= shift <= 46)
inline void radial_map(long long D, unsigned long long* mul, int* shift) {
    int s = 46;
    while (s > 0 && ((unsigned __int128)1 << (18 + s)) / (unsigned long long)D >= (1ull << 24)) --s;
    *shift = s;
    *mul = (unsigned long long)(((unsigned __int128)1 << (18 + s)) / (unsigned long long)D);
}

template <typename T>
__device__ __forceinline__ uint32_t radial_site(uint32_t v, int x, unsigned long long dy2, const RadialArgs& A, const uint32_t* lds,
                                                int black) {
    constexpr uint32_t maxv = sizeof(T) == 1 ? 255u : 65535u;
    const long long dx = 2ll * x - A.cx2;
    const unsigned long long d2 = (unsigned long long)(dx * dx) + dy2;
    unsigned long long q64 = (d2 * A.mul) >> A.shift;
    const uint32_t q = q64 > (unsigned long long)finish::Q_ONE ? (uint32_t)finish::Q_ONE : (uint32_t)q64;
    const uint32_t pair = lds[q >> 8], wt = q & 255u;
    const uint32_t g = ((pair & 65535u) * (256u - wt) + (pair >> 16) * wt + 128u) >> 8;
    const int e0 = (int)v - black;
    const uint32_t e = e0 < 0 ? 0u : (uint32_t)e0;
    const uint32_t o = ((e * g + 2048u) >> 12) + (uint32_t)black;
    return o > maxv ? maxv : o;
}

template <typename T>
__global__ __launch_bounds__(256) void mosaic_radial_gain(RadialArgs A) {
    using namespace finish;
    constexpr int V = VEC_BYTES / (int)sizeof(T);       // sites of a window
    constexpr int PER = 4 / (int)sizeof(T);             // samples of a 32-bit word
    constexpr int BITS = 8 * (int)sizeof(T);
    constexpr uint32_t MASK = sizeof(T) == 1 ? 255u : 65535u;
    __shared__ uint32_t lds[NODES];
    for (int i = (int)threadIdx.x; i < NODES; i += NT) {   // before any lane leaves: every thread reaches the barrier
        const int i1 = i + 1 < NODES ? i + 1 : NODES - 1;
        lds[i] = (uint32_t)A.table[i] | ((uint32_t)A.table[i1] << 16);
    }
    __syncthreads();
    const int by = (int)blockIdx.x / A.nbx, bx = (int)blockIdx.x - by * A.nbx;
    const int y = by * TILE_H + (int)threadIdx.x / LANES;
    if (y >= A.h) return;
    T* row = (T*)A.mosaic + (size_t)y * A.w;
    const int off = (int)(((uintptr_t)row & (VEC_BYTES - 1)) / sizeof(T));   // the row starts `off` sites into its first window
    const int x0 = (bx * LANES + ((int)threadIdx.x & (LANES - 1))) * V - off;
    if (x0 >= A.w) return;
    const int b0 = A.black[2 * (y & 1)], b1 = A.black[2 * (y & 1) + 1];
    const long long dy = 2ll * y - A.cy2;
    const unsigned long long dy2 = (unsigned long long)(dy * dy);
    if (x0 >= 0 && x0 + V <= A.w) {
        const uint4 mv = *(const uint4*)(row + x0);
        const uint32_t m[4] = {mv.x, mv.y, mv.z, mv.w};
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int sh = BITS * (k % PER);
            const uint32_t v = (m[k / PER] >> sh) & MASK;
            o[k / PER] |= radial_site<T>(v, x0 + k, dy2, A, lds, ((x0 + k) & 1) ? b1 : b0) << sh;
        }
        *(uint4*)(row + x0) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        const int xa = x0 < 0 ? 0 : x0, xb = x0 + V > A.w ? A.w : x0 + V;
        for (int x = xa; x < xb; ++x) row[x] = (T)radial_site<T>(row[x], x, dy2, A, lds, (x & 1) ? b1 : b0);
    }
}

// in place on `mosaic` (arguments checked by the caller: radial_check)
inline void radial_gain_launch(hipStream_t st, void* mosaic, int h, int w, int dtype, const int32_t* black, const mi_radial_gain_t& r) {
    const bool u8 = dtype == MI_U8;
    const int v = finish::VEC_BYTES / (u8 ? 1 : 2);
    RadialArgs A{};
    A.mosaic = mosaic; A.table = r.table; A.h = h; A.w = w; A.cx2 = r.cx2; A.cy2 = r.cy2;
    radial_map(radial_d2max(h, w, r.cx2, r.cy2), &A.mul, &A.shift);
    A.nbx = cdiv(w + v - 1, finish::LANES * v);       // a row off the alignment has one window more
    for (int k = 0; k < 4; ++k) A.black[k] = black[k];
    const dim3 grid((unsigned)A.nbx * (unsigned)cdiv(h, finish::TILE_H)), blk(finish::NT);
    if (u8) hipLaunchKernelGGL(mosaic_radial_gain<uint8_t>, grid, blk, 0, st, A);
    else hipLaunchKernelGGL(mosaic_radial_gain<uint16_t>, grid, blk, 0, st, A);
}

// ------------------------------------------------------------------------------------------------ crop + orientation
struct FinishArgs {
    const void* src;            // H x W x 3
    void* dst;                  // H' x W' x 3
    int w;                      // the source's width, pixels
    int cy, cx, ch, cw;         // the crop
    int fx, fy;                 // the flips (see the header)
    int nbx;                    // workgroups along a destination row / tiles across the crop
};

// 16 bytes at the samples' own alignment: one global_load_dwordx4 wherever they lie
struct __attribute__((packed)) FinishWindow1 { uint32_t v[4]; };
struct __attribute__((packed, aligned(2))) FinishWindow2 { uint32_t v[4]; };
template <typename T>
using FinishWindow = std::conditional_t<sizeof(T) == 1, FinishWindow1, FinishWindow2>;

// A whole destination window under the column flip.  Its V samples start at channel C0 of destination pixel p0 and touch NP
// pixels, whose sources are the 3 NP contiguous samples of source pixels cw - p0 - NP .. cw - 1 - p0 (inside the row: the
// window is).  3 NP is 18 samples at uint8, 9 or 12 at uint16: at least V and at most 2 V, so two 16-byte loads cover them,
// one from the span's first sample and one that ends at its last.  Which loaded sample goes where depends on C0 alone: with
// C0 a template argument every index below is a constant and the shuffle is shifts and masks on registers.
template <typename T, int C0>
__device__ __forceinline__ void finish_flip_window(const T* srow, int cw, int p0, uint32_t (&o)[4]) {
    constexpr int V = finish::VEC_BYTES / (int)sizeof(T), PER = 4 / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    constexpr uint32_t MASK = sizeof(T) == 1 ? 255u : 65535u;
    constexpr int NP = (C0 + V - 1) / 3 + 1, TAIL = 3 * NP - V;
    static_assert(TAIL >= 0 && TAIL <= V, "two windows cover the span");
    const T* lo = srow + 3 * (cw - p0 - NP);
    const FinishWindow<T> a = *(const FinishWindow<T>*)lo, b = *(const FinishWindow<T>*)(lo + TAIL);
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int dp = (C0 + k) / 3, c = (C0 + k) % 3;
        const int s = 3 * (NP - 1 - dp) + c;                      // the sample's place in the span
        const uint32_t word = s < V ? a.v[s / PER] : b.v[(s - TAIL) / PER];
        const int sh = BITS * ((s < V ? s : s - TAIL) % PER);
        o[k / PER] |= ((word >> sh) & MASK) << (BITS * (k % PER));
    }
}

template <typename T, bool TRANSPOSE>
__global__ __launch_bounds__(256) void frame_finish(FinishArgs A) {
    using namespace finish;
    const T* src = (const T*)A.src;
    T* dst = (T*)A.dst;
    if constexpr (!TRANSPOSE) {
        constexpr int V = VEC_BYTES / (int)sizeof(T);
        const int by = (int)blockIdx.x / A.nbx, bx = (int)blockIdx.x - by * A.nbx;
        const int i = by * TILE_H + (int)threadIdx.x / LANES;
        if (i >= A.ch) return;
        const int n = 3 * A.cw;                                          // samples of a row
        T* drow = dst + (size_t)i * n;
        const T* srow = src + ((size_t)(A.cy + (A.fy ? A.ch - 1 - i : i)) * A.w + A.cx) * 3;
        const int off = (int)(((uintptr_t)drow & (VEC_BYTES - 1)) / sizeof(T));
        const int e0 = (bx * LANES + ((int)threadIdx.x & (LANES - 1))) * V - off;
        if (e0 >= n) return;
        if (e0 >= 0 && e0 + V <= n) {
            uint32_t o[4] = {0, 0, 0, 0};
            if (!A.fx) {
                const FinishWindow<T> wv = *(const FinishWindow<T>*)(srow + e0);
                o[0] = wv.v[0]; o[1] = wv.v[1]; o[2] = wv.v[2]; o[3] = wv.v[3];
            } else {
                const int p0 = e0 / 3, c0 = e0 - 3 * p0;
                if (c0 == 0) finish_flip_window<T, 0>(srow, A.cw, p0, o);
                else if (c0 == 1) finish_flip_window<T, 1>(srow, A.cw, p0, o);
                else finish_flip_window<T, 2>(srow, A.cw, p0, o);
            }
            *(uint4*)(drow + e0) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            const int ea = e0 < 0 ? 0 : e0, eb = e0 + V > n ? n : e0 + V;
            for (int e = ea; e < eb; ++e) {
                const int p = e / 3, c = e - 3 * p;
                drow[e] = srow[A.fx ? 3 * (A.cw - 1 - p) + c : e];
            }
        }
    } else {
        __shared__ uint32_t tile[TILE * TSTRIDE];
        const int ty = (int)blockIdx.x / A.nbx, tx = (int)blockIdx.x - ty * A.nbx;
        const int y0 = ty * TILE, x0 = tx * TILE;
        const int R = A.ch - y0 < TILE ? A.ch - y0 : TILE, C = A.cw - x0 < TILE ? A.cw - x0 : TILE;   // the tile's rows, columns
        const T* s0 = src + ((size_t)(A.cy + y0) * A.w + A.cx + x0) * 3;
        for (int idx = (int)threadIdx.x; idx < TILE * TROW; idx += NT) {
            const int r = idx / TROW, k = idx - r * TROW;
            if (r < R && k < 3 * C) tile[r * TSTRIDE + k] = (uint32_t)s0[(size_t)r * A.w * 3 + k];
        }
        __syncthreads();
        // destination row of the tile's column xc, and the first destination pixel of the tile's rows
        const int j0 = A.fy ? A.ch - y0 - R : y0;
        for (int idx = (int)threadIdx.x; idx < TILE * TROW; idx += NT) {
            const int xc = idx / TROW, k = idx - xc * TROW;
            if (xc >= C || k >= 3 * R) continue;
            const int jj = k / 3, c = k - 3 * jj;
            const int r = A.fy ? R - 1 - jj : jj;
            const int i = A.fx ? A.cw - 1 - (x0 + xc) : x0 + xc;
            dst[((size_t)i * A.ch + j0) * 3 + k] = (T)tile[r * TSTRIDE + 3 * xc + c];
        }
    }
}

// orientation 1..8 -> (transpose, fx, fy)
inline void finish_flips(int orientation, bool* transpose, int* fx, int* fy) {
    *transpose = orientation >= 5;
    *fx = orientation == 2 || orientation == 3 || orientation == 7 || orientation == 8;
    *fy = orientation == 3 || orientation == 4 || orientation == 6 || orientation == 7;
}

// src (h x w x 3) -> dst (arguments checked by the caller: finish_check)
inline void frame_finish_launch(hipStream_t st, const void* src, void* dst, int w, int dtype, int cy, int cx, int ch, int cw,
                                int orientation) {
    const bool u8 = dtype == MI_U8;
    bool tr;
    FinishArgs A{};
    A.src = src; A.dst = dst; A.w = w; A.cy = cy; A.cx = cx; A.ch = ch; A.cw = cw;
    finish_flips(orientation, &tr, &A.fx, &A.fy);
    const dim3 blk(finish::NT);
    if (!tr) {
        const int v = finish::VEC_BYTES / (u8 ? 1 : 2);
        A.nbx = cdiv(3 * cw + v - 1, finish::LANES * v);
        const dim3 grid((unsigned)A.nbx * (unsigned)cdiv(ch, finish::TILE_H));
        if (u8) hipLaunchKernelGGL((frame_finish<uint8_t, false>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((frame_finish<uint16_t, false>), grid, blk, 0, st, A);
    } else {
        A.nbx = cdiv(cw, finish::TILE);
        const dim3 grid((unsigned)A.nbx * (unsigned)cdiv(ch, finish::TILE));
        if (u8) hipLaunchKernelGGL((frame_finish<uint8_t, true>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((frame_finish<uint16_t, true>), grid, blk, 0, st, A);
    }
}

}  // namespace mi
