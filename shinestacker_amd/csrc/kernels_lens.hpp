// kernels_lens.hpp -- lens correction: radial distortion and lateral chromatic aberration as ONE remap per frame, the radial
// part of DNG's WarpRectilinear per colour plane, destination -> source (what a gather needs).  No reference counterpart;
// tests/lens_restatement.py states the arithmetic in NumPy and the kernel is held to it bit for bit.
//
// Per destination pixel (x, y) and plane c (B, G, R), every step float64, every operation rounded once (no product and sum
// may fuse: the build passes -ffp-contract=off and the coordinate code below repeats it as a pragma):
//   dx = x - cx, dy = y - cy;  u = (dx*dx + dy*dy) * inv        inv = 1 / (the largest dx*dx + dy*dy of the four corner
//                                                               pixels), 0.0 when that is 0: computed on the host, lens_launch
//   s = ((k3*u + k2)*u + k1)*u + k0
//   px = min(max(cx + dx*s, -1.0), w),  py = min(max(cy + dy*s, -1.0), h)
//   X = rint(px * 32), Y = rint(py * 32)                        positions in 1/32 pixel, the alignment warp's grid
//   sx = X >> 5, fx = X & 31 (y alike); taps (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1), indices clamped to the frame
//   out = (v00*(32-fx)*(32-fy) + v01*fx*(32-fy) + v10*(32-fx)*fy + v11*fx*fy + 512) >> 10      at most 65535 * 1024 + 512
//   mask = 1 where 0 <= X <= 32 (w - 1) and 0 <= Y <= 32 (h - 1) for all three planes, else 0
// A plane of (1, 0, 0, 0) lands on X = 32 x, Y = 32 y for any centre the boundary admits (|cx|, |cy| <= 2^30: cx + (x - cx)
// is off x by an ulp of the centre at most, 2^-22 pixel), so it is
// its own source pixel: the kernel copies it.  Source and destination are distinct buffers (a gather reads what a
// neighbour writes).
//
// One launch per frame, one thread per destination pixel and row step, taps gathered straight from global memory through
// the caches.  A workgroup owns a 16 x 64 tile (four rows per thread: one source row more than the tile has rows is read
// by a tile, not one more than a wave has).  Two wave-uniform branches on kernel arguments:
//   shared    the three planes have the same coefficients (pure distortion): ONE coordinate set, and the two taps of a
//             source row come in with one unaligned load of 8 bytes (12 at 16 bits) -- the texture-address unit is what
//             a gather like this waits for (kernels_align.hpp: byte loads were that kernel's bottleneck), and 24 MP at 8
//             bits took 74 us this way against 93 us with a dword per tap, docs/studies.md.  Where the taps are no neighbours (clamped at
//             the frame's sides) or the load would leave the buffer (8 bits: the last two pixels) a tap is one dword,
//             and the image's last pixel comes byte by byte -- a 1 x 1 image is that pixel;
//   identity  per plane, the copy above (lateral CA leaves green alone).
// Otherwise a plane has its own coordinates and its taps are loads of that plane's samples (8 bits: the two samples of a
// source row with one dword where the taps are neighbours).
#pragma once
#include "common.hpp"

namespace mi {

namespace lens {
constexpr int TILE_W = 64, TILE_H = 16, NT = 256;
constexpr int ROWS = TILE_H / (NT / TILE_W);    // rows per thread
}  // namespace lens

struct LensArgs {
    const void* src;
    void* dst;
    uint8_t* mask;      // null: no mask
    int h, w, tiles_x;
    int shared;         // the three planes share one coefficient set
    int identity;       // bit c: plane c is (1, 0, 0, 0)
    double k[12];       // k[4 * c + i], c = B, G, R
    double cx, cy, inv;
};

// the source position of plane c in 1/32 pixel; dx, dy and u are the pixel's
// (px lies in [-1, w] and w, h < 2^26 -- lens_check -- so the positions fit an int)
__device__ __forceinline__ void lens_source(const LensArgs& A, int c, double dx, double dy, double u, int& X, int& Y) {
#pragma clang fp contract(off)
    const double k0 = A.k[4 * c], k1 = A.k[4 * c + 1], k2 = A.k[4 * c + 2], k3 = A.k[4 * c + 3];
    double s = k3 * u;
    s = s + k2;
    s = s * u;
    s = s + k1;
    s = s * u;
    s = s + k0;
    double px = dx * s, py = dy * s;
    px = A.cx + px;
    py = A.cy + py;
    px = fmin(fmax(px, -1.0), (double)A.w);
    py = fmin(fmax(py, -1.0), (double)A.h);
    X = (int)rint(px * 32.0);
    Y = (int)rint(py * 32.0);
}

__device__ __forceinline__ int lens_blend(int v00, int v01, int v10, int v11, int fx, int fy) {
    return (v00 * (32 - fx) * (32 - fy) + v01 * fx * (32 - fy) + v10 * (32 - fx) * fy + v11 * fx * fy + 512) >> 10;
}

// the three channels of pixel `pi`; `last`: the image's last pixel
template <typename T>
__device__ __forceinline__ void lens_pixel(const T* __restrict__ src, size_t pi, size_t last, int t[3]) {
    if constexpr (sizeof(T) == 1) {
        if (pi != last) {
            uint32_t v;
            __builtin_memcpy(&v, src + pi * 3, 4);
            t[0] = v & 255u; t[1] = (v >> 8) & 255u; t[2] = (v >> 16) & 255u;
        } else {
            t[0] = src[pi * 3]; t[1] = src[pi * 3 + 1]; t[2] = src[pi * 3 + 2];
        }
    } else {
        uint32_t v;
        uint16_t v2;
        __builtin_memcpy(&v, src + pi * 3, 4);
        __builtin_memcpy(&v2, src + pi * 3 + 2, 2);
        t[0] = v & 65535u; t[1] = v >> 16; t[2] = v2;
    }
}

// the pixels `pi` and `pi + 1` of one row with ONE load: 8 bytes at 8 bits, whose last two belong to pixel pi + 2 -- the caller
// keeps pi + 2 <= last --, 12 bytes at 16 bits
template <typename T>
__device__ __forceinline__ void lens_pixel_pair(const T* __restrict__ src, size_t pi, int a[3], int b[3]) {
    if constexpr (sizeof(T) == 1) {
        uint32_t v[2];
        __builtin_memcpy(v, src + pi * 3, 8);
        a[0] = v[0] & 255u; a[1] = (v[0] >> 8) & 255u; a[2] = (v[0] >> 16) & 255u;
        b[0] = v[0] >> 24; b[1] = v[1] & 255u; b[2] = (v[1] >> 8) & 255u;
    } else {
        uint32_t v[3];
        __builtin_memcpy(v, src + pi * 3, 12);
        a[0] = v[0] & 65535u; a[1] = v[0] >> 16; a[2] = v[1] & 65535u;
        b[0] = v[1] >> 16; b[1] = v[2] & 65535u; b[2] = v[2] >> 16;
    }
}

// the taps (row, x0) and (row, x1) of a row that starts at pixel `r`: together where they are neighbours in memory
template <typename T>
__device__ __forceinline__ void lens_row_taps(const T* __restrict__ src, size_t r, int x0, int x1, size_t last, int a[3], int b[3]) {
    if (x1 == x0 + 1 && (sizeof(T) == 2 || r + x0 + 2 <= last)) {
        lens_pixel_pair(src, r + x0, a, b);
    } else {
        lens_pixel(src, r + x0, last, a);
        lens_pixel(src, r + x1, last, b);
    }
}

// plane c's samples of the taps (row, x0) and (row, x1).  8 bits: neighbouring pixels' samples are the first and the last of
// four consecutive bytes -- one dword, which ends with the second tap's sample and so never leaves the buffer.  (16 bits: the
// same trick is an 8-byte load for 4 bytes of use, and measured SLOWER than the two 2-byte loads: docs/studies.md.)
template <typename T>
__device__ __forceinline__ void lens_row_samples(const T* __restrict__ src, size_t r, int x0, int x1, int c, int& a, int& b) {
    const T* p = src + (r + x0) * 3 + c;
    if (sizeof(T) == 1 && x1 == x0 + 1) {
        uint32_t v;
        __builtin_memcpy(&v, p, 4);
        a = v & 255u; b = v >> 24;
    } else {
        a = p[0];
        b = src[(r + x1) * 3 + c];
    }
}

template <typename T, bool MASK>
__global__ __launch_bounds__(lens::NT) void lens_remap(LensArgs A) {
    const T* __restrict__ src = (const T*)A.src;
    T* __restrict__ dst = (T*)A.dst;
    const int h = A.h, w = A.w;
    const int x = ((int)blockIdx.x % A.tiles_x) * lens::TILE_W + ((int)threadIdx.x & (lens::TILE_W - 1));
    const int yt = ((int)blockIdx.x / A.tiles_x) * lens::TILE_H + ((int)threadIdx.x / lens::TILE_W);
    if (x >= w) return;
    const size_t last = (size_t)h * w - 1;
    const int Xmax = 32 * (w - 1), Ymax = 32 * (h - 1);
    double dx, dx2;
    {
#pragma clang fp contract(off)
        dx = (double)x - A.cx;
        dx2 = dx * dx;
    }
#pragma unroll 1
    for (int r = 0; r < lens::ROWS; ++r) {
        const int y = yt + r * (lens::NT / lens::TILE_W);
        if (y >= h) return;
        double dy, u;
        {
#pragma clang fp contract(off)
            dy = (double)y - A.cy;
            const double dy2 = dy * dy;
            u = dx2 + dy2;
            u = u * A.inv;
        }
        const size_t po = (size_t)y * w + x;
        int out[3];
        bool ok = true;
        if (A.shared) {
            int X, Y;
            lens_source(A, 0, dx, dy, u, X, Y);
            ok = X >= 0 && X <= Xmax && Y >= 0 && Y <= Ymax;
            const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
            const int x0 = min(max(sx, 0), w - 1), x1 = min(max(sx + 1, 0), w - 1);
            const size_t r0 = (size_t)min(max(sy, 0), h - 1) * w, r1 = (size_t)min(max(sy + 1, 0), h - 1) * w;
            int q00[3], q01[3], q10[3], q11[3];
            lens_row_taps(src, r0, x0, x1, last, q00, q01);
            lens_row_taps(src, r1, x0, x1, last, q10, q11);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c] = lens_blend(q00[c], q01[c], q10[c], q11[c], fx, fy);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (A.identity >> c & 1) {
                    out[c] = src[po * 3 + c];
                    continue;
                }
                int X, Y;
                lens_source(A, c, dx, dy, u, X, Y);
                ok = ok && X >= 0 && X <= Xmax && Y >= 0 && Y <= Ymax;
                const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
                const int x0 = min(max(sx, 0), w - 1), x1 = min(max(sx + 1, 0), w - 1);
                const size_t r0 = (size_t)min(max(sy, 0), h - 1) * w, r1 = (size_t)min(max(sy + 1, 0), h - 1) * w;
                int v00, v01, v10, v11;
                lens_row_samples(src, r0, x0, x1, c, v00, v01);
                lens_row_samples(src, r1, x0, x1, c, v10, v11);
                out[c] = lens_blend(v00, v01, v10, v11, fx, fy);
            }
        }
        dst[po * 3] = (T)out[0];
        dst[po * 3 + 1] = (T)out[1];
        dst[po * 3 + 2] = (T)out[2];
        if constexpr (MASK) A.mask[po] = ok ? 1 : 0;
    }
}

// 1 / (the largest squared distance of a corner pixel from the centre), 0.0 when that is 0 (a 1 x 1 frame about its pixel)
inline double lens_inv_r2(int h, int w, double cx, double cy) {
#pragma clang fp contract(off)
    double r2 = 0.0;
    for (int i = 0; i < 4; ++i) {
        const double dx = (double)((i & 1) ? w - 1 : 0) - cx, dy = (double)((i & 2) ? h - 1 : 0) - cy;
        const double dx2 = dx * dx, dy2 = dy * dy;
        const double r = dx2 + dy2;
        if (r > r2) r2 = r;
    }
    return r2 == 0.0 ? 0.0 : 1.0 / r2;
}

// `src` -> `dst` (distinct), `mask` may be null (arguments checked by the caller: capi.hip, lens_check)
inline void lens_launch(hipStream_t st, const void* src, void* dst, void* mask, int h, int w, int dtype, const mi_lens_t& L) {
    LensArgs A{};
    A.src = src; A.dst = dst; A.mask = (uint8_t*)mask; A.h = h; A.w = w;
    A.tiles_x = cdiv(w, lens::TILE_W);
    memcpy(A.k, L.k, sizeof(A.k));
    A.cx = L.cx; A.cy = L.cy;
    A.inv = lens_inv_r2(h, w, L.cx, L.cy);
    A.shared = memcmp(L.k, L.k + 4, 4 * sizeof(double)) == 0 && memcmp(L.k, L.k + 8, 4 * sizeof(double)) == 0;
    for (int c = 0; c < 3; ++c)
        if (L.k[4 * c] == 1.0 && L.k[4 * c + 1] == 0.0 && L.k[4 * c + 2] == 0.0 && L.k[4 * c + 3] == 0.0) A.identity |= 1 << c;
    const dim3 grid((unsigned)A.tiles_x * (unsigned)cdiv(h, lens::TILE_H)), blk(lens::NT);
    const bool u8 = dtype == MI_U8;
    if (mask) {
        if (u8) hipLaunchKernelGGL((lens_remap<uint8_t, true>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((lens_remap<uint16_t, true>), grid, blk, 0, st, A);
    } else {
        if (u8) hipLaunchKernelGGL((lens_remap<uint8_t, false>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((lens_remap<uint16_t, false>), grid, blk, 0, st, A);
    }
}

}  // namespace mi
