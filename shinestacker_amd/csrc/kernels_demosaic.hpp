// kernels_demosaic.hpp -- raw Bayer mosaics in: black level, gain and Malvar-He-Cutler demosaic in one pass, H x W samples of
// uint8 / uint16 to H x W x 3 interleaved BGR of the same type (the layout every kernel here reads).  No reference
// counterpart -- the reference never sees a mosaic; tests/demosaic_restatement.py is the definition, held bit for bit.
//
//   step A, per site:  v' = min(white, (max(v - black[pos], 0) * gain_q[pos] + 2048) >> 12), pos = 2 (y & 1) + (x & 1);
//                      gain_q = round(gain * 4096) < 2^16 is quantised once by the caller, the product stays below 2^32
//   step B:            Malvar, He, Cutler (ICASSP 2004): the 5 x 5 linear kernels, the paper's coefficients times 2 so that
//                      every sum is an integer over 16 (|sum| < 2^22 at uint16):
//                          G at an R/B site            8 c + 4 (l + r + u + d) - 2 (ll + rr + uu + dd)
//                          C at a G site, C left/right 10 c + 8 (l + r) - 2 (4 diagonals) - 2 (ll + rr) + (uu + dd)
//                          C at a G site, C above/below: its transpose
//                          C at the opposite colour    12 c + 4 (4 diagonals) - 3 (ll + rr + uu + dd)
//                      out = clamp((sum + 8) >> 4, 0, white), arithmetic shift; a site's own colour is v' itself
//   borders:           BORDER_REFLECT_101 on the mosaic: the period 2 (n - 1) is even, so a reflected sample has the colour
//                      the tap expects at every size >= 2
//
// Raw development around it, each step optional (tests/develop_restatement.py is the definition, held bit for bit):
//   step 0, defect sites (mosaic_defects, in place on the raw samples, ahead of step A): a listed site becomes
//                      (S + (k >> 1)) / k over its k valid neighbours at distance 2 in its row and column -- the same cell
//                      position, so the same colour, black level and gain; valid: inside the image and not itself listed;
//                      k = 0 leaves the site.  One thread per listed site, "listed" by binary search in the ascending list.
//                      Listed sites are only written and unlisted ones only read: one launch in place has no hazard.
//   step C, colour matrix (demosaic_mhc<T, true, *>): on step B's clamped (b, g, r), M_q = round(M * 4096) in R, G, B order,
//                      out_i = clamp((M_q[i][0] r + M_q[i][1] g + M_q[i][2] b + 2048) >> 12, 0, white); a row's sum of
//                      |M_q| is at most 32767 (checked by the caller), so |sum| + 2048 <= 32767 * 65535 + 2048 < 2^31: int32
//   step D, tone curve (demosaic_mhc<T, *, true>): out = tone[out], a table of maxv + 1 entries of T built by the caller
// Steps C and D are an epilogue on the values the thread holds between demosaic_round and the packing of its stores: no
// extra pass over HBM.  The matrix is read from the kernel arguments (wave-uniform: scalar loads, as the cfa).  The uint8
// table (256 B) is staged in LDS beside the tile by the workgroup's 256 threads; the uint16 table (128 KB) is gathered from
// global memory, where it stays in L2 -- it would take the LDS of a whole CU and leave one workgroup resident per CU.
// Measured, 50 MP uint16 (plain 0.112 ms): matrix 0.127 ms, tone 0.385 ms on a uniform random frame, where every lane of a
// gather addresses another cache line; 24 MP uint8 (plain 0.043 ms): matrix 0.056 ms, tone 0.041 ms (docs/studies.md).
//
// One workgroup of 256 owns a TILE_H x TILE_W tile.  1. The tile and its halo of 2 sites, step A and the reflection applied, are
// staged in LDS as uint16 (20 x 132 x 2 B = 5.3 KB): the 13 taps read LDS only.  A thread stages (even, odd) column pairs, which
// share their black levels and gains and are one 32-bit LDS word, with all its loads issued before the first is used; a tile
// whose halo lies inside the image takes a path without reflection.  2. A thread owns whole 2 x 2 CFA cells -- one
// cell at uint16, two side by side at uint8, 12 bytes of BGR per output row either way -- so no lane branches on the colour of
// its site (which cell positions hold G and whether the first row's colour is R are wave-uniform), its 6 x (4 + 2 CX) window is
// read as aligned 32-bit LDS words with consecutive lanes on consecutive words (uint16) or word pairs (uint8), and a wave's
// stores of one row are one contiguous run: 768 bytes.  A row whose address is 4-byte aligned is stored as one 12-byte store per
// lane; other rows (odd widths at uint16, widths not a multiple of 4 at uint8) and the ragged last cell per sample.
// Traffic: itemsize bytes read, 3 * itemsize written per pixel.  Bound by instruction issue rather than memory: 50 MP uint16 in
// 0.113 ms, 1.5 x a device copy of the same bytes (docs/studies.md, raw mosaics).
#pragma once
#include <type_traits>

#include "common.hpp"

namespace mi {

namespace demosaic {
constexpr int TILE_H = 16;
constexpr int TILE_W = 128;
constexpr int NT = 256;
constexpr int PITCH = TILE_W + 4;   // LDS row of the tile and its halo, in samples (even: 32-bit reads stay aligned)
constexpr int ROWS = TILE_H + 4;
}  // namespace demosaic

struct DemosaicArgs {
    const void* src;   // H x W
    void* dst;         // H x W x 3
    int h, w;
    mi_cfa_t cfa;      // wave-uniform reads: scalar loads from the kernel arguments
};

// the developed kernels' arguments: the plain ones and the epilogue's tables
struct DevelopArgs : DemosaicArgs {
    int32_t mq[9];     // M_q, row-major, rows and columns in R, G, B order (MATRIX)
    const void* tone;  // maxv + 1 entries of T in device memory (TONE)
};

struct alignas(4) DemosaicRow {
    uint32_t w[3];
};

// One site of the window `v` (centre at row cy, column cx): CHROMA: (a, b, g) = (own, opposite colour, G); at a G site:
// (the colour left and right, the colour above and below, own).  Sums over 16, not yet rounded.
template <bool CHROMA, int NW>
__device__ __forceinline__ void demosaic_site(const int (&v)[6][NW], int cy, int cx, int& a, int& b, int& g) {
    const int c = v[cy][cx];
    const int h2 = v[cy][cx - 1] + v[cy][cx + 1], v2 = v[cy - 1][cx] + v[cy + 1][cx];
    const int d4 = v[cy - 1][cx - 1] + v[cy - 1][cx + 1] + v[cy + 1][cx - 1] + v[cy + 1][cx + 1];
    const int fh = v[cy][cx - 2] + v[cy][cx + 2], fv = v[cy - 2][cx] + v[cy + 2][cx];
    if constexpr (CHROMA) {
        a = 16 * c;
        b = 12 * c + 4 * d4 - 3 * (fh + fv);
        g = 8 * c + 4 * (h2 + v2) - 2 * (fh + fv);
    } else {
        a = 10 * c + 8 * h2 - 2 * d4 - 2 * fh + fv;
        b = 10 * c + 8 * v2 - 2 * d4 - 2 * fv + fh;
        g = 16 * c;
    }
}

__device__ __forceinline__ int demosaic_round(int sum, int white) {
    const int r = (sum + 8) >> 4;
    return r < 0 ? 0 : (r > white ? white : r);
}

// step C on one pixel: (b, g, r) in place
__device__ __forceinline__ void develop_matrix(const int32_t (&mq)[9], int& b, int& g, int& r, int white) {
    const int o_r = (mq[0] * r + mq[1] * g + mq[2] * b + 2048) >> 12;
    const int o_g = (mq[3] * r + mq[4] * g + mq[5] * b + 2048) >> 12;
    const int o_b = (mq[6] * r + mq[7] * g + mq[8] * b + 2048) >> 12;
    r = o_r < 0 ? 0 : (o_r > white ? white : o_r);
    g = o_g < 0 ? 0 : (o_g > white ? white : o_g);
    b = o_b < 0 ? 0 : (o_b > white ? white : o_b);
}

// the cells of one thread: G0: the cell's first site is G (GRBG, GBRG); else its first site is R or B (RGGB, BGGR).
// MATRIX / TONE: steps C and D on the rounded values (`mq`: the kernel's arguments; `tone`: LDS at uint8, global at uint16)
template <typename T, bool G0, int CX, bool MATRIX = false, bool TONE = false, typename TONE_PTR = const T*>
__device__ __forceinline__ void demosaic_unit(const uint16_t* tile, int ly, int lx, T* dst, int y, int x, int H, int W, bool r_first,
                                              int white, const int32_t (*mq)[9] = nullptr, TONE_PTR tone = nullptr) {
    using namespace demosaic;
    constexpr int NW = 4 + 2 * CX;
    int v[6][NW];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const uint32_t* p = (const uint32_t*)(tile + (ly + r) * PITCH + lx);
#pragma unroll
        for (int k = 0; k < NW / 2; ++k) {
            const uint32_t d = p[k];
            v[r][2 * k] = (int)(d & 0xffffu);
            v[r][2 * k + 1] = (int)(d >> 16);
        }
    }
    constexpr int NPX = 2 * CX;
#pragma unroll
    for (int sy = 0; sy < 2; ++sy) {
        if (y + sy >= H) break;
        T e[NPX * 3];
#pragma unroll
        for (int px = 0; px < NPX; ++px) {
            int a, b, g;
            if (((px & 1) == sy) != G0) demosaic_site<true, NW>(v, 2 + sy, 2 + px, a, b, g);
            else demosaic_site<false, NW>(v, 2 + sy, 2 + px, a, b, g);
            // `a` belongs to this row's chroma: R in the cell's first row when r_first, in its second row otherwise
            const bool a_is_r = (sy == 0) == r_first;
            if constexpr (!MATRIX && !TONE) {
                e[px * 3 + 0] = (T)demosaic_round(a_is_r ? b : a, white);
                e[px * 3 + 1] = (T)demosaic_round(g, white);
                e[px * 3 + 2] = (T)demosaic_round(a_is_r ? a : b, white);
            } else {
                int ob = demosaic_round(a_is_r ? b : a, white), og = demosaic_round(g, white), orr = demosaic_round(a_is_r ? a : b, white);
                if constexpr (MATRIX) develop_matrix(*mq, ob, og, orr, white);
                if constexpr (TONE) {   // 0 <= value <= white <= maxv: inside the table
                    ob = tone[ob];
                    og = tone[og];
                    orr = tone[orr];
                }
                e[px * 3 + 0] = (T)ob;
                e[px * 3 + 1] = (T)og;
                e[px * 3 + 2] = (T)orr;
            }
        }
        T* row = dst + ((size_t)(y + sy) * W + x) * 3;
        if (x + NPX <= W && ((uintptr_t)row & 3) == 0) {
            constexpr int PER = 4 / (int)sizeof(T);
            DemosaicRow o;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                uint32_t d = 0;
#pragma unroll
                for (int j = 0; j < PER; ++j) d |= (uint32_t)e[k * PER + j] << (8 * (int)sizeof(T) * j);
                o.w[k] = d;
            }
            *(DemosaicRow*)row = o;
        } else {
#pragma unroll
            for (int px = 0; px < NPX; ++px)
                if (x + px < W) {
                    row[px * 3 + 0] = e[px * 3 + 0];
                    row[px * 3 + 1] = e[px * 3 + 1];
                    row[px * 3 + 2] = e[px * 3 + 2];
                }
        }
    }
}

// The loads of one thread's share of the tile and its halo: pair i = the sites (row i / PAIRS, columns 2 (i % PAIRS) and + 1) of
// the staged tile.  INSIDE: the whole staged tile lies in the image -- no reflection, straight-line code.
template <typename T, bool INSIDE, int STEPS>
__device__ __forceinline__ void demosaic_load(const T* src, int H, int W, int ty0, int tx0, uint32_t (&raw)[STEPS][2]) {
    using namespace demosaic;
    constexpr int PAIRS = PITCH / 2, NPAIR = ROWS * PAIRS;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const int i = (int)threadIdx.x + k * NT;
        raw[k][0] = raw[k][1] = 0;
        if (k < NPAIR / NT || i < NPAIR) {      // (only the last step is ragged: the others are straight-line code)
            const int r = i / PAIRS, c = 2 * (i - r * PAIRS);
            int y = ty0 - 2 + r, x0 = tx0 - 2 + c, x1 = x0 + 1;
            if constexpr (!INSIDE) {
                // sites past n + 1 feed no output of this image (a ragged last tile): any in-bounds sample will do for them
                y = r101_loop(y > H + 1 ? H + 1 : y, H);
                x0 = r101_loop(x0 > W + 1 ? W + 1 : x0, W);
                x1 = r101_loop(x1 > W + 1 ? W + 1 : x1, W);
            }
            const T* row = src + (size_t)y * W;
            raw[k][0] = row[x0];
            raw[k][1] = row[x1];
        }
    }
}

template <typename T, bool MATRIX = false, bool TONE = false>
__global__ __launch_bounds__(256) void demosaic_mhc(std::conditional_t<MATRIX || TONE, DevelopArgs, DemosaicArgs> A) {
    using namespace demosaic;
    constexpr int CX = sizeof(T) == 1 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) uint16_t tile[ROWS * PITCH];
    constexpr bool TONE_LDS = TONE && sizeof(T) == 1;
    [[maybe_unused]] const uint8_t* tone_lds = nullptr;
    if constexpr (TONE_LDS) {   // NT == 256 == the table's length; visible behind the tile's barrier
        static_assert(NT == 256, "one table entry per thread");
        __shared__ uint8_t staged[256];
        staged[threadIdx.x] = ((const uint8_t*)A.tone)[threadIdx.x];
        tone_lds = staged;
    }
    const int H = A.h, W = A.w;
    const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
    const T* src = (const T*)A.src;
    const bool inside = tx0 >= 2 && ty0 >= 2 && tx0 + TILE_W + 2 <= W && ty0 + TILE_H + 2 <= H;
    const int white = A.cfa.white;
    // Staging, two sites of a row per step: the tile's first column and row are even, so a pair is an (even, odd) column pair
    // of one row parity and shares its black levels and gains.  All loads first, then step A: the loads of a thread are in
    // flight together.
    constexpr int PAIRS = PITCH / 2, NPAIR = ROWS * PAIRS, STEPS = (NPAIR + NT - 1) / NT;
    uint32_t raw[STEPS][2];
    if (inside) demosaic_load<T, true, STEPS>(src, H, W, ty0, tx0, raw);
    else demosaic_load<T, false, STEPS>(src, H, W, ty0, tx0, raw);
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
        const int i = (int)threadIdx.x + k * NT;
        if (k < NPAIR / NT || i < NPAIR) {      // (only the last step is ragged: the others are straight-line code)
            const bool odd_row = (i / PAIRS) & 1;      // the reflection keeps a coordinate's parity: its period is even
            uint32_t q[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int black = odd_row ? A.cfa.black[2 + j] : A.cfa.black[j];
                const uint32_t gain = odd_row ? A.cfa.gain_q[2 + j] : A.cfa.gain_q[j];
                const int d = (int)raw[k][j] - black;
                const uint32_t v = ((uint32_t)(d < 0 ? 0 : d) * gain + 2048u) >> 12;
                q[j] = v > (uint32_t)white ? (uint32_t)white : v;
            }
            ((uint32_t*)tile)[i] = q[0] | (q[1] << 16);
        }
    }
    __syncthreads();
    constexpr int UX = TILE_W / (2 * CX);        // threads' units along a tile row
    constexpr int UNITS = UX * (TILE_H / 2);
    const bool r_first = !(A.cfa.pattern & 1);   // RGGB, GRBG: the cell's first row holds R
    const bool g0 = (A.cfa.pattern & 2) != 0;    // GRBG, GBRG: the cell's first site is G
    for (int u = threadIdx.x; u < UNITS; u += NT) {
        const int uy = u / UX, ux = u - uy * UX;
        const int ly = 2 * uy, lx = 2 * CX * ux;
        const int y = ty0 + ly, x = tx0 + lx;
        if (y >= H || x >= W) continue;
        if constexpr (!MATRIX && !TONE) {
            if (g0) demosaic_unit<T, true, CX>(tile, ly, lx, (T*)A.dst, y, x, H, W, r_first, white);
            else demosaic_unit<T, false, CX>(tile, ly, lx, (T*)A.dst, y, x, H, W, r_first, white);
        } else if constexpr (TONE_LDS) {
            if (g0) demosaic_unit<T, true, CX, MATRIX, true, const uint8_t*>(tile, ly, lx, (T*)A.dst, y, x, H, W, r_first, white, &A.mq, tone_lds);
            else demosaic_unit<T, false, CX, MATRIX, true, const uint8_t*>(tile, ly, lx, (T*)A.dst, y, x, H, W, r_first, white, &A.mq, tone_lds);
        } else {
            if (g0) demosaic_unit<T, true, CX, MATRIX, TONE>(tile, ly, lx, (T*)A.dst, y, x, H, W, r_first, white, &A.mq, (const T*)A.tone);
            else demosaic_unit<T, false, CX, MATRIX, TONE>(tile, ly, lx, (T*)A.dst, y, x, H, W, r_first, white, &A.mq, (const T*)A.tone);
        }
    }
}

// step 0: one thread per listed site (ascending, unique, < h * w: the caller's precondition; a site outside is left alone)
template <typename T>
__global__ __launch_bounds__(256) void mosaic_defects(T* mosaic, int h, int w, const int32_t* sites, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = sites[i];
    if (s < 0 || s >= h * w) return;
    const int y = s / w, x = s - y * w;
    const int nb[4] = {s - 2 * w, s + 2 * w, s - 2, s + 2};
    const bool in[4] = {y >= 2, y + 2 < h, x >= 2, x + 2 < w};
    int sum = 0, k = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!in[j]) continue;
        int lo = 0, hi = n;   // is nb[j] listed? lower bound in the ascending list
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sites[mid] < nb[j]) lo = mid + 1;
            else hi = mid;
        }
        if (lo < n && sites[lo] == nb[j]) continue;
        sum += (int)mosaic[nb[j]];
        ++k;
    }
    if (k) mosaic[s] = (T)((sum + (k >> 1)) / k);
}

// the arguments were checked by the caller (capi.hip: demosaic_check)
inline void demosaic_launch(hipStream_t st, const void* src, void* dst, int h, int w, int dtype, const mi_cfa_t& cfa) {
    DemosaicArgs A{src, dst, h, w, cfa};
    const dim3 grid(cdiv(w, demosaic::TILE_W), cdiv(h, demosaic::TILE_H));
    if (dtype == MI_U8) hipLaunchKernelGGL(demosaic_mhc<uint8_t>, grid, dim3(demosaic::NT), 0, st, A);
    else hipLaunchKernelGGL(demosaic_mhc<uint16_t>, grid, dim3(demosaic::NT), 0, st, A);
}

// step 0 in place on `mosaic` (arguments checked by the caller: capi.hip, defects_check); n == 0 launches nothing
inline void defects_launch(hipStream_t st, void* mosaic, int h, int w, int dtype, const int32_t* dev_sites, int n) {
    if (n <= 0) return;
    if (dtype == MI_U8) hipLaunchKernelGGL(mosaic_defects<uint8_t>, dim3(cdiv(n, 256)), dim3(256), 0, st, (uint8_t*)mosaic, h, w, dev_sites, n);
    else hipLaunchKernelGGL(mosaic_defects<uint16_t>, dim3(cdiv(n, 256)), dim3(256), 0, st, (uint16_t*)mosaic, h, w, dev_sites, n);
}

// steps A to D (arguments checked by the caller: capi.hip, develop_check); no flag set: the plain kernel, as demosaic_launch
inline void develop_launch(hipStream_t st, const void* src, void* dst, int h, int w, int dtype, const mi_cfa_t& cfa,
                           const mi_develop_t& dev) {
    const bool mat = (dev.flags & MI_DEVELOP_MATRIX) != 0, tone = (dev.flags & MI_DEVELOP_TONE) != 0;
    if (!mat && !tone) return demosaic_launch(st, src, dst, h, w, dtype, cfa);
    DevelopArgs A{};
    A.src = src; A.dst = dst; A.h = h; A.w = w; A.cfa = cfa;
    for (int k = 0; k < 9; ++k) A.mq[k] = dev.matrix_q[k];
    A.tone = dev.dev_tone;
    const dim3 grid(cdiv(w, demosaic::TILE_W), cdiv(h, demosaic::TILE_H)), blk(demosaic::NT);
    const bool u8 = dtype == MI_U8;
    if (mat && tone) {
        if (u8) hipLaunchKernelGGL((demosaic_mhc<uint8_t, true, true>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((demosaic_mhc<uint16_t, true, true>), grid, blk, 0, st, A);
    } else if (mat) {
        if (u8) hipLaunchKernelGGL((demosaic_mhc<uint8_t, true, false>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((demosaic_mhc<uint16_t, true, false>), grid, blk, 0, st, A);
    } else {
        if (u8) hipLaunchKernelGGL((demosaic_mhc<uint8_t, false, true>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((demosaic_mhc<uint16_t, false, true>), grid, blk, 0, st, A);
    }
}

}  // namespace mi
