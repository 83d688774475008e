// kernels_sitecorr.hpp -- site corrections: the per-site corrections a raw file carries for its own samples (DNG:
// BlackLevelDeltaH/V, the GainMap, FixBadPixelsConstant, FixBadPixelsList), in place on the unpacked mosaic and ahead of
// everything else that touches the raw samples (kernels_calib.hpp, then kernels_demosaic.hpp).  No reference counterpart -- the
// reference never sees a mosaic; tests/sitecorr_restatement.py is the definition, held bit for bit.  H x W mosaics of uint8 /
// uint16, H, W >= 2, maxv the dtype's maximum, pos = 2 (y & 1) + (x & 1); nothing here depends on the colour pattern, and the
// kernels see integers only: all of the file's geometry is resolved on the host into the axis entries.
//
//   site correct (mosaic_site_correct, in place)
//                  b = black[pos] + dh[x] + dv[y] (int16 tables, each may be absent: 0; 0 <= b <= maxv is the caller's promise);
//                  e = max(v - b, 0).  Gain g in Q12: 4096 for a position without a map, else over the position's mv x mh grid of
//                  uint16 nodes n, with the row's axis entry (i, a) and the column's (j, b), weights in [0, 256], the second
//                  node min(i + 1, mv - 1) / min(j + 1, mh - 1):
//                    g = ((256 - a) ((256 - b) n[i][j] + b n[i][j+1]) + a ((256 - b) n[i+1][j] + b n[i+1][j+1]) + 32768) >> 16
//                  (at most 2^16 * 65535 + 32768: uint32).  e' = (e g + 2048) >> 12 (< 2^32); out = min(maxv, e' + black[pos]).
//                  The pedestal is put back, as mosaic_calibrate does: the result is an ordinary mosaic.
//   constant sites (defects_const_flags, mosaic_defects_const, in place)
//                  every site of the positions in `mask` whose value equals C becomes (S + (k >> 1)) / k over its valid
//                  neighbours (y -+ 2, x), (y, x -+ 2) -- inside the image and not themselves such a site; k = 0 leaves it.
//                  Step 0's rule (kernels_demosaic.hpp) with "listed" replaced by "equals C".  A neighbour's "equals C" must be
//                  that of the mosaic as it came, and a neighbour may be rewritten while it is looked at: pass 1 records
//                  "equals C, in mask" as one bit per site (a wave's ballot is 64 sites, one 8-byte store), pass 2 repairs
//                  from the bits.  Values are only read from sites whose bit is clear, and those are never written.  The bit
//                  plane is ordinary device memory of the caller (a handle's stage owns one): a plane taken from the
//                  stream-ordered allocator inside the call came back stale between the passes, for bits that a
//                  workgroup on another XCD had written, from the second call on.
//
// mosaic_site_correct has the shape of mosaic_calibrate: a workgroup of 256 is sitecorr::TILE_H = 4 rows of 64 lanes, a lane
// owns one 16-byte window of its row (8 sites at uint16, 16 at uint8), aligned in MEMORY; partial windows, and windows whose
// dh address is off the alignment, go site by site.  A wave is one row: the row's axis entries, its two positions and whether
// they have a map are wave-uniform.
//
// The node grids are READ THROUGH THE CACHE, not staged in LDS.  Why: a grid may have 257 x 257 nodes per position (132 KB, four
// of them: more than the 160 KB of LDS), so staging means working out, per workgroup, the node rows and columns its tile
// brackets -- and how many those are depends on the spacing: a map denser than the sites (9 x 11 nodes over 5 x 7 sites) brackets
// more nodes than the tile has sites, so the staged block has no useful bound short of the tile's own size.  Through the cache
// the same lines are fetched once per workgroup anyway: a row of the tile touches two node rows, neighbouring sites of a
// position share their four nodes whenever the spacing exceeds two sites (the usual case: 17 x 13 nodes over a sensor), so
// the gathers of a wave coalesce into a handful of 128-byte lines that stay in the 32 KB L1 for the tile's four rows, and all
// four grids (at most 528 KB) stay in the 4 MB L2.  Staging would add a barrier and a second pass over the axis tables to save
// loads that already hit.  The ISA shows what is left: per site one 4-byte axis load and four 2-byte node loads
// (global_load_ushort) beside the window's one 16-byte load and store -- the pass is bound by load issue, not by memory, when
// gains are on.
// Measured (docs/studies.md, raw mosaics; tools/sitecorr_time.py, each beside a device-to-device copy of the same mosaic in the
// same run, resident, 4 maps): 50 MP uint16: deltas 0.034 ms (copy 0.029), gains 0.146 with 17 x 13 and 0.147 with 257 x 257 nodes,
// both 0.151 / 0.151; 24 MP uint8: deltas 0.011 (copy 0.008), gains 0.068 / 0.068, both 0.070 / 0.070.  The deltas run at the
// rate of the copy, as mosaic_calibrate does; the gains take 5 (uint16) to 9 (uint8) copies and do not care about the grid's
// size -- the nodes hit in cache, the time is the issue of five narrow loads and some twenty integer operations per site
// (2.9 ns per thousand sites at either dtype).  Against the host link that brings the mosaic (about 1.9 ms per 50 MP uint16
// frame) it is 8 % of a frame's upload and runs beside the next one.  A row-blended node strip per workgroup in LDS would
// halve the loads; not done while the push path hides the pass.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace mi {

namespace sitecorr {
constexpr int VEC_BYTES = 16;              // one lane's window of a row
constexpr int NT = 256;
constexpr int LANES = 64;                  // windows of one row per workgroup
constexpr int TILE_H = NT / LANES;         // rows per workgroup
constexpr int GAIN_ONE = 4096;             // Q12
constexpr int MAX_NODES = 4096;            // mv, mh of one grid
constexpr int MAX_WEIGHT = 256;
}  // namespace sitecorr

struct SiteGainDev {
    const uint16_t* nodes;      // mv x mh, null: the position has no map
    const uint32_t* row_axis;   // h entries, node | weight << 16 (mi_site_axis_t)
    const uint32_t* col_axis;   // w entries
    int mv, mh;
};

struct SiteArgs {
    void* mosaic;               // H x W, in place
    const int16_t* dh;          // W entries or null
    const int16_t* dv;          // H entries or null
    SiteGainDev g[4];
    int h, w;
    int nbx;                    // workgroups along a row
    int32_t black[4];
};

// what a row needs of one position's map: the two node rows it lies between and its weight
struct SiteRowGain {
    const uint16_t *r0, *r1;
    const uint32_t* col;
    uint32_t a;
    int mh1;
    bool on;
};

__device__ __forceinline__ SiteRowGain site_row_gain(const SiteGainDev& G, int y) {
    SiteRowGain R{};
    R.on = G.nodes != nullptr;
    if (!R.on) return R;
    const uint32_t e = G.row_axis[y];
    int i = (int)(e & 65535u);
    i = i < G.mv - 1 ? i : G.mv - 1;      // (a valid table never needs it: no read outside the grid whatever it holds)
    const int i1 = i + 1 < G.mv ? i + 1 : G.mv - 1;
    R.a = e >> 16;
    R.r0 = G.nodes + (size_t)i * G.mh;
    R.r1 = G.nodes + (size_t)i1 * G.mh;
    R.col = G.col_axis;
    R.mh1 = G.mh - 1;
    return R;
}

// the column's axis entry `e` against the row's two node rows
__device__ __forceinline__ uint32_t site_gain(const SiteRowGain& R, uint32_t e) {
    int j = (int)(e & 65535u);
    j = j < R.mh1 ? j : R.mh1;
    const int j1 = j < R.mh1 ? j + 1 : R.mh1;
    const uint32_t b = e >> 16;
    const uint32_t top = (256u - b) * R.r0[j] + b * R.r0[j1];
    const uint32_t bot = (256u - b) * R.r1[j] + b * R.r1[j1];
    return ((256u - R.a) * top + R.a * bot + 32768u) >> 16;
}

template <typename T, bool DELTA, bool GAIN>
__device__ __forceinline__ uint32_t site_value(uint32_t v, int b, uint32_t g, int black) {
    constexpr uint32_t maxv = sizeof(T) == 1 ? 255u : 65535u;
    const int e0 = (int)v - (DELTA ? b : black);
    uint32_t e = e0 < 0 ? 0u : (uint32_t)e0;
    if constexpr (GAIN) e = (e * g + 2048u) >> 12;
    const uint32_t o = e + (uint32_t)black;
    return o > maxv ? maxv : o;
}

template <typename T, bool DELTA, bool GAIN>
__global__ __launch_bounds__(256) void mosaic_site_correct(SiteArgs A) {
    using namespace sitecorr;
    constexpr int V = VEC_BYTES / (int)sizeof(T);       // sites of a window
    constexpr int PER = 4 / (int)sizeof(T);             // samples of a 32-bit word
    constexpr int BITS = 8 * (int)sizeof(T);
    constexpr uint32_t MASK = sizeof(T) == 1 ? 255u : 65535u;
    const int by = (int)blockIdx.x / A.nbx, bx = (int)blockIdx.x - by * A.nbx;
    const int y = by * TILE_H + (int)threadIdx.x / LANES;
    if (y >= A.h) return;
    T* row = (T*)A.mosaic + (size_t)y * A.w;
    const int off = (int)(((uintptr_t)row & (VEC_BYTES - 1)) / sizeof(T));   // the row starts `off` sites into its first window
    const int x0 = (bx * LANES + ((int)threadIdx.x & (LANES - 1))) * V - off;
    if (x0 >= A.w) return;
    const int b0 = A.black[2 * (y & 1)], b1 = A.black[2 * (y & 1) + 1];
    int dvy = 0;
    if constexpr (DELTA) dvy = A.dv ? (int)A.dv[y] : 0;
    [[maybe_unused]] SiteRowGain R0{}, R1{};
    if constexpr (GAIN) {
        R0 = site_row_gain(A.g[2 * (y & 1)], y);
        R1 = site_row_gain(A.g[2 * (y & 1) + 1], y);
    }
    bool whole = x0 >= 0 && x0 + V <= A.w;
    if constexpr (DELTA) whole = whole && (!A.dh || ((uintptr_t)(A.dh + x0) & (VEC_BYTES - 1)) == 0);
    if (whole) {
        constexpr int DW = V / 2;                       // 32-bit words of a window's column deltas
        uint32_t m[4], d[DW] = {};
        const uint4 mv = *(const uint4*)(row + x0);     // all loads first: in flight together
        uint4 dv0 = {0, 0, 0, 0}, dv1 = {0, 0, 0, 0};
        if constexpr (DELTA) {
            if (A.dh) {
                dv0 = *(const uint4*)(A.dh + x0);
                if constexpr (DW == 8) dv1 = *(const uint4*)(A.dh + x0 + 8);
            }
        }
        uint32_t ce[V] = {};
        if constexpr (GAIN) {
            const bool odd0 = x0 & 1;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const SiteRowGain& R = (((k & 1) != 0) != odd0) ? R1 : R0;
                if (R.on) ce[k] = R.col[x0 + k];
            }
        }
        m[0] = mv.x; m[1] = mv.y; m[2] = mv.z; m[3] = mv.w;
        d[0] = dv0.x; d[1] = dv0.y; d[2] = dv0.z; d[3] = dv0.w;
        if constexpr (DW == 8) { d[4] = dv1.x; d[5] = dv1.y; d[6] = dv1.z; d[7] = dv1.w; }
        uint32_t o[4] = {0, 0, 0, 0};
        const bool odd0 = x0 & 1;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int sh = BITS * (k % PER);
            const uint32_t v = (m[k / PER] >> sh) & MASK;
            const bool second = ((k & 1) != 0) != odd0;
            const int black = second ? b1 : b0;
            const int dhx = (int)(int16_t)((d[k / 2] >> (16 * (k & 1))) & 65535u);
            uint32_t g = GAIN_ONE;
            if constexpr (GAIN) {
                const SiteRowGain& R = second ? R1 : R0;
                if (R.on) g = site_gain(R, ce[k]);
            }
            o[k / PER] |= site_value<T, DELTA, GAIN>(v, black + dhx + dvy, g, black) << sh;
        }
        *(uint4*)(row + x0) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        const int xa = x0 < 0 ? 0 : x0, xb = x0 + V > A.w ? A.w : x0 + V;
        for (int x = xa; x < xb; ++x) {
            const int black = (x & 1) ? b1 : b0;
            int dhx = 0;
            if constexpr (DELTA) dhx = A.dh ? (int)A.dh[x] : 0;
            uint32_t g = GAIN_ONE;
            if constexpr (GAIN) {
                const SiteRowGain& R = (x & 1) ? R1 : R0;
                if (R.on) g = site_gain(R, R.col[x]);
            }
            row[x] = (T)site_value<T, DELTA, GAIN>(row[x], black + dhx + dvy, g, black);
        }
    }
}

// in place on `mosaic` (arguments checked by the caller: mosaic_host.hpp, site_check); neither deltas nor gains: no launch
inline void site_correct_launch(hipStream_t st, void* mosaic, int h, int w, int dtype, const mi_cfa_t& cfa, const mi_site_correct_t& c) {
    const bool delta = (c.flags & (MI_SITE_DELTA_H | MI_SITE_DELTA_V)) != 0, gain = (c.flags & MI_SITE_GAIN) != 0;
    if (!delta && !gain) return;
    const bool u8 = dtype == MI_U8;
    const int v = sitecorr::VEC_BYTES / (u8 ? 1 : 2);
    SiteArgs A{};
    A.mosaic = mosaic; A.h = h; A.w = w;
    A.dh = (c.flags & MI_SITE_DELTA_H) ? c.delta_h : nullptr;
    A.dv = (c.flags & MI_SITE_DELTA_V) ? c.delta_v : nullptr;
    if (gain)
        for (int p = 0; p < 4; ++p) {
            const mi_site_gain_t& g = c.gain[p];
            A.g[p] = SiteGainDev{g.nodes, (const uint32_t*)g.row_axis, (const uint32_t*)g.col_axis, g.mv, g.mh};
        }
    A.nbx = cdiv(w + v - 1, sitecorr::LANES * v);     // a row off the alignment has one window more
    for (int k = 0; k < 4; ++k) A.black[k] = cfa.black[k];
    const dim3 grid((unsigned)A.nbx * (unsigned)cdiv(h, sitecorr::TILE_H)), blk(sitecorr::NT);
    if (delta && gain) {
        if (u8) hipLaunchKernelGGL((mosaic_site_correct<uint8_t, true, true>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((mosaic_site_correct<uint16_t, true, true>), grid, blk, 0, st, A);
    } else if (delta) {
        if (u8) hipLaunchKernelGGL((mosaic_site_correct<uint8_t, true, false>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((mosaic_site_correct<uint16_t, true, false>), grid, blk, 0, st, A);
    } else {
        if (u8) hipLaunchKernelGGL((mosaic_site_correct<uint8_t, false, true>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((mosaic_site_correct<uint16_t, false, true>), grid, blk, 0, st, A);
    }
}

// ------------------------------------------------------------------------------------------------ constant sites
// pass 1: bit s of `bits` (64 sites a word) = site s holds C and its position is in `mask`.  One thread per site; the grid
// covers whole waves, so a word is one wave's ballot.
template <typename T>
__global__ __launch_bounds__(256) void defects_const_flags(const T* mosaic, int h, int w, uint32_t c, int mask, unsigned long long* bits) {
    const unsigned n = (unsigned)h * (unsigned)w;
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    if (s < n) {
        const unsigned y = s / (unsigned)w, x = s - y * (unsigned)w;
        hit = (uint32_t)mosaic[s] == c && ((mask >> (2 * (y & 1) + (x & 1))) & 1);
    }
    const unsigned long long word = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && (s & ~63u) < n) bits[s >> 6] = word;
}

// pass 2: one thread per site; a flagged site is repaired from its unflagged neighbours
template <typename T>
__global__ __launch_bounds__(256) void mosaic_defects_const(T* mosaic, int h, int w, const unsigned long long* bits) {
    const unsigned n = (unsigned)h * (unsigned)w;
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    if (!((bits[s >> 6] >> (s & 63)) & 1ull)) return;
    const int y = (int)(s / (unsigned)w), x = (int)(s - (unsigned)y * (unsigned)w);
    const int is = (int)s;
    const int nb[4] = {is - 2 * w, is + 2 * w, is - 2, is + 2};
    const bool in[4] = {y >= 2, y + 2 < h, x >= 2, x + 2 < w};
    int sum = 0, k = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!in[j]) continue;
        if ((bits[nb[j] >> 6] >> (nb[j] & 63)) & 1ull) continue;
        sum += (int)mosaic[nb[j]];
        ++k;
    }
    if (k) mosaic[s] = (T)((sum + (k >> 1)) / k);
}

inline size_t defects_const_scratch_bytes(int h, int w) { return (((size_t)h * w + 63) / 64) * sizeof(unsigned long long); }

// in place on `mosaic`; `bits`: defects_const_scratch_bytes of device scratch (arguments checked by the caller)
inline void defects_const_launch(hipStream_t st, void* mosaic, int h, int w, int dtype, int constant, int mask, unsigned long long* bits) {
    const dim3 grid((unsigned)(((size_t)h * w + 255) / 256)), blk(256);
    if (dtype == MI_U8) {
        hipLaunchKernelGGL(defects_const_flags<uint8_t>, grid, blk, 0, st, (const uint8_t*)mosaic, h, w, (uint32_t)constant, mask, bits);
        hipLaunchKernelGGL(mosaic_defects_const<uint8_t>, grid, blk, 0, st, (uint8_t*)mosaic, h, w, bits);
    } else {
        hipLaunchKernelGGL(defects_const_flags<uint16_t>, grid, blk, 0, st, (const uint16_t*)mosaic, h, w, (uint32_t)constant, mask, bits);
        hipLaunchKernelGGL(mosaic_defects_const<uint16_t>, grid, blk, 0, st, (uint16_t*)mosaic, h, w, bits);
    }
}

}  // namespace mi
