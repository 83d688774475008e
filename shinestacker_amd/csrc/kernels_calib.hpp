// kernels_calib.hpp -- raw calibration frames: master dark / master flat, the flat's gain table, and the per-site correction
// (raw - dark) * flat_gain in place on a mosaic, ahead of everything else that touches the raw samples (kernels_demosaic.hpp:
// the defect repair, then steps A to D).  No reference counterpart -- the reference never sees a mosaic;
// tests/calib_restatement.py is the definition, held bit for bit.  H x W mosaics of uint8 / uint16, H, W >= 2, maxv the
// dtype's maximum, pos = 2 (y & 1) + (x & 1); nothing here depends on the colour pattern.
//
//   master (mosaic_master)     K exposures, 1 <= K <= 32, 0 <= 2 reject < K.  Per site the K samples sorted ascending s[0..K-1],
//                              n = K - 2 reject, S = s[reject] + ... + s[K - reject - 1], out = (S + (n >> 1)) / n: the rounded
//                              mean (reject 0), the median (reject (K - 1) / 2), min/max rejection between.  S < 2^21.
//                              A thread owns 4 neighbouring sites and keeps their K samples in registers as two columns of
//                              packed 16-bit pairs: one packed min and one packed max are one comparator for two sites.  K is
//                              padded to P in {4, 8, 16, 32} with samples of 65535 -- a pad that EQUALS a real sample is
//                              harmless, the sorted sequence of values is the same whichever of the equal ones comes first, so
//                              no 17th bit is needed -- and a bitonic network over the P registers sorts both columns; the sum
//                              takes positions reject .. K - reject - 1.  reject 0 skips the network.  One 8-byte (uint16) or
//                              4-byte (uint8) load per frame and thread, all K issued before the first is used; a wider load
//                              would double the 2 P registers the samples already take.  A frame size that is no multiple of 4
//                              sites (or a buffer off that alignment) takes per-sample loads and stores.
//   flat gain (flat_sums, flat_gain_table)
//                              f = max(F - B, 0) per site, B the flat-dark or black[pos]; S_p = the sum of f over the sites of
//                              position p, N_p their number.  G_q = 16384 where f == 0 or S_p == 0, else
//                              min(65535, (2 * 16384 * S_p + N_p f) / (2 N_p f)): the position's mean over the site's value in
//                              Q14, rounded.  H W < 2^31 (checked by the caller): S_p < 2^45, the numerator < 2^61, the
//                              denominator < 2^47 -- unsigned 64-bit arithmetic holds.  Two passes: the four sums (a thread's
//                              column parity is fixed, its rows alternate; wave reduction, LDS across the four waves, one 64-bit
//                              atomic add per workgroup and position -- integer sums do not depend on the order), then the
//                              quotient per site.  Runs once per session: not tuned.
//   calibrate (mosaic_calibrate, in place)
//                              e = max(v - (D[site] or black[pos]), 0); e' = (e G_q[site] + 8192) >> 14 (e G_q < 2^32: uint32);
//                              out = min(maxv, e' + black[pos]).  The pedestal is put back: a calibrated mosaic is an ordinary
//                              mosaic for the defect repair and for step A.
//
// Calibration is its own in-place pass over the mosaic, as mosaic_defects is, and is NOT fused into demosaic_mhc: the push path
// is bound by the host link (about 1.9 ms per 50 MP uint16 mosaic at the measured 52 GB/s), this pass moves at most 8 bytes per
// site -- a few per cent of that time -- and fusing would double demosaic_mhc's instantiations and re-read both tables at the
// halo sites.
//
// mosaic_calibrate: a workgroup of 256 is calib::TILE_H = 4 rows of 64 lanes, a lane owns one 16-byte window of its row:
// calib::VEC_BYTES / itemsize sites (8 at uint16, 16 at uint8), read and written as one 16-byte access beside 16 bytes of dark
// and 16 (uint16) or 32 (uint8) bytes of gains.  The windows are aligned in MEMORY, not in x: a row that does not start on a
// 16-byte boundary (odd widths at uint16, widths that are no multiple of 16 at uint8) has a partial first window, every row may
// have a partial last one, and partial windows -- as well as windows whose table addresses are off the alignment -- go site by
// site.  A window never crosses a row, so pos alternates with x alone.
// Measured (docs/studies.md, raw mosaics; each beside a device-to-device copy of the bytes the variant moves, in the same run):
//   50 MP uint16: dark 0.043 ms (copy 0.056), flat 0.044 (0.056), both 0.056 (0.075); 24 MP uint8: 0.013 (0.012), 0.016 (0.015),
//   0.020 (0.018) -- memory-bound, at the rate of a copy.  mosaic_master, K = 16: 50 MP uint16 0.291 ms with reject 0 and 0.292 with
//   reject 7, 24 MP uint8 0.087 and 0.112, against 0.617 and 0.158 ms for a device copy of the 16 frames (which writes them too).
//   Config 5's stage 1 from mosaics: 0.184 s calibrated against 0.183 s plain, inside the 0.9 % the plain runs spread over.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace mi {

namespace calib {
constexpr int VEC_BYTES = 16;              // one lane's window of a row
constexpr int NT = 256;
constexpr int LANES = 64;                  // windows of one row per workgroup
constexpr int TILE_H = NT / LANES;         // rows per workgroup
constexpr int MAX_FRAMES = 32;             // K of a master
constexpr int GAIN_ONE = 16384;            // Q14
}  // namespace calib

// ------------------------------------------------------------------------------------------------ calibrate
struct CalibArgs {
    void* mosaic;           // H x W, in place
    const void* dark;       // H x W of the mosaic's type (DARK)
    const uint16_t* gain;   // H x W, Q14 (FLAT)
    int h, w;
    int nbx;                // workgroups along a row
    int32_t black[4];
};

template <typename T, bool DARK, bool FLAT>
__device__ __forceinline__ uint32_t calib_site(uint32_t v, uint32_t d, uint32_t g, int black) {
    constexpr uint32_t maxv = sizeof(T) == 1 ? 255u : 65535u;
    const int e0 = (int)v - (DARK ? (int)d : black);
    uint32_t e = e0 < 0 ? 0u : (uint32_t)e0;
    if constexpr (FLAT) e = (e * g + 8192u) >> 14;
    const uint32_t o = e + (uint32_t)black;
    return o > maxv ? maxv : o;
}

template <typename T, bool DARK, bool FLAT>
__global__ __launch_bounds__(256) void mosaic_calibrate(CalibArgs A) {
    using namespace calib;
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
    [[maybe_unused]] const T* drow = DARK ? (const T*)A.dark + (size_t)y * A.w : nullptr;
    [[maybe_unused]] const uint16_t* grow = FLAT ? A.gain + (size_t)y * A.w : nullptr;
    bool whole = x0 >= 0 && x0 + V <= A.w;
    if constexpr (DARK) whole = whole && ((uintptr_t)(drow + x0) & (VEC_BYTES - 1)) == 0;
    if constexpr (FLAT) whole = whole && ((uintptr_t)(grow + x0) & (VEC_BYTES - 1)) == 0;
    if (whole) {
        constexpr int GW = V / 2;                       // 32-bit words of a window's gains
        uint32_t m[4], d[4] = {0, 0, 0, 0}, g[GW] = {};
        const uint4 mv = *(const uint4*)(row + x0);     // all loads first: in flight together
        uint4 dv = {0, 0, 0, 0}, gv0 = {0, 0, 0, 0}, gv1 = {0, 0, 0, 0};
        if constexpr (DARK) dv = *(const uint4*)(drow + x0);
        if constexpr (FLAT) {
            gv0 = *(const uint4*)(grow + x0);
            if constexpr (GW == 8) gv1 = *(const uint4*)(grow + x0 + 8);
        }
        m[0] = mv.x; m[1] = mv.y; m[2] = mv.z; m[3] = mv.w;
        d[0] = dv.x; d[1] = dv.y; d[2] = dv.z; d[3] = dv.w;
        g[0] = gv0.x; g[1] = gv0.y; g[2] = gv0.z; g[3] = gv0.w;
        if constexpr (GW == 8) { g[4] = gv1.x; g[5] = gv1.y; g[6] = gv1.z; g[7] = gv1.w; }
        uint32_t o[4] = {0, 0, 0, 0};
        const bool odd0 = x0 & 1;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int sh = BITS * (k % PER);
            const uint32_t v = (m[k / PER] >> sh) & MASK, dk = (d[k / PER] >> sh) & MASK;
            const uint32_t gk = (g[k / 2] >> (16 * (k & 1))) & 65535u;
            const int black = (((k & 1) != 0) != odd0) ? b1 : b0;
            o[k / PER] |= calib_site<T, DARK, FLAT>(v, dk, gk, black) << sh;
        }
        *(uint4*)(row + x0) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        const int xa = x0 < 0 ? 0 : x0, xb = x0 + V > A.w ? A.w : x0 + V;
        for (int x = xa; x < xb; ++x) {
            uint32_t dk = 0, gk = 0;
            if constexpr (DARK) dk = drow[x];
            if constexpr (FLAT) gk = grow[x];
            row[x] = (T)calib_site<T, DARK, FLAT>(row[x], dk, gk, (x & 1) ? b1 : b0);
        }
    }
}

// in place on `mosaic` (arguments checked by the caller: capi.hip, calib_check); no flag set launches nothing
inline void calibrate_launch(hipStream_t st, void* mosaic, int h, int w, int dtype, const mi_cfa_t& cfa, const mi_calib_t& c) {
    const bool dark = (c.flags & MI_CALIB_DARK) != 0, flat = (c.flags & MI_CALIB_FLAT) != 0;
    if (!dark && !flat) return;
    const bool u8 = dtype == MI_U8;
    const int v = calib::VEC_BYTES / (u8 ? 1 : 2);
    CalibArgs A{};
    A.mosaic = mosaic; A.dark = c.dev_dark; A.gain = c.dev_gain; A.h = h; A.w = w;
    A.nbx = cdiv(w + v - 1, calib::LANES * v);     // a row off the alignment has one window more
    for (int k = 0; k < 4; ++k) A.black[k] = cfa.black[k];
    const dim3 grid((unsigned)A.nbx * (unsigned)cdiv(h, calib::TILE_H)), blk(calib::NT);
    if (dark && flat) {
        if (u8) hipLaunchKernelGGL((mosaic_calibrate<uint8_t, true, true>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((mosaic_calibrate<uint16_t, true, true>), grid, blk, 0, st, A);
    } else if (dark) {
        if (u8) hipLaunchKernelGGL((mosaic_calibrate<uint8_t, true, false>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((mosaic_calibrate<uint16_t, true, false>), grid, blk, 0, st, A);
    } else {
        if (u8) hipLaunchKernelGGL((mosaic_calibrate<uint8_t, false, true>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((mosaic_calibrate<uint16_t, false, true>), grid, blk, 0, st, A);
    }
}

// ------------------------------------------------------------------------------------------------ master frame
typedef unsigned short calib_us2 __attribute__((ext_vector_type(2)));

struct MasterArgs {
    const void* frames;   // K x n sites, contiguous
    void* out;            // n sites
    size_t n;             // H * W
    int k, reject;
};

// bitonic network over P registers of packed 16-bit pairs, ascending: every index is a compile-time constant
template <int P>
__device__ __forceinline__ void master_sort(calib_us2 (&a)[P]) {
#pragma unroll
    for (int k = 2; k <= P; k *= 2) {
#pragma unroll
        for (int j = k / 2; j > 0; j /= 2) {
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const calib_us2 lo = __builtin_elementwise_min(a[i], a[l]), hi = __builtin_elementwise_max(a[i], a[l]);
                    if ((i & k) == 0) { a[i] = lo; a[l] = hi; }
                    else { a[i] = hi; a[l] = lo; }
                }
            }
        }
    }
}

// VEC: n is a multiple of 4 and both buffers are aligned to 4 samples: a thread's 4 sites are one load per frame, one store
template <typename T, int P, bool VEC>
__global__ __launch_bounds__(256) void mosaic_master(MasterArgs A) {
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= A.n) return;
    const T* src = (const T*)A.frames;
    const int K = A.k;
    uint32_t raw[P][2];      // sites (i0, i0 + 1) and (i0 + 2, i0 + 3) as 16-bit pairs; a pad frame is 65535 everywhere
#pragma unroll
    for (int f = 0; f < P; ++f) {
        raw[f][0] = raw[f][1] = 0xffffffffu;
        if (f < K) {
            const T* p = src + (size_t)f * A.n + i0;
            if constexpr (VEC && sizeof(T) == 2) {
                const uint2 r = *(const uint2*)p;
                raw[f][0] = r.x;
                raw[f][1] = r.y;
            } else if constexpr (VEC) {
                raw[f][0] = *(const uint32_t*)p;      // unpacked below, once every load is on its way
            } else {
                uint32_t s[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] = i0 + j < A.n ? (uint32_t)p[j] : 0u;
                raw[f][0] = s[0] | (s[1] << 16);
                raw[f][1] = s[2] | (s[3] << 16);
            }
        }
    }
    calib_us2 a[P], b[P];
#pragma unroll
    for (int f = 0; f < P; ++f) {
        uint32_t lo = raw[f][0], hi = raw[f][1];
        if constexpr (VEC && sizeof(T) == 1) {
            if (f < K) {
                const uint32_t r = raw[f][0];
                lo = (r & 255u) | ((r >> 8 & 255u) << 16);
                hi = (r >> 16 & 255u) | ((r >> 24) << 16);
            }
        }
        a[f] = __builtin_bit_cast(calib_us2, lo);
        b[f] = __builtin_bit_cast(calib_us2, hi);
    }
    const int reject = A.reject, n = K - 2 * reject;
    if (reject > 0) {     // (the plain mean needs no order)
        master_sort<P>(a);
        master_sort<P>(b);
    }
    uint32_t S[4] = {0, 0, 0, 0};
#pragma unroll
    for (int f = 0; f < P; ++f)
        if (f >= reject && f < K - reject) {      // wave-uniform
            S[0] += a[f].x; S[1] += a[f].y; S[2] += b[f].x; S[3] += b[f].y;
        }
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (S[j] + ((uint32_t)n >> 1)) / (uint32_t)n;
    T* dst = (T*)A.out + i0;
    if constexpr (VEC && sizeof(T) == 2) *(uint2*)dst = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
    else if constexpr (VEC) *(uint32_t*)dst = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < A.n) dst[j] = (T)o[j];
    }
}

template <typename T, int P>
inline void master_launch_p(hipStream_t st, const MasterArgs& A) {
    const dim3 grid((unsigned)((A.n + 4 * 256 - 1) / (4 * 256))), blk(256);
    const uintptr_t align = 4 * sizeof(T) - 1;
    const bool vec = A.n % 4 == 0 && ((uintptr_t)A.frames & align) == 0 && ((uintptr_t)A.out & align) == 0;
    if (vec) hipLaunchKernelGGL((mosaic_master<T, P, true>), grid, blk, 0, st, A);
    else hipLaunchKernelGGL((mosaic_master<T, P, false>), grid, blk, 0, st, A);
}

// arguments checked by the caller (capi.hip, master_check): 1 <= k <= 32, 0 <= 2 reject < k, h * w < 2^31
inline void master_launch(hipStream_t st, const void* frames, int k, int h, int w, int dtype, int reject, void* out) {
    MasterArgs A{frames, out, (size_t)h * (size_t)w, k, reject};
    const bool u8 = dtype == MI_U8;
    if (k <= 4) u8 ? master_launch_p<uint8_t, 4>(st, A) : master_launch_p<uint16_t, 4>(st, A);
    else if (k <= 8) u8 ? master_launch_p<uint8_t, 8>(st, A) : master_launch_p<uint16_t, 8>(st, A);
    else if (k <= 16) u8 ? master_launch_p<uint8_t, 16>(st, A) : master_launch_p<uint16_t, 16>(st, A);
    else u8 ? master_launch_p<uint8_t, 32>(st, A) : master_launch_p<uint16_t, 32>(st, A);
}

// ------------------------------------------------------------------------------------------------ flat gain table
struct FlatArgs {
    const void* flat;             // H x W
    const void* fdark;            // H x W (FDARK), else black[pos]
    uint16_t* gain;               // H x W out
    unsigned long long* sums;     // S_p, zeroed before pass 1
    int h, w;
    int32_t black[4];
};

template <typename T, bool FDARK>
__device__ __forceinline__ uint32_t flat_site(const FlatArgs& A, size_t i, int pos) {
    const int f = (int)((const T*)A.flat)[i] - (FDARK ? (int)((const T*)A.fdark)[i] : A.black[pos]);
    return f < 0 ? 0u : (uint32_t)f;
}

// pass 1: a workgroup walks rows blockIdx.x, + gridDim.x, ...; thread t the columns t, t + 256, ...: its column parity is t & 1
template <typename T, bool FDARK>
__global__ __launch_bounds__(256) void flat_sums(FlatArgs A) {
    __shared__ unsigned long long part[4][4];      // [wave][pos]
    const int t = (int)threadIdx.x, px = t & 1;
    unsigned long long s[2] = {0, 0};              // rows of parity 0 / 1
    for (int y = (int)blockIdx.x; y < A.h; y += (int)gridDim.x) {
        unsigned long long acc = 0;
        for (int x = t; x < A.w; x += 256) acc += flat_site<T, FDARK>(A, (size_t)y * A.w + x, 2 * (y & 1) + px);
        if (y & 1) s[1] += acc;
        else s[0] += acc;
    }
#pragma unroll
    for (int py = 0; py < 2; ++py) {
        uint32_t lo = (uint32_t)s[py], hi = (uint32_t)(s[py] >> 32);
#pragma unroll
        for (int o = 32; o > 1; o >>= 1) {         // (not 1: the lanes keep their column parity)
            const unsigned long long other = ((unsigned long long)(uint32_t)__shfl_xor((int)hi, o) << 32) | (uint32_t)__shfl_xor((int)lo, o);
            const unsigned long long mine = ((unsigned long long)hi << 32) | lo;
            const unsigned long long sum = mine + other;
            lo = (uint32_t)sum;
            hi = (uint32_t)(sum >> 32);
        }
        if ((t & 63) < 2) part[t >> 6][2 * py + px] = ((unsigned long long)hi << 32) | lo;
    }
    __syncthreads();
    if (t < 4) {
        const unsigned long long total = part[0][t] + part[1][t] + part[2][t] + part[3][t];
        if (total) atomicAdd(&A.sums[t], total);
    }
}

// pass 2: one thread per site
template <typename T, bool FDARK>
__global__ __launch_bounds__(256) void flat_gain_table(FlatArgs A) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)A.h * A.w) return;
    const int y = (int)(i / (size_t)A.w), x = (int)(i - (size_t)y * A.w);
    const int py = y & 1, px = x & 1, pos = 2 * py + px;
    const unsigned long long f = flat_site<T, FDARK>(A, i, pos);
    const unsigned long long S = A.sums[pos];
    const unsigned long long N = (unsigned long long)((A.h + 1 - py) >> 1) * (unsigned long long)((A.w + 1 - px) >> 1);
    unsigned long long g = calib::GAIN_ONE;
    if (f != 0 && S != 0) {
        g = (2ull * calib::GAIN_ONE * S + N * f) / (2ull * N * f);
        if (g > 65535ull) g = 65535ull;
    }
    A.gain[i] = (uint16_t)g;
}

// `sums`: 4 x uint64 of device scratch, zeroed here on `st` (arguments checked by the caller: capi.hip, flat_check)
inline hipError_t flat_gain_launch(hipStream_t st, const void* flat, const void* fdark, int h, int w, int dtype, const mi_cfa_t& cfa,
                                   unsigned long long* sums, uint16_t* gain) {
    FlatArgs A{};
    A.flat = flat; A.fdark = fdark; A.gain = gain; A.sums = sums; A.h = h; A.w = w;
    for (int k = 0; k < 4; ++k) A.black[k] = cfa.black[k];
    const hipError_t e = hipMemsetAsync(sums, 0, 4 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const dim3 g1((unsigned)(h < 1024 ? h : 1024)), g2((unsigned)(((size_t)h * w + 255) / 256)), blk(256);
    const bool u8 = dtype == MI_U8;
    if (fdark) {
        if (u8) {
            hipLaunchKernelGGL((flat_sums<uint8_t, true>), g1, blk, 0, st, A);
            hipLaunchKernelGGL((flat_gain_table<uint8_t, true>), g2, blk, 0, st, A);
        } else {
            hipLaunchKernelGGL((flat_sums<uint16_t, true>), g1, blk, 0, st, A);
            hipLaunchKernelGGL((flat_gain_table<uint16_t, true>), g2, blk, 0, st, A);
        }
    } else {
        if (u8) {
            hipLaunchKernelGGL((flat_sums<uint8_t, false>), g1, blk, 0, st, A);
            hipLaunchKernelGGL((flat_gain_table<uint8_t, false>), g2, blk, 0, st, A);
        } else {
            hipLaunchKernelGGL((flat_sums<uint16_t, false>), g1, blk, 0, st, A);
            hipLaunchKernelGGL((flat_gain_table<uint16_t, false>), g2, blk, 0, st, A);
        }
    }
    return hipGetLastError();
}

}  // namespace mi
