// kernels_composite.hpp -- the depth-selected composite (no reference counterpart): every pixel taken from the frame the depth
// map names, not from a fused Laplacian pyramid -- no halos, no amplified noise.  A gather across N resident frames steered by a
// float32 plane; shinestacker_amd/depth_render.py renders whole stacks with it in bounded memory.
//
// The operation (the specification; tests/depth_render_restatement.py states it in NumPy and is held bit for bit):
//
// **Inputs**
// - `N` frames of `H x W x 3` samples of one type (uint8, uint16 or float32), frame `i` having global index `i`.
// - A depth plane `D`, `H x W` float32, in global frame numbers.
// - `interp`, `'linear'` (default) or `'nearest'`.
//
// **Per pixel**, in float32, every operation rounded on its own.  This translation unit is compiled with contraction off.
// - `d = D[y, x]`.  NaN becomes `0`.  Then `d = min(max(d, 0), f32(N - 1))`.
// - `'nearest'`: `k = int32(rint(d))`, ties to even.  The three samples of frame `k` are copied, never computed.
// - `'linear'`:
//   - `k0 = int32(floor(d))`, `f = d - f32(k0)` (exact), `k1 = min(k0 + 1, N - 1)`.
//   - Per sample, `a` from frame `k0` and `b` from frame `k1`, both converted to float32: `v = a + f * (b - a)`, computed as one
//     subtract, one multiply and one add.
//   - Integer types store `rint(v)` clamped to the type's range.  The clamp never binds: with `f < 1` the rounded
//     `f * (b - a)` cannot exceed `b - a` in size, so `v` stays between `a` and `b`.  The clamp is kept all the same.
//   - float32 stores `v`.
//   - With `f == 0` the result is `a` bit for bit: the sample is selected, not computed (`a + 0 * (b - a)` would turn a
//     float32 `-0` into `+0`, and an infinite `b - a` into NaN).
//
// **Chunks**, so that a stack larger than what the caller wants resident can be rendered in bounded memory:
// - A call holds `count` consecutive frames starting at global index `first`, of a stack of `n_frames`.
// - A pixel belongs to the call when `first <= k0 < first + count - 1`, or when `k0 == n_frames - 1 == first + count - 1`
//   (`k0` decides for both `interp`; the `k` of `'nearest'` is `k0` or `k0 + 1`, so it lies inside the chunk).
// - Pixels that do not belong are not read in the frames and not written in the output.
// - `count >= 2` unless `n_frames == 1`.  Consecutive calls overlap by one frame.
// - The union of the calls over `[0, n_frames)` equals the one-call result exactly, for both `interp`.
//
// (Implementation notes, not part of the specification: max(d, 0) is written `d > 0 ? d : 0`, which turns a NaN and -0 into +0;
// n_frames <= 2^24 keeps f32(N - 1) exact.)
//
// depth_composite_kernel: one launch per call, no LDS, no atomics.  The frame is a flat run of H W pixels (rows are dense); a
// lane owns MI_DC_PX = 4 consecutive pixels -- one 16-byte depth load, 12 samples = 3 (uint8), 6 (uint16) or 12 (float32) whole
// 4-byte words of every frame and of the output, since 12 sizeof(T) is a multiple of 4 --, a wave 256 pixels, a workgroup of 256
// lanes 1024.  Grid: ceil(ceil(H W / 4) / 256) workgroups.  The frame addresses travel in a table of up to MI_DC_TAB = 64 pointers
// inside the kernel arguments: the launch copies them into the kernel-argument segment, device-visible memory that is read with
// scalar loads, so nothing is allocated, uploaded or freed around the launch.  A call over more than 64 frames is several
// launches over sub-chunks that overlap by one frame, which the chunk rule makes exact.
//   fast path: a ballot finds the waves whose every lane owns all four of its pixels (or none) with ONE frame index k0 (k for
//     'nearest'), and whose frames start on 4-byte boundaries.  The index goes through readfirstlane, so the one or two table
//     entries are scalar loads and every frame access is a plain coalesced vector load off a scalar base; the samples are unpacked
//     from the words, mixed, packed, and leave as whole words.
//   gather path (a mixed wave, a chunk boundary or the frame's ragged end inside the wave, or an unaligned frame): every pixel
//     loads its own table entries and its samples one by one; a word whose samples all belong still leaves as a word, the others
//     sample by sample.
//   Both paths run the same dc_mix on the same operands, so they give the same bits.
// HBM bytes per pixel, s = sizeof(T): depth 4, frames 3 s ('nearest') or 6 s ('linear'; the fast path skips frame k1 when the
// whole wave has f == 0), output 3 s: 10 / 13 B for uint8, 16 / 22 B for uint16, 28 / 40 B for float32.
#pragma once
#include "common.hpp"

namespace mi {

#define MI_DC_PX 4                      // pixels per lane
#define MI_DC_TAB 64                    // frame addresses per launch
#define MI_DC_LINEAR 0
#define MI_DC_NEAREST 1

// one sample of 'linear': a from frame k0, b from frame k1
template <typename T>
__device__ __forceinline__ T dc_mix(T a, T b, float f) {
    if (f == 0.0f) return a;
    const float fa = (float)a, fb = (float)b;
    const float df = fb - fa;
    const float m = f * df;
    const float v = fa + m;
    if constexpr (sizeof(T) == 4) {
        return v;
    } else {
        constexpr float top = sizeof(T) == 1 ? 255.0f : 65535.0f;
        float r = rintf(v);
        r = r > 0.0f ? r : 0.0f;
        r = r < top ? r : top;
        return (T)r;
    }
}

template <typename T>
__device__ __forceinline__ T dc_unpack(uint32_t w, int q) {
    if constexpr (sizeof(T) == 4) return __uint_as_float(w);
    else return (T)(w >> (8 * (int)sizeof(T) * q));
}

template <typename T>
__device__ __forceinline__ uint32_t dc_pack(T v, int q) {
    if constexpr (sizeof(T) == 4) return __float_as_uint(v);
    else return (uint32_t)v << (8 * (int)sizeof(T) * q);
}

struct DcTable {
    const void* p[MI_DC_TAB];
};

template <typename T>
__global__ __launch_bounds__(256) void depth_composite_kernel(const DcTable table, const float* __restrict__ depth, T* __restrict__ out,
                                                              size_t npx, int first, int count, int n_frames, int nearest) {
    const T* const* tab = reinterpret_cast<const T* const*>(table.p);
    constexpr int EPW = 4 / (int)sizeof(T);                 // samples per 4-byte word
    constexpr int NS = 3 * MI_DC_PX, NW = NS / EPW;         // samples and words per lane
    const size_t p0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * MI_DC_PX;
    const int n_here = p0 >= npx ? 0 : (int)(npx - p0 < (size_t)MI_DC_PX ? npx - p0 : (size_t)MI_DC_PX);
    const float top = (float)(n_frames - 1);
    const int last = first + count - 1;
    float dv[MI_DC_PX] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (n_here == MI_DC_PX) {
        const float4 d4 = *reinterpret_cast<const float4*>(depth + p0);      // the plane starts on a 16-byte boundary
        dv[0] = d4.x, dv[1] = d4.y, dv[2] = d4.z, dv[3] = d4.w;
    } else {
        for (int q = 0; q < n_here; ++q) dv[q] = depth[p0 + q];
    }
    int sel[MI_DC_PX], k1[MI_DC_PX];                        // the frame(s) of each pixel, relative to `first`
    float f[MI_DC_PX];
    bool own[MI_DC_PX];
    int n_own = 0, lane_k = -1;
    bool lane_one = true, lane_f0 = true;
#pragma unroll
    for (int q = 0; q < MI_DC_PX; ++q) {
        float d = dv[q];
        d = d > 0.0f ? d : 0.0f;
        d = d < top ? d : top;
        const int k0 = (int)floorf(d);
        own[q] = q < n_here && ((k0 >= first && k0 < last) || (k0 == n_frames - 1 && k0 == last));
        if (nearest) {
            sel[q] = (int)rintf(d) - first;
            k1[q] = sel[q];
            f[q] = 0.0f;
        } else {
            sel[q] = k0 - first;
            k1[q] = (k0 + 1 < n_frames ? k0 + 1 : n_frames - 1) - first;
            f[q] = d - (float)k0;
        }
        if (own[q]) {
            if (n_own == 0) lane_k = sel[q];
            lane_one = lane_one && sel[q] == lane_k;
            lane_f0 = lane_f0 && f[q] == 0.0f;
            ++n_own;
        }
    }
    const unsigned long long active = __ballot(n_own > 0);
    if (active == 0ull) return;                             // the wave owns nothing: no frame is read, nothing is written
    const int kref = __shfl(lane_k, __ffsll((long long)active) - 1);
    const bool wave_one = __ballot(n_own > 0 && (n_own != MI_DC_PX || !lane_one || lane_k != kref)) == 0ull;
    if (wave_one) {
        const int ku = __builtin_amdgcn_readfirstlane(kref);
        const bool need_b = !nearest && __ballot(n_own > 0 && !lane_f0) != 0ull;
        const T* __restrict__ fa = tab[ku];                 // wave-uniform: scalar loads
        const T* __restrict__ fb = need_b ? tab[(first + ku + 1 < n_frames ? ku + 1 : ku)] : fa;
        if (((((uintptr_t)fa) | ((uintptr_t)fb)) & 3u) == 0) {
            if (n_own > 0) {
                const uint32_t* __restrict__ wa = reinterpret_cast<const uint32_t*>(fa + p0 * 3);
                uint32_t* __restrict__ wo = reinterpret_cast<uint32_t*>(out + p0 * 3);
                uint32_t a[NW], b[NW];
#pragma unroll
                for (int j = 0; j < NW; ++j) a[j] = wa[j];
                if (need_b) {
                    const uint32_t* __restrict__ wb = reinterpret_cast<const uint32_t*>(fb + p0 * 3);
#pragma unroll
                    for (int j = 0; j < NW; ++j) b[j] = wb[j];
#pragma unroll
                    for (int j = 0; j < NW; ++j) {
                        uint32_t v = 0;
#pragma unroll
                        for (int q = 0; q < EPW; ++q)
                            v |= dc_pack<T>(dc_mix<T>(dc_unpack<T>(a[j], q), dc_unpack<T>(b[j], q), f[(j * EPW + q) / 3]), q);
                        a[j] = v;
                    }
                }
#pragma unroll
                for (int j = 0; j < NW; ++j) wo[j] = a[j];
            }
            return;
        }
    }
    if (n_own == 0) return;
    const T* pa[MI_DC_PX];
    const T* pb[MI_DC_PX];
#pragma unroll
    for (int q = 0; q < MI_DC_PX; ++q) {
        pa[q] = pb[q] = nullptr;
        if (own[q]) {
            pa[q] = tab[sel[q]] + (p0 + q) * 3;
            pb[q] = f[q] == 0.0f ? pa[q] : tab[k1[q]] + (p0 + q) * 3;
        }
    }
    T* __restrict__ o = out + p0 * 3;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        T s[EPW];
        bool all = true;
#pragma unroll
        for (int q = 0; q < EPW; ++q) {
            const int e = j * EPW + q, p = e / 3, c = e - 3 * p;
            all = all && own[p];
            s[q] = own[p] ? dc_mix<T>(pa[p][c], pb[p][c], f[p]) : (T)0;
        }
        if (all) {
            uint32_t v = 0;
#pragma unroll
            for (int q = 0; q < EPW; ++q) v |= dc_pack<T>(s[q], q);
            *reinterpret_cast<uint32_t*>(o + j * EPW) = v;
        } else {
#pragma unroll
            for (int q = 0; q < EPW; ++q)
                if (own[(j * EPW + q) / 3]) o[j * EPW + q] = s[q];
        }
    }
}

// `frames`: the HOST array of the call's `count` device addresses
template <typename T>
inline void depth_composite_launch(hipStream_t st, const void* const* frames, const float* depth, void* out, size_t npx, int first,
                                   int count, int n_frames, int nearest) {
    const size_t lanes = (npx + MI_DC_PX - 1) / MI_DC_PX;
    for (int f0 = 0;; f0 += MI_DC_TAB - 1) {        // (a sub-chunk that is not the last leaves at least 2 frames for the next)
        const int c = count - f0 < MI_DC_TAB ? count - f0 : MI_DC_TAB;
        DcTable table;
        for (int i = 0; i < MI_DC_TAB; ++i) table.p[i] = i < c ? frames[f0 + i] : nullptr;
        hipLaunchKernelGGL((depth_composite_kernel<T>), dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, table, depth, (T*)out, npx,
                           first + f0, c, n_frames, nearest);
        if (f0 + c >= count) break;
    }
}

}  // namespace mi
