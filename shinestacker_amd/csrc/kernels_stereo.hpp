// kernels_stereo.hpp -- stereo views from the depth map (no reference counterpart): the fused frame re-rendered from a
// viewpoint shifted sideways, every pixel displaced along its row by its nearness.  A forward scatter with occlusion and hole
// filling; shinestacker_amd/stereo.py builds pairs, anaglyphs and rocking sequences from it.
//
// The operation (the specification; tests/stereo_restatement.py states it in NumPy and is held bit for bit):
//
// One primitive: `view(image, depth, n_frames, shift, pivot, near)` gives an image of the same shape and type as `image`.
//
// **Inputs**
// - `image`: H x W x 3, uint8 or uint16, BGR.
// - `depth`: H x W float32, frame numbers as `depth_map()` returns them. It may exceed `[0, N-1]` by rounding.
// - `n_frames`: N >= 1.
// - `shift`: float, in pixels, signed, `|shift| <= MAX_SHIFT = 64`, and `ceil(|shift|) < W`.
// - `pivot`: float in [0, 1]. This is the normalised nearness that stays in place, the screen plane.
// - `near`: `'last'` or `'first'`. It says which end of the stack is closest to the viewer.
//
// **Nearness, per source pixel (y, x), all float32, each operation rounded on its own:**
// 1. `t = depth / float32(N - 1)`. This is one correctly rounded divide. `t = 0` when N == 1.
// 2. `t = min(max(t, 0), 1)`.  A NaN depth has nearness `t = 0`, like any depth at or below the first frame.
// 3. If `near == 'first'`: `t = 1 - t`.
//
// **Target:**
// 4. `d = int32(rint(float32(shift) * (t - float32(pivot))))`, round half to even.
// 5. `x' = x + d`. A target outside `[0, W)` is dropped.
//
// **Occlusion.** Among the sources of one row that land on the same `(y, x')`, the one with the largest `t` wins.
// - `d` is a function of `t` alone, so two sources with equal `t` can never collide. No tie rule is needed.
// - `t >= 0`, so its IEEE bits order like the value.
// - The winning source column can be recomputed as `x' - d(t_win)`. A 32-bit maximum per target is therefore enough state.
//
// **Holes.** A target that received no source is filled as follows:
// - Find the nearest target to its left and the nearest to its right, in the same row, that did receive a source.
// - Take the one with the smaller winning `t`, the background. On equal `t` take the left one.
// - If only one side exists, take that side.
// - If neither side exists, take the source pixel `(y, x')` itself.
//
// **Output.** `out[y, x'] = image[y, xs]`, all three channels copied unchanged. No arithmetic is done on pixel values.
//
// Rows are independent. This translation unit is compiled with contraction off, like `kernels_depth.hpp`.
//
// (Implementation notes, not part of the specification: max(t, 0) is written `t > 0 ? t : 0`, which also turns -0 into +0 --
// the same d, and bits that order like the value -- and is what gives a NaN depth its nearness 0.)
//
// stereo_view_kernel: a workgroup of 256 owns MI_SV_SEG = 512 consecutive targets of one output row.
//   1. scatter: every source column that can reach the segment or its hole-search halo -- targets [x0 - 66, x0 + 512 + 66),
//      so sources 64 further out on either side, 772 at most -- computes its t and d from the depth plane in registers and
//      posts bits(t) + 1 with a 32-bit LDS atomic maximum on its target's word (0: no source yet).  Each t is used once by
//      the workgroup, so the nearness is not staged in LDS on its own: the winner word per target is the staged state.
//   2. resolve: a lane per target.  A word that is set gives xs = x' - d(t_win).  A hole walks the words to its left and to
//      its right, at most MI_SV_HALO = 66 each way and never past the row's ends.  That reach is enough: consecutive
//      sources land at most 1 + (max d - min d) <= ceil(|shift|) + 2 targets apart, inside the row or past its ends, and the
//      row's last (first) source lands at most 64 targets left (right) of the row's last (first) target, so a side with no
//      winner inside the reach has none at all.  A whole row can be left without a winner: rint rounds both half-way ends of d
//      outward, so max d - min d can be ceil(|shift|) + 1 = W (pivot 0.5, shift 3, W = 4: d = -2 and +2), and a row whose
//      one half leaves over the left edge and whose other half over the right keeps its own pixels (`at < 0` below).
//      The source columns go to a second LDS array (2 KB; 4.6 KB with the winner words).
//   3. copy: the segment's 512 x 3 samples as 4-byte words (bytes at a ragged head and tail): a lane assembles a word from
//      the 4 / sizeof(T) samples it names -- gathers at x' - d with |d| <= 64, close to coalesced -- and stores it.
// HBM bytes per pixel: depth read 4 (the 260 extra source columns per segment, 1.5x the loads, come from L2: the neighbouring
// segments read them too), image read 3 sizeof(T), view written 3 sizeof(T): 10 B/px for uint8, 16 B/px for uint16.
//
// anaglyph_kernel: out = right view with channel 2 (red) of the left view, a masked merge of 4-byte words, 9 sizeof(T) B/px.
#pragma once
#include "common.hpp"

namespace mi {

#define MI_SV_MAX_SHIFT 64
#define MI_SV_SEG 512                               // targets per workgroup
#define MI_SV_HALO (MI_SV_MAX_SHIFT + 2)            // how far a hole looks for a winner past either end of the segment
#define MI_SV_SPAN (MI_SV_SEG + 2 * MI_SV_HALO)     // winner words per workgroup

// steps 1-3: `denom` = float32(N - 1), 0 for a single frame
__device__ __forceinline__ float sv_nearness(float depth, float denom, int near_first) {
    float t = denom > 0.0f ? depth / denom : 0.0f;
    t = t > 0.0f ? t : 0.0f;
    t = t < 1.0f ? t : 1.0f;
    return near_first ? 1.0f - t : t;
}

// step 4
__device__ __forceinline__ int sv_disp(float t, float shift, float pivot) {
    const float a = t - pivot;
    return (int)rintf(shift * a);
}

template <typename T>
__global__ __launch_bounds__(256) void stereo_view_kernel(const T* __restrict__ img, const float* __restrict__ depth, T* __restrict__ out,
                                                          int width, int nseg, float denom, float shift, float pivot, int near_first) {
    __shared__ uint32_t win[MI_SV_SPAN];            // bits(t) + 1 of the winner of target x0 - MI_SV_HALO + i, 0: none
    __shared__ int src[MI_SV_SEG];                  // the source column of target x0 + k
    const int tid = (int)threadIdx.x;
    const int row = (int)(blockIdx.x / (unsigned)nseg), x0 = (int)(blockIdx.x % (unsigned)nseg) * MI_SV_SEG;
    const int t0 = x0 - MI_SV_HALO;                 // the target of win[0]
    const size_t prow = (size_t)row * (size_t)width;
    for (int i = tid; i < MI_SV_SPAN; i += 256) win[i] = 0u;
    __syncthreads();
    const int s_lo = max(0, t0 - MI_SV_MAX_SHIFT), s_hi = min(width, t0 + MI_SV_SPAN + MI_SV_MAX_SHIFT);
    for (int x = s_lo + tid; x < s_hi; x += 256) {
        const float t = sv_nearness(depth[prow + x], denom, near_first);
        const int xt = x + sv_disp(t, shift, pivot), j = xt - t0;
        if (xt >= 0 && xt < width && j >= 0 && j < MI_SV_SPAN) atomicMax(&win[j], __float_as_uint(t) + 1u);
    }
    __syncthreads();
    const int n_t = min(MI_SV_SEG, width - x0);     // targets this segment really has
    for (int k = tid; k < n_t; k += 256) {
        const int xp = x0 + k, j = k + MI_SV_HALO;
        int at = -1;                                // index into win of the target whose winner is shown
        if (win[j]) {
            at = j;
        } else {
            int l = -1, r = -1;
            for (int m = 1; m <= MI_SV_HALO && xp - m >= 0; ++m)
                if (win[j - m]) { l = j - m; break; }
            for (int m = 1; m <= MI_SV_HALO && xp + m < width; ++m)
                if (win[j + m]) { r = j + m; break; }
            at = l < 0 ? r : (r < 0 ? l : (win[l] <= win[r] ? l : r));
        }
        src[k] = at < 0 ? xp : (t0 + at) - sv_disp(__uint_as_float(win[at] - 1u), shift, pivot);
    }
    __syncthreads();
    constexpr int EPW = 4 / (int)sizeof(T);         // samples per 4-byte word
    const T* __restrict__ srow = img + prow * 3;
    T* __restrict__ o = out + prow * 3 + (size_t)x0 * 3;
    const int n = n_t * 3;
    const int head = min(n, (int)(((4u - (unsigned)((uintptr_t)o & 3u)) & 3u) / sizeof(T)));
    const int words = (n - head) / EPW, tail = head + words * EPW;
    for (int i = tid; i < words; i += 256) {
        const int e = head + i * EPW;
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < EPW; ++q) {
            const int p = (e + q) / 3, c = (e + q) - 3 * p;
            v |= (uint32_t)srow[src[p] * 3 + c] << (8 * (int)sizeof(T) * q);
        }
        *reinterpret_cast<uint32_t*>(o + e) = v;
    }
    if (tid < head + (n - tail)) {                  // at most 3 + 3 samples outside the aligned words
        const int e = tid < head ? tid : tail + (tid - head);
        const int p = e / 3, c = e - 3 * p;
        o[e] = srow[src[p] * 3 + c];
    }
}

template <typename T>
inline void stereo_view_launch(hipStream_t st, const void* img, const float* depth, void* out, int h, int width, int n_frames,
                               float shift, float pivot, int near_first) {
    const int nseg = cdiv(width, MI_SV_SEG);
    hipLaunchKernelGGL((stereo_view_kernel<T>), dim3((unsigned)((size_t)nseg * (size_t)h)), dim3(256), 0, st, (const T*)img, depth, (T*)out,
                       width, nseg, (float)(n_frames - 1), shift, pivot, near_first);
}

// out = right with every third sample, from the third on (BGR channel 2), taken from left; `n_words` whole 4-byte words of
// the frames, the up to 3 bytes after them sample by sample.  All three frames start on a 4-byte boundary.
template <typename T>
__global__ __launch_bounds__(256) void anaglyph_kernel(const T* __restrict__ left, const T* __restrict__ right, T* __restrict__ out,
                                                       size_t n_words, size_t n_samples) {
    constexpr int EPW = 4 / (int)sizeof(T);
    constexpr uint32_t ONE = sizeof(T) == 1 ? 0xffu : 0xffffu;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) {
        const int phase = (int)((i * EPW) % 3);
        uint32_t m = 0;
#pragma unroll
        for (int q = 0; q < EPW; ++q)
            if ((phase + q) % 3 == 2) m |= ONE << (8 * (int)sizeof(T) * q);
        const uint32_t l = reinterpret_cast<const uint32_t*>(left)[i], r = reinterpret_cast<const uint32_t*>(right)[i];
        reinterpret_cast<uint32_t*>(out)[i] = (l & m) | (r & ~m);
    }
    const size_t e = n_words * EPW + i;             // the first lanes also take the ragged tail
    if (i < 4 && e < n_samples) out[e] = (e % 3 == 2 ? left : right)[e];
}

template <typename T>
inline void anaglyph_launch(hipStream_t st, const void* left, const void* right, void* out, size_t n_px) {
    const size_t n_samples = n_px * 3, n_words = n_samples * sizeof(T) / 4;
    hipLaunchKernelGGL((anaglyph_kernel<T>), dim3((unsigned)((n_words + 256) / 256)), dim3(256), 0, st, (const T*)left, (const T*)right,
                       (T*)out, n_words, n_samples);
}

}  // namespace mi
