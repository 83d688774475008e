// kernels_unsharp.hpp -- the reference's unsharp mask (algorithms/sharpen.py) on a three-channel frame, blur and combine in one
// pass: the blurred frame exists only in LDS.
//
//   blurred = cv2.GaussianBlur(image, (0, 0), radius): OpenCV's bit-exact fixed-point separable path as oracle/align_oracle.c
//             states it [from memory, unpinned] -- taps with 8 (uint8) / 16 (uint16) fractional bits that sum to exactly 1.0,
//             exact integer row sums R (8.8 / 16.16) and column sums S (16.16 / 32.32), (S + half) >> 16 / 32, saturated,
//             BORDER_REFLECT_101 reflected as often as it takes.  The taps come from the caller (shinestacker_amd/sharpen.py):
//             no exp is evaluated here.
//   threshold == 0:  cv2.addWeighted(image, 1 + amount, blurred, -amount, 0) in float32: each product rounded, their sum rounded
//             (no fused multiply-add: __fmul_rn / __fadd_rn are never contracted), rounded half to even, saturated
//   threshold != 0:  the reference's NumPy lines: diff = f32(image) - f32(blurred); where |diff| > threshold the value is
//             f32(image) + f32(amount) * diff (both rounded to float32), clipped to the range and TRUNCATED; elsewhere the input
//
// One workgroup of 256 owns a 32 x 32 pixel tile (96 interleaved samples per row).  With r = ksize / 2:
//   1. the tile and its halo of r pixels, (32 + 2r) x (32 + 2r) x 3 samples of the input type, are staged in LDS;
//   2. the row pass writes (32 + 2r) x 96 row sums to a second LDS plane: uint16 for uint8 frames (R <= 255 * 256), uint32 for
//      uint16 frames (R <= 65535 * 65536);
//   3. the column pass reads that plane with consecutive lanes on consecutive words (no bank conflict: the flat output index is
//      the flat word index plus a wave-uniform offset).  uint8: a lane takes one 32-bit word = two adjacent row sums, 32-bit
//      sums throughout (S < 2^24).  uint16: S needs 48 bits; it is carried as two 32-bit halves, S = (sum k * (R >> 16)) << 16
//      + sum k * (R & 0xffff), each half < 2^32 because the taps sum to 2^16 -- two 32-bit multiply-adds per tap in place of
//      one 64-bit multiply-add and a 64-bit register pair;
//   4. the combine takes the centre sample from the staged tile; 5. the store is one coalesced run of samples per row.
// LDS per workgroup: (32 + 2r)^2 * 3 * size + (32 + 2r) * 96 * (2 | 4) bytes -- uint8 ksize 7: 11.4 KB, ksize 25: 19.7 KB;
// uint16 ksize 9: 24.4 KB, ksize 33: 48 KB (3 workgroups = 12 waves per CU of the 160 KB; the smaller windows reach the
// 8-workgroup / 32-wave cap).
#pragma once
#include "common.hpp"

namespace mi {

#define MI_UNSHARP_TILE 32
#define MI_UNSHARP_MAX_KSIZE 33     // radius 4.0 on uint16: cvRound(4 * 8 + 1) | 1

struct UnsharpArgs {
    const void* src;        // H x W x 3
    void* dst;              // H x W x 3, != src
    int h, w;
    int ksize;              // odd, <= MI_UNSHARP_MAX_KSIZE
    int masked;             // 0: the addWeighted branch; 1: the thresholded branch
    float alpha, beta;      // float32(1 + amount), float32(-amount)
    float amount, threshold;
    uint32_t taps[MI_UNSHARP_MAX_KSIZE];    // wave-uniform reads: scalar loads from the kernel arguments
};

// cv::borderInterpolate(p, len, BORDER_REFLECT_101): any p ends inside [0, len)
__device__ __forceinline__ int unsharp_reflect101(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

template <typename T> struct UnsharpPix;
template <> struct UnsharpPix<uint8_t> {
    using Mid = uint16_t;
    static constexpr int MAXV = 255;
};
template <> struct UnsharpPix<uint16_t> {
    using Mid = uint32_t;
    static constexpr int MAXV = 65535;
};

// the two combines, on the centre sample v and the blurred sample b (both <= MAXV)
template <int MAXV>
__device__ __forceinline__ uint32_t unsharp_combine(const UnsharpArgs& a, uint32_t v, uint32_t b) {
    const float fv = (float)v, fb = (float)b;
    if (!a.masked) {
        const float r = rintf(__fadd_rn(__fmul_rn(a.alpha, fv), __fmul_rn(a.beta, fb)));    // rintf: half to even
        return (uint32_t)fminf(fmaxf(r, 0.0f), (float)MAXV);
    }
    const float diff = fv - fb;                 // exact: integers below 2^17
    if (!(fabsf(diff) > a.threshold)) return v;
    const float r = __fadd_rn(fv, __fmul_rn(a.amount, diff));
    return (uint32_t)fminf(fmaxf(r, 0.0f), (float)MAXV);    // clip, then truncate
}

inline size_t unsharp_lds_bytes(int dtype, int ksize) {
    const size_t side = MI_UNSHARP_TILE + 2 * (size_t)(ksize / 2);
    const size_t src = side * side * 3 * (dtype == MI_U8 ? 1 : 2), mid = side * MI_UNSHARP_TILE * 3 * (dtype == MI_U8 ? 2 : 4);
    return ((src + 15) & ~(size_t)15) + mid;
}

template <typename T>
__global__ __launch_bounds__(256) void unsharp_mask_kernel(UnsharpArgs a) {
    using Mid = typename UnsharpPix<T>::Mid;
    constexpr int TILE = MI_UNSHARP_TILE, TWS = TILE * 3, MAXV = UnsharpPix<T>::MAXV;
    extern __shared__ uint4 unsharp_smem[];
    const int r = a.ksize / 2, side = TILE + 2 * r, sws = side * 3;     // staged rows; staged samples per row
    T* tile = (T*)unsharp_smem;                                         // side x sws, origin (tile - r)
    Mid* mid = (Mid*)((char*)unsharp_smem + (((size_t)side * sws * sizeof(T) + 15) & ~(size_t)15));   // side x TWS row sums
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty0 = (int)blockIdx.y * TILE, tx0 = (int)blockIdx.x * TILE;
    const T* src = (const T*)a.src;

    // 1. stage: a wave per row, lanes along the interleaved samples
    for (int ly = wave; ly < side; ly += 4) {
        const T* row = src + (size_t)unsharp_reflect101(ty0 + ly - r, a.h) * a.w * 3;
        for (int ls = lane; ls < sws; ls += 64) {
            const int px = ls / 3, c = ls - px * 3;
            tile[ly * sws + ls] = row[unsharp_reflect101(tx0 + px - r, a.w) * 3 + c];
        }
    }
    __syncthreads();

    // 2. rows: mid[ly][ox] = sum_j k[j] * tile[ly][ox + 3 j]
    for (int i = tid; i < side * TWS; i += 256) {
        const int ly = i / TWS, ox = i - ly * TWS;
        const T* p = tile + ly * sws + ox;
        uint32_t sum = 0;
        for (int j = 0; j < a.ksize; ++j) sum += a.taps[j] * (uint32_t)p[3 * j];
        mid[i] = (Mid)sum;
    }
    __syncthreads();

    // 3.-5. columns, combine, store
    T* dst = (T*)a.dst;
    if constexpr (sizeof(T) == 1) {
        const uint32_t* mid2 = (const uint32_t*)mid;        // two adjacent row sums per word
        for (int i = tid; i < TILE * (TWS / 2); i += 256) {
            const int y = i / (TWS / 2), x = (i - y * (TWS / 2)) * 2;
            uint32_t s0 = 0, s1 = 0;
            for (int j = 0; j < a.ksize; ++j) {
                const uint32_t wd = mid2[j * (TWS / 2) + i], k = a.taps[j];
                s0 += k * (wd & 0xffffu);
                s1 += k * (wd >> 16);
            }
            const int gy = ty0 + y, gs = tx0 * 3 + x;
            if (gy >= a.h) continue;
            const T* ctr = tile + (y + r) * sws + 3 * r + x;
            T* o = dst + (size_t)gy * a.w * 3 + gs;
            if (gs < a.w * 3) o[0] = (T)unsharp_combine<MAXV>(a, ctr[0], min((s0 + 32768u) >> 16, (uint32_t)MAXV));
            if (gs + 1 < a.w * 3) o[1] = (T)unsharp_combine<MAXV>(a, ctr[1], min((s1 + 32768u) >> 16, (uint32_t)MAXV));
        }
    } else {
        for (int i = tid; i < TILE * TWS; i += 256) {
            const int y = i / TWS, x = i - y * TWS;
            uint32_t hi = 0, lo = 0;
            for (int j = 0; j < a.ksize; ++j) {
                const uint32_t wd = mid[j * TWS + i], k = a.taps[j];
                hi += k * (wd >> 16);
                lo += k * (wd & 0xffffu);
            }
            // S = hi * 2^16 + lo; (S + 2^31) >> 32 == (t + 2^15) >> 16 with t = hi + (lo >> 16) <= 2^32 - 1
            const uint32_t t = hi + (lo >> 16);
            const uint32_t b = min(((t >> 15) + 1u) >> 1, (uint32_t)MAXV);
            const int gy = ty0 + y, gs = tx0 * 3 + x;
            if (gy < a.h && gs < a.w * 3)
                dst[(size_t)gy * a.w * 3 + gs] = (T)unsharp_combine<MAXV>(a, tile[(y + r) * sws + 3 * r + x], b);
        }
    }
}

// ksize odd and <= MI_UNSHARP_MAX_KSIZE, taps summing to 1 << (8 | 16); the caller has validated everything
inline void unsharp_launch(hipStream_t st, const void* src, void* dst, int h, int w, int dtype, const uint32_t* taps, int ksize,
                           double amount, double threshold) {
    UnsharpArgs a{};
    a.src = src; a.dst = dst; a.h = h; a.w = w; a.ksize = ksize;
    a.masked = threshold != 0.0 ? 1 : 0;
    a.alpha = (float)(1.0 + amount);
    a.beta = (float)(-amount);
    a.amount = (float)amount;
    a.threshold = (float)threshold;
    for (int j = 0; j < ksize; ++j) a.taps[j] = taps[j];
    const size_t lds = unsharp_lds_bytes(dtype, ksize);
    const dim3 grid((unsigned)cdiv(w, MI_UNSHARP_TILE), (unsigned)cdiv(h, MI_UNSHARP_TILE));
    if (dtype == MI_U8) hipLaunchKernelGGL((unsharp_mask_kernel<uint8_t>), grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((unsharp_mask_kernel<uint16_t>), grid, dim3(256), lds, st, a);
}

}  // namespace mi
