// kernels_prestack.hpp -- the per-pixel passes of the corrections the reference applies to a frame before it is aligned:
// Vignetting (algorithms/vignetting.py:23-39 radial_mean_intensity, :71-97 correct_vignetting) and MaskNoise
// (algorithms/noise_detection.py:171-198).  The sigmoid fit between the two vignetting passes (scipy curve_fit / fsolve on
// r_steps numbers) stays on the host, shinestacker_amd/vignetting.py.
//
//   radial_ring_sums   integer sum and count of the sub-sampled 8-bit gray image per radial ring; the gray image itself is
//                      never written.  Order as vignetting.py:52-55: 8-bit first (img >> 8 for 16-bit), integer BGR2GRAY,
//                      THEN the sub-sampling of the one-channel image (the balance histogram and the ECC gray sub-sample
//                      BGR first; the two orders differ in integer arithmetic).
//   vignette_apply     image / gain in float64, gain = clip(sigmoid(r) / v0, 1e-6, 1) blended by max_correction, 1 where
//                      min(B, G, R) < threshold; clip, truncate.  One gain per pixel.
//   mask_noise_apply   mean / median of the non-zero values of the uncorrected channel around each hot pixel.
#pragma once
#include "common.hpp"
#include "kernels_balance.hpp"   // bgr2gray_int

namespace mi {

// ---------------------------------------------------------------- radial_ring_sums
#define MI_MAX_RINGS 2048

struct RingArgs {
    const void* img;        // H x W x 3, uint8 / uint16
    int h, w;               // full-resolution size
    int hs, ws;             // size of the sub-sampled gray image
    int s, fast;            // factor; img[::s, ::s] instead of the area mean
    int r_steps;
    const double* radii;    // [r_steps + 1], np.linspace(0, r_max, r_steps + 1) of the SUB-SAMPLED image
    double cx, cy;          // ws / 2, hs / 2
    double per_r;           // r_steps / r_max: the first guess of the ring
    unsigned long long* sums;   // [r_steps], zeroed by the caller
    uint32_t* counts;           // [r_steps], zeroed by the caller
};

// 8-bit gray of full-resolution pixel p (3 values): img_8bit then cv2.cvtColor(BGR2GRAY)
template <typename T>
__device__ __forceinline__ uint32_t gray8(const T* p) {
    constexpr int sh = sizeof(T) == 1 ? 0 : 8;
    return bgr2gray_int((uint32_t)p[0] >> sh, (uint32_t)p[1] >> sh, (uint32_t)p[2] >> sh);
}

// value of sub-sampled gray pixel (sy, sx)
template <typename T>
__device__ __forceinline__ uint32_t ring_pixel(const RingArgs& a, int sy, int sx) {
    const T* img = (const T*)a.img;
    if (a.s == 1 || a.fast) return gray8(img + ((size_t)sy * a.s * a.w + (size_t)sx * a.s) * 3);
    const int ny = min(a.s, a.h - sy * a.s), nx = min(a.s, a.w - sx * a.s);
    uint32_t sum = 0;
    for (int dy = 0; dy < ny; ++dy) {
        const T* row = img + ((size_t)(sy * a.s + dy) * a.w + (size_t)sx * a.s) * 3;
        for (int dx = 0; dx < nx; ++dx) sum += gray8(row + dx * 3);
    }
    return area_mean_int(sum, ny * nx, a.s);
}

// the ring i with radii[i] <= d < radii[i + 1] (vignetting.py:34), -1 when d >= radii[r_steps] (d == r_max: a corner pixel).
// (x - w/2)^2 + (y - h/2)^2 is an exact multiple of 0.25 and the float64 sqrt is correctly rounded, so d is the reference's
// number bit for bit; the guess d * r_steps / r_max is then moved until the table itself agrees.
__device__ __forceinline__ int ring_of(const RingArgs& a, int sy, int sx) {
    const double dx = (double)sx - a.cx, dy = (double)sy - a.cy;
    const double d = sqrt(dx * dx + dy * dy);
    int i = (int)(d * a.per_r);
    i = i < 0 ? 0 : (i > a.r_steps - 1 ? a.r_steps - 1 : i);
    while (i > 0 && d < a.radii[i]) --i;
    while (i < a.r_steps && d >= a.radii[i + 1]) ++i;
    return i < a.r_steps ? i : -1;
}

// One sub-sampled pixel per lane and step.  Neighbouring lanes are neighbouring pixels and mostly share a ring: a wave whose
// live lanes all agree adds its 64 values with shuffles and issues one LDS atomic pair; a wave that straddles a ring border
// falls back to one LDS atomic pair per lane.  Per workgroup one global atomic pair per ring it touched.  The workgroup's
// partial sums stay below 2^32: it sees at most total / gridDim.x + 256 <= 2^21 pixels of at most 255 (capi.hip sizes the grid).
template <typename T>
__global__ __launch_bounds__(256) void radial_ring_sums(RingArgs a) {
    __shared__ uint32_t sh_sum[MI_MAX_RINGS], sh_cnt[MI_MAX_RINGS];
    for (int i = threadIdx.x; i < a.r_steps; i += blockDim.x) { sh_sum[i] = 0; sh_cnt[i] = 0; }
    __syncthreads();
    const size_t total = (size_t)a.hs * a.ws, stride = (size_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (size_t base = (size_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < total; base += stride) {   // wave-uniform
        const size_t i = base + lane;
        int ring = -1;
        uint32_t v = 0;
        if (i < total) {
            const int sy = (int)(i / a.ws), sx = (int)(i - (size_t)sy * a.ws);
            ring = ring_of(a, sy, sx);
            if (ring >= 0) v = ring_pixel<T>(a, sy, sx);
        }
        const unsigned long long live = __ballot(ring >= 0);
        if (!live) continue;
        const int r0 = __shfl(ring, __ffsll((long long)live) - 1);
        if (__all(ring < 0 || ring == r0)) {
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) { atomicAdd(&sh_sum[r0], v); atomicAdd(&sh_cnt[r0], (uint32_t)__popcll(live)); }
        } else if (ring >= 0) {
            atomicAdd(&sh_sum[ring], v);
            atomicAdd(&sh_cnt[ring], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.r_steps; i += blockDim.x)
        if (sh_cnt[i]) { atomicAdd(&a.sums[i], (unsigned long long)sh_sum[i]); atomicAdd(&a.counts[i], sh_cnt[i]); }
}

// ---------------------------------------------------------------- vignette_apply
struct VignArgs {
    int h, w;
    double cx, cy;                    // w / 2, h / 2
    double i0, k, r0, v0;             // sigmoid_model's parameters (full-resolution pixels) and sigmoid(0)
    double max_correction, threshold; // threshold: black_threshold, x 256 for 16-bit
};

#define MI_VIGN_CLIP_EXP 10.0   // vignetting.py:13

// vignetting.py:16-20 and :86-89, float64, one rounding per written operation (contraction is off in this library):
// i0 / (1 + exp(min(CLIP_EXP, exp(clip(k (r - r0), -CLIP_EXP, CLIP_EXP))))) / v0, clipped to [1e-6, 1], then blended
__device__ __forceinline__ double vignette_gain(const VignArgs& a, int x, int y) {
    const double dx = (double)x - a.cx, dy = (double)y - a.cy;
    const double r = sqrt(dx * dx + dy * dy);
    double t = a.k * (r - a.r0);
    t = t < -MI_VIGN_CLIP_EXP ? -MI_VIGN_CLIP_EXP : (t > MI_VIGN_CLIP_EXP ? MI_VIGN_CLIP_EXP : t);
    double e = exp(t);
    e = e > MI_VIGN_CLIP_EXP ? MI_VIGN_CLIP_EXP : e;
    double g = (a.i0 / (1.0 + exp(e))) / a.v0;
    g = g < 1e-6 ? 1e-6 : (g > 1.0 ? 1.0 : g);
    if (a.max_correction < 1.0) g = (1.0 - a.max_correction) + g * a.max_correction;
    return g;
}

template <typename T>
__device__ __forceinline__ void vignette_pixel(const VignArgs& a, T* e, int x, int y) {
    const T mn = min(min(e[0], e[1]), e[2]);
    if ((double)mn < a.threshold) return;        // gain forced to 1 (vignetting.py:93): value / 1 is the value
    const double g = vignette_gain(a, x, y);
    if (g == 1.0) return;
    constexpr double vmax = sizeof(T) == 1 ? 255.0 : 65535.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double o = (double)e[c] / g;             // a true division, as numpy's: a reciprocal would round twice
        o = o > vmax ? vmax : o;                 // (o >= 0 always)
        e[c] = (T)o;                             // astype: truncation
    }
}

// One thread owns a span of 48 bytes = 16 uint8 or 8 uint16 whole pixels: three 16-byte loads, three 16-byte stores.
// In place is allowed: a thread reads its span before it writes it and no other thread touches it.
template <typename T>
__global__ __launch_bounds__(256) void vignette_apply(const T* src, T* dst, VignArgs a) {
    constexpr int PIX = 48 / (3 * (int)sizeof(T));
    const size_t npix = (size_t)a.h * a.w, nspan = npix / PIX;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nspan; q += (size_t)gridDim.x * blockDim.x) {
        union { uint4 v[3]; T e[PIX * 3]; } u;
        const uint4* s4 = (const uint4*)src + 3 * q;
        u.v[0] = s4[0]; u.v[1] = s4[1]; u.v[2] = s4[2];
        const size_t p = q * PIX;
        int y = (int)(p / a.w), x = (int)(p - (size_t)y * a.w);
#pragma unroll
        for (int i = 0; i < PIX; ++i) {
            vignette_pixel<T>(a, u.e + 3 * i, x, y);
            if (++x == a.w) { x = 0; ++y; }
        }
        uint4* d4 = (uint4*)dst + 3 * q;
        d4[0] = u.v[0]; d4[1] = u.v[1]; d4[2] = u.v[2];
    }
    // fewer than PIX pixels left
    if (blockIdx.x == 0)
        for (size_t p = nspan * PIX + threadIdx.x; p < npix; p += blockDim.x) {
            T e[3] = {src[p * 3], src[p * 3 + 1], src[p * 3 + 2]};
            const int y = (int)(p / a.w);
            vignette_pixel<T>(a, e, (int)(p - (size_t)y * a.w), y);
            dst[p * 3] = e[0]; dst[p * 3 + 1] = e[1]; dst[p * 3 + 2] = e[2];
        }
}

// ---------------------------------------------------------------- mask_noise_apply
enum { MASK_NOISE_MEAN = 0, MASK_NOISE_MEDIAN = 1 };

// One thread per (hot pixel, channel): noise_detection.py:187-197.  The window [y - ks2, y + ks2] x [x - ks2, x + ks2] is
// clipped to the image, only NON-ZERO values of the uncorrected channel count (the hot pixel's own value among them), and
// the float result is assigned into the integer image, i.e. truncated.  In integers that is exact:
//   MEAN    np.mean = float64(sum) / n, truncated = sum / n (integer division): sum < 2^32, so a quotient that is not
//           whole lies at least 1 / n from the next integer, far more than a float64 rounding;
//   MEDIAN  np.median = the middle value, or the float mean of the two middle values, truncated = (a + b) >> 1.
// The k-th smallest value is found by bisection on the value range (count of window values <= mid), so no window buffer
// and no limit on kernel_size.  No valid value: the pixel keeps its value.
// Results go to `stage` ([n][3] uint32); mask_noise_store writes them afterwards, so a hot pixel in another hot pixel's
// window is read uncorrected, in place included.
template <typename T>
__device__ __forceinline__ uint32_t window_kth(const T* src, int w, int y0, int y1, int x0, int x1, int c, uint32_t k) {
    uint32_t lo = 1, hi = sizeof(T) == 1 ? 255u : 65535u;   // smallest v with #{0 < p <= v} >= k + 1
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        uint32_t cnt = 0;
        for (int yy = y0; yy < y1; ++yy)
            for (int xx = x0; xx < x1; ++xx) {
                const uint32_t p = src[((size_t)yy * w + xx) * 3 + c];
                cnt += (p != 0 && p <= mid) ? 1u : 0u;
            }
        if (cnt >= k + 1) hi = mid; else lo = mid + 1;
    }
    return lo;
}

template <typename T>
__global__ __launch_bounds__(256) void mask_noise_apply(const T* __restrict__ src, int h, int w, const int32_t* __restrict__ coords,
                                                        int n, int ks2, int method, uint32_t* __restrict__ stage) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    const int i = t / 3, c = t - 3 * i;
    const int y = coords[2 * i], x = coords[2 * i + 1];
    if (y < 0 || y >= h || x < 0 || x >= w) { stage[t] = 0xffffffffu; return; }   // a mask of another size: never out of bounds
    const int y0 = max(0, y - ks2), y1 = min(h, y + ks2 + 1), x0 = max(0, x - ks2), x1 = min(w, x + ks2 + 1);
    unsigned long long sum = 0;
    uint32_t cnt = 0;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) {
            const uint32_t p = src[((size_t)yy * w + xx) * 3 + c];
            sum += p;
            cnt += p != 0 ? 1u : 0u;
        }
    uint32_t out = src[((size_t)y * w + x) * 3 + c];
    if (cnt) {
        if (method == MASK_NOISE_MEAN) out = (uint32_t)(sum / cnt);
        else if (cnt & 1u) out = window_kth<T>(src, w, y0, y1, x0, x1, c, cnt / 2);
        else out = (window_kth<T>(src, w, y0, y1, x0, x1, c, cnt / 2 - 1) + window_kth<T>(src, w, y0, y1, x0, x1, c, cnt / 2)) >> 1;
    }
    stage[t] = out;
}

template <typename T>
__global__ __launch_bounds__(256) void mask_noise_store(T* __restrict__ dst, int w, const int32_t* __restrict__ coords, int n,
                                                        const uint32_t* __restrict__ stage) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 3) return;
    const int i = t / 3, c = t - 3 * i;
    if (stage[t] != 0xffffffffu) dst[((size_t)coords[2 * i] * w + coords[2 * i + 1]) * 3 + c] = (T)stage[t];
}

// ---------------------------------------------------------------- NoiseDetection (noise_detection.py:21-45, :100-104)
// frame_accumulate: sum[i] += frames[0][i] + ... + frames[n - 1][i] over uint8 frames, uint32 sums (exact below 2^24 frames;
// the host refuses more).  Four elements per thread and step, dword loads of the frames, a 16-byte read-modify-write of the sums.
__global__ __launch_bounds__(256) void frame_accumulate(const uint8_t* __restrict__ frames, int n, size_t per_frame,
                                                        uint32_t* __restrict__ sum) {
    const size_t nq = per_frame / 4;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (size_t)gridDim.x * blockDim.x) {
        uint4 acc = ((const uint4*)sum)[q];
        for (int f = 0; f < n; ++f) {
            const uint32_t v = ((const uint32_t*)(frames + (size_t)f * per_frame))[q];
            acc.x += v & 255u; acc.y += (v >> 8) & 255u; acc.z += (v >> 16) & 255u; acc.w += v >> 24;
        }
        ((uint4*)sum)[q] = acc;
    }
    if (blockIdx.x == 0)
        for (size_t i = nq * 4 + threadIdx.x; i < per_frame; i += blockDim.x) {
            uint32_t a = sum[i];
            for (int f = 0; f < n; ++f) a += frames[(size_t)f * per_frame + i];
            sum[i] = a;
        }
}

// hot_pixel_map: from the sum image and the frame count, in one launch:
//   mean  = sum / n, integer division = the reference's float64 divide and truncating cast to uint8 (noise_detection.py:45);
//   blur  = cv2.GaussianBlur(mean, (k, k), 0) for k = 3, 5, 7 [from memory -- parity unpinned]: for these sizes and sigma 0
//           OpenCV takes its fixed small kernel ([1 2 1] / 4, [1 4 6 4 1] / 16, [2 7 14 18 14 7 2] / 64), which its 8-bit path
//           holds exactly in 8.8 fixed point, so nothing rounds before the end and the result is
//           (F^2 * sum_ij w_i w_j p_ij + 2^15) >> 16 with the integer weights w and F = 256 / sum(w); BORDER_REFLECT101;
//   diff  = |mean - blur|, hot_c = diff_c > threshold_c, map = 255 where any channel is hot (cv2.absdiff / threshold /
//           bitwise_or), counts = number of hot pixels in (map, channel 0, channel 1, channel 2).
// 16 x 16 pixels per workgroup; the mean tile with a k / 2 halo is staged in LDS once for the three channels.
#define MI_HOT_TILE 16
#define MI_HOT_MAX_R 3

struct HotArgs {
    const uint32_t* sum;   // H x W x 3
    int h, w, n;           // n frames were added
    int r;                 // blur_size / 2: 1, 2, 3
    int wt[2 * MI_HOT_MAX_R + 1];
    int f2;                // (256 / sum(wt))^2
    int th[3];
    uint8_t* mean;         // H x W x 3 out (may be null)
    uint8_t* map;          // H x W out
    uint32_t* counts;      // [4], zeroed by the caller
};

__global__ __launch_bounds__(MI_HOT_TILE * MI_HOT_TILE) void hot_pixel_map(HotArgs a) {
    constexpr int S = MI_HOT_TILE + 2 * MI_HOT_MAX_R;
    __shared__ uint8_t tile[S * S * 3];
    __shared__ uint32_t cnt[4];
    const int tid = threadIdx.y * MI_HOT_TILE + threadIdx.x;
    if (tid < 4) cnt[tid] = 0;
    const int side = MI_HOT_TILE + 2 * a.r;
    const int x0 = blockIdx.x * MI_HOT_TILE - a.r, y0 = blockIdx.y * MI_HOT_TILE - a.r;
    for (int i = tid; i < side * side; i += MI_HOT_TILE * MI_HOT_TILE) {
        const int ty = i / side, tx = i - ty * side;
        const int yy = r101_loop(y0 + ty, a.h), xx = r101_loop(x0 + tx, a.w);
        const uint32_t* p = a.sum + ((size_t)yy * a.w + xx) * 3;
        for (int c = 0; c < 3; ++c) tile[(ty * S + tx) * 3 + c] = (uint8_t)(p[c] / (uint32_t)a.n);
    }
    __syncthreads();
    const int x = blockIdx.x * MI_HOT_TILE + threadIdx.x, y = blockIdx.y * MI_HOT_TILE + threadIdx.y;
    if (x < a.w && y < a.h) {
        bool any = false;
        for (int c = 0; c < 3; ++c) {
            int acc = 0;
            for (int j = 0; j <= 2 * a.r; ++j) {
                int row = 0;
                for (int i = 0; i <= 2 * a.r; ++i) row += a.wt[i] * tile[((threadIdx.y + j) * S + threadIdx.x + i) * 3 + c];
                acc += a.wt[j] * row;
            }
            const int blur = (acc * a.f2 + (1 << 15)) >> 16;
            const int m = tile[((threadIdx.y + a.r) * S + threadIdx.x + a.r) * 3 + c];
            if (a.mean) a.mean[((size_t)y * a.w + x) * 3 + c] = (uint8_t)m;
            const int d = m > blur ? m - blur : blur - m;
            if (d > a.th[c]) { any = true; atomicAdd(&cnt[1 + c], 1u); }
        }
        a.map[(size_t)y * a.w + x] = any ? 255 : 0;
        if (any) atomicAdd(&cnt[0], 1u);
    }
    __syncthreads();
    if (tid < 4 && cnt[tid]) atomicAdd(&a.counts[tid], cnt[tid]);
}

}  // namespace mi
