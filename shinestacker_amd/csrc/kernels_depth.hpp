// kernels_depth.hpp -- the depth map both stackers can report (no reference counterpart): the frame index in focus at each
// pixel, optionally smoothed with the confidence of the decision as the weight.
//
//   weighted smoothing:  out = B(v * w) / B(w) where B(w) > 0, else v;  B = separable Gaussian, BORDER_REFLECT_101
//
// The evaluation order is fixed (tests/depth_restatement.py states it in NumPy and is held bit for bit), in the working type
// F = float for float-32 stacks, double for float-64 stacks:
//   1. p = F(v) * F(w): one multiply (an int32 index converts exactly);
//   2. rows:    acc = 0; for t = 0 .. K-1 ascending: acc = acc + tap[t] * x[reflect101(col - radius + t)], multiply and add
//               rounded separately (this translation unit is compiled with contraction off); p and w take the same taps;
//   3. columns: the same over rows, on the row results;
//   4. one correctly rounded divide, then the cast to float32 (the output type whatever F is).
// The taps come from the host (ws_gaussian_taps below; shinestacker_amd/depth_out.py builds the same numbers): no exp here.
//
// Two launches with an intermediate plane pair.  A radius-48 halo (sigma 16) does not fit an LDS tile of useful size in two
// dimensions, but it does in one:
//   ws_rows   : a workgroup of 256 owns 256 consecutive pixels of one row; v * w and w of the 256 + 2 * radius pixels it needs
//               are staged in LDS once (2.8 KB float, 5.6 KB double), each lane sums K taps from LDS and writes the row sums
//               P = Brow(v * w), Q = Brow(w) (type F).
//   ws_cols   : a lane owns MI_WS_ROWS = 8 consecutive output rows of one column and walks the K + 7 rows of P and Q they need
//               once, top to bottom, feeding each row to the (up to 8) outputs whose window holds it -- every output still
//               receives its taps in ascending order.  Consecutive lanes are consecutive columns: every load is a coalesced
//               row segment, K + 7 loads per 8 outputs instead of 8 K.  The tap index is wave-uniform (a scalar load from
//               the kernel arguments).  The centre v is read only where B(w) is not positive.
// HBM bytes per pixel (float-32 stack, int32 index + float32 energy): rows read 8, write 8; columns read 8 (the vertical
// re-reads of a workgroup's (32 + 2 radius) x 64 window come from L2), write 4: 28 B/px against the 12 B/px minimum of a
// single-launch form; float-64 stacks move 16-byte row sums: 44 B/px.
//
//   dm_depth_index: DepthMapStack's map from the N planes the handle holds after finish (type W):
//               D = (sum_i in_i * i) / total, i ascending, multiply and add separate, 0 where total == 0.  One pass over the
//               planes (N * sizeof(W) B/px read), their addresses in a device table.
#pragma once
#include <cmath>
#include <type_traits>

#include "common.hpp"

namespace mi {

#define MI_WS_MAX_SIGMA 16.0
#define MI_WS_MAX_RADIUS 48         // ceil(3 * 16)
#define MI_WS_MAX_TAPS (2 * MI_WS_MAX_RADIUS + 1)
#define MI_WS_ROWS 8                // output rows per lane of the column pass
#define MI_WS_SEG 256               // pixels per workgroup of the row pass

template <typename F>
struct WsTaps {
    F k[MI_WS_MAX_TAPS];            // wave-uniform reads: scalar loads from the kernel arguments
};

// radius = ceil(3 sigma); K = 2 radius + 1 taps exp(-x^2 / (2 sigma^2)) in double, normalised by their sum accumulated in
// ascending order.  Returns the radius; 0 < sigma <= MI_WS_MAX_SIGMA is the caller's check.
inline int ws_gaussian_taps(double sigma, double* taps) {
    const int radius = (int)std::ceil(3.0 * sigma);
    const int K = 2 * radius + 1;
    double sum = 0.0;
    for (int i = 0; i < K; ++i) {
        const double x = (double)(i - radius);
        taps[i] = std::exp(-(x * x) / (2.0 * sigma * sigma));
        sum += taps[i];
    }
    for (int i = 0; i < K; ++i) taps[i] = taps[i] / sum;
    return radius;
}

// the value plane's element in the working type; an int32 winner index stored in a handle's consecutive numbering turns into
// the global one first (first + k * stride; first = 0, stride = 1 leaves it as it is)
template <typename F, typename TV>
__device__ __forceinline__ F ws_value(TV x, int first, int stride) {
    if constexpr (std::is_same<TV, int32_t>::value) {
        const int32_t g = x >= first ? first + (x - first) * stride : x;
        return (F)g;
    } else {
        return (F)x;
    }
}

// rows: P = Brow(v * w), Q = Brow(w).  w == nullptr: every weight is 1.  radius < width.
template <typename TV, typename TW, typename F>
__global__ __launch_bounds__(MI_WS_SEG) void ws_rows(const TV* __restrict__ v, const TW* __restrict__ w, int h, int width, int radius,
                                                     int first, int stride, WsTaps<F> taps, F* __restrict__ P, F* __restrict__ Q) {
    __shared__ F sp[MI_WS_SEG + 2 * MI_WS_MAX_RADIUS], sw[MI_WS_SEG + 2 * MI_WS_MAX_RADIUS];
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * MI_WS_SEG;
    const size_t row = (size_t)blockIdx.y * (size_t)width;
    const int last = width - 1 + radius;            // the rightmost column any output of this row reads
    for (int i = tid; i < MI_WS_SEG + 2 * radius; i += MI_WS_SEG) {
        const int gx = x0 - radius + i;
        if (gx > last) break;
        const size_t at = row + (size_t)r101(gx, width);
        const F fv = ws_value<F, TV>(v[at], first, stride);
        const F fw = w ? (F)w[at] : (F)1;
        sp[i] = fv * fw;
        sw[i] = fw;
    }
    __syncthreads();
    const int x = x0 + tid;
    if (x >= width) return;
    const int K = 2 * radius + 1;
    F ap = 0, aw = 0;
    for (int t = 0; t < K; ++t) {
        const F k = taps.k[t];
        ap = ap + k * sp[tid + t];
        aw = aw + k * sw[tid + t];
    }
    P[row + x] = ap;
    Q[row + x] = aw;
}

// columns, divide, cast.  radius < h.  Launch: 256 threads = 64 columns x 4 groups of MI_WS_ROWS rows.
template <typename TV, typename F>
__global__ __launch_bounds__(256) void ws_cols(const F* __restrict__ P, const F* __restrict__ Q, const TV* __restrict__ v, int h, int width,
                                               int radius, int first, int stride, WsTaps<F> taps, float* __restrict__ out) {
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * 64 + (tid & 63);
    const int y0 = ((int)blockIdx.y * 4 + (tid >> 6)) * MI_WS_ROWS;     // wave-uniform
    if (x >= width || y0 >= h) return;
    const int K = 2 * radius + 1, last = h - 1 + radius;
    F ap[MI_WS_ROWS], aw[MI_WS_ROWS];
#pragma unroll
    for (int j = 0; j < MI_WS_ROWS; ++j) ap[j] = aw[j] = 0;
    for (int i = 0; i < K + MI_WS_ROWS - 1; ++i) {
        const int gy = y0 - radius + i;
        if (gy > last) break;                       // only rows past the image bottom would still take it
        const size_t at = (size_t)r101(gy, h) * (size_t)width + x;
        const F p = P[at], q = Q[at];
#pragma unroll
        for (int j = 0; j < MI_WS_ROWS; ++j) {
            const int t = i - j;                    // the tap of output row y0 + j that input row gy meets
            if (t >= 0 && t < K) {
                const F k = taps.k[t];
                ap[j] = ap[j] + k * p;
                aw[j] = aw[j] + k * q;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MI_WS_ROWS; ++j) {
        const int y = y0 + j;
        if (y >= h) break;
        const size_t at = (size_t)y * (size_t)width + x;
        out[at] = aw[j] > (F)0 ? (float)(ap[j] / aw[j]) : (float)ws_value<F, TV>(v[at], first, stride);
    }
}

// sigma == 0: the value plane as float32
template <typename TV, typename F>
__global__ __launch_bounds__(256) void ws_passthrough(const TV* __restrict__ v, size_t n, int first, int stride, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)ws_value<F, TV>(v[i], first, stride);
}

// out = B(v w) / B(w) on `st`; taps64: the 2 radius + 1 normalised double taps (rounded once to F here); P, Q: scratch planes
// of h * width elements of F.  0 < radius < min(h, width), radius <= MI_WS_MAX_RADIUS: the caller has checked.
template <typename TV, typename TW, typename F>
inline void ws_smooth_launch(hipStream_t st, const TV* v, const TW* w, int h, int width, int radius, const double* taps64, int first,
                             int stride, F* P, F* Q, float* out) {
    WsTaps<F> taps{};
    for (int i = 0; i < 2 * radius + 1; ++i) taps.k[i] = (F)taps64[i];
    hipLaunchKernelGGL((ws_rows<TV, TW, F>), dim3((unsigned)cdiv(width, MI_WS_SEG), (unsigned)h), dim3(MI_WS_SEG), 0, st, v, w, h, width,
                       radius, first, stride, taps, P, Q);
    hipLaunchKernelGGL((ws_cols<TV, F>), dim3((unsigned)cdiv(width, 64), (unsigned)cdiv(h, 4 * MI_WS_ROWS)), dim3(256), 0, st,
                       (const F*)P, (const F*)Q, v, h, width, radius, first, stride, taps, out);
}

template <typename TV, typename F>
inline void ws_passthrough_launch(hipStream_t st, const TV* v, size_t n, int first, int stride, float* out) {
    hipLaunchKernelGGL((ws_passthrough<TV, F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, v, n, first, stride, out);
}

// DepthMapStack: D = (sum_i planes[i] * i) / total in the planes' type W, 0 where total == 0; stored as TOut (W for the
// smoothing that follows, float for the map itself)
template <typename W, typename TOut>
__global__ __launch_bounds__(256) void dm_depth_index(const W* const* __restrict__ planes, int n, const W* __restrict__ tot, size_t np,
                                                      TOut* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    W acc = 0;
    for (int k = 0; k < n; ++k) {
        const W* __restrict__ e = planes[k];       // wave-uniform: a scalar load
        acc = acc + e[i] * (W)k;
    }
    const W t = tot[i];
    out[i] = (TOut)(t == (W)0 ? (W)0 : acc / t);
}

}  // namespace mi
