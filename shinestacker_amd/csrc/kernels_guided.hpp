// kernels_guided.hpp -- edge-aware refinement of the depth map (no reference counterpart): the confidence-weighted guided
// filter of He, Sun and Tang, with the fused frame's grey as the guide.  A local linear model depth ~ a * I + b is fitted in
// every (2 r + 1)^2 window under the weights w, and the models covering a pixel are averaged:
//
//   grey      g = (1868 B + 9617 G + 4899 R + 8192) >> 14 on the native samples (feat_gray's integer grey without its >> 8);
//             I = double(g) / 255.0 (8 bit) or / 65535.0 (16 bit)
//   products  P = double(p), Wd = double(w);  t1 = Wd * I, t2 = Wd * P, t3 = t1 * I, t4 = t1 * P
//   box sum   B(x): rows first, then columns.  R(y, x) = sum over k = -r .. r ascending of x(y, x + k): the accumulator starts
//             at +0.0, acc = acc + term, a term outside the frame is +0.0; B(x)(y, x) is the same sum over R(y + k, x).
//             (An accumulator that starts at +0.0 never becomes -0.0, so leaving an outside term out gives the same bits.)
//   model     sw = B(Wd), swI = B(t1), swp = B(t2), swII = B(t3), swIp = B(t4).  Where sw > 0:
//             mI = swI / sw, mp = swp / sw, var = swII / sw - mI * mI, cov = swIp / sw - mI * mp, a = cov / (var + eps),
//             b = mp - a * mI; elsewhere a = 0, b = P
//   output    n = double(rows of the window inside the frame * columns of it inside the frame);
//             q = (B(a) / n) * I + B(b) / n;  q = q < lo ? lo : q;  q = q > hi ? hi : q;  out = float(q)
//
// Everything is float64 and every operation is rounded on its own (contraction is off for the library and again below);
// tests/guided_restatement.py states the same in NumPy and the kernels are held to it bit for bit.  The order of the taps is
// the specification: a running sum or an integral image adds in another order and is not bit-equal.
//
// Four launches.  A radius-32 halo of five float64 planes does not fit an LDS tile in two dimensions; it does in one:
//   gf_rows_products  a workgroup of 256 owns MI_GF_SEG = 512 consecutive pixels of one row, a lane two neighbours.  The guide's
//                     bytes of the segment and its halo come in as aligned 16-byte loads into LDS (the few bytes of a chunk
//                     that crosses an end of the buffer one by one), the five products of the MI_GF_SEG + 2 r pixels are staged
//                     in LDS with +0.0 outside the frame, and a lane walks its r + 1 aligned pairs (ds_read_b128) -- every
//                     value feeds both of its sums, each in ascending order -- and writes five 16-byte row sums.
//   gf_cols_model     a lane owns MI_GF_ROWS = 8 consecutive output rows of one column (the ws_cols scheme) and walks the
//                     2 r + 8 rows of the five planes once, top to bottom; consecutive lanes are consecutive columns, every
//                     load a coalesced 512-byte row segment and no LDS at all.  Finishes the sums, writes a and b.
//   gf_rows_ab        the row pass over a and b.
//   gf_cols_out       the column pass over their row sums; re-derives I from the guide, combines, clamps, writes float32.
// Scratch: seven float64 planes (five row sums, a, b; the row sums of a and b reuse the first two).
// HBM bytes per pixel (8-bit guide, float32 weight): 11 read + 40 written; 40 + 4 read, 16 written; 16 read, 16 written;
// 16 + 3 read, 4 written: 166 B/px (the vertical re-reads of a workgroup's window come from L2).
#pragma once
#include "common.hpp"

#pragma clang fp contract(off)

namespace mi {

#define MI_GF_MAX_RADIUS 32
#define MI_GF_SEG 512               // pixels per workgroup of a row pass: two per lane
#define MI_GF_ROWS 8                // output rows per lane of a column pass
#define MI_GF_PLANES 7              // float64 scratch planes of one call

// the staged length of one LDS row: MI_GF_SEG outputs and the halo on both sides (the last lane's last pair ends there)
#define MI_GF_LDS (MI_GF_SEG + 2 * MI_GF_MAX_RADIUS)
// the guide's bytes of one staged row: three 16-bit samples a pixel, up to 15 bytes of lead and a whole last chunk
#define MI_GF_RAW ((MI_GF_SEG + 2 * MI_GF_MAX_RADIUS) * 6 + 32)

template <typename T>
__device__ __forceinline__ double gf_intensity(uint32_t b, uint32_t g, uint32_t r) {
#pragma clang fp contract(off)
    const uint32_t grey = (b * 1868u + g * 9617u + r * 4899u + (1u << 13)) >> 14;
    return (double)grey / (sizeof(T) == 1 ? 255.0 : 65535.0);
}

// The bytes [lo, hi) of the buffer at `g` (`total` bytes long, lo < hi <= total) into `raw`, so that byte lo lands at
// raw[(g + lo) & 15]: aligned 16-byte chunks; a chunk that is not wholly inside the buffer is read byte by byte, and what
// lies outside is not read at all.  raw: 16-byte aligned, at least hi - lo + 31 bytes.
__device__ __forceinline__ void gf_stage_bytes(const uint8_t* __restrict__ g, size_t lo, size_t hi, size_t total,
                                               uint8_t* __restrict__ raw, int tid, int nt) {
    const uintptr_t base = (uintptr_t)g, end = base + total;
    const uintptr_t a0 = (base + lo) & ~(uintptr_t)15;
    const int chunks = (int)((base + hi - a0 + 15) >> 4);
    for (int c = tid; c < chunks; c += nt) {
        const uintptr_t a = a0 + ((uintptr_t)c << 4);
        if (a >= base && a + 16 <= end) {
            *(uint4*)(raw + 16 * c) = *(const uint4*)a;
        } else {
            for (int k = 0; k < 16; ++k) {
                const uintptr_t q = a + (uintptr_t)k;
                raw[16 * c + k] = (q >= base && q < end) ? *(const uint8_t*)q : (uint8_t)0;
            }
        }
    }
}

// One lane's two row sums of every plane: s[k][0 .. n) holds the row from column x0 - radius on, the lane owns the outputs
// x0 + 2 t and x0 + 2 t + 1 and reads the r + 1 aligned pairs s[k][2 t + 2 m], s[k][2 t + 2 m + 1].
template <int NP>
__device__ __forceinline__ void gf_row_sums(const double (*s)[MI_GF_LDS], int t, int radius, double (*acc)[2]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k][0] = acc[k][1] = 0.0;
    for (int m = 0; m <= radius; ++m) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const double2 v = *(const double2*)&s[k][2 * t + 2 * m];
            // the left output's taps are the staged values 2 t .. 2 t + 2 r, the right one's 2 t + 1 .. 2 t + 2 r + 1
            acc[k][0] = acc[k][0] + v.x;
            if (m > 0) acc[k][1] = acc[k][1] + v.x;
            if (m < radius) acc[k][0] = acc[k][0] + v.y;
            acc[k][1] = acc[k][1] + v.y;
        }
    }
}

// the two sums of every plane to dst[k][at], dst[k][at + 1]: one 16-byte store where the address allows it
template <int NP>
__device__ __forceinline__ void gf_row_store(double* const* dst, size_t at, bool second, const double (*acc)[2]) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        double* q = dst[k] + at;
        if (second && ((uintptr_t)q & 15) == 0) {
            *(double2*)q = make_double2(acc[k][0], acc[k][1]);
        } else {
            q[0] = acc[k][0];
            if (second) q[1] = acc[k][1];
        }
    }
}

struct GfPlanes5 {
    double* p[5];
};
struct GfPlanes2 {
    double* p[2];
};

// rows: the row sums of Wd, t1, t2, t3, t4.  w == nullptr: every weight is 1.  grid (ceil(width / MI_GF_SEG), h).
// guide: h x width x 3 samples of T, aligned to T.
template <typename T, typename TW>
__global__ __launch_bounds__(256) void gf_rows_products(const float* __restrict__ p, const TW* __restrict__ w,
                                                        const T* __restrict__ guide, int h, int width, int radius, GfPlanes5 out) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double s[5][MI_GF_LDS];
    __shared__ __attribute__((aligned(16))) uint8_t raw[MI_GF_RAW];
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * MI_GF_SEG;
    const size_t row = (size_t)blockIdx.y * (size_t)width;
    // the columns of this row the workgroup needs: [c0, c1)
    const int c0 = max(x0 - radius, 0), c1 = min(x0 + MI_GF_SEG + radius, width);
    const size_t lo = (row + (size_t)c0) * 3 * sizeof(T), hi = (row + (size_t)c1) * 3 * sizeof(T);
    gf_stage_bytes((const uint8_t*)guide, lo, hi, (size_t)h * (size_t)width * 3 * sizeof(T), raw, tid, 256);
    __syncthreads();
    const int lead = (int)(((uintptr_t)guide + lo) & 15);
    const int n = MI_GF_SEG + 2 * radius;
    for (int i = tid; i < n; i += 256) {
        const int gx = x0 - radius + i;
        double fw = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0;
        if (gx >= 0 && gx < width) {
            const T* px = (const T*)(raw + lead) + (size_t)(gx - c0) * 3;
            const double I = gf_intensity<T>(px[0], px[1], px[2]);
            const double P = (double)p[row + gx];
            fw = w ? (double)w[row + gx] : 1.0;
            t1 = fw * I;
            t2 = fw * P;
            t3 = t1 * I;
            t4 = t1 * P;
        }
        s[0][i] = fw;
        s[1][i] = t1;
        s[2][i] = t2;
        s[3][i] = t3;
        s[4][i] = t4;
    }
    __syncthreads();
    const int x = x0 + 2 * tid;
    if (x >= width) return;
    double acc[5][2];
    gf_row_sums<5>(s, tid, radius, acc);
    gf_row_store<5>(out.p, row + x, x + 1 < width, acc);
}

// rows over two planes that exist already (a and b).  out must not be a or b.
__global__ __launch_bounds__(256) void gf_rows_ab(const double* __restrict__ a, const double* __restrict__ b, int h, int width,
                                                  int radius, GfPlanes2 out) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double s[2][MI_GF_LDS];
    const int tid = (int)threadIdx.x, x0 = (int)blockIdx.x * MI_GF_SEG;
    const size_t row = (size_t)blockIdx.y * (size_t)width;
    const int n = MI_GF_SEG + 2 * radius;
    for (int i = tid; i < n; i += 256) {
        const int gx = x0 - radius + i;
        const bool in = gx >= 0 && gx < width;
        s[0][i] = in ? a[row + gx] : 0.0;
        s[1][i] = in ? b[row + gx] : 0.0;
    }
    __syncthreads();
    const int x = x0 + 2 * tid;
    if (x >= width) return;
    double acc[2][2];
    gf_row_sums<2>(s, tid, radius, acc);
    gf_row_store<2>(out.p, row + x, x + 1 < width, acc);
}

// One lane's MI_GF_ROWS column sums of every plane: the rows y0 - r .. y0 + r + MI_GF_ROWS - 1 inside the frame, top to
// bottom, each fed to the outputs whose window holds it -- every output takes its rows in ascending order.
template <int NP>
__device__ __forceinline__ void gf_col_sums(const double* const* src, int x, int y0, int h, int width, int radius,
                                            double (*acc)[MI_GF_ROWS]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int j = 0; j < MI_GF_ROWS; ++j) acc[k][j] = 0.0;
    const int K = 2 * radius + 1;
    for (int i = 0; i < K + MI_GF_ROWS - 1; ++i) {
        const int gy = y0 - radius + i;             // wave-uniform
        if (gy < 0) continue;
        if (gy >= h) break;
        const size_t at = (size_t)gy * (size_t)width + x;
        double v[NP];
#pragma unroll
        for (int k = 0; k < NP; ++k) v[k] = src[k][at];
#pragma unroll
        for (int j = 0; j < MI_GF_ROWS; ++j) {
            const int t = i - j;                    // the tap of output row y0 + j that input row gy meets
            if (t >= 0 && t < K) {
#pragma unroll
                for (int k = 0; k < NP; ++k) acc[k][j] = acc[k][j] + v[k];
            }
        }
    }
}

// columns over the five row sums, the model, a and b.  Launch: 256 threads = 64 columns x 4 groups of MI_GF_ROWS rows.
__global__ __launch_bounds__(256) void gf_cols_model(GfPlanes5 in, const float* __restrict__ p, int h, int width, int radius, double eps,
                                                     double* __restrict__ A, double* __restrict__ B) {
#pragma clang fp contract(off)
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * 64 + (tid & 63);
    const int y0 = ((int)blockIdx.y * 4 + (tid >> 6)) * MI_GF_ROWS;     // wave-uniform
    if (x >= width || y0 >= h) return;
    double acc[5][MI_GF_ROWS];
    gf_col_sums<5>(in.p, x, y0, h, width, radius, acc);
#pragma unroll
    for (int j = 0; j < MI_GF_ROWS; ++j) {
        const int y = y0 + j;
        if (y >= h) break;
        const size_t at = (size_t)y * (size_t)width + x;
        const double sw = acc[0][j];
        double a = 0.0, b;
        if (sw > 0.0) {
            const double mI = acc[1][j] / sw;
            const double mp = acc[2][j] / sw;
            const double var = acc[3][j] / sw - mI * mI;
            const double cov = acc[4][j] / sw - mI * mp;
            a = cov / (var + eps);
            b = mp - a * mI;
        } else {
            b = (double)p[at];
        }
        A[at] = a;
        B[at] = b;
    }
}

// columns over the row sums of a and b, the average of the models at the pixel's own intensity, the clamp, float32
template <typename T>
__global__ __launch_bounds__(256) void gf_cols_out(GfPlanes2 in, const T* __restrict__ guide, int h, int width, int radius, double lo,
                                                   double hi, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * 64 + (tid & 63);
    const int y0 = ((int)blockIdx.y * 4 + (tid >> 6)) * MI_GF_ROWS;     // wave-uniform
    if (x >= width || y0 >= h) return;
    double acc[2][MI_GF_ROWS];
    gf_col_sums<2>(in.p, x, y0, h, width, radius, acc);
    const int nx = min(x + radius, width - 1) - max(x - radius, 0) + 1;
#pragma unroll
    for (int j = 0; j < MI_GF_ROWS; ++j) {
        const int y = y0 + j;
        if (y >= h) break;
        const size_t at = (size_t)y * (size_t)width + x;
        const double n = (double)((min(y + radius, h - 1) - max(y - radius, 0) + 1) * nx);
        const T* px = guide + at * 3;
        const double I = gf_intensity<T>(px[0], px[1], px[2]);
        double q = (acc[0][j] / n) * I + acc[1][j] / n;
        q = q < lo ? lo : q;
        q = q > hi ? hi : q;
        out[at] = (float)q;
    }
}

// The four launches on `st`.  p: h x width float32; w: h x width of TW, or nullptr for unit weights; guide: h x width x 3 of
// T; scratch: MI_GF_PLANES planes of h * width doubles, 16-byte aligned; out: h x width float32 (it may be p: the last pass
// reads no p).  1 <= radius <= MI_GF_MAX_RADIUS: the caller has checked.  Only enqueues.
template <typename T, typename TW>
inline void gf_launch(hipStream_t st, const float* p, const TW* w, const T* guide, int h, int width, int radius, double eps, double lo,
                      double hi, double* scratch, float* out) {
    const size_t np = (size_t)h * (size_t)width;
    GfPlanes5 s5;
    for (int k = 0; k < 5; ++k) s5.p[k] = scratch + (size_t)k * np;
    double *A = scratch + 5 * np, *B = scratch + 6 * np;
    GfPlanes2 s2{{scratch, scratch + np}};
    const dim3 rows((unsigned)cdiv(width, MI_GF_SEG), (unsigned)h), cols((unsigned)cdiv(width, 64), (unsigned)cdiv(h, 4 * MI_GF_ROWS));
    hipLaunchKernelGGL((gf_rows_products<T, TW>), rows, dim3(256), 0, st, p, w, guide, h, width, radius, s5);
    hipLaunchKernelGGL(gf_cols_model, cols, dim3(256), 0, st, s5, p, h, width, radius, eps, A, B);
    hipLaunchKernelGGL(gf_rows_ab, rows, dim3(256), 0, st, (const double*)A, (const double*)B, h, width, radius, s2);
    hipLaunchKernelGGL((gf_cols_out<T>), cols, dim3(256), 0, st, s2, guide, h, width, radius, lo, hi, out);
}

}  // namespace mi
