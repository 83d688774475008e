// kernels_jpeg.hpp -- a baseline JPEG frame (ITU-T T.81 SOF0, Huffman coded, with restart intervals), uploaded as it lies in
// the file, becomes the H x W x 3 BGR uint8 frame the stack takes.  No reference counterpart: the reference decodes on the
// host through OpenCV.  tests/jpeg_restatement.py is the definition, held bit for bit, and is itself pinned against
// libjpeg-turbo (tests/test_jpeg_host.py).
//
//   jpeg_entropy   one restart interval per WAVEFRONT (a workgroup of 64), walked by lane 0 with jpeg_core.hpp's
//                  decode_block over ljpeg_core.hpp's bit reader, straight from the span in HBM.  Lanes 0 .. 3 first put
//                  the four Huffman tables into canonical form in LDS.  Why a wavefront and not a lane: a camera file has
//                  one interval per MCU row, a few hundred in all -- fewer than the chip has wave slots, so every interval
//                  gets a wave of its own either way -- and 64 walkers in one wave would run each other's
//                  data-dependent branches (the code-length search, the end of block) under masks.  raw_ljpeg made the
//                  same choice for its tiles.  The other 63 lanes idle: decode INSIDE an interval is kernels_jpeg_split.hpp.
//   jpeg_idct      one block per lane: dequantise, the 13-bit "slow integer" inverse DCT (columns descaled by 11, rows by
//                  18, both with rounding), + 128, clip; in int64 throughout, as the restatement computes it, so that it
//                  holds for every int16 coefficient and every table entry.  Writes the component's padded sample plane.
//   jpeg_colour    one output pixel per lane: the chroma samples under libjpeg's "fancy" triangle filters, taken from the
//                  component cropped to its own size with the edge replicated (never from the block padding) -- or, where
//                  that component is 1 or 2 samples wide, plainly replicated, as libjpeg does it -- then the
//                  16-bit fixed-point YCbCr -> RGB, clipped, stored as BGR.
//
// Bounded by construction: an interval decodes min(dri, MCUs left) MCUs whatever its bytes hold; the offsets are clamped
// to the span, the reader returns 0 beyond the interval; every block index comes from the MCU counter, never the stream.
#pragma once
#include "common.hpp"
#include "jpeg_core.hpp"

namespace mi {

namespace jpeg {
// what the launch derives from mi_jpeg_t (the caller has checked it: capi.hip jpeg_check)
struct Geom {
    int mcus_x, mcus_y, n_mcus;
    int h[3], v[3];         // sampling of each component
    int bw[3], bh[3];       // its padded grid in blocks
    int cw[3], ch[3];       // its own size in samples: ceil(W h / hmax) x ceil(H v / vmax)
    size_t boff[3];         // its first block among all
    size_t nblocks;
};
inline Geom geom(const mi_jpeg_t& J) {
    Geom g{};
    g.mcus_x = (J.width + 8 * J.hmax - 1) / (8 * J.hmax);
    g.mcus_y = (J.height + 8 * J.vmax - 1) / (8 * J.vmax);
    g.n_mcus = g.mcus_x * g.mcus_y;
    size_t at = 0;
    for (int c = 0; c < 3; ++c) {
        g.h[c] = c == 0 ? J.hmax : 1;
        g.v[c] = c == 0 ? J.vmax : 1;
        if (c >= J.ncomp) continue;
        g.bw[c] = g.mcus_x * g.h[c];
        g.bh[c] = g.mcus_y * g.v[c];
        g.cw[c] = (J.width * g.h[c] + J.hmax - 1) / J.hmax;
        g.ch[c] = (J.height * g.v[c] + J.vmax - 1) / J.vmax;
        g.boff[c] = at;
        at += (size_t)g.bw[c] * g.bh[c];
    }
    g.nblocks = at;
    return g;
}
}  // namespace jpeg

struct JpegEntropyArgs {
    const uint8_t* span;
    const uint32_t* offsets;
    int16_t* coef;
    uint32_t* status;       // or null
    uint32_t span_bytes;
    jpeg::Geom G;
    mi_jpeg_t J;
};

__global__ __launch_bounds__(64) void jpeg_entropy(JpegEntropyArgs A) {
    using namespace jpeg;
    __shared__ Huff256 tabs[4];
    const int lane = (int)threadIdx.x, i = (int)blockIdx.x;
    if (lane < 4) huff_build(tabs[lane], A.J.counts[lane], A.J.values[lane]);
    __syncthreads();
    if (lane != 0) return;
    const uint32_t o0 = min(A.offsets[i], A.span_bytes), o1 = min(A.offsets[i + 1], A.span_bytes);
    const uint32_t len = o1 > o0 ? o1 - o0 : 0u;
    ljpeg::BitReader<ljpeg::SpanBytes> rd(ljpeg::SpanBytes{A.span + o0, len, len});
    rd.template fill<8>();
    uint32_t status = 0;
    uint32_t pred[3] = {0, 0, 0};
    const long long first = (long long)i * A.J.dri;
    const int n = first < A.G.n_mcus ? (int)min((long long)A.J.dri, A.G.n_mcus - first) : 0;
    int my = (int)(first / A.G.mcus_x), mx = (int)(first - (long long)my * A.G.mcus_x);
    for (int m = 0; m < n; ++m) {
        for (int c = 0; c < A.J.ncomp; ++c) {
            const Huff256& dc = tabs[A.J.td[c] & 1];
            const Huff256& ac = tabs[2 + (A.J.ta[c] & 1)];
            for (int by = 0; by < A.G.v[c]; ++by)
                for (int bx = 0; bx < A.G.h[c]; ++bx) {
                    const size_t b = A.G.boff[c] + (size_t)(my * A.G.v[c] + by) * A.G.bw[c] + (size_t)(mx * A.G.h[c] + bx);
                    decode_block(rd, dc, ac, pred[c], A.coef + b * 64, status);
                }
        }
        if (++mx == A.G.mcus_x) { mx = 0; ++my; }
    }
    if (rd.overrun()) status |= ST_OVERRUN;
    if (A.status) A.status[i] = status;
}

struct JpegRenderArgs {
    const int16_t* coef;
    uint8_t* planes;        // nblocks * 64 samples: each component's padded plane, bh * 8 rows of bw * 8
    uint8_t* out;           // height x width x 3 BGR
    jpeg::Geom G;
    int width, height, ncomp, hmax, vmax;
    uint8_t tq[4];
    uint8_t quant[4][64];
};

namespace jpeg {
__device__ __forceinline__ long long descale(long long x, int n) { return (x + (1ll << (n - 1))) >> n; }

// one pass of the slow-integer inverse DCT over eight values (libjpeg's jidctint.c, public since 1991): out[k] before the
// descale
__device__ __forceinline__ void idct8(const long long in[8], long long out[8]) {
    long long z2 = in[2], z3 = in[6];
    long long z1 = (z2 + z3) * 4433;
    long long tmp2 = z1 - z3 * 15137;
    long long tmp3 = z1 + z2 * 6270;
    z2 = in[0]; z3 = in[4];
    long long tmp0 = (z2 + z3) * 8192;
    long long tmp1 = (z2 - z3) * 8192;
    const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    long long z4 = tmp1 + tmp3;
    const long long z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3;
    out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
    out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1;
    out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}
}  // namespace jpeg

__global__ __launch_bounds__(256) void jpeg_idct(JpegRenderArgs A) {
    using namespace jpeg;
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= A.G.nblocks) return;
    const int c = A.ncomp == 3 && b >= A.G.boff[2] ? 2 : A.ncomp == 3 && b >= A.G.boff[1] ? 1 : 0;
    const size_t k = b - A.G.boff[c];
    const int by = (int)(k / A.G.bw[c]), bx = (int)(k - (size_t)by * A.G.bw[c]);
    const uint8_t* q = A.quant[A.tq[c] & 3];
    const int16_t* in = A.coef + b * 64;
    long long ws[64];
#pragma unroll
    for (int x = 0; x < 8; ++x) {       // columns
        long long col[8], o[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) col[y] = (long long)in[8 * y + x] * (long long)q[8 * y + x];
        idct8(col, o);
#pragma unroll
        for (int y = 0; y < 8; ++y) ws[8 * y + x] = descale(o[y], 11);
    }
    uint8_t* plane = A.planes + A.G.boff[c] * 64;
    const size_t stride = (size_t)A.G.bw[c] * 8;
#pragma unroll
    for (int y = 0; y < 8; ++y) {       // rows
        long long o[8];
        idct8(ws + 8 * y, o);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const long long s = descale(o[x], 18) + 128;
            const uint32_t u = (uint32_t)(s < 0 ? 0 : s > 255 ? 255 : s);
            if (x < 4) lo |= u << (8 * x);
            else hi |= u << (8 * (x - 4));
        }
        uint32_t* row = (uint32_t*)(plane + ((size_t)by * 8 + y) * stride + (size_t)bx * 8);    // (8-byte aligned)
        row[0] = lo;
        row[1] = hi;
    }
}

__global__ __launch_bounds__(256) void jpeg_colour(JpegRenderArgs A) {
    const int x = (int)(blockIdx.x * 64 + (threadIdx.x & 63)), y = (int)(blockIdx.y * 4 + (threadIdx.x >> 6));
    if (x >= A.width || y >= A.height) return;
    const jpeg::Geom& G = A.G;
    const int Y = A.planes[(size_t)y * G.bw[0] * 8 + x];
    uint8_t* o = A.out + ((size_t)y * A.width + x) * 3;
    if (A.ncomp == 1) {
        o[0] = o[1] = o[2] = (uint8_t)Y;
        return;
    }
    int cc[2];
#pragma unroll
    for (int c = 1; c <= 2; ++c) {
        const uint8_t* p = A.planes + G.boff[c] * 64;
        const size_t st = (size_t)G.bw[c] * 8;
        const int cw = G.cw[c], ch = G.ch[c];
        int v;
        if (A.hmax == 1) {
            v = p[(size_t)y * st + x];
        } else {
            const int cx = x >> 1, nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
            if (cw <= 2) {      // libjpeg filters only a component more than 2 samples wide: plain replication, both ways
                v = p[(size_t)(A.vmax == 2 ? y >> 1 : y) * st + cx];
            } else if (A.vmax == 1) {
                const uint8_t* r = p + (size_t)y * st;
                v = (3 * r[cx] + r[nx] + ((x & 1) ? 2 : 1)) >> 2;
            } else {
                const int cy = y >> 1, fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
                const uint8_t *r0 = p + (size_t)cy * st, *r1 = p + (size_t)fy * st;
                const int t = 3 * r0[cx] + r1[cx], tn = 3 * r0[nx] + r1[nx];
                v = (3 * t + tn + ((x & 1) ? 7 : 8)) >> 4;
            }
        }
        cc[c - 1] = v - 128;
    }
    const int cb = cc[0], cr = cc[1];
    const int r = Y + ((91881 * cr + 32768) >> 16);
    const int b = Y + ((116130 * cb + 32768) >> 16);
    const int g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    o[0] = (uint8_t)min(max(b, 0), 255);
    o[1] = (uint8_t)min(max(g, 0), 255);
    o[2] = (uint8_t)min(max(r, 0), 255);
}

// arguments checked by the caller (capi.hip: jpeg_check)
inline void jpeg_entropy_launch(hipStream_t st, const void* span, size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t& J,
                                int16_t* coef, uint32_t* status) {
    JpegEntropyArgs A{};
    A.span = (const uint8_t*)span; A.offsets = offsets; A.coef = coef; A.status = status;
    A.span_bytes = (uint32_t)span_bytes;
    A.G = jpeg::geom(J);
    A.J = J;
    hipLaunchKernelGGL(jpeg_entropy, dim3((unsigned)J.n_intervals), dim3(64), 0, st, A);
}

inline void jpeg_render_launch(hipStream_t st, const mi_jpeg_t& J, const int16_t* coef, uint8_t* planes, uint8_t* out) {
    JpegRenderArgs A{};
    A.coef = coef; A.planes = planes; A.out = out;
    A.G = jpeg::geom(J);
    A.width = J.width; A.height = J.height; A.ncomp = J.ncomp; A.hmax = J.hmax; A.vmax = J.vmax;
    for (int c = 0; c < 4; ++c) {
        A.tq[c] = J.tq[c];
        for (int k = 0; k < 64; ++k) A.quant[c][k] = J.quant[c][k];
    }
    hipLaunchKernelGGL(jpeg_idct, dim3((unsigned)((A.G.nblocks + 255) / 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(jpeg_colour, dim3((unsigned)((J.width + 63) / 64), (unsigned)((J.height + 3) / 4)), dim3(256), 0, st, A);
}

}  // namespace mi
