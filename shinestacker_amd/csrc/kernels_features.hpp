// kernels_features.hpp -- the feature estimator's device side: FAST-9 corners on a factor-2 grey pyramid, a 32-bin
// intensity-centroid orientation, 256 rotated box-sum tests (a BRIEF descriptor), brute-force Hamming matching and RANSAC
// hypotheses for a similarity or a homography.  An algorithm of the ORB family of our own, with no reference counterpart:
// tests/features_restatement.py states every stage in NumPy and the kernels are held to it -- bit for bit up to the
// matcher (all integer), and in float64 with one rounding per operation in RANSAC (nothing may fuse: the build passes
// -ffp-contract=off and the pragma below repeats it).
//
//   feat_gray      frame (h x w x 1 or 3, 8 / 16 bit) -> 8-bit grey: v >> 8 for 16 bits, then
//                  (1868 B + 9617 G + 4899 R + 8192) >> 14.  One thread per pixel, a streaming pass.
//   feat_halve     level l -> level l + 1: (a + b + c + d + 2) >> 2 of each 2 x 2 block, an odd last row / column dropped.
//   feat_score     grey -> the score plane after 3 x 3 suppression and its 256-bin histogram.  A workgroup owns a
//                  TILE_H x TILE_W tile: the grey tile with a halo of 4 goes to LDS, the thresholded FAST score of the tile
//                  and a halo of 1 is computed from it into LDS, and the suppression reads that.  score = the maximum
//                  over the 16 arcs of 9 contiguous circle pixels of max(min d, min -d), d = p_i - c; it counts when it
//                  exceeds the threshold and the pixel is at least EDGE from every border, else it is 0.  The minimum
//                  over 9 contiguous values comes from windows of 2, 4 and 8 (log steps) instead of 9 comparisons per
//                  arc.  The histogram is summed in LDS and leaves with at most 256 atomics per workgroup.
//   feat_compact   the pixels with score >= cut -> 64-bit keys ((255 - score) << 32 | y << 16 | x) in any order, one
//                  slot each from an atomic counter.  Ascending key order is score descending, then y, then x: the host
//                  sorts.  A slot beyond the capacity is not written.
//   feat_describe  one wave per keypoint: the 31 x 31 grey patch goes to LDS, the disc's moments m10, m01 are summed by
//                  the lanes and reduced by shuffles, bin = argmax_k (m10 C[k] + m01 S[k]) in 64-bit integers (no atan2),
//                  the 27 x 27 box sums around the keypoint go to LDS, and each lane evaluates 4 of the 256 tests of the
//                  bin's pattern; __ballot packs 64 of them at a time.
//   feat_match     one thread per query descriptor (4 x 64 bit in registers), the train descriptors staged through LDS in
//                  chunks of MATCH_CHUNK, __popcll, a running best (lowest index on ties) and second best.
//   feat_ransac    one wave per hypothesis.  The model is solved once per wave by lane 0 on a system kept in LDS (2-point
//                  similarity in closed form, 4-point homography by Gaussian elimination with partial pivoting on the
//                  8 x 8 system with h22 = 1), then the lanes stride over the matches and the inlier count is reduced by
//                  shuffles.  A sample index outside [0, n) makes the hypothesis invalid (count -1), as a vanishing
//                  denominator or pivot does: no index is trusted.
#pragma once
#include "common.hpp"

namespace mi {

namespace feat {
constexpr int EDGE = 16;                      // pixels nearer than this to a border score 0 (13 + 2 and 15 stay inside)
constexpr int TILE_W = 64, TILE_H = 16, NT = 256;
constexpr int HALO = 4;                       // 3 for the circle + 1 for the suppression
constexpr int GW = TILE_W + 2 * HALO, GH = TILE_H + 2 * HALO;
constexpr int SW = TILE_W + 2, SH = TILE_H + 2;
constexpr int PATCH = 31, PR = 15;            // the orientation disc's bounding box
constexpr int BOX = 27, BR = 13;              // the box sums a descriptor can read
constexpr int DISC_R2 = 225;
constexpr int BINS = 32, N_TESTS = 256;
constexpr int MATCH_NT = 64, MATCH_CHUNK = 256;
constexpr int RANSAC_NT = 256;                // 4 waves: 4 hypotheses per workgroup
constexpr int NO_SECOND = 0xFFFF;
}  // namespace feat

template <typename T>
__global__ void __launch_bounds__(256) feat_gray(const T* __restrict__ src, uint8_t* __restrict__ dst, size_t npx, int channels) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npx) return;
    constexpr int SH = sizeof(T) == 2 ? 8 : 0;
    if (channels == 1) {
        dst[i] = (uint8_t)(src[i] >> SH);
        return;
    }
    const uint32_t b = src[3 * i] >> SH, g = src[3 * i + 1] >> SH, r = src[3 * i + 2] >> SH;
    dst[i] = (uint8_t)((b * 1868u + g * 9617u + r * 4899u + (1u << 13)) >> 14);
}

// (h, w): the source level; the destination is (h / 2) x (w / 2)
__global__ void __launch_bounds__(256) feat_halve(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w) {
    const int h2 = h >> 1, w2 = w >> 1;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)h2 * w2) return;
    const int y = (int)(i / w2), x = (int)(i % w2);
    const uint8_t* p = src + (size_t)(2 * y) * w + 2 * x;
    dst[i] = (uint8_t)(((uint32_t)p[0] + p[1] + p[w] + p[w + 1] + 2u) >> 2);
}

// the FAST-9 score of the LDS pixel at g (row stride GW); the caller has checked the border
__device__ __forceinline__ int fast9_score(const uint8_t* g) {
    using namespace feat;
    constexpr int OX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int OY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
    const int c = g[0];
    int d[16], lo[16], hi[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) d[i] = (int)g[OY[i] * GW + OX[i]] - c;
    // lo[i] = min(d[i .. i + 8]), hi[i] = max(d[i .. i + 8]), indices mod 16: windows of 2, 4, 8, then one more
    int a2[16], b2[16], a4[16], b4[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { a2[i] = min(d[i], d[(i + 1) & 15]); b2[i] = max(d[i], d[(i + 1) & 15]); }
#pragma unroll
    for (int i = 0; i < 16; ++i) { a4[i] = min(a2[i], a2[(i + 2) & 15]); b4[i] = max(b2[i], b2[(i + 2) & 15]); }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        lo[i] = min(min(a4[i], a4[(i + 4) & 15]), d[(i + 8) & 15]);
        hi[i] = max(max(b4[i], b4[(i + 4) & 15]), d[(i + 8) & 15]);
    }
    int s = -256;
#pragma unroll
    for (int i = 0; i < 16; ++i) s = max(s, max(lo[i], -hi[i]));
    return s;
}

// grid: (ceil(w / TILE_W), ceil(h / TILE_H)); block NT.  `hist` (256 counters) is zeroed by the caller.
__device__ __forceinline__ void feat_score_tile(const uint8_t* __restrict__ gray, uint8_t* __restrict__ score,
                                                uint32_t* __restrict__ hist, int h, int w, int threshold) {
    using namespace feat;
    __shared__ uint8_t G[GH * GW];
    __shared__ uint8_t S[SH * SW];
    __shared__ uint32_t Hs[256];
    const int t = threadIdx.x, x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
    Hs[t] = 0;
    // outside the plane a pixel reads as 0: only pixels nearer than EDGE to the border see it, and they score 0.  (Loading
    // the tile four pixels at a time changed nothing, 66.0 against 66.1 us at 6 MP: the score arithmetic is the time.)
    for (int i = t; i < GH * GW; i += NT) {
        const int y = y0 - HALO + i / GW, x = x0 - HALO + i % GW;
        G[i] = (y >= 0 && y < h && x >= 0 && x < w) ? gray[(size_t)y * w + x] : (uint8_t)0;
    }
    __syncthreads();
    for (int i = t; i < SH * SW; i += NT) {
        const int ly = i / SW, lx = i % SW, y = y0 - 1 + ly, x = x0 - 1 + lx;
        int s = 0;
        if (y >= EDGE && y < h - EDGE && x >= EDGE && x < w - EDGE) {
            s = fast9_score(&G[(ly + HALO - 1) * GW + lx + HALO - 1]);
            s = s > threshold ? s : 0;
        }
        S[i] = (uint8_t)s;
    }
    __syncthreads();
    for (int i = t; i < TILE_H * TILE_W; i += NT) {
        const int ly = i / TILE_W, lx = i % TILE_W, y = y0 + ly, x = x0 + lx;
        if (y >= h || x >= w) continue;
        const uint8_t* p = &S[(ly + 1) * SW + lx + 1];
        const int s = p[0];
        const bool keep = s > 0 && s > p[-SW - 1] && s > p[-SW] && s > p[-SW + 1] && s > p[-1] && s >= p[1] &&
                          s >= p[SW - 1] && s >= p[SW] && s >= p[SW + 1];
        score[(size_t)y * w + x] = keep ? (uint8_t)s : (uint8_t)0;
        if (keep) atomicAdd(&Hs[s], 1u);
    }
    __syncthreads();
    if (Hs[t]) atomicAdd(&hist[t], Hs[t]);
}

__global__ void __launch_bounds__(feat::NT) feat_score(const uint8_t* __restrict__ gray, uint8_t* __restrict__ score,
                                                        uint32_t* __restrict__ hist, int h, int w, int threshold) {
    feat_score_tile(gray, score, hist, h, w, threshold);
}

// `counter` is zeroed by the caller; at most `capacity` keys are written
__global__ void __launch_bounds__(256) feat_compact(const uint8_t* __restrict__ score, int h, int w, int cut,
                                                     unsigned long long* __restrict__ keys, uint32_t* __restrict__ counter,
                                                     uint32_t capacity) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)h * w) return;
    const int s = score[i];
    if (s == 0 || s < cut) return;
    const uint32_t slot = atomicAdd(counter, 1u);
    if (slot >= capacity) return;
    const uint32_t y = (uint32_t)(i / w), x = (uint32_t)(i % w);
    keys[slot] = ((unsigned long long)(255 - s) << 32) | ((unsigned long long)y << 16) | x;
}

struct FeatTrig {
    int c[feat::BINS], s[feat::BINS];     // rint(16384 cos / sin (2 pi k / 32)), from the host
};

// grid: ceil(n / 4); block 256 = 4 waves, one keypoint each.  keys: the level's sorted keys; every keypoint lies at least
// EDGE from the border, so the 31 x 31 patch is inside the level.  kp: 5 ints per keypoint (x, y, level, score, bin),
// desc: 8 words per keypoint; both already offset to the level's first keypoint.
__device__ __forceinline__ void feat_describe_four(const uint8_t* __restrict__ gray, int h, int w, int level,
                                                   const unsigned long long* __restrict__ keys, int n,
                                                   const int8_t* __restrict__ pattern, const FeatTrig& trig,
                                                   int32_t* __restrict__ kp, uint32_t* __restrict__ desc) {
    using namespace feat;
    __shared__ uint8_t P[4][PATCH * PATCH + 3];
    __shared__ uint16_t B[4][BOX * BOX + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + wave;
    const bool live = k < n;
    int x = EDGE, y = EDGE, sc = 0;
    if (live) {
        const unsigned long long key = keys[k];
        x = (int)(key & 0xFFFF);
        y = (int)((key >> 16) & 0xFFFF);
        sc = 255 - (int)(key >> 32);
    }
    // (a key that does not lie EDGE inside the level is not described: nothing is read outside the plane)
    const bool ok = live && x >= EDGE && y >= EDGE && x < w - EDGE && y < h - EDGE;
    int m10 = 0, m01 = 0;
    if (ok) {
        for (int i = lane; i < PATCH * PATCH; i += 64) {
            const int dy = i / PATCH - PR, dx = i % PATCH - PR;
            const int v = gray[(size_t)(y + dy) * w + (x + dx)];
            P[wave][i] = (uint8_t)v;
            if (dx * dx + dy * dy <= DISC_R2) { m10 += dx * v; m01 += dy * v; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        m10 += __shfl_xor(m10, o);
        m01 += __shfl_xor(m01, o);
    }
    int bin = 0;
    long long best = (long long)m10 * trig.c[0] + (long long)m01 * trig.s[0];
    for (int b = 1; b < BINS; ++b) {
        const long long v = (long long)m10 * trig.c[b] + (long long)m01 * trig.s[b];
        if (v > best) { best = v; bin = b; }
    }
    __syncthreads();
    if (ok) {
        for (int i = lane; i < BOX * BOX; i += 64) {
            const int by = i / BOX, bx = i % BOX;      // box centre = patch (by + 2, bx + 2)
            int s = 0;
#pragma unroll
            for (int r = 0; r < 5; ++r)
#pragma unroll
                for (int c = 0; c < 5; ++c) s += P[wave][(by + r) * PATCH + bx + c];
            B[wave][i] = (uint16_t)s;
        }
    }
    __syncthreads();
    const int8_t* pat = pattern + (size_t)bin * N_TESTS * 4;
    for (int q = 0; q < 4; ++q) {
        const int j = q * 64 + lane;
        bool bit = false;
        if (ok) {
            const int xa = pat[4 * j], ya = pat[4 * j + 1], xb = pat[4 * j + 2], yb = pat[4 * j + 3];
            // (the table's offsets are within BR: checked by the host before the launch)
            bit = B[wave][(ya + BR) * BOX + xa + BR] < B[wave][(yb + BR) * BOX + xb + BR];
        }
        const unsigned long long m = __ballot(bit);
        if (ok && lane == 0) {
            desc[(size_t)k * 8 + 2 * q] = (uint32_t)m;
            desc[(size_t)k * 8 + 2 * q + 1] = (uint32_t)(m >> 32);
        }
    }
    if (live && lane == 0) {
        int32_t* o = kp + (size_t)k * 5;
        o[0] = x; o[1] = y; o[2] = level; o[3] = sc; o[4] = ok ? bin : 0;
        if (!ok)
            for (int q = 0; q < 8; ++q) desc[(size_t)k * 8 + q] = 0;
    }
}

__global__ void __launch_bounds__(256) feat_describe(const uint8_t* __restrict__ gray, int h, int w, int level,
                                                      const unsigned long long* __restrict__ keys, int n,
                                                      const int8_t* __restrict__ pattern, FeatTrig trig,
                                                      int32_t* __restrict__ kp, uint32_t* __restrict__ desc) {
    feat_describe_four(gray, h, w, level, keys, n, pattern, trig, kp, desc);
}

// grid: ceil(nq / MATCH_NT); out: 3 ints per query (train index, distance, second distance)
__device__ __forceinline__ void feat_match_block(const unsigned long long* __restrict__ query, int nq,
                                                 const unsigned long long* __restrict__ train, int nt,
                                                 int32_t* __restrict__ out) {
    using namespace feat;
    __shared__ unsigned long long T[MATCH_CHUNK * 4];
    const int q = blockIdx.x * MATCH_NT + threadIdx.x;
    const bool live = q < nq;
    unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    if (live) {
        a0 = query[(size_t)q * 4]; a1 = query[(size_t)q * 4 + 1]; a2 = query[(size_t)q * 4 + 2]; a3 = query[(size_t)q * 4 + 3];
    }
    int d1 = NO_SECOND, d2 = NO_SECOND, idx = -1;
    for (int base = 0; base < nt; base += MATCH_CHUNK) {
        const int m = min(MATCH_CHUNK, nt - base);
        __syncthreads();
        for (int i = threadIdx.x; i < m * 4; i += MATCH_NT) T[i] = train[(size_t)base * 4 + i];
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            const int d = __popcll(a0 ^ T[4 * j]) + __popcll(a1 ^ T[4 * j + 1]) + __popcll(a2 ^ T[4 * j + 2]) +
                          __popcll(a3 ^ T[4 * j + 3]);
            if (d < d1) { d2 = d1; d1 = d; idx = base + j; }
            else if (d < d2) d2 = d;
        }
    }
    if (live) {
        out[(size_t)q * 3] = idx; out[(size_t)q * 3 + 1] = d1; out[(size_t)q * 3 + 2] = d2;
    }
}

__global__ void __launch_bounds__(feat::MATCH_NT) feat_match(const unsigned long long* __restrict__ query, int nq,
                                                              const unsigned long long* __restrict__ train, int nt,
                                                              int32_t* __restrict__ out) {
    feat_match_block(query, nq, train, nt, out);
}

// The 8 x 9 augmented system at `a` solved in place by Gaussian elimination with partial pivoting (largest magnitude,
// lowest row on ties); h[0..7] = the solution.  false when a pivot is below 1e-12 in magnitude.
__device__ inline bool feat_solve8(double* a, double* h) {
#pragma clang fp contract(off)
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        double big = fabs(a[c * 9 + c]);
        for (int r = c + 1; r < 8; ++r) {
            const double v = fabs(a[r * 9 + c]);
            if (v > big) { big = v; piv = r; }
        }
        if (!(big >= 1e-12)) return false;
        if (piv != c)
            for (int j = 0; j < 9; ++j) { const double t = a[c * 9 + j]; a[c * 9 + j] = a[piv * 9 + j]; a[piv * 9 + j] = t; }
        for (int r = c + 1; r < 8; ++r) {
            const double f = a[r * 9 + c] / a[c * 9 + c];
            for (int j = c + 1; j < 9; ++j) {
                const double p = f * a[c * 9 + j];
                a[r * 9 + j] = a[r * 9 + j] - p;
            }
            a[r * 9 + c] = 0.0;
        }
    }
    for (int i = 7; i >= 0; --i) {
        double s = a[i * 9 + 8];
        for (int j = i + 1; j < 8; ++j) {
            const double p = a[i * 9 + j] * h[j];
            s = s - p;
        }
        h[i] = s / a[i * 9 + i];
    }
    return true;
}

// grid: ceil(k / 4); block 256 = 4 waves, one hypothesis each.  src, dst: n x 2 doubles; samples: k x (2 or 4) indices;
// counts: k ints; models: k x 9 doubles (a 3 x 3 matrix, row major; all zeros for an invalid hypothesis).
__device__ __forceinline__ void feat_ransac_four(const double* __restrict__ src, const double* __restrict__ dst, int n,
                                                 const int32_t* __restrict__ samples, int k, int model, double thr,
                                                 int32_t* __restrict__ counts, double* __restrict__ models) {
#pragma clang fp contract(off)
    __shared__ double A[4][72];
    __shared__ double M[4][9];
    __shared__ int V[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int hyp = blockIdx.x * 4 + wave;
    const bool live = hyp < k;
    if (live && lane == 0) {
        const int ns = model == MI_FEAT_HOMOGRAPHY ? 4 : 2;
        int id[4] = {0, 0, 0, 0};
        bool valid = true;
        for (int i = 0; i < ns; ++i) {
            id[i] = samples[(size_t)hyp * ns + i];
            if (id[i] < 0 || id[i] >= n) valid = false;
        }
        double* m = M[wave];
        for (int i = 0; i < 9; ++i) m[i] = 0.0;
        if (valid && model == MI_FEAT_SIMILARITY) {
            const double p0x = src[2 * (size_t)id[0]], p0y = src[2 * (size_t)id[0] + 1];
            const double q0x = dst[2 * (size_t)id[0]], q0y = dst[2 * (size_t)id[0] + 1];
            const double dpx = src[2 * (size_t)id[1]] - p0x, dpy = src[2 * (size_t)id[1] + 1] - p0y;
            const double dqx = dst[2 * (size_t)id[1]] - q0x, dqy = dst[2 * (size_t)id[1] + 1] - q0y;
            const double den = dpx * dpx + dpy * dpy;
            if (den == 0.0) {
                valid = false;
            } else {
                const double a = (dpx * dqx + dpy * dqy) / den;
                const double b = (dpx * dqy - dpy * dqx) / den;
                m[0] = a; m[1] = -b; m[2] = q0x - (a * p0x - b * p0y);
                m[3] = b; m[4] = a;  m[5] = q0y - (b * p0x + a * p0y);
                m[8] = 1.0;
            }
        } else if (valid) {
            double* a = A[wave];
            for (int i = 0; i < 4; ++i) {
                const double x = src[2 * (size_t)id[i]], y = src[2 * (size_t)id[i] + 1];
                const double u = dst[2 * (size_t)id[i]], v = dst[2 * (size_t)id[i] + 1];
                double* r0 = a + 18 * i;
                double* r1 = r0 + 9;
                r0[0] = x; r0[1] = y; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = -(u * x); r0[7] = -(u * y); r0[8] = u;
                r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = x; r1[4] = y; r1[5] = 1.0; r1[6] = -(v * x); r1[7] = -(v * y); r1[8] = v;
            }
            double hh[8];
            valid = feat_solve8(a, hh);
            if (valid) {
                for (int i = 0; i < 8; ++i) m[i] = hh[i];
                m[8] = 1.0;
            }
        }
        V[wave] = valid ? 1 : 0;
    }
    __syncthreads();
    if (!live) return;
    const bool valid = V[wave] != 0;
    int cnt = 0;
    if (valid) {
        double m[9];
        for (int i = 0; i < 9; ++i) m[i] = M[wave][i];
        const double t2 = thr * thr;
        for (int i = lane; i < n; i += 64) {
            const double x = src[2 * (size_t)i], y = src[2 * (size_t)i + 1], u = dst[2 * (size_t)i], v = dst[2 * (size_t)i + 1];
            double px = (m[0] * x + m[1] * y) + m[2];
            double py = (m[3] * x + m[4] * y) + m[5];
            bool good = true;
            if (model == MI_FEAT_HOMOGRAPHY) {
                const double wd = (m[6] * x + m[7] * y) + 1.0;
                good = !(fabs(wd) < 1e-12);
                px = px / wd;
                py = py / wd;
            }
            const double ex = px - u, ey = py - v;
            if (good && ex * ex + ey * ey <= t2) ++cnt;
        }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) {
        counts[hyp] = valid ? cnt : -1;
        for (int i = 0; i < 9; ++i) models[(size_t)hyp * 9 + i] = M[wave][i];
    }
}

__global__ void __launch_bounds__(feat::RANSAC_NT) feat_ransac(const double* __restrict__ src, const double* __restrict__ dst,
                                                                int n, const int32_t* __restrict__ samples, int k, int model,
                                                                double thr, int32_t* __restrict__ counts,
                                                                double* __restrict__ models) {
    feat_ransac_four(src, dst, n, samples, k, model, thr, counts, models);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The batch forms of mi_feat_aligner_t (features_host.hpp).  Every buffer is an array over frame slots -- slot f's part lies at
// base + f * stride -- and the frame index rides in the grid, so a stage is one launch whatever the batch holds.  What the
// host decided between the stages of the single-frame form is decided here: feat_cut the cut, feat_select the sort,
// feat_good the match filter and its order, feat_pick the winner.  Counts never leave the device: a stage reads the count
// its predecessor left and workgroups beyond it return.
//
//   feat_gray_sub  the frame sub-sampled by s and turned grey in one pass: the pixels of img[::s, ::s] (AREA false), or for
//                  s == 2 on even sides each channel's (a + b + c + d + 2) >> 2 of the 2 x 2 block (AREA true), then the
//                  grey formula of feat_gray (16-bit samples lose their low byte after the mean, as a mean of the frame does).
//   feat_cut       one wave per frame: lane k owns the bins 255 - 4k .. 252 - 4k; an inclusive scan over the lanes gives the
//                  tail count above each lane's bins, and the smallest c > threshold whose tail is at most the capacity is a
//                  minimum over the lanes.  Leaves (cut, count(score >= cut)); cut = 256 when nothing fits.
//   feat_select    one workgroup of 1024 per frame: the score plane is read 16 bytes at a time, a pixel with score >= cut
//                  takes a slot of the LDS key array from an LDS counter, the keys are sorted there by a bitonic network over
//                  the next power of two (padded with all-ones keys; keys are unique, so any correct sort gives the one
//                  answer, and this one has no data-dependent control flow), and the first min(count, n_level) leave in order.
//                  The capacity max(4 n_level, 4096) <= SORT_MAX = 16384 keys = 128 KiB of LDS is what bounds n_features.
//   feat_good      one workgroup per pair: the matches that pass the cross-check or the ratio test take LDS slots as keys --
//                  (distance, query, train) for NORM_HAMMING, (query, train, distance) for KNN -- and the same sort puts
//                  them into the order features.match gives.  Indices leave as positions in the frame's level-ordered list
//                  (the sum of the lower levels' counts + the position within the level) beside the level-0 positions.
//   feat_pick      one workgroup per pair: the largest count, the lowest index on ties, -1 below the sample size; then the
//                  inlier mask of that model in residuals2's order of operations.
namespace feat {
constexpr int SORT_MAX = 16384, SORT_NT = 1024;
constexpr int GOOD_MAX = 8192;                // sum of n_features >> level < 2 n_features <= 8192
constexpr int MAX_BATCH = 128;
constexpr int CC = 4;                         // ints per (slot, level): cut, count(score >= cut), keypoints kept, spare
}  // namespace feat

struct FeatFrames {
    const void* p[feat::MAX_BATCH];
};

struct FeatLevels {
    int n;                                    // levels of the handle
    int koff[8];                              // where a level's keypoints start within a slot
};

// grid: (ceil(gh * gw / 256), frames).  The frame is H x W x channels; the grey plane gh x gw.
template <typename T, bool AREA>
__global__ void __launch_bounds__(256) feat_gray_sub(FeatFrames frames, uint8_t* __restrict__ dst, size_t dst_stride, int W,
                                                      int channels, int s, int gh, int gw) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)gh * gw) return;
    const int y = (int)(i / gw), x = (int)(i % gw);
    const T* src = (const T*)frames.p[blockIdx.y];
    constexpr int SH = sizeof(T) == 2 ? 8 : 0;
    uint32_t v[3] = {0, 0, 0};
    for (int c = 0; c < channels; ++c) {
        if constexpr (AREA) {
            const T* p = src + ((size_t)(2 * y) * W + 2 * x) * channels + c;
            v[c] = (((uint32_t)p[0] + p[channels] + p[(size_t)W * channels] + p[(size_t)W * channels + channels] + 2u) >> 2) >> SH;
        } else {
            v[c] = (uint32_t)src[((size_t)(y * s) * W + (size_t)x * s) * channels + c] >> SH;
        }
    }
    uint8_t* out = dst + blockIdx.y * dst_stride;
    out[i] = channels == 1 ? (uint8_t)v[0] : (uint8_t)((v[0] * 1868u + v[1] * 9617u + v[2] * 4899u + (1u << 13)) >> 14);
}

// grid: (ceil((h / 2) * (w / 2) / 256), frames); src and dst are levels of the same slot
__global__ void __launch_bounds__(256) feat_halve_batch(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t stride,
                                                         int h, int w) {
    const int h2 = h >> 1, w2 = w >> 1;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)h2 * w2) return;
    const int y = (int)(i / w2), x = (int)(i % w2);
    const uint8_t* p = src + blockIdx.y * stride + (size_t)(2 * y) * w + 2 * x;
    dst[blockIdx.y * stride + i] = (uint8_t)(((uint32_t)p[0] + p[1] + p[w] + p[w + 1] + 2u) >> 2);
}

// grid: (ceil(w / TILE_W), ceil(h / TILE_H), frames)
__global__ void __launch_bounds__(feat::NT) feat_score_batch(const uint8_t* __restrict__ gray, size_t gray_stride,
                                                              uint8_t* __restrict__ score, size_t score_stride,
                                                              uint32_t* __restrict__ hist, size_t hist_stride, int h, int w,
                                                              int threshold) {
    const size_t f = blockIdx.z;
    feat_score_tile(gray + f * gray_stride, score + f * score_stride, hist + f * hist_stride, h, w, threshold);
}

// grid: frames; block 64.  hist, cc: already at the level.
__global__ void __launch_bounds__(64) feat_cut(const uint32_t* __restrict__ hist, size_t hist_stride, int32_t* __restrict__ cc,
                                                size_t cc_stride, int threshold, uint32_t cap) {
    const uint32_t* h = hist + blockIdx.x * hist_stride;
    const int lane = threadIdx.x;
    uint32_t v[4], sum = 0;
    for (int j = 0; j < 4; ++j) {
        v[j] = h[255 - 4 * lane - j];
        sum += v[j];
    }
    uint32_t inc = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    uint32_t tail = inc - sum;                // count(score > this lane's highest bin)
    uint32_t best_c = 256, best_n = 0;
    for (int j = 0; j < 4; ++j) {             // downwards: a later fit is a smaller cut
        const int c = 255 - 4 * lane - j;
        tail += v[j];
        if (c > threshold && tail <= cap) { best_c = (uint32_t)c; best_n = tail; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t oc = __shfl_xor(best_c, o), on = __shfl_xor(best_n, o);
        if (oc < best_c) { best_c = oc; best_n = on; }
    }
    if (lane == 0) {
        int32_t* o = cc + blockIdx.x * cc_stride;
        o[0] = (int32_t)best_c;
        o[1] = (int32_t)best_n;
    }
}

// K[0 .. n) ascending, by every thread of the workgroup (nt of them); n <= the array's power-of-two size
__device__ __forceinline__ void feat_sort_lds(unsigned long long* K, int n, int nt) {
    int p = 1;
    while (p < n) p <<= 1;
    const int t = threadIdx.x;
    for (int i = n + t; i < p; i += nt) K[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= p; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < p; i += nt) {
                const int o = i ^ j;
                if (o > i) {
                    const unsigned long long a = K[i], b = K[o];
                    if ((a > b) == ((i & k) == 0)) { K[i] = b; K[o] = a; }
                }
            }
            __syncthreads();
        }
}

// grid: frames; block SORT_NT.  score: the level's plane of slot 0; cc, keys: already at the level.
__global__ void __launch_bounds__(feat::SORT_NT) feat_select(const uint8_t* __restrict__ score, size_t score_stride, int h, int w,
                                                              int32_t* __restrict__ cc, size_t cc_stride,
                                                              unsigned long long* __restrict__ keys, size_t keys_stride,
                                                              int n_level, uint32_t cap) {
    using namespace feat;
    __shared__ unsigned long long K[SORT_MAX];
    __shared__ uint32_t cnt;
    const int t = threadIdx.x;
    int32_t* c = cc + blockIdx.x * cc_stride;
    const int cut = c[0];
    if (cap > (uint32_t)SORT_MAX) cap = SORT_MAX;
    if (t == 0) cnt = 0;
    __syncthreads();
    if (cut < 256) {
        const uint8_t* p = score + blockIdx.x * score_stride;       // 16-byte aligned: the strides are multiples of 256
        const size_t npx = (size_t)h * w, nvec = npx / 16;
        auto take = [&](size_t i, uint32_t s) {
            if (s < (uint32_t)cut || s == 0) return;
            const uint32_t slot = atomicAdd(&cnt, 1u);
            if (slot >= cap) return;
            K[slot] = ((unsigned long long)(255 - s) << 32) | ((unsigned long long)(i / w) << 16) | (unsigned long long)(i % w);
        };
        for (size_t i = t; i < nvec; i += SORT_NT) {
            const uint4 q = ((const uint4*)p)[i];
            if ((q.x | q.y | q.z | q.w) == 0) continue;
            const uint32_t word[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int b = 0; b < 16; ++b) take(i * 16 + b, (word[b >> 2] >> (8 * (b & 3))) & 0xFFu);
        }
        for (size_t i = nvec * 16 + t; i < npx; i += SORT_NT) take(i, p[i]);
    }
    __syncthreads();
    const int n = (int)min(cnt, cap);
    feat_sort_lds(K, n, SORT_NT);
    const int kept = min(n, n_level);
    unsigned long long* out = keys + blockIdx.x * keys_stride;
    for (int i = t; i < kept; i += SORT_NT) out[i] = K[i];
    if (t == 0) c[2] = kept;
}

// grid: (ceil(n_level / 4), frames); cc, keys, kp, desc: already at the level; kp_stride in keypoints
__global__ void __launch_bounds__(256) feat_describe_batch(const uint8_t* __restrict__ gray, size_t gray_stride, int h, int w,
                                                            int level, const unsigned long long* __restrict__ keys,
                                                            const int32_t* __restrict__ cc, size_t cc_stride,
                                                            const int8_t* __restrict__ pattern, FeatTrig trig,
                                                            int32_t* __restrict__ kp, uint32_t* __restrict__ desc, size_t kp_stride) {
    const size_t f = blockIdx.y;
    const int n = cc[f * cc_stride + 2];
    if ((int)blockIdx.x * 4 >= n) return;
    feat_describe_four(gray + f * gray_stride, h, w, level, keys + f * kp_stride, n, pattern, trig, kp + f * kp_stride * 5,
                       desc + f * kp_stride * 8);
}

// grid: (ceil(n_level / MATCH_NT), frames).  Either side may be the reference (stride 0).  q_stride, t_stride in 64-bit
// words, out_stride in ints, the cc strides in ints; all pointers already at the level.
__global__ void __launch_bounds__(feat::MATCH_NT) feat_match_batch(const unsigned long long* __restrict__ query, size_t q_stride,
                                                                    const int32_t* __restrict__ q_cc, size_t q_cc_stride,
                                                                    const unsigned long long* __restrict__ train, size_t t_stride,
                                                                    const int32_t* __restrict__ t_cc, size_t t_cc_stride,
                                                                    int32_t* __restrict__ out, size_t out_stride) {
    const size_t f = blockIdx.y;
    const int nq = q_cc[f * q_cc_stride + 2], nt = t_cc[f * t_cc_stride + 2];
    if ((int)blockIdx.x * feat::MATCH_NT >= nq || nt < 1) return;
    feat_match_block(query + f * q_stride, nq, train + f * t_stride, nt, out + f * out_stride);
}

// grid: frames; block SORT_NT.  cc: slot 0's level 0, ref_cc: the reference's; fwd, back, good: 3 ints per keypoint slot,
// kp 5; kp_stride in keypoints.  method: MI_FEAT_MATCH_KNN / MI_FEAT_MATCH_HAMMING.
__global__ void __launch_bounds__(feat::SORT_NT) feat_good(FeatLevels lv, const int32_t* __restrict__ cc, size_t cc_stride,
                                                            const int32_t* __restrict__ ref_cc, const int32_t* __restrict__ fwd,
                                                            const int32_t* __restrict__ back, const int32_t* __restrict__ kp,
                                                            const int32_t* __restrict__ ref_kp, size_t kp_stride, int method,
                                                            double ratio, int32_t* __restrict__ good, int32_t* __restrict__ n_good,
                                                            double* __restrict__ src, double* __restrict__ dst) {
#pragma clang fp contract(off)
    using namespace feat;
    __shared__ unsigned long long K[GOOD_MAX];
    __shared__ uint32_t cnt;
    __shared__ int P0[8], P1[8];              // keypoints of the lower levels: the moving frame's, the reference's
    const int t = threadIdx.x;
    const size_t f = blockIdx.x;
    const int32_t* c = cc + f * cc_stride;
    fwd += f * kp_stride * 3;
    back += f * kp_stride * 3;
    kp += f * kp_stride * 5;
    if (t == 0) {
        cnt = 0;
        int a = 0, b = 0;
        for (int l = 0; l < lv.n; ++l) {
            P0[l] = a;
            P1[l] = b;
            a += c[CC * l + 2];
            b += ref_cc[CC * l + 2];
        }
    }
    __syncthreads();
    for (int l = 0; l < lv.n; ++l) {
        const int nq = c[CC * l + 2], nt = ref_cc[CC * l + 2];
        if (nq < 1 || nt < 1) continue;
        for (int q = t; q < nq; q += SORT_NT) {
            const int32_t* e = fwd + (size_t)(lv.koff[l] + q) * 3;
            const int idx = e[0], d1 = e[1], d2 = e[2];
            if (idx < 0 || idx >= nt) continue;
            const bool ok = method == MI_FEAT_MATCH_HAMMING ? back[(size_t)(lv.koff[l] + idx) * 3] == q
                                                            : (double)d1 < ratio * (double)d2;
            if (!ok) continue;
            const uint32_t slot = atomicAdd(&cnt, 1u);
            if (slot >= (uint32_t)GOOD_MAX) continue;
            const unsigned long long r0 = (unsigned long long)(lv.koff[l] + q), r1 = (unsigned long long)(lv.koff[l] + idx);
            K[slot] = method == MI_FEAT_MATCH_HAMMING ? ((unsigned long long)d1 << 40) | (r0 << 20) | r1
                                                      : (r0 << 40) | (r1 << 20) | (unsigned long long)d1;
        }
    }
    __syncthreads();
    const int n = (int)min(cnt, (uint32_t)GOOD_MAX);
    feat_sort_lds(K, n, SORT_NT);
    good += f * kp_stride * 3;
    src += f * kp_stride * 2;
    dst += f * kp_stride * 2;
    for (int i = t; i < n; i += SORT_NT) {
        const unsigned long long key = K[i];
        int r0, r1, d;
        if (method == MI_FEAT_MATCH_HAMMING) {
            d = (int)(key >> 40); r0 = (int)((key >> 20) & 0xFFFFF); r1 = (int)(key & 0xFFFFF);
        } else {
            r0 = (int)(key >> 40); r1 = (int)((key >> 20) & 0xFFFFF); d = (int)(key & 0xFFFFF);
        }
        const int32_t* a = kp + (size_t)r0 * 5;
        const int32_t* b = ref_kp + (size_t)r1 * 5;
        const int l = a[2] & 7;               // a match stays within its level
        good[(size_t)i * 3] = r0 - lv.koff[l] + P0[l];
        good[(size_t)i * 3 + 1] = r1 - lv.koff[l] + P1[l];
        good[(size_t)i * 3 + 2] = d;
        const double s = (double)(1 << l), h = (s - 1.0) / 2.0;     // level-0 position: x 2^l + (2^l - 1) / 2, exact
        src[(size_t)i * 2] = (double)a[0] * s + h;
        src[(size_t)i * 2 + 1] = (double)a[1] * s + h;
        dst[(size_t)i * 2] = (double)b[0] * s + h;
        dst[(size_t)i * 2 + 1] = (double)b[1] * s + h;
    }
    if (t == 0) n_good[f] = n;
}

// grid: (ceil(k / 4), frames); pt_stride in points.  A pair with fewer good matches than `need` is left alone.
__global__ void __launch_bounds__(feat::RANSAC_NT) feat_ransac_batch(const double* __restrict__ src, const double* __restrict__ dst,
                                                                      size_t pt_stride, const int32_t* __restrict__ n_good, int need,
                                                                      const int32_t* __restrict__ samples, int k, int model,
                                                                      double thr, int32_t* __restrict__ counts,
                                                                      double* __restrict__ models) {
    const size_t f = blockIdx.y;
    const int n = n_good[f];
    if (n < need) return;
    const int ns = model == MI_FEAT_HOMOGRAPHY ? 4 : 2;
    feat_ransac_four(src + f * pt_stride * 2, dst + f * pt_stride * 2, n, samples + f * (size_t)k * ns, k, model, thr,
                     counts + f * (size_t)k, models + f * (size_t)k * 9);
}

// grid: frames; block 256.  head: 4 ints per frame (winner, its count, spare, spare); model: 9 doubles; mask: one byte per
// good match.
__global__ void __launch_bounds__(256) feat_pick(const int32_t* __restrict__ n_good, int need, const int32_t* __restrict__ counts,
                                                  const double* __restrict__ models, int k, int model, double thr,
                                                  const double* __restrict__ src, const double* __restrict__ dst, size_t pt_stride,
                                                  int32_t* __restrict__ head, double* __restrict__ out_model,
                                                  uint8_t* __restrict__ mask, size_t mask_stride) {
#pragma clang fp contract(off)
    __shared__ long long W[4];
    __shared__ double M[9];
    const int t = threadIdx.x;
    const size_t f = blockIdx.x;
    const int n = n_good[f];
    const int ns = model == MI_FEAT_HOMOGRAPHY ? 4 : 2;
    head += f * 4;
    out_model += f * 9;
    mask += f * mask_stride;
    if (n < need) {                           // nothing was evaluated for this pair
        if (t == 0) { head[0] = -1; head[1] = 0; }
        if (t < 9) out_model[t] = 0.0;
        for (int i = t; i < n; i += 256) mask[i] = 0;
        return;
    }
    counts += f * (size_t)k;
    // the largest count, then the lowest index: the maximum of (count + 1) << 32 | (2^31 - 1 - index)
    long long best = -1;
    for (int i = t; i < k; i += 256) {
        const long long v = ((long long)(counts[i] + 1) << 32) | (long long)(0x7FFFFFFF - i);
        best = v > best ? v : best;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int hi = __shfl_xor((int)(best >> 32), o);
        const int lo = __shfl_xor((int)(best & 0xFFFFFFFFll), o);
        const long long v = ((long long)hi << 32) | (long long)(uint32_t)lo;
        best = v > best ? v : best;
    }
    if ((t & 63) == 0) W[t >> 6] = best;
    __syncthreads();
    best = W[0];
    for (int i = 1; i < 4; ++i) best = W[i] > best ? W[i] : best;
    const int count = (int)(best >> 32) - 1;
    const int win = count >= ns ? 0x7FFFFFFF - (int)(best & 0xFFFFFFFFll) : -1;
    if (t < 9) {
        const double v = win >= 0 ? models[(f * (size_t)k + win) * 9 + t] : 0.0;
        M[t] = v;
        out_model[t] = v;
    }
    if (t == 0) { head[0] = win; head[1] = win >= 0 ? count : 0; }
    __syncthreads();
    src += f * pt_stride * 2;
    dst += f * pt_stride * 2;
    const double t2 = thr * thr;
    for (int i = t; i < n; i += 256) {
        bool in = false;
        if (win >= 0) {
            const double x = src[2 * (size_t)i], y = src[2 * (size_t)i + 1], u = dst[2 * (size_t)i], v = dst[2 * (size_t)i + 1];
            double px = (M[0] * x + M[1] * y) + M[2];
            double py = (M[3] * x + M[4] * y) + M[5];
            bool good = true;
            if (model == MI_FEAT_HOMOGRAPHY) {
                const double wd = (M[6] * x + M[7] * y) + 1.0;
                good = !(fabs(wd) < 1e-12);
                px = px / wd;
                py = py / wd;
            }
            const double ex = px - u, ey = py - v;
            in = good && ex * ex + ey * ey <= t2;
        }
        mask[i] = in ? 1 : 0;
    }
}

}  // namespace mi
