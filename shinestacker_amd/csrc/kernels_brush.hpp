// kernels_brush.hpp -- brush retouching (reference retouch/brush_tool.py, retouch/brush_preview.py and
// copy_brush_area_to_master in retouch/image_editor_ui.py): a source frame painted into the fused frame with a soft brush, a
// whole stroke in one launch.  shinestacker_amd/retouch.py builds the table and the stamp list and owns the public interface.
//
// The operation (the specification; tests/brush_restatement.py states it in NumPy, as the reference's stamp loop and as the
// per-pixel fold below, and both are held bit for bit to frames recorded from the reference's own code):
//
// **Inputs of one stroke**
// - `master`: H x W x 3, uint8 or uint16.  Written in place.
// - `source`: a frame of the same shape and type.  Read only.
// - `S`: the stamp table, float64, (2r + 1) x (2r + 1), r the brush radius.  The caller builds it:
//   `S = create_brush_mask(2r + 1, hardness, opacity) * flow / 100.0`, so it already holds `opacity / 100` once.
// - `stamps`: n centres (cx, cy), int32, in stroke order.  A centre may lie anywhere, outside the frame too.
// - `opacity`: `opacity / 100` as a double.  It enters a second time below, as in the reference.
//
// **Mask, per pixel (y, x), float64.**  M starts at 0.  For every stamp, in stroke order, whose square
// `|x - cx| <= r and |y - cy| <= r` holds the pixel:
//     M = min(max(M + S[y - cy + r, x - cx + r], 0), 1)         one rounded add, then the clip
// The order matters: the clip sits inside the fold.
//
// **Blend, per covered pixel and channel, float64, every operation rounded on its own (no fused multiply-add):**
//     e   = min(max(M * opacity, 0), 1)
//     v   = master * (1 - e) + source * e
//     out = trunc(min(max(v, 0), maxv))                         maxv = 255 or 65535
//
// **Coverage.**  A pixel that no stamp's square holds keeps the master's value and is not written.  A pixel that a square
// holds is written even where S is 0 there (the reference recomputes the whole footprint; the value is the master's).
// `mask_out`, when given, receives M at the covered pixels and is not touched elsewhere (the caller zeroes it).
//
// The reference keeps a copy of the master and a mask layer in memory and recomputes the footprint from them at every stamp.
// Its result at a pixel is a function of that pixel's final M alone, which is why the fold needs neither.
//
// brush_stroke_kernel: the launch covers the stroke's bounding box `[x0, x1) x [y0, y1)` (the union of the footprints clipped
// to the frame, computed on the host) with tiles of MI_BR_TW x MI_BR_TH = 64 x 16 pixels, a workgroup of 256 per tile; a wave
// owns rows w, w + 4, w + 8, w + 12 of the tile, a lane one column, so a lane carries four M in registers.
//   1. cull: the workgroup walks the stamp list 256 stamps at a time, a stamp per thread, and tests the stamp's square against
//      the tile in 64-bit arithmetic (a centre may be any int32).  The hits are appended to an LDS list in stroke order: a
//      wave ballot gives a hit's rank inside its wave, four wave counts in LDS give the wave's offset (ordered compaction).
//   2. fold: when the list cannot take another 256 hits (MI_BR_CAP = 512 entries, 4 KB), or the stamps are used up, every lane
//      folds its four pixels over the list -- the centre is an LDS broadcast, S[dy, dx] a gather whose lanes read consecutive
//      doubles -- and the list is emptied.  M stays in registers across chunks, so a stroke of any length works.
//   3. blend: once, after the last chunk, for the covered pixels.  A tile that no stamp meets has touched no memory.
// No atomics and no per-stamp launches: every pixel is independent.  A float64 add and two compares per (pixel, covering stamp).
//
// blend_mask_kernel: the blend alone over a whole frame from an H x W float64 mask (the reference's apply_mask for a caller
// that already has a mask): e = clip(mask * opacity, 0, 1), every pixel written.
#pragma once
#include "common.hpp"

namespace mi {

#define MI_BR_TW 64                 // tile width: a wave's lanes
#define MI_BR_TH 16                 // tile height: 4 waves x MI_BR_ROWS rows
#define MI_BR_ROWS 4
#define MI_BR_CAP 512               // culled stamps the LDS list holds
#define MI_BR_MIN_RADIUS 2
#define MI_BR_MAX_RADIUS 500
#define MI_BR_MAX_STAMPS 65536

static_assert(MI_BR_TH == 4 * MI_BR_ROWS && MI_BR_CAP >= 2 * 256, "a chunk takes one more block of 256 stamps before it is folded");

template <typename T>
__device__ __forceinline__ T brush_blend(T m, T s, double e, double one_minus_e, double maxv) {
    double v = __dadd_rn(__dmul_rn((double)m, one_minus_e), __dmul_rn((double)s, e));
    v = fmin(fmax(v, 0.0), maxv);
    return (T)v;                    // truncates
}

template <typename T>
__global__ __launch_bounds__(256) void brush_stroke_kernel(T* __restrict__ master, const T* __restrict__ source,
                                                           const double* __restrict__ table, const int2* __restrict__ stamps,
                                                           int n_stamps, int radius, int width, int bx0, int by0, int bx1, int by1,
                                                           double opacity, double* __restrict__ mask_out) {
    __shared__ int2 list[MI_BR_CAP];
    __shared__ int wave_hits[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tx0 = bx0 + (int)blockIdx.x * MI_BR_TW, ty0 = by0 + (int)blockIdx.y * MI_BR_TH;
    const int tx1 = min(tx0 + MI_BR_TW, bx1), ty1 = min(ty0 + MI_BR_TH, by1);
    const int x = tx0 + lane, side = 2 * radius + 1;
    const long long r = radius;
    double m[MI_BR_ROWS];
    bool covered[MI_BR_ROWS];
#pragma unroll
    for (int k = 0; k < MI_BR_ROWS; ++k) { m[k] = 0.0; covered[k] = false; }
    int count = 0;                  // entries in `list`; the same in every thread
    for (int base = 0; base < n_stamps; base += 256) {
        const int i = base + tid;
        int2 c = make_int2(0, 0);
        bool hit = false;
        if (i < n_stamps) {
            c = stamps[i];
            hit = (long long)c.x + r >= tx0 && (long long)c.x - r < tx1 && (long long)c.y + r >= ty0 && (long long)c.y - r < ty1;
        }
        const unsigned long long b = __ballot(hit);
        if (lane == 0) wave_hits[wv] = __popcll(b);
        __syncthreads();
        int at = count, total = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = wave_hits[q];
            if (q < wv) at += n;
            total += n;
        }
        if (hit) list[at + __popcll(b & ((1ull << lane) - 1ull))] = c;       // at most count + 256 <= MI_BR_CAP entries
        count += total;
        __syncthreads();
        if (count > MI_BR_CAP - 256 || base + 256 >= n_stamps) {
            if (x < tx1) {
                for (int j = 0; j < count; ++j) {
                    const int2 s = list[j];                                     // |x - s.x| <= radius + 64: no overflow
                    const int dx = x - s.x + radius;
                    if ((unsigned)dx < (unsigned)side) {
#pragma unroll
                        for (int k = 0; k < MI_BR_ROWS; ++k) {
                            const int dy = ty0 + wv + 4 * k - s.y + radius;
                            if ((unsigned)dy < (unsigned)side) {
                                m[k] = fmin(fmax(__dadd_rn(m[k], table[dy * side + dx]), 0.0), 1.0);
                                covered[k] = true;
                            }
                        }
                    }
                }
            }
            count = 0;              // the next block's entries are written after its barrier, when every fold is over
        }
    }
    if (x >= tx1) return;
    const double maxv = sizeof(T) == 1 ? 255.0 : 65535.0;
#pragma unroll
    for (int k = 0; k < MI_BR_ROWS; ++k) {
        const int y = ty0 + wv + 4 * k;
        if (y >= ty1 || !covered[k]) continue;
        const size_t p = (size_t)y * (size_t)width + (size_t)x;
        const double e = fmin(fmax(__dmul_rn(m[k], opacity), 0.0), 1.0), om = __dsub_rn(1.0, e);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) master[p * 3 + ch] = brush_blend<T>(master[p * 3 + ch], source[p * 3 + ch], e, om, maxv);
        if (mask_out) mask_out[p] = m[k];
    }
}

// the box lies inside the frame and is not empty, radius and n_stamps are within their limits (the entry points check)
template <typename T>
inline void brush_stroke_launch(hipStream_t st, void* master, const void* source, const double* table, const int32_t* stamps,
                                int n_stamps, int radius, int width, const int32_t* box, double opacity, double* mask_out) {
    const dim3 grid((unsigned)cdiv(box[2] - box[0], MI_BR_TW), (unsigned)cdiv(box[3] - box[1], MI_BR_TH));
    hipLaunchKernelGGL((brush_stroke_kernel<T>), grid, dim3(256), 0, st, (T*)master, (const T*)source, table, (const int2*)stamps,
                       n_stamps, radius, width, box[0], box[1], box[2], box[3], opacity, mask_out);
}

template <typename T>
__global__ __launch_bounds__(256) void blend_mask_kernel(T* __restrict__ master, const T* __restrict__ source,
                                                         const double* __restrict__ mask, size_t n_px, double opacity) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_px) return;
    const double maxv = sizeof(T) == 1 ? 255.0 : 65535.0;
    const double e = fmin(fmax(__dmul_rn(mask[p], opacity), 0.0), 1.0), om = __dsub_rn(1.0, e);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) master[p * 3 + ch] = brush_blend<T>(master[p * 3 + ch], source[p * 3 + ch], e, om, maxv);
}

template <typename T>
inline void blend_mask_launch(hipStream_t st, void* master, const void* source, const double* mask, size_t n_px, double opacity) {
    hipLaunchKernelGGL((blend_mask_kernel<T>), dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, (T*)master, (const T*)source,
                       mask, n_px, opacity);
}

}  // namespace mi
