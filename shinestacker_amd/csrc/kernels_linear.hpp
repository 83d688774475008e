// kernels_linear.hpp -- linear_develop: an already demosaiced raw frame (a DNG's LinearRaw IFD: what raw denoisers, pixel-shift
// composites, Foveon and monochrome bodies and any converter's "linear DNG" option write) developed in one pass, H x W x spp
// samples of uint8 / uint16 in file order (R, G, B; spp 1: one grey sample) to H x W x 3 interleaved BGR of the same type.  No
// reference counterpart; tests/linear_restatement.py is the definition, held bit for bit.
//
//   step A, per sample:  v' = min(white, (max(v - black[c], 0) * gain_q[c] + 2048) >> 12), c the sample's channel -- step A of
//                        kernels_demosaic.hpp with the channel in place of the cell position; at spp 1, b = g = r = v'
//   steps C and D:       the colour matrix and the tone table of mi_develop_t on (b, g, r), as behind the demosaic: the same
//                        device function (develop_matrix) and the same table placement (uint8: LDS, uint16: gathered from L2)
//
// The work is per pixel and a frame is dense, so the kernel sees one flat run of H * W pixels and no rows: a GROUP is the
// 4 / sizeof(T) pixels (4 at uint8, 2 at uint16) whose output is 12 bytes and whose input is 12 bytes (spp 3) or 4 (spp 1), and
// with both base pointers 4-byte aligned every group of the frame is aligned, whatever the width -- odd widths, a width of 1 and
// rows that start off a 4-byte boundary need no path of their own.  A thread takes linear::UNROLL groups, linear::NT groups
// apart, all loads issued before the first is used: a wave's loads and stores of one step are one contiguous run of 768 bytes.
// What does need care: the frame's last group when H * W is no multiple of the group (per sample, guarded by the pixel
// index), and a base pointer off a 4-byte boundary (frame i of a batch of odd-sized uint8 frames: every group then goes per
// sample -- slower, and as exact).  Traffic: spp * itemsize bytes read, 3 * itemsize written per pixel.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "kernels_demosaic.hpp"

namespace mi {

namespace linear {
constexpr int NT = 256;
constexpr int UNROLL = 4;                  // groups per thread
constexpr int GROUP_BYTES = 4;             // a group is 4 / sizeof(T) pixels: 4 bytes per channel
constexpr int SPAN_GROUPS = NT * UNROLL;   // groups of one workgroup
}  // namespace linear

struct LinearArgs {
    const void* src;   // H x W x spp
    void* dst;         // H x W x 3
    uint32_t npx;      // H * W
    mi_linear_t lin;   // wave-uniform reads: scalar loads from the kernel arguments
};

struct LinearDevelopArgs : LinearArgs {
    int32_t mq[9];     // M_q, row-major, rows and columns in R, G, B order (MATRIX)
    const void* tone;  // maxv + 1 entries of T in device memory (TONE)
};

struct alignas(4) LinearRow {
    uint32_t w[3];
};

__device__ __forceinline__ int linear_step_a(uint32_t v, int black, uint32_t gain, uint32_t white) {
    const int d = (int)v - black;
    const uint32_t q = ((uint32_t)(d < 0 ? 0 : d) * gain + 2048u) >> 12;
    return (int)(q > white ? white : q);
}

template <typename T, bool MATRIX = false, bool TONE = false>
__global__ __launch_bounds__(256) void linear_develop(std::conditional_t<MATRIX || TONE, LinearDevelopArgs, LinearArgs> A) {
    using namespace linear;
    constexpr int PX = GROUP_BYTES / (int)sizeof(T), BITS = 8 * (int)sizeof(T);
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    constexpr bool TONE_LDS = TONE && sizeof(T) == 1;
    [[maybe_unused]] const uint8_t* tone_lds = nullptr;
    if constexpr (TONE_LDS) {   // NT == 256 == the table's length
        static_assert(NT == 256, "one table entry per thread");
        __shared__ uint8_t staged[256];
        staged[threadIdx.x] = ((const uint8_t*)A.tone)[threadIdx.x];
        tone_lds = staged;
        __syncthreads();
    }
    const T* src = (const T*)A.src;
    T* dst = (T*)A.dst;
    const uint32_t npx = A.npx;
    const bool three = A.lin.spp == 3;
    const int spp = three ? 3 : 1;
    const bool aligned = (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
    const uint32_t g0 = blockIdx.x * (uint32_t)SPAN_GROUPS + threadIdx.x;
    const uint32_t white = (uint32_t)A.lin.white;
    uint32_t in[UNROLL][3];
    // all loads first: a thread's groups are in flight together
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const uint32_t g = g0 + (uint32_t)u * NT;
        const size_t p0 = (size_t)g * PX;               // the group's first pixel
        in[u][0] = in[u][1] = in[u][2] = 0;
        if (p0 >= npx) continue;
        if (aligned && p0 + PX <= npx) {
            if (three) {
                const LinearRow r = ((const LinearRow*)src)[g];
                in[u][0] = r.w[0]; in[u][1] = r.w[1]; in[u][2] = r.w[2];
            } else {
                in[u][0] = ((const uint32_t*)src)[g];
            }
        } else {
#pragma unroll
            for (int j = 0; j < PX * 3; ++j)            // sample j of the group: pixel j / spp of it
                if (j < PX * spp && p0 + (size_t)(three ? j / 3 : j) < npx)
                    in[u][j / PX] |= (uint32_t)src[p0 * spp + j] << (BITS * (j % PX));
        }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const uint32_t g = g0 + (uint32_t)u * NT;
        const size_t p0 = (size_t)g * PX;
        if (p0 >= npx) continue;
        T e[PX * 3];
#pragma unroll
        for (int px = 0; px < PX; ++px) {
            int b, gr, r;
            if (three) {
                const int j = 3 * px;
                r = linear_step_a((in[u][j / PX] >> (BITS * (j % PX))) & MASK, A.lin.black[0], A.lin.gain_q[0], white);
                gr = linear_step_a((in[u][(j + 1) / PX] >> (BITS * ((j + 1) % PX))) & MASK, A.lin.black[1], A.lin.gain_q[1], white);
                b = linear_step_a((in[u][(j + 2) / PX] >> (BITS * ((j + 2) % PX))) & MASK, A.lin.black[2], A.lin.gain_q[2], white);
            } else {
                b = gr = r = linear_step_a((in[u][0] >> (BITS * px)) & MASK, A.lin.black[0], A.lin.gain_q[0], white);
            }
            if constexpr (MATRIX) develop_matrix(A.mq, b, gr, r, (int)white);
            if constexpr (TONE) {   // 0 <= value <= white <= maxv: inside the table
                if constexpr (TONE_LDS) {
                    b = tone_lds[b]; gr = tone_lds[gr]; r = tone_lds[r];
                } else {
                    const T* tone = (const T*)A.tone;
                    b = tone[b]; gr = tone[gr]; r = tone[r];
                }
            }
            e[px * 3 + 0] = (T)b;
            e[px * 3 + 1] = (T)gr;
            e[px * 3 + 2] = (T)r;
        }
        if (aligned && p0 + PX <= npx) {
            LinearRow o;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                uint32_t d = 0;
#pragma unroll
                for (int j = 0; j < PX; ++j) d |= (uint32_t)e[k * PX + j] << (BITS * j);
                o.w[k] = d;
            }
            ((LinearRow*)dst)[g] = o;
        } else {
#pragma unroll
            for (int px = 0; px < PX; ++px)
                if (p0 + px < npx) {
                    T* q = dst + (p0 + px) * 3;
                    q[0] = e[px * 3 + 0];
                    q[1] = e[px * 3 + 1];
                    q[2] = e[px * 3 + 2];
                }
        }
    }
}

// the pixels one workgroup takes of frames of `dtype`
inline int linear_span(int dtype) { return linear::SPAN_GROUPS * (linear::GROUP_BYTES / (dtype == MI_U8 ? 1 : 2)); }

// step A and, with `dev`, steps C and D (arguments checked by the caller: capi.hip, linear_check, develop_check)
inline void linear_develop_launch(hipStream_t st, const void* src, void* dst, int h, int w, int dtype, const mi_linear_t& lin,
                                  const mi_develop_t* dev) {
    const bool mat = dev && (dev->flags & MI_DEVELOP_MATRIX) != 0, tone = dev && (dev->flags & MI_DEVELOP_TONE) != 0;
    const uint32_t npx = (uint32_t)h * (uint32_t)w;
    const uint32_t span = (uint32_t)linear_span(dtype);
    const dim3 grid((npx + span - 1) / span), blk(linear::NT);     // (npx * 3 < 2^32: the sum cannot wrap)
    const bool u8 = dtype == MI_U8;
    if (!mat && !tone) {
        LinearArgs A{src, dst, npx, lin};
        if (u8) hipLaunchKernelGGL(linear_develop<uint8_t>, grid, blk, 0, st, A);
        else hipLaunchKernelGGL(linear_develop<uint16_t>, grid, blk, 0, st, A);
        return;
    }
    LinearDevelopArgs A{};
    A.src = src; A.dst = dst; A.npx = npx; A.lin = lin;
    for (int k = 0; k < 9; ++k) A.mq[k] = dev->matrix_q[k];
    A.tone = dev->dev_tone;
    if (mat && tone) {
        if (u8) hipLaunchKernelGGL((linear_develop<uint8_t, true, true>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((linear_develop<uint16_t, true, true>), grid, blk, 0, st, A);
    } else if (mat) {
        if (u8) hipLaunchKernelGGL((linear_develop<uint8_t, true, false>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((linear_develop<uint16_t, true, false>), grid, blk, 0, st, A);
    } else {
        if (u8) hipLaunchKernelGGL((linear_develop<uint8_t, false, true>), grid, blk, 0, st, A);
        else hipLaunchKernelGGL((linear_develop<uint16_t, false, true>), grid, blk, 0, st, A);
    }
}

}  // namespace mi
