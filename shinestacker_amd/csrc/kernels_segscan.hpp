// kernels_segscan.hpp -- a segmented inclusive sum over uint32 words, the one helper of the split decoders
// (kernels_split_common.hpp): lanes per unit, counts per lane, the JPEG decoder's DC differences.
#pragma once
#include "common.hpp"

namespace mi {

// ---- a segmented inclusive sum over uint32 words: bits 0 .. 30 the value (sums mod 2^31), bit 31 set where a segment starts.
// Three kernels a level: the blocks of 1024 scan themselves, their totals are scanned the same way (recursively), and every
// block takes its predecessors' total in.  Integer addition is associative, so the result does not depend on the grouping.
namespace segscan {
constexpr uint32_t HEAD = 0x80000000u, MASK = 0x7fffffffu;
constexpr int THREADS = 256, ITEMS = 4, BLOCK = THREADS * ITEMS;
__host__ __device__ inline uint32_t op(uint32_t a, uint32_t b) { return (b & HEAD) ? b : ((a & HEAD) | ((a + b) & MASK)); }

__global__ __launch_bounds__(THREADS) void seg_scan_block(uint32_t* v, size_t n, uint32_t* totals) {
    __shared__ uint32_t part[THREADS];
    const int t = (int)threadIdx.x;
    const size_t at = ((size_t)blockIdx.x * THREADS + t) * ITEMS;
    uint32_t x[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) x[i] = at + i < n ? v[at + i] : 0u;
#pragma unroll
    for (int i = 1; i < ITEMS; ++i) x[i] = op(x[i - 1], x[i]);
    part[t] = x[ITEMS - 1];
    __syncthreads();
#pragma unroll
    for (int d = 1; d < THREADS; d <<= 1) {
        const uint32_t mine = part[t], left = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] = op(left, mine);
        __syncthreads();
    }
    const uint32_t before = t ? part[t - 1] : 0u;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i)
        if (at + i < n) v[at + i] = op(before, x[i]);
    if (t == THREADS - 1) totals[blockIdx.x] = part[t];
}

__global__ __launch_bounds__(THREADS) void seg_scan_carry(uint32_t* v, size_t n, const uint32_t* totals) {
    if (blockIdx.x == 0) return;
    const uint32_t carry = totals[blockIdx.x - 1];
    const size_t at = ((size_t)blockIdx.x * THREADS + threadIdx.x) * ITEMS;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i)
        if (at + i < n) v[at + i] = op(carry, v[at + i]);
}

inline size_t blocks(size_t n) { return (n + BLOCK - 1) / BLOCK; }
// the words of scratch a scan of n words needs
inline size_t tmp_words(size_t n) {
    size_t w = 0;
    while (n > 1) {
        n = blocks(n);
        w += (n + 63) & ~(size_t)63;
    }
    return w + 64;
}
inline void launch(hipStream_t st, uint32_t* v, size_t n, uint32_t* tmp) {
    if (n == 0) return;
    const size_t nb = blocks(n);
    hipLaunchKernelGGL(seg_scan_block, dim3((unsigned)nb), dim3(THREADS), 0, st, v, n, tmp);
    if (nb > 1) {
        launch(st, tmp, nb, tmp + ((nb + 63) & ~(size_t)63));
        hipLaunchKernelGGL(seg_scan_carry, dim3((unsigned)nb), dim3(THREADS), 0, st, v, n, (const uint32_t*)tmp);
    }
}
}  // namespace segscan

}  // namespace mi
