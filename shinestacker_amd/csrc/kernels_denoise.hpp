// kernels_denoise.hpp -- the post-stack denoise of the reference (algorithms/denoise.py): cv2.fastNlMeansDenoising on a
// three-channel frame, the way OpenCV's FastNlMeansDenoisingInvoker computes it for that call [from memory, unpinned: no
// OpenCV was at hand; tests/nlm_restatement.py states the same rule in NumPy and the kernel is held to it bit for bit]:
//
//   t = template / 2, s = search / 2, n = (2t + 1)^2, shift = smallest p with 2^p >= n
//   d(p, q)  = sum over the (2t + 1)^2 patch and the 3 channels of (a - b)^2 [uint8, NORM_L2] or |a - b| [uint16, NORM_L1]
//   weight   = table[d >> shift]                 (the table comes from the caller; entries past its length are zero)
//   out[p,c] = (sum_q weight * I[q,c] + W / 2) / W,  W = sum_q weight, q over the (2s + 1)^2 search window, unsigned division
//   borders: BORDER_REFLECT_101 over s + t pixels, reflected as often as it takes when the frame is smaller than that
//
// One workgroup of 256 owns a 32 x 32 output tile and stages it with its s + t halo in LDS once, one packed pixel per
// word (uint8: B | G << 8 | R << 16; uint16: two words).  Every one of the (2s + 1)^2 offsets is then served from LDS in
// three phases: the channel-summed difference of the tile + t halo, its horizontal box sum, and per thread a sliding
// vertical box sum over four rows with the table look-up and the weighted sums in registers.  Two barriers per offset:
// the difference plane is rewritten only after the barrier behind its last reader, and so is the row-sum plane.
// Everything is integer: uint8 sums fit 32 bits by the table's construction (fixed-point multiplier INT_MAX / (search^2 * 255)),
// uint16 sums are 64-bit.
#pragma once
#include "common.hpp"

namespace mi {

#define MI_NLM_TILE 32
#define MI_NLM_MAX_T 5      // template window up to 11
#define MI_NLM_MAX_S 10     // search window up to 21
#define MI_NLM_LDS_LIMIT 65536

struct NlmArgs {
    const void* src;        // H x W x 3
    void* dst;              // H x W x 3, != src
    int h, w;
    int s;                  // search half size
    int shift;
    const uint32_t* table;  // device, table_len entries
    uint32_t table_len;
    int table_in_lds;
};

// cv::borderInterpolate(p, len, BORDER_REFLECT_101): any p ends inside [0, len)
__device__ __forceinline__ int nlm_reflect101(int p, int len) {
    if (len == 1) return 0;
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

template <typename T> struct NlmPix;

template <> struct NlmPix<uint8_t> {
    using P = uint32_t;
    using Acc = uint32_t;
    static __device__ __forceinline__ P load(const uint8_t* p) { return (P)p[0] | ((P)p[1] << 8) | ((P)p[2] << 16); }
    static __device__ __forceinline__ uint32_t dist(P a, P b) {
        const int d0 = (int)(a & 255u) - (int)(b & 255u), d1 = (int)((a >> 8) & 255u) - (int)((b >> 8) & 255u),
                  d2 = (int)(a >> 16) - (int)(b >> 16);
        return (uint32_t)(d0 * d0 + d1 * d1 + d2 * d2);
    }
    static __device__ __forceinline__ void acc(Acc* e, uint32_t wt, P q) {
        e[0] += wt * (q & 255u);
        e[1] += wt * ((q >> 8) & 255u);
        e[2] += wt * (q >> 16);
    }
};

template <> struct NlmPix<uint16_t> {
    using P = uint2;
    using Acc = unsigned long long;
    static __device__ __forceinline__ P load(const uint16_t* p) { return make_uint2((uint32_t)p[0] | ((uint32_t)p[1] << 16), p[2]); }
    static __device__ __forceinline__ uint32_t absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
    static __device__ __forceinline__ uint32_t dist(P a, P b) {
        return absdiff(a.x & 0xffffu, b.x & 0xffffu) + absdiff(a.x >> 16, b.x >> 16) + absdiff(a.y, b.y);
    }
    static __device__ __forceinline__ void acc(Acc* e, uint32_t wt, P q) {
        e[0] += (Acc)wt * (q.x & 0xffffu);
        e[1] += (Acc)wt * (q.x >> 16);
        e[2] += (Acc)wt * q.y;
    }
};

template <int TH> constexpr int nlm_dw() { return MI_NLM_TILE + 2 * TH; }

// dynamic LDS of one workgroup without the table
inline size_t nlm_lds_bytes(int dtype, int th, int s) {
    const size_t iw = MI_NLM_TILE + 2 * (size_t)(s + th), dw = MI_NLM_TILE + 2 * (size_t)th;
    return iw * iw * (dtype == MI_U8 ? 4 : 8) + 4 * (dw * dw + dw * MI_NLM_TILE);
}

template <typename T, int TH>
__global__ __launch_bounds__(256) void nlm_denoise(NlmArgs a) {
    using PX = NlmPix<T>;
    using P = typename PX::P;
    using Acc = typename PX::Acc;
    constexpr int TILE = MI_NLM_TILE, DW = nlm_dw<TH>(), ROWS = 4;
    extern __shared__ uint4 nlm_smem[];
    const int s = a.s, halo = s + TH, iw = TILE + 2 * halo;
    P* img = (P*)nlm_smem;                                  // iw x iw packed pixels, origin (tile - halo)
    uint32_t* dpl = (uint32_t*)(img + iw * iw);             // DW x DW differences, origin (tile - TH)
    uint32_t* hpl = dpl + DW * DW;                          // DW x TILE horizontal box sums
    uint32_t* tab = hpl + DW * TILE;                        // the table, when it fits
    const int tid = (int)threadIdx.x;
    const int ty0 = (int)blockIdx.y * TILE, tx0 = (int)blockIdx.x * TILE;
    const T* src = (const T*)a.src;

    for (int i = tid; i < iw * iw; i += 256) {
        const int ly = i / iw, lx = i - ly * iw;
        const int gy = nlm_reflect101(ty0 + ly - halo, a.h), gx = nlm_reflect101(tx0 + lx - halo, a.w);
        img[i] = PX::load(src + ((size_t)gy * a.w + gx) * 3);
    }
    if (a.table_in_lds)
        for (uint32_t i = tid; i < a.table_len; i += 256) tab[i] = a.table[i];
    __syncthreads();

    const int x = tid & 31, y0 = (tid >> 5) * ROWS;     // this thread's outputs: column x, rows y0 .. y0 + 3 of the tile
    Acc est[ROWS][3], wsum[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) est[r][0] = est[r][1] = est[r][2] = wsum[r] = 0;

    for (int dy = -s; dy <= s; ++dy) {
        for (int dx = -s; dx <= s; ++dx) {
            // A: difference of every pixel of the tile + TH halo against its partner at (dy, dx)
            const int off = dy * iw + dx;
            for (int i = tid; i < DW * DW; i += 256) {
                const int ry = i / DW, rx = i - ry * DW;
                const int at = (ry + s) * iw + rx + s;
                dpl[i] = PX::dist(img[at], img[at + off]);
            }
            __syncthreads();
            // B: horizontal box sums, hpl[ry][cx] = sum of dpl[ry][cx .. cx + 2 TH]
            for (int i = tid; i < DW * TILE; i += 256) {
                const int ry = i >> 5, cx = i & 31;
                uint32_t sum = 0;
#pragma unroll
                for (int j = 0; j <= 2 * TH; ++j) sum += dpl[ry * DW + cx + j];
                hpl[i] = sum;
            }
            __syncthreads();
            // C: sliding vertical box sum, table, weighted sums
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j <= 2 * TH; ++j) v += hpl[(y0 + j) * TILE + x];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                if (r) v += hpl[(y0 + 2 * TH + r) * TILE + x] - hpl[(y0 + r - 1) * TILE + x];
                const uint32_t ad = v >> a.shift;
                uint32_t wt = 0;
                if (ad < a.table_len) wt = a.table_in_lds ? tab[ad] : a.table[ad];
                PX::acc(est[r], wt, img[(y0 + r + halo) * iw + x + halo + off]);
                wsum[r] += wt;
            }
        }
    }

    T* dst = (T*)a.dst;
    const int gx = tx0 + x;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int gy = ty0 + y0 + r;
        if (gy < a.h && gx < a.w) {
            T* o = dst + ((size_t)gy * a.w + gx) * 3;
            const Acc ws = wsum[r];     // >= table[0] > 0: the pixel itself is in its search window
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = (T)((est[r][c] + ws / 2) / ws);
        }
    }
}

template <typename T>
inline void nlm_launch_t(hipStream_t st, dim3 grid, size_t lds, int th, const NlmArgs& a) {
    switch (th) {
        case 0: hipLaunchKernelGGL((nlm_denoise<T, 0>), grid, dim3(256), lds, st, a); break;
        case 1: hipLaunchKernelGGL((nlm_denoise<T, 1>), grid, dim3(256), lds, st, a); break;
        case 2: hipLaunchKernelGGL((nlm_denoise<T, 2>), grid, dim3(256), lds, st, a); break;
        case 3: hipLaunchKernelGGL((nlm_denoise<T, 3>), grid, dim3(256), lds, st, a); break;
        case 4: hipLaunchKernelGGL((nlm_denoise<T, 4>), grid, dim3(256), lds, st, a); break;
        default: hipLaunchKernelGGL((nlm_denoise<T, 5>), grid, dim3(256), lds, st, a); break;
    }
}

// th <= MI_NLM_MAX_T, s <= MI_NLM_MAX_S, table on the device; the caller has validated everything
inline void nlm_launch(hipStream_t st, const void* src, void* dst, int h, int w, int dtype, const uint32_t* dev_table,
                       uint32_t table_len, int shift, int th, int s) {
    NlmArgs a{};
    a.src = src; a.dst = dst; a.h = h; a.w = w; a.s = s; a.shift = shift; a.table = dev_table; a.table_len = table_len;
    size_t lds = nlm_lds_bytes(dtype, th, s);
    a.table_in_lds = lds + 4 * (size_t)table_len <= MI_NLM_LDS_LIMIT ? 1 : 0;
    if (a.table_in_lds) lds += 4 * (size_t)table_len;
    const dim3 grid((unsigned)cdiv(w, MI_NLM_TILE), (unsigned)cdiv(h, MI_NLM_TILE));
    if (dtype == MI_U8) nlm_launch_t<uint8_t>(st, grid, lds, th, a);
    else nlm_launch_t<uint16_t>(st, grid, lds, th, a);
}

}  // namespace mi
