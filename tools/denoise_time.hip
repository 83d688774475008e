// denoise_time.hip -- the post-stack denoise kernel (mi_nlm_denoise_device) on full-size frames, hipEvents over warm runs.
//
//   hipcc --offload-arch=gfx950 -O2 -I include tools/denoise_time.hip -L shinestacker_amd/csrc -lmi355stack \
//         -Wl,-rpath,'$ORIGIN/../shinestacker_amd/csrc' -o tools/denoise_time
//   tools/denoise_time [runs per case = 20] [only case index]
//
// Frames: a smooth integer texture plus hash noise of +-6 counts (so that the table look-ups hit non-zero weights, as on
// a real stack result).  The table is built here the way shinestacker_amd/denoise.py builds it (long double exp, rounded
// once); h = 3 (uint16: 768).  The entry point allocates, uploads and frees its table and synchronises per call; that is
// inside the measured time, as it is for a caller.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <vector>

#include "mi355stack.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <typename T>
__global__ void fill(T* p, int h, int w) {
    const size_t n = (size_t)h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / w), x = (int)(i % w);
        const int tri = abs((x + 2 * y) % 240 - 120) + ((x / 500 + y / 400) & 1) * 30;     // 0 .. 150
        for (int c = 0; c < 3; ++c) {
            uint32_t v = (uint32_t)(i * 3 + c) * 0x9e3779b9u;
            v ^= v >> 15; v *= 0x2c1b3c6du; v ^= v >> 12;
            const int val = 50 + tri + 10 * c + (int)(v % 13u) - 6;
            p[i * 3 + c] = sizeof(T) == 1 ? (T)val : (T)((val << 8) | (v >> 24));
        }
    }
}

static std::vector<uint32_t> table_for(bool u16, double h, int tpl, int search, int* shift) {
    const int t = tpl / 2, s = search / 2, n = (2 * t + 1) * (2 * t + 1);
    *shift = 0;
    while ((1 << *shift) < n) ++*shift;
    const double mult = (double)(1 << *shift) / n;
    const long long sw2 = (2 * s + 1) * (2 * s + 1);
    const long long fpm = u16 ? 2147483647LL : 2147483647LL / (sw2 * 255);
    const float hf = (float)h, den = hf * hf * 3;
    std::vector<uint32_t> tab;
    for (int a = 0;; ++a) {
        const double dist = a * mult;
        const double w = (double)expl(-(long double)(u16 ? dist * dist : dist) / (long double)den);
        const double weight = nearbyint(fpm * w);
        if (weight < 0.001 * fpm) break;
        tab.push_back((uint32_t)weight);
    }
    return tab;
}

int main(int argc, char** argv) {
    const int runs = argc > 1 ? atoi(argv[1]) : 20, only = argc > 2 ? atoi(argv[2]) : -1;
    struct Case { const char* name; int h, w, dtype, tpl, search; } cases[] = {
        {"4000 x 6000 uint8  template 7 search 21", 4000, 6000, MI_U8, 7, 21}, {"4000 x 6000 uint8  template 3 search 21", 4000, 6000, MI_U8, 3, 21},
        {"5760 x 8640 uint16 template 7 search 21", 5760, 8640, MI_U16, 7, 21}, {"5760 x 8640 uint16 template 3 search 21", 5760, 8640, MI_U16, 3, 21}};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    int idx = 0;
    for (const Case& c : cases) {
        if (only >= 0 && only != idx++) continue;
        const bool u16 = c.dtype == MI_U16;
        const size_t bytes = (size_t)c.h * c.w * 3 * (u16 ? 2 : 1);
        void *src = nullptr, *dst = nullptr;
        CK(hipMalloc(&src, bytes));
        CK(hipMalloc(&dst, bytes));
        if (u16) hipLaunchKernelGGL(fill<uint16_t>, dim3(4096), dim3(256), 0, 0, (uint16_t*)src, c.h, c.w);
        else hipLaunchKernelGGL(fill<uint8_t>, dim3(4096), dim3(256), 0, 0, (uint8_t*)src, c.h, c.w);
        int shift = 0;
        const std::vector<uint32_t> tab = table_for(u16, u16 ? 768.0 : 3.0, c.tpl, c.search, &shift);
        auto run = [&]() { return mi_nlm_denoise_device(0, src, dst, c.h, c.w, c.dtype, tab.data(), (int)tab.size(), shift, c.tpl, c.search, nullptr); };
        for (int i = 0; i < 3; ++i) if (run()) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
        CK(hipDeviceSynchronize());
        float best = 1e30f, total = 0;
        for (int i = 0; i < runs; ++i) {
            float ms = 0;
            CK(hipEventRecord(e0, 0));
            if (run()) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms, e0, e1));
            best = ms < best ? ms : best;
            total += ms;
        }
        const double offsets = (2 * (c.search / 2) + 1) * (2 * (c.search / 2) + 1), px = (double)c.h * c.w;
        printf("%s: table %zu entries | mean %.2f ms best %.2f ms over %d runs | %.2f ns per pixel | %.1f ps per pixel-offset\n", c.name,
               tab.size(), total / runs, best, runs, 1e6 * (total / runs) / px, 1e9 * (total / runs) / (px * offsets));
        CK(hipFree(src));
        CK(hipFree(dst));
    }
    return 0;
}
