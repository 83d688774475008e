// unsharp_time.hip -- the retouch filters on full-size frames, hipEvents over warm runs: the unsharp kernel
// (mi_unsharp_mask_device) at radius 1, 2 and 4 in both branches, the white-balance table apply (mi_apply_lut_device with
// one table per channel), and a device-to-device copy of the same frame taken in the same run.  Each filter reads and
// writes the frame once, so the copy is its floor; every line reports the ratio to it.
//
//   hipcc --offload-arch=gfx950 -O2 -I include tools/unsharp_time.hip -L shinestacker_amd/csrc -lmi355stack \
//         -Wl,-rpath,'$ORIGIN/../shinestacker_amd/csrc' -o tools/unsharp_time
//   tools/unsharp_time [runs per case = 20]
//
// Frames: a smooth integer texture with block edges plus hash noise of +-6 counts.  The taps are built here by the rule
// shinestacker_amd/sharpen.py uses (double exp, error-diffused fixed point).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <functional>
#include <vector>

#include "mi355stack.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <typename T>
__global__ void fill(T* p, int h, int w) {
    const size_t n = (size_t)h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / w), x = (int)(i % w);
        const int tri = abs((x + 2 * y) % 240 - 120) + ((x / 50 + y / 40) & 1) * 60;     // 0 .. 180
        for (int c = 0; c < 3; ++c) {
            uint32_t v = (uint32_t)(i * 3 + c) * 0x9e3779b9u;
            v ^= v >> 15; v *= 0x2c1b3c6du; v ^= v >> 12;
            const int val = 30 + tri + 10 * c + (int)(v % 13u) - 6;
            p[i * 3 + c] = sizeof(T) == 1 ? (T)val : (T)((val << 8) | (v >> 24));
        }
    }
}

static std::vector<uint32_t> taps_for(bool u16, double sigma) {
    const int ksize = (int)nearbyint(sigma * (u16 ? 8 : 6) + 1) | 1, n2 = (ksize - 1) / 2, bits = u16 ? 16 : 8;
    std::vector<double> t(n2 + 1);
    const double scale2x = -0.125 / (sigma * sigma);
    double sum = 0;
    for (int i = 0, x = 1 - ksize; i < n2; ++i, x += 2) sum += t[i] = exp((double)(x * x) * scale2x);
    const double mul1 = 1.0 / (sum * 2.0 + 1.0), fixed_1 = (double)(1u << bits);
    std::vector<uint32_t> k(ksize);
    long long acc = 0;
    double carry = 0;
    for (int i = 0; i < n2; ++i) {
        const double adj = t[i] * mul1 * fixed_1 + carry;
        const long long v = (long long)nearbyint(adj);
        carry = adj - (double)v;
        k[i] = k[ksize - 1 - i] = (uint32_t)v;
        acc += 2 * v;
    }
    k[n2] = (uint32_t)((1LL << bits) - acc);
    return k;
}

int main(int argc, char** argv) {
    const int runs = argc > 1 ? atoi(argv[1]) : 20;
    struct Frame { const char* name; int h, w, dtype; } frames[] = {{"4000 x 6000 uint8 ", 4000, 6000, MI_U8}, {"5760 x 8640 uint16", 5760, 8640, MI_U16}};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (const Frame& f : frames) {
        const bool u16 = f.dtype == MI_U16;
        const size_t bytes = (size_t)f.h * f.w * 3 * (u16 ? 2 : 1);
        void *src = nullptr, *dst = nullptr, *lut = nullptr;
        CK(hipMalloc(&src, bytes));
        CK(hipMalloc(&dst, bytes));
        if (u16) hipLaunchKernelGGL(fill<uint16_t>, dim3(4096), dim3(256), 0, 0, (uint16_t*)src, f.h, f.w);
        else hipLaunchKernelGGL(fill<uint8_t>, dim3(4096), dim3(256), 0, 0, (uint8_t*)src, f.h, f.w);
        // a white-balance table: channel c scaled by 1.06 / 1.0 / 0.81, clipped (the values do not change the time)
        const int nbins = u16 ? 65536 : 256;
        std::vector<uint8_t> host_lut((size_t)3 * nbins * (u16 ? 2 : 1));
        const double scale[3] = {0.81, 1.0, 1.06};
        for (int c = 0; c < 3; ++c)
            for (int v = 0; v < nbins; ++v) {
                double s = v * scale[c];
                s = s > nbins - 1 ? nbins - 1 : s;
                if (u16) ((uint16_t*)host_lut.data())[c * nbins + v] = (uint16_t)s; else host_lut[c * nbins + v] = (uint8_t)s;
            }
        CK(hipMalloc(&lut, host_lut.size()));
        CK(hipMemcpy(lut, host_lut.data(), host_lut.size(), hipMemcpyHostToDevice));

        float copy_ms = 0;
        auto measure = [&](const char* what, const std::function<int()>& run) -> int {
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
            const float mean = total / runs;
            if (copy_ms == 0) copy_ms = mean;
            printf("%s %-34s mean %7.3f ms best %7.3f ms over %d runs | %5.2f x the copy | %.0f GB/s read + written\n", f.name, what, mean,
                   best, runs, mean / copy_ms, 2e-6 * bytes / mean);
            return 0;
        };
        if (measure("device-to-device copy", [&]() { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, 0) == hipSuccess ? 0 : 1; })) return 1;
        if (measure("white-balance table apply", [&]() { return mi_apply_lut_device(0, nullptr, src, dst, (size_t)f.h * f.w, f.dtype, lut, 3); })) return 1;
        for (double radius : {1.0, 2.0, 4.0})
            for (double threshold : {0.0, 10.0}) {
                const std::vector<uint32_t> taps = taps_for(u16, radius);
                char what[96];
                snprintf(what, sizeof what, "unsharp radius %.0f (%2zu taps) %s", radius, taps.size(), threshold ? "threshold" : "addWeighted");
                if (measure(what, [&]() { return mi_unsharp_mask_device(0, nullptr, src, dst, f.h, f.w, f.dtype, taps.data(), (int)taps.size(), 1.0,
                                                                         threshold * (u16 ? 256 : 1)); })) return 1;
            }
        CK(hipFree(src));
        CK(hipFree(dst));
        CK(hipFree(lut));
    }
    return 0;
}
