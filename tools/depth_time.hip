// depth_time.hip -- the depth map's weighted smoothing (csrc/kernels_depth.hpp: ws_rows + ws_cols) on a full-size plane pair,
// hipEvents over warm runs, against a device-to-device copy of the same two planes (index + energy, 8 B/px) taken in the
// same run.  The kernels move 28 B/px (float) / 44 B/px (double) against the copy's 16; every line reports the ratio.
//
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I include -I shinestacker_amd/csrc tools/depth_time.hip -o tools/depth_time
//   tools/depth_time [runs per case = 20]
//
// Planes: a banded winner index (8 frames) with hash noise, energies from a hash with patches of zeros.  The kernels are the
// library's own templates, included here, so that the time is the kernels' and not mi_weighted_smooth's uploads.
#include <stdarg.h>
#include <math.h>

#include <functional>

#include "kernels_depth.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ void fill(int32_t* idx, float* en, int h, int w) {
    const size_t n = (size_t)h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / w), x = (int)(i % w);
        const uint32_t v = mi::lowbias32((uint32_t)i);
        idx[i] = ((y * 8) / h + (int)(v % 3u)) % 8;
        en[i] = ((x / 200 + y / 150) % 7 == 0) ? 0.0f : (float)(v >> 8) * 0.37f;
    }
}

int main(int argc, char** argv) {
    const int runs = argc > 1 ? atoi(argv[1]) : 20;
    struct Plane { const char* name; int h, w; } planes[] = {{"4000 x 6000", 4000, 6000}, {"5760 x 8640", 5760, 8640}};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (const Plane& f : planes) {
        const size_t np = (size_t)f.h * f.w;
        int32_t *idx = nullptr, *idx2 = nullptr;
        float *en = nullptr, *en2 = nullptr, *out = nullptr;
        void *P = nullptr, *Q = nullptr;
        CK(hipMalloc(&idx, np * 4));
        CK(hipMalloc(&en, np * 4));
        CK(hipMalloc(&idx2, np * 4));
        CK(hipMalloc(&en2, np * 4));
        CK(hipMalloc(&out, np * 4));
        CK(hipMalloc(&P, np * 8));
        CK(hipMalloc(&Q, np * 8));
        hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, idx, en, f.h, f.w);
        float copy_ms = 0;
        auto measure = [&](const char* what, double bytes, const std::function<int()>& run) -> int {
            for (int i = 0; i < 3; ++i) if (run()) return 1;
            CK(hipDeviceSynchronize());
            float best = 1e30f, total = 0;
            for (int i = 0; i < runs; ++i) {
                float ms = 0;
                CK(hipEventRecord(e0, 0));
                if (run()) return 1;
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                CK(hipEventElapsedTime(&ms, e0, e1));
                best = ms < best ? ms : best;
                total += ms;
            }
            const float mean = total / runs;
            if (copy_ms == 0) copy_ms = mean;
            printf("%s %-40s mean %7.3f ms best %7.3f ms over %d runs | %5.2f x the copy | %.0f GB/s of the bytes it moves\n", f.name, what,
                   mean, best, runs, mean / copy_ms, 1e-6 * bytes / mean);
            return 0;
        };
        if (measure("device-to-device copy of both planes", 16.0 * np, [&]() {
                return hipMemcpyAsync(idx2, idx, np * 4, hipMemcpyDeviceToDevice, 0) == hipSuccess &&
                       hipMemcpyAsync(en2, en, np * 4, hipMemcpyDeviceToDevice, 0) == hipSuccess ? 0 : 1; })) return 1;
        if (measure("sigma 0 (index as float32)", 8.0 * np, [&]() {
                mi::ws_passthrough_launch<int32_t, float>(0, idx, np, 0, 1, out);
                return hipGetLastError() == hipSuccess ? 0 : 1; })) return 1;
        for (double sigma : {1.0, 2.0, 4.0, 16.0}) {
            double taps[MI_WS_MAX_TAPS];
            const int radius = mi::ws_gaussian_taps(sigma, taps);
            char what[96];
            snprintf(what, sizeof what, "sigma %2.0f (%2d taps) float", sigma, 2 * radius + 1);
            if (measure(what, 28.0 * np, [&]() {
                    mi::ws_smooth_launch<int32_t, float, float>(0, idx, en, f.h, f.w, radius, taps, 0, 1, (float*)P, (float*)Q, out);
                    return hipGetLastError() == hipSuccess ? 0 : 1; })) return 1;
            snprintf(what, sizeof what, "sigma %2.0f (%2d taps) double", sigma, 2 * radius + 1);
            if (measure(what, 44.0 * np, [&]() {
                    mi::ws_smooth_launch<int32_t, float, double>(0, idx, en, f.h, f.w, radius, taps, 0, 1, (double*)P, (double*)Q, out);
                    return hipGetLastError() == hipSuccess ? 0 : 1; })) return 1;
        }
        for (void* p : {(void*)idx, (void*)en, (void*)idx2, (void*)en2, (void*)out, P, Q}) CK(hipFree(p));
    }
    return 0;
}
