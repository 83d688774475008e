// prestack_time.hip -- vignette_apply against the device-to-device copy of the same buffers, in one process.
//
//   hipcc --offload-arch=gfx950 -O2 -I include tools/prestack_time.hip -L shinestacker_amd/csrc -lmi355stack \
//         -Wl,-rpath,'$ORIGIN/../shinestacker_amd/csrc' -o tools/prestack_time
//   tools/prestack_time [launches per round = 20] [rounds = 3]
//
// The kernel is launched through the library's own entry point (mi_vignette_apply_device), so the grid is the shipped one.
// Per size (24 MP uint8, 50 MP uint16): warm-up, then `rounds` times alternately `launches` copies and `launches` applies,
// each group between two hipEvents.  Rates count bytes read + bytes written; "of copy" is apply rate / copy rate.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <vector>

#include "mi355stack.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ void fill(uint32_t* p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t x = (uint32_t)i * 0x9e3779b9u;
        x ^= x >> 15;
        p[i] = (x & 0x7f7f7f7fu) + 0x20202020u;   // every byte in [32, 159]: never under the black threshold
    }
}

static double model(double r, double i0, double k, double r0) {
    double t = k * (r - r0);
    t = t < -10 ? -10 : (t > 10 ? 10 : t);
    double e = exp(t);
    return i0 / (1.0 + exp(e > 10 ? 10 : e));
}

int main(int argc, char** argv) {
    const int launches = argc > 1 ? atoi(argv[1]) : 20, rounds = argc > 2 ? atoi(argv[2]) : 3;
    struct Case { const char* name; int h, w, dtype, size; } cases[] = {
        {"24 MP uint8", 4000, 6000, MI_U8, 1}, {"50 MP uint16", 5792, 8688, MI_U16, 2}};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (const Case& c : cases) {
        const size_t bytes = (size_t)c.h * c.w * 3 * c.size;
        void *src = nullptr, *dst = nullptr;
        CK(hipMalloc(&src, bytes));
        CK(hipMalloc(&dst, bytes));
        hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, (uint32_t*)src, bytes / 4);
        const double r_max = sqrt((c.w / 2.0) * (c.w / 2.0) + (c.h / 2.0) * (c.h / 2.0));
        const double i0 = 320.0, k = 6.0 / r_max, r0 = 0.75 * r_max, v0 = model(0, i0, k, r0);
        auto apply = [&]() {
            return mi_vignette_apply_device(0, nullptr, src, dst, c.h, c.w, c.dtype, i0, k, r0, v0, 1.0, c.size == 1 ? 1.0 : 256.0);
        };
        for (int i = 0; i < 3; ++i) {
            CK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, 0));
            if (apply()) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
        }
        CK(hipDeviceSynchronize());
        for (int r = 0; r < rounds; ++r) {
            float ms_copy = 0, ms_apply = 0;
            CK(hipEventRecord(e0, 0));
            for (int i = 0; i < launches; ++i) CK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, 0));
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms_copy, e0, e1));
            CK(hipEventRecord(e0, 0));
            for (int i = 0; i < launches; ++i) if (apply()) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms_apply, e0, e1));
            const double gb = 2.0 * bytes * launches / 1e9;
            printf("%s round %d: copy %.1f us %.0f GB/s | vignette_apply %.1f us %.0f GB/s | %.2f of copy\n", c.name, r,
                   1e3 * ms_copy / launches, gb / (ms_copy / 1e3), 1e3 * ms_apply / launches, gb / (ms_apply / 1e3), ms_copy / ms_apply);
        }
        if (c.size == 1) {   // frame_accumulate: 8 uint8 frames into the uint32 sums, against a copy of the bytes it reads + writes
            const int nf = 8;
            const size_t el = bytes, moved = nf * el + 2 * 4 * el;
            void *fr = nullptr, *sum = nullptr, *sink = nullptr;
            CK(hipMalloc(&fr, nf * el));
            CK(hipMalloc(&sum, 4 * el));
            CK(hipMalloc(&sink, moved / 2));
            CK(hipMemset(sum, 0, 4 * el));
            for (int f = 0; f < nf; ++f) CK(hipMemcpy((char*)fr + f * el, src, el, hipMemcpyDeviceToDevice));
            if (mi_frame_accumulate_device(0, nullptr, fr, nf, el, sum)) { fprintf(stderr, "%s\n", mi_last_error()); return 1; }
            CK(hipDeviceSynchronize());
            for (int r = 0; r < rounds; ++r) {
                float ms_copy = 0, ms_acc = 0;
                CK(hipEventRecord(e0, 0));
                for (int i = 0; i < launches; ++i) CK(hipMemcpyAsync(sink, fr, moved / 2, hipMemcpyDeviceToDevice, 0));
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                CK(hipEventElapsedTime(&ms_copy, e0, e1));
                CK(hipMemset(sum, 0, 4 * el));
                CK(hipEventRecord(e0, 0));
                for (int i = 0; i < launches; ++i) if (mi_frame_accumulate_device(0, nullptr, fr, nf, el, sum)) return 1;
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                CK(hipEventElapsedTime(&ms_acc, e0, e1));
                const double gb = (double)moved * launches / 1e9;
                printf("%s round %d: copy of the same bytes %.1f us %.0f GB/s | frame_accumulate (8 frames) %.1f us %.0f GB/s | %.2f of copy\n",
                       c.name, r, 1e3 * ms_copy / launches, gb / (ms_copy / 1e3), 1e3 * ms_acc / launches, gb / (ms_acc / 1e3), ms_copy / ms_acc);
            }
            CK(hipFree(fr)); CK(hipFree(sum)); CK(hipFree(sink));
        }
        CK(hipFree(src));
        CK(hipFree(dst));
    }
    return 0;
}
