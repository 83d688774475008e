// capi.hip -- C ABI of libmi355stack.so (declared in include/mi355stack.h).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -shared -fPIC
#include <stdarg.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "common.hpp"
#include "host_scratch.hpp"
#include "kernels_simple.hpp"
#include "kernels_tiled.hpp"
#include "kernels_sep.hpp"
#include "kernels_align.hpp"
#include "kernels_ecc.hpp"
#include "kernels_phase.hpp"
#include "kernels_balance.hpp"
#include "kernels_prestack.hpp"
#include "kernels_denoise.hpp"
#include "kernels_unsharp.hpp"
#include "kernels_depth.hpp"
#include "kernels_guided.hpp"
#include "kernels_stereo.hpp"
#include "kernels_brush.hpp"
#include "kernels_composite.hpp"
#include "kernels_f64.hpp"
#include "kernels_steps.hpp"
#include "kernels_lens.hpp"
#include "kernels_finish.hpp"
#include "kernels_jpeg.hpp"
#include "kernels_jpeg_split.hpp"
#include "kernels_ljpeg_split.hpp"

using namespace mi;

struct mi_stack;
namespace mi {
// LDS-tiled production path + host-frame staging (tiled_host.hpp)
int tiled_create(mi_stack* s);
void tiled_destroy(mi_stack* s);
int tiled_reset(mi_stack* s);
int tiled_pending(const mi_stack* s);
void tiled_side_streams(const mi_stack* s, hipStream_t out[2]);
int tiled_push(mi_stack* s, const void* dev_frames, int n, size_t stride);
int tiled_push_host(mi_stack* s, const void* host_bgr, size_t row_stride_bytes, bool pinned = false);
int tiled_wait_uploads(mi_stack* s, int max_outstanding);
int tiled_flush(mi_stack* s);
int tiled_sync_all(mi_stack* s);
int tiled_sync_level0(mi_stack* s);
const float* tiled_last_gauss(mi_stack* s, int level);
int dispatch_push(mi_stack* s, const void* dev_frames, int n, size_t stride);
}  // namespace mi

namespace {

size_t dtype_size(int dt) {
    switch (dt) {
        case MI_U8: return 1;
        case MI_U16: return 2;
        case MI_F32: return 4;
        case MI_F64: return 8;
    }
    return 0;
}

struct ProfRec {
    int kind;
    hipEvent_t a, b;
    double bytes;
    int launches = 1;   // kernel launches between the two events (consecutive launches of one level share a pair)
};

}  // namespace

struct mi_stack {
    mi_stack_params_t p{};
    int L = 0;                // number of Laplacian levels; base is level L
    std::vector<int> lh, lw;  // level shapes, 0..L
    K25 K{};
    float k1d[3] = {0.f, 0.f, 0.f};   // MI_ARITH_SEPARABLE: float32 of the 1-D generating kernel (k0, k1, k2)
    float rk[4] = {0.f, 0.f, 0.f, 1.f};   // MI_ARITH_SEPARABLE, reduce: taps (w0, w1, w2) and final scale (red_taps)
    bool sep = false;         // p.arith == MI_ARITH_SEPARABLE
    K25d Kd{};                // float-64 mode: the float64 generating kernel (np.outer, pyramid.py:21)
    bool f64 = false;         // float_type == MI_F64: float buffers below hold doubles (allocated twice as large)
    int pad = 2;
    int nlevels_hist = 256;
    float maxv = 255.f;
    hipStream_t stream = nullptr;

    void* frame_dev = nullptr;  // staging for host-pushed frames (in_dtype)
    std::vector<float*> G;      // G[l], l = 1..L, of the frame being processed
    float* lap_tmp = nullptr;   // simple impl scratch
    float* q_tmp = nullptr;
    std::vector<float*> bestE, bestLap;
    std::vector<int32_t*> bestIdx;
    // float-32 stacks: the selection state of all levels and of the two base features lives in three
    // contiguous slabs (segments padded to 64 pixels), so the cross-GPU combine sees one flat vector
    float *slabE = nullptr, *slabL = nullptr;
    int32_t* slabI = nullptr;
    size_t slab_px = 0;

    int32_t* lev = nullptr;
    uint32_t* cnt = nullptr;
    float* logp = nullptr;
    float *bEnt = nullptr, *bDev = nullptr, *baseE = nullptr, *baseD = nullptr;
    int32_t *idxE = nullptr, *idxD = nullptr;
    float* fusedBase = nullptr;

    float *colA = nullptr, *colB = nullptr, *clipped = nullptr;
    const float* collapse_src = nullptr;   // float-32 stacks: input of the finest collapse step (set by finish)
    bool have_clipped = true;              // `clipped` holds the collapsed image (else the tap rebuilds it)
    void* out_dev = nullptr;

    int n_pushed = 0;
    int first_index = 0;
    int index_stride = 1;          // global index of the k-th pushed frame = first_index + k * index_stride (interleaved shards)
    uint64_t idx_exported = 0;     // bit l: the indices of state level l (L, L + 1: the base twins) are in their global form
    hipStream_t aux = nullptr;     // stream of the index export (not ordered behind the side streams as s->stream is after a push)
    bool finished = false;

    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> ev_pool;
    double prof_ms[MI_PROF_KINDS] = {};
    int64_t prof_n[MI_PROF_KINDS] = {};
    double prof_bytes[MI_PROF_KINDS] = {};

    std::vector<void*> allocs;
    void* tiled = nullptr;  // TiledState (tiled_host.hpp)
    void* mosaic = nullptr; // MosaicStage (mosaic_host.hpp): created by the first mi_stack_push_mosaic
};

namespace {

int dev_alloc(mi_stack* s, void** p, size_t bytes) {
    MI_HIP(hipMalloc(p, bytes ? bytes : 1));
    s->allocs.push_back(*p);
    return MI_OK;
}
template <typename T>
int dev_alloc_t(mi_stack* s, T** p, size_t count) {
    return dev_alloc(s, (void**)p, count * sizeof(T));
}

hipEvent_t get_event(mi_stack* s) {
    if (!s->ev_pool.empty()) {
        hipEvent_t e = s->ev_pool.back();
        s->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

struct ProfScope {
    mi_stack* s;
    ProfRec r{};
    bool on;
    hipStream_t st;
    ProfScope(mi_stack* s_, int kind, double bytes, hipStream_t stream = nullptr)
        : s(s_), on(s_->prof), st(stream ? stream : s_->stream) {
        if (!on) return;
        r.kind = kind;
        r.bytes = bytes;
        r.a = get_event(s);
        r.b = get_event(s);
        if (!r.a || !r.b) { on = false; return; }
        (void)hipEventRecord(r.a, st);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(r.b, st);
        s->recs.push_back(r);
    }
};

// fn(TIn{}, std::integral_constant<bool, FMA>{}) for the handle's input type and FMA switch: the one place that turns
// them into template arguments
template <typename Fn>
int dispatch_input(const mi_stack* s, Fn&& fn) {
    const bool fma = s->p.use_fma != 0;
    switch (s->p.in_dtype) {
        case MI_U8: return fma ? fn(uint8_t{}, std::true_type{}) : fn(uint8_t{}, std::false_type{});
        case MI_U16: return fma ? fn(uint16_t{}, std::true_type{}) : fn(uint16_t{}, std::false_type{});
        case MI_F32: return fma ? fn(float{}, std::true_type{}) : fn(float{}, std::false_type{});
    }
    return fail(MI_ERR_INVALID, "bad in_dtype %d", s->p.in_dtype);
}

int prof_drain(mi_stack* s) {
    if (s->recs.empty()) return MI_OK;
    int rc0 = tiled_sync_all(s);
    if (rc0) return rc0;
    MI_HIP(hipStreamSynchronize(s->stream));
    for (auto& r : s->recs) {
        float ms = 0.f;
        MI_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        s->prof_ms[r.kind] += ms;
        s->prof_n[r.kind] += r.launches;
        s->prof_bytes[r.kind] += r.bytes;
        s->ev_pool.push_back(r.a);
        s->ev_pool.push_back(r.b);
    }
    s->recs.clear();
    return MI_OK;
}

// algorithmic bytes of one frame's pyramid build + select:
// read level 0 once, write each G_l (l>=1) once and read it twice.
double algorithmic_bytes_per_frame(const mi_stack* s) {
    double b = (double)dtype_size(s->p.in_dtype) * 3.0 * s->lh[0] * s->lw[0];
    for (int l = 1; l <= s->L; ++l) b += 36.0 * s->lh[l] * s->lw[l];
    return b;
}

inline dim3 grid2d(int w, int h, dim3 blk) { return dim3(cdiv(w, blk.x), cdiv(h, blk.y)); }

// ------------------------------------------------------------------ simple implementation
template <typename TIn, bool FMA>
int process_frame_simple(mi_stack* s, const TIn* frame) {
    const dim3 blk(64, 4);
    const int idx = s->first_index + s->n_pushed;
    const int first = s->n_pushed == 0;
    if (s->sep) {   // MI_ARITH_SEPARABLE: the same sequence with the two-pass kernels (kernels_sep.hpp)
        ProfScope ps(s, MI_PROF_LEVEL, algorithmic_bytes_per_frame(s));
        const float k0 = s->k1d[0], k1 = s->k1d[1], k2 = s->k1d[2];
        hipLaunchKernelGGL((reduce_sep_simple<TIn>), grid2d(s->lw[1], s->lh[1], blk), blk, 0, s->stream, frame, s->lh[0],
                           s->lw[0], s->G[1], s->lh[1], s->lw[1], s->rk[0], s->rk[1], s->rk[2], s->rk[3]);
        for (int l = 1; l < s->L; ++l)
            hipLaunchKernelGGL((reduce_sep_simple<float>), grid2d(s->lw[l + 1], s->lh[l + 1], blk), blk, 0, s->stream,
                               (const float*)s->G[l], s->lh[l], s->lw[l], s->G[l + 1], s->lh[l + 1], s->lw[l + 1], s->rk[0],
                               s->rk[1], s->rk[2], s->rk[3]);
        for (int l = 0; l < s->L; ++l) {
            dim3 g = grid2d(s->lw[l], s->lh[l], blk);
            if (l == 0)
                hipLaunchKernelGGL((lapq_sep_simple<TIn>), g, blk, 0, s->stream, frame, s->lh[0], s->lw[0], (const float*)s->G[1],
                                   s->lh[1], s->lw[1], s->lap_tmp, s->q_tmp, k0, k1, k2);
            else
                hipLaunchKernelGGL((lapq_sep_simple<float>), g, blk, 0, s->stream, (const float*)s->G[l], s->lh[l], s->lw[l],
                                   (const float*)s->G[l + 1], s->lh[l + 1], s->lw[l + 1], s->lap_tmp, s->q_tmp, k0, k1, k2);
            hipLaunchKernelGGL(select_sep_simple, g, blk, 0, s->stream, (const float*)s->q_tmp, (const float*)s->lap_tmp,
                               s->lh[l], s->lw[l], idx, first, s->bestE[l], s->bestLap[l], s->bestIdx[l], k0, k1, k2);
        }
        MI_HIP(hipGetLastError());
        return MI_OK;
    }
    {
        ProfScope ps(s, MI_PROF_LEVEL, algorithmic_bytes_per_frame(s));
        // Gaussian pyramid
        hipLaunchKernelGGL((reduce_simple<TIn, FMA>), grid2d(s->lw[1], s->lh[1], blk), blk, 0,
                           s->stream, frame, s->lh[0], s->lw[0], s->G[1], s->lh[1], s->lw[1],
                           s->K);
        for (int l = 1; l < s->L; ++l)
            hipLaunchKernelGGL((reduce_simple<float, FMA>),
                               grid2d(s->lw[l + 1], s->lh[l + 1], blk), blk, 0, s->stream,
                               s->G[l], s->lh[l], s->lw[l], s->G[l + 1], s->lh[l + 1],
                               s->lw[l + 1], s->K);
        // Laplacian levels + selection
        for (int l = 0; l < s->L; ++l) {
            dim3 g = grid2d(s->lw[l], s->lh[l], blk);
            if (l == 0)
                hipLaunchKernelGGL((lapq_simple<TIn, FMA>), g, blk, 0, s->stream, frame,
                                   s->lh[0], s->lw[0], s->G[1], s->lh[1], s->lw[1], s->lap_tmp,
                                   s->q_tmp, s->K);
            else
                hipLaunchKernelGGL((lapq_simple<float, FMA>), g, blk, 0, s->stream, s->G[l],
                                   s->lh[l], s->lw[l], s->G[l + 1], s->lh[l + 1], s->lw[l + 1],
                                   s->lap_tmp, s->q_tmp, s->K);
            hipLaunchKernelGGL((select_simple<FMA>), g, blk, 0, s->stream, s->q_tmp, s->lap_tmp,
                               s->lh[l], s->lw[l], idx, first, s->bestE[l], s->bestLap[l],
                               s->bestIdx[l], s->K);
        }
    }
    MI_HIP(hipGetLastError());
    return MI_OK;
}

// base-level features of the frame whose G_L sits in s->G[L] (or `base` for L == 0)
template <bool FMA>
int process_base(mi_stack* s, const float* base) {
    ProfScope ps(s, MI_PROF_BASE, 0.0);
    const int hb = s->lh[s->L], wb = s->lw[s->L], npix = hb * wb;
    const int idx = s->first_index + s->n_pushed;
    const int first = s->n_pushed == 0;
    MI_HIP(hipMemsetAsync(s->cnt, 0, sizeof(uint32_t) * s->nlevels_hist, s->stream));
    hipLaunchKernelGGL((base_gray_hist<FMA>), dim3(cdiv(npix, 256)), dim3(256), 0, s->stream, base,
                       npix, s->nlevels_hist, s->lev, s->cnt);
    hipLaunchKernelGGL(base_logp, dim3(cdiv(s->nlevels_hist, 256)), dim3(256), 0, s->stream,
                       s->cnt, s->nlevels_hist, npix, s->logp);
    const dim3 blk(32, 8);
    hipLaunchKernelGGL(base_feat_select, grid2d(wb, hb, blk), blk, 0, s->stream, s->lev, s->logp,
                       base, hb, wb, s->pad, idx, first, s->bEnt, s->bDev, s->idxE, s->idxD,
                       s->baseE, s->baseD);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

// ------------------------------------------------------------------ float_type = float-64
template <typename TIn, bool FMA>
int process_frame_f64(mi_stack* s, const TIn* frame) {
    const dim3 blk(64, 4);
    const int idx = s->first_index + s->n_pushed;
    const int first = s->n_pushed == 0;
    auto G = [&](int l) { return reinterpret_cast<double*>(s->G[l]); };
    double* lap = reinterpret_cast<double*>(s->lap_tmp);
    {
        ProfScope ps(s, MI_PROF_LEVEL, algorithmic_bytes_per_frame(s));
        hipLaunchKernelGGL((reduce_f64<TIn, FMA>), grid2d(s->lw[1], s->lh[1], blk), blk, 0, s->stream, frame,
                           s->lh[0], s->lw[0], G(1), s->lh[1], s->lw[1], s->Kd);
        for (int l = 1; l < s->L; ++l)
            hipLaunchKernelGGL((reduce_f64<double, FMA>), grid2d(s->lw[l + 1], s->lh[l + 1], blk), blk, 0, s->stream,
                               (const double*)G(l), s->lh[l], s->lw[l], G(l + 1), s->lh[l + 1], s->lw[l + 1], s->Kd);
        for (int l = 0; l < s->L; ++l) {
            dim3 g = grid2d(s->lw[l], s->lh[l], blk);
            if (l == 0)
                hipLaunchKernelGGL((lapq_f64<TIn, FMA>), g, blk, 0, s->stream, frame, s->lh[0], s->lw[0],
                                   (const double*)G(1), s->lh[1], s->lw[1], lap, s->q_tmp, s->Kd);
            else
                hipLaunchKernelGGL((lapq_f64<double, FMA>), g, blk, 0, s->stream, (const double*)G(l), s->lh[l],
                                   s->lw[l], (const double*)G(l + 1), s->lh[l + 1], s->lw[l + 1], lap, s->q_tmp, s->Kd);
            hipLaunchKernelGGL((select_f64<FMA>), g, blk, 0, s->stream, s->q_tmp, (const double*)lap, s->lh[l],
                               s->lw[l], idx, first, s->bestE[l], reinterpret_cast<double*>(s->bestLap[l]),
                               s->bestIdx[l], s->K);
        }
    }
    MI_HIP(hipGetLastError());
    return MI_OK;
}

// base features in float64; the 256 / 65536-entry table log(count / npix) is filled on the host
// (logl rounded to double, see kernels_f64.hpp)
template <bool FMA>
int process_base_f64(mi_stack* s, const double* base) {
    ProfScope ps(s, MI_PROF_BASE, 0.0);
    const int hb = s->lh[s->L], wb = s->lw[s->L], npix = hb * wb;
    const int idx = s->first_index + s->n_pushed;
    const int first = s->n_pushed == 0;
    MI_HIP(hipMemsetAsync(s->cnt, 0, sizeof(uint32_t) * s->nlevels_hist, s->stream));
    hipLaunchKernelGGL((base_gray_hist_f64<FMA>), dim3(cdiv(npix, 256)), dim3(256), 0, s->stream, base, npix,
                       s->nlevels_hist, s->lev, s->cnt);
    std::vector<uint32_t> cnt(s->nlevels_hist);
    std::vector<double> lp(s->nlevels_hist, 0.0);
    MI_HIP(hipMemcpyAsync(cnt.data(), s->cnt, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    MI_HIP(hipStreamSynchronize(s->stream));
    for (int l = 0; l < s->nlevels_hist; ++l)
        if (cnt[l]) {
            const double pr = (double)cnt[l] / (double)npix;   // counts.astype(float64) / counts.sum()
            lp[l] = (double)logl((long double)pr);
        }
    MI_HIP(hipMemcpyAsync(s->logp, lp.data(), lp.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
    MI_HIP(hipStreamSynchronize(s->stream));   // lp goes out of scope
    const dim3 blk(32, 8);
    hipLaunchKernelGGL(base_feat_select_f64, grid2d(wb, hb, blk), blk, 0, s->stream, s->lev,
                       (const double*)s->logp, base, hb, wb, s->pad, idx, first, reinterpret_cast<double*>(s->bEnt),
                       reinterpret_cast<double*>(s->bDev), s->idxE, s->idxD, reinterpret_cast<double*>(s->baseE),
                       reinterpret_cast<double*>(s->baseD));
    MI_HIP(hipGetLastError());
    return MI_OK;
}

template <typename TIn, bool FMA>
int push_device_frames_f64(mi_stack* s, const void* dev_frames, int n, size_t stride) {
    for (int f = 0; f < n; ++f) {
        const TIn* fr = (const TIn*)((const char*)dev_frames + (size_t)f * stride);
        int rc;
        if (s->L == 0) {
            const size_t cnt = (size_t)s->lh[0] * s->lw[0] * 3;
            hipLaunchKernelGGL((frame_to_f64<TIn>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s->stream, fr,
                               cnt, reinterpret_cast<double*>(s->colA));
            rc = process_base_f64<FMA>(s, reinterpret_cast<const double*>(s->colA));
        } else {
            rc = process_frame_f64<TIn, FMA>(s, fr);
            if (rc) return rc;
            rc = process_base_f64<FMA>(s, reinterpret_cast<const double*>(s->G[s->L]));
        }
        if (rc) return rc;
        s->n_pushed++;
    }
    return MI_OK;
}

template <bool FMA>
int finish_f64(mi_stack* s) {
    ProfScope ps(s, MI_PROF_COLLAPSE, 0.0);
    const int L = s->L;
    const size_t nb = (size_t)s->lh[L] * s->lw[L] * 3;
    double* fused = reinterpret_cast<double*>(s->fusedBase);
    hipLaunchKernelGGL(base_fuse_f64, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s->stream,
                       (const double*)s->baseE, (const double*)s->baseD, nb, fused);
    const double* up = fused;
    double* bufs[2] = {reinterpret_cast<double*>(s->colA), reinterpret_cast<double*>(s->colB)};
    const dim3 blk(64, 4);
    for (int l = L - 1; l >= 0; --l) {
        double* out = bufs[l & 1];
        hipLaunchKernelGGL((collapse_f64<FMA>), grid2d(s->lw[l], s->lh[l], blk), blk, 0, s->stream, up, s->lh[l + 1],
                           s->lw[l + 1], (const double*)s->bestLap[l], s->lh[l], s->lw[l], out, s->Kd);
        up = out;
    }
    const size_t n = (size_t)s->lh[0] * s->lw[0] * 3;
    const dim3 g((unsigned)((n + 255) / 256));
    double* clipped = reinterpret_cast<double*>(s->clipped);
    if (s->p.out_dtype == MI_U8)
        hipLaunchKernelGGL((finalize_cast_f64<uint8_t>), g, dim3(256), 0, s->stream, up, n, (double)s->maxv, clipped,
                           (uint8_t*)s->out_dev);
    else
        hipLaunchKernelGGL((finalize_cast_f64<uint16_t>), g, dim3(256), 0, s->stream, up, n, (double)s->maxv, clipped,
                           (uint16_t*)s->out_dev);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

template <typename TIn, bool FMA>
int push_device_frames(mi_stack* s, const void* dev_frames, int n, size_t stride) {
    for (int f = 0; f < n; ++f) {
        const TIn* fr = (const TIn*)((const char*)dev_frames + (size_t)f * stride);
        int rc;
        if (s->L == 0) {
            // frames smaller than 2*min_size: no Laplacian levels, the frame itself is the base
            // (colA is free until the collapse)
            const size_t n = (size_t)s->lh[0] * s->lw[0] * 3;
            hipLaunchKernelGGL((frame_to_f32<TIn>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream,
                               fr, n, s->colA);
            rc = process_base<FMA>(s, s->colA);
            if (rc) return rc;
            s->n_pushed++;
            continue;
        }
        rc = process_frame_simple<TIn, FMA>(s, fr);
        if (rc) return rc;
        rc = process_base<FMA>(s, s->G[s->L]);
        if (rc) return rc;
        s->n_pushed++;
    }
    return MI_OK;
}

}  // namespace
int mi::dispatch_push(mi_stack* s, const void* dev_frames, int n, size_t stride) {
    if (s->p.impl == MI_IMPL_TILED) return tiled_push(s, dev_frames, n, stride);
    if (s->f64)
        return dispatch_input(s, [&](auto tin, auto fma) {
            return push_device_frames_f64<decltype(tin), decltype(fma)::value>(s, dev_frames, n, stride);
        });
    return dispatch_input(s, [&](auto tin, auto fma) {
        return push_device_frames<decltype(tin), decltype(fma)::value>(s, dev_frames, n, stride);
    });
}
namespace {

template <bool FMA>
int finish_impl(mi_stack* s) {
    ProfScope ps(s, MI_PROF_COLLAPSE, 0.0);
    const int L = s->L;
    size_t nb = (size_t)s->lh[L] * s->lw[L] * 3;
    hipLaunchKernelGGL(base_fuse, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s->stream,
                       s->baseE, s->baseD, nb, s->fusedBase);
    const float* up = s->fusedBase;
    float* bufs[2] = {s->colA, s->colB};
    const dim3 blk(64, 4);
    if (s->sep && L >= 1) {   // MI_ARITH_SEPARABLE: two-pass expand (kernels_sep.hpp), same structure
        const float k0 = s->k1d[0], k1 = s->k1d[1], k2 = s->k1d[2];
        for (int l = L - 1; l >= 1; --l) {
            float* out = bufs[l & 1];
            hipLaunchKernelGGL((collapse_sep<float>), grid2d(cdiv(s->lw[l], 2), cdiv(s->lh[l], 2), blk), blk, 0, s->stream, up, s->lh[l + 1],
                               s->lw[l + 1], (const float*)s->bestLap[l], s->lh[l], s->lw[l], s->maxv, out, k0, k1, k2);
            up = out;
        }
        s->collapse_src = up;
        s->have_clipped = false;
        const dim3 g0 = grid2d(cdiv(s->lw[0], 2), cdiv(s->lh[0], 2), blk);
        if (s->p.out_dtype == MI_U8)
            hipLaunchKernelGGL((collapse_sep<uint8_t>), g0, blk, 0, s->stream, up, s->lh[1], s->lw[1],
                               (const float*)s->bestLap[0], s->lh[0], s->lw[0], s->maxv, (uint8_t*)s->out_dev, k0, k1, k2);
        else
            hipLaunchKernelGGL((collapse_sep<uint16_t>), g0, blk, 0, s->stream, up, s->lh[1], s->lw[1],
                               (const float*)s->bestLap[0], s->lh[0], s->lw[0], s->maxv, (uint16_t*)s->out_dev, k0, k1, k2);
        MI_HIP(hipGetLastError());
        return MI_OK;
    }
    for (int l = L - 1; l >= 1; --l) {
        float* out = bufs[l & 1];
        hipLaunchKernelGGL((collapse_exact_quad<FMA, float>), grid2d(cdiv(s->lw[l], 2), cdiv(s->lh[l], 2), blk), blk, 0,
                           s->stream, up, s->lh[l + 1], s->lw[l + 1], (const float*)s->bestLap[l], s->lh[l],
                           s->lw[l], s->maxv, out, s->K);
        up = out;
    }
    s->collapse_src = up;     // level-1 image (or the fused base): what the collapsed-image tap restarts from
    s->have_clipped = false;
    if (L >= 1) {             // finest step fused with clip(abs) and the cast
        const dim3 g0 = grid2d(cdiv(s->lw[0], 2), cdiv(s->lh[0], 2), blk);
        if (s->p.out_dtype == MI_U8)
            hipLaunchKernelGGL((collapse_exact_quad<FMA, uint8_t>), g0, blk, 0, s->stream, up, s->lh[1], s->lw[1],
                               (const float*)s->bestLap[0], s->lh[0], s->lw[0], s->maxv, (uint8_t*)s->out_dev, s->K);
        else
            hipLaunchKernelGGL((collapse_exact_quad<FMA, uint16_t>), g0, blk, 0, s->stream, up, s->lh[1], s->lw[1],
                               (const float*)s->bestLap[0], s->lh[0], s->lw[0], s->maxv, (uint16_t*)s->out_dev, s->K);
        MI_HIP(hipGetLastError());
        return MI_OK;
    }
    s->have_clipped = true;
    size_t n = (size_t)s->lh[0] * s->lw[0] * 3;
    dim3 g((unsigned)((n + 255) / 256));
    if (s->p.out_dtype == MI_U8)
        hipLaunchKernelGGL((finalize_cast<uint8_t>), g, dim3(256), 0, s->stream, up, n, s->maxv,
                           s->clipped, (uint8_t*)s->out_dev);
    else
        hipLaunchKernelGGL((finalize_cast<uint16_t>), g, dim3(256), 0, s->stream, up, n, s->maxv,
                           s->clipped, (uint16_t*)s->out_dev);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int check_handle(const mi_stack* s) {
    if (!s) return fail(MI_ERR_INVALID, "null handle");
    return MI_OK;
}

}  // namespace

// tiled implementation hooks (kernels_tiled.hpp) need the handle layout
#include "tiled_host.hpp"
// raw-mosaic staging in front of it (kernels_demosaic.hpp)
#include "mosaic_host.hpp"

namespace {
// every frame staged from host memory, of either kind, is handed to the kernels (at most one kind is pending at a time)
int stack_flush(mi_stack* s) {
    int rc = mosaic_flush(s);
    return rc ? rc : tiled_flush(s);
}
int stack_pending(const mi_stack* s) { return tiled_pending(s) + mosaic_pending(s); }
}  // namespace

namespace {

void invert_affine_host(const double* M, double* iM) {
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0.0 ? 1.0 / D : 0.0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    iM[0] = A11;
    iM[1] = M[1] * (-D);
    iM[3] = M[3] * (-D);
    iM[4] = A22;
    iM[2] = -iM[0] * M[2] - iM[1] * M[5];
    iM[5] = -iM[3] * M[2] - iM[4] * M[5];
}

int round_sat(double v, int hi) {
    double r = std::nearbyint(v);
    return r < 0 ? 0 : (r > hi ? hi : (int)r);
}

// Scratch of the border blur's tile list (kernels_align.hpp): [count, pad to 64 B][bitmap: one bit per 32 x 64 tile]
// [list: one entry per tile].  One buffer per (device, stream) -- calls on one stream are ordered by the stream, calls on
// different streams must not share it -- grown on demand, kept for the life of the process.
struct WarpScratch {
    void* ptr = nullptr;
    size_t bytes = 0;
};
int warp_scratch(int device, hipStream_t st, size_t ntiles, uint32_t** cnt, uint32_t** bitmap, uint32_t** list, size_t* clear_bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, WarpScratch> cache;
    const size_t bm_bytes = (((ntiles + 31) / 32) * 4 + 63) & ~(size_t)63;
    const size_t need = 64 + bm_bytes + ntiles * 4;
    std::lock_guard<std::mutex> lk(mu);
    WarpScratch& w = cache[{device, st}];
    if (w.bytes < need) {
        if (w.ptr) {
            MI_HIP(hipStreamSynchronize(st));
            (void)hipFree(w.ptr);
            w.ptr = nullptr;
            w.bytes = 0;
        }
        MI_HIP(hipMalloc(&w.ptr, need));
        w.bytes = need;
    }
    *cnt = (uint32_t*)w.ptr;
    *bitmap = (uint32_t*)((char*)w.ptr + 64);
    *list = (uint32_t*)((char*)w.ptr + 64 + bm_bytes);
    *clear_bytes = 64 + bm_bytes;
    return MI_OK;
}

// the coordinate tables of one warp (warp_coord_tables): one buffer per (device, stream), as above
int warp_coord_scratch(int device, hipStream_t st, size_t n_ints, int** tab) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, WarpScratch> cache;
    const size_t need = n_ints * sizeof(int);
    std::lock_guard<std::mutex> lk(mu);
    WarpScratch& w = cache[{device, st}];
    if (w.bytes < need) {
        if (w.ptr) {
            MI_HIP(hipStreamSynchronize(st));
            (void)hipFree(w.ptr);
            w.ptr = nullptr;
            w.bytes = 0;
        }
        MI_HIP(hipMalloc(&w.ptr, need));
        w.bytes = need;
    }
    *tab = (int*)w.ptr;
    return MI_OK;
}

// the blurred-border composite behind a warp (align.py:245-251): passes over the tiles that hold a masked pixel
template <typename T>
int blur_launch(int device, hipStream_t st, void* side, void* out, uint8_t* valid, int h, int w, const GaussArgs& g,
                bool tiles_marked) {
    auto kb = border_blur_tiles<T>;
    const int r = g.ksize / 2;
    const size_t lds_blur = ((size_t)(BT_H + 2 * r) * (BT_W + 2 * r) * (sizeof(T) == 1 ? 1 : 2) + 3 * (size_t)(BT_H + 2 * r) * BT_W) * 4;
    static thread_local bool attr_set = false;
    if (!attr_set) {
        // largest blur kernel (31 taps): 62 x 94 raw pixels + 3 x 62 x 64 floats
        MI_HIP(hipFuncSetAttribute((const void*)kb, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(((size_t)62 * 94 * 2 + 3 * 62 * 64) * 4)));
        attr_set = true;
    }
    const int tiles_x = cdiv(w, BT_W), tiles_y = cdiv(h, BT_H);
    uint32_t *cnt = nullptr, *bitmap = nullptr, *list = nullptr;
    size_t clear = 0;
    int rc = warp_scratch(device, st, (size_t)tiles_x * tiles_y, &cnt, &bitmap, &list, &clear);
    if (rc) return rc;
    const size_t npx = (size_t)h * w;
    if (!tiles_marked) {   // the warp kernel did not mark the tiles with masked pixels itself: scan the mask
        MI_HIP(hipMemsetAsync(cnt, 0, clear, st));
        hipLaunchKernelGGL(mask_scan_tiles, dim3((unsigned)std::min<size_t>(2048, (npx / 16 + 256) / 256)), dim3(256), 0, st,
                           (const uint8_t*)valid, h, w, tiles_x, bitmap);
    }
    if (!tiles_marked)   // (the affine warp kernel lists the tiles it marks)
        hipLaunchKernelGGL(tile_bitmap_to_list, dim3(1), dim3(1024), 0, st, (const uint32_t*)bitmap, (tiles_x * tiles_y + 31) / 32, cnt, list);
    hipLaunchKernelGGL(kb, dim3(1024), dim3(256), lds_blur, st, (const T*)out, (const uint8_t*)valid, (T*)side, h, w, tiles_x, g,
                       (const uint32_t*)cnt, (const uint32_t*)list);
    hipLaunchKernelGGL((border_blur_scatter<T>), dim3(1024), dim3(256), 0, st, (T*)out, (const uint8_t*)valid, (const T*)side,
                       h, w, tiles_x, (const uint32_t*)cnt, (const uint32_t*)list);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

template <typename T>
int warp_launch(int device, hipStream_t st, const void* src, void* side, void* out, uint8_t* valid, int h, int w,
                const AffineArgs& a, bool blur, const GaussArgs& g, const PerspArgs* persp) {
    bool tiles_marked = false;
    if (sizeof(T) == 1 && (size_t)h * w == 1) {   // three bytes: no 4-byte tap load fits (warp_one_pixel_u8); its blur is itself
        hipLaunchKernelGGL(warp_one_pixel_u8, dim3(1), dim3(1), 0, st, (const uint8_t*)src, (uint8_t*)out, valid, a,
                           persp ? *persp : PerspArgs{}, persp != nullptr);
        MI_HIP(hipGetLastError());
        return MI_OK;
    }
    if (persp) {
        const dim3 blk(64, 4), grid(cdiv(w, 64), cdiv(h, 4));
        hipLaunchKernelGGL((warp_perspective_kernel<T>), grid, blk, 0, st, (const T*)src, (T*)out, valid, a, *persp);
    } else {
        uint32_t *bitmap = nullptr, *cnt = nullptr, *list = nullptr;
        size_t clear = 0;
        const int blur_tiles_x = cdiv(w, BT_W);
        if (blur) {   // the kernel marks and lists the blur tiles that hold masked pixels (the scratch is zeroed by warp_coord_tables)
            int rc = warp_scratch(device, st, (size_t)blur_tiles_x * cdiv(h, BT_H), &cnt, &bitmap, &list, &clear);
            if (rc) return rc;
            tiles_marked = true;
        }
        // LDS-staged tiles of 256 x 32 (16) destination pixels, four pixels x 8 (4) rows per thread; whole-dword stores
        // when every row starts 4-byte aligned
        int* tab = nullptr;
        {
            int rc = warp_coord_scratch(device, st, 2 * ((size_t)w + h), &tab);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(warp_coord_tables, dim3(cdiv(std::max(w, h), 256)), dim3(256), 0, st, a, tab, cnt, (int)(clear / 4));
        const bool vec = (w % 4) == 0 && ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(valid)) & 3) == 0;
        const int gx = cdiv(w, WT_W), gy = cdiv(h, WarpTile<T>::TH);   // tiles; the kernel's header has the block order
        const dim3 grid(gx >= 3 && gy >= 3 ? (2 * gx + 2 * (gy - 2)) * WT_SPLIT + gx * (gy - 2) : gx * gy);
        const size_t lds = (size_t)WT_LDS_DWORDS * 4;
        auto kv = warp_affine_tiled<T, true>;
        auto ks = warp_affine_tiled<T, false>;
        static thread_local bool attr_set = false;
        if (!attr_set) {
            MI_HIP(hipFuncSetAttribute((const void*)kv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            MI_HIP(hipFuncSetAttribute((const void*)ks, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr_set = true;
        }
        if (vec) hipLaunchKernelGGL(kv, grid, dim3(256), lds, st, (const T*)src, (T*)out, valid, a, bitmap, list, blur_tiles_x, (const int*)tab, gx, gy);
        else hipLaunchKernelGGL(ks, grid, dim3(256), lds, st, (const T*)src, (T*)out, valid, a, bitmap, list, blur_tiles_x, (const int*)tab, gx, gy);
    }
    MI_HIP(hipGetLastError());
    // the warped image went straight to `out`; the few pixels outside the source frame are blurred from it into `side`
    // and copied back
    return blur ? blur_launch<T>(device, st, side, out, valid, h, w, g, tiles_marked) : MI_OK;
}

}  // namespace

namespace {

// solve the symmetric 4x4 system H d = r (column-scaled Gaussian elimination, partial pivoting)
bool solve4(const double Hs[10], const double r[4], double d[4]) {
    double A[4][5];
    int k = 0;
    double Hm[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j) Hm[i][j] = Hm[j][i] = Hs[k++];
    double sc[4];
    for (int i = 0; i < 4; ++i) {
        if (!(Hm[i][i] > 0)) return false;
        sc[i] = 1.0 / std::sqrt(Hm[i][i]);
    }
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 4; ++j) A[i][j] = Hm[i][j] * sc[i] * sc[j];
        A[i][4] = r[i] * sc[i];
    }
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        for (int i = c + 1; i < 4; ++i)
            if (std::fabs(A[i][c]) > std::fabs(A[piv][c])) piv = i;
        if (std::fabs(A[piv][c]) < 1e-12) return false;
        if (piv != c)
            for (int j = 0; j < 5; ++j) std::swap(A[c][j], A[piv][j]);
        for (int i = c + 1; i < 4; ++i) {
            const double f = A[i][c] / A[c][c];
            for (int j = c; j < 5; ++j) A[i][j] -= f * A[c][j];
        }
    }
    for (int i = 3; i >= 0; --i) {
        double v = A[i][4];
        for (int j = i + 1; j < 4; ++j) v -= A[i][j] * d[j];
        d[i] = v / A[i][i];
    }
    for (int i = 0; i < 4; ++i) d[i] *= sc[i];
    return true;
}

struct EccLevel {
    int h, w;
    float *tmpl, *img;
};

}  // namespace

// Device-resident aligner: the pyramids of the reference (template) and of the moving frame, the
// scratch for the sums, all allocated once per (shape, dtype, subsample).
struct mi_aligner {
    int device = 0, height = 0, width = 0, dtype = 0, subsample = 1;
    int area = 0;      // sub-sample by area mean (cv2.resize INTER_AREA) instead of img[::s, ::s]
    int h = 0, w = 0;  // size of the sub-sampled images the estimate works on
    std::vector<EccLevel> lv;   // tmpl: one image; img: `cap` images (frame f at + f * h * w)
    float* gray = nullptr;
    int cap = 0;                     // moving frames the per-frame buffers hold
    double* partial = nullptr;       // [cap][ECC_MAX_BLOCKS][ECC_NSUM]
    unsigned int* ticket = nullptr;  // [cap]
    EccState* dstate = nullptr;      // [cap] the frames' Gauss-Newton state (device memory: the kernels iterate on it)
    EccState* hstate = nullptr;      // pinned host copy: initial values up, `active` flags and results down
    EccStateH* dstate_h = nullptr;   // [cap] state of the 8-DoF refinement (ALIGN_HOMOGRAPHY)
    EccStateH* hstate_h = nullptr;   // pinned host copy
    std::vector<void*> bufs;         // template pyramid + gray scratch
    std::vector<void*> fbufs;        // per-frame buffers (re-allocated when the capacity grows)
    hipStream_t own = nullptr;       // used when the caller passes no stream: handles on different host
                                     // threads then run side by side instead of serialising on stream 0
    bool have_ref = false;
    // mi_align_stack_device: side lanes of the warp stage.  The frames of a batch are warped round-robin on the stacker's
    // stream and on WARP_LANES - 1 streams of the handle, each with its own border-blur scratch, so that one frame's short,
    // latency-bound kernels (tables, tile list, border blur of a few hundred tiles, scatter) run beside the next frame's warp
    // instead of in front of it.
    hipStream_t wst[3] = {nullptr, nullptr, nullptr};   // (the stacker's side streams: borrowed per call, never destroyed here)
    hipEvent_t wev[3] = {nullptr, nullptr, nullptr}, wstart = nullptr;
    void *wtmp[3] = {nullptr, nullptr, nullptr}, *wmask[3] = {nullptr, nullptr, nullptr};
    // optional coarse initialiser (mi_aligner_set_phase_init): phase correlation on pyramid level `pc_level`
    bool phase_init = false;
    int pc_level = 0, pc_P = 0, pc_Q = 0;
    float2 *pc_ref = nullptr, *pc_mov = nullptr;   // P x Q spectra: the template's (kept per reference) and a frame's
    double* pc_out = nullptr;                      // [cap][3] (dx, dy, response) on the device
    bool pc_ref_valid = false;
};

namespace {

int pc_log2(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }

// 2-D DFT of a P x Q complex plane in place (rows, then columns)
template <bool INVERSE>
void pc_fft2(hipStream_t st, float2* d, int P, int Q) {
    hipLaunchKernelGGL((pc_fft_lines<INVERSE>), dim3(P), dim3(std::max(Q / 2, 1)), 0, st, d, Q, pc_log2(Q), (size_t)1, (size_t)Q);
    hipLaunchKernelGGL((pc_fft_lines<INVERSE>), dim3(Q), dim3(std::max(P / 2, 1)), 0, st, d, P, pc_log2(P), (size_t)Q, (size_t)1);
}

constexpr int PC_WHOLE = -1;   // `last` of the two functions below: no stage is the last one, run to the end

// spectrum of one windowed, padded plane.  `last` (mi_phase_correlate_tap_device): MI_PC_TAP_WINDOWED_MOV stops in front of
// the transform
void pc_spectrum(hipStream_t st, const float* plane, int h, int w, float2* out, int P, int Q, int last = PC_WHOLE) {
    hipLaunchKernelGGL(pc_prepare, dim3(cdiv(Q, 64), cdiv(P, 4)), dim3(64, 4), 0, st, plane, h, w, out, P, Q);
    if (last == MI_PC_TAP_WINDOWED_MOV) return;
    pc_fft2<false>(st, out, P, Q);
}

// mov's spectrum (in `fm`, destroyed) against the reference's `fr`: (dx, dy, response) -> dev_out3.  `last`: the tap's
// stage, left in `fm` (MI_PC_TAP_CROSS_POWER, MI_PC_TAP_SURFACE); dev_out3 is not written then
void pc_correlate(hipStream_t st, const float2* fr, float2* fm, int P, int Q, double* dev_out3, int last = PC_WHOLE) {
    const size_t n = (size_t)P * Q;
    hipLaunchKernelGGL(pc_cross_power, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, fm, fr, n);
    if (last == MI_PC_TAP_CROSS_POWER) return;
    pc_fft2<true>(st, fm, P, Q);
    if (last == MI_PC_TAP_SURFACE) return;
    hipLaunchKernelGGL(pc_peak, dim3(1), dim3(1024), 0, st, (const float2*)fm, P, Q, dev_out3);
}

void aligner_free_frames(mi_aligner* al) {
    for (void* b : al->fbufs) (void)hipFree(b);
    al->fbufs.clear();
    if (al->hstate) (void)hipHostFree(al->hstate);
    al->hstate = nullptr;
    if (al->hstate_h) (void)hipHostFree(al->hstate_h);
    al->hstate_h = nullptr;
    al->cap = 0;
}

void aligner_free(mi_aligner* al) {
    aligner_free_frames(al);
    for (void* b : al->bufs) (void)hipFree(b);
    al->bufs.clear();
    if (al->own) (void)hipStreamDestroy(al->own);
    al->own = nullptr;
    for (int j = 0; j < 3; ++j) {
        if (al->wev[j]) (void)hipEventDestroy(al->wev[j]);
        (void)hipFree(al->wtmp[j]);
        (void)hipFree(al->wmask[j]);
        al->wst[j] = nullptr; al->wev[j] = nullptr; al->wtmp[j] = al->wmask[j] = nullptr;
    }
    if (al->wstart) (void)hipEventDestroy(al->wstart);
    al->wstart = nullptr;
}

// The side lanes of mi_align_stack_device's warp stage (scratch created on first use; one frame + one mask each).
// Round 5 built them on streams of their own (1 against 4 lanes: 0.0371 vs 0.0369 s) -- with the stacker's three streams and
// the estimator's that made seven streams on the runtime's four hardware queues, so the lanes queued behind each
// other anyway.  Round 6: the lanes ARE the stacker's side streams (border tiles / levels >= 1), which carry nothing while a
// batch buffer fills: no stream is added.
#ifndef MI_WARP_LANES
#define MI_WARP_LANES 2
#endif
constexpr int WARP_LANES = MI_WARP_LANES;
int aligner_warp_lanes(mi_aligner* al, size_t frame_bytes, size_t mask_bytes) {
    if (al->wstart) return MI_OK;
    static_assert(WARP_LANES >= 1 && WARP_LANES <= 3, "lanes: the stacker's own stream and its two side streams");
    for (int j = 0; j < WARP_LANES - 1; ++j) {
        MI_HIP(hipEventCreateWithFlags(&al->wev[j], hipEventDisableTiming));
        if (hipMalloc(&al->wtmp[j], frame_bytes) != hipSuccess || hipMalloc(&al->wmask[j], mask_bytes) != hipSuccess)
            return fail(MI_ERR_NOMEM, "out of device memory");
    }
    MI_HIP(hipEventCreateWithFlags(&al->wstart, hipEventDisableTiming));
    return MI_OK;
}

// per-frame buffers for `n` moving frames
int aligner_reserve(mi_aligner* al, int n) {
    if (n <= al->cap) return MI_OK;
    MI_HIP(hipDeviceSynchronize());
    aligner_free_frames(al);
    auto dalloc = [&](size_t bytes) -> void* {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        al->fbufs.push_back(p);
        return p;
    };
    bool ok = true;
    for (auto& L : al->lv) {
        const size_t nb = (size_t)L.h * L.w * 4 * n;
        L.img = (float*)dalloc(nb);
        ok = ok && L.img;
    }
    al->partial = (double*)dalloc((size_t)n * ECC_MAX_BLOCKS * (ECC_NSUM_H > ECC_NSUM ? ECC_NSUM_H : ECC_NSUM) * sizeof(double));
    al->ticket = (unsigned int*)dalloc(sizeof(unsigned int) * n);
    ok = ok && al->partial && al->ticket;
    // (null stream: complete before any kernel on the aligner's non-blocking streams reads the tickets)
    if (ok) ok = hipMemset(al->ticket, 0, sizeof(unsigned int) * n) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
    al->dstate = (EccState*)dalloc(sizeof(EccState) * n);
    ok = ok && al->dstate;
    al->pc_out = (double*)dalloc(sizeof(double) * 3 * n);
    ok = ok && al->pc_out;
    if (ok) ok = hipHostMalloc((void**)&al->hstate, sizeof(EccState) * n, hipHostMallocDefault) == hipSuccess;
    al->dstate_h = (EccStateH*)dalloc(sizeof(EccStateH) * n);
    ok = ok && al->dstate_h;
    if (ok) ok = hipHostMalloc((void**)&al->hstate_h, sizeof(EccStateH) * n, hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        aligner_free_frames(al);
        return fail(MI_ERR_NOMEM, "out of device memory");
    }
    al->cap = n;
    return MI_OK;
}

// gray + pyramid (+ gradients) of one image: the template, or moving frame `slot`
// `upto`: build levels 0 .. upto-1 only (the batch builds the small levels of all its frames with one launch each)
int aligner_build(mi_aligner* al, hipStream_t st, const void* dev_img, bool is_tmpl, int slot, int upto = 1 << 30) {
    const dim3 blk(64, 4), g0(cdiv(al->w, 64), cdiv(al->h, 4));
    auto& lv = al->lv;
    auto at = [&](float* base, size_t l) { return base + (size_t)slot * lv[l].h * lv[l].w; };
    size_t first = 0;   // first level the loop below still has to build
    if (al->subsample == 2 && lv.size() >= 2 && upto >= 2) {
        // the common factor: gray, level 0 and level 1 in one pass over the frame (ecc_pyramid2)
        float* d0 = is_tmpl ? lv[0].tmpl : at(lv[0].img, 0);
        float* d1 = is_tmpl ? lv[1].tmpl : at(lv[1].img, 1);
        const dim3 gp(cdiv(al->w, 64), cdiv(al->h, 32));
        if (al->dtype == MI_U8) {
            if (al->area) hipLaunchKernelGGL((ecc_pyramid2<uint8_t, true>), gp, dim3(256), 0, st, (const uint8_t*)dev_img, al->height, al->width, al->h, al->w, d0, lv[1].h, lv[1].w, d1);
            else hipLaunchKernelGGL((ecc_pyramid2<uint8_t, false>), gp, dim3(256), 0, st, (const uint8_t*)dev_img, al->height, al->width, al->h, al->w, d0, lv[1].h, lv[1].w, d1);
        } else {
            if (al->area) hipLaunchKernelGGL((ecc_pyramid2<uint16_t, true>), gp, dim3(256), 0, st, (const uint16_t*)dev_img, al->height, al->width, al->h, al->w, d0, lv[1].h, lv[1].w, d1);
            else hipLaunchKernelGGL((ecc_pyramid2<uint16_t, false>), gp, dim3(256), 0, st, (const uint16_t*)dev_img, al->height, al->width, al->h, al->w, d0, lv[1].h, lv[1].w, d1);
        }
        first = 2;
    } else if (al->subsample == 2) {   // the common factor: four outputs per thread from 8-byte loads
        const dim3 g2(cdiv(cdiv(al->w, 4), 64), cdiv(al->h, 4));
        if (al->dtype == MI_U8) {
            if (al->area) hipLaunchKernelGGL((ecc_gray_s2<uint8_t, true>), g2, blk, 0, st, (const uint8_t*)dev_img, al->height, al->width, al->h, al->w, al->gray);
            else hipLaunchKernelGGL((ecc_gray_s2<uint8_t, false>), g2, blk, 0, st, (const uint8_t*)dev_img, al->height, al->width, al->h, al->w, al->gray);
        } else {
            if (al->area) hipLaunchKernelGGL((ecc_gray_s2<uint16_t, true>), g2, blk, 0, st, (const uint16_t*)dev_img, al->height, al->width, al->h, al->w, al->gray);
            else hipLaunchKernelGGL((ecc_gray_s2<uint16_t, false>), g2, blk, 0, st, (const uint16_t*)dev_img, al->height, al->width, al->h, al->w, al->gray);
        }
    } else if (al->dtype == MI_U8)
        hipLaunchKernelGGL((ecc_gray<uint8_t>), g0, blk, 0, st, (const uint8_t*)dev_img, al->height, al->width, al->h, al->w,
                           al->subsample, al->area, al->gray);
    else
        hipLaunchKernelGGL((ecc_gray<uint16_t>), g0, blk, 0, st, (const uint16_t*)dev_img, al->height, al->width, al->h, al->w,
                           al->subsample, al->area, al->gray);
    for (size_t l = first; l < lv.size() && (int)l < upto; ++l) {
        float* dst = is_tmpl ? lv[l].tmpl : at(lv[l].img, l);
        const float* src = l == 0 ? al->gray : (is_tmpl ? lv[l - 1].tmpl : at(lv[l - 1].img, l - 1));
        const int sh = l == 0 ? al->h : lv[l - 1].h, sw = l == 0 ? al->w : lv[l - 1].w;
        const dim3 gt(cdiv(lv[l].w, 64), cdiv(lv[l].h, 16));
        if (l == 0) hipLaunchKernelGGL((ecc_blur_tile<0>), gt, dim3(256), 0, st, src, sh, sw, dst, lv[l].h, lv[l].w);
        else hipLaunchKernelGGL((ecc_blur_tile<1>), gt, dim3(256), 0, st, src, sh, sw, dst, lv[l].h, lv[l].w);
    }
    MI_HIP(hipGetLastError());
    return MI_OK;
}

// gray + pyramid of the n moving frames of a batch (slots 0 .. n-1): levels 0 and 1 of all frames in one launch where
// ecc_pyramid2 applies (sub-sampling 2, n > 1), frame by frame otherwise; the levels from `split` on, one launch per level
int aligner_build_batch(mi_aligner* al, hipStream_t st, const void* const* dev_movs, int n) {
    static_assert(ECC_MAXF <= 128, "EccFramePtrs holds 128 frames");
    auto& lv = al->lv;
    const int split = n > 1 ? 2 : 1 << 30;
    int rc;
    if (n > 1 && al->subsample == 2 && lv.size() >= 2) {
        EccFramePtrs fr{};
        for (int k = 0; k < n; ++k) fr.p[k] = dev_movs[k];
        const dim3 gp(cdiv(al->w, 64), cdiv(al->h, 32), n);
        float *d0 = lv[0].img, *d1 = lv[1].img;
        if (al->dtype == MI_U8) {
            if (al->area) hipLaunchKernelGGL((ecc_pyramid2_batch<uint8_t, true>), gp, dim3(256), 0, st, fr, al->height, al->width, al->h, al->w, d0, lv[1].h, lv[1].w, d1);
            else hipLaunchKernelGGL((ecc_pyramid2_batch<uint8_t, false>), gp, dim3(256), 0, st, fr, al->height, al->width, al->h, al->w, d0, lv[1].h, lv[1].w, d1);
        } else {
            if (al->area) hipLaunchKernelGGL((ecc_pyramid2_batch<uint16_t, true>), gp, dim3(256), 0, st, fr, al->height, al->width, al->h, al->w, d0, lv[1].h, lv[1].w, d1);
            else hipLaunchKernelGGL((ecc_pyramid2_batch<uint16_t, false>), gp, dim3(256), 0, st, fr, al->height, al->width, al->h, al->w, d0, lv[1].h, lv[1].w, d1);
        }
    } else {
        for (int k = 0; k < n; ++k)
            if ((rc = aligner_build(al, st, dev_movs[k], false, k, split))) return rc;
    }
    for (size_t l = (size_t)split; l < lv.size(); ++l) {
        const auto& a = lv[l - 1];
        const auto& b = lv[l];
        hipLaunchKernelGGL((ecc_blur_tile<1>), dim3(cdiv(b.w, 64), cdiv(b.h, 16), n), dim3(256), 0, st, (const float*)a.img, a.h, a.w,
                           b.img, b.h, b.w);
    }
    MI_HIP(hipGetLastError());
    return MI_OK;
}

// Coarse-to-fine forward-additive ECC of `n` <= ECC_MAXF moving frames (pyramids in slots 0..n-1)
// against the template: one launch and one host round trip per Gauss-Newton iteration for the whole
// batch; frames that converged on a level sit out the rest of it.  M_out[f] in FULL-resolution pixel
// coordinates (translation scaled by the sub-sampling factor, as align.py:224-231 does).  A frame
// the method fails on (no overlap, constant image, degenerate transform) gets cc = -2.
// iterations enqueued between two looks at the frames' `active` flags: the first look of a level comes late (a level
// rarely converges in fewer), the following ones sooner
// (the two coarsest levels start far from their optimum; the finer ones inherit it and stop after one to three steps)
#ifndef MI_ECC_CHUNK_FINE
#define MI_ECC_CHUNK_FINE 4
#endif
constexpr int ECC_CHUNK_FIRST = 8, ECC_CHUNK_FIRST_FINE = MI_ECC_CHUNK_FINE, ECC_CHUNK_NEXT = 4;
// samples per Gauss-Newton sum at least: levels with more pixels are sampled on every `step`-th row and column
#ifndef MI_ECC_MIN_SAMPLES
#define MI_ECC_MIN_SAMPLES 300000
#endif
inline int ecc_sample_step(size_t np) {
    int step = 1;
    while ((size_t)(step + 1) * (step + 1) * (size_t)MI_ECC_MIN_SAMPLES <= np) ++step;
    return step;
}

// `M9_out` (optional): ALIGN_HOMOGRAPHY -- the similarity is refined to 8 degrees of freedom on the finest level
// (ecc_accumulate_h) and row f of M9_out receives the 3 x 3 matrix (moving -> reference, full-resolution pixels, M[8] = 1);
// a frame whose refinement fails or does not raise the correlation keeps its similarity, as a 3 x 3.
// `M_init` (n x 6, moving -> reference in full-resolution pixels, what a previous estimate returned) + `start_level`: the
// iteration starts from that transform on pyramid level `start_level` instead of from the identity on the coarsest level
// (mi_aligner_refine_batch).
// `tslots` (n, optional): frame k is registered against the pyramid of the batch's frame tslots[k] instead of the handle's
// reference (mi_aligner_estimate_pairs; no phase-correlation start there).
int aligner_solve(mi_aligner* al, hipStream_t st, int n, int max_iters, double eps, double* M_out, double* cc_out,
                  int* iters_out, double* M9_out = nullptr, const double* M_init = nullptr, int start_level = -1,
                  const int* tslots = nullptr) {
    if (max_iters < 1) max_iters = 50;
    if (!(eps > 0)) eps = 1e-8;
    auto& lv = al->lv;
    EccState* const hs = al->hstate;
    const int l_first = M_init ? std::min(std::max(start_level, 0), (int)lv.size() - 1) : (int)lv.size() - 1;
    for (int k = 0; k < n; ++k) {
        hs[k] = EccState{};
        hs[k].a = 1.0;
        hs[k].rho = -1.0;
        hs[k].last_rho = -2.0;
        hs[k].tslot = tslots ? tslots[k] : -1;
        if (M_init) {
            // W = M^-1 (reference -> moving, what the iteration works on): A = [a -b; b a], T in origin coordinates of level
            // l_first (sub-sampled pixels / 2^l_first) -- the inverse of the read-out at the end of this function
            const double* M = M_init + 6 * k;
            const double ia = M[0], ib = M[3], det = ia * ia + ib * ib;
            if (!(det > 1e-12)) return fail(MI_ERR_INVALID, "degenerate starting transform for frame %d", k);
            const double a = ia / det, b = -ib / det, sc = (double)al->subsample * std::ldexp(1.0, l_first);
            hs[k].a = a;
            hs[k].b = b;
            hs[k].T0 = -(a * M[2] - b * M[5]) / sc;
            hs[k].T1 = -(b * M[2] + a * M[5]) / sc;
        }
    }
    if (al->phase_init && !M_init && !tslots) {
        // coarse initialiser: the translation phase correlation finds on level pc_level (<= 512 pixels per side) becomes
        // the starting translation of the Gauss-Newton iteration at the coarsest level
        const EccLevel& PL = lv[al->pc_level];
        const int P = al->pc_P, Q = al->pc_Q;
        if (!al->pc_ref) {
            void *a = nullptr, *b = nullptr;
            if (hipMalloc(&a, sizeof(float2) * P * Q) != hipSuccess || hipMalloc(&b, sizeof(float2) * P * Q) != hipSuccess)
                return fail(MI_ERR_NOMEM, "out of device memory");
            al->bufs.push_back(a);
            al->bufs.push_back(b);
            al->pc_ref = (float2*)a;
            al->pc_mov = (float2*)b;
        }
        if (!al->pc_ref_valid) {
            pc_spectrum(st, PL.tmpl, PL.h, PL.w, al->pc_ref, P, Q);
            al->pc_ref_valid = true;
        }
        for (int k = 0; k < n; ++k) {
            pc_spectrum(st, PL.img + (size_t)k * PL.h * PL.w, PL.h, PL.w, al->pc_mov, P, Q);
            pc_correlate(st, al->pc_ref, al->pc_mov, P, Q, al->pc_out + 3 * k);
        }
        MI_HIP(hipGetLastError());
        std::vector<double> o3((size_t)3 * n);
        MI_HIP(hipMemcpyAsync(o3.data(), al->pc_out, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st));
        MI_HIP(hipStreamSynchronize(st));
        const double down = std::ldexp(1.0, al->pc_level - ((int)lv.size() - 1));   // level pc_level -> the coarsest level
        for (int k = 0; k < n; ++k) {
            // R = Mov conj(Ref): the peak sits at d with mov(x) = ref(x - d), i.e. ref(x) ~ mov(x + d) -- exactly the
            // translation of W (kernels_ecc.hpp); a weak peak (flat or unrelated content) is not used
            if (o3[3 * k + 2] > 0.02) {
                hs[k].T0 = o3[3 * k] * down;
                hs[k].T1 = o3[3 * k + 1] * down;
            }
        }
    }
    MI_HIP(hipMemcpyAsync(al->dstate, hs, sizeof(EccState) * n, hipMemcpyHostToDevice, st));
    for (int l = l_first; l >= 0; --l) {
        const EccLevel& L = lv[l];
        const double cx = 0.5 * (L.w - 1), cy = 0.5 * (L.h - 1);
        const size_t np = (size_t)L.h * L.w;
        // sample every `step`-th pixel in both directions: a third of a million samples and more are plenty for 4 parameters
        // (6 MP level: step 4 = 375 K samples, 1.5 MP level: step 2; rounds 3-4 kept half a million -- 667 K and all 1.5 M --:
        // the recovered transforms of config 4 stay ten times inside the tolerances either way, profiles/r05)
        const int step = ecc_sample_step(np);
        // ~48 samples per thread (the 28 double sums cost a thread ~500 instructions to reduce, as much as 5 samples),
        // at most ECC_MAX_BLOCKS blocks (4 per CU).  Measured (round 3, config 4 / the estimate of a 16-frame batch alone):
        // 3072 -> 0.054 s / 6.6 ms, 6144 -> 0.047 / 5.5, 12288 -> 0.042 / 5.5, 24576 -> 0.041 / 6.7: fewer, longer
        // workgroups leave more of the GPU to the warps and the fuse that run beside the estimate
        constexpr size_t per_blk = 12288;
        const size_t work = (np / ((size_t)step * step) + per_blk - 1) / per_blk;
        const unsigned nblk = (unsigned)(work < 1 ? 1 : (work > (size_t)ECC_MAX_BLOCKS ? ECC_MAX_BLOCKS : work));
        hipLaunchKernelGGL(ecc_level_begin, dim3(cdiv(n, 64)), dim3(64), 0, st, al->dstate, n, cx, cy);
        const double reach = std::hypot(cx, cy);
        for (int it = 0; it < max_iters;) {
            const int chunk = std::min(it == 0 ? (l + 2 >= (int)lv.size() ? ECC_CHUNK_FIRST : ECC_CHUNK_FIRST_FINE) : ECC_CHUNK_NEXT,
                                       max_iters - it);
            for (int j = 0; j < chunk; ++j)   // frames that have stopped leave at once
                hipLaunchKernelGGL(ecc_accumulate, dim3(nblk, n), dim3(256), 0, st, L.tmpl, L.img, np, L.h, L.w, al->dstate, step,
                                   al->partial, al->ticket, reach, eps);
            it += chunk;
            MI_HIP(hipMemcpyAsync(hs, al->dstate, sizeof(EccState) * n, hipMemcpyDeviceToHost, st));
            MI_HIP(hipStreamSynchronize(st));
            int nact = 0;
            for (int k = 0; k < n; ++k) nact += hs[k].active;
            if (!nact) break;
        }
        // back to origin coordinates, then up to the next finer level (u_f = 2 u_c, x_f = 2 x_c)
        hipLaunchKernelGGL(ecc_level_end, dim3(cdiv(n, 64)), dim3(64), 0, st, al->dstate, n, cx, cy, l > 0 ? 1 : 0);
    }
    EccStateH* const hh = al->hstate_h;
    double Rn = 1.0, cx0 = 0.0, cy0 = 0.0;
    if (M9_out) {
        // 8-DoF refinement on the finest level, from the converged similarity
        const EccLevel& L = lv[0];
        cx0 = 0.5 * (L.w - 1);
        cy0 = 0.5 * (L.h - 1);
        Rn = (double)hypotf((float)cx0, (float)cy0);   // the kernel's own (float) radius
        const size_t np = (size_t)L.h * L.w;
        const int step = ecc_sample_step(np);
        const size_t work = (np / ((size_t)step * step) + 12287) / 12288;
        const unsigned nblk = (unsigned)(work < 1 ? 1 : (work > (size_t)ECC_MAX_BLOCKS ? ECC_MAX_BLOCKS : work));
        hipLaunchKernelGGL(ecc_h_from_similarity, dim3(cdiv(n, 64)), dim3(64), 0, st, (const EccState*)al->dstate, al->dstate_h, n, Rn);
        for (int it = 0; it < max_iters;) {
            const int chunk = std::min(it == 0 ? ECC_CHUNK_FIRST : ECC_CHUNK_NEXT, max_iters - it);
            for (int j = 0; j < chunk; ++j)
                hipLaunchKernelGGL(ecc_accumulate_h, dim3(nblk, n), dim3(256), 0, st, L.tmpl, L.img, np, L.h, L.w, al->dstate_h, step,
                                   al->partial, al->ticket, eps);
            it += chunk;
            MI_HIP(hipMemcpyAsync(hh, al->dstate_h, sizeof(EccStateH) * n, hipMemcpyDeviceToHost, st));
            MI_HIP(hipStreamSynchronize(st));
            int nact = 0;
            for (int k = 0; k < n; ++k) nact += hh[k].active;
            if (!nact) break;
        }
        MI_HIP(hipGetLastError());
    }
    MI_HIP(hipMemcpyAsync(hs, al->dstate, sizeof(EccState) * n, hipMemcpyDeviceToHost, st));
    if (M9_out) MI_HIP(hipMemcpyAsync(hh, al->dstate_h, sizeof(EccStateH) * n, hipMemcpyDeviceToHost, st));
    MI_HIP(hipStreamSynchronize(st));
    const double s = (double)al->subsample;
    for (int k = 0; k < n; ++k) {
        const EccState& f = hs[k];
        double Msim[6];
        double* M = M_out ? M_out + 6 * k : Msim;
        // M (moving -> reference) = W^-1, translation back to full-resolution pixels
        const double det = f.a * f.a + f.b * f.b;
        const bool bad = f.failed || !(det > 1e-12);
        const double ia = bad ? 1.0 : f.a / det, ib = bad ? 0.0 : -f.b / det;  // A^-1 = [ia -ib; ib ia]
        M[0] = ia;  M[1] = -ib; M[2] = bad ? 0.0 : -(ia * f.T0 - ib * f.T1) * s;
        M[3] = ib;  M[4] = ia;  M[5] = bad ? 0.0 : -(ib * f.T0 + ia * f.T1) * s;
        if (cc_out) cc_out[k] = bad ? -2.0 : f.rho;
        if (iters_out) iters_out[k] = f.iters;
        if (M9_out) {
            double* M9 = M9_out + 9 * k;
            const EccStateH& g = hh[k];
            bool use_h = !bad && !g.failed && g.iters > 0 && g.rho >= f.rho - 1e-9;
            if (use_h) {
                // W (reference -> moving) = T(c) S(R) Hn S(1/R) T(-c) at the sub-sampled scale, S(s) W S(1/s) in full-resolution
                // pixels; M = W^-1, normalised
                const double Hn[9] = {g.h[0], g.h[1], g.h[2], g.h[3], g.h[4], g.h[5], g.h[6], g.h[7], 1.0};
                auto mul = [](const double* A, const double* B, double* C) {
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
                };
                const double L1[9] = {s * Rn, 0, s * cx0, 0, s * Rn, s * cy0, 0, 0, 1};                 // S(s) T(c) S(R)
                const double R1[9] = {1 / (s * Rn), 0, -cx0 / Rn, 0, 1 / (s * Rn), -cy0 / Rn, 0, 0, 1};   // S(1/R) T(-c) S(1/s)
                double t1[9], Wm[9];
                mul(L1, Hn, t1);
                mul(t1, R1, Wm);
                const double det = Wm[0] * (Wm[4] * Wm[8] - Wm[5] * Wm[7]) - Wm[1] * (Wm[3] * Wm[8] - Wm[5] * Wm[6]) +
                                   Wm[2] * (Wm[3] * Wm[7] - Wm[4] * Wm[6]);
                if (fabs(det) > 1e-12) {
                    const double id = 1.0 / det;
                    double I[9] = {(Wm[4] * Wm[8] - Wm[5] * Wm[7]) * id, (Wm[2] * Wm[7] - Wm[1] * Wm[8]) * id, (Wm[1] * Wm[5] - Wm[2] * Wm[4]) * id,
                                   (Wm[5] * Wm[6] - Wm[3] * Wm[8]) * id, (Wm[0] * Wm[8] - Wm[2] * Wm[6]) * id, (Wm[2] * Wm[3] - Wm[0] * Wm[5]) * id,
                                   (Wm[3] * Wm[7] - Wm[4] * Wm[6]) * id, (Wm[1] * Wm[6] - Wm[0] * Wm[7]) * id, (Wm[0] * Wm[4] - Wm[1] * Wm[3]) * id};
                    if (fabs(I[8]) > 1e-12) {
                        for (int q = 0; q < 9; ++q) M9[q] = I[q] / I[8];
                        if (cc_out) cc_out[k] = g.rho;
                        if (iters_out) iters_out[k] = f.iters + g.iters;
                    } else use_h = false;
                } else use_h = false;
            }
            if (!use_h) {
                for (int q = 0; q < 6; ++q) M9[q] = M[q];
                M9[6] = 0.0; M9[7] = 0.0; M9[8] = 1.0;
            }
        }
    }
    return MI_OK;
}

}  // namespace

extern "C" {

int mi_abi_version(void) { return MI_ABI_VERSION; }

const char* mi_last_error(void) { return last_error().c_str(); }

int mi_device_count(int* count) {
    if (!count) return fail(MI_ERR_INVALID, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(MI_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return MI_OK;
}

int mi_device_name(int device, char* buf, size_t buflen) {
    if (!buf || !buflen) return fail(MI_ERR_INVALID, "null buffer");
    hipDeviceProp_t prop;
    MI_HIP(hipGetDeviceProperties(&prop, device));
    snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return MI_OK;
}

void mi_stack_default_params(mi_stack_params_t* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->in_dtype = MI_U8;
    p->out_dtype = MI_U8;
    p->min_size = 32;
    p->kernel_size = 5;
    p->gen_kernel = 0.4;
    p->float_type = MI_F32;
    p->use_fma = 1;
    p->device = 0;
    p->impl = MI_IMPL_AUTO;
    p->batch_frames = 0;
}

int mi_device_malloc(int device, size_t bytes, void** dev_ptr) {
    if (!dev_ptr) return fail(MI_ERR_INVALID, "null out pointer");
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipMalloc(dev_ptr, bytes ? bytes : 1));
    return MI_OK;
}
int mi_device_free(int device, void* dev_ptr) {
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipFree(dev_ptr));
    return MI_OK;
}
int mi_memcpy_h2d(int device, void* dev_dst, const void* host_src, size_t bytes) {
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
    return MI_OK;
}
int mi_memcpy_d2h(int device, void* host_dst, const void* dev_src, size_t bytes) {
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi_memcpy_d2d(int device, void* dev_dst, const void* dev_src, size_t bytes) {
    if (!dev_dst || !dev_src) return fail(MI_ERR_INVALID, "null pointer");
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipMemcpy(dev_dst, dev_src, bytes, hipMemcpyDeviceToDevice));
    return MI_OK;
}

int mi_memcpy_d2d_async(int device, void* stream, void* dev_dst, const void* dev_src, size_t bytes) {
    if (!dev_dst || !dev_src) return fail(MI_ERR_INVALID, "null pointer");
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipMemcpyAsync(dev_dst, dev_src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MI_OK;
}
int mi_device_synchronize(int device) {
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipDeviceSynchronize());
    return MI_OK;
}

int mi_pyr_step(int device, int op, int use_fma, double gen_kernel, const void* host_in, const void* host_in2, int n, int h,
                int w, int c, int h2, int w2, double maxv, void* host_out) {
    if (!host_in || !host_out) return fail(MI_ERR_INVALID, "null argument");
    if (h < 1 || w < 1 || (c != 1 && c != 3) || n < 1) return fail(MI_ERR_INVALID, "bad geometry");
    if (op < MI_PYR_CONVOLVE || op > MI_PYR_CLIP_ABS) return fail(MI_ERR_INVALID, "bad op %d", op);
    MI_HIP(hipSetDevice(device));
    K25 K{};
    {
        const double a = gen_kernel, k[5] = {0.25 - a / 2.0, 0.25, a, 0.25, 0.25 - a / 2.0};
        for (int i = 0; i < 5; ++i)
            for (int j = 0; j < 5; ++j) K.k[i * 5 + j] = (float)(k[i] * k[j]);
    }
    const size_t npx = (size_t)h * w;
    size_t in_elems = npx * c, out_elems = npx * c, in2_elems = 0;
    if (op == MI_PYR_REDUCE) out_elems = (size_t)((h + 1) / 2) * ((w + 1) / 2) * c;
    else if (op == MI_PYR_EXPAND) out_elems = npx * 4 * c;
    else if (op == MI_PYR_FUSE_LAPLACIAN) {
        if (c != 3) return fail(MI_ERR_INVALID, "fuse_laplacian takes 3-channel images");
        in_elems = npx * 3 * n;
        out_elems = npx * 3;
    } else if (op == MI_PYR_COLLAPSE_STEP) {
        if (!host_in2 || h2 < 1 || w2 < 1 || 2 * h2 < h || 2 * w2 < w) return fail(MI_ERR_INVALID, "bad coarse level");
        in2_elems = (size_t)h2 * w2 * c;
    }
    hipStream_t st = nullptr;
    DevScratch tmp(st);
    float *din = nullptr, *dout = nullptr;
    int rc;
    if ((rc = tmp.upload(&din, host_in, in_elems * sizeof(float))) || (rc = tmp.alloc(&dout, out_elems * sizeof(float)))) return rc;
    const bool fma = use_fma != 0;
    if (op <= MI_PYR_EXPAND) {
        if (c == 3) fma ? pyr_step_launch<3, true>(op, st, din, h, w, dout, K) : pyr_step_launch<3, false>(op, st, din, h, w, dout, K);
        else fma ? pyr_step_launch<1, true>(op, st, din, h, w, dout, K) : pyr_step_launch<1, false>(op, st, din, h, w, dout, K);
    } else if (op == MI_PYR_FUSE_LAPLACIAN) {
        float *q = nullptr, *e = nullptr;
        if ((rc = tmp.alloc(&q, npx * n * sizeof(float))) || (rc = tmp.alloc(&e, npx * n * sizeof(float)))) return rc;
        const unsigned g1 = (unsigned)((npx * n + 255) / 256);
        if (fma) hipLaunchKernelGGL((step_gray_sq<true>), dim3(g1), dim3(256), 0, st, (const float*)din, npx * n, q);
        else hipLaunchKernelGGL((step_gray_sq<false>), dim3(g1), dim3(256), 0, st, (const float*)din, npx * n, q);
        for (int i = 0; i < n; ++i)
            fma ? pyr_step_launch<1, true>(MI_PYR_CONVOLVE, st, q + (size_t)i * npx, h, w, e + (size_t)i * npx, K)
                : pyr_step_launch<1, false>(MI_PYR_CONVOLVE, st, q + (size_t)i * npx, h, w, e + (size_t)i * npx, K);
        hipLaunchKernelGGL(step_fuse, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, st, (const float*)e, (const float*)din, n, npx, dout);
    } else if (op == MI_PYR_COLLAPSE_STEP) {
        float *din2 = nullptr, *up = nullptr;
        if ((rc = tmp.upload(&din2, host_in2, in2_elems * sizeof(float))) || (rc = tmp.alloc(&up, (size_t)h2 * w2 * 4 * c * sizeof(float))))
            return rc;
        if (c == 3) fma ? pyr_step_launch<3, true>(MI_PYR_EXPAND, st, din2, h2, w2, up, K) : pyr_step_launch<3, false>(MI_PYR_EXPAND, st, din2, h2, w2, up, K);
        else fma ? pyr_step_launch<1, true>(MI_PYR_EXPAND, st, din2, h2, w2, up, K) : pyr_step_launch<1, false>(MI_PYR_EXPAND, st, din2, h2, w2, up, K);
        hipLaunchKernelGGL(step_add_crop, dim3(cdiv(w, 64), cdiv(h, 4)), dim3(64, 4), 0, st, (const float*)up, 2 * w2, (const float*)din, h, w, c, dout);
    } else {   // MI_PYR_CLIP_ABS
        hipLaunchKernelGGL(step_clip_abs, dim3((unsigned)((out_elems + 255) / 256)), dim3(256), 0, st, (const float*)din, out_elems, (float)maxv, dout);
    }
    return tmp.download(host_out, dout, out_elems * sizeof(float));
}

int mi_device_mem_info(int device, size_t* free_bytes, size_t* total_bytes) {
    if (!free_bytes || !total_bytes) return fail(MI_ERR_INVALID, "null argument");
    MI_HIP(hipSetDevice(device));
    MI_HIP(hipMemGetInfo(free_bytes, total_bytes));
    return MI_OK;
}

int mi_stack_create(mi_stack_t** out, const mi_stack_params_t* params) {
    if (!out || !params) return fail(MI_ERR_INVALID, "null argument");
    *out = nullptr;
    const mi_stack_params_t& p = *params;
    if (p.height < 1 || p.width < 1) return fail(MI_ERR_INVALID, "bad frame size %dx%d", p.width, p.height);
    // the kernels address pixels inside a frame with 32-bit byte offsets (12 bytes per float pixel)
    if ((uint64_t)p.height * (uint64_t)p.width * 12ull >= (1ull << 32))
        return fail(MI_ERR_UNSUPPORTED, "frames of %dx%d exceed the 357-megapixel limit of the 32-bit in-frame addressing",
                    p.width, p.height);
    if (p.in_dtype != MI_U8 && p.in_dtype != MI_U16 && p.in_dtype != MI_F32)
        return fail(MI_ERR_INVALID, "in_dtype must be MI_U8, MI_U16 or MI_F32");
    if (p.out_dtype != MI_U8 && p.out_dtype != MI_U16)
        return fail(MI_ERR_INVALID, "out_dtype must be MI_U8 or MI_U16");
    if (p.float_type != MI_F32 && p.float_type != MI_F64) return fail(MI_ERR_INVALID, "bad float_type %d", p.float_type);
    if (p.min_size < 1) return fail(MI_ERR_INVALID, "min_size must be >= 1");
    if (p.kernel_size < 1 || p.kernel_size > 12)
        return fail(MI_ERR_INVALID, "kernel_size must be in [1, 12] (base window <= 11x11)");
    if (p.impl < MI_IMPL_AUTO || p.impl > MI_IMPL_TILED) return fail(MI_ERR_INVALID, "bad impl %d", p.impl);
    if (p.arith != MI_ARITH_EXACT && p.arith != MI_ARITH_SEPARABLE) return fail(MI_ERR_INVALID, "bad arith %d", p.arith);
    if (p.arith == MI_ARITH_SEPARABLE && p.float_type != MI_F32)
        return fail(MI_ERR_INVALID, "MI_ARITH_SEPARABLE needs float_type MI_F32");
    if (p.pair_levels < 0 || p.pair_levels > 3) return fail(MI_ERR_INVALID, "pair_levels must be 0 (automatic), 1 (pairs from level 0 on), 2 (none) or 3 (pairs from level 1 on)");
    int ndev = 0;
    int rc = visible_devices(&ndev);
    if (rc) return rc;
    if (p.device < 0 || p.device >= ndev) return fail(MI_ERR_INVALID, "device %d out of range (have %d)", p.device, ndev);
    MI_HIP(hipSetDevice(p.device));

    mi_stack* s = new mi_stack();
    s->p = p;
    if (s->p.impl == MI_IMPL_AUTO) s->p.impl = MI_IMPL_TILED;
    // levels = int(log2(min(h,w)/min_size)), pyramid.py:165; stop when a side < 4, :129-130
    {
        double r = (double)(p.height < p.width ? p.height : p.width) / (double)p.min_size;
        int req = r >= 1.0 ? (int)std::log2(r) : 0;
        // guard against log2 rounding at exact powers of two (np.log2 is exact there)
        while (req > 0 && (double)(1 << req) > r) --req;
        while ((double)(1 << (req + 1)) <= r) ++req;
        int h = p.height, w = p.width;
        s->lh.push_back(h);
        s->lw.push_back(w);
        for (int i = 0; i < req; ++i) {
            h = (h + 1) / 2;
            w = (w + 1) / 2;
            if ((h < w ? h : w) < 4) break;
            s->lh.push_back(h);
            s->lw.push_back(w);
        }
        s->L = (int)s->lh.size() - 1;
    }
    if (s->L == 0) s->p.impl = MI_IMPL_SIMPLE;  // base-only stacks (tiny frames): one frame at a time
    s->f64 = p.float_type == MI_F64;
    if (s->f64) s->p.impl = MI_IMPL_SIMPLE;     // the precision option runs the one-frame-at-a-time formulation
    {
        double a = p.gen_kernel;
        double k[5] = {0.25 - a / 2.0, 0.25, a, 0.25, 0.25 - a / 2.0};
        for (int i = 0; i < 5; ++i)
            for (int j = 0; j < 5; ++j) {
                s->K.k[i * 5 + j] = (float)(k[i] * k[j]);
                s->Kd.k[i * 5 + j] = k[i] * k[j];
            }
        for (int i = 0; i < 3; ++i) s->k1d[i] = (float)k[i];
        s->sep = p.arith == MI_ARITH_SEPARABLE;
        red_taps(a, s->rk);
    }
    s->pad = (p.kernel_size - 1) / 2;
    s->nlevels_hist = p.out_dtype == MI_U8 ? 256 : 65536;
    s->maxv = p.out_dtype == MI_U8 ? 255.f : 65535.f;

#define TRY(x)                     \
    do {                           \
        rc = (x);                  \
        if (rc) {                  \
            mi_stack_destroy(s);   \
            return rc;             \
        }                          \
    } while (0)
    hipError_t he = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (he != hipSuccess) {
        delete s;
        return fail(MI_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(he));
    }
    const int L = s->L;
    const size_t P0 = (size_t)p.height * p.width;
    const size_t fm = s->f64 ? 2 : 1;   // float_type-sized buffers are allocated in units of float
    TRY(dev_alloc(s, &s->frame_dev, P0 * 3 * dtype_size(p.in_dtype)));
    s->G.assign(L + 1, nullptr);
    s->bestE.assign(L, nullptr);
    s->bestLap.assign(L, nullptr);
    s->bestIdx.assign(L, nullptr);
    for (int l = 1; l <= L; ++l) TRY(dev_alloc_t(s, &s->G[l], (size_t)s->lh[l] * s->lw[l] * 3 * fm));
    std::vector<size_t> seg_off(L + 2, 0);
    if (!s->f64) {
        size_t off = 0;
        for (int k = 0; k < L + 2; ++k) {
            seg_off[k] = off;
            const int lv = k < L ? k : L;
            off += (((size_t)s->lh[lv] * s->lw[lv]) + 63) / 64 * 64;
        }
        s->slab_px = off;
        TRY(dev_alloc_t(s, &s->slabE, off));
        TRY(dev_alloc_t(s, &s->slabI, off));
        TRY(dev_alloc_t(s, &s->slabL, off * 3));
        // on the handle's stream, and waited for: a plain hipMemset runs on the null stream, which the handle's non-blocking
        // streams do not wait for -- it could land after the first pushed frame's kernels and zero part of their state
        MI_HIP(hipMemsetAsync(s->slabE, 0, off * 4, s->stream));
        MI_HIP(hipMemsetAsync(s->slabI, 0, off * 4, s->stream));
        MI_HIP(hipMemsetAsync(s->slabL, 0, off * 12, s->stream));
        MI_HIP(hipStreamSynchronize(s->stream));
    }
    for (int l = 0; l < L; ++l) {
        size_t np = (size_t)s->lh[l] * s->lw[l];
        if (!s->f64) {
            s->bestE[l] = s->slabE + seg_off[l];
            s->bestLap[l] = s->slabL + seg_off[l] * 3;
            s->bestIdx[l] = s->slabI + seg_off[l];
            continue;
        }
        TRY(dev_alloc_t(s, &s->bestE[l], np));
        TRY(dev_alloc_t(s, &s->bestLap[l], np * 3 * fm));
        TRY(dev_alloc_t(s, &s->bestIdx[l], np));
    }
    if (s->p.impl == MI_IMPL_SIMPLE) {
        TRY(dev_alloc_t(s, &s->lap_tmp, P0 * 3 * fm));
        TRY(dev_alloc_t(s, &s->q_tmp, P0));
    }
    {
        size_t nb = (size_t)s->lh[L] * s->lw[L];
        TRY(dev_alloc_t(s, &s->lev, nb));
        TRY(dev_alloc_t(s, &s->cnt, (size_t)s->nlevels_hist));
        TRY(dev_alloc_t(s, &s->logp, (size_t)s->nlevels_hist * fm));
        if (!s->f64) {
            s->bEnt = s->slabE + seg_off[L];      s->bDev = s->slabE + seg_off[L + 1];
            s->idxE = s->slabI + seg_off[L];      s->idxD = s->slabI + seg_off[L + 1];
            s->baseE = s->slabL + seg_off[L] * 3; s->baseD = s->slabL + seg_off[L + 1] * 3;
        } else {
            TRY(dev_alloc_t(s, &s->bEnt, nb * fm));
            TRY(dev_alloc_t(s, &s->bDev, nb * fm));
            TRY(dev_alloc_t(s, &s->idxE, nb));
            TRY(dev_alloc_t(s, &s->idxD, nb));
            TRY(dev_alloc_t(s, &s->baseE, nb * 3 * fm));
            TRY(dev_alloc_t(s, &s->baseD, nb * 3 * fm));
        }
        TRY(dev_alloc_t(s, &s->fusedBase, nb * 3 * fm));
    }
    TRY(dev_alloc_t(s, &s->colA, P0 * 3 * fm));
    TRY(dev_alloc_t(s, &s->colB, (L >= 2 ? (size_t)s->lh[1] * s->lw[1] * 3 : 1) * fm));
    TRY(dev_alloc_t(s, &s->clipped, P0 * 3 * fm));
    TRY(dev_alloc(s, &s->out_dev, P0 * 3 * dtype_size(p.out_dtype)));
    TRY(tiled_create(s));
#undef TRY
    *out = s;
    return MI_OK;
}

void mi_stack_destroy(mi_stack_t* s) {
    if (!s) return;
    (void)hipSetDevice(s->p.device);
    (void)tiled_sync_all(s);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    mosaic_destroy(s);
    tiled_destroy(s);
    for (auto& r : s->recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (auto e : s->ev_pool) (void)hipEventDestroy(e);
    for (void* p : s->allocs) (void)hipFree(p);
    if (s->aux) (void)hipStreamDestroy(s->aux);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

int mi_stack_reset(mi_stack_t* s) {
    int rc = check_handle(s);
    if (rc) return rc;
    MI_HIP(hipSetDevice(s->p.device));
    rc = tiled_sync_all(s);
    if (rc) return rc;
    if ((rc = mosaic_sync(s))) return rc;
    MI_HIP(hipStreamSynchronize(s->stream));
    rc = prof_drain(s);
    if (rc) return rc;
    mosaic_reset(s);
    s->n_pushed = 0;
    s->finished = false;
    s->idx_exported = 0;
    return tiled_reset(s);
}

int mi_stack_levels(const mi_stack_t* s, int* levels) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!levels) return fail(MI_ERR_INVALID, "null levels");
    *levels = s->L;
    return MI_OK;
}

int mi_stack_level_shape(const mi_stack_t* s, int level, int* h, int* w) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (level < 0 || level > s->L || !h || !w) return fail(MI_ERR_INVALID, "bad level %d", level);
    *h = s->lh[level];
    *w = s->lw[level];
    return MI_OK;
}

int mi_stack_frames_pushed(const mi_stack_t* s, int* n) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!n) return fail(MI_ERR_INVALID, "null n");
    *n = s->n_pushed + stack_pending(s);
    return MI_OK;
}

int mi_stack_set_first_index(mi_stack_t* s, int first_global_index) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (s->n_pushed + stack_pending(s) != 0) return fail(MI_ERR_STATE, "set_first_index after frames were pushed");
    s->first_index = first_global_index;
    return MI_OK;
}

int mi_stack_set_index_stride(mi_stack_t* s, int stride) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (stride < 1) return fail(MI_ERR_INVALID, "index stride must be >= 1");
    if (s->n_pushed + stack_pending(s) != 0) return fail(MI_ERR_STATE, "set_index_stride after frames were pushed");
    s->index_stride = stride;
    return MI_OK;
}

// The kernels number the frames of a handle consecutively from first_index; with an index stride the stored winner indices
// are rewritten once, in place, into the global numbering (first + k * stride), level by level: the level's bit in
// idx_exported is set, and the handle takes no more frames until it is reset (the payload passes look winners up by the
// consecutive numbers).
static int export_level_indices(mi_stack* s, int level) {
    if (s->index_stride == 1 || ((s->idx_exported >> level) & 1ull)) return MI_OK;
    int32_t* idx = level < s->L ? s->bestIdx[level] : level == s->L ? s->idxE : s->idxD;
    const size_t n = (size_t)s->lh[std::min(level, s->L)] * s->lw[std::min(level, s->L)];
    if (!s->aux) MI_HIP(hipStreamCreateWithFlags(&s->aux, hipStreamNonBlocking));
    hipLaunchKernelGGL(idx_export, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->aux, idx, n, s->first_index, s->index_stride);
    MI_HIP(hipGetLastError());
    s->idx_exported |= 1ull << level;
    return MI_OK;
}

int mi_stack_export_indices(mi_stack_t* s, int level) {
    int rc = check_handle(s);
    if (rc) return rc;
    MI_HIP(hipSetDevice(s->p.device));
    if (level < -1 || level > s->L + 1) return fail(MI_ERR_INVALID, "bad level %d", level);
    if ((rc = stack_flush(s))) return rc;
    // the level's state must be final: level 0 is, once its last payload pass is through; everything else needs all of it
    if (level == 0) rc = tiled_sync_level0(s);
    else { rc = tiled_sync_all(s); if (!rc) MI_HIP(hipStreamSynchronize(s->stream)); }
    if (rc) return rc;
    for (int l = (level < 0 ? 0 : level); l <= (level < 0 ? s->L + 1 : level); ++l)
        if ((rc = export_level_indices(s, l))) return rc;
    if (s->aux) MI_HIP(hipStreamSynchronize(s->aux));
    return MI_OK;
}

int mi_stack_push_frames_device(mi_stack_t* s, const void* dev_frames, int n, size_t frame_stride_bytes) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (s->idx_exported) return fail(MI_ERR_STATE, "the winner indices were exported (index stride > 1): reset the handle before pushing more frames");
    if (!dev_frames || n < 0) return fail(MI_ERR_INVALID, "bad frames argument");
    if (s->finished) return fail(MI_ERR_STATE, "push after finish; call mi_stack_reset first");
    size_t fb = (size_t)s->p.height * s->p.width * 3 * dtype_size(s->p.in_dtype);
    if (frame_stride_bytes == 0) frame_stride_bytes = fb;
    if (frame_stride_bytes < fb) return fail(MI_ERR_INVALID, "frame stride smaller than a frame");
    MI_HIP(hipSetDevice(s->p.device));
    if ((rc = mosaic_flush(s))) return rc;   // call order: mosaics staged before these frames are fused first
    return dispatch_push(s, dev_frames, n, frame_stride_bytes);
}

int mi_stack_push_frame(mi_stack_t* s, const void* host_bgr, size_t row_stride_bytes) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (s->idx_exported) return fail(MI_ERR_STATE, "the winner indices were exported (index stride > 1): reset the handle before pushing more frames");
    if (!host_bgr) return fail(MI_ERR_INVALID, "null frame");
    if (s->finished) return fail(MI_ERR_STATE, "push after finish; call mi_stack_reset first");
    MI_HIP(hipSetDevice(s->p.device));
    if ((rc = mosaic_flush(s))) return rc;   // call order
    return tiled_push_host(s, host_bgr, row_stride_bytes);
}

// a zero-copy push reads `p` in place: it must lie in pinned host memory (`fn`: the entry point, `what`: the noun of its message)
static int pinned_probe(const void* p, const char* fn, const char* what) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost) return MI_OK;
    (void)hipGetLastError();
    return fail(MI_ERR_INVALID, "%s: the %s is not in pinned host memory (mi_host_alloc / mi_host_register)", fn, what);
}

int mi_stack_push_frame_pinned(mi_stack_t* s, const void* host_bgr, size_t row_stride_bytes) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!host_bgr) return fail(MI_ERR_INVALID, "null frame");
    if (s->finished) return fail(MI_ERR_STATE, "push after finish; call mi_stack_reset first");
    if (s->idx_exported) return fail(MI_ERR_STATE, "the winner indices were exported (index stride > 1): reset the handle before pushing more frames");
    if (s->p.impl != MI_IMPL_TILED || s->f64) return mi_stack_push_frame(s, host_bgr, row_stride_bytes);   // synchronous paths
    MI_HIP(hipSetDevice(s->p.device));
    if ((rc = pinned_probe(host_bgr, "mi_stack_push_frame_pinned", "frame"))) return rc;
    if ((rc = mosaic_flush(s))) return rc;   // call order
    return tiled_push_host(s, host_bgr, row_stride_bytes, true);
}

int mi_stack_wait_uploads(mi_stack_t* s, int max_outstanding) {
    int rc = check_handle(s);
    if (rc) return rc;
    MI_HIP(hipSetDevice(s->p.device));
    return mosaic_wait_uploads(s, max_outstanding);
}

// ---------------------------------------------------------------- raw mosaics (kernels_demosaic.hpp, mosaic_host.hpp)
static int demosaic_check(const void* mosaic, const void* bgr, int height, int width, int dtype, const mi_cfa_t* cfa) {
    if (!mosaic) return fail(MI_ERR_INVALID, "null mosaic");
    if (!bgr) return fail(MI_ERR_INVALID, "null bgr output");
    if (height < 2 || width < 2) return fail(MI_ERR_INVALID, "height and width must be >= 2 for a mosaic (got %dx%d)", width, height);
    if ((uint64_t)height * (uint64_t)width * 3ull >= (1ull << 32)) return fail(MI_ERR_INVALID, "height x width too large");
    return cfa_check(cfa, dtype);
}

int mi_demosaic_device(int device, void* stream, const void* dev_mosaic, void* dev_bgr, int height, int width, int dtype,
                       const mi_cfa_t* cfa) {
    int rc = demosaic_check(dev_mosaic, dev_bgr, height, width, dtype, cfa);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    demosaic_launch((hipStream_t)stream, dev_mosaic, dev_bgr, height, width, dtype, *cfa);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_demosaic(int device, const void* host_mosaic, void* host_bgr, int height, int width, int dtype, const mi_cfa_t* cfa) {
    int rc = demosaic_check(host_mosaic, host_bgr, height, width, dtype, cfa);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nb = (size_t)height * width * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *src = nullptr, *dst = nullptr;
    if ((rc = tmp.upload(&src, host_mosaic, nb)) || (rc = tmp.alloc(&dst, nb * 3)) ||
        (rc = mi_demosaic_device(device, nullptr, src, dst, height, width, dtype, cfa)))
        return rc;
    return tmp.download(host_bgr, dst, nb * 3);
}

// The raw pushes (mi_stack_push_mosaic*, mi_stack_push_packed, mi_stack_push_ljpeg) check in one order: the source, the
// arguments below, the handle's state, the pinned source.  `need_calib`, `need_develop`: a null one is an error, not "none";
// `sites`: the entry point takes defect sites.
static int raw_args_check(const mi_stack_t* s, const mi_cfa_t* cfa, const mi_calib_t* calib, bool need_calib, const mi_develop_t* develop,
                          bool need_develop, bool sites, const int32_t* dev_sites, int n_sites) {
    int rc;
    if ((rc = cfa_check(cfa, s->p.in_dtype)) || ((calib || need_calib) && (rc = calib_check(calib))) ||
        ((develop || need_develop) && (rc = develop_check(develop))) || (sites && (rc = sites_check(dev_sites, n_sites, s->p.height, s->p.width))))
        return rc;
    return MI_OK;
}
// the handle takes a raw frame now; *async: it takes it on the copy stream, so a pinned source is read in place
static int raw_state_check(const mi_stack_t* s, bool* async) {
    if (s->idx_exported) return fail(MI_ERR_STATE, "the winner indices were exported (index stride > 1): reset the handle before pushing more frames");
    if (s->finished) return fail(MI_ERR_STATE, "push after finish; call mi_stack_reset first");
    MI_HIP(hipSetDevice(s->p.device));
    *async = s->p.impl == MI_IMPL_TILED && !s->f64;
    return MI_OK;
}

// the three mosaic pushes behind check_handle; `fn`: the entry point's name.  Absent arguments are null and not needed.
static int mosaic_entry(mi_stack_t* s, const char* fn, const void* host_mosaic, size_t row_stride_bytes, const mi_cfa_t* cfa,
                        const mi_calib_t* calib, bool need_calib, const mi_develop_t* develop, bool need_develop, const int32_t* dev_sites,
                        int n_sites, int pinned) {
    int rc;
    bool async;
    if (!host_mosaic) return fail(MI_ERR_INVALID, "null mosaic");
    if (s->p.height < 2 || s->p.width < 2) return fail(MI_ERR_INVALID, "height and width must be >= 2 for a mosaic");
    if ((rc = raw_args_check(s, cfa, calib, need_calib, develop, need_develop, need_calib || need_develop, dev_sites, n_sites))) return rc;
    const size_t rb = (size_t)s->p.width * dtype_size(s->p.in_dtype);
    if (row_stride_bytes == 0) row_stride_bytes = rb;
    if (row_stride_bytes < rb) return fail(MI_ERR_INVALID, "row stride smaller than a row");
    if ((rc = raw_state_check(s, &async))) return rc;
    if (pinned && async) {
        if (row_stride_bytes != rb) return fail(MI_ERR_INVALID, "a pinned mosaic must have contiguous rows");
        if ((rc = pinned_probe(host_mosaic, fn, "mosaic"))) return rc;
    }
    return mosaic_push(s, MosaicFrame{host_mosaic, row_stride_bytes, nullptr, cfa, pinned && async, calib, develop, dev_sites, n_sites});
}

int mi_stack_push_mosaic(mi_stack_t* s, const void* host_mosaic, size_t row_stride_bytes, const mi_cfa_t* cfa, int pinned) {
    int rc = check_handle(s);
    if (rc) return rc;
    return mosaic_entry(s, "mi_stack_push_mosaic", host_mosaic, row_stride_bytes, cfa, nullptr, false, nullptr, false, nullptr, 0, pinned);
}

// ---------------------------------------------------------------- raw development: defect sites, colour matrix, tone curve
int mi_mosaic_defects_device(int device, void* stream, void* dev_mosaic, int height, int width, int dtype, const int32_t* dev_sites,
                             int n) {
    if (!dev_mosaic) return fail(MI_ERR_INVALID, "null mosaic");
    if (height < 2 || width < 2) return fail(MI_ERR_INVALID, "height and width must be >= 2 for a mosaic (got %dx%d)", width, height);
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16 for a mosaic (got %d)", dtype);
    int rc = sites_check(dev_sites, n, height, width);
    if (rc) return rc;
    if (n == 0) return MI_OK;
    MI_HIP(hipSetDevice(device));
    defects_launch((hipStream_t)stream, dev_mosaic, height, width, dtype, dev_sites, n);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_develop_device(int device, void* stream, const void* dev_mosaic, void* dev_bgr, int height, int width, int dtype,
                      const mi_cfa_t* cfa, const mi_develop_t* develop) {
    int rc = demosaic_check(dev_mosaic, dev_bgr, height, width, dtype, cfa);
    if (rc || (rc = develop_check(develop))) return rc;
    MI_HIP(hipSetDevice(device));
    develop_launch((hipStream_t)stream, dev_mosaic, dev_bgr, height, width, dtype, *cfa, *develop);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_develop(int device, const void* host_mosaic, void* host_bgr, int height, int width, int dtype, const mi_cfa_t* cfa,
               const int32_t* matrix_q, const void* host_tone, const int32_t* host_sites, int n) {
    int rc = demosaic_check(host_mosaic, host_bgr, height, width, dtype, cfa);
    if (rc || (matrix_q && (rc = matrix_check(matrix_q))) || (rc = sites_check(host_sites, n, height, width)) ||
        (rc = host_sites_check(host_sites, n, height, width)))
        return rc;
    if ((rc = open_device(device))) return rc;
    const size_t isz = dtype_size(dtype), nb = (size_t)height * width * isz;
    mi_develop_t d{};
    if (matrix_q) {
        d.flags |= MI_DEVELOP_MATRIX;
        memcpy(d.matrix_q, matrix_q, sizeof(d.matrix_q));
    }
    DevScratch tmp(nullptr);
    void *src = nullptr, *dst = nullptr, *tone = nullptr;
    int32_t* sites = nullptr;
    if ((rc = tmp.upload(&src, host_mosaic, nb)) || (rc = tmp.alloc(&dst, nb * 3))) return rc;
    if (host_tone) {
        if ((rc = tmp.upload(&tone, host_tone, (dtype == MI_U8 ? 256 : 65536) * isz))) return rc;
        d.flags |= MI_DEVELOP_TONE;
        d.dev_tone = tone;
    }
    if (n > 0 && ((rc = tmp.upload(&sites, host_sites, (size_t)n * sizeof(int32_t))) ||
                  (rc = mi_mosaic_defects_device(device, nullptr, src, height, width, dtype, sites, n))))
        return rc;
    if ((rc = mi_develop_device(device, nullptr, src, dst, height, width, dtype, cfa, &d))) return rc;
    return tmp.download(host_bgr, dst, nb * 3);
}

int mi_stack_push_mosaic_developed(mi_stack_t* s, const void* host_mosaic, size_t row_stride_bytes, const mi_cfa_t* cfa,
                                   const mi_develop_t* develop, const int32_t* dev_sites, int n_sites, int pinned) {
    int rc = check_handle(s);
    if (rc) return rc;
    return mosaic_entry(s, "mi_stack_push_mosaic_developed", host_mosaic, row_stride_bytes, cfa, nullptr, false, develop, true, dev_sites,
                        n_sites, pinned);
}

// ---------------------------------------------------------------- linear raw frames (kernels_linear.hpp)
// argument checks of mi_linear_develop*: no device call
// (the levels alone: mi_stack_push_linear shares them)
static int linear_levels_check(const mi_linear_t* lin, int dtype);
static int linear_check(const void* samples, const void* bgr, int height, int width, int dtype, const mi_linear_t* lin) {
    if (!samples) return fail(MI_ERR_INVALID, "null samples");
    if (!bgr) return fail(MI_ERR_INVALID, "null bgr output");
    if (height < 1 || width < 1) return fail(MI_ERR_INVALID, "height and width must be >= 1 for a linear frame (got %dx%d)", width, height);
    if ((uint64_t)height * (uint64_t)width * 3ull >= (1ull << 32)) return fail(MI_ERR_INVALID, "height x width too large");
    return linear_levels_check(lin, dtype);
}
static int linear_levels_check(const mi_linear_t* lin, int dtype) {
    if (!lin) return fail(MI_ERR_INVALID, "null linear");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16 for a linear frame (got %d)", dtype);
    if (lin->spp != 1 && lin->spp != 3) return fail(MI_ERR_INVALID, "linear spp must be 1 or 3 (got %d)", lin->spp);
    const int maxv = dtype == MI_U8 ? 255 : 65535;
    for (int k = 0; k < 3; ++k) {
        if (lin->black[k] < 0) return fail(MI_ERR_INVALID, "linear black[%d] must be >= 0 (got %d)", k, lin->black[k]);
        if (lin->gain_q[k] > 65535u) return fail(MI_ERR_INVALID, "linear gain_q[%d] must be <= 65535 (got %u)", k, lin->gain_q[k]);
    }
    if (lin->white < 1 || lin->white > maxv) return fail(MI_ERR_INVALID, "linear white must be in [1, %d] (got %d)", maxv, lin->white);
    return MI_OK;
}

int mi_linear_span(int dtype) { return dtype == MI_U8 || dtype == MI_U16 ? linear_span(dtype) : 0; }

int mi_linear_develop_device(int device, void* stream, const void* dev_samples, void* dev_bgr, int height, int width, int dtype,
                             const mi_linear_t* linear, const mi_develop_t* develop) {
    int rc = linear_check(dev_samples, dev_bgr, height, width, dtype, linear);
    if (rc || (develop && (rc = develop_check(develop)))) return rc;
    if (((uintptr_t)dev_samples | (uintptr_t)dev_bgr) & (dtype_size(dtype) - 1))
        return fail(MI_ERR_INVALID, "dev_samples and dev_bgr must be aligned to their samples");
    MI_HIP(hipSetDevice(device));
    linear_develop_launch((hipStream_t)stream, dev_samples, dev_bgr, height, width, dtype, *linear, develop);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_linear_develop(int device, const void* host_samples, void* host_bgr, int height, int width, int dtype, const mi_linear_t* linear,
                      const int32_t* matrix_q, const void* host_tone) {
    int rc = linear_check(host_samples, host_bgr, height, width, dtype, linear);
    if (rc || (matrix_q && (rc = matrix_check(matrix_q)))) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t isz = dtype_size(dtype), npx = (size_t)height * width;
    mi_develop_t d{};
    if (matrix_q) {
        d.flags |= MI_DEVELOP_MATRIX;
        memcpy(d.matrix_q, matrix_q, sizeof(d.matrix_q));
    }
    DevScratch tmp(nullptr);
    void *src = nullptr, *dst = nullptr, *tone = nullptr;
    if ((rc = tmp.upload(&src, host_samples, npx * linear->spp * isz)) || (rc = tmp.alloc(&dst, npx * 3 * isz))) return rc;
    if (host_tone) {
        if ((rc = tmp.upload(&tone, host_tone, (dtype == MI_U8 ? 256 : 65536) * isz))) return rc;
        d.flags |= MI_DEVELOP_TONE;
        d.dev_tone = tone;
    }
    if ((rc = mi_linear_develop_device(device, nullptr, src, dst, height, width, dtype, linear, &d))) return rc;
    return tmp.download(host_bgr, dst, npx * 3 * isz);
}

// ---------------------------------------------------------------- raw calibration frames (kernels_calib.hpp)
int mi_mosaic_master_device(int device, void* stream, const void* dev_frames, int n, int height, int width, int dtype, int reject,
                            void* dev_out) {
    if (!dev_frames) return fail(MI_ERR_INVALID, "null frames");
    if (!dev_out) return fail(MI_ERR_INVALID, "null master output");
    int rc = calib_shape_check(height, width, dtype);
    if (rc || (rc = master_check(n, reject))) return rc;
    MI_HIP(hipSetDevice(device));
    master_launch((hipStream_t)stream, dev_frames, n, height, width, dtype, reject, dev_out);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_mosaic_master(int device, const void* const* host_frames, int n, int height, int width, int dtype, int reject, void* host_out) {
    if (!host_frames) return fail(MI_ERR_INVALID, "null frames");
    if (!host_out) return fail(MI_ERR_INVALID, "null master output");
    int rc = calib_shape_check(height, width, dtype);
    if (rc || (rc = master_check(n, reject))) return rc;
    for (int i = 0; i < n; ++i)
        if (!host_frames[i]) return fail(MI_ERR_INVALID, "null frames[%d]", i);
    if ((rc = open_device(device))) return rc;
    const size_t nb = (size_t)height * width * dtype_size(dtype);
    DevScratch tmp(nullptr);
    char* frames = nullptr;
    void* out = nullptr;
    if ((rc = tmp.alloc(&frames, nb * n)) || (rc = tmp.alloc(&out, nb))) return rc;
    for (int i = 0; i < n; ++i) MI_HIP(hipMemcpyAsync(frames + (size_t)i * nb, host_frames[i], nb, hipMemcpyHostToDevice, nullptr));
    if ((rc = mi_mosaic_master_device(device, nullptr, frames, n, height, width, dtype, reject, out))) return rc;
    return tmp.download(host_out, out, nb);
}

static int flat_check(const void* flat, const void* gain, int height, int width, int dtype, const mi_cfa_t* cfa) {
    if (!flat) return fail(MI_ERR_INVALID, "null flat");
    if (!gain) return fail(MI_ERR_INVALID, "null gain output");
    int rc = calib_shape_check(height, width, dtype);
    if (rc) return rc;
    return cfa_check(cfa, dtype);
}

int mi_flat_gain_device(int device, void* stream, const void* dev_flat, const void* dev_flat_dark, int height, int width, int dtype,
                        const mi_cfa_t* cfa, uint16_t* dev_gain_out) {
    int rc = flat_check(dev_flat, dev_gain_out, height, width, dtype, cfa);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    // the four position sums between the two passes: stream-ordered scratch, so the call does not wait
    unsigned long long* sums = nullptr;
    MI_HIP(hipMallocAsync((void**)&sums, 4 * sizeof(unsigned long long), (hipStream_t)stream));
    const hipError_t e = flat_gain_launch((hipStream_t)stream, dev_flat, dev_flat_dark, height, width, dtype, *cfa, sums, dev_gain_out);
    MI_HIP(hipFreeAsync(sums, (hipStream_t)stream));
    MI_HIP(e);
    return MI_OK;
}

int mi_flat_gain(int device, const void* host_flat, const void* host_flat_dark, int height, int width, int dtype, const mi_cfa_t* cfa,
                 uint16_t* host_gain_out) {
    int rc = flat_check(host_flat, host_gain_out, height, width, dtype, cfa);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t npx = (size_t)height * width, nb = npx * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *flat = nullptr, *fdark = nullptr;
    uint16_t* gain = nullptr;
    if ((rc = tmp.upload(&flat, host_flat, nb)) || (host_flat_dark && (rc = tmp.upload(&fdark, host_flat_dark, nb))) ||
        (rc = tmp.alloc(&gain, npx * sizeof(uint16_t))) ||
        (rc = mi_flat_gain_device(device, nullptr, flat, fdark, height, width, dtype, cfa, gain)))
        return rc;
    return tmp.download(host_gain_out, gain, npx * sizeof(uint16_t));
}

int mi_mosaic_calibrate_device(int device, void* stream, void* dev_mosaic, int height, int width, int dtype, const mi_cfa_t* cfa,
                               const mi_calib_t* calib) {
    if (!dev_mosaic) return fail(MI_ERR_INVALID, "null mosaic");
    int rc = calib_shape_check(height, width, dtype);
    if (rc || (rc = cfa_check(cfa, dtype)) || (rc = calib_check(calib))) return rc;
    if (calib->flags == 0) return MI_OK;   // nothing to do, no device call
    MI_HIP(hipSetDevice(device));
    calibrate_launch((hipStream_t)stream, dev_mosaic, height, width, dtype, *cfa, *calib);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_mosaic_calibrate(int device, const void* host_mosaic, void* host_out, int height, int width, int dtype, const mi_cfa_t* cfa,
                        const void* host_dark, const uint16_t* host_gain) {
    if (!host_mosaic) return fail(MI_ERR_INVALID, "null mosaic");
    if (!host_out) return fail(MI_ERR_INVALID, "null mosaic output");
    int rc = calib_shape_check(height, width, dtype);
    if (rc || (rc = cfa_check(cfa, dtype))) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t npx = (size_t)height * width, nb = npx * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *m = nullptr, *dark = nullptr;
    uint16_t* gain = nullptr;
    mi_calib_t c{};
    if ((rc = tmp.upload(&m, host_mosaic, nb))) return rc;
    if (host_dark) {
        if ((rc = tmp.upload(&dark, host_dark, nb))) return rc;
        c.flags |= MI_CALIB_DARK;
        c.dev_dark = dark;
    }
    if (host_gain) {
        if ((rc = tmp.upload(&gain, host_gain, npx * sizeof(uint16_t)))) return rc;
        c.flags |= MI_CALIB_FLAT;
        c.dev_gain = gain;
    }
    if ((rc = mi_mosaic_calibrate_device(device, nullptr, m, height, width, dtype, cfa, &c))) return rc;
    return tmp.download(host_out, m, nb);
}

// ---------------------------------------------------------------- site corrections (kernels_sitecorr.hpp)
int mi_mosaic_defects_const_device(int device, void* stream, void* dev_mosaic, int height, int width, int dtype, int constant,
                                   int phase_mask, void* dev_scratch) {
    if (!dev_mosaic) return fail(MI_ERR_INVALID, "null mosaic");
    int rc = calib_shape_check(height, width, dtype);
    if (rc) return rc;
    mi_site_correct_t c{};
    c.flags = MI_SITE_BAD_CONST;
    c.bad_constant = constant;
    c.bad_phase_mask = phase_mask;
    c.dev_scratch = dev_scratch;
    if ((rc = site_check(&c, dtype, true))) return rc;
    MI_HIP(hipSetDevice(device));
    defects_const_launch((hipStream_t)stream, dev_mosaic, height, width, dtype, constant, phase_mask, (unsigned long long*)dev_scratch);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_mosaic_site_correct_device(int device, void* stream, void* dev_mosaic, int height, int width, int dtype, const mi_cfa_t* cfa,
                                  const mi_site_correct_t* sc) {
    if (!dev_mosaic) return fail(MI_ERR_INVALID, "null mosaic");
    int rc = calib_shape_check(height, width, dtype);
    if (rc || (rc = cfa_check(cfa, dtype)) || (rc = site_check(sc, dtype, true))) return rc;
    if (sc->flags == 0) return MI_OK;   // nothing to do, no device call
    MI_HIP(hipSetDevice(device));
    site_kernels((hipStream_t)stream, dev_mosaic, height, width, dtype, *cfa, *sc, (unsigned long long*)sc->dev_scratch);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_mosaic_site_correct(int device, const void* host_mosaic, void* host_out, int height, int width, int dtype, const mi_cfa_t* cfa,
                           const mi_site_correct_t* sc) {
    if (!host_mosaic) return fail(MI_ERR_INVALID, "null mosaic");
    if (!host_out) return fail(MI_ERR_INVALID, "null mosaic output");
    int rc = calib_shape_check(height, width, dtype);
    if (rc || (rc = cfa_check(cfa, dtype)) || (rc = site_check(sc, dtype))) return rc;
    int64_t dmin[4], dmax[4];
    if ((rc = site_host_check(sc, height, width, dmin, dmax)) || (rc = site_black_check(cfa->black, dmin, dmax, dtype))) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nb = (size_t)height * width * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void* m = nullptr;
    mi_site_correct_t d = *sc;
    if ((rc = tmp.upload(&m, host_mosaic, nb))) return rc;
    const auto up = [&tmp](auto& field, const void* src, size_t bytes) {     // a table up, its device pointer into the descriptor
        void* q = nullptr;
        const int r = tmp.upload(&q, src, bytes);
        field = (std::remove_reference_t<decltype(field)>)q;
        return r;
    };
    if ((sc->flags & MI_SITE_DELTA_H) && (rc = up(d.delta_h, sc->delta_h, (size_t)width * sizeof(int16_t)))) return rc;
    if ((sc->flags & MI_SITE_DELTA_V) && (rc = up(d.delta_v, sc->delta_v, (size_t)height * sizeof(int16_t)))) return rc;
    if (sc->flags & MI_SITE_GAIN)
        for (int p = 0; p < 4; ++p) {
            const mi_site_gain_t& g = sc->gain[p];
            if (!g.nodes) continue;
            if ((rc = up(d.gain[p].nodes, g.nodes, (size_t)g.mv * g.mh * sizeof(uint16_t))) ||
                (rc = up(d.gain[p].row_axis, g.row_axis, (size_t)height * sizeof(mi_site_axis_t))) ||
                (rc = up(d.gain[p].col_axis, g.col_axis, (size_t)width * sizeof(mi_site_axis_t))))
                return rc;
        }
    if ((sc->flags & MI_SITE_BAD_LIST) && sc->n_bad > 0 && (rc = up(d.bad_sites, sc->bad_sites, (size_t)sc->n_bad * sizeof(int32_t))))
        return rc;
    if ((sc->flags & MI_SITE_BAD_CONST) && (rc = tmp.alloc(&d.dev_scratch, defects_const_scratch_bytes(height, width)))) return rc;
    if ((rc = mi_mosaic_site_correct_device(device, nullptr, m, height, width, dtype, cfa, &d))) return rc;
    return tmp.download(host_out, m, nb);
}

int mi_stack_set_site_correction(mi_stack_t* s, const mi_site_correct_t* sc) {
    int rc = check_handle(s);
    if (rc) return rc;
    int64_t dmin[4] = {}, dmax[4] = {};
    if (sc) {
        if ((rc = calib_shape_check(s->p.height, s->p.width, s->p.in_dtype)) || (rc = site_check(sc, s->p.in_dtype)) ||
            (rc = site_host_check(sc, s->p.height, s->p.width, dmin, dmax)))
            return rc;
        // (black is the push's own: every level the handle's dtype allows must leave room for the deltas somewhere)
        const int maxv = s->p.in_dtype == MI_U8 ? 255 : 65535;
        for (int p = 0; p < 4; ++p)
            if (dmax[p] - dmin[p] > maxv)
                return fail(MI_ERR_INVALID, "site correction: delta_h + delta_v spans %lld .. %lld at position %d: no black level keeps it inside [0, %d]",
                            (long long)dmin[p], (long long)dmax[p], p, maxv);
    }
    return mosaic_set_site(s, sc, dmin, dmax);
}

// ---------------------------------------------------------------- lens correction (kernels_lens.hpp)
static int lens_check(const void* src, const void* dst, int height, int width, int dtype, const mi_lens_t* lens) {
    if (!src) return fail(MI_ERR_INVALID, "null source frame");
    if (!dst) return fail(MI_ERR_INVALID, "null destination frame");
    if (!lens) return fail(MI_ERR_INVALID, "null lens");
    if (src == dst) return fail(MI_ERR_INVALID, "source and destination must be distinct buffers (the remap is a gather)");
    if (height < 1 || width < 1) return fail(MI_ERR_INVALID, "height and width must be >= 1 (got %dx%d)", width, height);
    // (a side below 2^26: positions in 1/32 pixel fit an int)
    if ((uint64_t)height * (uint64_t)width >= (1ull << 31) || height >= (1 << 26) || width >= (1 << 26))
        return fail(MI_ERR_INVALID, "height x width too large");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16 for a lens remap (got %d)", dtype);
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(lens->k[i])) return fail(MI_ERR_INVALID, "lens k[%d] must be finite", i);
    // (a centre within 2^30 pixels of the origin: cx + (x - cx) is then x to far below 1/64 pixel, which makes an identity plane a copy)
    if (!std::isfinite(lens->cx) || std::fabs(lens->cx) > 1073741824.0) return fail(MI_ERR_INVALID, "lens cx must be finite and at most 2^30 in magnitude");
    if (!std::isfinite(lens->cy) || std::fabs(lens->cy) > 1073741824.0) return fail(MI_ERR_INVALID, "lens cy must be finite and at most 2^30 in magnitude");
    return MI_OK;
}

int mi_lens_remap_device(int device, void* stream, const void* dev_src, void* dev_dst, void* dev_mask, int height, int width,
                         int dtype, const mi_lens_t* lens) {
    int rc = lens_check(dev_src, dev_dst, height, width, dtype, lens);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    lens_launch((hipStream_t)stream, dev_src, dev_dst, dev_mask, height, width, dtype, *lens);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_lens_remap(int device, const void* host_src, void* host_dst, void* host_mask, int height, int width, int dtype,
                  const mi_lens_t* lens) {
    int rc = lens_check(host_src, host_dst, height, width, dtype, lens);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t npx = (size_t)height * width, nb = npx * 3 * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *src = nullptr, *dst = nullptr, *mask = nullptr;
    if ((rc = tmp.upload(&src, host_src, nb)) || (rc = tmp.alloc(&dst, nb)) || (host_mask && (rc = tmp.alloc(&mask, npx))) ||
        (rc = mi_lens_remap_device(device, nullptr, src, dst, mask, height, width, dtype, lens)))
        return rc;
    if (host_mask && (rc = tmp.download(host_mask, mask, npx))) return rc;
    return tmp.download(host_dst, dst, nb);
}

// ---------------------------------------------------------------- finishing a raw frame (kernels_finish.hpp)
// argument checks of mi_mosaic_radial_gain*: no device call, the table is not read
static int radial_check(const void* mosaic, int height, int width, int dtype, const mi_cfa_t* cfa, const mi_radial_gain_t* rg) {
    if (!mosaic) return fail(MI_ERR_INVALID, "null mosaic");
    int rc = calib_shape_check(height, width, dtype);
    if (rc || (rc = cfa_check(cfa, dtype))) return rc;
    if (!rg) return fail(MI_ERR_INVALID, "null radial gain");
    if (!rg->table) return fail(MI_ERR_INVALID, "radial gain: null table");
    const int maxv = dtype == MI_U8 ? 255 : 65535;
    for (int k = 0; k < 4; ++k)
        if (cfa->black[k] > maxv) return fail(MI_ERR_INVALID, "cfa black[%d] must be <= %d (got %d)", k, maxv, cfa->black[k]);
    if (rg->cx2 < -finish::CENTRE_MAX || rg->cx2 > finish::CENTRE_MAX || rg->cy2 < -finish::CENTRE_MAX || rg->cy2 > finish::CENTRE_MAX)
        return fail(MI_ERR_INVALID, "radial gain: the centre (%d, %d) half pixels must be at most 2^24 in magnitude", rg->cx2, rg->cy2);
    const long long D = radial_d2max(height, width, rg->cx2, rg->cy2);
    if (D < 1 || D >= finish::D2_MAX)
        return fail(MI_ERR_INVALID, "radial gain: the farthest corner lies %lld half pixels squared from the centre (1 to 2^40 - 1)", D);
    return MI_OK;
}

int mi_mosaic_radial_gain_device(int device, void* stream, void* dev_mosaic, int height, int width, int dtype, const mi_cfa_t* cfa,
                                 const mi_radial_gain_t* rg) {
    int rc = radial_check(dev_mosaic, height, width, dtype, cfa, rg);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    radial_gain_launch((hipStream_t)stream, dev_mosaic, height, width, dtype, cfa->black, *rg);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_mosaic_radial_gain(int device, const void* host_mosaic, void* host_out, int height, int width, int dtype, const mi_cfa_t* cfa,
                          const mi_radial_gain_t* rg) {
    if (!host_out) return fail(MI_ERR_INVALID, "null mosaic output");
    int rc = radial_check(host_mosaic, height, width, dtype, cfa, rg);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nb = (size_t)height * width * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *m = nullptr, *table = nullptr;
    mi_radial_gain_t d = *rg;
    if ((rc = tmp.upload(&m, host_mosaic, nb)) || (rc = tmp.upload(&table, rg->table, MI_RADIAL_NODES * sizeof(uint16_t)))) return rc;
    d.table = (const uint16_t*)table;
    if ((rc = mi_mosaic_radial_gain_device(device, nullptr, m, height, width, dtype, cfa, &d))) return rc;
    return tmp.download(host_out, m, nb);
}

// argument checks of mi_frame_finish*: no device call
static int finish_check(const void* src, const void* dst, int height, int width, int dtype, int crop_y, int crop_x, int crop_h,
                        int crop_w, int orientation) {
    if (!src) return fail(MI_ERR_INVALID, "null source frame");
    if (!dst) return fail(MI_ERR_INVALID, "null destination frame");
    if (src == dst) return fail(MI_ERR_INVALID, "source and destination must be distinct buffers (the finish is out of place)");
    if (height < 1 || width < 1) return fail(MI_ERR_INVALID, "height and width must be >= 1 (got %dx%d)", width, height);
    // (the kernels count a row's SAMPLES in an int: three per pixel)
    if (3 * (uint64_t)height * (uint64_t)width >= (1ull << 31)) return fail(MI_ERR_INVALID, "height x width too large (3 x height x width must be below 2^31)");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16 for a frame finish (got %d)", dtype);
    if (crop_y < 0 || crop_x < 0 || crop_h < 1 || crop_w < 1 || (int64_t)crop_y + crop_h > height || (int64_t)crop_x + crop_w > width)
        return fail(MI_ERR_INVALID, "the crop (y %d, x %d, %d x %d) must be a rectangle inside the %d x %d frame", crop_y, crop_x, crop_h,
                    crop_w, height, width);
    if (orientation < 1 || orientation > 8) return fail(MI_ERR_INVALID, "orientation must be in [1, 8] (got %d)", orientation);
    return MI_OK;
}

int mi_frame_finish_device(int device, void* stream, const void* dev_src, void* dev_dst, int height, int width, int dtype, int crop_y,
                           int crop_x, int crop_h, int crop_w, int orientation) {
    int rc = finish_check(dev_src, dev_dst, height, width, dtype, crop_y, crop_x, crop_h, crop_w, orientation);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    frame_finish_launch((hipStream_t)stream, dev_src, dev_dst, width, dtype, crop_y, crop_x, crop_h, crop_w, orientation);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_frame_finish(int device, const void* host_src, void* host_dst, int height, int width, int dtype, int crop_y, int crop_x,
                    int crop_h, int crop_w, int orientation) {
    int rc = finish_check(host_src, host_dst, height, width, dtype, crop_y, crop_x, crop_h, crop_w, orientation);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nb = (size_t)height * width * 3 * dtype_size(dtype), ob = (size_t)crop_h * crop_w * 3 * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *src = nullptr, *dst = nullptr;
    if ((rc = tmp.upload(&src, host_src, nb)) || (rc = tmp.alloc(&dst, ob)) ||
        (rc = mi_frame_finish_device(device, nullptr, src, dst, height, width, dtype, crop_y, crop_x, crop_h, crop_w, orientation)))
        return rc;
    return tmp.download(host_dst, dst, ob);
}

int mi_stack_push_mosaic_calibrated(mi_stack_t* s, const void* host_mosaic, size_t row_stride_bytes, const mi_cfa_t* cfa,
                                    const mi_calib_t* calib, const mi_develop_t* develop, const int32_t* dev_sites, int n_sites,
                                    int pinned) {
    int rc = check_handle(s);
    if (rc) return rc;
    return mosaic_entry(s, "mi_stack_push_mosaic_calibrated", host_mosaic, row_stride_bytes, cfa, calib, true, develop, false, dev_sites,
                        n_sites, pinned);
}

// ---------------------------------------------------------------- packed raw samples (kernels_unpack.hpp)
// argument checks of mi_raw_unpack*, mi_stack_push_packed: no device call
static int raw_layout_check(const void* span, size_t span_bytes, const uint32_t* seg_offsets, const mi_raw_layout_t* L,
                            const uint16_t* table, const void* out) {
    if (!span) return fail(MI_ERR_INVALID, "null span");
    if (!seg_offsets) return fail(MI_ERR_INVALID, "null seg_offsets");
    if (!L) return fail(MI_ERR_INVALID, "null layout");
    if (!out) return fail(MI_ERR_INVALID, "null output");
    if (L->bits != 8 && L->bits != 10 && L->bits != 12 && L->bits != 14 && L->bits != 16)
        return fail(MI_ERR_INVALID, "layout bits must be 8, 10, 12, 14 or 16 (got %d)", L->bits);
    if (L->dtype != (L->bits == 8 ? MI_U8 : MI_U16))
        return fail(MI_ERR_INVALID, "layout dtype must be MI_U8 for 8 bits and MI_U16 otherwise (got dtype %d for %d bits)", L->dtype, L->bits);
    if (L->image_height < 1 || L->image_width < 1)
        return fail(MI_ERR_INVALID, "layout image_height and image_width must be >= 1 (got %dx%d)", L->image_width, L->image_height);
    if (L->seg_height < 1 || L->seg_width < 1)
        return fail(MI_ERR_INVALID, "layout seg_height and seg_width must be >= 1 (got %dx%d)", L->seg_width, L->seg_height);
    if (!L->tiled && L->seg_width != L->image_width)
        return fail(MI_ERR_INVALID, "layout seg_width of strips must be image_width (got %d for %d)", L->seg_width, L->image_width);
    if (L->height < 1 || L->width < 1) return fail(MI_ERR_INVALID, "layout height and width must be >= 1 (got %dx%d)", L->width, L->height);
    if (L->crop_y < 0 || L->crop_x < 0 || (int64_t)L->crop_y + L->height > L->image_height || (int64_t)L->crop_x + L->width > L->image_width)
        return fail(MI_ERR_INVALID, "layout crop (%d, %d) + %dx%d lies outside the %dx%d image", L->crop_x, L->crop_y, L->width, L->height,
                    L->image_width, L->image_height);
    if ((uint64_t)L->height * (uint64_t)L->width >= (1ull << 31)) return fail(MI_ERR_INVALID, "layout height x width too large");
    if (span_bytes == 0 || (uint64_t)span_bytes >= (1ull << 32))
        return fail(MI_ERR_INVALID, "span_bytes must be in [1, 2^32) (got %llu)", (unsigned long long)span_bytes);
    if (L->shift < 0 || L->shift > 15) return fail(MI_ERR_INVALID, "layout shift must be in [0, 15] (got %d)", L->shift);
    if (L->table_len < 0 || L->table_len > unpack::MAX_TABLE)
        return fail(MI_ERR_INVALID, "layout table_len must be in [0, %d] (got %d)", unpack::MAX_TABLE, L->table_len);
    if (L->table_len > 0 && !table) return fail(MI_ERR_INVALID, "layout table_len is %d and the table is null", L->table_len);
    if (L->table_len > 0 && L->bits == 8) return fail(MI_ERR_INVALID, "layout table_len must be 0 for 8-bit samples (the table holds uint16)");
    return MI_OK;
}
// offsets in host memory: every segment ends inside the span
static int raw_segments_check(size_t span_bytes, const uint32_t* seg_offsets, const mi_raw_layout_t* L) {
    const int nsx = unpack_nsx(*L), nsy = cdiv(L->image_height, L->seg_height);
    const uint64_t rowb = unpack_row_bytes(*L);
    for (int sy = 0; sy < nsy; ++sy) {
        const int rows = L->tiled ? L->seg_height : std::min(L->seg_height, L->image_height - sy * L->seg_height);
        for (int sx = 0; sx < nsx; ++sx) {
            const uint64_t a = seg_offsets[sy * nsx + sx], e = a + rowb * (uint64_t)rows;
            if (e > span_bytes)
                return fail(MI_ERR_INVALID, "seg_offsets[%d] = %llu: the segment ends at %llu, outside the span of %llu bytes", sy * nsx + sx,
                            (unsigned long long)a, (unsigned long long)e, (unsigned long long)span_bytes);
        }
    }
    return MI_OK;
}

int mi_raw_unpack_device(int device, void* stream, const void* dev_span, size_t span_bytes, const uint32_t* dev_seg_offsets,
                         const mi_raw_layout_t* layout, const uint16_t* dev_table, void* dev_out) {
    int rc = raw_layout_check(dev_span, span_bytes, dev_seg_offsets, layout, dev_table, dev_out);
    if (rc) return rc;
    // (the kernel fetches aligned dwords of the span and 16-byte windows of the output)
    if ((uintptr_t)dev_span & 3) return fail(MI_ERR_INVALID, "dev_span must be 4-byte aligned");
    if ((uintptr_t)dev_out & (dtype_size(layout->dtype) - 1)) return fail(MI_ERR_INVALID, "dev_out must be aligned to its samples");
    MI_HIP(hipSetDevice(device));
    unpack_launch((hipStream_t)stream, dev_span, span_bytes, dev_seg_offsets, *layout, dev_table, dev_out);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_raw_unpack(int device, const void* host_span, size_t span_bytes, const uint32_t* seg_offsets, const mi_raw_layout_t* layout,
                  const uint16_t* host_table, void* host_out) {
    int rc = raw_layout_check(host_span, span_bytes, seg_offsets, layout, host_table, host_out);
    if (rc || (rc = raw_segments_check(span_bytes, seg_offsets, layout))) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nb = (size_t)layout->height * layout->width * dtype_size(layout->dtype);
    DevScratch tmp(nullptr);
    void *span = nullptr, *out = nullptr;
    uint32_t* seg = nullptr;
    uint16_t* table = nullptr;
    if ((rc = tmp.upload(&span, host_span, span_bytes)) || (rc = tmp.upload(&seg, seg_offsets, (size_t)unpack_nsegs(*layout) * sizeof(uint32_t))) ||
        (layout->table_len > 0 && (rc = tmp.upload(&table, host_table, (size_t)layout->table_len * sizeof(uint16_t)))) ||
        (rc = tmp.alloc(&out, nb)) || (rc = mi_raw_unpack_device(device, nullptr, span, span_bytes, seg, layout, table, out)))
        return rc;
    return tmp.download(host_out, out, nb);
}

// descriptors in host memory (mi_raw_ljpeg, mi_stack_push_ljpeg): what the kernel would flag or mis-decode is refused here
// (SEG: mi_ljpeg_seg_t, or mi_ljpeg_seg3_t for the three-component entry points; a template has C++ linkage)
extern "C++" {
template <typename SEG>
static int ljpeg_segs_check(size_t span_bytes, const SEG* segs, const mi_raw_layout_t* L) {
    const int nsx = unpack_nsx(*L), nsy = cdiv(L->image_height, L->seg_height);
    for (int k = 0; k < nsx * nsy; ++k) {
        const SEG& S = segs[k];
        const int rows = L->tiled ? L->seg_height : std::min(L->seg_height, L->image_height - (k / nsx) * L->seg_height);
        if constexpr (std::is_same<SEG, mi_ljpeg_seg3_t>::value) {
            if (S.ncomp != 3) return fail(MI_ERR_INVALID, "segs[%d].ncomp must be 3 (got %d)", k, S.ncomp);
        } else {
            if (S.ncomp != 1 && S.ncomp != 2) return fail(MI_ERR_INVALID, "segs[%d].ncomp must be 1 or 2 (got %d)", k, S.ncomp);
        }
        if (S.predictor < 1 || S.predictor > 7) return fail(MI_ERR_INVALID, "segs[%d].predictor must be in [1, 7] (got %d)", k, S.predictor);
        if (S.precision < 2 || S.precision > L->bits)
            return fail(MI_ERR_INVALID, "segs[%d].precision must be in [2, layout bits = %d] (got %d)", k, L->bits, S.precision);
        if (S.x < 1 || (int64_t)S.x * S.ncomp != L->seg_width || S.y != rows)
            return fail(MI_ERR_INVALID, "segs[%d]: a frame of %d lines of %d x %d samples does not match its segment of %d x %d", k, S.y, S.x,
                        S.ncomp, rows, L->seg_width);
        if (S.predictor != 1 && L->seg_width > ljpeg::MAX_LINE)
            return fail(MI_ERR_INVALID, "segs[%d].predictor %d keeps the line above: layout seg_width must be <= %d for it (got %d)", k,
                        S.predictor, ljpeg::MAX_LINE, L->seg_width);
        for (int c = 0; c < S.ncomp; ++c) {
            uint32_t code = 0, total = 0;
            for (int l = 1; l <= 16; ++l) {
                code += S.counts[c][l - 1];
                total += S.counts[c][l - 1];
                if (code > (1u << l)) return fail(MI_ERR_INVALID, "segs[%d].counts[%d] overflow the code space at length %d", k, c, l);
                code <<= 1;
            }
            if (total < 1 || total > 17) return fail(MI_ERR_INVALID, "segs[%d].counts[%d] must sum to 1 .. 17 (got %u)", k, c, total);
            for (uint32_t i = 0; i < total; ++i)
                if (S.values[c][i] > 16) return fail(MI_ERR_INVALID, "segs[%d].values[%d][%u] must be <= 16 (got %d)", k, c, i, S.values[c][i]);
        }
        const uint64_t e = (uint64_t)S.scan_off + S.scan_bytes;
        if (e > span_bytes)
            return fail(MI_ERR_INVALID, "segs[%d].scan_off = %u: the data ends at %llu, outside the span of %llu bytes", k, S.scan_off,
                        (unsigned long long)e, (unsigned long long)span_bytes);
    }
    return MI_OK;
}
}  // extern "C++"
// raw_layout_check for the lossless-JPEG entry points: the descriptors stand where the offsets do
static int ljpeg_layout_check(const void* span, size_t span_bytes, const mi_ljpeg_seg_t* segs, const mi_raw_layout_t* L, const uint16_t* table,
                              const void* out) {
    if (span && !segs) return fail(MI_ERR_INVALID, "null segs");
    return raw_layout_check(span, span_bytes, (const uint32_t*)segs, L, table, out);
}

int mi_raw_ljpeg_device(int device, void* stream, const void* dev_span, size_t span_bytes, const mi_ljpeg_seg_t* dev_segs,
                        const mi_raw_layout_t* layout, const uint16_t* dev_table, void* dev_out, uint32_t* dev_status) {
    int rc = ljpeg_layout_check(dev_span, span_bytes, dev_segs, layout, dev_table, dev_out);
    if (rc) return rc;
    // (the kernel stages aligned dwords of the span and reads the descriptors as structs)
    if ((uintptr_t)dev_span & 3) return fail(MI_ERR_INVALID, "dev_span must be 4-byte aligned");
    if ((uintptr_t)dev_segs & 15) return fail(MI_ERR_INVALID, "dev_segs must be 16-byte aligned");
    if ((uintptr_t)dev_out & (dtype_size(layout->dtype) - 1)) return fail(MI_ERR_INVALID, "dev_out must be aligned to its samples");
    if ((uintptr_t)dev_status & 3) return fail(MI_ERR_INVALID, "dev_status must be 4-byte aligned");
    MI_HIP(hipSetDevice(device));
    ljpeg_launch((hipStream_t)stream, dev_span, span_bytes, dev_segs, *layout, dev_table, dev_out, dev_status, nullptr);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_raw_ljpeg(int device, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs, const mi_raw_layout_t* layout,
                 const uint16_t* host_table, void* host_out, uint32_t* status_out) {
    int rc = ljpeg_layout_check(host_span, span_bytes, segs, layout, host_table, host_out);
    if (rc || (rc = ljpeg_segs_check(span_bytes, segs, layout))) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nb = (size_t)layout->height * layout->width * dtype_size(layout->dtype);
    const size_t nseg = (size_t)unpack_nsegs(*layout);
    DevScratch tmp(nullptr);
    void *span = nullptr, *out = nullptr;
    mi_ljpeg_seg_t* seg = nullptr;
    uint16_t* table = nullptr;
    uint32_t* status = nullptr;
    if ((rc = tmp.upload(&span, host_span, span_bytes)) || (rc = tmp.upload(&seg, segs, nseg * sizeof(mi_ljpeg_seg_t))) ||
        (layout->table_len > 0 && (rc = tmp.upload(&table, host_table, (size_t)layout->table_len * sizeof(uint16_t)))) ||
        (rc = tmp.alloc(&out, nb)) || (rc = tmp.alloc(&status, nseg * sizeof(uint32_t))) ||
        (rc = mi_raw_ljpeg_device(device, nullptr, span, span_bytes, seg, layout, table, out, status)))
        return rc;
    if (status_out && (rc = tmp.download(status_out, status, nseg * sizeof(uint32_t)))) return rc;
    return tmp.download(host_out, out, nb);
}

// three components (mi_ljpeg_seg3_t): the same checks, the same order
int mi_ljpeg3_batch(void) { return ljpeg::BATCH3; }
int mi_raw_ljpeg3_device(int device, void* stream, const void* dev_span, size_t span_bytes, const mi_ljpeg_seg3_t* dev_segs,
                         const mi_raw_layout_t* layout, const uint16_t* dev_table, void* dev_out, uint32_t* dev_status) {
    if (dev_span && !dev_segs) return fail(MI_ERR_INVALID, "null segs");
    int rc = raw_layout_check(dev_span, span_bytes, (const uint32_t*)dev_segs, layout, dev_table, dev_out);
    if (rc) return rc;
    if ((uintptr_t)dev_span & 3) return fail(MI_ERR_INVALID, "dev_span must be 4-byte aligned");
    if ((uintptr_t)dev_segs & 15) return fail(MI_ERR_INVALID, "dev_segs must be 16-byte aligned");
    if ((uintptr_t)dev_out & (dtype_size(layout->dtype) - 1)) return fail(MI_ERR_INVALID, "dev_out must be aligned to its samples");
    if ((uintptr_t)dev_status & 3) return fail(MI_ERR_INVALID, "dev_status must be 4-byte aligned");
    MI_HIP(hipSetDevice(device));
    ljpeg3_launch((hipStream_t)stream, dev_span, span_bytes, dev_segs, *layout, dev_table, dev_out, dev_status, nullptr);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_raw_ljpeg3(int device, const void* host_span, size_t span_bytes, const mi_ljpeg_seg3_t* segs, const mi_raw_layout_t* layout,
                  const uint16_t* host_table, void* host_out, uint32_t* status_out) {
    if (host_span && !segs) return fail(MI_ERR_INVALID, "null segs");
    int rc = raw_layout_check(host_span, span_bytes, (const uint32_t*)segs, layout, host_table, host_out);
    if (rc || (rc = ljpeg_segs_check(span_bytes, segs, layout))) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nb = (size_t)layout->height * layout->width * dtype_size(layout->dtype);
    const size_t nseg = (size_t)unpack_nsegs(*layout);
    DevScratch tmp(nullptr);
    void *span = nullptr, *out = nullptr;
    mi_ljpeg_seg3_t* seg = nullptr;
    uint16_t* table = nullptr;
    uint32_t* status = nullptr;
    if ((rc = tmp.upload(&span, host_span, span_bytes)) || (rc = tmp.upload(&seg, segs, nseg * sizeof(mi_ljpeg_seg3_t))) ||
        (layout->table_len > 0 && (rc = tmp.upload(&table, host_table, (size_t)layout->table_len * sizeof(uint16_t)))) ||
        (rc = tmp.alloc(&out, nb)) || (rc = tmp.alloc(&status, nseg * sizeof(uint32_t))) ||
        (rc = mi_raw_ljpeg3_device(device, nullptr, span, span_bytes, seg, layout, table, out, status)))
        return rc;
    if (status_out && (rc = tmp.download(status_out, status, nseg * sizeof(uint32_t)))) return rc;
    return tmp.download(host_out, out, nb);
}

// ---- baseline JPEG frames (kernels_jpeg.hpp): the descriptor lies in host memory and is checked here, whole
// (split: the entry points of kernels_jpeg_split.hpp, which take an interval of any length)
static int jpeg_check(const mi_jpeg_t* J, bool split = false) {
    if (!J) return fail(MI_ERR_INVALID, "null jpeg");
    if (J->width < 1 || J->width > 65535 || J->height < 1 || J->height > 65535)
        return fail(MI_ERR_INVALID, "jpeg width and height must be in [1, 65535] (got %d x %d)", J->width, J->height);
    if (J->ncomp != 1 && J->ncomp != 3) return fail(MI_ERR_INVALID, "jpeg ncomp must be 1 or 3 (got %d)", J->ncomp);
    const bool samp = (J->hmax == 1 && J->vmax == 1) || (J->ncomp == 3 && J->hmax == 2 && (J->vmax == 1 || J->vmax == 2));
    if (!samp) return fail(MI_ERR_INVALID, "jpeg hmax, vmax must be (1,1), or (2,1) or (2,2) at ncomp 3 (got (%d,%d))", J->hmax, J->vmax);
    const jpeg::Geom g = jpeg::geom(*J);
    const int max_dri = split ? g.n_mcus : MI_JPEG_MAX_DRI;
    if (J->dri < 1 || J->dri > max_dri) return fail(MI_ERR_INVALID, "jpeg dri must be in [1, %d] (got %d)", max_dri, J->dri);
    const long long want = ((long long)g.n_mcus + J->dri - 1) / J->dri;
    if (J->n_intervals != want)
        return fail(MI_ERR_INVALID, "jpeg n_intervals must be ceil(%d MCUs / dri %d) = %lld (got %d)", g.n_mcus, J->dri, want, J->n_intervals);
    bool used[4] = {false, false, false, false};
    for (int c = 0; c < J->ncomp; ++c) {
        if (J->tq[c] > 3) return fail(MI_ERR_INVALID, "jpeg tq[%d] must be in [0, 3] (got %d)", c, J->tq[c]);
        if (J->td[c] > 1) return fail(MI_ERR_INVALID, "jpeg td[%d] must be 0 or 1 (got %d)", c, J->td[c]);
        if (J->ta[c] > 1) return fail(MI_ERR_INVALID, "jpeg ta[%d] must be 0 or 1 (got %d)", c, J->ta[c]);
        used[J->td[c]] = used[2 + J->ta[c]] = true;
        for (int k = 0; k < 64; ++k)
            if (J->quant[J->tq[c]][k] < 1) return fail(MI_ERR_INVALID, "jpeg quant[%d][%d] must be >= 1", J->tq[c], k);
    }
    for (int t = 0; t < 4; ++t) {
        uint32_t code = 0, total = 0;
        for (int l = 1; l <= 16; ++l) {
            code += J->counts[t][l - 1];
            total += J->counts[t][l - 1];
            if (code > (1u << l)) return fail(MI_ERR_INVALID, "jpeg counts[%d] overflow the code space at length %d", t, l);
            code <<= 1;
        }
        if (total > 256 || (used[t] && total < 1))
            return fail(MI_ERR_INVALID, "jpeg counts[%d] must sum to %d .. 256 (got %u)", t, used[t] ? 1 : 0, total);
        if (t < 2)
            for (uint32_t k = 0; k < total; ++k)
                if (J->values[t][k] > 15) return fail(MI_ERR_INVALID, "jpeg values[%d][%u] must be <= 15 in a DC table (got %d)", t, k, J->values[t][k]);
    }
    return MI_OK;
}
static int jpeg_args_check(const void* span, size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t* J, const void* out,
                           bool split = false) {
    if (!span) return fail(MI_ERR_INVALID, "null span");
    if (!offsets) return fail(MI_ERR_INVALID, "null offsets");
    int rc = jpeg_check(J, split);
    if (rc) return rc;
    if (!out) return fail(MI_ERR_INVALID, "null output");
    if (span_bytes < 1 || span_bytes >= (1ull << 32))
        return fail(MI_ERR_INVALID, "span_bytes must be in [1, 2^32) (got %llu)", (unsigned long long)span_bytes);
    return MI_OK;
}
static int jpeg_offsets_check(size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t* J) {
    for (int i = 0; i <= J->n_intervals; ++i) {
        if (offsets[i] > span_bytes)
            return fail(MI_ERR_INVALID, "offsets[%d] = %u lies outside the span of %llu bytes", i, offsets[i], (unsigned long long)span_bytes);
        if (i && offsets[i] < offsets[i - 1]) return fail(MI_ERR_INVALID, "offsets[%d] = %u lies in front of offsets[%d] = %u", i, offsets[i], i - 1, offsets[i - 1]);
    }
    return MI_OK;
}

int mi_jpeg_coef_count(const mi_jpeg_t* jpeg, size_t* count) {
    int rc = jpeg_check(jpeg);
    if (rc) return rc;
    if (!count) return fail(MI_ERR_INVALID, "null count");
    *count = jpeg::geom(*jpeg).nblocks * 64;
    return MI_OK;
}
// the coefficients (int16), then the sample planes (uint8)
int mi_jpeg_scratch_bytes(const mi_jpeg_t* jpeg, size_t* bytes) {
    int rc = jpeg_check(jpeg);
    if (rc) return rc;
    if (!bytes) return fail(MI_ERR_INVALID, "null bytes");
    *bytes = jpeg::geom(*jpeg).nblocks * 192;
    return MI_OK;
}

int mi_jpeg_coefficients_device(int device, void* stream, const void* dev_span, size_t span_bytes, const uint32_t* dev_offsets,
                                const mi_jpeg_t* jpeg, int16_t* dev_coef, uint32_t* dev_status) {
    int rc = jpeg_args_check(dev_span, span_bytes, dev_offsets, jpeg, dev_coef);
    if (rc) return rc;
    if ((uintptr_t)dev_span & 3) return fail(MI_ERR_INVALID, "dev_span must be 4-byte aligned");
    if ((uintptr_t)dev_offsets & 3) return fail(MI_ERR_INVALID, "dev_offsets must be 4-byte aligned");
    if ((uintptr_t)dev_coef & 15) return fail(MI_ERR_INVALID, "dev_coef must be 16-byte aligned");
    if ((uintptr_t)dev_status & 3) return fail(MI_ERR_INVALID, "dev_status must be 4-byte aligned");
    MI_HIP(hipSetDevice(device));
    jpeg_entropy_launch((hipStream_t)stream, dev_span, span_bytes, dev_offsets, *jpeg, dev_coef, dev_status);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_jpeg_decode_device(int device, void* stream, const void* dev_span, size_t span_bytes, const uint32_t* dev_offsets,
                          const mi_jpeg_t* jpeg, void* dev_scratch, size_t scratch_bytes, uint8_t* dev_out, uint32_t* dev_status) {
    int rc = jpeg_args_check(dev_span, span_bytes, dev_offsets, jpeg, dev_out);
    if (rc) return rc;
    if (!dev_scratch) return fail(MI_ERR_INVALID, "null scratch");
    const size_t nblocks = jpeg::geom(*jpeg).nblocks;
    if (scratch_bytes < nblocks * 192)
        return fail(MI_ERR_INVALID, "scratch_bytes must be >= %llu (got %llu)", (unsigned long long)(nblocks * 192), (unsigned long long)scratch_bytes);
    if ((uintptr_t)dev_scratch & 255) return fail(MI_ERR_INVALID, "dev_scratch must be 256-byte aligned");
    int16_t* coef = (int16_t*)dev_scratch;
    if ((rc = mi_jpeg_coefficients_device(device, stream, dev_span, span_bytes, dev_offsets, jpeg, coef, dev_status))) return rc;
    jpeg_render_launch((hipStream_t)stream, *jpeg, coef, (uint8_t*)dev_scratch + nblocks * 128, dev_out);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_jpeg_coefficients(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t* jpeg,
                         int16_t* host_coef, uint32_t* status_out) {
    int rc = jpeg_args_check(host_span, span_bytes, offsets, jpeg, host_coef);
    if (rc || (rc = jpeg_offsets_check(span_bytes, offsets, jpeg))) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nb = jpeg::geom(*jpeg).nblocks * 128, ns = (size_t)jpeg->n_intervals * sizeof(uint32_t);
    DevScratch tmp(nullptr);
    void* span = nullptr;
    uint32_t *off = nullptr, *status = nullptr;
    int16_t* coef = nullptr;
    if ((rc = tmp.upload(&span, host_span, span_bytes)) || (rc = tmp.upload(&off, offsets, ns + sizeof(uint32_t))) ||
        (rc = tmp.alloc(&coef, nb)) || (rc = tmp.alloc(&status, ns)) ||
        (rc = mi_jpeg_coefficients_device(device, nullptr, span, span_bytes, off, jpeg, coef, status)))
        return rc;
    if (status_out && (rc = tmp.download(status_out, status, ns))) return rc;
    return tmp.download(host_coef, coef, nb);
}

int mi_jpeg_decode(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t* jpeg,
                   uint8_t* host_out, uint32_t* status_out) {
    int rc = jpeg_args_check(host_span, span_bytes, offsets, jpeg, host_out);
    if (rc || (rc = jpeg_offsets_check(span_bytes, offsets, jpeg))) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nscratch = jpeg::geom(*jpeg).nblocks * 192, ns = (size_t)jpeg->n_intervals * sizeof(uint32_t);
    const size_t nb = (size_t)jpeg->height * jpeg->width * 3;
    DevScratch tmp(nullptr);
    void *span = nullptr, *scratch = nullptr;
    uint32_t *off = nullptr, *status = nullptr;
    uint8_t* out = nullptr;
    if ((rc = tmp.upload(&span, host_span, span_bytes)) || (rc = tmp.upload(&off, offsets, ns + sizeof(uint32_t))) ||
        (rc = tmp.alloc(&scratch, nscratch)) || (rc = tmp.alloc(&out, nb)) || (rc = tmp.alloc(&status, ns)) ||
        (rc = mi_jpeg_decode_device(device, nullptr, span, span_bytes, off, jpeg, scratch, nscratch, out, status)))
        return rc;
    if (status_out && (rc = tmp.download(status_out, status, ns))) return rc;
    return tmp.download(host_out, out, nb);
}

// ---- the split entropy decoder (kernels_jpeg_split.hpp): the same checks, an interval of any length
static int jpeg_split_opt(const mi_jpeg_split_t* opt, uint32_t* sub, uint32_t* rounds) {
    *sub = opt && opt->sub_bytes ? opt->sub_bytes : split::SUB_DEFAULT;
    *rounds = opt && opt->max_rounds ? opt->max_rounds : split::ROUNDS_DEFAULT;
    if (*sub != 8 && *sub != 16 && *sub != 32 && *sub != 64 && *sub != 128)
        return fail(MI_ERR_INVALID, "split sub_bytes must be 0, 8, 16, 32, 64 or 128 (got %u)", *sub);
    return MI_OK;
}
static size_t jpeg_split_bytes(const mi_jpeg_t* J, size_t span_bytes, uint32_t sub, uint32_t rounds) {
    const size_t nblocks = jpeg::geom(*J).nblocks;
    return nblocks * 192 + jpeg::split_layout(span_bytes, sub, rounds, *J, nblocks).words * sizeof(uint32_t);
}

int mi_jpeg_split_scratch_bytes(const mi_jpeg_t* jpeg, size_t span_bytes, const mi_jpeg_split_t* opt, size_t* bytes) {
    int rc = jpeg_check(jpeg, true);
    if (rc) return rc;
    if (span_bytes < 1 || span_bytes >= (1ull << 32))
        return fail(MI_ERR_INVALID, "span_bytes must be in [1, 2^32) (got %llu)", (unsigned long long)span_bytes);
    uint32_t sub, rounds;
    if ((rc = jpeg_split_opt(opt, &sub, &rounds))) return rc;
    if (!bytes) return fail(MI_ERR_INVALID, "null bytes");
    *bytes = jpeg_split_bytes(jpeg, span_bytes, sub, rounds);
    return MI_OK;
}

// the checks of both device forms; `out`: the coefficients or the frame
static int jpeg_split_device_check(const void* dev_span, size_t span_bytes, const uint32_t* dev_offsets, const mi_jpeg_t* jpeg,
                                   const mi_jpeg_split_t* opt, const void* dev_scratch, size_t scratch_bytes, const void* out,
                                   const uint32_t* dev_status, uint32_t* sub, uint32_t* rounds) {
    int rc = jpeg_args_check(dev_span, span_bytes, dev_offsets, jpeg, out, true);
    if (rc || (rc = jpeg_split_opt(opt, sub, rounds))) return rc;
    if (!dev_scratch) return fail(MI_ERR_INVALID, "null scratch");
    const size_t need = jpeg_split_bytes(jpeg, span_bytes, *sub, *rounds);
    if (scratch_bytes < need)
        return fail(MI_ERR_INVALID, "scratch_bytes must be >= %llu (got %llu)", (unsigned long long)need, (unsigned long long)scratch_bytes);
    if ((uintptr_t)dev_scratch & 255) return fail(MI_ERR_INVALID, "dev_scratch must be 256-byte aligned");
    if ((uintptr_t)dev_span & 3) return fail(MI_ERR_INVALID, "dev_span must be 4-byte aligned");
    if ((uintptr_t)dev_offsets & 3) return fail(MI_ERR_INVALID, "dev_offsets must be 4-byte aligned");
    if ((uintptr_t)dev_status & 3) return fail(MI_ERR_INVALID, "dev_status must be 4-byte aligned");
    return MI_OK;
}

int mi_jpeg_split_coefficients_device(int device, void* stream, const void* dev_span, size_t span_bytes, const uint32_t* dev_offsets,
                                      const mi_jpeg_t* jpeg, const mi_jpeg_split_t* opt, void* dev_scratch, size_t scratch_bytes,
                                      int16_t* dev_coef, uint32_t* dev_status) {
    uint32_t sub, rounds;
    int rc = jpeg_split_device_check(dev_span, span_bytes, dev_offsets, jpeg, opt, dev_scratch, scratch_bytes, dev_coef, dev_status, &sub, &rounds);
    if (rc) return rc;
    if ((uintptr_t)dev_coef & 15) return fail(MI_ERR_INVALID, "dev_coef must be 16-byte aligned");
    MI_HIP(hipSetDevice(device));
    uint32_t* words = (uint32_t*)((uint8_t*)dev_scratch + jpeg::geom(*jpeg).nblocks * 192);
    jpeg_split_launch((hipStream_t)stream, dev_span, span_bytes, dev_offsets, *jpeg, sub, rounds, words, dev_coef, dev_status);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_jpeg_split_decode_device(int device, void* stream, const void* dev_span, size_t span_bytes, const uint32_t* dev_offsets,
                                const mi_jpeg_t* jpeg, const mi_jpeg_split_t* opt, void* dev_scratch, size_t scratch_bytes,
                                uint8_t* dev_out, uint32_t* dev_status) {
    uint32_t sub, rounds;
    int rc = jpeg_split_device_check(dev_span, span_bytes, dev_offsets, jpeg, opt, dev_scratch, scratch_bytes, dev_out, dev_status, &sub, &rounds);
    if (rc) return rc;
    int16_t* coef = (int16_t*)dev_scratch;
    if ((rc = mi_jpeg_split_coefficients_device(device, stream, dev_span, span_bytes, dev_offsets, jpeg, opt, dev_scratch, scratch_bytes, coef,
                                                dev_status)))
        return rc;
    jpeg_render_launch((hipStream_t)stream, *jpeg, coef, (uint8_t*)dev_scratch + jpeg::geom(*jpeg).nblocks * 128, dev_out);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

// both host forms: upload, run, look at the status words, run once more with every round where they say the rounds were too
// few, download
static int jpeg_split_host(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t* jpeg,
                           const mi_jpeg_split_t* opt, int16_t* host_coef, uint8_t* host_out, uint32_t* status_out) {
    int rc = jpeg_args_check(host_span, span_bytes, offsets, jpeg, host_coef ? (const void*)host_coef : (const void*)host_out, true);
    uint32_t sub, rounds;
    if (rc || (rc = jpeg_split_opt(opt, &sub, &rounds)) || (rc = jpeg_offsets_check(span_bytes, offsets, jpeg))) return rc;
    if ((rc = open_device(device))) return rc;
    const mi_jpeg_split_t full{sub, 0xffffffffu};
    const size_t nblocks = jpeg::geom(*jpeg).nblocks, ns = (size_t)jpeg->n_intervals * sizeof(uint32_t);
    const size_t nscratch = jpeg_split_bytes(jpeg, span_bytes, sub, full.max_rounds), nb = (size_t)jpeg->height * jpeg->width * 3;
    DevScratch tmp(nullptr);
    void *span = nullptr, *scratch = nullptr;
    uint32_t *off = nullptr, *status = nullptr;
    uint8_t* out = nullptr;
    if ((rc = tmp.upload(&span, host_span, span_bytes)) || (rc = tmp.upload(&off, offsets, ns + sizeof(uint32_t))) ||
        (rc = tmp.alloc(&scratch, nscratch)) || (rc = tmp.alloc(&status, ns)) || (host_out && (rc = tmp.alloc(&out, nb))))
        return rc;
    std::vector<uint32_t> words((size_t)jpeg->n_intervals);
    const mi_jpeg_split_t first{sub, rounds};
    for (int attempt = 0; attempt < 2; ++attempt) {
        const mi_jpeg_split_t* o = attempt ? &full : &first;
        rc = host_out ? mi_jpeg_split_decode_device(device, nullptr, span, span_bytes, off, jpeg, o, scratch, nscratch, out, status)
                      : mi_jpeg_split_coefficients_device(device, nullptr, span, span_bytes, off, jpeg, o, scratch, nscratch, (int16_t*)scratch, status);
        if (rc || (rc = tmp.download(words.data(), status, ns))) return rc;
        bool unsynced = false;
        for (uint32_t w : words) unsynced = unsynced || (w & MI_JPEG_UNSYNCED);
        if (!unsynced) break;
    }
    if (status_out) memcpy(status_out, words.data(), ns);
    return host_out ? tmp.download(host_out, out, nb) : tmp.download(host_coef, scratch, nblocks * 128);
}

int mi_jpeg_split_coefficients(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t* jpeg,
                               const mi_jpeg_split_t* opt, int16_t* host_coef, uint32_t* status_out) {
    return jpeg_split_host(device, host_span, span_bytes, offsets, jpeg, opt, host_coef, nullptr, status_out);
}

int mi_jpeg_split_decode(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t* jpeg,
                         const mi_jpeg_split_t* opt, uint8_t* host_out, uint32_t* status_out) {
    return jpeg_split_host(device, host_span, span_bytes, offsets, jpeg, opt, nullptr, host_out, status_out);
}

// ---- the split path of the lossless-JPEG decoder (kernels_ljpeg_split.hpp): mi_raw_ljpeg's checks, and mi_jpeg_split_*'s for
// `opt` and the scratch
static int ljpeg_split_size_check(const mi_raw_layout_t* L) {
    if ((uint64_t)unpack_nsegs(*L) * (uint64_t)L->seg_height * (uint64_t)L->seg_width >= (1ull << 32))
        return fail(MI_ERR_INVALID, "layout segments x seg_height x seg_width must be below 2^32 for the split path");
    return MI_OK;
}
static size_t ljpeg_split_bytes(const mi_raw_layout_t* L, size_t span_bytes, uint32_t sub, uint32_t rounds) {
    return ljpeg::split_layout(*L, span_bytes, sub, rounds).words * sizeof(uint32_t);
}

int mi_ljpeg_split_scratch_bytes(const mi_raw_layout_t* layout, size_t span_bytes, const mi_jpeg_split_t* opt, size_t* bytes) {
    static const uint16_t some = 0;     // (the layout's own checks: what stands for the buffers is not looked at)
    int rc = raw_layout_check(&some, span_bytes, (const uint32_t*)&some, layout, &some, &some);
    uint32_t sub, rounds;
    if (rc || (rc = ljpeg_split_size_check(layout)) || (rc = jpeg_split_opt(opt, &sub, &rounds))) return rc;
    if (!bytes) return fail(MI_ERR_INVALID, "null bytes");
    *bytes = ljpeg_split_bytes(layout, span_bytes, sub, rounds);
    return MI_OK;
}

// the checks of both device forms; `out`: the mosaic or the difference plane
static int ljpeg_split_device_check(const void* dev_span, size_t span_bytes, const mi_ljpeg_seg_t* dev_segs, const mi_raw_layout_t* layout,
                                    const uint16_t* dev_table, const mi_jpeg_split_t* opt, const void* dev_scratch, size_t scratch_bytes,
                                    const void* out, const uint32_t* dev_status, uint32_t* sub, uint32_t* rounds) {
    int rc = ljpeg_layout_check(dev_span, span_bytes, dev_segs, layout, dev_table, out);
    if (rc || (rc = ljpeg_split_size_check(layout)) || (rc = jpeg_split_opt(opt, sub, rounds))) return rc;
    if (!dev_scratch) return fail(MI_ERR_INVALID, "null scratch");
    const size_t need = ljpeg_split_bytes(layout, span_bytes, *sub, *rounds);
    if (scratch_bytes < need)
        return fail(MI_ERR_INVALID, "scratch_bytes must be >= %llu (got %llu)", (unsigned long long)need, (unsigned long long)scratch_bytes);
    if ((uintptr_t)dev_scratch & 255) return fail(MI_ERR_INVALID, "dev_scratch must be 256-byte aligned");
    if ((uintptr_t)dev_span & 3) return fail(MI_ERR_INVALID, "dev_span must be 4-byte aligned");
    if ((uintptr_t)dev_segs & 15) return fail(MI_ERR_INVALID, "dev_segs must be 16-byte aligned");
    if ((uintptr_t)dev_status & 3) return fail(MI_ERR_INVALID, "dev_status must be 4-byte aligned");
    return MI_OK;
}

// both device forms behind their checks; `rounds` as given (0: round 0 alone)
static int ljpeg_split_run(int device, void* stream, const void* dev_span, size_t span_bytes, const mi_ljpeg_seg_t* dev_segs,
                           const mi_raw_layout_t* layout, const uint16_t* dev_table, uint32_t sub, uint32_t rounds, void* dev_scratch,
                           void* dev_out, uint16_t* dev_plane, uint32_t* dev_status) {
    MI_HIP(hipSetDevice(device));
    ljpeg_split_launch((hipStream_t)stream, dev_span, span_bytes, dev_segs, *layout, dev_table, sub, rounds, (uint32_t*)dev_scratch, dev_out,
                       dev_plane, dev_status, nullptr);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_raw_ljpeg_split_device(int device, void* stream, const void* dev_span, size_t span_bytes, const mi_ljpeg_seg_t* dev_segs,
                              const mi_raw_layout_t* layout, const uint16_t* dev_table, const mi_jpeg_split_t* opt, void* dev_scratch,
                              size_t scratch_bytes, void* dev_out, uint32_t* dev_status) {
    uint32_t sub, rounds;
    int rc = ljpeg_split_device_check(dev_span, span_bytes, dev_segs, layout, dev_table, opt, dev_scratch, scratch_bytes, dev_out, dev_status,
                                      &sub, &rounds);
    if (rc) return rc;
    if ((uintptr_t)dev_out & (dtype_size(layout->dtype) - 1)) return fail(MI_ERR_INVALID, "dev_out must be aligned to its samples");
    return ljpeg_split_run(device, stream, dev_span, span_bytes, dev_segs, layout, dev_table, sub, rounds, dev_scratch, dev_out, nullptr, dev_status);
}

int mi_ljpeg_split_differences_device(int device, void* stream, const void* dev_span, size_t span_bytes, const mi_ljpeg_seg_t* dev_segs,
                                      const mi_raw_layout_t* layout, const mi_jpeg_split_t* opt, void* dev_scratch, size_t scratch_bytes,
                                      uint16_t* dev_plane, uint32_t* dev_status) {
    static const uint16_t no_table = 0;     // (the table is not applied to differences; the layout may name one)
    uint32_t sub, rounds;
    int rc = ljpeg_split_device_check(dev_span, span_bytes, dev_segs, layout, &no_table, opt, dev_scratch, scratch_bytes, dev_plane, dev_status,
                                      &sub, &rounds);
    if (rc) return rc;
    if ((uintptr_t)dev_plane & 1) return fail(MI_ERR_INVALID, "dev_plane must be 2-byte aligned");
    return ljpeg_split_run(device, stream, dev_span, span_bytes, dev_segs, layout, nullptr, sub, rounds, dev_scratch, nullptr, dev_plane, dev_status);
}

// both host forms: upload, run, look at the status words, run once more with the exact bound where they say the rounds were
// too few, download.  max_rounds 0: the exact bound at once.
static int ljpeg_split_host(int device, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs, const mi_raw_layout_t* layout,
                            const uint16_t* host_table, const mi_jpeg_split_t* opt, void* host_out, uint16_t* host_plane, uint32_t* status_out) {
    static const uint16_t no_table = 0;
    int rc = ljpeg_layout_check(host_span, span_bytes, segs, layout, host_out ? host_table : &no_table,
                                host_out ? (const void*)host_out : (const void*)host_plane);
    uint32_t sub, rounds;
    if (rc || (rc = ljpeg_split_size_check(layout)) || (rc = jpeg_split_opt(opt, &sub, &rounds)) ||
        (rc = ljpeg_segs_check(span_bytes, segs, layout)))
        return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nb = (size_t)layout->height * layout->width * dtype_size(layout->dtype);
    const size_t nseg = (size_t)unpack_nsegs(*layout), ns = nseg * sizeof(uint32_t);
    const size_t np = nseg * (size_t)layout->seg_height * layout->seg_width * sizeof(uint16_t);
    const uint32_t exact = ljpeg::split_exact_rounds(segs, nseg, span_bytes, sub);
    const uint32_t first = opt && opt->max_rounds ? opt->max_rounds : exact;
    const size_t nscratch = ljpeg_split_bytes(layout, span_bytes, sub, 0xffffffffu);
    DevScratch tmp(nullptr);
    void *span = nullptr, *out = nullptr, *scratch = nullptr;
    mi_ljpeg_seg_t* seg = nullptr;
    uint16_t *table = nullptr, *plane = nullptr;
    uint32_t* status = nullptr;
    if ((rc = tmp.upload(&span, host_span, span_bytes)) || (rc = tmp.upload(&seg, segs, nseg * sizeof(mi_ljpeg_seg_t))) ||
        (host_out && layout->table_len > 0 && (rc = tmp.upload(&table, host_table, (size_t)layout->table_len * sizeof(uint16_t)))) ||
        (host_out && (rc = tmp.alloc(&out, nb))) || (host_plane && (rc = tmp.alloc(&plane, np))) || (rc = tmp.alloc(&scratch, nscratch)) ||
        (rc = tmp.alloc(&status, ns)))
        return rc;
    std::vector<uint32_t> words(nseg);
    for (int attempt = 0; attempt < 2; ++attempt) {
        if ((rc = ljpeg_split_run(device, nullptr, span, span_bytes, seg, layout, table, sub, attempt ? exact : first, scratch, out, plane, status)) ||
            (rc = tmp.download(words.data(), status, ns)))
            return rc;
        bool unsynced = false;
        for (uint32_t w : words) unsynced = unsynced || (w & MI_LJPEG_UNSYNCED);
        if (!unsynced) break;
    }
    if (status_out) memcpy(status_out, words.data(), ns);
    return host_out ? tmp.download(host_out, out, nb) : tmp.download(host_plane, plane, np);
}

int mi_raw_ljpeg_split(int device, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs, const mi_raw_layout_t* layout,
                       const uint16_t* host_table, const mi_jpeg_split_t* opt, void* host_out, uint32_t* status_out) {
    return ljpeg_split_host(device, host_span, span_bytes, segs, layout, host_table, opt, host_out, nullptr, status_out);
}

int mi_ljpeg_split_differences(int device, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs, const mi_raw_layout_t* layout,
                               const mi_jpeg_split_t* opt, uint16_t* host_plane, uint32_t* status_out) {
    return ljpeg_split_host(device, host_span, span_bytes, segs, layout, nullptr, opt, nullptr, host_plane, status_out);
}

int mi_stack_set_ljpeg_split(mi_stack_t* s, const mi_jpeg_split_t* opt) {
    int rc = check_handle(s);
    if (rc) return rc;
    uint32_t sub = 0, rounds = 0;
    if (opt && (rc = jpeg_split_opt(opt, &sub, &rounds))) return rc;
    return mosaic_set_ljpeg_split(s, opt != nullptr, sub);
}

// the part of mi_stack_push_packed and mi_stack_push_ljpeg behind the span's checks
static int packed_push(mi_stack_t* s, const void* host_span, size_t span_bytes, const uint32_t* seg_offsets, const mi_ljpeg_seg_t* segs,
                       const mi_raw_layout_t* layout, const uint16_t* host_table, const mi_cfa_t* cfa, const mi_calib_t* calib,
                       const mi_develop_t* develop, const int32_t* dev_sites, int n_sites, int pinned) {
    int rc;
    bool async;
    if (s->p.height < 2 || s->p.width < 2) return fail(MI_ERR_INVALID, "height and width must be >= 2 for a mosaic");
    if (layout->height != s->p.height || layout->width != s->p.width || layout->dtype != s->p.in_dtype)
        return fail(MI_ERR_INVALID, "layout height, width and dtype must be the handle's (got %dx%d dtype %d for %dx%d dtype %d)", layout->width,
                    layout->height, layout->dtype, s->p.width, s->p.height, s->p.in_dtype);
    if ((rc = raw_args_check(s, cfa, calib, false, develop, false, true, dev_sites, n_sites)) || (rc = raw_state_check(s, &async))) return rc;
    if (pinned && async && (rc = pinned_probe(host_span, segs ? "mi_stack_push_ljpeg" : "mi_stack_push_packed", "span"))) return rc;
    const PackedSrc pk{host_span, span_bytes, seg_offsets, segs, unpack_nsegs(*layout), layout, host_table};
    return mosaic_push(s, MosaicFrame{nullptr, 0, &pk, cfa, pinned && async, calib, develop, dev_sites, n_sites});
}

int mi_stack_push_packed(mi_stack_t* s, const void* host_span, size_t span_bytes, const uint32_t* seg_offsets,
                         const mi_raw_layout_t* layout, const uint16_t* host_table, const mi_cfa_t* cfa, const mi_calib_t* calib,
                         const mi_develop_t* develop, const int32_t* dev_sites, int n_sites, int pinned) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = raw_layout_check(host_span, span_bytes, seg_offsets, layout, host_table, s)) ||
        (rc = raw_segments_check(span_bytes, seg_offsets, layout)))
        return rc;
    return packed_push(s, host_span, span_bytes, seg_offsets, nullptr, layout, host_table, cfa, calib, develop, dev_sites, n_sites, pinned);
}

int mi_stack_push_ljpeg(mi_stack_t* s, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs, const mi_raw_layout_t* layout,
                        const uint16_t* host_table, const mi_cfa_t* cfa, const mi_calib_t* calib, const mi_develop_t* develop,
                        const int32_t* dev_sites, int n_sites, int pinned) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = ljpeg_layout_check(host_span, span_bytes, segs, layout, host_table, s)) || (rc = ljpeg_segs_check(span_bytes, segs, layout)))
        return rc;
    return packed_push(s, host_span, span_bytes, nullptr, segs, layout, host_table, cfa, calib, develop, dev_sites, n_sites, pinned);
}

// A linear frame through the one ingest path: the span goes up as a packed or compressed span does, raw_unpack / raw_ljpeg /
// raw_ljpeg3 fill a linear slot of height x width x spp samples and linear_develop takes it to the batch's BGR frame.
int mi_stack_push_linear(mi_stack_t* s, const void* host_span, size_t span_bytes, const void* segs, int compressed,
                         const mi_raw_layout_t* layout, const uint16_t* host_table, const mi_linear_t* linear, const mi_develop_t* develop,
                         int pinned) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (host_span && !segs) return fail(MI_ERR_INVALID, compressed ? "null segs" : "null seg_offsets");
    if ((rc = raw_layout_check(host_span, span_bytes, (const uint32_t*)segs, layout, host_table, s)) ||
        (rc = linear_levels_check(linear, s->p.in_dtype)))
        return rc;
    const bool three = compressed && linear->spp == 3;
    if (!compressed) rc = raw_segments_check(span_bytes, (const uint32_t*)segs, layout);
    else if (three) rc = ljpeg_segs_check(span_bytes, (const mi_ljpeg_seg3_t*)segs, layout);
    else rc = ljpeg_segs_check(span_bytes, (const mi_ljpeg_seg_t*)segs, layout);
    if (rc || (develop && (rc = develop_check(develop)))) return rc;
    if (layout->height != s->p.height || (int64_t)layout->width != (int64_t)s->p.width * linear->spp || layout->dtype != s->p.in_dtype)
        return fail(MI_ERR_INVALID, "layout height, width / spp and dtype must be the handle's (got %dx%d samples at spp %d, dtype %d for %dx%d dtype %d)",
                    layout->width, layout->height, linear->spp, layout->dtype, s->p.width, s->p.height, s->p.in_dtype);
    bool async;
    if ((rc = raw_state_check(s, &async))) return rc;
    if (pinned && async && (rc = pinned_probe(host_span, "mi_stack_push_linear", "span"))) return rc;
    PackedSrc pk{host_span, span_bytes, compressed ? nullptr : (const uint32_t*)segs,
                 compressed && !three ? (const mi_ljpeg_seg_t*)segs : nullptr, unpack_nsegs(*layout), layout, host_table};
    if (three) pk.ljseg3 = (const mi_ljpeg_seg3_t*)segs;
    MosaicFrame f{nullptr, 0, &pk, nullptr, pinned && async, nullptr, develop, nullptr, 0};
    f.lin = linear;
    return mosaic_push(s, f);
}

int mi_stack_ljpeg_status(mi_stack_t* s, uint32_t* flags) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!flags) return fail(MI_ERR_INVALID, "null flags");
    *flags = 0;
    MosaicStage* m = mstage(s);
    if (!m || !m->ljstatus) return MI_OK;
    MI_HIP(hipSetDevice(s->p.device));
    if ((rc = mosaic_sync(s))) return rc;
    MI_HIP(hipStreamSynchronize(s->stream));   // (the decode kernels run on the handle's stream behind their uploads)
    MI_HIP(hipMemcpy(flags, m->ljstatus, sizeof(uint32_t), hipMemcpyDeviceToHost));
    MI_HIP(hipMemsetAsync(m->ljstatus, 0, sizeof(uint32_t), s->stream));   // (in order with the next frame's decode kernel)
    return MI_OK;
}

int mi_host_alloc(void** ptr, size_t bytes) {
    if (!ptr || !bytes) return fail(MI_ERR_INVALID, "bad argument");
    MI_HIP(hipHostMalloc(ptr, bytes, hipHostMallocPortable));
    return MI_OK;
}

int mi_host_free(void* ptr) {
    if (ptr) MI_HIP(hipHostFree(ptr));
    return MI_OK;
}

int mi_host_register(void* ptr, size_t bytes) {
    if (!ptr || !bytes) return fail(MI_ERR_INVALID, "bad argument");
    MI_HIP(hipHostRegister(ptr, bytes, hipHostRegisterPortable));
    return MI_OK;
}

int mi_host_unregister(void* ptr) {
    if (ptr) MI_HIP(hipHostUnregister(ptr));
    return MI_OK;
}

int mi_stack_sync(mi_stack_t* s) {
    int rc = check_handle(s);
    if (rc) return rc;
    MI_HIP(hipSetDevice(s->p.device));
    rc = tiled_sync_all(s);
    if (rc) return rc;
    if ((rc = mosaic_sync(s))) return rc;
    MI_HIP(hipStreamSynchronize(s->stream));
    return MI_OK;
}

int mi_stack_sync_level(mi_stack_t* s, int level) {
    int rc = check_handle(s);
    if (rc) return rc;
    MI_HIP(hipSetDevice(s->p.device));
    rc = stack_flush(s);
    if (rc) return rc;
    if (level != 0) return mi_stack_sync(s);
    return tiled_sync_level0(s);
}

int mi_stack_finish_device(mi_stack_t* s, void* dev_out) {
    int rc = check_handle(s);
    if (rc) return rc;
    MI_HIP(hipSetDevice(s->p.device));
    rc = stack_flush(s);
    if (rc) return rc;
    if (s->n_pushed == 0) return fail(MI_ERR_STATE, "finish with no frames pushed");
    if (s->f64) rc = s->p.use_fma ? finish_f64<true>(s) : finish_f64<false>(s);
    else rc = s->p.use_fma ? finish_impl<true>(s) : finish_impl<false>(s);
    if (rc) return rc;
    s->finished = true;
    if (dev_out) {
        size_t nb = (size_t)s->p.height * s->p.width * 3 * dtype_size(s->p.out_dtype);
        MI_HIP(hipMemcpyAsync(dev_out, s->out_dev, nb, hipMemcpyDeviceToDevice, s->stream));
    }
    return MI_OK;
}

int mi_stack_finish(mi_stack_t* s, void* host_out, size_t row_stride_bytes) {
    int rc = mi_stack_finish_device(s, nullptr);
    if (rc) return rc;
    if (!host_out) return fail(MI_ERR_INVALID, "null output buffer");
    size_t rb = (size_t)s->p.width * 3 * dtype_size(s->p.out_dtype);
    if (row_stride_bytes == 0) row_stride_bytes = rb;
    if (row_stride_bytes < rb) return fail(MI_ERR_INVALID, "row stride smaller than a row");
    MI_HIP(hipMemcpy2DAsync(host_out, row_stride_bytes, s->out_dev, rb, rb, s->p.height,
                            hipMemcpyDeviceToHost, s->stream));
    MI_HIP(hipStreamSynchronize(s->stream));
    return MI_OK;
}

int mi_stack_get_level(mi_stack_t* s, int level, int what, void* host_out, size_t out_bytes) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!host_out) return fail(MI_ERR_INVALID, "null output");
    MI_HIP(hipSetDevice(s->p.device));
    rc = stack_flush(s);
    if (rc) return rc;
    const int L = s->L;
    const void* src = nullptr;
    size_t bytes = 0;
    auto np = [&](int l) { return (size_t)s->lh[l] * s->lw[l]; };
    const size_t fb = s->f64 ? 8 : 4;   // bytes of a float_type element
    switch (what) {
        case MI_TAP_GAUSS:
            if (level < 1 || level > L) return fail(MI_ERR_INVALID, "MI_TAP_GAUSS: level in [1, %d]", L);
            src = tiled_last_gauss(s, level);
            bytes = np(level) * 3 * fb;
            break;
        case MI_TAP_FUSED_LAP:
            if (level < 0 || level >= L) return fail(MI_ERR_INVALID, "bad level %d", level);
            src = s->bestLap[level]; bytes = np(level) * 3 * fb; break;
        case MI_TAP_ENERGY:
            if (level < 0 || level >= L) return fail(MI_ERR_INVALID, "bad level %d", level);
            src = s->bestE[level]; bytes = np(level) * 4; break;
        case MI_TAP_INDEX:
            if (level < 0 || level >= L) return fail(MI_ERR_INVALID, "bad level %d", level);
            if ((rc = mi_stack_export_indices(s, level))) return rc;   // (index stride > 1: the tap shows global frame numbers)
            src = s->bestIdx[level]; bytes = np(level) * 4; break;
        case MI_TAP_FUSED_BASE:
            if (!s->finished) return fail(MI_ERR_STATE, "fused base is available after finish");
            src = s->fusedBase; bytes = np(L) * 3 * fb; break;
        case MI_TAP_BASE_IDX_E:
            if ((rc = mi_stack_export_indices(s, L))) return rc;
            src = s->idxE; bytes = np(L) * 4; break;
        case MI_TAP_BASE_IDX_D:
            if ((rc = mi_stack_export_indices(s, L + 1))) return rc;
            src = s->idxD; bytes = np(L) * 4; break;
        case MI_TAP_BASE_ENT: src = s->bEnt; bytes = np(L) * fb; break;
        case MI_TAP_BASE_DEV: src = s->bDev; bytes = np(L) * fb; break;
        case MI_TAP_COLLAPSED:
            if (!s->finished) return fail(MI_ERR_STATE, "collapsed image is available after finish");
            if (!s->f64 && !s->have_clipped) {   // finish fused the finest collapse step with the cast: redo it unfused
                const dim3 blk(64, 4);
                if (s->sep)
                    hipLaunchKernelGGL((collapse_sep<float>), grid2d(cdiv(s->lw[0], 2), cdiv(s->lh[0], 2), blk), blk, 0, s->stream, s->collapse_src,
                                       s->lh[1], s->lw[1], (const float*)s->bestLap[0], s->lh[0], s->lw[0], s->maxv, s->colA,
                                       s->k1d[0], s->k1d[1], s->k1d[2]);
                else if (s->p.use_fma)
                    hipLaunchKernelGGL((collapse_simple<true>), grid2d(s->lw[0], s->lh[0], blk), blk, 0, s->stream,
                                       s->collapse_src, s->lh[1], s->lw[1], s->bestLap[0], s->lh[0], s->lw[0], s->colA, s->K);
                else
                    hipLaunchKernelGGL((collapse_simple<false>), grid2d(s->lw[0], s->lh[0], blk), blk, 0, s->stream,
                                       s->collapse_src, s->lh[1], s->lw[1], s->bestLap[0], s->lh[0], s->lw[0], s->colA, s->K);
                const size_t n = np(0) * 3;
                const dim3 g((unsigned)((n + 255) / 256));
                if (s->p.out_dtype == MI_U8)
                    hipLaunchKernelGGL((finalize_cast<uint8_t>), g, dim3(256), 0, s->stream, s->colA, n, s->maxv, s->clipped,
                                       (uint8_t*)s->out_dev);
                else
                    hipLaunchKernelGGL((finalize_cast<uint16_t>), g, dim3(256), 0, s->stream, s->colA, n, s->maxv, s->clipped,
                                       (uint16_t*)s->out_dev);
                MI_HIP(hipGetLastError());
                s->have_clipped = true;
            }
            src = s->clipped; bytes = np(0) * 3 * fb; break;
        default: return fail(MI_ERR_INVALID, "unknown tap %d", what);
    }
    if (out_bytes < bytes) return fail(MI_ERR_INVALID, "output buffer too small: need %zu bytes", bytes);
    MI_HIP(hipMemcpyAsync(host_out, src, bytes, hipMemcpyDeviceToHost, s->stream));
    MI_HIP(hipStreamSynchronize(s->stream));
    return MI_OK;
}

int mi_stack_state(mi_stack_t* s, int level, void** dev_energy, void** dev_lap, void** dev_index, size_t* npixels) {
    int rc = check_handle(s);
    if (rc) return rc;
    MI_HIP(hipSetDevice(s->p.device));
    rc = stack_flush(s);
    if (rc) return rc;
    // hand-off point to foreign streams (RCCL, hipMemcpy on the null stream ...): everything this
    // handle enqueued on its own non-blocking streams must have finished
    rc = tiled_sync_all(s);
    if (rc) return rc;
    MI_HIP(hipStreamSynchronize(s->stream));
    if (s->f64) return fail(MI_ERR_UNSUPPORTED, "the frame-sharded combine works on float-32 state only");
    const int L = s->L;
    void *e = nullptr, *l = nullptr, *i = nullptr;
    size_t n = 0;
    if (level == -1) {   // everything at once: the contiguous slabs (padding pixels included)
        e = s->slabE; l = s->slabL; i = s->slabI; n = s->slab_px;
    } else if (level >= 0 && level < L) {
        e = s->bestE[level]; l = s->bestLap[level]; i = s->bestIdx[level];
        n = (size_t)s->lh[level] * s->lw[level];
    } else if (level == L) {
        e = s->bEnt; l = s->baseE; i = s->idxE; n = (size_t)s->lh[L] * s->lw[L];
    } else if (level == L + 1) {
        e = s->bDev; l = s->baseD; i = s->idxD; n = (size_t)s->lh[L] * s->lw[L];
    } else
        return fail(MI_ERR_INVALID, "bad level %d", level);
    if (dev_energy) *dev_energy = e;
    if (dev_lap) *dev_lap = l;
    if (dev_index) *dev_index = i;
    if (npixels) *npixels = n;
    return MI_OK;
}

int mi_stack_stream(mi_stack_t* s, void** stream) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!stream) return fail(MI_ERR_INVALID, "null stream out");
    *stream = (void*)s->stream;
    return MI_OK;
}

int mi_stack_profile(mi_stack_t* s, int enable) {
    int rc = check_handle(s);
    if (rc) return rc;
    MI_HIP(hipSetDevice(s->p.device));
    rc = prof_drain(s);
    if (rc) return rc;
    if (enable) {  // (re)enabling starts a fresh accumulation
        for (int k = 0; k < MI_PROF_KINDS; ++k) {
            s->prof_ms[k] = 0;
            s->prof_n[k] = 0;
            s->prof_bytes[k] = 0;
        }
    }
    s->prof = enable != 0;
    return MI_OK;
}

int mi_stack_profile_get(mi_stack_t* s, int kind, double* total_ms, int64_t* launches, double* algorithmic_bytes) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (kind < 0 || kind >= MI_PROF_KINDS) return fail(MI_ERR_INVALID, "bad kind %d", kind);
    MI_HIP(hipSetDevice(s->p.device));
    rc = prof_drain(s);
    if (rc) return rc;
    if (total_ms) *total_ms = s->prof_ms[kind];
    if (launches) *launches = s->prof_n[kind];
    if (algorithmic_bytes) *algorithmic_bytes = s->prof_bytes[kind];
    return MI_OK;
}

int mi_combine_select(int device, void* stream, int n, const void* cand_e, const void* cand_lap,
                      const void* cand_idx, size_t npix, void* out_e, void* out_lap, void* out_idx) {
    if (n < 1 || !cand_e || !cand_lap || !out_e || !out_lap) return fail(MI_ERR_INVALID, "bad argument");
    if (npix == 0) return MI_OK;
    MI_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(combine_select, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, n, (const float*)cand_e, (const float*)cand_lap,
                       (const int32_t*)cand_idx, npix, (float*)out_e, (float*)out_lap,
                       (int32_t*)out_idx);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_combine_winner(int device, void* stream, int n, const void* cand_e, size_t npix, void* win) {
    if (npix == 0) return MI_OK;   // an empty chunk (its buffers may be null pointers) is a no-op
    if (n < 1 || n > CB_MAXR || !cand_e || !win) return fail(MI_ERR_INVALID, "bad argument (1 <= ranks <= %d)", CB_MAXR);
    MI_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(combine_winner, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       (const float*)cand_e, npix, (uint8_t*)win);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_combine_winner_idx(int device, void* stream, int n, const void* cand_e, const void* cand_idx, size_t npix, void* win) {
    if (npix == 0) return MI_OK;
    if (n < 1 || n > CB_MAXR || !cand_e || !cand_idx || !win) return fail(MI_ERR_INVALID, "bad argument (1 <= ranks <= %d)", CB_MAXR);
    MI_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(combine_winner_idx, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       (const float*)cand_e, (const int32_t*)cand_idx, npix, (uint8_t*)win);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

size_t mi_combine_plan_bytes(size_t npix, int n_ranks) {
    return ((npix + CB_PX - 1) / CB_PX) * (size_t)n_ranks * sizeof(uint32_t) + CB_MAXR * sizeof(unsigned long long);
}

int mi_combine_plan(int device, void* stream, const void* win, size_t npix, int n_ranks, void* plan, int64_t* totals) {
    if (n_ranks < 1 || n_ranks > CB_MAXR || !totals || (npix && (!win || !plan))) return fail(MI_ERR_INVALID, "bad argument");
    if (npix == 0) {   // nothing to plan: no launch, no synchronisation
        for (int r = 0; r < n_ranks; ++r) totals[r] = 0;
        return MI_OK;
    }
    MI_HIP(hipSetDevice(device));
    const size_t nblocks = (npix + CB_PX - 1) / CB_PX;
    uint32_t* counts = (uint32_t*)plan;
    unsigned long long* tot = (unsigned long long*)(counts + nblocks * n_ranks);
    hipStream_t st = (hipStream_t)stream;
    if (nblocks) {
        switch ((n_ranks + 3) / 4) {
            case 1: hipLaunchKernelGGL(combine_count<1>, dim3((unsigned)nblocks), dim3(256), 0, st, (const uint8_t*)win, npix, n_ranks, counts); break;
            case 2: hipLaunchKernelGGL(combine_count<2>, dim3((unsigned)nblocks), dim3(256), 0, st, (const uint8_t*)win, npix, n_ranks, counts); break;
            default: hipLaunchKernelGGL(combine_count<CB_WORDS>, dim3((unsigned)nblocks), dim3(256), 0, st, (const uint8_t*)win, npix, n_ranks, counts); break;
        }
        hipLaunchKernelGGL(combine_scan, dim3(n_ranks), dim3(1024), 0, st, counts, (int)nblocks, n_ranks, tot);
        MI_HIP(hipGetLastError());
        unsigned long long h[CB_MAXR];
        MI_HIP(hipMemcpyAsync(h, tot, sizeof(unsigned long long) * n_ranks, hipMemcpyDeviceToHost, st));
        MI_HIP(hipStreamSynchronize(st));
        for (int r = 0; r < n_ranks; ++r) totals[r] = (int64_t)h[r];
    } else {
        for (int r = 0; r < n_ranks; ++r) totals[r] = 0;
    }
    return MI_OK;
}

int mi_combine_pack(int device, void* stream, const void* win, size_t npix, int n_ranks, int rank, const void* plan,
                    const void* src, int width, void* out) {
    if (npix == 0) return MI_OK;
    if (n_ranks < 1 || n_ranks > CB_MAXR || rank < 0 || rank >= n_ranks || !win || !plan || !src || !out || width < 1)
        return fail(MI_ERR_INVALID, "bad argument");
    MI_HIP(hipSetDevice(device));
    const dim3 grd((unsigned)((npix + CB_PX - 1) / CB_PX));
#define MI_CB_PACK(NW) hipLaunchKernelGGL((combine_move<true, NW>), grd, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)win, npix, \
                                          n_ranks, rank, (const uint32_t*)plan, (const float*)src, (const float* const*)nullptr, width, (float*)out)
    switch ((n_ranks + 3) / 4) {
        case 1: MI_CB_PACK(1); break;
        case 2: MI_CB_PACK(2); break;
        default: MI_CB_PACK(CB_WORDS); break;
    }
#undef MI_CB_PACK
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_combine_unpack(int device, void* stream, const void* win, size_t npix, int n_ranks, int rank, const void* plan,
                      const void* const* dev_bufs, int width, void* dst) {
    if (npix == 0) return MI_OK;
    if (n_ranks < 1 || n_ranks > CB_MAXR || rank < 0 || rank >= n_ranks || !win || !plan || !dev_bufs || !dst || width < 1)
        return fail(MI_ERR_INVALID, "bad argument");
    MI_HIP(hipSetDevice(device));
    const dim3 grd((unsigned)((npix + CB_PX - 1) / CB_PX));
#define MI_CB_UNPACK(NW) hipLaunchKernelGGL((combine_move<false, NW>), grd, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)win, npix, \
                                            n_ranks, rank, (const uint32_t*)plan, (const float*)nullptr, (const float* const*)dev_bufs, width, (float*)dst)
    switch ((n_ranks + 3) / 4) {
        case 1: MI_CB_UNPACK(1); break;
        case 2: MI_CB_UNPACK(2); break;
        default: MI_CB_UNPACK(CB_WORDS); break;
    }
#undef MI_CB_UNPACK
    MI_HIP(hipGetLastError());
    return MI_OK;
}

namespace {
// shared body of mi_warp_affine_device (M: 2x3, persp == false) and mi_warp_perspective_device (M: 3x3)
int warp_device_impl(int device, void* stream, const void* dev_src, void* dev_dst, void* dev_tmp, void* dev_mask, int height,
                     int width, int dtype, const double* M, bool persp, int border_mode, const double* border_value,
                     int blur_ksize, double blur_sigma) {
    if (!dev_src || !dev_dst || !M || height < 1 || width < 1) return fail(MI_ERR_INVALID, "bad argument");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (border_mode < 0 || border_mode > 2) return fail(MI_ERR_INVALID, "bad border_mode %d", border_mode);
    const bool blur = border_mode == 2;
    if (blur && (!dev_tmp || !dev_mask)) return fail(MI_ERR_INVALID, "border blur needs dev_tmp and dev_mask");
    if (blur && (blur_ksize < 1 || blur_ksize > 31 || !(blur_ksize & 1) || !(blur_sigma > 0)))
        return fail(MI_ERR_INVALID, "blur kernel size must be odd and <= 31, sigma > 0");
    MI_HIP(hipSetDevice(device));
    AffineArgs a{};
    PerspArgs pa{};
    if (persp) {
        // cv::invert of a 3x3 double matrix: cofactors times 1 / det [from memory]; singular -> zeros
        const double* m = M;
        double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
        d = d != 0.0 ? 1.0 / d : 0.0;
        pa.iM[0] = (m[4] * m[8] - m[5] * m[7]) * d; pa.iM[1] = (m[2] * m[7] - m[1] * m[8]) * d; pa.iM[2] = (m[1] * m[5] - m[2] * m[4]) * d;
        pa.iM[3] = (m[5] * m[6] - m[3] * m[8]) * d; pa.iM[4] = (m[0] * m[8] - m[2] * m[6]) * d; pa.iM[5] = (m[2] * m[3] - m[0] * m[5]) * d;
        pa.iM[6] = (m[3] * m[7] - m[4] * m[6]) * d; pa.iM[7] = (m[1] * m[6] - m[0] * m[7]) * d; pa.iM[8] = (m[0] * m[4] - m[1] * m[3]) * d;
        const int bh0 = height < 16 ? height : 16;
        pa.bw0 = 1024 / bh0 < width ? 1024 / bh0 : width;
    } else {
        invert_affine_host(M, a.iM);
    }
    a.h = height;
    a.w = width;
    a.mode = border_mode == 0 ? 0 : 1;
    const int hi = dtype == MI_U8 ? 255 : 65535;
    for (int c = 0; c < 3; ++c) a.border[c] = border_value ? round_sat(border_value[c], hi) : 0;
    GaussArgs g{};
    if (blur) {
        // OpenCV's fixed-point taps for 8- / 16-bit images (getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED,
        // restated in oracle/align_oracle.c::orc_gauss_kernel_fixed [from memory]): exp(x^2 * (-0.125 / sigma^2)) at
        // x = 2i - (n - 1), normalised in double; outer taps rounded half to even with the error carried inwards, the
        // centre tap takes the rest so that the sum is exactly 1 << bits
        g.ksize = blur_ksize;
        const int n = blur_ksize, n2 = (n - 1) / 2, bits = dtype == MI_U8 ? 8 : 16;
        const double sg = blur_sigma > 0 ? blur_sigma : n * 0.15 + 0.35;
        const double scale2x = -0.125 / (sg * sg);
        double t[16], sum = 0.0;
        for (int i = 0, x = 1 - n; i < n2; ++i, x += 2) {
            t[i] = std::exp((double)(x * x) * scale2x);
            sum += t[i];
        }
        sum = sum * 2.0 + 1.0;
        const double mul1 = 1.0 / sum, fixed_1 = (double)(1u << bits);
        int64_t acc = 0;
        double carry = 0.0;
        for (int i = 0; i < n2; ++i) {
            const double adj = t[i] * mul1 * fixed_1 + carry;
            const int64_t v = (int64_t)std::nearbyint(adj);
            carry = adj - (double)v;
            g.k[i] = g.k[n - 1 - i] = (uint32_t)v;
            acc += 2 * v;
        }
        g.k[n2] = (uint32_t)(((int64_t)1 << bits) - acc);
    }
    // The tile scratch (counter / bitmap / list) is cached per (device, stream): two host threads that warp on the SAME
    // stream -- the two step_process chains of pipeline._align_chains_device on the default stream -- must not interleave
    // their enqueue sequences (memset, warp marks tiles, bitmap -> list, blur, scatter), or one warp's memset lands between
    // the other's marks and its list.  One lock across the whole sequence; the stream then runs the sequences in order.
    // The lock is per (device, stream) -- the key of the scratch cache: warps on other GPUs or streams of the same process
    // (the threads of a multi-GPU job) neither serialise here nor wait behind another device's scratch re-allocation.
    static std::mutex map_mu;
    static std::map<std::pair<int, void*>, std::unique_ptr<std::mutex>> enqueue_mus;
    std::mutex* enqueue_mu;
    {
        std::lock_guard<std::mutex> lk(map_mu);
        auto& slot = enqueue_mus[{device, stream}];
        if (!slot) slot.reset(new std::mutex);
        enqueue_mu = slot.get();
    }
    std::lock_guard<std::mutex> lk(*enqueue_mu);
    if (dtype == MI_U8)
        return warp_launch<uint8_t>(device, (hipStream_t)stream, dev_src, dev_tmp, dev_dst, (uint8_t*)dev_mask, height, width, a,
                                    blur, g, persp ? &pa : nullptr);
    return warp_launch<uint16_t>(device, (hipStream_t)stream, dev_src, dev_tmp, dev_dst, (uint8_t*)dev_mask, height, width, a, blur,
                                 g, persp ? &pa : nullptr);
}

// host-buffer form of both
int warp_host_impl(int device, const void* host_src, void* host_dst, void* host_mask, int height, int width, int dtype,
                   const double* M, bool persp, int border_mode, const double* border_value, int blur_ksize, double blur_sigma) {
    if (!host_src || !host_dst) return fail(MI_ERR_INVALID, "null image");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (height < 1 || width < 1) return fail(MI_ERR_INVALID, "bad image size");
    int rc = open_device(device);
    if (rc) return rc;
    const size_t nb = (size_t)height * width * 3 * dtype_size(dtype), np = (size_t)height * width;
    DevScratch scratch(nullptr);
    void *src = nullptr, *dst = nullptr, *tmp = nullptr, *mask = nullptr;
    if ((rc = scratch.upload(&src, host_src, nb)) || (rc = scratch.alloc(&dst, nb)) || (rc = scratch.alloc(&tmp, nb)) ||
        (rc = scratch.alloc(&mask, np)))
        return rc;
    rc = warp_device_impl(device, nullptr, src, dst, tmp, mask, height, width, dtype, M, persp, border_mode, border_value,
                          blur_ksize, blur_sigma);
    if (!rc) rc = scratch.download(host_dst, dst, nb);
    if (!rc && host_mask) rc = scratch.download(host_mask, mask, np);
    return rc;
}
}  // namespace

int mi_warp_affine_device(int device, void* stream, const void* dev_src, void* dev_dst, void* dev_tmp,
                          void* dev_mask, int height, int width, int dtype, const double* M,
                          int border_mode, const double* border_value, int blur_ksize, double blur_sigma) {
    return warp_device_impl(device, stream, dev_src, dev_dst, dev_tmp, dev_mask, height, width, dtype, M, false, border_mode,
                            border_value, blur_ksize, blur_sigma);
}

int mi_warp_perspective_device(int device, void* stream, const void* dev_src, void* dev_dst, void* dev_tmp,
                               void* dev_mask, int height, int width, int dtype, const double* M,
                               int border_mode, const double* border_value, int blur_ksize, double blur_sigma) {
    return warp_device_impl(device, stream, dev_src, dev_dst, dev_tmp, dev_mask, height, width, dtype, M, true, border_mode,
                            border_value, blur_ksize, blur_sigma);
}

int mi_warp_perspective(int device, const void* host_src, void* host_dst, void* host_mask, int height, int width,
                        int dtype, const double* M, int border_mode, const double* border_value,
                        int blur_ksize, double blur_sigma) {
    return warp_host_impl(device, host_src, host_dst, host_mask, height, width, dtype, M, true, border_mode, border_value,
                          blur_ksize, blur_sigma);
}

int mi_warp_affine(int device, const void* host_src, void* host_dst, void* host_mask, int height, int width,
                   int dtype, const double* M, int border_mode, const double* border_value,
                   int blur_ksize, double blur_sigma) {
    return warp_host_impl(device, host_src, host_dst, host_mask, height, width, dtype, M, false, border_mode, border_value,
                          blur_ksize, blur_sigma);
}

int mi_aligner_create(mi_aligner_t* out, int device, int height, int width, int dtype, int subsample,
                      int max_levels) {
    if (!out) return fail(MI_ERR_INVALID, "null argument");
    *out = nullptr;
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (subsample < 1) return fail(MI_ERR_INVALID, "subsample must be >= 1");
    const int h = (height + subsample - 1) / subsample, w = (width + subsample - 1) / subsample;
    if (h < 16 || w < 16) return fail(MI_ERR_INVALID, "image too small for ECC");
    int rc = open_device(device);
    if (rc) return rc;
    mi_aligner* al = new (std::nothrow) mi_aligner();
    if (!al) return fail(MI_ERR_NOMEM, "out of host memory");
    al->device = device; al->height = height; al->width = width; al->dtype = dtype; al->subsample = subsample;
    al->h = h; al->w = w;
    auto dalloc = [&](size_t bytes) -> void* {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        al->bufs.push_back(p);
        return p;
    };
    bool ok = true;
    al->gray = (float*)dalloc((size_t)h * w * 4);
    ok = al->gray != nullptr;
    // pyramid geometry: halve while the short side stays >= 48 pixels
    {
        int lh = h, lw = w;
        for (int l = 0; l < (max_levels > 0 ? max_levels : 8); ++l) {
            al->lv.push_back({lh, lw, nullptr, nullptr});
            if ((lh < lw ? lh : lw) / 2 < 48) break;
            lh = (lh + 1) / 2;
            lw = (lw + 1) / 2;
        }
    }
    for (auto& L : al->lv) {
        L.tmpl = (float*)dalloc((size_t)L.h * L.w * 4);
        ok = ok && L.tmpl;
    }
    if (ok) ok = hipStreamCreateWithFlags(&al->own, hipStreamNonBlocking) == hipSuccess;
    if (!ok || aligner_reserve(al, 1)) {
        aligner_free(al);
        delete al;
        return fail(MI_ERR_NOMEM, "out of device memory");
    }
    *out = al;
    return MI_OK;
}

int mi_aligner_set_area_subsampling(mi_aligner_t al, int enable) {
    if (!al) return fail(MI_ERR_INVALID, "null handle");
    al->area = enable != 0;
    al->have_ref = false;   // the reference pyramid was built with the other rule
    // cv2.resize(INTER_AREA) by 1/s keeps round-half-even(dim / s) pixels where img[::s, ::s] keeps ceil(dim / s): the
    // sub-sampled grid, its centre and the pyramid geometry follow the rule in force (the buffers were allocated for the
    // larger of the two sizes)
    const int s = al->subsample;
    const int h = al->area ? (int)std::nearbyint(al->height * (1.0 / s)) : (al->height + s - 1) / s;
    const int w = al->area ? (int)std::nearbyint(al->width * (1.0 / s)) : (al->width + s - 1) / s;
    if (h < 16 || w < 16) return fail(MI_ERR_INVALID, "image too small for ECC");
    al->h = h;
    al->w = w;
    int lh = h, lw = w;
    for (size_t l = 0; l < al->lv.size(); ++l) {
        al->lv[l].h = lh;
        al->lv[l].w = lw;
        lh = (lh + 1) / 2;
        lw = (lw + 1) / 2;
    }
    return MI_OK;
}

int mi_aligner_destroy(mi_aligner_t al) {
    if (!al) return MI_OK;
    (void)hipSetDevice(al->device);
    (void)hipDeviceSynchronize();
    aligner_free(al);
    delete al;
    return MI_OK;
}

int mi_aligner_set_reference(mi_aligner_t al, void* stream, const void* dev_ref) {
    if (!al || !dev_ref) return fail(MI_ERR_INVALID, "null argument");
    MI_HIP(hipSetDevice(al->device));
    int rc = aligner_build(al, stream ? (hipStream_t)stream : al->own, dev_ref, true, 0);
    if (rc) return rc;
    al->have_ref = true;
    al->pc_ref_valid = false;
    return MI_OK;
}

int mi_aligner_set_phase_init(mi_aligner_t al, int enable) {
    if (!al) return fail(MI_ERR_INVALID, "null argument");
    al->phase_init = enable != 0;
    if (al->phase_init && al->pc_P == 0) {
        // the finest pyramid level with at most 512 pixels per side (the coarsest one if every level is larger)
        int lp = (int)al->lv.size() - 1;
        for (int l = 0; l < (int)al->lv.size(); ++l)
            if (std::max(al->lv[l].h, al->lv[l].w) <= 512) { lp = l; break; }
        al->pc_level = lp;
        al->pc_P = 1 << pc_log2(al->lv[lp].h);
        al->pc_Q = 1 << pc_log2(al->lv[lp].w);
        if (al->pc_P > PC_MAX_N || al->pc_Q > PC_MAX_N || al->pc_P < 2 || al->pc_Q < 2) {
            al->phase_init = false;
            al->pc_P = al->pc_Q = 0;
            return fail(MI_ERR_UNSUPPORTED, "phase correlation: no pyramid level between 2 and %d pixels per side", PC_MAX_N);
        }
    }
    return MI_OK;
}

namespace {

// what mi_phase_correlate_device and its tap share: the argument checks, the scratch and the launches.  `last`: PC_WHOLE
// -> (dx, dy, response) to `host_out`; a MI_PC_TAP_* stage -> the launches up to that stage, its P x Q float2 plane to `host_out`
int pc_run(int device, void* stream, const void* dev_ref, const void* dev_mov, int height, int width, int last, void* host_out) {
    if (!dev_ref || !dev_mov || !host_out) return fail(MI_ERR_INVALID, "null argument");
    if (height < 2 || width < 2) return fail(MI_ERR_INVALID, "plane too small");
    const int P = 1 << pc_log2(height), Q = 1 << pc_log2(width);
    if (P > PC_MAX_N || Q > PC_MAX_N) return fail(MI_ERR_UNSUPPORTED, "phase correlation takes planes of at most %d pixels per side", PC_MAX_N);
    MI_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    DevScratch tmp(st);
    const size_t plane = sizeof(float2) * P * Q;
    float2 *a = nullptr, *b = nullptr;
    double* o = nullptr;
    int rc;
    if ((rc = tmp.alloc(&a, plane)) || (rc = tmp.alloc(&b, plane)) || (rc = tmp.alloc(&o, 3 * sizeof(double)))) return rc;
    if (last == MI_PC_TAP_WINDOWED_MOV) {
        pc_spectrum(st, (const float*)dev_mov, height, width, b, P, Q, last);
        return tmp.download(host_out, b, plane);
    }
    pc_spectrum(st, (const float*)dev_ref, height, width, a, P, Q);
    if (last == MI_PC_TAP_SPECTRUM_REF) return tmp.download(host_out, a, plane);
    pc_spectrum(st, (const float*)dev_mov, height, width, b, P, Q);
    if (last == MI_PC_TAP_SPECTRUM_MOV) return tmp.download(host_out, b, plane);
    pc_correlate(st, a, b, P, Q, o, last);
    if (last != PC_WHOLE) return tmp.download(host_out, b, plane);
    return tmp.download(host_out, o, 3 * sizeof(double));
}

}  // namespace

int mi_phase_correlate_device(int device, void* stream, const void* dev_ref, const void* dev_mov, int height, int width,
                              double* out3) {
    return pc_run(device, stream, dev_ref, dev_mov, height, width, PC_WHOLE, out3);
}

int mi_phase_correlate_tap_device(int device, void* stream, const void* dev_ref, const void* dev_mov, int height, int width,
                                  int what, void* host_out) {
    if (what < MI_PC_TAP_WINDOWED_MOV || what > MI_PC_TAP_SURFACE) return fail(MI_ERR_INVALID, "unknown phase-correlation tap %d", what);
    return pc_run(device, stream, dev_ref, dev_mov, height, width, what, host_out);
}

int mi_aligner_estimate_batch(mi_aligner_t al, void* stream, const void* const* dev_movs, int n, int max_iters,
                              double eps, double* M_out, double* cc_out, int* iters_out) {
    if (!al || !dev_movs || !M_out) return fail(MI_ERR_INVALID, "null argument");
    if (n < 1 || n > ECC_MAXF) return fail(MI_ERR_INVALID, "batch of %d frames (1..%d)", n, ECC_MAXF);
    if (!al->have_ref) return fail(MI_ERR_STATE, "mi_aligner_set_reference has not been called");
    for (int k = 0; k < n; ++k)
        if (!dev_movs[k]) return fail(MI_ERR_INVALID, "null frame %d", k);
    MI_HIP(hipSetDevice(al->device));
    hipStream_t st = stream ? (hipStream_t)stream : al->own;
    int rc = aligner_reserve(al, n);
    if (rc) return rc;
    if ((rc = aligner_build_batch(al, st, dev_movs, n))) return rc;   // gray + pyramids of the batch's frames
    return aligner_solve(al, st, n, max_iters, eps, M_out, cc_out, iters_out);
}

int mi_aligner_estimate_pairs(mi_aligner_t al, void* stream, const void* const* dev_frames, int n, const int* ref_of,
                              int max_iters, double eps, double* M_out, double* cc_out, int* iters_out) {
    if (!al || !dev_frames || !ref_of || !M_out) return fail(MI_ERR_INVALID, "null argument");
    if (n < 1 || n > ECC_MAXF) return fail(MI_ERR_INVALID, "batch of %d frames (1..%d)", n, ECC_MAXF);
    for (int k = 0; k < n; ++k) {
        if (!dev_frames[k]) return fail(MI_ERR_INVALID, "null frame %d", k);
        if (ref_of[k] < 0 || ref_of[k] >= n) return fail(MI_ERR_INVALID, "frame %d: reference %d is not a frame of the batch", k, ref_of[k]);
    }
    MI_HIP(hipSetDevice(al->device));
    hipStream_t st = stream ? (hipStream_t)stream : al->own;
    int rc = aligner_reserve(al, n);
    if (rc) return rc;
    if ((rc = aligner_build_batch(al, st, dev_frames, n))) return rc;   // gray + pyramids of the batch's frames
    return aligner_solve(al, st, n, max_iters, eps, M_out, cc_out, iters_out, nullptr, nullptr, -1, ref_of);
}

int mi_aligner_refine_batch(mi_aligner_t al, void* stream, const void* const* dev_movs, int n, const double* M_init, int levels,
                            int max_iters, double eps, double* M_out, double* cc_out, int* iters_out) {
    if (!al || !dev_movs || !M_out || !M_init) return fail(MI_ERR_INVALID, "null argument");
    if (n < 1 || n > ECC_MAXF) return fail(MI_ERR_INVALID, "batch of %d frames (1..%d)", n, ECC_MAXF);
    if (levels < 1) return fail(MI_ERR_INVALID, "levels must be >= 1");
    if (!al->have_ref) return fail(MI_ERR_STATE, "mi_aligner_set_reference has not been called");
    for (int k = 0; k < n; ++k)
        if (!dev_movs[k]) return fail(MI_ERR_INVALID, "null frame %d", k);
    MI_HIP(hipSetDevice(al->device));
    hipStream_t st = stream ? (hipStream_t)stream : al->own;
    int rc = aligner_reserve(al, n);
    if (rc) return rc;
    if ((rc = aligner_build_batch(al, st, dev_movs, n))) return rc;   // gray + pyramids of the batch's frames
    return aligner_solve(al, st, n, max_iters, eps, M_out, cc_out, iters_out, nullptr, M_init, levels - 1);
}

int mi_aligner_estimate_homography_batch(mi_aligner_t al, void* stream, const void* const* dev_movs, int n, int max_iters,
                                         double eps, double* M9_out, double* cc_out, int* iters_out) {
    if (!al || !dev_movs || !M9_out) return fail(MI_ERR_INVALID, "null argument");
    if (n < 1 || n > ECC_MAXF) return fail(MI_ERR_INVALID, "batch of %d frames (1..%d)", n, ECC_MAXF);
    if (!al->have_ref) return fail(MI_ERR_STATE, "mi_aligner_set_reference has not been called");
    for (int k = 0; k < n; ++k)
        if (!dev_movs[k]) return fail(MI_ERR_INVALID, "null frame %d", k);
    MI_HIP(hipSetDevice(al->device));
    hipStream_t st = stream ? (hipStream_t)stream : al->own;
    int rc = aligner_reserve(al, n);
    if (rc) return rc;
    if ((rc = aligner_build_batch(al, st, dev_movs, n))) return rc;   // gray + pyramids of the batch's frames
    return aligner_solve(al, st, n, max_iters, eps, nullptr, cc_out, iters_out, M9_out);
}

int mi_aligner_estimate(mi_aligner_t al, void* stream, const void* dev_mov, int max_iters, double eps,
                        double* M_out, double* cc_out, int* iters_out) {
    if (!dev_mov) return fail(MI_ERR_INVALID, "null argument");
    double cc = -2.0;
    int rc = mi_aligner_estimate_batch(al, stream, &dev_mov, 1, max_iters, eps, M_out, &cc, iters_out);
    if (rc) return rc;
    if (cc_out) *cc_out = cc;
    if (cc == -2.0) return fail(MI_ERR_STATE, "ECC: no overlap, constant image or degenerate transform");
    return MI_OK;
}

int mi_align_stack_device(mi_stack_t* st, mi_aligner_t al, const void* dev_frames, int n_frames, size_t frame_stride,
                          int ref_idx, const mi_align_stack_opts_t* o, const mi_balance_linear_opts_t* bal, void* dev_batches,
                          void* dev_tmp, void* dev_mask, double* M_out, double* cc_out, int* failed_frame) {
    int rc = check_handle(st);
    if (rc) return rc;
    if (!al || !dev_frames || !o || !dev_batches || !M_out || !cc_out) return fail(MI_ERR_INVALID, "null argument");
    if (n_frames < 1 || ref_idx < 0 || ref_idx >= n_frames) return fail(MI_ERR_INVALID, "bad frame count / reference index");
    if (o->ecc_batch < 1 || o->ecc_batch > ECC_MAXF || o->batch_frames < 1) return fail(MI_ERR_INVALID, "bad batch sizes");
    if (al->height != st->p.height || al->width != st->p.width || al->dtype != st->p.in_dtype || al->device != st->p.device)
        return fail(MI_ERR_INVALID, "the estimator and the stack handle are for different frames / devices");
    if (failed_frame) *failed_frame = -1;
    const int H = st->p.height, W = st->p.width, B = o->batch_frames;
    const size_t fb = (size_t)H * W * 3 * dtype_size(st->p.in_dtype);
    if (frame_stride == 0) frame_stride = fb;
    const char* frames = (const char*)dev_frames;
    MI_HIP(hipSetDevice(st->p.device));
    if ((rc = mi_aligner_set_reference(al, nullptr, frames + (size_t)ref_idx * frame_stride))) return rc;
    const bool persp = o->transform == 1;
    std::vector<double> est((size_t)n_frames * 9, 0.0);
    std::vector<char> have((size_t)n_frames, 0);
    for (int i = 0; i < n_frames; ++i) {
        for (int k = 0; k < 9; ++k) M_out[(size_t)i * 9 + k] = 0.0;
        cc_out[i] = 1.0;
    }
    // warp lanes (see mi_aligner): not with the in-place balance, whose histogram / table scratch is one per call
    hipStream_t side[2] = {nullptr, nullptr};
    tiled_side_streams(st, side);
    const int lanes = bal || !side[0] || !side[1] ? 1 : WARP_LANES;
    if (lanes > 1 && (rc = aligner_warp_lanes(al, fb, (size_t)H * W))) return rc;
    for (int j = 0; j < lanes - 1; ++j) al->wst[j] = side[j];
    unsigned lanes_used = 0;
    int cur = 0, filled = 0;
    auto flush = [&]() -> int {
        if (!filled) return MI_OK;
        for (int j = 1; j < lanes; ++j)   // the batch is complete when every lane's warps are
            if (lanes_used & (1u << j)) {
                MI_HIP(hipEventRecord(al->wev[j - 1], al->wst[j - 1]));
                MI_HIP(hipStreamWaitEvent(st->stream, al->wev[j - 1], 0));
            }
        lanes_used = 0;
        // no host synchronisation: the warps ran on the stacker's stream, where the level-0 kernels that read this batch
        // are enqueued next, and the stacker joins its side streams into that stream after every push
        int r = mi_stack_push_frames_device(st, (char*)dev_batches + (size_t)cur * B * fb, filled, fb);
        cur ^= 1;
        filled = 0;
        return r;
    };
    for (int i = 0; i < n_frames; ++i) {
        char* dst = (char*)dev_batches + ((size_t)cur * B + filled) * fb;
        if (filled == 0 && lanes > 1) MI_HIP(hipEventRecord(al->wstart, st->stream));   // this batch buffer is free from here on
        if (i == ref_idx) {
            MI_HIP(hipMemcpyAsync(dst, frames + (size_t)i * frame_stride, fb, hipMemcpyDeviceToDevice, st->stream));
        } else {
            if (!have[i]) {   // the next ecc_batch moving frames in one batched Gauss-Newton (the estimator's own stream)
                const void* ptrs[ECC_MAXF];
                int idx[ECC_MAXF], nb = 0;
                for (int k = i; k < n_frames && nb < o->ecc_batch; ++k)
                    if (k != ref_idx) { idx[nb] = k; ptrs[nb++] = frames + (size_t)k * frame_stride; }
                double Ms[ECC_MAXF * 9], ccs[ECC_MAXF];
                int its[ECC_MAXF];
                if (persp) {   // ALIGN_HOMOGRAPHY: the similarity refined to 8 degrees of freedom
                    if ((rc = mi_aligner_estimate_homography_batch(al, nullptr, ptrs, nb, o->max_iters, o->eps, Ms, ccs, its))) return rc;
                } else if ((rc = mi_aligner_estimate_batch(al, nullptr, ptrs, nb, o->max_iters, o->eps, Ms, ccs, its))) return rc;
                const int per = persp ? 9 : 6;
                for (int k = 0; k < nb; ++k) {
                    for (int q = 0; q < per; ++q) est[(size_t)idx[k] * 9 + q] = Ms[k * per + q];
                    cc_out[idx[k]] = ccs[k];
                    have[idx[k]] = 1;
                }
            }
            if (!(cc_out[i] >= o->min_correlation)) {
                if (failed_frame) *failed_frame = i;
                return fail(MI_ERR_ALIGNMENT, "frame %d: correlation %.3f < %.3f", i, cc_out[i], o->min_correlation);
            }
            double* m = M_out + (size_t)i * 9;
            for (int q = 0; q < (persp ? 9 : 6); ++q) m[q] = est[(size_t)i * 9 + q];
            // lane of this frame: the stacker's stream itself (0) or a side stream, which first waits for everything the
            // stacker's stream has done when this batch buffer started to fill (the push that last read it, joined)
            const int lane = lanes > 1 ? filled % lanes : 0;
            hipStream_t ws = st->stream;
            if (lane) {
                ws = al->wst[lane - 1];
                if (!(lanes_used & (1u << lane))) MI_HIP(hipStreamWaitEvent(ws, al->wstart, 0));
                lanes_used |= 1u << lane;
            }
            if ((rc = warp_device_impl(st->p.device, ws, frames + (size_t)i * frame_stride, dst, lane ? al->wtmp[lane - 1] : dev_tmp,
                                       lane ? al->wmask[lane - 1] : dev_mask, H, W, st->p.in_dtype, m, persp, o->border_mode,
                                       o->border_value, o->blur_ksize, o->blur_sigma)))
                return rc;
            if (bal) {   // LINEAR balance of the aligned frame, in place, no host round trip
                const size_t npx = (size_t)H * W;
                if (bal->cvt_to >= 0 && (rc = mi_cvt_color_device(st->p.device, st->stream, dst, dst, npx, st->p.in_dtype, bal->cvt_to))) return rc;
                if ((rc = mi_balance_linear_device(st->p.device, st->stream, dst, bal->dev_hist_scratch, bal->dev_lut, H, W,
                                                   st->p.in_dtype, bal->mode, bal->subsample, bal->fast, bal->mask_size, bal->lo,
                                                   bal->hi, bal->first_channel, bal->ref_means,
                                                   bal->dev_corr_out ? bal->dev_corr_out + (size_t)i * bal->ncorr : nullptr)))
                    return rc;
                if (bal->cvt_from >= 0 && (rc = mi_cvt_color_device(st->p.device, st->stream, dst, dst, npx, st->p.in_dtype, bal->cvt_from))) return rc;
            }
        }
        if (++filled == B && (rc = flush())) return rc;
    }
    return flush();
}

int mi_ecc_similarity(int device, const void* host_ref, const void* host_mov, int height, int width,
                      int dtype, int max_levels, int max_iters, double eps, double* M_out, double* cc_out,
                      int* iters_out) {
    if (!host_ref || !host_mov || !M_out) return fail(MI_ERR_INVALID, "null argument");
    mi_aligner_t al = nullptr;
    int rc = mi_aligner_create(&al, device, height, width, dtype, 1, max_levels);
    if (rc) return rc;
    const size_t nb = (size_t)height * width * 3 * dtype_size(dtype);
    auto run = [&]() -> int {
        DevScratch tmp(al->own);   // the aligner's stream: `raw` is freed behind its work, and before the handle goes
        void* raw = nullptr;
        int r = tmp.upload(&raw, host_ref, nb);
        if (r || (r = mi_aligner_set_reference(al, nullptr, raw))) return r;
        MI_HIP(hipStreamSynchronize(al->own));   // the pyramid is built before `raw` is reused
        MI_HIP(hipMemcpy(raw, host_mov, nb, hipMemcpyHostToDevice));
        return mi_aligner_estimate(al, nullptr, raw, max_iters, eps, M_out, cc_out, iters_out);
    };
    rc = run();
    mi_aligner_destroy(al);
    return rc;
}

namespace {
// histogram of a device frame into dev_scratch (uint32 counts, channel-major), enqueued on `st`, no synchronisation
int hist_enqueue(int device, hipStream_t st, const void* dev_img, void* dev_scratch, int height, int width, int dtype, int mode,
                 int subsample, int fast, double mask_size) {
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (height < 1 || width < 1 || subsample < 1 || (mode != 0 && mode != 1)) return fail(MI_ERR_INVALID, "bad argument");
    MI_HIP(hipSetDevice(device));
    const int nbins = dtype == MI_U8 ? 256 : 65536, nch = mode == 0 ? 3 : 1;
    HistArgs a{};
    a.img = dev_img; a.h = height; a.w = width; a.s = subsample; a.fast = fast ? 1 : 0; a.gray = mode;
    if (subsample == 1) { a.hs = height; a.ws = width; }
    else if (fast) { a.hs = cdiv(height, subsample); a.ws = cdiv(width, subsample); }
    else {   // cv2.resize's output size: round half to even of dim / s
        a.hs = (int)std::nearbyint((double)height * (1.0 / subsample));
        a.ws = (int)std::nearbyint((double)width * (1.0 / subsample));
    }
    if (a.hs < 1 || a.ws < 1) return fail(MI_ERR_INVALID, "image smaller than the sub-sampling factor");
    a.masked = mask_size > 0.0;
    if (a.masked) {   // balance.py:165-175 on the sub-sampled grid
        const double r = (double)(a.ws < a.hs ? a.ws : a.hs) * mask_size / 2.0;
        a.cx = (double)a.ws / 2.0; a.cy = (double)a.hs / 2.0; a.r2 = r * r;
    }
    a.counts = (uint32_t*)dev_scratch;
    MI_HIP(hipMemsetAsync(dev_scratch, 0, sizeof(uint32_t) * nch * nbins, st));
    const size_t total = (size_t)a.hs * a.ws;
    const unsigned nblk = (unsigned)std::min<size_t>((total + 255) / 256, 256 * 8);
    if (dtype == MI_U8) hipLaunchKernelGGL(hist_u8, dim3(nblk), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(hist_u16, dim3(nblk), dim3(256), 0, st, a);
    MI_HIP(hipGetLastError());
    return MI_OK;
}
}  // namespace

int mi_histogram_device(int device, void* stream, const void* dev_img, void* dev_scratch, int height,
                        int width, int dtype, int mode, int subsample, int fast, double mask_size,
                        int64_t* counts) {
    if (!dev_img || !dev_scratch || !counts) return fail(MI_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    int rc = hist_enqueue(device, st, dev_img, dev_scratch, height, width, dtype, mode, subsample, fast, mask_size);
    if (rc) return rc;
    const int nbins = dtype == MI_U8 ? 256 : 65536, nch = mode == 0 ? 3 : 1;
    std::vector<uint32_t> tmp((size_t)nch * nbins);
    MI_HIP(hipMemcpyAsync(tmp.data(), dev_scratch, tmp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MI_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < tmp.size(); ++i) counts[i] = (int64_t)tmp[i];
    return MI_OK;
}

int mi_histogram_device_batch(int device, void* stream, const void* const* dev_imgs, int n, void* dev_scratch, int height,
                              int width, int dtype, int mode, int subsample, int fast, double mask_size, int64_t* counts) {
    if (!dev_imgs || !dev_scratch || !counts || n < 1) return fail(MI_ERR_INVALID, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int nbins = dtype == MI_U8 ? 256 : 65536, nch = mode == 0 ? 3 : 1;
    const size_t per = (size_t)nch * nbins;
    for (int k = 0; k < n; ++k) {
        if (!dev_imgs[k]) return fail(MI_ERR_INVALID, "null frame %d", k);
        int rc = hist_enqueue(device, st, dev_imgs[k], (uint32_t*)dev_scratch + (size_t)k * per, height, width, dtype, mode,
                              subsample, fast, mask_size);
        if (rc) return rc;
    }
    std::vector<uint32_t> tmp(per * n);   // one copy and ONE synchronisation for the whole batch
    MI_HIP(hipMemcpyAsync(tmp.data(), dev_scratch, tmp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MI_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < tmp.size(); ++i) counts[i] = (int64_t)tmp[i];
    return MI_OK;
}

int mi_histogram(int device, const void* host_img, int height, int width, int dtype, int mode,
                 int subsample, int fast, double mask_size, int64_t* counts) {
    if (!host_img || !counts) return fail(MI_ERR_INVALID, "null argument");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (height < 1 || width < 1) return fail(MI_ERR_INVALID, "bad image size");
    int rc = open_device(device);
    if (rc) return rc;
    const size_t nb = (size_t)height * width * 3 * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *img = nullptr, *scr = nullptr;
    if ((rc = tmp.upload(&img, host_img, nb)) || (rc = tmp.alloc(&scr, sizeof(uint32_t) * 3 * 65536))) return rc;
    return mi_histogram_device(device, nullptr, img, scr, height, width, dtype, mode, subsample, fast, mask_size, counts);
}

int mi_apply_lut_device(int device, void* stream, const void* dev_src, void* dev_dst, size_t npixels,
                        int dtype, const void* dev_lut, int nlut) {
    if (!dev_src || !dev_dst || !dev_lut) return fail(MI_ERR_INVALID, "null argument");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (nlut != 1 && nlut != 3) return fail(MI_ERR_INVALID, "nlut must be 1 or 3");
    MI_HIP(hipSetDevice(device));
    const size_t n = npixels * 3;
    if (n == 0) return MI_OK;
    const unsigned nblk = (unsigned)std::min<size_t>((n / 12 + 255) / 256 + 1, 256 * 16);
    if (dtype == MI_U8) {
        if (((uintptr_t)dev_src | (uintptr_t)dev_dst) & 3) return fail(MI_ERR_INVALID, "images must be 4-byte aligned");
        hipLaunchKernelGGL(lut_apply_u8, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)dev_src,
                           (uint8_t*)dev_dst, n, (const uint8_t*)dev_lut, nlut);
    } else {
        hipLaunchKernelGGL(lut_apply_u16, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)dev_src,
                           (uint16_t*)dev_dst, n, (const uint16_t*)dev_lut, nlut);
    }
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_balance_linear_device(int device, void* stream, void* dev_img, void* dev_hist_scratch, void* dev_lut, int height,
                             int width, int dtype, int mode, int subsample, int fast, double mask_size, int lo, int hi,
                             int first_channel, const double* ref_means, double* dev_corr_out) {
    if (!dev_img || !dev_hist_scratch || !dev_lut || !ref_means) return fail(MI_ERR_INVALID, "null argument");
    const int nbins = dtype == MI_U8 ? 256 : 65536, ntab = mode == 0 ? 3 : 1;
    if (first_channel < 0 || first_channel >= ntab) return fail(MI_ERR_INVALID, "bad first_channel %d", first_channel);
    if (lo < 0 || hi > nbins || lo >= hi) return fail(MI_ERR_INVALID, "bad intensity interval [%d, %d)", lo, hi);
    hipStream_t st = (hipStream_t)stream;
    int rc = hist_enqueue(device, st, dev_img, dev_hist_scratch, height, width, dtype, mode, subsample, fast, mask_size);
    if (rc) return rc;
    LinRef ref{};
    for (int c = 0; c < ntab - first_channel; ++c) ref.mean[c] = ref_means[c];
    if (dtype == MI_U8)
        hipLaunchKernelGGL((lut_linear_build<uint8_t>), dim3(ntab), dim3(256), 0, st, (const uint32_t*)dev_hist_scratch, nbins, lo, hi,
                           first_channel, ref, (uint8_t*)dev_lut, dev_corr_out);
    else
        hipLaunchKernelGGL((lut_linear_build<uint16_t>), dim3(ntab), dim3(256), 0, st, (const uint32_t*)dev_hist_scratch, nbins, lo,
                           hi, first_channel, ref, (uint16_t*)dev_lut, dev_corr_out);
    MI_HIP(hipGetLastError());
    return mi_apply_lut_device(device, stream, dev_img, dev_img, (size_t)height * width, dtype, dev_lut, ntab);
}

int mi_cvt_color_device(int device, void* stream, const void* dev_src, void* dev_dst, size_t npixels, int dtype, int code) {
    if (!dev_src || !dev_dst) return fail(MI_ERR_INVALID, "null argument");
    if (dtype != MI_U8)
        return fail(MI_ERR_UNSUPPORTED, "BGR <-> HSV / HLS is defined for 8-bit images only (as cv2.cvtColor: CV_8U / CV_32F)");
    if (code < CVT_BGR2HSV || code > CVT_HLS2BGR) return fail(MI_ERR_INVALID, "bad conversion code %d", code);
    MI_HIP(hipSetDevice(device));
    if (npixels == 0) return MI_OK;
    const dim3 grid((unsigned)std::min<size_t>((npixels + 255) / 256, 256 * 16)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* s = (const uint8_t*)dev_src;
    uint8_t* d = (uint8_t*)dev_dst;
    switch (code) {
        case CVT_BGR2HSV: hipLaunchKernelGGL((cvt_color_u8<CVT_BGR2HSV>), grid, blk, 0, st, s, d, npixels); break;
        case CVT_HSV2BGR: hipLaunchKernelGGL((cvt_color_u8<CVT_HSV2BGR>), grid, blk, 0, st, s, d, npixels); break;
        case CVT_BGR2HLS: hipLaunchKernelGGL((cvt_color_u8<CVT_BGR2HLS>), grid, blk, 0, st, s, d, npixels); break;
        default: hipLaunchKernelGGL((cvt_color_u8<CVT_HLS2BGR>), grid, blk, 0, st, s, d, npixels); break;
    }
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_cvt_color(int device, const void* host_src, void* host_dst, int height, int width, int dtype, int code) {
    if (!host_src || !host_dst || height < 1 || width < 1) return fail(MI_ERR_INVALID, "bad argument");
    if (dtype != MI_U8)
        return fail(MI_ERR_UNSUPPORTED, "BGR <-> HSV / HLS is defined for 8-bit images only (as cv2.cvtColor: CV_8U / CV_32F)");
    int rc = open_device(device);
    if (rc) return rc;
    const size_t np = (size_t)height * width, nb = np * 3;
    DevScratch tmp(nullptr);
    void* buf = nullptr;     // converted in place
    if ((rc = tmp.upload(&buf, host_src, nb)) || (rc = mi_cvt_color_device(device, nullptr, buf, buf, np, dtype, code))) return rc;
    return tmp.download(host_dst, buf, nb);
}

int mi_apply_lut(int device, const void* host_src, void* host_dst, int height, int width, int dtype,
                 const void* host_lut, int nlut) {
    if (!host_src || !host_dst || !host_lut) return fail(MI_ERR_INVALID, "null argument");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (height < 1 || width < 1 || (nlut != 1 && nlut != 3)) return fail(MI_ERR_INVALID, "bad argument");
    int rc = open_device(device);
    if (rc) return rc;
    const size_t np = (size_t)height * width, nb = np * 3 * dtype_size(dtype);
    const size_t lb = (size_t)nlut * (dtype == MI_U8 ? 256 : 65536) * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *src = nullptr, *dst = nullptr, *lut = nullptr;
    if ((rc = tmp.upload(&src, host_src, nb)) || (rc = tmp.alloc(&dst, nb)) || (rc = tmp.upload(&lut, host_lut, lb)) ||
        (rc = mi_apply_lut_device(device, nullptr, src, dst, np, dtype, lut, nlut)))
        return rc;
    return tmp.download(host_dst, dst, nb);
}

// ---------------------------------------------------------------- Vignetting / MaskNoise (kernels_prestack.hpp)
int mi_subsampled_size(int height, int width, int subsample, int fast, int* hs, int* ws) {
    if (!hs || !ws || height < 1 || width < 1 || subsample < 1) return fail(MI_ERR_INVALID, "bad argument");
    if (subsample == 1) { *hs = height; *ws = width; }
    else if (fast) { *hs = cdiv(height, subsample); *ws = cdiv(width, subsample); }   // img[::s, ::s]
    else {   // cv2.resize's output size: round half to even of dim / s
        *hs = (int)std::nearbyint((double)height * (1.0 / subsample));
        *ws = (int)std::nearbyint((double)width * (1.0 / subsample));
    }
    if (*hs < 1 || *ws < 1) return fail(MI_ERR_INVALID, "image smaller than the sub-sampling factor");
    return MI_OK;
}

size_t mi_radial_ring_scratch_bytes(int r_steps) {
    return r_steps < 1 ? 0 : sizeof(double) * ((size_t)r_steps + 1) + (sizeof(uint64_t) + sizeof(uint32_t)) * (size_t)r_steps;
}

int mi_radial_ring_sums_device(int device, void* stream, const void* dev_img, void* dev_scratch, int height, int width, int dtype,
                               int subsample, int fast, int r_steps, const double* radii, uint64_t* sums, uint32_t* counts) {
    if (!dev_img || !dev_scratch || !radii || !sums || !counts) return fail(MI_ERR_INVALID, "null argument");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (r_steps < 1 || r_steps > MI_MAX_RINGS) return fail(MI_ERR_INVALID, "r_steps must be in [1, %d]", MI_MAX_RINGS);
    RingArgs a{};
    int rc = mi_subsampled_size(height, width, subsample, fast, &a.hs, &a.ws);
    if (rc) return rc;
    if (!(radii[r_steps] > 0.0)) return fail(MI_ERR_INVALID, "radii[r_steps] must be positive");
    const size_t total = (size_t)a.hs * a.ws;
    if (total > ((size_t)1 << 31)) return fail(MI_ERR_INVALID, "image too large");
    MI_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    // scratch: radii [r_steps + 1] double | sums [r_steps] uint64 | counts [r_steps] uint32
    double* d_radii = (double*)dev_scratch;
    unsigned long long* d_sums = (unsigned long long*)(d_radii + r_steps + 1);
    uint32_t* d_counts = (uint32_t*)(d_sums + r_steps);
    MI_HIP(hipMemcpyAsync(d_radii, radii, sizeof(double) * (r_steps + 1), hipMemcpyHostToDevice, st));
    MI_HIP(hipMemsetAsync(d_sums, 0, (sizeof(uint64_t) + sizeof(uint32_t)) * (size_t)r_steps, st));
    a.img = dev_img; a.h = height; a.w = width; a.s = subsample; a.fast = fast ? 1 : 0; a.r_steps = r_steps;
    a.radii = d_radii; a.cx = (double)a.ws / 2.0; a.cy = (double)a.hs / 2.0; a.per_r = (double)r_steps / radii[r_steps];
    a.sums = d_sums; a.counts = d_counts;
    const unsigned nblk = (unsigned)std::min<size_t>((total + 255) / 256, 2048);   // <= 2^20 + 256 pixels per workgroup
    if (dtype == MI_U8) hipLaunchKernelGGL(radial_ring_sums<uint8_t>, dim3(nblk), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(radial_ring_sums<uint16_t>, dim3(nblk), dim3(256), 0, st, a);
    MI_HIP(hipGetLastError());
    MI_HIP(hipMemcpyAsync(sums, d_sums, sizeof(uint64_t) * r_steps, hipMemcpyDeviceToHost, st));
    MI_HIP(hipMemcpyAsync(counts, d_counts, sizeof(uint32_t) * r_steps, hipMemcpyDeviceToHost, st));
    MI_HIP(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_vignette_apply_device(int device, void* stream, const void* dev_src, void* dev_dst, int height, int width, int dtype,
                             double i0, double k, double r0, double v0, double max_correction, double threshold) {
    if (!dev_src || !dev_dst) return fail(MI_ERR_INVALID, "null argument");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (height < 1 || width < 1) return fail(MI_ERR_INVALID, "bad image size");
    if (((uintptr_t)dev_src | (uintptr_t)dev_dst) & 15) return fail(MI_ERR_INVALID, "images must be 16-byte aligned");
    MI_HIP(hipSetDevice(device));
    VignArgs a{};
    a.h = height; a.w = width; a.cx = (double)width / 2.0; a.cy = (double)height / 2.0;
    a.i0 = i0; a.k = k; a.r0 = r0; a.v0 = v0; a.max_correction = max_correction; a.threshold = threshold;
    const size_t nspan = (size_t)height * width * 3 * dtype_size(dtype) / 48;
    const unsigned nblk = (unsigned)std::min<size_t>((nspan + 255) / 256 + 1, 256 * 16);
    if (dtype == MI_U8)
        hipLaunchKernelGGL(vignette_apply<uint8_t>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)dev_src,
                           (uint8_t*)dev_dst, a);
    else
        hipLaunchKernelGGL(vignette_apply<uint16_t>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)dev_src,
                           (uint16_t*)dev_dst, a);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_mask_noise_device(int device, void* stream, const void* dev_src, void* dev_dst, int height, int width, int dtype,
                         const int32_t* dev_coords, int n, int kernel_size, int method, void* dev_stage) {
    if (!dev_src || !dev_dst) return fail(MI_ERR_INVALID, "null argument");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (height < 1 || width < 1 || n < 0) return fail(MI_ERR_INVALID, "bad argument");
    if (kernel_size < 1 || !(kernel_size & 1)) return fail(MI_ERR_INVALID, "kernel_size must be odd and >= 1");
    if (method != MASK_NOISE_MEAN && method != MASK_NOISE_MEDIAN) return fail(MI_ERR_INVALID, "bad method %d", method);
    if (n > 0 && (!dev_coords || !dev_stage)) return fail(MI_ERR_INVALID, "null argument");
    MI_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    if (dev_dst != dev_src)
        MI_HIP(hipMemcpyAsync(dev_dst, dev_src, (size_t)height * width * 3 * dtype_size(dtype), hipMemcpyDeviceToDevice, st));
    if (n == 0) return MI_OK;
    const dim3 grid((unsigned)cdiv(n * 3, 256)), blk(256);
    if (dtype == MI_U8) {
        hipLaunchKernelGGL(mask_noise_apply<uint8_t>, grid, blk, 0, st, (const uint8_t*)dev_src, height, width, dev_coords, n,
                           kernel_size / 2, method, (uint32_t*)dev_stage);
        hipLaunchKernelGGL(mask_noise_store<uint8_t>, grid, blk, 0, st, (uint8_t*)dev_dst, width, dev_coords, n,
                           (const uint32_t*)dev_stage);
    } else {
        hipLaunchKernelGGL(mask_noise_apply<uint16_t>, grid, blk, 0, st, (const uint16_t*)dev_src, height, width, dev_coords, n,
                           kernel_size / 2, method, (uint32_t*)dev_stage);
        hipLaunchKernelGGL(mask_noise_store<uint16_t>, grid, blk, 0, st, (uint16_t*)dev_dst, width, dev_coords, n,
                           (const uint32_t*)dev_stage);
    }
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_frame_accumulate_device(int device, void* stream, const void* dev_frames, int n, size_t elements_per_frame, void* dev_sum) {
    if (!dev_frames || !dev_sum || n < 0) return fail(MI_ERR_INVALID, "bad argument");
    if (((uintptr_t)dev_sum & 15) || ((uintptr_t)dev_frames & 3) || (n > 1 && (elements_per_frame & 3)))
        return fail(MI_ERR_INVALID, "sums must be 16-byte aligned, frames 4-byte aligned");
    if (n == 0 || elements_per_frame == 0) return MI_OK;
    MI_HIP(hipSetDevice(device));
    const unsigned nblk = (unsigned)std::min<size_t>((elements_per_frame / 4 + 255) / 256 + 1, 256 * 16);
    hipLaunchKernelGGL(frame_accumulate, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)dev_frames, n,
                       elements_per_frame, (uint32_t*)dev_sum);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_hot_pixel_map_device(int device, void* stream, const void* dev_sum, int n_frames, int height, int width, int blur_size,
                            const int* thresholds, void* dev_mean, void* dev_map, void* dev_counts, uint32_t* counts) {
    if (!dev_sum || !thresholds || !dev_map || !dev_counts || !counts) return fail(MI_ERR_INVALID, "null argument");
    if (height < 1 || width < 1 || n_frames < 1) return fail(MI_ERR_INVALID, "bad argument");
    if (blur_size != 3 && blur_size != 5 && blur_size != 7)
        return fail(MI_ERR_UNSUPPORTED, "blur_size must be 3, 5 or 7 (OpenCV's fixed small Gaussian kernels)");
    static const int W3[3] = {1, 2, 1}, W5[5] = {1, 4, 6, 4, 1}, W7[7] = {2, 7, 14, 18, 14, 7, 2};
    HotArgs a{};
    a.sum = (const uint32_t*)dev_sum; a.h = height; a.w = width; a.n = n_frames; a.r = blur_size / 2;
    const int* wt = blur_size == 3 ? W3 : (blur_size == 5 ? W5 : W7);
    int total = 0;
    for (int i = 0; i < blur_size; ++i) { a.wt[i] = wt[i]; total += wt[i]; }
    a.f2 = (256 / total) * (256 / total);
    for (int c = 0; c < 3; ++c) a.th[c] = thresholds[c];
    a.mean = (uint8_t*)dev_mean; a.map = (uint8_t*)dev_map; a.counts = (uint32_t*)dev_counts;
    MI_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    MI_HIP(hipMemsetAsync(dev_counts, 0, 4 * sizeof(uint32_t), st));
    hipLaunchKernelGGL(hot_pixel_map, dim3(cdiv(width, MI_HOT_TILE), cdiv(height, MI_HOT_TILE)), dim3(MI_HOT_TILE, MI_HOT_TILE), 0, st, a);
    MI_HIP(hipGetLastError());
    MI_HIP(hipMemcpyAsync(counts, dev_counts, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MI_HIP(hipStreamSynchronize(st));
    return MI_OK;
}

// ---------------------------------------------------------------- post-stack denoise (kernels_denoise.hpp)
static int nlm_check(const void* src, const void* dst, int height, int width, int dtype, const uint32_t* table, int table_len,
                     int shift, int template_size, int search_size, bool may_alias) {
    if (!src || !dst || !table) return fail(MI_ERR_INVALID, "null argument");
    if (src == dst && !may_alias) return fail(MI_ERR_INVALID, "src and dst must differ (every output reads a neighbourhood of inputs)");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (height < 1 || width < 1) return fail(MI_ERR_INVALID, "bad image size");
    if (template_size < 1 || search_size < 1) return fail(MI_ERR_INVALID, "window sizes must be positive");
    if (template_size / 2 > MI_NLM_MAX_T || search_size / 2 > MI_NLM_MAX_S)
        return fail(MI_ERR_UNSUPPORTED, "template window 1-%d and search window 1-%d are supported (got %d, %d)",
                    2 * MI_NLM_MAX_T + 1, 2 * MI_NLM_MAX_S + 1, template_size, search_size);
    const int n = (2 * (template_size / 2) + 1) * (2 * (template_size / 2) + 1);
    int want = 0;
    while ((1 << want) < n) ++want;
    if (shift != want) return fail(MI_ERR_INVALID, "shift must be %d for template window %d", want, template_size);
    if (table_len < 1 || table_len > (1 << 24)) return fail(MI_ERR_INVALID, "table_len must be in [1, 2^24]");
    if (table[0] == 0) return fail(MI_ERR_INVALID, "table[0] (the weight of a pixel with itself) must be positive");
    return MI_OK;
}

int mi_nlm_denoise_device(int device, const void* dev_src, void* dev_dst, int height, int width, int dtype, const uint32_t* table,
                          int table_len, int shift, int template_size, int search_size, void* stream) {
    int rc = nlm_check(dev_src, dev_dst, height, width, dtype, table, table_len, shift, template_size, search_size, false);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    DevScratch tmp(st);
    uint32_t* dev_table = nullptr;
    if ((rc = tmp.upload(&dev_table, table, sizeof(uint32_t) * (size_t)table_len))) return rc;
    nlm_launch(st, dev_src, dev_dst, height, width, dtype, dev_table, (uint32_t)table_len, shift, template_size / 2, search_size / 2);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(st));     // synchronous by design: a failed run is reported here, the table goes with `tmp`
    return MI_OK;
}

int mi_nlm_denoise(int device, const void* host_src, void* host_dst, int height, int width, int dtype, const uint32_t* table,
                   int table_len, int shift, int template_size, int search_size) {
    // host_src == host_dst is fine here: the frame passes through two device buffers
    int rc = nlm_check(host_src, host_dst, height, width, dtype, table, table_len, shift, template_size, search_size, true);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nb = (size_t)height * width * 3 * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *src = nullptr, *dst = nullptr;
    if ((rc = tmp.upload(&src, host_src, nb)) || (rc = tmp.alloc(&dst, nb)) ||
        (rc = mi_nlm_denoise_device(device, src, dst, height, width, dtype, table, table_len, shift, template_size, search_size, nullptr)))
        return rc;
    return tmp.download(host_dst, dst, nb);
}

// ---------------------------------------------------------------- unsharp mask (kernels_unsharp.hpp)
static int unsharp_check(const void* src, const void* dst, int height, int width, int dtype, const uint32_t* taps, int ksize,
                         double amount, double threshold, bool may_alias) {
    if (!src || !dst || !taps) return fail(MI_ERR_INVALID, "null argument");
    if (src == dst && !may_alias) return fail(MI_ERR_INVALID, "src and dst must differ (every output reads a neighbourhood of inputs)");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (height < 1 || width < 1 || (size_t)width * 3 > (size_t)INT32_MAX) return fail(MI_ERR_INVALID, "bad image size");
    if (ksize < 1 || !(ksize & 1) || ksize > MI_UNSHARP_MAX_KSIZE)
        return fail(MI_ERR_INVALID, "ksize must be odd and in [1, %d] (got %d)", MI_UNSHARP_MAX_KSIZE, ksize);
    uint64_t sum = 0;
    for (int j = 0; j < ksize; ++j) sum += taps[j];
    const uint64_t one = dtype == MI_U8 ? 256 : 65536;     // what keeps the row and column sums inside their words
    if (sum != one) return fail(MI_ERR_INVALID, "the taps must sum to %llu (got %llu)", (unsigned long long)one, (unsigned long long)sum);
    if (!std::isfinite(amount) || !std::isfinite(threshold)) return fail(MI_ERR_INVALID, "amount and threshold must be finite");
    return MI_OK;
}

int mi_unsharp_mask_device(int device, void* stream, const void* dev_src, void* dev_dst, int height, int width, int dtype,
                           const uint32_t* taps, int ksize, double amount, double threshold) {
    int rc = unsharp_check(dev_src, dev_dst, height, width, dtype, taps, ksize, amount, threshold, false);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    unsharp_launch((hipStream_t)stream, dev_src, dev_dst, height, width, dtype, taps, ksize, amount, threshold);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_unsharp_mask(int device, const void* host_src, void* host_dst, int height, int width, int dtype, const uint32_t* taps,
                    int ksize, double amount, double threshold) {
    // host_src == host_dst is fine here: the frame passes through two device buffers
    int rc = unsharp_check(host_src, host_dst, height, width, dtype, taps, ksize, amount, threshold, true);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t nb = (size_t)height * width * 3 * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *src = nullptr, *dst = nullptr;
    if ((rc = tmp.upload(&src, host_src, nb)) || (rc = tmp.alloc(&dst, nb)) ||
        (rc = mi_unsharp_mask_device(device, nullptr, src, dst, height, width, dtype, taps, ksize, amount, threshold)))
        return rc;
    return tmp.download(host_dst, dst, nb);
}

// ---------------------------------------------------------------- depth map output (kernels_depth.hpp)
enum { WS_I32 = 0, WS_F32 = 1, WS_F64 = 2 };   // element types of the value and weight planes

// out = B(v w) / B(w) (sigma > 0) or v (sigma == 0) as float32, for device planes, on `st`; waits for it (the scratch planes
// go with the call).  vtype / wtype: the planes' element types; dev_w == nullptr: every weight is 1.  f64: the working type.
// first / stride: the consecutive -> global numbering of an int32 index plane (0, 1: none).
static int ws_run(hipStream_t st, int vtype, const void* dev_v, int wtype, const void* dev_w, bool f64, int h, int w, double sigma,
                  int first, int stride, float* dev_out) {
    if (!dev_v || !dev_out) return fail(MI_ERR_INVALID, "null argument");
    if (h < 1 || w < 1) return fail(MI_ERR_INVALID, "bad plane size");
    if (!(sigma >= 0.0) || sigma > MI_WS_MAX_SIGMA) return fail(MI_ERR_INVALID, "sigma must be in [0, %g] (got %g)", MI_WS_MAX_SIGMA, sigma);
    const size_t np = (size_t)h * w;
    const int combo = vtype * 100 + wtype * 10 + (f64 ? 1 : 0);
    if (sigma == 0.0) {
        switch (vtype * 10 + (f64 ? 1 : 0)) {
            case WS_I32 * 10 + 0: ws_passthrough_launch<int32_t, float>(st, (const int32_t*)dev_v, np, first, stride, dev_out); break;
            case WS_I32 * 10 + 1: ws_passthrough_launch<int32_t, double>(st, (const int32_t*)dev_v, np, first, stride, dev_out); break;
            case WS_F32 * 10 + 0: ws_passthrough_launch<float, float>(st, (const float*)dev_v, np, first, stride, dev_out); break;
            case WS_F64 * 10 + 1: ws_passthrough_launch<double, double>(st, (const double*)dev_v, np, first, stride, dev_out); break;
            default: return fail(MI_ERR_INVALID, "unsupported plane types");
        }
        MI_HIP(hipGetLastError());
        MI_HIP(hipStreamSynchronize(st));
        return MI_OK;
    }
    double taps[MI_WS_MAX_TAPS];
    const int radius = ws_gaussian_taps(sigma, taps);
    if (radius >= std::min(h, w))
        return fail(MI_ERR_INVALID, "sigma %g needs a radius of %d pixels: the plane must be larger in both directions", sigma, radius);
    DevScratch tmp(st);
    void *P = nullptr, *Q = nullptr;
    const size_t fb = f64 ? 8 : 4;
    int rc;
    if ((rc = tmp.alloc(&P, np * fb)) || (rc = tmp.alloc(&Q, np * fb))) return rc;
    switch (combo) {
        case WS_I32 * 100 + WS_F32 * 10 + 0:
            ws_smooth_launch<int32_t, float, float>(st, (const int32_t*)dev_v, (const float*)dev_w, h, w, radius, taps, first, stride,
                                                    (float*)P, (float*)Q, dev_out);
            break;
        case WS_I32 * 100 + WS_F32 * 10 + 1:
            ws_smooth_launch<int32_t, float, double>(st, (const int32_t*)dev_v, (const float*)dev_w, h, w, radius, taps, first, stride,
                                                     (double*)P, (double*)Q, dev_out);
            break;
        case WS_I32 * 100 + WS_F64 * 10 + 1:
            ws_smooth_launch<int32_t, double, double>(st, (const int32_t*)dev_v, (const double*)dev_w, h, w, radius, taps, first, stride,
                                                      (double*)P, (double*)Q, dev_out);
            break;
        case WS_F32 * 100 + WS_F32 * 10 + 0:
            ws_smooth_launch<float, float, float>(st, (const float*)dev_v, (const float*)dev_w, h, w, radius, taps, first, stride,
                                                  (float*)P, (float*)Q, dev_out);
            break;
        case WS_F64 * 100 + WS_F64 * 10 + 1:
            ws_smooth_launch<double, double, double>(st, (const double*)dev_v, (const double*)dev_w, h, w, radius, taps, first, stride,
                                                     (double*)P, (double*)Q, dev_out);
            break;
        default: return fail(MI_ERR_INVALID, "unsupported plane types");
    }
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_stack_depth_map_device(mi_stack_t* s, double sigma, void* dev_out) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!dev_out) return fail(MI_ERR_INVALID, "null output");
    MI_HIP(hipSetDevice(s->p.device));
    rc = stack_flush(s);
    if (rc) return rc;
    if (s->n_pushed == 0) return fail(MI_ERR_STATE, "depth map with no frames pushed");
    if (s->L < 1) return fail(MI_ERR_UNSUPPORTED, "the stack has no Laplacian level: no per-pixel winner exists");
    rc = tiled_sync_all(s);
    if (rc) return rc;
    MI_HIP(hipStreamSynchronize(s->stream));
    if (s->aux) MI_HIP(hipStreamSynchronize(s->aux));   // an index export in flight
    // the stored indices are consecutive from first_index until they are exported (export_level_indices)
    const bool local = s->index_stride != 1 && !(s->idx_exported & 1ull);
    return ws_run(s->stream, WS_I32, s->bestIdx[0], WS_F32, s->bestE[0], s->f64, s->lh[0], s->lw[0], sigma, local ? s->first_index : 0,
                  local ? s->index_stride : 1, (float*)dev_out);
}

int mi_stack_depth_map(mi_stack_t* s, double sigma, void* host_out) {
    int rc = check_handle(s);
    if (rc) return rc;
    if (!host_out) return fail(MI_ERR_INVALID, "null output");
    MI_HIP(hipSetDevice(s->p.device));
    const size_t nb = (size_t)s->p.height * s->p.width * sizeof(float);
    DevScratch tmp(s->stream);
    void* out = nullptr;
    if ((rc = tmp.alloc(&out, nb)) || (rc = mi_stack_depth_map_device(s, sigma, out))) return rc;
    return tmp.download(host_out, out, nb);
}

int mi_weighted_smooth(int device, const void* host_value, const void* host_weight, int height, int width, int value_is_int32,
                       int float_type, double sigma, void* host_out) {
    if (!host_value || !host_weight || !host_out) return fail(MI_ERR_INVALID, "null argument");
    if (height < 1 || width < 1) return fail(MI_ERR_INVALID, "bad plane size");
    if (float_type != MI_F32 && float_type != MI_F64) return fail(MI_ERR_INVALID, "float_type must be MI_F32 or MI_F64");
    int rc = open_device(device);
    if (rc) return rc;
    const bool f64 = float_type == MI_F64;
    const size_t np = (size_t)height * width, fb = f64 ? 8 : 4, vb = value_is_int32 ? 4 : fb;
    DevScratch tmp(nullptr);
    void *v = nullptr, *w = nullptr;
    float* out = nullptr;
    const int ft = f64 ? WS_F64 : WS_F32;
    if ((rc = tmp.upload(&v, host_value, np * vb)) || (rc = tmp.upload(&w, host_weight, np * fb)) || (rc = tmp.alloc(&out, np * 4)) ||
        (rc = ws_run(nullptr, value_is_int32 ? WS_I32 : ft, v, ft, w, f64, height, width, sigma, 0, 1, out)))
        return rc;
    return tmp.download(host_out, out, np * 4);
}

// ---------------------------------------------------------------- depth refinement (kernels_guided.hpp)
static_assert(MI_GUIDED_SCRATCH_PLANES == MI_GF_PLANES, "the header's scratch size is the kernels'");
static_assert(MI_GUIDED_MAX_RADIUS == MI_GF_MAX_RADIUS, "the header's radius limit is the kernels'");

// the options every entry point of the family takes, by name
static int gf_check_options(const void* guide, int guide_dtype, int radius, double eps, const void* out) {
    if (!guide) return fail(MI_ERR_INVALID, "guide is null");
    if (!out) return fail(MI_ERR_INVALID, "out is null");
    if (guide_dtype != MI_U8 && guide_dtype != MI_U16) return fail(MI_ERR_INVALID, "guide_dtype must be MI_U8 or MI_U16 (got %d)", guide_dtype);
    if (radius < 1 || radius > MI_GF_MAX_RADIUS)
        return fail(MI_ERR_INVALID, "radius must be in [1, %d] (got %d)", MI_GF_MAX_RADIUS, radius);
    if (!std::isfinite(eps) || eps < 1e-9 || eps > 1e3) return fail(MI_ERR_INVALID, "eps must be in [1e-9, 1e3] (got %g)", eps);
    return MI_OK;
}

static int gf_check(const void* value, const void* weight, int weight_float_type, const void* guide, int guide_dtype, int height,
                    int width, int radius, double eps, double lo, double hi, const void* out) {
    if (!value) return fail(MI_ERR_INVALID, "value is null");
    if (!weight) return fail(MI_ERR_INVALID, "weight is null");
    int rc = gf_check_options(guide, guide_dtype, radius, eps, out);
    if (rc) return rc;
    if (weight_float_type != MI_F32 && weight_float_type != MI_F64)
        return fail(MI_ERR_INVALID, "weight_float_type must be MI_F32 or MI_F64 (got %d)", weight_float_type);
    if (height < 1) return fail(MI_ERR_INVALID, "height must be at least 1 (got %d)", height);
    if (width < 1) return fail(MI_ERR_INVALID, "width must be at least 1 (got %d)", width);
    if ((size_t)height * (size_t)width * 3 > (size_t)INT32_MAX) return fail(MI_ERR_INVALID, "height x width is too large a plane");
    if (!std::isfinite(lo) || !std::isfinite(hi)) return fail(MI_ERR_INVALID, "lo and hi must be finite (got %g, %g)", lo, hi);
    if (lo > hi) return fail(MI_ERR_INVALID, "lo must not exceed hi (got %g > %g)", lo, hi);
    return MI_OK;
}

// the four launches on `st`, for device planes: p float32, w of `wtype` (WS_F32 / WS_F64) or nullptr for unit weights,
// scratch MI_GF_PLANES planes of doubles.  Only enqueues.
static void gf_run(hipStream_t st, const float* p, int wtype, const void* w, const void* guide, int guide_dtype, int h, int width,
                   int radius, double eps, double lo, double hi, double* scratch, float* out) {
    const bool w64 = w && wtype == WS_F64, g8 = guide_dtype == MI_U8;
    if (g8 && w64)
        gf_launch<uint8_t, double>(st, p, (const double*)w, (const uint8_t*)guide, h, width, radius, eps, lo, hi, scratch, out);
    else if (g8)
        gf_launch<uint8_t, float>(st, p, (const float*)w, (const uint8_t*)guide, h, width, radius, eps, lo, hi, scratch, out);
    else if (w64)
        gf_launch<uint16_t, double>(st, p, (const double*)w, (const uint16_t*)guide, h, width, radius, eps, lo, hi, scratch, out);
    else
        gf_launch<uint16_t, float>(st, p, (const float*)w, (const uint16_t*)guide, h, width, radius, eps, lo, hi, scratch, out);
}

static inline size_t gf_round16(size_t n) { return (n + 15) & ~(size_t)15; }

// The refined map of a handle: `unrefined` writes the handle's own depth map into a plane (and waits for it), the filter runs
// on `st` with the handle's weight plane and frame numbers, and the call waits for it.  One allocation holds the scratch
// planes, the unrefined map and, for host pointers, the guide and the result; DevScratch frees it on every way out.
extern "C++" {
template <typename Unrefined, typename Range>
static int gf_refine_handle(hipStream_t st, int h, int width, Unrefined unrefined, int wtype, const void* dev_w, Range range,
                            const void* guide, int guide_dtype, int radius, double eps, void* out, bool host) {
    const size_t np = (size_t)h * (size_t)width, gb = np * 3 * dtype_size(guide_dtype);
    const size_t off_p = MI_GF_PLANES * np * sizeof(double), off_out = off_p + gf_round16(np * 4);
    const size_t off_guide = off_out + (host ? gf_round16(np * 4) : 0), total = off_guide + (host ? gb : 0);
    DevScratch tmp(st);
    uint8_t* buf = nullptr;
    int rc = tmp.alloc(&buf, total);
    if (rc) return rc;
    float* p = (float*)(buf + off_p);
    if ((rc = unrefined(p))) return rc;
    const void* dev_guide = guide;
    if (host) {
        MI_HIP(hipMemcpyAsync(buf + off_guide, guide, gb, hipMemcpyHostToDevice, st));
        dev_guide = buf + off_guide;
    }
    double lo = 0.0, hi = 0.0;
    range(&lo, &hi);
    float* dev_out = host ? (float*)(buf + off_out) : (float*)out;
    gf_run(st, p, wtype, dev_w, dev_guide, guide_dtype, h, width, radius, eps, lo, hi, (double*)buf, dev_out);
    MI_HIP(hipGetLastError());
    if (host) return tmp.download(out, dev_out, np * 4);
    MI_HIP(hipStreamSynchronize(st));
    return MI_OK;
}
}  // extern "C++"

static int stack_depth_map_refined(mi_stack_t* s, double sigma, const void* guide, int guide_dtype, int radius, double eps, void* out,
                                   bool host) {
    int rc = check_handle(s);
    if (rc) return rc;
    if ((rc = gf_check_options(guide, guide_dtype, radius, eps, out))) return rc;
    if (!host && guide_dtype == MI_U16 && ((uintptr_t)guide & 1)) return fail(MI_ERR_INVALID, "guide is not aligned to its samples");
    MI_HIP(hipSetDevice(s->p.device));
    return gf_refine_handle(
        s->stream, s->p.height, s->p.width, [&](float* p) { return mi_stack_depth_map_device(s, sigma, p); }, WS_F32, s->bestE[0],
        [&](double* lo, double* hi) {      // the handle's frame numbers: first, first + (n - 1) * stride
            *lo = (double)s->first_index;
            *hi = (double)(s->first_index + (s->n_pushed - 1) * s->index_stride);
        },
        guide, guide_dtype, radius, eps, out, host);
}

int mi_stack_depth_map_refined_device(mi_stack_t* s, double sigma, const void* dev_guide, int guide_dtype, int radius, double eps,
                                      void* dev_out) {
    return stack_depth_map_refined(s, sigma, dev_guide, guide_dtype, radius, eps, dev_out, false);
}

int mi_stack_depth_map_refined(mi_stack_t* s, double sigma, const void* host_guide, int guide_dtype, int radius, double eps,
                               void* host_out) {
    return stack_depth_map_refined(s, sigma, host_guide, guide_dtype, radius, eps, host_out, true);
}

int mi_depth_guided_device(int device, void* stream, const void* dev_value, const void* dev_weight, int weight_float_type,
                           const void* dev_guide, int guide_dtype, int height, int width, int radius, double eps, double lo, double hi,
                           void* dev_scratch, void* dev_out) {
    int rc = gf_check(dev_value, dev_weight, weight_float_type, dev_guide, guide_dtype, height, width, radius, eps, lo, hi, dev_out);
    if (rc) return rc;
    if (!dev_scratch) return fail(MI_ERR_INVALID, "scratch is null");
    if ((uintptr_t)dev_scratch & 15) return fail(MI_ERR_INVALID, "scratch is not aligned to 16 bytes");
    if (((uintptr_t)dev_value & 3) || ((uintptr_t)dev_out & 3)) return fail(MI_ERR_INVALID, "value and out are float32 planes: not aligned");
    if ((uintptr_t)dev_weight & (weight_float_type == MI_F64 ? 7 : 3)) return fail(MI_ERR_INVALID, "weight is not aligned to its type");
    if (guide_dtype == MI_U16 && ((uintptr_t)dev_guide & 1)) return fail(MI_ERR_INVALID, "guide is not aligned to its samples");
    MI_HIP(hipSetDevice(device));
    gf_run((hipStream_t)stream, (const float*)dev_value, weight_float_type == MI_F64 ? WS_F64 : WS_F32, dev_weight, dev_guide, guide_dtype,
           height, width, radius, eps, lo, hi, (double*)dev_scratch, (float*)dev_out);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_depth_guided(int device, const void* host_value, const void* host_weight, int weight_float_type, const void* host_guide,
                    int guide_dtype, int height, int width, int radius, double eps, double lo, double hi, void* host_out) {
    int rc = gf_check(host_value, host_weight, weight_float_type, host_guide, guide_dtype, height, width, radius, eps, lo, hi, host_out);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t np = (size_t)height * width, wb = weight_float_type == MI_F64 ? 8 : 4;
    DevScratch tmp(nullptr);
    void *v = nullptr, *w = nullptr, *g = nullptr, *scratch = nullptr, *out = nullptr;
    if ((rc = tmp.upload(&v, host_value, np * 4)) || (rc = tmp.upload(&w, host_weight, np * wb)) ||
        (rc = tmp.upload(&g, host_guide, np * 3 * dtype_size(guide_dtype))) ||
        (rc = tmp.alloc(&scratch, MI_GF_PLANES * np * sizeof(double))) || (rc = tmp.alloc(&out, np * 4)) ||
        (rc = mi_depth_guided_device(device, nullptr, v, w, weight_float_type, g, guide_dtype, height, width, radius, eps, lo, hi, scratch,
                                     out)))
        return rc;
    return tmp.download(host_out, out, np * 4);
}

// ---------------------------------------------------------------- stereo views (kernels_stereo.hpp)
static int stereo_check(const void* img, const void* depth, const void* out, int height, int width, int dtype, int n_frames, double shift,
                        double pivot, int near_first, bool may_alias) {
    if (!img || !depth || !out) return fail(MI_ERR_INVALID, "null argument");
    if (img == out && !may_alias) return fail(MI_ERR_INVALID, "the image and the view must differ (a view gathers from the whole row)");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (height < 1 || width < 1 || (size_t)width * 3 > (size_t)INT32_MAX ||
        (size_t)height * (size_t)cdiv(width, MI_SV_SEG) > (size_t)INT32_MAX)
        return fail(MI_ERR_INVALID, "bad image size");
    if (n_frames < 1) return fail(MI_ERR_INVALID, "n_frames must be at least 1 (got %d)", n_frames);
    if (!std::isfinite(shift) || std::fabs(shift) > (double)MI_SV_MAX_SHIFT)
        return fail(MI_ERR_INVALID, "shift must be in [-%d, %d] (got %g)", MI_SV_MAX_SHIFT, MI_SV_MAX_SHIFT, shift);
    if (std::ceil(std::fabs(shift)) >= (double)width)
        return fail(MI_ERR_INVALID, "a shift of %g pixels does not fit a row of %d", shift, width);
    if (!(pivot >= 0.0 && pivot <= 1.0)) return fail(MI_ERR_INVALID, "pivot must be in [0, 1] (got %g)", pivot);
    if (near_first != 0 && near_first != 1) return fail(MI_ERR_INVALID, "near_first must be 0 or 1");
    return MI_OK;
}

int mi_stereo_view_device(int device, void* stream, const void* dev_img, const void* dev_depth, void* dev_out, int height, int width,
                          int dtype, int n_frames, double shift, double pivot, int near_first) {
    int rc = stereo_check(dev_img, dev_depth, dev_out, height, width, dtype, n_frames, shift, pivot, near_first, false);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    if (dtype == MI_U8)
        stereo_view_launch<uint8_t>((hipStream_t)stream, dev_img, (const float*)dev_depth, dev_out, height, width, n_frames, (float)shift,
                                    (float)pivot, near_first);
    else
        stereo_view_launch<uint16_t>((hipStream_t)stream, dev_img, (const float*)dev_depth, dev_out, height, width, n_frames, (float)shift,
                                     (float)pivot, near_first);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_stereo_view(int device, const void* host_img, const void* host_depth, void* host_out, int height, int width, int dtype,
                   int n_frames, double shift, double pivot, int near_first) {
    // host_img == host_out is fine here: the frame passes through two device buffers
    int rc = stereo_check(host_img, host_depth, host_out, height, width, dtype, n_frames, shift, pivot, near_first, true);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t np = (size_t)height * width, nb = np * 3 * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *img = nullptr, *depth = nullptr, *out = nullptr;
    if ((rc = tmp.upload(&img, host_img, nb)) || (rc = tmp.upload(&depth, host_depth, np * 4)) || (rc = tmp.alloc(&out, nb)) ||
        (rc = mi_stereo_view_device(device, nullptr, img, depth, out, height, width, dtype, n_frames, shift, pivot, near_first)))
        return rc;
    return tmp.download(host_out, out, nb);
}

int mi_stereo_compose_device(int device, void* stream, const void* dev_left, const void* dev_right, void* dev_out, int height, int width,
                             int dtype, int layout) {
    if (!dev_left || !dev_right || !dev_out) return fail(MI_ERR_INVALID, "null argument");
    if (dev_out == dev_left || dev_out == dev_right) return fail(MI_ERR_INVALID, "the composition needs a buffer of its own");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (height < 1 || width < 1) return fail(MI_ERR_INVALID, "bad image size");
    if (layout != MI_STEREO_PARALLEL && layout != MI_STEREO_CROSS && layout != MI_STEREO_ANAGLYPH)
        return fail(MI_ERR_INVALID, "layout must be MI_STEREO_PARALLEL, MI_STEREO_CROSS or MI_STEREO_ANAGLYPH (got %d)", layout);
    if (layout == MI_STEREO_ANAGLYPH && (((uintptr_t)dev_left | (uintptr_t)dev_right | (uintptr_t)dev_out) & 3u))
        return fail(MI_ERR_INVALID, "the anaglyph's frames must start on 4-byte boundaries");
    MI_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    if (layout == MI_STEREO_ANAGLYPH) {
        if (dtype == MI_U8) anaglyph_launch<uint8_t>(st, dev_left, dev_right, dev_out, (size_t)height * width);
        else anaglyph_launch<uint16_t>(st, dev_left, dev_right, dev_out, (size_t)height * width);
        MI_HIP(hipGetLastError());
        return MI_OK;
    }
    const size_t rb = (size_t)width * 3 * dtype_size(dtype);        // bytes of one view's row
    const void* first = layout == MI_STEREO_PARALLEL ? dev_left : dev_right;
    const void* second = layout == MI_STEREO_PARALLEL ? dev_right : dev_left;
    MI_HIP(hipMemcpy2DAsync(dev_out, 2 * rb, first, rb, rb, (size_t)height, hipMemcpyDeviceToDevice, st));
    MI_HIP(hipMemcpy2DAsync((char*)dev_out + rb, 2 * rb, second, rb, rb, (size_t)height, hipMemcpyDeviceToDevice, st));
    return MI_OK;
}

// ---------------------------------------------------------------- brush retouching (kernels_brush.hpp)
static int brush_frame_check(const void* master, const void* source, int height, int width, int dtype, double opacity) {
    if (!master || !source) return fail(MI_ERR_INVALID, "null argument");
    if (master == source) return fail(MI_ERR_INVALID, "the master and the source must be two frames");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16");
    if (height < 1 || width < 1 || (size_t)width * 3 > (size_t)INT32_MAX || (size_t)height > (size_t)65535 * MI_BR_TH ||
        (size_t)height * (size_t)width > ((size_t)1 << 40))
        return fail(MI_ERR_INVALID, "bad image size");
    if (!(opacity >= 0.0 && opacity <= 1.0)) return fail(MI_ERR_INVALID, "opacity must be in [0, 1] (got %g)", opacity);
    return MI_OK;
}

static int brush_stroke_check(const void* master, const void* source, int height, int width, int dtype, const double* table, int radius,
                              const int32_t* stamps, int n_stamps, double opacity) {
    int rc = brush_frame_check(master, source, height, width, dtype, opacity);
    if (rc) return rc;
    if (!table) return fail(MI_ERR_INVALID, "null argument");
    if (radius < MI_BR_MIN_RADIUS || radius > MI_BR_MAX_RADIUS)
        return fail(MI_ERR_INVALID, "radius must be in [%d, %d] (got %d)", MI_BR_MIN_RADIUS, MI_BR_MAX_RADIUS, radius);
    if (n_stamps < 0 || n_stamps > MI_BR_MAX_STAMPS)
        return fail(MI_ERR_INVALID, "a call takes 0 to %d stamps (got %d)", MI_BR_MAX_STAMPS, n_stamps);
    if (n_stamps > 0 && !stamps) return fail(MI_ERR_INVALID, "null argument");
    return MI_OK;
}

int mi_brush_stroke_device(int device, void* stream, void* dev_master, const void* dev_source, int height, int width, int dtype,
                           const double* dev_table, int radius, const int32_t* dev_stamps, int n_stamps, const int32_t* box,
                           double opacity, double* dev_mask) {
    int rc = brush_stroke_check(dev_master, dev_source, height, width, dtype, dev_table, radius, dev_stamps, n_stamps, opacity);
    if (rc) return rc;
    if (!box) return fail(MI_ERR_INVALID, "null argument");
    const bool empty = box[0] >= box[2] || box[1] >= box[3];
    if (!empty && (box[0] < 0 || box[1] < 0 || box[2] > width || box[3] > height))
        return fail(MI_ERR_INVALID, "the box (%d, %d, %d, %d) leaves the frame", box[0], box[1], box[2], box[3]);
    MI_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    if (dev_mask) MI_HIP(hipMemsetAsync(dev_mask, 0, (size_t)height * (size_t)width * sizeof(double), st));
    if (empty || n_stamps == 0) return MI_OK;
    if (dtype == MI_U8)
        brush_stroke_launch<uint8_t>(st, dev_master, dev_source, dev_table, dev_stamps, n_stamps, radius, width, box, opacity, dev_mask);
    else
        brush_stroke_launch<uint16_t>(st, dev_master, dev_source, dev_table, dev_stamps, n_stamps, radius, width, box, opacity, dev_mask);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

// the union of the stamps' footprints clipped to the frame, (x_start, y_start, x_end, y_end), or (0, 0, 0, 0)
static void brush_area(const int32_t* stamps, int n_stamps, int radius, int height, int width, int32_t* area) {
    int64_t x0 = INT64_MAX, y0 = INT64_MAX, x1 = 0, y1 = 0;
    for (int i = 0; i < n_stamps; ++i) {
        const int64_t cx = stamps[2 * i], cy = stamps[2 * i + 1];
        const int64_t xs = std::max<int64_t>(0, cx - radius), xe = std::min<int64_t>(width, cx + radius + 1);
        const int64_t ys = std::max<int64_t>(0, cy - radius), ye = std::min<int64_t>(height, cy + radius + 1);
        if (xs >= xe || ys >= ye) continue;
        x0 = std::min(x0, xs); y0 = std::min(y0, ys); x1 = std::max(x1, xe); y1 = std::max(y1, ye);
    }
    if (x1 == 0) x0 = y0 = y1 = 0;
    area[0] = (int32_t)x0; area[1] = (int32_t)y0; area[2] = (int32_t)x1; area[3] = (int32_t)y1;
}

int mi_brush_stroke(int device, void* host_master, const void* host_source, int height, int width, int dtype, const double* host_table,
                    int radius, const int32_t* host_stamps, int n_stamps, double opacity, double* host_mask, int32_t* area) {
    int rc = brush_stroke_check(host_master, host_source, height, width, dtype, host_table, radius, host_stamps, n_stamps, opacity);
    if (rc) return rc;
    int ndev = 0;
    if ((rc = visible_devices(&ndev))) return rc;
    int32_t box[4];
    brush_area(host_stamps, n_stamps, radius, height, width, box);
    if (area) memcpy(area, box, sizeof(box));
    const size_t np = (size_t)height * width, nb = np * 3 * dtype_size(dtype);
    if (box[0] >= box[2]) {           // nothing is painted: the master stays as it is
        if (host_mask) memset(host_mask, 0, np * sizeof(double));
        return MI_OK;
    }
    MI_HIP(hipSetDevice(device));
    const size_t side = 2 * (size_t)radius + 1, tb = side * side * sizeof(double), sb = (size_t)n_stamps * 2 * sizeof(int32_t);
    DevScratch tmp(nullptr);
    void *master = nullptr, *source = nullptr;
    double *table = nullptr, *mask = nullptr;
    int32_t* stamps = nullptr;
    if ((rc = tmp.upload(&master, host_master, nb)) || (rc = tmp.upload(&source, host_source, nb)) ||
        (rc = tmp.upload(&table, host_table, tb)) || (rc = tmp.upload(&stamps, host_stamps, sb)) ||
        (host_mask && (rc = tmp.alloc(&mask, np * sizeof(double)))) ||
        (rc = mi_brush_stroke_device(device, nullptr, master, source, height, width, dtype, table, radius, stamps, n_stamps, box, opacity, mask)))
        return rc;
    rc = tmp.download(host_master, master, nb);
    if (!rc && host_mask) rc = tmp.download(host_mask, mask, np * sizeof(double));
    return rc;
}

int mi_blend_mask_device(int device, void* stream, void* dev_master, const void* dev_source, const double* dev_mask, int height,
                         int width, int dtype, double opacity) {
    int rc = brush_frame_check(dev_master, dev_source, height, width, dtype, opacity);
    if (rc) return rc;
    if (!dev_mask) return fail(MI_ERR_INVALID, "null argument");
    MI_HIP(hipSetDevice(device));
    if (dtype == MI_U8) blend_mask_launch<uint8_t>((hipStream_t)stream, dev_master, dev_source, dev_mask, (size_t)height * width, opacity);
    else blend_mask_launch<uint16_t>((hipStream_t)stream, dev_master, dev_source, dev_mask, (size_t)height * width, opacity);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_blend_mask(int device, void* host_master, const void* host_source, const double* host_mask, int height, int width, int dtype,
                  double opacity) {
    int rc = brush_frame_check(host_master, host_source, height, width, dtype, opacity);
    if (rc) return rc;
    if (!host_mask) return fail(MI_ERR_INVALID, "null argument");
    if ((rc = open_device(device))) return rc;
    const size_t np = (size_t)height * width, nb = np * 3 * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *master = nullptr, *source = nullptr;
    double* mask = nullptr;
    if ((rc = tmp.upload(&master, host_master, nb)) || (rc = tmp.upload(&source, host_source, nb)) ||
        (rc = tmp.upload(&mask, host_mask, np * sizeof(double))) ||
        (rc = mi_blend_mask_device(device, nullptr, master, source, mask, height, width, dtype, opacity)))
        return rc;
    return tmp.download(host_master, master, nb);
}

// ---------------------------------------------------------------- depth-selected composite (kernels_composite.hpp)
static int composite_check(const void* const* frame_ptrs, int first, int count, int n_frames, const void* depth, const void* out,
                           int height, int width, int dtype, int interp, bool on_device) {
    if (!frame_ptrs || !depth || !out) return fail(MI_ERR_INVALID, "null argument");
    if (dtype != MI_U8 && dtype != MI_U16 && dtype != MI_F32) return fail(MI_ERR_INVALID, "dtype must be MI_U8, MI_U16 or MI_F32");
    if (interp != MI_COMPOSITE_LINEAR && interp != MI_COMPOSITE_NEAREST)
        return fail(MI_ERR_INVALID, "interp must be MI_COMPOSITE_LINEAR or MI_COMPOSITE_NEAREST (got %d)", interp);
    if (height < 1 || width < 1 || (size_t)height * (size_t)width > ((size_t)1 << 40)) return fail(MI_ERR_INVALID, "bad image size");
    if (n_frames < 1 || n_frames > (1 << 24)) return fail(MI_ERR_INVALID, "n_frames must be in [1, 2^24] (got %d)", n_frames);
    if (count < 1) return fail(MI_ERR_INVALID, "count must be at least 1 (got %d)", count);
    if (first < 0 || first > n_frames - count)
        return fail(MI_ERR_INVALID, "the chunk [%d, %d + %d) leaves the stack's [0, %d)", first, first, count, n_frames);
    if (count == 1 && n_frames > 1) return fail(MI_ERR_INVALID, "a chunk of a stack of %d frames holds at least 2 of them", n_frames);
    const size_t fb = (size_t)height * width * 3 * dtype_size(dtype);
    for (int i = 0; i < count; ++i) {
        const char* p = (const char*)frame_ptrs[i];
        if (!p) return fail(MI_ERR_INVALID, "null frame (chunk entry %d)", i);
        if (p < (const char*)out + fb && (const char*)out < p + fb)
            return fail(MI_ERR_INVALID, "the output must not alias a frame (chunk entry %d): frames are only read", i);
        if (on_device && ((uintptr_t)p & (dtype_size(dtype) - 1))) return fail(MI_ERR_INVALID, "frame %d is not aligned to its sample type", i);
    }
    if (depth == out) return fail(MI_ERR_INVALID, "the output must not alias the depth plane");
    if (on_device && (((uintptr_t)depth & 15u) || ((uintptr_t)out & 3u)))
        return fail(MI_ERR_INVALID, "the depth plane starts on a 16-byte boundary and the output on a 4-byte boundary");
    return MI_OK;
}

int mi_depth_composite_device(int device, void* stream, const void* const* frame_ptrs, int first, int count, int n_frames,
                              const void* dev_depth, void* dev_out, int height, int width, int dtype, int interp) {
    int rc = composite_check(frame_ptrs, first, count, n_frames, dev_depth, dev_out, height, width, dtype, interp, true);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const size_t npx = (size_t)height * width;
    const int nearest = interp == MI_COMPOSITE_NEAREST;
    // the addresses travel in the kernel arguments (64 per launch): nothing is allocated or copied, the call never waits
    if (dtype == MI_U8) depth_composite_launch<uint8_t>(st, frame_ptrs, (const float*)dev_depth, dev_out, npx, first, count, n_frames, nearest);
    else if (dtype == MI_U16) depth_composite_launch<uint16_t>(st, frame_ptrs, (const float*)dev_depth, dev_out, npx, first, count, n_frames, nearest);
    else depth_composite_launch<float>(st, frame_ptrs, (const float*)dev_depth, dev_out, npx, first, count, n_frames, nearest);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_depth_composite(int device, const void* const* frame_ptrs, int first, int count, int n_frames, const void* host_depth,
                       void* host_out, int height, int width, int dtype, int interp) {
    int rc = composite_check(frame_ptrs, first, count, n_frames, host_depth, host_out, height, width, dtype, interp, false);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t np = (size_t)height * width, nb = np * 3 * dtype_size(dtype);
    DevScratch tmp(nullptr);
    void *depth = nullptr, *out = nullptr;
    std::vector<void*> frames((size_t)count, nullptr);
    if ((rc = tmp.upload(&depth, host_depth, np * 4)) || (rc = tmp.upload(&out, host_out, nb))) return rc;   // `out`: pixels of other chunks keep what they hold
    for (int i = 0; i < count; ++i)
        if ((rc = tmp.upload(&frames[(size_t)i], frame_ptrs[i], nb))) return rc;
    if ((rc = mi_depth_composite_device(device, nullptr, frames.data(), first, count, n_frames, depth, out, height, width, dtype, interp)))
        return rc;
    return tmp.download(host_out, out, nb);
}

int mi_synth_frames_device(int device, void* dev_out, int dtype, int height, int width,
                           int first_frame, int n_frames, int stack_size, uint32_t seed) {
    if (!dev_out || height < 1 || width < 1 || n_frames < 0 || stack_size < 1)
        return fail(MI_ERR_INVALID, "bad argument");
    MI_HIP(hipSetDevice(device));
    size_t per = (size_t)height * width * 3;
    // one launch per frame keeps the grid within 32-bit block counts
    for (int f = 0; f < n_frames; ++f) {
        dim3 g((unsigned)((per + 255) / 256));
        char* dst = (char*)dev_out + (size_t)f * per * dtype_size(dtype);
        switch (dtype) {
            case MI_U8:
                hipLaunchKernelGGL((synth_frames<uint8_t>), g, dim3(256), 0, 0, (uint8_t*)dst,
                                   height, width, first_frame + f, 1, stack_size, seed, 1);
                break;
            case MI_U16:
                hipLaunchKernelGGL((synth_frames<uint16_t>), g, dim3(256), 0, 0, (uint16_t*)dst,
                                   height, width, first_frame + f, 1, stack_size, seed, 257);
                break;
            case MI_F32:
                hipLaunchKernelGGL((synth_frames<float>), g, dim3(256), 0, 0, (float*)dst, height,
                                   width, first_frame + f, 1, stack_size, seed, 1);
                break;
            default: return fail(MI_ERR_INVALID, "bad dtype %d", dtype);
        }
    }
    MI_HIP(hipGetLastError());
    MI_HIP(hipDeviceSynchronize());
    return MI_OK;
}

}  // extern "C"

// DepthMapStack handle (mi_dmap_*)
#include "depthmap_host.hpp"

// the feature estimator (mi_feat_*)
#include "features_host.hpp"
