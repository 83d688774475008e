// features_host.hpp -- the mi_feat_* entry points: the feature estimator's host side (kernels_features.hpp has the kernels
// and the stage list, tests/features_restatement.py the specification).  Included by capi.hip (one translation unit).
//
// Every entry point checks all of its arguments and names the one it refuses before the first device call.  The device
// forms of gray, score, match and ransac enqueue on `stream` and do not wait.  Extraction cannot be a pure enqueue: per
// level the histogram comes back to choose the cut and the compacted keys come back to be sorted (at most capacity x 8
// bytes), so both of its forms wait, and its results land in host memory.
#pragma once
#include "kernels_features.hpp"

namespace {

using namespace mi;

constexpr int FEAT_MAX_SIDE = 32768;          // a key holds x and y in 16 bits each
constexpr int FEAT_MAX_LEVELS = 8;
constexpr int FEAT_MAX_FEATURES = 1 << 16;
constexpr int FEAT_MAX_DESCRIPTORS = 1 << 20;
constexpr int FEAT_MAX_MATCHES = 1 << 24;
constexpr int FEAT_MAX_HYPOTHESES = 1 << 20;

int feat_shape_check(int height, int width) {
    if (height < 1 || width < 1) return fail(MI_ERR_INVALID, "height and width must be >= 1 (got %dx%d)", width, height);
    if (height > FEAT_MAX_SIDE || width > FEAT_MAX_SIDE)
        return fail(MI_ERR_INVALID, "height and width must be <= %d (got %dx%d)", FEAT_MAX_SIDE, width, height);
    return MI_OK;
}

int feat_frame_check(const void* frame, int height, int width, int channels, int dtype) {
    if (!frame) return fail(MI_ERR_INVALID, "null frame");
    int rc = feat_shape_check(height, width);
    if (rc) return rc;
    if (channels != 1 && channels != 3) return fail(MI_ERR_INVALID, "channels must be 1 or 3 (got %d)", channels);
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16 for a feature frame (got %d)", dtype);
    return MI_OK;
}

int feat_threshold_check(int threshold) {
    if (threshold < 0 || threshold > 254) return fail(MI_ERR_INVALID, "threshold must be in [0, 254] (got %d)", threshold);
    return MI_OK;
}

int feat_gray_check(const void* frame, int height, int width, int channels, int dtype, const void* gray) {
    int rc = feat_frame_check(frame, height, width, channels, dtype);
    if (rc) return rc;
    if (!gray) return fail(MI_ERR_INVALID, "null gray plane");
    return MI_OK;
}

int feat_score_check(const void* gray, int height, int width, int threshold, const void* score, const void* hist) {
    if (!gray) return fail(MI_ERR_INVALID, "null gray plane");
    int rc = feat_shape_check(height, width);
    if (rc || (rc = feat_threshold_check(threshold))) return rc;
    if (!score) return fail(MI_ERR_INVALID, "null score plane");
    if (!hist) return fail(MI_ERR_INVALID, "null histogram");
    return MI_OK;
}

int feat_extract_check(const void* frame, int height, int width, int channels, int dtype, int levels, int n_features,
                       int threshold, const int8_t* pattern, int max_kp, const void* kp, const void* desc, const int* n_kp) {
    int rc = feat_frame_check(frame, height, width, channels, dtype);
    if (rc) return rc;
    if (levels < 1 || levels > FEAT_MAX_LEVELS) return fail(MI_ERR_INVALID, "levels must be in [1, %d] (got %d)", FEAT_MAX_LEVELS, levels);
    if (n_features < 1 || n_features > FEAT_MAX_FEATURES)
        return fail(MI_ERR_INVALID, "n_features must be in [1, %d] (got %d)", FEAT_MAX_FEATURES, n_features);
    if ((rc = feat_threshold_check(threshold))) return rc;
    if (!pattern) return fail(MI_ERR_INVALID, "null pattern");
    for (int i = 0; i < feat::BINS * feat::N_TESTS * 4; ++i)
        if (pattern[i] < -feat::BR || pattern[i] > feat::BR)
            return fail(MI_ERR_INVALID, "pattern[%d] must be within %d (got %d)", i, feat::BR, (int)pattern[i]);
    int total = 0;
    for (int l = 0; l < levels; ++l) total += n_features >> l;
    if (max_kp < total) return fail(MI_ERR_INVALID, "max_kp must hold the sum of n_features >> level, %d (got %d)", total, max_kp);
    if (!kp) return fail(MI_ERR_INVALID, "null keypoint array");
    if (!desc) return fail(MI_ERR_INVALID, "null descriptor array");
    if (!n_kp) return fail(MI_ERR_INVALID, "null n_kp");
    return MI_OK;
}

int feat_match_check(const void* query, int nq, const void* train, int nt, const void* out) {
    if (!query) return fail(MI_ERR_INVALID, "null query descriptors");
    if (!train) return fail(MI_ERR_INVALID, "null train descriptors");
    if (nq < 1 || nq > FEAT_MAX_DESCRIPTORS) return fail(MI_ERR_INVALID, "nq must be in [1, %d] (got %d)", FEAT_MAX_DESCRIPTORS, nq);
    if (nt < 1 || nt > FEAT_MAX_DESCRIPTORS) return fail(MI_ERR_INVALID, "nt must be in [1, %d] (got %d)", FEAT_MAX_DESCRIPTORS, nt);
    if (!out) return fail(MI_ERR_INVALID, "null match output");
    return MI_OK;
}

int feat_ransac_check(const void* src, const void* dst, int n, const void* samples, int k, int model, double thr,
                      const void* counts, const void* models) {
    if (!src) return fail(MI_ERR_INVALID, "null source points");
    if (!dst) return fail(MI_ERR_INVALID, "null destination points");
    if (model != MI_FEAT_SIMILARITY && model != MI_FEAT_HOMOGRAPHY) return fail(MI_ERR_INVALID, "unknown model %d", model);
    const int ns = model == MI_FEAT_HOMOGRAPHY ? 4 : 2;
    if (n < ns || n > FEAT_MAX_MATCHES) return fail(MI_ERR_INVALID, "n must be in [%d, %d] for this model (got %d)", ns, FEAT_MAX_MATCHES, n);
    if (!samples) return fail(MI_ERR_INVALID, "null sample table");
    if (k < 1 || k > FEAT_MAX_HYPOTHESES) return fail(MI_ERR_INVALID, "k must be in [1, %d] (got %d)", FEAT_MAX_HYPOTHESES, k);
    if (!(thr > 0.0) || !std::isfinite(thr)) return fail(MI_ERR_INVALID, "thr must be finite and > 0");
    if (!counts) return fail(MI_ERR_INVALID, "null counts");
    if (!models) return fail(MI_ERR_INVALID, "null models");
    return MI_OK;
}

void feat_gray_launch(hipStream_t st, const void* frame, int height, int width, int channels, int dtype, uint8_t* gray) {
    const size_t npx = (size_t)height * width;
    const dim3 grid((unsigned)((npx + 255) / 256));
    if (dtype == MI_U8)
        hipLaunchKernelGGL((feat_gray<uint8_t>), grid, dim3(256), 0, st, (const uint8_t*)frame, gray, npx, channels);
    else
        hipLaunchKernelGGL((feat_gray<uint16_t>), grid, dim3(256), 0, st, (const uint16_t*)frame, gray, npx, channels);
}

int feat_score_launch(hipStream_t st, const uint8_t* gray, int height, int width, int threshold, uint8_t* score, uint32_t* hist) {
    MI_HIP(hipMemsetAsync(hist, 0, 256 * sizeof(uint32_t), st));
    const dim3 grid(cdiv(width, feat::TILE_W), cdiv(height, feat::TILE_H));
    hipLaunchKernelGGL(feat_score, grid, dim3(feat::NT), 0, st, gray, score, hist, height, width, threshold);
    return MI_OK;
}

FeatTrig feat_trig() {
    FeatTrig t;
    for (int k = 0; k < feat::BINS; ++k) {
        t.c[k] = (int)std::nearbyint(16384.0 * std::cos(2.0 * M_PI * k / feat::BINS));
        t.s[k] = (int)std::nearbyint(16384.0 * std::sin(2.0 * M_PI * k / feat::BINS));
    }
    return t;
}

// the frame at dev_frame -> keypoints and descriptors of all levels in host memory; arguments already checked
int feat_extract_run(hipStream_t st, DevScratch& tmp, const void* dev_frame, int height, int width, int channels, int dtype,
                     int levels, int n_features, int threshold, const int8_t* host_pattern, int32_t* host_kp, uint8_t* host_desc,
                     int* n_kp) {
    int rc;
    const size_t npx = (size_t)height * width;
    int total = 0;
    for (int l = 0; l < levels; ++l) total += n_features >> l;
    size_t max_cap = 0;
    for (int l = 0; l < levels; ++l) max_cap = std::max<size_t>(max_cap, std::max(4 * (n_features >> l), 4096));
    // one allocation, carved: an allocation costs more than any kernel here
    size_t off = 0;
    auto carve = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_gray = carve(npx), o_next = carve(npx / 4 + 1), o_score = carve(npx), o_hist = carve(257 * sizeof(uint32_t)),
                 o_pattern = carve((size_t)feat::BINS * feat::N_TESTS * 4), o_kp = carve((size_t)total * 5 * sizeof(int32_t)),
                 o_desc = carve((size_t)total * 32), o_keys = carve(max_cap * sizeof(unsigned long long));
    uint8_t* arena = nullptr;
    if ((rc = tmp.alloc(&arena, off))) return rc;
    uint8_t *gray = arena + o_gray, *next = arena + o_next, *score = arena + o_score;
    uint32_t* hist = (uint32_t*)(arena + o_hist);       // 256 bins, then the compaction counter
    int8_t* pattern = (int8_t*)(arena + o_pattern);
    int32_t* kp = (int32_t*)(arena + o_kp);
    uint32_t* desc = (uint32_t*)(arena + o_desc);
    unsigned long long* keys = (unsigned long long*)(arena + o_keys);
    MI_HIP(hipMemcpyAsync(pattern, host_pattern, (size_t)feat::BINS * feat::N_TESTS * 4, hipMemcpyHostToDevice, st));
    const FeatTrig trig = feat_trig();
    feat_gray_launch(st, dev_frame, height, width, channels, dtype, gray);
    std::vector<std::vector<unsigned long long>> level_keys(levels);    // each outlives its upload
    uint32_t host_hist[257];
    int h = height, w = width, found = 0;
    for (int l = 0; l < levels; ++l) {
        if (l > 0) {
            if (h < 2 || w < 2) break;
            hipLaunchKernelGGL(feat_halve, dim3((unsigned)(((size_t)(h / 2) * (w / 2) + 255) / 256)), dim3(256), 0, st, gray, next, h, w);
            std::swap(gray, next);
            h /= 2;
            w /= 2;
        }
        const int n_level = n_features >> l;
        if (n_level < 1 || h < 2 * feat::EDGE + 1 || w < 2 * feat::EDGE + 1) continue;
        if ((rc = feat_score_launch(st, gray, h, w, threshold, score, hist)) || (rc = tmp.download(host_hist, hist, 256 * sizeof(uint32_t))))
            return rc;
        const uint32_t cap = (uint32_t)std::max(4 * n_level, 4096);
        int cut = 256;
        uint64_t tail = 0;      // count(score >= c), walked down from 255: the cut is the smallest c whose tail fits
        for (int c = 255; c > threshold; --c) {
            tail += host_hist[c];
            if (tail > cap) break;
            cut = c;
        }
        uint64_t n_sel = 0;
        for (int c = cut; c < 256; ++c) n_sel += host_hist[c];
        if (n_sel == 0) continue;
        MI_HIP(hipMemsetAsync(hist + 256, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(feat_compact, dim3((unsigned)(((size_t)h * w + 255) / 256)), dim3(256), 0, st, score, h, w, cut, keys,
                           hist + 256, cap);
        std::vector<unsigned long long>& host_keys = level_keys[l];
        host_keys.resize(n_sel);
        if ((rc = tmp.download(host_keys.data(), keys, n_sel * sizeof(unsigned long long)))) return rc;
        std::sort(host_keys.begin(), host_keys.end());
        const int n = (int)std::min<uint64_t>(n_sel, (uint64_t)n_level);
        MI_HIP(hipMemcpyAsync(keys, host_keys.data(), (size_t)n * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(feat_describe, dim3(cdiv(n, 4)), dim3(256), 0, st, gray, h, w, l, keys, n, pattern, trig,
                           kp + (size_t)found * 5, desc + (size_t)found * 8);
        found += n;
    }
    *n_kp = found;
    if (found == 0) {
        MI_HIP(hipStreamSynchronize(st));
        MI_HIP(hipGetLastError());
        return MI_OK;
    }
    if ((rc = tmp.download(host_kp, kp, (size_t)found * 5 * sizeof(int32_t)))) return rc;
    return tmp.download(host_desc, desc, (size_t)found * 32);
}

}  // namespace

extern "C" {

int mi_feat_gray_device(int device, void* stream, const void* dev_frame, int height, int width, int channels, int dtype,
                        void* dev_gray) {
    int rc = feat_gray_check(dev_frame, height, width, channels, dtype, dev_gray);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    feat_gray_launch((hipStream_t)stream, dev_frame, height, width, channels, dtype, (uint8_t*)dev_gray);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_feat_gray(int device, const void* host_frame, int height, int width, int channels, int dtype, void* host_gray) {
    int rc = feat_gray_check(host_frame, height, width, channels, dtype, host_gray);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t npx = (size_t)height * width;
    DevScratch tmp(nullptr);
    void *src = nullptr, *dst = nullptr;
    if ((rc = tmp.upload(&src, host_frame, npx * channels * (dtype == MI_U16 ? 2 : 1))) || (rc = tmp.alloc(&dst, npx)) ||
        (rc = mi_feat_gray_device(device, nullptr, src, height, width, channels, dtype, dst)))
        return rc;
    return tmp.download(host_gray, dst, npx);
}

int mi_feat_score_device(int device, void* stream, const void* dev_gray, int height, int width, int threshold, void* dev_score,
                         void* dev_hist) {
    int rc = feat_score_check(dev_gray, height, width, threshold, dev_score, dev_hist);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    if ((rc = feat_score_launch((hipStream_t)stream, (const uint8_t*)dev_gray, height, width, threshold, (uint8_t*)dev_score,
                                (uint32_t*)dev_hist)))
        return rc;
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_feat_score(int device, const void* host_gray, int height, int width, int threshold, void* host_score, uint32_t* host_hist) {
    int rc = feat_score_check(host_gray, height, width, threshold, host_score, host_hist);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    const size_t npx = (size_t)height * width;
    DevScratch tmp(nullptr);
    void *gray = nullptr, *score = nullptr, *hist = nullptr;
    if ((rc = tmp.upload(&gray, host_gray, npx)) || (rc = tmp.alloc(&score, npx)) || (rc = tmp.alloc(&hist, 256 * sizeof(uint32_t))) ||
        (rc = mi_feat_score_device(device, nullptr, gray, height, width, threshold, score, hist)) ||
        (rc = tmp.download(host_hist, hist, 256 * sizeof(uint32_t))))
        return rc;
    return tmp.download(host_score, score, npx);
}

int mi_feat_extract_device(int device, void* stream, const void* dev_frame, int height, int width, int channels, int dtype,
                           int levels, int n_features, int threshold, const int8_t* host_pattern, int max_kp, int32_t* host_kp,
                           uint8_t* host_desc, int* n_kp) {
    int rc = feat_extract_check(dev_frame, height, width, channels, dtype, levels, n_features, threshold, host_pattern, max_kp,
                                host_kp, host_desc, n_kp);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    DevScratch tmp((hipStream_t)stream);
    return feat_extract_run((hipStream_t)stream, tmp, dev_frame, height, width, channels, dtype, levels, n_features, threshold,
                            host_pattern, host_kp, host_desc, n_kp);
}

int mi_feat_extract(int device, const void* host_frame, int height, int width, int channels, int dtype, int levels, int n_features,
                    int threshold, const int8_t* host_pattern, int max_kp, int32_t* host_kp, uint8_t* host_desc, int* n_kp) {
    int rc = feat_extract_check(host_frame, height, width, channels, dtype, levels, n_features, threshold, host_pattern, max_kp,
                                host_kp, host_desc, n_kp);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    DevScratch tmp(nullptr);
    void* frame = nullptr;
    if ((rc = tmp.upload(&frame, host_frame, (size_t)height * width * channels * (dtype == MI_U16 ? 2 : 1)))) return rc;
    return feat_extract_run(nullptr, tmp, frame, height, width, channels, dtype, levels, n_features, threshold, host_pattern,
                            host_kp, host_desc, n_kp);
}

int mi_feat_match_device(int device, void* stream, const void* dev_query, int nq, const void* dev_train, int nt, void* dev_out) {
    int rc = feat_match_check(dev_query, nq, dev_train, nt, dev_out);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(feat_match, dim3(cdiv(nq, feat::MATCH_NT)), dim3(feat::MATCH_NT), 0, (hipStream_t)stream,
                       (const unsigned long long*)dev_query, nq, (const unsigned long long*)dev_train, nt, (int32_t*)dev_out);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_feat_match(int device, const void* host_query, int nq, const void* host_train, int nt, int32_t* host_out) {
    int rc = feat_match_check(host_query, nq, host_train, nt, host_out);
    if (rc) return rc;
    if ((rc = open_device(device))) return rc;
    DevScratch tmp(nullptr);
    void *q = nullptr, *t = nullptr, *out = nullptr;
    if ((rc = tmp.upload(&q, host_query, (size_t)nq * 32)) || (rc = tmp.upload(&t, host_train, (size_t)nt * 32)) ||
        (rc = tmp.alloc(&out, (size_t)nq * 3 * sizeof(int32_t))) || (rc = mi_feat_match_device(device, nullptr, q, nq, t, nt, out)))
        return rc;
    return tmp.download(host_out, out, (size_t)nq * 3 * sizeof(int32_t));
}

int mi_feat_ransac_device(int device, void* stream, const double* dev_src, const double* dev_dst, int n, const int32_t* dev_samples,
                          int k, int model, double thr, int32_t* dev_counts, double* dev_models) {
    int rc = feat_ransac_check(dev_src, dev_dst, n, dev_samples, k, model, thr, dev_counts, dev_models);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(feat_ransac, dim3(cdiv(k, 4)), dim3(feat::RANSAC_NT), 0, (hipStream_t)stream, dev_src, dev_dst, n, dev_samples,
                       k, model, thr, dev_counts, dev_models);
    MI_HIP(hipGetLastError());
    return MI_OK;
}

int mi_feat_ransac(int device, const double* host_src, const double* host_dst, int n, const int32_t* host_samples, int k, int model,
                   double thr, int32_t* host_counts, double* host_models) {
    int rc = feat_ransac_check(host_src, host_dst, n, host_samples, k, model, thr, host_counts, host_models);
    if (rc) return rc;
    for (int i = 0; i < 2 * n; ++i)
        if (!std::isfinite(host_src[i]) || !std::isfinite(host_dst[i])) return fail(MI_ERR_INVALID, "point %d must be finite", i / 2);
    const int ns = model == MI_FEAT_HOMOGRAPHY ? 4 : 2;
    for (size_t i = 0; i < (size_t)k * ns; ++i)
        if (host_samples[i] < 0 || host_samples[i] >= n)
            return fail(MI_ERR_INVALID, "sample %zu of hypothesis %zu must be in [0, %d) (got %d)", i % ns, i / ns, n, host_samples[i]);
    if ((rc = open_device(device))) return rc;
    DevScratch tmp(nullptr);
    double *src = nullptr, *dst = nullptr, *models = nullptr;
    int32_t *samples = nullptr, *counts = nullptr;
    if ((rc = tmp.upload(&src, host_src, (size_t)n * 16)) || (rc = tmp.upload(&dst, host_dst, (size_t)n * 16)) ||
        (rc = tmp.upload(&samples, host_samples, (size_t)k * ns * sizeof(int32_t))) || (rc = tmp.alloc(&counts, (size_t)k * sizeof(int32_t))) ||
        (rc = tmp.alloc(&models, (size_t)k * 72)) ||
        (rc = mi_feat_ransac_device(device, nullptr, src, dst, n, samples, k, model, thr, counts, models)) ||
        (rc = tmp.download(host_counts, counts, (size_t)k * sizeof(int32_t))))
        return rc;
    return tmp.download(host_models, models, (size_t)k * 72);
}

}  // extern "C"
