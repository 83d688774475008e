// features_host.hpp -- the mi_feat_* entry points: the feature estimator's host side (kernels_features.hpp has the kernels
// and the stage list, tests/features_restatement.py the specification).  Included by capi.hip (one translation unit).
//
// Every entry point checks all of its arguments and names the one it refuses before the first device call.  The device
// forms of gray, score, match and ransac enqueue on `stream` and do not wait.  Extraction cannot be a pure enqueue: per
// level the histogram comes back to choose the cut and the compacted keys come back to be sorted (at most capacity x 8
// bytes), so both of its forms wait, and its results land in host memory.  mi_feat_aligner_t (below) is the form that does
// not: the cut and the sort happen on the device, for a batch of resident frames at a time.
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

// ---- mi_feat_aligner_t: the stages above for a batch of resident frames against one reference frame.  Every buffer is an
// array over frame slots (slot max_batch is the reference), allocated once; the kernels take the frame index from the grid and
// the counts from the device (kernels_features.hpp), so the host waits only for the good-match counts -- it draws the sample
// tables from them -- and for the results.
struct mi_feat_aligner {
    int device = 0, height = 0, width = 0, dtype = 0, channels = 0, subsample = 1, fast = 1;
    int levels = 0, n_features = 0, threshold = 0, max_batch = 0;
    int gh = 0, gw = 0;                              // the grey plane: the sub-sampled frame
    int n_lv = 0;                                    // pyramid levels that exist (a level without a pixel ends the pyramid)
    int lh[8] = {}, lw[8] = {}, n_level[8] = {};
    bool scored[8] = {};                             // large enough to score, and n_features >> level >= 1
    size_t goff[8] = {};                             // a level's offset in a slot's pyramid
    mi::FeatLevels lv = {};                          // keypoint offsets of the levels within a slot
    int total = 0;                                   // keypoint slots per frame: the sum of n_features >> level
    hipStream_t st = nullptr;
    uint8_t* arena = nullptr;
    // arrays over slots; the strides are in the array's elements
    uint8_t *pyr = nullptr, *score = nullptr, *mask = nullptr;
    size_t pyr_stride = 0, score_stride = 0, hist_stride = 0, cc_stride = 0, mask_stride = 0;
    uint32_t *hist = nullptr, *desc = nullptr;
    int32_t *cc = nullptr, *kp = nullptr, *fwd = nullptr, *back = nullptr, *good = nullptr, *n_good = nullptr, *samples = nullptr,
            *counts = nullptr, *head = nullptr;
    unsigned long long* keys = nullptr;
    double *src = nullptr, *dst = nullptr, *models = nullptr, *win_model = nullptr;
    int8_t* pattern = nullptr;
    // pinned host memory: the counts, the sample tables, the results
    int32_t *h_n_good = nullptr, *h_samples = nullptr, *h_head = nullptr;
    double *h_model = nullptr, *h_src = nullptr, *h_dst = nullptr;
    uint8_t* h_mask = nullptr;
    mi::FeatTrig trig;
    bool have_ref = false;
    int last_n = 0, last_k = 0, last_ns = 0;         // the last batch, for the taps
    uint64_t waits = 0, launches = 0;
};

namespace {

constexpr int FEAT_ALIGNER_MAX_FEATURES = 4096;      // feat::SORT_MAX / 4: the selection's candidates fit one workgroup's LDS
constexpr int FEAT_ALIGNER_MAX_ITERS = 4096;         // the hypothesis buffers are allocated in create

void feat_aligner_free(mi_feat_aligner* fa) {
    if (fa->st) (void)hipStreamSynchronize(fa->st);
    if (fa->arena) (void)hipFree(fa->arena);
    for (void* p : {(void*)fa->h_n_good, (void*)fa->h_samples, (void*)fa->h_head, (void*)fa->h_model, (void*)fa->h_src,
                    (void*)fa->h_dst, (void*)fa->h_mask})
        if (p) (void)hipHostFree(p);
    if (fa->st) (void)hipStreamDestroy(fa->st);
}

int feat_aligner_wait(mi_feat_aligner* fa) {
    ++fa->waits;
    MI_HIP(hipStreamSynchronize(fa->st));
    MI_HIP(hipGetLastError());
    return MI_OK;
}

// splitmix64(seed) % n, k rows of m distinct values: features.sample_table value for value
void feat_sample_table(int n, int k, int m, uint64_t seed, int32_t* out) {
    uint64_t state = seed;
    for (int r = 0; r < k; ++r) {
        int32_t* row = out + (size_t)r * m;
        int have = 0;
        while (have < m) {
            state += 0x9E3779B97F4A7C15ull;
            uint64_t z = state;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            const int32_t v = (int32_t)(z % (uint64_t)n);
            bool seen = false;
            for (int i = 0; i < have; ++i) seen = seen || row[i] == v;
            if (!seen) row[have++] = v;
        }
    }
}

// grey, pyramid, score, cut, selection and descriptors of `n` frames into the slots from `slot0` on; enqueues only
int feat_aligner_extract(mi_feat_aligner* fa, const mi::FeatFrames& frames, int n, int slot0) {
    using namespace mi;
    hipStream_t st = fa->st;
    const size_t s0 = (size_t)slot0;
    uint8_t* pyr = fa->pyr + s0 * fa->pyr_stride;
    uint8_t* score = fa->score + s0 * fa->score_stride;
    uint32_t* hist = fa->hist + s0 * fa->hist_stride;
    int32_t* cc = fa->cc + s0 * fa->cc_stride;
    const size_t ks = (size_t)fa->total;
    MI_HIP(hipMemsetAsync(hist, 0, (size_t)n * fa->hist_stride * sizeof(uint32_t), st));
    MI_HIP(hipMemsetAsync(cc, 0, (size_t)n * fa->cc_stride * sizeof(int32_t), st));
    {
        const dim3 grid((unsigned)(((size_t)fa->gh * fa->gw + 255) / 256), (unsigned)n);
        const bool area = !fa->fast && fa->subsample == 2;
#define MI_FEAT_GRAY(T, A) \
    hipLaunchKernelGGL((feat_gray_sub<T, A>), grid, dim3(256), 0, st, frames, pyr, fa->pyr_stride, fa->width, fa->channels, \
                       fa->subsample, fa->gh, fa->gw)
        if (fa->dtype == MI_U8) {
            if (area) MI_FEAT_GRAY(uint8_t, true); else MI_FEAT_GRAY(uint8_t, false);
        } else {
            if (area) MI_FEAT_GRAY(uint16_t, true); else MI_FEAT_GRAY(uint16_t, false);
        }
#undef MI_FEAT_GRAY
        ++fa->launches;
    }
    for (int l = 0; l < fa->n_lv; ++l) {
        const int h = fa->lh[l], w = fa->lw[l];
        if (l > 0) {
            const dim3 grid((unsigned)(((size_t)h * w + 255) / 256), (unsigned)n);
            hipLaunchKernelGGL(feat_halve_batch, grid, dim3(256), 0, st, pyr + fa->goff[l - 1], pyr + fa->goff[l], fa->pyr_stride,
                               fa->lh[l - 1], fa->lw[l - 1]);
            ++fa->launches;
        }
        if (!fa->scored[l]) continue;
        const int n_level = fa->n_level[l];
        const uint32_t cap = (uint32_t)std::max(4 * n_level, 4096);
        const size_t ko = (size_t)fa->lv.koff[l];
        hipLaunchKernelGGL(feat_score_batch, dim3(cdiv(w, feat::TILE_W), cdiv(h, feat::TILE_H), n), dim3(feat::NT), 0, st,
                           pyr + fa->goff[l], fa->pyr_stride, score, fa->score_stride, hist + 256 * l, fa->hist_stride, h, w,
                           fa->threshold);
        hipLaunchKernelGGL(feat_cut, dim3(n), dim3(64), 0, st, hist + 256 * l, fa->hist_stride, cc + feat::CC * l, fa->cc_stride,
                           fa->threshold, cap);
        hipLaunchKernelGGL(feat_select, dim3(n), dim3(feat::SORT_NT), 0, st, score, fa->score_stride, h, w, cc + feat::CC * l,
                           fa->cc_stride, fa->keys + s0 * ks + ko, ks, n_level, cap);
        hipLaunchKernelGGL(feat_describe_batch, dim3(cdiv(n_level, 4), n), dim3(256), 0, st, pyr + fa->goff[l], fa->pyr_stride, h, w,
                           l, fa->keys + s0 * ks + ko, cc + feat::CC * l, fa->cc_stride, fa->pattern, fa->trig,
                           fa->kp + (s0 * ks + ko) * 5, fa->desc + (s0 * ks + ko) * 8, ks);
        fa->launches += 4;
    }
    MI_HIP(hipGetLastError());
    return MI_OK;
}

}  // namespace

extern "C" {

int mi_feat_aligner_create(mi_feat_aligner_t* out, int device, int height, int width, int dtype, int channels, int subsample,
                           int fast, int levels, int n_features, int threshold, const int8_t* host_pattern, int max_batch) {
    if (!out) return fail(MI_ERR_INVALID, "null handle pointer");
    *out = nullptr;
    int rc = feat_shape_check(height, width);
    if (rc) return rc;
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16 for a feature frame (got %d)", dtype);
    if (channels != 1 && channels != 3) return fail(MI_ERR_INVALID, "channels must be 1 or 3 (got %d)", channels);
    if (subsample < 1 || subsample > 64) return fail(MI_ERR_INVALID, "subsample must be in [1, 64] (got %d)", subsample);
    if (!fast && subsample > 1 && (subsample != 2 || (height & 1) || (width & 1)))
        return fail(MI_ERR_INVALID, "fast must be set for subsample %d on a %dx%d frame: area sub-sampling is built for subsample 2 "
                    "on even sides", subsample, width, height);
    if (levels < 1 || levels > FEAT_MAX_LEVELS) return fail(MI_ERR_INVALID, "levels must be in [1, %d] (got %d)", FEAT_MAX_LEVELS, levels);
    if (n_features < 1 || n_features > FEAT_ALIGNER_MAX_FEATURES)
        return fail(MI_ERR_INVALID, "n_features must be in [1, %d] on a handle (got %d): a level's candidates are sorted in one "
                    "workgroup's LDS", FEAT_ALIGNER_MAX_FEATURES, n_features);
    if ((rc = feat_threshold_check(threshold))) return rc;
    if (!host_pattern) return fail(MI_ERR_INVALID, "null pattern");
    for (int i = 0; i < feat::BINS * feat::N_TESTS * 4; ++i)
        if (host_pattern[i] < -feat::BR || host_pattern[i] > feat::BR)
            return fail(MI_ERR_INVALID, "pattern[%d] must be within %d (got %d)", i, feat::BR, (int)host_pattern[i]);
    if (max_batch < 1 || max_batch > feat::MAX_BATCH)
        return fail(MI_ERR_INVALID, "max_batch must be in [1, %d] (got %d)", feat::MAX_BATCH, max_batch);
    if ((rc = open_device(device))) return rc;
    mi_feat_aligner* fa = new (std::nothrow) mi_feat_aligner();
    if (!fa) return fail(MI_ERR_NOMEM, "out of host memory");
    fa->device = device; fa->height = height; fa->width = width; fa->dtype = dtype; fa->channels = channels;
    fa->subsample = subsample; fa->fast = fast || subsample == 1; fa->levels = levels; fa->n_features = n_features;
    fa->threshold = threshold; fa->max_batch = max_batch;
    fa->gh = fa->fast ? (height + subsample - 1) / subsample : height / 2;
    fa->gw = fa->fast ? (width + subsample - 1) / subsample : width / 2;
    fa->trig = feat_trig();
    size_t pyr = 0;
    int h = fa->gh, w = fa->gw;
    for (int l = 0; l < levels; ++l) {
        if (l > 0) {
            if (h < 2 || w < 2) break;
            h /= 2;
            w /= 2;
        }
        fa->lh[l] = h; fa->lw[l] = w; fa->n_level[l] = n_features >> l;
        fa->scored[l] = fa->n_level[l] >= 1 && h >= 2 * feat::EDGE + 1 && w >= 2 * feat::EDGE + 1;
        fa->goff[l] = pyr;
        pyr += ((size_t)h * w + 255) & ~(size_t)255;
        fa->n_lv = l + 1;
    }
    fa->lv.n = levels;
    for (int l = 0; l < levels; ++l) {
        fa->lv.koff[l] = fa->total;
        fa->total += n_features >> l;
    }
    const size_t slots = (size_t)max_batch + 1, total = (size_t)fa->total, kmax = FEAT_ALIGNER_MAX_ITERS;
    size_t off = 0;
    auto carve = [&off](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    fa->pyr_stride = pyr;
    fa->score_stride = ((size_t)fa->gh * fa->gw + 255) & ~(size_t)255;
    fa->hist_stride = (size_t)levels * 256;
    fa->cc_stride = (size_t)levels * feat::CC;
    fa->mask_stride = (total + 255) & ~(size_t)255;
    const size_t o_pyr = carve(slots * fa->pyr_stride), o_score = carve(slots * fa->score_stride),
                 o_hist = carve(slots * fa->hist_stride * 4), o_cc = carve(slots * fa->cc_stride * 4),
                 o_keys = carve(slots * total * 8), o_kp = carve(slots * total * 20), o_desc = carve(slots * total * 32),
                 o_fwd = carve(slots * total * 12), o_back = carve(slots * total * 12), o_good = carve(slots * total * 12),
                 o_ngood = carve(slots * 4), o_src = carve(slots * total * 16), o_dst = carve(slots * total * 16),
                 o_samples = carve((size_t)max_batch * kmax * 16), o_counts = carve((size_t)max_batch * kmax * 4),
                 o_models = carve((size_t)max_batch * kmax * 72), o_head = carve(slots * 16), o_win = carve(slots * 72),
                 o_mask = carve(slots * fa->mask_stride), o_pattern = carve((size_t)feat::BINS * feat::N_TESTS * 4);
    bool ok = hipMalloc((void**)&fa->arena, off) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&fa->st, hipStreamNonBlocking) == hipSuccess;
    const size_t mb = (size_t)max_batch;
    ok = ok && hipHostMalloc((void**)&fa->h_n_good, mb * 4) == hipSuccess &&
         hipHostMalloc((void**)&fa->h_samples, mb * kmax * 16) == hipSuccess &&
         hipHostMalloc((void**)&fa->h_head, mb * 16) == hipSuccess && hipHostMalloc((void**)&fa->h_model, mb * 72) == hipSuccess &&
         hipHostMalloc((void**)&fa->h_src, mb * total * 16) == hipSuccess &&
         hipHostMalloc((void**)&fa->h_dst, mb * total * 16) == hipSuccess &&
         hipHostMalloc((void**)&fa->h_mask, mb * fa->mask_stride) == hipSuccess;
    if (ok) {
        uint8_t* a = fa->arena;
        fa->pyr = a + o_pyr; fa->score = a + o_score; fa->hist = (uint32_t*)(a + o_hist); fa->cc = (int32_t*)(a + o_cc);
        fa->keys = (unsigned long long*)(a + o_keys); fa->kp = (int32_t*)(a + o_kp); fa->desc = (uint32_t*)(a + o_desc);
        fa->fwd = (int32_t*)(a + o_fwd); fa->back = (int32_t*)(a + o_back); fa->good = (int32_t*)(a + o_good);
        fa->n_good = (int32_t*)(a + o_ngood); fa->src = (double*)(a + o_src); fa->dst = (double*)(a + o_dst);
        fa->samples = (int32_t*)(a + o_samples); fa->counts = (int32_t*)(a + o_counts); fa->models = (double*)(a + o_models);
        fa->head = (int32_t*)(a + o_head); fa->win_model = (double*)(a + o_win); fa->mask = a + o_mask;
        fa->pattern = (int8_t*)(a + o_pattern);
        ok = hipMemcpyAsync(fa->pattern, host_pattern, (size_t)feat::BINS * feat::N_TESTS * 4, hipMemcpyHostToDevice, fa->st) == hipSuccess &&
             hipStreamSynchronize(fa->st) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        feat_aligner_free(fa);
        delete fa;
        return fail(MI_ERR_NOMEM, "out of device memory");
    }
    *out = fa;
    return MI_OK;
}

int mi_feat_aligner_destroy(mi_feat_aligner_t fa) {
    if (!fa) return MI_OK;
    (void)hipSetDevice(fa->device);
    feat_aligner_free(fa);
    delete fa;
    return MI_OK;
}

int mi_feat_aligner_stats(mi_feat_aligner_t fa, uint64_t* waits, uint64_t* launches) {
    if (!fa) return fail(MI_ERR_INVALID, "null handle");
    if (!waits) return fail(MI_ERR_INVALID, "null waits");
    if (!launches) return fail(MI_ERR_INVALID, "null launches");
    *waits = fa->waits;
    *launches = fa->launches;
    return MI_OK;
}

int mi_feat_aligner_set_reference(mi_feat_aligner_t fa, const void* dev_ref) {
    if (!fa) return fail(MI_ERR_INVALID, "null handle");
    if (!dev_ref) return fail(MI_ERR_INVALID, "null reference frame");
    MI_HIP(hipSetDevice(fa->device));
    fa->have_ref = false;
    FeatFrames frames = {};
    frames.p[0] = dev_ref;
    int rc = feat_aligner_extract(fa, frames, 1, fa->max_batch);
    if (rc || (rc = feat_aligner_wait(fa))) return rc;
    fa->have_ref = true;
    return MI_OK;
}

int mi_feat_aligner_estimate_batch(mi_feat_aligner_t fa, const void* const* dev_movs, int n, int match_method, double ratio, int kind,
                                   double rans_threshold, int max_iters, uint64_t seed, int max_matches, int32_t* n_good,
                                   int32_t* winner, double* models, int32_t* inliers, uint8_t* mask, double* src, double* dst) {
    if (!fa) return fail(MI_ERR_INVALID, "null handle");
    if (!dev_movs) return fail(MI_ERR_INVALID, "null frame list");
    if (n < 1 || n > fa->max_batch) return fail(MI_ERR_INVALID, "n must be in [1, max_batch = %d] (got %d)", fa->max_batch, n);
    for (int i = 0; i < n; ++i)
        if (!dev_movs[i]) return fail(MI_ERR_INVALID, "null frame %d", i);
    if (match_method != MI_FEAT_MATCH_KNN && match_method != MI_FEAT_MATCH_HAMMING)
        return fail(MI_ERR_INVALID, "unknown match_method %d", match_method);
    if (!(ratio > 0.0) || !std::isfinite(ratio)) return fail(MI_ERR_INVALID, "ratio must be finite and > 0");
    if (kind != MI_FEAT_SIMILARITY && kind != MI_FEAT_HOMOGRAPHY) return fail(MI_ERR_INVALID, "unknown kind %d", kind);
    if (!(rans_threshold > 0.0) || !std::isfinite(rans_threshold)) return fail(MI_ERR_INVALID, "rans_threshold must be finite and > 0");
    if (max_iters < 1 || max_iters > FEAT_ALIGNER_MAX_ITERS)
        return fail(MI_ERR_INVALID, "max_iters must be in [1, %d] on a handle (got %d)", FEAT_ALIGNER_MAX_ITERS, max_iters);
    if (max_matches < fa->total)
        return fail(MI_ERR_INVALID, "max_matches must hold the sum of n_features >> level, %d (got %d)", fa->total, max_matches);
    if (!n_good) return fail(MI_ERR_INVALID, "null n_good");
    if (!winner) return fail(MI_ERR_INVALID, "null winner");
    if (!models) return fail(MI_ERR_INVALID, "null models");
    if (!inliers) return fail(MI_ERR_INVALID, "null inliers");
    if (!mask) return fail(MI_ERR_INVALID, "null mask");
    if (!src) return fail(MI_ERR_INVALID, "null src");
    if (!dst) return fail(MI_ERR_INVALID, "null dst");
    if (!fa->have_ref) return fail(MI_ERR_STATE, "mi_feat_aligner_set_reference has not been called");
    MI_HIP(hipSetDevice(fa->device));
    hipStream_t st = fa->st;
    fa->last_n = 0;
    FeatFrames frames = {};
    for (int i = 0; i < n; ++i) frames.p[i] = dev_movs[i];
    int rc = feat_aligner_extract(fa, frames, n, 0);
    if (rc) return rc;
    const size_t ks = (size_t)fa->total, ref = (size_t)fa->max_batch;
    const int32_t* ref_cc = fa->cc + ref * fa->cc_stride;
    for (int l = 0; l < fa->n_lv; ++l) {
        if (!fa->scored[l]) continue;
        const size_t ko = (size_t)fa->lv.koff[l];
        const dim3 grid(cdiv(fa->n_level[l], feat::MATCH_NT), n);
        const unsigned long long* mov_desc = (const unsigned long long*)(fa->desc + ko * 8);
        const unsigned long long* ref_desc = (const unsigned long long*)(fa->desc + (ref * ks + ko) * 8);
        hipLaunchKernelGGL(feat_match_batch, grid, dim3(feat::MATCH_NT), 0, st, mov_desc, ks * 4, fa->cc + feat::CC * l, fa->cc_stride,
                           ref_desc, (size_t)0, ref_cc + feat::CC * l, (size_t)0, fa->fwd + ko * 3, ks * 3);
        ++fa->launches;
        if (match_method == MI_FEAT_MATCH_HAMMING) {
            hipLaunchKernelGGL(feat_match_batch, grid, dim3(feat::MATCH_NT), 0, st, ref_desc, (size_t)0, ref_cc + feat::CC * l, (size_t)0,
                               mov_desc, ks * 4, fa->cc + feat::CC * l, fa->cc_stride, fa->back + ko * 3, ks * 3);
            ++fa->launches;
        }
    }
    hipLaunchKernelGGL(feat_good, dim3(n), dim3(feat::SORT_NT), 0, st, fa->lv, fa->cc, fa->cc_stride, ref_cc, fa->fwd, fa->back, fa->kp,
                       fa->kp + ref * ks * 5, ks, match_method, ratio, fa->good, fa->n_good, fa->src, fa->dst);
    ++fa->launches;
    MI_HIP(hipMemcpyAsync(fa->h_n_good, fa->n_good, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if ((rc = feat_aligner_wait(fa))) return rc;                                         // wait 1: the good-match counts
    const int ns = kind == MI_FEAT_HOMOGRAPHY ? 4 : 2, need = kind == MI_FEAT_HOMOGRAPHY ? 4 : 3, k = max_iters;
    int most = 0;
    for (int f = 0; f < n; ++f) {
        const int g = fa->h_n_good[f];
        most = std::max(most, g);
        int32_t* table = fa->h_samples + (size_t)f * k * ns;
        if (g >= need) feat_sample_table(g, k, ns, seed, table);
        else std::fill(table, table + (size_t)k * ns, 0);
    }
    MI_HIP(hipMemcpyAsync(fa->samples, fa->h_samples, (size_t)n * k * ns * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MI_HIP(hipMemsetAsync(fa->counts, 0xFF, (size_t)n * k * sizeof(int32_t), st));      // -1: a pair that is not evaluated
    hipLaunchKernelGGL(feat_ransac_batch, dim3(cdiv(k, 4), n), dim3(feat::RANSAC_NT), 0, st, fa->src, fa->dst, ks, fa->n_good, need,
                       fa->samples, k, kind, rans_threshold, fa->counts, fa->models);
    hipLaunchKernelGGL(feat_pick, dim3(n), dim3(256), 0, st, fa->n_good, need, fa->counts, fa->models, k, kind, rans_threshold, fa->src,
                       fa->dst, ks, fa->head, fa->win_model, fa->mask, fa->mask_stride);
    fa->launches += 2;
    MI_HIP(hipMemcpyAsync(fa->h_head, fa->head, (size_t)n * 16, hipMemcpyDeviceToHost, st));
    MI_HIP(hipMemcpyAsync(fa->h_model, fa->win_model, (size_t)n * 72, hipMemcpyDeviceToHost, st));
    if (most > 0) {
        MI_HIP(hipMemcpy2DAsync(fa->h_mask, fa->mask_stride, fa->mask, fa->mask_stride, (size_t)most, n, hipMemcpyDeviceToHost, st));
        MI_HIP(hipMemcpy2DAsync(fa->h_src, ks * 16, fa->src, ks * 16, (size_t)most * 16, n, hipMemcpyDeviceToHost, st));
        MI_HIP(hipMemcpy2DAsync(fa->h_dst, ks * 16, fa->dst, ks * 16, (size_t)most * 16, n, hipMemcpyDeviceToHost, st));
    }
    if ((rc = feat_aligner_wait(fa))) return rc;                                         // wait 2: the results
    for (int f = 0; f < n; ++f) {
        const int g = fa->h_n_good[f];
        n_good[f] = g;
        winner[f] = fa->h_head[4 * f];
        inliers[f] = fa->h_head[4 * f + 1];
        std::copy(fa->h_model + 9 * f, fa->h_model + 9 * f + 9, models + 9 * (size_t)f);
        std::copy(fa->h_mask + f * fa->mask_stride, fa->h_mask + f * fa->mask_stride + g, mask + (size_t)f * max_matches);
        std::copy(fa->h_src + f * ks * 2, fa->h_src + f * ks * 2 + 2 * (size_t)g, src + 2 * (size_t)f * max_matches);
        std::copy(fa->h_dst + f * ks * 2, fa->h_dst + f * ks * 2 + 2 * (size_t)g, dst + 2 * (size_t)f * max_matches);
    }
    fa->last_n = n; fa->last_k = k; fa->last_ns = ns;
    return MI_OK;
}

int mi_feat_aligner_tap(mi_feat_aligner_t fa, int frame_slot, int what, int level, void* host_out, size_t capacity, int* n_out) {
    if (!fa) return fail(MI_ERR_INVALID, "null handle");
    if (what < MI_FEAT_TAP_GRAY || what > MI_FEAT_TAP_COUNTS) return fail(MI_ERR_INVALID, "unknown tap %d", what);
    const bool is_ref = frame_slot == -1;
    if (is_ref && what > MI_FEAT_TAP_DESC) return fail(MI_ERR_INVALID, "frame_slot -1 (the reference) has no tap %d: it has the stages up to the descriptors", what);
    if (!is_ref && (frame_slot < 0 || frame_slot >= fa->max_batch))
        return fail(MI_ERR_INVALID, "frame_slot must be -1 or in [0, max_batch = %d) (got %d)", fa->max_batch, frame_slot);
    if (what == MI_FEAT_TAP_GRAY && (level < 0 || level >= fa->n_lv))
        return fail(MI_ERR_INVALID, "level must be in [0, %d) (got %d)", fa->n_lv, level);
    if (!host_out) return fail(MI_ERR_INVALID, "null output");
    if (!n_out) return fail(MI_ERR_INVALID, "null n_out");
    if (is_ref && !fa->have_ref) return fail(MI_ERR_STATE, "mi_feat_aligner_set_reference has not been called");
    if (!is_ref && frame_slot >= fa->last_n)
        return fail(MI_ERR_STATE, "frame_slot %d is not part of the last batch (%d frames)", frame_slot, fa->last_n);
    MI_HIP(hipSetDevice(fa->device));
    const size_t s = is_ref ? (size_t)fa->max_batch : (size_t)frame_slot, ks = (size_t)fa->total;
    hipStream_t st = fa->st;
    int rc;
    auto fetch = [&](void* to, const void* from, size_t bytes) -> int {
        if (!bytes) return MI_OK;
        MI_HIP(hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToHost, st));
        return feat_aligner_wait(fa);
    };
    if (what == MI_FEAT_TAP_GRAY) {
        const size_t bytes = (size_t)fa->lh[level] * fa->lw[level];
        if (capacity < bytes) return fail(MI_ERR_INVALID, "capacity must be at least %zu bytes (got %zu)", bytes, capacity);
        *n_out = fa->lh[level];
        return fetch(host_out, fa->pyr + s * fa->pyr_stride + fa->goff[level], bytes);
    }
    std::vector<int32_t> cc(fa->cc_stride);
    if ((rc = fetch(cc.data(), fa->cc + s * fa->cc_stride, fa->cc_stride * sizeof(int32_t)))) return rc;
    if (what == MI_FEAT_TAP_CUT) {
        const size_t bytes = fa->cc_stride * sizeof(int32_t);
        if (capacity < bytes) return fail(MI_ERR_INVALID, "capacity must be at least %zu bytes (got %zu)", bytes, capacity);
        std::copy(cc.begin(), cc.end(), (int32_t*)host_out);
        *n_out = fa->levels;
        return MI_OK;
    }
    if (what == MI_FEAT_TAP_KP || what == MI_FEAT_TAP_DESC) {
        const size_t row = what == MI_FEAT_TAP_KP ? 20 : 32;
        size_t found = 0;
        for (int l = 0; l < fa->levels; ++l) found += (size_t)cc[feat::CC * l + 2];
        if (capacity < found * row) return fail(MI_ERR_INVALID, "capacity must be at least %zu bytes (got %zu)", found * row, capacity);
        const uint8_t* base = what == MI_FEAT_TAP_KP ? (const uint8_t*)(fa->kp + s * ks * 5) : (const uint8_t*)(fa->desc + s * ks * 8);
        size_t at = 0;
        for (int l = 0; l < fa->levels; ++l) {       // the levels follow each other in the output, as mi_feat_extract leaves them
            const size_t c = (size_t)cc[feat::CC * l + 2];
            if (c) MI_HIP(hipMemcpyAsync((uint8_t*)host_out + at * row, base + (size_t)fa->lv.koff[l] * row, c * row, hipMemcpyDeviceToHost, st));
            at += c;
        }
        *n_out = (int)found;
        return feat_aligner_wait(fa);
    }
    if (what == MI_FEAT_TAP_GOOD) {
        int32_t g = 0;
        if ((rc = fetch(&g, fa->n_good + s, sizeof g))) return rc;
        if (capacity < (size_t)g * 12) return fail(MI_ERR_INVALID, "capacity must be at least %zu bytes (got %zu)", (size_t)g * 12, capacity);
        *n_out = g;
        return fetch(host_out, fa->good + s * ks * 3, (size_t)g * 12);
    }
    const size_t row = what == MI_FEAT_TAP_SAMPLES ? (size_t)fa->last_ns * 4 : 4, bytes = (size_t)fa->last_k * row;
    if (capacity < bytes) return fail(MI_ERR_INVALID, "capacity must be at least %zu bytes (got %zu)", bytes, capacity);
    *n_out = fa->last_k;
    if (what == MI_FEAT_TAP_SAMPLES) return fetch(host_out, fa->samples + s * (size_t)fa->last_k * fa->last_ns, bytes);
    return fetch(host_out, fa->counts + s * (size_t)fa->last_k, bytes);
}

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
