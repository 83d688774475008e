// mosaic_host.hpp -- the mosaic stage of a stack handle: a host frame arrives raw -- as a Bayer mosaic (a third of the bytes of a
// BGR frame over the host link) or as the packed sample bytes of a raw file (0.75 of a uint16 mosaic's bytes at 12 bits) -- and
// becomes a BGR frame on the device.  Included by capi.hip after tiled_host.hpp; nothing of it exists until a handle's first raw
// push or mi_stack_set_site_correction.  Every raw entry point of capi.hip describes its frame as one MosaicFrame and hands it to
// mosaic_push, which has one path:
//
//   upload      on stc, the stage's copy stream (the low priority class, as the ring's copy stream and for its reason), into
//               device slot k % NSLOT, then evCopied[slot]; uploads run ahead of the kernels by NSLOT frames.  A mosaic goes
//               into slot[slot].  A packed span goes into pslot[slot], laid out [span | segment offsets or lossless-JPEG
//               descriptors | table], the part behind the span out of the pinned meta[slot].  With site corrections set
//               (mi_stack_set_site_correction: the setter copies every table into one pinned block, laid out as it will lie
//               on the device) the block goes up into cslot[slot] ahead of both.  Pinned sources are read in place (evUp, for
//               mi_stack_wait_uploads); pageable ones go through a ring of pinned bounce buffers (PinRing, copy_rows).
//   kernels     frame_kernels, on s->stream behind evCopied[slot], into frame `pending` of `bgr`: raw_unpack or raw_ljpeg
//               (packed spans; the latter ORs every segment's status flags into `ljstatus`, which mi_stack_ljpeg_status reads
//               and clears; with mi_stack_set_ljpeg_split the split path's kernels stand in for raw_ljpeg and share ONE scratch
//               of the stage, which is safe because all of them run here, in order), the bad-site kernels and mosaic_site_correct (site corrections), calibration, the defect kernel,
//               the (developed) demosaic -- all but the last in place on slot[slot].  evSlotFree[slot] follows them, and the
//               copy stream waits for it before it overwrites any of the slot's buffers.  The kernels are a twelfth of the
//               copy's time; on the copy stream they would run in the low class behind another handle's level kernels and
//               hold the next upload back (measured: docs/studies.md, "raw mosaics").  On s->stream they need no stream of
//               their own -- the handle stays inside its four hardware queues -- and are in order with the batch that reads
//               their output.  The caller's device tables (tone, sites, dark frame, gains) are read by those kernels.
//   bgr         bcap BGR frames -- what the ring is for host BGR frames.  A full buffer, or a flush, hands it to dispatch_push
//               as one batch: the level-0 interior kernel follows the demosaics on s->stream, run_batch's evInput carries them
//               to the border stream, and tiled_push joins the side streams back into s->stream, so the next demosaic into
//               `bgr` is ordered behind every reader of the batch.
//   growing     pslot, meta, cslot and the span bounce ring belong to the stage (not to s->allocs) and grow when a later frame
//               needs more (set_realloc), after a wait for whatever reads them: the device slots for both streams, the pinned
//               blocks for stc.
//   linear      a linear frame (mi_stack_push_linear: MosaicFrame::lin in place of the cfa) is a packed span whose layout counts
//               SAMPLES, spp of them per pixel.  Its span goes into pslot[slot] as any span does; raw_unpack, raw_ljpeg or
//               raw_ljpeg3 write H x W x spp samples -- into lslot[slot], never into slot[slot], which holds H x W and is
//               allocated once -- and linear_develop takes them to the frame in `bgr`; nothing runs per site.  lslot belongs to
//               the stage and grows as pslot does (linear_reserve), shares the slot index and both events with the mosaic slots,
//               and is written by kernels of s->stream only, which are in order: no further ordering is needed.
//   float-64 and MI_IMPL_SIMPLE handles
//               one slot, no copy stream: upload, frame_kernels, dispatch_push and a wait, one frame at a time on s->stream.
//   order       frames are fused in call order: the first raw frame after host BGR frames flushes the ring (mosaic_push), and
//               every call that takes frames of another kind or reads state flushes this stage first (stack_flush in capi.hip).
#pragma once

#include "kernels_calib.hpp"
#include "kernels_demosaic.hpp"
#include "kernels_linear.hpp"
#include "kernels_ljpeg.hpp"
#include "kernels_ljpeg_split.hpp"
#include "kernels_sitecorr.hpp"
#include "kernels_unpack.hpp"

namespace mi {

// free the `n` buffers of a set and allocate them again with `bytes` each, in device memory or (`pinned`) in pinned host memory.
// The caller has waited for whatever reads them.  A failure leaves capacity 0 and the buffer that failed null.
inline int set_realloc(void** buf, int n, size_t* cap, size_t bytes, bool pinned) {
    for (int i = 0; i < n; ++i) {
        if (buf[i]) (void)(pinned ? hipHostFree(buf[i]) : hipFree(buf[i]));
        buf[i] = nullptr;
    }
    *cap = 0;
    for (int i = 0; i < n; ++i) {
        if (pinned) MI_HIP(hipHostMalloc(&buf[i], bytes, hipHostMallocDefault));
        else if (hipMalloc(&buf[i], bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(MI_ERR_NOMEM, "out of device memory");
        }
    }
    *cap = bytes;
    return MI_OK;
}

// a ring of pinned bounce buffers for sources in pageable memory, each with the event of the upload out of it
struct PinRing {
    static constexpr int N = 3;
    void* buf[N] = {};
    hipEvent_t ev[N] = {};
    size_t cap = 0;
    long no = 0;
};
inline int pin_reserve(PinRing& r, size_t bytes) {
    int rc = set_realloc(r.buf, PinRing::N, &r.cap, bytes, true);
    for (int i = 0; !rc && i < PinRing::N; ++i)
        if (!r.ev[i]) MI_HIP(hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming));
    return rc;
}
inline void pin_destroy(PinRing& r) {
    for (int i = 0; i < PinRing::N; ++i) {
        if (r.buf[i]) (void)hipHostFree(r.buf[i]);
        if (r.ev[i]) (void)hipEventDestroy(r.ev[i]);
    }
}
// `rows` rows of `row_bytes` (a span: one row) through the ring's next buffer into `dst` on `stc`; the caller's memory is free
// again on return
inline int pin_upload(PinRing& r, hipStream_t stc, void* dst, const void* src, size_t src_stride, size_t row_bytes, size_t rows) {
    const int k = (int)(r.no++ % PinRing::N);
    MI_HIP(hipEventSynchronize(r.ev[k]));   // bounce buffer free again? (no-op when unused)
    copy_rows(r.buf[k], src, src_stride, row_bytes, rows, copy_threads(row_bytes * rows));
    MI_HIP(hipMemcpyAsync(dst, r.buf[k], row_bytes * rows, hipMemcpyHostToDevice, stc));
    MI_HIP(hipEventRecord(r.ev[k], stc));
    return MI_OK;
}

struct MosaicStage {
    static constexpr int NSLOT = 4;
    static constexpr int NUP = MI_NUP;
    hipStream_t stc = nullptr;                // copy stream
    void* slot[NSLOT] = {};                   // H x W mosaics on the device
    hipEvent_t evCopied[NSLOT] = {};          // the upload into slot[i] finished
    hipEvent_t evSlotFree[NSLOT] = {};        // the demosaic out of slot[i] finished
    void* bgr = nullptr;                      // bcap BGR frames
    PinRing pin;                              // bounce buffers of mosaics that are not pinned
    hipEvent_t evUp[NUP] = {};                // pinned mosaics: one event per upload, for mi_stack_wait_uploads
    size_t mosaic_bytes = 0;
    int pending = 0;                          // frames demosaiced (or being) into `bgr`, not yet handed over
    long slot_no = 0, up_no = 0;
    long frames_up_seen = 0;                  // TiledState::up_no at the most recent pinned mosaic
    long run = 0;                             // pinned mosaics since the most recent pinned BGR frame
    // packed spans (mi_stack_push_packed)
    void* pslot[NSLOT] = {};                  // [span | segment offsets | table] on the device, each part 256-byte aligned
    size_t pslot_cap = 0;
    void* meta[NSLOT] = {};                   // pinned: the offsets and the table that go with pslot[i]
    size_t meta_cap = 0;
    PinRing ppin;                             // bounce buffers of spans that are not pinned
    uint32_t* ljstatus = nullptr;             // lossless-JPEG spans: every frame's status flags ORed (in s->allocs)
    // the split path (mi_stack_set_ljpeg_split): one scratch for every frame -- the decode kernels of all frames run in order on
    // s->stream --, owned by the stage and grown on demand; lj_rounds is the frame's exact bound, from its host descriptors
    bool lj_split = false;
    uint32_t lj_sub = 0, lj_rounds = 0;
    void* lj_scratch = nullptr;
    size_t lj_scratch_cap = 0;
    // linear frames (mi_stack_push_linear): the unpacked H x W x spp samples; they belong to the stage and grow as pslot does
    void* lslot[NSLOT] = {};
    size_t lslot_cap = 0;
    // site corrections (mi_stack_set_site_correction)
    bool sc_on = false;
    mi_site_correct_t sc = {};                // its pointers hold OFFSETS into the block
    void* sc_host = nullptr;                  // pinned: every table, each part 256-byte aligned
    size_t sc_bytes = 0, sc_host_cap = 0;
    void* cslot[NSLOT] = {};                  // the block on the device, one per mosaic slot
    size_t cslot_cap = 0;
    unsigned long long* sc_bits = nullptr;    // the constant repair's bit plane (in s->allocs; kernels of one stream share it)
    int64_t sc_dmin[4] = {}, sc_dmax[4] = {}; // per position, the range of delta_h[x] + delta_v[y]
};

// what mi_stack_push_packed brings in place of a mosaic (arguments checked by the caller)
struct PackedSrc {
    const void* span;
    size_t span_bytes;
    const uint32_t* seg;        // host: the segment offsets, or null ...
    const mi_ljpeg_seg_t* ljseg;    // ... when the span is lossless JPEG: host, one descriptor per segment
    int nseg;
    const mi_raw_layout_t* layout;
    const uint16_t* table;      // host, layout->table_len entries, or null
    const mi_ljpeg_seg3_t* ljseg3 = nullptr;   // ... or its three-component descriptors (a linear frame of three samples)
};
inline size_t packed_align(size_t n) { return (n + 255) & ~(size_t)255; }
inline const void* packed_seg(const PackedSrc& pk) {
    return pk.ljseg3 ? (const void*)pk.ljseg3 : pk.ljseg ? (const void*)pk.ljseg : (const void*)pk.seg;
}
inline size_t packed_seg_bytes(const PackedSrc& pk) {
    return (size_t)pk.nseg * (pk.ljseg3 ? sizeof(mi_ljpeg_seg3_t) : pk.ljseg ? sizeof(mi_ljpeg_seg_t) : sizeof(uint32_t));
}

inline MosaicStage* mstage(const mi_stack* s) { return reinterpret_cast<MosaicStage*>(s->mosaic); }

inline int mosaic_pending(const mi_stack* s) { return mstage(s) ? mstage(s)->pending : 0; }

// argument checks shared by mi_demosaic, mi_demosaic_device and mi_stack_push_mosaic: no device call
inline int cfa_check(const mi_cfa_t* cfa, int dtype) {
    if (!cfa) return fail(MI_ERR_INVALID, "null cfa");
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16 for a mosaic (got %d)", dtype);
    if (cfa->pattern < MI_CFA_RGGB || cfa->pattern > MI_CFA_GBRG) return fail(MI_ERR_INVALID, "unknown cfa pattern %d", cfa->pattern);
    const int maxv = dtype == MI_U8 ? 255 : 65535;
    for (int k = 0; k < 4; ++k) {
        if (cfa->black[k] < 0) return fail(MI_ERR_INVALID, "cfa black[%d] must be >= 0 (got %d)", k, cfa->black[k]);
        if (cfa->gain_q[k] > 65535u) return fail(MI_ERR_INVALID, "cfa gain_q[%d] must be <= 65535 (got %u)", k, cfa->gain_q[k]);
    }
    if (cfa->white < 1 || cfa->white > maxv) return fail(MI_ERR_INVALID, "cfa white must be in [1, %d] (got %d)", maxv, cfa->white);
    return MI_OK;
}

// argument checks of the development entry points (mi_develop*, mi_mosaic_defects_device, mi_stack_push_mosaic_developed):
// no device call.  The kernel accumulates step C in int32: that holds while a row's sum of |matrix_q| is at most 32767.
inline int matrix_check(const int32_t* matrix_q) {
    for (int i = 0; i < 3; ++i) {
        int64_t sum = 0;
        for (int j = 0; j < 3; ++j) sum += std::llabs((long long)matrix_q[3 * i + j]);
        if (sum > 32767) return fail(MI_ERR_INVALID, "matrix_q row %d: the sum of |entries| must be <= 32767 (got %lld)", i, (long long)sum);
    }
    return MI_OK;
}
inline int develop_check(const mi_develop_t* d) {
    if (!d) return fail(MI_ERR_INVALID, "null develop");
    if (d->flags & ~(MI_DEVELOP_MATRIX | MI_DEVELOP_TONE)) return fail(MI_ERR_INVALID, "unknown develop flags %d", d->flags);
    if ((d->flags & MI_DEVELOP_TONE) && !d->dev_tone) return fail(MI_ERR_INVALID, "develop: MI_DEVELOP_TONE is set and dev_tone is null");
    if (d->flags & MI_DEVELOP_MATRIX) return matrix_check(d->matrix_q);
    return MI_OK;
}
inline int sites_check(const int32_t* sites, int n, int height, int width) {
    if (n < 0) return fail(MI_ERR_INVALID, "the number of sites must be >= 0 (got %d)", n);
    if (n > 0 && !sites) return fail(MI_ERR_INVALID, "null sites");
    if (height > 0 && width > 0 && (uint64_t)height * (uint64_t)width >= (1ull << 31)) return fail(MI_ERR_INVALID, "height x width too large");
    return MI_OK;
}
// argument checks of the calibration entry points (mi_mosaic_master*, mi_flat_gain*, mi_mosaic_calibrate*,
// mi_stack_push_mosaic_calibrated): no device call.  The kernels index sites with 31 bits, as the defect list does, and the
// flat's 64-bit sums hold under the same bound (kernels_calib.hpp).
inline int calib_shape_check(int height, int width, int dtype) {
    if (height < 2 || width < 2) return fail(MI_ERR_INVALID, "height and width must be >= 2 for a mosaic (got %dx%d)", width, height);
    if (dtype != MI_U8 && dtype != MI_U16) return fail(MI_ERR_INVALID, "dtype must be MI_U8 or MI_U16 for a mosaic (got %d)", dtype);
    if ((uint64_t)height * (uint64_t)width >= (1ull << 31)) return fail(MI_ERR_INVALID, "height x width too large");
    return MI_OK;
}
inline int master_check(int n, int reject) {
    if (n < 1 || n > calib::MAX_FRAMES) return fail(MI_ERR_INVALID, "the number of frames must be in [1, %d] (got %d)", calib::MAX_FRAMES, n);
    if (reject < 0 || 2 * (int64_t)reject >= n) return fail(MI_ERR_INVALID, "reject must be >= 0 with 2 * reject < n (got %d, n = %d)", reject, n);
    return MI_OK;
}
inline int calib_check(const mi_calib_t* c) {
    if (!c) return fail(MI_ERR_INVALID, "null calib");
    if (c->flags & ~(MI_CALIB_DARK | MI_CALIB_FLAT)) return fail(MI_ERR_INVALID, "unknown calib flags %d", c->flags);
    if ((c->flags & MI_CALIB_DARK) && !c->dev_dark) return fail(MI_ERR_INVALID, "calib: MI_CALIB_DARK is set and dev_dark is null");
    if ((c->flags & MI_CALIB_FLAT) && !c->dev_gain) return fail(MI_ERR_INVALID, "calib: MI_CALIB_FLAT is set and dev_gain is null");
    return MI_OK;
}
// a list in host memory: every site inside the image, strictly ascending
inline int host_sites_check(const int32_t* sites, int n, int height, int width) {
    const int64_t npx = (int64_t)height * width;
    for (int i = 0; i < n; ++i) {
        if (sites[i] < 0 || sites[i] >= npx) return fail(MI_ERR_INVALID, "sites[%d] = %d lies outside the %d x %d image", i, sites[i], width, height);
        if (i && sites[i] <= sites[i - 1]) return fail(MI_ERR_INVALID, "sites must be strictly ascending (sites[%d] = %d follows %d)", i, sites[i], sites[i - 1]);
    }
    return MI_OK;
}

// argument checks of the site-correction entry points (mi_mosaic_site_correct*, mi_stack_set_site_correction): no device call,
// no table is read
inline int site_check(const mi_site_correct_t* c, int dtype, bool need_scratch = false) {
    if (!c) return fail(MI_ERR_INVALID, "null site correction");
    const int all = MI_SITE_DELTA_H | MI_SITE_DELTA_V | MI_SITE_GAIN | MI_SITE_BAD_LIST | MI_SITE_BAD_CONST;
    if (c->flags & ~all) return fail(MI_ERR_INVALID, "unknown site correction flags %d", c->flags);
    if ((c->flags & MI_SITE_DELTA_H) && !c->delta_h) return fail(MI_ERR_INVALID, "site correction: MI_SITE_DELTA_H is set and delta_h is null");
    if ((c->flags & MI_SITE_DELTA_V) && !c->delta_v) return fail(MI_ERR_INVALID, "site correction: MI_SITE_DELTA_V is set and delta_v is null");
    if (c->flags & MI_SITE_GAIN) {
        int maps = 0;
        for (int p = 0; p < 4; ++p) {
            const mi_site_gain_t& g = c->gain[p];
            if (!g.nodes) continue;
            ++maps;
            if (!g.row_axis) return fail(MI_ERR_INVALID, "site correction: gain[%d] has nodes and row_axis is null", p);
            if (!g.col_axis) return fail(MI_ERR_INVALID, "site correction: gain[%d] has nodes and col_axis is null", p);
            if (g.mv < 1 || g.mv > sitecorr::MAX_NODES) return fail(MI_ERR_INVALID, "site correction: gain[%d].mv must be in [1, %d] (got %d)", p, sitecorr::MAX_NODES, g.mv);
            if (g.mh < 1 || g.mh > sitecorr::MAX_NODES) return fail(MI_ERR_INVALID, "site correction: gain[%d].mh must be in [1, %d] (got %d)", p, sitecorr::MAX_NODES, g.mh);
        }
        if (!maps) return fail(MI_ERR_INVALID, "site correction: MI_SITE_GAIN is set and every gain[].nodes is null");
    }
    if (c->flags & MI_SITE_BAD_LIST) {
        if (c->n_bad < 0) return fail(MI_ERR_INVALID, "site correction: n_bad must be >= 0 (got %d)", c->n_bad);
        if (c->n_bad > 0 && !c->bad_sites) return fail(MI_ERR_INVALID, "site correction: MI_SITE_BAD_LIST is set and bad_sites is null");
    }
    if (c->flags & MI_SITE_BAD_CONST) {
        const int maxv = dtype == MI_U8 ? 255 : 65535;
        if (c->bad_constant < 0 || c->bad_constant > maxv) return fail(MI_ERR_INVALID, "site correction: bad_constant must be in [0, %d] (got %d)", maxv, c->bad_constant);
        if (c->bad_phase_mask < 1 || c->bad_phase_mask > 15) return fail(MI_ERR_INVALID, "site correction: bad_phase_mask must be in [1, 15] (got %d)", c->bad_phase_mask);
        if (need_scratch && !c->dev_scratch) return fail(MI_ERR_INVALID, "site correction: MI_SITE_BAD_CONST is set and dev_scratch is null");
    }
    return MI_OK;
}
// tables in host memory: weights, node indices, the bad-site list; dmin / dmax receive, per position, the range of
// delta_h[x] + delta_v[y] over the position's sites
inline int site_host_check(const mi_site_correct_t* c, int height, int width, int64_t* dmin, int64_t* dmax) {
    int64_t hlo[2] = {0, 0}, hhi[2] = {0, 0}, vlo[2] = {0, 0}, vhi[2] = {0, 0};
    if (c->flags & MI_SITE_DELTA_H)
        for (int px = 0; px < 2; ++px) {
            hlo[px] = 32767; hhi[px] = -32768;
            for (int x = px; x < width; x += 2) { hlo[px] = std::min<int64_t>(hlo[px], c->delta_h[x]); hhi[px] = std::max<int64_t>(hhi[px], c->delta_h[x]); }
        }
    if (c->flags & MI_SITE_DELTA_V)
        for (int py = 0; py < 2; ++py) {
            vlo[py] = 32767; vhi[py] = -32768;
            for (int y = py; y < height; y += 2) { vlo[py] = std::min<int64_t>(vlo[py], c->delta_v[y]); vhi[py] = std::max<int64_t>(vhi[py], c->delta_v[y]); }
        }
    for (int p = 0; p < 4; ++p) { dmin[p] = hlo[p & 1] + vlo[p >> 1]; dmax[p] = hhi[p & 1] + vhi[p >> 1]; }
    if (c->flags & MI_SITE_GAIN)
        for (int p = 0; p < 4; ++p) {
            const mi_site_gain_t& g = c->gain[p];
            if (!g.nodes) continue;
            for (int y = p >> 1; y < height; y += 2) {
                if (g.row_axis[y].weight > sitecorr::MAX_WEIGHT) return fail(MI_ERR_INVALID, "site correction: gain[%d].row_axis[%d].weight must be <= 256 (got %d)", p, y, g.row_axis[y].weight);
                if (g.row_axis[y].node >= g.mv) return fail(MI_ERR_INVALID, "site correction: gain[%d].row_axis[%d].node = %d lies outside the %d rows of its grid", p, y, g.row_axis[y].node, g.mv);
            }
            for (int x = p & 1; x < width; x += 2) {
                if (g.col_axis[x].weight > sitecorr::MAX_WEIGHT) return fail(MI_ERR_INVALID, "site correction: gain[%d].col_axis[%d].weight must be <= 256 (got %d)", p, x, g.col_axis[x].weight);
                if (g.col_axis[x].node >= g.mh) return fail(MI_ERR_INVALID, "site correction: gain[%d].col_axis[%d].node = %d lies outside the %d columns of its grid", p, x, g.col_axis[x].node, g.mh);
            }
        }
    if (c->flags & MI_SITE_BAD_LIST) return host_sites_check(c->bad_sites, c->n_bad, height, width);
    return MI_OK;
}
// b = black[pos] + delta_h[x] + delta_v[y] inside [0, maxv] for every site
inline int site_black_check(const int32_t* black, const int64_t* dmin, const int64_t* dmax, int dtype) {
    const int maxv = dtype == MI_U8 ? 255 : 65535;
    for (int p = 0; p < 4; ++p)
        if (black[p] + dmin[p] < 0 || black[p] + dmax[p] > maxv)
            return fail(MI_ERR_INVALID, "site correction: black[%d] + delta_h + delta_v must stay inside [0, %d] (it spans %lld .. %lld)", p, maxv,
                        (long long)(black[p] + dmin[p]), (long long)(black[p] + dmax[p]));
    return MI_OK;
}

// the site-correction kernels of one mosaic, in place (arguments checked by the caller); `bits`: the constant repair's scratch
inline void site_kernels(hipStream_t st, void* mosaic, int H, int W, int dtype, const mi_cfa_t& cfa, const mi_site_correct_t& c,
                         unsigned long long* bits) {
    if (c.flags & MI_SITE_BAD_LIST) defects_launch(st, mosaic, H, W, dtype, c.bad_sites, c.n_bad);
    if (c.flags & MI_SITE_BAD_CONST) defects_const_launch(st, mosaic, H, W, dtype, c.bad_constant, c.bad_phase_mask, bits);
    site_correct_launch(st, mosaic, H, W, dtype, cfa, c);
}

inline int mosaic_create(mi_stack* s) {
    auto* m = new MosaicStage();
    s->mosaic = m;
    const TiledState* t = tstate(s);
    m->mosaic_bytes = (size_t)s->p.height * s->p.width * dtype_size(s->p.in_dtype);
    int rc;
    if (s->p.impl != MI_IMPL_TILED) return dev_alloc(s, &m->slot[0], m->mosaic_bytes);   // the synchronous route: one slot
    // the copy stream's priority class, for the reason tiled_push_host gives: the low one
    int prio_lo = 0, prio_hi = 0;
    MI_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    MI_HIP(hipStreamCreateWithPriority(&m->stc, hipStreamNonBlocking, prio_lo));
    for (int i = 0; i < MosaicStage::NSLOT; ++i) {
        MI_HIP(hipEventCreateWithFlags(&m->evCopied[i], hipEventDisableTiming));
        MI_HIP(hipEventCreateWithFlags(&m->evSlotFree[i], hipEventDisableTiming));
        if ((rc = dev_alloc(s, &m->slot[i], m->mosaic_bytes))) return rc;
    }
    return dev_alloc(s, &m->bgr, t->frame_bytes * t->bcap);
}

inline int mosaic_sync(mi_stack* s) {
    MosaicStage* m = mstage(s);
    if (m && m->stc) MI_HIP(hipStreamSynchronize(m->stc));
    return MI_OK;
}

inline void mosaic_destroy(mi_stack* s) {
    MosaicStage* m = mstage(s);
    if (!m) return;
    if (m->stc) (void)hipStreamSynchronize(m->stc);
    pin_destroy(m->pin);
    pin_destroy(m->ppin);
    if (m->pslot[0]) (void)hipStreamSynchronize(s->stream);   // (the unpack kernels read the packed slots, and write the linear ones)
    for (int i = 0; i < MosaicStage::NSLOT; ++i) {
        if (m->meta[i]) (void)hipHostFree(m->meta[i]);
        if (m->pslot[i]) (void)hipFree(m->pslot[i]);
        if (m->lslot[i]) (void)hipFree(m->lslot[i]);
    }
    if (m->lj_scratch) (void)hipFree(m->lj_scratch);    // (s->stream was waited for above: a split frame came as a packed span)
    for (int i = 0; i < MosaicStage::NUP; ++i)
        if (m->evUp[i]) (void)hipEventDestroy(m->evUp[i]);
    for (int i = 0; i < MosaicStage::NSLOT; ++i) {
        if (m->evCopied[i]) (void)hipEventDestroy(m->evCopied[i]);
        if (m->evSlotFree[i]) (void)hipEventDestroy(m->evSlotFree[i]);
    }
    if (m->cslot[0]) (void)hipStreamSynchronize(s->stream);   // (the site kernels read the table slots)
    for (int i = 0; i < MosaicStage::NSLOT; ++i)
        if (m->cslot[i]) (void)hipFree(m->cslot[i]);
    if (m->sc_host) (void)hipHostFree(m->sc_host);
    if (m->stc) (void)hipStreamDestroy(m->stc);
    delete m;   // (the device buffers are in s->allocs)
    s->mosaic = nullptr;
}

// mi_stack_set_site_correction behind its checks (site_check, site_host_check): copy every table of `c` into the stage's
// pinned block, or clear.  The stage is created here when no mosaic came before.
inline int mosaic_set_site(mi_stack* s, const mi_site_correct_t* c, const int64_t* dmin, const int64_t* dmax) {
    int rc;
    if (!c && !mstage(s)) return MI_OK;
    if (!mstage(s) && (rc = mosaic_create(s))) return rc;
    MosaicStage* m = mstage(s);
    if (!c || c->flags == 0) {
        m->sc_on = false;
        return MI_OK;
    }
    const int H = s->p.height, W = s->p.width;
    const int nslot = s->p.impl == MI_IMPL_TILED ? MosaicStage::NSLOT : 1;
    // the block's layout: [delta_h | delta_v | per position: nodes, row axis, column axis | bad sites], each part aligned
    mi_site_correct_t d = *c;
    size_t at = 0;
    struct Part { const void* src; size_t off, bytes; };
    std::vector<Part> parts;
    const auto place = [&](const void* src, size_t bytes) {
        parts.push_back(Part{src, at, bytes});
        const size_t off = at;
        at += packed_align(bytes ? bytes : 1);
        return off;
    };
    d.delta_h = d.delta_v = nullptr;
    d.bad_sites = nullptr;
    if (c->flags & MI_SITE_DELTA_H) d.delta_h = (const int16_t*)place(c->delta_h, (size_t)W * sizeof(int16_t));
    if (c->flags & MI_SITE_DELTA_V) d.delta_v = (const int16_t*)place(c->delta_v, (size_t)H * sizeof(int16_t));
    for (int p = 0; p < 4; ++p) {
        d.gain[p] = mi_site_gain_t{};
        const mi_site_gain_t& g = c->gain[p];
        if (!(c->flags & MI_SITE_GAIN) || !g.nodes) continue;
        d.gain[p].mv = g.mv;
        d.gain[p].mh = g.mh;
        d.gain[p].nodes = (const uint16_t*)place(g.nodes, (size_t)g.mv * g.mh * sizeof(uint16_t));
        d.gain[p].row_axis = (const mi_site_axis_t*)place(g.row_axis, (size_t)H * sizeof(mi_site_axis_t));
        d.gain[p].col_axis = (const mi_site_axis_t*)place(g.col_axis, (size_t)W * sizeof(mi_site_axis_t));
    }
    if ((c->flags & MI_SITE_BAD_LIST) && c->n_bad > 0) d.bad_sites = (const int32_t*)place(c->bad_sites, (size_t)c->n_bad * sizeof(int32_t));
    const size_t bytes = at ? at : 256;
    MI_HIP(hipSetDevice(s->p.device));
    if (m->stc) MI_HIP(hipStreamSynchronize(m->stc));      // no upload reads the block that is rewritten
    else MI_HIP(hipStreamSynchronize(s->stream));          // (the synchronous route uploads on the handle's stream)
    if (bytes > m->sc_host_cap && (rc = set_realloc(&m->sc_host, 1, &m->sc_host_cap, bytes, true))) return rc;
    if (bytes > m->cslot_cap) {
        MI_HIP(hipStreamSynchronize(s->stream));           // nothing reads what is freed
        if ((rc = set_realloc(m->cslot, nslot, &m->cslot_cap, bytes, false))) return rc;
    }
    if ((c->flags & MI_SITE_BAD_CONST) && !m->sc_bits && (rc = dev_alloc(s, (void**)&m->sc_bits, defects_const_scratch_bytes(H, W)))) return rc;
    memset(m->sc_host, 0, bytes);
    for (const Part& q : parts) memcpy((char*)m->sc_host + q.off, q.src, q.bytes);
    m->sc = d;
    m->sc_bytes = bytes;
    for (int p = 0; p < 4; ++p) { m->sc_dmin[p] = dmin[p]; m->sc_dmax[p] = dmax[p]; }
    m->sc_on = true;
    return MI_OK;
}

// the stage's descriptor with its offsets turned into pointers into the device block `base`
inline mi_site_correct_t site_at(const MosaicStage* m, const char* base) {
    mi_site_correct_t d = m->sc;
    const auto fix = [&](const auto*& p, bool on) {
        using P = std::remove_reference_t<decltype(p)>;
        p = on ? (P)(base + (size_t)(uintptr_t)p) : nullptr;
    };
    fix(d.delta_h, (d.flags & MI_SITE_DELTA_H) != 0);
    fix(d.delta_v, (d.flags & MI_SITE_DELTA_V) != 0);
    for (int p = 0; p < 4; ++p) {
        const bool on = d.gain[p].mv > 0;
        fix(d.gain[p].nodes, on);
        fix(d.gain[p].row_axis, on);
        fix(d.gain[p].col_axis, on);
    }
    fix(d.bad_sites, (d.flags & MI_SITE_BAD_LIST) != 0 && d.n_bad > 0);
    return d;
}

// mi_stack_reset: the stage is empty again and keeps its buffers (the caller has waited for its stream and the handle's)
inline void mosaic_reset(mi_stack* s) {
    if (mstage(s)) mstage(s)->pending = 0;
}

// hand the frames demosaiced so far to the stack as one batch
inline int mosaic_flush(mi_stack* s) {
    MosaicStage* m = mstage(s);
    if (!m || m->pending == 0) return MI_OK;
    const TiledState* t = tstate(s);
    const int n = m->pending;
    m->pending = 0;
    // the frames are complete in s->stream order, which is what a device push asks for; behind it s->stream is ordered
    // after every reader of `bgr` (tiled_push joins the side streams), and so is the next demosaic into it
    return dispatch_push(s, m->bgr, n, t->frame_bytes);
}

// the frame one raw push brings (arguments checked by the caller, capi.hip)
struct MosaicFrame {
    const void* mosaic = nullptr;           // host: H rows, `row_stride` bytes apart, or ...
    size_t row_stride = 0;
    const PackedSrc* pk = nullptr;          // ... the packed span the mosaic is unpacked or decoded from (`mosaic` is not read)
    const mi_cfa_t* cfa = nullptr;
    bool pinned = false;                    // the source lies in pinned memory, contiguous: uploaded out of it
    const mi_calib_t* cal = nullptr;        // calibration, or null
    const mi_develop_t* dev = nullptr;      // development, or null: the plain demosaic
    const int32_t* dev_sites = nullptr;     // device: the defect sites
    int n_sites = 0;
    const mi_linear_t* lin = nullptr;       // a linear frame (with `pk`, in place of `cfa`): its levels; no site is corrected,
                                            // calibrated or repaired, and linear_develop stands where the demosaic does
};

// a packed span's device layout: [span | offsets or descriptors | table], each part 256-byte aligned
struct PackedAt {
    size_t seg_at = 0, seg_bytes = 0, table_at = 0, table_bytes = 0;
    explicit PackedAt(const PackedSrc* pk) {
        if (!pk) return;
        seg_at = packed_align(pk->span_bytes);
        seg_bytes = packed_align(packed_seg_bytes(*pk));
        table_at = seg_at + seg_bytes;
        table_bytes = (size_t)pk->layout->table_len * sizeof(uint16_t);
    }
};

// the kernels of one frame on `st`: unpack or decode the packed slot `ps` into `slot`, then in place on `slot` the site
// corrections (tables in the device block `cs`), calibration and the defect sites, then the (developed) demosaic into `frame`.
// A plain mosaic without site corrections: the demosaic alone, exactly the launches of a handle that never heard of the others.
inline void frame_kernels(hipStream_t st, const mi_stack* s, const MosaicFrame& f, const char* ps, const void* cs, void* slot, void* frame) {
    const MosaicStage* m = mstage(s);
    const int H = s->p.height, W = s->p.width, dtype = s->p.in_dtype;
    if (f.pk) {
        const PackedSrc& pk = *f.pk;
        const PackedAt at(f.pk);
        if (pk.ljseg3)
            ljpeg3_launch(st, ps, pk.span_bytes, (const mi_ljpeg_seg3_t*)(ps + at.seg_at), *pk.layout, (const uint16_t*)(ps + at.table_at), slot,
                          nullptr, m->ljstatus);
        else if (pk.ljseg && m->lj_split)
            ljpeg_split_launch(st, ps, pk.span_bytes, (const mi_ljpeg_seg_t*)(ps + at.seg_at), *pk.layout, (const uint16_t*)(ps + at.table_at),
                               m->lj_sub, m->lj_rounds, (uint32_t*)m->lj_scratch, slot, nullptr, nullptr, m->ljstatus);
        else if (pk.ljseg)
            ljpeg_launch(st, ps, pk.span_bytes, (const mi_ljpeg_seg_t*)(ps + at.seg_at), *pk.layout, (const uint16_t*)(ps + at.table_at), slot,
                         nullptr, m->ljstatus);
        else
            unpack_launch(st, ps, pk.span_bytes, (const uint32_t*)(ps + at.seg_at), *pk.layout, (const uint16_t*)(ps + at.table_at), slot);
    }
    if (f.lin) {        // `slot` holds H x W x spp samples (a linear slot): one pass to the BGR frame, nothing per site
        linear_develop_launch(st, slot, frame, H, W, dtype, *f.lin, f.dev);
        return;
    }
    if (m->sc_on) site_kernels(st, slot, H, W, dtype, *f.cfa, site_at(m, (const char*)cs), m->sc_bits);
    if (f.cal) calibrate_launch(st, slot, H, W, dtype, *f.cfa, *f.cal);
    defects_launch(st, slot, H, W, dtype, f.dev_sites, f.n_sites);   // (n_sites == 0 launches nothing)
    if (f.dev) develop_launch(st, slot, frame, H, W, dtype, *f.cfa, *f.dev);
    else demosaic_launch(st, slot, frame, H, W, dtype, *f.cfa);
}

// room for a span of `span_bytes` with `meta_bytes` of offsets and table behind it, in every packed slot the handle uses.
// Growing waits for both streams first: nothing reads what is freed.
inline int packed_reserve(mi_stack* s, size_t span_bytes, size_t meta_bytes) {
    MosaicStage* m = mstage(s);
    const int nslot = s->p.impl == MI_IMPL_TILED ? MosaicStage::NSLOT : 1;
    const size_t need = packed_align(span_bytes) + meta_bytes;
    int rc;
    if (need <= m->pslot_cap && meta_bytes <= m->meta_cap) return MI_OK;
    if (m->stc) MI_HIP(hipStreamSynchronize(m->stc));
    MI_HIP(hipStreamSynchronize(s->stream));
    if (need > m->pslot_cap && (rc = set_realloc(m->pslot, nslot, &m->pslot_cap, need, false))) return rc;
    if (meta_bytes > m->meta_cap && (rc = set_realloc(m->meta, nslot, &m->meta_cap, meta_bytes, true))) return rc;
    return MI_OK;
}

// room for H x W x spp samples in every linear slot the handle uses.  Growing waits for both streams first: nothing reads or
// writes what is freed.  (The mosaic slots stay H x W samples: a linear frame never lands in one.)
inline int linear_reserve(mi_stack* s, int spp) {
    MosaicStage* m = mstage(s);
    const int nslot = s->p.impl == MI_IMPL_TILED ? MosaicStage::NSLOT : 1;
    const size_t need = m->mosaic_bytes * (size_t)spp;
    if (need <= m->lslot_cap) return MI_OK;
    if (m->stc) MI_HIP(hipStreamSynchronize(m->stc));
    MI_HIP(hipStreamSynchronize(s->stream));
    return set_realloc(m->lslot, nslot, &m->lslot_cap, need, false);
}

// the split path's scratch for this frame, and its exact round bound.  Growing waits for s->stream first: the decode kernels
// of earlier frames, the scratch's only users, run there.
inline int ljpeg_split_reserve(mi_stack* s, const PackedSrc& pk) {
    MosaicStage* m = mstage(s);
    uint64_t samples = (uint64_t)pk.nseg * (uint64_t)pk.layout->seg_height * (uint64_t)pk.layout->seg_width;
    if (samples >= (1ull << 32)) return fail(MI_ERR_INVALID, "layout segments x seg_height x seg_width must be below 2^32 for the split path");
    m->lj_rounds = ljpeg::split_exact_rounds(pk.ljseg, (size_t)pk.nseg, pk.span_bytes, m->lj_sub);
    const size_t need = ljpeg::split_layout(*pk.layout, pk.span_bytes, m->lj_sub, m->lj_rounds).words * sizeof(uint32_t);
    if (need <= m->lj_scratch_cap) return MI_OK;
    MI_HIP(hipStreamSynchronize(s->stream));
    return set_realloc(&m->lj_scratch, 1, &m->lj_scratch_cap, need, false);
}

// mi_stack_set_ljpeg_split behind its checks: holds until replaced or cleared
inline int mosaic_set_ljpeg_split(mi_stack* s, bool on, uint32_t sub) {
    int rc;
    if (!on && !mstage(s)) return MI_OK;
    if (!mstage(s) && (rc = mosaic_create(s))) return rc;
    mstage(s)->lj_split = on;
    mstage(s)->lj_sub = sub;
    return MI_OK;
}

// One raw host frame: stage it, start its upload and its kernels, return.
inline int mosaic_push(mi_stack* s, const MosaicFrame& f) {
    TiledState* t = tstate(s);
    int rc = tiled_flush(s);   // call order: host BGR frames staged before this frame are fused first
    if (rc) return rc;
    if (!mstage(s) && (rc = mosaic_create(s))) return rc;
    MosaicStage* m = mstage(s);
    const PackedSrc* pk = f.pk;
    const size_t rb = (size_t)s->p.width * dtype_size(s->p.in_dtype);
    const bool sc = m->sc_on && !f.lin;      // site corrections: the stage's tables go up with this frame (a linear one has no sites)
    if (sc && (rc = site_black_check(f.cfa->black, m->sc_dmin, m->sc_dmax, s->p.in_dtype))) return rc;
    const PackedAt at(pk);
    if (pk && (rc = packed_reserve(s, pk->span_bytes, at.seg_bytes + at.table_bytes))) return rc;
    if (f.lin && (rc = linear_reserve(s, f.lin->spp))) return rc;
    if (pk && (pk->ljseg || pk->ljseg3) && !m->ljstatus) {
        if ((rc = dev_alloc(s, (void**)&m->ljstatus, sizeof(uint32_t)))) return rc;
        MI_HIP(hipMemsetAsync(m->ljstatus, 0, sizeof(uint32_t), s->stream));
    }
    if (pk && pk->ljseg && m->lj_split && (rc = ljpeg_split_reserve(s, *pk))) return rc;
    if (s->p.impl != MI_IMPL_TILED) {
        // float-64 and MI_IMPL_SIMPLE handles: upload, kernels, push, wait -- one frame at a time on the handle's stream
        char* ps = (char*)m->pslot[0];
        if (pk) {
            MI_HIP(hipMemcpyAsync(ps, pk->span, pk->span_bytes, hipMemcpyHostToDevice, s->stream));
            MI_HIP(hipMemcpyAsync(ps + at.seg_at, packed_seg(*pk), packed_seg_bytes(*pk), hipMemcpyHostToDevice, s->stream));
            if (at.table_bytes) MI_HIP(hipMemcpyAsync(ps + at.table_at, pk->table, at.table_bytes, hipMemcpyHostToDevice, s->stream));
        } else MI_HIP(hipMemcpy2DAsync(m->slot[0], rb, f.mosaic, f.row_stride, rb, s->p.height, hipMemcpyHostToDevice, s->stream));
        if (sc) MI_HIP(hipMemcpyAsync(m->cslot[0], m->sc_host, m->sc_bytes, hipMemcpyHostToDevice, s->stream));
        frame_kernels(s->stream, s, f, ps, m->cslot[0], f.lin ? m->lslot[0] : m->slot[0], s->frame_dev);
        MI_HIP(hipGetLastError());
        rc = dispatch_push(s, s->frame_dev, 1, t->frame_bytes);
        MI_HIP(hipStreamSynchronize(s->stream));   // (also on failure: the copies read the caller's arrays)
        return rc;
    }
    const int si = (int)(m->slot_no % MosaicStage::NSLOT);
    void* slot = f.lin ? m->lslot[si] : m->slot[si];
    if (m->slot_no >= MosaicStage::NSLOT) MI_HIP(hipStreamWaitEvent(m->stc, m->evSlotFree[si], 0));
    m->slot_no++;
    char* ps = pk ? (char*)m->pslot[si] : nullptr;
    if (sc) MI_HIP(hipMemcpyAsync(m->cslot[si], m->sc_host, m->sc_bytes, hipMemcpyHostToDevice, m->stc));   // ahead of evCopied[si]
    if (pk) {
        // offsets and table through the slot's pinned block: its previous upload is through once evCopied[si] is
        MI_HIP(hipEventSynchronize(m->evCopied[si]));   // (no-op on an event never recorded)
        char* mb = (char*)m->meta[si];
        memcpy(mb, packed_seg(*pk), packed_seg_bytes(*pk));
        if (at.table_bytes) memcpy(mb + at.seg_bytes, pk->table, at.table_bytes);
        MI_HIP(hipMemcpyAsync(ps + at.seg_at, mb, at.seg_bytes + at.table_bytes, hipMemcpyHostToDevice, m->stc));
    }
    // the frame itself: the span into the packed slot, or the mosaic into the mosaic slot
    void* dst = pk ? (void*)ps : slot;
    const void* src = pk ? pk->span : f.mosaic;
    const size_t bytes = pk ? pk->span_bytes : m->mosaic_bytes;
    if (f.pinned) {
        hipEvent_t& ev = m->evUp[m->up_no % MosaicStage::NUP];
        if (!ev) MI_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        else MI_HIP(hipEventSynchronize(ev));   // (only when more than NUP uploads are in flight)
        MI_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, m->stc));
        MI_HIP(hipEventRecord(ev, m->stc));
        if (m->frames_up_seen != t->up_no) { m->frames_up_seen = t->up_no; m->run = 0; }
        m->run++;
        m->up_no++;
    } else {
        PinRing& ring = pk ? m->ppin : m->pin;   // (mosaics are all of one size: their ring is allocated once)
        if (bytes > ring.cap) {
            if (pk) MI_HIP(hipStreamSynchronize(m->stc));   // (no upload reads a bounce buffer that is freed)
            if ((rc = pin_reserve(ring, bytes))) return rc;
        }
        if (pk) rc = pin_upload(ring, m->stc, dst, src, bytes, bytes, 1);
        else rc = pin_upload(ring, m->stc, dst, src, f.row_stride, rb, (size_t)s->p.height);
        if (rc) return rc;
    }
    MI_HIP(hipEventRecord(m->evCopied[si], m->stc));
    MI_HIP(hipStreamWaitEvent(s->stream, m->evCopied[si], 0));
    frame_kernels(s->stream, s, f, ps, m->cslot[si], slot, (char*)m->bgr + (size_t)m->pending * t->frame_bytes);
    MI_HIP(hipGetLastError());
    MI_HIP(hipEventRecord(m->evSlotFree[si], s->stream));
    m->pending++;
    if (m->pending == t->bcap) return mosaic_flush(s);
    return MI_OK;
}

// mi_stack_wait_uploads over both kinds of pinned upload.  Each kind keeps its own ring of events, and the two copy streams
// are not ordered against each other, so of the `max_outstanding` most recent uploads only the run of the most recent kind is
// left in flight; every upload of the other kind is waited for.  Never fewer waits than the contract asks for.
inline int mosaic_wait_uploads(mi_stack* s, int max_outstanding) {
    MosaicStage* m = mstage(s);
    const TiledState* t = tstate(s);
    if (!m || m->up_no == 0) return tiled_wait_uploads(s, max_outstanding);
    if (max_outstanding < 0) max_outstanding = 0;
    const long frames_since = (t ? t->up_no : 0) - m->frames_up_seen;   // pinned BGR frames after the last pinned mosaic
    const long keep_m = frames_since > 0 ? 0 : std::min<long>(max_outstanding, m->run);
    const long keep_f = frames_since > 0 ? std::min<long>(max_outstanding, frames_since) : 0;
    int rc = tiled_wait_uploads(s, (int)keep_f);
    if (rc) return rc;
    const long upto = m->up_no - keep_m;
    if (upto <= 0 || keep_m >= MosaicStage::NUP) return MI_OK;
    hipEvent_t ev = m->evUp[(upto - 1) % MosaicStage::NUP];
    if (ev) MI_HIP(hipEventSynchronize(ev));
    return MI_OK;
}

}  // namespace mi
