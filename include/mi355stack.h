/*
 * mi355stack.h -- C ABI of libmi355stack.so: the MI355X (gfx950) focus-stacking
 * hot path behind shinestacker's PyramidStack / align_images.
 *
 * Plain pointers and sizes only; no exceptions cross this boundary: every entry
 * point returns an MI_* status and mi_last_error() gives the thread-local text
 * (the Python shim maps codes to shinestacker's exception types,
 * reference core/exceptions.py:2-52).
 *
 * Reference interfaces replaced (paths under /root/reference/src/shinestacker):
 *   mi_stack_create / _reset / _destroy   PyramidStack.__init__ + per-stack state,
 *                                         algorithms/pyramid.py:114-123, :150-165
 *   mi_stack_push_frame[_device]          process_single_image per frame,
 *                                         pyramid.py:125-139 (called at :173), fused with
 *                                         the per-level selection of fuse_laplacian :48-55
 *                                         and the base features of get_fused_base :95-102
 *                                         as a running first-max (frames in index order)
 *   mi_stack_finish[_device]              fuse_pyramids tail + collapse + cast,
 *                                         pyramid.py:103-111, :57-64, :178-179
 *   mi_stack_get_level                    debug/parity taps (no reference counterpart)
 *   mi_stack_state / _set_first_index     hooks for the frame-sharded multi-GPU combine
 *   mi_warp_affine[_device]               cv2.warpAffine + warped mask + border blur composite,
 *                                         algorithms/align.py:238-251
 *
 * Ownership: the caller owns every host buffer it passes and every device
 * buffer obtained from mi_device_malloc; the library owns all device memory
 * inside a handle; nothing returned by pointer outlives mi_stack_destroy.
 * Threading: one thread at a time per handle; any thread may call (the device
 * is selected per call).  The library never calls back into the host language.
 */
#ifndef MI355STACK_H
#define MI355STACK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ABI_VERSION 1
#define MI_API __attribute__((visibility("default")))

/* status codes */
enum {
    MI_OK = 0,
    MI_ERR_INVALID = 1,   /* bad argument / option            -> InvalidOptionError / ValueError */
    MI_ERR_NO_DEVICE = 2, /* no HIP device visible            -> RuntimeError                    */
    MI_ERR_HIP = 3,       /* a HIP runtime call failed        -> RuntimeError                    */
    MI_ERR_STATE = 4,     /* call order (finish before push)  -> RuntimeError                    */
    MI_ERR_NOMEM = 5,     /* device allocation failed         -> MemoryError                     */
    MI_ERR_UNSUPPORTED = 6,
    MI_ERR_ALIGNMENT = 7  /* a frame could not be registered    -> AlignmentError                  */
};

/* pixel / arithmetic types */
enum { MI_U8 = 0, MI_U16 = 1, MI_F32 = 2, MI_F64 = 3 };

/* mi_stack_get_level selectors */
enum {
    MI_TAP_GAUSS = 0,      /* G_l of the most recently pushed frame, h x w x 3 f32 (l >= 1)   */
    MI_TAP_FUSED_LAP = 1,  /* running fused Laplacian of level l, h x w x 3 f32               */
    MI_TAP_ENERGY = 2,     /* running max energy of level l, h x w f32                        */
    MI_TAP_INDEX = 3,      /* running arg-max (global frame index), h x w i32                 */
    MI_TAP_FUSED_BASE = 4, /* fused base (level == levels), hb x wb x 3 f32; valid after finish */
    MI_TAP_BASE_IDX_E = 5, /* hb x wb i32 */
    MI_TAP_BASE_IDX_D = 6, /* hb x wb i32 */
    MI_TAP_COLLAPSED = 7,  /* clip(abs(collapse)), H x W x 3 f32; valid after finish            */
    MI_TAP_BASE_ENT = 8,   /* running max entropy, hb x wb f32 */
    MI_TAP_BASE_DEV = 9    /* running max deviation, hb x wb f32 */
};

/* implementation selector (both give bit-identical results) */
enum {
    MI_IMPL_AUTO = 0,
    MI_IMPL_SIMPLE = 1, /* one thread per output, global-memory taps: the on-GPU cross-check */
    MI_IMPL_TILED = 2   /* LDS-tiled fused level kernels                                     */
};

/* arithmetic of the pyramid stencils (mi_stack_params.arith)
 *   MI_ARITH_EXACT      every 5x5 stencil as the reference's own 25-tap row-major chain (cv2.filter2D order as
 *                       restated in oracle/): every intermediate bit-identical to the oracle.  The value of a
 *                       zero-initialised struct and of mi_stack_default_params: at the C boundary the caller NAMES the
 *                       arithmetic, and what it gets without naming one is the bit-pinned order (the audit mode).  The
 *                       Python host mirror's high-level entry points (PyramidStack, align_and_stack[_device],
 *                       bunches_then_stack) all pass ONE default explicitly -- defaults.resolve_arith, "separable" -- so no
 *                       two of them differ for the same input (round 5).
 *   MI_ARITH_SEPARABLE  the same stencils as two 5-tap passes with the float32 generating kernel (polyphase for
 *                       the expand): ~half the arithmetic, coefficients within the float32 forward-error bound
 *                       of a float64 evaluation, per-pixel arg-max may flip at near ties (tolerance in
 *                       tests/test_sep_tolerance.py).  float_type must be MI_F32. */
enum { MI_ARITH_EXACT = 0, MI_ARITH_SEPARABLE = 1 };

typedef struct mi_stack mi_stack_t;

typedef struct mi_stack_params {
    int32_t height, width; /* frame geometry; channels fixed at 3, BGR interleaved            */
    int32_t in_dtype;      /* MI_U8 / MI_U16 / MI_F32 (f32 frames hold integer pixel values)  */
    int32_t out_dtype;     /* MI_U8 / MI_U16: dtype of the fused image (pyramid.py:159-164)   */
    int32_t min_size;      /* pyramid.py:115,165  default 32                                  */
    int32_t kernel_size;   /* pyramid.py:116,18   base-level window only; default 5           */
    double gen_kernel;     /* pyramid.py:117,19   default 0.4                                 */
    int32_t float_type;    /* MI_F32 / MI_F64 (base_stack_algo.py:14-22; MI_F64 runs one frame at a time) */
    int32_t use_fma;       /* 1: fma chain (OpenCV AVX2 path) 0: mul+add (SSE baseline path)  */
    int32_t device;        /* HIP device ordinal                                              */
    int32_t impl;          /* MI_IMPL_*                                                       */
    int32_t batch_frames;  /* frames per batch (tiled impl).  0 = automatic: host frames are staged in a ring of 32;
                            * MI_ARITH_SEPARABLE takes a resident push as ONE batch of up to 256 frames while its
                            * per-batch buffers fit a quarter of the free device memory (allocated on demand).
                            * > 0: batches of exactly this many frames, buffers allocated by mi_stack_create (for
                            * callers that push batch after batch and must not stall on an allocation)           */
    int32_t arith;         /* MI_ARITH_*; 0 = exact (the C default, see the enum's comment)     */
    int32_t pair_levels;   /* MI_ARITH_SEPARABLE: pyramid levels as pass PAIRS (l, l + 1) -- level l's kernel hands level l + 1
                            * gray(G_{l+1}) and G_{l+2}, the three-channel G_{l+1} of the batch never reaches HBM (pyramid.py:27-46,
                            * :125-139: the reduce -> expand dependency), the winners' pixels of it are recomputed once per batch.
                            * Results are bit-identical either way.  0 = automatic = where it measured faster: the pair (0, 1)
                            * for float-32 frames in batches of 192 and more; 1 = pairs (0, 1), (2, 3), ...; 2 = none;
                            * 3 = pairs (1, 2), (3, 4), ...                                                */
    int32_t reserved[3];
} mi_stack_params_t;

/* ---- library ---- */
MI_API int mi_abi_version(void);
MI_API const char* mi_last_error(void);
MI_API int mi_device_count(int* count);
MI_API int mi_device_name(int device, char* buf, size_t buflen);
MI_API void mi_stack_default_params(mi_stack_params_t* p);

/* ---- device memory helpers (so a host language needs no other GPU binding) ---- */
MI_API int mi_device_malloc(int device, size_t bytes, void** dev_ptr);
MI_API int mi_device_free(int device, void* dev_ptr);
MI_API int mi_memcpy_h2d(int device, void* dev_dst, const void* host_src, size_t bytes);
MI_API int mi_memcpy_d2h(int device, void* host_dst, const void* dev_src, size_t bytes);
MI_API int mi_memcpy_d2d(int device, void* dev_dst, const void* dev_src, size_t bytes);
MI_API int mi_memcpy_d2d_async(int device, void* stream, void* dev_dst, const void* dev_src, size_t bytes);
MI_API int mi_device_synchronize(int device);
/* ---- PyramidStack's step methods, one at a time, on host float32 images of c = 1 or 3 interleaved channels -- the
 * reference's public methods of the same names (pyramid.py:24-63), always in ITS evaluation order (row-major 25-tap chain):
 *   MI_PYR_CONVOLVE        in (h, w, c)                  -> out (h, w, c)             cv2.filter2D, REFLECT101   (:24-25)
 *   MI_PYR_REDUCE          in (h, w, c)                  -> out (ceil(h/2), ceil(w/2), c)                      (:27-32)
 *   MI_PYR_EXPAND          in (h, w, c)                  -> out (2h, 2w, c)                                    (:34-46)
 *   MI_PYR_FUSE_LAPLACIAN  in (n, h, w, 3)               -> out (h, w, 3)   energy, first arg-max, where-sum  (:48-55)
 *   MI_PYR_COLLAPSE_STEP   in = layer (h, w, c), in2 = coarser image (h2, w2, c) -> expand(in2)[:h, :w] + in   (:59-63)
 *   MI_PYR_CLIP_ABS        in (h, w, c)                  -> clip(abs(in), 0, maxv)                             (:64)    */
enum { MI_PYR_CONVOLVE = 0, MI_PYR_REDUCE = 1, MI_PYR_EXPAND = 2, MI_PYR_FUSE_LAPLACIAN = 3, MI_PYR_COLLAPSE_STEP = 4,
       MI_PYR_CLIP_ABS = 5 };
MI_API int mi_pyr_step(int device, int op, int use_fma, double gen_kernel, const void* host_in, const void* host_in2, int n,
                int h, int w, int c, int h2, int w2, double maxv, void* host_out);
/* free / total device memory in bytes (hipMemGetInfo): callers size resident stacks and batches with it */
MI_API int mi_device_mem_info(int device, size_t* free_bytes, size_t* total_bytes);

/* ---- stacker handle ---- */
MI_API int mi_stack_create(mi_stack_t** out, const mi_stack_params_t* params);
MI_API void mi_stack_destroy(mi_stack_t* s);
MI_API int mi_stack_reset(mi_stack_t* s);
MI_API int mi_stack_levels(const mi_stack_t* s, int* levels);
MI_API int mi_stack_level_shape(const mi_stack_t* s, int level, int* h, int* w);
MI_API int mi_stack_frames_pushed(const mi_stack_t* s, int* n);
/* global index of this handle's first frame (multi-GPU frame sharding); default 0 */
MI_API int mi_stack_set_first_index(mi_stack_t* s, int first_global_index);
/* interleaved frame shards (rank r of W holds frames r, r + W, ...: every rank sees the whole focus range, so its winners are
 * as coherent as the whole stack's): the global index of the handle's k-th frame = first_global_index + k * stride.  The
 * kernels number the frames consecutively; mi_stack_export_indices rewrites the winner indices of one level (level == levels,
 * levels + 1: the base twins; -1: all) into the global numbering, in place -- before they leave the handle (the cross-GPU
 * combine breaks ties by them: np.argmax's first maximum, pyramid.py:51; the index taps call it themselves).  After an export
 * the handle takes no more frames until mi_stack_reset.  Default stride 1: nothing to export. */
MI_API int mi_stack_set_index_stride(mi_stack_t* s, int stride);
MI_API int mi_stack_export_indices(mi_stack_t* s, int level);

/* One frame from host memory (H rows of row_stride_bytes; 0 = tightly packed).
 * Returns after the work is enqueued; the host buffer may be reused on return. */
MI_API int mi_stack_push_frame(mi_stack_t* s, const void* host_bgr, size_t row_stride_bytes);
/* The same for a frame that already lies in PINNED host memory with contiguous rows (mi_host_alloc, or any buffer pinned
 * with mi_host_register -- e.g. the array an image decoder writes into): the upload reads the caller's buffer directly, no
 * bounce copy (the reference's frames come from cv2.imread, stack.py:61-97 -> utils.py:10-19; config 5 is upload-bound).
 * The buffer must stay untouched until mi_stack_wait_uploads reports the upload done.  MI_ERR_INVALID when the memory is
 * not pinned. */
MI_API int mi_stack_push_frame_pinned(mi_stack_t* st, const void* host_bgr, size_t row_stride_bytes);
/* blocks until at most `max_outstanding` of the frames pushed with mi_stack_push_frame_pinned -- and of the pinned mosaics
 * pushed with mi_stack_push_mosaic -- are still being uploaded (0: all of them are on the device; a decoder that cycles k
 * pinned buffers calls it with k - 1 before it reuses one).  On a handle that received both kinds, only the most recent run
 * of one kind is left in flight: it may wait for more uploads than asked, never for fewer. */
MI_API int mi_stack_wait_uploads(mi_stack_t* st, int max_outstanding);
/* pinned host memory: allocate / free, or pin / unpin memory the caller owns */
MI_API int mi_host_alloc(void** ptr, size_t bytes);
MI_API int mi_host_free(void* ptr);
MI_API int mi_host_register(void* ptr, size_t bytes);
MI_API int mi_host_unregister(void* ptr);
/* n frames already resident in device memory (tightly packed rows, frames
 * frame_stride_bytes apart), dtype = params.in_dtype.  The frames must be complete either on the host's
 * timeline (a finished copy / kernel) or in the order of the handle's stream (mi_stack_stream): work the
 * caller enqueued there -- a warp, a table apply -- is waited for on the device, not on the host. */
MI_API int mi_stack_push_frames_device(mi_stack_t* s, const void* dev_frames, int n,
                                size_t frame_stride_bytes);
/* wait for everything enqueued so far */
MI_API int mi_stack_sync(mi_stack_t* s);

/* wait until the selection state of `level` covers every pushed frame.  level 0 (3/4 of the state) is final while the
 * coarser levels of the last batch are still running: the cross-GPU exchange of level 0 can start behind this call
 * (multigpu.Combiner does).  Any other level: same as mi_stack_sync. */
MI_API int mi_stack_sync_level(mi_stack_t* s, int level);

/* base fusion + collapse + abs/clip/truncating cast.  The handle stays valid
 * (taps readable) until reset/destroy.  host_out: H x W x 3 of out_dtype. */
MI_API int mi_stack_finish(mi_stack_t* s, void* host_out, size_t row_stride_bytes);
MI_API int mi_stack_finish_device(mi_stack_t* s, void* dev_out);

MI_API int mi_stack_get_level(mi_stack_t* s, int level, int what, void* host_out, size_t out_bytes);

/* Device pointers of the running selection state of one level (level ==
 * levels addresses the base: energy -> entropy max, lap -> base_e; the
 * deviation twin comes from level == levels + 1).  level == -1: the state of ALL levels and of both
 * base twins at once -- float-32 stacks keep it in three contiguous slabs (per-level segments padded
 * to 64 pixels; npixels counts the padding) so that the combine can move it as one flat vector.
 * For the cross-GPU combine.
 * Synchronises the handle: on return all enqueued work has finished, so the pointers may be
 * used from any other stream. */
MI_API int mi_stack_state(mi_stack_t* s, int level, void** dev_energy, void** dev_lap, void** dev_index,
                   size_t* npixels);
/* the HIP stream the handle launches on (hipStream_t as void*) */
MI_API int mi_stack_stream(mi_stack_t* s, void** stream);

/* ---- depth map output (csrc/kernels_depth.hpp; no reference counterpart) ----
 * The frame index in focus at each pixel, height x width float32, in global frame numbers (first + k * stride under
 * mi_stack_set_first_index / _set_index_stride, whether or not the indices were exported).  Computed from the level-0 state
 * of the frames pushed so far: v = the winner index, w = the running energy.  sigma == 0: the index itself.  0 < sigma <= 16:
 * confidence-weighted smoothing, out = B(v * w) / B(w) where B(w) > 0, else v, with B the separable Gaussian of radius
 * ceil(3 sigma) < min(height, width) and BORDER_REFLECT_101, in a fixed evaluation order in the stack's float_type (the header
 * of kernels_depth.hpp states it; tests/depth_restatement.py is held to it bit for bit).  Reads the state only: it may be
 * called before or after finish, any number of times.  MI_ERR_STATE with no frame pushed, MI_ERR_UNSUPPORTED for a stack
 * without a Laplacian level, MI_ERR_INVALID for a sigma outside [0, 16] or a radius that does not fit the frame.
 * mi_stack_depth_map_device: `dev_out` in device memory; synchronises the handle, as mi_stack_state does. */
MI_API int mi_stack_depth_map(mi_stack_t* s, double sigma, void* host_out);
MI_API int mi_stack_depth_map_device(mi_stack_t* s, double sigma, void* dev_out);
/* The smoothing above on caller-made host planes (tests, other callers): `host_value` is int32 (value_is_int32 != 0) or of
 * `float_type` (MI_F32 / MI_F64), `host_weight` (>= 0) of `float_type`, `host_out` float32, all height x width. */
MI_API int mi_weighted_smooth(int device, const void* host_value, const void* host_weight, int height, int width, int value_is_int32,
                       int float_type, double sigma, void* host_out);

/* ---- edge-aware refinement of the depth map (kernels_guided.hpp; no reference counterpart) ----
 * The confidence-weighted guided filter: out = mean over the windows holding a pixel of (a I + b), where depth ~ a I + b is
 * the weighted least-squares fit of the window, I the grey of `guide` (height x width x 3 BGR, MI_U8 / MI_U16:
 * (1868 B + 9617 G + 4899 R + 8192) >> 14 over 255 or 65535), windows of (2 radius + 1)^2 clipped to the frame, clamped to
 * [lo, hi].  All in float64 in a fixed evaluation order (the header of kernels_guided.hpp states it;
 * tests/guided_restatement.py is held to it bit for bit).  value, out: height x width float32; weight: height x width of
 * weight_float_type (MI_F32 / MI_F64), finite and >= 0.
 * MI_ERR_INVALID, with the argument's name in the message and before any device call: null pointers, height / width < 1,
 * radius outside [1, 32], eps outside [1e-9, 1e3] or not finite, lo / hi not finite or lo > hi, another guide_dtype or
 * weight_float_type, and for the device form planes off their types' alignment.
 * mi_depth_guided_device: device pointers; `dev_scratch` is MI_GUIDED_SCRATCH_PLANES * height * width doubles on a 16-byte
 * boundary; four launches are queued on `stream` and not waited for. */
enum { MI_GUIDED_SCRATCH_PLANES = 7, MI_GUIDED_MAX_RADIUS = 32 };
MI_API int mi_depth_guided(int device, const void* host_value, const void* host_weight, int weight_float_type, const void* host_guide,
                    int guide_dtype, int height, int width, int radius, double eps, double lo, double hi, void* host_out);
MI_API int mi_depth_guided_device(int device, void* stream, const void* dev_value, const void* dev_weight, int weight_float_type,
                           const void* dev_guide, int guide_dtype, int height, int width, int radius, double eps, double lo, double hi,
                           void* dev_scratch, void* dev_out);
/* mi_stack_depth_map(sigma) refined against `guide` (the fused frame, height x width x 3 of guide_dtype): the weight is the
 * running level-0 energy, lo / hi the handle's frame numbers first and first + (n - 1) * stride.  Reads the state only;
 * every status of mi_stack_depth_map, and MI_ERR_INVALID as above.  One device allocation per call, freed on every way out.
 * The _device form takes `dev_guide` and `dev_out` in device memory; both wait for the handle's stream. */
MI_API int mi_stack_depth_map_refined(mi_stack_t* s, double sigma, const void* host_guide, int guide_dtype, int radius, double eps,
                               void* host_out);
MI_API int mi_stack_depth_map_refined_device(mi_stack_t* s, double sigma, const void* dev_guide, int guide_dtype, int radius, double eps,
                                      void* dev_out);

/* ---- per-kernel timing (hipEvent pairs on the handle's stream) ---- */
enum {
    MI_PROF_LEVEL = 0,    /* fused level launches of levels >= 1 (simple impl: whole frames) */
    MI_PROF_BASE = 1,     /* base-level feature kernels                                      */
    MI_PROF_COLLAPSE = 2, /* base fusion + collapse + finalise                               */
    MI_PROF_LEVEL0 = 3,   /* fused level-0 launches: the dominant kernel                     */
    MI_PROF_KINDS = 4
};
MI_API int mi_stack_profile(mi_stack_t* s, int enable);
/* sums since the last reset; algorithmic_bytes follows SURVEY.md 8(d).  The consecutive launches of one level pass on
 * one stream share an event pair (first start .. last end, idle gaps between them included); `launches` counts kernels. */
MI_API int mi_stack_profile_get(mi_stack_t* s, int kind, double* total_ms, int64_t* launches,
                         double* algorithmic_bytes);

/* ---- cross-GPU combine kernels (local parts of the frame-sharded reduce) ---- */
/* cand_e: [n][npix] f32, cand_lap: [n][npix*3] f32, cand_idx: [n][npix] i32 (may be
 * NULL), candidates in ascending global-frame order; writes the first-max winner's
 * energy / lap / index to out_*.  `stream` is a hipStream_t (NULL = default stream). */
MI_API int mi_combine_select(int device, void* stream, int n, const void* cand_e, const void* cand_lap,
                      const void* cand_idx, size_t npix, void* out_e, void* out_lap, void* out_idx);

/* "Winners only" form of the same reduce (what multigpu.Combiner uses; <= 16 ranks): the ranks exchange energies only,
 * mi_combine_winner names the winning rank of every pixel of a chunk (first maximum in rank order), every rank learns the
 * whole winner map (1 byte per pixel), and each rank sends just the payload rows it WON -- packed in pixel order by
 * mi_combine_pack -- straight to the collapsing rank, which puts them in place with mi_combine_unpack.
 * mi_combine_plan: per-block start positions of every rank's rows in its packed buffer (`plan`: device scratch of
 * mi_combine_plan_bytes) and the row totals per rank on the host (synchronises the stream).
 * dev_bufs: DEVICE array of n_ranks device pointers, entry r = rank r's packed rows (the entry of `rank` itself unused). */
MI_API int mi_combine_winner(int device, void* stream, int n_ranks, const void* cand_e, size_t npix, void* win_u8);
/* the same for interleaved shards (mi_stack_set_index_stride): the candidates' global frame indices travel with their
 * energies and break ties (the lower index wins) -- the rank order is not the frame order there */
MI_API int mi_combine_winner_idx(int device, void* stream, int n_ranks, const void* cand_e, const void* cand_idx, size_t npix,
                                 void* win_u8);
MI_API size_t mi_combine_plan_bytes(size_t npix, int n_ranks);
MI_API int mi_combine_plan(int device, void* stream, const void* win_u8, size_t npix, int n_ranks, void* plan,
                           int64_t* totals);
MI_API int mi_combine_pack(int device, void* stream, const void* win_u8, size_t npix, int n_ranks, int rank,
                           const void* plan, const void* src, int width, void* out);
MI_API int mi_combine_unpack(int device, void* stream, const void* win_u8, size_t npix, int n_ranks, int rank,
                             const void* plan, const void* const* dev_bufs, int width, void* dst);

/* ---- alignment apply step: cv2.warpAffine(img, M, (w,h), borderMode, borderValue) for the
 * ALIGN_RIGID transform of align_images (reference algorithms/align.py:238-251), H x W x 3
 * uint8 / uint16.  M is the 2x3 src->dst matrix as OpenCV takes it (row-major, 6 doubles).
 * border_mode: 0 = BORDER_CONSTANT(border_value), 1 = BORDER_REPLICATE,
 *              2 = BORDER_REPLICATE_BLUR: replicate, then pixels whose warped all-ones mask is 0
 *                  are replaced by GaussianBlur(warp, (blur_ksize, blur_ksize), blur_sigma).
 * mask (optional, H x W bytes): the warped all-ones uint8 mask (align.py:245-247).
 * The _device form works on device buffers (dev_tmp: one image of scratch, needed for mode 2). */
MI_API int mi_warp_affine(int device, const void* host_src, void* host_dst, void* host_mask, int height,
                   int width, int dtype, const double* M, int border_mode, const double* border_value,
                   int blur_ksize, double blur_sigma);
MI_API int mi_warp_affine_device(int device, void* stream, const void* dev_src, void* dev_dst, void* dev_tmp,
                          void* dev_mask, int height, int width, int dtype, const double* M,
                          int border_mode, const double* border_value, int blur_ksize, double blur_sigma);

/* The same for the ALIGN_HOMOGRAPHY transform: cv2.warpPerspective(img, M, (w, h), borderMode, borderValue) of image and
 * all-ones mask (reference algorithms/align.py:231-237) + the same blurred-border composite.  M: the 3x3 src->dst matrix
 * as OpenCV takes it (row-major, 9 doubles). */
MI_API int mi_warp_perspective(int device, const void* host_src, void* host_dst, void* host_mask, int height, int width,
                        int dtype, const double* M, int border_mode, const double* border_value, int blur_ksize,
                        double blur_sigma);
MI_API int mi_warp_perspective_device(int device, void* stream, const void* dev_src, void* dev_dst, void* dev_tmp,
                               void* dev_mask, int height, int width, int dtype, const double* M, int border_mode,
                               const double* border_value, int blur_ksize, double blur_sigma);

/* ---- GPU transform estimator (new capability; north_star's "ECC warp-affine alignment loop"):
 * Enhanced-Correlation-Coefficient maximisation of a 4-DoF similarity -- the motion model of the
 * reference's default ALIGN_RIGID estimate (cv2.estimateAffinePartial2D, algorithms/align.py:141-148)
 * -- coarse-to-fine on a Gaussian pyramid of the two H x W x 3 uint8/uint16 images.
 * M_out: 2x3 row-major matrix mapping the MOVING image onto the REFERENCE, i.e. what
 * cv2.warpAffine / mi_warp_affine take.  cc_out: final correlation coefficient, iters_out: total
 * Gauss-Newton iterations.  max_levels <= 0: automatic pyramid depth. */
MI_API int mi_ecc_similarity(int device, const void* host_ref, const void* host_mov, int height, int width,
                      int dtype, int max_levels, int max_iters, double eps, double* M_out, double* cc_out,
                      int* iters_out);

/* Device-resident form of the same estimator for the AlignFrames loop (align.py:255-330): the
 * pyramids are allocated once, the reference frame's pyramid is built once per reference, every
 * moving frame costs one pyramid build plus the Gauss-Newton iterations.  `subsample` folds the
 * reference's fast sub-sampling img[::s, ::s] (utils.py img_subsample) into the first kernel; the
 * returned M is in full-resolution pixels (translation scaled back as align.py:224-231 does).
 * dev_ref / dev_mov: H x W x 3 device images of the handle's dtype.  The kernels run on `stream`, or on
 * a stream the handle owns when `stream` is NULL (handles driven from different host threads then
 * run side by side);
 * mi_aligner_estimate returns after the last iteration (the Gauss-Newton steps run on the device; the host reads the frames'
 * `active` flags back every few iterations). */
typedef struct mi_aligner* mi_aligner_t;
MI_API int mi_aligner_create(mi_aligner_t* out, int device, int height, int width, int dtype, int subsample,
                      int max_levels);
/* sub-sample like the reference's default (fast_subsampling = False: cv2.resize(INTER_AREA), the mean of every s x s
 * block, utils.py:83) instead of img[::s, ::s]; call before mi_aligner_set_reference */
MI_API int mi_aligner_set_area_subsampling(mi_aligner_t al, int enable);
/* Coarse initialiser (north_star: "ECC/phase-correlation"): before the Gauss-Newton iteration every estimate takes the
 * TRANSLATION that phase correlation finds on the finest pyramid level of at most 512 pixels per side (Hann window, DFT,
 * normalised cross-power spectrum, inverse DFT, 5 x 5 centroid around the peak -- cv2.phaseCorrelate's recipe) as the
 * starting point; a peak with a response below 0.02 is ignored.  Extends the capture range from a few pixels of the
 * coarsest level to half the frame.  Off by default. */
MI_API int mi_aligner_set_phase_init(mi_aligner_t al, int enable);
/* The correlation alone, for two float32 planes (height x width, at most 1024 pixels per side) on the device:
 * out3 = (dx, dy, response) with mov(x + dx, y + dy) ~ ref(x, y). */
MI_API int mi_phase_correlate_device(int device, void* stream, const void* dev_ref, const void* dev_mov, int height, int width,
                              double* out3);
/* Read-only tap (tests): the same launches as mi_phase_correlate_device up to one stage, and that stage's plane to host
 * memory as P x Q complex float32 (re, im; P, Q = height, width rounded up to powers of two).  Same argument checks;
 * `what` out of range is MI_ERR_INVALID. */
enum {
    MI_PC_TAP_WINDOWED_MOV = 0, /* mov times the Hann window, zero-padded to P x Q                                    */
    MI_PC_TAP_SPECTRUM_REF = 1, /* forward DFT of the windowed ref                                                    */
    MI_PC_TAP_SPECTRUM_MOV = 2, /* forward DFT of the windowed mov                                                    */
    MI_PC_TAP_CROSS_POWER = 3,  /* R = Mov conj(Ref) / |Mov conj(Ref)|, 0 where the magnitude is not above 1e-20      */
    MI_PC_TAP_SURFACE = 4       /* un-normalised inverse DFT of R: the correlation surface, imaginary part included   */
};
MI_API int mi_phase_correlate_tap_device(int device, void* stream, const void* dev_ref, const void* dev_mov, int height,
                                  int width, int what, void* host_out);
MI_API int mi_aligner_destroy(mi_aligner_t al);
MI_API int mi_aligner_set_reference(mi_aligner_t al, void* stream, const void* dev_ref);
MI_API int mi_aligner_estimate(mi_aligner_t al, void* stream, const void* dev_mov, int max_iters, double eps,
                        double* M_out, double* cc_out, int* iters_out);
/* n <= 128 moving frames against the same reference in one batched Gauss-Newton: one launch per iteration for the
 * whole batch, the step itself on the device.  M_out: n x 6, cc_out / iters_out: n entries; a frame
 * the method fails on (no overlap, constant image) gets cc = -2 and an identity matrix. */
MI_API int mi_aligner_estimate_batch(mi_aligner_t al, void* stream, const void* const* dev_movs, int n, int max_iters,
                              double eps, double* M_out, double* cc_out, int* iters_out);

/* Every frame of a batch against ANOTHER FRAME OF THE BATCH (ref_of[k] = index of frame k's reference; a frame may name itself:
 * identity, correlation 1): the pyramids of the n frames are built once, frame k's template is frame ref_of[k]'s pyramid.  The
 * chained order of the reference's jobs (stack_framework.py:214-232: frame f against frame f - 1) as ONE batched Gauss-Newton
 * -- the steps are then composed by the caller.  M_out[k]: frame k -> frame ref_of[k], full-resolution pixels. */
MI_API int mi_aligner_estimate_pairs(mi_aligner_t al, void* stream, const void* const* dev_frames, int n_frames, const int* ref_of,
                                     int max_iters, double eps, double* M_out, double* cc_out, int* iters_out);
/* The same iteration started from given transforms instead of from the identity: `M_init` (n x 6, moving -> reference,
 * full-resolution pixels: what an earlier estimate returned) is refined on the `levels` finest pyramid levels (1 = the
 * finest alone).  The chained order of the reference's jobs (step_process, stack_framework.py:214-232) uses it to pull
 * every frame's chain estimate back onto the GLOBAL reference frame, so that the steps' errors do not add up
 * (shinestacker_amd/pipeline.py::_align_chains_device).  Outputs as mi_aligner_estimate_batch. */
MI_API int mi_aligner_refine_batch(mi_aligner_t al, void* stream, const void* const* dev_movs, int n, const double* M_init,
                            int levels, int max_iters, double eps, double* M_out, double* cc_out, int* iters_out);

/* ALIGN_HOMOGRAPHY (align.py:138-140, cv2.findHomography): the same estimate refined to 8 degrees of freedom -- the
 * forward-additive ECC iteration in cv2.findTransformECC's MOTION_HOMOGRAPHY form, on the finest level, from the
 * converged similarity.  M9_out: n x 9 doubles, row-major 3 x 3 (moving -> reference, full-resolution pixels, M[8] = 1),
 * ready for mi_warp_perspective; a frame whose refinement fails or does not raise the correlation keeps its similarity. */
MI_API int mi_aligner_estimate_homography_batch(mi_aligner_t al, void* stream, const void* const* dev_movs, int n, int max_iters,
                                         double eps, double* M9_out, double* cc_out, int* iters_out);

/* ---- the resident align -> stack loop in ONE call (reference: CombinedActions.run_frame over AlignFrames with a fixed
 * reference frame, stack_framework.py:191-232, :269-297, followed by FocusStack, stack.py:101-113; BASELINE config 4).
 * Every frame of `dev_frames` (n_frames x H x W x 3, `frame_stride` bytes apart, the stack handle's in_dtype) except
 * frame `ref_idx` is registered against frame `ref_idx` with the device estimator (`ecc_batch` <= 128 frames per batched
 * Gauss-Newton), warped with align.py:230-251's border handling straight into the stacker's input batch and pushed
 * (`batch_frames` warped frames per push; two batches alternate, so the next one fills while the last is fused); the
 * reference frame passes through untouched (align.py:279-280).  The host-side sequencing that
 * shinestacker_amd/pipeline.py does call by call (~25 library calls per frame) runs inside the library here -- same kernels
 * in the same order on the same streams, same results.
 *   dev_batches : 2 * batch_frames frames of scratch; dev_tmp: one frame, dev_mask: H x W bytes (border blur).
 *   M_out       : n_frames x 9 doubles; row i holds the 2x3 (transform 0) or 3x3 (transform 1: the similarity applied through
 *                 warpPerspective) matrix of frame i, zeros for the reference frame;  cc_out: n_frames correlation coefficients.
 * A frame whose correlation stays below min_correlation stops the loop: MI_ERR_ALIGNMENT, *failed_frame = its index
 * (-> AlignmentError).  Only COMPLETE batches of `batch_frames` warped frames before it have been pushed: the frames
 * already warped into the partially filled batch are not flushed, so the stack holds a prefix of the frames and must be
 * reset (mi_stack_reset) before it is used again. */
typedef struct mi_align_stack_opts {
    int transform;            /* 0: ALIGN_RIGID (warpAffine), 1: ALIGN_HOMOGRAPHY (warpPerspective) */
    int border_mode;          /* as mi_warp_affine_device */
    double border_value[4];
    int blur_ksize;
    double blur_sigma;
    double min_correlation;
    int max_iters;
    double eps;
    int ecc_batch;            /* 1..128 */
    int batch_frames;         /* >= 1 */
} mi_align_stack_opts_t;
/* optional: every aligned frame (not the reference frame) is balanced in place with the LINEAR map before it is pushed
 * (the example projects' order: align, balance, stack -- CombinedActions([AlignFrames, BalanceFrames])); the fields are
 * mi_balance_linear_device's, plus the 8-bit colour conversions around it for the HSV / HLS channel modes (-1 = none) */
typedef struct mi_balance_linear_opts {
    int mode, subsample, fast;
    double mask_size;
    int lo, hi, first_channel;
    int cvt_to, cvt_from;      /* MI_CVT_* codes applied before / after; -1 = stay in BGR */
    double ref_means[3];
    void* dev_hist_scratch;    /* 3 * nbins uint32 */
    void* dev_lut;             /* 3 * nbins entries of the image dtype */
    double* dev_corr_out;      /* NULL or device array of n_frames * ncorr doubles (row i = frame i) */
    int ncorr;
} mi_balance_linear_opts_t;
MI_API int mi_align_stack_device(mi_stack_t* st, mi_aligner_t al, const void* dev_frames, int n_frames, size_t frame_stride,
                          int ref_idx, const mi_align_stack_opts_t* opts, const mi_balance_linear_opts_t* balance,
                          void* dev_batches, void* dev_tmp, void* dev_mask, double* M_out, double* cc_out, int* failed_frame);

/* ---- BalanceFrames device steps (reference algorithms/balance.py).
 * mi_histogram: histogram of an H x W x 3 uint8/uint16 BGR image as balance.py:158-180
 * (calc_hist_1ch) takes it -- after sub-sampling by `subsample` (fast: img[::s, ::s]; otherwise the
 * integer-factor area mean of cv2.resize(INTER_AREA), utils.py:79-86) and, when mask_size > 0,
 * inside the centred circle of radius min(w, h) * mask_size / 2 of the sub-sampled image.
 * mode 0: one histogram per channel B, G, R (RGBCorrection, balance.py:264-266) -> counts[3][nbins];
 * mode 1: histogram of cv2.cvtColor(BGR2GRAY) (LumiCorrection, balance.py:235-236) -> counts[1][nbins];
 * nbins = 256 (uint8) or 65536 (uint16).  counts: int64, as np.histogram returns.
 * The _device form takes a device image and a device scratch of 3 * nbins uint32. */
MI_API int mi_histogram(int device, const void* host_img, int height, int width, int dtype, int mode,
                 int subsample, int fast, double mask_size, int64_t* counts);
MI_API int mi_histogram_device(int device, void* stream, const void* dev_img, void* dev_scratch, int height,
                        int width, int dtype, int mode, int subsample, int fast, double mask_size,
                        int64_t* counts);
/* the same for n frames with ONE host round trip: frame k's histogram lands in counts + k * nch * nbins; dev_scratch holds
 * n * 3 * nbins uint32 (the resident pipeline balances a whole batch of warped frames behind one synchronisation instead
 * of one per frame: balance.py:181-201 for the GAMMA / MATCH_HIST maps, whose tables SciPy builds on the host) */
MI_API int mi_histogram_device_batch(int device, void* stream, const void* const* dev_imgs, int n, void* dev_scratch,
                              int height, int width, int dtype, int mode, int subsample, int fast, double mask_size,
                              int64_t* counts);
/* mi_apply_lut: dst[p][c] = lut[nlut == 1 ? 0 : c][src[p][c]] -- cv2.LUT (uint8) / np.take (uint16)
 * as balance.py:30-50 applies them: one table for all channels (LUMI) or one per channel (RGB).
 * lut: nlut tables of nbins entries of the image dtype. */
MI_API int mi_apply_lut(int device, const void* host_src, void* host_dst, int height, int width, int dtype,
                 const void* host_lut, int nlut);
MI_API int mi_apply_lut_device(int device, void* stream, const void* dev_src, void* dev_dst, size_t npixels,
                        int dtype, const void* dev_lut, int nlut);
/* The whole LINEAR correction of one device frame, in place, enqueued on `stream` without any host round trip: histogram
 * (as mi_histogram_device) -> LinearMap's table (balance.py:87-105: ratio = reference mean / histogram mean over the bins
 * [lo, hi), table[i] = trunc(clip(i * ratio, 0, max)), float64) -> table apply.  mode 1 (luminance): one table for the
 * three channels; mode 0: one per channel, the channels below `first_channel` unchanged (1 = HSV / HLS: hue passes).
 * ref_means: host array of the reference frame's means, one per corrected channel.  dev_hist_scratch: 3 * nbins uint32;
 * dev_lut: 3 * nbins entries of the image dtype; dev_corr_out: NULL or device array that receives the ratios.
 * A histogram that is empty inside [lo, hi) -- np.average raises ZeroDivisionError in the reference there, which an
 * asynchronous call cannot do -- gives ratio 1 (the channel is left unchanged). */
MI_API int mi_balance_linear_device(int device, void* stream, void* dev_img, void* dev_hist_scratch, void* dev_lut,
                             int height, int width, int dtype, int mode, int subsample, int fast, double mask_size,
                             int lo, int hi, int first_channel, const double* ref_means, double* dev_corr_out);

/* 8-bit BGR <-> HSV / HLS (cv2.cvtColor COLOR_BGR2HSV, _HSV2BGR, _BGR2HLS, _HLS2BGR): the pre- and post-processing of the
 * HSV / HLS channel modes of BalanceFrames (balance.py:340-363: SVCorrection / LSCorrection balance S and V, or L and S,
 * and leave the hue alone).  uint8 only, as in OpenCV (MI_ERR_UNSUPPORTED for 16-bit; the reference raises there too).
 * In place is allowed (dev_dst == dev_src). */
enum { MI_CVT_BGR2HSV = 0, MI_CVT_HSV2BGR = 1, MI_CVT_BGR2HLS = 2, MI_CVT_HLS2BGR = 3 };
MI_API int mi_cvt_color(int device, const void* host_src, void* host_dst, int height, int width, int dtype, int code);
MI_API int mi_cvt_color_device(int device, void* stream, const void* dev_src, void* dev_dst, size_t npixels, int dtype,
                        int code);

/* ---- Vignetting and MaskNoise: the corrections a frame gets before it is aligned (reference algorithms/vignetting.py,
 * algorithms/noise_detection.py:145-198; kernels in csrc/kernels_prestack.hpp).
 * mi_subsampled_size: the size of an image sub-sampled by `subsample` as utils.py:79-86 does it (fast: img[::s, ::s] ->
 * ceil(dim / s); otherwise cv2.resize(INTER_AREA) -> round-half-even(dim / s)).
 * mi_radial_ring_sums_device: vignetting.py:23-39 (radial_mean_intensity) over the sub-sampled 8-bit gray image of a device
 * BGR frame (vignetting.py:52-55: img >> 8 for 16-bit, integer BGR2GRAY, then the sub-sampling), as integers: sums[i] and
 * counts[i] of the pixels with radii[i] <= d < radii[i + 1], d = sqrt((x - ws/2)^2 + (y - hs/2)^2) in float64 on the
 * sub-sampled grid.  radii: host array of r_steps + 1 doubles (np.linspace(0, r_max, r_steps + 1)); sums / counts: host
 * arrays of r_steps.  The ring mean is sums[i] / counts[i] (NaN where counts[i] == 0).  dev_scratch:
 * mi_radial_ring_scratch_bytes(r_steps) bytes.  r_steps <= 2048.  Synchronises `stream`. */
MI_API int mi_subsampled_size(int height, int width, int subsample, int fast, int* hs, int* ws);
MI_API size_t mi_radial_ring_scratch_bytes(int r_steps);
MI_API int mi_radial_ring_sums_device(int device, void* stream, const void* dev_img, void* dev_scratch, int height, int width,
                               int dtype, int subsample, int fast, int r_steps, const double* radii, uint64_t* sums,
                               uint32_t* counts);
/* mi_vignette_apply_device: vignetting.py:84-97 (correct_vignetting) with the model's parameters given: per pixel
 * gain = clip(sigmoid_model(r, i0, k, r0) / v0, 1e-6, 1), blended (1 - max_correction) + gain * max_correction when
 * max_correction < 1, 1 where min(B, G, R) < threshold; dst = trunc(clip(src / gain, 0, max)), float64.  uint8 / uint16 BGR,
 * 16-byte aligned, in place allowed (dev_dst == dev_src).  Enqueued on `stream`, no synchronisation. */
MI_API int mi_vignette_apply_device(int device, void* stream, const void* dev_src, void* dev_dst, int height, int width,
                             int dtype, double i0, double k, double r0, double v0, double max_correction, double threshold);
/* mi_mask_noise_device: noise_detection.py:171-198 for n hot pixels: dev_coords = n (y, x) int32 pairs; every channel of
 * each of them becomes the truncated mean (method 0) or median (method 1) of the non-zero values of the UNCORRECTED channel
 * in the kernel_size x kernel_size window clipped to the image (unchanged when there is none).  dev_stage: n * 3 uint32.
 * dev_dst may be dev_src (in place) or a distinct image, which first receives a copy of the source.  Coordinates outside
 * the image are ignored.  Enqueued on `stream`, no synchronisation. */
enum { MI_MASK_NOISE_MEAN = 0, MI_MASK_NOISE_MEDIAN = 1 };
MI_API int mi_mask_noise_device(int device, void* stream, const void* dev_src, void* dev_dst, int height, int width,
                         int dtype, const int32_t* dev_coords, int n, int kernel_size, int method, void* dev_stage);

/* ---- NoiseDetection (noise_detection.py:21-143).
 * mi_frame_accumulate_device: dev_sum[i] += sum over the n contiguous uint8 frames of frame[i]; dev_sum: uint32, 16-byte
 * aligned, zeroed by the caller before the first batch; exact below 2^24 frames.  Enqueued, no synchronisation.
 * mi_hot_pixel_map_device: mean = sum / n_frames (truncated, uint8) -> cv2.GaussianBlur(mean, (blur_size, blur_size), 0) for
 * blur_size 3, 5, 7 (OpenCV's fixed small kernels in its 8.8 fixed-point path, BORDER_REFLECT101; MI_ERR_UNSUPPORTED
 * otherwise) -> |mean - blur| > thresholds[c] per channel -> dev_map (H x W uint8, 255 where any channel is hot); dev_mean:
 * NULL or H x W x 3 uint8 that receives the mean image; counts[4] (host): hot pixels in the map and in channels 0, 1, 2;
 * dev_counts: 16 bytes of device scratch.  Synchronises `stream`. */
MI_API int mi_frame_accumulate_device(int device, void* stream, const void* dev_frames, int n, size_t elements_per_frame,
                               void* dev_sum);
MI_API int mi_hot_pixel_map_device(int device, void* stream, const void* dev_sum, int n_frames, int height, int width,
                            int blur_size, const int* thresholds, void* dev_mean, void* dev_map, void* dev_counts,
                            uint32_t* counts);

/* ---- Post-stack denoise (reference algorithms/denoise.py -> cv2.fastNlMeansDenoising on a three-channel frame; kernel in
 * csrc/kernels_denoise.hpp): non-local means, all three channels filtered jointly.  MI_U8: squared differences (NORM_L2), 32-bit
 * sums; MI_U16: absolute differences (NORM_L1), 64-bit sums.  Window sizes are forced odd as OpenCV does (2 * (size / 2) + 1);
 * borders are BORDER_REFLECT_101 over search / 2 + template / 2 pixels.  Per output pixel p and channel c
 *     out[p, c] = (sum_q w(p, q) * in[q, c] + W / 2) / W,   w(p, q) = table[d(p, q) >> shift],   W = sum_q w(p, q)
 * with q over the search window around p and d the patch distance summed over the template window and the channels.
 * `table`: HOST array of table_len uint32 weights, the non-zero prefix of the weight table (entries at and past table_len are
 * zero; table[0] > 0); `shift`: the smallest p with 2^p >= (2 * (template_size / 2) + 1)^2.  The library builds none of it:
 * shinestacker_amd/denoise.py does.  template_size 1-11 and search_size 1-21, MI_ERR_UNSUPPORTED beyond.
 * The weights are the caller's responsibility: for MI_U8 sum_q w * 255 must fit 32 bits (the builder's fixed-point multiplier
 * INT_MAX / (search^2 * 255) guarantees it); larger weights wrap the sums -- wrong numbers, no fault.
 * mi_nlm_denoise: host frames (host_dst may be host_src).  mi_nlm_denoise_device: a frame resident in device memory,
 * dev_src != dev_dst; runs on `stream` and is synchronous by design: it allocates, uploads and frees its copy of the table and
 * waits for `stream` before it returns, so it cannot be queued behind later work (a once-per-job filter of milliseconds). */
MI_API int mi_nlm_denoise(int device, const void* host_src, void* host_dst, int height, int width, int dtype,
                   const uint32_t* table, int table_len, int shift, int template_size, int search_size);
MI_API int mi_nlm_denoise_device(int device, const void* dev_src, void* dev_dst, int height, int width, int dtype,
                          const uint32_t* table, int table_len, int shift, int template_size, int search_size, void* stream);

/* ---- Unsharp mask (reference algorithms/sharpen.py: cv2.GaussianBlur(image, (0, 0), radius), then cv2.addWeighted or the
 * thresholded NumPy combine; kernel in csrc/kernels_unsharp.hpp): blur and combine in one pass, the blurred frame never leaves LDS.
 * `taps`: HOST array of `ksize` uint32 fixed-point Gaussian taps, 8 fractional bits for MI_U8 and 16 for MI_U16, summing to
 * exactly 256 / 65536 (OpenCV's getGaussianKernelBitExact + error diffusion; shinestacker_amd/sharpen.py builds them, the
 * library evaluates no exp).  ksize odd, 1 (the identity blur) to 33.  Blur: exact integer row and column sums,
 * (S + half) >> 16 / 32, saturated, BORDER_REFLECT_101 reflected as often as it takes.
 * threshold == 0: out = saturate(round_half_even(f32(f32(1 + amount) * in) + f32(f32(-amount) * blurred))), float32, no fused
 * multiply-add.  threshold != 0: where |in - blurred| > f32(threshold), out = trunc(clip(f32(in + f32(f32(amount) * (in -
 * blurred))))), elsewhere out = in.  `threshold` is in sample units (the reference multiplies its argument by 256 for 16-bit
 * frames before this point; so does the Python layer).
 * MI_ERR_INVALID: null pointers, an even or oversized ksize, taps with another sum, a non-finite amount or threshold, and for
 * the device form dev_src == dev_dst.  mi_unsharp_mask: host frames (host_dst may be host_src).  mi_unsharp_mask_device: a frame
 * resident in device memory; the launch is queued on `stream` and not waited for (the taps travel in the kernel arguments). */
MI_API int mi_unsharp_mask(int device, const void* host_src, void* host_dst, int height, int width, int dtype,
                    const uint32_t* taps, int ksize, double amount, double threshold);
MI_API int mi_unsharp_mask_device(int device, void* stream, const void* dev_src, void* dev_dst, int height, int width, int dtype,
                           const uint32_t* taps, int ksize, double amount, double threshold);

/* ---- Stereo views from the depth map (csrc/kernels_stereo.hpp; no reference counterpart) ----
 * The frame re-rendered from a viewpoint shifted sideways: every source pixel moves along its row by
 * d = rint(f32(shift) * (t - f32(pivot))) pixels, t = clamp(depth / f32(n_frames - 1), 0, 1) (1 - t with near_first; 0 for a single
 * frame), all float32 and separately rounded; where several land on one target the largest t wins; a target nothing landed on
 * takes the nearer-to-the-background (smaller t, left on a tie) of the nearest filled targets to its left and right, the
 * source pixel itself when the row has none.  Samples are copied, never computed.  The header of kernels_stereo.hpp is the
 * specification; tests/stereo_restatement.py is held to it bit for bit.
 * `img`, `out`: height x width x 3 of `dtype` (MI_U8 / MI_U16); `depth`: height x width float32 in frame numbers, as the
 * depth map entry points write it.  MI_ERR_INVALID: null pointers, another dtype, n_frames < 1, a shift that is not finite,
 * exceeds 64 in size or whose ceil(|shift|) does not stay below width, a pivot outside [0, 1], near_first other than 0 / 1,
 * and for the device form dev_img == dev_out -- all before any device call.
 * mi_stereo_view: host frames (host_out may be host_img).  mi_stereo_view_device: frames resident in device memory; the
 * launch is queued on `stream` and not waited for. */
MI_API int mi_stereo_view(int device, const void* host_img, const void* host_depth, void* host_out, int height, int width, int dtype,
                   int n_frames, double shift, double pivot, int near_first);
MI_API int mi_stereo_view_device(int device, void* stream, const void* dev_img, const void* dev_depth, void* dev_out, int height,
                          int width, int dtype, int n_frames, double shift, double pivot, int near_first);
/* Two views of height x width x 3 composed on the device, queued on `stream`: side by side into height x 2 width x 3 (left
 * then right: MI_STEREO_PARALLEL, right then left: MI_STEREO_CROSS), or the red-cyan anaglyph, height x width x 3 with BGR
 * channel 2 from the left view and channels 0 and 1 from the right one (MI_STEREO_ANAGLYPH; its three frames start on 4-byte
 * boundaries).  A copy of samples; `dev_out` is a buffer of its own. */
enum {
    MI_STEREO_PARALLEL = 0,
    MI_STEREO_CROSS = 1,
    MI_STEREO_ANAGLYPH = 2
};
MI_API int mi_stereo_compose_device(int device, void* stream, const void* dev_left, const void* dev_right, void* dev_out, int height,
                             int width, int dtype, int layout);

/* ---- Brush retouching (reference retouch/brush_tool.py, brush_preview.py, image_editor_ui.py copy_brush_area_to_master; kernels
 * in csrc/kernels_brush.hpp, whose header is the specification): a source frame painted into the master frame, a whole stroke
 * in one launch.  Per pixel, over the stamps whose square |x - cx| <= radius, |y - cy| <= radius holds it, in stroke order:
 * M = min(max(M + table[y - cy + radius][x - cx + radius], 0), 1) from M = 0, then once e = clip(M * opacity, 0, 1) and
 * master = trunc(clip(master * (1 - e) + source * e, 0, max)), float64 throughout and without fused multiply-add.  Pixels no
 * square holds are not written.
 * `master` (written in place), `source`: height x width x 3 of `dtype` (MI_U8 / MI_U16), two distinct frames.  `table`:
 * (2 radius + 1)^2 doubles, the reference's create_brush_mask(2 radius + 1, hardness, opacity) * flow / 100 (shinestacker_amd/
 * retouch.py builds it; the library evaluates no cosine).  `stamps`: n_stamps (x, y) int32 centres, anywhere.  `opacity`:
 * the brush's opacity / 100, which the reference applies a second time in the blend.  `mask`: optional height x width doubles
 * that receive M (0 where nothing was painted).
 * MI_ERR_INVALID, before any device call: null pointers, master == source, another dtype, a radius outside [2, 500], n_stamps
 * outside [0, 65536], an opacity outside [0, 1], and for the device form a box that leaves the frame.
 * mi_brush_stroke_device: everything resident in device memory; `box` (HOST, 4 int32: x_start, y_start, x_end, y_end) is the region
 * the launch covers -- the union of the stamps' footprints clipped to the frame; an empty box launches nothing.  Queued on
 * `stream`, not waited for.  mi_brush_stroke: host arrays; `area` (optional, 4 int32) receives that union, (0, 0, 0, 0) when
 * every stamp misses the frame. */
MI_API int mi_brush_stroke_device(int device, void* stream, void* dev_master, const void* dev_source, int height, int width, int dtype,
                           const double* dev_table, int radius, const int32_t* dev_stamps, int n_stamps, const int32_t* box,
                           double opacity, double* dev_mask);
MI_API int mi_brush_stroke(int device, void* host_master, const void* host_source, int height, int width, int dtype,
                    const double* host_table, int radius, const int32_t* host_stamps, int n_stamps, double opacity,
                    double* host_mask, int32_t* area);
/* The blend alone, over the whole frame, from a height x width float64 mask (the reference's apply_mask): e = clip(mask * opacity,
 * 0, 1), master = trunc(clip(master * (1 - e) + source * e, 0, max)), in place.  The device form is queued on `stream`. */
MI_API int mi_blend_mask_device(int device, void* stream, void* dev_master, const void* dev_source, const double* dev_mask, int height,
                         int width, int dtype, double opacity);
MI_API int mi_blend_mask(int device, void* host_master, const void* host_source, const double* host_mask, int height, int width,
                  int dtype, double opacity);

/* ---- Depth-selected composite (csrc/kernels_composite.hpp, whose header is the specification; no reference counterpart) ----
 * Every pixel taken from the frame the depth plane names.  Per pixel, float32, every operation rounded on its own:
 * d = depth (NaN -> 0) clamped to [0, n_frames - 1]; MI_COMPOSITE_NEAREST copies the three samples of frame rint(d) (ties to
 * even); MI_COMPOSITE_LINEAR takes k0 = floor(d), f = d - k0, k1 = min(k0 + 1, n_frames - 1) and stores a + f * (b - a) per
 * sample (a, b the samples of frames k0, k1; rint and a clamp for the integer types; a itself when f == 0).
 * A call holds `count` consecutive frames of the stack, global indices first .. first + count - 1, and writes the pixels with
 * first <= k0 < first + count - 1, or k0 == n_frames - 1 == first + count - 1; every other pixel of `out` keeps what it holds and
 * is not read in the frames.  Calls whose chunks overlap by one frame and cover [0, n_frames) give the one-call result.
 * `frame_ptrs`: HOST array of `count` frame addresses, height x width x 3 of `dtype` (MI_U8 / MI_U16 / MI_F32) each; `depth`:
 * height x width float32; `out`: height x width x 3 of `dtype`.  The frames and the depth plane are only read.
 * MI_ERR_INVALID, before any device call: null pointers (a null table entry too), another dtype or interp, count < 1, a chunk
 * outside [0, n_frames), count == 1 with n_frames > 1, n_frames > 2^24, an output that overlaps a frame or is the depth plane,
 * and for the device form a frame that is not aligned to its sample type, a depth plane off a 16-byte or an output off a 4-byte
 * boundary.
 * mi_depth_composite_device: the addresses are device addresses; they travel in the kernel arguments, 64 per launch (more frames:
 * several launches over overlapping sub-chunks), so the call allocates nothing, is queued on `stream` and waits for nothing.  mi_depth_composite: host frames; `host_out` is uploaded first, so that the
 * pixels of other chunks survive. */
enum {
    MI_COMPOSITE_LINEAR = 0,
    MI_COMPOSITE_NEAREST = 1
};
MI_API int mi_depth_composite_device(int device, void* stream, const void* const* frame_ptrs, int first, int count, int n_frames,
                              const void* dev_depth, void* dev_out, int height, int width, int dtype, int interp);
MI_API int mi_depth_composite(int device, const void* const* frame_ptrs, int first, int count, int n_frames, const void* host_depth,
                       void* host_out, int height, int width, int dtype, int interp);

/* ---- DepthMapStack: the second stacker behind the same plug-in boundary ----
 * Replaces the arithmetic of DepthMapStack.focus_stack (reference algorithms/depth_map.py:64-123) for
 * both float types: push = the first file loop (:67-75: read, img_bw, then per frame get_sobel_map :28-34
 * or get_laplacian_map :36-41 and the running np.max :88); finish = energies / max (:90), smooth_energy
 * (:43-52), get_focus_map (:54-62), the per-frame pyrDown / pyrUp weighted Laplacian pyramids (:94-112),
 * the collapse and np.clip(np.absolute()).astype (:117-123).  The handle keeps every pushed frame and one
 * float32 plane per frame in device memory (the reference re-reads every file in its second loop).
 * Parity: oracle/depth_map_oracle.py (OpenCV primitives restated, unpinned -- see DESIGN.md). */
enum { MI_DM_MAP_AVERAGE = 0, MI_DM_MAP_MAX = 1 };          /* constants.py:147-148 */
enum { MI_DM_ENERGY_LAPLACIAN = 0, MI_DM_ENERGY_SOBEL = 1 };  /* constants.py:145-146 */
typedef struct mi_dmap mi_dmap_t;
typedef struct mi_dmap_params {
    int32_t height, width;
    int32_t dtype;         /* MI_U8 / MI_U16: frames in, fused frame out                       */
    int32_t device;
    int32_t map_type;      /* MI_DM_MAP_*       (depth_map.py:11)                              */
    int32_t energy;        /* MI_DM_ENERGY_*    (:12)                                          */
    int32_t kernel_size;   /* cv2.Laplacian aperture, odd, <= 15 (:13)                         */
    int32_t blur_size;     /* cv2.GaussianBlur size, odd, <= 31 (:14)                          */
    int32_t smooth_size;   /* cv2.bilateralFilter diameter, <= 0: no smoothing, <= 31 (:15)    */
    int32_t levels;        /* blend pyramid levels, >= 1 (:17)                                 */
    float temperature;     /* softmax temperature of the MAX map (:16)                         */
    int32_t float_type;    /* MI_F32 / MI_F64 (:18, base_stack_algo.py:14-17)                  */
} mi_dmap_params_t;
MI_API void mi_dmap_default_params(mi_dmap_params_t* p);   /* constants.py:151-157 */
MI_API int mi_dmap_create(mi_dmap_t** out, const mi_dmap_params_t* params);
MI_API void mi_dmap_destroy(mi_dmap_t* d);
MI_API int mi_dmap_reset(mi_dmap_t* d);                    /* forget the frames, keep the buffers */
MI_API int mi_dmap_frames_pushed(const mi_dmap_t* d, int* n);
/* the MAX map's temperature as a double: mi_dmap_params_t carries it as a float, which is exact for float-32 stacks (NumPy
 * divides a float32 array by the float32 of a Python float) but not for float-64 ones (depth_map.py:60) */
MI_API int mi_dmap_set_temperature(mi_dmap_t* d, double temperature);
/* The stacker's steps one at a time, on n host planes of height x width -- the reference's public methods of the same
 * names (depth_map.py:28-62; its tests call them), run by the kernels of the fused path with the handle's options:
 *   stage 0  get_sobel_map      gray planes (float_type) -> |Sobel x| + |Sobel y|                (:28-34)
 *   stage 1  get_laplacian_map  gray planes (float_type) -> |Laplacian(GaussianBlur)|            (:36-41)
 *   stage 2  smooth_energy      energy planes (float_type) -> float32 planes, cv2.bilateralFilter (:43-52)
 *   stage 3  get_focus_map      n energy planes -> n weight planes; both float32 when smooth_size > 0 or float_type is
 *                               float-32, else float64; a zero total gives weight 0          (:54-62) */
MI_API int mi_dmap_planes(mi_dmap_t* d, int stage, const void* host_in, int n, void* host_out);
/* H x W x 3 BGR frame of `dtype`; row_stride_bytes 0 = packed.  The host form returns once the caller's
 * buffer may be reused; the device form copies on the handle's stream. */
MI_API int mi_dmap_push_frame(mi_dmap_t* d, const void* host_bgr, size_t row_stride_bytes);
MI_API int mi_dmap_push_frame_device(mi_dmap_t* d, const void* dev_bgr);
/* fused frame (dtype, H x W x 3) to host / device memory; both return after the work has completed */
MI_API int mi_dmap_finish(mi_dmap_t* d, void* host_out, size_t row_stride_bytes);
MI_API int mi_dmap_finish_device(mi_dmap_t* d, void* dev_out);

/* Read-only taps (tests): a copy of a plane the handle already holds, height x width, to host memory.  F = float_type;
 * W = float32 when smooth_size > 0 or float_type is float-32, else float64.  Each plane exists in one phase only; a tap
 * outside it returns MI_ERR_STATE before anything is read. */
enum {
    MI_DM_TAP_ENERGY_RAW = 0, /* F: energy of frame `frame` as pushed; between push and finish                        */
    MI_DM_TAP_ENERGY_IN = 1,  /* W: what the focus map divides for frame `frame` (normalised, smoothed, or the MAX
                                 map's relative exp((e - max) / T)); after finish                                     */
    MI_DM_TAP_TOTAL = 2,      /* W: sum over the frames of the planes above (`frame` ignored); after finish           */
    MI_DM_TAP_MAX = 3         /* W: MAX map only, maximum over the frames of the (smoothed) energies; after finish    */
};
MI_API int mi_dmap_tap(mi_dmap_t* d, int what, int frame, void* host_out);

/* The depth map of a finished stack, height x width float32: D = (sum_i in_i * i) / total over the MI_DM_TAP_ENERGY_IN planes,
 * i ascending, multiply and add rounded separately, in their type W; 0 where total == 0.  sigma > 0 smooths it as
 * mi_stack_depth_map does, in W, with w = total for the AVERAGE map and w = 1 for the MAX map.  Reads the state only.
 * MI_ERR_STATE before finish.  mi_dmap_depth_map_device: `dev_out` in device memory; waits for the handle's stream. */
MI_API int mi_dmap_depth_map(mi_dmap_t* d, double sigma, void* host_out);
MI_API int mi_dmap_depth_map_device(mi_dmap_t* d, double sigma, void* dev_out);
/* mi_dmap_depth_map(sigma) refined as mi_stack_depth_map_refined does: w = total for the AVERAGE map and 1 for the MAX map,
 * lo = 0, hi = N - 1.  MI_ERR_STATE before finish. */
MI_API int mi_dmap_depth_map_refined(mi_dmap_t* d, double sigma, const void* host_guide, int guide_dtype, int radius, double eps,
                              void* host_out);
MI_API int mi_dmap_depth_map_refined_device(mi_dmap_t* d, double sigma, const void* dev_guide, int guide_dtype, int radius, double eps,
                                     void* dev_out);

/* ---- raw Bayer mosaics in (kernels_demosaic.hpp; no reference counterpart: the reference reads developed frames) ----
 * A height x width mosaic of MI_U8 / MI_U16, one colour sample per site, becomes a height x width x 3 BGR frame of the same
 * dtype.  Per site: v' = min(white, (max(v - black[pos], 0) * gain_q[pos] + 2048) >> 12) with pos = 2 (y & 1) + (x & 1), then
 * the Malvar-He-Cutler 5 x 5 linear interpolation in integers over 16, clamp((sum + 8) >> 4, 0, white), BORDER_REFLECT_101 on
 * the mosaic.  Exact: tests/demosaic_restatement.py states it in NumPy and the kernel is held to it bit for bit. */
enum { MI_CFA_RGGB = 0, MI_CFA_BGGR = 1, MI_CFA_GRBG = 2, MI_CFA_GBRG = 3 };   /* the 2 x 2 cell at (y & 1, x & 1), row-major */
typedef struct mi_cfa {
    int32_t pattern;      /* MI_CFA_*                                                                            */
    int32_t black[4];     /* black level per cell position, >= 0                                                 */
    uint32_t gain_q[4];   /* round(gain * 4096) per cell position, <= 65535 (gain < 16): white balance, bit depth */
    int32_t white;        /* output clamp, 1 .. the dtype's maximum                                              */
} mi_cfa_t;
/* height, width >= 2 (odd sizes are fine).  MI_ERR_INVALID names the argument; the checks come before the first device call.
 * The device form enqueues on `stream`; the host form uploads, runs and downloads, and waits. */
MI_API int mi_demosaic_device(int device, void* stream, const void* dev_mosaic, void* dev_bgr, int height, int width, int dtype,
                              const mi_cfa_t* cfa);
MI_API int mi_demosaic(int device, const void* host_mosaic, void* host_bgr, int height, int width, int dtype, const mi_cfa_t* cfa);
/* One frame from host memory as its mosaic (the handle's height x width samples of in_dtype, MI_U8 / MI_U16; rows
 * row_stride_bytes apart, 0 = packed): a third of the bytes of mi_stack_push_frame over the host link.  The mosaic is
 * uploaded on a copy stream of the handle's mosaic stage and demosaiced behind the copy into a device buffer of batch_frames
 * BGR frames; a full buffer is fused as one batch, a partly filled one by whatever flushes pending host frames (finish, a tap,
 * mi_stack_sync_level, mi_stack_export_indices, a push of another kind).  Frames are fused in call order, mixed with
 * mi_stack_push_frame and mi_stack_push_frames_device as the calls came.  pinned != 0: the mosaic lies in pinned host memory
 * with contiguous rows and is read directly -- leave it alone until mi_stack_wait_uploads says so (MI_ERR_INVALID when it is
 * not pinned); else it goes through a pinned bounce buffer and may be reused on return.  Float-64 and MI_IMPL_SIMPLE handles
 * take the synchronous route: upload, demosaic, push, wait. */
MI_API int mi_stack_push_mosaic(mi_stack_t* s, const void* host_mosaic, size_t row_stride_bytes, const mi_cfa_t* cfa, int pinned);

/* ---- raw development around the demosaic: defect sites, colour matrix, tone curve (kernels_demosaic.hpp) ----
 * Integer and exact like the demosaic, each step optional; tests/develop_restatement.py states it in NumPy.
 *   step 0  defect sites, in place on the raw samples ahead of everything else: a listed site becomes (S + (k >> 1)) / k over
 *           its k valid neighbours (y -+ 2, x) and (y, x -+ 2) -- the same colour, black level and gain; valid: inside the
 *           image and not itself listed; k = 0 leaves the site.  Sites are linear indices y * width + x, int32, strictly
 *           ascending, each < height * width.
 *   step C  colour matrix on the demosaic's clamped output: matrix_q[3 i + j] = round(M[i][j] * 4096), i the output and j the
 *           input channel, both in R, G, B order; out_i = clamp((sum_j matrix_q[3 i + j] * in_j + 2048) >> 12, 0, cfa.white),
 *           arithmetic shift.  Per row sum_j |matrix_q[3 i + j]| <= 32767, so the sum fits int32.
 *   step D  tone curve: out = tone[out], a table of 256 (MI_U8) or 65536 (MI_U16) entries of the frame's dtype. */
enum { MI_DEVELOP_MATRIX = 1, MI_DEVELOP_TONE = 2 };
typedef struct mi_develop {
    int32_t flags;          /* MI_DEVELOP_* or-ed; 0: the plain demosaic                                    */
    int32_t matrix_q[9];    /* step C, read when MI_DEVELOP_MATRIX is set                                   */
    const void* dev_tone;   /* step D, device memory, read when MI_DEVELOP_TONE is set: it must stay valid  */
                            /* until the kernels enqueued with it have run                                  */
} mi_develop_t;
/* MI_ERR_INVALID names the argument; every check comes before the first device call: null pointers, a flag without its
 * table, the row-sum bound, height * width >= 2^31, n < 0 and, in the host form, a site >= height * width or a list that is
 * not strictly ascending (the device forms take a valid list as their precondition; a kernel leaves a site outside the
 * image alone).  mi_mosaic_defects_device: step 0 in place on `dev_mosaic`, enqueued on `stream`, not waited for; n == 0 (then
 * dev_sites may be null) enqueues nothing.  mi_develop_device: steps A to D, `dev_mosaic` is only read; enqueued, not waited
 * for.  mi_develop: the host form -- uploads, runs steps 0 to D, downloads and waits; matrix_q (9 ints) or NULL, host_tone
 * (the table in host memory) or NULL, host_sites (n ints) or NULL with n == 0. */
MI_API int mi_mosaic_defects_device(int device, void* stream, void* dev_mosaic, int height, int width, int dtype,
                                    const int32_t* dev_sites, int n);
MI_API int mi_develop_device(int device, void* stream, const void* dev_mosaic, void* dev_bgr, int height, int width, int dtype,
                             const mi_cfa_t* cfa, const mi_develop_t* develop);
MI_API int mi_develop(int device, const void* host_mosaic, void* host_bgr, int height, int width, int dtype, const mi_cfa_t* cfa,
                      const int32_t* matrix_q, const void* host_tone, const int32_t* host_sites, int n);
/* mi_stack_push_mosaic with development: step 0 runs on the handle's stream behind the mosaic's upload, in place on the
 * stage's device slot, and the developed demosaic follows it.  `develop` is copied by the call; its dev_tone and `dev_sites`
 * (device memory, n_sites ints, NULL with 0) are read by the queued kernels and must stay valid until the frame is fused
 * (mi_stack_sync, mi_stack_finish, mi_stack_reset or the handle's destruction).  Plain and developed pushes may mix on one
 * handle, frame by frame.  Everything else as mi_stack_push_mosaic. */
MI_API int mi_stack_push_mosaic_developed(mi_stack_t* s, const void* host_mosaic, size_t row_stride_bytes, const mi_cfa_t* cfa,
                                          const mi_develop_t* develop, const int32_t* dev_sites, int n_sites, int pinned);

/* ---- linear raw frames in: an already demosaiced frame developed without a demosaic (kernels_linear.hpp) ----
 * height x width x spp samples of MI_U8 / MI_U16 in file order (R, G, B; spp 1: one grey sample per pixel) become a
 * height x width x 3 BGR frame of the same dtype in one pass.  Per sample: v' = min(white, (max(v - black[c], 0) * gain_q[c] +
 * 2048) >> 12), c the sample's channel (0 at spp 1, where b = g = r = v'); then steps C and D of mi_develop_t on (b, g, r), as
 * behind the demosaic.  Exact: tests/linear_restatement.py states it in NumPy and the kernel is held to it bit for bit. */
typedef struct mi_linear {
    int32_t black[3];     /* black level per channel (R, G, B), >= 0; spp 1 reads entry 0                      */
    uint32_t gain_q[3];   /* round(gain * 4096) per channel, <= 65535: white balance, bit depth; spp 1: entry 0 */
    int32_t white;        /* output clamp, 1 .. the dtype's maximum                                            */
    int32_t spp;          /* samples per pixel: 1 or 3                                                         */
} mi_linear_t;
/* height, width >= 1 with height * width * 3 < 2^32.  MI_ERR_INVALID names the argument; the checks come before the first
 * device call.  mi_linear_develop_device: `develop` may be null (step A alone); the pointers are aligned to their samples
 * (4-byte aligned ones take the wide path); enqueued on `stream`, not waited for.  mi_linear_develop: the host form -- uploads,
 * runs, downloads and waits; matrix_q (9 ints) or NULL, host_tone (the table in host memory) or NULL. */
MI_API int mi_linear_develop_device(int device, void* stream, const void* dev_samples, void* dev_bgr, int height, int width, int dtype,
                                    const mi_linear_t* linear, const mi_develop_t* develop);
MI_API int mi_linear_develop(int device, const void* host_samples, void* host_bgr, int height, int width, int dtype,
                             const mi_linear_t* linear, const int32_t* matrix_q, const void* host_tone);
/* the pixels one workgroup of linear_develop takes of frames of `dtype` (for tests that aim at its edges); 0: unknown dtype */
MI_API int mi_linear_span(int dtype);

/* ---- raw calibration frames: master dark / flat, the flat's gain table, (raw - dark) * flat_gain (kernels_calib.hpp) ----
 * Integer and exact, on height x width mosaics of MI_U8 / MI_U16 (height, width >= 2, height * width < 2^31), maxv the dtype's
 * maximum, pos = 2 (y & 1) + (x & 1); nothing depends on the colour pattern.  tests/calib_restatement.py states it in NumPy.
 *   master     n exposures, 1 <= n <= 32, 0 <= 2 reject < n.  Per site the samples sorted ascending s[0 .. n - 1],
 *              m = n - 2 reject, S = s[reject] + ... + s[n - reject - 1], out = (S + (m >> 1)) / m: reject 0 the rounded mean,
 *              (n - 1) / 2 the median (even n: the rounded mean of the two middle samples), between: min/max rejection.
 *   flat gain  f = max(F - B, 0) per site, B the flat-dark (a dark frame at the flat's exposure) or cfa.black[pos]; S_p the sum
 *              of f over the sites of position p and N_p their number.  gain = 16384 where f == 0 or S_p == 0, else
 *              min(65535, (2 * 16384 * S_p + N_p f) / (2 N_p f)): the position's mean over the site's value in Q14, rounded.
 *              Normalised per position, so a flat does not change the white balance.  A uint16 table, height x width.
 *   calibrate  in place on the raw samples, ahead of step 0:  e = max(v - (dark[site] or cfa.black[pos]), 0);
 *              e' = (e * gain[site] + 8192) >> 14 with a flat, else e;  out = min(maxv, e' + cfa.black[pos]).  The pedestal is
 *              put back: a calibrated mosaic is an ordinary mosaic for step 0 and steps A to D, which follow in that order.
 * Of `cfa` only black[] is read, and all of it is checked. */
enum { MI_CALIB_DARK = 1, MI_CALIB_FLAT = 2 };
typedef struct mi_calib {
    int32_t flags;              /* MI_CALIB_* or-ed; 0: nothing is done                                        */
    const void* dev_dark;       /* height x width of the mosaic's dtype, device memory, read under MI_CALIB_DARK */
    const uint16_t* dev_gain;   /* height x width Q14 gains, device memory, read under MI_CALIB_FLAT            */
} mi_calib_t;
/* MI_ERR_INVALID names the argument; every check comes before the first device call: null pointers, height or width < 2,
 * another dtype, n outside [1, 32], reject < 0 or 2 reject >= n, unknown flags, a flag whose pointer is null,
 * height * width >= 2^31.  The device forms enqueue on `stream` and do not wait; the host forms upload, run, download and wait.
 * mi_mosaic_master_device: `dev_frames` holds the n mosaics one behind the other.  mi_mosaic_master: `host_frames` is a HOST
 * array of n host pointers.  mi_flat_gain*: the flat-dark may be null.  mi_mosaic_calibrate_device: in place; flags == 0
 * enqueues nothing and touches no device.  mi_mosaic_calibrate: host_dark / host_gain may each be null; host_out may equal
 * host_mosaic. */
MI_API int mi_mosaic_master_device(int device, void* stream, const void* dev_frames, int n, int height, int width, int dtype,
                                   int reject, void* dev_out);
MI_API int mi_mosaic_master(int device, const void* const* host_frames, int n, int height, int width, int dtype, int reject,
                            void* host_out);
MI_API int mi_flat_gain_device(int device, void* stream, const void* dev_flat, const void* dev_flat_dark, int height, int width,
                               int dtype, const mi_cfa_t* cfa, uint16_t* dev_gain_out);
MI_API int mi_flat_gain(int device, const void* host_flat, const void* host_flat_dark, int height, int width, int dtype,
                        const mi_cfa_t* cfa, uint16_t* host_gain_out);
MI_API int mi_mosaic_calibrate_device(int device, void* stream, void* dev_mosaic, int height, int width, int dtype,
                                      const mi_cfa_t* cfa, const mi_calib_t* calib);
MI_API int mi_mosaic_calibrate(int device, const void* host_mosaic, void* host_out, int height, int width, int dtype,
                               const mi_cfa_t* cfa, const void* host_dark, const uint16_t* host_gain);
/* mi_stack_push_mosaic with calibration: the calibration kernel runs on the handle's stream behind the mosaic's upload, in
 * place on the stage's device slot; step 0 (n_sites > 0) and the demosaic -- developed when `develop` is not null -- follow
 * it, and the slot is released behind all of them.  `calib` and `develop` are copied by the call; the device tables they and
 * `dev_sites` point to must stay valid until the handle is synchronised (mi_stack_sync, mi_stack_finish, mi_stack_reset or its
 * destruction).  Plain, developed and calibrated pushes may mix on one handle, frame by frame.  Everything else as
 * mi_stack_push_mosaic. */
MI_API int mi_stack_push_mosaic_calibrated(mi_stack_t* s, const void* host_mosaic, size_t row_stride_bytes, const mi_cfa_t* cfa,
                                           const mi_calib_t* calib, const mi_develop_t* develop, const int32_t* dev_sites,
                                           int n_sites, int pinned);

/* ---- lens correction: radial distortion and lateral chromatic aberration, one remap per frame (kernels_lens.hpp) ----
 * The radial part of DNG's WarpRectilinear per colour plane, destination -> source, on height x width x 3 BGR frames of
 * MI_U8 / MI_U16.  tests/lens_restatement.py states it in NumPy.  For the destination pixel (x, y) and plane c, every step in
 * double and every operation rounded once (nothing fused):
 *   dx = x - cx, dy = y - cy;  R2 = the largest dx*dx + dy*dy of the four corner pixels;  inv = 1.0 / R2, 0.0 when R2 == 0
 *   u = (dx*dx + dy*dy) * inv;  s = ((k3*u + k2)*u + k1)*u + k0     with k0..k3 = k[4 * c .. 4 * c + 3]
 *   px = min(max(cx + dx*s, -1.0), width),  py = min(max(cy + dy*s, -1.0), height)
 *   X = (int)rint(px * 32), Y = (int)rint(py * 32): 1/32 pixel, the alignment warp's grid;  sx = X >> 5, fx = X & 31, y alike
 *   v00, v01, v10, v11 = the plane's samples at (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1), indices clamped to the frame
 *   out = (v00*(32-fx)*(32-fy) + v01*fx*(32-fy) + v10*(32-fx)*fy + v11*fx*fy + 512) >> 10
 * The optional mask (height x width bytes) receives 1 where 0 <= X <= 32 (width - 1) and 0 <= Y <= 32 (height - 1) hold for all
 * three planes, else 0.  A plane of (1, 0, 0, 0) comes out as it went in, for any centre; a saturated frame stays saturated. */
typedef struct mi_lens {
    double k[12];               /* k[4 * c + i], c = B, G, R: the radial polynomial of plane c */
    double cx;                  /* the optical centre in pixels, column */
    double cy;                  /* and row */
} mi_lens_t;
/* MI_ERR_INVALID names the argument; every check comes before the first device call: a null source, destination or lens,
 * source == destination (the remap is a gather: distinct buffers), height or width < 1, height * width too large (2^31 pixels
 * or more, or a side of 2^26 or more: the positions are ints), another dtype, a coefficient that is not finite (its index is
 * named), a centre that is not finite or lies more than 2^30 pixels from the origin (cx + (x - cx) is then x to far below 1/64
 * pixel, which is what makes a plane of (1, 0, 0, 0) a copy).  The mask may be null.  mi_lens_remap_device enqueues on `stream`
 * and does not wait; mi_lens_remap uploads, runs, downloads and waits. */
MI_API int mi_lens_remap_device(int device, void* stream, const void* dev_src, void* dev_dst, void* dev_mask, int height, int width,
                                int dtype, const mi_lens_t* lens);
MI_API int mi_lens_remap(int device, const void* host_src, void* host_dst, void* host_mask, int height, int width, int dtype,
                         const mi_lens_t* lens);

/* ---- packed raw samples in: a raw file's sample bytes unpacked on the device (kernels_unpack.hpp) ----
 * A raw file (DNG: a TIFF) stores its mosaic as strips or tiles of 8, 10, 12, 14 or 16-bit samples.  `span` is one contiguous
 * run of the file's bytes that holds every segment, uploaded as it lies; seg_offsets[k] is the start of segment k inside it
 * (segments in any order, gaps between them), k = (ys / seg_height) * ceil(image_width / seg_width) + xs / seg_width for the
 * stored site (ys, xs).  Packing (TIFF FillOrder 1): every row of a segment starts on a byte boundary and takes
 * ceil(seg_width * bits / 8) bytes; 10, 12 and 14-bit samples follow each other most significant bit first in a big-endian
 * bit stream; 16-bit samples are two bytes in the file's byte order; edge tiles are stored at full tile size, the last strip
 * holds the rows that are left.  The output is the crop: height x width samples of `dtype` from (crop_y, crop_x), rows packed.
 * Per site: v = the sample; with a table v = table[min(v, table_len - 1)]; out = (v << shift) truncated to the dtype.
 * tests/unpack_restatement.py states it in NumPy. */
typedef struct mi_raw_layout {
    int32_t bits;           /* 8, 10, 12, 14 or 16                                                      */
    int32_t big_endian;     /* 16-bit samples: 1 when the most significant byte comes first             */
    int32_t image_height;   /* the stored image                                                         */
    int32_t image_width;
    int32_t tiled;          /* 0: strips (seg_width == image_width), 1: tiles                           */
    int32_t seg_height;     /* RowsPerStrip, or TileLength                                              */
    int32_t seg_width;      /* image_width, or TileWidth                                                */
    int32_t crop_y;         /* the output's origin in the stored image                                  */
    int32_t crop_x;
    int32_t height;         /* the output                                                               */
    int32_t width;
    int32_t shift;          /* 0 .. 15                                                                  */
    int32_t table_len;      /* entries of the linearisation table, 0: none                              */
    int32_t dtype;          /* of the output: MI_U8 for 8 bits, MI_U16 otherwise                        */
} mi_raw_layout_t;
/* MI_ERR_INVALID names the argument; every check comes before the first device call: null pointers, bits outside the five,
 * a dtype that does not belong to the bits, sizes < 1, a crop outside the stored image, strips narrower than the image,
 * height * width >= 2^31, span_bytes == 0 or >= 2^32, shift outside [0, 15], table_len outside [0, 65536], a table (uint16
 * entries) without its pointer or with 8-bit samples.  The host form and mi_stack_push_packed also refuse a segment that ends
 * outside the span; the device form takes offsets inside the span as its precondition (the kernel reads no byte at or beyond
 * span_bytes whatever they hold: such a byte counts as 0).  mi_raw_unpack_device enqueues on `stream` and does not wait;
 * mi_raw_unpack uploads, runs, downloads and waits. */
MI_API int mi_raw_unpack_device(int device, void* stream, const void* dev_span, size_t span_bytes, const uint32_t* dev_seg_offsets,
                                const mi_raw_layout_t* layout, const uint16_t* dev_table, void* dev_out);
MI_API int mi_raw_unpack(int device, const void* host_span, size_t span_bytes, const uint32_t* seg_offsets,
                         const mi_raw_layout_t* layout, const uint16_t* host_table, void* host_out);
/* mi_stack_push_mosaic_calibrated with the packed span uploaded instead of the mosaic: layout->height, width and dtype are the
 * handle's.  The span goes up on the mosaic stage's copy stream into a packed slot beside the stage's mosaic slot (sized on
 * first use, grown when a later span is larger), the offsets and the table behind it; the unpack kernel writes the mosaic slot
 * behind the copy, and calibration (`calib` may be null), defect repair and the plain or developed demosaic follow as they do
 * for a mosaic.  Packed, mosaic and BGR pushes may mix on one handle, frame by frame.  pinned != 0: the SPAN lies in pinned
 * host memory and is read directly, as in mi_stack_push_mosaic (mi_stack_wait_uploads tells when); seg_offsets and host_table
 * are copied by the call either way.  Float-64 and MI_IMPL_SIMPLE handles take the synchronous route. */
MI_API int mi_stack_push_packed(mi_stack_t* s, const void* host_span, size_t span_bytes, const uint32_t* seg_offsets,
                                const mi_raw_layout_t* layout, const uint16_t* host_table, const mi_cfa_t* cfa,
                                const mi_calib_t* calib, const mi_develop_t* develop, const int32_t* dev_sites, int n_sites,
                                int pinned);

/* ---- lossless-JPEG raw samples in: DNG Compression 7 decoded on the device (kernels_ljpeg.hpp) ----
 * Every strip or tile of such a file is one JPEG stream (ITU-T T.81 lossless, Huffman coded, SOF3).  The host reads the
 * stream's headers into one descriptor per segment, in grid order (k as for mi_raw_layout_t); the span is uploaded as it lies
 * and the kernel decodes the entropy-coded data: Huffman categories, differences, prediction per component (Ra: the sample
 * ncomp columns to the left, Rb: above, Rc: above-left; the first sample is predicted by 2^(precision-1), the rest of the
 * first line by Ra, the first sample of every other line by Rb), value = (prediction + difference) mod 2^16.  The sample of
 * line r, x, component c lands at segment row r, column x * ncomp + c; table, shift and crop then apply as in raw_unpack.
 * `layout` describes the grid, the crop and the output exactly as for mi_raw_unpack; its `bits` is the file's BitsPerSample
 * and only picks the dtype.  tests/ljpeg_restatement.py states all of it in Python. */
typedef struct mi_ljpeg_seg {
    uint32_t scan_off;      /* the entropy-coded data: its first byte in the span ...                   */
    uint32_t scan_bytes;    /* ... and its length; a marker inside it ends it earlier                   */
    int32_t x;              /* samples per line of one component: x * ncomp == the segment's columns    */
    int32_t y;              /* lines: the segment's rows                                                */
    uint8_t ncomp;          /* 1 or 2                                                                   */
    uint8_t predictor;      /* 1 .. 7                                                                   */
    uint8_t precision;      /* 2 .. 16                                                                  */
    uint8_t reserved;
    uint8_t counts[2][16];  /* per component: the number of codes of length 1 .. 16                     */
    uint8_t values[2][17];  /* per component: the categories (0 .. 16) in code order                    */
    uint8_t pad[10];        /* to 96 bytes                                                              */
} mi_ljpeg_seg_t;
#define MI_LJPEG_NOCODE 1u      /* status bit 0: a 16-bit prefix matched no code                             */
#define MI_LJPEG_OVERRUN 2u     /* status bit 1: the last sample needed bits from beyond the end of the data */
#define MI_LJPEG_UNDECODED 4u   /* status bit 2: a descriptor in device memory that the host forms refuse    */
#define MI_LJPEG_MAX_LINE 24576 /* predictors 2 .. 7 keep the line above on chip: segments up to this wide   */
/* Status: one uint32 per segment.  A flagged segment's samples are unspecified, but every one of them is written inside the
 * output; all other segments are exact.  Argument checks are those of mi_raw_unpack (the offsets array is replaced by `segs`:
 * "null segs") and, where the descriptors lie in host memory, per segment: ncomp 1 or 2, predictor 1 .. 7, precision 2 ..
 * layout->bits, x * ncomp and y equal to the segment's columns and rows, a predictor other than 1 only on segments of at most
 * MI_LJPEG_MAX_LINE columns, counts that fit the code space with at most 17 values none above 16, scan_off + scan_bytes
 * inside the span.  dev_span must be 4-byte aligned, dev_segs 16-byte, dev_out to its samples, dev_status to 4 bytes.
 * mi_raw_ljpeg_device enqueues on `stream` and does not wait; dev_status (one word per segment) may be null.  mi_raw_ljpeg
 * uploads, runs, downloads and waits; it returns MI_OK with the flags in status_out (may be null). */
MI_API int mi_raw_ljpeg_device(int device, void* stream, const void* dev_span, size_t span_bytes, const mi_ljpeg_seg_t* dev_segs,
                               const mi_raw_layout_t* layout, const uint16_t* dev_table, void* dev_out, uint32_t* dev_status);
MI_API int mi_raw_ljpeg(int device, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs,
                        const mi_raw_layout_t* layout, const uint16_t* host_table, void* host_out, uint32_t* status_out);
/* Three components: the tiles or strips of a LinearRaw frame, each one SOF3 stream with Nf = 3 (R, G, B interleaved along the
 * line) and X equal to the segment's PIXEL width; `layout` counts samples (seg_width = 3 X).  The same head as mi_ljpeg_seg_t
 * with three tables; everything stated above holds with ncomp == 3 -- placement, prediction, status bits, the
 * MI_LJPEG_MAX_LINE rule (in samples), the alignment rules.  The host form checks, per segment: ncomp == 3, x * 3 == the
 * segment's columns, the rest as mi_raw_ljpeg.  A descriptor in device memory that the host form would refuse sets
 * MI_LJPEG_UNDECODED and leaves its segment unwritten. */
typedef struct mi_ljpeg_seg3 {
    uint32_t scan_off;
    uint32_t scan_bytes;
    int32_t x;              /* pixels per line: x * 3 == the segment's columns                          */
    int32_t y;
    uint8_t ncomp;          /* 3                                                                        */
    uint8_t predictor;
    uint8_t precision;
    uint8_t reserved;
    uint8_t counts[3][16];
    uint8_t values[3][17];
    uint8_t pad[9];         /* to 128 bytes                                                             */
} mi_ljpeg_seg3_t;
MI_API int mi_raw_ljpeg3_device(int device, void* stream, const void* dev_span, size_t span_bytes, const mi_ljpeg_seg3_t* dev_segs,
                                const mi_raw_layout_t* layout, const uint16_t* dev_table, void* dev_out, uint32_t* dev_status);
/* the samples of one batch of raw_ljpeg3's walker, a whole number of pixels (for tests that aim at its edges) */
MI_API int mi_ljpeg3_batch(void);
MI_API int mi_raw_ljpeg3(int device, const void* host_span, size_t span_bytes, const mi_ljpeg_seg3_t* segs,
                         const mi_raw_layout_t* layout, const uint16_t* host_table, void* host_out, uint32_t* status_out);
/* mi_stack_push_packed for a lossless-JPEG span: the packed slot holds [span | descriptors | table], raw_ljpeg takes the place
 * of raw_unpack, and everything else -- routes, the pinned rule, the kernels behind it -- is the same.  Packed, compressed,
 * mosaic and BGR pushes may mix on one handle.  The stage ORs every frame's status flags into one device word of its own:
 * mi_stack_ljpeg_status waits for the stage, returns that word in *flags and clears it (0 on a handle that never took a
 * compressed frame). */
MI_API int mi_stack_push_ljpeg(mi_stack_t* s, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs,
                               const mi_raw_layout_t* layout, const uint16_t* host_table, const mi_cfa_t* cfa,
                               const mi_calib_t* calib, const mi_develop_t* develop, const int32_t* dev_sites, int n_sites,
                               int pinned);
MI_API int mi_stack_ljpeg_status(mi_stack_t* s, uint32_t* flags);
/* mi_stack_push_packed for a linear frame (mi_linear_t: an already demosaiced frame of spp = 1 or 3 samples per pixel): the
 * span goes up exactly as a packed or compressed span does and `layout` counts SAMPLES -- height the handle's, width the handle's
 * times linear->spp.  compressed == 0: `segs` are the uint32 segment offsets and raw_unpack runs; else they are the descriptors,
 * mi_ljpeg_seg3_t at spp 3 and mi_ljpeg_seg_t at spp 1, and raw_ljpeg3 / raw_ljpeg runs (status: mi_stack_ljpeg_status).  The
 * samples land in a slot of the stage that holds height x width x spp of them and mi_linear_develop_device's kernel takes them
 * to the batch's BGR frame (`develop` may be null); nothing is corrected per site, calibrated or repaired, and a site
 * correction set on the handle does not touch such a frame.  The checks are those of mi_raw_unpack / mi_raw_ljpeg[3], of
 * mi_linear_t and of mi_develop_t.  Linear, packed, compressed, mosaic and BGR pushes may mix on one handle, frame by frame. */
MI_API int mi_stack_push_linear(mi_stack_t* s, const void* host_span, size_t span_bytes, const void* segs, int compressed,
                                const mi_raw_layout_t* layout, const uint16_t* host_table, const mi_linear_t* linear,
                                const mi_develop_t* develop, int pinned);

/* ---- site corrections: the per-site corrections a raw file carries for its own samples (kernels_sitecorr.hpp) ----
 * DNG's BlackLevelDeltaH/V, GainMap, FixBadPixelsList and FixBadPixelsConstant, resolved on the host into integer tables.
 * Integer and exact, in place on height x width mosaics of MI_U8 / MI_U16 (height, width >= 2, height * width < 2^31), maxv the
 * dtype's maximum, pos = 2 (y & 1) + (x & 1); nothing depends on the colour pattern.  tests/sitecorr_restatement.py states it
 * in NumPy.  The steps run in this order, each under its flag, ahead of calibration and of step 0:
 *   bad list   MI_SITE_BAD_LIST: step 0's rule (mi_mosaic_defects_device) on `bad_sites`: linear indices, strictly ascending.
 *   bad const  MI_SITE_BAD_CONST: every site of the positions in `bad_phase_mask` (bit pos) whose value equals `bad_constant`
 *              becomes (S + (k >> 1)) / k over its valid neighbours (y -+ 2, x), (y, x -+ 2): inside the image and not
 *              themselves such a site, judged on the mosaic as it is when the step begins; k = 0 leaves the site.
 *   correct    b = cfa.black[pos] + delta_h[x] + delta_v[y] (each table under its flag, else 0), 0 <= b <= maxv for every site;
 *              e = max(v - b, 0).  Gain g in Q12: 4096 for a position whose gain[pos].nodes is null or without MI_SITE_GAIN,
 *              else with the row's axis entry (i, a) = row_axis[y], the column's (j, b) = col_axis[x], i1 = min(i + 1, mv - 1),
 *              j1 = min(j + 1, mh - 1) over the position's mv x mh nodes n:
 *                g = ((256 - a) * ((256 - b) * n[i][j] + b * n[i][j1]) + a * ((256 - b) * n[i1][j] + b * n[i1][j1]) + 32768) >> 16
 *              e' = (e * g + 2048) >> 12;  out = min(maxv, e' + cfa.black[pos]).  The pedestal is put back, as calibration
 *              does: the result is an ordinary mosaic for everything behind it.
 * Of `cfa` only black[] is read, and all of it is checked.  A position's axis tables have height and width entries; only the
 * entries of the position's own rows and columns are read.  Positions may share tables. */
enum { MI_SITE_DELTA_H = 1, MI_SITE_DELTA_V = 2, MI_SITE_GAIN = 4, MI_SITE_BAD_LIST = 8, MI_SITE_BAD_CONST = 16 };
typedef struct mi_site_axis {
    uint16_t node;              /* the first of the two nodes a row or column lies between, < mv or mh         */
    uint16_t weight;            /* of the second node, 0 .. 256                                                */
} mi_site_axis_t;
typedef struct mi_site_gain {
    const uint16_t* nodes;              /* mv x mh Q12 gains, row-major; NULL: the position has no map         */
    const mi_site_axis_t* row_axis;     /* height entries                                                      */
    const mi_site_axis_t* col_axis;     /* width entries                                                       */
    int32_t mv;                         /* node rows, 1 .. 4096                                                */
    int32_t mh;                         /* node columns, 1 .. 4096                                             */
} mi_site_gain_t;
typedef struct mi_site_correct {
    int32_t flags;                      /* MI_SITE_* or-ed; 0: nothing is done                                 */
    const int16_t* delta_h;             /* width entries, read under MI_SITE_DELTA_H                           */
    const int16_t* delta_v;             /* height entries, read under MI_SITE_DELTA_V                          */
    mi_site_gain_t gain[4];             /* per position, read under MI_SITE_GAIN (at least one with nodes)     */
    const int32_t* bad_sites;           /* n_bad sites, read under MI_SITE_BAD_LIST                            */
    int32_t n_bad;
    int32_t bad_constant;               /* 0 .. maxv, read under MI_SITE_BAD_CONST                             */
    int32_t bad_phase_mask;             /* 1 .. 15                                                             */
    void* dev_scratch;                  /* device form, under MI_SITE_BAD_CONST: 8 * ceil(height * width / 64)  */
                                        /* bytes of device memory, the bit plane between the step's two passes */
} mi_site_correct_t;
/* MI_ERR_INVALID names the argument; every check comes before the first device call: null pointers, height or width < 2,
 * another dtype, height * width >= 2^31, unknown flags, a flag without its table, mv or mh outside [1, 4096], n_bad < 0, a
 * constant outside [0, maxv], a mask outside [1, 15], MI_SITE_BAD_CONST without dev_scratch (device forms; the host form and a
 * handle's stage bring their own and ignore the member).  Where the tables lie in host memory (mi_mosaic_site_correct,
 * mi_stack_set_site_correction) also: a weight above 256, a node index outside its grid, b outside [0, maxv], a bad-site list
 * that is not strictly ascending or lies outside the image.  The device form takes those as its precondition (the kernel reads
 * no node outside a grid whatever an entry holds).
 * mi_mosaic_site_correct_device: every pointer of `sc` is device memory; enqueues on `stream`, does not wait; flags == 0
 * enqueues nothing and touches no device.  mi_mosaic_site_correct: every pointer of `sc` is host memory; uploads, runs,
 * downloads and waits; host_out may equal host_mosaic.  mi_mosaic_defects_const_device: the bad-const step alone, `dev_scratch`
 * as in the struct; enqueued, not waited for.  The scratch must stay valid until the kernels have run, and two streams must
 * not share one. */
MI_API int mi_mosaic_site_correct_device(int device, void* stream, void* dev_mosaic, int height, int width, int dtype,
                                         const mi_cfa_t* cfa, const mi_site_correct_t* sc);
MI_API int mi_mosaic_site_correct(int device, const void* host_mosaic, void* host_out, int height, int width, int dtype,
                                  const mi_cfa_t* cfa, const mi_site_correct_t* sc);
MI_API int mi_mosaic_defects_const_device(int device, void* stream, void* dev_mosaic, int height, int width, int dtype,
                                          int constant, int phase_mask, void* dev_scratch);
/* The site corrections of a handle's mosaic stage: `sc` (host memory, or NULL to clear) is checked against the handle's
 * height, width and in_dtype and copied by the call, tables included.  From then on every mi_stack_push_mosaic*,
 * mi_stack_push_packed and mi_stack_push_ljpeg uploads the tables into the stage's slot beside the mosaic (or the span, its
 * offsets and its linearisation table), and the steps above run on the handle's stream behind the upload or the unpack and
 * ahead of calibration, step 0 and the demosaic, with the push's own cfa.black.  It holds until it is replaced or cleared;
 * frames pushed before the call are not touched.  Float-64 and MI_IMPL_SIMPLE handles take the synchronous route. */
MI_API int mi_stack_set_site_correction(mi_stack_t* s, const mi_site_correct_t* sc);

/* ---- finishing a raw frame (csrc/kernels_finish.hpp; tests/finish_restatement.py is the definition) ----
 * A radial gain on the H x W mosaic (a DNG's FixVignetteRadial), in place, integer and exact: the centre in HALF pixels,
 * d2 = (2x - cx2)^2 + (2y - cy2)^2, D the largest d2 of the four corner sites, u = d2 / D looked up in `table`:
 * MI_RADIAL_NODES uint16 Q12 gains at u = i / 1024, blended with an 8-bit weight; out = min(maxv, (((v - black[pos]) g + 2048)
 * >> 12) + black[pos]), v - black clamped at 0.  The library derives D and the multiplier and shift that replace the
 * division from (height, width, cx2, cy2).  Refused before any device call: |cx2|, |cy2| above 2^24, D outside [1, 2^40), a
 * black level above the dtype's maximum. */
#define MI_RADIAL_NODES 1025
typedef struct mi_radial_gain {
    int32_t cx2;             /* the centre, half pixels */
    int32_t cy2;
    const uint16_t* table;   /* MI_RADIAL_NODES entries, Q12 */
} mi_radial_gain_t;
/* mi_mosaic_radial_gain_device: `rg->table` is device memory; enqueues on `stream`, does not wait.  mi_mosaic_radial_gain: the
 * table is host memory; uploads, runs, downloads and waits; host_out may equal host_mosaic. */
MI_API int mi_mosaic_radial_gain_device(int device, void* stream, void* dev_mosaic, int height, int width, int dtype,
                                        const mi_cfa_t* cfa, const mi_radial_gain_t* rg);
MI_API int mi_mosaic_radial_gain(int device, const void* host_mosaic, void* host_out, int height, int width, int dtype,
                                 const mi_cfa_t* cfa, const mi_radial_gain_t* rg);
/* Crop and orientation of a developed frame, out of place: src (height x width x 3, MI_U8 / MI_U16) -> dst, the crop
 * a[y, x] = src[crop_y + y, crop_x + x] (crop_h x crop_w) turned by the TIFF `orientation` 1..8:
 *   1: a  2: a[:, ::-1]  3: a[::-1, ::-1]  4: a[::-1]  (dst is crop_h x crop_w x 3)
 *   5: a transposed  6: a turned 90 degrees clockwise  7: a[::-1, ::-1] transposed  8: a turned 90 degrees anticlockwise
 *   (dst is crop_w x crop_h x 3).  The samples of a pixel keep their order.  src and dst must not overlap; 3 x height x width
 *   stays below 2^31.  The _device form enqueues on `stream` and does not wait; the host form uploads, runs, downloads, waits. */
MI_API int mi_frame_finish_device(int device, void* stream, const void* dev_src, void* dev_dst, int height, int width, int dtype,
                                  int crop_y, int crop_x, int crop_h, int crop_w, int orientation);
MI_API int mi_frame_finish(int device, const void* host_src, void* host_dst, int height, int width, int dtype, int crop_y,
                           int crop_x, int crop_h, int crop_w, int orientation);

/* ---- the feature estimator: FAST-9 corners, rotated box-sum descriptors, Hamming matching, RANSAC (kernels_features.hpp) ----
 * An algorithm of the ORB family of this library's own, pinned against nothing but tests/features_restatement.py, which states
 * every stage in NumPy.  All stages up to the matcher are integer and exact; RANSAC is double with one rounding per operation.
 *   gray     frame (height x width x channels, channels 1 or 3 in B, G, R order, MI_U8 / MI_U16) -> height x width bytes:
 *            16-bit samples lose their low byte, then (1868 B + 9617 G + 4899 R + 8192) >> 14.
 *   score    grey plane -> the FAST-9 score (16-pixel circle of radius 3, arcs of 9) of every pixel that exceeds `threshold`,
 *            lies at least 16 pixels from every border and survives the 3 x 3 suppression (greater than the four neighbours
 *            before it in raster order, not less than the four after it), 0 elsewhere; and the 256-bin histogram of those
 *            scores (bin 0 stays empty).
 *   extract  frame -> keypoints and descriptors of `levels` pyramid levels (level l + 1 = the rounded 2 x 2 mean of level l).
 *            Level l keeps the first n_features >> l of {score >= cut} by score descending, then y, then x, where cut is the
 *            smallest c > threshold with count(score >= c) <= max(4 (n_features >> l), 4096).  A keypoint is 5 int32
 *            (x, y, level, score, bin): level coordinates, bin = argmax_k (m10 C[k] + m01 S[k]) over the moments of the disc
 *            of radius 15.  A descriptor is 32 bytes: bit j = box5(p + a_j) < box5(p + b_j) for test j of the bin's pattern
 *            (`host_pattern`: 32 x 256 x 4 int8 (xa, ya, xb, yb), every offset within 13), least significant bit first.
 *            Levels follow each other in the output; *n_kp receives the total.  Zero keypoints is not an error.
 *   match    32-byte descriptors: per query 3 int32 -- the train descriptor with the smallest Hamming distance (lowest index
 *            on ties), that distance, and the smallest distance among all other train descriptors (0xFFFF when nt == 1).
 *   ransac   src, dst: n x 2 doubles; samples: k x 2 (MI_FEAT_SIMILARITY) or k x 4 (MI_FEAT_HOMOGRAPHY) match indices.  Per
 *            hypothesis the model (9 doubles, a 3 x 3 matrix row by row) and the number of matches with
 *            ex*ex + ey*ey <= thr*thr; -1 and a zero model for coincident sample points, a pivot below 1e-12 in magnitude
 *            or a sample index outside [0, n).
 * Every entry point returns MI_ERR_INVALID naming the argument before any device call.  The device forms of gray, score, match
 * and ransac enqueue on `stream` and do not wait; mi_feat_score_device clears dev_hist (256 uint32) itself.  Both extract forms
 * wait for their work: the cut and the sort of each level happen on the host. */
enum { MI_FEAT_SIMILARITY = 0, MI_FEAT_HOMOGRAPHY = 1 };
MI_API int mi_feat_gray_device(int device, void* stream, const void* dev_frame, int height, int width, int channels, int dtype,
                               void* dev_gray);
MI_API int mi_feat_gray(int device, const void* host_frame, int height, int width, int channels, int dtype, void* host_gray);
MI_API int mi_feat_score_device(int device, void* stream, const void* dev_gray, int height, int width, int threshold,
                                void* dev_score, void* dev_hist);
MI_API int mi_feat_score(int device, const void* host_gray, int height, int width, int threshold, void* host_score,
                         uint32_t* host_hist);
MI_API int mi_feat_extract_device(int device, void* stream, const void* dev_frame, int height, int width, int channels, int dtype,
                                  int levels, int n_features, int threshold, const int8_t* host_pattern, int max_kp,
                                  int32_t* host_kp, uint8_t* host_desc, int* n_kp);
MI_API int mi_feat_extract(int device, const void* host_frame, int height, int width, int channels, int dtype, int levels,
                           int n_features, int threshold, const int8_t* host_pattern, int max_kp, int32_t* host_kp,
                           uint8_t* host_desc, int* n_kp);
MI_API int mi_feat_match_device(int device, void* stream, const void* dev_query, int nq, const void* dev_train, int nt,
                                void* dev_out);
MI_API int mi_feat_match(int device, const void* host_query, int nq, const void* host_train, int nt, int32_t* host_out);
MI_API int mi_feat_ransac_device(int device, void* stream, const double* dev_src, const double* dev_dst, int n,
                                 const int32_t* dev_samples, int k, int model, double thr, int32_t* dev_counts,
                                 double* dev_models);
MI_API int mi_feat_ransac(int device, const double* host_src, const double* host_dst, int n, const int32_t* host_samples, int k,
                          int model, double thr, int32_t* host_counts, double* host_models);

/* ---- the feature estimator on resident frames: one handle, buffers kept, the cut and the sort on the device ----
 * The stages above for a batch of frames that lie in device memory, against a reference frame whose keypoints and descriptors
 * are extracted once.  Every device buffer for max_batch moving frames and the reference is allocated in create; estimate_batch
 * allocates nothing.  A frame is first sub-sampled by `subsample`: `fast` takes the pixels of img[::s, ::s]; otherwise each
 * channel is the rounded mean (a + b + c + d + 2) >> 2 of a 2 x 2 block, which is built for subsample == 2 on even sides only
 * (anything else without `fast` is MI_ERR_INVALID; subsample == 1 ignores `fast`).
 *   create          n_features <= 4096 here: the selection sorts a level's candidates, at most max(4 (n_features >> l), 4096) of
 *                   them, as 64-bit keys in one workgroup's LDS, and 16384 keys are 128 KiB of the 160 KiB a workgroup may use.
 *                   max_batch in [1, 128].  `host_pattern` as for mi_feat_extract.
 *   set_reference   extracts the reference frame's keypoints and descriptors and keeps them; waits once.
 *   estimate_batch  n <= max_batch frames: grey, pyramid, score, cut, selection, descriptors, matches per level (forwards, and
 *                   backwards for MI_FEAT_MATCH_HAMMING), the good matches -- cross-check sorted by distance then query, or the
 *                   ratio test distance < ratio * second distance in double in query order --, RANSAC over max_iters
 *                   hypotheses (<= 4096) and the winner: the largest count, the lowest index on ties, -1 when the count is below
 *                   the sample size or the frame has fewer than 3 (similarity) / 4 (homography) good matches.  The frame index
 *                   rides in every launch's grid: the number of launches does not depend on n.  The host waits twice: for the
 *                   good-match counts, from which it draws every pair's sample table (splitmix64(seed) % n_good, a repeat
 *                   within a row drawn again; the same seed for every pair) and uploads them; and for the results.  Per frame f:
 *                   n_good[f]; winner[f]; models[9 f ..] (zeros without a winner); inliers[f] = the winner's count;
 *                   mask[f max_matches ..] one byte per good match; src / dst[2 f max_matches ..] the matched level-0
 *                   positions in the moving frame / the reference, in the sub-sampled frame's pixels.  max_matches must be at
 *                   least the sum of n_features >> level.  MI_ERR_STATE before set_reference.
 *   tap             one stage's result for one frame of the last batch (frame_slot in [0, n); -1 = the reference, which has the
 *                   stages up to DESC), downloaded to host_out, *n_out = the number of rows:  GRAY the grey plane of pyramid
 *                   level `level` (rows of its width);  CUT per level 4 int32 (cut, count(score >= cut), keypoints kept, 0),
 *                   zeros for a level that is not scored;  KP 5 int32 per keypoint;  DESC 32 bytes per keypoint;  GOOD 3 int32
 *                   per good match (index into KP of the frame, of the reference, distance);  SAMPLES 2 or 4 int32 per
 *                   hypothesis;  COUNTS one int32 per hypothesis.  `capacity` = the bytes host_out holds: too few is
 *                   MI_ERR_INVALID.  `level` is read by GRAY only.
 *   stats           running totals since create: host waits and kernel launches this handle made (taps included). */
enum { MI_FEAT_MATCH_KNN = 0, MI_FEAT_MATCH_HAMMING = 1 };
enum {
    MI_FEAT_TAP_GRAY = 0,
    MI_FEAT_TAP_CUT = 1,
    MI_FEAT_TAP_KP = 2,
    MI_FEAT_TAP_DESC = 3,
    MI_FEAT_TAP_GOOD = 4,
    MI_FEAT_TAP_SAMPLES = 5,
    MI_FEAT_TAP_COUNTS = 6
};
typedef struct mi_feat_aligner* mi_feat_aligner_t;
MI_API int mi_feat_aligner_create(mi_feat_aligner_t* out, int device, int height, int width, int dtype, int channels,
                                  int subsample, int fast, int levels, int n_features, int threshold, const int8_t* host_pattern,
                                  int max_batch);
MI_API int mi_feat_aligner_set_reference(mi_feat_aligner_t fa, const void* dev_ref);
MI_API int mi_feat_aligner_estimate_batch(mi_feat_aligner_t fa, const void* const* dev_movs, int n, int match_method, double ratio,
                                          int kind, double rans_threshold, int max_iters, uint64_t seed, int max_matches,
                                          int32_t* n_good, int32_t* winner, double* models, int32_t* inliers, uint8_t* mask,
                                          double* src, double* dst);
MI_API int mi_feat_aligner_tap(mi_feat_aligner_t fa, int frame_slot, int what, int level, void* host_out, size_t capacity,
                               int* n_out);
MI_API int mi_feat_aligner_stats(mi_feat_aligner_t fa, uint64_t* waits, uint64_t* launches);
MI_API int mi_feat_aligner_destroy(mi_feat_aligner_t fa);

/* ---- baseline JPEG frames in: Huffman decode, inverse DCT, upsampling and colour on the device (kernels_jpeg.hpp) ----
 * The host reads the file's headers (jpeg.read) into one mi_jpeg_t, which always lies in HOST memory, and finds the restart
 * intervals: `offsets` holds n_intervals + 1 uint32 offsets into the span, offsets[i] the first data byte of interval i and
 * offsets[n_intervals] the end of the scan; an interval's bytes run to the next offset and end earlier at a marker (FF
 * followed by anything but 00).  The span is uploaded as it lies in the file.  Interval i decodes exactly min(dri, MCUs left)
 * MCUs from MCU i * dri on, in scan order, blocks within an MCU in T.81 order, predictors 0 at its start.  Per component the
 * coefficient plane is its padded block grid, mcus_y * v rows of mcus_x * h blocks of 64 int16 in natural order; the planes
 * of components 0, 1, 2 follow each other (mi_jpeg_coef_count int16 in all).  The render dequantises, runs the 13-bit
 * "slow integer" inverse DCT, upsamples chroma with the triangle filters on the component cropped to its own size, converts
 * YCbCr to BGR (a grey frame: the plane three times) and writes height x width x 3 uint8.  tests/jpeg_restatement.py states
 * all of it in Python.  One status word per interval, the MI_JPEG_* bits ORed; a flagged interval's blocks are unspecified
 * and every one is written inside the plane, all other intervals are exact. */
typedef struct mi_jpeg {
    int32_t width, height;  /* 1 .. 65535 each                                                          */
    int32_t ncomp;          /* 1 (grey) or 3 (YCbCr)                                                    */
    int32_t hmax, vmax;     /* the first component's sampling: (1,1), (2,1) or (2,2); (1,1) at ncomp 1  */
    int32_t dri;            /* MCUs per restart interval, 1 .. MI_JPEG_MAX_DRI (mi_jpeg_split_*: 1 .. MCUs) */
    int32_t n_intervals;    /* ceil(MCUs / dri)                                                         */
    int32_t reserved;
    uint8_t tq[4];          /* per component: its quantisation table, 0 .. 3                            */
    uint8_t td[4];          /* ... its DC table, 0 or 1                                                 */
    uint8_t ta[4];          /* ... its AC table, 0 or 1                                                 */
    uint8_t pad[4];
    uint8_t counts[4][16];  /* tables DC 0, DC 1, AC 0, AC 1: the number of codes of length 1 .. 16     */
    uint8_t values[4][256]; /* ... their symbols in code order                                          */
    uint8_t quant[4][64];   /* the quantisation tables in natural order, entries 1 .. 255               */
} mi_jpeg_t;                /* 1392 bytes */
#define MI_JPEG_NOCODE 1u   /* status bit 0: a 16-bit prefix matched no code                      */
#define MI_JPEG_OVERRUN 2u  /* status bit 1: bits were taken from beyond the interval's end       */
#define MI_JPEG_RUN 4u      /* status bit 2: a run carried the coefficient index past 63          */
#define MI_JPEG_MAX_DRI 8192 /* one wavefront walks an interval serially: at most the MCU row of a picture 65 535 wide */
/* Checks, each MI_ERR_INVALID naming the argument before any device call: null span, offsets, jpeg, output; span_bytes in
 * [1, 2^32); the fields of `jpeg` in the ranges above, n_intervals equal to ceil(MCUs / dri), every table a component
 * selects non-empty, counts that fit the code space with at most 256 values, DC symbols <= 15, quant entries >= 1; where the
 * offsets lie in host memory: non-decreasing and inside the span.  dev_span, dev_offsets and dev_status must be 4-byte
 * aligned, dev_coef 16-byte, dev_scratch 256-byte with at least mi_jpeg_scratch_bytes.  The _device forms enqueue on
 * `stream` and do not wait; dev_status (one word per interval) may be null.  The host forms upload, run, download and wait,
 * and return MI_OK with the flags in status_out (may be null). */
MI_API int mi_jpeg_coef_count(const mi_jpeg_t* jpeg, size_t* count);
MI_API int mi_jpeg_scratch_bytes(const mi_jpeg_t* jpeg, size_t* bytes);
MI_API int mi_jpeg_coefficients_device(int device, void* stream, const void* dev_span, size_t span_bytes, const uint32_t* dev_offsets,
                                       const mi_jpeg_t* jpeg, int16_t* dev_coef, uint32_t* dev_status);
MI_API int mi_jpeg_coefficients(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t* jpeg,
                                int16_t* host_coef, uint32_t* status_out);
MI_API int mi_jpeg_decode_device(int device, void* stream, const void* dev_span, size_t span_bytes, const uint32_t* dev_offsets,
                                 const mi_jpeg_t* jpeg, void* dev_scratch, size_t scratch_bytes, uint8_t* dev_out,
                                 uint32_t* dev_status);
MI_API int mi_jpeg_decode(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t* jpeg,
                          uint8_t* host_out, uint32_t* status_out);

/* ---- the split entropy decoder (kernels_jpeg_split.hpp): restart intervals of any length, a scan in one piece included ----
 * The same frames, checks and outputs as the entry points above, with one difference in `jpeg`: dri may be anything from 1 to
 * the number of MCUs, so a file WITHOUT a restart interval is passed as dri = MCUs, n_intervals = 1.  Every interval is cut into
 * subsequences of sub_bytes bytes, each walked by a lane of its own from a guessed decoder state; the guesses are repaired --
 * inside a workgroup of 256 lanes in LDS, across workgroups in up to max_rounds launches -- until every lane starts where its
 * predecessor stopped, which makes the result exact (jpeg_sync_core.hpp; tests/jpeg_split_restatement.py states it in Python).
 * Photographs settle in no round or one; an interval whose rounds were too few reports MI_JPEG_UNSYNCED and nothing else, and
 * its blocks are unspecified.  The _device forms enqueue on `stream` and never wait, so they may report that bit; the host
 * forms wait anyway, run once more with every round (workgroups - 1) when they find it, and never return it.
 * A truncated or corrupt interval is deterministic: its walk ends at the first symbol that would start at or beyond the end
 * of its data; MI_JPEG_OVERRUN is set when a block of the interval is then incomplete or missing, or when a symbol took bits
 * from beyond the end; coefficients not reached are 0 and DC differences not reached are 0 (the serial walker above goes on
 * reading zeros instead: a flagged interval's blocks are unspecified there too).
 * Still refused, by jpeg.read: progressive and arithmetic-coded files, 12-bit samples, CMYK / RGB components, several scans,
 * fill bytes inside the scan.
 * Checks beyond those above: sub_bytes 0 (the default, 128) or 8, 16, 32, 64, 128; max_rounds 0 (the default, 8) or a count;
 * a null `opt` means both defaults; dev_scratch 256-byte aligned with at least mi_jpeg_split_scratch_bytes (for the same
 * span_bytes and opt; both device forms take the same size). */
typedef struct {
    uint32_t sub_bytes;
    uint32_t max_rounds;
} mi_jpeg_split_t;
#define MI_JPEG_UNSYNCED 8u /* status bit 3 (split decoder, device forms only): the rounds enqueued were too few */
MI_API int mi_jpeg_split_scratch_bytes(const mi_jpeg_t* jpeg, size_t span_bytes, const mi_jpeg_split_t* opt, size_t* bytes);
MI_API int mi_jpeg_split_coefficients_device(int device, void* stream, const void* dev_span, size_t span_bytes,
                                             const uint32_t* dev_offsets, const mi_jpeg_t* jpeg, const mi_jpeg_split_t* opt,
                                             void* dev_scratch, size_t scratch_bytes, int16_t* dev_coef, uint32_t* dev_status);
MI_API int mi_jpeg_split_coefficients(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets,
                                      const mi_jpeg_t* jpeg, const mi_jpeg_split_t* opt, int16_t* host_coef, uint32_t* status_out);
MI_API int mi_jpeg_split_decode_device(int device, void* stream, const void* dev_span, size_t span_bytes, const uint32_t* dev_offsets,
                                       const mi_jpeg_t* jpeg, const mi_jpeg_split_t* opt, void* dev_scratch, size_t scratch_bytes,
                                       uint8_t* dev_out, uint32_t* dev_status);
MI_API int mi_jpeg_split_decode(int device, const void* host_span, size_t span_bytes, const uint32_t* offsets, const mi_jpeg_t* jpeg,
                                const mi_jpeg_split_t* opt, uint8_t* host_out, uint32_t* status_out);

/* ---- the split path of the lossless-JPEG decoder (kernels_ljpeg_split.hpp): decode INSIDE a segment ----
 * mi_raw_ljpeg gives one segment to one wavefront, whose first lane walks every symbol; a file in long strips, or written as
 * one strip, is then bound by one serial walk.  The split path cuts every segment (mi_ljpeg_seg_t: one or two components, every
 * predictor, every precision) into subsequences of sub_bytes bytes, walks each on a lane of its own from a guessed decoder
 * state -- the bit position and the component -- and repairs the guesses, inside a workgroup of 256 lanes in LDS and across
 * workgroups in up to max_rounds launches, until every lane starts where its predecessor stopped: the differences are then
 * exact, and prefix sums mod 2^16 (predictor 1: down the first columns, then along every row, all rows at once; predictors 2
 * to 7: one wavefront per segment) turn them into samples (ljpeg_sync_core.hpp; tests/ljpeg_split_restatement.py states it in
 * Python).  Descriptors, layout, crop, table, shift and output are exactly mi_raw_ljpeg's, and so is every unflagged segment.
 * Three-component streams (mi_ljpeg_seg3_t, mi_raw_ljpeg3) stay on the serial kernel: the step deliberately left for later.
 * Status: the bits of mi_raw_ljpeg, with these differences.  MI_LJPEG_OVERRUN: the data ended before the segment's last
 * sample, or a sample took bits from beyond the end; the walk stops there and samples not reached have difference 0 (the
 * serial kernel goes on reading zeros: a flagged segment's samples are unspecified in both).  MI_LJPEG_UNDECODED: as
 * mi_raw_ljpeg, and the segment is NOT written (as mi_raw_ljpeg3); also set where descriptors in device memory overlap so far
 * that they hold more subsequences than span_bytes / sub_bytes + segments.  MI_LJPEG_UNSYNCED: the rounds enqueued were too
 * few -- the segment reports that bit and nothing else, and its samples are unspecified.
 * `opt` is mi_jpeg_split_t: sub_bytes 0 (the default, 128) or 8, 16, 32, 64, 128; max_rounds 0 for the default or a count.  The
 * default is 8 where the descriptors lie only on the device (the _device forms, which enqueue on `stream`, never wait and may
 * report MI_LJPEG_UNSYNCED); where they lie in host memory it is the exact bound -- the largest number of workgroups any one
 * segment's lanes touch, minus 1 -- which never leaves a segment unsynced (rounds not needed return at once).  The host forms
 * upload, run and wait, run once more with the exact bound when a given max_rounds left a segment unsynced, and never return
 * that bit.  Checks: those of mi_raw_ljpeg[_device], those of mi_jpeg_split_* for `opt` and the scratch (null, too small -- the
 * message names the size --, 256-byte alignment; mi_ljpeg_split_scratch_bytes for the same layout, span_bytes and opt), and
 * segments x seg_height x seg_width below 2^32.
 * mi_ljpeg_split_differences[_device] is the tap for tests: the difference plane -- seg_height x seg_width uint16 per segment,
 * in segment order, unreached samples 0 -- and the status words, with no prediction. */
#define MI_LJPEG_UNSYNCED 8u    /* status bit 3 (split path, device forms only): the rounds enqueued were too few */
MI_API int mi_ljpeg_split_scratch_bytes(const mi_raw_layout_t* layout, size_t span_bytes, const mi_jpeg_split_t* opt, size_t* bytes);
MI_API int mi_raw_ljpeg_split_device(int device, void* stream, const void* dev_span, size_t span_bytes, const mi_ljpeg_seg_t* dev_segs,
                                     const mi_raw_layout_t* layout, const uint16_t* dev_table, const mi_jpeg_split_t* opt,
                                     void* dev_scratch, size_t scratch_bytes, void* dev_out, uint32_t* dev_status);
MI_API int mi_raw_ljpeg_split(int device, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs,
                              const mi_raw_layout_t* layout, const uint16_t* host_table, const mi_jpeg_split_t* opt, void* host_out,
                              uint32_t* status_out);
MI_API int mi_ljpeg_split_differences_device(int device, void* stream, const void* dev_span, size_t span_bytes,
                                             const mi_ljpeg_seg_t* dev_segs, const mi_raw_layout_t* layout, const mi_jpeg_split_t* opt,
                                             void* dev_scratch, size_t scratch_bytes, uint16_t* dev_plane, uint32_t* dev_status);
MI_API int mi_ljpeg_split_differences(int device, const void* host_span, size_t span_bytes, const mi_ljpeg_seg_t* segs,
                                      const mi_raw_layout_t* layout, const mi_jpeg_split_t* opt, uint16_t* host_plane,
                                      uint32_t* status_out);
/* The stack: with `opt` set (it holds until replaced, or cleared with null, as mi_stack_set_site_correction does),
 * mi_stack_push_ljpeg and one-sample compressed mi_stack_push_linear frames go through the split path, always with the exact
 * round bound from their host descriptors (opt->max_rounds is not looked at: a stack never sees MI_LJPEG_UNSYNCED); three-sample
 * linear frames keep going to raw_ljpeg3.  The stage owns one scratch, grown on demand -- the decode kernels of all frames run
 * in order on the handle's stream.  mi_stack_ljpeg_status keeps ORing the flags; everything behind the decode is unchanged. */
MI_API int mi_stack_set_ljpeg_split(mi_stack_t* s, const mi_jpeg_split_t* opt);

/* ---- synthetic stack generator, device side ---- */
MI_API int mi_synth_frames_device(int device, void* dev_out, int dtype, int height, int width,
                           int first_frame, int n_frames, int stack_size, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif /* MI355STACK_H */
