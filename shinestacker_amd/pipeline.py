"""In-memory align -> stack pipeline (BASELINE config 4).

The reference round-trips every frame through image files between `AlignFrames` and
`FocusStack` (stack_framework.py:269-297, pyramid.py:158,172).  Here a frame is uploaded once,
warped on the device (`mi_warp_affine_device`) straight into the stacker's input batch and fused
(`mi_stack_push_frames_device`); only the transform estimate runs on the host.

Result: identical to `align_images` on every frame (reference frame passed through untouched)
followed by `PyramidStack` on the aligned frames -- without the intermediate quantised files the
two-action reference job writes, which for lossless formats changes nothing.
"""
import ctypes as C
import time

import numpy as np

from . import _lib
from .align import (_BORDER_CODE, _DEFAULT_ALIGNMENT_CONFIG, _DEFAULT_FEATURE_CONFIG,
                    _DEFAULT_MATCHING_CONFIG, img_subsample, rescale_transform, resolve_estimator)
from .defaults import constants, resolve_arith
from .errors import AlignmentError, InvalidOptionError
from .imageio import validate_image


def _prestack_steps(mask_noise, vignetting, n_frames, device, lens=None):
    """The sub-actions that run on a frame before it is aligned, in the reference's order (constants.py:34 SUB_ACTION_TYPES:
    MaskNoise, Vignetting, AlignFrames, BalanceFrames), from the `mask_noise=` / `vignetting=` option dicts.  `mask_noise`
    takes MaskNoise's options; its `noise_mask` is the mask as an H x W array, or the path of the mask file (there is no
    working directory here: the path is used as given).  `lens`: a lens.Lens, or a dict of LensCorrection's options -- the
    lens correction, which the reference does not have, comes last: hot pixels are repaired before anything resamples them."""
    steps = []
    if mask_noise is not None:
        from .noise_detection import MaskNoise
        opts = dict(mask_noise)
        mask = opts.pop("noise_mask", constants.DEFAULT_NOISE_MAP_FILENAME)
        if isinstance(mask, str):
            mn = MaskNoise(noise_mask=mask, device=device, **opts)
            mn.load(mn.noise_mask)
        else:
            mn = MaskNoise(device=device, **opts)
            mn.set_mask(mask)
        steps.append(mn)
    if vignetting is not None:
        from .vignetting import Vignetting
        vg = Vignetting(device=device, **dict(vignetting))
        vg.begin(None, counts=n_frames)
        steps.append(vg)
    if lens is not None:
        from .lens import make_step
        lc = make_step(lens, device)
        lc.begin(None, counts=n_frames)
        steps.append(lc)
    return steps


def _prestack_info(steps, info):
    for s in steps:
        if info is not None and hasattr(s, "corrections"):
            info["vignetting_corrections"] = s.corrections
        s.end()


def _check_denoise_amount(denoise_amount):
    from .denoise import MAX_TEMPLATE_WINDOW
    if denoise_amount < 0 or denoise_amount != int(denoise_amount) or denoise_amount > MAX_TEMPLATE_WINDOW:
        raise InvalidOptionError("denoise_amount", denoise_amount, "the amount is also the template window size: a non-negative "
                                 f"integral value, at most {MAX_TEMPLATE_WINDOW}")


def _check_retouch(white_balance, unsharp, dtype):
    """The post-stack retouch options, refused before anything is stacked: `white_balance` an RGB triple, `unsharp` a
    (radius, amount, threshold) triple.  None for both (the default) imports nothing."""
    if white_balance is not None:
        from .white_balance import white_balance_table
        white_balance_table(dtype, white_balance)
    if unsharp is not None:
        from .sharpen import _prepare
        try:
            radius, amount, threshold = unsharp
        except (TypeError, ValueError):
            raise InvalidOptionError("unsharp", unsharp, "a (radius, amount, threshold) triple") from None
        _prepare(dtype, radius, amount, threshold)


def _check_depth_map(depth_map, info, shape):
    """`depth_map=`: None / False (off), True (the stacker's default sigma) or a sigma -> the sigma, or None when off.
    Refused before anything is allocated: a sigma out of range or too wide for the frame, and no `info` dict to put the map in."""
    if depth_map is None or depth_map is False:
        return None
    from . import depth_out
    sigma = depth_out.check_sigma(depth_out.PYRAMID_SIGMA if depth_map is True else depth_map, shape)
    if info is None:
        raise InvalidOptionError("depth_map", depth_map, "the map is returned in the info dict: pass info={}")
    return sigma


def _depth_map_info(stack, sigma, info, on_device, height, width, device):
    """info["depth_map"] = the stacker's depth map (Stack.depth_map): an H x W float32 array, or -- `on_device`, when the fused
    image stays on the device too -- a DeviceBuffer of H x W float32 that the caller frees.  Reads the stack's state only."""
    if sigma is None:
        return
    if not on_device:
        info["depth_map"] = stack.depth_map(sigma)
        return
    buf = _lib.DeviceBuffer(height * width * 4, device)
    try:
        stack.depth_map(sigma, buf.ptr)
    except BaseException:
        buf.free()
        raise
    info["depth_map"] = buf


def _check_depth_refine(depth_refine, shape, *consumers):
    """`depth_refine=`: None (off) or a dict of `radius` and `eps` (depth_out.check_refine) -> the options with both filled in,
    or None when off.  Refused before anything is allocated: an unknown key, a value out of range, and the option without any
    consumer of a depth map (`consumers`: the checked depth_map=, stereo=, depth_composite= options)."""
    if depth_refine is None:
        return None
    from . import depth_out
    opts = depth_out.check_refine(depth_refine, shape)
    if all(c is None for c in consumers):
        raise InvalidOptionError("depth_refine", depth_refine, "nothing asks for a depth map: it goes with depth_map=, stereo= or "
                                 "depth_composite=")
    return opts


class _RefinedStack:
    """A stacker handle whose every depth map is refined (`depth_refine=`): it stands where the handle stands in `_finish`,
    `_stereo_render`, `_composite_render` and `_depth_map_info`.  The guide is the fused frame as the stacker returned it:
    `finish` / `finish_device` keep a device copy before any post-stack filter or stroke sees the frame, and `depth_map` refines
    against that copy (Stack.depth_map's refine=).  `release` frees the copy; the handle itself is the caller's."""

    def __init__(self, stack, opts, height, width, dtype, device):
        self._stack, self._opts, self._dt, self._device = stack, opts, np.dtype(dtype), device
        self._shape = (height, width)
        self._guide = None

    def __getattr__(self, name):
        return getattr(self._stack, name)

    def _keep(self):
        if self._guide is None:
            self._guide = _lib.DeviceBuffer(self._shape[0] * self._shape[1] * 3 * self._dt.itemsize, self._device)
        return self._guide

    def finish(self):
        out = self._stack.finish()
        self._keep().upload(out)
        return out

    def finish_device(self, dev_ptr):
        self._stack.finish_device(dev_ptr)
        self._stack.sync()
        g = self._keep()
        _lib.check(_lib.load().mi_memcpy_d2d(self._device, g.ptr, dev_ptr, g.nbytes))

    def depth_map(self, sigma=0.0, dev_ptr=None):
        if self._guide is None:
            raise RuntimeError("depth_map: refine needs the fused frame, and the stack has not finished yet")
        guide = (self._guide.ptr, self._dt)
        if dev_ptr is not None:
            return self._stack.depth_map(sigma, dev_ptr, self._opts, guide)
        buf = _lib.DeviceBuffer(self._shape[0] * self._shape[1] * 4, self._device)
        try:
            self._stack.depth_map(sigma, buf.ptr, self._opts, guide)
            return buf.download(self._shape, np.float32)
        finally:
            buf.free()

    def release(self):
        if self._guide is not None:
            self._guide.free()
            self._guide = None


def _refined(stack, opts, height, width, dtype, device):
    """the handle the depth consumers read: `stack` itself with depth_refine off (nothing is built or copied)"""
    return stack if opts is None else _RefinedStack(stack, opts, height, width, dtype, device)


def _release(dstack):
    if isinstance(dstack, _RefinedStack):
        dstack.release()


def _check_stereo(stereo, info, shape, dm_sigma):
    """`stereo=`: None (off) or a dict of stereo.pair's options -- layout (default 'anaglyph'), separation, pivot, near -- and
    `sigma`, the smoothing of the depth map the views are rendered from (default: the `depth_map=` sigma when that is given,
    else the stacker's own).  Returns the options with every default filled in, or None when off.  Refused before anything
    is allocated: an unknown key, an option out of range and no `info` dict to put the result in."""
    if stereo is None:
        return None
    from . import depth_out
    from . import stereo as sv
    try:
        opts = dict(stereo)
    except (TypeError, ValueError):
        raise InvalidOptionError("stereo", stereo, "a dict of layout, separation, pivot, near, sigma") from None
    unknown = sorted(set(opts) - {"layout", "separation", "pivot", "near", "sigma"})
    if unknown:
        raise InvalidOptionError("stereo", unknown, "a dict of layout, separation, pivot, near, sigma")
    opts = {"layout": "anaglyph", "separation": sv.DEFAULT_SEPARATION, "pivot": 0.5, "near": "last", "sigma": None, **opts}
    sv.check_options(opts["layout"], opts["separation"], opts["pivot"], opts["near"], None if shape is None else shape[1])
    if opts["sigma"] is None:
        opts["sigma"] = depth_out.PYRAMID_SIGMA if dm_sigma is None else dm_sigma
    opts["sigma"] = depth_out.check_sigma(opts["sigma"], shape)
    if info is None:
        raise InvalidOptionError("stereo", stereo, "the pair is returned in the info dict: pass info={}")
    return opts


def _stereo_render(stack, opts, info, n_frames, height, width, dtype, device):
    """What `_finish` calls with the device address of the final frame when `stereo=` is set: info["stereo"] = stereo.pair of
    that frame and of the stacker's depth map (written to a device plane, never downloaded), rendered and composed in HBM;
    the pair is the one thing downloaded: an H x W x 3 ('anaglyph') or H x 2W x 3 array.  None when the option is off."""
    if opts is None:
        return None

    def render(dev_frame):
        from . import stereo as sv
        depth = _lib.DeviceBuffer(height * width * 4, device)
        try:
            stack.depth_map(opts["sigma"], depth.ptr)
            out = sv.pair_device(dev_frame, depth.ptr, height, width, dtype, n_frames, opts["separation"], opts["pivot"],
                                 opts["near"], opts["layout"], device)
            try:
                info["stereo"] = out.download((height, width if opts["layout"] == "anaglyph" else 2 * width, 3), dtype)
            finally:
                out.free()
        finally:
            depth.free()
    return render


def _check_depth_composite(depth_composite, info, shape, dm_sigma):
    """`depth_composite=`: None (off) or a dict of `interp` (default 'linear') and `sigma`, the smoothing of the depth map the
    composite is gathered by (default: the `depth_map=` sigma when that is given, else the stacker's own).  Returns the options
    with every default filled in, or None when off.  Refused before anything is allocated: an unknown key, an option out of range
    and no `info` dict to put the result in."""
    if depth_composite is None:
        return None
    from . import depth_out, depth_render
    try:
        opts = dict(depth_composite)
    except (TypeError, ValueError):
        raise InvalidOptionError("depth_composite", depth_composite, "a dict of interp, sigma") from None
    unknown = sorted(set(opts) - {"interp", "sigma"}, key=repr)
    if unknown:
        raise InvalidOptionError("depth_composite", unknown, "a dict of interp, sigma")
    opts = {"interp": "linear", "sigma": None, **opts}
    depth_render.check_options(opts["interp"])
    if opts["sigma"] is None:
        opts["sigma"] = depth_out.PYRAMID_SIGMA if dm_sigma is None else dm_sigma
    opts["sigma"] = depth_out.check_sigma(opts["sigma"], shape)
    if info is None:
        raise InvalidOptionError("depth_composite", depth_composite, "the composite is returned in the info dict: pass info={}")
    return opts


def _check_brush(retouch, n_frames, depth_composite=None):
    """`retouch=`: None (off) or a sequence of retouch.Stroke whose `source` is a frame index in [0, n_frames), or the string
    "depth_composite" when that option (`depth_composite`: its checked options) is on.  Returns the strokes as a list, or None
    when off.  Refused before anything is allocated."""
    if retouch is None:
        return None
    from .retouch import check_strokes
    strokes = check_strokes(retouch)
    for s in strokes:
        if s.source == "depth_composite":
            if depth_composite is None:
                raise InvalidOptionError("source", s.source, "a stroke paints from the composite only with depth_composite= set")
            continue
        if isinstance(s.source, str) or not 0 <= s.source < n_frames:
            raise InvalidOptionError("source", s.source, f"a stroke names a frame by its index in [0, {n_frames})")
    return strokes


def _composite_render(stack, opts, info, frame_ptrs, height, width, dtype, device, on_device):
    """The render of `depth_composite=`, a callable for `_brush_paint`: the stacker's depth map written to a device plane (never
    downloaded) and the frames at the device addresses `frame_ptrs` -- all of the stack, as they were pushed -- gathered by it
    into a new DeviceBuffer, which is returned.  None when the option is off."""
    if opts is None:
        return None

    def render():
        from . import depth_render
        ptrs = list(frame_ptrs())
        fb = height * width * 3 * np.dtype(dtype).itemsize
        depth = _lib.DeviceBuffer(height * width * 4, device)
        out = None
        try:
            stack.depth_map(opts["sigma"], depth.ptr)
            stack.sync()
            out = _lib.DeviceBuffer(fb, device)
            depth_render.composite_device(ptrs, 0, len(ptrs), len(ptrs), depth.ptr, out.ptr, height, width, dtype, opts["interp"], device)
            _lib.check(_lib.load().mi_device_synchronize(device))      # the depth plane is freed below
        except BaseException:
            if out is not None:
                out.free()
            raise
        finally:
            depth.free()
        return out
    render.on_device = on_device
    render.info = info
    return render


def _brush_paint(strokes, kept, height, width, dtype, device, composite=None):
    """What `_finish` calls with the device address of the fused frame when `retouch=` or `depth_composite=` is set: the
    composite rendered (`composite`: `_composite_render`'s callable), then the strokes painted into the fused frame in place from
    `kept`, {frame index: DeviceBuffer of that frame as it was pushed to the stacker}, and from the composite under the name
    "depth_composite"; info["depth_composite"] then receives the composite, downloaded or as the DeviceBuffer.  None when both
    options are off."""
    if not strokes and composite is None:
        return None

    def paint(dev_frame):
        sources = {i: b.ptr for i, b in kept.items() if b is not None}
        comp = composite() if composite is not None else None
        try:
            if comp is not None:
                sources["depth_composite"] = comp.ptr
            if strokes:
                from .retouch import apply_device
                apply_device(dev_frame, height, width, dtype, strokes, sources, device)
            if comp is not None:
                if composite.on_device:
                    composite.info["depth_composite"], comp = comp, None
                else:
                    composite.info["depth_composite"] = comp.download((height, width, 3), dtype)
        finally:
            if comp is not None:
                comp.free()
    return paint


def _finish(stack, out_dev, denoise_amount, height, width, dtype, device, white_balance=None, unsharp=None, on_device_frame=None,
            on_fused_frame=None):
    """The stacker's result: downloaded (returned), or written to the device address `out_dev` (None returned).  With
    `denoise_amount` > 0 the result first passes through the post-stack denoise on the device, with the reference's
    arguments (stack.py:33-35: the amount is the filter strength and the template window size); then through the white
    balance (`white_balance`: the RGB triple) and the unsharp mask (`unsharp`: radius, amount, threshold) when given --
    denoise -> white balance -> unsharp, all in HBM, one download.  `on_device_frame` (`_stereo_render`): called with the
    device address of the final frame, after the last filter and before the download.  `on_fused_frame` (`_brush_paint`): called
    with the device address of the fused frame before the first filter; it may change the frame in place."""
    if not denoise_amount and white_balance is None and unsharp is None and on_device_frame is None and on_fused_frame is None:
        if out_dev is not None:
            stack.finish_device(out_dev)
            stack.sync()
            return None
        return stack.finish()
    dt = np.dtype(dtype)
    fb = height * width * 3 * dt.itemsize
    steps = []      # (run(src, dst), may src be dst)
    if denoise_amount:
        from .denoise import denoise_device
        steps.append((lambda s, d: denoise_device(s, d, height, width, dt, denoise_amount, int(denoise_amount), device=device), False))
    if white_balance is not None:
        from .white_balance import white_balance_device
        steps.append((lambda s, d: white_balance_device(s, d, height * width, dt, white_balance, device=device), True))
    if unsharp is not None:
        from .sharpen import unsharp_mask_device
        steps.append((lambda s, d: unsharp_mask_device(s, d, height, width, dt, *unsharp, device=device), False))
    if not steps:       # only the hooks ask for the frame in HBM
        res = _lib.DeviceBuffer(fb, device) if out_dev is None else None
        try:
            final = out_dev if res is None else res.ptr
            stack.finish_device(final)
            stack.sync()
            if on_fused_frame is not None:
                on_fused_frame(final)
            if on_device_frame is not None:
                on_device_frame(final)
            return None if res is None else res.download((height, width, 3), dt)
        finally:
            if res is not None:
                res.free()
    bufs = []
    try:
        bufs.append(_lib.DeviceBuffer(fb, device))
        cur = bufs[0].ptr
        stack.finish_device(cur)
        stack.sync()
        if on_fused_frame is not None:
            on_fused_frame(cur)
        res = None
        if out_dev is None:
            res = _lib.DeviceBuffer(fb, device)
            bufs.append(res)
        final = res.ptr if res is not None else out_dev
        for i, (run, in_place) in enumerate(steps):
            if i == len(steps) - 1:
                dst = final
            elif in_place:
                dst = cur
            else:
                if len(bufs) < (3 if res is not None else 2):
                    bufs.append(_lib.DeviceBuffer(fb, device))
                dst = bufs[-1].ptr if cur == bufs[0].ptr else bufs[0].ptr
            run(cur, dst)
            cur = dst
        if on_device_frame is not None:
            on_device_frame(final)
        if res is not None:
            return res.download((height, width, 3), dt)
        _lib.check(_lib.load().mi_device_synchronize(device))
        return None
    finally:
        for b in bufs:
            b.free()


def align_and_stack(frames, ref_idx=-1, estimator=None, alignment_config=None, feature_config=None,
                    matching_config=None, device=0, batch_frames=16, check_running=None, mask_noise=None, vignetting=None,
                    info=None, denoise_amount=0, white_balance=None, unsharp=None, depth_map=None, stereo=None, retouch=None,
                    depth_composite=None, lens=None, depth_refine=None, **stack_kwargs):
    """Align every frame to frames[ref_idx] (fixed reference, `step_process=False` order,
    stack_framework.py:191-232) and fuse them.  `frames`: sequence of H x W x 3 uint8/uint16 BGR
    arrays.  Returns (fused image, list of n_good_matches).

    `mask_noise` / `vignetting`: optional dicts of the MaskNoise / Vignetting sub-actions' options (`_prestack_steps`);
    every frame, the reference frame included, then passes through them, in that order, before it is estimated or warped
    -- the reference's sub-action order.  None (default): the frames are taken as they are.  `info`: an optional dict that
    receives `info["vignetting_corrections"]` (the sub-action's percentile radii per frame).

    `lens`: a `lens.Lens`, or a dict of `LensCorrection`'s options (lens, autoscale): every frame, the reference frame
    included, passes through the lens correction (lens.py) behind `mask_noise` and `vignetting` and before it is estimated
    or warped.  None (default): nothing is built, allocated, loaded or called.

    `denoise_amount`: the stack actions' option (`_finish`): when positive the fused frame is denoised on the device before
    it is downloaded.  0 (default): nothing is touched.  `white_balance` (an RGB triple) / `unsharp` ((radius, amount,
    threshold)): the retouch filters (white_balance.py, sharpen.py), applied on the device after the denoise, in that order,
    before the download.  None (default): nothing is built, loaded or called.

    `depth_map`: a sigma, or True for the stacker's default -- `info["depth_map"]` then receives the frame index in focus at
    each pixel (H x W float32, `Stack.depth_map`, depth_out.py).  None (default): nothing is computed; the return values are
    the same either way.

    `stereo`: a dict of `stereo.pair`'s options (layout -- default 'anaglyph' --, separation, pivot, near) and `sigma`, the
    depth map's smoothing (default: the `depth_map=` sigma, else the stacker's own) -- `info["stereo"]` then receives the
    stereo pair of the fused frame as an array, rendered on the device from the final frame and the depth plane before
    anything is downloaded (stereo.py).  None (default): nothing is built, loaded or called; the return values are the same
    either way.

    `retouch`: a sequence of `retouch.Stroke` (retouch.py) painted into the fused frame on the device, in order, right after the
    fusion: before the denoise, the white balance, the unsharp mask, the stereo render and the one download.  A stroke's
    `source` is a frame index and means that frame as it was pushed to the stacker -- after the pre-stack corrections and the
    warp; the reference frame untouched -- of which a device copy is kept as it passes.  None (default): nothing is built,
    loaded, copied or called.

    `depth_composite`: a dict of `interp` ('linear', the default, or 'nearest') and `sigma`, the depth map's smoothing (default:
    the `depth_map=` sigma, else the stacker's own) -- `info["depth_composite"]` then receives the depth-selected composite
    (depth_render.py) as an array: every pixel taken from the frame the depth map names, the frames being those pushed to the
    stacker.  A device copy of EVERY frame is kept as it passes (InvalidOptionError, before anything is allocated, when the free
    device memory does not hold them), and the composite is rendered in HBM from the depth plane, which is not downloaded.  A
    stroke of `retouch=` whose `source` is the string "depth_composite" paints from it.  None (default): nothing is built, loaded,
    copied or called; the return values are the same either way.

    `depth_refine`: a dict of `radius` (1 .. 32, default 6) and `eps` (1e-9 .. 1e3, default 1e-4) -- EVERY depth map this call
    makes is then refined against the fused frame (depth_out.py, the edge-aware guided filter): the map `depth_map=` returns,
    the map under the `stereo=` render and the map under the `depth_composite=` render, and so a stroke that paints from the
    composite.  The guide is the fused frame as the stacker returned it, before the strokes and the post-stack filters, so the
    map does not depend on them.  Refinement works best on the unsmoothed index, `depth_map=0.0`: a Gaussian has already spread
    the subject's depth across the edge, and the filter cannot tell that bleed from the truth.  Without any of the three
    consumers the option is refused.  None (default): nothing is built, copied or called."""
    _check_denoise_amount(denoise_amount)
    dm_sigma = _check_depth_map(depth_map, info, np.asarray(frames[0]).shape if len(frames) else None)
    dc_opts = _check_depth_composite(depth_composite, info, np.asarray(frames[0]).shape if len(frames) else None, dm_sigma) \
        if depth_composite is not None else None
    strokes = _check_brush(retouch, len(frames), dc_opts)
    sv_opts = _check_stereo(stereo, info, np.asarray(frames[0]).shape if len(frames) else None, dm_sigma) if stereo is not None else None
    rf_opts = _check_depth_refine(depth_refine, np.asarray(frames[0]).shape if len(frames) else None, dm_sigma, sv_opts, dc_opts)
    if white_balance is not None or unsharp is not None:
        _check_retouch(white_balance, unsharp, np.asarray(frames[0]).dtype if len(frames) else np.uint8)
    _lib.require_device()
    n = len(frames)
    if n == 0:
        raise ValueError("no frames")
    pre = _prestack_steps(mask_noise, vignetting, n, device, lens)
    if pre:
        fixed = []
        for i, fr in enumerate(frames):
            for step in pre:
                fr = step.run_frame(i, ref_idx, fr)
            fixed.append(fr)
        frames = fixed
        _prestack_info(pre, info)
    feature_config = {**_DEFAULT_FEATURE_CONFIG, **(feature_config or {})}
    matching_config = {**_DEFAULT_MATCHING_CONFIG, **(matching_config or {})}
    cfg = {**_DEFAULT_ALIGNMENT_CONFIG, **(alignment_config or {})}
    if cfg['border_mode'] not in _BORDER_CODE:
        raise InvalidOptionError("border_mode", cfg['border_mode'])
    if cfg['transform'] not in (constants.ALIGN_RIGID, constants.ALIGN_HOMOGRAPHY):
        raise InvalidOptionError("transform", cfg['transform'])
    homography = cfg['transform'] == constants.ALIGN_HOMOGRAPHY
    min_matches = 4 if homography else 3
    estimator = resolve_estimator(estimator, device)
    if ref_idx == -1:
        ref_idx = n // 2
    ref = np.ascontiguousarray(frames[ref_idx])
    h, w = ref.shape[:2]
    dt = ref.dtype
    fb = h * w * 3 * dt.itemsize
    lib = _lib.load()
    if dc_opts is not None:     # n kept frames, the composite and the depth plane, beside what the stack itself takes
        need = (n + 1) * fb + h * w * 4
        free, _total = _lib.mem_info(device)
        if need > free:
            raise InvalidOptionError("depth_composite", depth_composite, f"keeping the {n} frames resident needs {need} bytes of device "
                                     f"memory and {free} bytes are free")
    stack_kwargs["arith"] = resolve_arith(stack_kwargs.get("arith"), stack_kwargs.get("float_type"))   # one default for every entry point
    stack = _lib.Stack(h, w, in_dtype=dt, out_dtype=dt, device=device, batch_frames=batch_frames,
                       **stack_kwargs)
    src = _lib.DeviceBuffer(fb, device)            # uploaded moving frame
    tmp = _lib.DeviceBuffer(fb, device)            # warp scratch (border blur)
    mask = _lib.DeviceBuffer(h * w, device)
    batch = _lib.DeviceBuffer(fb * batch_frames, device)
    mode = _BORDER_CODE[cfg['border_mode']]
    bv = (C.c_double * 4)(*(list(cfg['border_value']) + [0, 0, 0, 0])[:4])
    matches, filled = [], 0
    # frame index -> device copy of the frame as pushed: the frames the strokes name, or every frame for the composite
    kept = dict.fromkeys(range(n)) if dc_opts is not None else {s.source: None for s in strokes} if strokes else {}

    def flush():
        nonlocal filled
        if filled:
            lib.mi_device_synchronize(device)  # warps ran on the default stream
            stack.push_frames_device(batch.ptr, filled, fb)
            stack.sync()                       # the batch buffer is reused next
            filled = 0

    for i, fr in enumerate(frames):
        fr = np.ascontiguousarray(fr)
        validate_image(fr, (h, w), dt)
        dst = batch.ptr + filled * fb
        if i == ref_idx:
            batch.upload(fr, filled * fb)      # reference frame: untouched (align.py:279-280)
            matches.append(0)
        else:
            sub = cfg['subsample']
            while True:
                a, b = (img_subsample(fr, sub, cfg['fast_subsampling']),
                        img_subsample(ref, sub, cfg['fast_subsampling'])) if sub > 1 else (fr, ref)
                ng, m = estimator(a, b, feature_config, matching_config, cfg)
                if ng > cfg['min_good_matches'] or sub == 1:
                    break
                sub = 1
            matches.append(ng)
            if ng < min_matches or m is None:
                raise AlignmentError(i, f"too few matches found: {ng} < {min_matches}")
            m = np.asarray(m)
            if homography and m.shape == (2, 3):
                m = np.vstack([m, [0.0, 0.0, 1.0]])
            if sub > 1:
                m = rescale_transform(m, cfg['transform'], sub, fr.shape, a.shape)
            mm = (C.c_double * m.size)(*np.asarray(m, dtype=np.float64).reshape(-1))
            src.upload(fr)
            warp = lib.mi_warp_perspective_device if homography else lib.mi_warp_affine_device
            _lib.check(warp(device, None, src.ptr, dst, tmp.ptr, mask.ptr, h, w, _lib.DTYPE_CODE[dt], mm, mode, bv, 21,
                            float(cfg['border_blur'])))
        if i in kept:
            kept[i] = _lib.DeviceBuffer(fb, device)
            _lib.check(lib.mi_memcpy_d2d(device, kept[i].ptr, dst, fb))     # on the stream the warp ran on: after it
        filled += 1
        if filled == batch_frames:
            flush()
        if check_running is not None and check_running() is False:
            from .errors import RunStopException
            raise RunStopException("align_and_stack")
    flush()
    dstack = _refined(stack, rf_opts, h, w, dt, device)
    try:
        try:
            out = _finish(dstack, None, denoise_amount, h, w, dt, device, white_balance, unsharp,
                          _stereo_render(dstack, sv_opts, info, n, h, w, dt, device),
                          _brush_paint(strokes, kept, h, w, dt, device,
                                       _composite_render(dstack, dc_opts, info, lambda: [kept[i].ptr for i in range(n)], h, w, dt, device,
                                                         False)))
        finally:
            for b in kept.values():
                if b is not None:
                    b.free()
        _depth_map_info(dstack, dm_sigma, info, False, h, w, device)
    finally:
        _release(dstack)
    stack.close()
    return out, matches


# chain_refine: how far (pixels, at the frame corners) the refinement against the global reference frame may move a chain
# estimate before it is distrusted and the chain estimate kept
CHAIN_REFINE_MAX_SHIFT = 2.0


def _corner_shift(m0, m1, height, width):
    """largest displacement between two 2x3 transforms at the frame corners"""
    pts = np.array([[0.0, 0.0, 1.0], [width - 1.0, 0.0, 1.0], [0.0, height - 1.0, 1.0], [width - 1.0, height - 1.0, 1.0]]).T
    return float(np.abs(np.asarray(m0) @ pts - np.asarray(m1) @ pts).max())


CHAIN_PAIR_WORKERS = 4   # estimator handles (one host thread each) that share the chain's neighbour pairs


def _to33(m):
    m = np.asarray(m, np.float64)
    return m if m.shape == (3, 3) else np.vstack([m, [0.0, 0.0, 1.0]])


def _align_chains_pairs_device(lib, dev_frames, aligned, n_frames, height, width, dt, ref_idx, cfg, min_correlation, max_iters,
                               device, corr=None, chain_refine=True, reuse=None):
    """`step_process=True` without its serial dependency (round 6).  The reference registers frame f against the ALIGNED frame
    f - 1 (stack_framework.py:214-232): neighbours look alike, so the estimate is easy, and the aligned neighbour carries the
    transform found so far.  The same chain, factored: every frame is registered against its UNWARPED neighbour -- independent
    estimates: ALIGN_RIGID as batched Gauss-Newton over up to 127 pairs at once (mi_aligner_estimate_pairs), ALIGN_HOMOGRAPHY
    pair by pair on CHAIN_PAIR_WORKERS estimator handles --, the steps are composed along each chain in
    float64 (frame -> neighbour -> ... -> reference), and, as in the serial form, every composed estimate is refined against
    the GLOBAL reference frame (one batched call for all frames: the datum that keeps the steps' errors from adding up,
    `chain_refine`); then all frames are warped.  No step waits for a warp, nothing synchronises the device per frame.
    Differences from the serial form: a step's reference has not been resampled (its estimate sees the sharper image) and,
    with `corr`, has not been balanced yet (the ECC criterion is invariant to gain and offset); the balanced, aligned frames
    the stack sees are produced exactly as before.  `reuse` (ALIGN_RIGID): (pair estimator, global-reference estimator, frame
    scratch, mask scratch) of an earlier call -- nothing is allocated then.  Returns (transforms, correlation coefficients
    -- the refinement's where it was accepted)."""
    import threading
    fb = height * width * 3 * dt.itemsize
    mode = _BORDER_CODE[cfg['border_mode']]
    bv = (C.c_double * 4)(*(list(cfg['border_value']) + [0, 0, 0, 0])[:4])
    homography = cfg['transform'] == constants.ALIGN_HOMOGRAPHY
    sub = max(1, int(cfg['subsample']))
    transforms, ccs = [None] * n_frames, [1.0] * n_frames
    _lib.check(lib.mi_memcpy_d2d(device, aligned + ref_idx * fb, dev_frames + ref_idx * fb, fb))   # align.py:279-280
    chains = [list(range(ref_idx + 1, n_frames)), list(range(ref_idx - 1, -1, -1))]
    pairs = []                      # (frame, its neighbour towards the reference frame)
    for ch in chains:
        prev = ref_idx
        for i in ch:
            pairs.append((i, prev))
            prev = i
    if not pairs:
        return transforms, ccs
    step_m, step_cc, errors = {}, {}, []
    import os, time
    _t = [time.perf_counter()]
    def _lap(label):
        if os.environ.get("MI_CHAIN_TIMING"):
            lib.mi_device_synchronize(device)
            _t.append(time.perf_counter())
            print(f"[chain] {label}: {(_t[-1] - _t[-2]) * 1e3:.1f} ms", flush=True)

    if not homography:
        # ALIGN_RIGID: the pairs of a chain as batches of ONE Gauss-Newton each (mi_aligner_estimate_pairs: the pyramids of the
        # batch's frames are built once, a frame's template is its neighbour's pyramid).  A batch = a run of up to MAX_BATCH
        # frames along a chain, led by the frame the run's first step refers to (the reference frame, or the last frame of
        # the run before), which is registered against itself.
        al = None
        try:
            al = reuse[0] if reuse else _lib.Aligner(height, width, dt, subsample=sub, device=device, fast=bool(cfg['fast_subsampling']))
            for ch in chains:
                lead = ref_idx
                for b0 in range(0, len(ch), _lib.Aligner.MAX_BATCH - 1):
                    run = ch[b0:b0 + _lib.Aligner.MAX_BATCH - 1]
                    frames_b = [lead] + run
                    ms, cs, _ = al.estimate_pairs([dev_frames + i * fb for i in frames_b], [0] + list(range(len(run))),
                                                  max_iters=max_iters)
                    for k, i in enumerate(run, start=1):
                        if not cs[k] >= min_correlation:
                            raise AlignmentError(i, f"correlation {cs[k]:.3f} < {min_correlation}")
                        step_m[i], step_cc[i] = _to33(ms[k]), float(cs[k])
                    lead = run[-1]
        finally:
            if al is not None and not reuse:
                al.close()
    else:
        nw = max(1, min(CHAIN_PAIR_WORKERS, len(pairs)))

        def worker(k):
            al = None
            try:
                al = _lib.Aligner(height, width, dt, subsample=sub, device=device, fast=bool(cfg['fast_subsampling']))
                lo, hi = k * len(pairs) // nw, (k + 1) * len(pairs) // nw
                for i, prev in pairs[lo:hi]:
                    al.set_reference(dev_frames + prev * fb)
                    ms, cs, _ = al.estimate_homography_batch([dev_frames + i * fb], max_iters=max_iters)
                    if not cs[0] >= min_correlation:
                        raise AlignmentError(i, f"correlation {cs[0]:.3f} < {min_correlation}")
                    step_m[i], step_cc[i] = _to33(ms[0]), float(cs[0])
            except Exception as e:  # noqa: BLE001  re-raised on the calling thread
                errors.append(e)
            finally:
                if al is not None:
                    al.close()

        threads = [threading.Thread(target=worker, args=(k,)) for k in range(nw)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:
            raise errors[0]
    _lap("pair estimates")
    # frame -> reference: the steps composed along the chain (x_ref = M_prev_total M_step x_frame)
    for ch in chains:
        total = np.eye(3)
        for i in ch:
            total = total @ step_m[i]
            transforms[i] = total.copy() if homography else total[:2].copy()
            ccs[i] = step_cc[i]
    if chain_refine and not homography:
        gref = None
        try:
            gref = reuse[1] if reuse else _lib.Aligner(height, width, dt, subsample=sub, device=device, fast=bool(cfg['fast_subsampling']))
            gref.set_reference(dev_frames + ref_idx * fb)
            todo = [i for ch in chains for i in ch[1:]]     # (a chain's first step IS an estimate against the global reference)
            for b0 in range(0, len(todo), _lib.Aligner.MAX_BATCH):
                idx = todo[b0:b0 + _lib.Aligner.MAX_BATCH]
                try:
                    m2, c2, _ = gref.refine_batch([dev_frames + i * fb for i in idx], np.stack([transforms[i] for i in idx]),
                                                  levels=2, max_iters=max_iters)
                except (_lib.DeviceError, ValueError):
                    continue
                for j, i in enumerate(idx):
                    if c2[j] >= min_correlation and _corner_shift(transforms[i], m2[j], height, width) <= CHAIN_REFINE_MAX_SHIFT:
                        transforms[i], ccs[i] = m2[j], float(c2[j])
        finally:
            if gref is not None and not reuse:
                gref.close()
    _lap("refine")
    tmp = mask = None
    try:
        tmp = reuse[2] if reuse else _lib.DeviceBuffer(fb, device)
        mask = reuse[3] if reuse else _lib.DeviceBuffer(height * width, device)
        warp = lib.mi_warp_perspective_device if homography else lib.mi_warp_affine_device
        for ch in chains:
            for i in ch:
                m = np.asarray(transforms[i], np.float64)
                arr = (C.c_double * m.size)(*m.reshape(-1))
                _lib.check(warp(device, None, dev_frames + i * fb, aligned + i * fb, tmp.ptr, mask.ptr, height, width,
                                _lib.DTYPE_CODE[dt], arr, mode, bv, 21, float(cfg['border_blur'])))
                if corr is not None:
                    corr.apply_correction_device(i, aligned + i * fb, None)
        _lib.check(lib.mi_device_synchronize(device))
        _lap("warps")
    finally:
        for b in (tmp, mask):
            if b is not None and not reuse:
                b.free()
    return transforms, ccs


def _align_chains_device(lib, dev_frames, aligned, n_frames, height, width, dt, ref_idx, cfg, min_correlation, max_iters,
                         device, corr=None, chain_refine=True):
    """`step_process=True` (stack_framework.py:214-232, the documented default of the reference's jobs): frame ref+1 is
    aligned to the reference frame, ref+2 to the ALIGNED ref+1, ... and ref-1, ref-2, ... the same way downwards -- two
    serial chains.  Every step needs the previous step's warped frame, so the batched estimator does not apply; the two
    chains are independent and run side by side (one host thread and one estimator handle each).  Aligned frames are
    written to `aligned` at their own index.  `corr` (a BalanceFrames correction, already begun on the reference frame):
    every aligned frame is balanced BEFORE it becomes the next step's reference, as the reference's CombinedActions does
    (the step reference is read back from the output directory, i.e. after align AND balance,
    stack_framework.py:259-262, :282-289).  Returns (transforms, correlation coefficients).

    `chain_refine` (ALIGN_RIGID): the errors of the chain's steps add up like a random walk (0.5 px at the ends of a
    128-frame stack, against the 0.2 px a single pair is held to, tests/test_0031_align_precision.py:62-65), because each
    step only sees the previous step's output.  Every step's estimate is therefore refined against the GLOBAL reference
    frame -- the same iteration on the two finest pyramid levels, started from the chain estimate -- before the frame is
    warped: the chain supplies the capture range (neighbouring frames look alike), the global frame the datum.  A
    refinement that fails, correlates worse than `min_correlation` or moves a corner by more than CHAIN_REFINE_MAX_SHIFT
    pixels is distrusted and the chain estimate is kept."""
    import threading
    corr_lock = threading.Lock()   # one correction object (its histogram / table scratch) serves both chains
    fb = height * width * 3 * dt.itemsize
    mode = _BORDER_CODE[cfg['border_mode']]
    bv = (C.c_double * 4)(*(list(cfg['border_value']) + [0, 0, 0, 0])[:4])
    homography = cfg['transform'] == constants.ALIGN_HOMOGRAPHY
    transforms, ccs, errors = [None] * n_frames, [1.0] * n_frames, []
    _lib.check(lib.mi_memcpy_d2d(device, aligned + ref_idx * fb, dev_frames + ref_idx * fb, fb))   # align.py:279-280

    def chain(indices):
        aligner = gref = tmp = mask = None
        try:
            aligner = _lib.Aligner(height, width, dt, subsample=max(1, int(cfg['subsample'])), device=device,
                                   fast=bool(cfg['fast_subsampling']))
            if chain_refine and not homography and indices:
                gref = _lib.Aligner(height, width, dt, subsample=max(1, int(cfg['subsample'])), device=device,
                                    fast=bool(cfg['fast_subsampling']))
                gref.set_reference(dev_frames + ref_idx * fb)
            tmp = _lib.DeviceBuffer(fb, device)
            mask = _lib.DeviceBuffer(height * width, device)
            prev = ref_idx
            for i in indices:
                aligner.set_reference(aligned + prev * fb)
                if homography:   # the similarity refined to 8 degrees of freedom
                    ms, cs, _ = aligner.estimate_homography_batch([dev_frames + i * fb], max_iters=max_iters)
                    m, cc = ms[0], cs[0]
                else:
                    m, cc, _ = aligner.estimate(dev_frames + i * fb, max_iters=max_iters)
                if not cc >= min_correlation:
                    raise AlignmentError(i, f"correlation {cc:.3f} < {min_correlation}")
                if gref is not None and prev != ref_idx:   # (the first step IS an estimate against the global reference)
                    try:
                        m2, c2, _ = gref.refine_batch([dev_frames + i * fb], m[None], levels=2, max_iters=max_iters)
                        if c2[0] >= min_correlation and _corner_shift(m, m2[0], height, width) <= CHAIN_REFINE_MAX_SHIFT:
                            m, cc = m2[0], c2[0]     # (the coefficient reported is that of the transform that is used)
                    except (_lib.DeviceError, ValueError):
                        pass
                transforms[i], ccs[i] = m, float(cc)
                arr = (C.c_double * m.size)(*m.reshape(-1))
                warp = lib.mi_warp_perspective_device if homography else lib.mi_warp_affine_device
                _lib.check(warp(device, None, dev_frames + i * fb, aligned + i * fb, tmp.ptr, mask.ptr, height, width,
                                _lib.DTYPE_CODE[dt], arr, mode, bv, 21, float(cfg['border_blur'])))
                if corr is not None:
                    with corr_lock:
                        corr.apply_correction_device(i, aligned + i * fb, None)
                _lib.check(lib.mi_device_synchronize(device))    # the next step's reference is this step's output
                prev = i
        except Exception as e:  # noqa: BLE001  re-raised on the calling thread
            errors.append(e)
        finally:   # a chain that raises must not leak its estimator handle and buffers
            for al in (aligner, gref):
                if al is not None:
                    al.close()
            for b in (tmp, mask):
                if b is not None:
                    b.free()

    threads = [threading.Thread(target=chain, args=(list(range(ref_idx + 1, n_frames)),)),
               threading.Thread(target=chain, args=(list(range(ref_idx - 1, -1, -1)),))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return transforms, ccs


class StackHandles:
    """What `align_and_stack_device(keep_handles=True)` returns and `handles=` takes back: the stacker, the estimator and
    the scratch buffers of ONE geometry.  The library never sees the sizes of `batches` / `tmp` / `mask`, so the geometry
    they were made for travels with them and a later call is checked against it (`matches`)."""

    def __init__(self, stack, aligner, batches, tmp, mask, gref=None, **geometry):
        self.stack, self.aligner, self.batches, self.tmp, self.mask = stack, aligner, batches, tmp, mask
        self.gref = gref    # step_process: the estimator that holds the GLOBAL reference frame (chain_refine)
        self.geometry = geometry

    def __iter__(self):    # (stack, aligner, batches, tmp, mask), as rounds 2-3 returned them
        return iter((self.stack, self.aligner, self.batches, self.tmp, self.mask))

    def mismatch(self, **geometry):
        """names of the geometry items that differ from what the handles were created for"""
        return [k for k, v in geometry.items() if self.geometry.get(k) != v]

    def close(self):
        self.aligner.close()
        if self.gref is not None:
            self.gref.close()
        self.stack.close()
        for b in (self.batches, self.tmp, self.mask):
            b.free()


def close_handles(handles):
    """release what `align_and_stack_device(keep_handles=True)` returned"""
    handles.close()


def _make_correction(balance, device):
    """The correction object of BalanceFrames for a dict of its options (balance.py:366-388: channel -> class; the
    sub-sampling default depends on the map)."""
    from .balance import LSCorrection, LumiCorrection, RGBCorrection, SVCorrection
    classes = {constants.BALANCE_LUMI: LumiCorrection, constants.BALANCE_RGB: RGBCorrection,
               constants.BALANCE_HSV: SVCorrection, constants.BALANCE_HLS: LSCorrection}
    opts = dict(balance)
    channel = opts.pop('channel', constants.DEFAULT_CHANNEL)
    if channel not in classes:
        raise InvalidOptionError("channel", channel)
    if opts.get('subsample', -1) == -1:
        opts['subsample'] = 1 if opts.get('corr_map') == constants.BALANCE_MATCH_HIST \
            else constants.DEFAULT_BALANCE_SUBSAMPLE
    return classes[channel](device=device, **opts)


def auto_batch_frames(n_frames, height, width, dtype, device=0, share=0.25):
    """Warped frames per push into the stacker for the resident align -> stack flow: as many as the job has (a multiple of 16,
    at most 128) while two input batches plus the stacker's two sets of coarser Gaussian levels stay inside `share` of the
    free device memory.  Bigger pushes fuse more efficiently (the coarse levels of a 16-frame push are launch-bound): config 4,
    128 x 24 MP u8, 0.0417 s at 16 frames per push, 0.0400 at 32, 0.0387 at 64, 0.0367 at 128."""
    dt = np.dtype(dtype)
    px = int(height) * int(width)
    per_frame = 2 * px * 3 * dt.itemsize + 2 * (px // 3 + 1) * 12   # two batch buffers + two sets of G_1.. (fp32 RGB, P_0 / 3 pixels)
    free, _total = _lib.mem_info(device)
    fit = int(share * free // max(per_frame, 1))
    want = min(128, -(-int(n_frames) // 16) * 16)
    return max(16, min(want, fit // 16 * 16))


def align_and_stack_device(dev_frames, n_frames, height, width, dtype, ref_idx=-1, alignment_config=None,
                           min_correlation=0.5, max_iters=60, device=0, batch_frames=None, out_dev=None,
                           balance=None, ecc_batch=16, step_process=False, native_loop=True, handles=None,
                           keep_handles=False, info=None, chain_refine=True, chain_serial=False, mask_noise=None,
                           vignetting=None, denoise_amount=0, white_balance=None, unsharp=None, depth_map=None, stereo=None,
                           depth_composite=None, lens=None, estimator=None, matching_config=None, feature_params=None,
                           depth_refine=None,
                           **stack_kwargs):
    """BASELINE config 4 with every frame resident in HBM: `dev_frames` is the device address of
    `n_frames` contiguous H x W x 3 frames.  Each frame is registered against frames[ref_idx] by
    the device ECC estimator (mi_aligner_*), warped with the blurred replicate border of
    align.py:238-251 straight into the stacker's input batch, and fused.  No frame crosses PCIe;
    per frame the host sees 28 doubles per Gauss-Newton iteration.

    The transforms are estimated `ecc_batch` (<= 16) frames at a time in one batched Gauss-Newton
    (mi_aligner_estimate_batch: one launch and one host round trip per iteration for the whole batch --
    a single frame's chain of small kernels leaves the GPU mostly idle), then the frames are warped and
    fused in order.  (Estimating on helper threads, one handle each or one batch ahead, measured no
    faster: the round trips serialise in the runtime.)

    `batch_frames`: warped frames per push into the stacker; None (default) = `auto_batch_frames`: the whole job in one
    push when the device memory allows it (the coarse pyramid levels of small pushes are launch-bound: config 4 takes 0.042 s
    at 16 frames per push, 0.037 s at 128); handles of an earlier call keep the value they were created with.

    `balance`: optional dict of BalanceFrames options (channel, corr_map, subsample, fast_subsampling,
    mask_size, intensity_interval): every aligned frame is then balanced against the reference frame
    (balance.py; the order of the reference's example projects: align, balance, stack) in place on the
    device -- histogram on the GPU, the 256/65536-entry table on the host, table apply on the GPU.

    `keep_handles` / `handles`: a job that fuses many stacks of one geometry keeps the stacker, the estimator and the
    scratch buffers between calls (`keep_handles=True` returns them as a fourth value, `handles=` takes them back; close them
    with `close_handles`): creating them costs 10-35 ms -- pinned host buffers, several GB of device buffers -- beside a
    128-frame job of 45-80 ms.

    `native_loop` (default): without balancing the frame loop runs inside the library (`mi_align_stack_device`); False
    keeps the call-by-call Python loop below (the two are tested equal).

    `info`: an optional dict; with `balance` it receives `info["corrections"]` = the per-frame correction factors the
    reference's sub-action records (balance.py: `self.corrections`), for the frames that were processed.

    `mask_noise` / `vignetting`: optional dicts of the MaskNoise / Vignetting sub-actions' options (`_prestack_steps`).
    Every resident frame, the reference frame included, is then corrected IN PLACE in `dev_frames` -- hot pixels first, then
    the vignetting, the reference's sub-action order -- before any frame is estimated or warped, and the Python frame loop
    is used (as with a non-LINEAR `balance=`; the native loop does not know these steps).  Per frame the vignetting fit costs
    one host round trip (the ring sums).  `info["vignetting_corrections"]` receives the sub-action's percentile radii.
    None (default): nothing is touched.  With `vignetting=` the byte size of a frame must be a multiple of 16
    (InvalidOptionError otherwise: the apply pass needs every frame of the contiguous stack 16-byte aligned).  Because the
    corrections overwrite `dev_frames`, a second call on the same buffer
    with the options set would correct the frames a second time: upload the frames again, or leave the options out.

    `lens`: a `lens.Lens`, or a dict of `LensCorrection`'s options (lens, autoscale): the lens correction (lens.py), a third
    pre-stack step behind those two and under the same terms -- in place in `dev_frames` through one scratch frame, the
    Python frame loop, no handle reuse.  None (default): nothing is built, allocated, loaded or called.

    `step_process=True`: the reference's chained order (see `_align_chains_device`): every frame is registered against
    its already-aligned neighbour; the aligned frames are kept in one extra device buffer (n_frames frames) and fused in
    file order afterwards, so that the stack sees them exactly as the reference's FocusStack reads the aligned files.
    `chain_refine` (default True; ALIGN_RIGID): every chain estimate is refined against the global reference frame before the
    frame is warped, so that the steps' errors do not add up (`_align_chains_device`); False = the plain chain.
    `chain_serial` (default False): the chain as rounds 3-5 ran it -- every step registered against the WARPED neighbour, one
    device synchronisation per frame (`_align_chains_device`); the default factors the chain into independent
    neighbour estimates + composition (`_align_chains_pairs_device`).

    `denoise_amount`: the stack actions' option (`_finish`): when positive the fused frame is denoised on the device before
    it is downloaded or written to `out_dev`.  0 (default): nothing is touched.  `white_balance` (an RGB triple) / `unsharp`
    ((radius, amount, threshold)): the retouch filters, applied on the device after the denoise, in that order; None
    (default): nothing is built, loaded or called.

    `depth_map`: a sigma, or True for the stacker's default -- `info["depth_map"]` then receives the frame index in focus at
    each pixel (H x W float32, `Stack.depth_map`, depth_out.py): an array, or with `out_dev` a `DeviceBuffer` the caller frees.
    None (default): nothing is computed; the return values are the same either way.

    `stereo`: a dict of `stereo.pair`'s options (layout -- default 'anaglyph' --, separation, pivot, near) and `sigma`, the
    depth map's smoothing (default: the `depth_map=` sigma, else the stacker's own) -- `info["stereo"]` then receives the
    stereo pair of the fused frame, rendered on the device from the final frame and the depth plane before anything is
    downloaded (stereo.py); it is an array, with `out_dev` too.  None (default): nothing is built, loaded or called.

    `depth_composite`: a dict of `interp` ('linear' or 'nearest') and `sigma` (default: the `depth_map=` sigma, else the
    stacker's own) -- `info["depth_composite"]` then receives the depth-selected composite (depth_render.py) of the aligned
    (and balanced) frames as the stacker saw them, as a `DeviceBuffer` the caller frees.  The aligned frames are gathered where
    they lie -- the `step_process` buffer, or the stacker's input batch -- so no copy is made; without `step_process` that needs
    the whole job in one push (`batch_frames` >= `n_frames`, InvalidOptionError otherwise).  None (default): nothing is built,
    loaded or called.

    `estimator`: None / "ecc" (default) is the ECC estimator described above.  "features": every frame is registered by the
    feature estimator instead (features.py: FAST-9 corners, rotated box-sum descriptors, Hamming matches, RANSAC), which has no
    capture range, on one `features.FeatureAligner` handle -- `ecc_batch` frames per call, two host waits per call -- in the
    Python frame loop.  `matching_config` (match_method, threshold) and `alignment_config` (transform, rans_threshold, max_iters,
    subsample, fast_subsampling, min_good_matches) are read as `align_images` reads them; `feature_params`: a
    `features.FeatureParams`.  The third return value then holds every frame's inlier fraction (1.0 at ref_idx);
    `min_correlation` and `max_iters` (ECC's) are not used.  A frame without a model raises AlignmentError.  A frame with no
    more than `min_good_matches` good matches while `subsample` > 1 is estimated again at subsample 1, on a second handle
    created on first need (the reference's `align_images` retries the same way): `info["feature_retries"]` lists those frames,
    `info["good_matches"]` receives every frame's count.  Refused with InvalidOptionError before anything is allocated:
    `step_process=True`, `handles=` / `keep_handles=`, `align_method='LMEDS'`, area sub-sampling other than by 2 on even sides
    (`fast_subsampling=True` runs those), more than 4096 features or RANSAC iterations.

    `depth_refine`: a dict of `radius` and `eps`, as `align_and_stack` takes it -- every depth map this call makes (`depth_map=`,
    the `stereo=` render, the `depth_composite=` render) is refined against the fused frame as the stacker returned it, kept in a
    device copy until the call ends; best with the unsmoothed index, `depth_map=0.0`.  Refused without any of the three
    consumers.  None (default): nothing is built, copied or called.

    Brush retouching (`align_and_stack`'s `retouch=`) is not offered here: the frames live in the caller's buffer and the handles
    are reused between calls, so the caller paints the result itself with `retouch.apply_device`.

    Returns (fused image as ndarray, or None when `out_dev` -- a device address for the result --
    is given; list of 2x3 transforms, None at ref_idx; list of correlation coefficients)."""
    _check_denoise_amount(denoise_amount)
    if white_balance is not None or unsharp is not None:
        _check_retouch(white_balance, unsharp, dtype)
    dm_sigma = _check_depth_map(depth_map, info, (height, width))
    sv_opts = _check_stereo(stereo, info, (height, width), dm_sigma) if stereo is not None else None
    dc_opts = _check_depth_composite(depth_composite, info, (height, width), dm_sigma) if depth_composite is not None else None
    rf_opts = _check_depth_refine(depth_refine, (height, width), dm_sigma, sv_opts, dc_opts)
    stack_kwargs["arith"] = resolve_arith(stack_kwargs.get("arith"), stack_kwargs.get("float_type"))   # one default for every entry point
    if vignetting is not None and (height * width * 3 * np.dtype(dtype).itemsize) % 16:
        # mi_vignette_apply_device works on 16-byte accesses: every frame of the contiguous stack must start on one
        raise InvalidOptionError("vignetting", f"{height} x {width} {np.dtype(dtype).name}",
                                 "with vignetting= the byte size of a resident frame must be a multiple of 16 (the frames are "
                                 "contiguous and the apply pass needs each 16-byte aligned); use Vignetting.run_frame on host frames")
    # estimator='features': what it does not offer is refused before a device is looked for
    if estimator not in (None, "ecc", "features"):
        raise InvalidOptionError("estimator", estimator, ". Valid options are: None, 'ecc', 'features' (the resident frames are "
                                 "registered on the device)")
    use_features = estimator == "features"
    if use_features:
        from . import features as _features
        if step_process:
            raise InvalidOptionError("estimator", estimator, ": step_process=True is not implemented with estimator='features'")
        if handles is not None or keep_handles:
            raise InvalidOptionError("estimator", estimator, ": handle reuse (handles= / keep_handles=) is not implemented with "
                                     "estimator='features'")
        fcfg = {**_DEFAULT_ALIGNMENT_CONFIG, **(alignment_config or {})}
        _features.FeatureAligner.options(matching_config, fcfg)
        _features.check_subsampling(height, width, max(1, int(fcfg['subsample'])), bool(fcfg['fast_subsampling']))
        if feature_params is not None and feature_params.n_features > _lib.FeatureAligner.MAX_FEATURES:
            raise InvalidOptionError("n_features", feature_params.n_features,
                                     f": the resident feature estimator keeps at most {_lib.FeatureAligner.MAX_FEATURES} keypoints on level 0")
        native_loop = False
    _lib.require_device()
    if n_frames < 1:
        raise ValueError("no frames")
    cfg = {**_DEFAULT_ALIGNMENT_CONFIG, **(alignment_config or {})}
    if cfg['border_mode'] not in _BORDER_CODE:
        raise InvalidOptionError("border_mode", cfg['border_mode'])
    if cfg['transform'] not in (constants.ALIGN_RIGID, constants.ALIGN_HOMOGRAPHY):
        raise InvalidOptionError("transform", cfg['transform'])
    # the device estimator finds a similarity; with ALIGN_HOMOGRAPHY it is applied through the projective warp
    homography = cfg['transform'] == constants.ALIGN_HOMOGRAPHY
    if ref_idx == -1:
        ref_idx = n_frames // 2
    dt = np.dtype(dtype)
    fb = height * width * 3 * dt.itemsize
    lib = _lib.load()
    pre = _prestack_steps(mask_noise, vignetting, n_frames, device, lens)
    if pre:
        if handles is not None or keep_handles:
            raise InvalidOptionError("handles", "reuse", ": handle reuse is not implemented with mask_noise= / vignetting= / lens=")
        native_loop = False
        for i in range(n_frames):
            for step in pre:
                step.run_frame_device(i, dev_frames + i * fb, height, width, dt)
        _lib.check(lib.mi_device_synchronize(device))   # the corrections ran on the default stream
        _prestack_info(pre, info)
    if step_process:
        reusing = handles is not None or keep_handles
        if reusing and (chain_serial or homography):
            raise InvalidOptionError("handles", "reuse", ": with step_process, handle reuse is implemented for the factored ALIGN_RIGID "
                                     "chain (not chain_serial, not ALIGN_HOMOGRAPHY)")
        sub = max(1, int(cfg['subsample']))
        geometry = dict(height=int(height), width=int(width), dtype=dt.name, step_process=True, frames=int(n_frames), subsample=sub,
                        fast=bool(cfg['fast_subsampling']), device=int(device),
                        stack_kwargs=tuple(sorted((k, repr(v)) for k, v in stack_kwargs.items())))
        created = []
        if handles is not None:
            bad = handles.mismatch(**geometry)
            if bad:
                raise InvalidOptionError("handles", {k: geometry[k] for k in bad},
                                         f": these handles were created for {({k: handles.geometry.get(k) for k in bad})}")
            stack, aligner, aligned, tmp, mask = handles
            gref = handles.gref
            stack.reset()
        else:
            aligned = _lib.DeviceBuffer(fb * n_frames, device)
            created.append(aligned.free)
            aligner = gref = tmp = mask = None
            if reusing:
                aligner = _lib.Aligner(height, width, dt, subsample=sub, device=device, fast=bool(cfg['fast_subsampling']))
                gref = _lib.Aligner(height, width, dt, subsample=sub, device=device, fast=bool(cfg['fast_subsampling']))
                tmp, mask = _lib.DeviceBuffer(fb, device), _lib.DeviceBuffer(height * width, device)
                created += [aligner.close, gref.close, tmp.free, mask.free]
            stack = None
        done = False
        try:
            corr = None
            if balance is not None:
                corr = _make_correction(balance, device)
                corr.begin_device(dev_frames + ref_idx * fb, height, width, dt, n_frames)
            if chain_serial:
                transforms, ccs = _align_chains_device(lib, dev_frames, aligned.ptr, n_frames, height, width, dt, ref_idx, cfg,
                                                       min_correlation, max_iters, device, corr, chain_refine=chain_refine)
            else:
                transforms, ccs = _align_chains_pairs_device(lib, dev_frames, aligned.ptr, n_frames, height, width, dt, ref_idx, cfg,
                                                             min_correlation, max_iters, device, corr, chain_refine=chain_refine,
                                                             reuse=(aligner, gref, tmp, mask) if reusing else None)
            if stack is None:
                stack = _lib.Stack(height, width, in_dtype=dt, out_dtype=dt, device=device, **stack_kwargs)
                created.append(stack.close)
            stack.push_frames_device(aligned.ptr, n_frames, fb)
            dstack = _refined(stack, rf_opts, height, width, dt, device)
            try:
                out = _finish(dstack, out_dev, denoise_amount, height, width, dt, device, white_balance, unsharp,
                              _stereo_render(dstack, sv_opts, info, n_frames, height, width, dt, device),
                              _brush_paint(None, {}, height, width, dt, device,
                                           _composite_render(dstack, dc_opts, info, lambda: [aligned.ptr + i * fb for i in range(n_frames)],
                                                             height, width, dt, device, True)))
                _depth_map_info(dstack, dm_sigma, info, out_dev is not None, height, width, device)
            finally:
                _release(dstack)
            done = True
        finally:
            if not (keep_handles and done):
                for release in reversed(created):
                    release()
        if keep_handles:
            return out, transforms, ccs, (handles if handles is not None else
                                          StackHandles(stack, aligner, aligned, tmp, mask, gref=gref, **geometry))
        return out, transforms, ccs
    ecc_batch = max(1, min(int(ecc_batch), _lib.Aligner.MAX_BATCH))
    if batch_frames is None:   # handles of an earlier call fix it; else as many frames per push as memory allows
        batch_frames = handles.geometry["batch_frames"] if handles is not None else auto_batch_frames(n_frames, height, width, dt, device)
    geometry = dict(height=int(height), width=int(width), dtype=dt.name, batch_frames=int(batch_frames),
                    subsample=max(1, int(cfg['subsample'])), fast=bool(cfg['fast_subsampling']), device=int(device),
                    stack_kwargs=tuple(sorted((k, repr(v)) for k, v in stack_kwargs.items())))   # the stacker's own options
    # everything that can be refused is refused BEFORE anything is allocated
    if dc_opts is not None and n_frames > batch_frames:
        raise InvalidOptionError("depth_composite", depth_composite, f"the composite gathers the aligned frames where they lie: the {n_frames} "
                                 f"frames must pass in one push (batch_frames = {batch_frames}), or use step_process=True")
    corr = bal_opts = None
    if balance is not None:
        corr = _make_correction(balance, device)
    native = native_loop and (balance is None or corr.supports_native_linear())
    if (handles is not None or keep_handles) and not native:
        raise InvalidOptionError("handles", "reuse", ": handle reuse is implemented for the native loop (no balancing, or the "
                                 "LINEAR map)")
    if handles is not None:   # handles of an earlier call (a job of many stacks): nothing is allocated here
        bad = handles.mismatch(**geometry)
        if bad:
            raise InvalidOptionError("handles", {k: geometry[k] for k in bad},
                                     f": these handles were created for {({k: handles.geometry.get(k) for k in bad})}; the "
                                     "scratch buffers are sized for that geometry (close them and let the call allocate)")
        stack, aligner, batches, tmp, mask = handles
        stack.reset()
        created = None
    else:
        stack = _lib.Stack(height, width, in_dtype=dt, out_dtype=dt, device=device, batch_frames=batch_frames,
                           **stack_kwargs)
        try:
            if use_features:
                aligner = _features.FeatureAligner(height, width, dt, feature_params, subsample=max(1, int(cfg['subsample'])),
                                                   fast=bool(cfg['fast_subsampling']), max_batch=ecc_batch, device=device)
            else:
                aligner = _lib.Aligner(height, width, dt, subsample=max(1, int(cfg['subsample'])), device=device,
                                       fast=bool(cfg['fast_subsampling']))
        except BaseException:
            stack.close()
            raise
        created = [stack, aligner]     # released here whenever an exception leaves this call
    if native:
        # the whole loop below in ONE library call (mi_align_stack_device): same kernels in the same order on the same
        # streams; the ~25 ctypes calls per frame of the Python loop made the pipeline's pace depend on how busy the host is
        # (0.08 s on an idle box, 0.3 s on a shared one, for 128 x 24 MP)
        done = False
        try:
            if corr is not None:
                corr.begin_device(dev_frames + ref_idx * fb, height, width, dt, n_frames)
                bal_opts = corr.native_linear_opts()
            if handles is None:
                batches = _lib.DeviceBuffer(2 * fb * batch_frames, device)
                created.append(batches)
                tmp = _lib.DeviceBuffer(fb, device)
                created.append(tmp)
                mask = _lib.DeviceBuffer(height * width, device)
                created.append(mask)
            opts = _lib.AlignStackOpts(transform=int(homography), border_mode=_BORDER_CODE[cfg['border_mode']],
                                       border_value=(C.c_double * 4)(*(list(cfg['border_value']) + [0, 0, 0, 0])[:4]),
                                       blur_ksize=21, blur_sigma=float(cfg['border_blur']),
                                       min_correlation=float(min_correlation), max_iters=int(max_iters), eps=1e-9,
                                       ecc_batch=ecc_batch, batch_frames=int(batch_frames))
            M = (C.c_double * (9 * n_frames))()
            cc = (C.c_double * n_frames)()
            failed = C.c_int(-1)
            rc = lib.mi_align_stack_device(stack._h, aligner._h, dev_frames, n_frames, fb, ref_idx, C.byref(opts),
                                           C.byref(bal_opts) if bal_opts is not None else None, batches.ptr,
                                           tmp.ptr, mask.ptr, M, cc, C.byref(failed))
            if bal_opts is not None:
                # only the frames the library got to have a correction row on the device (it stops at the first
                # frame whose correlation is too low: those from `failed` on were never balanced)
                stop = failed.value if rc == _lib.MI_ERR_ALIGNMENT and failed.value >= 0 else n_frames
                corr._corr_pending.extend(i for i in range(stop) if i != ref_idx)
                if info is not None:
                    info["corrections"] = corr.fetch_corrections()
            if rc == _lib.MI_ERR_ALIGNMENT:
                raise AlignmentError(failed.value, f"correlation {cc[failed.value]:.3f} < {min_correlation}")
            _lib.check(rc)
            ms = np.array(M, dtype=np.float64).reshape(n_frames, 9)
            transforms = [None if i == ref_idx else (ms[i].reshape(3, 3).copy() if homography else ms[i, :6].reshape(2, 3).copy())
                          for i in range(n_frames)]
            ccs = [float(c) for c in cc]
            dstack = _refined(stack, rf_opts, height, width, dt, device)
            try:
                out = _finish(dstack, out_dev, denoise_amount, height, width, dt, device, white_balance, unsharp,
                              _stereo_render(dstack, sv_opts, info, n_frames, height, width, dt, device),
                              _brush_paint(None, {}, height, width, dt, device,
                                           _composite_render(dstack, dc_opts, info, lambda: [batches.ptr + i * fb for i in range(n_frames)],
                                                             height, width, dt, device, True)))
                _depth_map_info(dstack, dm_sigma, info, out_dev is not None, height, width, device)
            finally:
                _release(dstack)
            done = True
        finally:
            if created is not None and not (keep_handles and done):
                for obj in created:
                    obj.close() if hasattr(obj, "close") else obj.free()
        if keep_handles:
            return out, transforms, ccs, (handles if handles is not None else
                                          StackHandles(stack, aligner, batches, tmp, mask, **geometry))
        return out, transforms, ccs
    try:
        if corr is not None:
            corr.begin_device(dev_frames + ref_idx * fb, height, width, dt, n_frames)
    except BaseException:
        for obj in created or ():
            obj.close()
        raise
    tmp = _lib.DeviceBuffer(fb, device)
    mask = _lib.DeviceBuffer(height * width, device)
    # two batches of warped frames: one is being fused while the next is being filled
    batches = [_lib.DeviceBuffer(fb * batch_frames, device) for _ in range(2)]
    mode = _BORDER_CODE[cfg['border_mode']]
    bv = (C.c_double * 4)(*(list(cfg['border_value']) + [0, 0, 0, 0])[:4])
    transforms, ccs = [], []
    cur, filled = 0, 0
    st = stack.stream   # warps, balance and the reference-frame copy run on the stacker's own stream
    aligner.set_reference(dev_frames + ref_idx * fb)
    estimates = {}
    retry = []                              # estimator='features': the handle at subsample 1, created on first need
    good_matches, feature_retries = [0] * n_frames, []
    if use_features and info is not None:
        info["good_matches"], info["feature_retries"] = good_matches, feature_retries

    def estimate_from(i):
        """transforms of the next `ecc_batch` moving frames starting at frame i"""
        idx = [k for k in range(i, n_frames) if k != ref_idx][:ecc_batch]
        if use_features:
            for k, (ng, m, frac) in zip(idx, aligner.estimate_batch([dev_frames + k * fb for k in idx], matching_config, cfg)):
                if ng <= cfg['min_good_matches'] and aligner.subsample > 1:     # align_images' retry without sub-sampling
                    if not retry:
                        retry.append(_features.FeatureAligner(height, width, dt, feature_params, subsample=1, max_batch=1,
                                                              device=device))
                        retry[0].set_reference(dev_frames + ref_idx * fb)
                    ng, m, frac = retry[0].estimate_batch([dev_frames + k * fb], matching_config, cfg)[0]
                    feature_retries.append(k)
                good_matches[k] = ng
                estimates[k] = (m, frac)
            return
        fit = aligner.estimate_homography_batch if homography else aligner.estimate_batch
        ms, cs, _ = fit([dev_frames + k * fb for k in idx], max_iters=max_iters)
        for k, m, c in zip(idx, ms, cs):
            estimates[k] = (m, float(c))

    to_balance = []   # (frame index, device address) of the warped frames of the batch being filled

    def flush():
        nonlocal cur, filled
        if filled and corr is not None and to_balance:
            # the whole batch behind ONE host round trip (GAMMA / MATCH_HIST: the histograms come back together, SciPy
            # builds the tables, the table applies are enqueued; LINEAR: no round trip at all)
            corr.apply_correction_device_batch([i for i, _ in to_balance], [p for _, p in to_balance], st)
            to_balance.clear()
        if filled:
            # No host synchronisation here: the warps run on the stacker's stream, where the level-0 kernels that read
            # this batch are enqueued next, and the stacker joins its side streams into that stream after every push --
            # so the batch buffer written two flushes later is free by stream order.  The host goes straight on to the
            # next batch's estimate (its own stream), which then overlaps these warps and the fuse.
            stack.push_frames_device(batches[cur].ptr, filled, fb)
            cur ^= 1
            filled = 0

    try:
        for i in range(n_frames):
            src = dev_frames + i * fb
            dst = batches[cur].ptr + filled * fb
            if i == ref_idx:
                _lib.check(lib.mi_memcpy_d2d_async(device, st, dst, src, fb))   # align.py:279-280
                transforms.append(None)
                ccs.append(1.0)
            else:
                if i not in estimates:
                    estimate_from(i)
                m, cc = estimates.pop(i)
                if use_features:
                    if m is None:
                        raise AlignmentError(i, f"no transform found from {good_matches[i]} good matches")
                    mm = (C.c_double * m.size)(*np.asarray(m, dtype=np.float64).reshape(-1))
                else:
                    if not cc >= min_correlation:
                        raise AlignmentError(i, f"correlation {cc:.3f} < {min_correlation}")
                    mm = (C.c_double * m.size)(*m.reshape(-1))
                warp = lib.mi_warp_perspective_device if homography else lib.mi_warp_affine_device
                _lib.check(warp(device, st, src, dst, tmp.ptr, mask.ptr, height, width, _lib.DTYPE_CODE[dt], mm, mode, bv, 21,
                                float(cfg['border_blur'])))
                if corr is not None:
                    to_balance.append((i, dst))
                transforms.append(m)
                ccs.append(cc)
            filled += 1
            if filled == batch_frames:
                flush()
        flush()
        dstack = _refined(stack, rf_opts, height, width, dt, device)
        try:
            out = _finish(dstack, out_dev, denoise_amount, height, width, dt, device, white_balance, unsharp,
                          _stereo_render(dstack, sv_opts, info, n_frames, height, width, dt, device),
                          _brush_paint(None, {}, height, width, dt, device,
                                       _composite_render(dstack, dc_opts, info, lambda: [batches[0].ptr + i * fb for i in range(n_frames)],
                                                         height, width, dt, device, True)))
            _depth_map_info(dstack, dm_sigma, info, out_dev is not None, height, width, device)
        finally:
            _release(dstack)
        if corr is not None and info is not None:
            info["corrections"] = corr.fetch_corrections()
    finally:
        aligner.close()
        for extra in retry:
            extra.close()
        stack.close()
        for b in [tmp, mask] + batches:
            b.free()
    return out, transforms, ccs


def bunches_then_stack(get_frame, n_frames, height, width, dtype, frames=constants.DEFAULT_FRAMES,
                       overlap=constants.DEFAULT_OVERLAP, device=0, out_dev=None, on_bunch=None, on_final=None,
                       check_running=None, stacks=None, results_buf=None, info=None, zero_copy=False, denoise_amount=0,
                       white_balance=None, unsharp=None, mosaic=None, develop=None, calibration=None, packed=False,
                       depth_refine=None, **stack_kwargs):
    """BASELINE config 5's two-stage flow in memory (the reference's `FocusStackBunch` followed by `FocusStack`,
    stack.py:61-113, examples/stack-from-frames): the frames are fused in bunches of `frames` with `overlap` shared
    (`get_bunches`), every bunch result is the stacker's OUTPUT type -- truncated to the input dtype exactly as the file
    the reference writes between the two actions (stack.py:33-36, pyramid.py:179) -- and the bunch results are fused once
    more.  Stage 1 takes the frames from HOST memory through the pinned asynchronous upload of `mi_stack_push_frame`
    (`get_frame(i) -> H x W x 3 array`; decode / generate, PCIe and kernels overlap); the bunch results never leave the
    device: they are written side by side into one buffer and stage 2 consumes them in place.

    The reference fuses the bunches in the order `chunks[count - 1]` (stack.py:97: the last one first); every bunch is an
    independent stack and the second action reads the results sorted by the name of each bunch's first frame, i.e. in
    bunch order -- which is the order used here.

    `on_bunch(k, stack)` / `on_final(stack, results_buffer)`: called after a bunch's / the final stack's frames were pushed and before it is
    finished (tests tap the selection state there).  `stacks`: optional `_lib.Stack` handles to reuse, the LAST one for stage 2
    and the others (one, or two that alternate so that uploads and kernels of neighbouring bunches overlap) for stage 1 -- a handle owns pinned upload buffers and gigabytes of device buffers whose allocation costs more than a
    short job; they are reset, not closed.  `results_buf`: an optional `_lib.DeviceBuffer` of at least n_bunches frames for the
    bunch results (`hipMalloc` / `hipFree` of the 38 GB a 1024-frame job needs cost ~2 s: a caller that runs job after job
    keeps it); it is not freed here.  `info`: an optional dict that receives `stage1_s` (first push to the last bunch result
    on the device) and `stage2_s` (the stack over the bunch results, to its result).  `denoise_amount`: when positive the final
    result is denoised on the device before it is downloaded or written to `out_dev` (`_finish`; the reference's
    FocusStack(denoise_amount=...) behind a FocusStackBunch without it); 0 (default) touches nothing.  `white_balance` /
    `unsharp`: the retouch filters on the final result, after the denoise (`_finish`); None (default) touches nothing.
    `mosaic`: a `demosaic.Cfa` -- `get_frame(i)` then returns the frame's raw H x W mosaic, stage 1 pushes mosaics (a third of
    the bytes over the host link, demosaiced on the device behind the upload) and stage 2 is what it is without it: bunch
    results are BGR on the device.  None (default): nothing of that is called.  `develop`: a `demosaic.Develop` beside `mosaic`
    -- defect sites, colour matrix and tone curve around stage 1's demosaic; it must stay open until this returns.  `calibration`: a `demosaic.Calibration` beside `mosaic` -- master dark and flat field
    on the raw samples of stage 1, ahead of both; it too stays open until this returns.  `packed`: `get_frame(i)` returns a
    `dng.DngFrame` and stage 1 pushes its packed span (`Stack.push_packed`: the file's sample bytes as they lie, unpacked on the
    device, demosaiced with the frame's own Cfa; `develop` and `calibration` apply as beside `mosaic`).  Returns the fused image (or None when `out_dev` is given) and the list of
    bunches (frame indices).  `depth_refine`: the option of `align_and_stack`; this flow returns no depth map, so anything but
    None is refused, as the option without a consumer is there."""
    from .actions import get_bunches
    _check_denoise_amount(denoise_amount)
    _check_depth_refine(depth_refine, (height, width))     # (this flow returns no depth map: the option has no consumer here)
    if white_balance is not None or unsharp is not None:
        _check_retouch(white_balance, unsharp, dtype)
    if packed and mosaic is not None:
        raise InvalidOptionError("packed", packed, "a packed frame carries its own Cfa: mosaic= does not go with it")
    if (develop is not None or calibration is not None) and not packed:
        from .demosaic import require_mosaic
        require_mosaic(mosaic, develop, calibration)
    stack_kwargs["arith"] = resolve_arith(stack_kwargs.get("arith"), stack_kwargs.get("float_type"))   # one default for every entry point
    _lib.require_device()
    if overlap >= frames:
        raise InvalidOptionError("overlap", overlap, "overlap must be smaller than batch size")
    dt = np.dtype(dtype)
    fb = height * width * 3 * dt.itemsize
    bunches = get_bunches(list(range(n_frames)), frames, overlap)
    if not bunches:
        raise ValueError("no frames")
    if stacks is not None and len(stacks) < 2:
        raise InvalidOptionError("stacks", len(stacks), ": at least two handles are needed (the last one is stage 2, the others stage 1)")
    own_results = results_buf is None
    if not own_results and results_buf.nbytes < fb * len(bunches):
        raise InvalidOptionError("results_buf", results_buf.nbytes, f": {len(bunches)} bunch results need {fb * len(bunches)} bytes")
    results = _lib.DeviceBuffer(fb * len(bunches), device) if own_results else results_buf
    t_start = time.perf_counter()
    # Stage 1 alternates between TWO handles: resetting a handle waits for ITS previous bunch only, so the uploads of bunch
    # k + 1 (handle B's copy stream) run while bunch k is still being fused (handle A) -- with one handle the PCIe link
    # idled through every bunch's kernels and collapse (measured: 38 GB/s of a 57 GB/s link; config 5 is upload-bound).
    if stacks:
        stage1 = list(stacks[:-1])
    else:
        stage1 = [_lib.Stack(height, width, in_dtype=dt, out_dtype=dt, device=device, **stack_kwargs)
                  for _ in range(2 if len(bunches) > 1 else 1)]
    try:
        for k, bunch in enumerate(bunches):
            st = stage1[k % len(stage1)]
            st.reset()      # a handle serves every other bunch, as one stacker object serves FocusStackBunch (stack.py:94-97)
            for i in bunch:
                if packed:
                    st.push_packed(get_frame(i), zero_copy=zero_copy, develop=develop, calibration=calibration)
                elif mosaic is None:
                    st.push_frame(get_frame(i), zero_copy=zero_copy)
                elif calibration is not None:
                    st.push_mosaic(get_frame(i), mosaic, zero_copy=zero_copy, develop=develop, calibration=calibration)
                elif develop is None:
                    st.push_mosaic(get_frame(i), mosaic, zero_copy=zero_copy)
                else:
                    st.push_mosaic(get_frame(i), mosaic, zero_copy=zero_copy, develop=develop)
                if check_running is not None and check_running() is False:
                    from .errors import RunStopException
                    raise RunStopException("bunches_then_stack")
            if on_bunch is not None:
                on_bunch(k, st)
            st.finish_device(results.ptr + k * fb)
        for st in stage1:
            st.sync()
            if packed and st.ljpeg_status():
                from .errors import ImageLoadError
                raise ImageLoadError("stage 1", "lossless JPEG: a segment of a pushed frame did not decode")
    except BaseException:
        for st in stage1:
            try:                # the cleanup must not mask the exception that brought us here
                if stacks:
                    st.sync()   # a reused handle may still be writing into `results`
                else:
                    st.close()
            except Exception:   # noqa: BLE001
                pass
        if own_results:
            results.free()
        raise
    if not stacks:
        for st in stage1:
            st.close()
    st2 = stacks[-1] if stacks else _lib.Stack(height, width, in_dtype=dt, out_dtype=dt, device=device, **stack_kwargs)
    t_stage1 = time.perf_counter()
    try:
        st2.reset()
        st2.push_frames_device(results.ptr, len(bunches), fb)
        if on_final is not None:
            on_final(st2, results)
        out = _finish(st2, out_dev, denoise_amount, height, width, dt, device, white_balance, unsharp)
    finally:
        if not stacks:
            st2.close()
        else:
            st2.sync()      # `results` is freed below
        if own_results:
            results.free()
    if info is not None:
        info.update(stage1_s=t_stage1 - t_start, stage2_s=time.perf_counter() - t_stage1)
    return out, bunches
