"""Stereo views from the depth map: the fused frame re-rendered from viewpoints shifted sideways (no reference counterpart).

`PyramidStack.depth_map()` / `DepthMapStack.depth_map()` say which frame is in focus at each pixel, and the frame number is a
distance.  `view` moves every pixel of the fused image along its row by `shift * (t - pivot)` pixels, t its nearness in
[0, 1]: nearer pixels cover farther ones, and what a moved foreground uncovers is filled from the background beside it.
`pair` puts two such views side by side or into a red-cyan anaglyph, `rocking` gives the sequence of views a viewer flips
through.  One HIP kernel does the work (csrc/kernels_stereo.hpp, whose header is the specification;
tests/stereo_restatement.py restates it in NumPy, bit for bit):

    t  = clamp(depth / float32(N - 1), 0, 1)          0 for a single frame; 1 - t when near == 'first'
    d  = int32(rint(float32(shift) * (t - float32(pivot))))      float32, each operation rounded on its own
    x' = x + d: the largest t wins a target; a target nothing lands on takes the smaller t of the nearest filled targets to its
    left and right (the left one on a tie, the one side that exists, else the source pixel itself).  Samples are copied.

There is no CPU path: without a GPU or the library every entry point raises DeviceError.
"""
import math

import numpy as np

from . import _lib
from .errors import BitDepthError, InvalidOptionError

MAX_SHIFT = 64.0                # MI_SV_MAX_SHIFT: the kernel's halo
MAX_SEPARATION = 2 * MAX_SHIFT
DEFAULT_SEPARATION = 32.0       # pixels between the two viewpoints' renderings of the nearest and the farthest plane
LAYOUTS = {"parallel": 0, "cross": 1, "anaglyph": 2}     # MI_STEREO_PARALLEL / _CROSS / _ANAGLYPH
NEAR = ("last", "first")


def _number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v)


def check_shift(shift, width=None):
    """Raise InvalidOptionError unless |shift| <= 64 and, with `width`, ceil(|shift|) < width; returns float32(shift) as a float"""
    if not _number(shift) or abs(shift) > MAX_SHIFT:
        raise InvalidOptionError("shift", shift, f"a view is shifted by at most {MAX_SHIFT:g} pixels either way")
    if width is not None and math.ceil(abs(shift)) >= width:
        raise InvalidOptionError("shift", shift, f"it does not fit a row of {width} pixels")
    return float(np.float32(shift))


def check_separation(separation, width=None):
    """Raise InvalidOptionError unless 0 < separation <= 128 and, with `width`, half of it fits a row"""
    if not _number(separation) or not 0 < separation <= MAX_SEPARATION:
        raise InvalidOptionError("separation", separation, f"the two views are more than 0 and at most {MAX_SEPARATION:g} pixels apart")
    check_shift(float(separation) / 2.0, width)
    return float(separation)


def check_pivot(pivot):
    if not _number(pivot) or not 0 <= pivot <= 1:
        raise InvalidOptionError("pivot", pivot, "the nearness that stays in place lies in [0, 1]")
    return float(pivot)


def check_near(near):
    if near not in NEAR:
        raise InvalidOptionError("near", near, "which end of the stack is closest to the viewer: 'last' or 'first'")
    return near


def check_layout(layout):
    if layout not in LAYOUTS:
        raise InvalidOptionError("layout", layout, "one of " + ", ".join(repr(k) for k in LAYOUTS))
    return layout


def check_views(views):
    if isinstance(views, bool) or not isinstance(views, (int, np.integer)) or views < 2:
        raise InvalidOptionError("views", views, "a rocking sequence has at least 2 views")
    return int(views)


def check_n_frames(n_frames):
    if isinstance(n_frames, bool) or not isinstance(n_frames, (int, np.integer)) or n_frames < 1:
        raise InvalidOptionError("n_frames", n_frames, "a stack has at least one frame")
    return int(n_frames)


def check_options(layout="anaglyph", separation=DEFAULT_SEPARATION, pivot=0.5, near="last", width=None):
    """Every check of `pair`'s options that needs no image (the actions and the pipeline call this before they stack)"""
    check_layout(layout)
    check_separation(separation, width)
    check_pivot(pivot)
    check_near(near)


def rocking_shifts(separation, views=9):
    """The `views` shifts of a rocking sequence, evenly spaced over [-separation / 2, +separation / 2]:
    float32(-s / 2 + k * s / (views - 1)), computed in float64 and rounded once"""
    s, views = check_separation(separation), check_views(views)
    return [float(np.float32(-s / 2.0 + k * s / (views - 1))) for k in range(views)]


def compose(left, right, layout):
    """The two views of a pair as one image, on host arrays: 'parallel' left | right, 'cross' right | left, 'anaglyph' BGR
    channel 2 from the left view and channels 0 and 1 from the right view"""
    check_layout(layout)
    left, right = np.asarray(left), np.asarray(right)
    if left.shape != right.shape or left.dtype != right.dtype or left.ndim != 3 or left.shape[2] != 3:
        raise InvalidOptionError("views", (left.shape, right.shape), "a pair is two H x W x 3 views of one shape and type")
    if layout == "parallel":
        return np.concatenate([left, right], axis=1)
    if layout == "cross":
        return np.concatenate([right, left], axis=1)
    out = right.copy()
    out[:, :, 2] = left[:, :, 2]
    return out


def _check_frame(image, depth):
    image, depth = np.asarray(image), np.asarray(depth)
    if image.dtype not in (np.uint8, np.uint16):
        raise BitDepthError("uint8 or uint16", image.dtype)
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise InvalidOptionError("image", image.shape, "a view is rendered from an H x W x 3 frame")
    if depth.shape != image.shape[:2]:
        raise InvalidOptionError("depth", depth.shape, f"the depth map is the frame's H x W plane ({image.shape[0]} x {image.shape[1]})")
    return np.ascontiguousarray(image), np.ascontiguousarray(depth, np.float32)


# ---------------------------------------------------------------------------------------------------- device forms
def view_device(dev_img, dev_depth, dev_out, height, width, dtype, n_frames, shift, pivot=0.5, near="last", device=0, stream=None):
    """view() for a frame and a depth plane resident in HBM: `dev_img`, `dev_depth` -> `dev_out` (a buffer of its own).
    Queued on `stream`, not waited for."""
    dt = np.dtype(dtype)
    if dt not in (np.uint8, np.uint16):
        raise BitDepthError("uint8 or uint16", dt)
    if height < 1 or width < 1:
        raise InvalidOptionError("image", (height, width), "a view is rendered from an H x W x 3 frame")
    n_frames, shift, pivot = check_n_frames(n_frames), check_shift(shift, width), check_pivot(pivot)
    near_first = int(check_near(near) == "first")
    _lib.require_device()
    _lib.check(_lib.load().mi_stereo_view_device(int(device), stream, dev_img, dev_depth, dev_out, int(height), int(width),
                                                 _lib.DTYPE_CODE[dt], n_frames, shift, pivot, near_first))


def pair_device(dev_img, dev_depth, height, width, dtype, n_frames, separation=DEFAULT_SEPARATION, pivot=0.5, near="last",
                layout="parallel", device=0):
    """pair() for a frame and a depth plane resident in HBM.  Returns a DeviceBuffer the caller frees: H x 2W x 3 ('parallel',
    'cross') or H x W x 3 ('anaglyph') of `dtype`; the work is queued on the default stream and not waited for (a download
    through the buffer waits)."""
    dt = np.dtype(dtype)
    separation = check_separation(separation, width)
    check_layout(layout)
    fb = int(height) * int(width) * 3 * dt.itemsize
    half = float(np.float32(separation / 2.0))
    bufs = []
    try:
        for _ in range(2):
            bufs.append(_lib.DeviceBuffer(fb, device))
        view_device(dev_img, dev_depth, bufs[0].ptr, height, width, dt, n_frames, half, pivot, near, device)
        view_device(dev_img, dev_depth, bufs[1].ptr, height, width, dt, n_frames, -half, pivot, near, device)
        out = _lib.DeviceBuffer(fb if layout == "anaglyph" else 2 * fb, device)
        try:
            _lib.check(_lib.load().mi_stereo_compose_device(int(device), None, bufs[0].ptr, bufs[1].ptr, out.ptr, int(height),
                                                            int(width), _lib.DTYPE_CODE[dt], LAYOUTS[layout]))
            _lib.check(_lib.load().mi_device_synchronize(int(device)))      # the two views are freed below
        except BaseException:
            out.free()
            raise
        return out
    finally:
        for b in bufs:
            b.free()


# ---------------------------------------------------------------------------------------------------- host forms
def view(image, depth, n_frames, shift, pivot=0.5, near="last", device=0):
    """The frame `image` (H x W x 3 uint8 / uint16, BGR) seen from a viewpoint `shift` pixels to the side: every pixel moves by
    rint(shift * (t - pivot)), t the nearness its `depth` (H x W float32 frame numbers of an `n_frames` stack) gives it.
    Returns a new array of the image's shape and type."""
    image, depth = _check_frame(image, depth)
    n_frames, shift, pivot = check_n_frames(n_frames), check_shift(shift, image.shape[1]), check_pivot(pivot)
    near_first = int(check_near(near) == "first")
    _lib.require_device()
    out = np.empty_like(image)
    _lib.check(_lib.load().mi_stereo_view(int(device), image.ctypes.data, depth.ctypes.data, out.ctypes.data, image.shape[0],
                                          image.shape[1], _lib.DTYPE_CODE[image.dtype], n_frames, shift, pivot, near_first))
    return out


def _resident(image, depth, device):
    """the frame and its depth plane uploaded: (image buffer, depth buffer)"""
    img = _lib.DeviceBuffer(image.nbytes, device)
    try:
        dep = _lib.DeviceBuffer(depth.nbytes, device)
    except BaseException:
        img.free()
        raise
    try:
        img.upload(image)
        dep.upload(depth)
    except BaseException:
        img.free()
        dep.free()
        raise
    return img, dep


def pair(image, depth, n_frames, separation=DEFAULT_SEPARATION, pivot=0.5, near="last", layout="parallel", device=0):
    """A stereo pair: left = view(+separation / 2), right = view(-separation / 2).  layout 'parallel': H x 2W, left then right;
    'cross': right then left; 'anaglyph': H x W, BGR channel 2 from the left view, channels 0 and 1 from the right view."""
    image, depth = _check_frame(image, depth)
    h, w = image.shape[:2]
    check_n_frames(n_frames)
    check_options(layout, separation, pivot, near, w)
    _lib.require_device()
    img, dep = _resident(image, depth, device)
    try:
        out = pair_device(img.ptr, dep.ptr, h, w, image.dtype, n_frames, separation, pivot, near, layout, device)
        try:
            return out.download((h, w if layout == "anaglyph" else 2 * w, 3), image.dtype)
        finally:
            out.free()
    finally:
        img.free()
        dep.free()


def rocking(image, depth, n_frames, separation=DEFAULT_SEPARATION, views=9, pivot=0.5, near="last", device=0):
    """`views` views with shifts evenly spaced over [-separation / 2, +separation / 2] (`rocking_shifts`), as a list of images:
    shown in turn, back and forth, they rock the subject.  The frame is uploaded once."""
    image, depth = _check_frame(image, depth)
    h, w = image.shape[:2]
    check_n_frames(n_frames)
    check_separation(separation, w)
    check_pivot(pivot)
    check_near(near)
    shifts = rocking_shifts(separation, views)
    _lib.require_device()
    img, dep = _resident(image, depth, device)
    out = None
    try:
        out = _lib.DeviceBuffer(image.nbytes, device)
        frames = []
        for s in shifts:
            view_device(img.ptr, dep.ptr, out.ptr, h, w, image.dtype, n_frames, s, pivot, near, device)
            frames.append(out.download(image.shape, image.dtype))
        return frames
    finally:
        for b in (img, dep, out):
            if b is not None:
                b.free()
