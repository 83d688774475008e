"""Depth map output: the frame index in focus at each pixel, from either stacker (no reference counterpart).

Both stackers decide per pixel which frame is in focus; `PyramidStack.depth_map()` and `DepthMapStack.depth_map()` return that
decision as an H x W float32 array in frame numbers [0, N - 1], computed on the device from the state the last stack left
behind (csrc/kernels_depth.hpp).  This module holds what needs no device -- the Gaussian taps, the option checks and the
16-bit quantiser of the PNG the actions write -- and the binding of the stand-alone smoothing primitive.

Confidence-weighted smoothing of a value plane v with weights w >= 0:

    out = B(v * w) / B(w)  where B(w) > 0,  else v          B: separable Gaussian, BORDER_REFLECT_101

in a fixed evaluation order (the header of kernels_depth.hpp; tests/depth_restatement.py restates it in NumPy, bit for bit):
radius = ceil(3 sigma), 2 radius + 1 taps exp(-x^2 / (2 sigma^2)) computed and normalised in float64 (sum in ascending order),
rounded once to the working type; p = v * w; rows, then columns, each `acc = acc + tap * x` over ascending taps with the
product and the sum rounded separately; one divide; float32 out.  The working type is float32 or float64.
There is no CPU path: without a GPU or the library `weighted_smooth` and the `depth_map` methods raise DeviceError.

Edge-aware refinement (`refine=` of the depth_map methods, `depth_refine=` of the actions and the pipeline, `guided_refine`
here; csrc/kernels_guided.hpp, restated in tests/guided_restatement.py): the Gaussian above knows nothing of where the subject
ends, so a sharp subject's depth bleeds several sigma into a smooth background whose own weights are tiny.  The
confidence-weighted guided filter (He, Sun, Tang) fits depth ~ a I + b to the fused frame's grey I in every (2 radius + 1)^2
window, clipped to the frame, under the same weights, and averages the fits that cover a pixel:

    I = ((1868 B + 9617 G + 4899 R + 8192) >> 14) / 255 or / 65535      t1 = w I, t2 = w p, t3 = t1 I, t4 = t1 p
    sw, swI, swp, swII, swIp = B(w), B(t1), B(t2), B(t3), B(t4)          B: box sum, rows then columns, taps ascending, 0 outside
    where sw > 0: mI = swI / sw, mp = swp / sw, a = (swIp / sw - mI mp) / (swII / sw - mI mI + eps), b = mp - a mI; else a = 0, b = p
    out = clamp((B(a) / n) I + B(b) / n, lo, hi)                         n: the pixels of the clipped window

all in float64, every operation rounded on its own, float32 out.  The clamp is there because a linear model overshoots and the
stereo views and the composite assume frame numbers inside the stack.  Refinement works best on the unsmoothed map
(`depth_map=0.0`): a map the Gaussian has smoothed already carries the bleed in its values, where the weights along the edge no
longer tell it from the truth -- refining the sigma-2 map gains almost nothing over the Gaussian alone.
"""
import math
import os
import struct
import zlib

import numpy as np

from . import _lib
from .errors import InvalidOptionError

MAX_SIGMA = 16.0            # MI_WS_MAX_SIGMA: a radius of at most 48
PYRAMID_SIGMA = 2.0         # PyramidStack.depth_map's default: a hard arg-max wants smoothing
DEPTH_MAP_SIGMA = 0.0       # DepthMapStack.depth_map's default: a weighted mean is smooth already
REFINE_RADIUS = 6           # the refinement's defaults: a window of 13 x 13 ...
REFINE_EPS = 1e-4           # ... and a regulariser of (1 % of the grey range)^2
MAX_REFINE_RADIUS = 32      # MI_GUIDED_MAX_RADIUS
MIN_REFINE_EPS, MAX_REFINE_EPS = 1e-9, 1e3
SCRATCH_PLANES = 7          # MI_GUIDED_SCRATCH_PLANES: float64 planes of one call of the device form


def _number(sigma):
    return isinstance(sigma, (int, float, np.integer, np.floating)) and not isinstance(sigma, bool) and math.isfinite(sigma)


def radius_of(sigma):
    """ceil(3 sigma): the half width of the window"""
    return int(math.ceil(3.0 * float(sigma)))


def check_sigma(sigma, shape=None):
    """Raise InvalidOptionError unless 0 <= sigma <= 16 and, with `shape` = (H, W), its radius fits the plane"""
    if not _number(sigma) or sigma < 0 or sigma > MAX_SIGMA:
        raise InvalidOptionError("sigma", sigma, f"the depth map's smoothing takes 0 (none) to {MAX_SIGMA:g}")
    if shape is not None and sigma > 0 and radius_of(sigma) >= min(shape[0], shape[1]):
        raise InvalidOptionError("sigma", sigma, f"its radius of {radius_of(sigma)} pixels does not fit a plane of "
                                 f"{shape[1]}x{shape[0]}")
    return float(sigma)


def gaussian_taps(sigma, dtype=np.float32):
    """The 2 ceil(3 sigma) + 1 taps of the smoothing in `dtype` (float32 / float64): exp(-x^2 / (2 sigma^2)) in float64,
    divided by their sum (accumulated in ascending order), rounded once"""
    if not _number(sigma) or not 0 < sigma <= MAX_SIGMA:
        raise InvalidOptionError("sigma", sigma, f"the taps exist for 0 < sigma <= {MAX_SIGMA:g}")
    dt = np.dtype(dtype)
    if dt not in (np.float32, np.float64):
        raise InvalidOptionError("dtype", dt, "the working type is float32 or float64")
    sigma = float(sigma)
    radius = radius_of(sigma)
    t = [math.exp(-(float(x) * float(x)) / (2.0 * sigma * sigma)) for x in range(-radius, radius + 1)]
    total = 0.0
    for v in t:
        total += v
    return np.array([v / total for v in t], np.float64).astype(dt)


def quantize(depth, n_frames):
    """The 16-bit grey value of a depth map: floor(D / (N - 1) * 65535 + 0.5), 0 for a single frame"""
    d = np.asarray(depth, np.float64)
    if int(n_frames) < 1:
        raise InvalidOptionError("n_frames", n_frames, "a stack has at least one frame")
    if int(n_frames) == 1:
        return np.zeros(d.shape, np.uint16)
    q = np.floor(d / float(int(n_frames) - 1) * 65535.0 + 0.5)
    return np.clip(q, 0, 65535).astype(np.uint16)


def write_png16(path, grey):
    """H x W uint16 -> 16-bit grey PNG (big-endian samples, Up filter, zlib level 1)"""
    g = np.asarray(grey)
    if g.ndim != 2 or g.dtype != np.uint16 or g.size == 0:
        raise InvalidOptionError("grey", (g.shape, g.dtype), "a 16-bit grey PNG takes an H x W uint16 plane")
    h, w = g.shape
    be = np.ascontiguousarray(g).astype(">u2").view(np.uint8).reshape(h, w * 2)
    rows = np.empty((h, 1 + w * 2), np.uint8)
    rows[0, 0], rows[0, 1:] = 0, be[0]
    rows[1:, 0], rows[1:, 1:] = 2, be[1:] - be[:-1]

    def chunk(typ, body):
        return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body) & 0xffffffff)
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)) +
                 chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + chunk(b"IEND", b""))


def save(directory, name, depth, n_frames):
    """Write quantize(depth, n_frames) to `directory`/`name`.png (the directory is created); returns the file's path"""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, name + ".png")
    write_png16(path, quantize(depth, n_frames))
    return path


def weighted_smooth(value, weight, sigma, device=0):
    """out = B(value * weight) / B(weight) where B(weight) > 0, else value, on the GPU (mi_weighted_smooth).

    `weight`: H x W float32 or float64, >= 0 -- its type is the working type; `value`: H x W int32, or the weight's type.
    Returns H x W float32."""
    w = np.asarray(weight)
    v = np.asarray(value)
    if w.dtype not in (np.float32, np.float64):
        raise InvalidOptionError("weight", w.dtype, "the weight plane is float32 or float64")
    if v.dtype != np.int32 and v.dtype != w.dtype:
        raise InvalidOptionError("value", v.dtype, f"the value plane is int32 or {w.dtype}, the weight's type")
    if v.ndim != 2 or v.shape != w.shape or v.size == 0:
        raise InvalidOptionError("value", v.shape, f"value and weight are H x W planes of one shape (weight: {w.shape})")
    sigma = check_sigma(sigma, v.shape)
    _lib.require_device()
    v, w = np.ascontiguousarray(v), np.ascontiguousarray(w)
    out = np.empty(v.shape, np.float32)
    _lib.check(_lib.load().mi_weighted_smooth(int(device), v.ctypes.data, w.ctypes.data, v.shape[0], v.shape[1],
                                              int(v.dtype == np.int32), _lib.MI_F64 if w.dtype == np.float64 else _lib.MI_F32,
                                              sigma, out.ctypes.data))
    return out


def check_refine(opts, shape=None):
    """None, or {"radius": 1 .. 32, "eps": 1e-9 .. 1e3} with both keys optional (an empty dict: the defaults), normalised to
    None or a dict with both.  Raises InvalidOptionError on anything else, an unknown key or a value out of range; `shape` =
    (H, W) is the plane the options are meant for (a window may be larger than the plane: it is clipped)."""
    if opts is None:
        return None
    if not isinstance(opts, dict):
        raise InvalidOptionError("depth_refine", opts, "None, or a dict of radius and eps")
    unknown = sorted(str(k) for k in opts if k not in ("radius", "eps"))
    if unknown:
        raise InvalidOptionError("depth_refine", unknown[0], "the keys are radius and eps")
    radius, eps = opts.get("radius", REFINE_RADIUS), opts.get("eps", REFINE_EPS)
    if (isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or radius < 1 or radius > MAX_REFINE_RADIUS):
        raise InvalidOptionError("radius", radius, f"the refinement's window has an integer radius of 1 to {MAX_REFINE_RADIUS}")
    if not _number(eps) or eps < MIN_REFINE_EPS or eps > MAX_REFINE_EPS:
        raise InvalidOptionError("eps", eps, f"the refinement's regulariser is {MIN_REFINE_EPS:g} to {MAX_REFINE_EPS:g}")
    if shape is not None and (len(shape) < 2 or shape[0] < 1 or shape[1] < 1):
        raise InvalidOptionError("shape", shape, "the refinement takes an H x W plane")
    return {"radius": int(radius), "eps": float(eps)}


def _limits(lo, hi):
    if not _number(lo) or not _number(hi) or lo > hi:
        raise InvalidOptionError("lo", (lo, hi), "the clamp takes finite limits with lo <= hi")
    return float(lo), float(hi)


def guided_refine(depth, weight, guide, radius=REFINE_RADIUS, eps=REFINE_EPS, lo=None, hi=None, device=0):
    """The depth map `depth` refined against `guide` on the GPU (mi_depth_guided): the weighted guided filter of the module's
    docstring.  depth: H x W float32 (as depth_map(sigma) returns it; best the unsmoothed depth_map(0.0)); weight: H x W float32
    or float64, finite and >= 0; guide: H x W x 3 BGR uint8 or uint16 (the fused frame).  lo / hi default to the minimum and
    maximum of `depth`.  Returns H x W float32."""
    d, w, g = np.asarray(depth), np.asarray(weight), np.asarray(guide)
    if d.ndim != 2 or d.dtype != np.float32 or d.size == 0:
        raise InvalidOptionError("depth", (d.shape, d.dtype), "the depth map is an H x W float32 plane")
    if w.dtype not in (np.float32, np.float64) or w.shape != d.shape:
        raise InvalidOptionError("weight", (w.shape, w.dtype), f"the weight plane is float32 or float64 of the map's shape {d.shape}")
    if g.dtype not in (np.uint8, np.uint16) or g.shape != d.shape + (3,):
        raise InvalidOptionError("guide", (g.shape, g.dtype), f"the guide is a uint8 or uint16 BGR frame of {d.shape + (3,)}")
    o = check_refine({"radius": radius, "eps": eps}, d.shape)
    lo, hi = _limits(d.min() if lo is None else lo, d.max() if hi is None else hi)
    _lib.require_device()
    d, w, g = np.ascontiguousarray(d), np.ascontiguousarray(w), np.ascontiguousarray(g)
    out = np.empty(d.shape, np.float32)
    _lib.check(_lib.load().mi_depth_guided(int(device), d.ctypes.data, w.ctypes.data, _lib.MI_F64 if w.dtype == np.float64 else _lib.MI_F32,
                                           g.ctypes.data, _lib.DTYPE_CODE[g.dtype], d.shape[0], d.shape[1], o["radius"], o["eps"], lo, hi,
                                           out.ctypes.data))
    return out


def guided_refine_device(depth_ptr, weight_ptr, weight_dtype, guide_ptr, guide_dtype, height, width, out_ptr, lo, hi,
                         radius=REFINE_RADIUS, eps=REFINE_EPS, scratch_ptr=None, device=0, stream=None):
    """mi_depth_guided_device on planes resident in device memory: float32 depth and output, a weight of `weight_dtype`
    (float32 / float64), a guide of `guide_dtype` (uint8 / uint16).  With `scratch_ptr` (SCRATCH_PLANES * height * width
    float64, 16-byte aligned) the four launches are only queued on `stream`; without it a scratch buffer lives for the call,
    which then waits for the device before it frees it."""
    wt, gt = np.dtype(weight_dtype), np.dtype(guide_dtype)
    if wt not in (np.float32, np.float64):
        raise InvalidOptionError("weight_dtype", wt, "the weight plane is float32 or float64")
    if gt not in (np.uint8, np.uint16):
        raise InvalidOptionError("guide_dtype", gt, "the guide is uint8 or uint16")
    o = check_refine({"radius": radius, "eps": eps}, (height, width))
    lo, hi = _limits(lo, hi)
    own = None
    if scratch_ptr is None:
        own = _lib.DeviceBuffer(SCRATCH_PLANES * int(height) * int(width) * 8, device)
        scratch_ptr = own.ptr
    try:
        _lib.check(_lib.load().mi_depth_guided_device(int(device), stream, depth_ptr, weight_ptr,
                                                      _lib.MI_F64 if wt == np.float64 else _lib.MI_F32, guide_ptr, _lib.DTYPE_CODE[gt],
                                                      int(height), int(width), o["radius"], o["eps"], lo, hi, scratch_ptr, out_ptr))
        if own is not None:
            _lib.check(_lib.load().mi_device_synchronize(int(device)))
    finally:
        if own is not None:
            own.free()


def refined_from_host_guide(handle, sigma, dev_ptr, refine, fused, device=0):
    """handle.depth_map(sigma, refine=...) with a fused frame that lies in host memory: to the host directly, or -- the map
    going to `dev_ptr` -- through a device copy of the frame that lives for the call"""
    if dev_ptr is None:
        return handle.depth_map(sigma, None, refine, fused)
    g = np.ascontiguousarray(fused)
    buf = _lib.DeviceBuffer(g.nbytes, device)
    try:
        buf.upload(g)
        return handle.depth_map(sigma, dev_ptr, refine, (buf.ptr, g.dtype))     # (waits for the handle's stream)
    finally:
        buf.free()
