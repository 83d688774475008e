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
