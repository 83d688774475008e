"""Unsharp mask on the MI355X path (reference algorithms/sharpen.py).

The reference blurs with `cv2.GaussianBlur(image, (0, 0), radius)` and combines either with `cv2.addWeighted(image, 1 + amount,
blurred, -amount, 0)` (threshold == 0) or with its own NumPy lines (threshold != 0).  Here the window and the fixed-point taps
are built on the host (`window_size`, `gaussian_taps`) and one HIP kernel (csrc/kernels_unsharp.hpp) blurs and combines in a
single pass over the frame.  There is no CPU path: without a GPU or the library every entry point raises DeviceError.

The blur's rule is OpenCV's as remembered [from memory, unpinned -- see INTEGRATION.md, "Retouch filters"]:

    ksize = cvRound(radius * 6 + 1) | 1 [uint8]  or  cvRound(radius * 8 + 1) | 1 [uint16]     (cvRound: half to even)
    taps:  t_i = exp(x_i^2 * (-0.125 / sigma^2)), x_i = 2 i - (n - 1), normalised by 1 / sum in double, then quantised to
           8 [uint8] / 16 [uint16] fractional bits from the outside in, half to even, the rounding error carried to the next
           tap; the centre tap takes what is left so that the taps sum to exactly 1.0     (oracle/align_oracle.c states it in C)
"""
import math

import numpy as np

from . import _lib
from .errors import BitDepthError, InvalidOptionError

MAX_KSIZE = 33      # MI_UNSHARP_MAX_KSIZE: radius 4.0 on uint16


def _bits(dtype):
    """fractional bits of the taps for a supported dtype"""
    dt = np.dtype(dtype)
    if dt == np.uint8:
        return 8
    if dt == np.uint16:
        return 16
    raise BitDepthError("uint8 or uint16", dt)


def window_size(dtype, radius):
    """The window cv2.GaussianBlur derives from sigma = `radius` when it is given ksize (0, 0)"""
    bits = _bits(dtype)
    if not (isinstance(radius, (int, float, np.integer, np.floating)) and math.isfinite(radius) and radius > 0):
        raise InvalidOptionError("radius", radius, "the blur radius must be positive")
    ksize = round(float(radius) * (6 if bits == 8 else 8) + 1) | 1      # round(): half to even on the double, as cvRound
    if ksize > MAX_KSIZE:
        raise InvalidOptionError("radius", radius, f"its window of {ksize} taps exceeds the supported {MAX_KSIZE} "
                                 f"(radius 4.0 for both depths)")
    return ksize


def gaussian_taps(dtype, ksize, sigma):
    """`ksize` fixed-point taps of cv2's bit-exact Gaussian as uint32; they sum to 1 << bits"""
    bits = _bits(dtype)
    if ksize < 1 or not ksize & 1:
        raise InvalidOptionError("ksize", ksize, "the window must be odd")
    n2 = (ksize - 1) // 2
    scale2x = -0.125 / (sigma * sigma)
    t = [math.exp(float(x * x) * scale2x) for x in range(1 - ksize, 0, 2)]
    total = 0.0
    for v in t:
        total += v
    mul1 = 1.0 / (total * 2.0 + 1.0)
    fixed_1 = float(1 << bits)
    taps = np.zeros(ksize, np.uint32)
    acc, carry = 0, 0.0
    for i in range(n2):
        adj = t[i] * mul1 * fixed_1 + carry
        v = round(adj)
        carry = adj - v
        taps[i] = taps[ksize - 1 - i] = v
        acc += 2 * v
    taps[n2] = (1 << bits) - acc
    return taps


def _prepare(dtype, radius, amount, threshold):
    """(taps, ksize, amount, threshold in sample units) after every check that needs no device"""
    dt = np.dtype(dtype)
    ksize = window_size(dt, radius)
    for name, v in (("amount", amount), ("threshold", threshold)):
        if not (isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)):
            raise InvalidOptionError(name, v, "must be a finite number")
    threshold = float(threshold) * 256 if dt == np.uint16 else float(threshold)
    return gaussian_taps(dt, ksize, float(radius)), ksize, float(amount), threshold


def check_options(radius, amount, threshold):
    """Raise for arguments no frame of either depth could take (the pipeline calls this before it stacks)"""
    _prepare(np.uint8, radius, amount, threshold)


def unsharp_mask_device(dev_src, dev_dst, height, width, dtype, radius=1.0, amount=1.0, threshold=0.0, device=0, stream=None):
    """unsharp_mask() for a frame resident in HBM: `dev_src` -> `dev_dst` (distinct buffers).  Queued on `stream`, not waited for."""
    dt = np.dtype(dtype)
    taps, ksize, amount, threshold = _prepare(dt, radius, amount, threshold)
    if height < 1 or width < 1:
        raise InvalidOptionError("image", (height, width), "the unsharp mask takes H x W x 3 frames")
    _lib.require_device()
    _lib.check(_lib.load().mi_unsharp_mask_device(device, stream, dev_src, dev_dst, int(height), int(width), _lib.DTYPE_CODE[dt],
                                                  taps.ctypes.data, ksize, amount, threshold))


def unsharp_mask(image, radius=1.0, amount=1.0, threshold=0.0, device=0):
    """The reference's unsharp_mask() for H x W x 3 uint8 / uint16 frames; returns a new array."""
    image = np.asarray(image)
    _bits(image.dtype)
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise InvalidOptionError("image", image.shape, "the unsharp mask takes H x W x 3 frames")
    taps, ksize, amount, threshold = _prepare(image.dtype, radius, amount, threshold)
    _lib.require_device()
    src = np.ascontiguousarray(image)
    out = np.empty_like(src)
    _lib.check(_lib.load().mi_unsharp_mask(device, src.ctypes.data, out.ctypes.data, src.shape[0], src.shape[1],
                                           _lib.DTYPE_CODE[src.dtype], taps.ctypes.data, ksize, amount, threshold))
    return out
