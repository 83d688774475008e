"""Post-stack denoise on the MI355X path (reference algorithms/denoise.py).

The reference calls `cv2.fastNlMeansDenoising(image, [h], None, template, search, norm)`: non-local means over the three
channels jointly, NORM_L2 for uint8 and NORM_L1 with `h * 256` for uint16.  Here the weight table is built on the host
(`weight_table`: one `exp` per entry, evaluated in long double and rounded once, so the table does not depend on the libm
or the NumPy build) and the filter runs in one HIP kernel (csrc/kernels_denoise.hpp) that is integer arithmetic
throughout.  There is no CPU path: without a GPU or the library every entry point raises DeviceError.

The table's rule is OpenCV's as remembered [from memory, unpinned -- see INTEGRATION.md, "Post-stack denoise"]:

    t = template // 2, n = (2t + 1)^2, shift = smallest p with 2^p >= n, fpm = min(max(IT) // (search^2 * max(T)), INT_MAX)
    entry a: dist = a * (2^shift / n);  w = exp(-dist / (h * h * 3)) [L2]  or  exp(-dist * dist / (h * h * 3)) [L1]
             (h * h * 3 in float32, as OpenCV's float h gives it);  weight = cvRound(fpm * w), 0 when weight < 0.001 * fpm

The weights fall monotonically, so only the entries before the first zero are kept and handed to the library.
"""
import numpy as np

from . import _lib
from .errors import BitDepthError, InvalidOptionError

MAX_TEMPLATE_WINDOW = 11
MAX_SEARCH_WINDOW = 21
_INT_MAX = 2**31 - 1
_CHUNK = 4096


def _dtype_rule(dtype):
    """(largest sample, largest value of the sum type IT, L1?) for a supported dtype"""
    dt = np.dtype(dtype)
    if dt == np.uint8:
        return 255, _INT_MAX, False
    if dt == np.uint16:
        return 65535, 2**63 - 1, True
    raise BitDepthError("uint8 or uint16", dt)


def window_half_sizes(template_window_size, search_window_size):
    """(t, s): OpenCV forces both windows odd, size = 2 * (size // 2) + 1"""
    tw, sw = int(template_window_size), int(search_window_size)
    if tw != template_window_size or sw != search_window_size:
        raise InvalidOptionError("window size", (template_window_size, search_window_size), "window sizes must be integral")
    if not (1 <= tw <= MAX_TEMPLATE_WINDOW and 1 <= sw <= MAX_SEARCH_WINDOW):
        raise InvalidOptionError("window size", (tw, sw), f"template window 1-{MAX_TEMPLATE_WINDOW} and search window "
                                 f"1-{MAX_SEARCH_WINDOW} are supported")
    return tw // 2, sw // 2


def weight_table(dtype, h, template_window_size=7, search_window_size=21):
    """(table, shift): the non-zero prefix of the weight table as uint32 and the shift that turns a patch distance into
    its index.  `h` is the value OpenCV receives (for uint16 already multiplied by 256)."""
    sample_max, it_max, l1 = _dtype_rule(dtype)
    t, s = window_half_sizes(template_window_size, search_window_size)
    n = (2 * t + 1) ** 2
    shift = (n - 1).bit_length()
    mult = float(1 << shift) / n
    fpm = min(it_max // ((2 * s + 1) ** 2 * sample_max), _INT_MAX)
    max_dist = sample_max * 3 if l1 else sample_max * sample_max * 3
    entries = int(max_dist / mult + 1)
    h32 = np.float32(h)
    den = np.longdouble(float(np.float32(h32 * h32) * np.float32(3)))
    parts = []
    for first in range(0, entries, _CHUNK):
        dist = (np.arange(first, min(first + _CHUNK, entries), dtype=np.float64) * mult).astype(np.longdouble)
        w = np.exp(-(dist * dist if l1 else dist) / den).astype(np.float64)
        weight = np.rint(fpm * w)
        weight[weight < 0.001 * fpm] = 0
        zero = np.flatnonzero(weight == 0)
        if zero.size:
            parts.append(weight[:zero[0]])
            break
        parts.append(weight)
    return np.ascontiguousarray(np.concatenate(parts), np.uint32), shift


def _h_for(dtype, h_luminance):
    if not h_luminance > 0:
        raise InvalidOptionError("h_luminance", h_luminance, "the filter strength must be positive")
    return h_luminance * 256 if np.dtype(dtype) == np.uint16 else h_luminance


def denoise_device(dev_src, dev_dst, height, width, dtype, h_luminance, template_window_size=7, search_window_size=21,
                   device=0, stream=None):
    """denoise() for a frame resident in HBM: `dev_src` -> `dev_dst` (distinct buffers).  Runs on `stream` and synchronises it."""
    dt = np.dtype(dtype)
    _dtype_rule(dt)
    table, shift = weight_table(dt, _h_for(dt, h_luminance), template_window_size, search_window_size)
    _lib.require_device()
    _lib.check(_lib.load().mi_nlm_denoise_device(device, dev_src, dev_dst, int(height), int(width), _lib.DTYPE_CODE[dt],
                                                 table.ctypes.data, int(table.size), int(shift), int(template_window_size),
                                                 int(search_window_size), stream))


def denoise(image, h_luminance, template_window_size=7, search_window_size=21, device=0):
    """The reference's denoise(): uint8 -> NORM_L2, uint16 -> NORM_L1 and h * 256.  H x W x 3 frames; returns a new array."""
    image = np.asarray(image)
    _dtype_rule(image.dtype)
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise InvalidOptionError("image", image.shape, "post-stack denoise takes H x W x 3 frames")
    table, shift = weight_table(image.dtype, _h_for(image.dtype, h_luminance), template_window_size, search_window_size)
    _lib.require_device()
    src = np.ascontiguousarray(image)
    out = np.empty_like(src)
    _lib.check(_lib.load().mi_nlm_denoise(device, src.ctypes.data, out.ctypes.data, src.shape[0], src.shape[1],
                                          _lib.DTYPE_CODE[src.dtype], table.ctypes.data, int(table.size), int(shift),
                                          int(template_window_size), int(search_window_size)))
    return out
