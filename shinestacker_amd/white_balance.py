"""White balance from a picked RGB value on the MI355X path (reference algorithms/white_balance.py).

The reference scales every channel in float64 by target_gray / target_channel (1.0 for a zero channel), clips to the dtype's
range and truncates.  That is a function of (channel, value), so `white_balance_table` evaluates the reference's own
expression once per value -- the same NumPy operations, in the same order, over arange(nbins) -- and the frame passes through
the per-channel look-up kernel the balance step already uses (`mi_apply_lut`).  The result is the reference's by
construction: no new kernel, no FP64 on the device.  There is no CPU path: without a GPU or the library the entry points
raise DeviceError.
"""
import math

import numpy as np

from . import _lib
from .errors import BitDepthError, InvalidOptionError


def _nbins(dtype):
    dt = np.dtype(dtype)
    if dt == np.uint8:
        return 256
    if dt == np.uint16:
        return 65536
    raise BitDepthError("uint8 or uint16", dt)


def white_balance_table(dtype, target_rgb):
    """(3, nbins) table of `dtype`, row c for channel c of a BGR frame: the reference's arithmetic on every possible value"""
    dt = np.dtype(dtype)
    nbins = _nbins(dt)
    try:
        rgb = tuple(target_rgb)
        ok = len(rgb) == 3 and all(isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v) for v in rgb)
    except TypeError:
        ok = False
    if not ok:
        raise InvalidOptionError("target_rgb", target_rgb, "three finite numbers (R, G, B)")
    # white_balance.py:6-14, on arange(nbins) in place of the frame
    img_float = np.repeat(np.arange(nbins, dtype=dt)[:, None], 3, axis=1).astype(np.float64)
    target_bgr = (rgb[2], rgb[1], rgb[0])
    target_gray = sum(target_bgr) / 3.0
    scales = [target_gray / val if val != 0 else 1.0 for val in target_bgr]
    for c in range(3):
        img_float[..., c] *= scales[c]
    max_val = np.iinfo(dt).max
    img_float = np.clip(img_float, 0, max_val)
    return np.ascontiguousarray(img_float.astype(dt).T)


def white_balance_device(dev_src, dev_dst, npixels, dtype, target_rgb, device=0, stream=None):
    """white_balance_from_rgb() for a frame resident in HBM: `dev_src` -> `dev_dst` (may be the same buffer).  Runs on `stream`
    and waits for the device: the table's device copy is freed before the return."""
    dt = np.dtype(dtype)
    table = white_balance_table(dt, target_rgb)
    _lib.require_device()
    lut = _lib.DeviceBuffer(table.nbytes, device)
    try:
        lut.upload(table)
        _lib.check(_lib.load().mi_apply_lut_device(device, stream, dev_src, dev_dst, int(npixels), _lib.DTYPE_CODE[dt], lut.ptr, 3))
        _lib.check(_lib.load().mi_device_synchronize(device))
    finally:
        lut.free()


def white_balance_from_rgb(img, target_rgb, device=0):
    """The reference's white_balance_from_rgb() for H x W x 3 uint8 / uint16 BGR frames; returns a new array."""
    img = np.asarray(img)
    _nbins(img.dtype)
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise InvalidOptionError("image", img.shape, "white balance takes H x W x 3 frames")
    table = white_balance_table(img.dtype, target_rgb)
    _lib.require_device()
    return _lib.apply_lut(img, table, device)
