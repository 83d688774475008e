"""Raw Bayer mosaics in: black level, gains and the Malvar-He-Cutler demosaic on the MI355X (csrc/kernels_demosaic.hpp).

The reference reads developed frames (`cv2.imread`) and never sees a mosaic, so this has no reference counterpart.  A sensor
produces one colour sample per site -- 2 bytes per pixel at 16 bits where a BGR frame takes 6 -- and the one job this project
runs from host memory is bound by the host link: a raw stack pushed as mosaics (`Stack.push_mosaic`,
`PyramidStack.focus_stack_arrays(mosaic=)`, `pipeline.bunches_then_stack(mosaic=)`) crosses it at a third of the bytes and is
demosaiced on the device behind its upload.

The arithmetic is integer and exact, the same for uint8 and uint16 (tests/demosaic_restatement.py is its definition):

    step A, per site   v' = min(white, (max(v - black, 0) * gain_q + 2048) >> 12),   gain_q = round(gain * 4096) < 2^16
    step B             Malvar, He, Cutler (ICASSP 2004), the 5 x 5 linear kernels MATLAB's `demosaic` uses, coefficients times 2:
                       out = clamp((sum + 8) >> 4, 0, white), BORDER_REFLECT_101 on the mosaic, H x W x 3 BGR of the input dtype

There is no CPU path: without a GPU or the library `debayer` and its kin raise DeviceError.  `mosaic_of` is host NumPy.
"""
import math

import numpy as np

from . import _lib
from .errors import BitDepthError, InvalidOptionError

PATTERNS = ("RGGB", "BGGR", "GRBG", "GBRG")     # MI_CFA_*: the 2 x 2 cell at (y & 1, x & 1), row-major
TILE_H, TILE_W = 16, 128                        # demosaic::TILE_H / TILE_W of csrc/kernels_demosaic.hpp
GAIN_ONE = 4096                                 # gain_q of gain 1.0
_BGR = {"B": 0, "G": 1, "R": 2}


def _dtype(dtype):
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.uint8), np.dtype(np.uint16)):
        raise BitDepthError("uint8 or uint16", dt)
    return dt


def _four(name, value, kinds):
    """a scalar broadcast to the four cell positions, or four values"""
    if isinstance(value, kinds) and not isinstance(value, bool):
        return [value] * 4
    try:
        vals = list(value)
    except TypeError:
        vals = None
    if vals is None or len(vals) != 4 or not all(isinstance(v, kinds) and not isinstance(v, bool) for v in vals):
        raise InvalidOptionError(name, value, "one number, or four (one per position of the 2 x 2 cell, row-major)")
    return vals


class Cfa:
    """The colour filter array of a mosaic and the per-site corrections applied before interpolation.

    pattern  "RGGB", "BGGR", "GRBG" or "GBRG": the colours of the 2 x 2 cell at (y & 1, x & 1), row-major
    black    black level, one non-negative int or four (one per cell position)
    gains    one float or four in [0, 16): white balance and bit-depth scaling (a 12-bit sensor reaches 16 bits with gains
             near 16); quantised once, here, as round(gain * 4096)
    white    the output clamp; None: the dtype's maximum
    """

    def __init__(self, pattern="RGGB", black=0, gains=1.0, white=None):
        if not isinstance(pattern, str) or pattern.upper() not in PATTERNS:
            raise InvalidOptionError("pattern", pattern, "valid values are " + ", ".join(PATTERNS))
        self.pattern = pattern.upper()
        self.black = [int(b) for b in _four("black", black, (int, np.integer))]
        if min(self.black) < 0 or max(self.black) > 65535:
            raise InvalidOptionError("black", black, "black levels lie in [0, 65535]")
        self.gains = [float(g) for g in _four("gains", gains, (int, float, np.integer, np.floating))]
        if not all(math.isfinite(g) and 0.0 <= g < 16.0 for g in self.gains):
            raise InvalidOptionError("gains", gains, "gains lie in [0, 16)")
        self.gain_q = [int(math.floor(g * 4096.0 + 0.5)) for g in self.gains]
        if max(self.gain_q) > 65535:
            raise InvalidOptionError("gains", gains, "round(gain * 4096) must fit 16 bits")
        if white is not None:
            if isinstance(white, bool) or not isinstance(white, (int, np.integer)) or not 1 <= int(white) <= 65535:
                raise InvalidOptionError("white", white, "the white level is an int in [1, the dtype's maximum]")
            white = int(white)
        self.white = white

    def __repr__(self):
        return f"Cfa({self.pattern!r}, black={self.black}, gains={self.gains}, white={self.white})"

    def quantised(self, dtype=np.uint16):
        """the ints the kernel sees for mosaics of `dtype`: (pattern code, black[4], gain_q[4], white)"""
        maxv = int(np.iinfo(_dtype(dtype)).max)
        white = maxv if self.white is None else self.white
        if white > maxv:
            raise InvalidOptionError("white", white, f"exceeds the maximum {maxv} of {np.dtype(dtype)}")
        return PATTERNS.index(self.pattern), tuple(self.black), tuple(self.gain_q), white

    def struct(self, dtype):
        """mi_cfa_t for mosaics of `dtype`"""
        code, black, gain_q, white = self.quantised(dtype)
        return _lib.CfaStruct(code, (_lib.C.c_int32 * 4)(*black), (_lib.C.c_uint32 * 4)(*gain_q), white)


def _check_cfa(cfa):
    if not isinstance(cfa, Cfa):
        raise InvalidOptionError("cfa", cfa, "a shinestacker_amd.demosaic.Cfa is expected")
    return cfa


def check_mosaic(mosaic, shape=None, dtype=None):
    """an H x W uint8 / uint16 plane with H, W >= 2 (and of `shape`, `dtype` when given)"""
    a = np.asarray(mosaic)
    _dtype(a.dtype)
    if a.ndim != 2 or a.shape[0] < 2 or a.shape[1] < 2:
        raise InvalidOptionError("mosaic", a.shape, "a mosaic is an H x W plane with H, W >= 2")
    if shape is not None and a.shape != tuple(shape):
        raise InvalidOptionError("mosaic", a.shape, f"expected {tuple(shape)}")
    if dtype is not None and a.dtype != np.dtype(dtype):
        raise BitDepthError(np.dtype(dtype), a.dtype)
    return a


def mosaic_of(bgr, pattern="RGGB"):
    """Sample an H x W x 3 BGR frame down to its H x W mosaic (host NumPy: tests, tools, the example)."""
    bgr = np.asarray(bgr)
    if bgr.ndim != 3 or bgr.shape[2] != 3:
        raise InvalidOptionError("bgr", bgr.shape, "an H x W x 3 frame is expected")
    if not isinstance(pattern, str) or pattern.upper() not in PATTERNS:
        raise InvalidOptionError("pattern", pattern, "valid values are " + ", ".join(PATTERNS))
    pattern = pattern.upper()
    out = np.empty(bgr.shape[:2], bgr.dtype)
    for py in range(2):
        for px in range(2):
            out[py::2, px::2] = bgr[py::2, px::2, _BGR[pattern[2 * py + px]]]
    return out


def debayer_device(dev_mosaic, dev_bgr, h, w, dtype, cfa, device=0, stream=None):
    """debayer() for a mosaic resident in HBM: `dev_mosaic` (h x w) -> `dev_bgr` (h x w x 3).  Queued on `stream`, not waited for."""
    dt = _dtype(dtype)
    c = _check_cfa(cfa).struct(dt)
    if h < 2 or w < 2:
        raise InvalidOptionError("mosaic", (h, w), "a mosaic is an H x W plane with H, W >= 2")
    _lib.require_device()
    _lib.check(_lib.load().mi_demosaic_device(device, stream, dev_mosaic, dev_bgr, int(h), int(w), _lib.DTYPE_CODE[dt],
                                              _lib.C.byref(c)))


def debayer(mosaic, cfa, device=0):
    """H x W uint8 / uint16 mosaic -> H x W x 3 BGR array of the same dtype."""
    a = np.ascontiguousarray(check_mosaic(mosaic))
    c = _check_cfa(cfa).struct(a.dtype)
    _lib.require_device()
    out = np.empty(a.shape + (3,), a.dtype)
    _lib.check(_lib.load().mi_demosaic(device, a.ctypes.data, out.ctypes.data, a.shape[0], a.shape[1], _lib.DTYPE_CODE[a.dtype],
                                       _lib.C.byref(c)))
    return out


def debayer_frames_device(mosaics, dev_out, cfa, device=0):
    """Upload the n host mosaics (equal shape and dtype) and demosaic them side by side into `dev_out` (device pointer,
    n x H x W x 3 of their dtype): exactly what pipeline.align_and_stack_device(dev_frames, ...) takes.  Waits for the device."""
    _check_cfa(cfa)
    if len(mosaics) == 0:
        raise ValueError("no mosaics")
    first = check_mosaic(mosaics[0])
    h, w = first.shape
    frame_bytes = h * w * 3 * first.itemsize
    _lib.require_device()
    stage = _lib.DeviceBuffer(h * w * first.itemsize, device)
    try:
        for i, m in enumerate(mosaics):
            stage.upload(check_mosaic(m, first.shape, first.dtype))
            debayer_device(stage.ptr, dev_out + i * frame_bytes, h, w, first.dtype, cfa, device=device)
            # the stage is reused: the null stream's kernel must be through before the next (blocking) upload lands
            _lib.check(_lib.load().mi_device_synchronize(device))
    finally:
        stage.free()
