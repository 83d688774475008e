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

Raw development around it, `Develop`, each step optional and as exact (tests/develop_restatement.py is the definition):

    step 0, defect sites   on the raw samples, ahead of step A: a listed site becomes (S + (k >> 1)) // k over its k valid
                           neighbours (y -+ 2, x), (y, x -+ 2) -- same colour, black level and gain; valid: inside the image and
                           not itself listed; k = 0 leaves the site
    step C, colour matrix  on step B's output: M_q = round(M * 4096), rows and columns in R, G, B order,
                           out_i = clamp((sum_j M_q[i][j] * in_j + 2048) >> 12, 0, white); per row sum_j |M_q[i][j]| <= 32767
    step D, tone curve     out = tone[out], a table of maxv + 1 entries of the frame's dtype (`srgb_tone`, `gamma_tone`)

Calibration frames ahead of all of it, `Calibration`, as exact (csrc/kernels_calib.hpp; tests/calib_restatement.py is the
definition); pos = 2 (y & 1) + (x & 1), nothing here depends on the colour pattern:

    master frame           K <= 32 exposures, per site sorted s[0..K-1]: out = (S + (n >> 1)) // n over s[reject .. K - reject - 1],
                           n = K - 2 reject -- the rounded mean (reject 0), the median ((K - 1) // 2), min/max rejection between
    flat gain table        f = max(F - B, 0), B the flat-dark or black[pos]; per position the sum S_p and count N_p of f;
                           G_q = 16384 where f == 0 or S_p == 0, else min(65535, (2 * 16384 * S_p + N_p * f) // (2 * N_p * f)), uint16
    calibrate              in place on the raw samples, ahead of step 0: e = max(v - (dark or black[pos]), 0),
                           e' = (e * G_q + 8192) >> 14 with a flat, out = min(maxv, e' + black[pos])

Linear raw frames, `Linear` and `develop_linear[_device]` (csrc/kernels_linear.hpp; tests/linear_restatement.py is the
definition): an already demosaiced frame -- a DNG's LinearRaw IFD -- needs no step B.  H x W x 3 samples in R, G, B order (or
H x W: one grey sample per pixel) become H x W x 3 BGR in one pass:

    step A, per sample     v' = min(white, (max(v - black[c], 0) * gain_q[c] + 2048) >> 12), c the channel; spp 1: b = g = r = v'
    steps C and D          `Develop`'s colour matrix and tone curve, as above; lens and finish run behind it as behind `debayer`

There is no CPU path: without a GPU or the library `debayer` and its kin raise DeviceError.  `mosaic_of`, `srgb_tone`,
`gamma_tone` and `defects_from_dark` are host NumPy.
"""
import math

import numpy as np

from . import _lib
from .errors import BitDepthError, InvalidOptionError

PATTERNS = ("RGGB", "BGGR", "GRBG", "GBRG")     # MI_CFA_*: the 2 x 2 cell at (y & 1, x & 1), row-major
TILE_H, TILE_W = 16, 128                        # demosaic::TILE_H / TILE_W of csrc/kernels_demosaic.hpp
GAIN_ONE = 4096                                 # gain_q of gain 1.0
CALIB_VEC_BYTES = 16                            # calib::VEC_BYTES of csrc/kernels_calib.hpp: one lane's window of a row
CALIB_TILE_H, CALIB_LANES = 4, 64               # calib::TILE_H / LANES: a workgroup is 4 rows of 64 windows
CALIB_MAX_FRAMES = 32                           # calib::MAX_FRAMES: exposures of one master
FLAT_GAIN_ONE = 16384                           # calib::GAIN_ONE: Q14


def calib_vec(dtype):
    """the calibration kernel's vector width in sites for mosaics of `dtype`"""
    return CALIB_VEC_BYTES // _dtype(dtype).itemsize


def calib_tile(dtype):
    """(rows, sites of a row) of one workgroup of the calibration kernel, for rows that start on a 16-byte boundary"""
    return CALIB_TILE_H, CALIB_LANES * calib_vec(dtype)
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


MATRIX_ONE = 4096                               # M_q of 1.0
MATRIX_ROW_BOUND = 32767                        # per row, sum |M_q|: the kernel's int32 accumulator holds


def _tone_from(f, dtype, white):
    dt = _dtype(dtype)
    maxv = int(np.iinfo(dt).max)
    if white is None:
        white = maxv
    if isinstance(white, bool) or not isinstance(white, (int, np.integer)) or not 1 <= int(white) <= maxv:
        raise InvalidOptionError("white", white, f"the white level is an int in [1, {maxv}]")
    x = np.minimum(np.arange(maxv + 1, dtype=np.float64), float(white)) / float(white)
    return np.floor(maxv * f(x) + 0.5).astype(dt)


def srgb_tone(dtype, white=None):
    """The sRGB transfer curve as a tone table of `dtype`: round(maxv * srgb(i / white)), i > white as white (float64 NumPy)."""
    return _tone_from(lambda x: np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055), dtype, white)


def gamma_tone(dtype, gamma, white=None):
    """A pure power law as a tone table of `dtype`: round(maxv * (i / white) ** (1 / gamma)), i > white as white."""
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)) or not math.isfinite(gamma) or gamma <= 0:
        raise InvalidOptionError("gamma", gamma, "a positive finite number is expected")
    return _tone_from(lambda x: np.power(x, 1.0 / float(gamma)), dtype, white)


def defects_from_dark(dark_mosaic, threshold):
    """The sites of a dark frame (an H x W mosaic taken with the shutter closed) above `threshold`, as an (n, 2) array of
    (y, x) in ascending order: what Develop(defects=) takes.  Host NumPy.  (`master_frame` reduces several dark exposures
    to the one frame this takes.)"""
    a = check_mosaic(dark_mosaic)
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not math.isfinite(threshold):
        raise InvalidOptionError("threshold", threshold, "a finite number is expected")
    return np.argwhere(a > threshold).astype(np.int32)


class Develop:
    """Raw development around the demosaic: defect sites before it, colour matrix and tone curve behind it.

    matrix   3 x 3 floats, output = matrix @ (R, G, B) of the camera; quantised once, here, as round(m * 4096); the sum of
             |quantised entries| of a row is at most 32767 (a little under 8.0)
    tone     a table of 256 uint8 / 65536 uint16 entries, or "srgb", or a float gamma (`srgb_tone`, `gamma_tone` over the
             dtype's full range, resolved per dtype at first use)
    defects  an (n, 2) int array of (y, x), or a boolean H x W mask; sorted, made unique and checked against the frame at
             first use

    The tone table and the site list are uploaded per device (and dtype, frame shape) at first use and held until close().
    Kernels queued by a Stack read them: the Stack keeps the object until finish / reset / sync / close, and close() here
    must not come before that."""

    def __init__(self, matrix=None, tone=None, defects=None):
        self.matrix = self.matrix_q = None
        if matrix is not None:
            try:
                m = np.array(matrix, dtype=np.float64)
            except (TypeError, ValueError):
                m = None
            if m is None or m.shape != (3, 3) or not np.isfinite(m).all():
                raise InvalidOptionError("matrix", matrix, "3 x 3 finite numbers are expected")
            q = np.floor(m * float(MATRIX_ONE) + 0.5)
            if (np.abs(q).sum(axis=1) > MATRIX_ROW_BOUND).any():
                raise InvalidOptionError("matrix", matrix, f"per row, the sum of |round(m * 4096)| must be <= {MATRIX_ROW_BOUND}")
            self.matrix, self.matrix_q = m, tuple(int(v) for v in q.reshape(9))
        self.tone = None
        if tone is not None:
            if isinstance(tone, str):
                if tone.lower() != "srgb":
                    raise InvalidOptionError("tone", tone, 'a table, "srgb" or a float gamma is expected')
                self.tone = "srgb"
            elif isinstance(tone, (int, float, np.integer, np.floating)) and not isinstance(tone, bool):
                gamma_tone(np.uint8, tone)      # (validates the gamma)
                self.tone = float(tone)
            else:
                t = np.asarray(tone)
                _dtype(t.dtype)
                if t.ndim != 1 or t.shape[0] != int(np.iinfo(t.dtype).max) + 1:
                    raise InvalidOptionError("tone", t.shape, f"a {t.dtype} table has {int(np.iinfo(t.dtype).max) + 1} entries")
                self.tone = np.ascontiguousarray(t).copy()
        self.defects = None
        if defects is not None:
            d = np.asarray(defects)
            if d.dtype == np.bool_ and d.ndim == 2:
                self.defects = d.copy()
            elif d.ndim == 2 and d.shape[1] == 2 and (d.dtype.kind in "iu" or d.size == 0):
                self.defects = d.astype(np.int64)
            else:
                raise InvalidOptionError("defects", d.shape, "an (n, 2) int array of (y, x) or a boolean H x W mask is expected")
        self._tones = {}        # dtype -> host table
        self._sites = {}        # (h, w) -> host int32 list
        self._dev = {}          # (device, "tone", dtype) / (device, "sites", h, w) -> _lib.DeviceBuffer

    def __repr__(self):
        tone = self.tone if not isinstance(self.tone, np.ndarray) else f"<{self.tone.dtype} table>"
        n = None if self.defects is None else (int(self.defects.sum()) if self.defects.dtype == np.bool_ else len(self.defects))
        return f"Develop(matrix={None if self.matrix is None else self.matrix.tolist()}, tone={tone}, defects={n})"

    def tone_table(self, dtype):
        """the host tone table for frames of `dtype`, or None"""
        dt = _dtype(dtype)
        if self.tone is None:
            return None
        if isinstance(self.tone, np.ndarray):
            if self.tone.dtype != dt:
                raise BitDepthError(dt, self.tone.dtype)
            return self.tone
        if dt not in self._tones:
            self._tones[dt] = srgb_tone(dt) if self.tone == "srgb" else gamma_tone(dt, self.tone)
        return self._tones[dt]

    def sites(self, shape):
        """the defect sites of an H x W frame as linear indices y * W + x: int32, ascending, unique (empty without defects)"""
        h, w = int(shape[0]), int(shape[1])
        if (h, w) not in self._sites:
            if self.defects is None:
                s = np.zeros(0, np.int64)
            elif self.defects.dtype == np.bool_:
                if self.defects.shape != (h, w):
                    raise InvalidOptionError("defects", self.defects.shape, f"the mask of a {h} x {w} frame has its shape")
                s = np.flatnonzero(self.defects)
            else:
                y, x = self.defects[:, 0], self.defects[:, 1]
                if len(y) and (y.min() < 0 or y.max() >= h or x.min() < 0 or x.max() >= w):
                    raise InvalidOptionError("defects", (int(y.max()), int(x.max())), f"a site lies outside the {h} x {w} frame")
                s = np.unique(y * w + x)
            if h * w >= 2 ** 31:
                raise InvalidOptionError("defects", (h, w), "height x width must be below 2^31")
            self._sites[(h, w)] = s.astype(np.int32)
        return self._sites[(h, w)]

    def host_args(self, shape, dtype):
        """(matrix_q as int32[9] or None, tone table or None, sites): what the host form mi_develop takes"""
        mq = None if self.matrix_q is None else (_lib.C.c_int32 * 9)(*self.matrix_q)
        return mq, self.tone_table(dtype), self.sites(shape)

    def prepared(self, shape, dtype, device=0):
        """(mi_develop_t, device pointer of the sites or None, their number) for H x W frames of `dtype` on `device`; uploads
        the tone table and the site list on first use"""
        dt = _dtype(dtype)
        d = _lib.DevelopStruct()
        if self.matrix_q is not None:
            d.flags |= _lib.MI_DEVELOP_MATRIX
            d.matrix_q = (_lib.C.c_int32 * 9)(*self.matrix_q)
        tone = self.tone_table(dt)
        sites = self.sites(shape)
        if tone is not None:
            d.flags |= _lib.MI_DEVELOP_TONE
            d.dev_tone = self._resident((device, "tone", dt), tone).ptr
        ptr = self._resident((device, "sites", int(shape[0]), int(shape[1])), sites).ptr if len(sites) else None
        return d, ptr, len(sites)

    def _resident(self, key, arr):
        if key not in self._dev:
            _lib.require_device()
            buf = _lib.DeviceBuffer(arr.nbytes, key[0])
            buf.upload(arr)
            self._dev[key] = buf
        return self._dev[key]

    def close(self):
        """free the device tables (not before every kernel queued with them has run: Stack.finish / sync / reset / close)"""
        for buf in self._dev.values():
            buf.free()
        self._dev = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_develop(develop):
    if not isinstance(develop, Develop):
        raise InvalidOptionError("develop", develop, "a shinestacker_amd.demosaic.Develop is expected")
    return develop


def require_mosaic(mosaic, develop, calibration=None):
    """`develop=` and `calibration=` only mean something beside `mosaic=`"""
    if develop is not None:
        if mosaic is None:
            raise InvalidOptionError("develop", develop, "develop= needs mosaic=: only raw mosaics are developed")
        check_develop(develop)
    if calibration is not None:
        if mosaic is None:
            raise InvalidOptionError("calibration", calibration, "calibration= needs mosaic=: only raw mosaics are calibrated")
        check_calibration(calibration)


# ---------------------------------------------------------------- calibration frames: master dark, flat field
def _resolve_reject(reject, k):
    """the number of samples dropped at each end of a site's k sorted samples"""
    if isinstance(reject, str):
        if reject.lower() == "mean":
            return 0
        if reject.lower() == "median":
            return (k - 1) // 2
    elif isinstance(reject, (int, np.integer)) and not isinstance(reject, bool):
        if reject < 0 or 2 * int(reject) >= k:
            raise InvalidOptionError("reject", reject, f"0 <= reject and 2 * reject < {k}, the number of frames")
        return int(reject)
    raise InvalidOptionError("reject", reject, '"mean", "median" or an int is expected')


def _exposures(name, frames):
    """K mosaics of one shape and dtype, 1 <= K <= 32, as a list of contiguous arrays"""
    if isinstance(frames, np.ndarray):
        if frames.ndim != 3:
            raise InvalidOptionError(name, frames.shape, "K mosaics (K x H x W, or a sequence of H x W planes) are expected")
        frames = list(frames)
    try:
        frames = list(frames)
    except TypeError:
        raise InvalidOptionError(name, frames, "a sequence of H x W mosaics is expected") from None
    if not 1 <= len(frames) <= CALIB_MAX_FRAMES:
        raise InvalidOptionError(name, len(frames), f"1 to {CALIB_MAX_FRAMES} frames are expected")
    first = check_mosaic(frames[0])
    return [np.ascontiguousarray(check_mosaic(f, first.shape, first.dtype)) for f in frames]


def master_frame(mosaics, reject="median", device=0):
    """K <= 32 exposures (H x W mosaics of one shape and dtype) reduced to their master, H x W of that dtype: per site the
    samples sorted, `reject` dropped at each end and the rest averaged, rounded.  reject: "mean" (0), "median" ((K - 1) // 2) or
    an int with 2 * reject < K -- min/max rejection, which removes a cosmic-ray hit or a passing insect."""
    frames = _exposures("mosaics", mosaics)
    r = _resolve_reject(reject, len(frames))
    _lib.require_device()
    h, w = frames[0].shape
    out = np.empty((h, w), frames[0].dtype)
    ptrs = (_lib.C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
    _lib.check(_lib.load().mi_mosaic_master(device, ptrs, len(frames), h, w, _lib.DTYPE_CODE[out.dtype], r, out.ctypes.data))
    return out


def flat_gain(flat, cfa, flat_dark=None, device=0):
    """The Q14 gain table of a master flat, uint16 H x W: per cell position the mean of max(flat - B, 0) over the site's value,
    B the `flat_dark` (a master dark at the flat's exposure) or the Cfa's black level.  Normalised per position: the flat does
    not change the white balance."""
    f = np.ascontiguousarray(check_mosaic(flat))
    c = _check_cfa(cfa).struct(f.dtype)
    fd = None if flat_dark is None else np.ascontiguousarray(check_mosaic(flat_dark, f.shape, f.dtype))
    if f.shape[0] * f.shape[1] >= 2 ** 31:
        raise InvalidOptionError("flat", f.shape, "height x width must be below 2^31")
    _lib.require_device()
    out = np.empty(f.shape, np.uint16)
    _lib.check(_lib.load().mi_flat_gain(device, f.ctypes.data, None if fd is None else fd.ctypes.data, f.shape[0], f.shape[1],
                                        _lib.DTYPE_CODE[f.dtype], _lib.C.byref(c), out.ctypes.data))
    return out


class Calibration:
    """Calibration frames of a raw workflow: (raw - dark) * flat_gain per site, before anything else touches the samples.

    dark       the sensor's fixed pattern at the exposure of the frames: one master H x W mosaic, or a sequence (or K x H x W
               array) of up to 32 exposures reduced with `master_frame` at first use
    flat       an evenly lit frame: vignetting, dust shadows, per-site gain.  As `dark`.
    flat_dark  a dark at the flat's exposure, subtracted from the flat; None: the Cfa's black level.  As `dark`.
    reject     how exposures are reduced: "mean", "median" or an int (`master_frame`)

    The gain table is built at first use against the Cfa it is used with (its black levels).  Masters and table are uploaded
    per device at first use and held until close().  Kernels queued by a Stack read them: the Stack keeps the object until
    finish / reset / sync / close, and close() here must not come before that."""

    def __init__(self, dark=None, flat=None, flat_dark=None, reject="median"):
        _resolve_reject(reject, 2 * CALIB_MAX_FRAMES + 1)     # (the kind of value; against K once the frames are counted)
        self.reject = reject
        self._given = {}
        self.shape = self.dtype = None
        for name, v in (("dark", dark), ("flat", flat), ("flat_dark", flat_dark)):
            if v is None:
                continue
            if isinstance(v, np.ndarray) and v.ndim == 2:
                first = np.ascontiguousarray(check_mosaic(v)).copy()
                self._given[name] = first
            else:
                frames = _exposures(name, v)
                _resolve_reject(reject, len(frames))
                first = frames[0]
                self._given[name] = frames
            if self.shape is None:
                self.shape, self.dtype = first.shape, first.dtype
            elif first.shape != self.shape:
                raise InvalidOptionError(name, first.shape, f"the calibration frames have one shape (so far {self.shape})")
            elif first.dtype != self.dtype:
                raise BitDepthError(self.dtype, first.dtype)
        if flat_dark is not None and flat is None:
            raise InvalidOptionError("flat_dark", "given", "flat_dark= needs flat=")
        self._gains = {}        # the Cfa's black levels -> host gain table
        self._dev = {}          # (device, "dark") / (device, "gain", black) -> _lib.DeviceBuffer

    def __repr__(self):
        def kind(v):
            return None if v is None else "master" if isinstance(v, np.ndarray) else f"{len(v)} frames"
        return (f"Calibration(dark={kind(self._given.get('dark'))}, flat={kind(self._given.get('flat'))}, "
                f"flat_dark={kind(self._given.get('flat_dark'))}, reject={self.reject!r})")

    def master(self, name):
        """the master "dark", "flat" or "flat_dark" (reduced at first use), or None"""
        v = self._given.get(name)
        if v is not None and not isinstance(v, np.ndarray):
            v = self._given[name] = master_frame(v, self.reject)
        return v

    def check_frame(self, shape, dtype):
        """the calibration frames are those of H x W mosaics of `dtype`"""
        dt = _dtype(dtype)
        if self.shape is not None:
            if tuple(shape) != tuple(self.shape):
                raise InvalidOptionError("calibration", self.shape, f"the calibration frames of a {tuple(shape)} mosaic have its shape")
            if dt != self.dtype:
                raise BitDepthError(dt, self.dtype)

    def gain_table(self, cfa):
        """the uint16 Q14 gain table against `cfa` (built at first use), or None without a flat"""
        if "flat" not in self._given:
            return None
        key = tuple(_check_cfa(cfa).black)
        if key not in self._gains:
            self._gains[key] = flat_gain(self.master("flat"), cfa, self.master("flat_dark"))
        return self._gains[key]

    def host_tables(self, shape, dtype, cfa):
        """(master dark or None, gain table or None) for H x W mosaics of `dtype`: what the host form mi_mosaic_calibrate takes"""
        _check_cfa(cfa)
        self.check_frame(shape, dtype)
        return self.master("dark"), self.gain_table(cfa)

    def prepared(self, shape, dtype, cfa, device=0):
        """mi_calib_t for H x W mosaics of `dtype` on `device`; reduces, builds and uploads the tables on first use"""
        dark, gain = self.host_tables(shape, dtype, cfa)
        c = _lib.CalibStruct()
        if dark is not None:
            c.flags |= _lib.MI_CALIB_DARK
            c.dev_dark = self._resident((device, "dark"), dark).ptr
        if gain is not None:
            c.flags |= _lib.MI_CALIB_FLAT
            c.dev_gain = self._resident((device, "gain", tuple(cfa.black)), gain).ptr
        return c

    def _resident(self, key, arr):
        if key not in self._dev:
            _lib.require_device()
            buf = _lib.DeviceBuffer(arr.nbytes, key[0])
            buf.upload(arr)
            self._dev[key] = buf
        return self._dev[key]

    def close(self):
        """free the device tables (not before every kernel queued with them has run: Stack.finish / sync / reset / close)"""
        for buf in self._dev.values():
            buf.free()
        self._dev = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def check_calibration(calibration):
    if not isinstance(calibration, Calibration):
        raise InvalidOptionError("calibration", calibration, "a shinestacker_amd.demosaic.Calibration is expected")
    return calibration


def calibrate_device(dev_mosaic, h, w, dtype, cfa, calibration, device=0, stream=None):
    """calibrate() in place on a mosaic resident in HBM.  Queued on `stream`, not waited for; the Calibration's device tables
    must outlive the queued kernel."""
    dt = _dtype(dtype)
    c = _check_cfa(cfa).struct(dt)
    cal = check_calibration(calibration).prepared((h, w), dt, cfa, device)
    _lib.check(_lib.load().mi_mosaic_calibrate_device(device, stream, dev_mosaic, int(h), int(w), _lib.DTYPE_CODE[dt], _lib.C.byref(c),
                                                      _lib.C.byref(cal)))


def calibrate(mosaic, cfa, calibration, device=0):
    """(mosaic - dark) * flat_gain per site with the black pedestal put back: an H x W mosaic of the same dtype, an ordinary
    mosaic for everything downstream."""
    a = np.ascontiguousarray(check_mosaic(mosaic))
    c = _check_cfa(cfa).struct(a.dtype)
    check_calibration(calibration).check_frame(a.shape, a.dtype)
    _lib.require_device()
    dark, gain = calibration.host_tables(a.shape, a.dtype, cfa)
    out = np.empty_like(a)
    _lib.check(_lib.load().mi_mosaic_calibrate(device, a.ctypes.data, out.ctypes.data, a.shape[0], a.shape[1], _lib.DTYPE_CODE[a.dtype],
                                               _lib.C.byref(c), None if dark is None else dark.ctypes.data,
                                               None if gain is None else gain.ctypes.data))
    return out


def correct_sites_device(dev_mosaic, h, w, dtype, cfa, corrections, device=0, stream=None):
    """correct_sites() in place on a mosaic resident in HBM.  Queued on `stream`, not waited for; the SiteCorrections' device
    tables must outlive the queued kernels."""
    from .dng import check_corrections
    dt = _dtype(dtype)
    c = _check_cfa(cfa).struct(dt)
    _check_site_black(cfa, check_corrections(corrections).quantised((h, w), dt), dt)
    sc = corrections.prepared((h, w), dt, device)
    _lib.check(_lib.load().mi_mosaic_site_correct_device(device, stream, dev_mosaic, int(h), int(w), _lib.DTYPE_CODE[dt], _lib.C.byref(c),
                                                         _lib.C.byref(sc)))


def _check_site_black(cfa, q, dt):
    """black[pos] + black_h[x] + black_v[y] stays inside [0, maxv]: what the kernel is promised"""
    maxv = int(np.iinfo(dt).max)
    for pos in range(4):
        lo = hi = cfa.black[pos]
        for d, sl in ((q.dh, slice(pos & 1, None, 2)), (q.dv, slice(pos >> 1, None, 2))):
            if d is not None:
                lo, hi = lo + int(d[sl].min()), hi + int(d[sl].max())
        if lo < 0 or hi > maxv:
            raise InvalidOptionError("corrections", (lo, hi), f"black level plus deltas leaves [0, {maxv}] at position {pos}")


def correct_sites(mosaic, cfa, corrections, device=0):
    """The site corrections of a raw frame (dng.SiteCorrections: bad sites, black deltas, gain maps) applied to an H x W
    mosaic: a mosaic of the same dtype with the black pedestal in place, an ordinary mosaic for everything downstream."""
    from .dng import check_corrections
    a = np.ascontiguousarray(check_mosaic(mosaic))
    c = _check_cfa(cfa).struct(a.dtype)
    q = check_corrections(corrections).quantised(a.shape, a.dtype)
    _check_site_black(cfa, q, a.dtype)
    _lib.require_device()
    sc = q.host_struct()
    out = np.empty_like(a)
    _lib.check(_lib.load().mi_mosaic_site_correct(device, a.ctypes.data, out.ctypes.data, a.shape[0], a.shape[1], _lib.DTYPE_CODE[a.dtype],
                                                  _lib.C.byref(c), _lib.C.byref(sc)))
    return out


def _check_radial(gain, cfa, dt):
    from .dng import RadialGain
    if not isinstance(gain, RadialGain):
        raise InvalidOptionError("vignette", gain, "a shinestacker_amd.dng.RadialGain is expected")
    maxv = int(np.iinfo(dt).max)
    if max(_check_cfa(cfa).black) > maxv:
        raise InvalidOptionError("cfa", tuple(cfa.black), f"a black level exceeds the maximum of {dt}")
    return gain


def radial_gain_device(dev_mosaic, h, w, dtype, cfa, gain, device=0, stream=None, lens=None):
    """radial_gain() in place on a mosaic resident in HBM.  Queued on `stream`, not waited for; the RadialGain's device table
    must outlive the queued kernel.  `lens`: the lens.Lens applied to the developed frame later, or None (dng.RadialGain)."""
    dt = _dtype(dtype)
    if h < 2 or w < 2:
        raise InvalidOptionError("mosaic", (h, w), "a mosaic is an H x W plane with H, W >= 2")
    c = _check_cfa(cfa).struct(dt)
    rg = _check_radial(gain, cfa, dt).prepared((h, w), device, lens)
    _lib.check(_lib.load().mi_mosaic_radial_gain_device(device, stream, dev_mosaic, int(h), int(w), _lib.DTYPE_CODE[dt], _lib.C.byref(c),
                                                        _lib.C.byref(rg)))


def radial_gain(mosaic, cfa, gain, device=0, lens=None):
    """A dng.RadialGain (a DNG's FixVignetteRadial) applied to an H x W mosaic: (v - black) * g(r^2) with the black pedestal
    put back, a mosaic of the same dtype (csrc/kernels_finish.hpp; integer and exact: tests/finish_restatement.py)."""
    a = np.ascontiguousarray(check_mosaic(mosaic))
    c = _check_cfa(cfa).struct(a.dtype)
    rg, _table = _check_radial(gain, cfa, a.dtype).struct(a.shape, lens)
    _lib.require_device()
    out = np.empty_like(a)
    _lib.check(_lib.load().mi_mosaic_radial_gain(device, a.ctypes.data, out.ctypes.data, a.shape[0], a.shape[1], _lib.DTYPE_CODE[a.dtype],
                                                 _lib.C.byref(c), _lib.C.byref(rg)))
    return out


def _check_finish_frame(shape, dtype, finish):
    """(dtype, (y, x, h, w), orientation) of dng.Finish `finish` on an H x W x 3 frame"""
    from .dng import check_finish
    if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
        raise InvalidOptionError("frame", tuple(shape), "an H x W x 3 BGR frame is expected")
    dt = _dtype(dtype)
    return dt, check_finish(finish).crop_for(shape[:2]), finish.orientation


def finish_frame_device(dev_src, dev_dst, h, w, dtype, finish, device=0, stream=None):
    """finish_frame() for a frame resident in HBM: `dev_src` (h x w x 3) -> `dev_dst` (H' x W' x 3, finish.finished_shape; a
    distinct buffer).  Queued on `stream`, not waited for."""
    dt, (cy, cx, ch, cw), orientation = _check_finish_frame((h, w, 3), dtype, finish)
    _lib.require_device()
    _lib.check(_lib.load().mi_frame_finish_device(device, stream, dev_src, dev_dst, int(h), int(w), _lib.DTYPE_CODE[dt], cy, cx, ch, cw,
                                                  orientation))


def finish_frame(frame, finish, device=0):
    """Crop and orientation of a dng.Finish applied to an H x W x 3 uint8 / uint16 BGR frame: the H' x W' x 3 frame (its
    vignette is not touched here: it belongs on the mosaic, `radial_gain`)."""
    a = np.ascontiguousarray(frame)
    dt, (cy, cx, ch, cw), orientation = _check_finish_frame(a.shape, a.dtype, finish)
    _lib.require_device()
    out = np.empty(finish.finished_shape(a.shape[:2]) + (3,), dt)
    _lib.check(_lib.load().mi_frame_finish(device, a.ctypes.data, out.ctypes.data, a.shape[0], a.shape[1], _lib.DTYPE_CODE[dt], cy, cx, ch,
                                           cw, orientation))
    return out


def defects_device(dev_mosaic, h, w, dtype, develop, device=0, stream=None):
    """Step 0 alone, in place on a mosaic resident in HBM.  Queued on `stream`, not waited for."""
    dt = _dtype(dtype)
    _, sites, n = check_develop(develop).prepared((h, w), dt, device)
    if n:
        _lib.check(_lib.load().mi_mosaic_defects_device(device, stream, dev_mosaic, int(h), int(w), _lib.DTYPE_CODE[dt], sites, n))


def debayer_device(dev_mosaic, dev_bgr, h, w, dtype, cfa, device=0, stream=None, develop=None, calibration=None, lens=None,
                   lens_scratch=None, corrections=None, finish=None, finish_scratch=None):
    """debayer() for a mosaic resident in HBM: `dev_mosaic` (h x w) -> `dev_bgr` (h x w x 3).  Queued on `stream`, not waited
    for.  `develop`: a Develop -- its defect sites are repaired IN PLACE in `dev_mosaic` first (no other site is written),
    then colour matrix and tone curve ride on the demosaic; its device tables must outlive the queued kernels.
    `calibration`: a Calibration -- `dev_mosaic` is calibrated IN PLACE ahead of all of that.
    `lens`: a lens.Lens -- the demosaic / develop kernel writes one scratch frame and the lens remap (lens.py) takes it to
    `dev_bgr`.  `lens_scratch`: that frame, a DeviceBuffer of h x w x 3 samples which must outlive the queued kernels; None:
    one is allocated here, and the call then WAITS for the device before it frees it.
    `corrections`: a dng.SiteCorrections -- `dev_mosaic` is corrected IN PLACE ahead of the calibration.
    `finish`: a dng.Finish -- its vignette gain is applied IN PLACE to `dev_mosaic` behind the corrections and ahead of the
    calibration; its crop and orientation are the last stage: everything above writes one scratch frame and frame_finish
    takes it to `dev_bgr`, which is then H' x W' x 3 (finish.finished_shape).  `finish_scratch`: that frame, as
    `lens_scratch` (a second one: the lens remap is out of place too)."""
    if corrections is not None:
        correct_sites_device(dev_mosaic, h, w, dtype, cfa, corrections, device=device, stream=stream)
    if finish is not None:
        from .dng import check_finish
        dt = _dtype(dtype)
        if check_finish(finish).vignette is not None:
            radial_gain_device(dev_mosaic, h, w, dt, cfa, finish.vignette, device=device, stream=stream, lens=lens)
        if finish.geometry((h, w)):
            own = finish_scratch is None
            need = int(h) * int(w) * 3 * dt.itemsize
            if not own and getattr(finish_scratch, "nbytes", 0) < need:
                raise InvalidOptionError("finish_scratch", getattr(finish_scratch, "nbytes", finish_scratch),
                                         f"a DeviceBuffer of at least {need} bytes (h x w x 3 samples) is expected")
            if own:
                _lib.require_device()
                finish_scratch = _lib.DeviceBuffer(need, device)
            try:
                debayer_device(dev_mosaic, finish_scratch.ptr, h, w, dt, cfa, device=device, stream=stream, develop=develop,
                               calibration=calibration, lens=lens, lens_scratch=lens_scratch)
                finish_frame_device(finish_scratch.ptr, dev_bgr, h, w, dt, finish, device=device, stream=stream)
                if own:
                    _lib.check(_lib.load().mi_device_synchronize(device))
            finally:
                if own:
                    finish_scratch.free()
            return
    if lens is not None:
        from .lens import check_lens, correct_device
        lens = check_lens(lens)
        dt = _dtype(dtype)
        own = lens_scratch is None
        need = int(h) * int(w) * 3 * dt.itemsize
        if not own and getattr(lens_scratch, "nbytes", 0) < need:
            raise InvalidOptionError("lens_scratch", getattr(lens_scratch, "nbytes", lens_scratch),
                                     f"a DeviceBuffer of at least {need} bytes (h x w x 3 samples) is expected")
        if own:
            _lib.require_device()
            lens_scratch = _lib.DeviceBuffer(int(h) * int(w) * 3 * dt.itemsize, device)
        try:
            debayer_device(dev_mosaic, lens_scratch.ptr, h, w, dt, cfa, device=device, stream=stream, develop=develop,
                           calibration=calibration)
            correct_device(lens_scratch.ptr, dev_bgr, h, w, dt, lens, device=device, stream=stream)
            if own:
                _lib.check(_lib.load().mi_device_synchronize(device))
        finally:
            if own:
                lens_scratch.free()
        return
    dt = _dtype(dtype)
    c = _check_cfa(cfa).struct(dt)
    if h < 2 or w < 2:
        raise InvalidOptionError("mosaic", (h, w), "a mosaic is an H x W plane with H, W >= 2")
    if calibration is not None:
        calibrate_device(dev_mosaic, h, w, dt, cfa, calibration, device=device, stream=stream)
    if develop is None:
        _lib.require_device()
        _lib.check(_lib.load().mi_demosaic_device(device, stream, dev_mosaic, dev_bgr, int(h), int(w), _lib.DTYPE_CODE[dt],
                                                  _lib.C.byref(c)))
        return
    d, sites, n = check_develop(develop).prepared((h, w), dt, device)
    lib = _lib.load()
    if n:
        _lib.check(lib.mi_mosaic_defects_device(device, stream, dev_mosaic, int(h), int(w), _lib.DTYPE_CODE[dt], sites, n))
    _lib.check(lib.mi_develop_device(device, stream, dev_mosaic, dev_bgr, int(h), int(w), _lib.DTYPE_CODE[dt], _lib.C.byref(c),
                                     _lib.C.byref(d)))


def debayer(mosaic, cfa, develop=None, device=0, calibration=None, lens=None, corrections=None, finish=None):
    """H x W uint8 / uint16 mosaic -> H x W x 3 BGR array of the same dtype.  `develop`: a Develop (defect sites, colour
    matrix, tone curve); None: the plain demosaic.  `calibration`: a Calibration applied to the mosaic first.  `lens`: a
    lens.Lens -- the lens correction behind all of it, on the device: equal to lens.correct(debayer(...), lens).
    `corrections`: a dng.SiteCorrections applied ahead of the calibration: equal to debayer(correct_sites(...), ...).
    `finish`: a dng.Finish -- equal to finish_frame(debayer(radial_gain(...), ...), finish): the vignette gain on the mosaic
    behind the corrections, crop and orientation last; the result is H' x W' x 3."""
    if corrections is not None:
        mosaic = correct_sites(mosaic, cfa, corrections, device=device)
    a = np.ascontiguousarray(check_mosaic(mosaic))
    c = _check_cfa(cfa).struct(a.dtype)
    if lens is not None:
        from .lens import check_lens
        lens = check_lens(lens)
    if finish is not None:
        from .dng import check_finish
        if calibration is not None:
            check_calibration(calibration).check_frame(a.shape, a.dtype)
        if develop is not None:
            check_develop(develop)
        oh, ow = check_finish(finish).finished_shape(a.shape)
        _lib.require_device()
        h, w = a.shape
        bufs = [_lib.DeviceBuffer(a.nbytes, device), _lib.DeviceBuffer(oh * ow * 3 * a.itemsize, device), _lib.DeviceBuffer(a.nbytes * 3, device)]
        try:
            if lens is not None:
                bufs.append(_lib.DeviceBuffer(a.nbytes * 3, device))
            bufs[0].upload(a)
            debayer_device(bufs[0].ptr, bufs[1].ptr, h, w, a.dtype, cfa, device=device, develop=develop, calibration=calibration, lens=lens,
                           lens_scratch=bufs[3] if lens is not None else None, finish=finish, finish_scratch=bufs[2])
            return bufs[1].download((oh, ow, 3), a.dtype)     # (a blocking copy on the null stream: behind the kernels)
        finally:
            for b in bufs:
                b.free()
    if calibration is not None or lens is not None:
        if calibration is not None:
            check_calibration(calibration).check_frame(a.shape, a.dtype)
        if develop is not None:
            check_develop(develop)
        _lib.require_device()
        h, w = a.shape
        stage, bgr = _lib.DeviceBuffer(a.nbytes, device), _lib.DeviceBuffer(a.nbytes * 3, device)
        scratch = None
        try:
            stage.upload(a)
            if lens is None:
                debayer_device(stage.ptr, bgr.ptr, h, w, a.dtype, cfa, device=device, develop=develop, calibration=calibration)
            else:
                scratch = _lib.DeviceBuffer(a.nbytes * 3, device)
                debayer_device(stage.ptr, bgr.ptr, h, w, a.dtype, cfa, device=device, develop=develop, calibration=calibration,
                               lens=lens, lens_scratch=scratch)
            return bgr.download((h, w, 3), a.dtype)     # (a blocking copy on the null stream: behind the kernels)
        finally:
            stage.free()
            bgr.free()
            if scratch is not None:
                scratch.free()
    if develop is not None:
        mq, tone, sites = check_develop(develop).host_args(a.shape, a.dtype)
    _lib.require_device()
    out = np.empty(a.shape + (3,), a.dtype)
    if develop is None:
        _lib.check(_lib.load().mi_demosaic(device, a.ctypes.data, out.ctypes.data, a.shape[0], a.shape[1], _lib.DTYPE_CODE[a.dtype],
                                           _lib.C.byref(c)))
        return out
    _lib.check(_lib.load().mi_develop(device, a.ctypes.data, out.ctypes.data, a.shape[0], a.shape[1], _lib.DTYPE_CODE[a.dtype],
                                      _lib.C.byref(c), mq, None if tone is None else tone.ctypes.data,
                                      sites.ctypes.data if len(sites) else None, len(sites)))
    return out


# ---------------------------------------------------------------- linear raw frames: no demosaic (csrc/kernels_linear.hpp)
class Linear:
    """The levels of an already demosaiced raw frame (a DNG's LinearRaw IFD), applied per sample where `Cfa` applies them per
    cell position: v' = min(white, (max(v - black[c], 0) * gain_q[c] + 2048) >> 12), c the sample's channel in file order
    (R, G, B); at spp 1 the one grey sample becomes b = g = r (tests/linear_restatement.py is the definition).

    black    black level, one non-negative int or `spp` of them
    gains    one float or `spp` in [0, 16): white balance and bit-depth scaling; quantised once, here, as round(gain * 4096)
    white    the output clamp; None: the dtype's maximum
    spp      samples per pixel: 1 or 3
    """

    def __init__(self, black=0, gains=1.0, white=None, spp=3):
        if isinstance(spp, bool) or not isinstance(spp, (int, np.integer)) or spp not in (1, 3):
            raise InvalidOptionError("spp", spp, "a linear frame has 1 or 3 samples per pixel")
        self.spp = int(spp)

        def per_channel(name, value, kinds):
            if isinstance(value, kinds) and not isinstance(value, bool):
                return [value] * self.spp
            try:
                vals = list(value)
            except TypeError:
                vals = None
            if vals is None or len(vals) not in (1, self.spp) or not all(isinstance(v, kinds) and not isinstance(v, bool) for v in vals):
                raise InvalidOptionError(name, value, f"one number, or {self.spp} (one per sample of a pixel)")
            return vals * self.spp if len(vals) == 1 and self.spp > 1 else vals
        self.black = [int(b) for b in per_channel("black", black, (int, np.integer))]
        if min(self.black) < 0 or max(self.black) > 65535:
            raise InvalidOptionError("black", black, "black levels lie in [0, 65535]")
        self.gains = [float(g) for g in per_channel("gains", gains, (int, float, np.integer, np.floating))]
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
        return f"Linear(black={self.black}, gains={self.gains}, white={self.white}, spp={self.spp})"

    def quantised(self, dtype=np.uint16):
        """the ints the kernel sees for frames of `dtype`: (black[spp], gain_q[spp], white, spp)"""
        maxv = int(np.iinfo(_dtype(dtype)).max)
        white = maxv if self.white is None else self.white
        if white > maxv:
            raise InvalidOptionError("white", white, f"exceeds the maximum {maxv} of {np.dtype(dtype)}")
        return tuple(self.black), tuple(self.gain_q), white, self.spp

    def struct(self, dtype):
        """mi_linear_t for frames of `dtype` (at spp 1 the entries 1 and 2 repeat entry 0; the kernel reads entry 0)"""
        black, gain_q, white, spp = self.quantised(dtype)
        return _lib.LinearStruct((_lib.C.c_int32 * 3)(*(black * 3)[:3]), (_lib.C.c_uint32 * 3)(*(gain_q * 3)[:3]), white, spp)


def _check_linear(linear):
    if not isinstance(linear, Linear):
        raise InvalidOptionError("linear", linear, "a shinestacker_amd.demosaic.Linear is expected")
    return linear


def check_samples(samples, linear, shape=None, dtype=None):
    """the samples of a linear frame: H x W x 3 (spp 3) or H x W (spp 1; H x W x 1 is taken too) of uint8 / uint16"""
    a = np.asarray(samples)
    _dtype(a.dtype)
    spp = _check_linear(linear).spp
    if a.ndim == 3 and a.shape[2] == 1 and spp == 1:
        a = a[:, :, 0]
    if a.ndim != (3 if spp == 3 else 2) or a.shape[0] < 1 or a.shape[1] < 1 or (spp == 3 and a.shape[2] != 3):
        raise InvalidOptionError("samples", a.shape, "a linear frame is H x W x 3 samples (spp 3) or H x W (spp 1)")
    if shape is not None and a.shape[:2] != tuple(shape):
        raise InvalidOptionError("samples", a.shape, f"expected {tuple(shape)} pixels")
    if dtype is not None and a.dtype != np.dtype(dtype):
        raise BitDepthError(np.dtype(dtype), a.dtype)
    return a


def _linear_options(develop, finish):
    """what a linear frame does not take: defect sites and a vignette gain address the sites of a CFA mosaic"""
    if develop is not None and check_develop(develop).defects is not None:
        raise InvalidOptionError("develop", develop, "Develop.defects lists the sites of a CFA mosaic: a LinearRaw frame has none")
    if finish is not None:
        from .dng import check_finish
        if check_finish(finish).vignette is not None:
            raise InvalidOptionError("finish", finish, "Finish.vignette is a gain on the sites of a CFA mosaic: a LinearRaw frame has none")


def develop_linear_device(dev_samples, dev_bgr, h, w, dtype, linear, device=0, stream=None, develop=None, lens=None, lens_scratch=None,
                          finish=None, finish_scratch=None):
    """develop_linear() for samples resident in HBM: `dev_samples` (h x w x linear.spp, only read) -> `dev_bgr` (h x w x 3).
    Queued on `stream`, not waited for.  `develop`: a Develop without defect sites -- its colour matrix and tone curve ride
    on the kernel; its device tables must outlive it.  `lens`, `lens_scratch`, `finish`, `finish_scratch`: as in
    debayer_device -- the lens remap and then crop and orientation behind the development, each through one scratch frame of
    h x w x 3 samples; a Finish with a vignette is refused (it is a gain on mosaic sites)."""
    dt = _dtype(dtype)
    _linear_options(develop, finish)
    need = int(h) * int(w) * 3 * dt.itemsize
    if finish is not None and finish.geometry((h, w)):
        own = finish_scratch is None
        if not own and getattr(finish_scratch, "nbytes", 0) < need:
            raise InvalidOptionError("finish_scratch", getattr(finish_scratch, "nbytes", finish_scratch),
                                     f"a DeviceBuffer of at least {need} bytes (h x w x 3 samples) is expected")
        if own:
            _lib.require_device()
            finish_scratch = _lib.DeviceBuffer(need, device)
        try:
            develop_linear_device(dev_samples, finish_scratch.ptr, h, w, dt, linear, device=device, stream=stream, develop=develop,
                                  lens=lens, lens_scratch=lens_scratch)
            finish_frame_device(finish_scratch.ptr, dev_bgr, h, w, dt, finish, device=device, stream=stream)
            if own:
                _lib.check(_lib.load().mi_device_synchronize(device))
        finally:
            if own:
                finish_scratch.free()
        return
    if lens is not None:
        from .lens import check_lens, correct_device
        lens = check_lens(lens)
        own = lens_scratch is None
        if not own and getattr(lens_scratch, "nbytes", 0) < need:
            raise InvalidOptionError("lens_scratch", getattr(lens_scratch, "nbytes", lens_scratch),
                                     f"a DeviceBuffer of at least {need} bytes (h x w x 3 samples) is expected")
        if own:
            _lib.require_device()
            lens_scratch = _lib.DeviceBuffer(need, device)
        try:
            develop_linear_device(dev_samples, lens_scratch.ptr, h, w, dt, linear, device=device, stream=stream, develop=develop)
            correct_device(lens_scratch.ptr, dev_bgr, h, w, dt, lens, device=device, stream=stream)
            if own:
                _lib.check(_lib.load().mi_device_synchronize(device))
        finally:
            if own:
                lens_scratch.free()
        return
    L = _check_linear(linear).struct(dt)
    if h < 1 or w < 1:
        raise InvalidOptionError("samples", (h, w), "a linear frame is at least 1 x 1")
    _lib.require_device()
    d = None
    if develop is not None:
        d, _, _ = develop.prepared((h, w), dt, device)
    _lib.check(_lib.load().mi_linear_develop_device(device, stream, dev_samples, dev_bgr, int(h), int(w), _lib.DTYPE_CODE[dt], _lib.C.byref(L),
                                                    None if d is None else _lib.C.byref(d)))


def develop_linear(samples, linear, develop=None, lens=None, finish=None, device=0):
    """The samples of a linear raw frame (H x W x 3 in R, G, B order, or H x W at spp 1; uint8 / uint16) -> H x W x 3 BGR of
    the same dtype: the levels of `linear` per sample, then `develop`'s colour matrix and tone curve (a Develop without defect
    sites), one pass on the device.  `lens`: a lens.Lens behind it: equal to lens.correct(develop_linear(...), lens).
    `finish`: a dng.Finish without a vignette: equal to finish_frame(develop_linear(...), finish); the result is H' x W' x 3."""
    a = np.ascontiguousarray(check_samples(samples, linear))
    L = linear.struct(a.dtype)
    _linear_options(develop, finish)
    h, w = a.shape[:2]
    if lens is not None or finish is not None:
        if lens is not None:
            from .lens import check_lens
            lens = check_lens(lens)
        oh, ow = (h, w) if finish is None else finish.finished_shape((h, w))
        _lib.require_device()
        nb = h * w * 3 * a.itemsize
        bufs = [_lib.DeviceBuffer(a.nbytes, device), _lib.DeviceBuffer(oh * ow * 3 * a.itemsize, device), _lib.DeviceBuffer(nb, device),
                _lib.DeviceBuffer(nb, device)]
        try:
            bufs[0].upload(a)
            develop_linear_device(bufs[0].ptr, bufs[1].ptr, h, w, a.dtype, linear, device=device, develop=develop, lens=lens,
                                  lens_scratch=bufs[2], finish=finish, finish_scratch=bufs[3])
            return bufs[1].download((oh, ow, 3), a.dtype)     # (a blocking copy on the null stream: behind the kernels)
        finally:
            for b in bufs:
                b.free()
    mq = tone = None
    if develop is not None:
        mq, tone, _ = develop.host_args((h, w), a.dtype)
    _lib.require_device()
    out = np.empty((h, w, 3), a.dtype)
    _lib.check(_lib.load().mi_linear_develop(device, a.ctypes.data, out.ctypes.data, h, w, _lib.DTYPE_CODE[a.dtype], _lib.C.byref(L), mq,
                                             None if tone is None else tone.ctypes.data))
    return out


def debayer_frames_device(mosaics, dev_out, cfa, device=0, develop=None, calibration=None, lens=None):
    """Upload the n host mosaics (equal shape and dtype) and demosaic them side by side into `dev_out` (device pointer,
    n x H x W x 3 of their dtype): exactly what pipeline.align_and_stack_device(dev_frames, ...) takes.  Waits for the device.
    `develop`: a Develop applied to every frame; `calibration`: a Calibration applied to every mosaic first; `lens`: a
    lens.Lens -- every frame passes through the lens correction behind its demosaic, through one scratch frame."""
    _check_cfa(cfa)
    if lens is not None:
        from .lens import check_lens
        lens = check_lens(lens)
    if develop is not None:
        check_develop(develop)
    if calibration is not None:
        check_calibration(calibration)
    if len(mosaics) == 0:
        raise ValueError("no mosaics")
    first = check_mosaic(mosaics[0])
    h, w = first.shape
    frame_bytes = h * w * 3 * first.itemsize
    _lib.require_device()
    stage = _lib.DeviceBuffer(h * w * first.itemsize, device)
    scratch = None
    try:
        if lens is not None:
            scratch = _lib.DeviceBuffer(frame_bytes, device)
        for i, m in enumerate(mosaics):
            stage.upload(check_mosaic(m, first.shape, first.dtype))
            if lens is not None:
                debayer_device(stage.ptr, dev_out + i * frame_bytes, h, w, first.dtype, cfa, device=device, develop=develop,
                               calibration=calibration, lens=lens, lens_scratch=scratch)
            elif calibration is not None:
                debayer_device(stage.ptr, dev_out + i * frame_bytes, h, w, first.dtype, cfa, device=device, develop=develop,
                               calibration=calibration)
            elif develop is None:
                debayer_device(stage.ptr, dev_out + i * frame_bytes, h, w, first.dtype, cfa, device=device)
            else:
                debayer_device(stage.ptr, dev_out + i * frame_bytes, h, w, first.dtype, cfa, device=device, develop=develop)
            # the stage is reused: the null stream's kernel must be through before the next (blocking) upload lands
            _lib.check(_lib.load().mi_device_synchronize(device))
    finally:
        stage.free()
        if scratch is not None:
            scratch.free()
