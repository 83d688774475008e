"""Lens correction on the MI355X: radial distortion and lateral chromatic aberration as one remap (csrc/kernels_lens.hpp).

The reference stacks developed frames and never corrects the lens, so this has no reference counterpart.  Two defects of a
real macro lens matter to a focus stacker: barrel / pincushion distortion, under which two frames at different
magnifications (focus breathing) are not related by the similarity or homography `AlignFrames` fits, and lateral chromatic
aberration, whose colour fringes are high-contrast detail that the stack selects and accumulates.

The model is the radial part of DNG's `WarpRectilinear` per colour plane, destination -> source (tests/lens_restatement.py
is the definition; every step float64, every operation rounded once):

    dx = x - cx, dy = y - cy;  u = (dx*dx + dy*dy) / R2       R2: the largest dx*dx + dy*dy of the four corner pixels
    s = ((k3*u + k2)*u + k1)*u + k0                            per plane c = B, G, R
    source = (cx + dx*s, cy + dy*s), limited to [-1, w] x [-1, h], rounded to 1/32 pixel (the alignment warp's grid)
    out = the bilinear blend of the four taps around it, replicate border, (sum + 512) >> 10

One `Lens` carries both corrections, since the coefficients are per plane: distortion is the part the planes share, lateral
CA the part in which red and blue differ from green.  A plane of (1, 0, 0, 0) comes out bit for bit as it went in.

There is no CPU path: without a GPU or the library `correct` and its kin raise DeviceError.  `Lens` and `autoscale` are
host NumPy.
"""
import math

import numpy as np

from . import _lib
from .actions import SubAction
from .errors import BitDepthError, InvalidOptionError

IDENTITY = (1.0, 0.0, 0.0, 0.0)
CENTRE_MAX = 2.0 ** 30                          # mi_lens_remap's bound: cx + (x - cx) is then x to far below 1/64 pixel
TILE_H, TILE_W = 16, 64                         # lens::TILE_H / TILE_W of csrc/kernels_lens.hpp


def _number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _plane(name, value, exact=True):
    """(k0, k1, k2, k3) as floats: four finite numbers (`exact`), or one to four with the rest 0"""
    try:
        vals = list(value)
    except TypeError:
        vals = None
    if vals is None or not all(_number(v) for v in vals) or not (len(vals) == 4 if exact else 1 <= len(vals) <= 4):
        raise InvalidOptionError(name, value, "four numbers (k0, k1, k2, k3)" if exact else "one to four numbers (k0, k1, k2, k3)")
    vals = [float(v) for v in vals] + [0.0] * (4 - len(vals))
    if not all(math.isfinite(v) for v in vals):
        raise InvalidOptionError(name, value, "the coefficients must be finite")
    return tuple(vals)


class Lens:
    """The radial polynomials of the three colour planes and the optical centre.

    radial   (k0, k1, k2, k3) for all planes, or three such tuples in B, G, R order like the frames
    centre   (cx, cy) in pixels; None: the middle of the frame it is used on, ((w - 1) / 2, (h - 1) / 2)
    """

    def __init__(self, radial=IDENTITY, centre=None):
        try:
            items = list(radial)
        except TypeError:
            items = None
        if items is not None and len(items) == 3 and not any(_number(v) for v in items):
            self.k = tuple(_plane("radial", p) for p in items)
        else:
            self.k = (_plane("radial", radial),) * 3
        if centre is not None:
            try:
                c = list(centre)
            except TypeError:
                c = None
            if c is None or len(c) != 2 or not all(_number(v) and math.isfinite(v) and abs(v) <= CENTRE_MAX for v in c):
                raise InvalidOptionError("centre", centre, "two finite numbers (cx, cy) in pixels, at most 2^30 in magnitude, or None")
            centre = (float(c[0]), float(c[1]))
        self.centre = centre

    def __repr__(self):
        return f"Lens(radial={[list(p) for p in self.k]}, centre={self.centre})"

    def __eq__(self, other):
        return isinstance(other, Lens) and self.k == other.k and self.centre == other.centre

    __hash__ = None

    @classmethod
    def distortion(cls, k1, k2=0, k3=0, k0=1, centre=None):
        """a distortion-only lens: the same polynomial on every plane"""
        return cls((k0, k1, k2, k3), centre)

    @classmethod
    def chromatic(cls, red=IDENTITY, blue=IDENTITY, centre=None):
        """a lateral-CA-only lens: `red` and `blue` are (k0, k1, ...) of those planes (the rest 0), green stays at identity"""
        return cls((_plane("blue", blue, exact=False), IDENTITY, _plane("red", red, exact=False)), centre)

    @classmethod
    def from_warp_rectilinear(cls, coeffs, centre=None):
        """from the DNG opcode's coefficients: one plane, or three in R, G, B order (the opcode's), each kr0..kr3 optionally
        followed by the tangential kt0, kt1 -- which must be 0: the tangential terms are not modelled.  The opcode's radius
        is normalised as this model's is (1 at the farthest corner)."""
        try:
            items = list(coeffs)
        except TypeError:
            items = None
        if items is None or len(items) == 0:
            raise InvalidOptionError("coeffs", coeffs, "kr0..kr3 (and kt0, kt1) of one plane or of three")
        planes = [items] if all(_number(v) for v in items) else items
        if len(planes) not in (1, 3):
            raise InvalidOptionError("coeffs", coeffs, "the opcode has one plane or three (R, G, B)")
        out = []
        for p in planes:
            try:
                p = list(p)
            except TypeError:
                p = []
            if len(p) not in (4, 6) or not all(_number(v) for v in p):
                raise InvalidOptionError("coeffs", coeffs, "a plane has kr0..kr3, or kr0..kr3, kt0, kt1")
            if any(float(v) != 0.0 for v in p[4:]):
                raise InvalidOptionError("coeffs", coeffs, "the tangential terms kt0, kt1 are not modelled and must be 0")
            out.append(_plane("coeffs", p[:4]))
        return cls(out[0] if len(out) == 1 else (out[2], out[1], out[0]), centre)

    def resolved_centre(self, h, w):
        """the centre on an h x w frame, float64"""
        return ((w - 1) / 2.0, (h - 1) / 2.0) if self.centre is None else self.centre

    def coefficients(self):
        """the 12 coefficients k[4 * c + i], c = B, G, R, as a float64 array"""
        return np.array(self.k, np.float64).reshape(12)

    def struct(self, h, w):
        """mi_lens_t for h x w frames, the centre resolved"""
        cx, cy = self.resolved_centre(h, w)
        return _lib.LensStruct((_lib.C.c_double * 12)(*self.coefficients()), cx, cy)

    def scaled(self, f):
        """the lens with all 12 coefficients multiplied by `f`: the corrected frame magnified by 1 / f about the centre"""
        if not _number(f) or not math.isfinite(f):
            raise InvalidOptionError("f", f, "a finite number is expected")
        with np.errstate(over="ignore"):
            k = (self.coefficients() * np.float64(f)).reshape(3, 4)
        if not np.isfinite(k).all():
            raise InvalidOptionError("f", f, "the scaled coefficients must be finite")
        return Lens([tuple(p) for p in k.tolist()], self.centre)

    def autoscale(self, h, w):
        """The largest f for which `scaled(f)` keeps the source position of every border pixel inside
        [0, w - 1] x [0, h - 1], on every plane: the minimum, over border pixels, planes and the two axes, of the allowed
        offset from the centre over the actual one.  1.0 when no border pixel moves off the centre's row and column.
        Without it the replicated border shows as sharp radial streaks, which the stack would select.  Host float64."""
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise InvalidOptionError("shape", (h, w), "height and width must be >= 1")
        cx, cy = self.resolved_centre(h, w)
        if not (0.0 <= cx <= w - 1 and 0.0 <= cy <= h - 1):
            raise InvalidOptionError("centre", (cx, cy), f"autoscale needs the centre inside the {h} x {w} frame")
        border = np.zeros((h, w), bool)
        border[[0, -1], :] = True
        border[:, [0, -1]] = True
        y, x = np.nonzero(border)
        dx, dy = x.astype(np.float64) - cx, y.astype(np.float64) - cy
        u = (dx * dx + dy * dy) * inv_r2(h, w, cx, cy)
        best = np.inf
        with np.errstate(divide="ignore", invalid="ignore"):
            for k0, k1, k2, k3 in self.k:
                s = ((k3 * u + k2) * u + k1) * u + k0
                for off, lo, hi in ((dx * s, -cx, (w - 1) - cx), (dy * s, -cy, (h - 1) - cy)):
                    ratio = np.where(off > 0, hi / off, np.where(off < 0, lo / off, np.inf))
                    best = min(best, float(ratio.min()))
        return best if math.isfinite(best) else 1.0


def inv_r2(h, w, cx, cy):
    """1 / (the largest squared distance of a corner pixel from the centre), 0.0 when that is 0: lens_inv_r2 of the library"""
    r2 = 0.0
    for x in (0.0, float(w - 1)):
        for y in (0.0, float(h - 1)):
            ddx, ddy = np.float64(x) - np.float64(cx), np.float64(y) - np.float64(cy)
            r2 = max(r2, float(ddx * ddx + ddy * ddy))
    return 0.0 if r2 == 0.0 else float(np.float64(1.0) / np.float64(r2))


def check_lens(lens):
    """a Lens; anything else `Lens(radial=...)` takes is made one"""
    return lens if isinstance(lens, Lens) else Lens(lens)


def _check_frame(shape, dtype):
    if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
        raise InvalidOptionError("frame", tuple(shape), "an H x W x 3 BGR frame is expected")
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.uint8), np.dtype(np.uint16)):
        raise BitDepthError("uint8 or uint16", dt)
    return dt


def correct_device(dev_src, dev_dst, h, w, dtype, lens, device=0, stream=None, dev_mask=None):
    """The remap of a frame resident in HBM: `dev_src` -> `dev_dst` (h x w x 3 of `dtype`, distinct buffers); `dev_mask`
    (h x w bytes, optional) receives 1 where every plane's source position lies inside the frame.  Queued on `stream`, not
    waited for."""
    dt = _check_frame((h, w, 3), dtype)
    L = check_lens(lens).struct(h, w)
    _lib.require_device()
    _lib.check(_lib.load().mi_lens_remap_device(device, stream, dev_src, dev_dst, dev_mask, int(h), int(w), _lib.DTYPE_CODE[dt],
                                                _lib.C.byref(L)))


def correct(frame, lens, device=0, return_mask=False):
    """H x W x 3 uint8 / uint16 BGR frame -> the corrected frame of the same shape and dtype; with `return_mask` also the
    H x W uint8 mask of the pixels whose source positions lie inside the frame on every plane."""
    a = np.ascontiguousarray(frame)
    dt = _check_frame(a.shape, a.dtype)
    h, w = a.shape[:2]
    L = check_lens(lens).struct(h, w)
    _lib.require_device()
    out = np.empty_like(a)
    mask = np.empty((h, w), np.uint8) if return_mask else None
    _lib.check(_lib.load().mi_lens_remap(device, a.ctypes.data, out.ctypes.data, None if mask is None else mask.ctypes.data, h, w,
                                         _lib.DTYPE_CODE[dt], _lib.C.byref(L)))
    return (out, mask) if return_mask else out


class LensCorrection(SubAction):
    """Sub-action of CombinedActions with Vignetting's protocol (begin(process) / run_frame(idx, ref_idx, image) / end());
    `run_frame_device` is the same step for a frame that lives in HBM.  Its place is behind MaskNoise and Vignetting and
    ahead of AlignFrames: hot pixels are repaired before anything resamples them, and the alignment then fits frames whose
    geometry its model describes.  Every frame passes through it, the reference frame included: `corrects_reference` makes
    CombinedActions.img_ref hand AlignFrames the reference frame corrected too (without step_process it reads the input file).

    lens       a Lens (or what `Lens(radial=...)` takes)
    autoscale  True: the lens is scaled by `Lens.autoscale` of the frame, so that no replicated border enters the frame
    """

    corrects_reference = True

    def __init__(self, lens, autoscale=False, device=0, enabled=True):
        super().__init__(enabled)
        self.lens = check_lens(lens)
        if not isinstance(autoscale, (bool, np.bool_)):
            raise InvalidOptionError("autoscale", autoscale, "True or False")
        self.autoscale = bool(autoscale)
        self.device = device
        self.process = None
        self._scaled = {}       # (h, w) -> the lens used on frames of that shape
        self._scratch = None    # a device frame: the remap's source when a resident frame is corrected in place

    def lens_for(self, h, w):
        """the lens applied to h x w frames"""
        if not self.autoscale:
            return self.lens
        if (h, w) not in self._scaled:
            self._scaled[(h, w)] = self.lens.scaled(self.lens.autoscale(h, w))
        return self._scaled[(h, w)]

    def begin(self, process, counts=None):
        self.process = process

    def run_frame_device(self, idx, dev_img, height, width, dtype, stream=None):
        """run_frame for a frame resident in HBM, corrected in place: the frame is copied to a scratch frame and remapped
        from there, both enqueued on `stream`."""
        dt = _check_frame((height, width, 3), dtype)
        lens = self.lens_for(height, width)
        fb = height * width * 3 * dt.itemsize
        if self._scratch is not None and self._scratch.nbytes != fb:
            _lib.check(_lib.load().mi_device_synchronize(self.device))
            self._scratch.free()
            self._scratch = None
        if self._scratch is None:
            self._scratch = _lib.DeviceBuffer(fb, self.device)
        _lib.check(_lib.load().mi_memcpy_d2d_async(self.device, stream, self._scratch.ptr, dev_img, fb))
        correct_device(self._scratch.ptr, dev_img, height, width, dt, lens, self.device, stream)

    def run_frame(self, idx, _ref_idx, img_0):
        f = getattr(self.process, "sub_message_r", None)
        if f is not None:
            f(": correct lens")
        return correct(img_0, self.lens_for(img_0.shape[0], img_0.shape[1]), self.device)

    def end(self):
        if self._scratch is not None:
            _lib.check(_lib.load().mi_device_synchronize(self.device))
            self._scratch.free()
            self._scratch = None


def make_step(lens, device=0):
    """the LensCorrection of a `lens=` option: a Lens (or what Lens takes), or a dict of LensCorrection's options"""
    if isinstance(lens, dict):
        opts = dict(lens)
        if "lens" not in opts:
            raise InvalidOptionError("lens", lens, "a dict of LensCorrection's options names the lens under 'lens'")
        unknown = sorted(set(opts) - {"lens", "autoscale"})
        if unknown:
            raise InvalidOptionError("lens", unknown, "a dict of lens, autoscale")
        return LensCorrection(device=device, **opts)
    return LensCorrection(lens, device=device)
