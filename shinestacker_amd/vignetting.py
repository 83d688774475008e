"""Vignetting on the MI355X path (reference algorithms/vignetting.py).

Per frame the reference takes the mean intensity of the (sub-sampled, 8-bit gray) frame in `r_steps` radial rings, fits
the double-exponential sigmoid `sigmoid_model` to them, and divides the full-resolution frame by the fitted curve
(normalised to its value at the centre, blended by `max_correction`, left alone where the frame is black).

Here the two passes over pixels run on the GPU (`mi_radial_ring_sums_device`, `mi_vignette_apply_device`:
csrc/kernels_prestack.hpp).  The ring sums are integers, so the ring means are the reference's `np.mean` exactly; the fit
(`scipy.optimize.curve_fit`), `v0` and the percentile radii (`scipy.optimize.fsolve`) are the reference's calls on
`r_steps` numbers on the host; the apply pass is float64 like the reference's NumPy expression.

Same class, constructor arguments and sub-action protocol (begin(process) / run_frame(idx, ref_idx, image) / end()) as the
reference; `run_frame_device` is the same step for a frame that lives in HBM.  The plots are drawn only where matplotlib
imports.
"""
import logging
import traceback

import numpy as np

from . import _lib
from .actions import SubAction
from .defaults import constants

CLIP_EXP = 10


def _exp(x):
    """float64 exp rounded once from long double: the same number on every NumPy build (NumPy's own float64 exp is SIMD-
    dispatch dependent), and the one the fixtures were recorded with.  Where np.longdouble is float64 (some platforms) this
    is NumPy's own exp and the results are close to the fixtures', not equal.  Every model evaluation of curve_fit and
    fsolve pays the round trip: it is part of the per-frame host time stated in docs/studies.md."""
    return np.exp(np.asarray(x, np.float64).astype(np.longdouble)).astype(np.float64)


def sigmoid_model(r, i0, k, r0):
    """The vignetting model, i0 / (1 + exp(exp(k (r - r0)))), both exponents limited to CLIP_EXP as the reference limits
    them (its vignetting.py:16-20): the inner argument to [-CLIP_EXP, CLIP_EXP], the outer one to at most CLIP_EXP."""
    inner = _exp(np.clip(k * (r - r0), -CLIP_EXP, CLIP_EXP))
    return i0 / (1.0 + _exp(np.minimum(CLIP_EXP, inner)))


def subsampled_shape(height, width, subsample, fast_subsampling):
    """(rows, columns) of the gray image the rings are taken of (utils.py:79-86; mi_subsampled_size)"""
    import ctypes as C
    hs, ws = C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().mi_subsampled_size(int(height), int(width), int(subsample), int(bool(fast_subsampling)),
                                              C.byref(hs), C.byref(ws)))
    return hs.value, ws.value


def ring_table(hs, ws, r_steps):
    """The ring borders of an hs x ws image (vignetting.py:26-29): r_steps + 1 float64"""
    r_max = np.sqrt((ws / 2)**2 + (hs / 2)**2)
    return np.linspace(0, r_max, r_steps + 1)


def ring_means(sums, counts):
    """sum / count per ring in float64 = np.mean of the ring's uint8 values (an exact integer sum, one division); NaN for
    an empty ring (vignetting.py:35-38)"""
    sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.float64)
    out = np.full(sums.shape, np.nan)
    np.divide(sums, counts, out=out, where=counts > 0)
    return out


def fit_sigmoid(radii, intensities):
    """Least-squares (i0, k, r0) of the model over the rings that have a mean; start and bounds are the reference's
    (vignetting.py:42-49): twice the brightest ring, 10 / r_max, 0.8 r_max; all three parameters non-negative."""
    from scipy.optimize import curve_fit
    keep = ~np.isnan(intensities)
    r_max = radii.max()
    start = [2 * np.max(intensities[keep]), 10 / r_max, 0.8 * r_max]
    popt, _pcov = curve_fit(sigmoid_model, radii[keep], intensities[keep], p0=start, bounds=(0.0, np.inf))
    return popt


def percentile_radii(params, v0, percentiles):
    """vignetting.py:162-164: the radius at which the fitted curve has fallen to each percentile of its centre value"""
    from scipy.optimize import fsolve
    return [fsolve(lambda x, p=p: sigmoid_model(x, *params) / v0 - p, params[2])[0] for p in percentiles]


class _DeviceFrame:
    """A host frame uploaded for the duration of one call."""

    def __init__(self, image, device):
        self.a = np.ascontiguousarray(image)
        self.buf = _lib.DeviceBuffer(self.a.nbytes, device)
        self.buf.upload(self.a)

    def download(self):
        return self.buf.download(self.a.shape, self.a.dtype)

    def free(self):
        self.buf.free()


def _check_frame(shape, dtype):
    if len(shape) != 3 or shape[2] != 3 or np.dtype(dtype) not in (np.dtype(np.uint8), np.dtype(np.uint16)):
        raise ValueError("expected an H x W x 3 uint8/uint16 BGR frame")


def radial_ring_sums_device(dev_img, height, width, dtype, r_steps, subsample=constants.DEFAULT_VIGN_SUBSAMPLE,
                            fast_subsampling=constants.DEFAULT_VIGN_FAST_SUBSAMPLING, device=0, stream=None, scratch=None):
    """(ring centres, ring means, sums, counts) of the device frame: vignetting.py:52-55 + :23-39 with the pixel pass on
    the GPU.  `scratch`: a DeviceBuffer of mi_radial_ring_scratch_bytes(r_steps), allocated here when None."""
    lib = _lib.load()
    hs, ws = subsampled_shape(height, width, subsample, fast_subsampling)
    table = np.ascontiguousarray(ring_table(hs, ws, r_steps), np.float64)
    sums, counts = np.zeros(r_steps, np.uint64), np.zeros(r_steps, np.uint32)
    own = scratch is None
    if own:
        scratch = _lib.DeviceBuffer(lib.mi_radial_ring_scratch_bytes(int(r_steps)), device)
    try:
        _lib.check(lib.mi_radial_ring_sums_device(device, stream, dev_img, scratch.ptr, int(height), int(width),
                                                  _lib.DTYPE_CODE[np.dtype(dtype)], int(subsample), int(bool(fast_subsampling)),
                                                  int(r_steps), table.ctypes.data, sums.ctypes.data, counts.ctypes.data))
    finally:
        if own:
            scratch.free()
    return (table[1:] + table[:-1]) / 2, ring_means(sums, counts), sums, counts


def radial_mean_intensity(image, r_steps, subsample=1, fast_subsampling=False, device=0):
    """Ring centres and ring means of a host BGR frame (the reference's img_subsampled + radial_mean_intensity)."""
    _check_frame(image.shape, image.dtype)
    _lib.require_device()
    f = _DeviceFrame(image, device)
    try:
        radii, means, _, _ = radial_ring_sums_device(f.buf.ptr, image.shape[0], image.shape[1], image.dtype, r_steps, subsample,
                                                     fast_subsampling, device)
    finally:
        f.free()
    return radii, means


def vignette_apply_device(dev_src, dev_dst, height, width, dtype, params, v0, max_correction=constants.DEFAULT_MAX_CORRECTION,
                          black_threshold=constants.DEFAULT_BLACK_THRESHOLD, device=0, stream=None):
    """vignetting.py:84-97 on a device frame (dev_dst may be dev_src); enqueued, not synchronised"""
    dt = np.dtype(dtype)
    threshold = black_threshold if dt == np.uint8 else black_threshold * 256
    i0, k, r0 = (float(p) for p in params)
    _lib.check(_lib.load().mi_vignette_apply_device(device, stream, dev_src, dev_dst, int(height), int(width), _lib.DTYPE_CODE[dt],
                                                    i0, k, r0, float(v0), float(max_correction), float(threshold)))


def correct_vignetting(image, max_correction=constants.DEFAULT_MAX_CORRECTION,
                       black_threshold=constants.DEFAULT_BLACK_THRESHOLD, r_steps=constants.DEFAULT_R_STEPS, params=None, v0=None,
                       subsample=constants.DEFAULT_VIGN_SUBSAMPLE, fast_subsampling=constants.DEFAULT_VIGN_FAST_SUBSAMPLING,
                       device=0):
    """vignetting.py:71-97 for a host BGR frame: fit when `params` is None, then the apply pass on the GPU"""
    _check_frame(image.shape, image.dtype)
    _lib.require_device()
    h, w = image.shape[:2]
    f = _DeviceFrame(image, device)
    try:
        if params is None:
            if r_steps is None:
                raise RuntimeError("Either r_steps or pars must not be None")
            radii, means, _, _ = radial_ring_sums_device(f.buf.ptr, h, w, image.dtype, r_steps, subsample, fast_subsampling, device)
            params = fit_sigmoid(radii, means)
            params[1] /= subsample
            params[2] *= subsample
        if v0 is None:
            v0 = sigmoid_model(0, *params)
        vignette_apply_device(f.buf.ptr, f.buf.ptr, h, w, image.dtype, params, v0, max_correction, black_threshold, device)
        _lib.check(_lib.load().mi_device_synchronize(device))
        return f.download()
    finally:
        f.free()


def _pyplot():
    try:
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
        return plt
    except Exception:  # noqa: BLE001  no matplotlib: no plots
        return None


def _save_plot(plt, filename):
    import os
    os.makedirs(os.path.dirname(filename) or '.', exist_ok=True)
    plt.savefig(filename, dpi=150)
    plt.close('all')


class Vignetting(SubAction):
    """Sub-action of CombinedActions (vignetting.py:100-210)."""

    def __init__(self, enabled=True, percentiles=(0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95), **kwargs):
        super().__init__(enabled)
        self.r_steps = kwargs.get('r_steps', constants.DEFAULT_R_STEPS)
        self.black_threshold = kwargs.get('black_threshold', constants.DEFAULT_BLACK_THRESHOLD)
        self.plot_correction = kwargs.get('plot_correction', False)
        self.plot_summary = kwargs.get('plot_summary', False)
        self.max_correction = kwargs.get('max_correction', constants.DEFAULT_MAX_CORRECTION)
        self.percentiles = np.sort(percentiles)
        self.subsample = kwargs.get('subsample', constants.DEFAULT_VIGN_SUBSAMPLE)
        self.fast_subsampling = kwargs.get('fast_subsampling', constants.DEFAULT_VIGN_FAST_SUBSAMPLING)
        self.device = kwargs.get('device', 0)
        self.w_2 = None
        self.h_2 = None
        self.v0 = None
        self.r_max = None
        self.process = None
        self.corrections = None
        self.params = None       # the last frame's fitted (i0, k, r0), full-resolution pixels; None when the fit failed
        self._scratch = None

    # -- messages go to the owning process when it has the reference's methods
    def _msg_r(self, text):
        f = getattr(self.process, "sub_message_r", None)
        if f is not None:
            f(text)

    def _msg(self, text, level=logging.INFO):
        f = getattr(self.process, "sub_message", None)
        if f is not None:
            f(text, level=level)
        else:
            logging.getLogger(__name__).log(level, text)

    def begin(self, process, counts=None):
        self.process = process
        if counts is None:   # rows are indexed by the GLOBAL frame index (a sharded process counts only its own block)
            names = getattr(process, "filenames", None)
            counts = len(names) if names is not None else process.counts
        self.corrections = [np.full(counts, None, dtype=float) for p in self.percentiles]

    def _fit(self, idx, radii, intensities):
        """vignetting.py:126-143 + :162-164: parameters in full-resolution pixels, or None (warning) when the fit raises"""
        try:
            params = fit_sigmoid(radii, intensities)
            params[1] /= self.subsample  # k
            params[2] *= self.subsample  # r0
        except Exception as e:  # noqa: BLE001  as the reference: any failure of the fit leaves the frame alone
            traceback.print_tb(e.__traceback__)
            self._msg(": could not find vignetting model", level=logging.WARNING)
            self.params = None
            return None
        self.params = params
        self.v0 = sigmoid_model(0, *params)
        i0_fit, k_fit, r0_fit = params
        self._msg(f": vignetting model parameters: i0={i0_fit / 2:.4f}, k={k_fit * self.r_max:.4f}, "
                  f"r0={r0_fit / self.r_max:.4f}", level=logging.DEBUG)
        if self.plot_correction:
            self._plot_correction(idx, radii, intensities, params)
        for i, r in enumerate(percentile_radii(params, self.v0, self.percentiles)):
            self.corrections[i][idx] = r
        return params

    def run_frame_device(self, idx, dev_img, height, width, dtype, stream=None):
        """run_frame for a frame resident in HBM, corrected in place.  The ring sums synchronise `stream` (the fit needs
        them on the host); the apply pass is enqueued on it.  Returns the fitted parameters, or None when the fit failed
        and the frame was left unchanged."""
        self._msg_r(": compute vignetting")
        self.w_2, self.h_2 = width / 2, height / 2
        self.r_max = np.sqrt((width / 2)**2 + (height / 2)**2)
        if self._scratch is None:
            self._scratch = _lib.DeviceBuffer(_lib.load().mi_radial_ring_scratch_bytes(int(self.r_steps)), self.device)
        radii, intensities, _, _ = radial_ring_sums_device(dev_img, height, width, dtype, self.r_steps, self.subsample,
                                                           self.fast_subsampling, self.device, stream, self._scratch)
        params = self._fit(idx, radii, intensities)
        if params is None:
            return None
        self._msg_r(": correct vignetting")
        vignette_apply_device(dev_img, dev_img, height, width, dtype, params, self.v0, self.max_correction,
                              self.black_threshold, self.device, stream)
        return params

    def run_frame(self, idx, _ref_idx, img_0):
        _check_frame(img_0.shape, img_0.dtype)
        _lib.require_device()
        f = _DeviceFrame(img_0, self.device)
        try:
            if self.run_frame_device(idx, f.buf.ptr, img_0.shape[0], img_0.shape[1], img_0.dtype) is None:
                return img_0
            _lib.check(_lib.load().mi_device_synchronize(self.device))
            return f.download()
        finally:
            f.free()

    def end(self):
        if self._scratch is not None:
            self._scratch.free()
            self._scratch = None
        if self.plot_summary:
            self._plot_summary()

    def _plot_path(self, tail):
        p = self.process
        return f"{p.working_path}/{p.plot_path}/{p.name}-{tail}.pdf"

    def _plot_correction(self, idx, radii, intensities, params):
        """ring means and fitted curve of one frame (file name and callback as the reference's)"""
        plt = _pyplot()
        if plt is None:
            return
        fig, ax = plt.subplots(figsize=(10, 5))
        ax.plot(radii, intensities, label="image mean intensity")
        ax.plot(radii, sigmoid_model(radii * self.subsample, *params), label="sigmoid fit")
        ax.set(xlabel="radius (pixels)", ylabel="mean intensity", xlim=(radii[0], radii[-1]))
        ax.set_ylim(bottom=0)
        ax.legend()
        tag = f"{idx:04d}"
        path = self._plot_path(f"radial-intensity-{tag}")
        _save_plot(plt, path)
        self.process.callback('save_plot', self.process.id, f"{self.process.name}: intensity\nframe {tag}", path)

    def _plot_summary(self):
        """percentile radii over the frames, with the frame's half sizes and largest radius for scale"""
        plt = _pyplot()
        if plt is None or self.r_max is None:
            return
        rows, pct = self.corrections, list(self.percentiles)
        frame_no = np.arange(1, len(rows[0]) + 1)
        fig, ax = plt.subplots(figsize=(10, 5))
        for j, (p, row) in enumerate(zip(pct, rows)):
            style = '-.' if p == 0.5 else ('dotted' if j in (0, len(pct) - 1) else 'solid')
            ax.plot(frame_no, row, linestyle=style, color="blue", label=f"{p:.0%} correction")
        ax.fill_between(frame_no, rows[-1], rows[0], color="#0000ff20")
        if 0.5 in pct and 0 < pct.index(0.5) < len(pct) - 1:
            mid = pct.index(0.5)
            ax.fill_between(frame_no, rows[mid - 1], rows[mid + 1], color="#0000ff20")
        ends = frame_no[[0, -1]]
        for level, label, color in ((self.r_max, "max. radius", "darkred"), (self.w_2, "half width", "limegreen"),
                                    (self.h_2, "half height", "darkgreen")):
            ax.plot(ends, [level, level], linestyle="--", color=color, label=label)
        ax.set(xlabel="frame", ylabel="distance from center (pixels)", xlim=(ends[0], ends[1]), ylim=(0, 1.05 * self.r_max))
        ax.legend(ncols=2)
        path = self._plot_path("r0")
        _save_plot(plt, path)
        self.process.callback('save_plot', self.process.id, f"{self.process.name}: vignetting", path)
