"""The cases of tests/test_gpu_phase_edges.py, their planes and their statements (tests/phase_restatement.py in float64
and float32), computed once per process and shared by that module and by tests/test_phase_restatement.py, which proves
from the statements alone that every case is decided before a kernel is asked."""
import functools
import types

import numpy as np

import phase_restatement as pr

FACTOR = 8.0   # a kernel's bound = FACTOR x the deviation of the float32 statement from the float64 statement (see the
#                header of tests/test_gpu_phase_edges.py for the reason)

# name -> (h, w, (dx, dy)): mov(x, y) = ref(x - dx, y - dy), both cut from one white-noise field
STAGE_CASES = {
    "3x3": (3, 3, (0, 0)),            # the 4-point line, 2 threads; Hann leaves the centre pixel
    "5x7": (5, 7, (1, 0)),            # an 8-point line
    "3x1000": (3, 1000, (-37, 0)),    # a 4-point column pass beside a 1024-point row pass
    "1000x3": (1000, 3, (0, 52)),     # ... and the other way round
    "513x9": (513, 9, (1, -200)),     # one over 512: the 1024-point column pass with stride Q = 16
    "9x513": (9, 513, (150, -1)),     # the 1024-point row pass
    "64x64": (64, 64, (-5, 9)),       # no padding
    "65x64": (65, 64, (7, -3)),       # one row over: P = 128
    "250x375": (250, 375, (17, -9)),  # the shape of the test in test_gpu_ecc.py
    "1023x600": (1023, 600, (-60, 101)),   # a ragged 1024-point column pass
    "1024x1024": (1024, 1024, (-203, 77)),  # the largest plane the entry point takes
}

MARGIN = 256


@functools.lru_cache(maxsize=None)
def _field(seed, h, w):
    return (np.random.default_rng(seed).random((h + 2 * MARGIN, w + 2 * MARGIN)) * 255).astype(np.float32)


def noise_pair(h, w, shift, seed=0, extra_noise=0.0):
    """ref and mov = ref displaced by the integer `shift` = (dx, dy), float32 white noise in [0, 255)"""
    dx, dy = shift
    assert abs(dx) <= MARGIN and abs(dy) <= MARGIN
    big = _field(1000 + seed, h, w)
    ref = big[MARGIN:MARGIN + h, MARGIN:MARGIN + w]
    mov = big[MARGIN - dy:MARGIN - dy + h, MARGIN - dx:MARGIN - dx + w]
    if extra_noise:
        rng = np.random.default_rng(2000 + seed)
        ref = ref + rng.normal(0, extra_noise, ref.shape).astype(np.float32)
        mov = mov + rng.normal(0, extra_noise, mov.shape).astype(np.float32)
    return np.ascontiguousarray(ref, np.float32), np.ascontiguousarray(mov, np.float32)


def smooth_pair(h, w, shift, seed=7):
    """a fractional shift of a lightly smoothed white-noise field (the construction of test_gpu_ecc.py's phase test)"""
    from scipy import ndimage
    big = ndimage.gaussian_filter(np.random.default_rng(seed).random((h + 64, w + 64)) * 255, 1.0)
    dx, dy = shift
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ref = ndimage.map_coordinates(big, [yy + 32, xx + 32], order=3)
    mov = ndimage.map_coordinates(big, [yy + 32 - dy, xx + 32 - dx], order=3)
    return ref.astype(np.float32), mov.astype(np.float32)


def unrelated_pair(h, w, seed=0):
    return noise_pair(h, w, (0, 0), seed=seed + 50)[0], noise_pair(h, w, (0, 0), seed=seed + 51)[0]


def _half_shifts(h, w):
    P, Q = pr.pow2(h), pr.pow2(w)
    return [(Q // 2 - 3, 0), (-(Q // 2 - 3), 0), (0, P // 2 - 3), (0, -(P // 2 - 3))]


# name -> (maker, args): what goes through the public phase_correlate
RESULT_CASES = {}
for _h, _w in ((64, 64), (250, 375)):
    RESULT_CASES[f"zero-{_h}x{_w}"] = (noise_pair, (_h, _w, (0, 0), 3, 40.0))   # peak at the origin: the window wraps on both axes
for _s in (1, -1, 2, -2):
    RESULT_CASES[f"dx{_s:+d}-65x64"] = (noise_pair, (65, 64, (_s, 0), 4))       # the window wraps on one side
    RESULT_CASES[f"dy{_s:+d}-65x64"] = (noise_pair, (65, 64, (0, _s), 5))
for _h, _w in ((64, 64), (250, 500)):                                           # (w = 375 loses the peak: the overlap is too short)
    for _sh in _half_shifts(_h, _w):                                            # the wrap to negative shifts
        RESULT_CASES[f"half{_sh[0]:+d}{_sh[1]:+d}-{_h}x{_w}"] = (noise_pair, (_h, _w, _sh, 6))
RESULT_CASES["fractional-125x188"] = (smooth_pair, (125, 188, (3.4, 7.7)))
UNRELATED = "unrelated-1000x1000"   # only its response is compared: its centroid is a quotient of two noise sums
SAME = "same-"                      # prefix: SAME + a stage case's name is that case's ref plane against itself


@functools.lru_cache(maxsize=None)
def planes(name):
    if name in STAGE_CASES:
        h, w, shift = STAGE_CASES[name]
        return noise_pair(h, w, shift, seed=sum(map(ord, name)))
    if name == UNRELATED:
        return unrelated_pair(1000, 1000)
    if name.startswith(SAME):
        return (planes(name[len(SAME):])[0],) * 2
    maker, args = RESULT_CASES[name]
    return maker(*args)


@functools.lru_cache(maxsize=None)
def statement(name, dtype):
    ref, mov = planes(name)
    return pr.phase_correlate(ref, mov, dtype)


def rel(a, b, scale):
    """largest |a - b| over `scale`"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / scale)


def own_stage(kind, prev, prev_ref=None):
    """The float64 statement of one stage applied to the complex plane(s) `prev` some float32 program left"""
    if kind == "spectrum":
        return np.fft.fft2(prev.astype(np.complex128))
    if kind == "cross_power":
        x = prev.astype(np.complex128) * np.conj(prev_ref.astype(np.complex128))
        mag = np.abs(x)
        return np.where(mag > 1e-20, x / np.where(mag > 1e-20, mag, 1.0), 0.0)
    if kind == "surface":
        return np.fft.ifft2(prev.astype(np.complex128)) * prev.size
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def deviations(name):
    """What the float32 statement deviates from the float64 one, per quantity: `e2e_*` against the whole float64 statement,
    `own_*` against the float64 statement of one stage applied to the float32 statement's own previous stage.  Spectra
    relative to the largest float64 bin, the surface (and its imaginary part) relative to P Q, the rest absolute."""
    s32, s64 = statement(name, np.float32), statement(name, np.float64)
    PQ = float(s64.P * s64.Q)
    d = types.SimpleNamespace()
    wmax = float(np.abs(s64.windowed_mov).max()) or 1.0
    d.windowed = rel(s32.windowed_mov, s64.windowed_mov, wmax)
    d.windowed_ref = rel(s32.windowed_ref, s64.windowed_ref, float(np.abs(s64.windowed_ref).max()) or 1.0)
    for k in ("ref", "mov"):
        big = float(np.abs(getattr(s64, "spectrum_" + k)).max()) or 1.0
        setattr(d, "e2e_spectrum_" + k, rel(getattr(s32, "spectrum_" + k), getattr(s64, "spectrum_" + k), big))
        own = own_stage("spectrum", getattr(s32, "windowed_" + k))
        setattr(d, "own_spectrum_" + k, rel(getattr(s32, "spectrum_" + k), own, float(np.abs(own).max()) or 1.0))
    d.e2e_cross_power = rel(s32.cross_power, s64.cross_power, 1.0)
    d.own_cross_power = rel(s32.cross_power, own_stage("cross_power", s32.spectrum_mov, s32.spectrum_ref), 1.0)
    d.e2e_surface = rel(s32.surface, s64.surface, PQ)
    d.own_surface = rel(s32.surface, own_stage("surface", s32.cross_power), PQ)
    d.imag = float(np.abs(s32.surface.imag).max() / PQ)
    d.dx, d.dy, d.response = abs(s32.dx - s64.dx), abs(s32.dy - s64.dy), abs(s32.response - s64.response)
    d.result = max(d.dx, d.dy, d.response)
    return d


def held(got, want, dev, scale=1.0):
    """The comparison every bound uses: == where the statements' own deviation is exactly 0, else within FACTOR x it.
    -> (ok, measured deviation)"""
    err = rel(got, want, scale)
    return (err == 0.0 if dev == 0.0 else err <= FACTOR * dev), err
