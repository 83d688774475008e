"""Phase correlation restated in plain NumPy from the header comment of csrc/kernels_phase.hpp, stage by stage (imports
nothing from the project): Hann window (cv2.createHanningWindow's 0.5 (1 - cos(2 pi i / (n - 1)))), zero-padding to P x Q
(powers of two), forward DFT of both planes, R = Mov conj(Ref) / |Mov conj(Ref)| (0 where the magnitude is not above
1e-20), un-normalised inverse DFT, first arg-max of the real part in raster order, weighted centroid of the wrapping 5 x 5
window, positions beyond half the size wrapped to negative shifts, response = window sum / (P Q).

The working type is a parameter.  float64 is the reference.  float32 repeats the kernels' own order of operations --
radix-2 decimation in time, bit-reversed load, stages half = 1, 2, 4, ..., butterfly a +- b e^{-+ i pi k / half}, rows
then columns, every multiply and add rounded on its own (real and imaginary parts are separate real arrays, so nothing is
fused) -- with twiddles and window computed in float64 and rounded once: its distance from the float64 result is the
rounding noise of a correct float32 program, which is what the kernels' bounds are sized from."""
import types

import numpy as np


def pow2(n):
    return 1 << max(int(n) - 1, 0).bit_length()


def hann(n, dtype=np.float64):
    if n == 1:
        return np.ones(1, dtype)
    return (0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / (n - 1)))).astype(dtype)


def windowed(plane, P, Q, dtype=np.float64):
    """plane * (wy * wx), zero-padded to P x Q, as a (re, im) pair of `dtype`"""
    h, w = plane.shape
    win = hann(h, dtype)[:, None] * hann(w, dtype)[None, :]
    re = np.zeros((P, Q), dtype)
    re[:h, :w] = plane.astype(dtype) * win
    return re, np.zeros((P, Q), dtype)


def _twiddles(half, inverse, dtype):
    """e^{-+ i pi k / half}, k < half: exact 0 / 1 where the angle is a multiple of pi / 2, as sincospi gives them"""
    x = np.arange(half, dtype=np.float64) / half
    cs, sn = np.cos(np.pi * x), np.sin(np.pi * x)
    cs[x == 0.5] = 0.0
    if not inverse:
        sn = -sn
    return cs.astype(dtype), sn.astype(dtype)


def fft_lines(re, im, inverse, dtype):
    """radix-2 DFT along the last axis (length a power of two), no scaling"""
    n = re.shape[-1]
    log2n = n.bit_length() - 1
    assert 1 << log2n == n
    idx = np.arange(n)
    rev = np.zeros(n, np.int64)
    for b in range(log2n):
        rev |= ((idx >> b) & 1) << (log2n - 1 - b)
    lead = re.shape[:-1]
    re, im = re[..., rev].astype(dtype), im[..., rev].astype(dtype)     # s[rev(i)] = line[i], rev is an involution
    for sft in range(log2n):
        half = 1 << sft
        cs, sn = _twiddles(half, inverse, dtype)
        re, im = re.reshape(*lead, n // (2 * half), 2, half), im.reshape(*lead, n // (2 * half), 2, half)
        ax, ay, bx, by = re[..., 0, :], im[..., 0, :], re[..., 1, :], im[..., 1, :]
        tx, ty = bx * cs - by * sn, bx * sn + by * cs
        re, im = np.stack([ax + tx, ax - tx], axis=-2), np.stack([ay + ty, ay - ty], axis=-2)
        re, im = re.reshape(*lead, n), im.reshape(*lead, n)
    return re, im


def fft2(re, im, inverse=False, dtype=np.float64):
    """rows, then columns"""
    re, im = fft_lines(np.asarray(re, dtype), np.asarray(im, dtype), inverse, dtype)
    re, im = fft_lines(np.ascontiguousarray(re.T), np.ascontiguousarray(im.T), inverse, dtype)
    return np.ascontiguousarray(re.T), np.ascontiguousarray(im.T)


def cross_power(mov, ref, dtype=np.float64):
    """(re, im) pairs of the two spectra -> R = Mov conj(Ref) / |.|"""
    xx, xy, yx, yy = (np.asarray(v, dtype) for v in (*mov, *ref))
    re, im = xx * yx + xy * yy, xy * yx - xx * yy
    mag = np.sqrt(re * re + im * im)
    ok = mag > dtype(1e-20)
    inv = np.where(ok, dtype(1.0) / np.where(ok, mag, dtype(1.0)), dtype(0.0))
    return re * inv, im * inv, mag


def peak(surface_re):
    """first arg-max, 5 x 5 wrapping centroid, signed shift, response; float64 arithmetic whatever the surface's type
    -> (dx, dy, response, (py, px))"""
    P, Q = surface_re.shape
    py, px = (int(v) for v in np.unravel_index(np.argmax(surface_re), surface_re.shape))
    m = mx = my = 0.0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            v = float(surface_re[(py + dy) % P, (px + dx) % Q])
            m, mx, my = m + v, mx + v * (px + dx), my + v * (py + dy)
    cx, cy = (mx / m, my / m) if m != 0.0 else (float(px), float(py))
    if cx > 0.5 * Q:
        cx -= Q
    if cy > 0.5 * P:
        cy -= P
    return cx, cy, m / (float(P) * float(Q)), (py, px)


def _c(pair):
    return pair[0] + 1j * pair[1]


def phase_correlate(ref, mov, dtype=np.float64):
    """Every stage for one pair of planes (complex arrays of the working precision; `cross_mag` is |Mov conj(Ref)|)"""
    dtype = np.dtype(dtype).type
    h, w = ref.shape
    assert mov.shape == ref.shape
    P, Q = pow2(h), pow2(w)
    wr, wm = windowed(ref, P, Q, dtype), windowed(mov, P, Q, dtype)
    sr, sm = fft2(*wr, False, dtype), fft2(*wm, False, dtype)
    rre, rim, mag = cross_power(sm, sr, dtype)
    cre, cim = fft2(rre, rim, True, dtype)
    dx, dy, response, at = peak(cre)
    return types.SimpleNamespace(P=P, Q=Q, windowed_ref=_c(wr), windowed_mov=_c(wm), spectrum_ref=_c(sr), spectrum_mov=_c(sm),
                                 cross_power=rre + 1j * rim, cross_mag=mag, surface=cre + 1j * cim, peak=at, dx=dx, dy=dy,
                                 response=response)
