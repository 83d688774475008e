"""The depth refinement's arithmetic restated in NumPy (csrc/kernels_guided.hpp states the same evaluation order; the kernels are
held to this bit for bit).  There is no reference counterpart: this file is the specification.

The confidence-weighted guided filter (He, Sun, Tang): in every (2 r + 1)^2 window, clipped to the frame, the weighted
least-squares line depth ~ a I + b over the guide's grey I; a pixel's result is the mean of the lines of the windows that
hold it, evaluated at its own I.  Everything in float64, every operation rounded on its own:

    grey      g = (1868 B + 9617 G + 4899 R + 8192) >> 14 on the native samples; I = float64(g) / 255.0 (uint8) or / 65535.0
    products  P = float64(p), Wd = float64(w); t1 = Wd * I, t2 = Wd * P, t3 = t1 * I, t4 = t1 * P
    box sum   B(x): rows first, then columns.  R(y, x) = sum of x(y, x + k) over k = -r .. r ascending, the accumulator starting
              at +0.0, acc = acc + term, a term outside the frame +0.0; B(x)(y, x) the same sum over R(y + k, x)
    model     sw = B(Wd), swI = B(t1), swp = B(t2), swII = B(t3), swIp = B(t4); where sw > 0: mI = swI / sw, mp = swp / sw,
              var = swII / sw - mI * mI, cov = swIp / sw - mI * mp, a = cov / (var + eps), b = mp - a * mI; elsewhere a = 0, b = P
    output    n = float64(rows of the window in the frame * columns of it in the frame); q = (B(a) / n) * I + B(b) / n;
              q = min(max(q, lo), hi); float32

Written for the tests; it shares nothing with shinestacker_amd/depth_out.py or the kernels.
"""
import numpy as np

MAX_RADIUS = 32


def grey(guide):
    """the integer grey of an H x W x 3 BGR frame, on its native samples"""
    g = np.asarray(guide)
    assert g.ndim == 3 and g.shape[2] == 3 and g.dtype in (np.uint8, np.uint16)
    v = g.astype(np.uint64)
    return ((v[:, :, 0] * 1868 + v[:, :, 1] * 9617 + v[:, :, 2] * 4899 + 8192) >> 14).astype(np.int64)


def intensity(guide):
    """I in [0, 1], float64: one divide"""
    return grey(guide).astype(np.float64) / (255.0 if np.asarray(guide).dtype == np.uint8 else 65535.0)


def _sum_axis(x, r, axis):
    n = x.shape[axis]
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    xp = np.pad(x, pad, mode="constant", constant_values=0.0)     # +0.0 outside the frame
    acc = np.zeros(x.shape, np.float64)
    for k in range(2 * r + 1):                                      # ascending taps, one rounded add each
        sl = [slice(None), slice(None)]
        sl[axis] = slice(k, k + n)
        acc = acc + xp[tuple(sl)]
    return acc


def box(x, r):
    """B(x): rows (along the columns of each row), then columns"""
    return _sum_axis(_sum_axis(np.asarray(x, np.float64), r, 1), r, 0)


def window_counts(shape, r):
    """n(y, x): the pixels of the clipped window, as float64"""
    h, w = shape
    y, x = np.arange(h), np.arange(w)
    ny = np.minimum(y + r, h - 1) - np.maximum(y - r, 0) + 1
    nx = np.minimum(x + r, w - 1) - np.maximum(x - r, 0) + 1
    return (ny[:, None] * nx[None, :]).astype(np.float64)


def model(p, w, guide, radius, eps):
    """(a, b, sw): the planes of the linear models and the summed weight"""
    P = np.asarray(p, np.float32).astype(np.float64)
    Wd = np.asarray(w).astype(np.float64)
    I = intensity(guide)
    assert P.ndim == 2 and P.shape == Wd.shape == I.shape
    r, eps = int(radius), float(eps)
    t1 = Wd * I
    t2 = Wd * P
    t3 = t1 * I
    t4 = t1 * P
    sw, swI, swp, swII, swIp = box(Wd, r), box(t1, r), box(t2, r), box(t3, r), box(t4, r)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mI = swI / sw
        mp = swp / sw
        var = swII / sw - mI * mI
        cov = swIp / sw - mI * mp
        a = cov / (var + eps)
        b = mp - a * mI
    has = sw > 0
    return np.where(has, a, 0.0), np.where(has, b, P), sw


def guided_refine(p, w, guide, radius, eps, lo, hi):
    """the kernels' result: H x W float32"""
    r = int(radius)
    assert 1 <= r <= MAX_RADIUS and 1e-9 <= float(eps) <= 1e3 and float(lo) <= float(hi)
    a, b, _ = model(p, w, guide, r, eps)
    n = window_counts(a.shape, r)
    q = (box(a, r) / n) * intensity(guide) + box(b, r) / n
    q = np.minimum(np.maximum(q, np.float64(lo)), np.float64(hi))
    return q.astype(np.float32)
