"""The depth map's arithmetic restated in NumPy (csrc/kernels_depth.hpp states the same evaluation order; the kernels are held
to this bit for bit).  There is no reference counterpart: this file is the specification.

    weighted smoothing   out = B(v * w) / B(w) where B(w) > 0, else v;  B = separable Gaussian, BORDER_REFLECT_101

    taps     radius = ceil(3 sigma); 2 radius + 1 taps exp(-x^2 / (2 sigma^2)) in float64 (libm's exp, one tap at a time),
             divided by their sum (accumulated in ascending order), rounded once to the working type
    1.       p = v * w: one multiply in the working type (an int32 index converts exactly)
    2. rows  acc = 0; for t ascending: acc = acc + tap[t] * x[reflect101(col - radius + t)]; product and sum rounded separately
    3. cols  the same over rows, on the row results; p and w take the same taps
    4.       one divide, then the cast to float32

Written for the tests; it shares nothing with shinestacker_amd/depth_out.py or the kernels.
"""
import math

import numpy as np


def radius_of(sigma):
    return int(math.ceil(3.0 * float(sigma)))


def taps_of(sigma, dtype):
    """the rounded taps, in `dtype`"""
    sigma = float(sigma)
    r = radius_of(sigma)
    t = [math.exp(-(float(x) * float(x)) / (2.0 * sigma * sigma)) for x in range(-r, r + 1)]
    total = 0.0
    for v in t:
        total += v
    return np.array([v / total for v in t], np.float64).astype(dtype)


def _blur_axis(x, taps, axis):
    """acc = acc + tap[t] * x[reflect101(i - radius + t)] along `axis`, in x's type (np.pad 'reflect' is REFLECT_101)"""
    dt = x.dtype
    r = len(taps) // 2
    n = x.shape[axis]
    assert r < n, "the radius must be smaller than the plane"
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    xp = np.pad(x, pad, mode="reflect")
    acc = np.zeros(x.shape, dt)
    for t in range(len(taps)):
        sl = [slice(None), slice(None)]
        sl[axis] = slice(t, t + n)
        prod = (dt.type(taps[t]) * xp[tuple(sl)]).astype(dt)
        acc = (acc + prod).astype(dt)
    return acc


def blur(x, taps):
    """rows (along the columns of each row), then columns"""
    return _blur_axis(_blur_axis(x, taps, 1), taps, 0)


def _smooth(value, weight, taps, dtype):
    dt = np.dtype(dtype)
    v = np.asarray(value).astype(dt)
    w = np.asarray(weight).astype(dt)
    k = np.asarray(taps).astype(dt)
    num = blur((v * w).astype(dt), k)
    den = blur(w, k)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (num / den).astype(dt)
    return np.where(den > 0, q, v)


def weighted_smooth(value, weight, sigma, dtype=np.float32):
    """the kernel's result: working type `dtype`, float32 out"""
    dt = np.dtype(dtype)
    if sigma == 0:
        return np.asarray(value).astype(dt).astype(np.float32)
    return _smooth(value, weight, taps_of(sigma, dt), dt).astype(np.float32)


def weighted_smooth_f64(value, weight, sigma, taps_dtype=np.float32):
    """the same in float64 arithmetic WITH the taps rounded to `taps_dtype`: what the float32 form is measured against;
    returned in float64"""
    if sigma == 0:
        return np.asarray(value).astype(np.float64)
    return _smooth(value, weight, taps_of(sigma, taps_dtype), np.float64)


def depth_index(planes, total):
    """DepthMapStack: D = (sum_i planes[i] * i) / total in the planes' type, i ascending, multiply and add separate;
    0 where total == 0"""
    planes = np.asarray(planes)
    dt = planes.dtype
    acc = np.zeros(planes.shape[1:], dt)
    for i in range(planes.shape[0]):
        acc = (acc + (planes[i] * dt.type(i)).astype(dt)).astype(dt)
    total = np.asarray(total).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (acc / total).astype(dt)
    return np.where(total == 0, dt.type(0), q)


def depth_map_stack(planes, total, sigma, average):
    """DepthMapStack.depth_map: depth_index, then the smoothing in the planes' type with w = total (AVERAGE) or 1 (MAX)"""
    d = depth_index(planes, total)
    if sigma == 0:
        return d.astype(np.float32)
    w = np.asarray(total).astype(d.dtype) if average else np.ones(d.shape, d.dtype)
    return weighted_smooth(d, w, sigma, d.dtype)
