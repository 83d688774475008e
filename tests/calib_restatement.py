"""NumPy restatement of raw calibration (shinestacker_amd/csrc/kernels_calib.hpp: mosaic_master, flat_sums / flat_gain_table and
mosaic_calibrate): the definition the HIP kernels are held to bit for bit.  Integers only (int64; Python ints where a product
could leave int64).  H x W mosaics of uint8 / uint16, H, W >= 2, maxv the dtype's maximum; pos = 2 (y & 1) + (x & 1) is the cell
position of a site.  Nothing depends on the colour pattern.

Master frame:  K mosaics of one shape and dtype, 1 <= K <= 32, 0 <= reject, 2 reject < K.  Per site the K samples sorted
               ascending s[0 .. K - 1]; n = K - 2 reject; S = s[reject] + ... + s[K - reject - 1]; out = (S + (n >> 1)) // n.
               reject 0: the rounded mean; (K - 1) // 2: the median (even K: the rounded mean of the two middle samples).
Flat gain:     f = max(F - B, 0) per site, B the flat-dark or black[pos].  Per position p the sum S_p of f and the number N_p
               of sites.  G_q = 16384 where f == 0 or S_p == 0, else min(65535, (2 * 16384 * S_p + N_p f) // (2 N_p f)); uint16.
               With H W < 2^31: S_p < 2^45, numerator < 2^61, denominator < 2^47 -- unsigned 64 bits hold.
Calibrate:     e = max(v - (D[site] if dark else black[pos]), 0);  e' = (e G_q[site] + 8192) >> 14 if flat else e;
               out = min(maxv, e' + black[pos]).  With neither a dark nor a flat nothing is done: out = v.
"""
import numpy as np

GAIN_ONE = 16384
MAX_FRAMES = 32
SITE_BOUND = 2 ** 31


def position_map(shape):
    """pos = 2 (y & 1) + (x & 1) per site"""
    y, x = np.indices(shape)
    return 2 * (y & 1) + (x & 1)


def black_map(shape, black):
    return np.asarray(black, dtype=np.int64)[position_map(shape)]


def master(frames, reject):
    frames = [np.asarray(f) for f in frames]
    k = len(frames)
    assert 1 <= k <= MAX_FRAMES and 0 <= reject and 2 * reject < k
    assert all(f.shape == frames[0].shape and f.dtype == frames[0].dtype for f in frames)
    s = np.sort(np.stack(frames).astype(np.int64), axis=0)
    n = k - 2 * reject
    total = s[reject:k - reject].sum(axis=0)
    return ((total + (n >> 1)) // n).astype(frames[0].dtype)


def flat_signal(flat, black, flat_dark=None):
    """f = max(F - B, 0)"""
    flat = np.asarray(flat)
    b = black_map(flat.shape, black) if flat_dark is None else np.asarray(flat_dark).astype(np.int64)
    return np.maximum(flat.astype(np.int64) - b, 0)


def flat_gain(flat, black=(0, 0, 0, 0), flat_dark=None, return_sums=False):
    flat = np.asarray(flat)
    h, w = flat.shape
    assert h >= 2 and w >= 2 and h * w < SITE_BOUND
    f = flat_signal(flat, black, flat_dark)
    pos = position_map(flat.shape)
    out = np.full(flat.shape, GAIN_ONE, dtype=np.int64)
    sums, counts = [], []
    for p in range(4):
        sel = pos == p
        s_p, n_p = int(f[sel].sum()), int(sel.sum())
        sums.append(s_p)
        counts.append(n_p)
        assert 2 * GAIN_ONE * s_p + n_p * 65535 < 2 ** 64
        if s_p == 0:
            continue
        fp = f[sel]
        live = fp > 0
        g = np.full(fp.shape, GAIN_ONE, dtype=np.int64)
        g[live] = np.minimum(65535, (2 * GAIN_ONE * s_p + n_p * fp[live]) // (2 * n_p * fp[live]))   # < 2^61: int64 holds
        out[sel] = g
    out = out.astype(np.uint16)
    return (out, sums, counts) if return_sums else out


def calibrate(mosaic, black=(0, 0, 0, 0), dark=None, gain=None, return_parts=False):
    """return_parts: (out, e, e' + black before the clamp) as int64 too"""
    mosaic = np.asarray(mosaic)
    maxv = int(np.iinfo(mosaic.dtype).max)
    b = black_map(mosaic.shape, black)
    v = mosaic.astype(np.int64)
    if dark is not None:
        assert np.asarray(dark).shape == mosaic.shape and np.asarray(dark).dtype == mosaic.dtype
    if dark is None and gain is None:       # nothing is enqueued: the samples stay, those below the black level too
        z = np.zeros_like(v)
        return (mosaic.copy(), z, z) if return_parts else mosaic.copy()
    e = np.maximum(v - (b if dark is None else np.asarray(dark).astype(np.int64)), 0)
    e2 = e
    if gain is not None:
        g = np.asarray(gain)
        assert g.shape == mosaic.shape and g.dtype == np.uint16
        prod = e * g.astype(np.int64)
        assert int(prod.max(initial=0)) + 8192 < 2 ** 32
        e2 = (prod + 8192) >> 14
    pre = e2 + b
    out = np.minimum(maxv, pre).astype(mosaic.dtype)
    return (out, e, pre) if return_parts else out
