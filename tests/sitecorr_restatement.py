"""The site corrections of csrc/kernels_sitecorr.hpp restated in NumPy: integers only, the formulas of include/mi355stack.h.

This module is the definition the kernels are held to bit for bit.  It takes the QUANTISED tables (what
dng.SiteCorrections.quantised returns, or tables made by hand): no float appears here.

    pos = 2 (y & 1) + (x & 1), maxv the dtype's maximum
    bad list    a listed site becomes (S + (k >> 1)) // k over its k valid neighbours (y -+ 2, x), (y, x -+ 2): inside the image
                and not listed; k = 0 leaves the site
    bad const   the same with "listed" replaced by "holds C and lies on a position of the mask", judged before the step
    correct     b = black[pos] + dh[x] + dv[y];  e = max(v - b, 0)
                g = 4096 without a map, else with (i, a) = row_axis[y], (j, b) = col_axis[x], i1 = min(i + 1, mv - 1), j1 alike:
                g = ((256 - a) ((256 - b) n[i][j] + b n[i][j1]) + a ((256 - b) n[i1][j] + b n[i1][j1]) + 32768) >> 16
                e' = (e g + 2048) >> 12;  out = min(maxv, e' + black[pos])
"""
import numpy as np


def maxv(dtype):
    return int(np.iinfo(np.dtype(dtype)).max)


def repair(mosaic, bad):
    """step 0's rule for the boolean H x W mask `bad`: values are read from sites outside the mask only"""
    a = np.asarray(mosaic)
    h, w = a.shape
    v = a.astype(np.int64)
    s = np.zeros((h, w), np.int64)
    k = np.zeros((h, w), np.int64)
    ok = ~bad
    for dy, dx in ((-2, 0), (2, 0), (0, -2), (0, 2)):
        ys = slice(max(0, -dy), h - max(0, dy))
        yn = slice(max(0, dy), h - max(0, -dy))
        xs = slice(max(0, -dx), w - max(0, dx))
        xn = slice(max(0, dx), w - max(0, -dx))
        s[ys, xs] += np.where(ok[yn, xn], v[yn, xn], 0)
        k[ys, xs] += ok[yn, xn]
    out = v.copy()
    hit = bad & (k > 0)
    out[hit] = (s[hit] + (k[hit] >> 1)) // k[hit]
    return out.astype(a.dtype)


def repair_list(mosaic, sites):
    a = np.asarray(mosaic)
    bad = np.zeros(a.size, bool)
    bad[np.asarray(sites, np.int64)] = True
    return repair(a, bad.reshape(a.shape))


def repair_const(mosaic, constant, mask):
    a = np.asarray(mosaic)
    h, w = a.shape
    pos = 2 * (np.arange(h)[:, None] & 1) + (np.arange(w)[None, :] & 1)
    return repair(a, (a == constant) & (((mask >> pos) & 1) == 1))


def _pairs(axis):
    """(n, 2) ints of (node, weight) from pairs or from records with those two fields"""
    a = np.asarray(axis)
    if a.dtype.names:
        return np.stack([a["node"].astype(np.int64), a["weight"].astype(np.int64)], axis=1)
    return a.astype(np.int64).reshape(-1, 2)


def gain_plane(shape, gains):
    """the Q12 gain of every site: `gains` is four entries (one per position), each None or (nodes, row_axis, col_axis) with
    nodes mv x mh, row_axis (H, 2) and col_axis (W, 2) of (node, weight)"""
    h, w = shape
    g = np.full((h, w), 4096, np.int64)
    for p, m in enumerate(gains):
        if m is None:
            continue
        n = np.asarray(m[0], np.int64)
        mv, mh = n.shape
        ra, ca = _pairs(m[1]), _pairs(m[2])
        ys, xs = np.arange(p >> 1, h, 2), np.arange(p & 1, w, 2)
        i, a = ra[ys, 0][:, None], ra[ys, 1][:, None]
        j, b = ca[xs, 0][None, :], ca[xs, 1][None, :]
        i1, j1 = np.minimum(i + 1, mv - 1), np.minimum(j + 1, mh - 1)
        top = (256 - b) * n[i, j] + b * n[i, j1]
        bot = (256 - b) * n[i1, j] + b * n[i1, j1]
        s = (256 - a) * top + a * bot + 32768
        assert s.max() < 2 ** 32
        g[p >> 1::2, p & 1::2] = s >> 16
    return g


def correct(mosaic, black, dh=None, dv=None, gains=None):
    a = np.asarray(mosaic)
    h, w = a.shape
    top = maxv(a.dtype)
    bl = np.asarray(black, np.int64).reshape(2, 2)
    blk = bl[np.arange(h)[:, None] & 1, np.arange(w)[None, :] & 1]
    b = blk.copy()
    if dh is not None:
        b = b + np.asarray(dh, np.int64)[None, :]
    if dv is not None:
        b = b + np.asarray(dv, np.int64)[:, None]
    assert b.min() >= 0 and b.max() <= top, "the caller's promise: 0 <= b <= maxv"
    e = np.maximum(a.astype(np.int64) - b, 0)
    if gains is not None and any(m is not None for m in gains):
        eg = e * gain_plane((h, w), gains) + 2048
        assert eg.max() < 2 ** 32
        e = eg >> 12
    return np.minimum(top, e + blk).astype(a.dtype)


def site_correct(mosaic, black, dh=None, dv=None, gains=None, bad_sites=None, bad_constant=None):
    """the whole stage in its order: bad list, bad constant (value, mask), deltas and gains"""
    a = np.asarray(mosaic)
    if bad_sites is not None and len(bad_sites):
        a = repair_list(a, bad_sites)
    if bad_constant is not None:
        a = repair_const(a, int(bad_constant[0]), int(bad_constant[1]))
    if dh is None and dv is None and (gains is None or all(m is None for m in gains)):
        return a.copy()
    return correct(a, black, dh, dv, gains)
