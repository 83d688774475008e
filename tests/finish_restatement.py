"""The finishing kernels of csrc/kernels_finish.hpp restated in NumPy: integers only, the formulas of include/mi355stack.h.

This module is the definition the kernels are held to bit for bit.  It takes the QUANTISED inputs (what dng.RadialGain
hands the library: the centre in half pixels and the Q12 table): no float appears in `radial_gain` or `finish`.

    radial gain   d2 = (2x - cx2)^2 + (2y - cy2)^2;  D = the largest d2 of the four corner sites (1 <= D < 2^40)
                  shift = the largest s with floor(2^(18+s) / D) < 2^24,  mul = floor(2^(18+shift) / D)
                  q = min((d2 mul) >> shift, 2^18);  node = q >> 8, weight = q & 255
                  g = (t[node] (256 - weight) + t[min(node + 1, 1024)] weight + 128) >> 8
                  e = max(v - black[pos], 0);  e' = (e g + 2048) >> 12;  out = min(maxv, e' + black[pos]),  pos = 2 (y & 1) + (x & 1)
    finish        a = frame[cy:cy + ch, cx:cx + cw] turned by the TIFF orientation (ORIENT)

`gain_error_bound` is the DERIVED distance between the quantised gain and the float64 polynomial (see its docstring).
"""
import numpy as np

NODES = 1025
Q_ONE = 1 << 18
D2_MAX = 1 << 40

# the orientation table: TIFF Orientation -> what becomes of a[y, x, c]
ORIENT = {
    1: lambda a: a,
    2: lambda a: a[:, ::-1],
    3: lambda a: a[::-1, ::-1],
    4: lambda a: a[::-1],
    5: lambda a: a.transpose(1, 0, 2),
    6: lambda a: np.rot90(a, -1),
    7: lambda a: a[::-1, ::-1].transpose(1, 0, 2),
    8: lambda a: np.rot90(a, 1),
}


def maxv(dtype):
    return int(np.iinfo(np.dtype(dtype)).max)


def d2max(h, w, cx2, cy2):
    return max((2 * x - cx2) ** 2 + (2 * y - cy2) ** 2 for x in (0, w - 1) for y in (0, h - 1))


def radial_map(D):
    """(mul, shift): Python ints, no rounding anywhere"""
    assert 1 <= D < D2_MAX
    s = 46
    while s > 0 and (1 << (18 + s)) // D >= 1 << 24:
        s -= 1
    return (1 << (18 + s)) // D, s


def radial_q(h, w, cx2, cy2):
    """q of every site, H x W int64"""
    mul, shift = radial_map(d2max(h, w, cx2, cy2))
    dx = 2 * np.arange(w, dtype=np.int64) - cx2
    dy = 2 * np.arange(h, dtype=np.int64) - cy2
    d2 = ((dx * dx)[None, :] + (dy * dy)[:, None]).astype(np.uint64)     # below 2^40
    q = (d2 * np.uint64(mul)) >> np.uint64(shift)                         # d2 * mul < 2^64: exact in uint64
    return np.minimum(q, np.uint64(Q_ONE)).astype(np.int64)


def radial_g(h, w, cx2, cy2, table):
    """the Q12 gain of every site, H x W int64"""
    t = np.asarray(table).astype(np.int64)
    assert t.shape == (NODES,)
    q = radial_q(h, w, cx2, cy2)
    node, wt = q >> 8, q & 255
    return (t[node] * (256 - wt) + t[np.minimum(node + 1, NODES - 1)] * wt + 128) >> 8


def radial_gain(mosaic, black, cx2, cy2, table):
    a = np.asarray(mosaic)
    h, w = a.shape
    pos = 2 * (np.arange(h)[:, None] & 1) + (np.arange(w)[None, :] & 1)
    b = np.asarray(black, np.int64)[pos]
    e = np.maximum(a.astype(np.int64) - b, 0)
    e = (e * radial_g(h, w, cx2, cy2, table) + 2048) >> 12
    return np.minimum(e + b, maxv(a.dtype)).astype(a.dtype)


def finish(frame, crop, orientation):
    """crop = (y, x, h, w) or None"""
    a = np.asarray(frame)
    if crop is not None:
        y, x, ch, cw = crop
        assert 0 <= y and 0 <= x and ch >= 1 and cw >= 1 and y + ch <= a.shape[0] and x + cw <= a.shape[1]
        a = a[y:y + ch, x:x + cw]
    return np.ascontiguousarray(ORIENT[orientation](a))


def gain_error_bound(k, h, w, cx2, cy2, centre_exact=False):
    """An upper bound on |g_quantised / 4096 - g(u)| over the sites of an H x W mosaic, for g(u) = 1 + k0 u + ... + k4 u^5 whose
    table holds round-half-up(4096 g(i / 1024)) without the clamp at 65535, u taken about the EXACT centre (within a quarter
    pixel per axis of (cx2 / 2, cy2 / 2)) and normalised by the exact farthest corner.  Derived, not measured:

      G1 = sum (i + 1) |k_i| >= max |g'|,  G2 = sum (i + 1) i |k_i| >= max |g''| on [0, 1]
      table spacing   linear interpolation between exact nodes 1 / 1024 apart:                      G2 / (8 * 1024^2)
      Q12 format      every node is within 2^-13 of g, a blend of two such nodes too; the blend's own rounding (+128 >> 8)
                      is another 2^-13:                                                              2^-12
      8-bit weight    mul >= 2^23 (the shift is the largest that keeps it below 2^24), so d2 (2^(18+s) / D - mul) / 2^s <=
                      D / 2^s <= 2^-5, and the floor loses less than 1: q is within 33/32 of 2^18 d2 / D, u within
                      (33/32) 2^-18.  The table's slope is at most G1 + 2 * 2^-13 * 1024 (rounded nodes):  (G1 + 1/4) (33/32) 2^-18
      half-pixel centre   the centre moves by at most delta = sqrt(2) / 4 pixel, so the distance d of a site and the
                      normalising distance R change by at most delta each: |d'/R' - d/R| <= (delta R + d delta) / (R R') <=
                      2 delta / R', and |u' - u| <= 2 * that (both roots are at most 1).  With R' = sqrt(D) / 2 pixels:
                      |u' - u| <= 2 sqrt(2) / sqrt(D):                                              G1 * 2 sqrt(2) / sqrt(D)
                      (`centre_exact`: the centre lies on the half-pixel grid and this term is 0)
    """
    k = [abs(float(v)) for v in k]
    g1 = sum((i + 1) * k[i] for i in range(5))
    g2 = sum((i + 1) * i * k[i] for i in range(5))
    D = d2max(h, w, cx2, cy2)
    centre = 0.0 if centre_exact else g1 * 2.0 * 2.0 ** 0.5 / float(D) ** 0.5
    return g2 / (8.0 * 1024.0 ** 2) + 2.0 ** -12 + (g1 + 0.25) * (33.0 / 32.0) * 2.0 ** -18 + centre
