"""The calibration cases shared by test_calib_host.py (CPU: the cases mean something) and test_gpu_calib.py (GPU: the kernels
equal the restatement on them).  Seeded inputs; every reference is computed once and shared.

Shapes, against the calibration kernel's geometry (demosaic.calib_vec: a lane's 16-byte window is V = 8 sites at uint16, 16 at
uint8; demosaic.calib_tile: a workgroup is 4 rows of 64 windows) and the master kernel's 4 sites per thread:
  * demosaic_cases.TINY: 2x2, 2x3, 3x2, 3x3 and two rows / two columns across a tile -- and the same across THIS kernel's tile
  * widths V - 1, V, V + 1 and 2 V + 1 at an even and an odd height: rows that start off the 16-byte boundary, a partial
    first and last window, site counts that are no multiple of 4
  * one workgroup tile minus, exactly and plus one site in both directions
  * demosaic_cases.RAGGED (53 x 391)"""
import functools

import numpy as np

import calib_restatement as C
from demosaic_cases import DTYPES, RAGGED, TINY, random_mosaic  # noqa: F401  (re-exported)
from shinestacker_amd import demosaic as D


def shapes(dtype):
    v = D.calib_vec(dtype)
    th, tw = D.calib_tile(dtype)
    out = list(TINY) + [(2, tw + 3), (th + 3, 2)]
    out += [(h, w) for h in (4, 5) for w in (v - 1, v, v + 1, 2 * v + 1)]
    out += [(h, w) for h in (th - 1, th, th + 1) for w in (tw - 1, tw, tw + 1)]
    out.append(RAGGED)
    return list(dict.fromkeys(out))


def maxv(dtype):
    return int(np.iinfo(dtype).max)


def black_per_position(dtype):
    mx = maxv(dtype)
    return [mx // 16, mx // 32, mx // 24, mx // 10]


# ---------------------------------------------------------------------------------------------- masters
KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)


def rejects(k):
    """0, 1 where allowed, the median's (k - 1) // 2 and one value between"""
    med = (k - 1) // 2
    r = {0, med}
    if 2 * 1 < k:
        r.add(1)
    if med >= 3:
        r.add((1 + med) // 2)
    return sorted(r)


MASTER_CASES = [(k, r) for k in KS for r in rejects(k)]
SMALL_ODD = (3, 3)              # 9 sites: the per-sample path of the master kernel, a ragged last thread


@functools.lru_cache(maxsize=None)
def random_frames(shape, dtype, k):
    """k full-range random exposures"""
    return tuple(random_mosaic(shape, dtype, salt=100 + i) for i in range(k))


@functools.lru_cache(maxsize=None)
def outlier_frames(shape, dtype, k=9):
    """k exposures of a quiet scene (a base plus -3 .. 3 of noise, away from both ends of the range); frames 2 and 5 carry maxv
    at a seeded 3 % of the sites each (a cosmic-ray hit): (frames, the quiet frames, the two masks)"""
    mx = maxv(dtype)
    rng = np.random.default_rng([shape[0], shape[1], np.dtype(dtype).itemsize, k, 7])
    base = rng.integers(mx // 8, mx // 2, size=shape, dtype=np.int64)
    quiet = [(base + rng.integers(-3, 4, size=shape)).astype(dtype) for _ in range(k)]
    frames, masks = [q.copy() for q in quiet], []
    for j in (2, 5):
        mask = rng.random(shape) < 0.03
        frames[j][mask] = mx
        masks.append(mask)
    for a in frames + quiet:
        a.setflags(write=False)
    return tuple(frames), tuple(quiet), tuple(masks)


def identical_frames(shape, dtype, k=8):
    return (random_mosaic(shape, dtype, salt=55),) * k


def saturated_frames(shape, dtype, k=16):
    full = np.full(shape, maxv(dtype), dtype)
    full.setflags(write=False)
    return (full,) * k


def special_master_sets(dtype):
    """(name, frames, reject) at the ragged shape"""
    out = []
    frames = outlier_frames(RAGGED, dtype)[0]
    for r in (0, 1, 2, 4):
        out.append((f"outliers, reject {r}", frames, r))
    for r in (0, 1, 3):
        out.append((f"identical frames, reject {r}", identical_frames(RAGGED, dtype), r))
    for r in (0, 7):
        out.append((f"all samples maxv, reject {r}", saturated_frames(RAGGED, dtype), r))
    return out


@functools.lru_cache(maxsize=None)
def master_reference(shape, dtype, k, reject):
    out = C.master(random_frames(shape, dtype, k), reject)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------- flats
RESPONSE = (0.55, 0.9, 0.85, 0.4)        # per cell position: the colour of the lamp through the filters


@functools.lru_cache(maxsize=None)
def falloff_flat(shape, dtype, black=(0, 0, 0, 0)):
    """a real flat: a smooth fall-off (1 at the centre, 0.27 in the corners, mean about 0.76) times a per-position colour
    response, 1 % of noise, on the black pedestal; the signal stays above zero and below the maximum everywhere"""
    mx = maxv(dtype)
    h, w = shape
    y, x = np.indices(shape).astype(np.float64)
    r2 = (((y - (h - 1) / 2) / max((h - 1) / 2, 1)) ** 2 + ((x - (w - 1) / 2) / max((w - 1) / 2, 1)) ** 2) / 2
    rng = np.random.default_rng([h, w, np.dtype(dtype).itemsize, 11])
    level = 0.8 * (mx - max(black)) * (1 - 0.73 * r2) * (1 + 0.01 * rng.standard_normal(shape))
    resp = np.asarray(RESPONSE)[C.position_map(shape)]
    f = np.maximum(np.floor(level * resp), 3).astype(np.int64) + C.black_map(shape, black)
    assert f.max() <= mx
    out = f.astype(dtype)
    out.setflags(write=False)
    return out


def flat_cases(dtype, shape=RAGGED):
    """(name, flat, black, flat_dark or None)"""
    mx = maxv(dtype)
    rng = np.random.default_rng([shape[0], shape[1], np.dtype(dtype).itemsize, 13])
    bpp = tuple(black_per_position(dtype))
    plain = falloff_flat(shape, dtype)
    pedestal = falloff_flat(shape, dtype, bpp)
    bmap = C.black_map(shape, bpp)
    # sites equal to and below the black level: f = 0 there
    holes = pedestal.astype(np.int64)
    at, below = rng.random(shape) < 0.02, rng.random(shape) < 0.02
    holes[at] = bmap[at]
    holes[below] = bmap[below] // 2
    # every site at or below black: S_p = 0
    dead = np.minimum(bmap, rng.integers(0, mx // 8, size=shape))
    # a bright flat with a few nearly dark sites: the position's mean over 1, 2 or 3 counts is far above 4.0
    dusty = plain.astype(np.int64)
    specks = rng.random(shape) < 0.01
    dusty[specks] = rng.integers(1, 4, size=int(specks.sum()))
    # a flat-dark around the pedestal, above the flat at the flat's dark specks
    fdark = np.clip(bmap + rng.integers(-2, 3, size=shape), 0, mx)
    fdark_dusty = np.clip(rng.integers(0, 3, size=shape), 0, mx)
    cases = [
        ("plain", plain, (0, 0, 0, 0), None),
        ("plain, black per position", pedestal, bpp, None),
        ("plain, flat-dark", pedestal, bpp, fdark),
        ("plain, flat-dark, black 0 (the black level is not read)", pedestal, (0, 0, 0, 0), fdark),
        ("sites at and below black", holes, bpp, None),
        ("sites at and below the flat-dark", holes, bpp, fdark),
        ("all black", dead, bpp, None),
        ("all black under the flat-dark", np.minimum(dead, fdark), bpp, fdark),
        ("all zero", np.zeros(shape, np.int64), (0, 0, 0, 0), None),
        ("dark specks: the gain clamps", dusty, (0, 0, 0, 0), None),
        ("dark specks under a flat-dark: clamps and f = 0", dusty, (0, 0, 0, 0), fdark_dusty),
    ]
    return [(n, np.ascontiguousarray(f.astype(dtype)), b, None if fd is None else np.ascontiguousarray(fd.astype(dtype)))
            for n, f, b, fd in cases]


@functools.lru_cache(maxsize=None)
def falloff_gain(shape, dtype, black=(0, 0, 0, 0)):
    """the gain table of falloff_flat: what an ordinary session calibrates with"""
    g = C.flat_gain(falloff_flat(shape, dtype, black), black)
    g.setflags(write=False)
    return g


# ---------------------------------------------------------------------------------------------- calibrate
@functools.lru_cache(maxsize=None)
def ordinary_dark(shape, dtype):
    """a dark below maxv / 8"""
    rng = np.random.default_rng([shape[0], shape[1], np.dtype(dtype).itemsize, 17])
    d = rng.integers(0, maxv(dtype) // 8, size=shape, dtype=np.int64).astype(dtype)
    d.setflags(write=False)
    return d


def shape_cases(shape, dtype):
    """(name, mosaic, black, dark or None, gain or None) at one shape: dark only, flat only, both"""
    m = random_mosaic(shape, dtype, salt=3)
    bpp = tuple(black_per_position(dtype))
    d, g = ordinary_dark(shape, dtype), falloff_gain(shape, dtype, bpp)
    return [("dark", m, bpp, d, None), ("flat", m, bpp, None, g), ("dark and flat", m, bpp, d, g)]


def option_cases(dtype, shape=RAGGED):
    """(name, mosaic, black, dark or None, gain or None): the corrections' edge cases at the ragged shape"""
    mx = maxv(dtype)
    rng = np.random.default_rng([shape[0], shape[1], np.dtype(dtype).itemsize, 19])
    m = random_mosaic(shape, dtype, salt=3)
    bpp = tuple(black_per_position(dtype))
    high = (mx // 4, mx // 3, mx // 5, mx // 2)              # a black above many samples
    d, g0, g = ordinary_dark(shape, dtype), falloff_gain(shape, dtype), falloff_gain(shape, dtype, bpp)
    wild_dark = random_mosaic(shape, dtype, salt=4)          # above the sample at half the sites
    big_gain = rng.choice(np.array([65535, 40000, 16384, 20000], np.uint16), size=shape)
    zero_gain = np.where(rng.random(shape) < 0.5, 0, 1).astype(np.uint16)
    full, zero = np.full(shape, mx, dtype), np.zeros(shape, dtype)
    return [
        ("ordinary: dark and flat, black 0", m, (0, 0, 0, 0), d, g0),
        ("neither", m, bpp, None, None),
        ("black per position, dark", m, bpp, d, None),
        ("black per position, flat", m, bpp, None, g),
        ("black per position, both", m, bpp, d, g),
        ("black above some samples, flat", m, high, None, g),
        ("black above some samples, both", m, high, d, g),
        ("dark above the sample", m, bpp, wild_dark, None),
        ("dark above the sample, flat", m, bpp, wild_dark, g),
        ("gain past maxv", m, bpp, None, big_gain),
        ("gain past maxv, dark", m, bpp, d, big_gain),
        ("gains 0 and 1", m, bpp, None, zero_gain),
        ("all zero", zero, bpp, d, g),
        ("all maxv", full, bpp, d, g),
        ("all maxv, dark 0, gain 65535", full, (0, 0, 0, 0), zero, np.full(shape, 65535, np.uint16)),
    ]


def restate(mosaic, black, dark, gain):
    return C.calibrate(mosaic, black, dark, gain)
