"""The cases the depth map's weighted smoothing (csrc/kernels_depth.hpp) is run at beyond the files it arrived with: the
shape / sigma table, the value and weight planes, the restatement's results for them (computed once per process, read-only)
and what the restatement's own B(w) says about every case.  A plain module shared by test_depth_outputs_cases_host.py, which
checks that no case is vacuous, and test_gpu_depth_outputs_edges.py, which holds the kernels to the restatement.  NumPy only,
seeded, no device.

Shapes: a row pass workgroup owns MI_WS_SEG = 256 pixels and stages 256 + 2 radius of them, the column pass workgroup owns 64
columns x 32 rows, a lane 8 rows.  (49, 255 .. 257): one segment, exactly one, one pixel into a second, each with the widest
halo (48) the height allows; (49, 304): the second segment is as wide as the halo, (49, 305) one more; (70, 49): the radius at
the width's limit; (31 .. 33, 70) and (63 .. 65, 70): heights below, on and above one and two column workgroups, with the
largest radius that fits; (5, 513): three segments, the last one pixel wide, a small radius."""
import functools
from collections import namedtuple

import numpy as np

import depth_restatement as dr

SEG = 256               # MI_WS_SEG
COL_ROWS = 32           # rows of a column-pass workgroup
MAX_PIXELS = 1025 * 70

SmoothCase = namedtuple("SmoothCase", "shape sigma radius")

TABLE = ([SmoothCase((49, w), 16.0, 48) for w in (255, 256, 257, 304, 305)] + [SmoothCase((70, 49), 16.0, 48)] +
         [SmoothCase((h, 70), 10.0, 30) for h in (31, 32, 33)] + [SmoothCase((h, 70), 16.0, 48) for h in (63, 64, 65)] +
         [SmoothCase((5, 513), 0.5, 2)])
WORK_TYPES = [np.float32, np.float64]
VALUE_KINDS = ["int32", "floating"]
WEIGHT_KINDS = ["positive", "mixed", "special"]


def case_name(c):
    return "%dx%d sigma %g" % (c.shape + (c.sigma,))


def seed_of(shape):
    return 7 + shape[0] * 1000 + shape[1]


@functools.lru_cache(maxsize=None)
def value_plane(shape, kind, work):
    """int32 frame indices 0 .. 12, or the same plus a quarter in the working type"""
    rng = np.random.default_rng(seed_of(shape))
    v = rng.integers(0, 13, shape).astype(np.int32)
    if kind == "floating":
        v = (v.astype(work) + np.dtype(work).type(0.25)).astype(work)
    v.setflags(write=False)
    return v


def special_sites(shape, radius):
    """{name: (y, x)}: where the `special` weight plane holds -0.0, NaN and +inf.  A NaN weight makes B(w) NaN over its whole
    window, where the output is the value itself; a +inf weight makes B(v w) / B(w) = inf / inf = NaN over its whole window.
    At radius 2 both stand alone in mid-plane (the +inf makes 25 NaN samples).  At the large radii a window is most of the
    plane, so both sit in the first row: the NaN in column 1, the +inf in column 2 of the planes of two segments -- the NaN's
    window covers all of the +inf's but its last column, 49 samples -- and in column 0 of the narrow planes, where even one
    column would be more than 1 % of the samples: there the NaN's window covers the +inf's altogether."""
    h, w = shape
    if radius <= 2:
        return {"-0 a": (0, 0), "-0 b": (h - 1, w - 1), "-0 c": (h // 2, w // 3), "nan": (h // 2, (2 * w) // 3), "inf": (2, w // 5)}
    return {"-0 a": (0, 3), "-0 b": (h - 1, w - 1), "-0 c": (h // 2, w - 1 - w // 3), "nan": (0, 1), "inf": (0, 2) if w >= 255 else (0, 0)}


@functools.lru_cache(maxsize=None)
def weight_plane(shape, radius, kind, work):
    """positive: energies in [0, 50); mixed: the same with the sign of a wavy left / right split, so that the blurred weight is
    positive on one side and negative on the other; special: positive with isolated -0.0, NaN and +inf"""
    h, w = shape
    rng = np.random.default_rng(seed_of(shape) + 1)
    wt = (rng.random(shape) * 50.0).astype(work)
    if kind == "mixed":
        y, x = np.mgrid[:h, :w]
        wt = np.where(x < w / 2.0 + 3.0 * np.sin(y / 3.0), wt, -wt).astype(work)
    elif kind == "special":
        s = special_sites(shape, radius)
        for name, at in s.items():
            wt[at] = {"-": -0.0, "n": np.nan, "i": np.inf}[name[0]]
    else:
        assert kind == "positive"
    wt.setflags(write=False)
    return wt


@functools.lru_cache(maxsize=None)
def blurred_weight(c, kind, work):
    """the restatement's B(w) in the working type"""
    with np.errstate(all="ignore"):
        out = dr.blur(np.asarray(weight_plane(c.shape, c.radius, kind, work)), dr.taps_of(c.sigma, work))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(c, value_kind, weight_kind, work):
    with np.errstate(all="ignore"):
        out = dr.weighted_smooth(value_plane(c.shape, value_kind, work), weight_plane(c.shape, c.radius, weight_kind, work), c.sigma,
                                 work)
    assert out.dtype == np.float32 and out.shape == c.shape
    out.setflags(write=False)
    return out


def runs():
    """every (case, value kind, weight kind, working type)"""
    return [(c, vk, wk, wt) for c in TABLE for wt in WORK_TYPES for vk in VALUE_KINDS for wk in WEIGHT_KINDS]


def same_but_nan(got, want):
    """bit for bit wherever `want` is not NaN, NaN wherever it is (an x86 NaN and a gfx950 NaN differ in the sign bit)"""
    nan = np.isnan(want)
    return (got.dtype == want.dtype and got.shape == want.shape and np.array_equal(np.isnan(got), nan) and
            got[~nan].tobytes() == want[~nan].tobytes())


# ---------------------------------------------------------------- the unweighted path: DepthMapStack(map_type="max")
MAX_MAP_SHAPE = (50, 300)       # two row segments, radius 48 fits
MAX_MAP_SIGMAS = [16.0, 2.0]


@functools.lru_cache(maxsize=None)
def max_map_frames(n=3):
    """`n` uint8 frames, each sharp (noise) in its own third of the width and smooth elsewhere"""
    h, w = MAX_MAP_SHAPE
    rng = np.random.default_rng(31)
    y, x = np.mgrid[:h, :w]
    out = []
    for i in range(n):
        smooth = 120.0 + 50.0 * np.sin(x / 23.0 + i) * np.cos(y / 17.0)
        noise = rng.integers(-60, 61, (h, w, 3))
        sharp = ((x * n) // w == i)[:, :, None]
        fr = np.clip(np.rint(smooth)[:, :, None] + np.where(sharp, noise, noise // 20), 0, 255).astype(np.uint8)
        fr.setflags(write=False)
        out.append(fr)
    return tuple(out)
