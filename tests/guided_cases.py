"""The cases the depth refinement (csrc/kernels_guided.hpp) is run at: the table, the planes, the restatement's results for them
(computed once per process, read-only) and a predictor of the kernel paths a case reaches.  A plain module shared by
test_guided_host.py, which checks that no case is vacuous and every path is reached, and test_gpu_guided.py, which holds the
kernels to the restatement.  NumPy only, seeded, no device.

The grid comes from the kernels' constants: a row pass workgroup owns SEG = 512 pixels of one row (a lane two neighbours, stored
as one 16-byte pair where the address is even, else as two values; an odd last pixel alone) and stages SEG + 2 radius of them;
a column pass workgroup owns COL_W = 64 columns x COL_H = 32 rows, a lane ROWS = 8 rows."""
import functools
from collections import namedtuple

import numpy as np

import guided_restatement as gr

SEG = 512               # MI_GF_SEG
ROWS = 8                # MI_GF_ROWS
COL_W = 64              # columns of a column-pass workgroup: one wave wide
COL_H = 4 * ROWS        # rows of a column-pass workgroup: four waves
MAX_RADIUS = 32         # MI_GF_MAX_RADIUS
EPS = 1e-4

GuidedCase = namedtuple("GuidedCase", "shape radius guide weight gkind wkind clamp")


def _c(shape, radius, guide=np.uint8, weight=np.float32, gkind="random", wkind="random", clamp="full"):
    return GuidedCase(tuple(shape), radius, guide, weight, gkind, wkind, clamp)


NARROW = (4.0, 8.0)     # inside the data's 0 .. 12.5
BLOCK = (slice(10, 50), slice(20, 70))      # the zero-weight block of the 70 x 90 cases: 40 x 50, a radius-6 window is 13 x 13

TABLE = (
    # frames smaller than anything: one pixel, one row, one column, a window larger than the frame
    [_c((1, 1), 1), _c((1, 70), 2, np.uint16), _c((70, 1), 2, weight=np.float64), _c((5, 7), 32), _c((5, 7), 32, np.uint16, np.float64)] +
    # the row passes' segments: one pixel short of the grid, on it, one past it; one, two and three segments
    [_c((3, w), 6) for w in (SEG - 1, SEG, SEG + 1)] +
    [_c((3, w), 32, np.uint16, np.float64) for w in (2 * SEG - 1, 2 * SEG, 2 * SEG + 1)] + [_c((2, 3 * SEG + 1), 1)] +
    # the column passes' workgroups, sideways and downwards
    [_c((9, w), 2, np.uint16) for w in (COL_W - 1, COL_W, COL_W + 1)] +
    [_c((h, 70), 6, weight=np.float64) for h in (COL_H - 1, COL_H, COL_H + 1)] +
    [_c((h, 66), 32) for h in (3 * COL_H - 1, 3 * COL_H, 3 * COL_H + 1)] +
    # every radius the issue names, both guide types, both weight types
    [_c((40, 75), r, g, w) for r in (1, 2, 6, 32) for g, w in ((np.uint8, np.float64), (np.uint16, np.float32))] +
    # contents
    [_c((70, 90), 6, gkind="constant"), _c((70, 90), 6, np.uint16, np.float64, gkind="constant"),
     _c((70, 90), 6, wkind="zero block"), _c((70, 90), 6, np.uint16, np.float64, wkind="zero block"),
     _c((70, 90), 6, wkind="zero"), _c((70, 90), 6, np.uint16, np.float64, wkind="zero"),
     _c((70, 90), 6, clamp="narrow"), _c((70, 90), 2, np.uint16, clamp="narrow"),
     _c((70, 90), 6, wkind="span"), _c((70, 90), 6, np.uint16, np.float64, wkind="span")])


def case_name(c):
    return "%dx%d r%d %s %s %s/%s/%s" % (c.shape + (c.radius, np.dtype(c.guide).name, np.dtype(c.weight).name, c.gkind, c.wkind,
                                                    c.clamp))


def seed_of(shape):
    return 11 + shape[0] * 4099 + shape[1]


@functools.lru_cache(maxsize=None)
def depth_plane(shape):
    """float32 frame numbers 0 .. 12.5: a step across the middle column, noise on top"""
    h, w = shape
    rng = np.random.default_rng(seed_of(shape))
    x = np.arange(w)[None, :]
    p = np.where(x < w / 2.0, 3.0, 9.0) + rng.integers(-3, 4, shape) + rng.random(shape) * 0.5
    p = p.astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def guide_frame(shape, dtype, kind):
    """BGR: dark left of the middle column and bright right of it with noise in every channel, or one colour everywhere"""
    h, w = shape
    top = 255 if np.dtype(dtype) == np.uint8 else 65535
    if kind == "constant":
        g = np.empty(shape + (3,), dtype)
        g[:] = np.array([0.2 * top, 0.5 * top, 0.7 * top]).astype(dtype)
    else:
        assert kind == "random"
        rng = np.random.default_rng(seed_of(shape) + 1)
        x = np.arange(w)[None, :, None]
        v = np.where(x < w / 2.0, 0.25, 0.75) + rng.normal(0.0, 0.08, shape + (3,))
        g = np.rint(np.clip(v, 0.0, 1.0) * top).astype(dtype)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def weight_plane(shape, dtype, kind):
    """random: energies in [0.5, 50); zero block: the same with BLOCK zeroed; zero: none anywhere; span: 10^u, u in [-6, 6]"""
    rng = np.random.default_rng(seed_of(shape) + 2)
    if kind == "zero":
        wt = np.zeros(shape, dtype)
    elif kind == "span":
        wt = (10.0 ** rng.uniform(-6.0, 6.0, shape)).astype(dtype)
    else:
        wt = (0.5 + rng.random(shape) * 49.5).astype(dtype)
        if kind == "zero block":
            wt[BLOCK] = 0
        else:
            assert kind == "random"
    wt.setflags(write=False)
    return wt


def limits(c):
    """(lo, hi) of the clamp: the data's own range, or NARROW"""
    if c.clamp == "narrow":
        return NARROW
    assert c.clamp == "full"
    p = depth_plane(c.shape)
    return float(p.min()), float(p.max())


def planes(c):
    return depth_plane(c.shape), weight_plane(c.shape, c.weight, c.wkind), guide_frame(c.shape, c.guide, c.gkind)


@functools.lru_cache(maxsize=None)
def expected(c):
    p, w, g = planes(c)
    lo, hi = limits(c)
    out = gr.guided_refine(p, w, g, c.radius, EPS, lo, hi)
    assert out.dtype == np.float32 and out.shape == c.shape
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- which kernel paths a case reaches
def _tiles(n, size, name):
    """the positions of the tiles of `size` along an axis of `n`: a lone tile is first and last at once"""
    k = -(-n // size)
    out = {name + " first", name + " last"}
    if k >= 3:
        out.add(name + " interior")
    if k >= 2:
        out.add(name + " several")
    return out


def _clips(n, r, name):
    """how the windows along an axis of `n` are clipped: not at all, on one side, on both"""
    i = np.arange(n)
    left, right = i - r < 0, i + r > n - 1
    out = set()
    if (~left & ~right).any():
        out.add(name + " window whole")
    if (left ^ right).any():
        out.add(name + " window clipped on one side")
    if (left & right).any():
        out.add(name + " window clipped on both sides")
    return out


def paths(c):
    """the names of the kernel paths the case reaches, predicted from its shape and options alone"""
    h, w = c.shape
    out = _tiles(w, SEG, "row tile") | _tiles(w, COL_W, "column tile across") | _tiles(h, COL_H, "column tile down")
    out |= _clips(w, c.radius, "row") | _clips(h, c.radius, "column")
    # the row passes' stores: row * w + x is even for every pair of an even row; an odd width makes odd rows start odd
    if w >= 2:
        out.add("store pair")
        if w % 2 and h >= 2:
            out.add("store split")
    if w % 2:
        out.add("store single")
    if h % ROWS:
        out.add("lane rows ragged")
    if h >= ROWS:
        out.add("lane rows full")
    if c.wkind == "zero" or (c.wkind == "zero block" and 2 * c.radius + 1 < min(BLOCK[0].stop - BLOCK[0].start,
                                                                                BLOCK[1].stop - BLOCK[1].start)):
        out.add("sw == 0")
    if c.wkind != "zero":
        out.add("sw > 0")
    out.add("guide " + np.dtype(c.guide).name)
    out.add("weight " + np.dtype(c.weight).name)
    return out


ALL_PATHS = ({"%s %s" % (t, k) for t in ("row tile", "column tile across", "column tile down")
              for k in ("first", "last", "interior", "several")} |
             {"%s window %s" % (a, k) for a in ("row", "column") for k in ("whole", "clipped on one side", "clipped on both sides")} |
             {"store pair", "store split", "store single", "lane rows ragged", "lane rows full", "sw == 0", "sw > 0",
              "guide uint8", "guide uint16", "weight float32", "weight float64"})
