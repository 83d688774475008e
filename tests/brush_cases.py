"""The strokes the brush kernel's ordered compaction (csrc/kernels_brush.hpp) is run at beyond the file it arrived with.  A
workgroup walks the stamp list in blocks of 256, a stamp per thread, appends a block's hits on its 64 x 16 tile to an LDS list
of MI_BR_CAP = 512 entries in stroke order -- a ballot ranks a hit inside its wave of 64, four wave counts give the wave's offset
-- and folds the list when it holds more than 256 entries or the stamps are used up.  Two kinds of case: stamp lists that all
hit one tile, with hit counts on either side of those limits, and one long stroke over several tiles, each of which takes a
ragged share of several blocks.  Flow 7 and a low opacity keep the mask from saturating, so the order of the adds shows.  A
plain module shared by test_depth_outputs_cases_host.py and test_gpu_depth_outputs_edges.py.  NumPy only, seeded, no device."""
import functools
import math

import numpy as np

import brush_restatement as br

TW, TH = 64, 16         # MI_BR_TW, MI_BR_TH
BLOCK = 256             # stamps per block of the cull
WAVE = 64
DTYPES = [np.uint8, np.uint16]
MAX_RADIUS = 65

# ---------------------------------------------------------------- one tile, hit counts at the chunk limits
ONE_TILE_SHAPE = (TH, TW)
ONE_TILE_BRUSH = (131, 20, 0.9, 7)              # size (radius 65 >= the tile's extent), hardness, opacity, flow
HIT_COUNTS = [255, 256, 257, 511, 512, 513, 769]

# ---------------------------------------------------------------- one stroke over several tiles
RAGGED_SHAPE = (56, 200)
RAGGED_BRUSH = (21, 30, 30, 7)                  # radius 10
RAGGED_STAMPS = 900


@functools.lru_cache(maxsize=None)
def frames(shape, dtype, seed=0):
    rng = np.random.default_rng(300 + seed)
    hi = np.iinfo(dtype).max + 1
    out = rng.integers(0, hi, shape + (3,)).astype(dtype), rng.integers(0, hi, shape + (3,)).astype(dtype)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def one_tile_points(n):
    """`n` positions inside the tile, some on half-way coordinates: every square of radius 65 holds the whole tile"""
    rng = np.random.default_rng(n)
    xs = rng.integers(20, 44, n) + rng.integers(0, 2, n) * 0.5
    ys = rng.integers(0, TH, n)
    return tuple((float(x), float(y)) for x, y in zip(xs, ys))


@functools.lru_cache(maxsize=None)
def ragged_points():
    """a Lissajous walk over the whole frame and a little past its edges, with a seeded jitter of half pixels"""
    h, w = RAGGED_SHAPE
    rng = np.random.default_rng(77)
    t = np.linspace(0.0, 2.0 * math.pi, RAGGED_STAMPS)
    xs = w / 2.0 + (w / 2.0 + 3.0) * np.sin(3.0 * t) + rng.integers(-2, 3, RAGGED_STAMPS) * 0.5
    ys = h / 2.0 + (h / 2.0 + 2.0) * np.sin(4.0 * t + 0.7) + rng.integers(-2, 3, RAGGED_STAMPS) * 0.5
    return tuple(zip(xs.tolist(), ys.tolist()))


def shuffled(points, seed=9):
    return tuple(points[i] for i in np.random.default_rng(seed).permutation(len(points)))


def table_of(brush):
    """the stamp table without the flow (brush_restatement's strokes apply it): the package's brush_mask, which the CPU tests of
    the brush hold to tables recorded from the reference"""
    from shinestacker_amd import retouch
    size, hardness, opacity, _flow = brush
    return retouch.brush_mask(2 * br.radius_of(size) + 1, hardness, opacity)


@functools.lru_cache(maxsize=None)
def expected(shape, dtype, points, brush):
    """brush_restatement.stroke_fold: (frame, mask layer, area)"""
    master, source = frames(shape, dtype)
    size, _hardness, opacity, flow = brush
    out, layer, area = br.stroke_fold(master, source, table_of(brush), br.centres(points), br.radius_of(size), opacity, flow)
    out.setflags(write=False)
    layer.setflags(write=False)
    return out, layer, tuple(area)


def stroke_box(stamps, radius, shape):
    """the union of the footprints that meet the frame: where the launch's tiles start"""
    fps = [fp for fp in (br.footprint(cx, cy, radius, shape[0], shape[1]) for cx, cy in stamps) if fp is not None]
    return (min(f[0] for f in fps), min(f[1] for f in fps), max(f[2] for f in fps), max(f[3] for f in fps))


def tile_hits(stamps, radius, shape):
    """hits[ty, tx, block, wave]: how many stamps of that wave of 64 of that block of 256 have a square that meets the tile
    (the kernel's cull test, on the tiles of the stroke's box)"""
    x0, y0, x1, y1 = stroke_box(stamps, radius, shape)
    nx, ny = -(-(x1 - x0) // TW), -(-(y1 - y0) // TH)
    nb = -(-len(stamps) // BLOCK)
    hits = np.zeros((ny, nx, nb, BLOCK // WAVE), np.int64)
    for i, (cx, cy) in enumerate(stamps):
        for ty in range(ny):
            ty0 = y0 + ty * TH
            ty1 = min(ty0 + TH, y1)
            if not (cy + radius >= ty0 and cy - radius < ty1):
                continue
            for tx in range(nx):
                tx0 = x0 + tx * TW
                tx1 = min(tx0 + TW, x1)
                if cx + radius >= tx0 and cx - radius < tx1:
                    hits[ty, tx, i // BLOCK, (i % BLOCK) // WAVE] += 1
    return hits
