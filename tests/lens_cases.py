"""The lens cases shared by test_lens_host.py (CPU: the cases mean something) and test_gpu_lens.py (GPU: the kernel equals the
restatement on them).  Seeded inputs; every reference is computed once and shared.

Shapes, against the kernel's geometry (lens.TILE_H x lens.TILE_W = 16 x 64 destination pixels per workgroup, one pixel per
thread and row step, four row steps per thread; no per-thread vector, no staged tile: ONE kernel path, direct gathers.  Inside
it the two taps of a source row come in together or one by one, pixel by pixel -- `tap_loads` predicts which, and
test_lens_host.py asserts that every way occurs):
  * 1 x 1 (a 3-byte image: no dword tap), a single row, a single column, 2 x 2, 3 x 5, 33 x 47
  * one pixel under, on and over the tile's edge in both directions: 15 / 16 / 17 rows by 63 / 64 / 65 columns
  * 35 x 130: three tiles by three, so interior, edge and corner workgroups all occur"""
import functools

import numpy as np

import lens_restatement as R
from shinestacker_amd import lens as L

DTYPES = (np.uint8, np.uint16)
TILE_H, TILE_W = L.TILE_H, L.TILE_W
SMALL = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (33, 47)]
EDGES = [(h, w) for h in (TILE_H - 1, TILE_H, TILE_H + 1) for w in (TILE_W - 1, TILE_W, TILE_W + 1)]
SHAPES = SMALL + EDGES + [(2 * TILE_H + 3, 2 * TILE_W + 2)]

LENSES = {
    "identity": (1, 0, 0, 0),
    "barrel": (1, -0.12, 0.02, 0),
    "pincushion": (0.93, 0.08, -0.03, 0.01),
    "outward": (1, 0.1, 0, 0),                                       # its corners leave the frame
    "CA": ((0.97, 0.02, 0, 0), (1, 0, 0, 0), (1.03, -0.01, 0, 0)),   # B, G, R; exaggerated: a real 0.1 % moves < 1/64 pixel here
    "mixed": ((1.002, -0.1, 0.03, 0), (1, -0.1, 0.03, 0), (0.998, -0.1, 0.03, 0)),
    "zoom-out": (3, 0, 0, 0),                                        # almost everything clamps
    "collapse": (0, 0, 0, 0),                                        # every pixel reads the centre
}
CENTRES = ("default", "off")
FRAMES = ("random", "saturated", "ramp")


def maxv(dtype):
    return int(np.iinfo(dtype).max)


def centre(kind, shape):
    """None (the middle of the frame) or (0.3 (w - 1), 0.8 (h - 1))"""
    h, w = shape
    return None if kind == "default" else (0.3 * (w - 1), 0.8 * (h - 1))


def lens_of(name, kind, shape):
    """the package's Lens of a case"""
    return L.Lens(LENSES[name], centre(kind, shape))


@functools.lru_cache(maxsize=None)
def frame(kind, shape, dtype):
    h, w = shape
    if kind == "random":        # full range
        rng = np.random.default_rng([h, w, np.dtype(dtype).itemsize, 23])
        f = rng.integers(0, maxv(dtype) + 1, size=(h, w, 3), dtype=np.int64).astype(dtype)
    elif kind == "saturated":
        f = np.full((h, w, 3), maxv(dtype), dtype)
    else:                       # a ramp along both axes, another slope per plane, ending at the maximum
        y, x = np.indices((h, w)).astype(np.float64)
        t = (x + y) / max(h + w - 2, 1)
        f = np.stack([np.floor(maxv(dtype) * t ** p) for p in (1.0, 0.5, 2.0)], axis=-1).astype(dtype)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(name, kind, frame_kind, shape, dtype):
    """(remapped frame, mask) of a case by the restatement"""
    out, mask = R.remap(frame(frame_kind, shape, dtype), LENSES[name], centre(kind, shape), return_mask=True)
    out.setflags(write=False)
    mask.setflags(write=False)
    return out, mask


TAP_LOADS = ("pair", "clamped", "buffer end", "last pixel")


def tap_loads(name, kind, shape, dtype=np.uint8):
    """The ways the two taps of a source row reach the kernel in a case whose planes share their coefficients
    (lens_row_taps of csrc/kernels_lens.hpp): "pair" -- neighbours in memory, one load of 8 bytes (12 at 16 bits); "clamped" --
    the same pixel twice, at the frame's sides; and at 8 bits only: "buffer end" -- neighbours, but the 8-byte load would leave
    the buffer (it starts in one of the image's last two pixels); "last pixel" -- a tap on the image's last pixel, read byte by
    byte.  (At 16 bits a pair's 12 bytes end with the second tap and a single tap's loads with the tap.)"""
    h, w = shape
    k = R.planes(LENSES[name])
    assert (k == k[0]).all(), "the planes of this lens have their own coordinates"
    X, Y = R.positions(h, w, k[0], centre(kind, shape))
    sx, sy = X >> 5, Y >> 5
    x0, x1 = np.clip(sx, 0, w - 1), np.clip(sx + 1, 0, w - 1)
    last = h * w - 1
    seen = set()
    for row in (np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)):
        p0, p1 = row * w + x0, row * w + x1
        neighbours = x1 == x0 + 1
        if np.dtype(dtype).itemsize == 2:
            ways = (("pair", neighbours), ("clamped", ~neighbours))
        else:
            together = neighbours & (p0 + 2 <= last)
            ways = (("pair", together), ("clamped", ~neighbours), ("buffer end", neighbours & ~together),
                    ("last pixel", ~together & ((p0 == last) | (p1 == last))))
        for label, hit in ways:
            if hit.any():
                seen.add(label)
    return seen


SAMPLE_LOADS = ("dword", "apart")


def sample_loads(name, kind, shape):
    """The ways a plane's two samples of a source row reach the kernel at 8 bits in a case whose planes have their own
    coordinates (lens_row_samples): "dword" -- the taps are neighbours, one load; "apart" -- clamped to one pixel, two byte
    loads.  (At 16 bits it is two loads either way; an identity plane is copied and has no taps.)"""
    h, w = shape
    k = R.planes(LENSES[name])
    assert not (k == k[0]).all(), "the planes of this lens share their coordinates"
    seen = set()
    for c in range(3):
        if tuple(k[c]) == R.IDENTITY:
            continue
        X, _ = R.positions(h, w, k[c], centre(kind, shape))
        sx = X >> 5
        neighbours = np.clip(sx + 1, 0, w - 1) == np.clip(sx, 0, w - 1) + 1
        seen |= ({"dword"} if neighbours.any() else set()) | ({"apart"} if (~neighbours).any() else set())
    return seen


# coefficients at the end of the float64 range: s overflows to inf, 0 * inf and inf - inf give NaN, and min / max must treat a
# NaN as C's fmin / fmax do (the other operand).  Not part of the case table: test_gpu_lens.py runs them on their own.
OVERFLOWING = {
    "huge": (1e308, 1e308, 1e308, 1e308),
    "huge, mixed signs": ((1e308, -1e308, 1e308, -1e308), (1, 0, 0, 0), (-1e308, 1e308, 1e308, 1e308)),
}


def cases(shape, dtype):
    """(lens name, centre kind, frame kind) of every case at one shape and dtype"""
    return [(n, c, f) for n in LENSES for c in CENTRES for f in FRAMES]
