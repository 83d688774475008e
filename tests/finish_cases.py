"""The cases shared by test_finish_host.py (CPU: every case means something, the parser reads what was written) and
test_gpu_finish.py (GPU: the kernels of csrc/kernels_finish.hpp equal tests/finish_restatement.py on them), the writers of the
opcode and the tags on top of dng_cases.write_dng, and a predictor of the kernel paths a case reaches.

Shapes against the kernels' geometry:
  mosaic_radial_gain  a workgroup is 4 rows of 64 lanes, a lane owns a 16-byte window of its row (8 uint16 / 16 uint8 sites),
                      aligned in memory: one workgroup spans 512 uint16 or 1024 uint8 sites of a row.  2 x 2 and 2 x N; a width one
                      below, at and one above that span; odd widths (rows off the 16-byte grid); the centre mid-frame, on a
                      corner, outside the frame; a gain that saturates, one below 1
  frame_finish        rows (orientations 1..4): a lane owns a 16-byte window of a destination row of 3 cw samples; transposing
                      (5..8): tiles of 32 x 32 pixels.  H != W; 1 x 1, one row, one column; 31 / 32 / 33 each way; a crop with an
                      odd origin, to 1 x 1, equal to the frame; a row of more than one workgroup
"""
import struct

import numpy as np

from dng_cases import rational

VEC_BYTES, LANES, TILE = 16, 64, 32


# ------------------------------------------------------------------------------------------------ writers
def fix_vignette_radial(k, centre):
    """(opcode id, data) of a FixVignetteRadial: k0..k4, cx, cy as big-endian doubles; for dng_cases.write_dng(opcodes3=[...])"""
    return 3, struct.pack(">7d", *(tuple(k) + tuple(centre)))


def default_crop(origin, size, typ=4):
    """DefaultCropOrigin / DefaultCropSize entries (horizontal, vertical) for write_dng(extra=...); typ 3 SHORT, 4 LONG, 5 RATIONAL"""
    conv = (lambda v: rational(v)) if typ == 5 else int
    return {50719: (typ, [conv(v) for v in origin]), 50720: (typ, [conv(v) for v in size])}


def default_scale(h, v):
    return {50718: (5, [rational(h), rational(v)])}


# ------------------------------------------------------------------------------------------------ radial-gain cases
VIG = (0.3, 0.1, 0.0, 0.0, 0.0)             # the tests' polynomial: 1 at the centre, 1.4 at the corner
VIG5 = (0.5, -0.3, 0.2, -0.1, 0.05)         # all five terms
VIG_DARKEN = (-0.5, 0.0, 0.0, 0.0, 0.0)     # below 1: 0.5 at the corner
VIG_SATURATE = (10.0, 0.0, 0.0, 0.0, 0.0)   # up to 11: full-range samples saturate


class RadialCase:
    def __init__(self, name, h, w, dtype, k=VIG, centre="mid", black=(0, 0, 0, 0)):
        self.name, self.h, self.w, self.dtype, self.k = name, h, w, np.dtype(dtype), k
        self.centre = {"mid": ((w - 1) / 2.0 + 0.3, (h - 1) / 2.0 - 0.2), "corner": (0.0, 0.0),
                       "outside": (-20.0, 2.0 * h + 30.0)}.get(centre, centre)
        self.black = tuple(black)

    def __repr__(self):
        return self.name

    def mosaic(self):
        """seeded, full range, with the extremes present"""
        top = int(np.iinfo(self.dtype).max)
        rng = np.random.default_rng([self.h, self.w, self.dtype.itemsize, 7])
        a = rng.integers(0, top + 1, size=(self.h, self.w), dtype=np.int64)
        a.flat[0], a.flat[-1] = top, 0
        return a.astype(self.dtype)


RADIAL_CASES = [
    RadialCase("u16-2x2", 2, 2, np.uint16),
    RadialCase("u8-2x2", 2, 2, np.uint8),
    RadialCase("u16-2x37", 2, 37, np.uint16, black=(256, 260, 258, 262)),
    RadialCase("u8-2x37", 2, 37, np.uint8, black=(16, 17, 18, 19)),
    RadialCase("u16-5x511-below-a-span", 5, 511, np.uint16, k=VIG5),
    RadialCase("u16-5x512-one-span", 5, 512, np.uint16, k=VIG5),
    RadialCase("u16-5x513-above-a-span", 5, 513, np.uint16, k=VIG5, black=(256, 256, 256, 256)),
    RadialCase("u8-5x1023-below-a-span", 5, 1023, np.uint8),
    RadialCase("u8-5x1024-one-span", 5, 1024, np.uint8),
    RadialCase("u8-5x1025-above-a-span", 5, 1025, np.uint8, black=(16, 16, 16, 16)),
    RadialCase("u16-9x37-rows-off-the-grid", 9, 37, np.uint16, black=(1024, 1024, 1024, 1024)),
    RadialCase("u8-9x37-rows-off-the-grid", 9, 37, np.uint8),
    RadialCase("u16-21x40-centre-on-a-corner", 21, 40, np.uint16, centre="corner"),
    RadialCase("u16-21x40-centre-outside", 21, 40, np.uint16, centre="outside", k=VIG5),
    RadialCase("u8-21x40-centre-outside", 21, 40, np.uint8, centre="outside"),
    RadialCase("u16-21x40-saturates", 21, 40, np.uint16, k=VIG_SATURATE, black=(256, 256, 256, 256)),
    RadialCase("u8-21x40-saturates", 21, 40, np.uint8, k=VIG_SATURATE),
    RadialCase("u16-21x40-darkens", 21, 40, np.uint16, k=VIG_DARKEN, black=(256, 260, 258, 262)),
    RadialCase("u8-21x40-darkens", 21, 40, np.uint8, k=VIG_DARKEN),
]

RADIAL_PATHS = ("whole", "partial", "misaligned row", "second workgroup")


def radial_paths(case, base=0):
    """the paths of mosaic_radial_gain a case reaches, from the geometry alone; `base`: the mosaic's first byte modulo 16"""
    item = case.dtype.itemsize
    V = VEC_BYTES // item
    seen = set()
    for y in range(case.h):
        off = ((base + y * case.w * item) % VEC_BYTES) // item
        if off:
            seen.add("misaligned row")
        for n, x0 in enumerate(range(-off, case.w, V)):
            seen.add("whole" if x0 >= 0 and x0 + V <= case.w else "partial")
            if n >= LANES:
                seen.add("second workgroup")
    return seen


# ------------------------------------------------------------------------------------------------ frame-finish cases
class FinishCase:
    def __init__(self, name, h, w, crop=None):
        self.name, self.h, self.w, self.crop = name, h, w, crop

    def __repr__(self):
        return self.name

    def frame(self, dtype):
        dt = np.dtype(dtype)
        rng = np.random.default_rng([self.h, self.w, dt.itemsize, 11])
        return rng.integers(0, int(np.iinfo(dt).max) + 1, size=(self.h, self.w, 3), dtype=np.int64).astype(dt)

    def rect(self):
        return (0, 0, self.h, self.w) if self.crop is None else self.crop


FINISH_CASES = [
    FinishCase("5x7", 5, 7),
    FinishCase("1x1", 1, 1),
    FinishCase("one-row-1x45", 1, 45),
    FinishCase("one-column-45x1", 45, 1),
    FinishCase("31x33-tile-edge", 31, 33),
    FinishCase("32x32-one-tile", 32, 32),
    FinishCase("33x31-tile-edge", 33, 31),
    FinishCase("70x40-tiles-down", 70, 40),
    FinishCase("3x350-two-workgroups-along-a-row", 3, 350),
    FinishCase("40x50-crop-odd-origin", 40, 50, crop=(3, 5, 33, 37)),
    FinishCase("40x50-crop-to-1x1", 40, 50, crop=(7, 9, 1, 1)),
    FinishCase("40x50-crop-equal-to-the-frame", 40, 50, crop=(0, 0, 40, 50)),
    FinishCase("40x50-crop-even-origin-64-wide", 40, 80, crop=(2, 16, 32, 64)),
]
ORIENTATIONS = tuple(range(1, 9))

FINISH_PATHS = ("whole", "partial", "misaligned row", "misaligned source", "second workgroup", "flip phase 0", "flip phase 1",
                "flip phase 2", "tile interior", "tile edge")


def finish_paths(case, dtype, orientation):
    """the paths of frame_finish a case reaches at `orientation`; both buffers are taken to start on a 16-byte boundary
      whole / partial     (1..4) a destination window inside / hanging over its row
      misaligned row      (1..4) a destination row that starts off the 16-byte grid
      misaligned source   (1, 4) a whole window whose 16 source bytes start off the 16-byte grid (the crop's origin)
      second workgroup    (1..4) more than 64 windows along a row
      flip phase c        (2, 3) a whole window that starts at channel c of a pixel: finish_flip_window<T, c>
      tile interior / tile edge   (5..8) a tile of 32 x 32 pixels / one with fewer rows or columns"""
    item = np.dtype(dtype).itemsize
    cy, cx, ch, cw = case.rect()
    seen = set()
    if orientation >= 5:
        for y0 in range(0, ch, TILE):
            for x0 in range(0, cw, TILE):
                seen.add("tile interior" if min(TILE, ch - y0) == TILE and min(TILE, cw - x0) == TILE else "tile edge")
        return seen
    V = VEC_BYTES // item
    n = 3 * cw
    fy, fx = orientation in (3, 4), orientation in (2, 3)
    for i in range(ch):
        off = ((i * n * item) % VEC_BYTES) // item
        if off:
            seen.add("misaligned row")
        sy = cy + (ch - 1 - i if fy else i)
        for k, e0 in enumerate(range(-off, n, V)):
            whole = e0 >= 0 and e0 + V <= n
            seen.add("whole" if whole else "partial")
            if k >= LANES:
                seen.add("second workgroup")
            if whole and not fx and (((sy * case.w + cx) * 3 + e0) * item) % VEC_BYTES:
                seen.add("misaligned source")
            if whole and fx:
                seen.add(f"flip phase {e0 % 3}")
    return seen
