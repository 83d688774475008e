"""The demosaic cases shared by test_demosaic_host.py (CPU: the cases mean something) and test_gpu_demosaic.py (GPU: the kernel
equals the restatement on them).  Seeded full-range random mosaics; every reference is computed once and shared.

Shapes, against the kernel's tile (demosaic.TILE_H x demosaic.TILE_W, a halo of 2 sites, threads that own 2 x 2 cells -- one
at uint16, two side by side at uint8):
  * the smallest frames, where every tap reflects, some of them twice: 2x2, 2x3, 3x2, 3x3
  * two rows / two columns across a tile boundary
  * TILE - 1, TILE and TILE + 1 in both directions, every combination: even and odd sizes, a tile that ends on the frame's
    edge, one site before it and one past it (odd widths also take the per-sample store path on every other row)
  * several tiles in both directions with a ragged last tile"""
import functools

import numpy as np

import demosaic_restatement as R
from shinestacker_amd import demosaic as D

TH, TW = D.TILE_H, D.TILE_W
DTYPES = (np.uint8, np.uint16)
PATTERNS = R.PATTERNS
TINY = [(2, 2), (2, 3), (3, 2), (3, 3), (2, TW + 3), (TH + 3, 2)]
EDGES = [(h, w) for h in (TH - 1, TH, TH + 1) for w in (TW - 1, TW, TW + 1)]
RAGGED = (3 * TH + 5, 3 * TW + 7)          # 53 x 391: 4 x 4 tiles, the last ones ragged, both sizes odd
SHAPES = TINY + EDGES + [RAGGED]
BIG_ENOUGH = EDGES + [RAGGED]               # thousands of sites: both clamps act on random data (test_demosaic_host.py)


@functools.lru_cache(maxsize=None)
def random_mosaic(shape, dtype, salt=0):
    rng = np.random.default_rng([shape[0], shape[1], np.dtype(dtype).itemsize, salt])
    m = rng.integers(0, int(np.iinfo(dtype).max) + 1, size=shape, dtype=np.int64).astype(dtype)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def reference(shape, dtype, pattern, with_sums=False):
    """the restatement on random_mosaic(shape, dtype), default Cfa"""
    out = R.demosaic(random_mosaic(shape, dtype), pattern, return_sums=with_sums)
    for a in (out if with_sums else (out,)):
        a.setflags(write=False)
    return out


def option_cases(dtype):
    """(name, mosaic, Cfa) at the ragged shape: the per-site corrections and the saturated frames"""
    mx = int(np.iinfo(dtype).max)
    m = random_mosaic(RAGGED, dtype, salt=1)
    full = np.full(RAGGED, mx, dtype)
    zero = np.zeros(RAGGED, dtype)
    return [
        ("black and gains per position", m, D.Cfa("GRBG", black=[mx // 16, 0, mx // 32, mx // 8], gains=[1.9, 1.0, 0.75, 2.31])),
        ("gains near 16", m, D.Cfa("BGGR", black=mx // 64, gains=[15.99, 7.5, 7.5, 12.25])),
        ("white below the maximum", m, D.Cfa("RGGB", white=mx - mx // 3)),
        ("white below the maximum, with gains", m, D.Cfa("GBRG", gains=[1.5, 1.0, 1.0, 1.25], white=mx // 2)),
        ("gains 0", m, D.Cfa("RGGB", gains=0)),
        ("one gain 0", m, D.Cfa("GBRG", gains=[1.0, 0.0, 1.0, 1.0])),
        ("all maximum", full, D.Cfa("GRBG")),
        ("all maximum, gains", full, D.Cfa("RGGB", gains=[2.0, 1.0, 1.0, 0.5])),
        ("all zero", zero, D.Cfa("BGGR", gains=3.0)),
    ]


def restate(mosaic, cfa):
    code, black, gain_q, white = cfa.quantised(mosaic.dtype)
    return R.demosaic(mosaic, R.PATTERNS[code], black, gain_q, white)
