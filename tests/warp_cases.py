"""The cases the alignment apply step (csrc/kernels_align.hpp; warp_launch / blur_launch / warp_device_impl in csrc/capi.hip) is
run at beyond the first rounds' inputs: a restatement of the warp kernel's per-tile decision (`tile_paths`), the blur pass's
tile list (`blur_tiles`), the case tables, and the oracle's results for them (computed once per process, read-only).  A plain
module shared by test_warp_cases_host.py, which checks on the CPU that every case reaches what its name says, and
test_gpu_warp_edges.py, which holds the kernels bit for bit to oracle/align_oracle.c on every case.  Integers and NumPy only,
seeded, no device.  The tile constants are read from the kernel's text, so a retuned tile makes the host test name the cases
that no longer reach their path.

group        cases reach (tile_paths / blur_tiles; test_warp_cases_host.py asserts every entry)
-----------  ---------------------------------------------------------------------------------------------------------------
paths        bufend: shift (+1, +1) at 96 x 768 -- exactly one tile, the last, in both dtypes -- and (0.5, 0.5) at 64 x 512 and
             33 x 260 (no ring);  lds: scale 0.7 about the centre at 130 x 1030 (inner tiles, whole tiles of warp_pixel_inside
             thread-rows; its ring tiles all leave the image) and a shear of 0.1 at 130 x 1030 (ring and inner tiles, both
             dtypes);  a 2.2 degree rotation at 130 x 1030 (uint16: lds, tiled and outside in one frame);  2x zoom-in at
             200 x 800 (every tile staged, the four-way split ring included);  identity and (-3, -2) at 96 x 768 (on the tile
             grid, 3 x 3 tiles of uint8: the smallest ring) and 97 x 1024 (one row past it);  40 x 800 (uint16: 24 x 800) --
             three tile columns, fewer than three tile rows: no ring.  Modes 0, 1, 2.
transforms   180 degrees, a mirror, 90 degrees at 300 x 300, 2x zoom-out, a singular matrix (inverse all zeros: every pixel
             is source pixel (0, 0)), half-pixel shifts (mask weight exactly 16384; rintf ties in 16 bit), a shift of 1e5 px.
values       constant max, constant 0, a 0 / max checkerboard and 0 / max columns (cells two pixels wide, so that footprints
             inside one cell exist): outputs at both ends of the type's range.
tiny         (1, 1), (1, 9), (9, 1), (2, 3), (5, 7), (3, 300), (33, 257): w < 4, one row, one column, one pixel, frames
             smaller than the blur radius (reflect-101 loops several times), blur (21, 50) and (31, 4).
blur         ksize 1 .. 31, sigma 0.2 .. 200 on wedge masks (15 degree rotation) and edge strips (shift); two identities
             (ksize 1; sigma 0.2 -- every tap but the centre rounds to 0); an all-masked 40 x 70 frame at ksize 31, the largest
             LDS request of the blur pass.
many_tiles   1025 x 1985 shifted out of frame: 33 x 32 = 1056 blur tiles, more than the blur grid, so the grid-stride loop
             takes a second tile per workgroup; through warp_affine (tiles listed by the warp kernel) and warp_perspective
             (mask_scan_tiles + tile_bitmap_to_list).
perspective  h < 16 (bw0 = 1024 / h), w <= bw0, w a multiple of bw0, one pixel, a 3 x 3 of determinant 0, and the involution
             whose W is exactly 0 along column 64 and changes sign across it.
"""
import functools
import os
import re
import zlib
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_TEXT = os.path.join(ROOT, "shinestacker_amd", "csrc", "kernels_align.hpp")
HOST_TEXT = os.path.join(ROOT, "shinestacker_amd", "csrc", "capi.hip")
DTYPES = [np.uint8, np.uint16]
DEFAULT_BLUR = (21, 50.0)

# what the constants look like in the kernel's text; each pattern has one group per name
CONSTANT_PATTERNS = {
    KERNEL_TEXT: [
        (("WT_W",), r"constexpr\s+int\s+WT_W\s*=\s*(\d+)\s*;"),
        (("TH_U8",), r"#define\s+MI_WARP_TH_U8\s+(\d+)"),
        (("TH_U16",), r"TH\s*=\s*sizeof\(T\)\s*==\s*1\s*\?\s*MI_WARP_TH_U8\s*:\s*(\d+)\s*;"),
        (("LDS_DWORDS",), r"#define\s+MI_WARP_LDS_DWORDS\s+(\d+)"),
        (("WT_SPLIT",), r"constexpr\s+int\s+WT_SPLIT\s*=\s*(\d+)\s*;"),
        (("BT_H", "BT_W"), r"constexpr\s+int\s+BT_H\s*=\s*(\d+)\s*,\s*BT_W\s*=\s*(\d+)\s*;"),
    ],
    HOST_TEXT: [
        (("BLUR_GRID",), r"hipLaunchKernelGGL\(kb,\s*dim3\((\d+)\)"),
        (("SCATTER_GRID",), r"hipLaunchKernelGGL\(\(border_blur_scatter<T>\),\s*dim3\((\d+)\)"),
    ],
}


def read_constants(kernel_text=None, host_text=None):
    """the tile constants, from the source text (the two arguments replace the files: the host test edits a copy)"""
    out = {}
    for path, patterns in CONSTANT_PATTERNS.items():
        text = kernel_text if path == KERNEL_TEXT else host_text
        if text is None:
            with open(path) as f:
                text = f.read()
        for names, pattern in patterns:
            found = re.findall(pattern, text)
            if len(found) != 1:
                raise RuntimeError(f"{os.path.basename(path)}: {names} matched {len(found)} times, expected once: {pattern}")
            values = found[0] if isinstance(found[0], tuple) else (found[0],)
            out.update({n: int(v) for n, v in zip(names, values)})
    return out


CONSTANTS = read_constants()


def vmax_of(dtype):
    return int(np.iinfo(dtype).max)


# ---------------------------------------------------------------- the kernel's per-tile decision
def invert_affine(M):
    """invert_affine_host / orc_invert_affine, operation by operation in double"""
    M = [float(v) for v in np.asarray(M, np.float64).reshape(6)]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0.0 else 0.0
    iM = [0.0] * 6
    iM[0] = M[4] * D
    iM[1] = M[1] * (-D)
    iM[3] = M[3] * (-D)
    iM[4] = M[0] * D
    iM[2] = -iM[0] * M[2] - iM[1] * M[5]
    iM[5] = -iM[3] * M[2] - iM[4] * M[5]
    return iM


def cv_round(v):
    """cvRound of a float64 array: half to even, saturated to int32"""
    return np.clip(np.rint(np.asarray(v, np.float64)), -2147483648.0, 2147483647.0).astype(np.int64)


def coord_tables(M, h, w):
    """warp_coord_tables: ad[w], bd[w], X0[h], Y0[h] (the row terms with their + 16)"""
    iM = invert_affine(M)
    x, y = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    ad = cv_round(iM[0] * x * 1024.0)
    bd = cv_round(iM[3] * x * 1024.0)
    X0 = cv_round((iM[1] * y + iM[2]) * 1024.0) + 16
    Y0 = cv_round((iM[4] * y + iM[5]) * 1024.0) + 16
    return ad, bd, X0, Y0


TilePaths = namedtuple("TilePaths", "gx gy ring tiles rows_inside rows_xy")
TILE_CLASSES = ("outside", "lds", "bufend", "tiled")


def tile_paths(M, h, w, dtype, constants=None):
    """What warp_affine_tiled decides for an h x w frame of `dtype` under M (2 x 3, src -> dst).
    tiles[(ty, tx)]: 'tiled' (staged through LDS) or why not -- 'outside' (the source window leaves the image), 'lds' (it is
    inside but over the LDS budget), 'bufend' (the last staged row's 16-byte reads would pass the buffer's end);
    rows_inside / rows_xy[(ty, tx)]: for the per-pixel tiles, how many thread-rows (one thread's four pixels of one row) take
    warp_pixel_inside and how many warp_pixel_xy."""
    k = constants or CONSTANTS
    size = np.dtype(dtype).itemsize
    bpp, WT_W, TH = 3 * size, k["WT_W"], k["TH_U8"] if size == 1 else k["TH_U16"]
    ad, bd, X0, Y0 = coord_tables(M, h, w)
    gx, gy = -(-w // WT_W), -(-h // TH)
    ring = gx >= 3 and gy >= 3
    tiles, rows_inside, rows_xy = {}, {}, {}
    for ty in range(gy):
        for tx in range(gx):
            x_t, y_t = tx * WT_W, ty * TH
            cxs = np.array([x_t, min(x_t + WT_W, w) - 1])
            cys = np.array([y_t, min(y_t + TH, h) - 1])
            sx = ((X0[cys][:, None] + ad[cxs][None, :]) >> 5) >> 5
            sy = ((Y0[cys][:, None] + bd[cxs][None, :]) >> 5) >> 5
            sxmin, sxmax, symin, symax = int(sx.min()), int(sx.max()), int(sy.min()), int(sy.max())
            nc, nr = sxmax - sxmin + 2, symax - symin + 2
            pitch = (((nc * bpp + 3 + 3) >> 2) + 3) & ~3
            row_bytes = w * bpp
            start0 = (max(symin, 0) * w + max(sxmin, 0)) * bpp
            if not (sxmin >= 0 and symin >= 0 and sxmax + 1 < w and symax + 1 < h):
                cls = "outside"
            elif nr * pitch > k["LDS_DWORDS"]:
                cls = "lds"
            elif start0 + (nr - 1) * row_bytes + pitch * 4 > h * w * bpp:
                cls = "bufend"
            else:
                cls = "tiled"
            tiles[(ty, tx)] = cls
            if cls == "tiled":
                continue
            ys = np.arange(y_t, min(y_t + TH, h))
            xq = np.arange(x_t, min(x_t + WT_W, w), 4)
            inside = np.broadcast_to((xq + 3 < w)[None, :], (len(ys), len(xq))).copy()
            for e in (0, 3):
                xe = np.minimum(xq + e, w - 1)
                ex = ((X0[ys][:, None] + ad[xe][None, :]) >> 5) >> 5
                ey = ((Y0[ys][:, None] + bd[xe][None, :]) >> 5) >> 5
                inside &= (ex >= 0) & (ex + 1 < w) & (ey >= 0) & (ey + 1 < h - 1)
            rows_inside[(ty, tx)] = int(inside.sum())
            rows_xy[(ty, tx)] = int(inside.size - inside.sum())
    return TilePaths(gx, gy, ring, tiles, rows_inside, rows_xy)


def on_ring(p, ty, tx):
    """the tile is one of the outer ring that warp_affine_tiled splits four ways"""
    return p.ring and (ty in (0, p.gy - 1) or tx in (0, p.gx - 1))


def blur_tiles(mask, constants=None):
    """the (ty, tx) of the BT_H x BT_W tiles that hold a masked pixel: what the blur pass's list must hold"""
    k = constants or CONSTANTS
    ys, xs = np.nonzero(np.asarray(mask) == 0)
    return set(zip((ys // k["BT_H"]).tolist(), (xs // k["BT_W"]).tolist()))


# ---------------------------------------------------------------- transforms
def rot(theta_deg, s=1.0, tx=0.0, ty=0.0, cx=0.0, cy=0.0):
    """a similarity src -> dst: rotation by theta and scale s about (cx, cy), then a shift"""
    t = np.deg2rad(theta_deg)
    a, b = s * np.cos(t), s * np.sin(t)
    return ((a, b, (1 - a) * cx - b * cy + tx), (-b, a, b * cx + (1 - a) * cy + ty))


def about_centre(theta_deg, s, h, w, tx=0.0, ty=0.0):
    return rot(theta_deg, s, tx, ty, (w - 1) / 2, (h - 1) / 2)


def shift(dx, dy):
    return ((1.0, 0.0, float(dx)), (0.0, 1.0, float(dy)))


def as_3x3(M):
    return tuple(tuple(r) for r in M) + ((0.0, 0.0, 1.0),)


IDENTITY = shift(0, 0)
SHEAR = ((1.0, 0.0, 0.0), (-0.1, 1.0, 0.0))   # dst (x, y) reads src (x, y + 0.1 x): tall source windows that stay in the frame
SINGULAR = ((0.0, 0.0, 1.0), (0.0, 0.0, 2.0))
SIMILARITY = (0.37, 1.0003, 3.37, -2.21)      # the near-identity of the first rounds' tests: (degrees, scale, tx, ty)
MILD = ((1.002, 0.004, -3.1), (-0.003, 0.998, 4.4), (1.5e-5, -2.5e-5, 1.0))
STRONG = ((0.9, 0.1, 12.0), (-0.08, 1.1, -9.0), (6e-4, 3e-4, 1.0))
SINGULAR_3X3 = ((1.0, 2.0, 3.0), (2.0, 4.0, 6.0), (0.5, -1.0, 1.0))      # rows 0 and 1 are parallel: determinant exactly 0
INVOLUTION = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0 / 64, 0.0, -1.0))   # its own inverse, exactly; W = x / 64 - 1


# ---------------------------------------------------------------- the case tables
# kind: 'affine' (2 x 3) or 'perspective' (3 x 3);  modes: border modes to run;  blurs: (ksize, sigma) pairs for mode 2;
# frame: 'random' | 'max' | 'zero' | 'checker' | 'columns';  reach: what the host test must find (see there)
WarpCase = namedtuple("WarpCase", "group name kind shape dtype M modes blurs frame reach")


def _both(group, name, kind, shape, M, modes=(0, 1, 2), blurs=(DEFAULT_BLUR,), frame="random", reach=(), reach16=None):
    return [WarpCase(group, name, kind, shape, dt, M, tuple(modes), tuple(blurs), frame,
                     tuple(reach if dt == np.uint8 or reach16 is None else reach16)) for dt in DTYPES]


def _paths():
    c = []
    c += _both("paths", "bufend_shift_1_1_96x768", "affine", (96, 768), shift(1, 1), reach=("bufend", "one_bufend", "ring"))
    c += _both("paths", "bufend_shift_half_64x512", "affine", (64, 512), shift(0.5, 0.5), reach=("bufend", "no_ring"))
    c += _both("paths", "bufend_shift_half_33x260", "affine", (33, 260), shift(0.5, 0.5), reach=("bufend", "no_ring"))
    c += _both("paths", "lds_scale_0.7_130x1030", "affine", (130, 1030), about_centre(0.0, 0.7, 130, 1030),
               reach=("lds", "ring", "lds_inner", "whole_tile_inside"))
    c += _both("paths", "lds_shear_0.1_130x1030", "affine", (130, 1030), SHEAR, reach=("lds", "ring", "lds_on_ring", "lds_inner"))
    c += _both("paths", "rotation_2.2_130x1030", "affine", (130, 1030), about_centre(2.2, 1.0, 130, 1030),
               reach=("ring", "outside"), reach16=("ring", "lds", "tiled", "outside"))
    c += _both("paths", "tiled_zoom_in_2x_200x800", "affine", (200, 800), about_centre(0.0, 2.0, 200, 800),
               reach=("ring", "all_tiled"))
    for shape in ((96, 768), (97, 1024)):
        tag = "%dx%d" % shape
        c += _both("paths", "identity_" + tag, "affine", shape, IDENTITY, reach=("ring", "tiled", "outside"))
        c += _both("paths", "shift_-3_-2_" + tag, "affine", shape, shift(-3, -2), reach=("ring", "tiled", "outside"))
    for dt, shape in ((np.uint8, (40, 800)), (np.uint16, (24, 800))):      # three tile columns, two tile rows of either type
        c += [x for x in _both("paths", "no_ring_wide_%dx%d" % shape, "affine", shape,
                               about_centre(*SIMILARITY[:2], *shape, *SIMILARITY[2:]), reach=("no_ring", "wide")) if x.dtype == dt]
    return c


def _transforms():
    c, g, m = [], "transforms", (1, 2)
    h, w = 100, 800
    c += _both(g, "rotation_180", "affine", (h, w), about_centre(180.0, 1.0, h, w), m)
    c += _both(g, "mirror_x", "affine", (h, w), ((-1.0, 0.0, float(w - 1)), (0.0, 1.0, 0.0)), m)
    c += _both(g, "rotation_90_300x300", "affine", (300, 300), about_centre(90.0, 1.0, 300, 300), m)
    c += _both(g, "zoom_out_2x_200x800", "affine", (200, 800), about_centre(0.0, 0.5, 200, 800), m)
    c += _both(g, "singular_9x11", "affine", (9, 11), SINGULAR, m, reach=("first_pixel",))
    c += _both(g, "singular_70x777", "affine", (70, 777), SINGULAR, m, reach=("first_pixel",))
    for dx, dy in ((0.5, 0.0), (0.0, 0.5), (0.5, 0.5)):
        c += _both(g, "half_pixel_%g_%g_70x777" % (dx, dy), "affine", (70, 777), shift(dx, dy), m, reach=("mask_tie",))
    c += _both(g, "shift_1e5", "affine", (h, w), shift(1e5, -1e5), m, reach=("all_masked",))
    return c


def _values():
    h, w = 70, 777
    M = about_centre(*SIMILARITY[:2], h, w, *SIMILARITY[2:])
    reach = {"max": ("has_max",), "zero": ("has_zero",), "checker": ("has_max", "has_zero"), "columns": ("has_max", "has_zero")}
    return [x for kind in ("max", "zero", "checker", "columns")
            for x in _both("values", kind + "_70x777", "affine", (h, w), M, frame=kind, reach=reach[kind])]


TINY_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 3), (5, 7), (3, 300), (33, 257)]
TINY_BLURS = ((21, 50.0), (31, 4.0))
TINY_PIVOT = (-2.0, -2.0)     # a 10 degree rotation about a point outside the frame moves every pixel by half a pixel or more


def _tiny():
    c = []
    for shape in TINY_SHAPES:
        tag = "%dx%d" % shape
        c += _both("tiny", "shift_0.75_-0.5_" + tag, "affine", shape, shift(0.75, -0.5), blurs=TINY_BLURS, reach=("masked",))
        c += _both("tiny", "rotation_10_" + tag, "affine", shape, rot(10.0, 1.0, 0.0, 0.0, *TINY_PIVOT), blurs=TINY_BLURS,
                   reach=("masked",) if shape == (1, 1) else ("masked", "unmasked"))
    return c


BLURS = [(1, 0.3), (3, 0.5), (5, 2.0), (21, 0.2), (21, 50.0), (21, 200.0), (31, 4.0), (31, 50.0)]
BLUR_IDENTITIES = [(1, 0.3), (21, 0.2)]       # one tap; every tap but the centre rounds to 0 in 8 and in 16 bits
ALL_MASKED = "all_masked_40x70"


def _blur():
    c = []
    for ks, sigma in BLURS:
        tag = "k%d_s%g" % (ks, sigma)
        reach = ("blur_identity",) if (ks, sigma) in BLUR_IDENTITIES else ("masked",)
        c += _both("blur", "wedges_rotation_15_100x200_" + tag, "affine", (100, 200), about_centre(15.0, 1.0, 100, 200), (2,),
                   ((ks, sigma),), reach=reach + ("unmasked",))
        c += _both("blur", "strips_shift_12.5_-7.25_70x130_" + tag, "affine", (70, 130), shift(12.5, -7.25), (2,),
                   ((ks, sigma),), reach=reach + ("unmasked",))
    c += _both("blur", ALL_MASKED + "_k31_s50", "affine", (40, 70), shift(0.0, 100.0), (2,), ((31, 50.0),),
               reach=("masked", "all_masked"))
    return c


MANY_TILES_SHAPE = (1025, 1985)
MANY_TILES_M = shift(4000.0, 0.0)     # every row becomes its first pixel: no pixel in frame, and the columns still differ
MANY_TILES_BLUR = (3, 0.5)


def _many_tiles():
    c = _both("many_tiles", "out_of_frame_1025x1985_affine", "affine", MANY_TILES_SHAPE, MANY_TILES_M, (2,), (MANY_TILES_BLUR,),
              reach=("many_tiles",))
    c += _both("many_tiles", "out_of_frame_1025x1985_perspective", "perspective", MANY_TILES_SHAPE, as_3x3(MANY_TILES_M), (2,),
               (MANY_TILES_BLUR,), reach=("many_tiles",))
    return c


PERSPECTIVE_SHAPES = [(5, 300), (1, 1100), (15, 68), (16, 128), (133, 203), (40, 50), (1, 1)]
QUARTER_SHIFT = ((1.0, 0.0, 0.25), (0.0, 1.0, 0.25), (0.0, 0.0, 1.0))    # the one pixel from a footprint three quarters in frame


def _perspective():
    c = []
    for shape in PERSPECTIVE_SHAPES:
        tag = "%dx%d" % shape
        for name, H in (("mild", MILD), ("strong", STRONG), ("singular", SINGULAR_3X3)):
            c += _both("perspective", name + "_" + tag, "perspective", shape, H, reach=("first_pixel",) if name == "singular" else ())
    c += _both("perspective", "involution_20x200", "perspective", (20, 200), INVOLUTION, reach=("horizon",))
    c += _both("perspective", "quarter_shift_1x1", "perspective", (1, 1), QUARTER_SHIFT, reach=("mixes_border",))
    return c


GROUPS = ["paths", "transforms", "values", "tiny", "blur", "many_tiles", "perspective"]
CASES = _paths() + _transforms() + _values() + _tiny() + _blur() + _many_tiles() + _perspective()
assert len({(c.name, c.dtype) for c in CASES}) == len(CASES)
assert {c.group for c in CASES} == set(GROUPS)


def cases_of(group, dtype=None):
    return [c for c in CASES if c.group == group and (dtype is None or c.dtype == dtype)]


def case_name(c):
    return "%s/%s/%s" % (c.group, c.name, np.dtype(c.dtype).name)


def runs_of(c):
    """the (mode, ksize, sigma) a case is run at: modes 0 and 1 once, mode 2 once per blur"""
    return [(m, *b) for m in c.modes for b in (c.blurs if m == 2 else (DEFAULT_BLUR,))]


def border_value(dtype):
    return (10, 200, 3000 if np.dtype(dtype) == np.uint16 else 77, 0)


# ---------------------------------------------------------------- frames and the oracle's results
def make_frame(kind, shape, dtype, seed):
    h, w = shape
    vmax = vmax_of(dtype)
    y, x = np.mgrid[:h, :w]
    if kind == "random":
        img = np.random.default_rng(seed).integers(0, vmax + 1, (h, w, 3)).astype(dtype)
    elif kind == "max":
        img = np.full((h, w, 3), vmax, dtype)
    elif kind == "zero":
        img = np.zeros((h, w, 3), dtype)
    elif kind == "checker":
        img = np.repeat(((((y >> 1) + (x >> 1)) & 1) * vmax)[:, :, None], 3, axis=2).astype(dtype)
    elif kind == "columns":
        img = np.repeat((((x >> 1) & 1) * vmax)[:, :, None], 3, axis=2).astype(dtype)
    else:
        raise ValueError(kind)
    assert img.dtype == np.dtype(dtype) and img.shape == (h, w, 3)
    img.setflags(write=False)
    return img


def frame_of(c):
    return _frame(c.frame, c.group, c.shape, c.dtype)


@functools.lru_cache(maxsize=None)
def _frame(kind, group, shape, dtype):
    """one frame per (group, shape, dtype): the cases of a group that share a shape share the pixels too"""
    return make_frame(kind, shape, dtype, zlib.crc32(("%s/%dx%d/%s" % (group, *shape, np.dtype(dtype).name)).encode()))


def matrix_of(c):
    return np.array(c.M, np.float64)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


def oracle_warp(kind, img, M, mode, ksize=DEFAULT_BLUR[0], sigma=DEFAULT_BLUR[1]):
    """(image, mask) of oracle/align_oracle.c, read-only"""
    fn = _oracle().warp_perspective if kind == "perspective" else _oracle().warp_affine
    out, mask = fn(img, M, border_mode=mode, border_value=border_value(img.dtype), blur_ksize=ksize, blur_sigma=sigma,
                   want_mask=True)
    out.setflags(write=False)
    mask.setflags(write=False)
    return out, mask


@functools.lru_cache(maxsize=None)
def expected(c, mode, ksize=DEFAULT_BLUR[0], sigma=DEFAULT_BLUR[1]):
    return oracle_warp(c.kind, frame_of(c), matrix_of(c), mode, ksize, sigma)


def gauss_taps(ksize, sigma, dtype):
    return _oracle().gauss_kernel_fixed(ksize, sigma, 8 * np.dtype(dtype).itemsize)


def perspective_w(c):
    """W of every pixel of a perspective case, by the stated recurrence in double: W0 = M6 * bx + M7 * y + M8 at the block's
    first column bx, W = W0 + M6 * (x - bx); blocks of bw0 = min(1024 / min(16, h), w) columns"""
    h, w = c.shape
    iM = np.array(_oracle_invert_3x3(c.M), np.float64)
    bw0 = min(1024 // min(16, h), w)
    y, x = np.mgrid[:h, :w].astype(np.float64)
    bx = np.floor(x / bw0) * bw0
    W0 = iM[6] * bx + iM[7] * y + iM[8]
    return W0 + iM[6] * (x - bx)


def _oracle_invert_3x3(M):
    """cv::invert of a 3 x 3 as orc_invert_3x3 and warp_device_impl state it: cofactors times 1 / det, singular -> zeros"""
    m = [float(v) for v in np.asarray(M, np.float64).reshape(9)]
    d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6])
    d = 1.0 / d if d != 0.0 else 0.0
    return [(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d, (m[1] * m[5] - m[2] * m[4]) * d,
            (m[5] * m[6] - m[3] * m[8]) * d, (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
            (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d, (m[0] * m[4] - m[1] * m[3]) * d]


# ---------------------------------------------------------------- the device entry points, the per-stream scratch
DEVICE_SHAPE = (37, 64)       # w % 4 == 0: dword stores unless a pointer says otherwise
DEVICE_BLUR = (5, 2.0)
DEVICE_TRANSFORMS = [
    ("zoom_in_1.25", about_centre(0.0, 1.25, *DEVICE_SHAPE)),       # every tile staged through LDS: the store variants
    ("shift_2.5_-1.25", shift(2.5, -1.25)),                          # per-pixel tiles, masked strips: the blur passes
]


def device_frame(dtype):
    return _frame("random", "device", DEVICE_SHAPE, dtype)


def scratch_sequence(dtype):
    """(kind, frame, M, ksize, sigma) in the order the scratch test runs them: the all-masked blur case, a `many_tiles` frame
    cropped to 200 rows (a larger tile list and coordinate table), the 5 x 7 frame, the first again; each as a 2 x 3 and a 3 x 3"""
    first, = [c for c in cases_of("blur", dtype) if "all_masked" in c.reach]
    wide, = [c for c in cases_of("many_tiles", dtype) if c.kind == "affine"]
    small, = [c for c in cases_of("tiny", dtype) if c.shape == (5, 7) and c.name.startswith("shift")]
    steps = [(first, frame_of(first)), (wide, frame_of(wide)[:200]), (small, frame_of(small)), (first, frame_of(first))]
    return [(kind, img, np.array(c.M if kind == "affine" else as_3x3(c.M), np.float64), *c.blurs[0])
            for c, img in steps for kind in ("affine", "perspective")]
