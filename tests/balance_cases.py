"""The cases the balance kernels (csrc/kernels_balance.hpp: hist_u8 / hist_u16, lut_apply_u8 / _u16, lut_linear_build,
cvt_color_u8) are run at beyond the recorded fixtures, and the restatement of lut_linear_build.  A plain module shared by
test_balance_cases_host.py, which shows from the oracle that no case is vacuous and that the launchers' grid caps are the
ones assumed here, and test_gpu_balance_edges.py, which holds the kernels to the oracle (oracle/oracle.py: balance_hist,
resize_area_int, apply_lut, cvt_color_u8) on every case.  Integers and NumPy only, seeded, cached, read-only, no device.

The launchers in csrc/capi.hip cap their grids; past the cap a thread walks a grid-stride loop.  The caps below are the
numbers written there (the host test reads them back out of the source), and the "long grid" shapes are the smallest
round ones past each."""
import functools
from collections import namedtuple

import numpy as np

DTYPES = [np.uint8, np.uint16]

# ---------------------------------------------------------------- the launchers' grid caps (csrc/capi.hip)
BLOCK = 256                      # threads per workgroup, every kernel of the family
HIST_MAX_BLOCKS = 256 * 8        # hist_enqueue: one sub-sampled pixel per thread and step
LUT_MAX_BLOCKS = 256 * 16        # mi_apply_lut_device, sized for 12 elements per thread whatever the dtype
LUT_U8_PER_THREAD = 12           # lut_apply_u8: 12 bytes (4 pixels) per thread and step, then a tail of n % 12
CVT_MAX_BLOCKS = 256 * 16        # mi_cvt_color_device: one pixel per thread and step

HIST_CAP = HIST_MAX_BLOCKS * BLOCK                        # sub-sampled pixels one pass of the grid covers
LUT_U8_CAP = LUT_MAX_BLOCKS * BLOCK * LUT_U8_PER_THREAD   # elements (pixels * 3)
LUT_U16_CAP = LUT_MAX_BLOCKS * BLOCK                      # elements; below it lut_apply_u16 already strides ~12 times,
                                                          # its grid being sized by n / 12 -- past it the grid is capped too
CVT_CAP = CVT_MAX_BLOCKS * BLOCK                          # pixels

LONG_LUT_SHAPE = {np.uint8: (2050, 2050), np.uint16: (600, 600)}
LONG_HIST_SHAPE, LONG_HIST_S, LONG_HIST_MASK = (1450, 1460), 2, 0.9
CUBE_SIDE = 4096                 # 4096 x 4096 pixels = 256^3 colours
CUBE_SLAB = 32                   # values of channel 0 per comparison with the oracle = 512 rows of the cube image


def nbins_of(dtype):
    return 256 if np.dtype(dtype) == np.uint8 else 65536


def vmax_of(dtype):
    return nbins_of(dtype) - 1


def dtype_name(dtype):
    return np.dtype(dtype).name


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------- frames
@functools.lru_cache(maxsize=None)
def random_frame(shape, dtype, seed=0):
    """uniform over the whole range, the first third of the rows divided by 3 so that the histogram is uneven"""
    rng = np.random.default_rng([seed, shape[0], shape[1], np.dtype(dtype).itemsize])
    img = rng.integers(0, nbins_of(dtype), tuple(shape) + (3,)).astype(dtype)
    img[: shape[0] // 3] //= 3
    return _frozen(img)


@functools.lru_cache(maxsize=None)
def constant_frame(shape, dtype, values):
    """every pixel (values[0], values[1], values[2])"""
    img = np.empty(tuple(shape) + (3,), dtype)
    img[...] = np.asarray(values, dtype)
    return _frozen(img)


def subsampled_size(h, w, s, fast):
    """the grid the histogram is taken of: img[::s, ::s], or cv2.resize's round-half-even(dim / s)"""
    if s == 1:
        return h, w
    if fast:
        return -(-h // s), -(-w // s)
    return int(np.rint(h * (1.0 / s))), int(np.rint(w * (1.0 / s)))


def has_partial_blocks(h, w, s, fast):
    """an area-mean grid whose last row or column of blocks hangs over the image edge"""
    hs, ws = subsampled_size(h, w, s, fast)
    return s > 1 and not fast and (hs * s > h or ws * s > w)


def drops_last_block(h, w, s, fast):
    """an area-mean grid that leaves the last, partial row or column of blocks out (round half to even went down)"""
    hs, ws = subsampled_size(h, w, s, fast)
    return s > 1 and not fast and (hs * s < h or ws * s < w)


def points_on_the_circle(hs, ws, mask_size):
    """grid points of the hs x ws grid exactly on the mask's circle, in the arithmetic of balance.py:165-175"""
    xv, yv = np.meshgrid(np.linspace(0, ws - 1, ws), np.linspace(0, hs - 1, hs))
    r = min(ws, hs) * mask_size / 2
    return int(((xv - ws / 2) ** 2 + (yv - hs / 2) ** 2 == r ** 2).sum())


# ---------------------------------------------------------------- histogram cases
HistCase = namedtuple("HistCase", "name kind shape s fast mask")   # kind: "random" or a (b, g, r) triple as fractions of vmax

HIST_CASES = [
    HistCase("1x1", "random", (1, 1), 1, True, 0.0),
    HistCase("2x2 area", "random", (2, 2), 2, False, 0.0),
    HistCase("2x2 fast", "random", (2, 2), 2, True, 0.0),
    HistCase("3x5 area", "random", (3, 5), 2, False, 0.0),          # rows: 1.5 -> 2, kept and partial; columns: 2.5 -> 2, dropped
    HistCase("3x5 fast", "random", (3, 5), 2, True, 0.0),
    HistCase("5x7 area", "random", (5, 7), 2, False, 0.0),          # rows: 2.5 -> 2, dropped; columns: 3.5 -> 4, partial
    HistCase("7x9 fast s4", "random", (7, 9), 4, True, 0.0),        # the ceiling size 2 x 3
    HistCase("121x152 area s3", "random", (121, 152), 3, False, 0.0),   # 40 x 51: a partial last column of blocks
    HistCase("121x152 area s5", "random", (121, 152), 5, False, 0.0),   # 24 x 30: whole blocks, the float32 product at 1/25
    HistCase("121x152 area s6", "random", (121, 152), 6, False, 0.0),   # 20 x 25: whole blocks, 1/36
    HistCase("121x152 area s7", "random", (121, 152), 7, False, 0.0),   # 17 x 22: a partial last column
    HistCase("119x154 area s3", "random", (119, 154), 3, False, 0.0),   # 40 x 51: a partial last row
    HistCase("119x154 area s5", "random", (119, 154), 5, False, 0.0),   # 24 x 31: partial row, column and corner
    HistCase("119x154 area s6", "random", (119, 154), 6, False, 0.0),   # 20 x 26: partial row, column and corner
    HistCase("64x64 mask 1.0", "random", (64, 64), 1, True, 1.0),
    HistCase("64x64 mask 0.5", "random", (64, 64), 1, True, 0.5),
    HistCase("64x64 area mask 1.0", "random", (64, 64), 2, False, 1.0),
    HistCase("constant max", (1.0, 1.0, 1.0), (300, 300), 1, True, 0.0),
    HistCase("constant 0", (0.0, 0.0, 0.0), (300, 300), 1, True, 0.0),
    HistCase("constant max area s3", (1.0, 1.0, 1.0), (300, 300), 3, False, 0.0),
    HistCase("three constants", (0.0125, 1.0, 0.3), (67, 45), 1, True, 0.0),
    HistCase("three constants area", (0.0125, 1.0, 0.3), (67, 45), 2, False, 0.7),
]
LONG_HIST_CASES = [
    HistCase("long area", "random", LONG_HIST_SHAPE, LONG_HIST_S, False, 0.0),
    HistCase("long area masked", "random", LONG_HIST_SHAPE, LONG_HIST_S, False, LONG_HIST_MASK),
]
S_NOT_POWER_OF_TWO = [c for c in HIST_CASES if c.kind == "random" and not c.fast and c.s in (3, 5, 6, 7)]
MASK_ON_CIRCLE = [c for c in HIST_CASES if c.mask == 1.0]


def hist_frame(case, dtype):
    if case.kind == "random":
        return random_frame(case.shape, dtype, seed=case.s)
    return constant_frame(case.shape, dtype, tuple(int(round(f * vmax_of(dtype))) for f in case.kind))


_HIST = {}


def hist_reference(orc, case, dtype, lumi):
    """oracle.balance_hist of the case's frame, computed once"""
    key = (case, dtype_name(dtype), bool(lumi))
    if key not in _HIST:
        _HIST[key] = _frozen(orc.balance_hist(hist_frame(case, dtype), bool(lumi), case.s, case.fast, case.mask))
    return _HIST[key]


# ---------------------------------------------------------------- batch histogram
BATCH_SHAPE = (37, 53)


def batch_frames(dtype):
    """three different frames, one of them constant"""
    return [random_frame(BATCH_SHAPE, dtype, seed=11), constant_frame(BATCH_SHAPE, dtype, (vmax_of(dtype),) * 3),
            random_frame(BATCH_SHAPE, dtype, seed=12)]


# ---------------------------------------------------------------- table apply
# n = 3 * pixels; lut_apply_u8 takes n // 12 whole steps and a tail of n % 12 in {0, 3, 6, 9}
LUT_SHAPES = [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (2, 3), (1, 7), (37, 53)]
LUT_KINDS = ["random", "identity", "repeated"]


@functools.lru_cache(maxsize=None)
def lut_tables(kind, dtype, nlut):
    n = nbins_of(dtype)
    if kind == "random":
        t = np.random.default_rng([41, nlut, n]).integers(0, n, (nlut, n)).astype(dtype)
    elif kind == "identity":
        t = np.repeat(np.arange(n, dtype=dtype)[None], nlut, axis=0)
    else:
        t = np.repeat(np.array([[n // 3], [n - 1], [7]], dtype)[:nlut], n, axis=1)
    return _frozen(np.ascontiguousarray(t))


# ---------------------------------------------------------------- the whole cube
@functools.lru_cache(maxsize=1)
def cube():
    """all 256^3 triples as one 4096 x 4096 x 3 uint8 image: pixel p = y * 4096 + x holds (p >> 16, (p >> 8) & 255, p & 255),
    so 512 rows hold 32 values of channel 0.  For the inverse codes channel 0 is the hue, all 256 values of it."""
    p = np.arange(1 << 24, dtype=np.uint32)
    img = np.empty((1 << 24, 3), np.uint8)
    img[:, 0] = p >> 16
    img[:, 1] = (p >> 8) & 255
    img[:, 2] = p & 255
    return _frozen(img.reshape(CUBE_SIDE, CUBE_SIDE, 3))


def cube_slabs():
    """(first row, last row + 1) of each slab of CUBE_SLAB values of channel 0"""
    rows = CUBE_SLAB * 65536 // CUBE_SIDE
    return [(y, y + rows) for y in range(0, CUBE_SIDE, rows)]


# ---------------------------------------------------------------- lut_linear_build restated
def linear_table(counts, lo, hi, ref_mean, dtype):
    """(table, ratio) as lut_linear_build writes them for one channel: mean = sum(i * counts[i]) / sum(counts[i]) over
    [lo, hi) with exact integers and one float64 division, ratio = ref_mean / mean (1.0 where the interval holds no counts),
    table[i] = trunc(clip(i * ratio, 0, vmax)) in float64; a NaN product (0 * inf) gives 0."""
    n = nbins_of(dtype)
    counts = np.asarray(counts).reshape(-1)
    assert counts.size == n and 0 <= lo < hi <= n
    s0 = sum(int(c) for c in counts[lo:hi])
    s1 = sum(i * int(counts[i]) for i in range(lo, hi))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.float64(ref_mean) / np.float64(s1 / s0)) if s0 else 1.0
        v = np.arange(n, dtype=np.float64) * np.float64(ratio)
        v = np.where(np.isnan(v), 0.0, np.trunc(np.clip(v, 0.0, float(n - 1))))
    return v.astype(dtype), ratio


def identity_table(dtype):
    return np.arange(nbins_of(dtype), dtype=dtype)


LinearCase = namedtuple("LinearCase", "name frame lo hi first ref s fast mask")
# ref: per built table, ("abs", fraction of vmax) or ("rel", factor of that channel's own mean inside [lo, hi))
LINEAR_SHAPE = (61, 83)        # 15189 elements: 1265 whole steps of lut_apply_u8 and a tail of 9


@functools.lru_cache(maxsize=None)
def linear_frame(kind, dtype):
    n = nbins_of(dtype)
    h, w = LINEAR_SHAPE
    if kind == "random":
        img = random_frame(LINEAR_SHAPE, dtype, seed=21).copy()
        img[:4, :9] = 1                     # some pixels of value 1 (luminance 1 too): the interval [1, 2) holds counts
    elif kind == "upper half":              # nothing below n / 2
        img = np.random.default_rng([22, n]).integers(n // 2, n, (h, w, 3)).astype(dtype)
    elif kind == "dim":                     # values in [0, n / 64): a reference mean 50 times the frame's clips most of the table
        img = np.random.default_rng([23, n]).integers(0, n // 64, (h, w, 3)).astype(dtype)
    else:
        assert kind == "black"
        img = np.zeros((h, w, 3), dtype)
    return _frozen(img)


def linear_cases(dtype, lumi):
    n = nbins_of(dtype)
    k = 1 if lumi else 3
    out = [
        LinearCase("random", "random", 0, n, 0, [("abs", 0.31), ("abs", 0.55), ("abs", 0.47)][:k], 1, True, 0.0),
        LinearCase("interval [1, 2)", "random", 1, 2, 0, [("abs", 2.5 / (n - 1)), ("abs", 0.4 / (n - 1)), ("abs", 1.0 / (n - 1))][:k], 1, True, 0.0),
        LinearCase("interval without counts", "upper half", 3, n // 4, 0, [("abs", 0.5)] * k, 1, True, 0.0),
        LinearCase("fifty times the mean", "dim", 0, n, 0, [("rel", 50.0)] * k, 1, True, 0.0),
        LinearCase("area s3 mask 0.8", "random", n // 16, n - n // 8, 0, [("rel", 0.8), ("rel", 1.3), ("rel", 1.05)][:k], 3, False, 0.8),
        LinearCase("black", "black", 0, n, 0, [("abs", 0.4)] * k, 1, True, 0.0),
        LinearCase("black, reference black", "black", 0, n, 0, [("abs", 0.0)] * k, 1, True, 0.0),
    ]
    if not lumi:
        out.append(LinearCase("first channel 1", "random", 0, n, 1, [("rel", 1.4), ("rel", 0.7)], 2, True, 0.0))
    return out


def linear_expectation(orc, case, dtype, lumi):
    """(frame, reference means, tables [ntab][nbins], ratios [ntab - first], corrected frame) of a LinearCase: the histogram
    half is oracle.balance_hist, the table half linear_table, the apply half oracle.apply_lut"""
    frame = linear_frame(case.frame, dtype)
    hist = orc.balance_hist(frame, bool(lumi), case.s, case.fast, case.mask)
    ntab = 1 if lumi else 3
    assert len(case.ref) == ntab - case.first
    refs, tables, ratios = [], [], []
    for t in range(ntab):
        if t < case.first:
            tables.append(identity_table(dtype))
            continue
        how, x = case.ref[t - case.first]
        if how == "abs":
            ref = x * vmax_of(dtype)
        else:
            idx = np.arange(case.lo, case.hi)
            ref = x * float((idx * hist[t][case.lo:case.hi]).sum() / hist[t][case.lo:case.hi].sum())
        table, ratio = linear_table(hist[t], case.lo, case.hi, ref, dtype)
        refs.append(float(ref))
        tables.append(table)
        ratios.append(ratio)
    tables = np.stack(tables)
    return frame, refs, tables, np.asarray(ratios, np.float64), orc.apply_lut(frame, tables)
