"""The cases the post-stack filters are run at beyond the recorded fixtures: frame builders, the denoise and unsharp case
tables, and the restatements' results for them (computed once per process, read-only).  A plain module shared by
test_poststack_cases_host.py, which checks from the restatements that no case is vacuous, and test_gpu_poststack_edges.py,
which holds the kernels to the restatements on every case.  Integers and NumPy only, seeded, no device.

Shapes: the smallest at which each edge of the 32 x 32 tile kernels exists -- a single pixel, one row, one column (the
`len == 1` branch of reflect-101), a frame smaller than any window, exactly one tile, 2 x 3 tiles with one-pixel tails both
ways, a frame below / on and on / above the tile grid."""
import functools
from collections import namedtuple

import numpy as np

import nlm_restatement as nlm
import unsharp_restatement as usr
from test_denoise_host import hash_noise, widen_u16

SHAPES = [(1, 1), (1, 37), (37, 1), (2, 3), (32, 32), (33, 65), (31, 64), (64, 33)]
SWEEP_SHAPES = [(33, 65), (1, 37), (37, 1), (32, 32)]
OTHER_SHAPES = [(1, 1), (2, 3), (31, 64), (64, 33)]
DTYPES = [np.uint8, np.uint16]


def vmax_of(dtype):
    return int(np.iinfo(dtype).max)


def dtype_name(dtype):
    return np.dtype(dtype).name


# ---------------------------------------------------------------- frames
def textured(h, w, seed, base=120, swing=60, amp=6):
    """the fixture recorder's uint8 frame (tools/gen_golden_denoise.py synth_noisy): a smooth sin * cos texture with a step at
    x > 0.6 w, a per-channel offset of +12 / 0 / -12 and integer hash noise in [-amp, amp], clipped"""
    y, x = np.mgrid[:h, :w]
    tex = base + swing * np.sin(x / 9.0) * np.cos(y / 7.0) + 40.0 * (x > 0.6 * w)
    img = np.rint(tex).astype(np.int64)[:, :, None] + np.array([12, 0, -12]) + hash_noise((h, w, 3), seed, amp)
    return np.clip(img, 0, 255).astype(np.uint8)


def bright(h, w, seed, amp=6):
    """textured at base 240, swing 30: close to half of the uint8 samples sit at 255"""
    return textured(h, w, seed, base=240, swing=30, amp=amp)


def dark(h, w, seed, amp=6):
    """the mirror image of `bright`, 255 - bright: base 15, every term with the other sign, so the share of its samples at 0 is
    the share of `bright` at 255"""
    return (255 - bright(h, w, seed, amp=amp)).astype(np.uint8)


def constant(h, w, dtype, value=None):
    return np.full((h, w, 3), vmax_of(dtype) if value is None else value, dtype)


def checkerboard(h, w, dtype):
    """0 / max with period 1 both ways"""
    y, x = np.mgrid[:h, :w]
    return np.repeat((((y + x) & 1) * vmax_of(dtype))[:, :, None], 3, axis=2).astype(dtype)


def columns(h, w, dtype):
    """0 / max columns with period 1"""
    y, x = np.mgrid[:h, :w]
    return np.repeat(((x & 1) * vmax_of(dtype))[:, :, None], 3, axis=2).astype(dtype)


@functools.lru_cache(maxsize=None)
def frame(kind, shape, dtype, seed=0, amp=6):
    """A read-only frame.  uint16 frames of the textured kinds come through widen_u16; `bright` then gains 256 before the clip,
    so that what is saturated in the uint8 frame is at 65535 here too, and `dark` is 65535 - bright."""
    h, w = shape
    wide = np.dtype(dtype) == np.uint16
    if kind in ("textured", "bright", "dark"):
        img = textured(h, w, seed, amp=amp) if kind == "textured" else bright(h, w, seed, amp=amp)
        if wide:
            img = np.clip(widen_u16(img).astype(np.int64) + (0 if kind == "textured" else 256), 0, 65535).astype(np.uint16)
        if kind == "dark":
            img = (vmax_of(dtype) - img).astype(dtype)
    elif kind == "constant":
        img = constant(h, w, dtype)
    elif kind == "checker":
        img = checkerboard(h, w, dtype)
    elif kind == "columns":
        img = columns(h, w, dtype)
    else:
        raise ValueError(kind)
    assert img.dtype == np.dtype(dtype) and img.shape == (h, w, 3)
    img.setflags(write=False)
    return img


def seed_of(shape):
    return 1 + shape[0] * 100 + shape[1]


# ---------------------------------------------------------------- denoise
# group: what one GPU test runs; identity: the restatement must return the input; branch: where nlm_launch must put the table
# amp: the noise amplitude of the textured frame
DenoiseCase = namedtuple("DenoiseCase", "group kind shape dtype h template search identity branch amp")
NOISE_AMP = 6
WEAK_NOISE_AMP = 3      # at h = 3 the restatement leaves most of a frame with noise 6 alone (12 % changed on 33 x 65)

SWEEP_TEMPLATES = [1, 3, 5, 7, 9, 11]       # TH 0 .. 5
SWEEP_SEARCHES = [1, 3, 11, 21]             # s 0, 1, 5, 10
SWEEP_H = 10

PLACEMENT = [
    # (dtype, h, template, search, branch)
    (np.uint8, 25, 7, 21, "lds"),           # 63 644 bytes: the largest request the kernel can make
    (np.uint8, 25, 11, 21, "global"),
    (np.uint8, 40, 3, 5, "global"),
    (np.uint8, 100, 1, 21, "global"),       # the whole table, no zero entry
    (np.uint8, 100, 7, 21, "global"),
    (np.uint16, 3, 11, 21, "lds"),          # 56 404 bytes
    (np.uint16, 10, 3, 5, "lds"),
    (np.uint16, 10, 7, 21, "global"),
    (np.uint16, 30, 3, 5, "global"),
]
PLACEMENT_SHAPES = [(33, 65), (64, 33)]
BOUNDS_SHAPES = [(33, 65), (1, 37)]      # a one-column frame has no step: too little of its `bright` is saturated
LARGEST_LDS = (np.uint8, 25, 7, 21)
LDS_LIMIT = 65536
LDS_MARGIN = 1800       # every placement case is at least this far from the limit


def cv2_h(dtype, h):
    """the strength cv2 receives from the reference's wrapper"""
    return h * 256 if np.dtype(dtype) == np.uint16 else h


def lds_request(dtype, h, template, search):
    """(bytes of LDS with the table in it, entries of the table up to its first zero): nlm_lds_bytes and nlm_launch's rule
    `lds + 4 * table_len <= MI_NLM_LDS_LIMIT` of csrc/kernels_denoise.hpp, with the restatement's table"""
    t, s = template // 2, search // 2
    iw, dw = 32 + 2 * (s + t), 32 + 2 * t
    norm = nlm.NORM_L2 if np.dtype(dtype) == np.uint8 else nlm.NORM_L1
    table_len = nlm.first_zero(nlm.weight_table(dtype, cv2_h(dtype, h), norm, template, search)[0])
    return iw * iw * (4 if np.dtype(dtype) == np.uint8 else 8) + 4 * (dw * dw + dw * 32) + 4 * table_len, table_len


def table_branch(dtype, h, template, search):
    return "lds" if lds_request(dtype, h, template, search)[0] <= LDS_LIMIT else "global"


def _denoise_cases():
    out = []
    for dt in DTYPES:
        for shape in SWEEP_SHAPES:
            group = "sweep %dx%d" % shape
            for tpl in SWEEP_TEMPLATES:
                for srch in SWEEP_SEARCHES:
                    out.append(DenoiseCase(group, "textured", shape, dt, SWEEP_H, tpl, srch, srch == 1, None, NOISE_AMP))
        group = "sweep rest"
        # the even windows fold to 9 and 21; a non-integral strength on a multi-tile frame
        out.append(DenoiseCase(group, "textured", (33, 65), dt, SWEEP_H, 8, 20, False, None, NOISE_AMP))
        out.append(DenoiseCase(group, "textured", (33, 65), dt, 7.5, 7, 21, False, None, NOISE_AMP))
        for shape in OTHER_SHAPES:
            for tpl, srch in ((7, 21), (9, 11)):
                out.append(DenoiseCase(group, "textured", shape, dt, SWEEP_H, tpl, srch, shape == (1, 1), None, NOISE_AMP))
    for dt, h, tpl, srch, branch in PLACEMENT:
        for shape in PLACEMENT_SHAPES:
            out.append(DenoiseCase("placement", "textured", shape, dt, h, tpl, srch, False, branch,
                                   WEAK_NOISE_AMP if h < SWEEP_H else NOISE_AMP))
    for dt in DTYPES:
        for shape in BOUNDS_SHAPES:
            # every weight of a constant frame is table[0]: the sums are at their largest; bright and dark hold whole windows
            # of saturated samples
            for kind in ("constant", "bright", "dark"):
                for tpl, srch in ((11, 21), (1, 21)):
                    out.append(DenoiseCase("bounds", kind, shape, dt, SWEEP_H, tpl, srch, kind == "constant", None, NOISE_AMP))
            # every cross-colour distance of the checkerboard is past the table: half the window has weight zero
            out.append(DenoiseCase("bounds", "checker", shape, dt, SWEEP_H, 7, 21, True, None, NOISE_AMP))
    # the same cut, `ad >= table_len`, with a long table that is read from global memory
    out.append(DenoiseCase("bounds", "checker", (33, 65), np.uint8, 25, 11, 21, True, "global", NOISE_AMP))
    out.append(DenoiseCase("bounds", "checker", (33, 65), np.uint16, 10, 7, 21, True, "global", NOISE_AMP))
    return out


DENOISE_CASES = _denoise_cases()
DENOISE_GROUPS = sorted({c.group for c in DENOISE_CASES})


def denoise_name(c):
    return "%s %s %dx%d %s h %s template %d search %d" % ((c.group, c.kind) + c.shape + (dtype_name(c.dtype), c.h, c.template,
                                                                                          c.search))


def denoise_frame(c):
    return frame(c.kind, c.shape, c.dtype, seed_of(c.shape), c.amp)


@functools.lru_cache(maxsize=None)
def denoise_expected(c):
    out = nlm.denoise(denoise_frame(c), c.h, c.template, c.search)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- unsharp
UnsharpCase = namedtuple("UnsharpCase", "group kind shape dtype radius amount threshold identity")

RADII = [0.01, 0.3, 0.5, 1, 1.7, 2.5, 3, 4]
U8_WINDOWS = [1, 3, 5, 7, 11, 17, 19, 25]
PAIRS = [(0.5, 0), (1.5, 0), (5.0, 0), (-0.5, 0), (0.0, 0), (1.5, 10), (3.0, 1), (0.3, 0.5), (1.0, 64)]
UNSHARP_AMP = 20
EXTREME_SHAPES = [(33, 65), (1, 37), (37, 1)]


def _unsharp_cases():
    out = []
    for dt in DTYPES:
        for shape in SHAPES:
            group = "%dx%d" % shape
            for radius in RADII:
                for amount, threshold in PAIRS:
                    identity = radius == 0.01 or amount == 0 or threshold == 64 or shape == (1, 1)
                    out.append(UnsharpCase(group, "textured", shape, dt, radius, amount, threshold, identity))
        for shape in EXTREME_SHAPES:
            for radius in (4, 0.5):
                for threshold in (0, 10):
                    # constant(max) on uint16: both halves of the split column sum at their largest
                    out.append(UnsharpCase("extreme", "constant", shape, dt, radius, 5.0, threshold, True))
                    for kind in ("checker", "columns"):
                        for amount in (5.0, -0.5):
                            # a 0 / max frame sharpened with a positive amount clips back onto itself; one column is all zeros
                            same = amount > 0 or (kind == "columns" and shape[1] == 1)
                            out.append(UnsharpCase("extreme", kind, shape, dt, radius, amount, threshold, same))
                    if shape in BOUNDS_SHAPES:
                        # the radius-0.5 blur moves no sample of the one-row frame by more than 10: threshold 1 there
                        masked = threshold if radius == 4 or threshold == 0 else 1
                        for kind in ("bright", "dark"):
                            out.append(UnsharpCase("extreme", kind, shape, dt, radius, 5.0, masked, False))
    return out


UNSHARP_CASES = _unsharp_cases()
UNSHARP_GROUPS = ["%dx%d" % s for s in SHAPES] + ["extreme"]


def unsharp_name(c):
    return "%s %s %dx%d %s radius %s amount %s threshold %s" % ((c.group, c.kind) + c.shape + (dtype_name(c.dtype), c.radius,
                                                                                              c.amount, c.threshold))


def unsharp_frame(c):
    return frame(c.kind, c.shape, c.dtype, seed_of(c.shape), UNSHARP_AMP)


@functools.lru_cache(maxsize=None)
def unsharp_expected(c):
    out = usr.unsharp_mask(unsharp_frame(c), c.radius, c.amount, c.threshold)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def unsharp_blurred(kind, shape, dtype, radius):
    out = usr.gaussian_blur(frame(kind, shape, dtype, seed_of(shape), UNSHARP_AMP), (0, 0), radius)
    out.setflags(write=False)
    return out
