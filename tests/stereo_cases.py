"""The cases the stereo view and the anaglyph (csrc/kernels_stereo.hpp) are run at beyond the file they arrived with: widths
next to the MI_SV_SEG = 512 targets of a workgroup, shifts with ceil(|shift|) == W - 1, depth planes that hold NaN, the
infinities and -0, rows that no source lands on at all, and a path predictor that labels, from the restatement's own
arithmetic, what every case reaches.  A plain module shared by test_depth_outputs_cases_host.py and
test_gpu_depth_outputs_edges.py.  NumPy only, seeded, no device.

A row with no filled target: rint rounds both half-way ends of the displacement outward, so with pivot 0.5 and an odd shift s
the nearness 0 moves by -(s + 1) / 2 and the nearness 1 by +(s + 1) / 2 -- a span of s + 1, which is W when ceil(|shift|) ==
W - 1.  A row whose left half is at nearness 0 and whose right half at nearness 1 (for s > 0; the other way round for s < 0)
then loses every source over one edge or the other, and every target keeps its own pixel."""
import functools
from collections import namedtuple

import numpy as np

import stereo_restatement as sr

SEG = 512               # MI_SV_SEG
N_FRAMES = 9
ROWS = 5                # the `steps` plane moves its steps by -2 .. 2 columns over five rows
WIDTHS = [65, 511, 512, 513, 1024, 1025]
SHIFTS = [64.0, -64.0]
PIVOTS = [0.0, 0.3, 1.0]
NEARS = ["last", "first"]
KINDS = ["steps", "random", "ramp", "special"]
NARROW = (8, 6.5)       # a fractional shift with ceil(|shift|) == W - 1
EMPTY_ROWS = [(4, 3.0), (8, 7.0), (64, 63.0)]       # (W, s): odd s = W - 1 at pivot 0.5, on the `halves` plane
DTYPES = [np.uint8, np.uint16]

NO_SIDE = "hole with no side"
LABELS = ["occluded", "hole from the left", "hole from the right", "hole with one side", NO_SIDE, "hole of 64",
          "source into another segment", "hole neighbour in another segment"]

ViewCase = namedtuple("ViewCase", "width kind shift pivot near")


def _view_cases():
    out = [ViewCase(w, k, s, p, n) for w in WIDTHS for k in KINDS for s in SHIFTS for p in PIVOTS for n in NEARS]
    w, s = NARROW
    out += [ViewCase(w, k, sg * s, p, n) for k in ("random", "special") for sg in (1, -1) for p in PIVOTS for n in NEARS]
    out += [ViewCase(w, "halves", sg * s, 0.5, n) for w, s in EMPTY_ROWS for sg in (1, -1) for n in NEARS]
    return out


VIEW_CASES = _view_cases()
GROUPS = sorted({c.width for c in VIEW_CASES})      # what one GPU test runs


def view_name(c):
    return "%d %s shift %g pivot %g near %s" % c


def depth_plane(kind, shape, n, seed=5):
    """the `ramp`, `steps` and `random` planes the view arrived with (tests/test_gpu_stereo.py builds the same)"""
    h, w = shape
    rng = np.random.default_rng(seed)
    if kind == "ramp":          # smooth, tilted, a little past both ends of the stack
        y, x = np.mgrid[0:h, 0:w]
        return (-0.01 + (n - 1 + 0.02) * ((x + 0.37 * y) / (w + 0.37 * h))).astype(np.float32)
    if kind == "steps":         # vertical steps between 0 and N - 1, at and next to the segment boundaries and elsewhere; a row
        z = np.zeros(shape, np.float32)     # shifts its steps by -2 .. 2 columns: the widest holes, the longest occlusions
        for y in range(h):
            edges = sorted({e + (y % 5) - 2 for e in list(range(SEG, w, SEG)) + [w // 3, (2 * w) // 3, 70, w - 70, SEG + 64, SEG - 64]}
                           & set(range(1, w)))
            val, prev = (y & 1) * (n - 1), 0
            for e in edges + [w]:
                z[y, prev:e] = val
                val, prev = (n - 1) - val, e
        return z
    assert kind == "random"     # integer + fraction
    return (rng.integers(0, n, shape) + rng.random(shape) * 0.999).clip(0, n - 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def plane(kind, width):
    """ROWS x width float32.  `special`: the random plane with NaN, +inf, -inf and -0.0 at a tenth of its pixels, each;
    `halves`: the left half of a row at frame 0 and the right half at frame N - 1 in the even rows, the other way round in the
    odd rows, and row 4 like row 0 but for its first pixel, which is at frame N - 1 too"""
    shape = (ROWS, width)
    if kind == "special":
        z = depth_plane("random", shape, N_FRAMES, seed=width + 1).copy()
        pick = np.random.default_rng(width).integers(0, 10, shape)
        for code, v in enumerate((np.nan, np.inf, -np.inf, -0.0)):
            z[pick == code] = v
        # whole runs of them too: a run of equal nearness is a translated block, and what follows it opens a hole
        if width > 40:
            z[0, 5:25], z[1, 5:25], z[2, 5:25], z[3, 5:25] = np.nan, np.inf, -np.inf, -0.0
    elif kind == "halves":
        z = np.zeros(shape, np.float32)
        z[0::2, width // 2:] = N_FRAMES - 1
        z[1::2, :width // 2] = N_FRAMES - 1
        z[4, 0] = N_FRAMES - 1
    else:
        z = depth_plane(kind, shape, N_FRAMES, seed=width)
    z = np.ascontiguousarray(z, np.float32)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def image(shape, dtype, seed=1):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, np.iinfo(dtype).max + 1, tuple(shape) + (3,)).astype(dtype)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def source_map(c):
    """the restatement's source column of every target, ROWS x width"""
    z = plane(c.kind, c.width)
    xs = np.stack([sr.source_columns(z[y], N_FRAMES, c.shift, c.pivot, c.near) for y in range(ROWS)])
    xs.setflags(write=False)
    return xs


def expected_view(c, dtype):
    """sr.view: out[y, x'] = image[y, xs[y, x']]"""
    img = image((ROWS, c.width), dtype)
    return img[np.arange(ROWS)[:, None], source_map(c)]


def row_labels(depth_row, n_frames, shift, pivot, near):
    """What one row reaches, from the restatement's nearness and displacement: a set of LABELS"""
    w = depth_row.shape[0]
    t = sr.nearness(depth_row, n_frames, near)
    d = sr.displacement(t, shift, pivot).astype(np.int64)
    x = np.arange(w)
    xt = x + d
    lands = (xt >= 0) & (xt < w)
    win_t = np.full(w, -1.0, np.float32)
    np.maximum.at(win_t, xt[lands], t[lands])
    filled = win_t >= 0
    out = set()
    if (lands & (t < win_t[np.clip(xt, 0, w - 1)])).any():
        out.add("occluded")
    if (lands & (x // SEG != xt // SEG)).any():
        out.add("source into another segment")
    holes = np.flatnonzero(~filled)
    at = np.flatnonzero(filled)
    if holes.size and not at.size:
        out.add(NO_SIDE)
        return out
    for h in holes:
        i = np.searchsorted(at, h)
        left = at[i - 1] if i > 0 else -1
        right = at[i] if i < at.size else -1
        if left < 0 or right < 0:
            out.add("hole with one side")
        else:
            out.add("hole from the left" if win_t[left] <= win_t[right] else "hole from the right")
        if any(n >= 0 and n // SEG != h // SEG for n in (left, right)):
            out.add("hole neighbour in another segment")
    if holes.size:
        runs = np.split(holes, np.flatnonzero(np.diff(holes) != 1) + 1)
        if any(len(r) == 64 for r in runs):
            out.add("hole of 64")
    return out


@functools.lru_cache(maxsize=None)
def labels(c):
    z = plane(c.kind, c.width)
    out = set()
    for y in range(ROWS):
        out |= row_labels(z[y], N_FRAMES, c.shift, c.pivot, c.near)
    return frozenset(out)


def displacement_span(n_frames, shift, pivot):
    """(a, b): every source moves by a displacement in [-a, b]"""
    d = sr.displacement(sr.nearness(np.float32([0.0, n_frames - 1]), n_frames), shift, pivot)
    return int(max(0, -d.min())), int(max(0, d.max()))


# ---------------------------------------------------------------- device form: alignment and guard bytes
# (dtype, bytes the frame starts after a 4-byte boundary, the same for the output): uint8 outputs on every byte, uint16 frames and
# outputs on both 2-byte phases
DEVICE_CASES = [(np.uint8, s, o) for s, o in ((0, 0), (3, 1), (1, 2), (2, 3))] + [(np.uint16, 2, 0), (np.uint16, 0, 2), (np.uint16, 2, 2)]
DEVICE_VIEW = ViewCase(513, "steps", -64.0, 0.3, "first")      # odd width: the rows start on every phase of the 4-byte words
GUARD = 32              # bytes on either side of the output that must stay as they were

# ---------------------------------------------------------------- anaglyph
ANAGLYPH_SHAPES = [(1, 1), (1, 2), (3, 5)]


def tail_samples(shape, dtype):
    """samples after the last whole 4-byte word of a frame"""
    n = shape[0] * shape[1] * 3
    per_word = 4 // np.dtype(dtype).itemsize
    return n - (n // per_word) * per_word
