"""The cases the depth-selected composite (csrc/kernels_composite.hpp) is run at beyond the file it arrived with: float32
frames that carry -0.0, the infinities and a NaN with a payload, frame sizes next to the 4 pixels of a lane and the 256 of a
wave, uint16 frames off a 4-byte boundary, a 128-frame stack (three launches, the last of exactly 2 frames), and a predictor
that says from depth_render_restatement.indices which path of the kernel every 64-lane wave takes.  A plain module shared by
test_depth_outputs_cases_host.py and test_gpu_depth_outputs_edges.py.  NumPy only, seeded, no device."""
import functools

import numpy as np

import depth_render_restatement as dr

LANE_PX = 4             # MI_DC_PX
WAVE_PX = 64 * LANE_PX
TAB = 64                # MI_DC_TAB: frame addresses per launch
SHAPES = [(1, 1), (1, 5), (31, 33), (32, 32), (25, 41)]         # H W = 1, 5, 1023, 1024, 1025
DTYPES = [np.uint8, np.uint16, np.float32]
PLANES = ["integer", "fractional", "ties"]
INTERPS = ["linear", "nearest"]
N_SHORT, CHUNK = 5, 3   # the short stack, and the chunk size it is also rendered with: calls (0, 3) and (2, 3)
N_LONG = 128
LONG_SHAPE = (25, 41)
PATHS = ["fast", "gather: mixed wave", "gather: chunk boundary", "gather: frame end"]
UNALIGNED = "gather: unaligned frame"
NAN_PAYLOAD = 0x7FC12345
SENTINEL = {np.uint8: 0xA5, np.uint16: 0xA5C3, np.float32: -12345.678}


def dtype_name(dtype):
    return np.dtype(dtype).name


def specials():
    """-0.0, +inf, -inf and a quiet NaN with a payload, as float32"""
    return np.array([0x80000000, 0x7F800000, 0xFF800000, NAN_PAYLOAD], np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def frames(shape, n, dtype):
    """`n` read-only frames.  float32: fractional values of either sign up to 1e6 with whole pixels of -0.0, +inf, -inf and the
    NaN (one channel of each left finite) where the `integer` plane selects them: all four in frame 1, -0.0 and the NaN in
    frame n // 2, +inf in frame 0, -inf in frame n - 1, one of the four anywhere in every other frame.  Frames of fewer than
    100 pixels carry them in frame n - 2 only, which no fractional depth of their planes touches: +inf, the NaN and -inf on
    pixel 0 and -0.0 on the last pixel; the single pixel holds -0.0, the NaN and +inf."""
    h, w = shape
    npx = h * w
    rng = np.random.default_rng(4000 + npx + n)
    sp = specials()
    selected = plane("integer", shape, n).reshape(-1).astype(np.int64)
    out = []
    for i in range(n):
        if np.dtype(dtype) == np.float32:
            fr = ((rng.random((npx, 3)) - 0.5) * 2.0e6).astype(np.float32)
            if npx < 100:
                if i == n - 2 and npx == 1:
                    fr[0] = sp[[0, 3, 1]]
                elif i == n - 2:
                    fr[0] = sp[[1, 3, 2]]
                    fr[npx - 1, 0] = sp[0]
            else:
                kinds = {1: [0, 1, 2, 3], n // 2: [0, 3], 0: [1], n - 1: [2]}.get(i)
                where = np.flatnonzero(selected == i) if kinds else np.arange(npx)
                kinds = kinds or [i % 4]
                for at, kind in zip(rng.choice(where, len(kinds), replace=False), kinds):
                    fr[at] = sp[kind]
                    fr[at, 1] = np.float32(3.25)
        else:
            fr = rng.integers(0, np.iinfo(dtype).max + 1, (npx, 3)).astype(dtype)
        fr = fr.reshape(h, w, 3)
        fr.setflags(write=False)
        out.append(fr)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def plane(kind, shape, n):
    """H x W float32 depths, laid out by the flat pixel number so that whole waves of 256 pixels take each path:
    wave 0 one frame (fast), wave 1 random frames (mixed), wave 2 two frames from either end of the stack changing every
    3 pixels (lanes that own a part of their pixels once the stack is rendered in chunks), the rest one frame again, so that
    what the frame's end leaves of the last wave is ragged on its own account only.
    `integer`: whole numbers; `fractional`: the same floors plus a fraction, zero at one pixel in 16; `ties`: the arrival
    tests' plane of half-way values, NaN, infinities and out-of-range depths."""
    h, w = shape
    npx = h * w
    rng = np.random.default_rng(5000 + npx + n)
    if kind == "ties":
        ties = np.array([0.5, 1.5, 2.5, 0.0, n - 1, n - 0.5, -0.5, n + 3.0, np.nan, np.inf, -np.inf, 1.0, 2.0, 0.25], np.float32)
        z = np.resize(ties, shape).astype(np.float32)
    else:
        i = np.arange(npx)
        wave = i // WAVE_PX
        k = np.full(npx, min(1, n - 1), np.int64)
        k[wave == 1] = rng.integers(0, n, int((wave == 1).sum()))
        k[wave == 2] = np.where((i[wave == 2] // 3) % 2 == 0, 0, n - 1)
        k[wave >= 3] = n // 2
        if npx < 100:
            k[:] = n - 2 if kind == "integer" else min(1, n - 1)  # frame n - 2 holds the small frames' infinities and NaN
        z = k.astype(np.float32)
        if kind == "fractional":
            frac = (rng.integers(1, 16, npx) / 16.0).astype(np.float32)
            frac[rng.integers(0, 16, npx) == 0] = 0
            z = np.minimum(z + frac, np.float32(n - 1))
        else:
            assert kind == "integer"
        z = z.reshape(shape)
    z.setflags(write=False)
    return z


def launches(first, count):
    """(first, count) of the kernel launches of one call: depth_composite_launch's walk over sub-chunks of at most TAB frames
    that overlap by one"""
    out = []
    f0 = 0
    while True:
        c = min(count - f0, TAB)
        out.append((first + f0, c))
        if f0 + c >= count:
            return out
        f0 += TAB - 1


def frame_offsets(shape, n, dtype, layout):
    """Where the `n` frames of a run lie, as byte offsets past a 4-byte boundary.  `separate`: every frame in an allocation of
    its own; `slots`: one allocation, a frame every 4-byte multiple of the frame size or above; `off 1` / `off 2`: slots four
    bytes longer, every frame / every second frame 2 bytes into its slot"""
    fb = shape[0] * shape[1] * 3 * np.dtype(dtype).itemsize
    slot = (fb + 3) // 4 * 4
    if layout == "separate":
        return [0] * n
    if layout == "slots":
        return [i * slot for i in range(n)]
    every = {"off 1": 1, "off 2": 2}[layout]
    assert np.dtype(dtype).itemsize == 2
    return [i * (slot + 4) + (2 if i % every == 0 else 0) for i in range(n)]


def wave_paths(depth, n_frames, first, count, nearest, offsets=None):
    """For one launch: {path: pixels written on it}, decided per 64-lane wave as the kernel does.  A wave is `fast` when every
    lane that owns a pixel owns all four of its pixels with one frame index, the same across the wave, and the one or two
    frames it then reads (the second when 'linear' meets a non-zero fraction) start on 4-byte boundaries -- `offsets` are the
    stack's frame_offsets, None for aligned frames.  Otherwise it gathers, and the reason named is the first that applies: two
    frame indices among the wave's owned pixels (mixed); a lane short of pixels because the frame ends inside it; a lane that
    owns a part of its pixels because the others belong to another chunk; an unaligned frame."""
    _, k0, f, _, k = dr.indices(depth, n_frames)
    k0, k, f = k0.reshape(-1), k.reshape(-1), f.reshape(-1)
    npx = k0.size
    own = dr.owned(k0, first, count, n_frames)
    sel = k if nearest else k0
    out = dict.fromkeys(PATHS + [UNALIGNED], 0)
    for p0 in range(0, npx, WAVE_PX):
        o = own[p0:p0 + WAVE_PX]
        if not o.any():
            continue
        s = sel[p0:p0 + WAVE_PX]
        n = int(o.sum())
        lanes = [o[q:q + LANE_PX] for q in range(0, o.size, LANE_PX)]
        partial = [ln for ln in lanes if ln.any() and not (ln.size == LANE_PX and ln.all())]
        if np.unique(s[o]).size > 1:
            out["gather: mixed wave"] += n
        elif any(ln.size < LANE_PX for ln in partial):
            out["gather: frame end"] += n
        elif partial:
            out["gather: chunk boundary"] += n
        else:
            ka = int(s[o][0])
            read = [ka]
            if not nearest and (f[p0:p0 + WAVE_PX][o] != 0).any():
                read.append(min(ka + 1, n_frames - 1))
            if offsets is not None and any(offsets[i] % 4 for i in read):
                out[UNALIGNED] += n
            else:
                out["fast"] += n
    return out


def add(total, part):
    for key, v in part.items():
        total[key] = total.get(key, 0) + v
    return total


def calls_of(run, n):
    """the (first, count) calls of a run: `whole` one call, `chunks` calls of CHUNK frames that overlap by one"""
    return [(0, n)] if run == "whole" else dr.chunks(n, CHUNK)


@functools.lru_cache(maxsize=None)
def expected(shape, n, dtype, kind, interp):
    with np.errstate(all="ignore"):
        out = dr.composite(list(frames(shape, n, dtype)), plane(kind, shape, n), interp)
    out.setflags(write=False)
    return out


def computed_nan(want, depth, n, interp):
    """where the restatement's output is a NaN that it computed: 'linear' at a non-zero fraction.  (A sample that is selected
    -- 'nearest', or a zero fraction -- is copied, a NaN with its payload.)"""
    if want.dtype != np.float32 or interp == "nearest":
        return np.zeros(want.shape, bool)
    f = dr.indices(depth, n)[2]
    return np.isnan(want) & (f != 0)[:, :, None]


def same_but_nan(got, want, computed):
    """byte for byte, except any NaN where `computed` is set"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return bool(np.isnan(got[computed]).all()) and got[~computed].tobytes() == want[~computed].tobytes()
