"""The stereo view of shinestacker_amd/stereo.py, restated in plain NumPy from its specification (the header of
csrc/kernels_stereo.hpp): the yardstick of tests/test_stereo_host.py and tests/test_gpu_stereo.py, which hold the HIP kernel
to it with array_equal.  Not a test module.

    nearness   t = depth / float32(N - 1)  (0 when N == 1),  t = min(max(t, 0), 1), 0 for a NaN depth,  t = 1 - t when
               near == 'first'
    target     d = int32(rint(float32(shift) * (t - float32(pivot)))),  x' = x + d,  dropped outside [0, W)
    occlusion  among the sources of a row on one target the largest t wins
    holes      the nearest filled target to the left and to the right: the smaller winning t, the left one on a tie, the one
               side that exists, the source pixel (y, x') itself when neither does
    output     out[y, x'] = image[y, xs]

Everything is float32, one NumPy operation per rounding.  Written row by row with a loop over the targets: clarity over speed.
"""
import numpy as np

MAX_SHIFT = 64.0


def nearness(depth, n_frames, near="last"):
    """steps 1-3 on an array of float32 depths"""
    depth = np.asarray(depth, np.float32)
    if int(n_frames) == 1:
        t = np.zeros(depth.shape, np.float32)
    else:
        t = depth / np.float32(int(n_frames) - 1)
    t = np.where(t > np.float32(0), t, np.float32(0))       # max(t, 0); a NaN depth has nearness 0
    t = np.minimum(t, np.float32(1))
    if near == "first":
        t = np.float32(1) - t
    assert t.dtype == np.float32
    return t


def displacement(t, shift, pivot):
    """step 4"""
    a = np.asarray(t, np.float32) - np.float32(pivot)
    p = np.float32(shift) * a
    assert np.asarray(p).dtype == np.float32
    return np.rint(p).astype(np.int32)


def source_columns(depth_row, n_frames, shift, pivot, near):
    """xs[x'] for one row: the source column every target shows"""
    w = depth_row.shape[0]
    t = nearness(depth_row, n_frames, near)
    d = displacement(t, shift, pivot)
    win_t = np.full(w, -1.0, np.float32)            # the winning t per target; -1: no source
    win_x = np.full(w, -1, np.int64)
    for x in range(w):
        xt = x + int(d[x])
        if 0 <= xt < w and t[x] > win_t[xt]:
            win_t[xt], win_x[xt] = t[x], x
    xs = win_x.copy()
    filled = np.flatnonzero(win_x >= 0)
    for xt in np.flatnonzero(win_x < 0):
        left = filled[filled < xt]
        right = filled[filled > xt]
        if left.size and right.size:
            l, r = left[-1], right[0]
            xs[xt] = win_x[l] if win_t[l] <= win_t[r] else win_x[r]
        elif left.size:
            xs[xt] = win_x[left[-1]]
        elif right.size:
            xs[xt] = win_x[right[0]]
        else:
            xs[xt] = xt
    return xs


def view(image, depth, n_frames, shift, pivot=0.5, near="last"):
    image = np.asarray(image)
    depth = np.asarray(depth, np.float32)
    h, w = depth.shape
    assert image.shape == (h, w, 3) and image.dtype in (np.uint8, np.uint16)
    assert int(n_frames) >= 1 and near in ("last", "first")
    assert abs(float(shift)) <= MAX_SHIFT and np.ceil(abs(float(shift))) < w and 0.0 <= float(pivot) <= 1.0
    out = np.empty_like(image)
    for y in range(h):
        out[y] = image[y, source_columns(depth[y], n_frames, shift, pivot, near)]
    return out


def pair(image, depth, n_frames, separation, pivot=0.5, near="last", layout="parallel"):
    """left = view(+separation / 2), right = view(-separation / 2); parallel: left | right, cross: right | left, anaglyph:
    BGR channel 2 from the left view, channels 0 and 1 from the right view"""
    half = np.float32(float(separation) / 2.0)
    left = view(image, depth, n_frames, half, pivot, near)
    right = view(image, depth, n_frames, -half, pivot, near)
    if layout == "parallel":
        return np.concatenate([left, right], axis=1)
    if layout == "cross":
        return np.concatenate([right, left], axis=1)
    assert layout == "anaglyph"
    out = right.copy()
    out[:, :, 2] = left[:, :, 2]
    return out


def rocking_shifts(separation, views):
    """float32(-s / 2 + k * s / (views - 1)), computed in float64 and rounded once"""
    s = float(separation)
    return [np.float32(-s / 2.0 + k * s / (views - 1)) for k in range(int(views))]


def rocking(image, depth, n_frames, separation, views=9, pivot=0.5, near="last"):
    return [view(image, depth, n_frames, s, pivot, near) for s in rocking_shifts(separation, views)]
