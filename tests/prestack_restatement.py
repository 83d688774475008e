"""The pre-stack corrections (Vignetting, MaskNoise, NoiseDetection) restated in NumPy from the reference's algorithm as the
header comments of csrc/kernels_prestack.hpp describe it: float64 and integers, whole arrays, no spans, no tiles, no bisection.
tests/test_prestack_restatement.py pins every function here to the reference's recordings (tests/golden/prestack.*); the GPU
tests in tests/test_gpu_prestack_edges.py then hold the kernels to these functions at the shapes the recordings do not reach.
NumPy only: nothing of the project is imported."""
import numpy as np

CLIP_EXP = 10.0
MEAN, MEDIAN = "MEAN", "MEDIAN"
BLUR_WEIGHTS = {3: (1, 2, 1), 5: (1, 4, 6, 4, 1), 7: (2, 7, 14, 18, 14, 7, 2)}


# ---------------------------------------------------------------- ring sums
def gray8(img):
    """8-bit first (img >> 8 for 16-bit), then the integer BGR2GRAY"""
    a = np.asarray(img)
    b, g, r = ((a[..., c] >> 8 if a.dtype == np.uint16 else a[..., c]).astype(np.uint32) for c in range(3))    # < 2^23 below
    return ((np.uint32(1868) * b + np.uint32(9617) * g + np.uint32(4899) * r + np.uint32(1 << 13)) >> np.uint32(14)).astype(np.int64)


def area_mean(plane, s):
    """The project's statement of the area mean by an integer factor on integer data: the output has
    round-half-even(dim / s) rows and columns; a block of s x s pixels gives (sum + 2) >> 2 for s == 2 and otherwise the
    float32 product sum * float32(1 / s^2) rounded half to even; a block cut by the frame's edge gives the float32
    quotient sum / count over the pixels it has, rounded half to even."""
    h, w = plane.shape
    hs, ws = int(np.rint(h * (1.0 / s))), int(np.rint(w * (1.0 / s)))
    out = np.zeros((hs, ws), np.int64)
    for by in range(hs):
        for bx in range(ws):
            blk = plane[by * s:min(by * s + s, h), bx * s:min(bx * s + s, w)]
            tot = int(blk.sum())
            if blk.size == s * s:
                out[by, bx] = (tot + 2) >> 2 if s == 2 else int(np.rint(np.float32(tot) * np.float32(1.0 / (s * s))))
            else:
                out[by, bx] = int(np.rint(np.float32(tot) / np.float32(blk.size)))
    return out


def subsampled_gray(img, subsample, fast):
    g = gray8(img)
    if subsample == 1:
        return g
    return g[::subsample, ::subsample] if fast else area_mean(g, subsample)


def ring_table(hs, ws, r_steps):
    return np.linspace(0, np.sqrt((ws / 2)**2 + (hs / 2)**2), r_steps + 1)


def ring_sums(img, r_steps, subsample=1, fast=False):
    """(sums, counts) as int64 [r_steps]: ring i holds the sub-sampled gray pixels with table[i] <= d < table[i + 1], d the
    float64 distance from (ws / 2, hs / 2); a pixel with d >= table[-1] belongs to no ring"""
    g = subsampled_gray(img, subsample, fast)
    hs, ws = g.shape
    table = ring_table(hs, ws, r_steps)
    y, x = np.ogrid[:hs, :ws]
    d = np.sqrt((x - ws / 2)**2 + (y - hs / 2)**2).reshape(-1)
    ring = np.searchsorted(table, d, "right") - 1
    keep = d < table[-1]
    assert np.array_equal(keep, ring < r_steps)
    counts = np.bincount(ring[keep], minlength=r_steps).astype(np.int64)
    sums = np.bincount(ring[keep], weights=g.reshape(-1)[keep], minlength=r_steps)       # below 2^53: exact in float64
    return sums.astype(np.int64), counts


def ring_means(sums, counts):
    """np.mean of each ring's values, NaN for an empty ring"""
    out = np.full(len(sums), np.nan)
    full = counts > 0
    out[full] = sums[full].astype(np.float64) / counts[full].astype(np.float64)
    return out


# ---------------------------------------------------------------- vignette
def model(r, i0, k, r0):
    return i0 / (1.0 + np.exp(np.minimum(CLIP_EXP, np.exp(np.clip(k * (r - r0), -CLIP_EXP, CLIP_EXP)))))


def vignette_gain(h, w, i0, k, r0, v0, max_correction, rel=0.0, rows=None):
    """the gain of rows `rows` = (first, last + 1) of an h x w frame (all rows when None), [rows, w] float64, before the
    black threshold"""
    y0, y1 = (0, h) if rows is None else rows
    y, x = np.ogrid[y0:y1, :w]
    r = np.sqrt((x - w / 2)**2 + (y - h / 2)**2)
    g = np.clip(model(r, i0, k, r0) / v0 * (1.0 + rel), 1e-6, 1.0)
    if max_correction < 1:
        g = (1.0 - max_correction) + g * max_correction
    return g


def vignette(img, i0, k, r0, v0, max_correction, black_threshold, rel=0.0, rows=None, height=None):
    """img / gain, clipped to the type's range and truncated; gain 1 where min(B, G, R) < black_threshold (x 256 for
    16-bit).  `rel` scales the unclipped ratio model / v0 by (1 + rel): the tests use it to find the values that an exp one
    ulp off could move.  With `rows` = (first, last + 1), `img` holds only those rows of a frame of `height` rows."""
    img = np.asarray(img)
    h = img.shape[0] if height is None else height
    assert img.shape[0] == (h if rows is None else rows[1] - rows[0])
    vmax, scale = (255, 1) if img.dtype == np.uint8 else (65535, 256)
    g = vignette_gain(h, img.shape[1], i0, k, r0, v0, max_correction, rel, rows)
    g = np.where(img.min(axis=2) < black_threshold * scale, 1.0, g)
    return np.minimum(img.astype(np.float64) / g[:, :, None], float(vmax)).astype(img.dtype)


# ---------------------------------------------------------------- mask noise
def mask_noise(img, coords, kernel_size, method):
    """every channel of every hot pixel (y, x) of `coords`: the mean / median of the non-zero values of the UNTOUCHED input in
    the kernel_size x kernel_size window clipped to the frame, float64, assigned back truncated; kept when there is none"""
    assert method in (MEAN, MEDIAN) and kernel_size % 2 == 1
    img = np.asarray(img)
    out = img.copy()
    h, w = img.shape[:2]
    r = kernel_size // 2
    for y, x in np.asarray(coords).reshape(-1, 2):
        win = img[max(0, y - r):min(h, y + r + 1), max(0, x - r):min(w, x + r + 1)]
        for c in range(3):
            vals = win[..., c][win[..., c] != 0].astype(np.float64)
            if vals.size:
                out[y, x, c] = np.mean(vals) if method == MEAN else np.median(vals)
    return out


# ---------------------------------------------------------------- noise detection
def accumulate(frames):
    return np.stack([np.asarray(f) for f in frames]).astype(np.uint32).sum(axis=0, dtype=np.uint32)


def reflect101(i, n):
    """index i of an axis of n samples mirrored about its end samples without repeating them, as often as it takes"""
    if n == 1:
        return np.zeros_like(i)
    i = np.mod(i, 2 * (n - 1))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur(mean, blur_size):
    """The fixed small Gaussian kernel of sizes 3 / 5 / 7 on 8-bit data: separable integer weights w, borders reflect-101,
    (F^2 sum_ij w_i w_j p_ij + 2^15) >> 16 with F = 256 / sum(w)"""
    wt = np.array(BLUR_WEIGHTS[blur_size], np.int64)
    f = 256 // int(wt.sum())
    r = blur_size // 2
    h, w = mean.shape[:2]
    ys, xs = reflect101(np.arange(-r, h + r), h), reflect101(np.arange(-r, w + r), w)
    pad = mean.astype(np.int64)[ys][:, xs]
    rows = sum(wt[i] * pad[:, i:i + w] for i in range(blur_size))
    acc = sum(wt[j] * rows[j:j + h] for j in range(blur_size))
    return (acc * f * f + (1 << 15)) >> 16


def hot_map(sums, n, blur_size, thresholds):
    """(mean uint8 [h, w, 3], map uint8 [h, w] of 0 / 255, counts [map, channel 0, 1, 2]) from the sums of n frames"""
    mean = (np.asarray(sums).astype(np.int64) // n).astype(np.uint8)
    diff = np.abs(mean.astype(np.int64) - blur(mean, blur_size))
    hot = diff > np.asarray(thresholds, np.int64)[None, None, :]
    any_hot = hot.any(axis=2)
    counts = [int(any_hot.sum())] + [int(hot[..., c].sum()) for c in range(3)]
    return mean, np.where(any_hot, 255, 0).astype(np.uint8), counts
