"""Non-local means as the reference's post-stack denoise runs it, restated in NumPy offset by offset.

The reference's algorithms/denoise.py is `cv2.fastNlMeansDenoising(image, [h], None, template, search, norm)` on a three-
channel frame: NORM_L2 for uint8, NORM_L1 and h * 256 for uint16.  What follows is OpenCV's FastNlMeansDenoisingInvoker for
that call [from memory, unpinned: no OpenCV was at hand when this was written; parity with a real cv2 is unpinned until
the fixtures' inputs have been run through it]:

    t = template // 2, s = search // 2 (both windows forced odd), n = (2t + 1)^2, shift = smallest p with 2^p >= n
    extended image: copyMakeBorder(BORDER_REFLECT_101) over s + t pixels
    d(p, q)  = sum over the patch and the 3 channels of (a - b)^2 [uint8]  or  |a - b| [uint16]          (int)
    table[a] : dist = a * (2^shift / n);  w = exp(-dist / (h*h*3)) [L2]  or  exp(-dist*dist / (h*h*3)) [L1],
               h*h*3 evaluated in float32 (OpenCV's h is a float);  weight = cvRound(fpm * w) (half to even),
               0 when weight < 0.001 * fpm;  a = 0 .. int(max_dist / (2^shift / n) + 1) - 1
    fpm      = min(max(IT) // (search^2 * max(T)), INT_MAX),  IT = int32 [uint8], int64 [uint16]
    out[p,c] = (sum_q table[d(p, q) >> shift] * I[q, c] + W // 2) // W,  W = sum_q table[...]   (unsigned division)

One `exp` per table entry, evaluated in long double and rounded once to float64, so the table is the same number on every
NumPy build.  Everything after the table is integer.  Written for the tests and the fixture recorder; it shares nothing
with shinestacker_amd/denoise.py or the kernel.
"""
import numpy as np

NORM_L1, NORM_L2 = 2, 4      # cv2's values

INT_MAX = np.iinfo(np.int32).max


def reflect101(idx, n):
    """cv::borderInterpolate(BORDER_REFLECT_101) on an index array: reflected until it lies inside [0, n)"""
    idx = np.array(idx, dtype=np.int64)
    if n == 1:
        return np.zeros_like(idx)
    while True:
        low, high = idx < 0, idx >= n
        if not (low.any() or high.any()):
            return idx
        idx = np.where(low, -idx, idx)
        idx = np.where(high, 2 * n - 2 - idx, idx)


def odd_windows(template, search):
    t, s = int(template) // 2, int(search) // 2
    return t, s


def table_params(dtype, template, search):
    """(shift, dist multiplier, fixed-point multiplier, number of table entries)"""
    t, s = odd_windows(template, search)
    n = (2 * t + 1) ** 2
    shift = 0
    while (1 << shift) < n:
        shift += 1
    mult = float(1 << shift) / float(n)
    sw2 = (2 * s + 1) ** 2
    if np.dtype(dtype) == np.uint8:
        fpm = min(int(np.iinfo(np.int32).max) // (sw2 * 255), INT_MAX)
        max_dist = 255 * 255 * 3
    else:
        fpm = min(int(np.iinfo(np.int64).max) // (sw2 * 65535), INT_MAX)
        max_dist = 65535 * 3
    return shift, mult, fpm, int(max_dist / mult + 1)


def weight_table(dtype, h, norm, template, search):
    """The whole table (int64 array), zeros included.  `h` is what cv2 receives."""
    shift, mult, fpm, entries = table_params(dtype, template, search)
    hf = np.float32(h)
    den = float(np.float32(np.float32(hf * hf) * np.float32(3)))
    dist = np.arange(entries, dtype=np.float64) * mult
    arg = -dist / den if norm == NORM_L2 else -dist * dist / den
    w = np.exp(arg.astype(np.longdouble)).astype(np.float64)
    w[np.isnan(w)] = 1.0
    weight = np.rint(fpm * w).astype(np.int64)
    weight[weight < 0.001 * fpm] = 0
    return weight, shift


def first_zero(table):
    z = np.flatnonzero(table == 0)
    return int(z[0]) if z.size else int(table.size)


def fast_nl_means(image, h, template=7, search=21, norm=None):
    """cv2.fastNlMeansDenoising(image, [h], None, template, search, norm) for an H x W x 3 uint8 (L2) / uint16 (L1) frame"""
    image = np.asarray(image)
    assert image.ndim == 3 and image.shape[2] == 3 and image.dtype in (np.uint8, np.uint16)
    if norm is None:
        norm = NORM_L2 if image.dtype == np.uint8 else NORM_L1
    assert (norm == NORM_L2 and image.dtype == np.uint8) or (norm == NORM_L1 and image.dtype == np.uint16)
    t, s = odd_windows(template, search)
    table, shift = weight_table(image.dtype, h, norm, template, search)
    acc_t = np.uint32 if image.dtype == np.uint8 else np.uint64
    hh, ww = image.shape[:2]
    b = s + t
    ext = image[reflect101(np.arange(-b, hh + b), hh)][:, reflect101(np.arange(-b, ww + b), ww)].astype(np.int64)
    base = ext[s:s + hh + 2 * t, s:s + ww + 2 * t]            # every pixel a patch around an output pixel touches
    est = np.zeros((hh, ww, 3), acc_t)
    wsum = np.zeros((hh, ww), acc_t)
    k = 2 * t + 1
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            other = ext[s + dy:s + dy + hh + 2 * t, s + dx:s + dx + ww + 2 * t]
            diff = base - other
            d = (diff * diff if norm == NORM_L2 else np.abs(diff)).sum(axis=2)
            ii = np.zeros((d.shape[0] + 1, d.shape[1] + 1), np.int64)
            ii[1:, 1:] = d.cumsum(axis=0).cumsum(axis=1)
            patch = ii[k:, k:] - ii[:-k, k:] - ii[k:, :-k] + ii[:-k, :-k]      # (hh, ww) sums over the template window
            a = patch >> shift
            wgt = table[np.minimum(a, table.size - 1)].astype(acc_t)
            q = ext[b + dy:b + dy + hh, b + dx:b + dx + ww].astype(acc_t)
            est += wgt[:, :, None] * q
            wsum += wgt
    out = (est + (wsum // acc_t(2))[:, :, None]) // wsum[:, :, None]
    return out.astype(image.dtype)


def denoise(image, h_luminance, template_window_size=7, search_window_size=21):
    """The reference's wrapper (algorithms/denoise.py) over the restatement"""
    image = np.asarray(image)
    norm = NORM_L2 if image.dtype == np.uint8 else NORM_L1
    if image.dtype == np.uint16:
        h_luminance = h_luminance * 256
    return fast_nl_means(image, h_luminance, template_window_size, search_window_size, norm)
