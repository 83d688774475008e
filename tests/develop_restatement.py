"""NumPy restatement of raw development around the demosaic (shinestacker_amd/csrc/kernels_demosaic.hpp: mosaic_defects and the
epilogue of demosaic_mhc<T, MATRIX, TONE>): the definition the HIP kernels are held to bit for bit.  Integers only (int64).

Step 0, defect sites:  in place on the raw samples, before step A.  Sites are linear indices y * W + x, ascending and unique.
                       A listed site's neighbours are (y - 2, x), (y + 2, x), (y, x - 2), (y, x + 2); a neighbour is valid when
                       it lies inside the image and is not itself listed.  With k valid neighbours of sum S the site becomes
                       (S + (k >> 1)) // k; with k = 0 it is unchanged.
Steps A and B:         demosaic_restatement.demosaic, as it is.
Step C, colour matrix: on step B's clamped (b, g, r): M_q[i][j] = round(M[i][j] * 4096), i the output and j the input channel in
                       R, G, B order; out_i = clamp((M_q[i][0] r + M_q[i][1] g + M_q[i][2] b + 2048) >> 12, 0, white), arithmetic
                       shift.  Per row sum_j |M_q[i][j]| <= 32767.
Step D, tone curve:    out = tone[out], a table of maxv + 1 entries of the frame's dtype.
"""
import numpy as np

import demosaic_restatement as R

ROW_BOUND = 32767
RGB_OF_BGR = (2, 1, 0)      # BGR storage: channel c of the array is R, G, B number RGB_OF_BGR[c]


def quantise_matrix(m):
    """round(M * 4096), half up, as nine ints (row-major, R, G, B order)"""
    q = np.floor(np.asarray(m, dtype=np.float64) * 4096.0 + 0.5).astype(np.int64)
    assert q.shape == (3, 3)
    return tuple(int(v) for v in q.reshape(9))


def defects(mosaic, sites, return_k=False):
    """step 0 on a copy of `mosaic`; return_k: the number of valid neighbours of every listed site as well"""
    mosaic = np.asarray(mosaic)
    h, w = mosaic.shape
    sites = np.asarray(sites, dtype=np.int64)
    assert sites.ndim == 1 and (np.diff(sites) > 0).all() and (len(sites) == 0 or (sites[0] >= 0 and sites[-1] < h * w))
    listed = np.zeros(h * w, dtype=bool)
    listed[sites] = True
    src = mosaic.astype(np.int64).reshape(-1)
    out = src.copy()
    ks = np.zeros(len(sites), dtype=np.int64)
    for i, s in enumerate(sites):
        y, x = divmod(int(s), w)
        total, k = 0, 0
        for ny, nx in ((y - 2, x), (y + 2, x), (y, x - 2), (y, x + 2)):
            if 0 <= ny < h and 0 <= nx < w and not listed[ny * w + nx]:
                total += int(src[ny * w + nx])
                k += 1
        ks[i] = k
        if k:
            out[s] = (total + (k >> 1)) // k
    out = out.reshape(h, w).astype(mosaic.dtype)
    return (out, ks) if return_k else out


def colour_matrix(bgr, matrix_q, white, return_sums=False):
    """step C on an H x W x 3 BGR array (any integer type; int64 inside); return_sums: the int64 values before the clamp too"""
    v = np.asarray(bgr).astype(np.int64)
    mq = np.asarray(matrix_q, dtype=np.int64).reshape(3, 3)
    assert (np.abs(mq).sum(axis=1) <= ROW_BOUND).all()
    r, g, b = v[..., 2], v[..., 1], v[..., 0]
    pre = np.empty_like(v)
    for c in range(3):
        i = RGB_OF_BGR[c]
        pre[..., c] = (mq[i, 0] * r + mq[i, 1] * g + mq[i, 2] * b + 2048) >> 12
    out = np.clip(pre, 0, int(white))
    return (out, pre) if return_sums else out


def tone_curve(values, tone):
    tone = np.asarray(tone)
    assert tone.ndim == 1 and tone.shape[0] == int(np.iinfo(tone.dtype).max) + 1
    return tone[np.asarray(values).astype(np.int64)]


def develop(mosaic, pattern="RGGB", black=(0, 0, 0, 0), gain_q=(4096, 4096, 4096, 4096), white=None, matrix_q=None, tone=None,
            sites=None):
    """steps 0 to D: H x W mosaic (uint8 / uint16) -> H x W x 3 BGR of the same dtype; every step but A and B optional"""
    mosaic = np.asarray(mosaic)
    if white is None:
        white = int(np.iinfo(mosaic.dtype).max)
    if sites is not None and len(sites):
        mosaic = defects(mosaic, sites)
    out = R.demosaic(mosaic, pattern, black, gain_q, white)
    if matrix_q is not None:
        out = colour_matrix(out, matrix_q, white)
    if tone is not None:
        assert np.asarray(tone).dtype == mosaic.dtype
        out = tone_curve(out, tone)
    return out.astype(mosaic.dtype)
