"""NumPy restatement of linear_develop (shinestacker_amd/csrc/kernels_linear.hpp): the definition the HIP kernel is held to bit
for bit.  Integers only (int64).

Step A, per sample:    v' = min(white, (max(v - black[c], 0) * gain_q[c] + 2048) >> 12), c the sample's channel in file order
                       (R, G, B) -- step A of demosaic_restatement with the channel in place of the cell position.  At one
                       sample per pixel b = g = r = v' (black[0], gain_q[0]).
Steps C and D:         develop_restatement.colour_matrix and tone_curve on the BGR frame, as they are.

And the placement of a three-component lossless-JPEG segment (raw_ljpeg3 of csrc/kernels_ljpeg.hpp): `unpack_three`.
"""
import numpy as np

import ljpeg_restatement
from develop_restatement import colour_matrix, tone_curve


def unpack_three(span, layout):
    """(H x W x 3 RGB samples, the status of every segment) of a three-sample lossless-JPEG layout: every segment one stream of
    three components (ljpeg_restatement.decode and parse take any ncomp); component c of the stream's pixel x lands at
    segment column 3 x + c, so the H x 3W samples ljpeg_restatement places are the frame's chunky rows"""
    assert layout.spp == 3 and layout.width % 3 == 0 and all(int(s["ncomp"]) == 3 for s in layout.segments)
    samples, status = ljpeg_restatement.unpack_layout(span, layout)
    return samples.reshape(layout.height, layout.width // 3, 3), status


def levels(samples, black, gain_q, white):
    """step A on H x W x spp samples (or H x W: spp 1): int64, same shape"""
    v = np.asarray(samples).astype(np.int64)
    spp = v.shape[2] if v.ndim == 3 else 1
    b = np.asarray(black, np.int64).reshape(-1)[:spp]
    g = np.asarray(gain_q, np.int64).reshape(-1)[:spp]
    assert len(b) == spp and len(g) == spp and (b >= 0).all() and (g >= 0).all() and (g <= 65535).all()
    if v.ndim == 2:
        b, g = b[0], g[0]
    return np.minimum(int(white), (np.maximum(v - b, 0) * g + 2048) >> 12)


def linear_develop(samples, black=(0, 0, 0), gain_q=(4096, 4096, 4096), white=None, matrix_q=None, tone=None):
    """H x W x 3 samples in R, G, B order, or H x W (one grey sample per pixel), uint8 / uint16 -> H x W x 3 BGR of that dtype"""
    samples = np.asarray(samples)
    assert samples.dtype in (np.dtype(np.uint8), np.dtype(np.uint16)) and samples.ndim in (2, 3)
    if white is None:
        white = int(np.iinfo(samples.dtype).max)
    v = levels(samples, black, gain_q, white)
    out = np.stack([v, v, v], axis=2) if v.ndim == 2 else v[:, :, ::-1]
    if matrix_q is not None:
        out = colour_matrix(out, matrix_q, white)
    if tone is not None:
        assert np.asarray(tone).dtype == samples.dtype
        out = tone_curve(out, tone)
    return np.ascontiguousarray(out).astype(samples.dtype)
