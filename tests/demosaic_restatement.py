"""NumPy restatement of the raw-mosaic demosaic (shinestacker_amd/csrc/kernels_demosaic.hpp): the definition the HIP
kernel is held to bit for bit.  Integers only (int64), no floats, and nothing of the kernel's tiling.

Step A, per site:   v' = min(white, (max(v - black, 0) * gain_q + 2048) >> 12)
Step B:             Malvar-He-Cutler 5 x 5 linear interpolation, the paper's coefficients times 2 (everything over 16),
                    out = clamp((sum + 8) >> 4, 0, white) with an arithmetic shift, BORDER_REFLECT_101 on the mosaic,
                    H x W x 3 interleaved BGR in the input dtype.
"""
import numpy as np

PATTERNS = ("RGGB", "BGGR", "GRBG", "GBRG")

# rows dy = -2 .. 2
G_AT_RB = np.array([[0, 0, -2, 0, 0],
                    [0, 0, 4, 0, 0],
                    [-2, 4, 8, 4, -2],
                    [0, 0, 4, 0, 0],
                    [0, 0, -2, 0, 0]], dtype=np.int64)
C_AT_G_ROW = np.array([[0, 0, 1, 0, 0],        # colour C at a G site whose C-neighbours are left and right
                       [0, -2, 0, -2, 0],
                       [-2, 8, 10, 8, -2],
                       [0, -2, 0, -2, 0],
                       [0, 0, 1, 0, 0]], dtype=np.int64)
C_AT_G_COL = C_AT_G_ROW.T.copy()               # ... above and below
C_AT_OPP = np.array([[0, 0, -3, 0, 0],
                     [0, 4, 0, 4, 0],
                     [-3, 0, 12, 0, -3],
                     [0, 4, 0, 4, 0],
                     [0, 0, -3, 0, 0]], dtype=np.int64)
OWN = np.zeros((5, 5), dtype=np.int64)
OWN[2, 2] = 16

BGR_CHANNEL = {"B": 0, "G": 1, "R": 2}


def step_a(mosaic, black, gain_q, white):
    """black level, gain and clamp per site; int64 in, int64 out"""
    h, w = mosaic.shape
    v = mosaic.astype(np.int64)
    out = np.empty_like(v)
    for py in range(2):
        for px in range(2):
            k = 2 * py + px
            s = v[py::2, px::2]
            out[py::2, px::2] = np.minimum(int(white), (np.maximum(s - int(black[k]), 0) * int(gain_q[k]) + 2048) >> 12)
    return out


def conv5(v, table):
    """sum over the 5 x 5 table with BORDER_REFLECT_101 (period 2 (n - 1), any overshoot)"""
    h, w = v.shape

    def refl(i, n):
        p = 2 * (n - 1)
        i = np.mod(i, p)
        return np.where(i >= n, p - i, i)

    ys = np.arange(h)
    xs = np.arange(w)
    acc = np.zeros((h, w), dtype=np.int64)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            c = int(table[dy + 2, dx + 2])
            if c:
                acc += c * v[refl(ys + dy, h)[:, None], refl(xs + dx, w)[None, :]]
    return acc


def demosaic(mosaic, pattern="RGGB", black=(0, 0, 0, 0), gain_q=(4096, 4096, 4096, 4096), white=None, return_sums=False):
    """H x W mosaic (uint8 / uint16) -> H x W x 3 BGR of the same dtype.  return_sums: the int64 sums before the
    rounding shift and the clamp as well (for the tests that count how often the clamps act)."""
    mosaic = np.asarray(mosaic)
    assert mosaic.ndim == 2 and mosaic.dtype in (np.uint8, np.uint16) and min(mosaic.shape) >= 2
    assert pattern in PATTERNS
    if white is None:
        white = int(np.iinfo(mosaic.dtype).max)
    h, w = mosaic.shape
    v = step_a(mosaic, black, gain_q, white)
    t = {name: conv5(v, tab) for name, tab in (("own", OWN), ("g", G_AT_RB), ("row", C_AT_G_ROW), ("col", C_AT_G_COL),
                                                ("opp", C_AT_OPP))}
    sums = np.zeros((h, w, 3), dtype=np.int64)
    for py in range(2):
        for px in range(2):
            colour = pattern[2 * py + px]
            sl = (slice(py, None, 2), slice(px, None, 2))
            if colour == "G":
                row_colour = pattern[2 * py + (1 - px)]      # the colour left and right of this G site
                col_colour = pattern[2 * (1 - py) + px]      # the colour above and below
                sums[sl + (BGR_CHANNEL["G"],)] = t["own"][sl]
                sums[sl + (BGR_CHANNEL[row_colour],)] = t["row"][sl]
                sums[sl + (BGR_CHANNEL[col_colour],)] = t["col"][sl]
            else:
                other = "B" if colour == "R" else "R"
                sums[sl + (BGR_CHANNEL[colour],)] = t["own"][sl]
                sums[sl + (BGR_CHANNEL["G"],)] = t["g"][sl]
                sums[sl + (BGR_CHANNEL[other],)] = t["opp"][sl]
    out = np.clip((sums + 8) >> 4, 0, int(white)).astype(mosaic.dtype)
    return (out, sums) if return_sums else out


def mosaic_of(bgr, pattern="RGGB"):
    """sample an H x W x 3 BGR frame down to its mosaic"""
    bgr = np.asarray(bgr)
    out = np.empty(bgr.shape[:2], dtype=bgr.dtype)
    for py in range(2):
        for px in range(2):
            out[py::2, px::2] = bgr[py::2, px::2, BGR_CHANNEL[pattern[2 * py + px]]]
    return out
