"""The development cases shared by test_develop_host.py (CPU: no case is vacuous) and test_gpu_develop.py (GPU: the kernels equal
the restatement on them).  Mosaics and shapes are those of demosaic_cases.py; every reference is computed once and shared.

Matrices (floats, as a user gives them): identity; a camera matrix with negative off-diagonals; one whose first row sits on
the bound sum |M_q| = 32767; one with an all-zero row; a permutation.
Tone tables: identity, sRGB, gamma 2.2, a reversed ramp, a seeded random table (a wrong index or channel shows), sRGB with
`white` below the maximum.
Defect lists: see defect_cases()."""
import functools

import numpy as np

import demosaic_cases as dc
import develop_restatement as DR
from shinestacker_amd import demosaic as D

TH, TW = dc.TH, dc.TW
TINY, EDGES, RAGGED, DTYPES, PATTERNS = dc.TINY, dc.EDGES, dc.RAGGED, dc.DTYPES, dc.PATTERNS
SHAPES = TINY + EDGES + [RAGGED]
random_mosaic = dc.random_mosaic

MATRICES = {
    "identity": [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],
    "camera": [[1.8, -0.6, -0.2], [-0.3, 1.6, -0.3], [0.05, -0.55, 1.5]],
    # 16384 + 8192 + 8191 = 32767: every entry is a multiple of 1 / 4096, so the quantisation is exact
    "row at the bound": [[4.0, -2.0, -8191.0 / 4096.0], [-0.25, 1.5, -0.25], [0.0, -0.5, 1.5]],
    "zero row": [[0.0, 0.0, 0.0], [-0.5, 1.8, -0.3], [0.0, -0.4, 1.6]],
    "permutation": [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]],
}
TONES = ("identity", "srgb", "gamma 2.2", "reversed", "random", "white below the maximum")


def white_below(dtype):
    mx = int(np.iinfo(dtype).max)
    return mx - mx // 3


@functools.lru_cache(maxsize=None)
def tone_table(name, dtype):
    """the host table of a tone case (what the restatement indexes)"""
    dt = np.dtype(dtype)
    n = int(np.iinfo(dt).max) + 1
    if name == "identity":
        t = np.arange(n).astype(dt)
    elif name == "srgb":
        t = D.srgb_tone(dt)
    elif name == "gamma 2.2":
        t = D.gamma_tone(dt, 2.2)
    elif name == "reversed":
        t = np.arange(n)[::-1].astype(dt)
    elif name == "random":
        t = np.random.default_rng([77, dt.itemsize]).integers(0, n, size=n).astype(dt)
    elif name == "white below the maximum":
        t = D.srgb_tone(dt, white=white_below(dt))
    else:
        raise KeyError(name)
    t.setflags(write=False)
    return t


def tone_arg(name, dtype):
    """what Develop(tone=) is given for a tone case: the string and the float where the class resolves them itself"""
    return {"srgb": "srgb", "gamma 2.2": 2.2}.get(name, tone_table(name, dtype))


def tone_cfa(name, dtype, pattern="GRBG"):
    return D.Cfa(pattern, white=white_below(dtype) if name == "white below the maximum" else None)


def linear_sites(defects, shape):
    """ascending unique linear indices of an (n, 2) list of (y, x) or of a boolean mask -- stated here, apart from Develop.sites"""
    d = np.asarray(defects)
    if d.dtype == np.bool_:
        assert d.shape == tuple(shape)
        return np.flatnonzero(d).astype(np.int64)
    d = d.reshape(-1, 2).astype(np.int64)
    return np.unique(d[:, 0] * shape[1] + d[:, 1])


@functools.lru_cache(maxsize=None)
def defect_cases(dtype):
    """(name, mosaic, defects as Develop takes them) -- the mosaics are read-only"""
    dt = np.dtype(dtype)
    mx = int(np.iinfo(dt).max)
    cases = []

    def add(name, mosaic, sites):
        mosaic = np.array(mosaic, dtype=dt)
        mosaic.setflags(write=False)
        cases.append((name, mosaic, sites if isinstance(sites, np.ndarray) and sites.dtype == np.bool_ else
                      np.array(sites, dtype=np.int64).reshape(-1, 2)))

    h, w = TH + 1, TW + 1
    add("the four corners (k = 2)", random_mosaic((h, w), dt, 20), [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)])
    # rows 0, 1, h - 2, h - 1 and columns 0, 1, w - 2, w - 1, every fifth site: one or two neighbours lie outside
    h, w = 23, 37
    edge = [(y, x) for y in (0, 1, h - 2, h - 1) for x in range(0, w, 5)] + [(y, x) for x in (0, 1, w - 2, w - 1) for y in range(0, h, 5)]
    add("every edge, second row and column", random_mosaic((h, w), dt, 21), edge)
    add("2 x 2, every site (k = 0)", random_mosaic((2, 2), dt, 22), [(0, 0), (0, 1), (1, 0), (1, 1)])
    add("3 x 3, the centre (k = 0)", random_mosaic((3, 3), dt, 23), [(1, 1)])
    add("a plus whose centre has four listed neighbours (k = 0)", random_mosaic((h, w), dt, 24),
        [(10, 10), (8, 10), (12, 10), (10, 8), (10, 12)])
    add("a corner beside a listed site (k = 1)", random_mosaic((h, w), dt, 25), [(0, 0), (0, 2)])
    # k = 3 with rounding up: (10, 22) is listed, the other three neighbours of (10, 20) sum to 32, and (32 + 1) // 3 = 11 > 32 // 3
    m = np.array(random_mosaic((h, w), dt, 26))
    m[8, 20], m[12, 20], m[10, 18] = 10, 10, 12
    add("three valid neighbours, rounding up", m, [(10, 20), (10, 22)])
    add("a dense 10 % mask", random_mosaic(RAGGED, dt, 27), np.random.default_rng(28).random(RAGGED) < 0.10)
    add("an empty list", random_mosaic((h, w), dt, 29), [])
    h, w = 2 * TH + 1, 2 * TW + 1
    add("both sides of a tile boundary", random_mosaic((h, w), dt, 30),
        [(TH - 1, TW - 1), (TH, TW), (TH - 2, TW + 1), (TH + 1, TW - 2), (TH - 1, 5), (TH, 7), (3, TW - 1), (4, TW), (TH, TW + 2)])
    # every neighbour at the dtype's maximum: S reaches 4 * maxv
    m = np.full((23, 37), mx, dtype=dt)
    sat = [(10, 10), (11, 15), (2, 2), (20, 34), (5, 30)]
    for y, x in sat:
        m[y, x] = 0
    add("neighbours at the maximum", m, sat)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def defects_reference(dtype, index):
    """(repaired mosaic, k per listed site, the linear sites) of defect_cases(dtype)[index]"""
    _, mosaic, sites = defect_cases(dtype)[index]
    lin = linear_sites(sites, mosaic.shape)
    out, ks = DR.defects(mosaic, lin, return_k=True)
    out.setflags(write=False)
    return out, ks, lin


def restate(mosaic, cfa, matrix=None, tone=None, defects=None):
    """the restatement of debayer(mosaic, cfa, Develop(matrix, tone table, defects))"""
    code, black, gain_q, white = cfa.quantised(mosaic.dtype)
    return DR.develop(mosaic, DR.R.PATTERNS[code], black, gain_q, white,
                      matrix_q=None if matrix is None else DR.quantise_matrix(matrix), tone=tone,
                      sites=None if defects is None else linear_sites(defects, mosaic.shape))


@functools.lru_cache(maxsize=None)
def shape_reference(shape, dtype, pattern, matrix_name, tone_name):
    """the developed random_mosaic(shape, dtype) under the default Cfa of `pattern`; a name None leaves its step out"""
    out = restate(random_mosaic(shape, dtype), D.Cfa(pattern), None if matrix_name is None else MATRICES[matrix_name],
                  None if tone_name is None else tone_table(tone_name, dtype))
    out.setflags(write=False)
    return out


def full_cases(dtype):
    """(name, mosaic, Cfa, matrix name, tone name, defects): steps 0 to D together, at the ragged shape"""
    dt = np.dtype(dtype)
    mx = int(np.iinfo(dt).max)
    m = random_mosaic(RAGGED, dt, 40)
    mask = np.random.default_rng(41).random(RAGGED) < 0.03
    few = np.array([(0, 0), (TH, TW), (TH - 1, TW - 1), (RAGGED[0] - 1, RAGGED[1] - 1), (7, 9), (7, 11)])
    return [
        ("camera, srgb, a 3 % mask", m, D.Cfa("RGGB", black=mx // 64, gains=[1.9, 1.0, 1.0, 1.5]), "camera", "srgb", mask),
        ("row at the bound, random table, a few sites", m, D.Cfa("GBRG"), "row at the bound", "random", few),
        ("zero row, reversed ramp, white below the maximum", m, D.Cfa("BGGR", gains=[1.5, 1.0, 1.0, 1.25], white=white_below(dt)),
         "zero row", "reversed", mask),
        ("defects and matrix only", m, D.Cfa("GRBG"), "permutation", None, few),
        ("defects and tone only", m, D.Cfa("GRBG", black=3), None, "gamma 2.2", mask),
    ]
