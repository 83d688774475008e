"""The case table of the site corrections (csrc/kernels_sitecorr.hpp), shared by test_sitecorr_host.py (CPU: no case is
vacuous) and test_gpu_sitecorr.py (GPU: the kernels equal tests/sitecorr_restatement.py on them).

Shapes against the kernel's geometry, taken from what the module exports (dng.site_vec, dng.site_tile): a workgroup is 4 rows
of 64 lanes, a lane owns one 16-byte window of its row -- 8 sites at uint16, 16 at uint8 -- aligned in memory; `paths` predicts
which windows go whole and which site by site.
  frames   2 x 2, 2 x 3, 3 x 2; 5 rows (one past the tile height) at widths one below, on and one past a window and two windows
           and one (7 / 8 / 9 / 17 at uint16, 15 / 16 / 17 / 33 at uint8); 64 windows and 9 sites wide: two workgroups along a row
  maps     1 x 1, 1 x N, N x 1, 2 x 2, 3 x 5; 9 x 11 over a 5 x 7 frame; 257 x 257 over a two-workgroup frame tall enough to
           reach every node; an origin and spacing that leave sites outside the grid on all four sides; four maps of four
           geometries; one map for all positions; one position mapped and three not
  values   nodes of 0 and of 65535 (Q12); deltas of both signs; one case that saturates at maxv
  bad      a site with 0, 1 and 4 valid neighbours, a 3 x 3 rectangle, the constant on one phase only
Inputs are chosen so that outside the saturation case nothing clamps: samples at most maxv / 3 against gains below 2 (the case
with a node of 65535 -- gain 16 -- has samples at most maxv / 17)."""
import functools
import struct

import numpy as np

from shinestacker_amd import dng

import sitecorr_restatement as rs

DTYPES = (np.dtype(np.uint8), np.dtype(np.uint16))


def paths(h, w, dtype, has_dh):
    """{"whole", "site"}: the kernel paths the row windows of an H x W mosaic take.  The mosaic and the column deltas are taken
    to start on a 16-byte boundary (a device allocation does).  A window is whole when it lies inside its row and, with column
    deltas, when the window's int16 deltas start on a 16-byte boundary."""
    item = np.dtype(dtype).itemsize
    v = dng.site_vec(dtype)
    seen = set()
    for y in range(h):
        off = (y * w * item % dng.SITE_VEC_BYTES) // item
        for x0 in range(-off, w, v):
            whole = x0 >= 0 and x0 + v <= w and (not has_dh or (2 * x0) % dng.SITE_VEC_BYTES == 0)
            seen.add("whole" if whole else "site")
    return seen


def workgroups_along_row(w, dtype):
    return -(-(w + dng.site_vec(dtype) - 1) // dng.site_tile(dtype)[1])


def _nodes(mv, mh, seed, lo=0.6, hi=1.9):
    return np.random.default_rng([mv, mh, seed]).uniform(lo, hi, size=(mv, mh))


def _full(mv, mh, seed, **kw):
    """a map whose grid spans the image: node 0 at relative 0, the last at 1"""
    return dng.GainMap(_nodes(mv, mh, seed, **kw), spacing=(1.0 / max(mv - 1, 1), 1.0 / max(mh - 1, 1)), origin=(0.0, 0.0))


class Case:
    """One frame with its corrections.  gains: None, a GainMap (all positions) or four entries; dh / dv: "both" signs or None"""

    def __init__(self, name, dtype, h, w, gains=None, deltas=False, black=(0, 0, 0, 0), top_div=3, saturate=False):
        self.name, self.dtype, self.h, self.w = name, np.dtype(dtype), h, w
        self.gains, self.deltas, self.black, self.top_div, self.saturate = gains, deltas, tuple(black), top_div, saturate

    def __repr__(self):
        return self.name

    @property
    def maxv(self):
        return rs.maxv(self.dtype)

    @functools.lru_cache(maxsize=None)
    def mosaic(self):
        rng = np.random.default_rng([self.h, self.w, self.dtype.itemsize, 7])
        hi = self.maxv if self.saturate else self.maxv // self.top_div
        a = rng.integers(hi // 2, hi + 1, size=(self.h, self.w)).astype(self.dtype)
        a.setflags(write=False)
        return a

    @functools.lru_cache(maxsize=None)
    def corrections(self):
        dh = dv = None
        if self.deltas:
            # both signs, both ends distinct, inside the black level's room: |dh| + |dv| <= min(black)
            room = max(1, min(self.black) // 2)
            rng = np.random.default_rng([self.h, self.w, 11])
            dh = rng.integers(-room, room + 1, size=self.w)
            dv = rng.integers(-room, room + 1, size=self.h)
            dh[0], dh[-1], dv[0], dv[-1] = -room, room, room, -room
        return dng.SiteCorrections(black_h=dh, black_v=dv, gains=self.gains)

    @functools.lru_cache(maxsize=None)
    def tables(self):
        return self.corrections().quantised((self.h, self.w), self.dtype)

    @functools.lru_cache(maxsize=None)
    def expected(self):
        q = self.tables()
        out = rs.site_correct(self.mosaic(), self.black, q.dh, q.dv, q.gains)
        out.setflags(write=False)
        return out

    def nodes_read(self):
        """per distinct grid of the case, the boolean mv x mh mask of the nodes some site reads"""
        q = self.tables()
        out = {}
        for p, g in enumerate(q.gains):
            if g is None:
                continue
            n, ra, ca = g
            m = out.setdefault(id(n), np.zeros(n.shape, bool))
            i, j = ra["node"][p >> 1::2].astype(int), ca["node"][p & 1::2].astype(int)
            for ii in (i, np.minimum(i + 1, n.shape[0] - 1)):
                for jj in (j, np.minimum(j + 1, n.shape[1] - 1)):
                    m[np.ix_(ii, jj)] = True
        return list(out.values())


def _frames(dtype):
    v = dng.site_vec(dtype)
    th = dng.site_tile(dtype)[0]
    return [(2, 2), (2, 3), (3, 2)] + [(th + 1, w) for w in (v - 1, v, v + 1, 2 * v + 1)]


def two_workgroup_width(dtype):
    return dng.site_tile(dtype)[1] + 9


CASES = []
for _dt in DTYPES:
    _n = _dt.name
    _blk = (6, 8, 10, 12) if _dt.itemsize == 1 else (256, 260, 258, 262)
    _maps = [_full(1, 1, 1), _full(1, 4, 2), _full(4, 1, 3), _full(2, 2, 4), _full(3, 5, 5)]
    for _k, (_h, _w) in enumerate(_frames(_dt)):
        CASES.append(Case(f"{_n}-{_h}x{_w}-deltas", _dt, _h, _w, deltas=True, black=_blk))
        CASES.append(Case(f"{_n}-{_h}x{_w}-gains-{_maps[_k % 5].nodes.shape}", _dt, _h, _w, gains=_maps[_k % 5], black=_blk))
        CASES.append(Case(f"{_n}-{_h}x{_w}-both", _dt, _h, _w, gains=_maps[(_k + 3) % 5], deltas=True, black=_blk))
    _w2 = two_workgroup_width(_dt)
    CASES += [
        Case(f"{_n}-3x{_w2}-two-workgroups-both", _dt, 3, _w2, gains=_full(3, 5, 6), deltas=True, black=_blk),
        Case(f"{_n}-9x11-over-5x7", _dt, 5, 7, gains=_full(9, 11, 7), black=_blk),
        Case(f"{_n}-outside-the-grid-on-four-sides", _dt, 9, 19,
             gains=dng.GainMap(_nodes(2, 3, 8), spacing=(0.4, 0.2), origin=(0.3, 0.3)), black=_blk),
        Case(f"{_n}-four-maps-four-geometries", _dt, 9, 19, deltas=True, black=_blk,
             gains=(_full(2, 2, 9), _full(1, 3, 10), dng.GainMap(_nodes(3, 1, 11), spacing=(0.3, 0.0), origin=(0.2, 0.0)), _full(2, 3, 12))),
        Case(f"{_n}-one-position-mapped", _dt, 5, 17, gains=(None, None, _full(2, 2, 13), None), deltas=True, black=_blk),
        Case(f"{_n}-nodes-0-and-65535", _dt, 5, 17, black=_blk, top_div=17,
             gains=dng.GainMap(np.array([[0.0, 65535.0 / 4096.0], [1.0, 0.5]]), spacing=(1.0, 1.0), origin=(0.0, 0.0))),
        Case(f"{_n}-saturates", _dt, 5, 17, gains=dng.GainMap(np.array([[3.0]])), black=_blk, saturate=True),
    ]
# 257 x 257 nodes, one map for all positions, over a two-workgroup frame tall enough for every node row (uint16: 517 x 521)
CASES.append(Case("uint16-257x257-over-two-workgroups", np.uint16, 517, two_workgroup_width(np.uint16), gains=_full(257, 257, 14),
                  deltas=True, black=(256, 260, 258, 262)))
SATURATING = {c.name for c in CASES if c.saturate}
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------ bad sites
class BadCase:
    """sites (y, x) of an H x W frame, repaired as a list, or -- `constant` -- by value on the positions of `mask`"""

    def __init__(self, name, h, w, sites, mask=15):
        self.name, self.h, self.w, self.sites_yx, self.mask = name, h, w, sites, mask

    def __repr__(self):
        return self.name

    def sites(self):
        return np.unique(np.array([y * self.w + x for y, x in self.sites_yx], np.int32))

    def constant(self, dtype):
        return rs.maxv(dtype)       # what a converter marks a dead site with

    def mosaic(self, dtype, by_constant):
        """seeded samples below the constant; by_constant: the sites hold it (on every position: the mask then picks)"""
        rng = np.random.default_rng([self.h, self.w, np.dtype(dtype).itemsize, 3])
        a = rng.integers(1, rs.maxv(dtype), size=(self.h, self.w)).astype(dtype)
        a.reshape(-1)[self.sites()] = self.constant(dtype) if by_constant else 0
        return a

    def valid_neighbours(self):
        """per listed site, the number of neighbours (y -+ 2, x), (y, x -+ 2) inside the image and not listed"""
        listed = set(self.sites_yx)
        return {(y, x): sum(1 for dy, dx in ((-2, 0), (2, 0), (0, -2), (0, 2))
                            if 0 <= y + dy < self.h and 0 <= x + dx < self.w and (y + dy, x + dx) not in listed)
                for y, x in self.sites_yx}


BAD_CASES = [
    BadCase("3x3-none-and-one-valid", 3, 3, [(0, 0), (0, 2), (2, 0)]),           # (0, 0): none valid; (0, 2), (2, 0): one
    BadCase("7x9-four-valid", 7, 9, [(3, 4), (2, 2)]),
    BadCase("9x11-rectangle-3x3", 9, 11, [(y, x) for y in range(3, 6) for x in range(4, 7)]),
    BadCase("5x37-row-of-sites", 5, 37, [(2, x) for x in range(0, 37, 3)]),
]
# the constant on one phase only: every position holds it somewhere, only position 2 (odd row, even column) is repaired
ONE_PHASE = BadCase("8x10-constant-on-one-phase", 8, 10, [(1, 2), (3, 4), (0, 0), (2, 3), (5, 5), (5, 6)], mask=1 << 2)


# ------------------------------------------------------------------------------------------------ opcodes, as a file holds them
def gain_map_opcode(nodes, rect, pitch=(1, 1), spacing=None, origin=(0.0, 0.0), planes=1, map_planes=1, cut=0):
    """(9, data): Top, Left, Bottom, Right, Plane, Planes, RowPitch, ColPitch, MapPointsV, MapPointsH (uint32), MapSpacingV/H,
    MapOriginV/H (double), MapPlanes (uint32), the points as float32 -- big-endian.  cut: bytes left off the end."""
    n = np.asarray(nodes, np.float64)
    mv, mh = n.shape
    if spacing is None:
        spacing = (1.0 / max(mv - 1, 1), 1.0 / max(mh - 1, 1))
    data = struct.pack(">10I", *rect, 0, planes, pitch[0], pitch[1], mv, mh) + struct.pack(">4d", *spacing, *origin)
    data += struct.pack(">I", map_planes) + struct.pack(f">{mv * mh}f", *n.reshape(-1))
    return 9, data[:len(data) - cut]


def bad_list_opcode(points=(), rects=(), phase=0):
    data = struct.pack(">3I", phase, len(points), len(rects))
    for y, x in points:
        data += struct.pack(">2I", y, x)
    for r in rects:
        data += struct.pack(">4I", *r)
    return 5, data


def bad_constant_opcode(constant, phase=0):
    return 4, struct.pack(">2I", constant, phase)


def f32(nodes):
    """the nodes as a file's float32 holds them"""
    return np.asarray(nodes, np.float32).astype(np.float64)
