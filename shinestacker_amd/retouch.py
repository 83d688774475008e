"""Brush retouching on the MI355X path (reference retouch/brush_tool.py, retouch/brush_preview.py, and
copy_brush_area_to_master in retouch/image_editor_ui.py): a source frame painted into the fused frame with a soft brush.

The reference paints a stroke stamp by stamp: a float64 mask layer takes `clip(layer + T * flow / 100, 0, 1)` over the stamp's
footprint, and the footprint of the frame is recomputed from a copy of the master as `master * (1 - e) + source * e` with
`e = clip(layer * opacity / 100, 0, 1)`.  T is `create_brush_mask(2 r + 1, hardness, opacity)`, which already holds
`opacity / 100`: the opacity enters twice, and that is kept.  Here the table and the stamp list are built on the host
(`brush_mask`, `stamps_along`) and one HIP kernel (csrc/kernels_brush.hpp, whose header is the specification) paints the whole
stroke in one launch: every pixel folds the stamps that hold it, in stroke order, and blends once.
tests/brush_restatement.py restates both forms in NumPy, bit for bit.

There is no CPU path: without a GPU or the library every entry point raises DeviceError.
"""
import math

import numpy as np

from . import _lib
from .errors import BitDepthError, InvalidOptionError, ShapeError

MIN_RADIUS, MAX_RADIUS = 2, 500     # MI_BR_MIN_RADIUS / MI_BR_MAX_RADIUS: the reference's brush sizes 5 to 1000
MAX_STAMPS = 65536                  # MI_BR_MAX_STAMPS: per stroke
UNDO_START = 65535                  # the reference's undo manager starts its area's minima here
_FAR = 1 << 30                      # centres are clamped to +-2^30: still far outside any frame


def _number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v)


def _cos(x):
    """cos through the long-double library function, rounded once to float64 (NumPy's float64 SIMD cos depends on the CPU)"""
    return np.cos(np.asarray(x, np.float64).astype(np.longdouble)).astype(np.float64)


def _power(x, k):
    return np.power(np.asarray(x, np.float64).astype(np.longdouble), np.longdouble(k)).astype(np.float64)


def brush_radius(size):
    """The reference's stamp radius for a brush `size`: int(round(size // 2)); InvalidOptionError outside [2, 500]"""
    if not _number(size):
        raise InvalidOptionError("size", size, "the brush size is a number")
    radius = int(round(size // 2))
    if not MIN_RADIUS <= radius <= MAX_RADIUS:
        raise InvalidOptionError("size", size, f"the brush radius size // 2 lies in [{MIN_RADIUS}, {MAX_RADIUS}]")
    return radius


def check_options(size=50, hardness=50, opacity=100, flow=100):
    """Raise InvalidOptionError unless the brush is one the reference's sliders can give; returns the radius"""
    radius = brush_radius(size)
    for name, v in (("hardness", hardness), ("opacity", opacity), ("flow", flow)):
        if not _number(v) or not 0 <= v <= 100:
            raise InvalidOptionError(name, v, "a percentage in [0, 100]")
    return radius


def brush_mask(size, hardness, opacity):
    """The reference's create_brush_mask(size, hardness_percent, opacity_percent): a size x size float64 table, the radial
    profile times opacity / 100.  cos and power go through long double and are rounded once; the rest is plain float64."""
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size < 1:
        raise InvalidOptionError("size", size, "the table's side is a positive integer")
    for name, v in (("hardness", hardness), ("opacity", opacity)):
        if not _number(v) or not 0 <= v <= 100:
            raise InvalidOptionError(name, v, "a percentage in [0, 100]")
    size = int(size)
    radius, centre = size / 2.0, (size - 1) / 2.0
    hard, opac = hardness / 100.0, opacity / 100.0
    y, x = np.ogrid[:size, :size]
    r = np.sqrt((x - centre) ** 2 + (y - centre) ** 2) / radius
    inner = np.where(r < 1.0, r, 1.0)
    h = 2.0 * hard - 1.0
    if h >= 1.0:
        profile = np.where(r < 1.0, 1.0, 0.0)
    elif h >= 0:
        profile = 0.5 * (_cos(np.pi * _power(inner, 1.0 / (1.0 - hard))) + 1.0)
    else:
        profile = np.where(r < 1.0, 0.5 * (1.0 - _cos(np.pi * _power(1.0 - inner, 1.0 / (1.0 + hard)))), 0.0)
    return np.clip(profile, 0.0, 1.0) * opac


def _points(points):
    try:
        pts = [(p[0], p[1]) for p in points]
    except (TypeError, IndexError, KeyError):
        raise InvalidOptionError("points", points, "a sequence of (x, y) positions") from None
    for x, y in pts:
        if not _number(x) or not _number(y):
            raise InvalidOptionError("points", (x, y), "a position is two finite numbers")
    return [(float(x), float(y)) for x, y in pts]


def stamps_along(points, size, zoom=1.0):
    """The stamp positions the reference's viewer emits while the mouse moves along the polyline `points`: the first point,
    then for every further point `n = int(distance / (size * 0.25 * zoom))` steps from the last anchor, stamps at
    `anchor + i * delta` for i = 0 .. n (the anchor is stamped again), the anchor moving on only when n > 0.  Positions stay
    floats; `stroke` rounds them.  [The viewer passes them through Qt's QPoint(float, float) first: see INTEGRATION.md.]"""
    pts = _points(points)
    if not _number(size) or size <= 0:
        raise InvalidOptionError("size", size, "the brush size is a positive number")
    if not _number(zoom) or zoom <= 0:
        raise InvalidOptionError("zoom", zoom, "the zoom factor is a positive number")
    if not pts:
        return []
    out = [pts[0]]
    last = pts[0]
    min_step = size * 0.25 * zoom
    for x, y in pts[1:]:
        xp, yp = last
        dist = math.sqrt((x - xp) ** 2 + (y - yp) ** 2)
        n_steps = int(float(dist) / min_step)
        if n_steps > 0:
            dx, dy = (x - xp) / n_steps, (y - yp) / n_steps
            out.extend((xp + i * dx, yp + i * dy) for i in range(n_steps + 1))
            last = (x, y)
    return out


def stamp_centres(points):
    """The pixel each position stamps: int(round(x)), int(round(y)) (half to even), as an n x 2 int32 array"""
    pts = _points(points)
    if len(pts) > MAX_STAMPS:
        raise InvalidOptionError("points", len(pts), f"a stroke has at most {MAX_STAMPS} stamps")
    c = np.empty((len(pts), 2), np.int32)
    for i, (x, y) in enumerate(pts):
        c[i] = (max(-_FAR, min(_FAR, int(round(x)))), max(-_FAR, min(_FAR, int(round(y)))))
    return c


def _footprints(centres, radius, height, width):
    """(x_start, y_start, x_end, y_end) per stamp as int64 columns, clipped to the frame, and which stamps meet the frame"""
    c = centres.astype(np.int64)
    xs, xe = np.maximum(0, c[:, 0] - radius), np.minimum(width, c[:, 0] + radius + 1)
    ys, ye = np.maximum(0, c[:, 1] - radius), np.minimum(height, c[:, 1] + radius + 1)
    return xs, ys, xe, ye, (xs < xe) & (ys < ye)


def stroke_box(centres, radius, height, width):
    """The region a stroke can change: the union of the footprints that meet the frame, or (0, 0, 0, 0)"""
    xs, ys, xe, ye, hit = _footprints(centres, radius, height, width)
    if not hit.any():
        return (0, 0, 0, 0)
    return (int(xs[hit].min()), int(ys[hit].min()), int(xe[hit].max()), int(ye[hit].max()))


def stroke_area(centres, radius, height, width):
    """The area the reference's undo manager holds after the stroke.  It takes minima (from 65535) and maxima (from 0) over
    what every stamp returned, and a stamp that misses the frame returned (0, 0, 0, 0): one such stamp pulls the area's start
    to the origin.  Always contains `stroke_box`.  (0, 0, 0, 0) when no stamp met the frame."""
    xs, ys, xe, ye, hit = _footprints(centres, radius, height, width)
    if not hit.any():
        return (0, 0, 0, 0)
    x0, y0 = min(UNDO_START, int(xs[hit].min())), min(UNDO_START, int(ys[hit].min()))
    if not hit.all():
        x0 = y0 = 0
    return (x0, y0, int(xe[hit].max()), int(ye[hit].max()))


class Stroke:
    """One brush stroke: `source` names the frame painted from (what a name means is the caller's: an index into `apply`'s
    `sources`, a frame index for the pipeline, an index or a file name for FocusStack), `points` are the stamp positions
    (`stamps_along` makes them from a polyline), the rest is the brush.  Checked on construction."""

    def __init__(self, source, points, size=50, hardness=50, opacity=100, flow=100):
        if isinstance(source, bool) or not isinstance(source, (int, np.integer, str)):
            raise InvalidOptionError("source", source, "a stroke's source is an index or a name")
        self.source = source if isinstance(source, str) else int(source)
        self.points = _points(points)
        if len(self.points) > MAX_STAMPS:
            raise InvalidOptionError("points", len(self.points), f"a stroke has at most {MAX_STAMPS} stamps")
        self.radius = check_options(size, hardness, opacity, flow)
        self.size, self.hardness, self.opacity, self.flow = size, hardness, opacity, flow

    def brush(self):
        return self.size, self.hardness, self.opacity, self.flow

    def __repr__(self):
        return (f"Stroke(source={self.source!r}, {len(self.points)} points, size={self.size}, hardness={self.hardness}, "
                f"opacity={self.opacity}, flow={self.flow})")


def check_strokes(strokes):
    """Raise InvalidOptionError unless `strokes` is a sequence of Stroke; returns it as a list"""
    try:
        strokes = list(strokes)
    except TypeError:
        raise InvalidOptionError("retouch", strokes, "a sequence of retouch.Stroke") from None
    for s in strokes:
        if not isinstance(s, Stroke):
            raise InvalidOptionError("retouch", s, "a sequence of retouch.Stroke")
    return strokes


def _check_pair(master, source):
    master, source = np.asarray(master), np.asarray(source)
    if master.dtype not in (np.uint8, np.uint16):
        raise BitDepthError("uint8 or uint16", master.dtype)
    if master.ndim != 3 or master.shape[2] != 3 or master.shape[0] < 1 or master.shape[1] < 1:
        raise InvalidOptionError("master", master.shape, "a brush paints on H x W x 3 frames")
    _check_source(master, source)
    return np.ascontiguousarray(master), np.ascontiguousarray(source)


def _check_source(master, source):
    if source.dtype != master.dtype:
        raise BitDepthError(master.dtype, source.dtype)
    if source.shape != master.shape:
        if source.ndim < 2:
            raise InvalidOptionError("source", source.shape, "a brush paints from H x W x 3 frames")
        raise ShapeError(master.shape, source.shape)


def _stamp_table(radius, hardness, opacity, flow):
    """S = T * flow / 100.0, in the reference's order of operations"""
    return np.ascontiguousarray(brush_mask(2 * radius + 1, hardness, opacity) * flow / 100.0, np.float64)


# ---------------------------------------------------------------------------------------------------- device forms
def stroke_device(dev_master, dev_source, height, width, dtype, points, size=50, hardness=50, opacity=100, flow=100, device=0,
                  dev_mask=None):
    """stroke() for frames resident in HBM: `dev_master` is painted in place from `dev_source`, which is only read;
    `dev_mask`, when given, is an H x W float64 plane that receives the mask layer.  The table and the stamps are uploaded for
    the call and freed after it, so the call waits for the launch.  Returns the area."""
    dt = np.dtype(dtype)
    if dt not in (np.uint8, np.uint16):
        raise BitDepthError("uint8 or uint16", dt)
    if height < 1 or width < 1:
        raise InvalidOptionError("master", (height, width), "a brush paints on H x W x 3 frames")
    radius = check_options(size, hardness, opacity, flow)
    centres = stamp_centres(points)
    _lib.require_device()
    lib = _lib.load()
    box = np.asarray(stroke_box(centres, radius, height, width), np.int32)
    if box[0] >= box[2] and dev_mask is None:
        return (0, 0, 0, 0)         # nothing meets the frame and no plane to zero: nothing to queue
    table = _stamp_table(radius, hardness, opacity, flow)
    bufs = []
    try:
        for a in (table, centres) if len(centres) else (table,):
            bufs.append(_lib.DeviceBuffer(a.nbytes, device))
            bufs[-1].upload(a)
        _lib.check(lib.mi_brush_stroke_device(int(device), None, dev_master, dev_source, int(height), int(width), _lib.DTYPE_CODE[dt],
                                              bufs[0].ptr, radius, bufs[1].ptr if len(centres) else None, len(centres),
                                              box.ctypes.data, opacity / 100.0, dev_mask))
        _lib.check(lib.mi_device_synchronize(int(device)))
    finally:
        for b in bufs:
            b.free()
    return stroke_area(centres, radius, height, width)


def apply_device(dev_master, height, width, dtype, strokes, dev_sources, device=0):
    """The strokes, in order, each on the previous one's result, on a master resident in HBM.  `dev_sources` maps every
    stroke's `source` to the device address of that frame.  Returns the list of areas."""
    strokes = check_strokes(strokes)
    for s in strokes:
        if s.source not in dev_sources:
            raise InvalidOptionError("source", s.source, "no such frame among the sources")
    return [stroke_device(dev_master, dev_sources[s.source], height, width, dtype, s.points, *s.brush(), device=device) for s in strokes]


def blend_device(dev_master, dev_source, dev_mask, height, width, dtype, opacity=100, device=0, stream=None):
    """blend() for frames and an H x W float64 mask resident in HBM, `dev_master` in place.  Queued on `stream`, not waited for."""
    dt = np.dtype(dtype)
    if dt not in (np.uint8, np.uint16):
        raise BitDepthError("uint8 or uint16", dt)
    if height < 1 or width < 1:
        raise InvalidOptionError("master", (height, width), "a mask blends H x W x 3 frames")
    if not _number(opacity) or not 0 <= opacity <= 100:
        raise InvalidOptionError("opacity", opacity, "a percentage in [0, 100]")
    _lib.require_device()
    _lib.check(_lib.load().mi_blend_mask_device(int(device), stream, dev_master, dev_source, dev_mask, int(height), int(width),
                                                _lib.DTYPE_CODE[dt], opacity / 100.0))


# ---------------------------------------------------------------------------------------------------- host forms
def stroke(master, source, points, size=50, hardness=50, opacity=100, flow=100, device=0, return_mask=False):
    """One stroke of the brush (`size`, and `hardness`, `opacity`, `flow` in per cent) along the stamp positions `points`,
    painting `source` into `master` (H x W x 3 uint8 / uint16 frames of one shape).  Returns (frame, area) -- a new array and
    `stroke_area`, the (x_start, y_start, x_end, y_end) the reference's undo manager holds -- or (frame, area, M) with
    `return_mask`, M the H x W float64 mask layer."""
    master, source = _check_pair(master, source)
    radius = check_options(size, hardness, opacity, flow)
    centres = stamp_centres(points)
    h, w = master.shape[:2]
    _lib.require_device()
    out = master.copy()
    mask = np.zeros((h, w), np.float64) if return_mask else None
    if len(centres):
        table = _stamp_table(radius, hardness, opacity, flow)
        _lib.check(_lib.load().mi_brush_stroke(int(device), out.ctypes.data, source.ctypes.data, h, w, _lib.DTYPE_CODE[out.dtype],
                                               table.ctypes.data, radius, centres.ctypes.data, len(centres), opacity / 100.0,
                                               None if mask is None else mask.ctypes.data, None))
    area = stroke_area(centres, radius, h, w)
    return (out, area, mask) if return_mask else (out, area)


def apply(master, strokes, sources, device=0):
    """The strokes, in order, each on the previous one's result.  `sources` maps a stroke's `source` to a frame (a dict, or a
    sequence indexed by it); the master and every frame a stroke names are uploaded once.  Returns a new array."""
    strokes = check_strokes(strokes)
    master = np.asarray(master)
    named = {}
    for s in strokes:
        if s.source in named:
            continue
        try:
            frame = sources[s.source]
        except (KeyError, IndexError, TypeError):
            raise InvalidOptionError("source", s.source, "no such frame among the sources") from None
        named[s.source] = frame
    if master.dtype not in (np.uint8, np.uint16):
        raise BitDepthError("uint8 or uint16", master.dtype)
    if master.ndim != 3 or master.shape[2] != 3 or master.shape[0] < 1 or master.shape[1] < 1:
        raise InvalidOptionError("master", master.shape, "a brush paints on H x W x 3 frames")
    named = {k: np.asarray(v) for k, v in named.items()}
    for v in named.values():
        _check_source(master, v)
    _lib.require_device()
    if not strokes:
        return master.copy()
    h, w = master.shape[:2]
    bufs = {}
    dev = None
    try:
        dev = _lib.DeviceBuffer(master.nbytes, device)
        dev.upload(master)
        for k, v in named.items():
            bufs[k] = _lib.DeviceBuffer(v.nbytes, device)
            bufs[k].upload(v)
        apply_device(dev.ptr, h, w, master.dtype, strokes, {k: b.ptr for k, b in bufs.items()}, device)
        return dev.download(master.shape, master.dtype)
    finally:
        for b in list(bufs.values()) + [dev]:
            if b is not None:
                b.free()


def blend(master, source, mask, opacity=100, device=0):
    """The reference's apply_mask over a whole frame, for a caller that already has a mask (H x W, taken as float64):
    e = clip(mask * opacity / 100, 0, 1), out = trunc(clip(master * (1 - e) + source * e, 0, max)).  Returns a new array."""
    master, source = _check_pair(master, source)
    mask = np.ascontiguousarray(mask, np.float64)
    if mask.shape != master.shape[:2]:
        raise InvalidOptionError("mask", mask.shape, f"the mask is the frame's H x W plane ({master.shape[0]} x {master.shape[1]})")
    if not np.isfinite(mask).all():
        raise InvalidOptionError("mask", "nan / inf", "the mask holds finite values")
    if not _number(opacity) or not 0 <= opacity <= 100:
        raise InvalidOptionError("opacity", opacity, "a percentage in [0, 100]")
    _lib.require_device()
    out = master.copy()
    _lib.check(_lib.load().mi_blend_mask(int(device), out.ctypes.data, source.ctypes.data, mask.ctypes.data, master.shape[0],
                                         master.shape[1], _lib.DTYPE_CODE[out.dtype], opacity / 100.0))
    return out
